// Attention-CRNN keyword spotter: forward and input VJP in one launch, one workgroup per clip (kws.h).
#include "kws.h"
#include "kernel_setup.h"

namespace dmad {

namespace {

constexpr int kThreads = 2 * kKwsG;      // 384 = 6 waves: one thread per gate row of the two directions (wave = direction x gate)
constexpr int kMaxLds = 160 * 1024;
constexpr int kW = 2 * kKwsH;            // 128: width of a layer's output (forward direction first)

// the step and head scratch at g.oSmall (floats)
constexpr int sZero = 0;                 // [64] zeros: h0
constexpr int sGh = 64;                  // [384] W_hh h + b_hh of the step
constexpr int sDgh = sGh + kThreads;     // [384] gradient at W_hh h + b_hh
constexpr int sPart = sDgh + kThreads;   // [384] W_hh^T dgh, one partial per gate
constexpr int sDir = sPart + kThreads;   // [128] the direct path dh * z
constexpr int sE = sDir + kW;            // [64] attention scores, then their softmax
constexpr int sDa = sE + 64;             // [64] gradient at the softmax, then at the scores
constexpr int sCtx = sDa + 64;           // [128] context
constexpr int sDctx = sCtx + kW;         // [128] its gradient
constexpr int sHead = sDctx + kW;        // [0,4) logits, [4,8) log-probabilities, [8,12) gradient at the logits, [12] log-sum-exp
static_assert(sHead + 16 <= kKwsSmall, "scratch");
static_assert(kKwsMaxT == 644, "kws_geometry's message and include/dmad.h name the cap");
static_assert(kKwsMaxSteps <= 64, "one wave holds the steps of the attention softmax");

struct KwsParams {
    KwsWeights w;
    KwsGeom g;
    const float* spec;
    float* logp;
    int32_t* cls;
    const float* g_logp;
    float* g_spec;
    int tape_stage;
    float* tape;
};

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// w (registers) . v (LDS, 16-byte aligned; the same address in every lane of a wave: a broadcast).  Four chains, joined in a fixed order
__device__ __forceinline__ float dot64(const float (&w)[kKwsH], const float* v) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int k = 0; k < kKwsH; k += 4) {
        const float4 x = *(const float4*)(v + k);
        a0 = fmaf(w[k], x.x, a0);
        a1 = fmaf(w[k + 1], x.y, a1);
        a2 = fmaf(w[k + 2], x.z, a2);
        a3 = fmaf(w[k + 3], x.w, a3);
    }
    return (a0 + a1) + (a2 + a3);
}

// GI[t][row] = b[row] + sum_k wT[k][row] in[t][k] for every step: no dependency between steps, eight of them share a weight read
template <int K>
__device__ __forceinline__ void input_proj(const float* in, const float* __restrict__ wT, const float* __restrict__ b, int T2, float* GI) {
    const int tid = threadIdx.x;
    const float bias = b[tid];
    for (int t0 = 0; t0 < T2; t0 += 8) {
        float acc[8], acd[8];                 // two chains per step (k % 4 < 2 and the rest), joined at the end
        const float* row[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            acc[i] = acd[i] = 0.f;
            row[i] = in + (t0 + i < T2 ? t0 + i : T2 - 1) * K;      // a step past the end repeats the last one and is not stored
        }
#pragma unroll 2
        for (int k = 0; k < K; k += 4) {
            const float w0 = wT[k * kThreads + tid], w1 = wT[(k + 1) * kThreads + tid], w2 = wT[(k + 2) * kThreads + tid],
                        w3 = wT[(k + 3) * kThreads + tid];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float4 x = *(const float4*)(row[i] + k);
                acc[i] = fmaf(w0, x.x, acc[i]);
                acc[i] = fmaf(w1, x.y, acc[i]);
                acd[i] = fmaf(w2, x.z, acd[i]);
                acd[i] = fmaf(w3, x.w, acd[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (t0 + i < T2) GI[(t0 + i) * kThreads + tid] = (acc[i] + acd[i]) + bias;
    }
}

// out[t][k] = sum_c w[c][k] dGI[t][c], c ascending in four chains: the walk back through input_proj (lanes over k, dGI a broadcast)
template <int K>
__device__ __forceinline__ void input_proj_back(const float* dGI, const float* __restrict__ w, int T2, float* out) {
    for (int item = threadIdx.x; item < K * T2; item += kThreads) {
        const int k = item % K, t = item / K;
        const float* g = dGI + t * kThreads;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
        for (int c = 0; c < kThreads; c += 4) {
            const float4 x = *(const float4*)(g + c);
            a0 = fmaf(w[c * K + k], x.x, a0);
            a1 = fmaf(w[(c + 1) * K + k], x.y, a1);
            a2 = fmaf(w[(c + 2) * K + k], x.z, a2);
            a3 = fmaf(w[(c + 3) * K + k], x.w, a3);
        }
        out[t * K + k] = (a0 + a1) + (a2 + a3);
    }
}

// One bidirectional GRU layer over the input projections GI: both directions in flight, the forward one at step s, the reverse one at
// T2 - 1 - s.  Thread (d, gate, j) holds row gate * 64 + j of direction d's W_hh in registers and h_{t-1} is a broadcast from H itself
__device__ __forceinline__ void gru_forward(const float* GI, const float* __restrict__ whhT, const float* __restrict__ bhh, int T2, float* H,
                                            float* small) {
    const int tid = threadIdx.x, d = tid / kKwsG, gate = (tid % kKwsG) / kKwsH, j = tid % kKwsH;
    float w[kKwsH];
#pragma unroll
    for (int k = 0; k < kKwsH; ++k) w[k] = whhT[k * kThreads + tid];
    const float bh = bhh[tid];
    float* gh = small + sGh;
    for (int s = 0; s < T2; ++s) {
        const int t = d ? T2 - 1 - s : s;
        const float* hp = s == 0 ? small + sZero : H + (d ? t + 1 : t - 1) * kW + d * kKwsH;
        gh[tid] = dot64(w, hp) + bh;
        __syncthreads();
        if (gate == 0) {
            const float* gi = GI + t * kThreads + d * kKwsG;
            const float* g = gh + d * kKwsG;
            const float r = sigm(gi[j] + g[j]);
            const float z = sigm(gi[kKwsH + j] + g[kKwsH + j]);
            const float n = tanhf(gi[2 * kKwsH + j] + r * g[2 * kKwsH + j]);
            H[t * kW + d * kKwsH + j] = (1.f - z) * n + z * hp[j];
        }
        __syncthreads();
    }
}

// The same layer walked back through time.  GH [T2][128] is the gradient at the layer's output; the gates are recomputed from GI, H and
// W_hh h_{t-1}, and GI[t] is overwritten with the gradient at the input projections (r, z, n pre-activations), which input_proj_back
// then takes to the layer's input.  Thread (d, gate, j) also holds column j of the gate's 64 rows of W_hh: its share of W_hh^T dgh
__device__ __forceinline__ void gru_backward(float* GI, const float* __restrict__ whhT, const float* __restrict__ whh,
                                             const float* __restrict__ bhh, int T2, const float* H, const float* GH, float* small) {
    const int tid = threadIdx.x, d = tid / kKwsG, gate = (tid % kKwsG) / kKwsH, j = tid % kKwsH;
    float w[kKwsH], wc[kKwsH];
#pragma unroll
    for (int k = 0; k < kKwsH; ++k) w[k] = whhT[k * kThreads + tid];
#pragma unroll
    for (int k = 0; k < kKwsH; ++k) wc[k] = whh[(d * kKwsG + gate * kKwsH + k) * kKwsH + j];
    const float bh = bhh[tid];
    float* gh = small + sGh;
    float* dgh = small + sDgh;
    float* part = small + sPart;
    float* dir = small + sDir;
    for (int s = T2 - 1; s >= 0; --s) {
        const int t = d ? T2 - 1 - s : s;
        const float* hp = s == 0 ? small + sZero : H + (d ? t + 1 : t - 1) * kW + d * kKwsH;
        gh[tid] = dot64(w, hp) + bh;
        __syncthreads();
        if (gate == 0) {
            float* gi = GI + t * kThreads + d * kKwsG;
            const float* g = gh + d * kKwsG;
            const float ghn = g[2 * kKwsH + j];
            const float r = sigm(gi[j] + g[j]);
            const float z = sigm(gi[kKwsH + j] + g[kKwsH + j]);
            const float n = tanhf(gi[2 * kKwsH + j] + r * ghn);
            float dh = GH[t * kW + d * kKwsH + j];
            if (s != T2 - 1) {                        // what the later step sent back: the direct path, then the three gates' W_hh^T dgh
                const float* pp = part + d * kKwsG;
                dh += ((dir[d * kKwsH + j] + pp[j]) + pp[kKwsH + j]) + pp[2 * kKwsH + j];
            }
            const float dn = dh * (1.f - z), dz = dh * (hp[j] - n);
            const float dnp = dn * (1.f - n * n);
            const float drp = dnp * ghn * (r * (1.f - r));
            const float dzp = dz * (z * (1.f - z));
            gi[j] = drp;
            gi[kKwsH + j] = dzp;
            gi[2 * kKwsH + j] = dnp;
            float* dg = dgh + d * kKwsG;
            dg[j] = drp;
            dg[kKwsH + j] = dzp;
            dg[2 * kKwsH + j] = dnp * r;
            dir[d * kKwsH + j] = dh * z;
        }
        __syncthreads();
        part[tid] = dot64(wc, dgh + d * kKwsG + gate * kKwsH);     // read after the next step's first barrier
    }
    __syncthreads();
}

// tape [T2 * width] of this clip <- an LDS map
__device__ __forceinline__ void tape_out(float* dst, const float* src, int n) {
    for (int i = threadIdx.x; i < n; i += kThreads) dst[i] = src[i];
}

__global__ __launch_bounds__(kThreads) void kws_kernel(const KwsParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const KwsGeom& g = p.g;
    const KwsWeights& W = p.w;
    const int tid = threadIdx.x, b = blockIdx.x, T = g.T, T2 = g.T2;
    float* X0 = lds + g.oX0;
    float* GI = lds + g.oGI;
    float* H0 = lds + g.oH[0];
    float* H1 = lds + g.oH[1];
    float* GH0 = lds + g.oGH[0];
    float* GH1 = lds + g.oGH[1];
    float* small = lds + g.oSmall;
    float* A = GH0;                                   // the attention's tanh units [T2][128], until layer 1 has been walked back
    const int ts = p.tape_stage;

    // ---- sepconv at the frames that are read: depthwise output j reads frames 16 j .. 16 j + 4 (k ascending), then the pointwise conv
    // (c ascending).  The depthwise frames [T2][32] borrow GH1
    const float* sp = p.spec + (long)b * kKwsIn * T;
    if (tid < kKwsH) small[sZero + tid] = 0.f;
    for (int item = tid; item < kKwsIn * T2; item += kThreads) {
        const int c = item % kKwsIn, j = item / kKwsIn;
        const float* x = sp + (long)c * T + kKwsHop * j;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < kKwsK; ++k) acc = fmaf(W.dw[c * kKwsK + k], x[k], acc);
        GH1[j * kKwsIn + c] = acc + W.dwb[c];
    }
    __syncthreads();
    for (int item = tid; item < kKwsH * T2; item += kThreads) {
        const int o = item % kKwsH, j = item / kKwsH;
        const float* r = GH1 + j * kKwsIn;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int c = 0; c < kKwsIn; c += 4) {
            a0 = fmaf(W.pwT[c * kKwsH + o], r[c], a0);
            a1 = fmaf(W.pwT[(c + 1) * kKwsH + o], r[c + 1], a1);
            a2 = fmaf(W.pwT[(c + 2) * kKwsH + o], r[c + 2], a2);
            a3 = fmaf(W.pwT[(c + 3) * kKwsH + o], r[c + 3], a3);
        }
        X0[j * kKwsH + o] = ((a0 + a1) + (a2 + a3)) + W.pwb[o];
    }
    __syncthreads();
    if (ts == 0) tape_out(p.tape + (long)b * T2 * kKwsH, X0, T2 * kKwsH);

    // ---- the two GRU layers: all input projections first, then the recurrence
    input_proj<kKwsH>(X0, W.wihT[0], W.bih[0], T2, GI);
    __syncthreads();
    gru_forward(GI, W.whhT[0], W.bhh[0], T2, H0, small);
    if (ts == 1) tape_out(p.tape + (long)b * T2 * kW, H0, T2 * kW);
    input_proj<kW>(H0, W.wihT[1], W.bih[1], T2, GI);
    __syncthreads();
    gru_forward(GI, W.whhT[1], W.bhh[1], T2, H1, small);
    if (ts == 2) tape_out(p.tape + (long)b * T2 * kW, H1, T2 * kW);

    // ---- attention: A[t][m] = tanh(Wx_b o_t + b), e_t = Vt . A[t], a = softmax(e) over time, ctx = sum_t a_t o_t (all ascending)
    for (int item = tid; item < kW * T2; item += kThreads) {
        const int m = item % kW, t = item / kW;
        const float* o = H1 + t * kW;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
        for (int k = 0; k < kW; k += 4) {
            const float4 x = *(const float4*)(o + k);
            a0 = fmaf(W.wxT[k * kW + m], x.x, a0);
            a1 = fmaf(W.wxT[(k + 1) * kW + m], x.y, a1);
            a2 = fmaf(W.wxT[(k + 2) * kW + m], x.z, a2);
            a3 = fmaf(W.wxT[(k + 3) * kW + m], x.w, a3);
        }
        A[t * kW + m] = tanhf(((a0 + a1) + (a2 + a3)) + W.wxb[m]);
    }
    __syncthreads();
    if (tid < T2) {
        const float* a = A + tid * kW;
        float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
        for (int m = 0; m < kW; m += 4) {
            e0 = fmaf(W.vt[m], a[m], e0);
            e1 = fmaf(W.vt[m + 1], a[m + 1], e1);
            e2 = fmaf(W.vt[m + 2], a[m + 2], e2);
            e3 = fmaf(W.vt[m + 3], a[m + 3], e3);
        }
        const float e = (e0 + e1) + (e2 + e3);
        small[sE + tid] = e;
        if (ts == 3) p.tape[(long)b * T2 + tid] = e;
    }
    __syncthreads();
    if (tid == 0) {
        float m = small[sE];
        for (int t = 1; t < T2; ++t) m = max_nan(small[sE + t], m);
        float sum = 0.f;
        for (int t = 0; t < T2; ++t) {
            const float v = expf(small[sE + t] - m);
            small[sE + t] = v;
            sum += v;
        }
        for (int t = 0; t < T2; ++t) small[sE + t] = small[sE + t] / sum;
    }
    __syncthreads();
    if (tid < kW) {
        float c = 0.f;
        for (int t = 0; t < T2; ++t) c = fmaf(small[sE + t], H1[t * kW + tid], c);
        small[sCtx + tid] = c;
    }
    __syncthreads();

    // ---- head: U ctx and log_softmax (class ascending); the first maximum decides, a NaN wins, the first one
    if (tid < kKwsOut) {
        float z0 = 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
        for (int k = 0; k < kW; k += 4) {
            z0 = fmaf(W.u[tid * kW + k], small[sCtx + k], z0);
            z1 = fmaf(W.u[tid * kW + k + 1], small[sCtx + k + 1], z1);
            z2 = fmaf(W.u[tid * kW + k + 2], small[sCtx + k + 2], z2);
            z3 = fmaf(W.u[tid * kW + k + 3], small[sCtx + k + 3], z3);
        }
        small[sHead + tid] = (z0 + z1) + (z2 + z3);
    }
    __syncthreads();
    if (tid == 0) {
        float m = small[sHead];
        int best = 0;
        for (int o = 1; o < kKwsOut; ++o) {
            const float z = small[sHead + o];
            m = max_nan(z, m);
            const float zb = small[sHead + best];
            if (z > zb || (z != z && zb == zb)) best = o;
        }
        float sum = 0.f;
        for (int o = 0; o < kKwsOut; ++o) sum += expf(small[sHead + o] - m);
        small[sHead + 12] = m + logf(sum);
        if (p.cls) p.cls[b] = best;
    }
    __syncthreads();
    if (tid < kKwsOut) {
        const float lp = small[sHead + tid] - small[sHead + 12];
        small[sHead + 4 + tid] = lp;
        if (p.logp) p.logp[(long)b * kKwsOut + tid] = lp;
    }
    if (!p.g_spec) return;
    __syncthreads();

    // ---- walk back.  log_softmax: g_z = g - softmax(z) sum(g); U^T; the context sum
    if (tid < kKwsOut) {
        const float* gl = p.g_logp + (long)b * kKwsOut;
        float sg = 0.f;
        for (int o = 0; o < kKwsOut; ++o) sg += gl[o];
        small[sHead + 8 + tid] = gl[tid] - expf(small[sHead + 4 + tid]) * sg;
    }
    __syncthreads();
    if (tid < kW) {
        float dc = 0.f;
        for (int o = 0; o < kKwsOut; ++o) dc = fmaf(W.u[o * kW + tid], small[sHead + 8 + o], dc);
        small[sDctx + tid] = dc;
    }
    __syncthreads();
    if (tid < T2) {                                   // da_t = dctx . o_t
        const float* o = H1 + tid * kW;
        float da = 0.f;
        for (int k = 0; k < kW; ++k) da = fmaf(small[sDctx + k], o[k], da);
        small[sDa + tid] = da;
    }
    __syncthreads();
    if (tid == 0) {                                   // softmax over time: de_t = a_t (da_t - sum_s a_s da_s)
        float dot = 0.f;
        for (int t = 0; t < T2; ++t) dot = fmaf(small[sE + t], small[sDa + t], dot);
        for (int t = 0; t < T2; ++t) small[sDa + t] = small[sE + t] * (small[sDa + t] - dot);
    }
    __syncthreads();
    for (int item = tid; item < kW * T2; item += kThreads) {        // Vt and tanh: A <- the gradient at Wx_b o_t + b
        const int m = item % kW, t = item / kW;
        const float a = A[item];
        A[item] = small[sDa + t] * W.vt[m] * (1.f - a * a);
    }
    __syncthreads();
    for (int item = tid; item < kW * T2; item += kThreads) {        // GH1[t][k] = a_t dctx[k] + sum_m Wx[m][k] A[t][m]
        const int k = item % kW, t = item / kW;
        const float* a = A + t * kW;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
        for (int m = 0; m < kW; m += 4) {
            const float4 x = *(const float4*)(a + m);
            a0 = fmaf(W.wx[m * kW + k], x.x, a0);
            a1 = fmaf(W.wx[(m + 1) * kW + k], x.y, a1);
            a2 = fmaf(W.wx[(m + 2) * kW + k], x.z, a2);
            a3 = fmaf(W.wx[(m + 3) * kW + k], x.w, a3);
        }
        GH1[item] = fmaf(small[sE + t], small[sDctx + k], (a0 + a1) + (a2 + a3));
    }
    __syncthreads();

    // ---- layer 1 (its input projections are still in GI), W_ih^T to layer 0's output, layer 0 on recomputed projections, W_ih^T to X0
    gru_backward(GI, W.whhT[1], W.whh[1], W.bhh[1], T2, H1, GH1, small);
    input_proj_back<kW>(GI, W.wih[1], T2, GH0);
    __syncthreads();
    input_proj<kKwsH>(X0, W.wihT[0], W.bih[0], T2, GI);
    __syncthreads();
    gru_backward(GI, W.whhT[0], W.whh[0], W.bhh[0], T2, H0, GH0, small);
    float* GX0 = GH1;                                 // [T2][64]
    input_proj_back<kKwsH>(GI, W.wih[0], T2, GX0);
    __syncthreads();

    // ---- the pointwise conv walked back (o ascending) to the depthwise frames [T2][32], which borrow GH0
    float* GD = GH0;
    for (int item = tid; item < kKwsIn * T2; item += kThreads) {
        const int c = item % kKwsIn, j = item / kKwsIn;
        const float* r = GX0 + j * kKwsH;
        float acc = 0.f;
#pragma unroll 8
        for (int o = 0; o < kKwsH; ++o) acc = fmaf(W.pw[o * kKwsIn + c], r[o], acc);
        GD[item] = acc;
    }
    __syncthreads();

    // ---- the depthwise conv: frame f = 16 j + k, k < 5, of channel c gets w[c][k] GD[j][c]; every other frame is an exact zero
    float* gs = p.g_spec + (long)b * kKwsIn * T;
    for (int i = tid; i < kKwsIn * T; i += kThreads) {
        const int c = i / T, f = i - c * T;
        const int j = f / kKwsHop, k = f - j * kKwsHop;
        gs[i] = (k < kKwsK && j < T2) ? W.dw[c * kKwsK + k] * GD[j * kKwsIn + c] : 0.f;
    }
}

}  // namespace

const char* kws_geometry(int T, KwsGeom* g) {
    if (T < kKwsMinT) return "T is below the depthwise kernel (5 frames)";
    if (T > kKwsMaxT) return "T is above kKwsMaxT (644 frames, 40 GRU steps): the activations do not fit the LDS of one CU";
    KwsGeom r;
    r.T = T;
    r.T1 = (T - kKwsK) / 2 + 1;
    r.T2 = (r.T1 - 1) / 8 + 1;
    r.oX0 = 0;
    r.oGI = r.oX0 + r.T2 * kKwsH;
    r.oH[0] = r.oGI + r.T2 * kThreads;
    r.oH[1] = r.oH[0] + r.T2 * kW;
    r.oGH[0] = r.oH[1] + r.T2 * kW;
    r.oGH[1] = r.oGH[0] + r.T2 * kW;
    r.oSmall = r.oGH[1] + r.T2 * kW;
    r.lds_bytes = (r.oSmall + kKwsSmall) * 4;
    if (r.lds_bytes > kMaxLds) return "T is too long: the activations do not fit the LDS of one CU";
    *g = r;
    return nullptr;
}

int kws_configure() { return set_max_lds({{(const void*)kws_kernel, kMaxLds}}); }      // KF_KWS (kernel_setup.hip, once per device)

void launch_kws(const KwsWeights& w, const KwsGeom& g, const float* spec, int B, float* logp, int32_t* cls, const float* g_logp,
                float* g_spec, int tape_stage, float* tape, hipStream_t s) {
    KwsParams p{w, g, spec, logp, cls, g_logp, g_spec, tape_stage, tape};
    hipLaunchKernelGGL(kws_kernel, dim3((unsigned)B), dim3(kThreads), (size_t)g.lds_bytes, s, p);
}

}  // namespace dmad
