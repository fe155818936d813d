// M5 forward and input VJP in one launch, one workgroup per clip (m5.h).
#include "m5.h"
#include "kernel_setup.h"
#include "philox.h"

namespace dmad {

namespace {

constexpr int kThreads = 512;            // 8 waves: two per SIMD
constexpr int kMaxLds = 160 * 1024;

struct M5Params {
    M5Weights w;
    M5Geom g;
    const float* x;
    float* logp;
    int32_t* cls;
    const float* g_logp;
    float* g_x;
    int tape_layer;
    float* pooled;
    uint8_t* dec;
    static constexpr bool kNoisy = false;
};

// The noisy-staging form (launch_m5_noisy): workgroup b evaluates Monte Carlo sample sample0 + b of the ONE clip x, forward and vote only
struct M5NoisyParams : M5Params {
    const float* delta;                  // [rows][L] caller's noise, or nullptr: sigma * Philox normal keyed (seed, sample0 + b)
    float sigma;
    uint64_t seed, sample0;
    unsigned long long* counts;          // [n_out]: the workgroup's decision is added here
    static constexpr bool kNoisy = true;
};

// BatchNorm (folded) -> ReLU -> the first maximum of four frames, as torch's max_pool1d scans them (a NaN wins and a later NaN replaces
// it); returns arg | on << 2
__device__ __forceinline__ int bn_relu_pool4(const float acc[4], float s, float sh, float* best_out) {
    float best = relu_nan(fmaf(acc[0], s, sh));
    int arg = 0;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const float r = relu_nan(fmaf(acc[j], s, sh));
        if (r > best || r != r) { best = r; arg = j; }
    }
    *best_out = best;
    return arg | ((best > 0.f) ? 4 : 0);
}

// Conv1d(CIN -> COUT, 3) on the pooled map `in` [CIN][pin] (LDS) -> BN -> ReLU -> MaxPool1d(4) -> out [COUT][pout] and the decisions
// dec [COUT][T].  One item = one output channel x one pooled frame (4 conv frames, 6 input frames); lanes run over the output channels,
// so the weights [ci][tap][co] are read coalesced through L2 and the input frames are LDS broadcasts.  ci, then tap, ascending
template <int CIN, int COUT>
__device__ __forceinline__ void conv3_pool(const float* in, int pin, const float* __restrict__ w, const float* __restrict__ scale,
                                           const float* __restrict__ shift, int T, float* out, int pout, uint8_t* dec, float* tape_p,
                                           uint8_t* tape_d) {
    for (int item = threadIdx.x; item < COUT * T; item += kThreads) {
        const int co = item % COUT, p = item / COUT;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const float* r = in + 4 * p;
#pragma unroll 4
        for (int ci = 0; ci < CIN; ++ci) {
            const float4 a = *(const float4*)(r + ci * pin);
            const float2 b = *(const float2*)(r + ci * pin + 4);
            const float v[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
            const float w0 = w[(ci * 3 + 0) * COUT + co], w1 = w[(ci * 3 + 1) * COUT + co], w2 = w[(ci * 3 + 2) * COUT + co];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[j] = fmaf(w0, v[j], acc[j]);
                acc[j] = fmaf(w1, v[j + 1], acc[j]);
                acc[j] = fmaf(w2, v[j + 2], acc[j]);
            }
        }
        float best;
        const int d = bn_relu_pool4(acc, scale[co], shift[co], &best);
        out[co * pout + p] = best;
        dec[co * T + p] = (uint8_t)d;
        if (tape_p) {
            tape_p[co * T + p] = best;
            tape_d[co * T + p] = (uint8_t)d;
        }
    }
}

// The same conv walked back: G [COUT][pg] holds the gradient at the conv's output frames (frame f at 2 + f, zero elsewhere), the result is
// the gradient at the conv's input, which is the previous layer's pooled map [CIN][Tin]; each value is routed at once through that
// layer's pool, ReLU and BatchNorm scale: to frame 4 t + arg of the previous dense map (frame f at 2 + f), or, `compact`, to [ci][t].
// Lanes run over the input channels (weights [co][tap][ci]); co, then tap, ascending
template <int CIN, int COUT>
__device__ __forceinline__ void conv3_back_route(const float* G, int pg, const float* __restrict__ w, int Tin, const uint8_t* dec_prev,
                                                 const float* __restrict__ scale_prev, float* Gprev, int pprev, bool compact) {
    const int TQ = (Tin + 3) >> 2;
    for (int item = threadIdx.x; item < CIN * TQ; item += kThreads) {
        const int ci = item % CIN, tq = item / CIN;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const float* r = G + 4 * tq;
#pragma unroll 4
        for (int co = 0; co < COUT; ++co) {
            const float4 a = *(const float4*)(r + co * pg);
            const float2 b = *(const float2*)(r + co * pg + 4);
            const float v[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
            const float w0 = w[(co * 3 + 0) * CIN + ci], w1 = w[(co * 3 + 1) * CIN + ci], w2 = w[(co * 3 + 2) * CIN + ci];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                  // input frame t = 4 tq + j meets output frame t - tap at slot j + 2 - tap
                acc[j] = fmaf(w0, v[j + 2], acc[j]);
                acc[j] = fmaf(w1, v[j + 1], acc[j]);
                acc[j] = fmaf(w2, v[j], acc[j]);
            }
        }
        const float s = scale_prev[ci];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = 4 * tq + j;
            if (t >= Tin) break;
            const int d = dec_prev[ci * Tin + t];
            const float val = (d & 4) ? acc[j] * s : 0.f;
            if (compact) Gprev[ci * pprev + t] = val;
            else if (d & 4) Gprev[ci * pprev + 2 + 4 * t + (d & 3)] = val;
        }
    }
}

// P = M5Params: one clip per workgroup.  P = M5NoisyParams: every workgroup reads the same clip and adds its own sample's noise while
// staging it; those branches are compile-time, so the M5Params kernel is the code it was without them
template <int K1, class P>
__global__ __launch_bounds__(kThreads) void m5_kernel(const P p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const M5Geom& g = p.g;
    const int tid = threadIdx.x, b = blockIdx.x, L = g.L;
    float* X = lds + g.oX;
    float* W1 = lds + g.oW1;
    float* small = lds + g.oSmall;       // [0,64) the time mean, [64,128) logits, [128] their log-sum-exp, [192,256) log-probabilities
    uint8_t* decs = (uint8_t*)lds + g.decB;
    const int tl = p.tape_layer;
    const int T1 = g.T[0];

    // ---- the clip, padded by one 16-byte slot per 64 samples (pooled frames 64 samples apart then sit on different banks), and conv1 [k][32]
    if constexpr (P::kNoisy) {           // clip + noise, in registers: the noisy clip exists in LDS only
        const float* dg = p.delta ? p.delta + (long)b * L : nullptr;
        for (int i = 4 * tid; i < L; i += 4 * kThreads)
            *(float4*)(X + i + ((i >> 6) << 2)) = noisy4(*(const float4*)(p.x + i), dg ? dg + i : nullptr, p.sigma, p.seed, p.sample0 + (uint64_t)b, (uint32_t)(i >> 2));
    } else {
        const float* xg = p.x + (long)b * L;
        for (int i = 4 * tid; i < L; i += 4 * kThreads) *(float4*)(X + i + ((i >> 6) << 2)) = *(const float4*)(xg + i);
    }
    for (int i = 4 * tid; i < K1 * kM5Ch; i += 4 * kThreads) *(float4*)(W1 + i) = *(const float4*)(p.w.w1t + i);
    __syncthreads();

    // ---- conv1 (stride 16) -> BN -> ReLU -> pool: one item = 4 channels x one pooled frame (4 conv frames); k ascending
    {
        float* P1 = lds + g.oP[0];
        uint8_t* d1 = decs + g.oDec[0];
        const int pit = g.pit[0];
        float* tp = tl == 1 ? p.pooled + (long)b * kM5Ch * T1 : nullptr;
        uint8_t* td = tl == 1 ? p.dec + (long)b * kM5Ch * T1 : nullptr;
        for (int item = tid; item < 8 * T1; item += kThreads) {
            const int cg = item & 7, pp = item >> 3;
            float acc[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[j][c] = 0.f;
            const float* xb = X + 68 * pp;
            const float* wb = W1 + 4 * cg;
#pragma unroll 2
            for (int k = 0; k < K1; k += 4) {
                float4 wv[4], xv[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) wv[kk] = *(const float4*)(wb + (k + kk) * kM5Ch);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int m = 16 * j + k;
                    xv[j] = *(const float4*)(xb + m + ((m >> 6) << 2));
                }
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float xs = kk == 0 ? xv[j].x : kk == 1 ? xv[j].y : kk == 2 ? xv[j].z : xv[j].w;
                        acc[j][0] = fmaf(wv[kk].x, xs, acc[j][0]);
                        acc[j][1] = fmaf(wv[kk].y, xs, acc[j][1]);
                        acc[j][2] = fmaf(wv[kk].z, xs, acc[j][2]);
                        acc[j][3] = fmaf(wv[kk].w, xs, acc[j][3]);
                    }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int ch = 4 * cg + c;
                const float a4[4] = {acc[0][c], acc[1][c], acc[2][c], acc[3][c]};
                float best;
                const int d = bn_relu_pool4(a4, p.w.scale[0][ch], p.w.shift[0][ch], &best);
                P1[ch * pit + pp] = best;
                d1[ch * T1 + pp] = (uint8_t)d;
                if (tp) {
                    tp[ch * T1 + pp] = best;
                    td[ch * T1 + pp] = (uint8_t)d;
                }
            }
        }
        // the pad columns of a row are read by nobody: conv2 reads frames <= 4 p + 5 <= T1 - 1
    }
    __syncthreads();
    {
        const long o2 = (long)b * 32 * g.T[1], o3 = (long)b * 64 * g.T[2], o4 = (long)b * 64 * g.T[3];
        conv3_pool<32, 32>(lds + g.oP[0], g.pit[0], p.w.wf[0], p.w.scale[1], p.w.shift[1], g.T[1], lds + g.oP[1], g.pit[1], decs + g.oDec[1],
                           tl == 2 ? p.pooled + o2 : nullptr, tl == 2 ? p.dec + o2 : nullptr);
        __syncthreads();
        conv3_pool<32, 64>(lds + g.oP[1], g.pit[1], p.w.wf[1], p.w.scale[2], p.w.shift[2], g.T[2], lds + g.oP[2], g.pit[2], decs + g.oDec[2],
                           tl == 3 ? p.pooled + o3 : nullptr, tl == 3 ? p.dec + o3 : nullptr);
        __syncthreads();
        conv3_pool<64, 64>(lds + g.oP[2], g.pit[2], p.w.wf[2], p.w.scale[3], p.w.shift[3], g.T[3], lds + g.oP[3], g.pit[3], decs + g.oDec[3],
                           tl == 4 ? p.pooled + o4 : nullptr, tl == 4 ? p.dec + o4 : nullptr);
        __syncthreads();
    }

    // ---- head: the mean over time, Linear, log_softmax (c / class ascending)
    const int T4 = g.T[3], NO = g.n_out;
    if (tid < 64) {
        const float* r = lds + g.oP[3] + tid * g.pit[3];
        float sum = 0.f;
        for (int t = 0; t < T4; ++t) sum += r[t];
        small[tid] = sum / (float)T4;
    }
    __syncthreads();
    if (tid < NO) {
        float z = 0.f;
        for (int c = 0; c < 64; ++c) z = fmaf(p.w.fcw[tid * 64 + c], small[c], z);
        small[64 + tid] = z + p.w.fcb[tid];
    }
    __syncthreads();
    if (tid == 0) {
        float m = small[64];
        int best = 0;
        for (int o = 1; o < NO; ++o) {
            const float z = small[64 + o];
            m = max_nan(z, m);
            const float zb = small[64 + best];
            if (z > zb || (z != z && zb == zb)) best = o;       // the first maximum; a NaN wins, the first one
        }
        float sum = 0.f;
        for (int o = 0; o < NO; ++o) sum += expf(small[64 + o] - m);
        small[128] = m + logf(sum);
        if (p.cls) p.cls[b] = best;
        if constexpr (P::kNoisy) atomicAdd(&p.counts[best], 1ull);
    }
    __syncthreads();
    if (tid < NO) {
        const float lp = small[64 + tid] - small[128];
        small[192 + tid] = lp;
        if (p.logp) p.logp[(long)b * NO + tid] = lp;
    }
    if constexpr (P::kNoisy) return;
    if (!p.g_x) return;
    __syncthreads();

    // ---- walk back.  The arena overlays the clip, conv1's image and the pooled maps: only the decisions are read from here on
    for (int i = 4 * tid; i < g.oG[0]; i += 4 * kThreads) *(float4*)(lds + i) = float4{0.f, 0.f, 0.f, 0.f};
    for (int i = 4 * tid; i < K1 * kM5Ch; i += 4 * kThreads) *(float4*)(lds + g.oW1c + i) = *(const float4*)(p.w.w1c + i);
    if (tid < NO) {                                   // g_z = g - softmax(z) * sum(g)
        const float* gl = p.g_logp + (long)b * NO;
        float sg = 0.f;
        for (int o = 0; o < NO; ++o) sg += gl[o];
        small[64 + tid] = gl[tid] - expf(small[192 + tid]) * sg;
    }
    __syncthreads();
    if (tid < 64) {                                   // fc1^T, 1 / T, pool4 / ReLU / BN4
        float gm = 0.f;
        for (int o = 0; o < NO; ++o) gm = fmaf(p.w.fcw[o * 64 + tid], small[64 + o], gm);
        gm = gm / (float)T4;
        const uint8_t* d4 = decs + g.oDec[3];
        float* G4 = lds + g.oG[3] + tid * g.pitG[3];
        const float s4 = p.w.scale[3][tid];
        for (int t = 0; t < T4; ++t) {
            const int d = d4[tid * T4 + t];
            if (d & 4) G4[2 + 4 * t + (d & 3)] = gm * s4;
        }
    }
    __syncthreads();
    conv3_back_route<64, 64>(lds + g.oG[3], g.pitG[3], p.w.wb[2], g.T[2], decs + g.oDec[2], p.w.scale[2], lds + g.oG[2], g.pitG[2], false);
    __syncthreads();
    conv3_back_route<32, 64>(lds + g.oG[2], g.pitG[2], p.w.wb[1], g.T[1], decs + g.oDec[1], p.w.scale[1], lds + g.oG[1], g.pitG[1], false);
    __syncthreads();
    conv3_back_route<32, 32>(lds + g.oG[1], g.pitG[1], p.w.wb[0], T1, decs + g.oDec[0], p.w.scale[0], lds + g.oG[0], g.pitG[0], true);
    __syncthreads();

    // ---- conv1^T: a gather per sample.  Of the frames that cover sample n only one per pool window carries a gradient, frame 4 p + arg;
    // a wave walks the windows that touch its 64 samples (the same ones for every lane), channel then window ascending
    {
        const float* G1 = lds + g.oG[0];
        const float* W1c = lds + g.oW1c;
        const uint8_t* d1 = decs + g.oDec[0];
        float* gx = p.g_x + (long)b * L;
        const int lane = tid & 63, wave = tid >> 6;
        for (int n0 = 64 * wave; n0 < L; n0 += 64 * (kThreads / 64)) {
            const int n = n0 + lane, n1 = n0 + 63;
            const int f_lo = n0 >= K1 - 1 ? (n0 - K1 + 1 + kM5Stride - 1) / kM5Stride : 0;
            const int f_hi = n1 / kM5Stride;
            const int p_lo = f_lo >> 2;
            int p_hi = f_hi >> 2;
            if (p_hi > T1 - 1) p_hi = T1 - 1;
            float acc = 0.f;
            for (int c = 0; c < kM5Ch; ++c)
                for (int pp = p_lo; pp <= p_hi; ++pp) {
                    const float gv = G1[c * T1 + pp];
                    if (gv == 0.f) continue;                     // wave-uniform: a unit behind a dead ReLU, or no gradient
                    const int k = n - kM5Stride * (4 * pp + (d1[c * T1 + pp] & 3));
                    if ((unsigned)k < (unsigned)K1) acc = fmaf(W1c[c * K1 + k], gv, acc);
                }
            if (n < L) gx[n] = acc;
        }
    }
}

int up4(int v) { return (v + 3) & ~3; }

}  // namespace

const char* m5_geometry(int L, int K1, int n_out, M5Geom* g) {
    if (K1 != 80 && K1 != 160) return "first_kernel_size must be 80 or 160";
    if (n_out < 1 || n_out > kM5MaxOut) return "n_output must be in [1, 64]";
    if (L < K1 || L % 64) return "clip_len must be a multiple of 64 and at least first_kernel_size";
    M5Geom r;
    r.L = L; r.K1 = K1; r.n_out = n_out;
    r.Tc[0] = (L - K1) / kM5Stride + 1;
    for (int l = 0; l < 4; ++l) {
        if (l) r.Tc[l] = r.T[l - 1] - 2;
        r.T[l] = r.Tc[l] / 4;
        if (r.T[l] < 1 || (l < 3 && r.T[l] < 3)) return "clip_len is too short for the four conv / pool blocks";
        r.pit[l] = up4(r.T[l]);
        r.pitG[l] = l ? up4(r.Tc[l] + 2) + 4 : r.T[0];
    }
    r.oX = 0;
    r.oW1 = up4(L + (L / 64) * 4);
    r.oP[0] = r.oW1 + K1 * kM5Ch;
    for (int l = 1; l < 4; ++l) r.oP[l] = r.oP[l - 1] + r.C[l - 1] * r.pit[l - 1];
    const int fwd_end = r.oP[3] + r.C[3] * r.pit[3];
    r.oG[3] = 0;
    r.oG[2] = r.oG[3] + r.C[3] * r.pitG[3];
    r.oG[1] = r.oG[2] + r.C[2] * r.pitG[2];
    r.oG[0] = r.oG[1] + r.C[1] * r.pitG[1];
    r.oW1c = up4(r.oG[0] + r.C[0] * r.T[0]);
    const int bwd_end = r.oW1c + K1 * kM5Ch;
    r.oSmall = up4(fwd_end > bwd_end ? fwd_end : bwd_end);
    r.decB = (r.oSmall + 256) * 4;
    int db = 0;
    for (int l = 0; l < 4; ++l) {
        r.oDec[l] = db;
        db += r.C[l] * r.T[l];
    }
    r.lds_bytes = (r.decB + db + 15) & ~15;
    if (r.lds_bytes > kMaxLds) return "clip_len is too long: the clip and the activations do not fit the LDS of one CU";
    *g = r;
    return nullptr;
}

// KF_M5 (kernel_setup.hip, once per device)
int m5_configure() {
    return set_max_lds({{(const void*)m5_kernel<80, M5Params>, kMaxLds}, {(const void*)m5_kernel<160, M5Params>, kMaxLds},
                        {(const void*)m5_kernel<80, M5NoisyParams>, kMaxLds}, {(const void*)m5_kernel<160, M5NoisyParams>, kMaxLds}});
}

void launch_m5(const M5Weights& w, const M5Geom& g, const float* x, int B, float* logp, int32_t* cls, const float* g_logp, float* g_x,
               int tape_layer, float* pooled, uint8_t* dec, hipStream_t s) {
    M5Params p{w, g, x, logp, cls, g_logp, g_x, tape_layer, pooled, dec};
    if (g.K1 == 80) hipLaunchKernelGGL((m5_kernel<80, M5Params>), dim3((unsigned)B), dim3(kThreads), (size_t)g.lds_bytes, s, p);
    else hipLaunchKernelGGL((m5_kernel<160, M5Params>), dim3((unsigned)B), dim3(kThreads), (size_t)g.lds_bytes, s, p);
}

void launch_m5_noisy(const M5Weights& w, const M5Geom& g, const float* clip, const float* delta, float sigma, uint64_t seed, uint64_t sample0,
                     int rows, unsigned long long* counts, float* logp, hipStream_t s) {
    M5NoisyParams p{{w, g, clip, logp, nullptr, nullptr, nullptr, 0, nullptr, nullptr}, delta, sigma, seed, sample0, counts};
    if (g.K1 == 80) hipLaunchKernelGGL((m5_kernel<80, M5NoisyParams>), dim3((unsigned)rows), dim3(kThreads), (size_t)g.lds_bytes, s, p);
    else hipLaunchKernelGGL((m5_kernel<160, M5NoisyParams>), dim3((unsigned)rows), dim3(kThreads), (size_t)g.lds_bytes, s, p);
}

}  // namespace dmad
