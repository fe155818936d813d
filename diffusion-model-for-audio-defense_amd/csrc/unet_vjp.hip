// See unet_vjp.h.
#include "unet_vjp.h"
#include "kernel_setup.h"

namespace dmad {

namespace {
inline unsigned nblk(long n, int b) { return (unsigned)((n + b - 1) / b); }

__global__ void unvjp_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int n0, int n1, int n2, long s0, long s1, long s2,
                                  int flip, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int i2 = (int)(i % n2);
    long r = i / n2;
    int i1 = (int)(r % n1);
    int i0 = (int)(r / n1);
    if (flip & 1) i0 = n0 - 1 - i0;
    if (flip & 2) i1 = n1 - 1 - i1;
    if (flip & 4) i2 = n2 - 1 - i2;
    dst[i] = src[s0 * i0 + s1 * i1 + s2 * i2];
}

// fixed-order sum over the 256 threads of a workgroup (a pairwise tree in LDS); every thread gets the result
template <int N>
__device__ void block_sum256(float (&v)[N], float (*red)[256]) {
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) red[k][t] = v[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int k = 0; k < N; ++k) red[k][t] += red[k][t + w];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = red[k][0];
}

// One workgroup per (group, sample): the group's HW x C/32 values are walked four times (statistics, then the two gradient sums, then
// the output), each thread in the same element order, from L2 after the first pass (<= 48 KiB per group).
__global__ void __launch_bounds__(256) groupnorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ x2, int c1,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ ss, int silu, const float* __restrict__ gy,
                                                            const float* __restrict__ add, const float* __restrict__ add2,
                                                            float* __restrict__ gx, float* __restrict__ gx2, int HW, int C) {
    __shared__ float red[2][256];
    const int grp = blockIdx.x, t = threadIdx.x, Cg = C >> 5;
    const long b = blockIdx.y;
    const int n = HW * Cg, c2 = C - c1;
    auto xat = [&](int e, long& pix, int& c) -> float {
        const int p = e / Cg;
        c = grp * Cg + e % Cg;
        pix = b * HW + p;
        return c < c1 ? x[pix * c1 + c] : x2[pix * c2 + (c - c1)];
    };
    float s1[1] = {0.f};
    for (int e = t; e < n; e += 256) { long pix; int c; s1[0] += xat(e, pix, c); }
    block_sum256(s1, red);
    const float mean = s1[0] / (float)n;
    float s2[1] = {0.f};
    for (int e = t; e < n; e += 256) { long pix; int c; const float d = xat(e, pix, c) - mean; s2[0] = fmaf(d, d, s2[0]); }
    block_sum256(s2, red);
    const float rstd = 1.0f / sqrtf(s2[0] / (float)n + 1e-5f);
    // gh = dL/d(xhat) of one value;  xh = xhat
    auto grad = [&](int e, float& xh, long& pix, int& c) -> float {
        xh = (xat(e, pix, c) - mean) * rstd;
        float g = gy[pix * C + c];
        float sc = 1.f;
        if (ss) sc = 1.f + ss[c];
        if (silu) {
            float u = xh * gamma[c] + beta[c];
            if (ss) u = u * sc + ss[C + c];
            const float sg = 1.f / (1.f + expf(-u));
            g *= sg * (1.f + u * (1.f - sg));
        }
        return g * sc * gamma[c];
    };
    float acc[2] = {0.f, 0.f};
    for (int e = t; e < n; e += 256) {
        float xh; long pix; int c;
        const float g = grad(e, xh, pix, c);
        acc[0] += g;
        acc[1] = fmaf(g, xh, acc[1]);
    }
    block_sum256(acc, red);
    const float mg = acc[0] / (float)n, mgx = acc[1] / (float)n;
    for (int e = t; e < n; e += 256) {
        float xh; long pix; int c;
        const float g = grad(e, xh, pix, c);
        float v = rstd * (g - mg - xh * mgx);
        if (add) v += add[pix * C + c];
        if (add2) v += add2[pix * C + c];
        if (c < c1) gx[pix * c1 + c] = v;
        else gx2[pix * c2 + (c - c1)] = v;
    }
}

// QKVAttention backward, one workgroup per (head, sample), one thread per row (T = 256: 256 threads; smaller T: 64, the rest idle).
// Phase A, thread i = query row i, K and V of the head in LDS:   s_ij = (q_i / 8) . k_j,  p_ij = exp(s_ij - m_i) / l_i,
//   dp_ij = dO_i . v_j,  D_i = sum_j p_ij dp_ij,  dq_i = (1/8) sum_j p_ij (dp_ij - D_i) k_j
// Phase B, thread j = key row j, Q / 8 and dO of the head in LDS (m, 1/l, D of every row beside them):
//   dv_j = sum_i p_ij dO_i,  dk_j = sum_i p_ij (dp_ij - D_i) q_i / 8
// (the reference's 1/sqrt(sqrt(64)) on q and on k: 1/8 on their product, taken on q as the forward kernel does).  Every sum runs over
// the rows in index order inside one thread: nothing is reduced across threads, nothing through memory.  The row reads of the inner
// loops are wave-uniform LDS addresses (broadcasts).
constexpr int HD = 64;
__global__ void __launch_bounds__(256) qkv_attention_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ go, float* __restrict__ gqkv,
                                                                int T, int heads) {
    extern __shared__ __attribute__((aligned(16))) float ab_lds[];
    float* R1 = ab_lds;                       // phase A: K rows, phase B: Q / 8 rows    [T][64]
    float* R2 = ab_lds + T * HD;              // phase A: V rows, phase B: dO rows       [T][64]
    float* Sm = ab_lds + 2 * T * HD;          // [T]: m_i, then [T]: 1 / l_i, then [T]: D_i
    float* Sl = Sm + T;
    float* Sd = Sl + T;
    const int h = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const long b = blockIdx.y;
    const int C3 = 3 * HD * heads, CO = HD * heads;
    const float* base = qkv + b * T * C3 + h * 3 * HD;
    const float* gbase = go + b * T * CO + h * HD;
    float* obase = gqkv + b * T * C3 + h * 3 * HD;
    for (int i = tid; i < T * 16; i += nt) {
        const int r = i >> 4, c4 = (i & 15) * 4;
        *(float4*)(R1 + r * HD + c4) = *(const float4*)(base + (long)r * C3 + HD + c4);
        *(float4*)(R2 + r * HD + c4) = *(const float4*)(base + (long)r * C3 + 2 * HD + c4);
    }
    __syncthreads();
    const int row = tid < T ? tid : T - 1;    // idle threads shadow the last row (loads only) and store nothing
    {
        float q[HD], g[HD], dq[HD];
#pragma unroll
        for (int c = 0; c < HD; c += 4) {
            const float4 v = *(const float4*)(base + (long)row * C3 + c), w = *(const float4*)(gbase + (long)row * CO + c);
            q[c] = v.x * 0.125f; q[c + 1] = v.y * 0.125f; q[c + 2] = v.z * 0.125f; q[c + 3] = v.w * 0.125f;
            g[c] = w.x; g[c + 1] = w.y; g[c + 2] = w.z; g[c + 3] = w.w;
            dq[c] = dq[c + 1] = dq[c + 2] = dq[c + 3] = 0.f;
        }
        auto dot = [&](const float* a, const float* r) -> float {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < HD; c += 4) {
                const float4 k = *(const float4*)(r + c);
                s = fmaf(a[c], k.x, s); s = fmaf(a[c + 1], k.y, s); s = fmaf(a[c + 2], k.z, s); s = fmaf(a[c + 3], k.w, s);
            }
            return s;
        };
        float m = -INFINITY;
        for (int j = 0; j < T; ++j) m = fmaxf(m, dot(q, R1 + j * HD));
        float l = 0.f, de = 0.f;
        for (int j = 0; j < T; ++j) {
            const float ex = expf(dot(q, R1 + j * HD) - m);
            l += ex;
            de = fmaf(ex, dot(g, R2 + j * HD), de);
        }
        const float inv = 1.f / l, D = de * inv;
        for (int j = 0; j < T; ++j) {
            const float p = expf(dot(q, R1 + j * HD) - m) * inv;
            const float ds = p * (dot(g, R2 + j * HD) - D);
            const float* kr = R1 + j * HD;
#pragma unroll
            for (int c = 0; c < HD; ++c) dq[c] = fmaf(ds, kr[c], dq[c]);
        }
        if (tid < T) {
#pragma unroll
            for (int c = 0; c < HD; c += 4)
                *(float4*)(obase + (long)row * C3 + c) = float4{dq[c] * 0.125f, dq[c + 1] * 0.125f, dq[c + 2] * 0.125f, dq[c + 3] * 0.125f};
            Sm[row] = m; Sl[row] = inv; Sd[row] = D;
        }
    }
    __syncthreads();
    for (int i = tid; i < T * 16; i += nt) {
        const int r = i >> 4, c4 = (i & 15) * 4;
        const float4 v = *(const float4*)(base + (long)r * C3 + c4);
        *(float4*)(R1 + r * HD + c4) = float4{v.x * 0.125f, v.y * 0.125f, v.z * 0.125f, v.w * 0.125f};
        *(float4*)(R2 + r * HD + c4) = *(const float4*)(gbase + (long)r * CO + c4);
    }
    __syncthreads();
    {
        float k[HD], acc[HD];
#pragma unroll
        for (int c = 0; c < HD; c += 4) {
            const float4 v = *(const float4*)(base + (long)row * C3 + HD + c);
            k[c] = v.x; k[c + 1] = v.y; k[c + 2] = v.z; k[c + 3] = v.w;
            acc[c] = acc[c + 1] = acc[c + 2] = acc[c + 3] = 0.f;
        }
        auto dotr = [&](const float* a, const float* r) -> float {      // sum_c r[c] * a[c]: the same products as phase A's s_ij
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < HD; c += 4) {
                const float4 w = *(const float4*)(r + c);
                s = fmaf(w.x, a[c], s); s = fmaf(w.y, a[c + 1], s); s = fmaf(w.z, a[c + 2], s); s = fmaf(w.w, a[c + 3], s);
            }
            return s;
        };
        // dv_j = sum_i p_ij dO_i
        for (int i = 0; i < T; ++i) {
            const float p = expf(dotr(k, R1 + i * HD) - Sm[i]) * Sl[i];
            const float* gr = R2 + i * HD;
#pragma unroll
            for (int c = 0; c < HD; ++c) acc[c] = fmaf(p, gr[c], acc[c]);
        }
        if (tid < T) {
#pragma unroll
            for (int c = 0; c < HD; c += 4) *(float4*)(obase + (long)row * C3 + 2 * HD + c) = float4{acc[c], acc[c + 1], acc[c + 2], acc[c + 3]};
        }
        // dk_j = sum_i p_ij (dp_ij - D_i) q_i / 8   (v_j re-read: registers hold k_j, v_j and the accumulator)
        float v[HD];
#pragma unroll
        for (int c = 0; c < HD; c += 4) {
            const float4 w = *(const float4*)(base + (long)row * C3 + 2 * HD + c);
            v[c] = w.x; v[c + 1] = w.y; v[c + 2] = w.z; v[c + 3] = w.w;
            acc[c] = acc[c + 1] = acc[c + 2] = acc[c + 3] = 0.f;
        }
        for (int i = 0; i < T; ++i) {
            const float p = expf(dotr(k, R1 + i * HD) - Sm[i]) * Sl[i];
            const float ds = p * (dotr(v, R2 + i * HD) - Sd[i]);
            const float* qr = R1 + i * HD;
#pragma unroll
            for (int c = 0; c < HD; ++c) acc[c] = fmaf(ds, qr[c], acc[c]);
        }
        if (tid < T) {
#pragma unroll
            for (int c = 0; c < HD; c += 4) *(float4*)(obase + (long)row * C3 + HD + c) = float4{acc[c], acc[c + 1], acc[c + 2], acc[c + 3]};
        }
    }
}

__global__ void dilate2x_nhwc_kernel(const float* __restrict__ g, float* __restrict__ d, int Ho, int C4, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // one float4 of d
    if (i >= total4) return;
    const int c = (int)(i % C4);
    long p = i / C4;
    const int xo = (int)(p % (2 * Ho)); p /= 2 * Ho;
    const int yo = (int)(p % (2 * Ho));
    const long b = p / (2 * Ho);
    float4 v = float4{0.f, 0.f, 0.f, 0.f};
    if (!(xo & 1) && !(yo & 1)) v = ((const float4*)g)[((b * Ho + (yo >> 1)) * Ho + (xo >> 1)) * C4 + c];
    ((float4*)d)[i] = v;
}

__global__ void upsample2x_bwd_nhwc_kernel(const float* __restrict__ g, const float* __restrict__ add, float* __restrict__ gin, int H, int C4, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // one float4 of gin
    if (i >= total4) return;
    const int c = (int)(i % C4);
    long p = i / C4;
    const int x = (int)(p % H); p /= H;
    const int y = (int)(p % H);
    const long b = p / H;
    const float4* G = (const float4*)g;
    const long r0 = (b * 2 * H + 2 * y) * 2 * H + 2 * x, r1 = r0 + 2 * H;
    const float4 a = G[r0 * C4 + c], e = G[(r0 + 1) * C4 + c], f = G[r1 * C4 + c], h = G[(r1 + 1) * C4 + c];
    float4 v = float4{((a.x + e.x) + f.x) + h.x, ((a.y + e.y) + f.y) + h.y, ((a.z + e.z) + f.z) + h.z, ((a.w + e.w) + f.w) + h.w};
    if (add) { const float4 q = ((const float4*)add)[i]; v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
    ((float4*)gin)[i] = v;
}
}  // namespace

void launch_unvjp_pack(const float* src, float* dst, int n0, int n1, int n2, long s0, long s1, long s2, int flip, hipStream_t s) {
    const long total = (long)n0 * n1 * n2;
    hipLaunchKernelGGL(unvjp_pack_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, src, dst, n0, n1, n2, s0, s1, s2, flip, total);
}

int launch_groupnorm_bwd(const float* x, const float* x2, int c1, const float* gamma, const float* beta, const float* ss, int silu,
                         const float* gy, const float* add, const float* add2, float* gx, float* gx2, int B, int HW, int C, hipStream_t s) {
    if (C % 32 || C < 32 || B < 1 || HW < 1) return -1;
    if (x2 && (c1 < 1 || c1 >= C || !gx2)) return -1;
    if (!x2) c1 = C;
    hipLaunchKernelGGL(groupnorm_bwd_kernel, dim3(32u, (unsigned)B), dim3(256), 0, s, x, x2, c1, gamma, beta, ss, silu, gy, add, add2, gx, gx2, HW, C);
    return 0;
}

static size_t att_bwd_lds(int T) { return ((size_t)2 * T * HD + 3 * T) * sizeof(float); }

int unvjp_configure() {
    return set_max_lds({{(const void*)qkv_attention_bwd_kernel, (int)att_bwd_lds(256)}});
}

int launch_qkv_attention_bwd(const float* qkv, const float* go, float* gqkv, int B, int T, int heads, hipStream_t s) {
    if (T != 256 && T != 64 && T != 16) return -1;
    hipLaunchKernelGGL(qkv_attention_bwd_kernel, dim3((unsigned)heads, (unsigned)B), dim3(T > 64 ? T : 64), att_bwd_lds(T), s, qkv, go, gqkv, T, heads);
    return 0;
}

void launch_dilate2x_nhwc(const float* g, float* d, int B, int Ho, int C, hipStream_t s) {
    const long total4 = (long)B * 4 * Ho * Ho * (C / 4);
    hipLaunchKernelGGL(dilate2x_nhwc_kernel, dim3(nblk(total4, 256)), dim3(256), 0, s, g, d, Ho, C / 4, total4);
}

void launch_upsample2x_bwd_nhwc(const float* g, const float* add, float* gin, int B, int H, int C, hipStream_t s) {
    const long total4 = (long)B * H * H * (C / 4);
    hipLaunchKernelGGL(upsample2x_bwd_nhwc_kernel, dim3(nblk(total4, 256)), dim3(256), 0, s, g, add, gin, H, C / 4, total4);
}

}  // namespace dmad
