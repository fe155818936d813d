// See densenet.h.
#include "densenet.h"

namespace dmad {

namespace {
typedef __attribute__((ext_vector_type(4))) float dn_f32x4;
inline unsigned nblk(long n, int b) { return (unsigned)((n + b - 1) / b); }

// v_mfma_f32_16x16x4_f32: lane l gives A[l & 15][l >> 4] and B[l >> 4][l & 15]; D: column l & 15, rows 4 (l >> 4) + r
__device__ __forceinline__ dn_f32x4 mfma4(float a, float b, dn_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// ---- the 1x1 product: 64 pixels x up to 64 output channels per workgroup (4 waves of 16 pixels, 4 row tiles each), K in chunks of 48.
// LDS rows of 50 floats: 50 = 18 mod 32 and 18 row mod 32 is even and different for the 16 rows, so the 16 rows x 2 k of a half wave fall
// on 32 different banks, and a float2 store stays aligned.
constexpr int kPwKC = 48, kPwP = 50;

template <bool BWD>
__global__ __launch_bounds__(256) void dn_pw_kernel(const DnPwArgs a) {
    __shared__ float As[64 * kPwP];
    __shared__ float Bs[64 * kPwP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = lane & 15, kq = lane >> 4;
    const long px0 = (long)blockIdx.x * 64;
    const int m0 = blockIdx.y * 64;
    const int left = (a.M - m0 + 15) >> 4, ntile = left < 4 ? left : 4;
    dn_f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = dn_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < a.K4; k0 += kPwKC) {
        const int kc = (a.K4 - k0) < kPwKC ? (a.K4 - k0) : kPwKC, kc2 = kc >> 1;      // kc: a multiple of 4
        for (int i = tid; i < ntile * 16 * kc2; i += 256) {
            const int r = i / kc2, k = (i - r * kc2) * 2, m = m0 + r;
            float2 v = make_float2(0.f, 0.f);
            if (m < a.M) v = *(const float2*)(a.A + (size_t)m * a.K4 + k0 + k);
            *(float2*)(As + r * kPwP + k) = v;
        }
        for (int i = tid; i < 64 * kc2; i += 256) {
            const int p = i / kc2, k = (i - p * kc2) * 2, kk = k0 + k;
            const long px = px0 + p;
            float2 v = make_float2(0.f, 0.f);
            if (px < a.n_px && kk < a.K) {                   // K is even: kk + 1 < K too.  Behind K: exact zeros, nothing is loaded
                if (!BWD) {
                    const float2 xv = *(const float2*)(a.in + px * a.ldi + kk);
                    v.x = dn_preact(a.s_in[kk], xv.x, a.b_in[kk]);
                    v.y = dn_preact(a.s_in[kk + 1], xv.y, a.b_in[kk + 1]);
                } else if (a.pool) {
                    const int H = a.H, hw = H * H;
                    const long b = px / hw;
                    const int rem = (int)(px - b * hw), y = rem / H, x = rem - y * H, Hh = H >> 1;
                    const long q = (b * Hh + (y >> 1)) * Hh + (x >> 1);
                    const float2 g = *(const float2*)(a.in + q * a.ldi + kk);
                    v = make_float2(0.25f * g.x, 0.25f * g.y);
                } else {
                    v = *(const float2*)(a.in + px * a.ldi + kk);
                }
            }
            *(float2*)(Bs + p * kPwP + k) = v;
        }
        __syncthreads();
        const float* bp = Bs + (wave * 16 + row) * kPwP + kq;
        const float* ap = As + row * kPwP + kq;
        for (int k = 0; k < kc; k += 4) {
            const float b = bp[k];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < ntile) acc[t] = mfma4(ap[t * 16 * kPwP + k], b, acc[t]);
        }
        __syncthreads();
    }
    const long px = px0 + wave * 16 + row;
    if (px >= a.n_px) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t >= ntile) break;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + t * 16 + kq * 4 + r;
            if (m >= a.M) continue;
            const float v = acc[t][r];
            float* o = a.out + px * a.ldo + m;
            if (!BWD) {
                *o = a.s_out ? dn_preact(a.s_out[m], v, a.b_out[m]) : v;
            } else {
                const float s = a.s1[m];
                const float d = dn_preact(s, a.x[px * a.ldx + m], a.b1[m]) > 0.f ? s * v : 0.f;
                *o = a.add ? *o + d : d;
            }
        }
    }
}

// ---- the 3x3 conv: 64 consecutive pixels of one image per workgroup (64 / H rows), their halo rows staged with the KC channels of the
// operand; one accumulation chain per row tile: taps in (ky, kx) order, then channels.  LDS pitches 9 KC + 2 and KC + 2 (434 / 50 forward,
// 110 / 14 backward): 2 x an odd number, so 16 rows x 2 k of a half wave fall on 32 different banks.
template <int KC, int MT, bool BWD>
__global__ __launch_bounds__(256) void dn_c3_kernel(const float* __restrict__ A, const float* __restrict__ in, int ldi, int off, int H, int lh,
                                                    const float* __restrict__ hmap, const float* __restrict__ s2, float* __restrict__ out, int ldo) {
    constexpr int KT = 9 * KC, AP = KT + 2, BP = KC + 2, KC2 = KC / 2;
    __shared__ float As[MT * 16 * AP];
    __shared__ float Bs[128 * BP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = lane & 15, kq = lane >> 4;
    const long px0 = (long)blockIdx.x * 64;
    const int hw = H * H, R = 64 >> lh;
    const long b = px0 / hw;
    const int y0 = (int)(px0 - b * hw) >> lh;
    for (int i = tid; i < MT * 16 * (KT / 2); i += 256) {
        const int r = i / (KT / 2), k = (i - r * (KT / 2)) * 2;
        *(float2*)(As + r * AP + k) = *(const float2*)(A + (size_t)r * KT + k);
    }
    for (int i = tid; i < (R + 2) * H * KC2; i += 256) {
        const int sp = i / KC2, k = (i - sp * KC2) * 2;
        const int y = y0 - 1 + (sp >> lh), x = sp & (H - 1);
        float2 v = make_float2(0.f, 0.f);
        if ((unsigned)y < (unsigned)H) v = *(const float2*)(in + ((b * H + y) * H + x) * ldi + off + k);
        *(float2*)(Bs + sp * BP + k) = v;
    }
    __syncthreads();
    const int p = wave * 16 + row, yl = p >> lh, x = p & (H - 1);
    dn_f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = dn_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3, sx = x + kx - 1;
        const bool ok = (unsigned)sx < (unsigned)H;              // rows outside the image are staged as zeros
        const float* bp = Bs + (ok ? ((yl + ky) << lh) + sx : 0) * BP + kq;
        const float* ap = As + row * AP + tap * KC + kq;
#pragma unroll
        for (int c = 0; c < KC; c += 4) {
            const float bv = ok ? bp[c] : 0.f;
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[t] = mfma4(ap[t * 16 * AP + c], bv, acc[t]);
        }
    }
    const long px = px0 + p;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = t * 16 + kq * 4 + r;
            if (!BWD) {
                if (m < 12) out[px * ldo + off + m] = acc[t][r];
            } else {
                out[px * 48 + m] = hmap[px * 48 + m] > 0.f ? s2[m] * acc[t][r] : 0.f;
            }
        }
}

// one float4 of the 24 output channels of one pixel: i = (b, y, x, c4 < 6)
__global__ void dn_stem_kernel(const float* __restrict__ spec, const float* __restrict__ w, float* __restrict__ out, int ld, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c0 = (int)(i % 6) * 4;
    const long p = i / 6, b = p >> 10;
    const int y = (int)((p >> 5) & 31), x = (int)(p & 31);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y + ky - 1, xx = x + kx - 1;
            if ((unsigned)yy >= 32u || (unsigned)xx >= 32u) continue;
            const float v = spec[(b << 10) + yy * 32 + xx];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = fmaf(w[(c0 + r) * 9 + ky * 3 + kx], v, acc[r]);
        }
    *(float4*)(out + p * ld + c0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// one input pixel (b, y, x): nine taps of 24 channels, six float4 loads per tap
__global__ void dn_stem_bwd_kernel(const float* __restrict__ g, int ld, const float* __restrict__ w, float* __restrict__ gspec, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long b = i >> 10;
    const int y = (int)((i >> 5) & 31), x = (int)(i & 31);
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y + 1 - ky, xx = x + 1 - kx;
            if ((unsigned)yy >= 32u || (unsigned)xx >= 32u) continue;
            const float* gp = g + ((b << 10) + yy * 32 + xx) * ld;
            const int t = ky * 3 + kx;
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const float4 v = *(const float4*)(gp + q * 4);
                const int c = q * 4;
                acc = fmaf(w[c * 9 + t], v.x, acc);
                acc = fmaf(w[(c + 1) * 9 + t], v.y, acc);
                acc = fmaf(w[(c + 2) * 9 + t], v.z, acc);
                acc = fmaf(w[(c + 3) * 9 + t], v.w, acc);
            }
        }
    gspec[i] = acc;
}

// one channel of one pooled pixel
__global__ void dn_pool_kernel(const float* __restrict__ t, int ldt, float* __restrict__ out, int ldo, int H, int C, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C), Hh = H >> 1;
    const long q = i / C, b = q / (Hh * Hh);
    const int rem = (int)(q - b * Hh * Hh), y = rem / Hh, x = rem - y * Hh;
    const float* p = t + ((b * H + 2 * y) * H + 2 * x) * ldt + c;
    out[q * ldo + c] = 0.25f * (((p[0] + p[ldt]) + p[(long)H * ldt]) + p[(long)(H + 1) * ldt]);
}

__global__ void dn_preact_map_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ scale, const float* __restrict__ shift,
                                     float* __restrict__ out, int C, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    out[i] = dn_preact(scale[c], x[(i / C) * ldx + c], shift[c]);
}

// one workgroup per spectrogram: thread c pools its channel over the pixels in ascending order, then thread k runs class k's chain
__global__ __launch_bounds__(384) void dn_head_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ bns, const float* __restrict__ bnb,
                                                      const float* __restrict__ fcw, const float* __restrict__ fcb, float* __restrict__ logits, int HW,
                                                      int C, int ncls) {
    __shared__ float pooled[384];
    const int b = blockIdx.x, c = threadIdx.x;
    if (c < C) {
        const float sc = bns[c], sh = bnb[c];
        const float* p = x + (long)b * HW * ldx + c;
        float sum = 0.f;
        for (int i = 0; i < HW; ++i) sum += dn_preact(sc, p[(long)i * ldx], sh);
        pooled[c] = sum * (1.f / (float)HW);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < ncls; k += blockDim.x) {
        float acc = fcb[k];
        for (int j = 0; j < C; ++j) acc = fmaf(fcw[(long)k * C + j], pooled[j], acc);
        logits[(long)b * ncls + k] = acc;
    }
}

__global__ void dn_head_bwd_kernel(const float* __restrict__ g_logits, const float* __restrict__ fcws, const float* __restrict__ x, int ldx,
                                   const float* __restrict__ bns, const float* __restrict__ bnb, float* __restrict__ g, int ldg, int HW, int C,
                                   int ncls, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const long px = i / C, b = px / HW;
    float acc = 0.f;
    for (int k = 0; k < ncls; ++k) acc = fmaf(fcws[(long)k * C + c], g_logits[b * ncls + k], acc);
    g[px * ldg + c] = dn_preact(bns[c], x[px * ldx + c], bnb[c]) > 0.f ? acc * (1.f / (float)HW) : 0.f;
}

inline int log2i(int H) { return H == 32 ? 5 : H == 16 ? 4 : 3; }
}  // namespace

void launch_dn_pw(const DnPwArgs& a, bool bwd, hipStream_t s) {
    const dim3 grid(nblk(a.n_px, 64), (unsigned)((a.M + 63) / 64));
    if (bwd) hipLaunchKernelGGL(dn_pw_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dn_pw_kernel<false>, grid, dim3(256), 0, s, a);
}

void launch_dn_growth(const float* A, const float* h, float* stream, int lds, int off, int B, int H, hipStream_t s) {
    hipLaunchKernelGGL((dn_c3_kernel<48, 1, false>), dim3((unsigned)((long)B * H * H / 64)), dim3(256), 0, s, A, h, 48, 0, H, log2i(H),
                       (const float*)nullptr, (const float*)nullptr, stream + off, lds);
}

void launch_dn_growth_bwd(const float* A, const float* g, int lds, int off, const float* h, const float* s2, float* gh, int B, int H, hipStream_t s) {
    hipLaunchKernelGGL((dn_c3_kernel<12, 3, true>), dim3((unsigned)((long)B * H * H / 64)), dim3(256), 0, s, A, g, lds, off, H, log2i(H), h, s2, gh, 48);
}

void launch_dn_stem(const float* spec, const float* w, float* stream, int ld, int B, hipStream_t s) {
    const long total = (long)B * 1024 * 6;
    hipLaunchKernelGGL(dn_stem_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, spec, w, stream, ld, total);
}

void launch_dn_stem_bwd(const float* g, int ld, const float* w, float* gspec, int B, hipStream_t s) {
    const long total = (long)B * 1024;
    hipLaunchKernelGGL(dn_stem_bwd_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, g, ld, w, gspec, total);
}

void launch_dn_pool(const float* t, int ldt, float* out, int ldo, int B, int H, int C, hipStream_t s) {
    const long total = (long)B * (H / 2) * (H / 2) * C;
    hipLaunchKernelGGL(dn_pool_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, t, ldt, out, ldo, H, C, total);
}

void launch_dn_preact_map(const float* x, int ldx, const float* scale, const float* shift, float* out, long n_px, int C, hipStream_t s) {
    const long total = n_px * C;
    hipLaunchKernelGGL(dn_preact_map_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, x, ldx, scale, shift, out, C, total);
}

void launch_dn_head(const float* x, int ldx, const float* bns, const float* bnb, const float* fcw, const float* fcb, float* logits, int B, int HW,
                    int C, int ncls, hipStream_t s) {
    hipLaunchKernelGGL(dn_head_kernel, dim3((unsigned)B), dim3(384), 0, s, x, ldx, bns, bnb, fcw, fcb, logits, HW, C, ncls);
}

void launch_dn_head_bwd(const float* g_logits, const float* fcws, const float* x, int ldx, const float* bns, const float* bnb, float* g, int ldg,
                        int B, int HW, int C, int ncls, hipStream_t s) {
    const long total = (long)B * HW * C;
    hipLaunchKernelGGL(dn_head_bwd_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, g_logits, fcws, x, ldx, bns, bnb, g, ldg, HW, C, ncls, total);
}

}  // namespace dmad
