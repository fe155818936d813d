// See wrn.h.
#include "wrn.h"

namespace dmad {

namespace {
inline unsigned nblk(long n, int b) { return (unsigned)((n + b - 1) / b); }

// one float4 of channels of one pixel; c4 = i % C4 picks its scale / shift
__global__ void wrn_preact_kernel(const float4* __restrict__ x, const float4* __restrict__ scale, const float4* __restrict__ shift,
                                  float4* __restrict__ out, int C4, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const int c = (int)(i % C4);
    const float4 v = x[i], sc = scale[c], sh = shift[c];
    out[i] = make_float4(relu_nan(fmaf(sc.x, v.x, sh.x)), relu_nan(fmaf(sc.y, v.y, sh.y)), relu_nan(fmaf(sc.z, v.z, sh.z)),
                         relu_nan(fmaf(sc.w, v.w, sh.w)));
}

__global__ void wrn_preact_bwd_kernel(const float4* __restrict__ g, const float4* __restrict__ o, const float4* __restrict__ scale,
                                      const float4* __restrict__ res, float4* __restrict__ gx, int C4, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const int c = (int)(i % C4);
    const float4 a = g[i], m = o[i], sc = scale[c];
    const float4 r = res ? res[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    gx[i] = make_float4(r.x + (m.x > 0.f ? sc.x * a.x : 0.f), r.y + (m.y > 0.f ? sc.y * a.y : 0.f), r.z + (m.z > 0.f ? sc.z * a.z : 0.f),
                        r.w + (m.w > 0.f ? sc.w * a.w : 0.f));
}

// one float4 of the 16 output channels of one pixel: i = (b, y, x, c4)
__global__ void wrn_stem_kernel(const float* __restrict__ spec, const float* __restrict__ w, float4* __restrict__ out, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const int c0 = (int)(i & 3) * 4;
    const long p = i >> 2, b = p >> 10;
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
    out[i] = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// one input pixel (b, y, x): nine taps of sixteen channels, four float4 loads per tap
__global__ void wrn_stem_bwd_kernel(const float4* __restrict__ g, const float* __restrict__ w, float* __restrict__ gspec, long total) {
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
            const long p = ((b << 10) + yy * 32 + xx) * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = g[p + q];
                const int t = ky * 3 + kx, c = q * 4;
                acc = fmaf(w[c * 9 + t], v.x, acc);
                acc = fmaf(w[(c + 1) * 9 + t], v.y, acc);
                acc = fmaf(w[(c + 2) * 9 + t], v.z, acc);
                acc = fmaf(w[(c + 3) * 9 + t], v.w, acc);
            }
        }
    gspec[i] = acc;
}
}  // namespace

void launch_wrn_preact(const float* x, const float* scale, const float* shift, float* out, long n_px, int C, hipStream_t s) {
    const long total4 = n_px * (C / 4);
    hipLaunchKernelGGL(wrn_preact_kernel, dim3(nblk(total4, 256)), dim3(256), 0, s, (const float4*)x, (const float4*)scale, (const float4*)shift,
                       (float4*)out, C / 4, total4);
}

void launch_wrn_preact_bwd(const float* g, const float* o, const float* scale, const float* res, float* gx, long n_px, int C, hipStream_t s) {
    const long total4 = n_px * (C / 4);
    hipLaunchKernelGGL(wrn_preact_bwd_kernel, dim3(nblk(total4, 256)), dim3(256), 0, s, (const float4*)g, (const float4*)o, (const float4*)scale,
                       (const float4*)res, (float4*)gx, C / 4, total4);
}

void launch_wrn_stem(const float* spec, const float* w, float* out, int B, hipStream_t s) {
    const long total4 = (long)B * 1024 * 4;
    hipLaunchKernelGGL(wrn_stem_kernel, dim3(nblk(total4, 256)), dim3(256), 0, s, spec, w, (float4*)out, total4);
}

void launch_wrn_stem_bwd(const float* g, const float* w, float* gspec, int B, hipStream_t s) {
    const long total = (long)B * 1024;
    hipLaunchKernelGGL(wrn_stem_bwd_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, (const float4*)g, w, gspec, total);
}

}  // namespace dmad
