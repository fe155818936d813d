// See classifier_vjp.h.
#include "classifier_vjp.h"

namespace dmad {

namespace {
inline unsigned nblk(long n, int b) { return (unsigned)((n + b - 1) / b); }

__global__ void cvjp_transpose_kernel(const float* __restrict__ src, int rows, long lds, const float* __restrict__ scale,
                                      float* __restrict__ dst, int ldd, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i % ldd);
    const long c = i / ldd;
    float v = 0.f;
    if (j < rows) {
        v = src[(long)j * lds + c];
        if (scale) v *= scale[j];
    }
    dst[i] = v;
}

__global__ void cvjp_pack_grouped_kernel(const float* __restrict__ src, const float* __restrict__ scale, float* __restrict__ dst, int G,
                                         long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // one element of dst [g][tap][k][m]
    if (i >= total) return;
    const int m = (int)(i % G);
    long r = i / G;
    const int k = (int)(r % G);
    r /= G;
    const int t = (int)(r % 9), g = (int)(r / 9);
    dst[i] = src[(((long)g * 9 + (8 - t)) * G + m) * G + k] * scale[g * G + m];
}

__global__ void cvjp_pack_dense_kernel(const float* __restrict__ src, const float* __restrict__ scale, float* __restrict__ dst, int M, int K,
                                       long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // one element of dst [tap][k][m]
    if (i >= total) return;
    const int m = (int)(i % M);
    const long r = i / M;
    const int k = (int)(r % K), t = (int)(r / K);
    const float v = src[((long)(8 - t) * M + m) * K + k];
    dst[i] = scale ? v * scale[m] : v;
}

// one float4 of channels of one pooled pixel: the window's first maximum in scan order takes g if it is > 0 (torch's max_pool2d keeps
// the earlier entry on a tie and lets a NaN win; threshold_backward passes where y > 0)
__global__ void vgg_pool_relu_bwd_kernel(const float4* __restrict__ g, const float4* __restrict__ y, float4* __restrict__ gpre, int H, int C4,
                                         long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const int Hp = H >> 1;
    const int c = (int)(i % C4);
    long r = i / C4;
    const int px = (int)(r % Hp);
    r /= Hp;
    const int py = (int)(r % Hp);
    const long b = r / Hp;
    const long p00 = ((b * H + 2 * py) * H + 2 * px) * C4 + c, p10 = p00 + (long)H * C4;
    const float4 gv = g[i];
    const float4 v[4] = {y[p00], y[p00 + C4], y[p10], y[p10 + C4]};
    float4 o[4];
    const float ga[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float w[4] = {(&v[0].x)[j], (&v[1].x)[j], (&v[2].x)[j], (&v[3].x)[j]};
        float m = w[0];
        int a = 0;
#pragma unroll
        for (int q = 1; q < 4; ++q)
            if (w[q] > m || w[q] != w[q]) { m = w[q]; a = q; }
        const float t = m > 0.f ? ga[j] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) (&o[q].x)[j] = a == q ? t : 0.f;
    }
    gpre[p00] = o[0];
    gpre[p00 + C4] = o[1];
    gpre[p10] = o[2];
    gpre[p10 + C4] = o[3];
}

__global__ void relu_mask_kernel(const float4* __restrict__ g, const float4* __restrict__ y, float4* out, long n4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 a = g[i], m = y[i];
    out[i] = make_float4(m.x > 0.f ? a.x : 0.f, m.y > 0.f ? a.y : 0.f, m.z > 0.f ? a.z : 0.f, m.w > 0.f ? a.w : 0.f);
}

__global__ void rx_head_bwd_kernel(const float* __restrict__ gl, const float* __restrict__ W, const float* __restrict__ y,
                                   float* __restrict__ gz, int ncls, int HW, int C, float inv_hw, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // one (b, p, c)
    if (i >= total) return;
    const int c = (int)(i % C);
    const long b = i / ((long)HW * C);
    float acc = 0.f;
    for (int k = 0; k < ncls; ++k) acc = fmaf(W[(long)k * C + c], gl[b * ncls + k], acc);
    gz[i] = y[i] > 0.f ? acc * inv_hw : 0.f;
}

__global__ void rx_conv1_bwd_kernel(const float* __restrict__ g, const float* __restrict__ a, const float* __restrict__ w,
                                    const float* __restrict__ scale, float* __restrict__ gspec, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // one input pixel (b, y, x)
    if (i >= total) return;
    const long b = i >> 10;
    const int y = (int)((i >> 5) & 31), x = (int)(i & 31);
    float acc = 0.f;
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y + 1 - ky, xx = x + 1 - kx;
            if ((unsigned)yy >= 32u || (unsigned)xx >= 32u) continue;
            const long p = ((b << 10) + yy * 32 + xx) * 64;
            for (int c = 0; c < 64; ++c) {
                const float v = a[p + c] > 0.f ? g[p + c] : 0.f;
                acc = fmaf(w[c * 9 + ky * 3 + kx] * scale[c], v, acc);
            }
        }
    gspec[i] = acc;
}

__global__ void mel_db_bwd_kernel(const float* __restrict__ gspec, const float* __restrict__ M, float* __restrict__ gM, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // one (b, mel, frame) of gspec
    if (i >= total) return;
    const long b = i >> 10;
    const int mel = (int)((i >> 5) & 31), fr = (int)(i & 31);
    const long o = (b * 32 + fr) * 32 + mel;
    const float m = M[o];
    // d/dM 10 log10(M) = 10 / (ln 10 M); clamp(min = 1e-10) passes the gradient where M >= min (torch's rule)
    gM[o] = m >= 1e-10f ? gspec[i] * (4.3429448190325182f / m) : 0.f;
}

__global__ void mel_power_bwd_kernel(const float* __restrict__ D, int ldd, const float* __restrict__ gP, int ldp, float* __restrict__ gD,
                                     int ldg, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // one (n, j), j < ldg - 1025
    if (i >= total) return;
    const int w = ldg - 1025;
    const long n = i / w;
    const int f = (int)(i - n * w);
    if (f < 1025) {
        const float gp = gP[n * ldp + f];
        gD[n * ldg + f] = 2.f * D[n * ldd + f] * gp;
        gD[n * ldg + 1025 + f] = 2.f * D[n * ldd + 1025 + f] * gp;
    } else {
        gD[n * ldg + 1025 + f] = 0.f;                                // K padding of the DFT^T GEMM (columns 2050 .. ldg - 1)
    }
}

__global__ void mel_ola_bwd_kernel(const float* __restrict__ gF, float* __restrict__ gx, int L, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // one (b, p)
    if (i >= total) return;
    const long b = i / L;
    const int q = (int)(i - b * L) + 1024;                           // position in the center-padded signal
    int f0 = q >= 2048 ? (q - 2048) / 512 + 1 : 0;                   // first frame with 512 f + 2048 > q
    int f1 = q / 512;
    if (f1 > 31) f1 = 31;
    float acc = 0.f;
    for (int fr = f0; fr <= f1; ++fr) acc += gF[(b * 32 + fr) * 2048 + (q - 512 * fr)];
    gx[i] = acc;
}
}  // namespace

void launch_cvjp_transpose(const float* src, int rows, int cols, long lds, const float* scale, float* dst, int ldd, hipStream_t s) {
    const long total = (long)cols * ldd;
    hipLaunchKernelGGL(cvjp_transpose_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, src, rows, lds, scale, dst, ldd, total);
}

void launch_cvjp_pack_grouped(const float* src, const float* scale, float* dst, int G, hipStream_t s) {
    const long total = 8l * 9 * G * G;
    hipLaunchKernelGGL(cvjp_pack_grouped_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, src, scale, dst, G, total);
}

void launch_cvjp_pack_dense(const float* src, const float* scale, float* dst, int M, int K, hipStream_t s) {
    const long total = 9l * M * K;
    hipLaunchKernelGGL(cvjp_pack_dense_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, src, scale, dst, M, K, total);
}

void launch_vgg_pool_relu_bwd(const float* g, const float* y, float* gpre, int B, int H, int C, hipStream_t s) {
    const long total4 = (long)B * (H / 2) * (H / 2) * (C / 4);
    hipLaunchKernelGGL(vgg_pool_relu_bwd_kernel, dim3(nblk(total4, 256)), dim3(256), 0, s, (const float4*)g, (const float4*)y, (float4*)gpre, H,
                       C / 4, total4);
}

void launch_relu_mask(const float* g, const float* y, float* out, long n, hipStream_t s) {
    const long n4 = n / 4;
    hipLaunchKernelGGL(relu_mask_kernel, dim3(nblk(n4, 256)), dim3(256), 0, s, (const float4*)g, (const float4*)y, (float4*)out, n4);
}

void launch_rx_head_bwd(const float* g_logits, const float* W, const float* y, float* gz, int B, int ncls, int HW, int C, hipStream_t s) {
    const long total = (long)B * HW * C;
    hipLaunchKernelGGL(rx_head_bwd_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, g_logits, W, y, gz, ncls, HW, C, 1.f / (float)HW, total);
}

void launch_rx_conv1_bwd(const float* g, const float* a, const float* w, const float* scale, float* gspec, int B, hipStream_t s) {
    const long total = (long)B * 1024;
    hipLaunchKernelGGL(rx_conv1_bwd_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, g, a, w, scale, gspec, total);
}

void launch_mel_db_bwd(const float* gspec, const float* M, float* gM, int B, hipStream_t s) {
    const long total = (long)B * 1024;
    hipLaunchKernelGGL(mel_db_bwd_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, gspec, M, gM, total);
}

void launch_mel_power_bwd(const float* D, int ldd, const float* gP, int ldp, float* gD, int ldg, long rows, hipStream_t s) {
    const long total = rows * (ldg - 1025);
    hipLaunchKernelGGL(mel_power_bwd_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, D, ldd, gP, ldp, gD, ldg, total);
}

void launch_mel_ola_bwd(const float* gF, float* gx, int B, int L, hipStream_t s) {
    const long total = (long)B * L;
    hipLaunchKernelGGL(mel_ola_bwd_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, gF, gx, L, total);
}

}  // namespace dmad
