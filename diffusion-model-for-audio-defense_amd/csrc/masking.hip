// Masking loss of the imperceptible attack and its gradient (masking.h): the hinge between the two DFT GEMMs, and the
// overlap-add of the uncentred framing with the loss sum and, optionally, the attack's update folded in.
#include "masking.h"
#include "gemm_f32.h"

namespace dmad {
namespace {

constexpr float kPsdGain = (8.f / 3.f) / (2048.f * 2048.f);       // gain_factor^2 / window_size^2 (reference l.670-672)

// One workgroup per frame row n = b * F + f of D; thread t walks the bins t, t + 256, ...  Writes gD's row (its K padding included),
// optionally psd[b][k][f], and the row's hinge sum: per thread ascending in k, then lanes and waves in a fixed tree.
__global__ __launch_bounds__(256) void masking_hinge_kernel(const float* __restrict__ D, int ldd, const float* __restrict__ theta,
                                                            const float* __restrict__ psd_scale, int F, float inv_kf,
                                                            float* __restrict__ gD, int ldg, float* __restrict__ psd,
                                                            float* __restrict__ part) {
    const int n = blockIdx.x, b = n / F, f = n - b * F;
    const float c = psd_scale[b] * kPsdGain, gc = 2.f * c * inv_kf;
    const float* d = D + (long)n * ldd;
    float* g = gD + (long)n * ldg;
    const long col = (long)b * kMaskBins * F + f;                  // (b, 0, f) of the [B][1025][F] maps
    float acc = 0.f;
    for (int k = threadIdx.x; k < ldg - kMaskBins; k += 256) {
        if (k < kMaskBins) {
            const float re = d[k], im = d[kMaskBins + k];
            const float p = (re * re + im * im) * c;
            const float t = theta[col + (long)k * F];
            const bool on = p > t;
            acc += on ? p - t : 0.f;
            g[k] = on ? re * gc : 0.f;
            g[kMaskBins + k] = on ? im * gc : 0.f;
            if (psd) psd[col + (long)k * F] = p;
        } else {
            g[kMaskBins + k] = 0.f;                                // columns 2050 .. ldg - 1: the K padding of the DFT^T GEMM
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    __shared__ float wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[n] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// One thread per (b, p): the frames that cover p, ascending.  STEP = 0 writes the gradient, STEP = 1 the reference's update; the
// thread of p = 0 sums its clip's F row sums, ascending, into the loss.
template <int STEP>
__global__ __launch_bounds__(256) void masking_ola_kernel(const float* __restrict__ gF, int F, int L, long total,
                                                          const float* __restrict__ part, float inv_kf, float* __restrict__ loss,
                                                          float* __restrict__ g_delta, const float* __restrict__ x, float* delta,
                                                          const float* __restrict__ g_net, const float* __restrict__ alpha,
                                                          float signed_lr) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long b = i / L;
    const int p = (int)(i - b * L);
    const int f0 = p >= kMaskWin ? (p - kMaskWin) / kMaskHop + 1 : 0;        // first frame with 512 f + 2048 > p
    int f1 = p / kMaskHop;
    if (f1 > F - 1) f1 = F - 1;
    float acc = 0.f;
    for (int f = f0; f <= f1; ++f) acc += gF[(b * F + f) * kMaskWin + (p - kMaskHop * f)];
    if (STEP) {
        const float xv = x[i];
        const float d = delta[i] + signed_lr * (g_net[i] + alpha[b] * acc);
        delta[i] = clamp_nan(xv + d, -1.f, 1.f) - xv;
    } else {
        g_delta[i] = acc;
    }
    if (p == 0) {
        float sum = 0.f;
        for (int f = 0; f < F; ++f) sum += part[b * F + f];
        loss[b] = sum * inv_kf;
    }
}

}  // namespace

int masking_pass(const MaskingWork& w, const float* delta, int B, int L, const float* theta, const float* psd_scale, float* loss, float* psd,
                 float* g_delta, const MaskingStep* step, hipStream_t s) {
    const int F = masking_frames(L);
    const long rows = (long)B * F;
    const float inv_kf = 1.f / (float)(kMaskBins * F);
    GemmF32Args g{};                                                   // D = dftA . frame, the frames read in place
    g.A = w.dftA; g.X = delta; g.C = w.D;
    g.M = 2 * kMaskBins; g.K = kMaskWin; g.taps = 1; g.ldc = w.ldd; g.N = rows; g.mode = 0;
    g.rows_per_batch = F; g.batch_stride = L; g.row_stride = kMaskHop; g.tap_stride = 0;
    if (launch_gemm_f32(g, s) != 0) return kGemmBadShape;
    hipLaunchKernelGGL(masking_hinge_kernel, dim3((unsigned)rows), dim3(256), 0, s, w.D, w.ldd, theta, psd_scale, F, inv_kf, w.gD, w.ldg, psd,
                       w.part);
    GemmF32Args t{};                                                   // gF = dftAT . gD
    t.A = w.dftAT; t.X = w.gD; t.C = w.gF;
    t.M = kMaskWin; t.K = w.ldg; t.taps = 1; t.ldc = kMaskWin; t.N = rows; t.mode = 0;
    t.rows_per_batch = rows; t.batch_stride = 0; t.row_stride = w.ldg; t.tap_stride = 0;
    if (launch_gemm_f32(t, s) != 0) return kGemmBadShape;
    const long total = (long)B * L;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (step)
        hipLaunchKernelGGL(masking_ola_kernel<1>, grid, dim3(256), 0, s, w.gF, F, L, total, w.part, inv_kf, loss, (float*)nullptr, step->x,
                           step->delta, step->g_net, step->alpha, step->signed_lr);
    else
        hipLaunchKernelGGL(masking_ola_kernel<0>, grid, dim3(256), 0, s, w.gF, F, L, total, w.part, inv_kf, loss, g_delta, (const float*)nullptr,
                           (float*)nullptr, (const float*)nullptr, (const float*)nullptr, 0.f);
    return 0;
}

}  // namespace dmad
