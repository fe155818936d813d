// Small kernels of the WaveNet's vector-Jacobian product (dmad_wavenet_eps_vjp): the final block's ReLU mask, the init conv's
// backward and the device-side packing of the transposed weight images.  Every reduction is in a fixed order (no atomics).
#include "wn_vjp.h"

namespace dmad {

namespace {
inline unsigned nblk(long n, int per) { return (unsigned)((n + per - 1) / per); }
}

__global__ void vjp_final_kernel(const float* __restrict__ y, const float* __restrict__ wz, const float* __restrict__ g_eps,
                                 float* __restrict__ g_y, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;          // one float4 (4 channels) each
    if (i >= total4) return;
    const long n = i >> 6;
    const int c = (int)(i & 63) * 4;
    const float4 v = ((const float4*)y)[i], w = *(const float4*)(wz + c);
    const float g = g_eps[n];
    ((float4*)g_y)[i] = float4{v.x > 0.f ? w.x * g : 0.f, v.y > 0.f ? w.y * g : 0.f, v.z > 0.f ? w.z * g : 0.f, v.w > 0.f ? w.w * g : 0.f};
}

// one wave per position (the layout of dot256_kernel): lane l holds channels 4l .. 4l+3, then a fixed butterfly.
// AFFINE (the reverse VP-SDE chain, dmad_vpsde_purify_vjp): g_x[p] = alpha * g_in[p] - gamma * sum instead of the sum, so the adjoint
// update of an Euler step costs no pass of its own.  g_in and g_x are two different buffers (the caller ping-pongs them).
template <bool AFFINE>
__global__ void __launch_bounds__(256) vjp_init_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       const float* __restrict__ g_h0, float* __restrict__ g_x, int L, int LP, long N,
                                                       const float* __restrict__ g_in, float alpha, float gamma) {
    const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= N) return;
    const long bb = p / L, t = p - bb * L;
    const float xv = x[p];
    const float4 g = *(const float4*)(g_h0 + (bb * LP + kPad + t) * kC + lane * 4);
    const float4 ww = *(const float4*)(w + lane * 4), b4 = *(const float4*)(bias + lane * 4);
    const float ga[4] = {g.x, g.y, g.z, g.w}, wa[4] = {ww.x, ww.y, ww.z, ww.w}, ba[4] = {b4.x, b4.y, b4.z, b4.w};
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)        // the forward's pre-activation, rounded as wn_init_f32_kernel rounds it: the same ReLU mask
        if (__fadd_rn(__fmul_rn(wa[j], xv), ba[j]) > 0.f) s = __fadd_rn(s, __fmul_rn(wa[j], ga[j]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
        if constexpr (AFFINE) g_x[p] = __fsub_rn(__fmul_rn(alpha, g_in[p]), __fmul_rn(gamma, s));
        else g_x[p] = s;
    }
}

// one thread per element of the forward image wdil[n][tap][R][ci]; R -> output channel as packed by finalize_wavenet (epi 1)
__global__ void vjp_pack_dil_kernel(const float* __restrict__ wdil, float* __restrict__ wdilT, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ci = (int)(i & 255), R = (int)((i >> 8) & 511);
    const long nt = i >> 17;                      // n * 3 + tap
    const int tap = (int)(nt % 3);
    const long n = nt / 3;
    const int bm = R / 128, wmr = (R % 128) / 64, ii = (R % 64) / 16, rr = R % 16;
    const int oc = (ii >= 2 ? 256 : 0) + bm * 64 + wmr * 32 + (ii & 1) * 16 + rr;
    wdilT[((n * 3 + (2 - tap)) * 256 + ci) * 512 + oc] = wdil[i];
}

// wgT[n][tap][c][k] from wrs[n][512][256] (rows 0-255: W_res[k][c], rows 256-511: W_skip[k][c])
__global__ void vjp_pack_gate_kernel(const float* __restrict__ wrs, float* __restrict__ wgT, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;          // index into wgT
    if (i >= total) return;
    const int k = (int)(i & 255), c = (int)((i >> 8) & 255), tap = (int)((i >> 16) & 1);
    const long n = i >> 17;
    const float v = wrs[(n * 512 + (tap ? 0 : 256) + k) * 256 + c];
    wgT[i] = tap ? __fmul_rn(v, 0.70710678118654752440f) : v;
}

__global__ void vjp_pack_f0_kernel(const float* __restrict__ wf0, float* __restrict__ wf0T, float scale) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;                // index into wf0T [c][k]
    if (i >= 65536) return;
    const int k = i & 255, c = i >> 8;
    wf0T[i] = __fmul_rn(wf0[k * 256 + c], scale);
}

void launch_vjp_final(const float* y, const float* wz, const float* g_eps, float* g_y, long N, hipStream_t s) {
    const long total4 = N * 64;
    hipLaunchKernelGGL(vjp_final_kernel, dim3(nblk(total4, 256)), dim3(256), 0, s, y, wz, g_eps, g_y, total4);
}
void launch_vjp_init(const float* x, const float* w, const float* bias, const float* g_h0, float* g_x, int B, int L, int LP, hipStream_t s,
                     const float* g_in, float alpha, float gamma) {
    const long N = (long)B * L;
    if (g_in) hipLaunchKernelGGL(vjp_init_kernel<true>, dim3(nblk(N, 4)), dim3(256), 0, s, x, w, bias, g_h0, g_x, L, LP, N, g_in, alpha, gamma);
    else hipLaunchKernelGGL(vjp_init_kernel<false>, dim3(nblk(N, 4)), dim3(256), 0, s, x, w, bias, g_h0, g_x, L, LP, N, nullptr, 0.f, 0.f);
}
void launch_vjp_pack(const float* wdil, const float* wrs, const float* wf0, float* wdilT, float* wgT, float* wf0T, int NL, hipStream_t s) {
    const long td = (long)NL * 3 * 512 * 256, tg = (long)NL * 2 * 256 * 256;
    hipLaunchKernelGGL(vjp_pack_dil_kernel, dim3(nblk(td, 256)), dim3(256), 0, s, wdil, wdilT, td);
    hipLaunchKernelGGL(vjp_pack_gate_kernel, dim3(nblk(tg, 256)), dim3(256), 0, s, wrs, wgT, tg);
    hipLaunchKernelGGL(vjp_pack_f0_kernel, dim3(256), dim3(256), 0, s, wf0, wf0T, (float)sqrt(1.0 / NL));
}

}  // namespace dmad
