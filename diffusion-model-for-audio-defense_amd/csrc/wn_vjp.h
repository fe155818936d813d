// Small kernels of the WaveNet's vector-Jacobian product (wn_vjp.hip); its GEMMs are gemm_f32.hip's epilogues 3 / 4.
#pragma once
#include "dmad_common.h"

namespace dmad {

// g_y[n][c] = (y[n][c] > 0) * wz[c] * g_eps[n]: y = the final block's post-ReLU f0 output [N][256]
void launch_vjp_final(const float* y, const float* wz, const float* g_eps, float* g_y, long N, hipStream_t s);
// g_x[p] = sum_c w[c] * [w[c] x[p] + b[c] > 0] * g_h0[row(p)][c]   (g_h0: zero-padded [B][LP][256] map), c in index order;
// with g_in: g_x[p] = alpha * g_in[p] - gamma * (that sum)  (the adjoint update of a reverse VP-SDE step; g_in != g_x)
void launch_vjp_init(const float* x, const float* w, const float* bias, const float* g_h0, float* g_x, int B, int L, int LP, hipStream_t s,
                     const float* g_in = nullptr, float alpha = 1.f, float gamma = 0.f);
// transposed weight images, packed on the device from the forward images (gemm_f32.h):
//   wdilT[n][tap][ci][oc] = W_dil,n[oc][ci][2 - tap]       from the permuted epi-1 image wdil[n][tap][R][ci]
//   wgT[n][0][c][k]       = W_skip,n[k][c],  wgT[n][1][c][k] = sqrt(1/2) W_res,n[k][c]     from wrs[n][res | skip][k][c]
//   wf0T[c][k]            = sqrt(1/NL) W_f0[k][c]
void launch_vjp_pack(const float* wdil, const float* wrs, const float* wf0, float* wdilT, float* wgT, float* wf0T, int NL, hipStream_t s);

}  // namespace dmad
