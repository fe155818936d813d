// Small kernels of WideResNet-28-10 (wrn.hip): the pre-activation BatchNorm + ReLU that sits on the residual stream (it
// cannot be folded into a producing conv), its backward with the residual sum, and the 1 -> 16 stem conv (no BN, no ReLU) with its
// backward.  The convs in between are gemm_f32.hip launches (dmad_api.hip: classify_wrn / wrn_vjp_pass).  All fp32, no atomics, every
// reduction in a fixed order, every output element written exactly once; accesses along C in float4s.
#pragma once
#include "dmad_common.h"

namespace dmad {

// out[p][c] = max(scale[c] * x[p][c] + shift[c], 0) over n_px pixels of C channels (NHWC, C % 4 == 0); a NaN stays a NaN.  Indexed by
// element, so a C whose float4s do not divide a wave (160: 40 per pixel) is served like any other
void launch_wrn_preact(const float* x, const float* scale, const float* shift, float* out, long n_px, int C, hipStream_t s);
// gx[p][c] = (res ? res[p][c] : 0) + (o[p][c] > 0 ? scale[c] * g[p][c] : 0): the pre-activation's backward (o: the saved post-ReLU map;
// torch's threshold_backward: -0.0 and negatives give 0) plus the identity shortcut's gradient; res may be null (a stage's first block)
void launch_wrn_preact_bwd(const float* g, const float* o, const float* scale, const float* res, float* gx, long n_px, int C, hipStream_t s);
// stem: out[b][y][x][c] = sum over taps (ky, kx ascending) of w[c][ky][kx] * spec[b][y + ky - 1][x + kx - 1] (zero padding), c < 16;
// spec [B][32][32], out NHWC [B][32][32][16]
void launch_wrn_stem(const float* spec, const float* w, float* out, int B, hipStream_t s);
// stem backward: gspec[b][y][x] = sum over taps (ky, kx ascending) and c ascending of w[c][ky][kx] * g at (y + 1 - ky, x + 1 - kx)
void launch_wrn_stem_bwd(const float* g, const float* w, float* gspec, int B, hipStream_t s);

}  // namespace dmad
