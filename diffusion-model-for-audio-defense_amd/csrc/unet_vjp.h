// Small kernels of the UNet's vector-Jacobian product (unet_vjp.hip); its convs and 1x1 layers are gemm_f32.hip's
// NHWC mode on transposed weight images.  Every reduction runs in a fixed order (no atomics): results do not depend on the batch.
#pragma once
#include "dmad_common.h"

namespace dmad {

// dst[(i0 * n1 + i1) * n2 + i2] = src[s0 * f0(i0) + s1 * f1(i1) + s2 * f2(i2)], fk(i) = (flip >> k & 1) ? nk - 1 - i : i — the transposed
// (and tap-flipped) weight images of the backward walk, packed on the device from the resident forward images
void launch_unvjp_pack(const float* src, float* dst, int n0, int n1, int n2, long s0, long s1, long s2, int flip, hipStream_t s);
// Backward of  y = SiLU?(((x - mean) * rstd * gamma + beta) [* (1 + ss[c]) + ss[C + c]])  (GroupNorm32, launch_groupnorm_nhwc) over
// [B][HW][C]: the statistics are recomputed from x (two-pass, like the forward);  g_x = rstd * (gh - mean(gh) - xh * mean(gh * xh)),
// gh = gamma * (1 + ss[c]) * SiLU'(pre) * gy, plus add / add2 ([B][HW][C], optional).  x2 != nullptr: the input is the concatenation
// [x : c1 channels | x2 : C - c1]; its gradient is written in the same two parts (gx pitch c1, gx2 pitch C - c1; gx2 may be null
// only without x2).  Returns -1 for a map it does not serve (C not a multiple of 32).
int launch_groupnorm_bwd(const float* x, const float* x2, int c1, const float* gamma, const float* beta, const float* ss, int silu,
                         const float* gy, const float* add, const float* add2, float* gx, float* gx2, int B, int HW, int C, hipStream_t s);
// Backward of QKVAttention (launch_qkv_attention's head-major split, head width 64): qkv [B*T][3C] the saved forward input, go [B*T][C]
// the gradient of its output; writes gqkv [B*T][3C] (dq, dk, dv in the positions of q, k, v).  P is recomputed from qkv.  T = 256, 64
// or 16; returns -1 for any other T, a hipError_t > 0 if the kernel could not be configured.
int launch_qkv_attention_bwd(const float* qkv, const float* go, float* gqkv, int B, int T, int heads, hipStream_t s);
// the zero-dilated map of a stride-2 gradient: d [B][2Ho][2Ho][C], d[2y][2x] = g[y][x], zero elsewhere (C % 4 == 0)
void launch_dilate2x_nhwc(const float* g, float* d, int B, int Ho, int C, hipStream_t s);
// backward of nearest x2 upsampling: gin [B][H][H][C] = sum of the 2x2 block of g [B][2H][2H][C] (+ add, optional), C % 4 == 0
void launch_upsample2x_bwd_nhwc(const float* g, const float* add, float* gin, int B, int H, int C, hipStream_t s);

}  // namespace dmad
