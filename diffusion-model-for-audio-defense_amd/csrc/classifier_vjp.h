// Small kernels of the classifier-side vector-Jacobian products (classifier_vjp.hip): the ResNeXt29 input VJP
// (dmad_classify_vjp), the VGG19_bn input VJP (dmad_vgg_vjp) and the mel front-end VJP (dmad_mel_db_vjp).  Their convs, 1x1 and Linear
// layers / DFT and filterbank products are
// gemm_f32.hip launches on transposed weight images packed here.  Every reduction runs in a fixed order (no atomics): results do not
// depend on the batch.
#pragma once
#include "dmad_common.h"

namespace dmad {

// dst[i][j] = src[j * lds + i] * (scale ? scale[j] : 1) for j < rows, 0 for rows <= j < ldd; i < cols.  The transposed image of a
// [rows][cols] matrix (a 1x1 conv [M][K] with its eval-BatchNorm scale folded into the columns, the DFT / filterbank images)
void launch_cvjp_transpose(const float* src, int rows, int cols, long lds, const float* scale, float* dst, int ldd, hipStream_t s);
// the grouped 3x3 conv's backward image: src [g][tap][m][k] (G x G per group, 8 groups) -> dst[g][8 - tap][k][m] * scale[g * G + m]
void launch_cvjp_pack_grouped(const float* src, const float* scale, float* dst, int G, hipStream_t s);
// the dense 3x3 conv's backward image (VGG19_bn, WideResNet): src [tap][M][K] -> dst[8 - tap][k][m] * scale[m] (scale null: the plain image)
void launch_cvjp_pack_dense(const float* src, const float* scale, float* dst, int M, int K, hipStream_t s);
// 2x2 max-pool and the ReLU in front of it, backward: y [B][H][H][C] the saved post-ReLU map (the pool's input), g [B][H/2][H/2][C] ->
// gpre [B][H][H][C], the gradient at the ReLU's input.  Each window's g goes to its maximum, the first in scan order (top-left, top-right,
// bottom-left, bottom-right) on a tie, and only where that maximum is > 0; every element of gpre is written once.  H even, C % 4 == 0
void launch_vgg_pool_relu_bwd(const float* g, const float* y, float* gpre, int B, int H, int C, hipStream_t s);
// ReLU backward on the saved post-ReLU map: out[i] = y[i] > 0 ? g[i] : 0 (torch's threshold_backward); out may alias g; n % 4 == 0
void launch_relu_mask(const float* g, const float* y, float* out, long n, hipStream_t s);
// head backward: gz[b][p][c] = y[b][p][c] > 0 ? (sum_k W[k][c] g[b][k]) / HW : 0 — the FC (W [ncls][C]), the HW-pixel average pool and
// the last block's ReLU; k ascending
void launch_rx_head_bwd(const float* g_logits, const float* W, const float* y, float* gz, int B, int ncls, int HW, int C, hipStream_t s);
// conv1 (1 -> 64, 3x3, BN scale) backward with its ReLU: gspec[b][y][x] = sum over taps (ky, kx ascending) and channels c (ascending)
// of w[c][ky][kx] * scale[c] * [a > 0] * g at (y + 1 - ky, x + 1 - kx); g, a: NHWC [B][32][32][64]
void launch_rx_conv1_bwd(const float* g, const float* a, const float* w, const float* scale, float* gspec, int B, hipStream_t s);
// dB backward: gM[b * 32 + fr][mel] = M >= 1e-10 ? gspec[b][mel][fr] * 10 / (ln 10 * M) : 0, M = melM[b * 32 + fr][mel]
void launch_mel_db_bwd(const float* gspec, const float* M, float* gM, int B, hipStream_t s);
// power backward: gD[n][f] = 2 re gP[n][f], gD[n][1025 + f] = 2 im gP[n][f] (D [n][ldd]: re at f, im at 1025 + f), zero up to ldg (>= 2050)
void launch_mel_power_bwd(const float* D, int ldd, const float* gP, int ldp, float* gD, int ldg, long rows, hipStream_t s);
// overlap-add backward of the framing (hop 512, 2048-sample frames, 32 frames, center padding 1024 cropped):
// gx[b][p] = sum over frames fr (ascending) covering p of gF[b * 32 + fr][p + 1024 - 512 fr]
void launch_mel_ola_bwd(const float* gF, float* gx, int B, int L, hipStream_t s);

}  // namespace dmad
