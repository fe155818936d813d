// Kernels of DenseNet-BC-100-12 (densenet.hip).  A dense block's concatenation is ONE NHWC stream per resolution, written in
// place at the stream's pitch; every BatchNorm + ReLU of the net sits on the load side of a conv and is applied while the consumer stages
// its pixel tile.  All fp32: the matrix work runs on v_mfma_f32_16x16x4_f32 (bitwise an fmaf chain in k order), no atomics, every
// reduction in one stated order, every output element written once per launch.  No kernel reads a stream channel >= the width it is
// given: the k columns that pad a width to the MFMA's 4 are exact zeros made in the staging, never loaded.
#pragma once
#include "dmad_common.h"

namespace dmad {

// THE pre-activation: max(fmaf(scale, x, shift), 0) with a NaN kept and -0.0 made +0.0.  The forward's staging, the backward's mask, the
// head and the tape reader all call it, so a ReLU decision is the same bit wherever it is recomputed.
__device__ __forceinline__ float dn_preact(float scale, float x, float shift) {
    const float t = fmaf(scale, x, shift);
    return t > 0.f ? t : (t != t ? t : 0.f);
}

// The 1x1 product  acc[p][m] = sum over k ascending of A[m][k] * b[p][k],  m < M, p < n_px (any n_px), k < K (even); A: [M][K4] with
// K4 = K rounded up to 4 and zero columns behind K.
//   forward  (bwd = 0): b[p][k] = dn_preact(s_in[k], in[p * ldi + k], b_in[k]);  out[p * ldo + m] = s_out ? dn_preact(s_out[m], acc,
//            b_out[m]) : acc.  The bottleneck's conv (M = 48, bn2 + ReLU as the epilogue) and a transition's (M = 108 / 150, no epilogue).
//   backward (bwd = 1): b[p][k] = in[q * ldi + k] (pool = 0: q = p) or 0.25 * in[q * ldi + k] with q the 2x2 window of pixel p in a map of
//            half the resolution H (pool = 1: the average pool's backward);  v = dn_preact(s1[m], x[p * ldx + m], b1[m]) > 0 ? s1[m] * acc
//            : 0 and out[p * ldo + m] = add ? out[p * ldo + m] + v : v — read and written by one thread; channels >= M are not touched.
struct DnPwArgs {
    const float* A; int M, K, K4;
    const float* in; int ldi; long n_px;
    const float *s_in, *b_in, *s_out, *b_out;
    float* out; int ldo;
    int pool, H, add;
    const float *x; int ldx; const float *s1, *b1;
};
void launch_dn_pw(const DnPwArgs& a, bool bwd, hipStream_t s);

// The 3x3 conv, zero padding, taps in (ky, kx) order and then channels, one accumulation chain per output element, on [B][H][H] maps
// with H in {8, 16, 32}:
//   growth forward:  stream[p * lds + off + j] = sum W[j][tap][c] * h[p + tap][c], j < 12, c < 48;  A: [16][432] (rows 12..15 zero)
//   growth backward: gh[p * 48 + c] = h[p * 48 + c] > 0 ? s2[c] * sum WT[c][tap][j] * g[(p + tap) * lds + off + j] : 0;  A: [48][108], the
//                    tap-flipped transpose WT[c][tap][j] = W[j][8 - tap][c]
void launch_dn_growth(const float* A, const float* h, float* stream, int lds, int off, int B, int H, hipStream_t s);
void launch_dn_growth_bwd(const float* A, const float* g, int lds, int off, const float* h, const float* s2, float* gh, int B, int H, hipStream_t s);

// stem: stream[p * ld + c] = sum over taps (ky, kx ascending) of w[c][tap] * spec[p + tap], c < 24 (no BN, no ReLU); its backward:
// gspec[p] = sum over taps (ky, kx ascending) and c ascending of w[c][tap] * g[(p - tap) * ld + c]
void launch_dn_stem(const float* spec, const float* w, float* stream, int ld, int B, hipStream_t s);
void launch_dn_stem_bwd(const float* g, int ld, const float* w, float* gspec, int B, hipStream_t s);
// 2x2 average pool of t [B][H][H][ldt], channels < C: out[q * ldo + c] = 0.25 * (((tl + tr) + bl) + br)
void launch_dn_pool(const float* t, int ldt, float* out, int ldo, int B, int H, int C, hipStream_t s);
// out[p * C + c] = dn_preact(scale[c], x[p * ldx + c], shift[c]), c < C: a post-ReLU map as the forward decided it (tape reader, test hook)
void launch_dn_preact_map(const float* x, int ldx, const float* scale, const float* shift, float* out, long n_px, int C, hipStream_t s);
// head: logits[b][k] = fcb[k] + sum over c ascending of fcw[k][c] * pooled[c], pooled[c] = (sum over p ascending of dn_preact(bns[c],
// x[(b * HW + p) * ldx + c], bnb[c])) / HW; HW a power of two
void launch_dn_head(const float* x, int ldx, const float* bns, const float* bnb, const float* fcw, const float* fcb, float* logits, int B, int HW,
                    int C, int ncls, hipStream_t s);
// head backward: g[(b * HW + p) * ldg + c] = dn_preact(bns[c], x[..], bnb[c]) > 0 ? (sum over k ascending of fcws[k][c] * g_logits[b][k]) / HW
// : 0, c < C; fcws: fc.w with the final bn's scale folded into its columns
void launch_dn_head_bwd(const float* g_logits, const float* fcws, const float* x, int ldx, const float* bns, const float* bnb, float* g, int ldg,
                        int B, int HW, int C, int ncls, hipStream_t s);

}  // namespace dmad
