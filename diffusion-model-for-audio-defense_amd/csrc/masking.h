// Masking loss of the imperceptible attack (Qin et al. 2019; reference robustness_eval/white_box_attack.py:606-678) and its gradient
// with respect to the perturbation (masking.hip).  One pass over B clips:
//   frames   row b * F + f = delta[b][512 f .. 512 f + 2048), F = (L - 2048) / 512 + 1: the uncentred framing of torch.stft(center=False),
//            read straight from delta by the fp32 GEMM's row form (no pad kernel)
//   D        = dftA . frame ([rows][ldd]: re at k, im at 1025 + k; dftA holds the Hann window)
//   hinge    psd = psd_scale[b] (8/3) / 2048^2 (re^2 + im^2); loss[b] = mean_{k,f} max(psd - theta, 0);
//            gD = 2 (re, im) psd_scale[b] (8/3) / 2048^2 / (1025 F) where psd > theta (strict: torch's ReLU'(0) = 0), else 0
//   gF       = dftAT . gD ([rows][2048])
//   last     g_delta[b][p] = sum over the frames f ascending that cover p of gF[b F + f][p - 512 f] (0 for p >= 512 (F - 1) + 2048),
//            or, with a MaskingStep, the reference's update (l.569-573) in its place; the same kernel sums the loss.
// Every sum runs in a fixed order (no atomics, no split-K): the results are bit-reproducible and a clip's bits do not depend on the
// batch or on its row.  Nothing is kept across calls.
#pragma once
#include "dmad_common.h"

namespace dmad {

constexpr int kMaskWin = 2048, kMaskHop = 512, kMaskBins = 1025;
constexpr int kMaskMaxFrames = 32;       // the frames per clip the mel front-end's DFT map holds

// frames of an L-sample clip, 0 when L < 2048
inline int masking_frames(long L) { return L < kMaskWin ? 0 : (int)((L - kMaskWin) / kMaskHop + 1); }

// The engine's buffers the pass works in (all shared with the mel front-end and its VJP)
struct MaskingWork {
    const float* dftA;      // [2050][2048] windowed DFT image
    const float* dftAT;     // [2048][ldg] its transpose, rows 2050 .. ldg - 1 zero
    float* D;               // [rows][ldd] DFT map
    float* gD;              // [rows][ldg] its gradient
    float* gF;              // [rows][2048] frame gradients
    float* part;            // [rows] per-frame hinge sums
    int ldd, ldg;
};

// the reference's update in place of the gradient: delta = clamp(x + delta + signed_lr (g_net + alpha[b] g_theta), -1, 1) - x
struct MaskingStep {
    const float* x;         // [B][L]
    float* delta;           // [B][L], updated in place (the tensor the frames were read from)
    const float* g_net;     // [B][L]
    const float* alpha;     // [B]
    float signed_lr;
};

// theta [B][1025][F], psd_scale [B], loss [B]; psd (optional) [B][1025][F]; exactly one of g_delta [B][L] and step is given.
// Returns 0, or kGemmBadShape when a GEMM refuses its shape (nothing further is launched).
int masking_pass(const MaskingWork& w, const float* delta, int B, int L, const float* theta, const float* psd_scale, float* loss, float* psd,
                 float* g_delta, const MaskingStep* step, hipStream_t s);

}  // namespace dmad
