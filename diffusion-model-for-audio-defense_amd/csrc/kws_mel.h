// Mel front-end of the keyword spotter (reference kws_adaptive_attack_eval.py: torchaudio MelSpectrogram(sample_rate=16000, n_mels=32)
// then AmplitudeToDB('power')) for clips of any length, exact fp32 (kws_mel.hip): n_fft = win_length = 400, hop 200,
// periodic Hann, center=True with reflect padding of 200 samples, one-sided power spectrum of 201 bins, htk mel scale without norm
// between 0 and 8000 Hz, 10 log10(max(., 1e-10)).  A clip of L samples has T = 1 + L / 200 frames.  The forward and the VJP are one
// launch each; the VJP recomputes the forward by the same code, uses no atomics and writes every element of g_x.  Every sum runs in a
// fixed order: a frame's bits depend on its own 400 samples only, g_x's on the clip and g_spec only.
#pragma once
#include <vector>

#include "dmad_common.h"

namespace dmad {

constexpr int kMelWin = 400;          // n_fft = win_length
constexpr int kMelHop = 200;          // hop = reflect padding
constexpr int kMelBins = 201;         // one-sided bins
constexpr int kMelCols = 2 * kMelBins;   // rows of the DFT matrix: 201 cos, then 201 -sin, the window folded in
constexpr int kMelLdc = 416;          // leading dimension of the forward image [400 n][416 >= 402 c]
constexpr int kMelFilters = 32;
constexpr int kMelTile = 8;           // frames of one forward workgroup (all frames); the VJP's workgroup owns kMelTile - 1 blocks of 200
constexpr int kMelMinL = kMelHop + 1; // the reflect padding needs one sample more than it mirrors

// Device constants, float64 on the host and rounded once (kws_mel_host_constants)
struct KwsMelConst {
    const float* af = nullptr;        // forward image [400 n][kMelLdc c]: lanes run over c
    const float* ab = nullptr;        // backward image [402 c][400 n]: lanes run over n
    const float* fb = nullptr;        // filterbank [32 m][201 k]
    const float* w0 = nullptr;        // [201] weight of bin k in its lowest filter m0[k] ...
    const float* w1 = nullptr;        // [201] ... and in filter m0[k] + 1 (0 where there is none)
    const int32_t* m0 = nullptr;      // [201]
    const int32_t* lo = nullptr;      // [32] first and ...
    const int32_t* hi = nullptr;      // [32] ... last bin of filter m
};

// Host images of the above.  Returns nullptr, or what is wrong with the filterbank (an empty filter, a bin in more than two filters)
struct KwsMelHost {
    std::vector<float> af, ab, fb, w0, w1;
    std::vector<int32_t> m0, lo, hi;
};
const char* kws_mel_host_constants(KwsMelHost* h);

// x [B][L] -> out [B][32][T] (power, or dB with to_db).  steps = 0: every frame.  steps = T2 > 0: only the frames the keyword spotter
// reads, 16 j + i for i < 5, j < T2, are computed and written; the rest of out is not touched.  L >= kMelMinL is the caller's check.
void launch_kws_mel(const KwsMelConst& c, const float* x, int B, int L, int steps, float* out, int to_db, hipStream_t s);

// g_x [B][L] = (d dB / d x)^T g_spec for g_spec [B][32][T]; spec: optional, the dB spectrogram of the forward (its bits).  steps as
// above: with steps > 0 only the read frames of g_spec are read (and of spec written), every other frame counts as zero.
void launch_kws_mel_vjp(const KwsMelConst& c, const float* x, const float* g_spec, int B, int L, int steps, float* g_x, float* spec,
                        hipStream_t s);

}  // namespace dmad
