// M5 raw-waveform classifier (reference audio_models/M5/M5Net.py:4-38) on the engine, exact fp32 (m5.hip): four blocks of
// Conv1d -> eval-BatchNorm (folded scale / shift) -> ReLU -> MaxPool1d(4), the mean over time, Linear and log_softmax in ONE launch,
// one workgroup per clip with every activation in LDS, and the input VJP in the same launch: the forward is recomputed, only each
// pooled unit's decision (its arg-max and whether the maximum is > 0) is kept, and the walk back needs no activation.  Every sum runs
// in a fixed order inside one workgroup: a clip's bits do not depend on the batch or on its row.  No workspace in global memory.
#pragma once
#include "dmad_common.h"

namespace dmad {

constexpr int kM5Ch = 32;          // n_channel: conv1 / conv2 have 32 output channels, conv3 / conv4 64
constexpr int kM5Stride = 16;      // conv1's stride
constexpr int kM5MaxOut = 64;      // n_output <= 64 (one wave holds the head)

// Device images of the folded weights (all in one buffer, packed by dmad_finalize_weights)
struct M5Weights {
    const float* w1t = nullptr;      // conv1 [k][32]: the forward's LDS image (lane = channel group)
    const float* w1c = nullptr;      // conv1 [32][k]: the backward's LDS image (lane = sample)
    const float* wf[3] = {};         // conv2..4 [ci][tap][co]: forward (lane = co)
    const float* wb[3] = {};         // conv2..4 [co][tap][ci]: backward (lane = ci)
    const float* scale[4] = {};      // s = gamma / sqrt(var + eps)
    const float* shift[4] = {};      // beta + (bias - mean) * s
    const float* fcw = nullptr;      // [n_out][64]
    const float* fcb = nullptr;
};

// Frames, pitches and the LDS layout for one (clip length, first kernel size); every offset in floats unless it says bytes
struct M5Geom {
    int L = 0, K1 = 0, n_out = 0;
    int C[4] = {32, 32, 64, 64};
    int Tc[4] = {}, T[4] = {};       // conv frames / pooled frames (the pool drops Tc % 4 frames)
    int pit[4] = {};                 // row pitch of pooled map l (T rounded up to 4)
    int pitG[4] = {};                // row pitch of the dense gradient map at conv l's output, l = 1..3 (frame f at 2 + f); [0]: T[0], compact
    int oX = 0, oW1 = 0, oP[4] = {}, oSmall = 0;     // forward: padded clip, conv1 image, pooled maps, head scratch (4 * 64 floats)
    int oG[4] = {}, oW1c = 0;                        // backward arena, overlaid on [oX, oSmall)
    int decB = 0, oDec[4] = {};                      // byte offset of the decisions, and layer l's bytes inside them ([c][T[l]])
    int lds_bytes = 0;
};

// Fills g for (L, K1, n_out); returns nullptr, or the reason the geometry is not supported (names the field)
const char* m5_geometry(int L, int K1, int n_out, M5Geom* g);

// One launch over B clips x [B][L].  logp [B][n_out], cls [B] (the first maximum of logp), g_x [B][L] are optional; g_x needs g_logp
// [B][n_out].  tape_layer 1..4: also writes that layer's pooled post-ReLU map, pooled [B][C][T] floats, and decisions dec [B][C][T]
// bytes (arg | on << 2).  The forward of every variant is the same code, so its bits are the same.
void launch_m5(const M5Weights& w, const M5Geom& g, const float* x, int B, float* logp, int32_t* cls, const float* g_logp, float* g_x,
               int tape_layer, float* pooled, uint8_t* dec, hipStream_t s);

// The forward over `rows` Monte Carlo samples of ONE clip [L] (certified_robust.py:34-67 with denoiser None): workgroup b stages
// clip + delta[b] (delta [rows][L]), or clip + sigma * the Philox normals keyed (seed, sample0 + b, stream 0) when delta is null (the
// bits of launch_mc_noise_scale at scale 1), into LDS, so the noisy clips never exist in device memory; the rest is launch_m5's forward,
// bit for bit.  counts [n_out] += 1 at each sample's first maximum; logp [rows][n_out] is optional.
void launch_m5_noisy(const M5Weights& w, const M5Geom& g, const float* clip, const float* delta, float sigma, uint64_t seed, uint64_t sample0,
                     int rows, unsigned long long* counts, float* logp, hipStream_t s);

}  // namespace dmad
