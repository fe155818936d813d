// Attention-CRNN keyword spotter (reference audio_models/RCNN_KWS/model.py:66-114 KWSModel) on the engine, exact fp32 (kws.hip):
// depthwise Conv1d(32,32,5,stride 2) -> pointwise Conv1d(32,64,1,stride 8) -> 2-layer bidirectional GRU(64) with h0 = 0 -> additive
// attention over time -> bias-free Linear to 4 classes -> log_softmax in ONE launch, one workgroup per clip with every activation in
// LDS, and the input VJP in the same launch: the forward is recomputed by the same code, the hidden states of both layers stay in LDS
// and the walk back goes through head, attention, layer 1, layer 0 and the two convs.  Every sum runs in a fixed order inside one
// workgroup: a clip's bits do not depend on the batch, on its row or on the call.  No workspace in global memory, nothing reserved.
// The longest row served is kKwsMaxT spectrogram frames (kKwsMaxSteps GRU steps): what 160 KB of LDS hold, see kws_geometry.
#pragma once
#include "dmad_common.h"

namespace dmad {

constexpr int kKwsIn = 32;         // in_size: mel bins = depthwise channels
constexpr int kKwsH = 64;          // hidden_size of the pointwise conv and of the GRU
constexpr int kKwsG = 3 * kKwsH;   // gate rows of one direction (r, z, n)
constexpr int kKwsK = 5;           // depthwise kernel, stride 2; the pointwise conv has stride 8: step j reads frames 16 j .. 16 j + 4
constexpr int kKwsHop = 16;
constexpr int kKwsOut = 4;         // num_classes
constexpr int kKwsMaxSteps = 40;   // GRU steps whose activations fit the LDS of one CU
constexpr int kKwsMaxT = kKwsHop * (kKwsMaxSteps - 1) + kKwsK + 15;   // 644: the longest row with kKwsMaxSteps steps (THE cap)
constexpr int kKwsMinT = kKwsK;

// Device images of the weights (all in one buffer, packed by dmad_finalize_weights).  "T" images are transposed so that lanes, which
// run over output rows there, read consecutive floats; the plain ones serve the walk back, where lanes run over the input columns
struct KwsWeights {
    const float* dw = nullptr;       // depthwise [32][5]
    const float* dwb = nullptr;      // [32]
    const float* pwT = nullptr;      // pointwise [32 c][64 o]
    const float* pw = nullptr;       // pointwise [64 o][32 c]
    const float* pwb = nullptr;      // [64]
    const float* wihT[2] = {};       // layer l: [K_l][384] (K_0 = 64, K_1 = 128; column = direction * 192 + gate row)
    const float* wih[2] = {};        // [384][K_l]
    const float* bih[2] = {};        // [384]
    const float* whhT[2] = {};       // [64][384]
    const float* whh[2] = {};        // [384][64]
    const float* bhh[2] = {};        // [384]
    const float* wxT = nullptr;      // attention Wx_b [128 k][128 m]
    const float* wx = nullptr;       // [128 m][128 k]
    const float* wxb = nullptr;      // [128]
    const float* vt = nullptr;       // [128]
    const float* u = nullptr;        // [4][128]
};

// Steps and the LDS layout for one row length; every offset in floats
struct KwsGeom {
    int T = 0, T1 = 0, T2 = 0;       // spectrogram frames, depthwise frames, GRU steps
    int oX0 = 0;                     // sepconv output [T2][64]
    int oGI = 0;                     // input projections of the layer in flight [T2][384]; the walk back overwrites them with their gradient
    int oH[2] = {};                  // layer outputs [T2][128], forward direction first
    int oGH[2] = {};                 // their gradients [T2][128]; oGH[0] first holds the attention's tanh units
    int oSmall = 0;                  // step and head scratch, kKwsSmall floats
    int lds_bytes = 0;
};
constexpr int kKwsSmall = 2048;

// Fills g for a row of T frames; returns nullptr, or the reason the geometry is not supported (names the field)
const char* kws_geometry(int T, KwsGeom* g);

// One launch over B rows spec [B][32][T] (4-byte aligned rows).  logp [B][4], cls [B] (the first maximum of logp) and g_spec [B][32][T]
// are optional; g_spec needs g_logp [B][4] and is written whole, exact zeros outside frames 16 j .. 16 j + 4 included.  tape_stage
// 0..3 (-1: none) also writes tape: 0 the sepconv output [B][T2][64], 1 / 2 the output of GRU layer 0 / 1 [B][T2][128], 3 the attention
// scores [B][T2].  The forward of every variant is the same code, so its bits are the same.
void launch_kws(const KwsWeights& w, const KwsGeom& g, const float* spec, int B, float* logp, int32_t* cls, const float* g_logp,
                float* g_spec, int tape_stage, float* tape, hipStream_t s);

}  // namespace dmad
