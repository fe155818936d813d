// Host side of the waveform defenses (wave_defense.hip): the plan of the time-parallel IIR filter and the validation of a
// dmad_wave_defense.  Plain C++ without a HIP include, so a stand-alone host program can compile and check it.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/dmad.h"

namespace dmad {

constexpr int kIirMaxOrder = 8;       // direct-form order n: b[n + 1], a[n + 1]
constexpr int kIirMaxSegs = 128;      // segments per row == threads per workgroup
constexpr int kIirMaxLen = 39936;     // the row and the segment states stay in LDS: 4 L + 4 KiB <= 160 KiB
constexpr int kWaveMaxTaps = 256;     // phases * taps of one FIR kernel (it travels as a kernel argument)
constexpr int kWaveMaxMean = 63;      // largest mean window

// b / a[0], a / a[0] as fp32, the segment geometry and the n x n zero-input transition matrix of one full segment
struct IirPlan {
    int n = 0, T = 0, nseg = 0;
    float b[kIirMaxOrder + 1] = {0}, a[kIirMaxOrder + 1] = {0};
    float M[kIirMaxOrder * kIirMaxOrder] = {0};      // [i][j]: state i after T zero-input steps from the unit state j
};

// Segment length of a row of L samples: at most kIirMaxSegs segments, odd so that the per-thread LDS walks (stride T words) touch
// 64 different banks
inline int iir_segment_len(int L) {
    int T = (L + kIirMaxSegs - 1) / kIirMaxSegs;
    if (T < 1) T = 1;
    return T | 1;
}

// The filter is scipy.signal.lfilter's transposed direct form II:  y = b0 x + z0;  z_i = b_{i+1} x - a_{i+1} y + z_{i+1}  (z_n = 0).
// With zero input it is linear in the state, z(T) = M z(0); M is computed here in float64 from the fp32 coefficients the kernel runs.
// Returns nullptr, or the reason the arguments are refused.
inline const char* iir_plan(const float* b, const float* a, int order, int L, IirPlan* p) {
    if (!b || !a || !p) return "null coefficient array";
    if (order < 1 || order > kIirMaxOrder) return "order outside [1, 8]";
    if (L < 1 || L > kIirMaxLen) return "row length outside [1, 39936]";
    if (!(a[0] != 0.f) || !isfinite(a[0])) return "a[0] must be finite and non-zero";
    *p = IirPlan();
    p->n = order;
    p->T = iir_segment_len(L);
    p->nseg = (L + p->T - 1) / p->T;
    for (int i = 0; i <= order; ++i) {
        if (!isfinite(b[i]) || !isfinite(a[i])) return "non-finite coefficient";
        p->b[i] = (float)((double)b[i] / (double)a[0]);
        p->a[i] = (float)((double)a[i] / (double)a[0]);
    }
    const int n = order;
    for (int j = 0; j < n; ++j) {
        double z[kIirMaxOrder + 1] = {0};
        z[j] = 1.0;
        for (int t = 0; t < p->T; ++t) {
            const double y = z[0];
            for (int i = 0; i < n; ++i) z[i] = z[i + 1] - (double)p->a[i + 1] * y;     // z[n] stays 0
        }
        for (int i = 0; i < n; ++i) {
            if (!isfinite(z[i]) || fabs(z[i]) > 3.0e38) return "unstable filter: the segment transition overflows fp32";
            p->M[i * n + j] = (float)z[i];
        }
    }
    return nullptr;
}

inline const char* wave_smooth_check(int kind, int window) {
    if (kind != 0 && kind != 1) return "kind must be 0 (mean) or 1 (median)";
    if (window < 1 || !(window & 1)) return "window must be odd and >= 1";
    if (kind == 0 && window > kWaveMaxMean) return "mean window above 63";
    if (kind == 1 && window != 3 && window != 5 && window != 7 && window != 9) return "median window must be 3, 5, 7 or 9";
    return nullptr;
}

inline const char* wave_resample_check(const float* ker, int L_in, int phases, int taps, int stride, int width, int L_out) {
    if (!ker) return "null FIR kernel";
    if (L_in < 1 || L_out < 1) return "L_in and L_out must be >= 1";
    if (phases < 1 || taps < 1 || stride < 1 || width < 0) return "phases, taps and stride must be >= 1, width >= 0";
    if ((long)phases * taps > kWaveMaxTaps) return "phases * taps above 256";
    // every output reads inside xpad = [width zeros | x | width + stride zeros]
    const long frames = ((long)L_out + phases - 1) / phases;
    if ((frames - 1) * stride + taps > (long)L_in + 2l * width + stride) return "L_out reaches past the padded input";
    return nullptr;
}

// dmad_wave_defense as dmad_defense_query_logits takes it; L is the engine's clip length
inline const char* wave_defense_check(const dmad_wave_defense* d, int L, IirPlan* plan) {
    if (!d) return "null dmad_wave_defense";
    if (d->struct_size != (int32_t)sizeof(dmad_wave_defense)) return "dmad_wave_defense.struct_size does not match this library";
    switch (d->kind) {
    case DMAD_WAVE_AS: return wave_smooth_check(0, d->window);
    case DMAD_WAVE_MS: return wave_smooth_check(1, d->window);
    case DMAD_WAVE_DS: {
        if (d->down_len < 1) return "down_len must be >= 1";
        if (const char* m = wave_resample_check(d->down_ker, L, d->down_phases, d->down_taps, d->down_stride, d->down_width, d->down_len)) return m;
        if (d->down_len > L) return "down_len above the clip length";
        return wave_resample_check(d->up_ker, d->down_len, d->up_phases, d->up_taps, d->up_stride, d->up_width, L);
    }
    case DMAD_WAVE_IIR:
        if (!(d->hi >= d->lo)) return "empty clamp range";
        return iir_plan(d->b, d->a, d->order, L, plan);
    default: return "unknown defense kind";
    }
}

}  // namespace dmad
