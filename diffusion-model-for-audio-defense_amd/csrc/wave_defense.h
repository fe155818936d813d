// Launchers of the waveform-defense kernels in wave_defense.hip (smoothing, polyphase FIR resampling, time-parallel IIR).
#pragma once
#include "dmad_common.h"
#include "wave_defense_host.h"

namespace dmad {

// kind 0 mean (odd window <= 63) / 1 median (window 3, 5, 7, 9), zero padding; arguments are checked by the caller (wave_smooth_check)
void launch_wave_smooth(const float* x, int B, int L, int kind, int window, float* y, hipStream_t s);
// median only (the mean's VJP is launch_wave_smooth on g_y): g_x[s] = sum_t g_y[t] [src(t) == s], a gather
void launch_wave_median_vjp(const float* x, const float* g_y, int B, int L, int window, float* g_x, hipStream_t s);
// y[i * P + j] = sum_k ker[j][k] xpad[i * stride + k]; ker is a HOST array of P * taps <= kWaveMaxTaps floats
void launch_wave_resample(const float* x, int B, int L_in, const float* ker, int P, int taps, int stride, int width, int L_out, float* y,
                          hipStream_t s);
void launch_wave_resample_vjp(const float* g_y, int B, int L_in, const float* ker, int P, int taps, int stride, int width, int L_out,
                              float* g_x, hipStream_t s);
// One workgroup per row.  reverse == 0:  u = lfilter(x);  y = clamp(u, lo, hi) and / or y_raw = u (either may be null).
// reverse != 0:  y = flip(lfilter(flip(x * m))),  m = [lo <= mask_src <= hi] (mask_src null: m = 1), no clamp.  Returns a hipError_t.
int launch_wave_iir(const IirPlan& p, const float* x, const float* mask_src, int B, int L, float lo, float hi, int reverse, float* y,
                    float* y_raw, hipStream_t s);

}  // namespace dmad
