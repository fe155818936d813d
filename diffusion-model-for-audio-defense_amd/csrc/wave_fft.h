// Whole-clip real FFT and its thresholded inverse (wave_fft.hip), and the bisection update of the Kenansville FFT attack.
// The plan and the twiddle table are plain C++ without a HIP include, so a stand-alone host program can compile and check them
// (tests/wave_fft_plan_main.cc); the launch functions below them are declared for HIP translation units only.
#pragma once
#include <math.h>
#include <stdint.h>

namespace dmad {

constexpr int kFftThreads = 1024;          // one workgroup per clip
constexpr int kFftPerThread = 4;           // radix-4 / radix-5 butterflies a thread holds in registers across a stage's barrier (radix 2: twice as many)
constexpr int kFftMaxStages = 8;
constexpr int kFftScratchBytes = 256;      // the workgroup reductions (one slot per wave)
constexpr int kFftLdsCap = 160 * 1024;     // LDS of one CU
constexpr int kFftMaxM = 4 * kFftPerThread * kFftThreads;      // 16384: a radix-4 stage of M points is M / 4 butterflies

// A clip of L real samples is M = L / 2 complex points z[n] = x[2n] + i x[2n+1]; their FFT runs as `nstages` Stockham stages of
// radix[s], the radix-4 stages first, then at most one radix-2 stage, then the radix-5 stages.
struct FftPlan {
    int L = 0, M = 0, nstages = 0;
    int radix[kFftMaxStages] = {0};
    int lds_bytes = 0;                     // M complex fp32 points (no padding) + kFftScratchBytes
};

// Returns nullptr, or the rule the length breaks.
inline const char* wave_fft_plan(int L, FftPlan* p) {
    if (!p) return "null plan";
    *p = FftPlan();
    if (L < 128 || L % 128) return "the length must be a positive multiple of 128";
    int m = L / 2, twos = 0, fives = 0;
    while (m % 2 == 0) { m /= 2; ++twos; }
    while (m % 5 == 0) { m /= 5; ++fives; }
    if (m != 1) return "M = L / 2 must factor into radices 4, 2 and 5 (it has another prime factor)";
    const int M = L / 2;
    if ((long)M * 8 + kFftScratchBytes > (long)kFftLdsCap) return "M = L / 2 complex fp32 points plus 256 B of scratch must fit in 160 KiB of LDS";
    if (M > kFftMaxM) return "M = L / 2 must be at most 16384 (4 radix-4 butterflies per thread and stage)";
    if (twos / 2 + twos % 2 + fives > kFftMaxStages) return "more than 8 stages";
    p->L = L;
    p->M = M;
    for (int i = 0; i < twos / 2; ++i) p->radix[p->nstages++] = 4;
    if (twos % 2) p->radix[p->nstages++] = 2;
    for (int i = 0; i < fives; ++i) p->radix[p->nstages++] = 5;
    p->lds_bytes = M * 8 + kFftScratchBytes;
    return nullptr;
}

// out[2j], out[2j+1] = cos, sin of -2 pi j / L for j in [0, L): float64 on the host, rounded once to fp32
inline void wave_fft_twiddles(int L, float* out) {
    for (int j = 0; j < L; ++j) {
        const double a = -2.0 * M_PI * (double)j / (double)L;
        out[2 * j] = (float)cos(a);
        out[2 * j + 1] = (float)sin(a);
    }
}

}  // namespace dmad

#ifdef __HIP__
#include <hip/hip_runtime.h>

namespace dmad {

// x [B][L] -> spec [B][M + 1][2] (torch.fft.rfft), maxmag [B] = max_k |spec[b][k]|.  `tw` is the device image of wave_fft_twiddles(L).
// The caller has made KF_WAVE_FFT ready (kernel_setup.h).  x and out rows are read and written as float2: 8-byte aligned bases.
void launch_wave_rfft(const FftPlan& p, const float* tw, const float* x, int B, float* spec, float* maxmag, hipStream_t s);
// spec -> out [B][L] = irfft of spec with every bin |X| < factor[b] zeroed (factor null: none), kept [B] = the surviving bins
void launch_wave_irfft_threshold(const FftPlan& p, const float* tw, const float* spec, const float* factor, int B, float* out, int32_t* kept,
                                hipStream_t s);
// one bisection step per clip: see dmad_kenan_update (include/dmad.h); the rows are copied as float4: 16-byte aligned bases
void launch_kenan_update(const long long* pred, const long long* label, int B, int L, int targeted, const float* perturbed, float* best,
                         float* fmin, float* fmax, float* factor, int32_t* succ, hipStream_t s);

}  // namespace dmad
#endif
