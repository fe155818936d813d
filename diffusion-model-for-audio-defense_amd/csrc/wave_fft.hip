// Whole-clip real FFT pair in LDS (wave_fft.h): one workgroup per clip, exact fp32 in a fixed order, no atomics.
//
// The L real samples of a clip are read as M = L / 2 complex points z[n] = x[2n] + i x[2n+1].  Their M-point FFT runs as Stockham stages
// (radix 4, 2, 5; FftPlan) in ONE LDS buffer of M float2: in a stage every thread reads the inputs of all its butterflies (j, j + M/R, ...:
// consecutive threads read consecutive 8-byte points, which is conflict-free), computes them in registers, and writes only after a
// barrier, so no second buffer is needed.  The writes of stage Ns go to (j / Ns) Ns R + j % Ns + r Ns: runs of Ns consecutive points R Ns
// apart, which is a 2R-dword stride in the first stage (an R-way write conflict there, none once Ns >= 32); the buffer is not padded,
// every byte of padding would come off the longest clip served.  The inverse is the same forward transform between two conjugations.
// Twiddles are table reads (exp(-2 pi i j / L), float64 rounded once), never recurrences.
#include "wave_fft.h"

#include "kernel_setup.h"

namespace dmad {

namespace {

__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return float2{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return float2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return float2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ float cmag(float2 a) { return sqrtf(a.x * a.x + a.y * a.y); }

// forward R-point DFT of v, in place
template <int R>
__device__ __forceinline__ void butterfly(float2* v);

template <>
__device__ __forceinline__ void butterfly<2>(float2* v) {
    const float2 a = v[0], b = v[1];
    v[0] = cadd(a, b);
    v[1] = csub(a, b);
}

template <>
__device__ __forceinline__ void butterfly<4>(float2* v) {
    const float2 a = cadd(v[0], v[2]), b = csub(v[0], v[2]), c = cadd(v[1], v[3]), d = csub(v[1], v[3]);
    v[0] = cadd(a, c);
    v[2] = csub(a, c);
    v[1] = float2{b.x + d.y, b.y - d.x};      // b - i d
    v[3] = float2{b.x - d.y, b.y + d.x};      // b + i d
}

template <>
__device__ __forceinline__ void butterfly<5>(float2* v) {
    constexpr float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f;      // cos(2 pi / 5), cos(4 pi / 5)
    constexpr float s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;       // sin(2 pi / 5), sin(4 pi / 5)
    const float2 x0 = v[0];
    const float2 a1 = cadd(v[1], v[4]), a2 = cadd(v[2], v[3]), b1 = csub(v[1], v[4]), b2 = csub(v[2], v[3]);
    const float2 t1 = float2{x0.x + c1 * a1.x + c2 * a2.x, x0.y + c1 * a1.y + c2 * a2.y};
    const float2 t2 = float2{x0.x + c2 * a1.x + c1 * a2.x, x0.y + c2 * a1.y + c1 * a2.y};
    const float2 u1 = float2{s1 * b1.x + s2 * b2.x, s1 * b1.y + s2 * b2.y};
    const float2 u2 = float2{s2 * b1.x - s1 * b2.x, s2 * b1.y - s1 * b2.y};
    v[0] = float2{x0.x + a1.x + a2.x, x0.y + a1.y + a2.y};
    v[1] = float2{t1.x + u1.y, t1.y - u1.x};  // t1 - i u1
    v[4] = float2{t1.x - u1.y, t1.y + u1.x};
    v[2] = float2{t2.x + u2.y, t2.y - u2.x};
    v[3] = float2{t2.x - u2.y, t2.y + u2.x};
}

// One Stockham stage of radix R on buf[0, M), Ns the product of the radices before it.  K butterflies per thread at the most
// (FftPlan: M / R <= K * kFftThreads).  Ends behind a barrier.
template <int R, int K>
__device__ __forceinline__ void fft_stage(float2* buf, const float2* __restrict__ tw, int M, int L, int Ns, int tid) {
    const int nb = M / R, step = L / (Ns * R);
    float2 v[K][R];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int j = tid + i * kFftThreads;
        if (j < nb) {
            const int k = j % Ns;
            v[i][0] = buf[j];
#pragma unroll
            for (int r = 1; r < R; ++r) v[i][r] = cmul(buf[j + r * nb], tw[r * k * step]);      // r k step < L
            butterfly<R>(v[i]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int j = tid + i * kFftThreads;
        if (j < nb) {
            const int k = j % Ns, j0 = (j - k) * R + k;                                         // j0 + (R - 1) Ns < M
#pragma unroll
            for (int r = 0; r < R; ++r) buf[j0 + r * Ns] = v[i][r];
        }
    }
    __syncthreads();
}

struct FftStages {
    int n;
    int radix[kFftMaxStages];
};

// buf <- its forward M-point FFT, in natural order.  Called by all threads, behind a barrier; ends behind one.
__device__ __forceinline__ void fft_forward(float2* buf, const float2* __restrict__ tw, const FftStages& st, int M, int L, int tid) {
    int Ns = 1;
    for (int s = 0; s < st.n; ++s) {
        const int R = st.radix[s];
        if (R == 4) fft_stage<4, kFftPerThread>(buf, tw, M, L, Ns, tid);
        else if (R == 2) fft_stage<2, 2 * kFftPerThread>(buf, tw, M, L, Ns, tid);
        else fft_stage<5, kFftPerThread>(buf, tw, M, L, Ns, tid);
        Ns *= R;
    }
}

constexpr int kFftWaves = kFftThreads / 64;

// the real-FFT post-pass:  X[k] = E + W^k O,  E = (Z[k] + conj Z[M-k]) / 2,  O = -i (Z[k] - conj Z[M-k]) / 2,  Z[M] = Z[0]
__global__ __launch_bounds__(kFftThreads) void wave_rfft_kernel(FftStages st, const float2* __restrict__ tw, const float* __restrict__ x,
                                                                  float2* __restrict__ spec, float* __restrict__ maxmag, int M) {
    extern __shared__ float2 fft_lds[];
    float2* buf = fft_lds;
    float* red = (float*)(fft_lds + M);
    const int tid = threadIdx.x, L = 2 * M;
    const float2* row = (const float2*)(x + (size_t)blockIdx.x * L);
    for (int n = tid; n < M; n += kFftThreads) buf[n] = row[n];
    __syncthreads();
    fft_forward(buf, tw, st, M, L, tid);
    float2* out = spec + (size_t)blockIdx.x * (M + 1);
    float top = 0.f;
    for (int k = tid; k <= M; k += kFftThreads) {
        const float2 a = buf[k == M ? 0 : k], bq = buf[(k == 0 || k == M) ? 0 : M - k];
        const float2 b = float2{bq.x, -bq.y};
        const float2 E = float2{0.5f * (a.x + b.x), 0.5f * (a.y + b.y)};
        const float2 O = float2{0.5f * (a.y - b.y), -0.5f * (a.x - b.x)};
        float2 X = cadd(E, cmul(O, tw[k]));
        if (k == 0 || k == M) X.y = 0.f;                     // real input: the DC and Nyquist bins are real
        out[k] = X;
        top = fmaxf(top, cmag(X));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) top = fmaxf(top, __shfl_xor(top, o));
    if ((tid & 63) == 0) red[tid >> 6] = top;
    __syncthreads();
    if (tid == 0) {
        float m = red[0];
        for (int w = 1; w < kFftWaves; ++w) m = fmaxf(m, red[w]);
        maxmag[blockIdx.x] = m;
    }
}

// the inverse pre-pass:  Z'[k] = (X[k] + conj X[M-k]) + i conj(W^k) (X[k] - conj X[M-k]);  z = conj(FFT(conj Z')) / L
__global__ __launch_bounds__(kFftThreads) void wave_irfft_threshold_kernel(FftStages st, const float2* __restrict__ tw,
                                                                             const float2* __restrict__ spec, const float* __restrict__ factor,
                                                                             float* __restrict__ out, int32_t* __restrict__ kept, int M) {
    extern __shared__ float2 fft_lds[];
    float2* buf = fft_lds;
    int* red = (int*)(fft_lds + M);
    const int tid = threadIdx.x, L = 2 * M;
    const float2* in = spec + (size_t)blockIdx.x * (M + 1);
    const bool cut = factor != nullptr;
    const float f = cut ? factor[blockIdx.x] : 0.f;
    int alive = 0;
    for (int k = tid; k < M; k += kFftThreads) {
        float2 a = in[k], b = in[M - k];
        const bool ka = !(cut && cmag(a) < f), kb = !(cut && cmag(b) < f);
        alive += (int)ka + (int)(k == 0 && kb);              // bin M is counted by the thread of bin 0
        if (!ka) a = float2{0.f, 0.f};
        if (!kb) b = float2{0.f, 0.f};
        if (k == 0) { a.y = 0.f; b.y = 0.f; }                // the imaginary parts of the DC and Nyquist bins are ignored
        const float2 sum = float2{a.x + b.x, a.y - b.y}, d = float2{a.x - b.x, a.y + b.y};
        const float2 w = tw[k];
        const float2 t = float2{w.x * d.x + w.y * d.y, w.x * d.y - w.y * d.x};       // conj(W^k) d
        buf[k] = float2{sum.x - t.y, -(sum.y + t.x)};        // conj Z'
    }
    __syncthreads();
    fft_forward(buf, tw, st, M, L, tid);
    const float inv = 1.0f / (float)L;
    float2* row = (float2*)(out + (size_t)blockIdx.x * L);
    for (int n = tid; n < M; n += kFftThreads) {
        const float2 z = buf[n];
        row[n] = float2{z.x * inv, -z.y * inv};
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) alive += __shfl_xor(alive, o);
    if ((tid & 63) == 0) red[tid >> 6] = alive;
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int w = 0; w < kFftWaves; ++w) n += red[w];
        kept[blockIdx.x] = n;
    }
}

// _KenanFFT.py l.233-243 for clip blockIdx.x: the row copy by all threads, the three scalars by thread 0 (nothing else reads them)
__global__ __launch_bounds__(256) void kenan_update_kernel(const long long* __restrict__ pred, const long long* __restrict__ label, int L,
                                                           int targeted, const float* __restrict__ perturbed, float* __restrict__ best,
                                                           float* __restrict__ fmin, float* __restrict__ fmax, float* __restrict__ factor,
                                                           int32_t* __restrict__ succ) {
    const int b = blockIdx.x;
    const bool same = pred[b] == label[b];
    const bool won = targeted ? same : !same;
    if (won) {
        const float4* src = (const float4*)(perturbed + (size_t)b * L);
        float4* dst = (float4*)(best + (size_t)b * L);
        for (int q = threadIdx.x; q < L / 4; q += 256) dst[q] = src[q];
    }
    if (threadIdx.x == 0) {
        const float f = factor[b];
        float lo = fmin[b], hi = fmax[b];
        if (won) {
            hi = f;
            fmax[b] = f;
            succ[b] = 1;
        } else {
            lo = f;
            fmin[b] = f;
        }
        factor[b] = fabsf(__fdiv_rn(__fadd_rn(lo, hi), 2.0f));
    }
}

FftStages stages_of(const FftPlan& p) {
    FftStages st;
    st.n = p.nstages;
    for (int i = 0; i < kFftMaxStages; ++i) st.radix[i] = p.radix[i];
    return st;
}

}  // namespace

// KF_WAVE_FFT (kernel_setup.hip, once per device; the exports ask for it before they launch): more than the default 64 KiB of dynamic
// LDS needs the attribute, and both kernels may take the longest clip the plan serves
int wave_fft_configure() {
    constexpr int lds = kFftMaxM * 8 + kFftScratchBytes;
    static_assert(lds <= kFftLdsCap, "the longest plan must fit in LDS");
    return set_max_lds({{(const void*)wave_rfft_kernel, lds}, {(const void*)wave_irfft_threshold_kernel, lds}});
}

void launch_wave_rfft(const FftPlan& p, const float* tw, const float* x, int B, float* spec, float* maxmag, hipStream_t s) {
    hipLaunchKernelGGL(wave_rfft_kernel, dim3(B), dim3(kFftThreads), (size_t)p.lds_bytes, s, stages_of(p), (const float2*)tw, x, (float2*)spec,
                       maxmag, p.M);
}

void launch_wave_irfft_threshold(const FftPlan& p, const float* tw, const float* spec, const float* factor, int B, float* out, int32_t* kept,
                                hipStream_t s) {
    hipLaunchKernelGGL(wave_irfft_threshold_kernel, dim3(B), dim3(kFftThreads), (size_t)p.lds_bytes, s, stages_of(p), (const float2*)tw,
                       (const float2*)spec, factor, out, kept, p.M);
}

void launch_kenan_update(const long long* pred, const long long* label, int B, int L, int targeted, const float* perturbed, float* best,
                         float* fmin, float* fmax, float* factor, int32_t* succ, hipStream_t s) {
    hipLaunchKernelGGL(kenan_update_kernel, dim3(B), dim3(256), 0, s, pred, label, L, targeted, perturbed, best, fmin, fmax, factor, succ);
}

}  // namespace dmad
