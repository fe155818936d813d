// Baseline waveform defenses (transforms/time_defense.py AS / MS, transforms/frequency_defense.py DS / LPF / BPF) on rows [B][len]:
// windowed mean and median with their VJPs, a polyphase FIR resampler with its transposed operator, and a time-parallel IIR filter
// that serves forward and adjoint.  fp32 throughout, one writer per output element, no atomics: an output row is a function of its own
// input row, bit-reproducible and independent of the batch.  Where include/dmad.h states a formula with fl() the products and sums are
// rounded on their own (__fmul_rn / __fadd_rn, no contraction), as in elementwise.hip; the FIR sums run in float64 and round once.  DESIGN.md section 17.
#include "wave_defense.h"
#include "kernel_setup.h"

namespace dmad {

namespace {

inline unsigned nblk(long n, int per) { return (unsigned)((n + per - 1) / per); }

// ---------------------------------------------------------------------------------------------------------------- smoothing
// y[t] = sum_k fl(x[t + k - p] * c), c = fl(1 / w), k ascending; a padding position adds fl(0 * c) = 0
__global__ void __launch_bounds__(256) wave_mean_kernel(const float* __restrict__ x, float* __restrict__ y, long total, int L, int w) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % L);
    const float* row = x + (i - t);
    const int p = (w - 1) / 2;
    const float c = __fdiv_rn(1.f, (float)w);
    float acc = 0.f;
    for (int k = 0; k < w; ++k) {
        const int u = t + k - p;
        const float v = (u >= 0 && u < L) ? row[u] : 0.f;
        acc = __fadd_rn(acc, __fmul_rn(v, c));
    }
    y[i] = acc;
}

// The window position the median is taken from: the LOWEST k whose value has rank p = (W - 1) / 2, i.e. #{v_j < v_k} <= p < #{v_j <= v_k}.
// A window with a NaN: its first NaN (torch.median propagates the NaN).
template <int W>
__device__ __forceinline__ int median_src(const float* v) {
    constexpr int p = (W - 1) / 2;
    int src = -1;
#pragma unroll
    for (int k = W - 1; k >= 0; --k) {
        int lt = 0, le = 0;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            lt += v[j] < v[k] ? 1 : 0;
            le += v[j] <= v[k] ? 1 : 0;
        }
        if (lt <= p && le > p) src = k;
    }
#pragma unroll
    for (int k = W - 1; k >= 0; --k)
        if (v[k] != v[k]) src = k;
    return src;
}

template <int W>
__global__ void __launch_bounds__(256) wave_median_kernel(const float* __restrict__ x, float* __restrict__ y, long total, int L) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    constexpr int p = (W - 1) / 2;
    const int t = (int)(i % L);
    const float* row = x + (i - t);
    float v[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int u = t + k - p;
        v[k] = (u >= 0 && u < L) ? row[u] : 0.f;
    }
    const int src = median_src<W>(v);
    float r = v[0];
#pragma unroll
    for (int k = 1; k < W; ++k)
        if (k == src) r = v[k];
    y[i] = r;
}

// g_x[s] = sum over the windows t in [s - p, s + p] (inside the row, ascending) of g_y[t] [src(t) == s]: window t holds the positions
// t - p .. t + p, so s is its slot p - (t - s).  The 4p + 1 samples around s are read once.
template <int W>
__global__ void __launch_bounds__(256) wave_median_vjp_kernel(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ gx,
                                                              long total, int L) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    constexpr int p = (W - 1) / 2;
    const int s = (int)(i % L);
    const float* row = x + (i - s);
    const float* grow = gy + (i - s);
    float nb[2 * W - 1];
#pragma unroll
    for (int k = 0; k < 2 * W - 1; ++k) {
        const int u = s + k - 2 * p;
        nb[k] = (u >= 0 && u < L) ? row[u] : 0.f;
    }
    float acc = 0.f;
#pragma unroll
    for (int d = -p; d <= p; ++d) {
        const int t = s + d;
        float v[W];
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = nb[d + p + k];
        const int src = median_src<W>(v);
        if (t >= 0 && t < L && src == p - d) acc = __fadd_rn(acc, grow[t]);
    }
    gx[i] = acc;
}

// ---------------------------------------------------------------------------------------------------------------- FIR resampling
struct FirTaps { float v[kWaveMaxTaps]; };

// one thread per output o = i * P + j; x index of xpad[m] is m - width.  The sum runs in float64 (fp32 products are exact there) and is
// rounded once: 28 taps summed in fp32 would spend the 4u sum|terms| the tests allow
__global__ void __launch_bounds__(256) wave_resample_kernel(FirTaps ker, const float* __restrict__ x, float* __restrict__ y, long total, int L_in,
                                                            int L_out, int P, int taps, int stride, int width) {
    __shared__ float kl[kWaveMaxTaps];
    for (int q = threadIdx.x; q < P * taps; q += 256) kl[q] = ker.v[q];
    __syncthreads();
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int o = (int)(g % L_out);
    const float* row = x + (g / L_out) * L_in;
    const int i = o / P, j = o - i * P;
    const int m0 = i * stride - width;
    double acc = 0.0;
    for (int k = 0; k < taps; ++k) {
        const int m = m0 + k;
        const float v = (m >= 0 && m < L_in) ? row[m] : 0.f;
        acc += (double)kl[j * taps + k] * (double)v;
    }
    y[g] = (float)acc;
}

// g_x[m] = sum over the outputs o = i * P + j < L_out that read x[m] with tap k = m + width - i * stride in [0, taps): frames i ascending,
// phases j ascending
__global__ void __launch_bounds__(256) wave_resample_vjp_kernel(FirTaps ker, const float* __restrict__ gy, float* __restrict__ gx, long total,
                                                                int L_in, int L_out, int P, int taps, int stride, int width) {
    __shared__ float kl[kWaveMaxTaps];
    for (int q = threadIdx.x; q < P * taps; q += 256) kl[q] = ker.v[q];
    __syncthreads();
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int m = (int)(g % L_in);
    const float* grow = gy + (g / L_in) * L_out;
    const int top = m + width;                               // k = top - i * stride
    int i_lo = top - taps + 1;
    i_lo = i_lo > 0 ? (i_lo + stride - 1) / stride : 0;
    const int i_hi = top / stride;
    double acc = 0.0;
    for (int i = i_lo; i <= i_hi; ++i) {
        const int k = top - i * stride;
        for (int j = 0; j < P; ++j) {
            const int o = i * P + j;
            if (o < L_out) acc += (double)kl[j * taps + k] * (double)grow[o];
        }
    }
    gx[g] = (float)acc;
}

// ---------------------------------------------------------------------------------------------------------------- IIR
struct IirArgs { float b[kIirMaxOrder + 1], a[kIirMaxOrder + 1], M[kIirMaxOrder * kIirMaxOrder]; };

// One step of lfilter's transposed direct form II on the n-vector state z
template <int N>
__device__ __forceinline__ float iir_step(const float (&b)[N + 1], const float (&a)[N + 1], float (&z)[N], float x) {
    const float y = fmaf(b[0], x, z[0]);
#pragma unroll
    for (int i = 0; i < N - 1; ++i) z[i] = fmaf(-a[i + 1], y, fmaf(b[i + 1], x, z[i + 1]));
    z[N - 1] = fmaf(-a[N], y, __fmul_rn(b[N], x));
    return y;
}

// One workgroup of 128 threads per row; LDS = the row [L] + the segment states [N][128] (state i of segment s at i * 128 + s, and the
// row walked with the odd stride T: both conflict-free over the 64 banks).  Global traffic is float4 and coalesced; a reversed row is
// turned around on its way into and out of LDS.
template <int N>
__global__ void __launch_bounds__(kIirMaxSegs) wave_iir_kernel(IirArgs c, const float* __restrict__ x, const float* __restrict__ mask_src,
                                                               float* __restrict__ y, float* __restrict__ y_raw, int L, int T, int nseg,
                                                               float lo, float hi, int reverse) {
    extern __shared__ float iir_lds[];
    float* row = iir_lds;
    float* st = iir_lds + L;
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * L;
    for (int q = tid * 4; q < L; q += kIirMaxSegs * 4) {
        const float4 v = *(const float4*)(x + base + q);
        float e[4] = {v.x, v.y, v.z, v.w};
        if (mask_src) {
            const float4 u = *(const float4*)(mask_src + base + q);
            const float m[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!(m[j] >= lo && m[j] <= hi)) e[j] = 0.f;
        }
        if (reverse) {
#pragma unroll
            for (int j = 0; j < 4; ++j) row[L - 1 - q - j] = e[j];
        } else {
            *(float4*)(row + q) = float4{e[0], e[1], e[2], e[3]};
        }
    }
    __syncthreads();
    float b[N + 1], a[N + 1];
#pragma unroll
    for (int i = 0; i <= N; ++i) { b[i] = c.b[i]; a[i] = c.a[i]; }
    const int t0 = tid * T;
    if (tid < nseg - 1) {                                    // (1) zero-state run of a full segment: its final state
        float z[N];
#pragma unroll
        for (int i = 0; i < N; ++i) z[i] = 0.f;
#pragma unroll 5
        for (int t = t0; t < t0 + T; ++t) (void)iir_step<N>(b, a, z, row[t]);
#pragma unroll
        for (int i = 0; i < N; ++i) st[i * kIirMaxSegs + tid] = z[i];
    }
    __syncthreads();
    if (tid == 0) {                                          // (2) the carry: slot s <- z_in(s);  z_in(s + 1) = M z_in(s) + z_zs(s)
        float z[N];
#pragma unroll
        for (int i = 0; i < N; ++i) z[i] = 0.f;
        for (int s = 0; s < nseg; ++s) {
            float f[N], nz[N];
#pragma unroll
            for (int i = 0; i < N; ++i) f[i] = s < nseg - 1 ? st[i * kIirMaxSegs + s] : 0.f;
#pragma unroll
            for (int i = 0; i < N; ++i) st[i * kIirMaxSegs + s] = z[i];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                nz[i] = f[i];
#pragma unroll
                for (int j = 0; j < N; ++j) nz[i] = fmaf(c.M[i * N + j], z[j], nz[i]);
            }
#pragma unroll
            for (int i = 0; i < N; ++i) z[i] = nz[i];
        }
    }
    __syncthreads();
    if (tid < nseg) {                                        // (3) the segment again, from its true initial state, in place
        float z[N];
#pragma unroll
        for (int i = 0; i < N; ++i) z[i] = st[i * kIirMaxSegs + tid];
        const int t1 = t0 + T < L ? t0 + T : L;
#pragma unroll 5
        for (int t = t0; t < t1; ++t) row[t] = iir_step<N>(b, a, z, row[t]);
    }
    __syncthreads();
    for (int q = tid * 4; q < L; q += kIirMaxSegs * 4) {
        float e[4];
        if (reverse) {
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = row[L - 1 - q - j];
            *(float4*)(y + base + q) = float4{e[0], e[1], e[2], e[3]};
        } else {
            const float4 v = *(const float4*)(row + q);
            if (y_raw) *(float4*)(y_raw + base + q) = v;
            if (y) *(float4*)(y + base + q) = float4{clamp_nan(v.x, lo, hi), clamp_nan(v.y, lo, hi), clamp_nan(v.z, lo, hi), clamp_nan(v.w, lo, hi)};
        }
    }
}

template <int N>
hipError_t iir_launch(const IirArgs& c, const float* x, const float* mask_src, float* y, float* y_raw, int B, int L, int T, int nseg, float lo,
                      float hi, int reverse, hipStream_t s) {
    const size_t lds = ((size_t)L + (size_t)kIirMaxOrder * kIirMaxSegs) * sizeof(float);
    if (int r = kernels_ready(KF_WAVE_IIR)) return (hipError_t)r;      // more than the default 64 KiB of dynamic LDS needs the attribute
    hipLaunchKernelGGL(wave_iir_kernel<N>, dim3(B), dim3(kIirMaxSegs), lds, s, c, x, mask_src, y, y_raw, L, T, nseg, lo, hi, reverse);
    return hipSuccess;
}

FirTaps fir_taps(const float* ker, int n) {
    FirTaps t;
    for (int i = 0; i < kWaveMaxTaps; ++i) t.v[i] = i < n ? ker[i] : 0.f;
    return t;
}

}  // namespace

// KF_WAVE_IIR (kernel_setup.hip, once per device): every order's kernel may take the longest clip
int wave_iir_configure() {
    constexpr int lds = (int)(((size_t)kIirMaxLen + (size_t)kIirMaxOrder * kIirMaxSegs) * sizeof(float));
    return set_max_lds({{(const void*)wave_iir_kernel<1>, lds}, {(const void*)wave_iir_kernel<2>, lds}, {(const void*)wave_iir_kernel<3>, lds},
                        {(const void*)wave_iir_kernel<4>, lds}, {(const void*)wave_iir_kernel<5>, lds}, {(const void*)wave_iir_kernel<6>, lds},
                        {(const void*)wave_iir_kernel<7>, lds}, {(const void*)wave_iir_kernel<8>, lds}});
}

void launch_wave_smooth(const float* x, int B, int L, int kind, int window, float* y, hipStream_t s) {
    const long total = (long)B * L;
    const dim3 grid(nblk(total, 256)), block(256);
    if (kind == 0) { hipLaunchKernelGGL(wave_mean_kernel, grid, block, 0, s, x, y, total, L, window); return; }
    switch (window) {
    case 3: hipLaunchKernelGGL(wave_median_kernel<3>, grid, block, 0, s, x, y, total, L); break;
    case 5: hipLaunchKernelGGL(wave_median_kernel<5>, grid, block, 0, s, x, y, total, L); break;
    case 7: hipLaunchKernelGGL(wave_median_kernel<7>, grid, block, 0, s, x, y, total, L); break;
    default: hipLaunchKernelGGL(wave_median_kernel<9>, grid, block, 0, s, x, y, total, L); break;
    }
}

void launch_wave_median_vjp(const float* x, const float* g_y, int B, int L, int window, float* g_x, hipStream_t s) {
    const long total = (long)B * L;
    const dim3 grid(nblk(total, 256)), block(256);
    switch (window) {
    case 3: hipLaunchKernelGGL(wave_median_vjp_kernel<3>, grid, block, 0, s, x, g_y, g_x, total, L); break;
    case 5: hipLaunchKernelGGL(wave_median_vjp_kernel<5>, grid, block, 0, s, x, g_y, g_x, total, L); break;
    case 7: hipLaunchKernelGGL(wave_median_vjp_kernel<7>, grid, block, 0, s, x, g_y, g_x, total, L); break;
    default: hipLaunchKernelGGL(wave_median_vjp_kernel<9>, grid, block, 0, s, x, g_y, g_x, total, L); break;
    }
}

void launch_wave_resample(const float* x, int B, int L_in, const float* ker, int P, int taps, int stride, int width, int L_out, float* y,
                          hipStream_t s) {
    const long total = (long)B * L_out;
    hipLaunchKernelGGL(wave_resample_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, fir_taps(ker, P * taps), x, y, total, L_in, L_out, P, taps,
                       stride, width);
}

void launch_wave_resample_vjp(const float* g_y, int B, int L_in, const float* ker, int P, int taps, int stride, int width, int L_out,
                              float* g_x, hipStream_t s) {
    const long total = (long)B * L_in;
    hipLaunchKernelGGL(wave_resample_vjp_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, fir_taps(ker, P * taps), g_y, g_x, total, L_in, L_out,
                       P, taps, stride, width);
}

int launch_wave_iir(const IirPlan& p, const float* x, const float* mask_src, int B, int L, float lo, float hi, int reverse, float* y,
                    float* y_raw, hipStream_t s) {
    IirArgs c;
    for (int i = 0; i <= kIirMaxOrder; ++i) { c.b[i] = p.b[i]; c.a[i] = p.a[i]; }
    for (int i = 0; i < kIirMaxOrder * kIirMaxOrder; ++i) c.M[i] = p.M[i];
    switch (p.n) {
#define DMAD_IIR_CASE(N) case N: return (int)iir_launch<N>(c, x, mask_src, y, y_raw, B, L, p.T, p.nseg, lo, hi, reverse, s);
    DMAD_IIR_CASE(1) DMAD_IIR_CASE(2) DMAD_IIR_CASE(3) DMAD_IIR_CASE(4) DMAD_IIR_CASE(5) DMAD_IIR_CASE(6) DMAD_IIR_CASE(7) DMAD_IIR_CASE(8)
#undef DMAD_IIR_CASE
    default: return (int)hipErrorInvalidValue;
    }
}

}  // namespace dmad
