// KWS mel front-end: forward and VJP, one launch each, for clips of any length (kws_mel.h).
#include "kws_mel.h"

#include <cmath>

namespace dmad {

namespace {

constexpr int kThreads = 448;                   // 7 waves: one thread per row of the DFT matrix (402), per sample of a frame (400)
constexpr int kLdD = 404;                       // LDS row of re | im (16-byte rows)
constexpr int kLdP = 204;
constexpr int kOwn = kMelTile - 1;              // blocks of 200 output samples a VJP workgroup owns (all frames)
constexpr int kKwsRead = 5, kKwsStep = 16;      // the frames KWSModel reads: 16 j .. 16 j + 4 (kws.h)
constexpr float kDbBack = 4.3429448190325175f;  // 10 / ln 10

struct MelLds {
    __attribute__((aligned(16))) float xs[(kMelTile + 1) * kMelHop];   // the samples of up to 8 frames, reflect map applied
    __attribute__((aligned(16))) float D[kMelTile][kLdD];              // re [201] | im [201] of each frame, then their gradients
    float P[kMelTile][kLdP];                                           // power
    float M[kMelTile][kMelFilters];                                    // mel power, then the gradient at it
};

// Frames f0 .. f0 + NF - 1 of one clip: stage, windowed DFT (four chains per bin, n ascending in each), power, filterbank (k ascending).
// Leaves re | im in S.D, the power in S.P and the mel power in S.M.  A frame at or past T is computed on whatever the map gives and
// used by nobody.  Reads of S.xs in the DFT are wave-uniform (every lane the same address: a broadcast), so the frame stride of 200
// floats meets no bank conflict and the staging needs no padding
template <int NF>
__device__ __forceinline__ void mel_frames(const KwsMelConst& C, const float* __restrict__ xr, int L, int f0, MelLds& S) {
    const int tid = threadIdx.x;
    __syncthreads();                                   // the previous pass is done with S
    for (int i = tid; i < (NF + 1) * kMelHop; i += kThreads) {
        long q = (long)f0 * kMelHop + i - kMelHop;     // padded index - 200
        if (q < 0) q = -q;
        else if (q >= L) q = 2l * (L - 1) - q;
        S.xs[i] = (q >= 0 && q < L) ? xr[q] : 0.f;
    }
    __syncthreads();
    if (tid < kMelCols) {
        float acc[NF][4];                              // chain j takes the samples n = j (mod 4), ascending; joined (0 + 1) + (2 + 3)
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f][0] = acc[f][1] = acc[f][2] = acc[f][3] = 0.f;
        const float* a = C.af + tid;
#pragma unroll 2
        for (int n = 0; n < kMelWin; n += 4) {
            const float a0 = a[n * kMelLdc], a1 = a[(n + 1) * kMelLdc], a2 = a[(n + 2) * kMelLdc], a3 = a[(n + 3) * kMelLdc];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const float4 v = *(const float4*)(S.xs + f * kMelHop + n);
                acc[f][0] = fmaf(a0, v.x, acc[f][0]);
                acc[f][1] = fmaf(a1, v.y, acc[f][1]);
                acc[f][2] = fmaf(a2, v.z, acc[f][2]);
                acc[f][3] = fmaf(a3, v.w, acc[f][3]);
            }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) S.D[f][tid] = (acc[f][0] + acc[f][1]) + (acc[f][2] + acc[f][3]);
    }
    __syncthreads();
    for (int i = tid; i < NF * kMelBins; i += kThreads) {
        const int f = i / kMelBins, k = i - f * kMelBins;
        const float re = S.D[f][k], im = S.D[f][kMelBins + k];
        S.P[f][k] = fmaf(im, im, __fmul_rn(re, re));
    }
    __syncthreads();
    if (tid < NF * kMelFilters) {
        const int f = tid % NF, m = tid / NF;
        const float* w = C.fb + m * kMelBins;
        float acc = 0.f;
        for (int k = C.lo[m]; k <= C.hi[m]; ++k) acc = fmaf(w[k], S.P[f][k], acc);
        S.M[f][m] = acc;
    }
    __syncthreads();
}

// The same frames walked back: dB, transposed filterbank (m ascending), 2 re / 2 im, transposed DFT (four chains per sample, c ascending
// in each) into gt[f][400].  gs: g_spec of the clip [32][T]; frames at or past T get a zero gradient.  sp: optional dB output of the
// first nwrite frames
template <int NF>
__device__ __forceinline__ void mel_frames_back(const KwsMelConst& C, const float* __restrict__ gs, int T, int f0, MelLds& S,
                                                float (*gt)[kMelWin], float* __restrict__ sp, int nwrite) {
    const int tid = threadIdx.x;
    if (tid < NF * kMelFilters) {
        const int f = tid % NF, m = tid / NF, t = f0 + f;
        const float mel = S.M[f][m];
        float g = 0.f;
        if (t < T) {
            if (sp && f < nwrite) sp[(long)m * T + t] = power_db(mel);
            if (mel > 1e-10f) g = __fmul_rn(gs[(long)m * T + t], kDbBack) / mel;
        }
        S.M[f][m] = g;
    }
    __syncthreads();
    for (int i = tid; i < NF * kMelBins; i += kThreads) {
        const int f = i / kMelBins, k = i - f * kMelBins;
        const int m0 = C.m0[k], m1 = m0 + 1 < kMelFilters ? m0 + 1 : m0;
        const float gp = fmaf(C.w1[k], S.M[f][m1], __fmul_rn(C.w0[k], S.M[f][m0]));
        const float re = S.D[f][k], im = S.D[f][kMelBins + k];
        S.D[f][k] = __fmul_rn(__fmul_rn(2.f, re), gp);
        S.D[f][kMelBins + k] = __fmul_rn(__fmul_rn(2.f, im), gp);
    }
    __syncthreads();
    if (tid < kMelWin) {
        float acc[NF][4];                              // chain j takes the rows c = j (mod 4), ascending; joined (0 + 1) + (2 + 3)
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f][0] = acc[f][1] = acc[f][2] = acc[f][3] = 0.f;
        const float* a = C.ab + tid;
#pragma unroll 2
        for (int c = 0; c < kMelCols - 2; c += 4) {
            const float a0 = a[c * kMelWin], a1 = a[(c + 1) * kMelWin], a2 = a[(c + 2) * kMelWin], a3 = a[(c + 3) * kMelWin];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const float4 v = *(const float4*)(&S.D[f][c]);
                acc[f][0] = fmaf(a0, v.x, acc[f][0]);
                acc[f][1] = fmaf(a1, v.y, acc[f][1]);
                acc[f][2] = fmaf(a2, v.z, acc[f][2]);
                acc[f][3] = fmaf(a3, v.w, acc[f][3]);
            }
        }
        const float t0 = a[(kMelCols - 2) * kMelWin], t1 = a[(kMelCols - 1) * kMelWin];       // rows 400 and 401
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            acc[f][0] = fmaf(t0, S.D[f][kMelCols - 2], acc[f][0]);
            acc[f][1] = fmaf(t1, S.D[f][kMelCols - 1], acc[f][1]);
            gt[f][tid] = (acc[f][0] + acc[f][1]) + (acc[f][2] + acc[f][3]);
        }
    }
    __syncthreads();
}

// grid: (tile, clip) flattened, tile fastest.  steps = 0: tile = kMelTile frames; steps > 0: tile j = frames 16 j .. 16 j + 4
__global__ __launch_bounds__(kThreads) void kws_mel_kernel(const KwsMelConst C, const float* __restrict__ x, int L, int T, int tiles,
                                                           int steps, float* __restrict__ out, int to_db) {
    __shared__ MelLds S;
    const int tile = blockIdx.x % tiles;
    const long b = blockIdx.x / tiles;
    const float* xr = x + b * L;
    int f0, nf;
    if (steps) {
        f0 = kKwsStep * tile;
        nf = kKwsRead;
        mel_frames<kKwsRead>(C, xr, L, f0, S);
    } else {
        f0 = kMelTile * tile;
        nf = T - f0 < kMelTile ? T - f0 : kMelTile;
        mel_frames<kMelTile>(C, xr, L, f0, S);
    }
    float* o = out + b * kMelFilters * T;
    for (int i = threadIdx.x; i < nf * kMelFilters; i += kThreads) {
        const int f = i % nf, m = i / nf;
        const float v = S.M[f][m];
        o[(long)m * T + f0 + f] = to_db ? power_db(v) : v;
    }
}

// A workgroup owns the output samples [s0, s1) of one clip and computes the time-domain gradient gt of every frame they need: the
// frames under them plus one halo frame, and frame T - 1 on its own pass where the right reflection folds it onto them from outside.
// g_x[s] = G[s + 200] + G[200 - s] (1 <= s <= 200) + G[2 (L - 1) - s + 200] (where that padded sample exists), in that order, with
// G[p] = gt[p / 200 - 1][p % 200 + 200] + gt[p / 200][p % 200]: frames ascending, direct before folded
__global__ __launch_bounds__(kThreads) void kws_mel_vjp_kernel(const KwsMelConst C, const float* __restrict__ x,
                                                               const float* __restrict__ g_spec, int L, int T, int tiles, int steps,
                                                               float* __restrict__ g_x, float* __restrict__ spec) {
    __shared__ MelLds S;
    __shared__ float gt[kMelTile + 1][kMelWin];
    const int tid = threadIdx.x, tile = blockIdx.x % tiles;
    const long b = blockIdx.x / tiles;
    const float* xr = x + b * L;
    const float* gs = g_spec + b * kMelFilters * T;
    float* sp = spec ? spec + b * kMelFilters * T : nullptr;
    int fm0, nmain;
    long s0, s1;
    if (steps) {
        fm0 = kKwsStep * tile;
        nmain = kKwsRead;
        s0 = tile ? (long)(kKwsStep * tile - 1) * kMelHop : 0;
        s1 = tile == tiles - 1 ? L : (long)(kKwsStep * tile + kKwsStep - 1) * kMelHop;
        mel_frames<kKwsRead>(C, xr, L, fm0, S);
        mel_frames_back<kKwsRead>(C, gs, T, fm0, S, gt, sp, kKwsRead);
    } else {
        fm0 = kOwn * tile;
        nmain = kMelTile;
        s0 = (long)fm0 * kMelHop;
        s1 = s0 + kOwn * kMelHop;
        mel_frames<kMelTile>(C, xr, L, fm0, S);
        mel_frames_back<kMelTile>(C, gs, T, fm0, S, gt, sp, kOwn);        // the halo frame's dB is the next workgroup's to write
    }
    if (s1 > L) s1 = L;
    // frame T - 1 from outside: some owned sample is a target of the right fold (s <= L - 2 and 2 (L - 1) - s < 200 T)
    const int fl = T - 1;
    const bool last_read = !steps || (fl % kKwsStep < kKwsRead && fl / kKwsStep < steps);
    const long r0 = 2l * (L - 1) - (long)kMelHop * T + 1 > s0 ? 2l * (L - 1) - (long)kMelHop * T + 1 : s0;
    const long r1 = L - 2 < s1 - 1 ? L - 2 : s1 - 1;
    const bool special = last_read && !(fl >= fm0 && fl < fm0 + nmain) && r0 <= r1;      // uniform over the workgroup
    if (special) {
        mel_frames<1>(C, xr, L, fl, S);
        mel_frames_back<1>(C, gs, T, fl, S, gt + kMelTile, nullptr, 0);
    }
    auto slot = [&](int f) -> int {
        if (f < 0 || f >= T) return -1;
        if (f >= fm0 && f < fm0 + nmain) return f - fm0;
        return (special && f == fl) ? kMelTile : -1;
    };
    auto G = [&](long p) -> float {
        const int u = (int)(p / kMelHop), n = (int)(p - (long)u * kMelHop);
        const int sl = slot(u - 1), sh = slot(u);
        const float lo = sl >= 0 ? gt[sl][n + kMelHop] : 0.f;
        const float hi = sh >= 0 ? gt[sh][n] : 0.f;
        return lo + hi;
    };
    float* gx = g_x + b * L;
    for (long s = s0 + tid; s < s1; s += kThreads) {
        float v = G(s + kMelHop);
        if (s >= 1 && s <= kMelHop) v += G(kMelHop - s);
        const long q = 2l * (L - 1) - s;
        if (s <= L - 2 && q < (long)kMelHop * T) v += G(q + kMelHop);
        gx[s] = v;
    }
}

}  // namespace

const char* kws_mel_host_constants(KwsMelHost* h) {
    const double two_pi = 2.0 * M_PI;
    h->af.assign((size_t)kMelWin * kMelLdc, 0.f);
    h->ab.assign((size_t)kMelCols * kMelWin, 0.f);
    for (int k = 0; k < kMelBins; ++k)
        for (int n = 0; n < kMelWin; ++n) {
            const double win = 0.5 - 0.5 * cos(two_pi * n / kMelWin);          // periodic Hann
            const double ang = two_pi * (double)(((long)k * n) % kMelWin) / kMelWin;   // exact argument reduction
            const float c = (float)(win * cos(ang)), s = (float)(-win * sin(ang));
            h->af[(size_t)n * kMelLdc + k] = c;
            h->af[(size_t)n * kMelLdc + kMelBins + k] = s;
            h->ab[(size_t)k * kMelWin + n] = c;
            h->ab[(size_t)(kMelBins + k) * kMelWin + n] = s;
        }
    // htk scale, no norm: 34 points equally spaced in mel between 0 and 8000 Hz, bins at linspace(0, 8000, 201)
    double pts[kMelFilters + 2];
    const double mel_max = 2595.0 * log10(1.0 + 8000.0 / 700.0);
    for (int i = 0; i < kMelFilters + 2; ++i) pts[i] = 700.0 * (pow(10.0, (mel_max * i / (kMelFilters + 1)) / 2595.0) - 1.0);
    h->fb.assign((size_t)kMelFilters * kMelBins, 0.f);
    h->w0.assign(kMelBins, 0.f);
    h->w1.assign(kMelBins, 0.f);
    h->m0.assign(kMelBins, 0);
    h->lo.assign(kMelFilters, kMelBins);
    h->hi.assign(kMelFilters, -1);
    std::vector<int> count(kMelBins, 0);
    for (int m = 0; m < kMelFilters; ++m)
        for (int k = 0; k < kMelBins; ++k) {
            const double f = 8000.0 * k / (kMelBins - 1);
            const double down = (f - pts[m]) / (pts[m + 1] - pts[m]), up = (pts[m + 2] - f) / (pts[m + 2] - pts[m + 1]);
            const float v = (float)fmax(0.0, fmin(down, up));
            h->fb[(size_t)m * kMelBins + k] = v;
            if (v == 0.f) continue;
            if (k < h->lo[m]) h->lo[m] = k;
            h->hi[m] = k;
            if (count[k] == 0) { h->m0[k] = m; h->w0[k] = v; }
            else if (count[k] == 1 && m == h->m0[k] + 1) h->w1[k] = v;
            else return "a bin of the htk filterbank feeds more than two (consecutive) filters";
            ++count[k];
        }
    for (int m = 0; m < kMelFilters; ++m) {
        if (h->hi[m] < h->lo[m]) return "the htk filterbank has an empty filter";
        for (int k = h->lo[m]; k <= h->hi[m]; ++k)
            if (h->fb[(size_t)m * kMelBins + k] == 0.f) return "a filter of the htk filterbank has a gap";
    }
    return nullptr;
}

void launch_kws_mel(const KwsMelConst& c, const float* x, int B, int L, int steps, float* out, int to_db, hipStream_t s) {
    const int T = 1 + L / kMelHop;
    const int tiles = steps ? steps : (T + kMelTile - 1) / kMelTile;
    hipLaunchKernelGGL(kws_mel_kernel, dim3((unsigned)((long)tiles * B)), dim3(kThreads), 0, s, c, x, L, T, tiles, steps, out, to_db);
}

void launch_kws_mel_vjp(const KwsMelConst& c, const float* x, const float* g_spec, int B, int L, int steps, float* g_x, float* spec,
                        hipStream_t s) {
    const int T = 1 + L / kMelHop;
    // all frames: a workgroup owns kOwn blocks of 200 output samples, and dB frames t < T are written by the owner of block t, so the
    // tiles cover block T - 1 even where L ends before it
    const int tiles = steps ? steps : (T + kOwn - 1) / kOwn;
    hipLaunchKernelGGL(kws_mel_vjp_kernel, dim3((unsigned)((long)tiles * B)), dim3(kThreads), 0, s, c, x, g_spec, L, T, tiles, steps, g_x,
                       spec);
}

}  // namespace dmad
