// Small HBM-bound kernels of the path: noise + scale (Philox), step-embedding MLP, scheduler
// updates, fp32-mode gate/update, mel post-processing, VGG helpers, arg-max votes.
#include "elementwise.h"
#include "philox.h"

namespace dmad {

__global__ void philox_raw_kernel(uint64_t seed, uint64_t sample, uint32_t stream, uint32_t nblocks, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblocks) return;
    uint32_t c[4] = {i, (uint32_t)sample, (uint32_t)(sample >> 32), stream};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    out[4 * i + 0] = c[0]; out[4 * i + 1] = c[1]; out[4 * i + 2] = c[2]; out[4 * i + 3] = c[3];
}

// z[b][l] ~ N(0,1), sample index = sample0 + b, or idx[b] when an index list is given (the recheck passes)
__global__ void philox_normal_kernel(uint64_t seed, uint64_t sample0, uint32_t stream, float* z, int B, int L, const long long* __restrict__ idx) {
    const int per = L / 4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * per) return;
    const int b = (int)(i / per), blk = (int)(i - (long)b * per);
    float v[4];
    philox_normal4(seed, idx ? (uint64_t)idx[b] : sample0 + b, stream, blk, v);
    *(float4*)(z + (long)b * L + blk * 4) = float4{v[0], v[1], v[2], v[3]};
}

// certified_robust.py:46-54:  x_in = x.repeat(B) + delta ; x_in = alpha_bar_star**0.5 * x_in
// delta = host noise [B][L] (parity mode) or sigma * Philox normal (fast mode)
__global__ void mc_noise_scale_kernel(const float* __restrict__ clip, const float* __restrict__ delta, float sigma,
                                      float scale, uint64_t seed, uint64_t sample0, float* __restrict__ xt, int B, int L) {
    const int per = L / 4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * per) return;
    const int b = (int)(i / per), blk = (int)(i - (long)b * per);
    const float4 x = *(const float4*)(clip + blk * 4);
    float d[4];
    if (delta) {
        const float4 dv = *(const float4*)(delta + (long)b * L + blk * 4);
        d[0] = dv.x; d[1] = dv.y; d[2] = dv.z; d[3] = dv.w;
    } else {
        philox_normal4(seed, sample0 + b, 0u, blk, d);
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = __fmul_rn(sigma, d[j]);
    }
    float4 o;
    o.x = __fmul_rn(scale, __fadd_rn(x.x, d[0])); o.y = __fmul_rn(scale, __fadd_rn(x.y, d[1]));
    o.z = __fmul_rn(scale, __fadd_rn(x.z, d[2])); o.w = __fmul_rn(scale, __fadd_rn(x.w, d[3]));
    *(float4*)(xt + (long)b * L + blk * 4) = o;
}

// The same sample, addressed through an index list (exact-vote recheck): row b is global sample idx[b]; its noise is
// the Philox draw keyed (seed, idx[b]) or row idx[b] - sample0 of the caller's delta — bit-identical to what the sample
// received in its first (bf16) evaluation.
__global__ void mc_noise_scale_idx_kernel(const float* __restrict__ clip, const float* __restrict__ delta, float sigma,
                                          float scale, uint64_t seed, uint64_t sample0, const long long* __restrict__ idx,
                                          float* __restrict__ xt, int B, int L) {
    const int per = L / 4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * per) return;
    const int b = (int)(i / per), blk = (int)(i - (long)b * per);
    const uint64_t sample = (uint64_t)idx[b];
    const float4 x = *(const float4*)(clip + blk * 4);
    float d[4];
    if (delta) {
        const float4 dv = *(const float4*)(delta + (long)(sample - sample0) * L + blk * 4);
        d[0] = dv.x; d[1] = dv.y; d[2] = dv.z; d[3] = dv.w;
    } else {
        philox_normal4(seed, sample, 0u, blk, d);
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = __fmul_rn(sigma, d[j]);
    }
    float4 o;
    o.x = __fmul_rn(scale, __fadd_rn(x.x, d[0])); o.y = __fmul_rn(scale, __fadd_rn(x.y, d[1]));
    o.z = __fmul_rn(scale, __fadd_rn(x.z, d[2])); o.w = __fmul_rn(scale, __fadd_rn(x.w, d[3]));
    *(float4*)(xt + (long)b * L + blk * 4) = o;
}

// dst[idx[b] - base][0:W] = src[b][0:W]  (rechecked rows of logits_out / x0_out); W % 4 == 0 or W < 4 handled scalar
__global__ void scatter_rows_kernel(const float* __restrict__ src, const long long* __restrict__ idx, long long base,
                                    float* __restrict__ dst, int B, int W) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * W) return;
    const int b = (int)(i / W), c = (int)(i - (long)b * W);
    dst[(idx[b] - base) * W + c] = src[i];
}

// out[i] = x[(row0 + i) % B]: rows [row0, row0 + nrows) of x.repeat(R, 1, 1)  (EOT's x_batch.repeat, _EOT.py:36)
__global__ void repeat_rows_kernel(const float* __restrict__ x, float* __restrict__ out, int B, long row0, int L, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const int per = L / 4;
    const long row = i / per;
    const int blk = (int)(i - row * per);
    ((float4*)out)[i] = ((const float4*)x)[((row0 + row) % B) * per + blk];
}

// ----------------------------------------------------------------------------------------------
// diffusion-step embedding (util.py:68-93) -> fc_t1, fc_t2 with swish (WaveNet.py:124-126) ->
// the 36 per-layer fc_t (WaveNet.py:82-83).  t is the same for every row of the batch in every
// inference caller, so the result is a [NL][256] bias table.  One block per layer.
// ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(512) embed_table_kernel(float t, const float* __restrict__ w1, const float* __restrict__ b1,
                                                          const float* __restrict__ w2, const float* __restrict__ b2,
                                                          const float* __restrict__ wt, const float* __restrict__ bt,
                                                          float* __restrict__ table, float* __restrict__ emb2_out,
                                                          const float* __restrict__ b_res, float* __restrict__ epi_c) {
    __shared__ float e0[128], e1[512], e2[512];
    const int tid = threadIdx.x, n = blockIdx.x;
    if (tid < 64) {
        const float f = expf((float)tid * -0.14619587892025687f);     // -ln(10000)/63 (util.py:88-89)
        const float v = t * f;
        e0[tid] = sinf(v);
        e0[64 + tid] = cosf(v);
    }
    __syncthreads();
    {
        float s = 0.f;
        for (int k = 0; k < 128; ++k) s = fmaf(w1[tid * 128 + k], e0[k], s);
        s += b1[tid];
        e1[tid] = s / (1.f + expf(-s));
    }
    __syncthreads();
    {
        float s = 0.f;
        for (int k = 0; k < 512; ++k) s = fmaf(w2[tid * 512 + k], e1[k], s);
        s += b2[tid];
        e2[tid] = s / (1.f + expf(-s));
    }
    __syncthreads();
    if (n == 0 && emb2_out) emb2_out[tid] = e2[tid];
    if (tid < 256) {
        const float* w = wt + ((long)n * 256 + tid) * 512;
        float s = 0.f;
        for (int k = 0; k < 512; ++k) s = fmaf(w[k], e2[k], s);
        const float v = s + bt[n * 256 + tid];
        table[n * 256 + tid] = v;
        // epilogue constant of layer n-1 (bf16 path): b_res_{n-1} * sqrt(1/2) + fc_t_n(emb)
        if (epi_c && n > 0) epi_c[(n - 1) * 256 + tid] = fmaf(b_res[(n - 1) * 256 + tid], 0.70710678118654752440f, v);
    }
}

// ----------------------------------------------------------------------------------------------
// scheduler updates (diffwave_ddpm.py); op order as in the reference, no FMA contraction
// ----------------------------------------------------------------------------------------------
__global__ void lincomb_kernel(int op, const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                               float c0, float c1, float c2, float* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r;
    switch (op) {
        case 0:  // one-shot x0 (l.199-203): c0 * x_t - c1 * eps
            r = __fsub_rn(__fmul_rn(c0, x[i]), __fmul_rn(c1, y[i])); break;
        case 1:  // diffusion (l.66-67): c0 * x0 + c1 * z
            r = __fadd_rn(__fmul_rn(c0, x[i]), __fmul_rn(c1, z[i])); break;
        case 2:  // reverse step (l.159-160,100): mu = (x - c0 * eps) / c1 ; x = mu + c2 * z
            r = __fdiv_rn(__fsub_rn(x[i], __fmul_rn(c0, y[i])), c1);
            if (z) r = __fadd_rn(r, __fmul_rn(c2, z[i]));
            break;
        default: r = 0.f;
    }
    out[i] = r;
}

// Reverse VP-SDE chain (dmad_vpsde_purify), one thread per 4 samples of a row; the N(0,1) draw stays in registers (Philox keyed
// (seed, sample0 + row, stream), the words of philox_normal_kernel) unless the caller passes z.
//   eps == nullptr: the initial diffusion       y = c0 * x + c1 * z                        (the rounding of lincomb op 1)
//   otherwise:      the Euler-Maruyama step     y = x + (c0 * x - c1 * eps) * h + c2 * z    (c2 == 0: no draw)
// y may alias x (each thread reads its elements before it writes them), so neither carries __restrict__; traj (optional)
// receives a second copy of y.
__global__ void vpsde_step_kernel(const float* x, const float* __restrict__ eps, const float* __restrict__ z, float c0, float c1, float h,
                                  float c2, uint64_t seed, uint64_t sample0, uint32_t stream, float* y, float* traj, int B, int L) {
    const int per = L / 4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * per) return;
    const int b = (int)(i / per), blk = (int)(i - (long)b * per);
    const long o = (long)b * L + blk * 4;
    const float4 xv = *(const float4*)(x + o);
    const float xa[4] = {xv.x, xv.y, xv.z, xv.w};
    const bool draw = eps == nullptr || c2 != 0.f;
    float za[4] = {0.f, 0.f, 0.f, 0.f};
    if (draw) {
        if (z) {
            const float4 zv = *(const float4*)(z + o);
            za[0] = zv.x; za[1] = zv.y; za[2] = zv.z; za[3] = zv.w;
        } else {
            philox_normal4(seed, sample0 + b, stream, blk, za);
        }
    }
    float r[4];
    if (!eps) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = __fadd_rn(__fmul_rn(c0, xa[j]), __fmul_rn(c1, za[j]));
    } else {
        const float4 ev = *(const float4*)(eps + o);
        const float ea[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = __fadd_rn(xa[j], __fmul_rn(__fsub_rn(__fmul_rn(c0, xa[j]), __fmul_rn(c1, ea[j])), h));
            if (draw) r[j] = __fadd_rn(r[j], __fmul_rn(c2, za[j]));
        }
    }
    const float4 out = float4{r[0], r[1], r[2], r[3]};
    *(float4*)(y + o) = out;
    if (traj) *(float4*)(traj + o) = out;
}

// ----------------------------------------------------------------------------------------------
// Any-length forms of the noise and scheduler kernels (the dmad_*_len exports): rows of `len` floats at a pitch of `len`, any
// len >= 1, so a row starts on a 16-byte boundary only where (row * len) % 4 == 0 and the base pointer allows it.  blockIdx.y walks
// the rows, one thread per Philox counter block (4 samples: block l / 4, the words of philox_normal_kernel) of its row.  A group is
// moved as one float4 where its address really is 16-byte aligned — a property of the row, so every wave of a row takes the same
// branch — and as scalars otherwise; the last group of a row holds len % 4 values (the leading words of its draw) and is the only
// partial one.  out may alias x (a thread reads its elements before it writes them).
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
__device__ __forceinline__ void load_group(const float* p, bool vec, int n, float v[4]) {
    if (vec) {
        const float4 t = *(const float4*)p;
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < n ? p[j] : 0.f;
    }
}
__device__ __forceinline__ void store_group(float* p, bool vec, int n, const float v[4]) {
    if (vec) {
        *(float4*)p = float4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) p[j] = v[j];
    }
}

__global__ void philox_normal_len_kernel(uint64_t seed, uint64_t sample0, uint32_t stream, float* __restrict__ z, int B, int len) {
    const int blk = blockIdx.x * blockDim.x + threadIdx.x;
    if ((long)blk * 4 >= len) return;
    const int n = len - blk * 4 < 4 ? len - blk * 4 : 4;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        float* p = z + (long)b * len + blk * 4;
        float v[4];
        philox_normal4(seed, sample0 + b, stream, blk, v);
        store_group(p, n == 4 && aligned16(p), n, v);
    }
}

// OP 1, the diffusion:   out = c0 * x + c1 * z                         (lincomb_kernel's op 1, the same roundings)
// OP 2, a reverse step:  out = (x - c0 * eps) / c1 [+ c2 * z if draw]  (lincomb_kernel's op 2)
// z == nullptr: the draw stays in registers, keyed (seed, sample0 + row, stream)
template <int OP>
__global__ void sched_len_kernel(const float* x, const float* __restrict__ eps, const float* __restrict__ z, float c0, float c1, float c2,
                                 int draw, uint64_t seed, uint64_t sample0, uint32_t stream, float* out, int B, int len) {
    const int blk = blockIdx.x * blockDim.x + threadIdx.x;
    if ((long)blk * 4 >= len) return;
    const int n = len - blk * 4 < 4 ? len - blk * 4 : 4;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const long o = (long)b * len + blk * 4;
        const bool vec = n == 4 && aligned16(x + o) && aligned16(out + o) && (OP == 1 || aligned16(eps + o)) && (!z || !draw || aligned16(z + o));
        float xa[4], ea[4] = {0.f, 0.f, 0.f, 0.f}, za[4] = {0.f, 0.f, 0.f, 0.f}, r[4];
        load_group(x + o, vec, n, xa);
        if (OP == 2) load_group(eps + o, vec, n, ea);
        if (draw) {
            if (z) load_group(z + o, vec, n, za);
            else philox_normal4(seed, sample0 + b, stream, blk, za);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (OP == 1) {
                r[j] = __fadd_rn(__fmul_rn(c0, xa[j]), __fmul_rn(c1, za[j]));
            } else {
                r[j] = __fdiv_rn(__fsub_rn(xa[j], __fmul_rn(c0, ea[j])), c1);
                if (draw) r[j] = __fadd_rn(r[j], __fmul_rn(c2, za[j]));
            }
        }
        store_group(out + o, vec, n, r);
    }
}

// zero `width4` float4 at offset `off4` of each of `rows` rows of `pitch4` float4: the band [kPad + len, kPad + dirty) of every clip of
// a zero-padded [..][LP][256 or 512] map (the padding invariant of the any-length exact-fp32 WaveNet path, dmad_api.hip)
__global__ void zero_band_kernel(float4* __restrict__ buf, long pitch4, long off4, long width4, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const long row = i / width4, c = i - row * width4;
    buf[row * pitch4 + off4 + c] = float4{0.f, 0.f, 0.f, 0.f};
}

// NES probes (dmad_nes_probes; robustness_eval/_NES.py:19-25), one thread per 4 samples of a query row.  Global row g = row0 + r is slot
// g % per_clip of clip g / per_clip (per_clip = 2H + with_origin): the optional slot 0 is x[b] itself, then H rows x[b] + sigma * u_j and
// H rows x[b] - sigma * u_j, with u_j the Philox row keyed (seed, draw0 + b * H + j, stream) — the words of philox_normal_kernel.  The
// product is rounded before the sum, as torch's `noise * sigma + x` rounds it, so the two probes of a pair are mirror images.
__global__ void nes_probes_kernel(const float* __restrict__ x, float sigma, int H, int with_origin, uint64_t seed, uint64_t draw0,
                                  uint32_t stream, long row0, int rows, float* __restrict__ out, int L) {
    const int per = L / 4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)rows * per) return;
    const int r = (int)(i / per), blk = (int)(i - (long)r * per);
    const long g = row0 + r;
    const int per_clip = 2 * H + with_origin;
    const long b = g / per_clip;
    const int slot = (int)(g - b * per_clip) - with_origin;        // -1: the unperturbed clip
    float4 v = *(const float4*)(x + b * L + blk * 4);
    if (slot >= 0) {
        const int j = slot < H ? slot : slot - H;
        const float sg = slot < H ? sigma : -sigma;
        float z[4];
        philox_normal4(seed, draw0 + (uint64_t)b * (uint64_t)H + (uint64_t)j, stream, blk, z);
        v.x = __fadd_rn(v.x, __fmul_rn(sg, z[0])); v.y = __fadd_rn(v.y, __fmul_rn(sg, z[1]));
        v.z = __fadd_rn(v.z, __fmul_rn(sg, z[2])); v.w = __fadd_rn(v.w, __fmul_rn(sg, z[3]));
    }
    *(float4*)(out + (long)r * L + blk * 4) = v;
}

// NES estimate (dmad_nes_grad; _NES.py:47,52,54): grad[b][l] = (accumulate ? grad[b][l] : 0) + scale * sum_j (w[b][j] - w[b][H + j]) u_{b,j}[l].
// One thread per 4 output samples regenerates the H directions of its clip in registers, in the keying of nes_probes_kernel, and sums
// them j ascending (product rounded, then added): no atomics, one store per output, the same bits for every batch size.
__global__ void nes_grad_kernel(const float* __restrict__ w, int H, float scale, uint64_t seed, uint64_t draw0, uint32_t stream,
                                int accumulate, float* __restrict__ grad, int B, int L) {
    const int per = L / 4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * per) return;
    const int b = (int)(i / per), blk = (int)(i - (long)b * per);
    const float* wb = w + (long)b * 2 * H;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < H; ++j) {
        const float d = __fsub_rn(wb[j], wb[H + j]);
        float z[4];
        philox_normal4(seed, draw0 + (uint64_t)b * (uint64_t)H + (uint64_t)j, stream, blk, z);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(d, z[k]));
    }
    float* o = grad + (long)b * L + blk * 4;
    float4 r = float4{__fmul_rn(scale, acc[0]), __fmul_rn(scale, acc[1]), __fmul_rn(scale, acc[2]), __fmul_rn(scale, acc[3])};
    if (accumulate) {
        const float4 g = *(const float4*)o;
        r.x = __fadd_rn(g.x, r.x); r.y = __fadd_rn(g.y, r.y); r.z = __fadd_rn(g.z, r.z); r.w = __fadd_rn(g.w, r.w);
    }
    *(float4*)o = r;
}

// ----------------------------------------------------------------------------------------------
// Particle swarm of SirenAttack (dmad_pso_*; robustness_eval/black_box_attack.py:344-498).  Row r = b * P + p of the [B * P][L] state
// arrays is particle p of clip b; its draws of one swarm event are the Philox rows keyed (seed, draw0 + r, DMAD_PHILOX_STREAM_PSO + k).
// One thread per 4 samples; every product, sum and difference is rounded on its own, so a row depends on its key and inputs only.
// ----------------------------------------------------------------------------------------------
// four uniforms in (0, 1) with 24 random bits each: the uniforms philox_normal4 feeds to Box-Muller
__device__ inline void philox_uniform4(uint64_t seed, uint64_t sample, uint32_t stream, uint32_t block, float u[4]) {
    uint32_t c[4] = {block, (uint32_t)sample, (uint32_t)(sample >> 32), stream};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = __fmul_rn(__fadd_rn((float)(c[k] >> 8), 0.5f), 5.9604644775390625e-8f);
}

__global__ void philox_uniform_kernel(uint64_t seed, uint64_t sample0, uint32_t stream, float* __restrict__ out, int B, int L) {
    const int per = L / 4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * per) return;
    const int b = (int)(i / per), blk = (int)(i - (long)b * per);
    float u[4];
    philox_uniform4(seed, sample0 + b, stream, blk, u);
    *(float4*)(out + (long)b * L + blk * 4) = float4{u[0], u[1], u[2], u[3]};
}

__device__ inline float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// black_box_attack.py:371-391,404: positions uniform in [lower, upper] (particle 0 of a clip = keep[b] when keep is given), velocities
// uniform in [-d, d] with d = |lower - upper|, loc = pbest_loc, queries = loc + x[b]
__global__ void pso_init_kernel(const float* __restrict__ x, const float* __restrict__ lower, const float* __restrict__ upper,
                                const float* __restrict__ keep, int P, uint64_t seed, uint64_t draw0, uint32_t stream,
                                float* __restrict__ pbest_loc, float* __restrict__ loc, float* __restrict__ vel,
                                float* __restrict__ queries, long rows, int L) {
    const int per = L / 4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * per) return;
    const long r = i / per, b = r / P;
    const int blk = (int)(i - r * per), p = (int)(r - b * P);
    const long ob = b * L + blk * 4, o = r * L + blk * 4;
    const float4 lo4 = *(const float4*)(lower + ob), up4 = *(const float4*)(upper + ob), x4 = *(const float4*)(x + ob);
    const float lo[4] = {lo4.x, lo4.y, lo4.z, lo4.w}, up[4] = {up4.x, up4.y, up4.z, up4.w}, xs[4] = {x4.x, x4.y, x4.z, x4.w};
    float pos[4], v[4], q[4], u[4];
    if (keep && p == 0) {
        const float4 k4 = *(const float4*)(keep + ob);
        pos[0] = k4.x; pos[1] = k4.y; pos[2] = k4.z; pos[3] = k4.w;
    } else {
        philox_uniform4(seed, draw0 + (uint64_t)r, stream + 0u, blk, u);
#pragma unroll
        for (int k = 0; k < 4; ++k) pos[k] = clampf(__fadd_rn(lo[k], __fmul_rn(__fsub_rn(up[k], lo[k]), u[k])), lo[k], up[k]);
    }
    philox_uniform4(seed, draw0 + (uint64_t)r, stream + 1u, blk, u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float d = fabsf(__fsub_rn(lo[k], up[k]));
        v[k] = __fadd_rn(-d, __fmul_rn(__fmul_rn(2.f, d), u[k]));
        q[k] = __fadd_rn(pos[k], xs[k]);
    }
    const float4 pos4 = float4{pos[0], pos[1], pos[2], pos[3]};
    *(float4*)(pbest_loc + o) = pos4;
    *(float4*)(loc + o) = pos4;
    *(float4*)(vel + o) = float4{v[0], v[1], v[2], v[3]};
    *(float4*)(queries + o) = float4{q[0], q[1], q[2], q[3]};
}

// black_box_attack.py:474-484,404: vel <- w vel + c1 r1 (pbest - loc) + c2 r2 (gbest[b] - loc), left to right; loc <- clamp(loc + vel);
// queries <- loc + x[b].  loc and vel are updated in place, each element by the thread that read it.
__global__ void pso_step_kernel(const float* __restrict__ x, const float* __restrict__ lower, const float* __restrict__ upper,
                                const float* __restrict__ pbest_loc, const float* __restrict__ gbest_loc, int P, float w, float c1, float c2,
                                uint64_t seed, uint64_t draw0, uint32_t stream, float* __restrict__ loc, float* __restrict__ vel,
                                float* __restrict__ queries, long rows, int L) {
    const int per = L / 4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * per) return;
    const long r = i / per, b = r / P;
    const int blk = (int)(i - r * per);
    const long ob = b * L + blk * 4, o = r * L + blk * 4;
    const float4 lo4 = *(const float4*)(lower + ob), up4 = *(const float4*)(upper + ob), x4 = *(const float4*)(x + ob);
    const float4 g4 = *(const float4*)(gbest_loc + ob), pb4 = *(const float4*)(pbest_loc + o);
    const float4 l4 = *(const float4*)(loc + o), v4 = *(const float4*)(vel + o);
    const float lo[4] = {lo4.x, lo4.y, lo4.z, lo4.w}, up[4] = {up4.x, up4.y, up4.z, up4.w}, xs[4] = {x4.x, x4.y, x4.z, x4.w};
    const float gb[4] = {g4.x, g4.y, g4.z, g4.w}, pb[4] = {pb4.x, pb4.y, pb4.z, pb4.w};
    float l[4] = {l4.x, l4.y, l4.z, l4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w}, q[4], u1[4], u2[4];
    philox_uniform4(seed, draw0 + (uint64_t)r, stream + 2u, blk, u1);
    philox_uniform4(seed, draw0 + (uint64_t)r, stream + 3u, blk, u2);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float r1 = __fadd_rn(u1[k], 1e-5f), r2 = __fadd_rn(u2[k], 1e-5f);
        const float t1 = __fmul_rn(__fmul_rn(c1, r1), __fsub_rn(pb[k], l[k]));
        const float t2 = __fmul_rn(__fmul_rn(c2, r2), __fsub_rn(gb[k], l[k]));
        v[k] = __fadd_rn(__fadd_rn(__fmul_rn(w, v[k]), t1), t2);
        l[k] = clampf(__fadd_rn(l[k], v[k]), lo[k], up[k]);
        q[k] = __fadd_rn(l[k], xs[k]);
    }
    *(float4*)(vel + o) = float4{v[0], v[1], v[2], v[3]};
    *(float4*)(loc + o) = float4{l[0], l[1], l[2], l[3]};
    *(float4*)(queries + o) = float4{q[0], q[1], q[2], q[3]};
}

// black_box_attack.py:420-437 in three passes that all decide from the scalars as they were before the call: (1) the personal-best
// rows, (2) the global-best rows, (3) the scalars.  A block serves one row, so its decision is one scalar read by thread 0.
__global__ void pso_pbest_rows_kernel(const float* __restrict__ loss, const float* __restrict__ pbests, const float* __restrict__ loc,
                                      float* __restrict__ pbest_loc, int bpr, int L) {
    const long r = blockIdx.x / bpr;
    const int t = (int)(blockIdx.x - r * bpr) * blockDim.x + threadIdx.x;
    if (t >= L / 4 || !(loss[r] < pbests[r])) return;
    *(float4*)(pbest_loc + r * L + t * 4) = *(const float4*)(loc + r * L + t * 4);
}

// first arg-min of the personal bests of clip b as they will be after the update, and its value
__device__ inline int pso_best_particle(const float* __restrict__ loss, const float* __restrict__ pbests, long b, int P, float* best) {
    int k = 0;
    float m = 0.f;
    for (int p = 0; p < P; ++p) {
        const float l = loss[b * P + p], pb = pbests[b * P + p];
        const float v = l < pb ? l : pb;
        if (p == 0 || v < m) { k = p; m = v; }
    }
    *best = m;
    return k;
}

__global__ void pso_gbest_rows_kernel(const float* __restrict__ loss, const float* __restrict__ pbests, const float* __restrict__ gbests,
                                      const long long* __restrict__ index, const float* __restrict__ pbest_loc,
                                      float* __restrict__ gbest_loc, int P, int bpr, int L) {
    __shared__ int sel;
    const long b = blockIdx.x / bpr;
    const long i = index ? (long)index[b] : b;
    if (threadIdx.x == 0) {
        float m;
        const int k = pso_best_particle(loss, pbests, b, P, &m);
        sel = m < gbests[i] ? k : -1;
    }
    __syncthreads();
    const int t = (int)(blockIdx.x - b * bpr) * blockDim.x + threadIdx.x;
    if (sel < 0 || t >= L / 4) return;
    *(float4*)(gbest_loc + i * L + t * 4) = *(const float4*)(pbest_loc + (b * P + sel) * L + t * 4);
}

__global__ void pso_best_scalars_kernel(const float* __restrict__ loss, const long long* __restrict__ predict,
                                        const long long* __restrict__ index, float* __restrict__ pbests, float* __restrict__ gbests,
                                        long long* __restrict__ gbest_predict, int B, int P) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const long i = index ? (long)index[b] : b;
    float m;
    const int k = pso_best_particle(loss, pbests, b, P, &m);
    for (int p = 0; p < P; ++p)
        if (loss[b * P + p] < pbests[b * P + p]) pbests[b * P + p] = loss[b * P + p];
    if (m < gbests[i]) {
        gbests[i] = m;
        gbest_predict[i] = predict[b * P + k];
    }
}

// ----------------------------------------------------------------------------------------------
// fp32 (parity) WaveNet helpers
// ----------------------------------------------------------------------------------------------
template <bool SPLIT>      // SPLIT: write the split-f16 storage format (dmad_common.h) for the x3 GEMM tier
__global__ void wn_init_f32_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                   const float* __restrict__ emb0, float* __restrict__ h, int L, int LP, long total, int hi_only) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;     // one float4 (4 channels) each
    if (idx >= total) return;
    const int c4 = (int)(idx & 63);
    const long pos = idx >> 6, bb = pos / L, t = pos - bb * L;
    const float xv = x[pos];
    float4 o;
    float* po = &o.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c4 * 4 + j;
        po[j] = __fadd_rn(relu_nan(__fadd_rn(__fmul_rn(w[c], xv), bias[c])), emb0[c]);
    }
    if (SPLIT) {
        u32x4_t v = split4(o.x, o.y, o.z, o.w);
        if (hi_only) { v[2] = 0u; v[3] = 0u; }      // error-attribution runs: the stored stream is f16 (GemmF32Args::diag bit 2)
        *(u32x4_t*)(h + ((bb * LP + kPad + t) * kC + c4 * 4)) = v;
    } else *(float4*)(h + ((bb * LP + kPad + t) * kC + c4 * 4)) = o;
}

template <bool SPLIT>
__global__ void scale_kernel(const float* __restrict__ x, float c, float* __restrict__ y, long n4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 v = ((const float4*)x)[i];
    v.x = __fmul_rn(v.x, c); v.y = __fmul_rn(v.y, c); v.z = __fmul_rn(v.z, c); v.w = __fmul_rn(v.w, c);
    if (SPLIT) ((u32x4_t*)y)[i] = split4(v.x, v.y, v.z, v.w);
    else ((float4*)y)[i] = v;
}

// eps[n] = w . f[n][:256] + b  (final_conv.2, WaveNet.py:160-162): one wave per position
__global__ void __launch_bounds__(256) dot256_kernel(const float* __restrict__ f, const float* __restrict__ w, float bias,
                                                     float* __restrict__ out, long N) {
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (n >= N) return;
    const float4 v = *(const float4*)(f + n * 256 + lane * 4);
    const float4 ww = *(const float4*)(w + lane * 4);
    float s = v.x * ww.x + v.y * ww.y + v.z * ww.z + v.w * ww.w;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[n] = s + bias;
}

// ----------------------------------------------------------------------------------------------
// mel front-end post-processing (torchaudio MelSpectrogram power=2 + AmplitudeToDB 'power')
// ----------------------------------------------------------------------------------------------
// xp[b][0:1024] = 0, xp[b][1024:1024+L] = x[b], xp[b][1024+L:] = 0       (center=True, constant pad)
__global__ void mel_pad_kernel(const float* __restrict__ x, float* __restrict__ xp, int L, int LPm, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long b = i / LPm;
    const int p = (int)(i - b * LPm) - 1024;
    xp[i] = (p >= 0 && p < L) ? x[b * L + p] : 0.f;
}

// The same padded rows for the Monte Carlo samples of ONE clip (certified_robust.py:34-67 with denoiser None): row b is
// clip + delta[b], or clip + sigma * the Philox normals of sample sample0 + b, the bits of mc_noise_scale_kernel at scale 1, written
// straight into the padded layout, so the noisy waveforms are never stored on their own.  One thread per float4: a Philox block is
// four consecutive samples and 1024, L and LPm are multiples of 4, so no float4 straddles a pad
__global__ void mel_pad_noise_kernel(const float* __restrict__ clip, const float* __restrict__ delta, float sigma, uint64_t seed,
                                     uint64_t sample0, float* __restrict__ xp, int L, int LPm, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const int per = LPm / 4;
    const long b = i / per;
    const int p = 4 * (int)(i - b * per) - 1024;
    float4 o{0.f, 0.f, 0.f, 0.f};
    if (p >= 0 && p < L)
        o = noisy4(*(const float4*)(clip + p), delta ? delta + b * L + p : nullptr, sigma, seed, sample0 + (uint64_t)b, (uint32_t)(p >> 2));
    *(float4*)(xp + 4 * i) = o;
}

// P[n][f] = re^2 + im^2, f < 1025 ; zero for the K padding up to ldp.  D is [n][ldd]: re at f, im at 1025 + f
__global__ void mel_power_kernel(const float* __restrict__ D, float* __restrict__ P, int ldd, int ldp, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long n = i / ldp;
    const int f = (int)(i - n * ldp);
    float v = 0.f;
    if (f < 1025) {
        const float re = D[n * ldd + f], im = D[n * ldd + 1025 + f];
        v = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
    }
    P[i] = v;
}

// spec[b][mel][frame] = 10 * log10(max(M[b*32 + frame][mel], 1e-10))
__global__ void mel_db_kernel(const float* __restrict__ M, float* __restrict__ spec, long total, int to_db) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long b = i >> 10;
    const int mel = (int)((i >> 5) & 31), fr = (int)(i & 31);
    if (!to_db) { spec[i] = M[(b * 32 + fr) * 32 + mel]; return; }     // MelSpectrogram alone: power, [b][mel][frame]
    const float v = clamp_min_nan(M[(b * 32 + fr) * 32 + mel], 1e-10f);
    // fp32 log10 rounded from a double evaluation (10*log10(1e-10f) must be exactly -100 like on the CPU)
    spec[i] = __fmul_rn(10.f, (float)log10((double)v));
}

// ----------------------------------------------------------------------------------------------
// VGG helpers
// ----------------------------------------------------------------------------------------------
// first conv (Cin = 1) + folded BN + relu: in [B][32][32] -> out NHWC [B][32][32][64]
__global__ void vgg_conv1_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ scale,
                                 const float* __restrict__ shift, float* __restrict__ out, long total, h16_t* __restrict__ out16) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // one (b, y, x, co) each
    if (i >= total) return;
    const int co = (int)(i & 63);
    const long p = i >> 6, b = p >> 10;
    const int y = (int)((p >> 5) & 31), x = (int)(p & 31);
    float s = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y + ky - 1, xx = x + kx - 1;
            if ((unsigned)yy < 32u && (unsigned)xx < 32u) s = fmaf(w[co * 9 + ky * 3 + kx], in[(b << 10) + yy * 32 + xx], s);
        }
    const float v = relu_nan(s * scale[co] + shift[co]);
    if (out) out[i] = v;
    if (out16) { const _Float16 hv = (_Float16)v; out16[i] = __builtin_bit_cast(unsigned short, hv); }     // f16 twin (the classifier's 16-bit tier)
}

// 2x2 max pool, NHWC
__global__ void maxpool2_nhwc_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // one float4 of output
    if (i >= total4) return;
    const int c4n = C >> 2, Ho = H >> 1, Wo = W >> 1;
    const int c4 = (int)(i % c4n);
    long p = i / c4n;
    const int xo = (int)(p % Wo); p /= Wo;
    const int yo = (int)(p % Ho);
    const long b = p / Ho;
    const float* s = in + (((b * H + 2 * yo) * W + 2 * xo) * (long)C) + c4 * 4;
    const float4 a = *(const float4*)s, bq = *(const float4*)(s + C), c = *(const float4*)(s + (long)W * C),
                 d = *(const float4*)(s + (long)W * C + C);
    float4 o;
    o.x = max_nan(max_nan(a.x, bq.x), max_nan(c.x, d.x)); o.y = max_nan(max_nan(a.y, bq.y), max_nan(c.y, d.y));
    o.z = max_nan(max_nan(a.z, bq.z), max_nan(c.z, d.z)); o.w = max_nan(max_nan(a.w, bq.w), max_nan(c.w, d.w));
    ((float4*)out)[i] = o;
}

// global average pool over the HW pixels of an NHWC map (F.avg_pool2d(x, 8, 1) on the 8x8 map of ResNeXt29,
// models/resnext.py:139): pixels summed in index order, then one division
__global__ void avgpool_nhwc_kernel(const float* __restrict__ in, float* __restrict__ out, int HW, int C, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // one output element [b][c]
    if (i >= total) return;
    const long b = i / C;
    const int c = (int)(i - b * C);
    const float* s = in + b * HW * (long)C + c;
    float acc = 0.f;
    for (int p = 0; p < HW; ++p) acc += s[(long)p * C];
    out[i] = acc / (float)HW;
}

// ----------------------------------------------------------------------------------------------
// votes: arg-max (first maximum wins, like torch.max) + per-class count (certified_robust.py:59-65)
// ----------------------------------------------------------------------------------------------
__global__ void vote_kernel(const float* __restrict__ logits, int B, int C, unsigned long long* __restrict__ counts,
                            int* __restrict__ pred_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int best = 0;
    float bv = logits[(long)b * C];
    for (int c = 1; c < C; ++c) {
        const float v = logits[(long)b * C + c];
        if (v > bv || (v != v && bv == bv)) { bv = v; best = c; }
    }
    if (pred_out) pred_out[b] = best;
    if (counts) atomicAdd(&counts[best], 1ull);
}

// Exact-vote mode: a sample votes from these (bf16-path) logits only if its top-2 margin is >= tau; otherwise its global
// index sample_base + b is queued for the exact-fp32 re-evaluation (any NaN fails the comparison and is queued too).
__global__ void vote_margin_kernel(const float* __restrict__ logits, int B, int C, unsigned long long* __restrict__ counts,
                                   float tau, long long sample_base, const long long* __restrict__ idx, long long* __restrict__ list,
                                   unsigned long long* __restrict__ list_n, long long list_cap, int* __restrict__ pred_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int best = 0;
    float bv = logits[(long)b * C], second = -INFINITY;
    bool nan = bv != bv;
    for (int c = 1; c < C; ++c) {
        const float v = logits[(long)b * C + c];
        nan |= v != v;
        if (v > bv) { second = bv; bv = v; best = c; }
        else if (v > second) second = v;
    }
    if (pred_out) pred_out[b] = best;
    if (!nan && (C == 1 || bv - second >= tau)) {
        atomicAdd(&counts[best], 1ull);
    } else {
        // the counter keeps counting past the capacity (the host reads it and reports the overflow); nothing is written there
        const unsigned long long slot = atomicAdd(list_n, 1ull);
        if (slot < (unsigned long long)list_cap) list[slot] = idx ? idx[b] : sample_base + b;     // row b is global sample idx[b] (a recheck pass) or sample_base + b
    }
}

// ---------------------------------------------------------------------------------------------- launchers
static inline unsigned nblk(long n, int bs) { return (unsigned)((n + bs - 1) / bs); }

void launch_philox_raw(uint64_t seed, uint64_t sample, uint32_t stream, uint32_t nblocks, uint32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(philox_raw_kernel, dim3(nblk(nblocks, 256)), dim3(256), 0, s, seed, sample, stream, nblocks, out);
}
void launch_philox_normal(uint64_t seed, uint64_t sample0, uint32_t stream, float* z, int B, int L, hipStream_t s, const long long* idx) {
    hipLaunchKernelGGL(philox_normal_kernel, dim3(nblk((long)B * (L / 4), 256)), dim3(256), 0, s, seed, sample0, stream, z, B, L, idx);
}
void launch_mc_noise_scale(const float* clip, const float* delta, float sigma, float scale, uint64_t seed, uint64_t sample0,
                           float* xt, int B, int L, hipStream_t s) {
    hipLaunchKernelGGL(mc_noise_scale_kernel, dim3(nblk((long)B * (L / 4), 256)), dim3(256), 0, s, clip, delta, sigma, scale,
                       seed, sample0, xt, B, L);
}
void launch_mc_noise_scale_idx(const float* clip, const float* delta, float sigma, float scale, uint64_t seed, uint64_t sample0,
                               const long long* idx, float* xt, int B, int L, hipStream_t s) {
    hipLaunchKernelGGL(mc_noise_scale_idx_kernel, dim3(nblk((long)B * (L / 4), 256)), dim3(256), 0, s, clip, delta, sigma, scale,
                       seed, sample0, idx, xt, B, L);
}
void launch_scatter_rows(const float* src, const long long* idx, long long base, float* dst, int B, int W, hipStream_t s) {
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(nblk((long)B * W, 256)), dim3(256), 0, s, src, idx, base, dst, B, W);
}
void launch_repeat_rows(const float* x, float* out, int B, long row0, int nrows, int L, hipStream_t s) {
    const long total4 = (long)nrows * (L / 4);
    hipLaunchKernelGGL(repeat_rows_kernel, dim3(nblk(total4, 256)), dim3(256), 0, s, x, out, B, row0, L, total4);
}
void launch_vote_margin(const float* logits, int B, int C, unsigned long long* counts, float tau, long long sample_base,
                        const long long* idx, long long* list, unsigned long long* list_n, long long list_cap, int* pred_out, hipStream_t s) {
    hipLaunchKernelGGL(vote_margin_kernel, dim3(nblk(B, 64)), dim3(64), 0, s, logits, B, C, counts, tau, sample_base, idx, list, list_n,
                       list_cap, pred_out);
}
void launch_embed_table(float t, const float* w1, const float* b1, const float* w2, const float* b2, const float* wt,
                        const float* bt, float* table, float* emb2_out, const float* b_res, float* epi_c, int NL, hipStream_t s) {
    hipLaunchKernelGGL(embed_table_kernel, dim3(NL), dim3(512), 0, s, t, w1, b1, w2, b2, wt, bt, table, emb2_out, b_res, epi_c);
}
void launch_lincomb(int op, const float* x, const float* y, const float* z, float c0, float c1, float c2, float* out, long n,
                    hipStream_t s) {
    hipLaunchKernelGGL(lincomb_kernel, dim3(nblk(n, 256)), dim3(256), 0, s, op, x, y, z, c0, c1, c2, out, n);
}
void launch_vpsde_step(const float* x, const float* eps, const float* z, float c0, float c1, float h, float c2, uint64_t seed,
                       uint64_t sample0, uint32_t stream, float* y, float* traj, int B, int L, hipStream_t s) {
    hipLaunchKernelGGL(vpsde_step_kernel, dim3(nblk((long)B * (L / 4), 256)), dim3(256), 0, s, x, eps, z, c0, c1, h, c2, seed, sample0, stream,
                       y, traj, B, L);
}
static inline dim3 len_grid(int B, int len) { return dim3(nblk((len + 3) / 4, 256), (unsigned)(B < 65535 ? B : 65535)); }
void launch_philox_normal_len(uint64_t seed, uint64_t sample0, uint32_t stream, float* z, int B, int len, hipStream_t s) {
    hipLaunchKernelGGL(philox_normal_len_kernel, len_grid(B, len), dim3(256), 0, s, seed, sample0, stream, z, B, len);
}
void launch_sched_len(int op, const float* x, const float* eps, const float* z, float c0, float c1, float c2, bool draw, uint64_t seed,
                      uint64_t sample0, uint32_t stream, float* out, int B, int len, hipStream_t s) {
    if (op == 1) hipLaunchKernelGGL(sched_len_kernel<1>, len_grid(B, len), dim3(256), 0, s, x, eps, z, c0, c1, c2, 1, seed, sample0, stream, out, B, len);
    else hipLaunchKernelGGL(sched_len_kernel<2>, len_grid(B, len), dim3(256), 0, s, x, eps, z, c0, c1, c2, draw ? 1 : 0, seed, sample0, stream, out, B, len);
}
void launch_zero_band(float* buf, long pitch, long off, long width, long rows, hipStream_t s) {
    const long total4 = rows * (width / 4);
    if (total4 > 0) hipLaunchKernelGGL(zero_band_kernel, dim3(nblk(total4, 256)), dim3(256), 0, s, (float4*)buf, pitch / 4, off / 4, width / 4, total4);
}
void launch_nes_probes(const float* x, float sigma, int H, int with_origin, uint64_t seed, uint64_t draw0, uint32_t stream, long row0,
                       int rows, float* out, int L, hipStream_t s) {
    hipLaunchKernelGGL(nes_probes_kernel, dim3(nblk((long)rows * (L / 4), 256)), dim3(256), 0, s, x, sigma, H, with_origin, seed, draw0,
                       stream, row0, rows, out, L);
}
void launch_nes_grad(const float* w, int H, float scale, uint64_t seed, uint64_t draw0, uint32_t stream, int accumulate, float* grad,
                     int B, int L, hipStream_t s) {
    hipLaunchKernelGGL(nes_grad_kernel, dim3(nblk((long)B * (L / 4), 256)), dim3(256), 0, s, w, H, scale, seed, draw0, stream, accumulate,
                       grad, B, L);
}
void launch_wn_init_f32(const float* x, const float* w, const float* bias, const float* emb0, float* h, int B, int L, int LP,
                        hipStream_t s, bool split, bool hi_only) {
    const long total = (long)B * L * 64;
    if (split) hipLaunchKernelGGL(wn_init_f32_kernel<true>, dim3(nblk(total, 256)), dim3(256), 0, s, x, w, bias, emb0, h, L, LP, total, hi_only ? 1 : 0);
    else hipLaunchKernelGGL(wn_init_f32_kernel<false>, dim3(nblk(total, 256)), dim3(256), 0, s, x, w, bias, emb0, h, L, LP, total, 0);
}
void launch_scale(const float* x, float c, float* y, long n, hipStream_t s, bool split) {
    if (split) hipLaunchKernelGGL(scale_kernel<true>, dim3(nblk(n / 4, 256)), dim3(256), 0, s, x, c, y, n / 4);
    else hipLaunchKernelGGL(scale_kernel<false>, dim3(nblk(n / 4, 256)), dim3(256), 0, s, x, c, y, n / 4);
}
void launch_dot256(const float* f, const float* w, float bias, float* out, long N, hipStream_t s) {
    hipLaunchKernelGGL(dot256_kernel, dim3(nblk(N, 4)), dim3(256), 0, s, f, w, bias, out, N);
}
void launch_mel_pad(const float* x, float* xp, int B, int L, int LPm, hipStream_t s) {
    const long total = (long)B * LPm;
    hipLaunchKernelGGL(mel_pad_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, x, xp, L, LPm, total);
}
void launch_mel_pad_noise(const float* clip, const float* delta, float sigma, uint64_t seed, uint64_t sample0, float* xp, int B, int L,
                          int LPm, hipStream_t s) {
    const long total4 = (long)B * (LPm / 4);
    hipLaunchKernelGGL(mel_pad_noise_kernel, dim3(nblk(total4, 256)), dim3(256), 0, s, clip, delta, sigma, seed, sample0, xp, L, LPm, total4);
}
void launch_mel_power(const float* D, float* P, int ldd, int ldp, long rows, hipStream_t s) {
    const long total = rows * ldp;
    hipLaunchKernelGGL(mel_power_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, D, P, ldd, ldp, total);
}
void launch_mel_db(const float* M, float* spec, int B, int to_db, hipStream_t s) {
    const long total = (long)B * 1024;
    hipLaunchKernelGGL(mel_db_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, M, spec, total, to_db);
}
// AmplitudeToDB(stype='power') on its own: y = 10 * log10(max(x, 1e-10))
__global__ void power_to_db_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = power_db(x[i]);
}
void launch_power_to_db(const float* x, float* y, long n, hipStream_t s) {
    hipLaunchKernelGGL(power_to_db_kernel, dim3(nblk(n, 256)), dim3(256), 0, s, x, y, n);
}
void launch_vgg_conv1(const float* in, const float* w, const float* scale, const float* shift, float* out, int B, hipStream_t s, h16_t* out16) {
    const long total = (long)B * 1024 * 64;
    hipLaunchKernelGGL(vgg_conv1_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, in, w, scale, shift, out, total, out16);
}
void launch_maxpool2_nhwc(const float* in, float* out, int B, int H, int W, int C, hipStream_t s) {
    const long total4 = (long)B * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(maxpool2_nhwc_kernel, dim3(nblk(total4, 256)), dim3(256), 0, s, in, out, H, W, C, total4);
}
void launch_avgpool_nhwc(const float* in, float* out, int B, int HW, int C, hipStream_t s) {
    const long total = (long)B * C;
    hipLaunchKernelGGL(avgpool_nhwc_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, in, out, HW, C, total);
}
void launch_vote(const float* logits, int B, int C, unsigned long long* counts, int* pred_out, hipStream_t s) {
    hipLaunchKernelGGL(vote_kernel, dim3(nblk(B, 64)), dim3(64), 0, s, logits, B, C, counts, pred_out);
}

// out[0:128] = v: a small host-computed vector travels as a kernel argument (copied at launch: no host buffer to keep alive,
// no stream synchronisation)
struct Vec128 { float v[128]; };
__global__ void store_vec128_kernel(Vec128 a, float* __restrict__ out) { out[threadIdx.x] = a.v[threadIdx.x]; }
void launch_store_vec128(const float* host128, float* out, hipStream_t s) {
    Vec128 a;
    for (int i = 0; i < 128; ++i) a.v[i] = host128[i];
    hipLaunchKernelGGL(store_vec128_kernel, dim3(1), dim3(128), 0, s, a, out);
}

void launch_philox_uniform(uint64_t seed, uint64_t sample0, uint32_t stream, float* out, int B, int L, hipStream_t s) {
    hipLaunchKernelGGL(philox_uniform_kernel, dim3(nblk((long)B * (L / 4), 256)), dim3(256), 0, s, seed, sample0, stream, out, B, L);
}
void launch_pso_init(const float* x, const float* lower, const float* upper, const float* keep, int B, int P, uint64_t seed, uint64_t draw0,
                     uint32_t stream, float* pbest_loc, float* loc, float* vel, float* queries, int L, hipStream_t s) {
    const long rows = (long)B * P;
    hipLaunchKernelGGL(pso_init_kernel, dim3(nblk(rows * (L / 4), 256)), dim3(256), 0, s, x, lower, upper, keep, P, seed, draw0, stream,
                       pbest_loc, loc, vel, queries, rows, L);
}
void launch_pso_step(const float* x, const float* lower, const float* upper, const float* pbest_loc, const float* gbest_loc, int B, int P,
                     float w, float c1, float c2, uint64_t seed, uint64_t draw0, uint32_t stream, float* loc, float* vel, float* queries,
                     int L, hipStream_t s) {
    const long rows = (long)B * P;
    hipLaunchKernelGGL(pso_step_kernel, dim3(nblk(rows * (L / 4), 256)), dim3(256), 0, s, x, lower, upper, pbest_loc, gbest_loc, P, w, c1, c2,
                       seed, draw0, stream, loc, vel, queries, rows, L);
}
void launch_pso_update_best(const float* loss, const long long* predict, const float* loc, const long long* index, int B, int P,
                            float* pbests, float* pbest_loc, float* gbests, float* gbest_loc, long long* gbest_predict, int L,
                            hipStream_t s) {
    const int bpr = (int)nblk(L / 4, 256);            // blocks per row
    hipLaunchKernelGGL(pso_pbest_rows_kernel, dim3((unsigned)((long)B * P * bpr)), dim3(256), 0, s, loss, pbests, loc, pbest_loc, bpr, L);
    hipLaunchKernelGGL(pso_gbest_rows_kernel, dim3((unsigned)((long)B * bpr)), dim3(256), 0, s, loss, pbests, gbests, index, pbest_loc,
                       gbest_loc, P, bpr, L);
    hipLaunchKernelGGL(pso_best_scalars_kernel, dim3(nblk(B, 64)), dim3(64), 0, s, loss, predict, index, pbests, gbests, gbest_predict, B, P);
}
void philox4x32_10_host(uint32_t c[4], uint32_t k0, uint32_t k1) { philox4x32_10(c, k0, k1); }

}  // namespace dmad
