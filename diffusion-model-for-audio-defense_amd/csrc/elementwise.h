// Launchers of the small kernels in elementwise.hip.
#pragma once
#include "dmad_common.h"

namespace dmad {

void launch_philox_raw(uint64_t seed, uint64_t sample, uint32_t stream, uint32_t nblocks, uint32_t* out, hipStream_t s);
void launch_philox_normal(uint64_t seed, uint64_t sample0, uint32_t stream, float* z, int B, int L, hipStream_t s,
                          const long long* idx = nullptr);      // idx != nullptr: row b is sample idx[b] instead of sample0 + b
void launch_mc_noise_scale(const float* clip, const float* delta, float sigma, float scale, uint64_t seed, uint64_t sample0,
                           float* xt, int B, int L, hipStream_t s);
void launch_mc_noise_scale_idx(const float* clip, const float* delta, float sigma, float scale, uint64_t seed, uint64_t sample0,
                               const long long* idx, float* xt, int B, int L, hipStream_t s);
void launch_scatter_rows(const float* src, const long long* idx, long long base, float* dst, int B, int W, hipStream_t s);
void launch_repeat_rows(const float* x, float* out, int B, long row0, int nrows, int L, hipStream_t s);
void launch_vote_margin(const float* logits, int B, int C, unsigned long long* counts, float tau, long long sample_base,
                        const long long* idx, long long* list, unsigned long long* list_n, long long list_cap, int* pred_out, hipStream_t s);
void launch_embed_table(float t, const float* w1, const float* b1, const float* w2, const float* b2, const float* wt,
                        const float* bt, float* table, float* emb2_out, const float* b_res, float* epi_c, int NL, hipStream_t s);
void launch_lincomb(int op, const float* x, const float* y, const float* z, float c0, float c1, float c2, float* out, long n,
                    hipStream_t s);
// reverse VP-SDE (dmad_vpsde_purify): eps == nullptr -> y = c0 x + c1 z; else y = x + (c0 x - c1 eps) h + c2 z; z == nullptr: Philox
// draw keyed (seed, sample0 + row, stream) in registers; y may alias x; traj (optional) gets a copy of y
void launch_vpsde_step(const float* x, const float* eps, const float* z, float c0, float c1, float h, float c2, uint64_t seed,
                       uint64_t sample0, uint32_t stream, float* y, float* traj, int B, int L, hipStream_t s);
// Any-length forms (dmad_*_len): rows of `len` floats at a pitch of `len` (any len >= 1, no alignment assumed).  philox_normal_len:
// row b = the first len values of launch_philox_normal's row of the same key.  sched_len: op 1 out = c0 x + c1 z (lincomb op 1),
// op 2 out = (x - c0 eps) / c1 + (draw ? c2 z : 0) (lincomb op 2); z == nullptr: the draw stays in registers; out may alias x.
void launch_philox_normal_len(uint64_t seed, uint64_t sample0, uint32_t stream, float* z, int B, int len, hipStream_t s);
void launch_sched_len(int op, const float* x, const float* eps, const float* z, float c0, float c1, float c2, bool draw, uint64_t seed,
                      uint64_t sample0, uint32_t stream, float* out, int B, int len, hipStream_t s);
// zero `width` floats at offset `off` of each of `rows` rows of `pitch` floats (all multiples of 4, buf 16-byte aligned)
void launch_zero_band(float* buf, long pitch, long off, long width, long rows, hipStream_t s);
// NES probes and estimate (dmad_nes_probes / dmad_nes_grad): direction j of clip b is the Philox row keyed (seed, draw0 + b * H + j, stream),
// regenerated in registers by both kernels.  probes: query rows [row0, row0 + rows) of the clip-major layout (2H + with_origin per clip);
// grad[b] = (accumulate ? grad[b] : 0) + scale * sum_j (w[b][j] - w[b][H + j]) u_{b,j}, w device fp32 [B][2H]
void launch_nes_probes(const float* x, float sigma, int H, int with_origin, uint64_t seed, uint64_t draw0, uint32_t stream, long row0,
                       int rows, float* out, int L, hipStream_t s);
void launch_nes_grad(const float* w, int H, float scale, uint64_t seed, uint64_t draw0, uint32_t stream, int accumulate, float* grad,
                     int B, int L, hipStream_t s);
// Particle swarm of SirenAttack (dmad_pso_init / dmad_pso_step / dmad_pso_update_best): row r = b * P + p of the [B * P][L] state arrays,
// its draws of one event keyed (seed, draw0 + r, stream + {0 position, 1 velocity, 2 r1, 3 r2}); out[b] of launch_philox_uniform is the
// uniform row of key (seed, sample0 + b, stream).  update_best decides everything from the scalars as they are before the call.
void launch_philox_uniform(uint64_t seed, uint64_t sample0, uint32_t stream, float* out, int B, int L, hipStream_t s);
void launch_pso_init(const float* x, const float* lower, const float* upper, const float* keep, int B, int P, uint64_t seed, uint64_t draw0,
                     uint32_t stream, float* pbest_loc, float* loc, float* vel, float* queries, int L, hipStream_t s);
void launch_pso_step(const float* x, const float* lower, const float* upper, const float* pbest_loc, const float* gbest_loc, int B, int P,
                     float w, float c1, float c2, uint64_t seed, uint64_t draw0, uint32_t stream, float* loc, float* vel, float* queries,
                     int L, hipStream_t s);
void launch_pso_update_best(const float* loss, const long long* predict, const float* loc, const long long* index, int B, int P,
                            float* pbests, float* pbest_loc, float* gbests, float* gbest_loc, long long* gbest_predict, int L,
                            hipStream_t s);
void launch_wn_init_f32(const float* x, const float* w, const float* bias, const float* emb0, float* h, int B, int L, int LP,
                        hipStream_t s, bool split = false, bool hi_only = false);
void launch_scale(const float* x, float c, float* y, long n, hipStream_t s, bool split = false);
void launch_dot256(const float* f, const float* w, float bias, float* out, long N, hipStream_t s);
void launch_mel_pad(const float* x, float* xp, int B, int L, int LPm, hipStream_t s);
// the padded rows of B Monte Carlo samples of one clip: clip + delta[b] (delta [B][L]), or clip + sigma * Philox normal of sample
// sample0 + b (delta == nullptr); clip and delta 16-byte aligned, L and LPm multiples of 4
void launch_mel_pad_noise(const float* clip, const float* delta, float sigma, uint64_t seed, uint64_t sample0, float* xp, int B, int L,
                          int LPm, hipStream_t s);
void launch_mel_power(const float* D, float* P, int ldd, int ldp, long rows, hipStream_t s);
void launch_mel_db(const float* M, float* spec, int B, int to_db, hipStream_t s);
void launch_power_to_db(const float* x, float* y, long n, hipStream_t s);
void launch_vgg_conv1(const float* in, const float* w, const float* scale, const float* shift, float* out, int B, hipStream_t s,
                      h16_t* out16 = nullptr);     // out / out16: fp32 map and / or its f16 twin (either may be null)
void launch_maxpool2_nhwc(const float* in, float* out, int B, int H, int W, int C, hipStream_t s);
void launch_avgpool_nhwc(const float* in, float* out, int B, int HW, int C, hipStream_t s);
void launch_vote(const float* logits, int B, int C, unsigned long long* counts, int* pred_out, hipStream_t s);
void launch_store_vec128(const float* host128, float* out, hipStream_t s);
void philox4x32_10_host(uint32_t c[4], uint32_t k0, uint32_t k1);

}  // namespace dmad
