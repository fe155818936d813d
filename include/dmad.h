/* dmad.h — C ABI of libdmad_hip.so, the MI355X (gfx950) engine behind the reference's Python
 * surfaces for the certified-smoothing hot path.
 *
 * The reference (cychomatica/Diffusion-Model-for-Audio-Defense) is 100 % Python on PyTorch and has
 * no FFI; the "plugin API" of this path is a set of Python call sites.  Each entry point below
 * names the reference call it replaces (paths relative to the reference repo root).  Device pointers
 * in, device pointers out, an explicit hipStream_t, no hidden allocation on the data path after
 * dmad_create() / dmad_finalize_weights() (the two diagnostic hooks at the end create HIP events), no torch types.  Every function returns 0 on success or a negative dmad_status; dmad_last_error()
 * gives the message (thread-local).  One engine per process per GPU; calls on one engine must come
 * from one thread at a time, and work given to one engine is ordered by the stream it is given on: an
 * engine owns ONE set of work buffers and per-step tables (activations, step embeddings, the recheck
 * queue), so two streams must not have calls on the same engine in flight together — switch streams
 * only after synchronising the previous one, or create one engine per stream.
 */
#ifndef DMAD_H
#define DMAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmad_engine dmad_engine;
typedef void* dmad_stream;      /* hipStream_t (torch.cuda.current_stream().cuda_stream) */

enum dmad_status {
    DMAD_OK = 0,
    DMAD_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
    DMAD_ERR_STATE = -2,        /* weights not finalised, batch larger than max_batch, ... */
    DMAD_ERR_HIP = -3,          /* a HIP runtime call failed */
    DMAD_ERR_SHAPE = -4         /* a weight set whose geometry no kernel serves (the M5 part, WideResNet, DenseNet); the message names the field */
};

enum dmad_precision {
    DMAD_BF16 = 0,              /* WaveNet on the 16-bit MFMA path alone (operands: dmad_half_type, fp32 accumulate); mel +
                                 * classifier fp32.  (The name is historical: the operand format is half_type's.) */
    DMAD_FP32 = 1,              /* everything on the exact-fp32 matrix path (parity mode) */
    DMAD_EXACT = 2              /* both WaveNet paths resident: the 16-bit path for throughput + re-evaluation, on the
                                 * split-f16 and exact-fp32 tiers, of every Monte Carlo sample whose 16-bit top-2 logit margin is
                                 * below the recheck bound, so that the vote counts of dmad_smooth_votes are the fp32 path's
                                 * up to the measured bound documented at dmad_set_mode (an empirical guarantee) */
};

/* Operand format of the 16-bit MFMA WaveNet path (DMAD_BF16 / DMAD_EXACT engines), fp32 accumulation either way. */
enum dmad_half_type {
    DMAD_HALF_BF16 = 0,         /* bfloat16: 8-bit significand (the format BASELINE.json's configuration names) */
    DMAD_HALF_F16 = 1           /* IEEE half: 11-bit significand, 8x smaller rounding error at the same MFMA rate; the
                                 * network's activations are O(1), far inside the half range */
};

/* Run-time mode of a DMAD_EXACT engine (the other two precisions have exactly one mode). */
enum dmad_mode {
    DMAD_MODE_FAST = 0,         /* 16-bit WaveNet, no recheck (what a DMAD_BF16 engine does) */
    DMAD_MODE_EXACT_VOTES = 1,  /* 16-bit WaveNet + margin-triggered recheck (split-f16 tier, then exact fp32) inside
                                 * dmad_smooth_votes; the waveform-returning entry points run the tier dmad_set_waveform_tier
                                 * selects (default: split-f16, fp32-grade) */
    DMAD_MODE_FP32 = 2          /* every WaveNet evaluation on the exact-fp32 path (what a DMAD_FP32 engine does) */
};

/* configs/config.json (wavenet_config + diffusion_config) as read by
 * diffusion_models/diffwave_ddpm.py:395-411 create_diffwave_model(). */
typedef struct dmad_config {
    int32_t struct_size;        /* sizeof(dmad_config) of the header the caller was built with: dmad_create refuses any
                                 * other value, so a caller of an older revision fails with a message instead of having
                                 * fields read past the end of its struct */
    int32_t res_channels;       /* 256 (the only supported value)       */
    int32_t skip_channels;      /* 256                                   */
    int32_t num_res_layers;     /* <= 64; 36 in the reference            */
    int32_t dilation_cycle;     /* <= 12 (max dilation 2048)             */
    int32_t embed_dim_in;       /* 128 */
    int32_t embed_dim_mid;      /* 512 */
    int32_t embed_dim_out;      /* 512 */
    int32_t clip_len;           /* 16000; must be a multiple of 128      */
    int32_t max_batch;          /* clips resident per pass               */
    int32_t num_classes;        /* 10  */
    int32_t precision;          /* enum dmad_precision                   */
    int32_t with_classifier;    /* 1: VGG19_bn + mel front-end buffers   */
    int32_t recheck_batch;      /* DMAD_EXACT: clips per pass of the recheck tiers (0 = 32; clamped to max_batch; the
                                 * Python engine and bench.py pass 64) */
    int32_t half_type;          /* enum dmad_half_type                   */
    int32_t with_wavenet;       /* 1: WaveNet workspace (residual streams, gate store: 330 MB per clip of max_batch on the
                                 * 16-bit path).  0: an engine for the spec-domain purifier / classifier only (BASELINE C5): no
                                 * WaveNet weights can be loaded, none of that memory is held */
} dmad_config;

int dmad_create(const dmad_config* cfg, dmad_engine** out);
void dmad_destroy(dmad_engine* e);
const char* dmad_last_error(void);
const char* dmad_version(void);
/* Non-fatal findings of the last dmad_finalize_weights() on this thread ("" if none): e.g. folded WaveNet weights that leave the
 * f16 normal range on an f16 engine (subnormals below 6.1e-5 lose significant bits, values above 65504 become inf). */
const char* dmad_last_warning(void);

/* Weights arrive as FOLDED fp32 host arrays (weight-norm and eval BatchNorm already folded by the
 * Python loader, exactly as the reference's modules compute them on every forward:
 * DiffWave_Unconditional/WaveNet.py:27-28,66-72; models/vgg.py:69-81).  Names:
 *   init.w[256] init.b[256]  fc_t1.w[512,128] fc_t1.b  fc_t2.w[512,512] fc_t2.b
 *   fc_t.{n}.w[256,512] fc_t.{n}.b   dil.{n}.w[512,256,3] dil.{n}.b   res.{n}.w[256,256] res.{n}.b
 *   skip.{n}.w[256,256] skip.{n}.b   f0.w[256,256] f0.b   f2.w[256] f2.b[1]
 *   vgg.conv{i}.w[cout,cin,3,3] vgg.conv{i}.scale[cout] vgg.conv{i}.shift[cout]  (i = 0..15)
 *   vgg.fc{j}.w[out,in] vgg.fc{j}.b   (j = 0..2)
 * or, instead of the vgg.* set, ResNeXt29 8x64d (models/resnext.py:23-142; bottleneck i = 3 * stage + k, i = 0..8):
 *   rx.conv1.w[64,1,3,3]  rx.b{i}.reduce.w[D,cin]  rx.b{i}.conv.w[D,D/8,3,3]  rx.b{i}.expand.w[cout,D]
 *   rx.b{i}.short.w[cout,cin] (where cin != cout), each with .scale[M] .shift[M];  rx.fc.w[classes,1024] rx.fc.b
 * or WideResNet-28-10 (models/wideresnet.py; block i = 4 * stage + k, i = 0..11; widths 16 / 160 / 320 / 640), recognised by wrn.conv1.w:
 *   wrn.conv1.w[16,1,3,3]  wrn.b{i}.bn1.scale[cin] .bn1.shift[cin] (the pre-activation on the residual stream)
 *   wrn.b{i}.conv1.w[cout,cin,3,3] .conv1.scale[cout] .conv1.shift[cout] (the folded bn2)  wrn.b{i}.conv2.w[cout,cout,3,3]
 *   wrn.b{i}.short.w[cout,cin] (where cin != cout)  wrn.bn.scale[640] wrn.bn.shift[640]  wrn.fc.w[classes,640] wrn.fc.b
 *   every shape is checked: DMAD_ERR_SHAPE for any other geometry, and the refused set is dropped.
 * or DenseNet-BC-100-12 (models/densenet.py; layer l = 16 * block + i, l = 0..47, cin = {24, 108, 150}[block] + 12 i), recognised by dn.conv1.w:
 *   dn.conv1.w[24,1,3,3]  dn.l{l}.bn1.scale[cin] .bn1.shift[cin]  dn.l{l}.conv1.w[48,cin] .conv1.scale[48] .conv1.shift[48] (the folded bn2)
 *   dn.l{l}.conv2.w[12,48,3,3]  dn.t{j}.bn.scale[cin] .bn.shift[cin] dn.t{j}.conv.w[cout,cin] (j = 0, 1: 216 -> 108, 300 -> 150)
 *   dn.bn.scale[342] dn.bn.shift[342]  dn.fc.w[classes,342] dn.fc.b;  checked and refused like the wrn.* set.
 * An engine holds one spectrogram classifier.
 * dmad_finalize_weights() packs whichever complete set (WaveNet, classifier) has been loaded and is not
 * packed yet into the MFMA/LDS layouts and uploads it; it may be called once per set. */
int dmad_load_weight(dmad_engine* e, const char* name, const float* host, const int64_t* shape, int32_t ndim);
int dmad_finalize_weights(dmad_engine* e);

/* eps = WaveNet((x_t, t * ones))  — DiffWave.model(...) at diffwave_ddpm.py:157-158,169-170,177-178
 * (WaveNet_Speech_Commands.forward, WaveNet.py:164-172).  x_t, eps: device fp32 [B][clip_len]. */
int dmad_wavenet_eps(dmad_engine* e, const float* x_t, int32_t t, int32_t B, float* eps, dmad_stream s);

/* x0_hat = c_a * x_t - c_b * eps(x_t, t)  — DiffWave.one_shot_denoise, diffwave_ddpm.py:174-182,195-205.
 * c_a = sqrt(1/Alpha_bar)[t], c_b = sqrt(1/Alpha_bar - 1)[t] are computed by the caller in fp32
 * exactly as the reference does (tables on the CPU, then indexed). */
int dmad_one_shot(dmad_engine* e, const float* x_t, int32_t t, float c_a, float c_b, int32_t B, float* x0, dmad_stream s);

/* One reverse step  x <- (x - c_eps * eps(x, t)) / c_div (+ c_sig * z)  — DiffWave.compute_coefficients
 * + the loop body of DiffWave._reverse, diffwave_ddpm.py:95-102,143-164.  z: device fp32 [B][L] noise
 * supplied by the caller, or NULL to draw Philox N(0,1) keyed (seed, sample0 + b, stream = 1 + t);
 * pass c_sig = 0 for the t == 0 step. */
int dmad_ddpm_step(dmad_engine* e, float* x, int32_t t, float c_eps, float c_div, float c_sig, const float* z,
                   uint64_t seed, uint64_t sample0, int32_t B, dmad_stream s);

/* x_t = c_a * x0 + c_b * z  — DiffWave._diffusion, diffwave_ddpm.py:49-73 (z as above, stream 0xD1FF). */
int dmad_diffuse(dmad_engine* e, const float* x0, float c_a, float c_b, const float* z, uint64_t seed,
                 uint64_t sample0, int32_t B, float* x_t, dmad_stream s);

/* spec = AmplitudeToDB('power')(MelSpectrogram(n_fft=2048, hop=512, n_mels=32, slaney)(x))
 * — the Wave2Spect transform built at certified_robustness_eval.py:85-87.  x: [B][clip_len],
 * spec: [B][32 mel][32 frames] fp32. */
int dmad_mel_db(dmad_engine* e, const float* x, int32_t B, float* spec, dmad_stream s);

/* The two stages of that transform on their own (for callers that keep torchaudio's two-module Compose):
 * mel = MelSpectrogram(...)(x): power mel spectrogram [B][32][32]; y = AmplitudeToDB('power')(x) elementwise. */
int dmad_mel_power(dmad_engine* e, const float* x, int32_t B, float* mel, dmad_stream s);
int dmad_power_to_db(dmad_engine* e, const float* x, int64_t n, float* y, dmad_stream s);

/* DiffWave.forward = _diffusion + _reverse in one call (diffwave_ddpm.py:36-104) with on-device Philox noise keyed
 * (seed, sample0 + row; stream 0xD1FF for the diffusion draw, 1 + t for reverse step t):
 *   x <- c_a * x0 + c_b * z;  for t = t_star-1 .. 0:  x <- (x - c_eps[t] * eps(x, t)) / c_div[t] (+ c_sig[t] * z_t, t > 0).
 * c_a = sqrt(Alpha_bar[t*-1]), c_b = sqrt(1 - Alpha_bar[t*-1]); c_eps / c_div / c_sig: HOST fp32 arrays of t_star
 * entries ((1 - Alpha[t]) / sqrt(1 - Alpha_bar[t]), sqrt(Alpha[t]), Sigma[t]), computed by the caller from the fp32
 * tables as the reference does.  x0, out: device fp32 [B][clip_len] (may alias). */
int dmad_ddpm_purify(dmad_engine* e, const float* x0, int32_t t_star, float c_a, float c_b, const float* c_eps, const float* c_div,
                     const float* c_sig, uint64_t seed, uint64_t sample0, int32_t B, float* out, dmad_stream s);

/* Improved-Diffusion UNet purifier on 1x32x32 mel spectrograms (the reference's configuration C5:
 * diffusion_models/improved_diffusion_ddpm.py:64-93 -> improved_diffusion/script_util.py:11-34,100-131).  Weights: the
 * reference's UNetModel state dict, names prefixed "un." (un.time_embed.0.weight, un.input_blocks.5.0.in_layers.2.weight,
 * ...), loaded with dmad_load_weight + dmad_finalize_weights like the other sets.
 * eps = UNetModel.forward(x_t, t * ones)  — improved_diffusion/unet.py:453-477.  x_t, eps: device fp32 [B][32][32]. */
int dmad_unet_eps(dmad_engine* e, const float* x_t, int32_t t, int32_t B, float* eps, dmad_stream s);

/* One GaussianDiffusion.p_sample step in place on x (gaussian_diffusion.py:232-257,331-387; epsilon prediction, fixed
 * variance, clip_denoised):  x0 = clamp(c_a * x - c_b * eps(x, t), -1, 1);  x <- c_1 * x0 + c_2 * x + c_sig * z.
 * c_a = sqrt_recip_alphas_cumprod[t], c_b = sqrt_recipm1_alphas_cumprod[t], c_1 / c_2 = posterior_mean_coef1/2[t],
 * c_sig = exp(0.5 * log_variance[t]) (0 at t == 0), all computed by the caller from the float64 tables.  z: device
 * fp32 [B][32][32] (the reference's randn_like draws) or NULL for on-device Philox noise keyed (seed, sample0 + row).
 * x0_out: optional [B][32][32] (pred_xstart). */
int dmad_unet_p_sample(dmad_engine* e, float* x, int32_t t, float c_a, float c_b, float c_1, float c_2, float c_sig, const float* z,
                       uint64_t seed, uint64_t sample0, int32_t B, float* x0_out, dmad_stream s);

/* logits = classifier(spec)  — VGG.forward, audio_models/ConvNets_SpeechCommands/models/vgg.py:48-52, or
 * CifarResNeXt.forward, models/resnext.py:133-142, whichever weight set was loaded.
 * spec: [B][32][32] fp32, logits: [B][num_classes] fp32. */
int dmad_classify(dmad_engine* e, const float* spec, int32_t B, float* logits, dmad_stream s);

/* The classifier's tiers.  Engines of precision DMAD_BF16 / DMAD_EXACT that hold ResNeXt29 — the default classifier of the
 * reference's certification script (certified_robustness_eval.py:57; models/resnext.py:23-142) — also hold a 16-BIT TIER of it:
 * every conv (1x1 reduce / expand / shortcut, the grouped 3x3) on f16 operands with fp32 accumulation, the eval-mode BatchNorm
 * scale folded into the f16 weights, shift / shortcut add / ReLU in fp32, maps kept as f16 between the convs; average pool and
 * the linear head stay fp32.  It is the classifier of DMAD_MODE_FAST (the vote loops' pass and the mode-default path of
 * dmad_eval_samples there).  Measured on the calibrated synthetic stand-in, its leader-difference error is 0.08-0.16 against
 * 0.016-0.030 for the f16 WaveNet in front of the fp32 classifier (profiles/r05b_resnext29_error_attribution.json) — a recheck bound
 * covering it would send a quarter of the samples to the recheck tiers — so since round 5 the first pass of the exact-vote mode runs
 * the classifier's SPLIT-F16 TIER instead (DMAD_EXACT engines): every conv on split-f16 operands (three f16 MFMAs per product, ~22
 * significant bits; BatchNorm scale / shift, shortcut add and ReLU in the fp32 epilogue), fp32-grade at a third of the fp32 tier's
 * time.  The split-f16 WaveNet recheck tier is paired with the same classifier tier (together 2.2e-4 from the all-fp32 logits, under
 * tau2 = 1e-3); the exact-fp32 recheck tier, dmad_query_logits and dmad_classify use the fp32 matrix cores, so a sample that reaches the
 * last tier carries the fp32 path's logits bit for bit.  dmad_classify_tier evaluates an explicit tier (0: fp32, 1: 16-bit, 2: split-f16; VGG19_bn has one tier and is
 * served on fp32 either way) — test / measurement hook. */
int dmad_classify_tier(dmad_engine* e, const float* spec, int32_t B, int32_t tier, float* logits, dmad_stream s);

/* The Monte Carlo loop of RobustCertificate.smooth_predict (+ forward, compute_t_star's result),
 * robustness_eval/certified_robust.py:17-31,33-67:  for samples i in [sample0, sample0 + n):
 *   x_in = sqrt(alpha_bar_star) * (clip + delta_i);  x0 = one_shot(x_in, t);  logits = classifier(mel_db(x0));
 *   counts[argmax logits] += 1.
 * clip: device fp32 [clip_len].  delta: device fp32 [n][clip_len] (the reference's CPU torch.normal
 * draws, parity mode) or NULL for on-device Philox noise keyed (seed, sample index).  counts: device
 * int64[num_classes], ACCUMULATED into (zero it first).  logits_out: optional [n][num_classes].
 * batch <= max_batch.  With with_classifier == 0, x0_out (optional, [n][clip_len]) receives the
 * purified clips and the caller classifies them. */
int dmad_smooth_votes(dmad_engine* e, const float* clip, float sigma, float sqrt_alpha_bar_star, int32_t t,
                      float c_a, float c_b, int64_t n, int32_t batch, uint64_t seed, uint64_t sample0,
                      const float* delta, int64_t* counts, float* logits_out, float* x0_out, dmad_stream s);

/* The same loop without a purifier, the plain randomized-smoothing baseline (certified_robust.py:34-67 with `denoiser is None`, the
 * driver's --defense_method randsmooth):  for samples i in [sample0, sample0 + n):
 *   x_in = clip + delta_i;  logits = classifier(mel_db(x_in));  counts[argmax logits] += 1     (the first maximum).
 * delta_i: row i of `delta` (device fp32 [n][clip_len], the reference's CPU torch.normal draws) or, delta == NULL, sigma * the Philox
 * normals keyed (seed, sample0 + i, stream 0, block l / 4): multiply, then add, each rounded (no FMA contraction), the bits of
 * x + sigma * dmad_philox_normal(...).  No sqrt(alpha_bar*) scaling: the reference applies it only when a denoiser is present.
 * The noisy rows are written straight into the mel front-end's padded layout; the noisy waveforms are not stored on their own.
 * The classifier runs its fp32 tier (dmad_classify's) on every engine precision and in every mode, so the counts are those of a host
 * loop over dmad_philox_normal / dmad_mel_db / dmad_classify / dmad_vote exactly, no recheck bound is involved, and WideResNet-28-10
 * and DenseNet-BC-100-12 are served in the exact-vote mode too.  Needs with_classifier and finalised classifier weights, not a WaveNet.
 * clip and delta 16-byte aligned.  counts: device int64[num_classes], ACCUMULATED into.  logits_out: optional [n][num_classes].
 * 1 <= batch <= max_batch: rows per pass; the result does not depend on it. */
int dmad_rs_smooth_votes(dmad_engine* e, const float* clip, float sigma, int64_t n, int32_t batch, uint64_t seed, uint64_t sample0,
                         const float* delta, int64_t* counts, float* logits_out, dmad_stream s);

/* DMAD_EXACT engines.  dmad_set_mode selects the dmad_mode (default DMAD_MODE_EXACT_VOTES).  dmad_set_recheck_margin sets
 * the bound tau: a sample whose 16-bit logits have (largest - second largest) < tau (or any NaN) does not vote from the 16-bit
 * logits; its global sample index is queued and the sample is re-evaluated from the SAME noise (Philox key (seed, index),
 * or its row of `delta`) on the higher tiers, and that result votes (and replaces its row of logits_out / x0_out).
 * With tau >= the largest error the 16-bit path makes on a logit DIFFERENCE AGAINST THE EXACT LEADER (E = max_j |e_j - e_i|,
 * e = 16-bit minus exact logits, i = the exact arg-max: a 16-bit leader j != i with margin >= tau would need e_j - e_i >= tau)
 * the counts equal the fp32 path's exactly (robustness_eval/certified_robust.py:59-65 is an arg-max: it only depends on the
 * order of the logits).  Defaults: 0.034 for f16 operands (measured E = 0.0244 over 36 864 samples), 0.30 for bf16 (0.207).
 *
 * The queued samples pass through two tiers.  Tier 2 is the fp32 pipeline on SPLIT-f16 operands: every fp32 value is kept
 * as hi = f16(x), lo = f16((x - hi) * 2^11) and every product is three f16 MFMAs (hi*hi + (hi*lo + lo*hi) * 2^-11, fp32
 * accumulate) — about 22 significant bits at several times the fp32 matrix rate.  It settles every queued sample whose
 * margin exceeds ITS error bound tau2 (dmad_set_recheck_margin2; default 1e-3, tau2 < 0 switches the tier off); the rest
 * (margins inside tau2) are evaluated on the exact-fp32 path, tier 3.  dmad_recheck_stats: samples voted, samples that
 * left the 16-bit pass, samples that reached the fp32 path.  dmad_wavenet_eps_path evaluates the eps-network on an
 * explicit path (0: the mode's default, 1: exact fp32, 2: split-f16) — test / measurement hook for the tiers. */
int dmad_set_mode(dmad_engine* e, int32_t mode);
/* Which WaveNet tier the WAVEFORM-returning entry points of a DMAD_EXACT engine run in DMAD_MODE_EXACT_VOTES — dmad_wavenet_eps,
 * dmad_one_shot, dmad_ddpm_step, dmad_ddpm_purify and the purifier inside dmad_query_logits (DiffWave.forward / one_shot_denoise /
 * compute_eps_t and AcousticSystem's query path, diffusion_models/diffwave_ddpm.py:36-47,166-182): 2 = the split-f16 tier (the DEFAULT:
 * eps within 8e-5 of the reference's, the fp32 tolerance class, at ~3.6 x the cost of the 16-bit path), 1 = exact fp32, 0 = the 16-bit
 * path (4e-3 with f16 operands).  Only the vote loop has a margin-triggered recheck, so these surfaces get their accuracy from the tier
 * itself.  DMAD_MODE_FAST / DMAD_MODE_FP32 keep their meaning (16-bit / fp32 everywhere); DMAD_BF16 / DMAD_FP32 engines have one path.
 * Tolerance delivered per surface: the vote counts of dmad_smooth_votes — exact (see below); its x0_out / logits_out rows — the tier the
 * row voted on; the entry points above — this setting. */
int dmad_set_waveform_tier(dmad_engine* e, int32_t tier);
int dmad_set_recheck_margin(dmad_engine* e, float tau);
int dmad_set_recheck_margin2(dmad_engine* e, float tau2);
int dmad_recheck_stats(dmad_engine* e, int64_t* samples, int64_t* rechecked, int64_t* rechecked_fp32, int32_t reset);
int dmad_wavenet_eps_path(dmad_engine* e, const float* x_t, int32_t t, int32_t B, int32_t path, float* eps, dmad_stream s);

/* Vector-Jacobian product of the eps-network on the exact-fp32 path — the gradient the white-box attack drivers take THROUGH the
 * DiffWave purifier (white_box_attack.py: loss.backward() through AcousticSystem; kws_adaptive_attack_eval.py:111).
 *
 * dmad_reserve_vjp reserves the VJP workspace for up to max_batch clips per pass: the saved residual streams h_n (step embedding
 * included) of every layer, NL x (L + 2 kPad) x 256 fp32 per clip (0.74 GB at the reference geometry, kPad = 2048), the zero-padded
 * gradient maps of the dilated conv input ((L + 2 kPad) x 512) and of the residual stream (3 x (L + 2 kPad) x 256), and the transposed
 * weight images (NL x 2.0 MB + 256 KB), packed on the device from the resident forward images.  max_batch is capped at the engine's
 * fp32 pass size (max_batch of a DMAD_FP32 engine, recheck_batch of a DMAD_EXACT one).  A larger reservation replaces a smaller one;
 * a smaller one keeps the present.  Counted by dmad_device_bytes.  This is the only allocation of the VJP: the data path below
 * allocates nothing.  DMAD_ERR_STATE for a DMAD_BF16 engine (it holds no fp32 weights) or before dmad_finalize_weights.
 * A failed reservation (out of memory) leaves no partial workspace behind: the pass-sized buffers it had allocated are released, the
 * packed weight images stay, and the next call packs only the missing ones.
 *
 * dmad_wavenet_eps_vjp:  g_x = (d eps / d x_t)^T g_eps  for eps = WaveNet((x_t, t * ones)) on the exact-fp32 path.
 * x_t, g_eps, g_x: device fp32 [B][clip_len].  eps: optional (NULL) device fp32 [B][clip_len], bit-identical to
 * dmad_wavenet_eps_path(.., path = 1, ..) (to dmad_wavenet_eps on a DMAD_FP32 engine).  DMAD_FP32 and DMAD_EXACT engines only;
 * B in [1, max_batch], processed in passes of the reservation's size.  Recompute scheme: a forward pass saves the residual streams
 * only; the backward recomputes each layer's dilated-conv output H inside the GEMM that applies the gate's derivative, so the
 * 512-channel H never reaches HBM.  Every reduction runs in a fixed order (no atomics, no split-K): g_x is bit-identical across
 * calls and independent of the batch a clip is in.  DMAD_ERR_STATE without a reservation. */
int dmad_reserve_vjp(dmad_engine* e, int32_t max_batch);
int dmad_wavenet_eps_vjp(dmad_engine* e, const float* x_t, int32_t t, int32_t B, const float* g_eps, float* g_x, float* eps,
                         dmad_stream s);

/* Clips of any length on the exact-fp32 DiffWave path (the keyword-spotting driver runs every clip at its own length, at batch 1).
 * Each export takes the arguments of its fixed-length twin with `len` after B: every waveform array is contiguous device fp32
 * [B][len], 1 <= len <= clip_len, at a pitch of len floats — rows are NOT 16-byte aligned when len % 4 != 0 and nothing assumes they
 * are.  Twins: dmad_wavenet_eps_len ~ dmad_wavenet_eps_path(.., path = 1, ..), dmad_wavenet_eps_vjp_len ~ dmad_wavenet_eps_vjp (the same
 * dmad_reserve_vjp reservation), dmad_philox_normal_len ~ dmad_philox_normal, dmad_diffuse_len / dmad_ddpm_step_len /
 * dmad_ddpm_purify_len ~ dmad_diffuse / dmad_ddpm_step / dmad_ddpm_purify.
 *   - They always run the exact-fp32 path, whatever the engine's mode: DMAD_FP32 and DMAD_EXACT engines; DMAD_ERR_STATE on a DMAD_BF16
 *     engine.  len < 1 or len > clip_len: DMAD_ERR_SHAPE.  B as in the twin.
 *   - len == clip_len makes the twin's launches: bit-identical results.  Same N = B * len, same launches: a clip's eps does not depend
 *     on the clip_len of the engine that ran it.
 *   - Noise is a prefix: a row of dmad_philox_normal_len is the first len values of dmad_philox_normal's row of the same (seed, sample,
 *     stream) — counter block l / 4, a last block of 1-3 values takes the leading words of its draw — and the draws the scheduler
 *     exports make in registers are those values (streams 0xD1FF and 1 + t, as the twins).  The scheduler arithmetic keeps the twins'
 *     operation order and roundings.
 *   - No allocation: they use the fp32 workspace and the VJP reservation as they stand (sized by clip_len); dmad_device_bytes is
 *     unchanged.  Before a call shorter than the longest one since, the engine zeroes rows [len, longest) of its zero-padded maps, so
 *     that the dilated taps past the clip's end read zeros; a run of calls at one length clears nothing. */
int dmad_wavenet_eps_len(dmad_engine* e, const float* x_t, int32_t t, int32_t B, int32_t len, float* eps, dmad_stream s);
int dmad_wavenet_eps_vjp_len(dmad_engine* e, const float* x_t, int32_t t, int32_t B, int32_t len, const float* g_eps, float* g_x, float* eps,
                             dmad_stream s);
int dmad_philox_normal_len(dmad_engine* e, uint64_t seed, uint64_t sample0, uint32_t stream, int32_t B, int32_t len, float* z, dmad_stream s);
int dmad_diffuse_len(dmad_engine* e, const float* x0, float c_a, float c_b, const float* z, uint64_t seed, uint64_t sample0, int32_t B,
                     int32_t len, float* x_t, dmad_stream s);
int dmad_ddpm_step_len(dmad_engine* e, float* x, int32_t t, float c_eps, float c_div, float c_sig, const float* z, uint64_t seed,
                       uint64_t sample0, int32_t B, int32_t len, dmad_stream s);
int dmad_ddpm_purify_len(dmad_engine* e, const float* x0, int32_t t_star, float c_a, float c_b, const float* c_eps, const float* c_div,
                         const float* c_sig, uint64_t seed, uint64_t sample0, int32_t B, int32_t len, float* out, dmad_stream s);

/* Vector-Jacobian product of the Improved-Diffusion UNet on its exact-fp32 tier — the gradient the white-box attack drivers take THROUGH
 * the spectrogram-domain purifier (AcousticSystem(.., defense_type='spec'); adaptive_attack_eval.py --defense Diffusion-Spec calls the
 * UNet outside no_grad, improved_diffusion_sde.py:90-118).
 *
 * dmad_reserve_unet_vjp reserves the workspace for up to max_batch spectrograms per pass: the TAPE of the forward — every module's output
 * map (so every module's input, both parts of a concatenated one), each ResBlock's conv1 output and each AttentionBlock's qkv, 5.89 M
 * floats (23.6 MB) per spectrogram, 1.51 GB at 64 —, the gradients of the 16 saved skip maps (3.3 MB), six work maps of 32 x 32 x 384
 * floats (9.4 MB) and, on the first reservation, the transposed weight images (3x3 convs tap-flipped with ci / co swapped, 1x1 layers
 * transposed; as large as the resident fp32 conv / 1x1 images), packed on the device from those.  max_batch is capped at the engine's fp32 pass size
 * (max_batch of a DMAD_FP32 engine, recheck_batch of a DMAD_EXACT one).  A larger reservation replaces a smaller one; a smaller one keeps
 * the present.  Counted by dmad_device_bytes.  This is the only allocation of the VJP: the data path below allocates nothing.
 * DMAD_ERR_STATE before the UNet weights are finalised, or for a DMAD_BF16 engine (the exact-fp32 UNet tier is a product path of
 * DMAD_FP32 and DMAD_EXACT engines only).
 * A failed reservation (out of memory) leaves no partial workspace behind: the pass-sized buffers it had allocated are released, the
 * packed weight images stay, and the next call packs only the missing ones.
 *
 * dmad_unet_eps_vjp:  g_x = (d eps / d x_t)^T g_eps  for eps = UNetModel(x_t, t * ones) on the exact-fp32 tier.  x_t, g_eps, g_x:
 * device fp32 [B][32][32].  eps: optional (NULL) device fp32 [B][32][32], bit-identical to dmad_unet_eps_tier(.., tier = 0, ..).  The input
 * gradient only: no weight gradients; the scale-shift rows depend on t alone, so nothing flows into the step embedding.  B in
 * [1, max_batch], processed in passes of the reservation's size.  Store scheme: the forward writes the tape, the backward walks the
 * modules in reverse — convs and 1x1 layers as the fp32 GEMM on the transposed images, GroupNorm (+ scale-shift + SiLU), attention,
 * stride-2 and upsampling backward as small kernels.  Every reduction runs in a fixed order (no atomics, no split-K): g_x is
 * bit-identical across calls and independent of the batch a spectrogram is in.  DMAD_ERR_STATE without a reservation. */
int dmad_reserve_unet_vjp(dmad_engine* e, int32_t max_batch);
int dmad_unet_eps_vjp(dmad_engine* e, const float* x_t, int32_t t, int32_t B, const float* g_eps, float* g_x, float* eps,
                      dmad_stream s);

/* Vector-Jacobian products of the classifier side — the last two stages of every gradient the white-box attack driver takes
 * (adaptive_attack_eval.py: AudioAttack's loss.backward() through AcousticSystem -> MelSpectrogram + AmplitudeToDB -> the classifier,
 * white_box_attack.py:356-376).  DESIGN §14.
 *
 * dmad_reserve_classifier_vjp reserves the ResNeXt29 VJP workspace for up to max_batch spectrograms per pass: the TAPE of the fp32
 * forward — conv1's output and, per bottleneck, its post-ReLU T1 (reduce) and T2 (grouped 3x3) and its block output Y, 8.13 M floats
 * (32.5 MB) per spectrogram —, six gradient work maps (4.0 M floats, 16.0 MB per spectrogram) and, on the first reservation, the
 * transposed weight images (1x1 convs transposed, the grouped 3x3 conv tap-flipped with m / k swapped per group, every eval-BatchNorm
 * scale folded in; as large as the resident fp32 images), packed on the device from those.  max_batch is capped at the engine's
 * max_batch.  A larger reservation replaces a smaller one; a smaller one keeps the present.  Counted by dmad_device_bytes.
 * DMAD_ERR_STATE before the classifier weights are finalised, or for an engine that holds VGG19_bn (its pair is dmad_reserve_vgg_vjp /
 * dmad_vgg_vjp below).
 * A failed reservation (out of memory) leaves no partial workspace behind: the pass-sized buffers it had allocated are released, the
 * packed weight images stay, and the next call packs only the missing ones.
 *
 * dmad_classify_vjp:  g_spec = (d logits / d spec)^T g_logits  for logits = CifarResNeXt(spec) (models/resnext.py:133-142) on the fp32
 * tier.  spec, g_spec: device fp32 [B][32][32]; g_logits: device fp32 [B][num_classes].  logits: optional (NULL) device fp32
 * [B][num_classes], bit-identical to dmad_classify_tier(.., tier = 0, ..).  Every engine precision (the fp32 images are resident on all
 * three).  The input gradient only: no weight gradients.  B in [1, max_batch], processed in passes of the reservation's size.  Store
 * scheme: the forward writes the tape, the backward walks the bottlenecks in reverse — every conv as the fp32 GEMM on the transposed
 * images (a stride-2 3x3 on the zero-dilated gradient; the stride-2 shortcut at the output resolution, scattered into the even
 * pixels), every ReLU as g * [y > 0] on the saved map, the shortcut gradient summed in the reduce conv's epilogue; head and conv1 as
 * small kernels.  No atomics, no split-K: g_spec is bit-identical across calls and independent of the batch.  DMAD_ERR_STATE without a
 * reservation or for a VGG19_bn engine (use dmad_vgg_vjp).
 *
 * dmad_mel_db_vjp:  g_x = (d melDB / d x)^T g_spec  for melDB = AmplitudeToDB(MelSpectrogram(x)) (certified_robustness_eval.py:85-87, the
 * forward of dmad_mel_db).  x, g_x: device fp32 [B][clip_len]; g_spec: device fp32 [B][32][32].  spec: optional (NULL) device fp32
 * [B][32][32], bit-identical to dmad_mel_db.  The forward is recomputed; nothing is kept across calls.  dB: g * 10 / (ln 10 M) where
 * M >= 1e-10 (torch's clamp rule), filterbank and DFT as fp32 GEMMs on transposed images, |.|^2 and the overlap-add (center padding
 * cropped) as small kernels in a fixed order.  The first call allocates the transposed images (17 MB) and the gradient maps of up to
 * 64 clips per pass (42 MB); B in [1, max_batch].  Every engine with a classifier. */
int dmad_reserve_classifier_vjp(dmad_engine* e, int32_t max_batch);
int dmad_classify_vjp(dmad_engine* e, const float* spec, int32_t B, const float* g_logits, float* g_spec, float* logits, dmad_stream s);
int dmad_mel_db_vjp(dmad_engine* e, const float* x, int32_t B, const float* g_spec, float* g_x, float* spec, dmad_stream s);

/* The masking loss of the imperceptible attack (Qin et al. 2019; stage 2 of AudioAttack, the driver's --attack Qin-I) and its gradient
 * with respect to the perturbation.  DESIGN §20.  With L = clip_len, F = (L - 2048) / 512 + 1 frames and K = 1025 bins:
 *
 * dmad_masking_loss_vjp replaces _loss_gradient_masking_threshold and _approximate_power_spectral_density
 * (robustness_eval/white_box_attack.py:606-678): torch.stft(n_fft = 2048, hop = 512, hann, center = False) of delta, the normalised
 * PSD estimate psd[b][k][f] = psd_scale[b] (8/3) / 2048^2 |stft|^2, loss[b] = mean over (k, f) of max(psd - theta[b][k][f], 0), and
 * g_delta = d sum(loss) / d delta.  delta, g_delta: device fp32 [B][L]; theta: device fp32 [B][K][F], the stabilised threshold
 * 10^(threshold / 10); psd_scale: device fp32 [B], 10^9.6 / psd_maximum_stabilized; loss: device fp32 [B]; psd: optional (NULL)
 * device fp32 [B][K][F].  The frames are read in place by the fp32 GEMM on the mel front-end's windowed DFT image, the hinge is one
 * kernel between that GEMM and the one on the transposed image (gradient where psd > theta, strictly: torch's ReLU), the
 * overlap-add of the uncentred framing sums the frames that cover a sample in ascending order; samples p >= 512 (F - 1) + 2048 lie
 * in no frame and get exactly 0.  Every sum has a fixed order (no atomics, no split-K): loss and g_delta are bit-identical across
 * calls and independent of the batch.  Nothing is kept across calls; the forward is not stored.  Works in the buffers of
 * dmad_mel_db_vjp (allocated on the first call of either), in passes of up to 64 clips.  B in [1, max_batch].  DMAD_ERR_STATE for an
 * engine without a classifier part (with_classifier = 0: no mel constants), B outside [1, max_batch], clip_len < 2048 or more than
 * 32 frames.
 *
 * dmad_masking_step is the same pass with the attack's update (white_box_attack.py:569-573) written in place of the gradient:
 * delta[b][p] = clamp(x + delta + signed_lr (g_net + alpha[b] g_theta), -1, 1) - x, g_theta the g_delta above; signed_lr = -lr for a
 * targeted attack, +lr otherwise.  x, g_net: device fp32 [B][L]; delta: device fp32 [B][L], updated in place; alpha: device fp32 [B].
 * loss as above (of delta before the update), bit-identical to dmad_masking_loss_vjp's. */
int dmad_masking_loss_vjp(dmad_engine* e, const float* delta, int32_t B, const float* theta, const float* psd_scale, float* g_delta, float* loss,
                          float* psd, dmad_stream s);
int dmad_masking_step(dmad_engine* e, const float* x, float* delta, const float* g_net, const float* alpha, float signed_lr, int32_t B,
                      const float* theta, const float* psd_scale, float* loss, dmad_stream s);

/* The same pair for the other classifier with a forward on the engine, VGG19_bn (models/vgg.py:31-52).  DESIGN §18.
 *
 * dmad_reserve_vgg_vjp reserves the VGG19_bn VJP workspace for up to max_batch spectrograms per pass: the TAPE of the fp32 forward — the
 * 16 post-ReLU conv maps and the two post-ReLU FC vectors, 311 296 floats (1.25 MB) per spectrogram —, two gradient ping-pong maps
 * (131 072 floats, 0.5 MB per spectrogram) and, on the first reservation, the backward weight images: convs 1 - 15 tap-flipped with m / k
 * swapped and the eval-BatchNorm scale folded in (wT[8 - tap][k][m] = w[tap][m][k] * scale[m]), classifier.0 and classifier.3 transposed
 * (38.9 M floats, 155 MB: as large as the resident fp32 images), packed on the device from those.  max_batch is capped at the engine's
 * max_batch.  A larger reservation replaces a smaller one; a smaller one keeps the present.  Counted by dmad_device_bytes.
 * DMAD_ERR_STATE before the classifier weights are finalised, or for an engine that holds ResNeXt29.
 *
 * dmad_vgg_vjp:  g_spec = (d logits / d spec)^T g_logits  for logits = VGG19_bn(spec) on the fp32 tier.  Shapes as dmad_classify_vjp.
 * logits: optional (NULL), bit-identical to dmad_classify_tier(.., tier = 0, ..): the forward runs dmad_classify's launches with the
 * tape's slots in place of its work maps.  Every engine precision.  The input gradient only.  B in [1, max_batch], processed in passes
 * of the reservation's size.  The backward walks the layers in reverse: classifier.6 and classifier.4's ReLU as one small kernel (k
 * ascending), classifier.3 / .0 as row-form fp32 GEMMs on the transposed images, each 2x2 max-pool together with the ReLU in front of
 * it as one kernel (the window's gradient goes to its first maximum in scan order — torch's max_pool2d rule — and only where that is
 * > 0; the arg-max is recomputed from the tape), every other ReLU as g * [y > 0], every 3x3 conv as the forward's fp32 GEMM on the
 * packed image, conv 0 as dmad_rx_conv1_bwd's kernel.  No atomics.  The deep layers use the forward's split-K slab with the forward's
 * reference row count (max_batch * H * H), so the split count follows from the layer and the engine: g_spec is bit-identical across
 * calls and does not depend on B, on the row's place in the batch or on the reservation's size.  DMAD_ERR_STATE without a reservation
 * or for a ResNeXt29 engine.
 *
 * dmad_vgg_vjp_tape (test hook): copies map `index` of the last dmad_vgg_vjp call's tape, rows [0, B), to out (device): index 0 - 15 the
 * conv maps, NHWC [B][H][H][C]; 16 - 17 the FC vectors [B][4096].  Valid when that call ran as one pass (its B <= the reservation) and
 * B <= its B; DMAD_ERR_STATE otherwise. */
int dmad_reserve_vgg_vjp(dmad_engine* e, int32_t max_batch);
int dmad_vgg_vjp(dmad_engine* e, const float* spec, int32_t B, const float* g_logits, float* g_spec, float* logits, dmad_stream s);
int dmad_vgg_vjp_tape(dmad_engine* e, int32_t index, int32_t B, float* out, dmad_stream s);

/* The same trio for WideResNet-28-10 (models/wideresnet.py).  DESIGN §21.  The forward (dmad_classify and every surface behind it) runs
 * on the fp32 tier whatever the tier asked for; its split counts follow from the layer and max_batch, so a sample's logits do not depend
 * on its batch.  No recheck bound has been measured for this classifier: dmad_smooth_votes, dmad_eval_samples, dmad_spec_smooth_votes and
 * dmad_spec_eval_samples return DMAD_ERR_STATE for it in DMAD_MODE_EXACT_VOTES (DMAD_MODE_FAST and DMAD_MODE_FP32 serve it;
 * dmad_eval_samples only when it is asked for logits: a call for purified waveforms alone never reaches the classifier).
 *
 * dmad_reserve_wrn_vjp reserves, for up to max_batch spectrograms per pass: the TAPE of the fp32 forward — the 25 post-ReLU maps in forward
 * order, o = relu(bn1(x)) and h = relu(bn2(conv1(o))) of blocks 0..11 and the final map, 2 310 144 floats (9.2 MB) per spectrogram —,
 * seven gradient work maps (1 187 840 floats, 4.8 MB per spectrogram) and, on the first reservation, the backward images: every 3x3
 * tap-flipped with m / k swapped (conv1's with bn2's scale folded in: wT[8 - tap][k][m] = w[tap][m][k] * scale[m]; conv2's plain), the
 * three 1x1 shortcuts transposed (36.5 M floats, as large as the forward images).  Capped at the engine's max_batch; a larger reservation
 * replaces a smaller one, a smaller one keeps the present.  Counted by dmad_device_bytes.
 *
 * dmad_wrn_vjp:  g_spec = (d logits / d spec)^T g_logits on the fp32 tier, shapes as dmad_vgg_vjp.  logits: optional (NULL), bit-identical
 * to dmad_classify_tier(.., 0, ..).  Every engine precision.  B in [1, max_batch], in passes of the reservation's size.  The backward:
 * dmad_rx_head_bwd's kernel on fc.w with the final bn's scale folded into its columns; per block, in reverse, conv2's data gradient, the
 * ReLU mask of h, the shortcut's 1x1 at the output resolution (scattered into the even pixels at stride 2), conv1's data gradient (at
 * stride 2 on the zero-dilated gradient) with the shortcut's as its residual, then dmad_wrn_preact_bwd; the stem's backward last.  No
 * atomics; every GEMM gets the forward's slab and max_batch * H * H reference rows, so g_spec does not depend on B, on the row's place or
 * on the reservation's size.  DMAD_ERR_STATE without a reservation, before the weights are finalised, or for another classifier.
 *
 * dmad_wrn_vjp_tape (test hook): map `index` (0..24: o / h of block index / 2, then the final map; NHWC) of the last call's tape, rows
 * [0, B); valid when that call ran as one pass and B <= its B, DMAD_ERR_STATE otherwise. */
int dmad_reserve_wrn_vjp(dmad_engine* e, int32_t max_batch);
int dmad_wrn_vjp(dmad_engine* e, const float* spec, int32_t B, const float* g_logits, float* g_spec, float* logits, dmad_stream s);
int dmad_wrn_vjp_tape(dmad_engine* e, int32_t index, int32_t B, float* out, dmad_stream s);

/* The same trio for DenseNet-BC-100-12 (models/densenet.py).  DESIGN §24.  The forward (dmad_classify and every surface behind it) runs on
 * the fp32 tier whatever the tier asked for, in 102 launches of the kernels of csrc/densenet.hip; every kernel works pixel by pixel, so a
 * sample's logits do not depend on its batch.  No recheck bound has been measured for this classifier: the four vote loops return
 * DMAD_ERR_STATE for it in DMAD_MODE_EXACT_VOTES, as for WideResNet-28-10.
 *
 * dmad_reserve_dn_vjp reserves, for up to max_batch spectrograms per pass: the TAPE of the fp32 forward — the three concatenation streams
 * at their pitches (32 x 32 x 216, 16 x 16 x 304, 8 x 8 x 344: 322 048 floats) and the 48 post-ReLU h maps (1 032 192 floats), 5.4 MB per
 * spectrogram — and the gradient streams with g_h (371 200 floats, 1.5 MB per spectrogram).  The backward images are built with the
 * forward's at dmad_finalize_weights.  Capped at the engine's max_batch; a larger reservation replaces a smaller one, a smaller one
 * keeps the present.  Counted by dmad_device_bytes.
 *
 * dmad_dn_vjp:  g_spec = (d logits / d spec)^T g_logits on the fp32 tier, shapes as dmad_vgg_vjp.  logits: optional (NULL), bit-identical
 * to dmad_classify_tier(.., 0, ..).  Every engine precision.  B in [1, max_batch], in passes of the reservation's size.  100 launches
 * behind the forward's 102; no atomics; a gradient channel collects its terms in layer order, last to first; g_spec does not depend on B,
 * on the row's place or on the reservation's size.  DMAD_ERR_STATE without a reservation, before the weights are finalised, or for
 * another classifier.
 *
 * dmad_dn_vjp_tape (test hook): post-ReLU map `index` of the last call's forward, rows [0, B), NHWC [B][H][H][C] without padding: 2 k and
 * 2 k + 1 are o = relu(bn1(x)) [24 + 12 k channels] and h [48] of layer k of dense1, 32 is trans1's o [216], 33..64 dense2, 65 trans2's o
 * [300], 66..97 dense3, 98 the final map [342].  h maps are copied from the tape; the others are recomputed from the tape's streams with
 * the forward's own pre-activation function.  Valid when that call ran as one pass and B <= its B, DMAD_ERR_STATE otherwise. */
int dmad_reserve_dn_vjp(dmad_engine* e, int32_t max_batch);
int dmad_dn_vjp(dmad_engine* e, const float* spec, int32_t B, const float* g_logits, float* g_spec, float* logits, dmad_stream s);
int dmad_dn_vjp_tape(dmad_engine* e, int32_t index, int32_t B, float* out, dmad_stream s);

/* The reverse VP-SDE purifier of the reference's adaptive-attack driver (adaptive_attack_eval.py --defense Diffusion ->
 * diffusion_models/diffwave_sde.py RevDiffWave.audio_editing_sample: torchsde.sdeint_adjoint(RevVPSDE, method='euler', dt = 1/T)).
 * The step schedule is built by the CALLER on the host, in float32 and in torchsde's order (diffusion_models/diffwave_sde.py
 * vpsde_schedule): the float32 time grid repeats and skips step indices, so no index sequence is assumed here.
 *
 * dmad_vpsde_purify:  x <- c_a * x0 + c_b * z_0;  for n = 0 .. n_steps-1:  x <- x + (hb[n] * x - q[n] * eps(x, k[n])) * h[n] + gs[n] * z_{n+1}
 * (gs[n] == 0: no draw).  k (step index of the eps-network), h (step length), hb (beta / 2), q (beta / sqrt(1 - alpha_bar[k])), gs (the
 * noise scale of the step): HOST arrays of n_steps.  Noise: z (optional, device fp32 [n_steps + 1][B][clip_len], test hook), or, with
 * z == NULL, Philox N(0,1) drawn in registers, keyed (seed, sample0 + b, stream 0x5DE00000 for the diffusion draw, 0x5DE00001 + n
 * for Euler step n).  path: 0 = the mode's default WaveNet path (dmad_set_waveform_tier's tier on an exact-vote engine, like the other
 * waveform-returning surfaces), 1 = exact fp32 (DMAD_FP32 / DMAD_EXACT engines).  x0, out: device fp32 [B][clip_len] (may alias).
 * traj: optional device fp32 [n_steps + 1][B][clip_len]; slot n receives the state entering Euler step n, slot n_steps the output.  B is
 * processed in passes of max_batch clips.  One fused kernel per step after the eps-network (read x and eps, draw z, write x and the
 * trajectory slot).
 *
 * dmad_vpsde_purify_vjp:  g_x0 = (d out / d x0)^T g_out of that chain on the exact-fp32 path, the draws held fixed: walking the steps
 * in reverse,  g <- (1 + h[n] hb[n]) g - (h[n] q[n]) J_n^T g  with J_n^T g the eps-network's VJP (dmad_wavenet_eps_vjp's recompute
 * scheme) at traj slot n, and g_x0 = c_a * g.  The update is the epilogue of the VJP's init-conv backward (two ping-pong buffers of the
 * reservation); the last step folds c_a in.  traj: as written by dmad_vpsde_purify(.., path = 1, ..) for the same B (slots 0 .. n_steps-1
 * are read).  g_out, g_x0: device fp32 [B][clip_len], must not alias.  B <= max_batch, processed in passes of the dmad_reserve_vjp
 * reservation; nothing is allocated.  Every reduction in a fixed order: g_x0 is bit-reproducible and independent of the batch. */
int dmad_vpsde_purify(dmad_engine* e, const float* x0, int32_t B, int32_t n_steps, float c_a, float c_b, const int32_t* k, const float* h,
                      const float* hb, const float* q, const float* gs, const float* z, uint64_t seed, uint64_t sample0, int32_t path, float* out,
                      float* traj, dmad_stream s);
int dmad_vpsde_purify_vjp(dmad_engine* e, const float* traj, int32_t B, int32_t n_steps, float c_a, const int32_t* k, const float* h,
                          const float* hb, const float* q, const float* g_out, float* g_x0, dmad_stream s);

/* The reverse VP-SDE purifier on standardised mel spectrograms (adaptive_attack_eval.py --defense Diffusion-Spec ->
 * diffusion_models/improved_diffusion_sde.py RevImprovedDiffusion.image_editing_sample: torchsde.sdeint_adjoint(RevVPSDE, method='euler')
 * at torchsde's default dt = 1e-3).  The same chain as dmad_vpsde_purify with the Improved-Diffusion UNet as the eps-network; the
 * schedule is again built by the CALLER on the host in float32 (diffusion_models/improved_diffusion_sde.py spec_vpsde_schedule; DESIGN
 * §13): beta and the score are continuous in t, so k[n] (the UNet's step input) indexes no table and may be anything in [0, 1000].
 *
 * dmad_spec_vpsde_purify:  x <- c_a * x0 + c_b * z_0;  for n:  x <- x + (hb[n] * x - q[n] * eps(x, k[n])) * h[n] + gs[n] * z_{n+1}.
 * x0, out: device fp32 [B][32][32] (standardised maps; may alias).  Host arrays k / h / hb / q / gs of n_steps.  Noise: z (optional,
 * device fp32 [n_steps + 1][B][1024], test hook) or Philox N(0,1) keyed (seed, sample0 + b, stream 0x5DF00000 for the diffusion draw,
 * 0x5DF00001 + n for Euler step n) — the first 1024 values of dmad_philox_normal's row.  path: 0 = the mode's UNet map tier (the tier
 * dmad_unet_eps runs), 1 = the exact-fp32 tier (DMAD_FP32 / DMAD_EXACT engines).  traj: optional device fp32 [n_steps + 1][B][1024];
 * slot n receives the state entering step n, slot n_steps the output.  B runs in passes of max_batch spectrograms.
 *
 * dmad_spec_vpsde_purify_vjp:  g_x0 = (d out / d x0)^T g_out of that chain on the exact-fp32 tier, the draws held fixed: walking the
 * steps in reverse,  g <- (1 + h[n] hb[n]) g - (h[n] q[n]) J_n^T g  with J_n^T g the UNet VJP (dmad_unet_eps_vjp's recompute: forward
 * with its tape at traj slot n, then the backward), and g_x0 = c_a * g.  The update is the epilogue of the input conv's transposed conv
 * (two ping-pong buffers of the dmad_reserve_unet_vjp reservation); the last step folds c_a in.  No tape is kept across steps.  traj:
 * as written by dmad_spec_vpsde_purify(.., path = 1, ..) for the same B.  g_out, g_x0: device fp32 [B][1024], must not alias.
 * B <= max_batch, processed in passes of the reservation; nothing is allocated.  Every reduction in a fixed order: g_x0 is
 * bit-reproducible and independent of the batch.  DMAD_ERR_STATE without a reservation or the fp32 tier; DMAD_ERR_INVALID for
 * n_steps < 1 or a k outside [0, 1000]. */
int dmad_spec_vpsde_purify(dmad_engine* e, const float* x0, int32_t B, int32_t n_steps, float c_a, float c_b, const int32_t* k, const float* h,
                           const float* hb, const float* q, const float* gs, const float* z, uint64_t seed, uint64_t sample0, int32_t path,
                           float* out, float* traj, dmad_stream s);
int dmad_spec_vpsde_purify_vjp(dmad_engine* e, const float* traj, int32_t B, int32_t n_steps, float c_a, const int32_t* k, const float* h,
                               const float* hb, const float* q, const float* g_out, float* g_x0, dmad_stream s);

/* The forward of RobustCertificate.smooth_predict's loop body (certified_robust.py:46-56) for an explicit LIST of Monte Carlo
 * samples on an explicit WaveNet path — the audit of the exact-vote mode (RobustCertificate.certify(audit=k): k samples that
 * voted on the 16-bit tier are re-evaluated on a higher one) and the measurement tools' hook:  row i of logits_out [n][num_classes]
 * / x0_out [n][clip_len] (either optional) is sample idx[i] (device int64, GLOBAL sample indices; noise = Philox key
 * (seed, idx[i]) or row idx[i] - sample0 of `delta`), evaluated on path 0 (the mode's default), 1 (exact fp32) or 2 (split-f16).
 * Nothing votes, no queue is touched. */
int dmad_eval_samples(dmad_engine* e, const float* clip, float sigma, float sqrt_alpha_bar_star, int32_t t, float c_a, float c_b,
                      uint64_t seed, uint64_t sample0, const float* delta, const int64_t* idx, int64_t n, int32_t path, float* logits_out,
                      float* x0_out, dmad_stream s);

/* Measurement hook (tools/gpu_error_attribution.py): switch single roundings of the 16-bit path on INSIDE the fp32-grade split-f16
 * tier, to attribute the 16-bit tier's logit error to its sources.  masks[0..3] act on the tier's dilated-conv, res-conv, skip and
 * final_conv.0 GEMM launches: bit 0 = weights rounded to f16, bit 1 = the MFMA eats f16(activation) while the stored value keeps
 * its 22 bits, bit 2 = the launch's split-format output (gate / residual stream) is stored as f16; masks[4] != 0 = the init
 * conv's output is stored as f16.  All zero (the default) = the product tier. */
int dmad_debug_rounding(dmad_engine* e, const int32_t masks[5]);

/* BASELINE configuration C5: the Monte Carlo vote loop with the SPEC-domain purifier (Improved-Diffusion UNet on 1x32x32 mel
 * spectrograms) in place of the waveform purifier.  The reference has no working composite for it
 * (diffusion_models/improved_diffusion_ddpm.py:53-59 discards its reverse chain), so the loop is DEFINED here as what its parts
 * are for — randomized smoothing in the input domain (certified_robust.py:46-48, no denoiser => no sqrt(alpha_bar*) scale), then
 * AcousticSystem's defense_type = 'spec' order (acoustic_system.py:40-49):  for samples i in [sample0, sample0 + n):
 *   x_i = clip + sigma * delta_i                    (Philox keyed (seed, i), stream 0)
 *   s   = mel_dB(x_i) ; s0 = 2 (s - lo) / (hi - lo) - 1            (melspec_standardize, sc09_spectrogram_dataset.py:62-72)
 *   s_t = q_a * s0 + q_b * z                        (q_sample at t = t_star, gaussian_diffusion.py:188-206; Philox stream 0x5BEC)
 *   for t = t_star .. 0:  s_t <- p_sample(s_t, t)   (dmad_unet_p_sample with c_a/c_b/c_1/c_2/c_sig[t]: HOST arrays of t_star + 1 entries)
 *   logits = classifier((s_0 + 1)(hi - lo) / 2 + lo) ; counts[argmax] += 1.
 * q_a / q_b = sqrt_alphas_cumprod[t_star] / sqrt_one_minus_alphas_cumprod[t_star].  counts: device int64[num_classes],
 * accumulated; logits_out [n][num_classes] and spec_out [n][32][32] (the purified dB spectrograms) optional. */
int dmad_spec_smooth_votes(dmad_engine* e, const float* clip, float sigma, int32_t t_star, float q_a, float q_b, const float* c_a,
                           const float* c_b, const float* c_1, const float* c_2, const float* c_sig, float mel_lo, float mel_hi, int64_t n,
                           int32_t batch, uint64_t seed, uint64_t sample0, int64_t* counts, float* logits_out, float* spec_out, dmad_stream s);

/* The UNet's tiers.  Engines of precision DMAD_BF16 / DMAD_EXACT hold, beside the exact-fp32 UNet, a 16-BIT TIER of it: every
 * conv / 1x1 (unet.py:107-252) on f16 operands with fp32 accumulation (v_mfma_f32_16x16x32_f16); the hidden state exists as f16 maps
 * only, GroupNorm statistics are sums over the f16-rounded outputs taken in the producing GEMM's epilogue (evaluated as E[x^2] - mean^2
 * in fp32), softmax, bias and residual sums in fp32 (measured: 4e-3 of max|eps| per evaluation).  DMAD_EXACT engines also hold a
 * SPLIT-F16 MIDDLE TIER: the fp32 pipeline (fp32 maps, GroupNorm, softmax, residual sums) with every conv / 1x1 on split-f16 operands
 * (three f16 MFMAs per product, ~22 significant bits: fp32-grade at several times the fp32 matrix rate).
 * dmad_unet_eps / dmad_unet_p_sample / dmad_spec_query_logits — map- and logit-returning surfaces without a recheck — follow
 * dmad_set_waveform_tier like the waveform-returning ones: on an exact-vote engine the split-f16 tier by default (within 1e-4 of the
 * reference fixtures at 2.2 x the fp32 rate), the exact-fp32 UNet with tier 1 (fp32) or in DMAD_MODE_FP32, the 16-bit tier with tier 0
 * or in DMAD_MODE_FAST (DMAD_FP32 engines have only the fp32 one).  In DMAD_MODE_EXACT_VOTES dmad_spec_smooth_votes runs every sample's chain on the 16-bit tier, queues the samples whose
 * top-2 logit margin is below tau_spec (dmad_set_spec_recheck_margin; default 0.13 = 1.5 x the largest leader-difference error (0.084;
 * Gaussian scale 0.020) of the 16-bit chain measured on 6 144 samples of the calibrated synthetic stand-in) and
 * re-runs their WHOLE chain from the same Philox keys on the split-f16 tier; a sample whose margin is still below tau_spec2
 * (dmad_set_spec_recheck_margin2, default 5e-4 = 2.2 x its measured error; < 0: no middle tier) goes on to the exact-fp32 UNet.  An EMPIRICAL guarantee like the
 * waveform loop's (dmad_set_mode), and like it a property of the WEIGHTS: calibrate (Engine.calibrate_spec_recheck) before certifying
 * with other checkpoints.  dmad_spec_recheck_stats: samples voted by dmad_spec_smooth_votes, samples whose chain left the 16-bit tier;
 * dmad_spec_recheck_stats2: + those that reached the exact-fp32 UNet. */
/* dmad_unet_eps on an explicit tier (0: exact fp32, 1: 16-bit, 2: split-f16) — test / measurement hook (DMAD_ERR_STATE for a tier the
 * engine's precision does not hold). */
int dmad_unet_eps_tier(dmad_engine* e, const float* x_t, int32_t t, int32_t B, int32_t tier, float* eps, dmad_stream s);
int dmad_set_spec_recheck_margin(dmad_engine* e, float tau);
int dmad_spec_recheck_stats(dmad_engine* e, int64_t* samples, int64_t* rechecked, int32_t reset);
int dmad_set_spec_recheck_margin2(dmad_engine* e, float tau2);
int dmad_spec_recheck_stats2(dmad_engine* e, int64_t* samples, int64_t* rechecked, int64_t* rechecked_fp32, int32_t reset);
/* The chain of dmad_spec_smooth_votes for an explicit LIST of Monte Carlo samples on an explicit UNet tier (0: exact fp32, 1: 16-bit,
 * 2: split-f16; the classifier is the fp32 one on tiers 0 and 2): row i of logits_out [n][num_classes] / spec_out [n][32][32] (either optional) is sample
 * idx[i] (device int64, GLOBAL indices: every draw of the row is Philox-keyed by it).  Nothing votes, no queue is touched — the hook
 * behind the calibration of tau_spec for the resident weights (Engine.calibrate_spec_recheck) and RobustCertificate.certify(audit=k)
 * on the spec-domain loop. */
int dmad_spec_eval_samples(dmad_engine* e, const float* clip, float sigma, int32_t t_star, float q_a, float q_b, const float* c_a,
                           const float* c_b, const float* c_1, const float* c_2, const float* c_sig, float mel_lo, float mel_hi, uint64_t seed,
                           const int64_t* idx, int64_t n, int32_t tier, float* logits_out, float* spec_out, dmad_stream s);

/* Batched query of the whole system for the gradient-free attack drivers: EOT.forward evaluates
 * model(x_batch.repeat(EOT_batch_size, 1, 1)) EOT_num_batches times (robustness_eval/_EOT.py:30-64; callers
 * black_box_attack.py:186-220, _NES.py:15-55) where model = AcousticSystem(classifier, transform, defender)
 * (acoustic_system.py:27-51).  One call does all of it:  row i = r * B + b  (r < repeats, b < B) is clip x[b];
 *   sampler 0: no wave defender;  1: DiffWave.forward (diffusion + t_star reverse steps, diffwave_ddpm.py:36-104;
 *   coefficients as for dmad_ddpm_purify);  2: one_shot_denoise at t = t_star - 1 (c_a, c_b as for dmad_one_shot);
 *   then mel dB -> classifier.  Noise of row i is Philox keyed (seed, sample0 + i): a row's logits do not depend on how
 *   the rows are batched.  x: device fp32 [B][clip_len]; logits: [repeats * B][num_classes]; decisions: optional
 *   int32 [repeats * B] arg-max (first maximum wins). */
int dmad_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, int32_t sampler, int32_t t_star, float c_a, float c_b,
                      const float* c_eps, const float* c_div, const float* c_sig, uint64_t seed, uint64_t sample0, float* logits,
                      int32_t* decisions, dmad_stream s);

/* The same batched query for AcousticSystem(defense_type = 'spec') (acoustic_system.py:40-49: transform, THEN the defender on the
 * spectrogram): row i = r * B + b is clip x[b] through  mel dB -> standardise -> q_sample(t_star) -> t_star + 1 p_sample steps ->
 * un-standardise -> classifier  — the chain of dmad_spec_smooth_votes without the smoothing noise, every draw of row i Philox-keyed
 * (seed, sample0 + i) (q_sample: stream 0x5BEC, p_sample at t: stream 0x0E70 + t), so a row's logits do not depend on how the rows are
 * batched.  The UNet runs the tier of the map-returning surfaces (dmad_set_waveform_tier: split-f16 by default on an exact-vote engine),
 * the classifier the fp32 one: a query hands logits back and has no recheck.  Coefficients as for dmad_spec_smooth_votes (HOST arrays of t_star + 1
 * entries).  logits: [repeats * B][num_classes]; decisions: optional int32 [repeats * B]. */
int dmad_spec_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, int32_t t_star, float q_a, float q_b, const float* c_a,
                           const float* c_b, const float* c_1, const float* c_2, const float* c_sig, float mel_lo, float mel_hi, uint64_t seed,
                           uint64_t sample0, float* logits, int32_t* decisions, dmad_stream s);

/* NES gradient estimate of the query-only attacks (robustness_eval/_NES.py:15-55; caller black_box_attack.py:180-184) without its
 * [n_audios, samples, 1, N] tensors: the probe directions are a pure function of a Philox key and are regenerated where they are used.
 * Direction j (0 <= j < H, H = P / 2) of clip b is the row that dmad_philox_normal(seed, sample = draw0 + b * H + j, stream =
 * DMAD_PHILOX_STREAM_NES) returns; both calls below produce exactly those bits.
 * Philox stream ids in use, which a new draw must not collide with: 0 (smoothing noise of the vote loops), 1 + t for t < T (DDPM reverse
 * step t), 0x0E70 + t (spec-domain p_sample at t), 0x5BEC (spec-domain q_sample), 0xD1FF (DiffWave diffusion draw), 0x5DE00000 + n
 * (reverse VP-SDE: diffusion draw and Euler steps), 0x5DF00000 + n (the same on the spectrogram), 0x4E450000 (NES directions),
 * 0x50530000 + k for k < 4 (particle swarm: 0 positions, 1 velocities, 2 r1, 3 r2). */
#define DMAD_PHILOX_STREAM_NES 0x4E450000u
#define DMAD_PHILOX_STREAM_PSO 0x50530000u

/* Query rows [row0, row0 + rows) of the reference's layout (_NES.py:19-25: noise = cat(noise, -noise), the zero probe in front on the
 * first draw batch, eval_input = noise * sigma + x).  The layout is clip-major with per_clip = P + with_origin rows per clip: the optional
 * slot 0 is x[b] unchanged, the next H slots are x[b] + sigma * u_j, the last H slots x[b] - sigma * u_j (product rounded, then the sum; no
 * clamping, as in the reference).  A row's content depends only on its global index, never on row0 or rows, so the queries can be made
 * a chunk at a time.  x: device fp32 [B][clip_len]; out: device fp32 [rows][clip_len].  P must be even and >= 2, and
 * 0 <= row0, row0 + rows <= B * per_clip (DMAD_ERR_INVALID otherwise). */
int dmad_nes_probes(dmad_engine* e, const float* x, int32_t B, int32_t P, float sigma, int32_t with_origin, uint64_t seed, uint64_t draw0,
                    int64_t row0, int32_t rows, float* out, dmad_stream s);

/* grad[b][l] = (accumulate ? grad[b][l] : 0) + scale * sum_{j < H} (w[b][j] - w[b][H + j]) * u_{b,j}[l]   (_NES.py:47,52,54:
 * torch.mean(loss * noise, 1) over the antithetic pairs, / sigma / num_batches folded into scale).  w: device fp32 [B][P], the losses of
 * the + probes in the first H entries of a clip and those of the - probes in the last H; grad: device fp32 [B][clip_len].  u is
 * regenerated in registers.  Each output element is summed by one thread, j ascending, every product and sum rounded to fp32, without
 * atomics: the result is bit-reproducible and a clip's row does not depend on B.  P even and >= 2. */
int dmad_nes_grad(dmad_engine* e, const float* w, int32_t B, int32_t P, float scale, uint64_t seed, uint64_t draw0, int32_t accumulate,
                  float* grad, dmad_stream s);

/* Particle swarm of SirenAttack (robustness_eval/black_box_attack.py:344-498) without its host-side draws and loops.  The state is
 * caller-owned device fp32; nothing is allocated.  Row r = b * P + p (clip-major, P = n_particles) of the [B * P][clip_len] arrays loc,
 * vel, pbest_loc and queries is particle p of clip b; x, lower, upper (and keep, gbest_loc of dmad_pso_step) are [B][clip_len]; pbests is
 * [B][P].  A uniform draw is u = ((float)(word >> 8) + 0.5f) * 2^-24 in fp32 — the uniforms dmad_philox_normal feeds to Box-Muller — of
 * the Philox words at counter (block = l / 4, sample, stream) under key seed, with sample = draw0 + b * P + p and stream =
 * DMAD_PHILOX_STREAM_PSO + {0 position, 1 velocity, 2 r1, 3 r2}.  One swarm event (an init or a step) consumes B * P sample keys: the
 * caller advances draw0 by that much.  Every product, sum and difference is rounded to fp32 on its own (no contraction), there are no
 * atomics, and a row is a function of its key and its inputs only, never of B.  B < 1, P < 1 or a required pointer that is null:
 * DMAD_ERR_INVALID.
 *
 * dmad_philox_uniform (test hook, the uniform twin of dmad_philox_normal): out[b] = the clip_len uniforms of key (seed, sample0 + b,
 * stream); out: device fp32 [B][clip_len]. */
int dmad_philox_uniform(dmad_engine* e, uint64_t seed, uint64_t sample0, uint32_t stream, int32_t B, float* out, dmad_stream s);

/* A new swarm (black_box_attack.py:371-391: the np.random.uniform positions and velocities of an epoch; l.404: the query rows).
 *   pbest_loc[r] = clamp(lower + (upper - lower) * u_pos, lower, upper);   vel[r] = -d + (2 d) * u_vel,  d = |lower - upper|;
 *   loc = pbest_loc;   queries[r] = loc[r] + x[b].
 * keep (optional, [B][clip_len]): particle 0 of clip b is keep[b] bit for bit — the best personal best an epoch carries into the next,
 * l.377-382; its position key is unused and every other particle is what the call without keep gives it. */
int dmad_pso_init(dmad_engine* e, const float* x, const float* lower, const float* upper, int32_t B, int32_t P, const float* keep,
                  uint64_t seed, uint64_t draw0, float* pbest_loc, float* loc, float* vel, float* queries, dmad_stream s);

/* One swarm move (black_box_attack.py:474-484: np.random.rand r1 and r2, the velocity and position update, the clamp; l.404), in place:
 *   r1 = fl(u_r1 + 1e-5f), r2 likewise;
 *   vel <- fl(fl(fl(w vel) + fl(fl(c1 r1) fl(pbest_loc - loc))) + fl(fl(c2 r2) fl(gbest_loc[b] - loc)))   (the reference's expression,
 *   left to right);   loc <- min(max(fl(loc + vel), lower), upper);   queries <- fl(loc + x[b]).
 * gbest_loc: [B][clip_len], the global best of every working clip, in working-set order. */
int dmad_pso_step(dmad_engine* e, const float* x, const float* lower, const float* upper, const float* pbest_loc, const float* gbest_loc,
                  int32_t B, int32_t P, float w, float c1, float c2, uint64_t seed, uint64_t draw0, float* loc, float* vel, float* queries,
                  dmad_stream s);

/* The bests after an evaluation (black_box_attack.py:420-437: torch.where(loss < pbests) with its loop of row copies, the arg-min and
 * the per-clip loop on gbests), without a host round trip.  loss: device fp32 [B][P]; predict: device int64 [B][P]; index: optional
 * device int64 [B] of distinct rows, the row of gbests / gbest_loc / gbest_predict a working clip owns (null: row b).
 *   where loss[b][p] < pbests[b][p]:  pbests[b][p] <- loss[b][p], pbest_loc[b * P + p] <- loc[b * P + p];
 *   then, k = the first arg-min of the updated pbests[b], i = index ? index[b] : b:  if pbests[b][k] < gbests[i]:
 *   gbests[i] <- pbests[b][k], gbest_loc[i] <- pbest_loc[b * P + k], gbest_predict[i] <- predict[b][k].
 * A comparison that is false, with a NaN too, changes nothing (pbests itself must be free of NaN, as it is when it starts at +inf).
 * Three launches in stream order — the personal-best rows, the global-best rows, then the scalars — so that every block that copies a
 * row decides from the scalars as they were before the call. */
int dmad_pso_update_best(dmad_engine* e, const float* loss, const int64_t* predict, const float* loc, const int64_t* index, int32_t B,
                         int32_t P, float* pbests, float* pbest_loc, float* gbests, float* gbest_loc, int64_t* gbest_predict, dmad_stream s);

/* Whole-clip real FFT pair and the bisection of the Kenansville FFT attack (robustness_eval/_KenanFFT.py: fft_compression l.57-82,
 * atk_bst_fft l.180-247).  With L = clip_len and M = L / 2, a clip is the M complex points z[n] = x[2n] + i x[2n+1]; one workgroup per
 * clip runs their M-point Stockham FFT in LDS and the real-FFT pass around it, in fp32, in a fixed order, without atomics: a row's bits
 * are a function of its own input row, never of B, and equal from call to call.  Twiddles are one device table of exp(-2 pi i j / L),
 * float64 on the host rounded once, built at the first call on an engine.  M must factor into radices 4, 2 and 5 with at most one radix-2
 * stage, and 8 M + 256 bytes must fit in a workgroup's LDS with M <= 16384; 16000 and 32000 are served.  Any other clip_len is
 * DMAD_ERR_SHAPE with a message that names the length and the rule.  Nothing is sized by max_batch (the grid is B), and the engine's
 * precision, mode and parts (with_wavenet, with_classifier) do not matter.  The kernels move rows as 8- and 16-byte vectors: x, spec
 * and out must be 8-byte aligned, perturbed and best of dmad_kenan_update 16-byte aligned (clip_len is a multiple of 128, so every row
 * then is).  B < 1, a required pointer that is null or a misaligned one: DMAD_ERR_INVALID.
 *
 * dmad_wave_rfft (l.68 torch.fft.rfft, and l.198 torch.fft.fft(data).abs().max(dim=2): for a real clip the maximum over the M + 1
 * bins is the maximum over all L):  x: device fp32 [B][L];  spec: device fp32 [B][M + 1][2] (re, im), the DC and Nyquist bins with
 * im = 0;  maxmag: device fp32 [B], max_k sqrt(re^2 + im^2), a fixed-order workgroup reduction. */
int dmad_wave_rfft(dmad_engine* e, const float* x, int32_t B, float* spec, float* maxmag, dmad_stream s);

/* l.72 (fft_image[fft_image.abs() < factor] = 0) and l.77 (torch.fft.irfft) in one launch:  spec as dmad_wave_rfft writes it;  factor:
 * device fp32 [B], or null for the plain inverse;  out: device fp32 [B][L] = irfft of spec with every bin sqrt(re^2 + im^2) < factor[b]
 * zeroed, scaled by 1 / L;  kept: device int32 [B], the bins that survive (M + 1 without factor).  The imaginary parts of the DC and
 * Nyquist bins are ignored, as torch.fft.irfft ignores them.  A comparison with a NaN is false: the bin stays. */
int dmad_wave_irfft_threshold(dmad_engine* e, const float* spec, const float* factor, int32_t B, float* out, int32_t* kept, dmad_stream s);

/* l.233-243, the per-clip loop body, without the host loop.  pred, label: device int64 [B];  perturbed, best: device fp32 [B][L];
 * fmin, fmax, factor: device fp32 [B];  succ: device int32 [B].  With won = targeted ? pred[b] == label[b] : pred[b] != label[b]:
 *   won:   best[b] <- perturbed[b];  fmax[b] <- factor[b];  succ[b] <- 1;
 *   else:  fmin[b] <- factor[b]   (best[b] and succ[b] stay);
 *   then   factor[b] <- |fl(fl(fmin[b] + fmax[b]) / 2)|,  torch's fp32 statements in torch's order: bit for bit. */
int dmad_kenan_update(dmad_engine* e, const int64_t* pred, const int64_t* label, int32_t B, int32_t targeted, const float* perturbed,
                      float* best, float* fmin, float* fmax, float* factor, int32_t* succ, dmad_stream s);

/* Baseline waveform defenses of the attack drivers (transforms/time_defense.py: AS l.102-127, MS l.130-157; transforms/
 * frequency_defense.py: DS l.37-60, LPF l.62-99, BPF l.101-141).  Everything is fp32 on rows [B][len]; an output row is a function of its
 * own input row only, never of B or of how a caller chunks the rows; there are no atomics, so results are bit-reproducible.  Unlike the
 * engine's network paths B is not limited by max_batch here (the kernels hold no per-row workspace), except where a VJP recomputes a
 * forward into the engine workspace (dmad_wave_iir_vjp: B <= max_batch).  A refused argument is DMAD_ERR_INVALID with a message that
 * names the export.
 *
 * Smoothing, odd window w, p = (w - 1) / 2 zeros on both sides (time_defense.py:124 F.conv1d(padding = p); l.151 F.pad(value = 0.) —
 * MS pads with zeros despite its "replicate" comment).  kind 0, mean, odd w <= 63:  y[t] = sum_k fl(x[t + k - p] * fl(1 / w)), k ascending,
 * every product and sum rounded on its own.  kind 1, median, w in {3, 5, 7, 9}:  y[t] = the middle element of the sorted window
 * (torch.median of an odd window, l.156; a window that holds a NaN gives NaN).
 * VJP of the mean: the same kernel on g_y (the operator is symmetric under zero padding; x is not read and may be null).  VJP of the
 * median:  g_x[s] = sum_t g_y[t] [src(t) = s],  t ascending, src(t) = the LOWEST window position that holds the median value of window
 * t (the tie rule; torch leaves it open); a padding position receives nothing.  It is a gather: the thread of s recomputes the medians
 * of the w windows that contain s. */
int dmad_wave_smooth(dmad_engine* e, const float* x, int32_t B, int32_t kind, int32_t window, float* y, dmad_stream s);
int dmad_wave_smooth_vjp(dmad_engine* e, const float* x, const float* g_y, int32_t B, int32_t kind, int32_t window, float* g_x, dmad_stream s);

/* Polyphase FIR resampling (frequency_defense.py:53-56, torchaudio.transforms.Resample: F.conv1d(F.pad(x, (width, width + orig)),
 * kernel, stride = orig), the phases interleaved, cut to L_out):
 *   y[i * phases + j] = sum_k ker[j][k] * xpad[i * stride + k],  k ascending, summed in float64 and rounded to fp32 once,
 * xpad = width zeros | x | width + stride zeros.  ker: HOST fp32 [phases][taps] (phases * taps <= 256; it travels as a kernel argument);
 * x: device [B][L_in], y: device [B][L_out]; L_in need not be the clip length.  DS is two calls: 16 kHz -> 8 kHz with phases 1, stride 2,
 * 28 taps, width 13, then 8 kHz -> 16 kHz with phases 2, stride 1, 15 taps, width 7.  The VJP is the transposed operator, written as a
 * gather over the outputs that read x[m]: g_x [B][L_in] from g_y [B][L_out], frames and phases ascending. */
int dmad_wave_resample(dmad_engine* e, const float* x, int32_t B, int32_t L_in, const float* ker, int32_t phases, int32_t taps, int32_t stride,
                       int32_t width, int32_t L_out, float* y, dmad_stream s);
int dmad_wave_resample_vjp(dmad_engine* e, const float* g_y, int32_t B, int32_t L_in, const float* ker, int32_t phases, int32_t taps,
                           int32_t stride, int32_t width, int32_t L_out, float* g_x, dmad_stream s);

/* y = clamp(lfilter(b, a, x), lo, hi)  (frequency_defense.py:85-98 / 125-139: Butterworth b, a, torch_lfilter one clip at a time on the
 * CPU, then clamp) for order n <= 8, parallel along time.  b, a: HOST fp32 [order + 1], a[0] != 0, both divided by a[0] (in float64,
 * rounded to fp32).  The filter is lfilter's transposed direct form II:  y = b0 x + z0;  z_i = b_{i+1} x - a_{i+1} y + z_{i+1}.  A row is
 * cut into at most 128 segments of odd length T (125 at clip_len 16000), one thread each, the row staged through LDS: (1) every segment
 * runs from the zero state and keeps its final state; (2) one thread carries the n-vector across the segments,
 * z_in(s + 1) = M z_in(s) + z_zero-state(s), M the n x n zero-input transition of T steps, computed on the host in float64; (3) every
 * segment runs again from its true initial state.  The scheme is exact in exact arithmetic for any pole position (nothing is
 * truncated); in fp32 the result is the sequential recurrence from an initial state that carries the rounding of step (2).
 * dmad_wave_iir_vjp:  g_x = flip(lfilter(b, a, flip(g_y * m))),  m[t] = 1 where the UNCLAMPED forward output lies in [lo, hi] (a NaN
 * is outside), the forward recomputed into the engine workspace (B <= max_batch); y_or_null optionally receives the clamped forward. */
int dmad_wave_iir(dmad_engine* e, const float* x, int32_t B, const float* b, const float* a, int32_t order, float lo, float hi, float* y,
                  dmad_stream s);
int dmad_wave_iir_vjp(dmad_engine* e, const float* x, const float* g_y, int32_t B, const float* b, const float* a, int32_t order, float lo,
                      float hi, float* g_x, float* y_or_null, dmad_stream s);

/* One defense as dmad_defense_query_logits runs it.  All pointers are HOST arrays.  struct_size = sizeof(dmad_wave_defense). */
enum dmad_wave_kind { DMAD_WAVE_AS = 0, DMAD_WAVE_MS = 1, DMAD_WAVE_DS = 2, DMAD_WAVE_IIR = 3 };
typedef struct dmad_wave_defense {
    int32_t struct_size;
    int32_t kind;                   /* enum dmad_wave_kind */
    int32_t window;                 /* AS, MS */
    int32_t order;                  /* IIR */
    const float* down_ker;          /* DS: [down_phases][down_taps], clip_len -> down_len */
    int32_t down_phases, down_taps, down_stride, down_width, down_len;
    int32_t up_phases, up_taps, up_stride, up_width;
    const float* up_ker;            /* DS: [up_phases][up_taps], down_len -> clip_len */
    const float* b;                 /* IIR: [order + 1] */
    const float* a;
    float lo, hi;                   /* IIR: clamp range */
} dmad_wave_defense;

/* dmad_query_logits with a baseline defense in the purifier's place (adaptive_attack_eval.py:190-201 builds
 * AcousticSystem(classifier, transform, TimeDomainDefense | FreqDomainDefense)): row i = r * B + b is clip x[b] through
 * defense -> mel dB -> fp32 classifier -> arg-max, max_batch rows at a time.  The defenses are deterministic, so the repeats are copies;
 * the layout is kept for the callers of dmad_query_logits.  logits: [repeats * B][num_classes]; decisions: optional int32. */
int dmad_defense_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, const dmad_wave_defense* d, float* logits,
                              int32_t* decisions, dmad_stream s);

/* ---- M5, the raw-waveform classifier (audio_models/M5/M5Net.py:4-38): a part of its own beside the WaveNet, the spectrogram
 * classifier and the UNet; an engine may hold VGG19_bn or ResNeXt29 AND M5.  In the reference driver it makes the system
 * AcousticSystem(classifier, transform=None, ...) (adaptive_attack_eval.py:121-122, 169-170): waveform in, log-probabilities out, no mel front-end.
 *
 * Weights (dmad_load_weight, BatchNorm folded on the host: s = gamma / sqrt(var + 1e-5), shift = beta + (bias - mean) * s):
 *   m5.conv1.w [32][1][k1]   m5.conv2.w [32][32][3]   m5.conv3.w [64][32][3]   m5.conv4.w [64][64][3]   m5.scale<i> / m5.shift<i> [C_i], i = 1..4
 *   m5.fc.w [n_output][64]   m5.fc.b [n_output]   m5.stride [1] (conv1's stride, as a float)
 * dmad_finalize_weights packs them.  Supported: n_input = 1, stride = 16, n_channel = 32, first_kernel_size k1 = 80 or 160,
 * n_output <= 64 and the engine's clip_len; anything else is DMAD_ERR_SHAPE with a message that names the field.  M5 is exact fp32 on
 * every engine precision.  Its kernels keep every activation of a clip in the LDS of one workgroup and use NO workspace in device
 * memory: nothing is reserved at finalisation (whatever max_batch is) and no call allocates.  Every sum runs in a fixed order inside
 * the clip's workgroup, so a clip's bits do not depend on B, on its row or on the call.  Any B >= 1 (no max_batch limit).
 * x must be 16-byte aligned (the clip is read 16 bytes at a time; clip_len is a multiple of 128, so every row then is):
 * DMAD_ERR_INVALID otherwise.
 * All of the calls below return DMAD_ERR_STATE before the M5 weights are finalised.
 *
 * dmad_m5_logits (M5Net.py:21-38 M5.forward in eval mode):  x device fp32 [B][clip_len] -> logp [B][n_output], the log-probabilities;
 * decisions: optional int32 [B], the arg-max (the first maximum wins).
 *
 * dmad_m5_vjp (what loss.backward() runs through M5.forward, white_box_attack.py:438, 562):  g_x = (d logp / d x)^T g_logp, [B][clip_len],
 * for g_logp [B][n_output].  The forward is recomputed in the same launch and only the decision of each pooled unit is kept (its
 * arg-max among the 4 frames, the first maximum winning, and whether that maximum is > 0: ReLU'(0) = 0).  logp: optional, bit-identical
 * to dmad_m5_logits.  First order only, no weight gradients.
 *
 * dmad_m5_tape (test hook):  layer 1..4 -> pooled [B][C][T] floats, that block's pooled post-ReLU map, and decisions [B][C][T] bytes,
 * arg | on << 2, both written by the launch dmad_m5_vjp makes (C, T: 32 x 247 / 32 x 61 / 64 x 14 / 64 x 3 at k1 = 160, clip_len 16000). */
int dmad_m5_logits(dmad_engine* e, const float* x, int32_t B, float* logp, int32_t* decisions, dmad_stream s);
int dmad_m5_vjp(dmad_engine* e, const float* x, int32_t B, const float* g_logp, float* g_x, float* logp, dmad_stream s);
int dmad_m5_tape(dmad_engine* e, const float* x, int32_t B, int32_t layer, float* pooled, uint8_t* decisions, dmad_stream s);

/* dmad_rs_smooth_votes for RobustCertificate(M5, transform=None, denoiser=None) (certified_robust.py:34-67 with `denoiser is None`):
 * sample i's input clip + delta_i, with the same delta / Philox keys and rounding, goes through M5; counts: device int64[n_output],
 * ACCUMULATED into at each sample's first maximum; logp_out: optional [n][n_output], dmad_m5_logits of the noisy clip bit for bit.
 * One workgroup per sample adds the noise while it copies the clip into LDS: the n noisy clips never exist in device memory.  Needs
 * the M5 weights and nothing else; no workspace, no max_batch limit; a fixed number of samples per launch, which the result does not
 * depend on.  clip and delta 16-byte aligned. */
int dmad_m5_rs_smooth_votes(dmad_engine* e, const float* clip, float sigma, int64_t n, uint64_t seed, uint64_t sample0,
                            const float* delta, int64_t* counts, float* logp_out, dmad_stream s);

/* dmad_query_logits with M5 in the place of  mel dB -> classifier  (EOT.forward on AcousticSystem(M5, None, defender),
 * robustness_eval/_EOT.py:30-64): the same arguments, samplers 0 / 1 / 2, row layout and Philox keys; logits: [repeats * B][n_output]
 * log-probabilities.  Samplers 1 and 2 return DMAD_ERR_STATE when the engine holds no WaveNet. */
int dmad_m5_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, int32_t sampler, int32_t t_star, float c_a, float c_b,
                         const float* c_eps, const float* c_div, const float* c_sig, uint64_t seed, uint64_t sample0, float* logits,
                         int32_t* decisions, dmad_stream s);
/* dmad_defense_query_logits with M5 in the place of  mel dB -> classifier  (adaptive_attack_eval.py:169-170 with a Time / FreqDomainDefense). */
int dmad_m5_defense_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, const dmad_wave_defense* d, float* logits,
                                 int32_t* decisions, dmad_stream s);

/* ---- KWS, the attention-CRNN keyword spotter (audio_models/RCNN_KWS/model.py:66-114 KWSModel): a part of its own beside the WaveNet,
 * the spectrogram classifier, the UNet and M5.  A dB mel spectrogram [B][32][T] in, 4 log-probabilities out: depthwise
 * Conv1d(32,32,5,stride 2) -> pointwise Conv1d(32,64,1,stride 8) -> 2-layer bidirectional GRU(64), h0 = 0 -> additive attention over
 * time -> bias-free Linear -> log_softmax.  Its mel front-end is not on the engine.
 *
 * Weights (dmad_load_weight): the 24 tensors of the module's state dict in their own shapes, each under "kws." + its key
 *   kws.CRNN_model.sepconv.0.weight [32][1][5]  .0.bias [32]  .1.weight [64][32][1]  .1.bias [64]
 *   kws.CRNN_model.gru.weight_ih_l<l><sfx> [192][64 or 128]  weight_hh_l<l><sfx> [192][64]  bias_ih_l<l><sfx> / bias_hh_l<l><sfx> [192],
 *     l = 0, 1 and <sfx> = "" or "_reverse" (torch's gate order r, z, n)
 *   kws.attn_layer.Wx_b.weight [128][128]  .bias [128]   kws.attn_layer.Vt.weight [1][128]   kws.apply_attn.U.weight [4][128]
 * and two arrays for what no tensor shows:  kws.kernel_size [2] = (20, 5)   kws.stride [2] = (8, 2)   (as floats).
 * dmad_finalize_weights packs them.  Supported: in_size 32, hidden_size 64, kernel_size (20, 5), stride (8, 2), 2 GRU layers, 2
 * directions, 4 classes; anything else is DMAD_ERR_SHAPE with a message that names the field.  KWS is exact fp32 on every engine
 * precision.  One workgroup serves one row and keeps its activations in LDS: NO workspace in device memory, nothing reserved at
 * finalisation, no call allocates.  Every sum runs in a fixed order inside the row's workgroup, so a row's bits do not depend on B, on
 * its row index or on the call.  Any B >= 1 (no max_batch limit); 5 <= T <= 644 (40 GRU steps: what the LDS of one CU holds), any
 * other T is DMAD_ERR_SHAPE; rows need no more than 4-byte alignment.  All three calls return DMAD_ERR_STATE before the KWS weights
 * are finalised.  Both checks are made on the host, before any launch.
 *
 * dmad_kws_logits (KWSModel.forward with hidden = None):  spec device fp32 [B][32][T] -> logp [B][4]; decisions: optional int32 [B],
 * the arg-max (the first maximum wins).
 *
 * dmad_kws_vjp (what loss.backward() runs through KWSModel.forward):  g_spec = (d logp / d spec)^T g_logp, [B][32][T], for g_logp
 * [B][4].  The forward is recomputed in the same launch.  Every element of g_spec is written: step j of the GRU reads frames
 * 16 j .. 16 j + 4 only, and every other frame gets an exact 0.  logp: optional, bit-identical to dmad_kws_logits.  First order only,
 * no weight gradients.
 *
 * dmad_kws_tape (test hook), written by the launch dmad_kws_vjp makes, T2 = ((T - 5) / 2) / 8 + 1 steps:  stage 0 the sepconv output
 * [B][T2][64]; stages 1 and 2 the output of GRU layer 0 and 1, [B][T2][128], forward direction first; stage 3 the attention scores
 * e, [B][T2]. */
int dmad_kws_logits(dmad_engine* e, const float* spec, int32_t B, int32_t T, float* logp, int32_t* decisions, dmad_stream s);
int dmad_kws_vjp(dmad_engine* e, const float* spec, int32_t B, int32_t T, const float* g_logp, float* g_spec, float* logp, dmad_stream s);
int dmad_kws_tape(dmad_engine* e, const float* spec, int32_t B, int32_t T, int32_t stage, float* out, dmad_stream s);

/* ---- The keyword spotter's mel front-end (kws_adaptive_attack_eval.py:74-76: torchaudio MelSpectrogram(sample_rate=16000, n_mels=32)
 * then AmplitudeToDB(stype='power')) for clips of ANY length L, an argument of every call: n_fft = win_length = 400,
 * hop 200, periodic Hann, center=True with reflect padding of 200 samples, 201 one-sided bins, power 2, htk mel scale without norm
 * between 0 and 8000 Hz, 10 log10(max(., 1e-10)).  T = 1 + L / 200 frames.  Exact fp32 on every engine; its constants are built at
 * the first call (no with_classifier, no weights) and dmad_device_bytes counts them.  Nothing is sized by max_batch: any B >= 1.  A
 * frame's bits depend on its own 400 samples only -- not on B, the row, the call, nor on which frames are computed beside it.
 * Refusals are made on the host before any launch and name L: DMAD_ERR_SHAPE for L < 201 (the reflect padding mirrors 200 samples)
 * in the three mel calls, and for L outside 800 .. 128 799 (T outside 5 .. 644) in the wave and query calls, which return
 * DMAD_ERR_STATE before the KWS weights are finalised.
 *
 * dmad_kws_mel_power (MelSpectrogram(sample_rate=16000, n_mels=32)(x), l.74):  x device fp32 [B][L] -> out [B][32][T], one launch.
 * dmad_kws_mel_db (Wave2Spect(x), l.76: ... then AmplitudeToDB('power')):  the same in dB.
 *
 * dmad_kws_mel_db_vjp (what loss.backward() runs through Wave2Spect):  g_x [B][L] = (d spec / d x)^T g_spec for g_spec [B][32][T], one
 * launch that recomputes the forward; no atomics, every element of g_x is written (the buffer need not be cleared), and the order of
 * every sum is fixed (frames ascending, direct before reflected).  spec: optional, bit-identical to dmad_kws_mel_db. */
int dmad_kws_mel_power(dmad_engine* e, const float* x, int32_t B, int32_t L, float* out, dmad_stream s);
int dmad_kws_mel_db(dmad_engine* e, const float* x, int32_t B, int32_t L, float* out, dmad_stream s);
int dmad_kws_mel_db_vjp(dmad_engine* e, const float* x, int32_t B, int32_t L, const float* g_spec, float* g_x, float* spec, dmad_stream s);
/* dmad_kws_wave_logits (AS_MODEL(waveforms, False), l.230: Classifier(Wave2Spect(x))):  x [B][L] -> logp [B][4] (decisions: optional
 * int32 [B]), bit-identical to dmad_kws_logits on dmad_kws_mel_db.  Only the frames KWSModel reads, 16 j .. 16 j + 4 per GRU step j,
 * are computed; the spectrogram lives in an engine-owned scratch of 512 rows (42 MB, and as much for its gradient), allocated at the
 * first call, and B is walked in passes of 512 rows (the pass size cannot change a bit). */
int dmad_kws_wave_logits(dmad_engine* e, const float* x, int32_t B, int32_t L, float* logp, int32_t* decisions, dmad_stream s);
/* dmad_kws_wave_vjp (loss.backward() of white_box_attack.py through AS_MODEL without a defender, l.103, 250):  g_x [B][L] =
 * (d logp / d x)^T g_logp: the KWS VJP, then the mel VJP on the read frames; bit-identical to dmad_kws_mel_db_vjp on dmad_kws_vjp.
 * logp: optional, bit-identical to dmad_kws_wave_logits. */
int dmad_kws_wave_vjp(dmad_engine* e, const float* x, int32_t B, int32_t L, const float* g_logp, float* g_x, float* logp, dmad_stream s);
/* dmad_m5_query_logits with  mel dB -> KWSModel  in the place of M5 (kws_adaptive_attack_eval.py:186-204: FAKEBOB / SirenAttack
 * queries of AS_MODEL with the DiffWave defender, l.109-111); L is the engine's clip_len. */
int dmad_kws_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, int32_t sampler, int32_t t_star, float c_a, float c_b,
                          const float* c_eps, const float* c_div, const float* c_sig, uint64_t seed, uint64_t sample0, float* logits,
                          int32_t* decisions, dmad_stream s);
/* dmad_m5_defense_query_logits the same way (kws_adaptive_attack_eval.py:117-136 with a Time / FreqDomainDefense as the defender). */
int dmad_kws_defense_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, const dmad_wave_defense* d, float* logits,
                                  int32_t* decisions, dmad_stream s);

/* counts[argmax_c logits[b][c]] += 1 (first maximum wins) — certified_robust.py:59-65. */
int dmad_vote(dmad_engine* e, const float* logits, int32_t B, int64_t* counts, dmad_stream s);

/* Test hooks: raw Philox4x32-10 words / N(0,1) draws of the generator used above. */
int dmad_philox_raw(dmad_engine* e, uint64_t seed, uint64_t sample, uint32_t stream, uint32_t nblocks, uint32_t* out, dmad_stream s);
int dmad_philox_normal(dmad_engine* e, uint64_t seed, uint64_t sample0, uint32_t stream, int32_t B, float* z, dmad_stream s);

/* Timing hook for bench.py: runs `iters` launches of residual layer `layer` (bf16 path) on the resident
 * buffers between two HIP events recorded on `s` and returns the average milliseconds per launch. */
int dmad_time_layer(dmad_engine* e, int32_t layer, int32_t B, int32_t iters, float* ms_per_launch, dmad_stream s);

/* Live timing of the dominant kernel (the fused residual layer, wn_layer_bf16) for bench.py's roofline:
 * after dmad_profile_layers(e, max_launches > 0) every non-final layer launch of the bf16 path is
 * bracketed by a HIP event pair recorded on the launch stream (until max_launches pairs are used);
 * dmad_profile_read() waits for the last pair, returns the summed elapsed milliseconds and the number of
 * launches, and switches the bracketing off. */
int dmad_profile_layers(dmad_engine* e, int32_t max_launches);
int dmad_profile_read(dmad_engine* e, float* total_ms, int32_t* launches);
/* The same for the launches of the tail kernel (wn_final: skip GEMM over the gate store + final convs) bracketed since
 * dmad_profile_layers(); call it BEFORE dmad_profile_read (which switches the bracketing off). */
int dmad_profile_read_final(dmad_engine* e, float* total_ms, int32_t* launches);

/* Test hook of the f16 conv-GEMM family (csrc/gemm_h16.hip: the kernels behind the UNet's and ResNeXt29's 16-bit tiers), standalone —
 * no engine state is read.  NHWC convolution  out[n][g*M + m] = relu?( sum_tap sum_k w[g][tap][m][k] x[pixel(n, tap)][g*K + k] + bias[g*M + m]
 * + res[n][g*M + m] )  with f16 operands and fp32 accumulation.  x: device f16 [B][H][H][ldx]; x2 / ksplit: optional second input
 * map holding channels [ksplit, K) (the UNet's th.cat read in place; x then has ksplit channels per pixel); w: device f16
 * [groups][taps][M][K] (taps 9 = 3x3 with zero padding 1, or 1); bias: fp32 [groups * M] or NULL; res16: optional f16 residual
 * [N][groups * M]; out32 / out16: fp32 map and / or f16 twin [N][groups * M], N = B * Ho * Ho, Ho = (H - 1) / stride + 1.
 * M and K are per group.  Which of the family's kernels serves a shape is the launcher's choice (the product's).
 * This and every other standalone op export below prepares its kernels for the current device on first use (no engine is needed before). */
int dmad_conv_h16(const uint16_t* x, const uint16_t* x2, int32_t ksplit, const uint16_t* w, const float* bias, const uint16_t* res16,
                  int32_t B, int32_t H, int32_t M, int32_t K, int32_t taps, int32_t stride, int32_t groups, int32_t relu,
                  float* out32, uint16_t* out16, dmad_stream s);
/* The UNet's Upsample (F.interpolate(scale_factor=2, mode="nearest") + 3x3 conv, unet.py:72-79) as ONE launch of the family's
 * slice-resident form: x_half is the HALF-resolution f16 map [B][H/2][H/2][K], the conv output is [B][H][H][M] (H even; stats: optional
 * GroupNorm statistics slab as below).  DMAD_ERR_STATE when the shape is not served by that form (fewer tiles than CUs, M % 256, maps wider
 * than 32 pixels ...: the product then materialises the x2 map and calls the plain conv).  Test hook like dmad_conv_h16. */
int dmad_conv_h16_up2(const uint16_t* x_half, const uint16_t* w, const float* bias, const uint16_t* res16, int32_t B, int32_t H, int32_t M, int32_t K,
                      float* out32, uint16_t* out16, float* stats, dmad_stream s);
/* The same with the consumer's GroupNorm statistics accumulated in the epilogue: stats [N / blk][groups * M / 4][2] fp32 = (sum, sum of
 * squares) of the f16-rounded outputs per block of blk = 64 pixels (16 when Ho * Ho == 16) and 4-channel quad — and the one-pass
 * GroupNorm32 + SiLU (+ scale-shift) that consumes them (nn.py:15-17, unet.py:186-199 on the 16-bit tier):
 * y = SiLU?(GroupNorm_32groups(cat(x, x2)) * gamma + beta [* (1 + ss[c]) + ss[C + c]]), x / x2 f16 NHWC maps [B][HW][c1 | C - c1] with
 * their slabs st / st2 (x2, st2 NULL: one map), y16 f16 or y32 fp32 [B][HW][C].  Test hooks like dmad_conv_h16. */
int dmad_conv_h16_stats(const uint16_t* x, const uint16_t* w, const float* bias, const uint16_t* res16, int32_t B, int32_t H, int32_t M, int32_t K,
                        int32_t taps, int32_t stride, uint16_t* out16, float* stats, dmad_stream s);
int dmad_groupnorm16_apply(const uint16_t* x, const float* st, const uint16_t* x2, const float* st2, int32_t c1, const float* gamma,
                           const float* beta, const float* ss, int32_t silu, int32_t B, int32_t HW, int32_t C, uint16_t* y16, float* y32,
                           dmad_stream s);

/* Test hooks of what sits between the GEMMs of the UNet's 16-bit tier (csrc/unet_ops.hip), standalone (no engine state is read).  Each
 * calls the launcher the engine path calls; a shape the launcher does not serve is DMAD_ERR_INVALID.
 *
 * dmad_qkv_attention_h16: QKVAttention on f16 maps — qkv16 [B][T][heads * 192] with the head-major split (head h: q, k, v = 64 channels
 *   each from h * 192), out16 [B][T][heads * 64]; both products on the f16 matrix cores, fp32 scores / softmax / accumulation.  T = 16, 64
 *   or 256.
 * dmad_groupnorm16: the two-pass GroupNorm32 (+ scale-shift, + SiLU) of an f16 map x16 [B][HW][c1] (| x2_16 [B][HW][C - c1]; NULL: one
 *   map) — the form the tier falls back to when a statistics slab is missing; y16 (f16) or y32 (fp32) [B][HW][C], exactly one of them.
 *   C % 128 == 0, C <= 512, c1 % 4 == 0.
 * dmad_conv1ch_3x3: the first layer, 1 -> Cout 3x3 conv with zero padding and bias on 32 x 32 maps: in [B][32][32], w [Cout][9], out32 /
 *   out16 [B][1024][Cout] (at least one), stats (optional) the GroupNorm statistics slab [B * 16][Cout / 4][2] of the f16-rounded outputs
 *   (64-pixel blocks = pairs of image rows).  Cout <= 128; with stats Cout % 4 == 0.
 * dmad_conv3x3_c128_to1: the last layer, 128 -> 1 3x3 conv with zero padding and bias: in [B][1024][128], w [9][128] (tap-major), bias
 *   [1], out [B][1024].  g_in != NULL ([B][1024], not out): out = alpha * g_in - gamma * (that conv), each product and the difference
 *   rounded once (the adjoint update of a reverse VP-SDE step).
 * dmad_conv3x3_c128_to1_h16: the same conv on an f16 map in16 [B][1024][128] with fp32 weights (the 16-bit tier's last layer).
 * dmad_upsample2x: nearest-neighbour x2 of an NHWC map in [B][H][H][C] -> out [B][2H][2H][C], fp32 (C % 4 == 0) or, with is_f16, f16
 *   (C % 8 == 0). */
int dmad_qkv_attention_h16(const uint16_t* qkv16, int32_t B, int32_t T, int32_t heads, uint16_t* out16, dmad_stream s);
int dmad_groupnorm16(const uint16_t* x16, const uint16_t* x2_16, int32_t c1, const float* gamma, const float* beta, const float* ss,
                     int32_t silu, int32_t B, int32_t HW, int32_t C, uint16_t* y16, float* y32, dmad_stream s);
int dmad_conv1ch_3x3(const float* in, const float* w, const float* bias, int32_t B, int32_t Cout, float* out32, uint16_t* out16, float* stats,
                     dmad_stream s);
int dmad_conv3x3_c128_to1(const float* in, const float* w, const float* bias, int32_t B, const float* g_in, float alpha, float gamma,
                          float* out, dmad_stream s);
int dmad_conv3x3_c128_to1_h16(const uint16_t* in16, const float* w, const float* bias, int32_t B, float* out, dmad_stream s);
int dmad_upsample2x(const void* in, int32_t B, int32_t H, int32_t C, int32_t is_f16, void* out, dmad_stream s);

/* Test hooks of the split-f16 conv GEMM (csrc/gemm_f32.hip, gemm_x3_kernel in its NHWC form: the kernel behind the UNet's middle tier),
 * standalone.  dmad_split_f16: y = the split-f16 storage form of the n fp32 values x (n % 4 == 0; hi = f16(v), lo = f16((v - hi) 2^11), four
 * values per 16-byte chunk: the bytes of four floats; x == y allowed).  dmad_conv_x3: NHWC convolution of split-format operands — x
 * [B][H][H][groups * K] (or, dense only, x | x2 with ksplit channels in x), w [groups][taps][M][K] (taps 9 = 3x3 zero padding 1, or 1),
 * fp32 bias [groups * M], optional residual [N][groups * M] (fp32, or a split-format map with res_split), stride 1 / 2, optional ReLU —
 * every product as three f16 MFMAs; out [N][groups * M] fp32, or in the split format (out_split).  M and K are per group;
 * M % 128 == 0, K % 32 == 0 (ksplit % 32 == 0). */
int dmad_split_f16(const float* x, int64_t n, float* y, dmad_stream s);
int dmad_conv_x3(const float* x, const float* x2, int32_t ksplit, const float* w, const float* bias, const float* res, int32_t B, int32_t H,
                 int32_t M, int32_t K, int32_t taps, int32_t stride, int32_t groups, int32_t relu, int32_t out_split, int32_t res_split, float* out,
                 dmad_stream s);

/* Test hooks of the exact-fp32 tier, standalone (no engine state is read): the ops every vector-Jacobian product is built from, one at a
 * time.  Each calls the launcher and the argument builders the engine paths call; a shape no kernel serves is DMAD_ERR_INVALID.
 *
 * dmad_conv_f32: NHWC convolution or plain GEMM on the fp32 matrix-core path of csrc/gemm_f32.hip (not the split-f16 one):
 *   out[n][g*M + m] = relu?( scale[g*M + m] * sum_tap sum_k w[g][tap][m][k] x[pixel(n, tap)][g*K + k] + shift[g*M + m] + res[n][g*M + m] )
 * x [B][H][H][groups * K] (or, dense only, x | x2 with ksplit channels in x; M > 64), w [groups][taps][M][K] (taps 9 = 3x3 with zero padding 1,
 * or 1), scale / shift [groups * M] or NULL, res [N][groups * M] or NULL, N = B * Ho * Ho, Ho = (H - 1) / stride + 1; M and K per group,
 * K % 16 == 0 (ksplit % 16 == 0).  H = 0: the row form the Linear layers and the mel DFT use — x [B][K], one tap, out [B][M].  slab /
 * slab_floats / n_ref: optional split-K workspace and the reference row count the split count is derived from (0: N), as the engine
 * passes them.  choice (optional, 4 ints): what the launcher chose — tile height (64 / 128), 1 for the 64 x 32 narrow tile with the
 * 8-slot ring, 1 for the two-part instantiation, the split count (> 1: partial sums through the slab and the reduce kernel).
 *
 * dmad_conv_f32_vjp: the data gradient g_y -> g_x of such a conv (w in the forward layout above, M / K / H / stride the FORWARD conv's)
 * through the engine's own sequence: the weight image packed into wT, the optional zero-dilation, the GEMM.
 *   form 0  the UNet's convs: wT [taps][K][M] with flipped taps; stride 2 dilates g_y into work [B][H][H][M]; acc (optional, g_x's shape)
 *           is added in the GEMM's epilogue.
 *   form 1  the UNet's Upsample (interpolate x2 + 3x3 conv at 2H; H: the half resolution): g_y [B][2H][2H][M], the conv's gradient at 2H
 *           in work [B][2H][2H][K], then g_x [B][H][H][K] = its 2x2 sums (+ acc).
 *   form 2  ResNeXt29's convs with the eval-mode BN scale [groups * M] folded into the image: a dense 1x1 (wT [K][ldt], ldt = 0 -> M, or a
 *           multiple of 16 >= M whose extra rows are zero; g_y then has ldt channels per pixel) or the 8-group 3x3 with M = K (wT
 *           [g][8 - tap][k][m]).  mask_y (optional, g_y's shape): g_y is first masked by mask_y > 0 into gm (the ReLU backward).  Stride 2:
 *           the 3x3 runs on the zero-dilated gradient (work [B][H][H][8 * M]); the 1x1 shortcut runs at Ho (work [B][Ho][Ho][K]) and is
 *           scattered into the even pixels of g_x.  acc: the GEMM's residual (not with the stride-2 1x1).
 *   form 3  VGG19_bn's dense 3x3 convs (stride 1, one group, K % 16 == 0) with the eval-mode BN scale [M] folded into the image: wT
 *           [8 - tap][k][m] = w[tap][m][k] * scale[m]; mask_y (optional, g_y's shape) as in form 2; no acc, no ldt.
 *   form 4  WideResNet's dense convs: the 3x3 (image as form 3, scale optional) or the 1x1 (wT [K][M]) at stride 1 or 2.  Stride 2: the 3x3
 *           runs on the zero-dilated gradient (work [B][H][H][M]); the 1x1 runs at Ho (work [B][Ho][Ho][K]) and is scattered into the even
 *           pixels of g_x.  acc: the GEMM's residual (not with the stride-2 1x1); mask_y as in form 2; no ldt.
 * M % 16 == 0, K % 4 == 0; H even with stride 2.  wT, gm and work are left as the kernels wrote them (the tests read them). */
int dmad_conv_f32(const float* x, const float* x2, int32_t ksplit, const float* w, const float* scale, const float* shift, const float* res,
                  int32_t B, int32_t H, int32_t M, int32_t K, int32_t taps, int32_t stride, int32_t groups, int32_t relu, float* slab,
                  int64_t slab_floats, int64_t n_ref, float* out, int32_t* choice, dmad_stream s);
int dmad_conv_f32_vjp(const float* g_y, const float* w, const float* scale, const float* mask_y, const float* acc, int32_t B, int32_t H,
                      int32_t M, int32_t K, int32_t taps, int32_t stride, int32_t groups, int32_t form, int32_t ldt, float* wT, float* gm,
                      float* work, float* g_x, dmad_stream s);
/* GroupNorm32 in fp32 and its backward (csrc/unet_ops.hip, csrc/unet_vjp.hip):  y = SiLU?(GN(cat(x, x2)) * gamma + beta [* (1 + ss[c]) +
 * ss[C + c]]) over [B][HW][C], x holding c1 channels and x2 the rest (x2 NULL: one map).  Forward: C % 128 == 0, C <= 512, c1 % 4 == 0, maps
 * up to 32 x 32 x 384 (16 float4s per thread); split: y is written in the split-f16 storage format of dmad_split_f16 (the operand form of
 * the split-f16 middle tier).  Backward: C % 32 == 0, any 0 < c1 < C; gx / gx2 = the gradient's two parts (+ add + add2, [B][HW][C]). */
int dmad_groupnorm_f32(const float* x, const float* x2, int32_t c1, const float* gamma, const float* beta, const float* ss, int32_t silu,
                       int32_t B, int32_t HW, int32_t C, int32_t split, float* y, dmad_stream s);
int dmad_groupnorm_bwd(const float* x, const float* x2, int32_t c1, const float* gamma, const float* beta, const float* ss, int32_t silu,
                       const float* gy, const float* add, const float* add2, int32_t B, int32_t HW, int32_t C, float* gx, float* gx2,
                       dmad_stream s);
/* QKVAttention in fp32 and its backward: qkv [B][T][heads * 192] with the head-major split (head h: q, k, v = 64 channels each from h * 192),
 * out / go [B][T][heads * 64], gqkv like qkv.  T = 16, 64 or 256; any other T is DMAD_ERR_INVALID.  split: out is written in the split-f16
 * storage format of dmad_split_f16. */
int dmad_qkv_attention_f32(const float* qkv, int32_t B, int32_t T, int32_t heads, int32_t split, float* out, dmad_stream s);
int dmad_qkv_attention_bwd(const float* qkv, const float* go, int32_t B, int32_t T, int32_t heads, float* gqkv, dmad_stream s);
/* The two ends of ResNeXt29's backward walk.  dmad_rx_head_bwd: gz [B][HW][C] = (y > 0) * (W^T g_logits)[c] / HW — FC [ncls][C], average
 * pool and the last ReLU.  dmad_rx_conv1_bwd: gspec [B][32][32] = the 1 <- 64 3x3 conv (w [64][9], BN scale [64]) of (a > 0) * g, both
 * [B][32][32][64]. */
int dmad_rx_head_bwd(const float* g_logits, const float* W, const float* y, int32_t B, int32_t ncls, int32_t HW, int32_t C, float* gz, dmad_stream s);
int dmad_rx_conv1_bwd(const float* g, const float* a, const float* w, const float* scale, int32_t B, float* gspec, dmad_stream s);
/* VGG19_bn's 2x2 max-pool and the ReLU in front of it, backward: y [B][H][H][C] the saved post-ReLU map, g [B][H/2][H/2][C] -> gpre
 * [B][H][H][C], every element written once: a window's g at its first maximum in scan order (top-left, top-right, bottom-left,
 * bottom-right) where that maximum is > 0, zero elsewhere.  H even, C % 4 == 0. */
int dmad_vgg_pool_relu_bwd(const float* g, const float* y, int32_t B, int32_t H, int32_t C, float* gpre, dmad_stream s);
/* WideResNet's small kernels (csrc/wrn.hip), NHWC maps of n_px pixels x C channels (C % 4 == 0).  dmad_wrn_preact: out = max(scale[c] * x +
 * shift[c], 0).  dmad_wrn_preact_bwd: gx = (res ? res : 0) + (o > 0 ? scale[c] * g : 0), o the saved post-ReLU map (-0.0 and negatives
 * give 0), res optional.  dmad_wrn_stem: spec [B][32][32] -> out [B][32][32][16], the 1 -> 16 3x3 conv (w [16][9], zero padding, no BN, no
 * ReLU).  dmad_wrn_stem_bwd: gspec [B][32][32] = sum over taps (ky, kx ascending) and c ascending of w[c][ky][kx] * g at (y + 1 - ky,
 * x + 1 - kx), g [B][32][32][16]. */
int dmad_wrn_preact(const float* x, const float* scale, const float* shift, int64_t n_px, int32_t C, float* out, dmad_stream s);
int dmad_wrn_preact_bwd(const float* g, const float* o, const float* scale, const float* res, int64_t n_px, int32_t C, float* gx, dmad_stream s);
int dmad_wrn_stem(const float* spec, const float* w, int32_t B, float* out, dmad_stream s);
int dmad_wrn_stem_bwd(const float* g, const float* w, int32_t B, float* gspec, dmad_stream s);
/* DenseNet-BC-100-12's kernels (csrc/densenet.hip), one hook each.  pre(s, x, b) = max(fmaf(s, x, b), 0) with a NaN kept and
 * -0.0 made +0.0: the one pre-activation function of the forward, the backward's masks and the tape reader.  Maps are NHWC with a pitch
 * (floats per pixel) >= their width; no kernel reads or writes a channel outside the widths named here.
 * dmad_dn_pw: out[p * ldo + m] = epi(sum over k < K ascending of A[m][k] * pre(s_in[k], x[p * ldx + k], b_in[k])), m < M, p < n_px (any
 *   count); A [M][K4], K4 = K rounded up to 4, zero columns behind K; epi = pre(s_out[m], ., b_out[m]), or the identity when s_out and
 *   b_out are NULL.  K and ldx even.  The bottleneck's 1x1 (M = 48) and a transition's (M = 108 / 150).
 * dmad_dn_pw_bwd: v = pre(s1[m], x[p * ldx + m], b1[m]) > 0 ? s1[m] * sum over k < K ascending of A[m][k] * g'[p][k] : 0, m < M;
 *   out[p * ldo + m] = add ? out[p * ldo + m] + v : v.  g'[p][k] = g[p * ldg + k], or with pool = 1 a quarter of g at the pixel of the
 *   half-resolution map whose 2x2 window holds p (H: the resolution of p; n_px whole maps).  A [M][K4] as above.  K and ldg even.
 * dmad_dn_growth: stream[p * ld + off + j] = sum over taps (ky, kx ascending), then c < 48 ascending, of A[j][tap * 48 + c] * h[(p + tap)
 *   * 48 + c] with zero padding, j < 12; A [16][432], rows 12..15 zero; h [B][H][H][48], H in {8, 16, 32}; ld and off even (dense3's slices start at 150 + 12 i: no multiple of 4).
 * dmad_dn_growth_bwd: gh[p * 48 + c] = h[p * 48 + c] > 0 ? s2[c] * sum over taps, then j < 12, of A[c][tap * 12 + j] * g[(p + tap) * ld +
 *   off + j] : 0; A [48][108], the tap-flipped transpose A[c][tap * 12 + j] = w[j][c][8 - tap].
 * dmad_dn_stem / _stem_bwd: the 1 -> 24 3x3 conv (w [24][9]) into channels [0, 24) of a stream, and its backward, as dmad_wrn_stem's.
 * dmad_dn_pool: out[q * ldo + c] = 0.25 * (((tl + tr) + bl) + br) of the 2x2 window of t [B][H][H][ldt], c < C.
 * dmad_dn_preact: out[p * C + c] = pre(scale[c], x[p * ldx + c], shift[c]).
 * dmad_dn_head: logits[b][k] = fcb[k] + sum over c < C ascending of fcw[k][c] * mean over the HW pixels (ascending) of pre(bns[c], x, bnb[c]);
 *   HW a power of two, C <= 384.  dmad_dn_head_bwd: g[p * ldg + c] = pre(bns[c], x[p * ldx + c], bnb[c]) > 0 ? (sum over k ascending of
 *   fcws[k][c] * g_logits[b][k]) / HW : 0. */
int dmad_dn_pw(const float* A, int32_t M, int32_t K, const float* x, int32_t ldx, int64_t n_px, const float* s_in, const float* b_in, const float* s_out,
               const float* b_out, float* out, int32_t ldo, dmad_stream s);
int dmad_dn_pw_bwd(const float* A, int32_t M, int32_t K, const float* g, int32_t ldg, int64_t n_px, int32_t pool, int32_t H, const float* x, int32_t ldx,
                   const float* s1, const float* b1, float* out, int32_t ldo, int32_t add, dmad_stream s);
int dmad_dn_growth(const float* A, const float* h, int32_t B, int32_t H, float* stream, int32_t ld, int32_t off, dmad_stream s);
int dmad_dn_growth_bwd(const float* A, const float* g, int32_t ld, int32_t off, const float* h, const float* s2, int32_t B, int32_t H, float* gh,
                       dmad_stream s);
int dmad_dn_stem(const float* spec, const float* w, int32_t B, float* stream, int32_t ld, dmad_stream s);
int dmad_dn_stem_bwd(const float* g, int32_t ld, const float* w, int32_t B, float* gspec, dmad_stream s);
int dmad_dn_pool(const float* t, int32_t ldt, int32_t B, int32_t H, int32_t C, float* out, int32_t ldo, dmad_stream s);
int dmad_dn_preact(const float* x, int32_t ldx, const float* scale, const float* shift, int64_t n_px, int32_t C, float* out, dmad_stream s);
int dmad_dn_head(const float* x, int32_t ldx, const float* bns, const float* bnb, const float* fcw, const float* fcb, int32_t B, int32_t HW, int32_t C,
                 int32_t ncls, float* logits, dmad_stream s);
int dmad_dn_head_bwd(const float* g_logits, const float* fcws, const float* x, int32_t ldx, const float* bns, const float* bnb, int32_t B, int32_t HW,
                     int32_t C, int32_t ncls, float* g, int32_t ldg, dmad_stream s);

/* Bytes of device memory held by the engine. */
int64_t dmad_device_bytes(const dmad_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* DMAD_H */
