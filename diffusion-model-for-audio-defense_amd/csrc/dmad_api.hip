// libdmad_hip.so — C ABI (include/dmad.h) and host-side engine: weight packing into MFMA/LDS
// layouts, device workspace (allocated once in dmad_create), kernel sequencing on the caller's stream.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/dmad.h"
#include "dmad_common.h"
#include "wn_vjp.h"
#include "unet_vjp.h"
#include "classifier_vjp.h"
#include "unet_ops.h"
#include "elementwise.h"
#include "wave_defense.h"
#include "wave_fft.h"
#include "m5.h"
#include "kws.h"
#include "kws_mel.h"
#include "masking.h"
#include "wrn.h"
#include "densenet.h"
#include "gemm_f32.h"
#include "gemm_h16.h"
#include "kernel_setup.h"
#include "wn_bf16.h"

using namespace dmad;

namespace {

thread_local std::string g_err, g_warn;

// WaveNet paths of an engine (dmad_wavenet_eps_path / dmad_set_waveform_tier): the mode's default (16-bit where resident), exact fp32,
// the fp32 pipeline on split-f16 operands
enum { PATH_DEFAULT = 0, PATH_FP32 = 1, PATH_X3 = 2 };
// Philox streams of the reverse VP-SDE chain (dmad_vpsde_purify, include/dmad.h): the initial diffusion draw, then one per Euler step
constexpr uint32_t kVpsdeStreamDiffuse = 0x5DE00000u, kVpsdeStreamStep0 = 0x5DE00001u;
// ... and of the spectrogram-domain chain (dmad_spec_vpsde_purify)
constexpr uint32_t kSpecVpsdeStreamDiffuse = 0x5DF00000u, kSpecVpsdeStreamStep0 = 0x5DF00001u;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t _e = (x);                                                                        \
        if (_e != hipSuccess) return fail(DMAD_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
#define CHK(x)                 \
    do {                       \
        int _r = (x);          \
        if (_r != 0) return _r; \
    } while (0)
// end of an entry point's launch sequence: a failed launch, or a GEMM argument block no kernel serves (gemm_f32.h)
#define LASTCHK()                                                                                   \
    do {                                                                                            \
        HIPCHK(hipGetLastError());                                                                  \
        if (int _b = gemm_take_bad_shapes() + gemm_h16_take_bad_shapes()) return fail(DMAD_ERR_INVALID, "%d GEMM launch(es) refused: unsupported shape", _b); \
    } while (0)

uint16_t f2bf(float f) {   // round-to-nearest-even, NaN stays NaN
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

uint16_t f2h(float f) {    // fp32 -> IEEE half, round-to-nearest-even (subnormals and overflow to inf included)
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u, ax = u & 0x7fffffffu;
    if (ax > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);                 // NaN
    if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                // >= 65520 rounds to inf
    if (ax < 0x33000001u) return (uint16_t)sign;                             // <= 2^-25 rounds to zero
    int e = (int)(ax >> 23) - 127;
    uint32_t m = (ax & 0x7fffffu) | 0x800000u;                               // 24-bit significand
    int shift = e < -14 ? 13 + (-14 - e) : 13;                               // bits dropped (subnormal: more)
    uint32_t h = m >> shift, rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (h & 1u))) ++h;
    if (e < -14) return (uint16_t)(sign | h);                                // subnormal (a carry into 0x400 is the smallest normal)
    return (uint16_t)(sign | (uint32_t)(((e + 15) << 10) + (h - 0x400u)));   // a significand carry bumps the exponent
}

// f2h with a census of what leaves the f16 normal range.  A Gaussian weight tensor always has a few values below 2^-14 (f16
// subnormals): their absolute rounding error (<= 2^-25) is far below the 2^-12 relative error of the tensor's typical weights
// and does not matter.  What does matter is a tensor (or a large part of one) that lives down there as a whole — a checkpoint
// with tiny weight-norm gains — or a value beyond 65504 (inf, NaN logits).  So the census is per packed tensor: the share of its
// squared norm carried by subnormal values; dmad_finalize_weights warns when that share exceeds 1e-6 in any tensor.
thread_local double g_h_sq = 0.0, g_h_sq_sub = 0.0;
thread_local long g_h_bad_tensors = 0, g_h_ovf = 0, g_h_tensors = 0;
thread_local double g_h_worst = 0.0;
uint16_t f2h_census(float f) {
    const float a = fabsf(f);
    g_h_sq += (double)a * a;
    if (a < 6.103515625e-05f) g_h_sq_sub += (double)a * a;
    if (a >= 65520.f) ++g_h_ovf;
    return f2h(f);
}
// Development switch of the low-toggle-weights experiment (tools/gpu_weight_toggle.py), compiled in ONLY with
// -DDMAD_DEV_WEIGHT_MASK (never in the product library: a leaked environment variable must not be able to void the exact-vote
// bounds): DMAD_WEIGHT_MASK_BITS = k rounds the f16 weight images of the 16-bit WaveNet path to 10 - k mantissa bits (round to nearest
// even on the f16 pattern, the k low bits then zero: fewer toggling bits on the L2 -> LDS -> register path at a precision cost);
// DMAD_WEIGHT_MASK_WHICH selects the images (bit 0 dilated conv, 1 res conv, 2 skip convs, 3 final_conv.0; default 3).
#ifdef DMAD_DEV_WEIGHT_MASK
thread_local int g_mask_bits = 0;
uint16_t f2h_census_masked(float f) {
    uint32_t h = f2h_census(f);
    const int k = g_mask_bits;
    if (k > 0 && (h & 0x7c00u) != 0x7c00u) {
        const uint32_t sign = h & 0x8000u;
        uint32_t m = h & 0x7fffu;
        m = (m + ((1u << (k - 1)) - 1u) + ((m >> k) & 1u)) & ~((1u << k) - 1u);      // a carry moves into the exponent as it should
        if (m > 0x7bffu) m = 0x7bffu & ~((1u << k) - 1u);
        h = sign | m;
    }
    return (uint16_t)h;
}
#endif
void census_close_tensor() {
    ++g_h_tensors;
    const double share = g_h_sq > 0.0 ? g_h_sq_sub / g_h_sq : 0.0;
    if (share > 1e-6) ++g_h_bad_tensors;
    if (share > g_h_worst) g_h_worst = share;
    g_h_sq = g_h_sq_sub = 0.0;
}

float h2f(uint16_t h) {    // IEEE half -> fp32 (exact)
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    uint32_t u;
    if (e == 0) {
        if (m == 0) u = sign;
        else {                                                               // subnormal: normalise
            int sh = 0;
            uint32_t mm = m;
            while (!(mm & 0x400u)) { mm <<= 1; ++sh; }
            u = sign | ((uint32_t)(127 - 15 - sh + 1) << 23) | ((mm & 0x3ffu) << 13);
        }
    } else if (e == 31) u = sign | 0x7f800000u | (m << 13);
    else u = sign | ((e + 112u) << 23) | (m << 13);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// fp32 matrix [rows][K] -> the split-f16 storage format of dmad_common.h (same bytes per row: every 4 consecutive k become
// the 16-byte chunk [hi0 hi1 hi2 hi3 lo0 lo1 lo2 lo3], lo = f16((x - hi) * 2^11))
void split_rows(const float* src, size_t count, float* dst) {
    uint16_t* o = (uint16_t*)dst;
    for (size_t i = 0; i < count; i += 4)
        for (int j = 0; j < 4; ++j) {
            const float x = src[i + j];
            const uint16_t hi = f2h(x);
            o[2 * i + j] = hi;
            o[2 * i + 4 + j] = f2h((x - h2f(hi)) * 2048.f);
        }
}

const int kVggCfg[] = {64, 64, -1, 128, 128, -1, 256, 256, 256, 256, -1, 512, 512, 512, 512, -1, 512, 512, 512, 512, -1};
const int kVggCfgLen = sizeof(kVggCfg) / sizeof(int);
constexpr int kMelLd = 1040;      // 1025 rFFT bins padded to a multiple of 16
constexpr int kDftM = 2050;       // 1025 cos rows + 1025 sin rows
constexpr int kDftLd = 2052;

struct HostW {
    std::vector<float> v;
    std::vector<int64_t> shape;
};

// The exact-vote state of one vote loop (dmad_smooth_votes / dmad_spec_smooth_votes): the bounds of its first pass and of its
// split-f16 middle tier (< 0: no middle tier), and the statistics dmad_recheck_stats / dmad_spec_recheck_stats2 report
struct RecheckTiers {
    float tau1 = 0.f, tau2 = 0.f;
    int64_t samples = 0, rechecked = 0, rechecked_fp32 = 0;
};

}  // namespace

struct dmad_engine {
    dmad_config cfg{};
    int L = 0, LP = 0, NL = 0, maxB = 0, LPm = 0;
    bool bf16 = true, f32 = false, wn_final = false, cls_final = false;   // bf16 / f32: which WaveNet paths are resident
    int maxB32 = 0;                        // clips per exact-fp32 WaveNet pass (== maxB for DMAD_FP32, recheck_batch for DMAD_EXACT)
    int mode = DMAD_MODE_FAST;             // enum dmad_mode (DMAD_EXACT engines switch at run time)
    int wave_tier = 2;                     // dmad_set_waveform_tier: WaveNet path of the waveform-returning entry points in DMAD_MODE_EXACT_VOTES
    RecheckTiers wave_rt, spec_rt;         // exact-vote bounds and statistics of the waveform / spec-domain vote loop
    long long* rc_list = nullptr;          // global indices of the samples queued for the re-evaluation
    unsigned long long* rc_n = nullptr;    // their number (device) ...
    unsigned long long* rc_n_host = nullptr;   // ... and its pinned host mirror
    long rc_cap = 0;
    int diag[5] = {0, 0, 0, 0, 0};         // dmad_debug_rounding: GemmF32Args::diag of the x3 tier's dil / res / skip / f0 launches, init hi-only
    std::string warn;                      // dmad_last_warning
    std::map<std::string, HostW> hw;
    std::vector<std::pair<void*, size_t>> allocs;    // every live buffer of alloc() and its bytes
    int64_t bytes = 0;
    int emb_t = -1;
    // optional per-launch timing of the dominant kernel (bench.py roofline): HIP event pairs on the launch stream
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev, prof_ev_f;      // layer launches / final-kernel launches
    size_t prof_used = 0, prof_used_f = 0;

    // WaveNet small fp32 params
    float *init_w = nullptr, *init_b = nullptr, *fc1w = nullptr, *fc1b = nullptr, *fc2w = nullptr, *fc2b = nullptr;
    float *fctw = nullptr, *fctb = nullptr, *emb_table = nullptr, *emb2 = nullptr, *epi_c = nullptr;
    float *bf0 = nullptr, *wz = nullptr;
    float bz = 0.f;
    // 16-bit MFMA path (operands bf16, or f16 when `f16` is set)
    bool f16 = false;
    h16_t *w1p = nullptr, *w2p = nullptr, *wsp = nullptr, *wf0p = nullptr;
    float *b1p = nullptr, *b2 = nullptr, *bskip_sum = nullptr;
    h16_t *hA = nullptr, *hB = nullptr, *gstore = nullptr;
    // fp32 path
    float *wdil = nullptr, *bdil = nullptr, *wrs = nullptr, *brs = nullptr, *wf0 = nullptr;
    float *wdil_x3 = nullptr, *wrs_x3 = nullptr, *wf0_x3 = nullptr;      // the same weights in the split-f16 storage format (x3 tier)
    float *wskip32 = nullptr, *wskip_x3 = nullptr, *bskip32 = nullptr;   // [NL][256][256] skip weights (fp32 / split-f16), sum of the skip biases
    float* gstore32 = nullptr;                                           // gate outputs of all layers [NL][maxB32 * L][256] (fp32 and x3 tiers)
    long long* rc_list2 = nullptr;         // samples the x3 tier leaves to the fp32 tier
    float *hA32 = nullptr, *hB32 = nullptr, *H32 = nullptr, *g32 = nullptr, *skip32 = nullptr;
    // VJP workspace (dmad_reserve_vjp): saved residual streams [NL][vjpB][LP][256], gradient maps, transposed weight images
    int vjpB = 0;
    float *vjp_save = nullptr, *vjp_gH = nullptr, *vjp_G = nullptr, *vjp_gg = nullptr;
    float *vjp_wdilT = nullptr, *vjp_wgT = nullptr, *vjp_wf0T = nullptr;
    float* vjp_g2 = nullptr;               // [2][vjpB][L]: the ping-pong adjoint of dmad_vpsde_purify_vjp
    // the longest clip written into each zero-padded fp32 map since it was last clean (clean_pad: the any-length exports)
    int dirty_hA32 = 0, dirty_hB32 = 0, dirty_save = 0, dirty_G = 0, dirty_gH = 0;
    // common work buffers
    float *xt = nullptr, *eps = nullptr, *x0 = nullptr, *znoise = nullptr;
    // classifier
    float *dftA = nullptr, *fbA = nullptr, *mel_xp = nullptr, *dftD = nullptr, *melP = nullptr, *melM = nullptr, *spec = nullptr;
    float *vconv1w = nullptr;
    float* vconvw[16] = {nullptr};
    float* vscale[16] = {nullptr};
    float* vshift[16] = {nullptr};
    float* vfcw[3] = {nullptr};
    float* vfcb[3] = {nullptr};
    float *act0 = nullptr, *act1 = nullptr, *logits = nullptr, *slab = nullptr;
    long slab_floats = 0;
    // ResNeXt29 8x64d (models/resnext.py): 9 bottlenecks, every conv with its folded eval-BatchNorm scale/shift
    int cls_kind = 0;                      // 0 = VGG19_bn, 1 = ResNeXt29, 2 = WideResNet-28-10, 3 = DenseNet-BC-100-12
    struct RxConv { float *w = nullptr, *scale = nullptr, *shift = nullptr; h16_t* wh = nullptr; float* wx = nullptr; float* wT = nullptr; };   // wh: f16 image with the BN scale folded in (16-bit tier); wx: split-f16 image (middle tier); wT: transposed (3x3: tap-flipped) image with the BN scale folded in (classifier VJP)
    struct RxBlock { RxConv reduce, conv, expand, shortc; bool has_short = false; int cin = 0, cout = 0, D = 0, stride = 1; };
    RxBlock rx[9];
    RxConv rxconv1;
    float *rxfcw = nullptr, *rxfcb = nullptr;
    float *rxX = nullptr, *rxY = nullptr, *rxT1 = nullptr, *rxT2 = nullptr, *rxS = nullptr;   // NHWC work buffers
    // ResNeXt29's 16-bit tier (engines with a 16-bit side): every conv through gemm_h16 on f16 operands (fp32 accumulate, BN shift /
    // shortcut add / ReLU in fp32), maps kept as f16 between the convs; tier 1 of the exact-vote loop uses it, the recheck tiers and
    // dmad_classify stay on the fp32 matrix cores
    bool rx_h16 = false;
    bool rx_x3 = false;                    // exact-vote engines: ResNeXt29's split-f16 tier (every conv as three f16 MFMAs per product: fp32-grade), tier 1 of the exact-vote loop
    h16_t *rxX16 = nullptr, *rxY16 = nullptr, *rxT1h = nullptr, *rxT2h = nullptr, *rxS16 = nullptr;
    // Classifier VJP workspace (dmad_reserve_classifier_vjp / _vgg_vjp / _wrn_vjp; an engine holds one classifier, so
    // one workspace serves all three): the tape of the fp32 forward — the slots of cls_tape_layout in forward order, [cvjpB] spectrograms
    // each — and the network's gradient work maps (kRxWork / kVggWork / kWrnWork)
    struct TapeSlot { float* p = nullptr; size_t floats = 0; };    // floats per spectrogram
    int cvjpB = 0, cvjp_lastB = 0;         // lastB: rows of the last pass when the last call ran as one pass (dmad_*_vjp_tape), else 0
    float *cvjp_tape = nullptr, *cvjp_work = nullptr;
    std::vector<TapeSlot> cvjp_slot;
    // VGG19_bn's backward weight images: convs 1 - 15 tap-flipped and transposed with the BN scale folded in, classifier.0 / .3 transposed
    float* vconvwT[16] = {nullptr};
    float* vfcwT[2] = {nullptr};
    // WideResNet-28-10 (models/wideresnet.py): 12 pre-activation blocks; w1 / w2: the 3x3 GEMM images [tap][cout][cin], ws the
    // 1x1 shortcut [cout][cin] of a stage's first block; s1 / b1: the folded bn1 (on the residual stream), s2 / b2: the folded bn2 (conv1's
    // epilogue); w1T / w2T / wsT: the backward images (conv1's with bn2's scale folded in), packed on the first VJP reservation
    struct WrnBlock {
        int cin = 0, cout = 0, stride = 1;
        float *s1 = nullptr, *b1 = nullptr, *w1 = nullptr, *s2 = nullptr, *b2 = nullptr, *w2 = nullptr, *ws = nullptr;
        float *w1T = nullptr, *w2T = nullptr, *wsT = nullptr;
    };
    WrnBlock wrn[12];
    float *wrn_stem = nullptr, *wrn_bns = nullptr, *wrn_bnb = nullptr, *wrn_fcw = nullptr, *wrn_fcb = nullptr;
    float* wrn_fcws = nullptr;              // fc.w with the final bn's scale folded into its columns: the head backward's image
    float *wrnX = nullptr, *wrnY = nullptr, *wrnO = nullptr, *wrnH = nullptr, *wrnS = nullptr, *wrnP = nullptr;   // NHWC work maps ([maxB] x 32 x 32 x 160) and the pooled vector
    // DenseNet-BC-100-12 (models/densenet.py): 48 bottleneck layers (16 per dense block), two transitions.  A layer: s1 / b1 the
    // folded bn1 [cin], w1 the 1x1 image [48][K4] (K4 = cin rounded up to 4, zero columns), s2 / b2 the folded bn2 [48], w2 the 3x3 image
    // [16][9 * 48] (rows 12..15 zero); w1T [cin][48] and w2T [48][9 * 12] (tap-flipped) the backward images.  All built on the host.
    struct DnLayer { int cin = 0, blk = 0; float *s1 = nullptr, *b1 = nullptr, *w1 = nullptr, *s2 = nullptr, *b2 = nullptr, *w2 = nullptr, *w1T = nullptr, *w2T = nullptr; };
    struct DnTrans { int cin = 0, cout = 0; float *s = nullptr, *b = nullptr, *w = nullptr, *wT = nullptr; };      // w [cout][cin4], wT [cin][cout4]
    DnLayer dn[48];
    DnTrans dnT[2];
    float *dn_stem = nullptr, *dn_bns = nullptr, *dn_bnb = nullptr, *dn_fcw = nullptr, *dn_fcb = nullptr, *dn_fcws = nullptr;
    float *dnS[3] = {nullptr, nullptr, nullptr}, *dnH = nullptr, *dnTm = nullptr;      // [maxB] streams (kDnPitch), the h map 32 x 32 x 48 and a transition's conv output 32 x 32 x 108
    // mel front-end VJP (dmad_mel_db_vjp): transposed filterbank [kMelLd][32] and DFT [2048][kDftKT] images, gradient maps of
    // melvjpB clips per pass (allocated on the first call)
    int melvjpB = 0;
    float *mel_fbT = nullptr, *mel_dftAT = nullptr, *melvjp_gM = nullptr, *melvjp_gP = nullptr, *melvjp_gD = nullptr, *melvjp_gF = nullptr;
    // Improved-Diffusion UNet purifier on 1x32x32 mel spectrograms (improved_diffusion/unet.py:278-477)
    struct UnOp {                          // one module of a TimestepEmbedSequential
        int kind = 0;                      // 0 conv_in, 1 res, 2 attn, 3 down, 4 up
        int cin = 0, cout = 0;
        float *gn1w = nullptr, *gn1b = nullptr, *w1 = nullptr, *b1 = nullptr;       // res: in_layers; attn: norm, qkv; down/up/conv_in: conv
        float *embw = nullptr, *embb = nullptr, *gn2w = nullptr, *gn2b = nullptr, *w2 = nullptr, *b2 = nullptr;   // res: emb, out_layers; attn: proj_out
        float *skw = nullptr, *skb = nullptr;                                       // res: 1x1 skip_connection
        h16_t *w1h = nullptr, *w2h = nullptr, *skwh = nullptr;                      // f16 images of w1 / w2 / skw (16-bit tier)
        float *w1x = nullptr, *w2x = nullptr, *skwx = nullptr;                      // the same weights in the split-f16 storage format (middle tier)
        float *w1T = nullptr, *w2T = nullptr, *skwT = nullptr;                      // transposed (3x3: tap-flipped) images of w1 / w2 / skw (UNet VJP)
        size_t ss_off = 0;                 // res: offset of its (scale, shift) row [2 * cout] inside a step's row of un_ss_table
        // its place in the forward order: its input resolution, the saved map of its concatenated input (top: output blocks' first modules), the
        // saved map whose gradient joins its input gradient (acc: the first module after each input block, which reads hs[acc]) and the saved
        // map its output is (save: the last module of each input block); -1: none
        int H = 0, top = -1, acc = -1, save = -1;
    };
    std::vector<UnOp> un_ops;              // the modules in forward order (input, middle, output blocks): every walk over the network iterates this list; a module's index is its tape slot
    std::vector<int> un_hs_ch, un_hs_hw;   // channels / pixels of the saved input-block outputs
    std::vector<float*> un_hs;
    bool un_final = false;
    int un_t = -1;
    // Every ResBlock's emb_layers output depends on the step t alone (unet.py:186-199), and a sampler walks the same few steps for
    // every batch: row t of un_ss_table caches all of them (kUnSsSteps = diffusion_steps rows of un_ss_total floats, ~54 MB, plus
    // one scratch row for steps beyond the schedule), filled the first time a step is seen — 24 small launches, ~1 ms, per step
    // instead of per network evaluation.
    size_t un_ss_total = 0;
    float* un_ss_table = nullptr;
    const float* un_ss_cur = nullptr;
    std::vector<char> un_ss_have;
    float *un_te0w = nullptr, *un_te0b = nullptr, *un_te2w = nullptr, *un_te2b = nullptr, *un_outgw = nullptr, *un_outgb = nullptr;
    float *un_outw = nullptr, *un_outb = nullptr, *un_temb = nullptr, *un_emb1 = nullptr, *un_emb = nullptr, *un_semb = nullptr;
    float* un_buf[8] = {nullptr};          // work maps: 3 rotating block outputs, T1, T2, skip, qkv / cat, attention
    float* un_eps = nullptr;
    // 16-bit tier of the UNet (gemm_h16: f16 operands, fp32 accumulate; GroupNorm / softmax / residual sums stay fp32): f16 twins of
    // the block outputs (the maps a GEMM reads without a GroupNorm in between), f16-only GroupNorm / upsample / attention outputs
    bool un_h16 = false;
    bool un_x3 = false;                    // exact-vote engines: the UNet's middle tier (fp32 pipeline on split-f16 operands, gemm_x3_kernel) is resident
    h16_t* un_buf16[3] = {nullptr};
    std::vector<h16_t*> un_hs16;
    h16_t *un_t1h = nullptr, *un_t2h = nullptr, *un_uph = nullptr, *un_atth = nullptr, *un_qkvh = nullptr;
    // GroupNorm statistics of the f16 maps, written by the GEMM that produces the map (GemmH16Args::stats): one slab per map buffer
    float* un_st_buf[3] = {nullptr};
    float* un_st_t2 = nullptr;
    std::vector<float*> un_st_hs;
    // UNet VJP workspace (dmad_reserve_unet_vjp): the tape of the exact-fp32 forward — per module (in forward order,
    // un_ops) its output map, and a ResBlock's conv1 output / an AttentionBlock's qkv — [unvjpB] spectrograms per slot,
    // the gradient maps of the saved skips (g_hs), six work maps and the transposed weight images
    struct UnTape { std::vector<float*> out, t2, qkv, hs; };     // hs[i]: the out slot that holds saved map i
    int unvjpB = 0;
    float *unvjp_tape = nullptr, *unvjp_ghs = nullptr, *unvjp_work = nullptr, *unvjp_zero = nullptr;
    float* unvjp_g2 = nullptr;              // [2][unvjpB][1024]: the ping-pong adjoint of dmad_spec_vpsde_purify_vjp
    float *un_inT = nullptr, *un_outT = nullptr;            // conv_in [9][128] / out.2 [128][9] images, tap-flipped
    UnTape un_tape;
    std::vector<float*> unvjp_ghs_at;
    // M5 raw-waveform classifier (m5.h): a part of its own, exact fp32 on every precision.  One buffer of weight images;
    // the kernels keep a clip's activations in LDS, so there is no workspace
    bool m5_final = false;
    float* m5_buf = nullptr;
    M5Weights m5w;
    M5Geom m5g;
    // Attention-CRNN keyword spotter (kws.h): a part of its own, exact fp32 on every precision.  One buffer of weight
    // images; the row length T is an argument of every call, so the LDS layout is worked out per call
    bool kws_final = false;
    float* kws_buf = nullptr;
    KwsWeights kwsw;
    // Mel front-end of the keyword spotter (kws_mel.h): constants built at first use on any engine, and the scratch of the
    // two wave exports -- dB spectrogram and its gradient of kKwsWaveRows (512) rows at the longest T, of which only the read frames are used
    KwsMelConst kmel;
    float* kws_spec = nullptr;
    float* kws_gspec = nullptr;
    // Whole-clip real FFT pair (wave_fft.h): the plan of clip_len and the twiddle table, built at first use on any engine
    FftPlan fft_plan;
    float* fft_tw = nullptr;

    template <typename T>
    int alloc(T** p, size_t n, bool zero = false) {
        void* d = nullptr;
        hipError_t e = hipMalloc(&d, n * sizeof(T));
        if (e != hipSuccess) return fail(DMAD_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e));
        if (zero) {
            e = hipMemset(d, 0, n * sizeof(T));
            if (e != hipSuccess) return fail(DMAD_ERR_HIP, "hipMemset failed: %s", hipGetErrorString(e));
        }
        allocs.push_back({d, n * sizeof(T)});
        bytes += (int64_t)(n * sizeof(T));
        *p = (T*)d;
        return 0;
    }
    template <typename T>
    void release(T** p) {                  // frees a buffer of alloc() (a reservation that is replaced)
        if (!*p) return;
        for (size_t i = 0; i < allocs.size(); ++i)
            if (allocs[i].first == (void*)*p) { bytes -= (int64_t)allocs[i].second; allocs.erase(allocs.begin() + i); break; }
        (void)hipFree(*p);
        *p = nullptr;
    }
    template <typename T>
    int upload(T** p, const std::vector<T>& h) {
        CHK(alloc(p, h.size()));
        HIPCHK(hipMemcpy(*p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
    int upload_bf(h16_t** p, const std::vector<uint16_t>& h) {
        CHK(alloc(p, h.size()));
        HIPCHK(hipMemcpy(*p, h.data(), h.size() * 2, hipMemcpyHostToDevice));
        return 0;
    }
    const HostW* get(const std::string& name, std::initializer_list<int64_t> shape) {
        auto it = hw.find(name);
        if (it == hw.end()) {
            fail(DMAD_ERR_STATE, "weight '%s' was not loaded", name.c_str());
            return nullptr;
        }
        int64_t n = 1;
        for (auto s : shape) n *= s;
        if ((int64_t)it->second.v.size() != n) {
            fail(DMAD_ERR_INVALID, "weight '%s' has %zu elements, expected %lld", name.c_str(), it->second.v.size(), (long long)n);
            return nullptr;
        }
        return &it->second;
    }
};

namespace {

// ---- preconditions of the entry points: each returns 0, or its error through fail()
int need_wavenet(const dmad_engine* e) { return e->wn_final ? 0 : fail(DMAD_ERR_STATE, "WaveNet weights are not finalised (dmad_load_weight + dmad_finalize_weights)"); }
int need_unet(const dmad_engine* e) { return e->un_final ? 0 : fail(DMAD_ERR_STATE, "UNet weights are not finalised (dmad_load_weight + dmad_finalize_weights)"); }
int need_with_classifier(const dmad_engine* e) { return e->cfg.with_classifier ? 0 : fail(DMAD_ERR_STATE, "engine was created with with_classifier = 0"); }
int need_classifier(const dmad_engine* e) {      // ... and its weights finalised
    if (int r = need_with_classifier(e)) return r;
    return e->cls_final ? 0 : fail(DMAD_ERR_STATE, "classifier weights are not finalised (dmad_load_weight + dmad_finalize_weights)");
}
// the classifiers by cls_kind: the network, the name its VJP goes by in the refusals, its VJP export and its reservation export
const struct { const char *net, *vjp_of, *vjp, *reserve; } kCls[4] = {
    {"VGG19_bn", "VGG19_bn", "dmad_vgg_vjp", "dmad_reserve_vgg_vjp"},
    {"ResNeXt29", "classifier", "dmad_classify_vjp", "dmad_reserve_classifier_vjp"},
    {"WideResNet-28-10", "WideResNet", "dmad_wrn_vjp", "dmad_reserve_wrn_vjp"},
    {"DenseNet-BC-100-12", "DenseNet", "dmad_dn_vjp", "dmad_reserve_dn_vjp"}};
int need_kind(const dmad_engine* e, int kind) {  // the finalised classifier is the one whose VJP, reservation or tape is asked for
    CHK(need_classifier(e));
    return e->cls_kind == kind ? 0 : fail(DMAD_ERR_STATE, "the %s VJP serves %s only: this engine holds %s (%s)", kCls[kind].vjp_of, kCls[kind].net,
                                          kCls[e->cls_kind].net, kCls[e->cls_kind].vjp);
}
int need_kws(const dmad_engine* e) { return e->kws_final ? 0 : fail(DMAD_ERR_STATE, "KWS weights are not finalised (dmad_load_weight + dmad_finalize_weights)"); }
int need_kws_mel(dmad_engine* e) {          // the constants of kws_mel.h, float64 on the host and rounded once
    if (e->kmel.af) return 0;
    KwsMelHost h;
    if (const char* m = kws_mel_host_constants(&h)) return fail(DMAD_ERR_STATE, "KWS mel constants: %s", m);
    float *af = nullptr, *ab = nullptr, *fb = nullptr, *w0 = nullptr, *w1 = nullptr;
    int32_t *m0 = nullptr, *lo = nullptr, *hi = nullptr;
    CHK(e->upload(&ab, h.ab)); CHK(e->upload(&fb, h.fb)); CHK(e->upload(&w0, h.w0)); CHK(e->upload(&w1, h.w1));
    CHK(e->upload(&m0, h.m0)); CHK(e->upload(&lo, h.lo)); CHK(e->upload(&hi, h.hi)); CHK(e->upload(&af, h.af));
    e->kmel = KwsMelConst{af, ab, fb, w0, w1, m0, lo, hi};       // af last: it is the guard
    return 0;
}
int need_wave_fft(dmad_engine* e, const char* who) {      // the plan of clip_len and exp(-2 pi i j / L), float64 on the host rounded once
    if (e->fft_tw) return 0;
    FftPlan p;
    if (const char* m = wave_fft_plan(e->L, &p)) return fail(DMAD_ERR_SHAPE, "%s: the wave FFT does not serve clip_len %d: %s", who, e->L, m);
    std::vector<float> tw(2 * (size_t)e->L);
    wave_fft_twiddles(e->L, tw.data());
    float* d = nullptr;
    CHK(e->upload(&d, tw));
    e->fft_plan = p;
    e->fft_tw = d;                          // last: it is the guard
    return 0;
}
int need_m5(const dmad_engine* e) { return e->m5_final ? 0 : fail(DMAD_ERR_STATE, "M5 weights are not finalised (dmad_load_weight + dmad_finalize_weights)"); }
// the kernel families of `mask` set up on the current device (kernel_setup.h); after the first call per device a table read each
int need_kernels(unsigned mask) {
    for (unsigned f = 1; f <= mask; f <<= 1)
        if (mask & f)
            if (int r = kernels_ready(f))
                return fail(DMAD_ERR_HIP, "kernel set-up (max dynamic LDS, %s) failed: %s", kernel_family_name(f), hipGetErrorString((hipError_t)r));
    return 0;
}
int need_batch(const dmad_engine* e, int B) { return B >= 1 && B <= e->maxB ? 0 : fail(DMAD_ERR_STATE, "batch %d outside [1, max_batch=%d]", B, e->maxB); }
int need_path(const dmad_engine* e, int path) {  // a WaveNet path the caller names (dmad_wavenet_eps_path / dmad_eval_samples)
    if (path != PATH_DEFAULT && path != PATH_FP32 && path != PATH_X3) return fail(DMAD_ERR_INVALID, "unknown path %d", path);
    return path == PATH_DEFAULT || (e->bf16 && e->f32) ? 0 : fail(DMAD_ERR_STATE, "explicit WaveNet paths need a DMAD_EXACT engine");
}

// walks [0, total) in passes of at most `cap`: fn(offset, count) per pass, until one fails
template <class Fn>
int for_passes(int64_t total, int64_t cap, Fn fn) {
    for (int64_t off = 0; off < total; off += cap) CHK(fn(off, (int)(total - off < cap ? total - off : cap)));
    return 0;
}

// ---- VJP reservations (dmad_reserve_*_vjp)
// A backward weight image, allocated and packed once.  Its own pointer is its guard: a reservation that failed part of the way (out of
// memory) keeps the images it had packed, and the next call packs exactly the missing ones
template <class Fn>
int pack_once(dmad_engine* e, float** image, size_t floats, Fn pack) {
    if (*image) return 0;
    CHK(e->alloc(image, floats));
    pack();
    return 0;
}

// One reservation of min(max_batch, e->*cap) clips per pass; e->*size is the present one.  need(): the export's preconditions in its own
// order; bufs(): the buffers that scale with the pass size; pack(): the backward images that are still missing (pack_once); lay(vB):
// allocates bufs() for vB clips and lays them out.  A smaller request returns 0 and touches nothing; a larger one releases the present
// buffers first, and if anything then fails every one of them is released again: no half reservation stays behind, e->*size stays 0
template <class Need, class Bufs, class Pack, class Lay>
int reserve_vjp(dmad_engine* e, int max_batch, int dmad_engine::*cap, int dmad_engine::*size, Need need, Bufs bufs, Pack pack, Lay lay) {
    if (!e) return fail(DMAD_ERR_INVALID, "null engine");
    if (max_batch < 1) return fail(DMAD_ERR_INVALID, "max_batch %d < 1", max_batch);
    CHK(need());
    const int vB = max_batch < e->*cap ? max_batch : e->*cap;
    if (vB <= e->*size) return 0;
    const std::vector<float**> held = bufs();
    for (float** p : held) e->release(p);
    e->*size = 0;
    auto fill = [&]() -> int {
        CHK(pack());
        HIPCHK(hipGetLastError());
        CHK(lay(vB));
        HIPCHK(hipDeviceSynchronize());
        return 0;
    };
    if (int r = fill()) {
        for (float** p : held) e->release(p);
        return r;
    }
    e->*size = vB;
    return 0;
}

// ---- gemm_f32 argument blocks
// a plain GEMM over N rows of K floats, ldx apart (mode 0)
GemmF32Args plain_gemm(const float* A, const float* X, float* C, const float* scale, const float* shift, int M, int K, long N,
                       int ldc, long ldx, int relu) {
    GemmF32Args g{};
    g.A = A; g.X = X; g.C = C; g.scale = scale; g.shift = shift;
    g.M = M; g.K = K; g.taps = 1; g.ldc = ldc; g.relu = relu; g.N = N; g.mode = 0;
    g.rows_per_batch = N > 0 ? N : 1; g.batch_stride = 0; g.row_stride = ldx; g.tap_stride = 0;
    return g;
}

// the WaveNet's strided 1-D form (mode 0): `rpb` positions per clip, clips / positions / taps batch_stride / row_stride / tap_stride floats apart
GemmF32Args wn_conv_args(const float* A, const float* X, float* C, const float* shift, int M, int K, int taps, long N, long rpb,
                         long batch_stride, long row_stride, long tap_stride) {
    GemmF32Args g{};
    g.A = A; g.X = X; g.C = C; g.shift = shift; g.M = M; g.K = K; g.taps = taps; g.ldc = M; g.N = N; g.mode = 0;
    g.rows_per_batch = rpb; g.batch_stride = batch_stride; g.row_stride = row_stride; g.tap_stride = tap_stride;
    return g;
}

// a 3x3 (zero padding 1) / 1x1 conv over B NHWC maps of H x H pixels (mode 2); M / K: output / input channels (per group), ldx / ldc: the
// pixel pitch of X / C (< 0: K / M)
GemmF32Args nhwc_conv_args(const float* A, const float* scale, const float* shift, const float* X, float* C, int M, int K, int taps, int B,
                           int H, int stride, const float* res, int relu = 0, int groups = 0, int ldx = -1, int ldc = -1) {
    GemmF32Args g{};
    const int Ho = (H - 1) / (stride > 1 ? stride : 1) + 1;
    g.A = A; g.X = X; g.C = C; g.scale = scale; g.shift = shift; g.M = M; g.K = K; g.taps = taps; g.ldc = ldc < 0 ? M : ldc; g.relu = relu;
    g.N = (long)B * Ho * Ho; g.mode = 2; g.H = H; g.W = H; g.Cin = K; g.ldx = ldx < 0 ? K : ldx; g.stride = stride; g.groups = groups; g.res = res;
    return g;
}

// a dense 3x3 conv's weights [M][K][3][3] as its GEMM image [tap][M][K]
std::vector<float> conv3_image(const std::vector<float>& cw, int M, int K) {
    std::vector<float> A((size_t)9 * M * K);
    for (int co = 0; co < M; ++co)
        for (int ci = 0; ci < K; ++ci)
            for (int t = 0; t < 9; ++t) A[((size_t)t * M + co) * K + ci] = cw[((size_t)co * K + ci) * 9 + t];
    return A;
}

int upload_h16(dmad_engine* e, const std::vector<float>& A, h16_t** wh) {
    std::vector<uint16_t> H(A.size());
    for (size_t i = 0; i < A.size(); ++i) H[i] = f2h(A[i]);
    return e->upload_bf(wh, H);
}

int upload_split(dmad_engine* e, const std::vector<float>& A, float** wx) {
    std::vector<float> t(A.size());
    split_rows(A.data(), A.size(), t.data());
    return e->upload(wx, t);
}

// [ksteps][rows][32] bf16 LDS image of W[row][K] (row-major, K = ksteps*32), 64-B rows, swz64 chunks
// k-step ks of W lands in stage ks * smul + sadd of the image (GEMM1 interleaves the three taps' k-steps)
void pack_rows(uint16_t (*cvt)(float), const float* W, int rows, int K, long ldw, const int* row_map, std::vector<uint16_t>& out,
               size_t base, int smul = 1, int sadd = 0) {
    const int ksteps = K / 32;
    for (int ks = 0; ks < ksteps; ++ks)
        for (int R = 0; R < rows; ++R) {
            const float* src = W + (long)(row_map ? row_map[R] : R) * ldw + ks * 32;
            for (int slot = 0; slot < 4; ++slot) {
                const int c = slot ^ swz64(R);
                for (int j = 0; j < 8; ++j) out[base + ((size_t)((ks * smul + sadd) * rows + R) * 32) + slot * 8 + j] = cvt(src[c * 8 + j]);
            }
        }
}

int finalize_wavenet(dmad_engine* e) {
    const int NL = e->NL;
    const HostW* w;
#define GETW(var, name, ...)                     \
    w = e->get(name, {__VA_ARGS__});             \
    if (!w) return DMAD_ERR_STATE;               \
    const std::vector<float>& var = w->v;
    GETW(init_w, "init.w", 256) GETW(init_b, "init.b", 256)
    GETW(fc1w, "fc_t1.w", 512, 128) GETW(fc1b, "fc_t1.b", 512)
    GETW(fc2w, "fc_t2.w", 512, 512) GETW(fc2b, "fc_t2.b", 512)
    GETW(f0w, "f0.w", 256, 256) GETW(f0b, "f0.b", 256)
    GETW(f2w, "f2.w", 256) GETW(f2b, "f2.b", 1)
    CHK(e->upload(&e->init_w, init_w)); CHK(e->upload(&e->init_b, init_b));
    CHK(e->upload(&e->fc1w, fc1w)); CHK(e->upload(&e->fc1b, fc1b));
    CHK(e->upload(&e->fc2w, fc2w)); CHK(e->upload(&e->fc2b, fc2b));
    CHK(e->upload(&e->bf0, f0b)); CHK(e->upload(&e->wz, f2w));
    e->bz = f2b[0];
    std::vector<float> fctw((size_t)NL * 256 * 512), fctb((size_t)NL * 256);
    for (int n = 0; n < NL; ++n) {
        char nm[64];
        snprintf(nm, sizeof nm, "fc_t.%d.w", n);
        GETW(a, nm, 256, 512)
        memcpy(&fctw[(size_t)n * 256 * 512], a.data(), a.size() * 4);
        snprintf(nm, sizeof nm, "fc_t.%d.b", n);
        GETW(bb, nm, 256)
        memcpy(&fctb[(size_t)n * 256], bb.data(), 1024);
    }
    CHK(e->upload(&e->fctw, fctw)); CHK(e->upload(&e->fctb, fctb));
    CHK(e->alloc(&e->emb_table, (size_t)NL * 256)); CHK(e->alloc(&e->emb2, 512)); CHK(e->alloc(&e->epi_c, (size_t)NL * 256, true));

    if (e->bf16) {
        uint16_t (*cvt)(float) = e->f16 ? f2h_census : f2bf;
        g_h_sq = g_h_sq_sub = g_h_worst = 0.0; g_h_bad_tensors = g_h_ovf = g_h_tensors = 0;
#ifdef DMAD_DEV_WEIGHT_MASK
        int mask_bits = 0, mask_which = 3;              // development build only, see f2h_census_masked
        if (const char* mb = getenv("DMAD_WEIGHT_MASK_BITS")) mask_bits = atoi(mb);
        if (const char* mw = getenv("DMAD_WEIGHT_MASK_WHICH")) mask_which = atoi(mw);
        if (mask_bits < 0 || mask_bits > 9 || !e->f16) mask_bits = 0;
        if (mask_bits) e->warn = "DEVELOPMENT BUILD: the f16 WaveNet weight images are rounded to fewer mantissa bits (DMAD_WEIGHT_MASK_BITS); the recheck bounds do not hold";
        auto cvt_for = [&](int which) -> uint16_t (*)(float) {
            g_mask_bits = mask_bits;
            return (mask_bits && (mask_which >> which & 1)) ? f2h_census_masked : cvt;
        };
#else
        auto cvt_for = [&](int) -> uint16_t (*)(float) { return cvt; };
#endif
        int rmap[512];
        // tile row R = wm*128 + half*64 + mt*16 + i  <->  gate row half*256 + (mt*64 + wm*16 + i): channel ownership is
        // interleaved over the M-waves so that GEMM2 can start on channels [64 mt, 64 mt + 64) as soon as tiles mt are gated
        for (int R = 0; R < 512; ++R) rmap[R] = ((R % 128) / 64) * 256 + ((R % 64) / 16) * 64 + (R / 128) * 16 + (R % 16);
        std::vector<uint16_t> w1p((size_t)NL * 24 * 512 * 32), w2p((size_t)NL * 8 * 256 * 32), wsp((size_t)NL * 8 * 256 * 32),
            wf0p((size_t)8 * 256 * 32);
        std::vector<float> b1p((size_t)NL * 512), b2((size_t)NL * 256), bsum(256, 0.f), tapw((size_t)512 * 256);
        for (int n = 0; n < NL; ++n) {
            char nm[64];
            snprintf(nm, sizeof nm, "dil.%d.w", n); GETW(dw, nm, 512, 256, 3)
            snprintf(nm, sizeof nm, "dil.%d.b", n); GETW(db, nm, 512)
            snprintf(nm, sizeof nm, "res.%d.w", n); GETW(rw, nm, 256, 256)
            snprintf(nm, sizeof nm, "res.%d.b", n); GETW(rb, nm, 256)
            snprintf(nm, sizeof nm, "skip.%d.w", n); GETW(sw, nm, 256, 256)
            snprintf(nm, sizeof nm, "skip.%d.b", n); GETW(sb, nm, 256)
            for (int tap = 0; tap < 3; ++tap) {
                for (int oc = 0; oc < 512; ++oc)
                    for (int ci = 0; ci < 256; ++ci)     // rows pre-scaled to exp2 arguments: tanh half by -2*log2(e), sigmoid half by -log2(e)
                        tapw[(size_t)oc * 256 + ci] = dw[((size_t)oc * 256 + ci) * 3 + tap] * (oc < 256 ? -2.8853900817779268f : -1.4426950408889634f);
                pack_rows(cvt_for(0), tapw.data(), 512, 256, 256, rmap, w1p, (size_t)n * 24 * 512 * 32, 3, tap);   // stage = 3 * kchunk + tap
            }
            census_close_tensor();
            for (int R = 0; R < 512; ++R) b1p[(size_t)n * 512 + R] = db[rmap[R]];
            std::vector<float> rws(rw.size());                      // res conv pre-scaled by sqrt(1/2): h' = h*sqrt(1/2) + (W_res' g + c)
            for (size_t i = 0; i < rw.size(); ++i) rws[i] = rw[i] * 0.70710678118654752440f;
            pack_rows(cvt_for(1), rws.data(), 256, 256, 256, nullptr, w2p, (size_t)n * 8 * 256 * 32);
            census_close_tensor();
            pack_rows(cvt_for(2), sw.data(), 256, 256, 256, nullptr, wsp, (size_t)n * 8 * 256 * 32);
            census_close_tensor();
            for (int c = 0; c < 256; ++c) { b2[(size_t)n * 256 + c] = rb[c]; bsum[c] += sb[c]; }
        }
        pack_rows(cvt_for(3), f0w.data(), 256, 256, 256, nullptr, wf0p, 0);
        census_close_tensor();
        CHK(e->upload_bf(&e->w1p, w1p)); CHK(e->upload_bf(&e->w2p, w2p)); CHK(e->upload_bf(&e->wsp, wsp));
        CHK(e->upload_bf(&e->wf0p, wf0p));
        CHK(e->upload(&e->b1p, b1p)); CHK(e->upload(&e->b2, b2)); CHK(e->upload(&e->bskip_sum, bsum));
        if (e->f16 && (g_h_bad_tensors || g_h_ovf)) {
            char buf[448];
            snprintf(buf, sizeof buf, "WaveNet weights on the f16 MFMA path: in %ld of %ld folded weight tensors f16 subnormals (|w| < 6.1e-5: fewer "
                     "than 11 significant bits) carry more than 1e-6 of the squared norm (worst: %.3g), and %ld values overflow to inf "
                     "(|w| > 65504); the 16-bit tier's error bound was not measured for such weights: calibrate the recheck margins on "
                     "these weights or use half_type = bf16", g_h_bad_tensors, g_h_tensors, g_h_worst, g_h_ovf);
            e->warn = buf;
        }
    }
    if (e->f32) {
        std::vector<float> wdil((size_t)NL * 3 * 512 * 256), bdil((size_t)NL * 512), wrs((size_t)NL * 512 * 256), brs((size_t)NL * 512);
        for (int n = 0; n < NL; ++n) {
            char nm[64];
            snprintf(nm, sizeof nm, "dil.%d.w", n); GETW(dw, nm, 512, 256, 3)
            snprintf(nm, sizeof nm, "dil.%d.b", n); GETW(db, nm, 512)
            snprintf(nm, sizeof nm, "res.%d.w", n); GETW(rw, nm, 256, 256)
            snprintf(nm, sizeof nm, "res.%d.b", n); GETW(rb, nm, 256)
            snprintf(nm, sizeof nm, "skip.%d.w", n); GETW(sw, nm, 256, 256)
            snprintf(nm, sizeof nm, "skip.%d.b", n); GETW(sb, nm, 256)
            // gate-fused epilogue (gemm_f32.h, epi 1): image row R of block bm holds H row (i >= 2 ? 256 : 0) + bm*64 + wm*32 + (i&1)*16 + r
            for (int tap = 0; tap < 3; ++tap)
                for (int R = 0; R < 512; ++R) {
                    const int bm = R / 128, wmr = (R % 128) / 64, i = (R % 64) / 16, rr = R % 16;
                    const int oc = (i >= 2 ? 256 : 0) + bm * 64 + wmr * 32 + (i & 1) * 16 + rr;
                    for (int ci = 0; ci < 256; ++ci)
                        wdil[(((size_t)n * 3 + tap) * 512 + R) * 256 + ci] = dw[((size_t)oc * 256 + ci) * 3 + tap];
                    if (tap == 0) bdil[(size_t)n * 512 + R] = db[oc];
                }
            memcpy(&wrs[(size_t)n * 512 * 256], rw.data(), 256 * 256 * 4);
            memcpy(&wrs[(size_t)n * 512 * 256 + 256 * 256], sw.data(), 256 * 256 * 4);
            memcpy(&brs[(size_t)n * 512], rb.data(), 1024);
            memcpy(&brs[(size_t)n * 512 + 256], sb.data(), 1024);
        }
        CHK(e->upload(&e->wdil, wdil)); CHK(e->upload(&e->bdil, bdil)); CHK(e->upload(&e->wrs, wrs)); CHK(e->upload(&e->brs, brs));
        CHK(e->upload(&e->wf0, f0w));
        // the NL skip convs run as ONE K = NL * 256 GEMM over the stored gate outputs of all layers (as the 16-bit path does):
        // no fp32 read-modify-write of the skip sum per layer
        std::vector<float> ws((size_t)NL * 256 * 256), bs(256, 0.f);
        for (int n = 0; n < NL; ++n) {
            memcpy(&ws[(size_t)n * 256 * 256], &wrs[(size_t)n * 512 * 256 + 256 * 256], 256 * 256 * 4);
            for (int c = 0; c < 256; ++c) bs[c] += brs[(size_t)n * 512 + 256 + c];
        }
        CHK(e->upload(&e->wskip32, ws));
        CHK(e->upload(&e->bskip32, bs));
        CHK(e->alloc(&e->gstore32, (size_t)NL * e->maxB32 * e->L * 256));      // [NL][maxB32 * L][256], shared by the fp32 and split-f16 tiers
        if (e->bf16) {                      // exact-vote engines: the middle (split-f16, three-MFMA) tier reads these
            std::vector<float> t(wdil.size());
            split_rows(wdil.data(), wdil.size(), t.data()); CHK(e->upload(&e->wdil_x3, t));
            t.resize(wrs.size()); split_rows(wrs.data(), wrs.size(), t.data()); CHK(e->upload(&e->wrs_x3, t));
            t.resize(f0w.size()); split_rows(f0w.data(), f0w.size(), t.data()); CHK(e->upload(&e->wf0_x3, t));
            t.resize(ws.size()); split_rows(ws.data(), ws.size(), t.data()); CHK(e->upload(&e->wskip_x3, t));
        }
    }
    return 0;
}

int init_mel_constants(dmad_engine* e) {
    // mel constants, float64 on the host then rounded once (torchaudio MelSpectrogram semantics)
    {
        std::vector<float> A((size_t)kDftM * 2048);
        std::vector<double> win(2048);
        for (int n = 0; n < 2048; ++n) win[n] = 0.5 - 0.5 * cos(2.0 * M_PI * n / 2048.0);
        for (int f = 0; f < 1025; ++f)
            for (int n = 0; n < 2048; ++n) {
                const long ph = ((long)f * n) % 2048;                 // exact argument reduction
                const double ang = 2.0 * M_PI * (double)ph / 2048.0;
                A[(size_t)f * 2048 + n] = (float)(win[n] * cos(ang));
                A[(size_t)(1025 + f) * 2048 + n] = (float)(-win[n] * sin(ang));
            }
        CHK(e->upload(&e->dftA, A));
        // slaney mel filterbank, [32][kMelLd]
        auto hz2mel = [](double f) { return f >= 1000.0 ? 15.0 + log(f / 1000.0) / (log(6.4) / 27.0) : f / (200.0 / 3); };
        auto mel2hz = [](double m) { return m >= 15.0 ? 1000.0 * exp((log(6.4) / 27.0) * (m - 15.0)) : (200.0 / 3) * m; };
        double fpts[34];
        const double m0 = hz2mel(0.0), m1 = hz2mel(8000.0);
        for (int i = 0; i < 34; ++i) fpts[i] = mel2hz(m0 + (m1 - m0) * i / 33.0);
        std::vector<float> fb((size_t)32 * kMelLd, 0.f);
        for (int m = 0; m < 32; ++m) {
            const double enorm = 2.0 / (fpts[m + 2] - fpts[m]);
            for (int f = 0; f < 1025; ++f) {
                const double fr = 8000.0 * f / 1024.0;
                const double down = (fr - fpts[m]) / (fpts[m + 1] - fpts[m]);
                const double up = (fpts[m + 2] - fr) / (fpts[m + 2] - fpts[m + 1]);
                const double v = fmax(0.0, fmin(down, up));
                fb[(size_t)m * kMelLd + f] = (float)(v * enorm);
            }
        }
        CHK(e->upload(&e->fbA, fb));
    }
    return 0;
}

int finalize_classifier(dmad_engine* e) {
    const HostW* w;
    // VGG19_bn
    int cin = 1, li = 0;
    for (int i = 0; i < kVggCfgLen; ++i) {
        const int v = kVggCfg[i];
        if (v < 0) continue;
        char nm[64];
        snprintf(nm, sizeof nm, "vgg.conv%d.w", li);
        w = e->get(nm, {v, cin, 3, 3});
        if (!w) return DMAD_ERR_STATE;
        if (li == 0) CHK(e->upload(&e->vconv1w, w->v));
        else CHK(e->upload(&e->vconvw[li], conv3_image(w->v, v, cin)));
        snprintf(nm, sizeof nm, "vgg.conv%d.scale", li);
        w = e->get(nm, {v}); if (!w) return DMAD_ERR_STATE;
        CHK(e->upload(&e->vscale[li], w->v));
        snprintf(nm, sizeof nm, "vgg.conv%d.shift", li);
        w = e->get(nm, {v}); if (!w) return DMAD_ERR_STATE;
        CHK(e->upload(&e->vshift[li], w->v));
        cin = v;
        ++li;
    }
    const int fin[3] = {512, 4096, 4096}, fout[3] = {4096, 4096, e->cfg.num_classes};
    for (int j = 0; j < 3; ++j) {
        char nm[64];
        snprintf(nm, sizeof nm, "vgg.fc%d.w", j);
        w = e->get(nm, {fout[j], fin[j]}); if (!w) return DMAD_ERR_STATE;
        CHK(e->upload(&e->vfcw[j], w->v));
        snprintf(nm, sizeof nm, "vgg.fc%d.b", j);
        w = e->get(nm, {fout[j]}); if (!w) return DMAD_ERR_STATE;
        CHK(e->upload(&e->vfcb[j], w->v));
    }
    return 0;
}

// ResNeXt29 8x64d: names rx.conv1.*, rx.b<i>.{reduce,conv,expand,short}.{w,scale,shift} (i = 3 * stage + bottleneck),
// rx.fc.{w,b}.  GEMM images: 1x1 convs [M][K]; the grouped 3x3 conv per group [tap][M/8][K/8] (models/resnext.py:23-62).
int finalize_resnext(dmad_engine* e) {
    const HostW* w;
    // A: the fp32 GEMM image; rows_of(i) = the output channel whose BN scale multiplies element i of the f16 image Ah (null: Ah = A)
    auto up3 = [&](const std::string& base, dmad_engine::RxConv& c, const std::vector<float>& A, int M, const std::vector<float>* Ah = nullptr,
                   const std::vector<int>* ch_of = nullptr, long row_len = 0) -> int {
        CHK(e->upload(&c.w, A));
        w = e->get(base + ".scale", {M}); if (!w) return DMAD_ERR_STATE;
        const std::vector<float> scale = w->v;
        CHK(e->upload(&c.scale, scale));
        w = e->get(base + ".shift", {M}); if (!w) return DMAD_ERR_STATE;
        CHK(e->upload(&c.shift, w->v));
        if (e->rx_h16 && row_len > 0) {     // f16 image, BN scale folded into the rows (the 16-bit kernel's epilogue only adds the shift)
            const std::vector<float>& S = Ah ? *Ah : A;
            std::vector<uint16_t> Hh(S.size());
            for (size_t i = 0; i < S.size(); ++i) {
                const long row = (long)(i / (size_t)row_len);
                const int ch = ch_of ? (*ch_of)[row] : (int)(row % M);
                Hh[i] = f2h(ch >= 0 ? S[i] * scale[ch] : 0.f);
            }
            CHK(e->upload_bf(&c.wh, Hh));
        }
        if (e->rx_x3 && row_len > 0) CHK(upload_split(e, Ah ? *Ah : A, &c.wx));      // the same image (grouped conv: the paired block-diagonal one), BN scale / shift stay in the epilogue
        return 0;
    };
    w = e->get("rx.conv1.w", {64, 1, 3, 3}); if (!w) return DMAD_ERR_STATE;
    CHK(up3("rx.conv1", e->rxconv1, w->v, 64));
    const int stages[4] = {64, 256, 512, 1024};
    for (int i = 0; i < 9; ++i) {
        dmad_engine::RxBlock& b = e->rx[i];
        const int st = i / 3, k = i % 3;
        b.cin = k == 0 ? stages[st] : stages[st + 1];
        b.cout = stages[st + 1];
        b.D = 8 * (64 * b.cout / 256);
        b.stride = (k == 0 && st > 0) ? 2 : 1;
        b.has_short = b.cin != b.cout;
        const std::string base = "rx.b" + std::to_string(i);
        w = e->get(base + ".reduce.w", {b.D, b.cin}); if (!w) return DMAD_ERR_STATE;
        CHK(up3(base + ".reduce", b.reduce, w->v, b.D, nullptr, nullptr, b.cin));
        const int G = b.D / 8;
        w = e->get(base + ".conv.w", {b.D, G, 3, 3}); if (!w) return DMAD_ERR_STATE;
        std::vector<float> A((size_t)8 * 9 * G * G);
        for (int g = 0; g < 8; ++g)
            for (int m = 0; m < G; ++m)
                for (int kk = 0; kk < G; ++kk)
                    for (int t = 0; t < 9; ++t)
                        A[(((size_t)g * 9 + t) * G + m) * G + kk] = w->v[(((size_t)g * G + m) * G + kk) * 9 + t];
        {   // f16 image of the grouped conv: [group][tap][Mg][Kg].  gemm_h16 needs Mg % 128 == 0: the 64-channel groups of stage 1
            // are paired into 128 x 128 block-diagonal groups (the off-diagonal blocks are zeros: twice the MFMAs on 17 % of the network)
            const int pair = G < 128 ? 2 : 1, Gp = G * pair, ngp = 8 / pair;
            std::vector<float> Ah((size_t)ngp * 9 * Gp * Gp, 0.f);
            std::vector<int> ch_of((size_t)ngp * 9 * Gp);
            for (int gp = 0; gp < ngp; ++gp)
                for (int t = 0; t < 9; ++t)
                    for (int m = 0; m < Gp; ++m) {
                        const int g = gp * pair + m / G, mm = m % G;
                        ch_of[((size_t)gp * 9 + t) * Gp + m] = g * G + mm;
                        for (int kk = 0; kk < G; ++kk)
                            Ah[(((size_t)gp * 9 + t) * Gp + m) * Gp + (m / G) * G + kk] = w->v[(((size_t)g * G + mm) * G + kk) * 9 + t];
                    }
            CHK(up3(base + ".conv", b.conv, A, b.D, &Ah, &ch_of, Gp));
        }
        w = e->get(base + ".expand.w", {b.cout, b.D}); if (!w) return DMAD_ERR_STATE;
        CHK(up3(base + ".expand", b.expand, w->v, b.cout, nullptr, nullptr, b.D));
        if (b.has_short) {
            w = e->get(base + ".short.w", {b.cout, b.cin}); if (!w) return DMAD_ERR_STATE;
            CHK(up3(base + ".short", b.shortc, w->v, b.cout, nullptr, nullptr, b.cin));
        }
    }
    w = e->get("rx.fc.w", {e->cfg.num_classes, 1024}); if (!w) return DMAD_ERR_STATE;
    CHK(e->upload(&e->rxfcw, w->v));
    w = e->get("rx.fc.b", {e->cfg.num_classes}); if (!w) return DMAD_ERR_STATE;
    CHK(e->upload(&e->rxfcb, w->v));
    const size_t B = (size_t)e->maxB;
    CHK(e->alloc(&e->rxX, B * 1024 * 256));
    CHK(e->alloc(&e->rxY, B * 1024 * 256));
    CHK(e->alloc(&e->rxS, B * 1024 * 256));
    CHK(e->alloc(&e->rxT1, B * 1024 * 1024));     // stage 2's first reduce: 32x32 pixels x D = 1024
    CHK(e->alloc(&e->rxT2, B * 1024 * 512));
    if (e->rx_h16) {
        CHK(e->alloc(&e->rxX16, B * 1024 * 256)); CHK(e->alloc(&e->rxY16, B * 1024 * 256)); CHK(e->alloc(&e->rxS16, B * 1024 * 256));
        CHK(e->alloc(&e->rxT1h, B * 1024 * 1024)); CHK(e->alloc(&e->rxT2h, B * 1024 * 512));
        CHK(need_kernels(KF_GEMM_H16));
    }
    if (e->rx_x3) CHK(need_kernels(KF_GEMM_X3));
    return 0;
}

// a loaded weight with its shape checked: DMAD_ERR_SHAPE names the network, the weight and both shapes (WideResNet, DenseNet)
int get_shaped(dmad_engine* e, const char* net, const std::string& name, std::initializer_list<int64_t> shape, const HostW** out) {
    auto it = e->hw.find(name);
    if (it == e->hw.end()) return fail(DMAD_ERR_STATE, "weight '%s' was not loaded", name.c_str());
    if (it->second.shape != std::vector<int64_t>(shape)) {
        std::string have, want;
        for (int64_t d : it->second.shape) have += (have.empty() ? "" : ",") + std::to_string(d);
        for (int64_t d : shape) want += (want.empty() ? "" : ",") + std::to_string(d);
        return fail(DMAD_ERR_SHAPE, "%s: weight '%s' is [%s], expected [%s]", net, name.c_str(), have.c_str(), want.c_str());
    }
    *out = &it->second;
    return 0;
}

// WideResNet-28-10 (models/wideresnet.py): names wrn.conv1.w [16,1,3,3]; per block i = 4 * stage + k: wrn.b<i>.bn1.{scale,
// shift} [cin], .conv1.w [cout,cin,3,3] with .conv1.{scale,shift} [cout] (the folded bn2), .conv2.w [cout,cout,3,3], .short.w [cout,cin]
// where cin != cout; wrn.bn.{scale,shift} [640], wrn.fc.w [classes,640], wrn.fc.b.  Every shape is checked (DMAD_ERR_SHAPE) before
// anything is uploaded.  The fp32 images serve every engine precision.
constexpr size_t kWrnMap = 163840;       // floats per spectrogram of the largest map: 32 x 32 x 160
int finalize_wrn(dmad_engine* e) {
    const int widths[4] = {16, 160, 320, 640}, nc = e->cfg.num_classes;
    auto wget = [&](const std::string& name, std::initializer_list<int64_t> shape, const HostW** out) { return get_shaped(e, "WideResNet-28-10", name, shape, out); };
    struct Src { const HostW *s1, *b1, *w1, *s2, *b2, *w2, *ws; };
    Src src[12];
    const HostW *stem, *bns, *bnb, *fcw, *fcb;
    CHK(wget("wrn.conv1.w", {16, 1, 3, 3}, &stem));
    for (int i = 0; i < 12; ++i) {
        dmad_engine::WrnBlock& b = e->wrn[i];
        const int st = i / 4, k = i % 4;
        b.cin = k == 0 ? widths[st] : widths[st + 1];
        b.cout = widths[st + 1];
        b.stride = (k == 0 && st > 0) ? 2 : 1;
        const std::string base = "wrn.b" + std::to_string(i);
        CHK(wget(base + ".bn1.scale", {b.cin}, &src[i].s1));
        CHK(wget(base + ".bn1.shift", {b.cin}, &src[i].b1));
        CHK(wget(base + ".conv1.w", {b.cout, b.cin, 3, 3}, &src[i].w1));
        CHK(wget(base + ".conv1.scale", {b.cout}, &src[i].s2));
        CHK(wget(base + ".conv1.shift", {b.cout}, &src[i].b2));
        CHK(wget(base + ".conv2.w", {b.cout, b.cout, 3, 3}, &src[i].w2));
        src[i].ws = nullptr;
        if (b.cin != b.cout) CHK(wget(base + ".short.w", {b.cout, b.cin}, &src[i].ws));
    }
    CHK(wget("wrn.bn.scale", {640}, &bns));
    CHK(wget("wrn.bn.shift", {640}, &bnb));
    CHK(wget("wrn.fc.w", {nc, 640}, &fcw));
    CHK(wget("wrn.fc.b", {nc}, &fcb));
    CHK(e->upload(&e->wrn_stem, stem->v));
    for (int i = 0; i < 12; ++i) {
        dmad_engine::WrnBlock& b = e->wrn[i];
        CHK(e->upload(&b.s1, src[i].s1->v)); CHK(e->upload(&b.b1, src[i].b1->v));
        CHK(e->upload(&b.w1, conv3_image(src[i].w1->v, b.cout, b.cin)));
        CHK(e->upload(&b.s2, src[i].s2->v)); CHK(e->upload(&b.b2, src[i].b2->v));
        CHK(e->upload(&b.w2, conv3_image(src[i].w2->v, b.cout, b.cout)));
        if (src[i].ws) CHK(e->upload(&b.ws, src[i].ws->v));
    }
    CHK(e->upload(&e->wrn_bns, bns->v)); CHK(e->upload(&e->wrn_bnb, bnb->v));
    CHK(e->upload(&e->wrn_fcw, fcw->v)); CHK(e->upload(&e->wrn_fcb, fcb->v));
    std::vector<float> ws((size_t)nc * 640);                  // the head backward's image: fc.w[k][c] * bn.scale[c], rounded once
    for (int k = 0; k < nc; ++k)
        for (int c = 0; c < 640; ++c) ws[(size_t)k * 640 + c] = (float)((double)fcw->v[(size_t)k * 640 + c] * (double)bns->v[c]);
    CHK(e->upload(&e->wrn_fcws, ws));
    const size_t B = (size_t)e->maxB;
    CHK(e->alloc(&e->wrnX, B * kWrnMap)); CHK(e->alloc(&e->wrnY, B * kWrnMap)); CHK(e->alloc(&e->wrnO, B * kWrnMap));
    CHK(e->alloc(&e->wrnH, B * kWrnMap)); CHK(e->alloc(&e->wrnS, B * kWrnMap));         // the shortcut's map: 32 x 32 x 160 in block 0
    CHK(e->alloc(&e->wrnP, B * 640));
    return 0;
}

// WideResNet.forward on NHWC fp32 maps: the stem kernel, then per block the pre-activation o = relu(bn1(x)) (wrn.hip), conv1 with bn2 and
// the ReLU in its epilogue, the shortcut (the raw x, or in a stage's first block the 1x1 conv of the ACTIVATED o) and conv2 with the
// shortcut as its residual; the final pre-activation, the 8 x 8 average pool and the FC.  Every GEMM gets the split-K slab and the row
// count of a max_batch launch, so a sample's logits do not depend on its batch.  tape != nullptr (the VJP; B <= cvjpB): o and h of block i go
// to the tape's slots 2 i and 2 i + 1 and the final map to slot 24 instead of the work maps (same launches, same n_ref, same bits)
int classify_wrn(dmad_engine* e, const float* spec, int B, float* logits, hipStream_t s, const dmad_engine::TapeSlot* tape = nullptr) {
    float *X = e->wrnX, *Y = e->wrnY;
    launch_wrn_stem(spec, e->wrn_stem, X, B, s);
    int H = 32;
    for (int i = 0; i < 12; ++i) {
        const dmad_engine::WrnBlock& b = e->wrn[i];
        float* O = tape ? tape[2 * i].p : e->wrnO;
        float* Hm = tape ? tape[2 * i + 1].p : e->wrnH;
        const int Ho = (H - 1) / b.stride + 1;
        const long nref_out = (long)e->maxB * Ho * Ho;
        launch_wrn_preact(X, b.s1, b.b1, O, (long)B * H * H, b.cin, s);
        launch_gemm_f32(nhwc_conv_args(b.w1, b.s2, b.b2, O, Hm, b.cout, b.cin, 9, B, H, b.stride, nullptr, 1), s, e->slab, e->slab_floats, nref_out);
        const float* res = X;
        if (b.ws) {
            launch_gemm_f32(nhwc_conv_args(b.ws, nullptr, nullptr, O, e->wrnS, b.cout, b.cin, 1, B, H, b.stride, nullptr), s, e->slab, e->slab_floats,
                            nref_out);
            res = e->wrnS;
        }
        launch_gemm_f32(nhwc_conv_args(b.w2, nullptr, nullptr, Hm, Y, b.cout, b.cout, 9, B, Ho, 1, res), s, e->slab, e->slab_floats, nref_out);
        std::swap(X, Y);
        H = Ho;
    }
    float* F = tape ? tape[24].p : e->wrnO;
    launch_wrn_preact(X, e->wrn_bns, e->wrn_bnb, F, (long)B * 64, 640, s);
    launch_avgpool_nhwc(F, e->wrnP, B, 64, 640, s);
    launch_gemm_f32(plain_gemm(e->wrn_fcw, e->wrnP, logits, nullptr, e->wrn_fcb, e->cfg.num_classes, 640, B, e->cfg.num_classes, 640, 0), s, e->slab,
                    e->slab_floats, (long)e->maxB);
    LASTCHK();
    return 0;
}

// DenseNet-BC-100-12 (models/densenet.py): names dn.conv1.w [24,1,3,3]; per layer l = 16 * block + i: dn.l<l>.bn1.{scale,shift}
// [cin], .conv1.w [48,cin] with .conv1.{scale,shift} [48] (the folded bn2), .conv2.w [12,48,3,3]; per transition j: dn.t<j>.bn.{scale,shift}
// [cin], .conv.w [cout,cin]; dn.bn.{scale,shift} [342], dn.fc.w [classes,342], dn.fc.b.  Every shape is checked (DMAD_ERR_SHAPE) before
// anything is uploaded.  One stream per resolution: logical widths kDnWidth at the pitches kDnPitch (multiples of 8: every row, every
// layer's slice and every float2 / float4 access is aligned); a block starts with kDnC0 channels.
constexpr int kDnH[3] = {32, 16, 8}, kDnC0[3] = {24, 108, 150}, kDnWidth[3] = {216, 300, 342}, kDnPitch[3] = {216, 304, 344};
inline int up4(int k) { return (k + 3) & ~3; }
int finalize_dn(dmad_engine* e) {
    const int nc = e->cfg.num_classes;
    auto wget = [&](const std::string& name, std::initializer_list<int64_t> shape, const HostW** out) { return get_shaped(e, "DenseNet-BC-100-12", name, shape, out); };
    struct Src { const HostW *s1, *b1, *w1, *s2, *b2, *w2; };
    Src src[48];
    const HostW *ts[2], *tb[2], *tw[2], *stem, *bns, *bnb, *fcw, *fcb;
    CHK(wget("dn.conv1.w", {24, 1, 3, 3}, &stem));
    for (int l = 0; l < 48; ++l) {
        dmad_engine::DnLayer& L = e->dn[l];
        L.blk = l / 16;
        L.cin = kDnC0[L.blk] + 12 * (l % 16);
        const std::string base = "dn.l" + std::to_string(l);
        CHK(wget(base + ".bn1.scale", {L.cin}, &src[l].s1));
        CHK(wget(base + ".bn1.shift", {L.cin}, &src[l].b1));
        CHK(wget(base + ".conv1.w", {48, L.cin}, &src[l].w1));
        CHK(wget(base + ".conv1.scale", {48}, &src[l].s2));
        CHK(wget(base + ".conv1.shift", {48}, &src[l].b2));
        CHK(wget(base + ".conv2.w", {12, 48, 3, 3}, &src[l].w2));
    }
    for (int j = 0; j < 2; ++j) {
        dmad_engine::DnTrans& T = e->dnT[j];
        T.cin = kDnWidth[j]; T.cout = kDnC0[j + 1];
        const std::string base = "dn.t" + std::to_string(j);
        CHK(wget(base + ".bn.scale", {T.cin}, &ts[j]));
        CHK(wget(base + ".bn.shift", {T.cin}, &tb[j]));
        CHK(wget(base + ".conv.w", {T.cout, T.cin}, &tw[j]));
    }
    CHK(wget("dn.bn.scale", {342}, &bns));
    CHK(wget("dn.bn.shift", {342}, &bnb));
    CHK(wget("dn.fc.w", {nc, 342}, &fcw));
    CHK(wget("dn.fc.b", {nc}, &fcb));
    // [M][K] -> [M][up4(K)] with zero columns (T = false) or its transpose [K][up4(M)] (T = true): the 1x1 images, forward and backward
    auto pw_image = [&](const std::vector<float>& w, int M, int K, bool T, float** dst) -> int {
        const int R = T ? K : M, Cn = T ? M : K, C4 = up4(Cn);
        std::vector<float> A((size_t)R * C4, 0.f);
        for (int r = 0; r < R; ++r)
            for (int c = 0; c < Cn; ++c) A[(size_t)r * C4 + c] = T ? w[(size_t)c * K + r] : w[(size_t)r * K + c];
        return e->upload(dst, A);
    };
    CHK(e->upload(&e->dn_stem, stem->v));
    for (int l = 0; l < 48; ++l) {
        dmad_engine::DnLayer& L = e->dn[l];
        CHK(e->upload(&L.s1, src[l].s1->v)); CHK(e->upload(&L.b1, src[l].b1->v));
        CHK(pw_image(src[l].w1->v, 48, L.cin, false, &L.w1));
        CHK(pw_image(src[l].w1->v, 48, L.cin, true, &L.w1T));
        CHK(e->upload(&L.s2, src[l].s2->v)); CHK(e->upload(&L.b2, src[l].b2->v));
        const std::vector<float>& w2 = src[l].w2->v;                       // [12][48][3][3]
        std::vector<float> A((size_t)16 * 432, 0.f), AT((size_t)48 * 108);
        for (int j = 0; j < 12; ++j)
            for (int c = 0; c < 48; ++c)
                for (int t = 0; t < 9; ++t) {
                    const float v = w2[((size_t)j * 48 + c) * 9 + t];
                    A[(size_t)j * 432 + t * 48 + c] = v;
                    AT[(size_t)c * 108 + (8 - t) * 12 + j] = v;
                }
        CHK(e->upload(&L.w2, A)); CHK(e->upload(&L.w2T, AT));
    }
    for (int j = 0; j < 2; ++j) {
        dmad_engine::DnTrans& T = e->dnT[j];
        CHK(e->upload(&T.s, ts[j]->v)); CHK(e->upload(&T.b, tb[j]->v));
        CHK(pw_image(tw[j]->v, T.cout, T.cin, false, &T.w));
        CHK(pw_image(tw[j]->v, T.cout, T.cin, true, &T.wT));
    }
    CHK(e->upload(&e->dn_bns, bns->v)); CHK(e->upload(&e->dn_bnb, bnb->v));
    CHK(e->upload(&e->dn_fcw, fcw->v)); CHK(e->upload(&e->dn_fcb, fcb->v));
    std::vector<float> ws((size_t)nc * 342);                  // the head backward's image: fc.w[k][c] * bn.scale[c], rounded once
    for (int k = 0; k < nc; ++k)
        for (int c = 0; c < 342; ++c) ws[(size_t)k * 342 + c] = (float)((double)fcw->v[(size_t)k * 342 + c] * (double)bns->v[c]);
    CHK(e->upload(&e->dn_fcws, ws));
    const size_t B = (size_t)e->maxB;
    for (int k = 0; k < 3; ++k) CHK(e->alloc(&e->dnS[k], B * kDnH[k] * kDnH[k] * kDnPitch[k]));
    CHK(e->alloc(&e->dnH, B * 1024 * 48));
    CHK(e->alloc(&e->dnTm, B * 1024 * 108));
    return 0;
}

DnPwArgs dn_pw_fwd(const float* A, int M, int K, const float* in, int ldi, long n_px, const float* s_in, const float* b_in, const float* s_out,
                   const float* b_out, float* out, int ldo) {
    DnPwArgs a{};
    a.A = A; a.M = M; a.K = K; a.K4 = up4(K); a.in = in; a.ldi = ldi; a.n_px = n_px;
    a.s_in = s_in; a.b_in = b_in; a.s_out = s_out; a.b_out = b_out; a.out = out; a.ldo = ldo;
    return a;
}
DnPwArgs dn_pw_bwd(const float* A, int M, int K, const float* g, int ldg, long n_px, int pool, int H, const float* x, int ldx, const float* s1,
                   const float* b1, float* out, int ldo, int add) {
    DnPwArgs a{};
    a.A = A; a.M = M; a.K = K; a.K4 = up4(K); a.in = g; a.ldi = ldg; a.n_px = n_px; a.pool = pool; a.H = H;
    a.x = x; a.ldx = ldx; a.s1 = s1; a.b1 = b1; a.out = out; a.ldo = ldo; a.add = add;
    return a;
}

// DenseNet.forward: the stem into stream 0; per layer the bottleneck kernel (bn1 + ReLU while staging, 1x1 on the MFMA, bn2 + ReLU as the
// epilogue -> h) and the growth kernel (3x3, 12 channels into the stream's next slice): 2 launches; per transition the same 1x1 kernel
// without epilogue and the 2x2 average pool into the next stream; the head kernel.  102 launches.  Every kernel works pixel by pixel, so
// a sample's logits do not depend on its batch.  tape != nullptr (the VJP; B <= cvjpB): the three streams and the 48 h maps go to the
// tape's slots instead of the work maps (same launches, same bits)
int classify_dn(dmad_engine* e, const float* spec, int B, float* logits, hipStream_t s, const dmad_engine::TapeSlot* tape = nullptr) {
    float* S[3];
    for (int k = 0; k < 3; ++k) S[k] = tape ? tape[k].p : e->dnS[k];
    launch_dn_stem(spec, e->dn_stem, S[0], kDnPitch[0], B, s);
    for (int blk = 0; blk < 3; ++blk) {
        const int H = kDnH[blk], ld = kDnPitch[blk];
        const long n_px = (long)B * H * H;
        for (int l = 16 * blk; l < 16 * blk + 16; ++l) {
            const dmad_engine::DnLayer& L = e->dn[l];
            float* Hm = tape ? tape[3 + l].p : e->dnH;
            launch_dn_pw(dn_pw_fwd(L.w1, 48, L.cin, S[blk], ld, n_px, L.s1, L.b1, L.s2, L.b2, Hm, 48), false, s);
            launch_dn_growth(L.w2, Hm, S[blk], ld, L.cin, B, H, s);
        }
        if (blk < 2) {
            const dmad_engine::DnTrans& T = e->dnT[blk];
            launch_dn_pw(dn_pw_fwd(T.w, T.cout, T.cin, S[blk], ld, n_px, T.s, T.b, nullptr, nullptr, e->dnTm, up4(T.cout)), false, s);
            launch_dn_pool(e->dnTm, up4(T.cout), S[blk + 1], kDnPitch[blk + 1], B, H, T.cout, s);
        }
    }
    launch_dn_head(S[2], kDnPitch[2], e->dn_bns, e->dn_bnb, e->dn_fcw, e->dn_fcb, logits, B, 64, 342, e->cfg.num_classes, s);
    LASTCHK();
    return 0;
}

// The same network on its SPLIT-F16 tier (exact-vote engines): the fp32 pipeline's structure with every conv on split-f16 operands (three f16
// MFMAs per product, ~22 significant bits: gemm_x3_kernel's NHWC form, grouped for the 3x3), the eval-mode BatchNorm scale / shift, the
// shortcut add and the ReLU in the fp32 epilogue; a map that only feeds GEMMs (and, as a block output, the next shortcut add) is written
// in the split format directly.  Stage 1's 64-channel groups are paired into 128 x 128 block-diagonal groups (the kernel's tiles need
// 128 rows), like on the 16-bit tier.  Average pool and head in fp32.
int classify_resnext_x3(dmad_engine* e, const float* spec, int B, float* logits, hipStream_t s) {
    float *X = e->rxX, *Y = e->rxY;
    launch_vgg_conv1(spec, e->rxconv1.w, e->rxconv1.scale, e->rxconv1.shift, X, B, s);      // 1 -> 64, 3x3, BN, ReLU (direct kernel, fp32)
    launch_scale(X, 1.f, X, (long)B * 1024 * 64, s, true);                                   // ... as a split-format operand, in place
    int H = 32;
    for (int i = 0; i < 9; ++i) {
        const dmad_engine::RxBlock& b = e->rx[i];
        const int Ho = (H - 1) / b.stride + 1;
        auto mk = [&](const dmad_engine::RxConv& c, const float* in, float* out, int M, int K, int taps, int Hin, int ldx, int ldc, int stride, int relu, int out_split) {
            GemmF32Args g = nhwc_conv_args(c.wx, c.scale, c.shift, in, out, M, K, taps, B, Hin, stride, nullptr, relu, 0, ldx, ldc);
            g.x3 = 1; g.out_split = out_split;
            return g;
        };
        launch_gemm_f32(mk(b.reduce, X, e->rxT1, b.D, b.cin, 1, H, b.cin, b.D, 1, 1, 1), s);                 // conv_reduce + bn + ReLU
        const int G = b.D / 8, pair = G < 128 ? 2 : 1;
        GemmF32Args c = mk(b.conv, e->rxT1, e->rxT2, G * pair, G * pair, 9, H, b.D, b.D, b.stride, 1, 1);    // grouped 3x3 (stride) + bn + ReLU
        c.groups = 8 / pair;
        launch_gemm_f32(c, s);
        GemmF32Args x = mk(b.expand, e->rxT2, Y, b.cout, b.D, 1, Ho, b.D, b.cout, 1, 1, i == 8 ? 0 : 1);    // conv_expand + bn + shortcut, ReLU
        if (b.has_short) {
            launch_gemm_f32(mk(b.shortc, X, e->rxS, b.cout, b.cin, 1, H, b.cin, b.cout, b.stride, 0, 0), s);  // shortcut conv + bn: fp32
            x.res = e->rxS;
        } else {
            x.res = X; x.res_split = 1;                                                                              // the block input exists in the split format only
        }
        launch_gemm_f32(x, s);
        float* t = X; X = Y; Y = t;
        H = Ho;
    }
    launch_avgpool_nhwc(X, e->rxT2, B, H * H, 1024, s);
    launch_gemm_f32(plain_gemm(e->rxfcw, e->rxT2, logits, nullptr, e->rxfcb, e->cfg.num_classes, 1024, B, e->cfg.num_classes, 1024, 0), s,
                    e->slab, e->slab_floats, (long)e->maxB);
    LASTCHK();
    return 0;
}

// The same network on its 16-bit tier: f16 maps, every conv through gemm_h16 (BN scale folded into the f16 weights, shift / shortcut /
// ReLU in the fp32 epilogue); the last bottleneck writes fp32 for the average pool and the fp32 classifier head.
int classify_resnext_h16(dmad_engine* e, const float* spec, int B, float* logits, hipStream_t s) {
    h16_t *X = e->rxX16, *Y = e->rxY16;
    launch_vgg_conv1(spec, e->rxconv1.w, e->rxconv1.scale, e->rxconv1.shift, nullptr, B, s, X);
    int H = 32;
    for (int i = 0; i < 9; ++i) {
        const dmad_engine::RxBlock& b = e->rx[i];
        const int Ho = (H - 1) / b.stride + 1;
        const long Nin = (long)B * H * H, Nout = (long)B * Ho * Ho;
        auto mk = [&](const dmad_engine::RxConv& c, const h16_t* in, h16_t* out16, int M, int K, int taps, long N, int Hin, int ldx, int ldc, int stride) {
            GemmH16Args g{};
            g.A = c.wh; g.X = in; g.C16 = out16; g.shift = c.shift; g.M = M; g.K = K; g.taps = taps; g.ldc = ldc; g.N = N; g.H = Hin; g.W = Hin;
            g.ldx = ldx; g.stride = stride; g.relu = 1;
            return g;
        };
        launch_gemm_h16(mk(b.reduce, X, e->rxT1h, b.D, b.cin, 1, Nin, H, b.cin, b.D, 1), s);                      // conv_reduce + bn + ReLU
        const int G = b.D / 8, pair = G < 128 ? 2 : 1;
        GemmH16Args c = mk(b.conv, e->rxT1h, e->rxT2h, G * pair, G * pair, 9, Nout, H, b.D, b.D, b.stride);         // grouped 3x3 (stride) + bn + ReLU
        c.groups = 8 / pair;
        launch_gemm_h16(c, s);
        const h16_t* res = X;
        if (b.has_short) {
            GemmH16Args h = mk(b.shortc, X, e->rxS16, b.cout, b.cin, 1, Nout, H, b.cin, b.cout, b.stride);         // shortcut conv + bn (no ReLU)
            h.relu = 0;
            launch_gemm_h16(h, s);
            res = e->rxS16;
        }
        GemmH16Args x = mk(b.expand, e->rxT2h, i == 8 ? nullptr : Y, b.cout, b.D, 1, Nout, Ho, b.D, b.cout, 1);   // conv_expand + bn + shortcut, ReLU
        x.res16 = res;
        if (i == 8) x.C = e->rxY;
        launch_gemm_h16(x, s);
        h16_t* t = X; X = Y; Y = t;
        H = Ho;
    }
    launch_avgpool_nhwc(e->rxY, e->rxT2, B, H * H, 1024, s);
    launch_gemm_f32(plain_gemm(e->rxfcw, e->rxT2, logits, nullptr, e->rxfcb, e->cfg.num_classes, 1024, B, e->cfg.num_classes, 1024, 0), s,
                    e->slab, e->slab_floats, (long)e->maxB);
    LASTCHK();
    return 0;
}

// CifarResNeXt.forward (models/resnext.py:133-142) on NHWC fp32 maps.  tape != nullptr (the classifier VJP; B <= cvjpB): conv1's
// output goes to the tape's slot 0 and bottleneck i's T1 / T2 / block output to slots 3 i + 1 / + 2 / + 3 instead of the work maps (same
// launches, same bits)
int classify_resnext(dmad_engine* e, const float* spec, int B, float* logits, hipStream_t s, const dmad_engine::TapeSlot* tape = nullptr) {
    float *X = tape ? tape[0].p : e->rxX, *Y = e->rxY;
    launch_vgg_conv1(spec, e->rxconv1.w, e->rxconv1.scale, e->rxconv1.shift, X, B, s);      // 1 -> 64, 3x3, BN, ReLU
    int H = 32;
    for (int i = 0; i < 9; ++i) {
        const dmad_engine::RxBlock& b = e->rx[i];
        float* T1 = tape ? tape[3 * i + 1].p : e->rxT1;
        float* T2 = tape ? tape[3 * i + 2].p : e->rxT2;
        if (tape) Y = tape[3 * i + 3].p;
        const int Ho = (H - 1) / b.stride + 1;
        const long Nin = (long)B * H * H, Nout = (long)B * Ho * Ho, nref_in = (long)e->maxB * H * H, nref_out = (long)e->maxB * Ho * Ho;
        // conv_reduce + bn_reduce + ReLU (1x1)
        GemmF32Args g = plain_gemm(b.reduce.w, X, T1, b.reduce.scale, b.reduce.shift, b.D, b.cin, Nin, b.D, b.cin, 1);
        launch_gemm_f32(g, s, e->slab, e->slab_floats, nref_in);
        // conv_conv (3x3, 8 groups, stride) + bn + ReLU
        launch_gemm_f32(nhwc_conv_args(b.conv.w, b.conv.scale, b.conv.shift, T1, T2, b.D / 8, b.D / 8, 9, B, H, b.stride, nullptr, 1, 8, b.D, b.D), s);
        // shortcut: identity, or 1x1 conv (stride) + BN
        const float* res = X;
        if (b.has_short) {
            launch_gemm_f32(nhwc_conv_args(b.shortc.w, b.shortc.scale, b.shortc.shift, X, e->rxS, b.cout, b.cin, 1, B, H, b.stride, nullptr), s, e->slab,
                            e->slab_floats, nref_out);
            res = e->rxS;
        }
        // conv_expand + bn_expand, + shortcut, ReLU
        GemmF32Args x = plain_gemm(b.expand.w, T2, Y, b.expand.scale, b.expand.shift, b.cout, b.D, Nout, b.cout, b.D, 1);
        x.res = res;
        launch_gemm_f32(x, s, e->slab, e->slab_floats, nref_out);
        if (tape) { X = Y; H = Ho; continue; }
        float* t = X; X = Y; Y = t;
        H = Ho;
    }
    launch_avgpool_nhwc(X, e->rxT2, B, H * H, 1024, s);
    launch_gemm_f32(plain_gemm(e->rxfcw, e->rxT2, logits, nullptr, e->rxfcb, e->cfg.num_classes, 1024, B, e->cfg.num_classes, 1024, 0), s,
                    e->slab, e->slab_floats, (long)e->maxB);
    LASTCHK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Improved-Diffusion UNet.  Configuration of the reference's wrapper (improved_diffusion_ddpm.py:
// 64-93 + script_util.py:11-34,100-131): 1 -> 128 channels, 3 ResBlocks per level, channel_mult (1,2,2,2), attention at
// 16x16 and 8x8 (+ the middle block), 4 heads, scale-shift norm, epsilon output.  Weight names = "un." + the reference's
// state-dict names.  Every conv / linear is a gemm_f32 launch over NHWC maps.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kUnMC = 128, kUnTE = 512, kUnHeads = 4, kUnRes = 3;
constexpr int kUnSsSteps = 1000;         // cached steps (create_improved_diffusion: diffusion_steps = 1000)
const int kUnMult[4] = {1, 2, 2, 2};
inline bool un_attn_at(int ds) { return ds == 2 || ds == 4; }

int un_conv3(dmad_engine* e, const std::string& name, int cout, int cin, float** w, float** b, h16_t** wh = nullptr, float** wx = nullptr) {
    const HostW* h = e->get(name + ".weight", {cout, cin, 3, 3}); if (!h) return DMAD_ERR_STATE;
    const std::vector<float> A = conv3_image(h->v, cout, cin);
    CHK(e->upload(w, A));
    if (wh && e->un_h16) CHK(upload_h16(e, A, wh));
    if (wx && e->un_x3) CHK(upload_split(e, A, wx));
    h = e->get(name + ".bias", {cout}); if (!h) return DMAD_ERR_STATE;
    CHK(e->upload(b, h->v));
    return 0;
}
int un_dense(dmad_engine* e, const std::string& name, int out, int in, float** w, float** b, h16_t** wh = nullptr, float** wx = nullptr) {
    const HostW* h = e->get(name + ".weight", {out, in}); if (!h) return DMAD_ERR_STATE;
    CHK(e->upload(w, h->v));
    if (wh && e->un_h16) CHK(upload_h16(e, h->v, wh));
    if (wx && e->un_x3) CHK(upload_split(e, h->v, wx));
    h = e->get(name + ".bias", {out}); if (!h) return DMAD_ERR_STATE;
    CHK(e->upload(b, h->v));
    return 0;
}
int un_load_op(dmad_engine* e, const std::string& p, dmad_engine::UnOp& o) {
    if (o.kind == 0) {
        const HostW* h = e->get(p + ".weight", {o.cout, 1, 3, 3}); if (!h) return DMAD_ERR_STATE;
        CHK(e->upload(&o.w1, h->v));
        h = e->get(p + ".bias", {o.cout}); if (!h) return DMAD_ERR_STATE;
        CHK(e->upload(&o.b1, h->v));
    } else if (o.kind == 1) {
        CHK(un_dense(e, p + ".in_layers.0", o.cin, 1, &o.gn1w, &o.gn1b));
        CHK(un_conv3(e, p + ".in_layers.2", o.cout, o.cin, &o.w1, &o.b1, &o.w1h, &o.w1x));
        CHK(un_dense(e, p + ".emb_layers.1", 2 * o.cout, kUnTE, &o.embw, &o.embb));
        CHK(un_dense(e, p + ".out_layers.0", o.cout, 1, &o.gn2w, &o.gn2b));
        CHK(un_conv3(e, p + ".out_layers.3", o.cout, o.cout, &o.w2, &o.b2, &o.w2h, &o.w2x));
        if (o.cin != o.cout) CHK(un_dense(e, p + ".skip_connection", o.cout, o.cin, &o.skw, &o.skb, &o.skwh, &o.skwx));
        o.ss_off = e->un_ss_total;
        e->un_ss_total += (size_t)2 * o.cout;
    } else if (o.kind == 2) {
        CHK(un_dense(e, p + ".norm", o.cin, 1, &o.gn1w, &o.gn1b));
        CHK(un_dense(e, p + ".qkv", 3 * o.cin, o.cin, &o.w1, &o.b1, &o.w1h, &o.w1x));
        CHK(un_dense(e, p + ".proj_out", o.cin, o.cin, &o.w2, &o.b2, &o.w2h, &o.w2x));
    } else if (o.kind == 3) {
        CHK(un_conv3(e, p + ".op", o.cout, o.cin, &o.w1, &o.b1, &o.w1h, &o.w1x));
    } else {
        CHK(un_conv3(e, p + ".conv", o.cout, o.cin, &o.w1, &o.b1, &o.w1h, &o.w1x));
    }
    return 0;
}

int finalize_unet(dmad_engine* e) {
    // enumerate the modules exactly as UNetModel.__init__ builds them (unet.py:338-421), in forward order; a module's weights are named
    // after its place there: <prefix of its block>.<index in the block>
    e->un_ops.clear(); e->un_hs_ch.clear(); e->un_hs_hw.clear();      // (a retry after a finalise that failed on a missing weight starts over)
    std::vector<std::string> names;
    std::string prefix;
    int ch = kUnMC, ds = 1, hw = 1024, H = 32, j = 0, pend = -1;
    auto block = [&](const char* list, int i) { prefix = std::string("un.") + list + (i < 0 ? "" : "." + std::to_string(i)); j = 0; };
    auto add = [&](int kind, int cin, int cout, int top = -1) {
        dmad_engine::UnOp o;
        o.kind = kind; o.cin = cin; o.cout = cout; o.H = H; o.top = top; o.acc = pend;
        e->un_ops.push_back(o);
        names.push_back(prefix + "." + std::to_string(j++));
        pend = -1;
        H = kind == 3 ? H / 2 : kind == 4 ? H * 2 : H;
    };
    auto saved = [&]() {                    // hs.append(h): the block's output is a saved map, and the next module reads it
        e->un_ops.back().save = pend = (int)e->un_hs_ch.size();
        e->un_hs_ch.push_back(ch); e->un_hs_hw.push_back(hw);
    };
    int nb = 0;
    block("input_blocks", nb++); add(0, 1, kUnMC); saved();
    for (int level = 0; level < 4; ++level) {
        for (int r = 0; r < kUnRes; ++r) {
            block("input_blocks", nb++); add(1, ch, kUnMult[level] * kUnMC);
            ch = kUnMult[level] * kUnMC;
            if (un_attn_at(ds)) add(2, ch, ch);
            saved();
        }
        if (level != 3) {
            block("input_blocks", nb++); add(3, ch, ch);
            ds *= 2; hw /= 4;
            saved();
        }
    }
    block("middle_block", -1); add(1, ch, ch); add(2, ch, ch); add(1, ch, ch);
    int top = (int)e->un_hs_ch.size();      // hs.pop()
    nb = 0;
    for (int level = 3; level >= 0; --level)
        for (int i = 0; i <= kUnRes; ++i) {
            --top;
            block("output_blocks", nb++); add(1, ch + e->un_hs_ch[top], kUnMC * kUnMult[level], top);
            ch = kUnMC * kUnMult[level];
            if (un_attn_at(ds)) add(2, ch, ch);
            if (level && i == kUnRes) { add(4, ch, ch); ds /= 2; }
        }
    for (size_t k = 0; k < names.size(); ++k) CHK(un_load_op(e, names[k], e->un_ops[k]));
    CHK(un_dense(e, "un.time_embed.0", kUnTE, kUnMC, &e->un_te0w, &e->un_te0b));
    CHK(un_dense(e, "un.time_embed.2", kUnTE, kUnTE, &e->un_te2w, &e->un_te2b));
    CHK(un_dense(e, "un.out.0", kUnMC, 1, &e->un_outgw, &e->un_outgb));
    CHK(un_conv3(e, "un.out.2", 1, kUnMC, &e->un_outw, &e->un_outb));
    const size_t B = (size_t)e->maxB;
    for (size_t i = 0; i < e->un_hs_ch.size(); ++i) {
        float* p = nullptr;
        CHK(e->alloc(&p, B * e->un_hs_hw[i] * e->un_hs_ch[i]));
        e->un_hs.push_back(p);
    }
    for (int i = 0; i < 8; ++i) CHK(e->alloc(&e->un_buf[i], B * 1024 * 384));     // largest map: 32x32 x (256 + 128) concat
    CHK(e->alloc(&e->un_eps, B * 1024));
    if (e->un_h16) {
        for (size_t i = 0; i < e->un_hs_ch.size(); ++i) {
            h16_t* p = nullptr;
            CHK(e->alloc(&p, B * e->un_hs_hw[i] * e->un_hs_ch[i]));
            e->un_hs16.push_back(p);
        }
        for (int i = 0; i < 3; ++i) CHK(e->alloc(&e->un_buf16[i], B * 1024 * 384));
        // statistics slabs: [pixels / 64][channels / 4][2] floats = 1 / 32 float per map value
        for (int i = 0; i < 3; ++i) CHK(e->alloc(&e->un_st_buf[i], B * 1024 * 384 / 32));
        CHK(e->alloc(&e->un_st_t2, B * 1024 * 256 / 32));
        for (size_t i = 0; i < e->un_hs_ch.size(); ++i) {
            float* p = nullptr;
            CHK(e->alloc(&p, B * e->un_hs_hw[i] * e->un_hs_ch[i] / 32 + 64));
            e->un_st_hs.push_back(p);
        }
        CHK(e->alloc(&e->un_t1h, B * 1024 * 384));
        CHK(e->alloc(&e->un_t2h, B * 1024 * 256));
        CHK(e->alloc(&e->un_uph, B * 1024 * 256));
        CHK(e->alloc(&e->un_atth, B * 256 * 256));
        CHK(e->alloc(&e->un_qkvh, B * 256 * 768));
        CHK(need_kernels(KF_GEMM_H16));
    }
    if (e->un_x3) CHK(need_kernels(KF_GEMM_X3));
    CHK(e->alloc(&e->un_ss_table, (size_t)(kUnSsSteps + 1) * e->un_ss_total));
    e->un_ss_have.assign(kUnSsSteps, 0);
    e->un_t = -1;
    CHK(e->alloc(&e->un_temb, kUnMC)); CHK(e->alloc(&e->un_emb1, kUnTE)); CHK(e->alloc(&e->un_emb, kUnTE)); CHK(e->alloc(&e->un_semb, kUnTE));
    return 0;
}

// emb = time_embed(timestep_embedding(t)) (unet.py:466, nn.py:103-121), SiLU(emb), and every ResBlock's (scale, shift) row
int unet_prepare_step(dmad_engine* e, int t, hipStream_t s) {
    if (e->un_t == t) return 0;
    const int slot = t < kUnSsSteps ? t : kUnSsSteps;
    float* row = e->un_ss_table + (size_t)slot * e->un_ss_total;
    e->un_ss_cur = row;
    e->un_t = t;
    if (slot < kUnSsSteps && e->un_ss_have[slot]) return 0;
    float te[kUnMC];
    const float a = (float)(-log(10000.0));
    for (int i = 0; i < kUnMC / 2; ++i) {
        const float f = expf(a * (float)i / (float)(kUnMC / 2));
        const float arg = (float)t * f;
        te[i] = cosf(arg);
        te[kUnMC / 2 + i] = sinf(arg);
    }
    static_assert(kUnMC == 128, "launch_store_vec128 carries 128 floats");
    launch_store_vec128(te, e->un_temb, s); // as a kernel argument: no host buffer to keep alive, no synchronisation
    launch_gemm_f32(plain_gemm(e->un_te0w, e->un_temb, e->un_emb1, nullptr, e->un_te0b, kUnTE, kUnMC, 1, kUnTE, kUnMC, 0), s);
    launch_silu(e->un_emb1, e->un_emb1, kUnTE, s);
    launch_gemm_f32(plain_gemm(e->un_te2w, e->un_emb1, e->un_emb, nullptr, e->un_te2b, kUnTE, kUnTE, 1, kUnTE, kUnTE, 0), s);
    launch_silu(e->un_emb, e->un_semb, kUnTE, s);
    for (const auto& o : e->un_ops)
        if (o.kind == 1)
            launch_gemm_f32(plain_gemm(o.embw, e->un_semb, row + o.ss_off, nullptr, o.embb, 2 * o.cout, kUnTE, 1, 2 * o.cout, kUnTE, 0), s);
    if (slot < kUnSsSteps) e->un_ss_have[slot] = 1;
    return 0;
}

// a dense layer over NHWC rows as a 1x1 conv (mode 2: the form both the fp32 and the split-f16 launch paths serve for any M % 128 == 0)
GemmF32Args plain_conv1x1(const float* A, const float* bias, const float* X, float* C, int M, int K, long N) {
    GemmF32Args g{};
    g.A = A; g.X = X; g.C = C; g.shift = bias; g.M = M; g.K = K; g.taps = 1; g.ldc = M; g.N = N; g.mode = 2; g.H = 1; g.W = 1; g.Cin = K; g.ldx = K; g.stride = 1;
    return g;
}

const float* gn_fail(int HW, int C) { fail(DMAD_ERR_STATE, "GroupNorm: no kernel for a %d-pixel x %d-channel map", HW, C); return nullptr; }

// applies one module; `in` [B][H*H][cin] -> returns the buffer holding [B][Ho*Ho][cout].  `dst`: where the result must
// land (a saved-skip buffer) or nullptr (take a rotating work buffer).
// `in2` != nullptr (ResBlocks of the output path only): the module's input is th.cat([in, in2], dim=1) (unet.py:473), `in` holding
// c1 channels and `in2` the rest — GroupNorm and the 1x1 skip conv read the two parts in place, nothing is concatenated.
// x3: the MIDDLE tier — the same fp32 pipeline (fp32 maps, GroupNorm, softmax, residual sums) with every conv / 1x1 on split-f16 operands
// (three f16 MFMAs per product, ~22 significant bits, gemm_x3_kernel): GroupNorm writes its output in the split format, the maps a GEMM
// reads without a GroupNorm in between (the block input of a 1x1 skip conv, of a Downsample / Upsample conv, the attention output) are
// converted by one elementwise pass.
// t2dst / qkvdst (the VJP's tape, fp32 tier): where a ResBlock's conv1 output / an AttentionBlock's qkv land instead of the work buffers.
const float* unet_apply(dmad_engine* e, const dmad_engine::UnOp& o, const float* in, int B, int& H, float* dst, int& rot, hipStream_t s,
                        const float* in2 = nullptr, int c1 = 0, bool x3 = false, float* t2dst = nullptr, float* qkvdst = nullptr) {
    float *T1 = e->un_buf[3], *T2 = t2dst ? t2dst : e->un_buf[4], *SK = e->un_buf[5], *QKV = qkvdst ? qkvdst : e->un_buf[6], *ATT = e->un_buf[7];
    auto next = [&]() { float* p = e->un_buf[rot]; rot = (rot + 1) % 3; if (p == in) { p = e->un_buf[rot]; rot = (rot + 1) % 3; } return p; };
    float* out = dst ? dst : next();
    const long nref = (long)e->maxB * H * H;
    auto gemm = [&](GemmF32Args g, const float* wx, long nr) {             // one conv / 1x1 on this pass's tier
        if (x3) { g.A = wx; g.x3 = 1; launch_gemm_f32(g, s); }
        else launch_gemm_f32(g, s, e->slab, e->slab_floats, nr);
    };
    if (o.kind == 1) {                      // ResBlock._forward, unet.py:186-199
        if (in2 && o.cin == o.cout) { fail(DMAD_ERR_STATE, "a concatenated input needs the ResBlock's skip conv"); return nullptr; }
        if (launch_groupnorm_nhwc(in, o.gn1w, o.gn1b, nullptr, 1, T1, B, H * H, o.cin, s, in2, c1, nullptr, nullptr, nullptr, x3)) return gn_fail(H * H, o.cin);
        gemm(nhwc_conv_args(o.w1, nullptr, o.b1, T1, T2, o.cout, o.cin, 9, B, H, 1, nullptr), o.w1x, nref);
        if (launch_groupnorm_nhwc(T2, o.gn2w, o.gn2b, e->un_ss_cur + o.ss_off, 1, T1, B, H * H, o.cout, s, nullptr, 0, nullptr, nullptr, nullptr, x3)) return gn_fail(H * H, o.cout);
        const float* skip = in;
        if (o.cin != o.cout) {
            const float *sin = in, *sin2 = in2;
            if (x3) {                       // the block input(s) as split-format operands (QKV / ATT are free inside a ResBlock)
                const int ca = in2 ? c1 : o.cin;
                launch_scale(in, 1.f, QKV, (long)B * H * H * ca, s, true);
                sin = QKV;
                if (in2) { launch_scale(in2, 1.f, ATT, (long)B * H * H * (o.cin - c1), s, true); sin2 = ATT; }
            }
            GemmF32Args g = nhwc_conv_args(o.skw, nullptr, o.skb, sin, SK, o.cout, o.cin, 1, B, H, 1, nullptr);
            if (in2) { g.ldx = c1; g.X2 = sin2; g.ksplit = c1; g.ldx2 = o.cin - c1; }
            gemm(g, o.skwx, nref);
            skip = SK;
        }
        gemm(nhwc_conv_args(o.w2, nullptr, o.b2, T1, out, o.cout, o.cout, 9, B, H, 1, skip), o.w2x, nref);
    } else if (o.kind == 2) {               // AttentionBlock._forward + QKVAttention, unet.py:225-258
        const int C = o.cin, T = H * H;
        if (launch_groupnorm_nhwc(in, o.gn1w, o.gn1b, nullptr, 0, T1, B, T, C, s, nullptr, 0, nullptr, nullptr, nullptr, x3)) return gn_fail(T, C);
        gemm(x3 ? plain_conv1x1(o.w1, o.b1, T1, QKV, 3 * C, C, (long)B * T) : plain_gemm(o.w1, T1, QKV, nullptr, o.b1, 3 * C, C, (long)B * T, 3 * C, C, 0), o.w1x, nref);
        if (int rc = launch_qkv_attention(QKV, ATT, B, T, kUnHeads, s, nullptr, x3 ? 1 : 0)) { fail(rc > 0 ? DMAD_ERR_HIP : DMAD_ERR_STATE, "UNet attention (T = %d): %s", T, rc > 0 ? hipGetErrorString((hipError_t)rc) : "unsupported map size"); return nullptr; }      // (x3: the output straight in the split format)
        GemmF32Args g = x3 ? plain_conv1x1(o.w2, o.b2, ATT, out, C, C, (long)B * T) : plain_gemm(o.w2, ATT, out, nullptr, o.b2, C, C, (long)B * T, C, C, 0);
        g.res = in;
        gemm(g, o.w2x, nref);
    } else if (o.kind == 3) {               // Downsample: conv 3x3 stride 2, unet.py:82-111
        const float* xin = in;
        if (x3) { launch_scale(in, 1.f, T1, (long)B * H * H * o.cin, s, true); xin = T1; }
        gemm(nhwc_conv_args(o.w1, nullptr, o.b1, xin, out, o.cout, o.cin, 9, B, H, 2, nullptr), o.w1x, nref / 4);
        H /= 2;
    } else if (o.kind == 4) {               // Upsample: nearest x2 + conv 3x3, unet.py:49-79
        launch_upsample2x_nhwc(in, T1, B, H, H, o.cin, s);
        H *= 2;
        if (x3) launch_scale(T1, 1.f, T1, (long)B * H * H * o.cin, s, true);
        gemm(nhwc_conv_args(o.w1, nullptr, o.b1, T1, out, o.cout, o.cin, 9, B, H, 1, nullptr), o.w1x, nref * 4);
    } else {
        if (launch_conv1ch_3x3(in, o.w1, o.b1, out, B, o.cout, s)) { fail(DMAD_ERR_STATE, "input conv: %d output channels > 128", o.cout); return nullptr; }
    }
    return out;
}

// ---- the same network on the 16-bit tier: every conv / 1x1 through gemm_h16 (f16 operands, fp32 accumulate); GroupNorm statistics,
// softmax and the bias / residual sums in fp32; the hidden state itself exists as f16 maps ONLY (a block output costs 2 bytes per
// value to write and 2 to read back as the next residual, against 4 + 2 and 4 with an fp32 copy beside it).  UMap::f of a block
// output is only the identity of its buffer slot on this tier (never written or read); the network input has f alone.
struct UMap { const float* f; const h16_t* h; const float* st; };      // st: the map's GroupNorm statistics slab (nullptr: none, e.g. maps of fewer than 64 pixels)

GemmH16Args un_h16_args(const h16_t* A, const float* bias, const h16_t* X, float* C, h16_t* C16, int cout, int cin, int taps, int B, int H,
                        int stride, const h16_t* res16, float* stats = nullptr) {
    GemmH16Args g{};
    const int Ho = (H - 1) / (stride > 1 ? stride : 1) + 1;
    g.A = A; g.X = X; g.C = C; g.C16 = C16; g.shift = bias; g.res16 = res16; g.M = cout; g.K = cin; g.taps = taps; g.ldc = cout;
    g.N = (long)B * Ho * Ho; g.H = H; g.W = H; g.ldx = cin; g.stride = stride;
    g.stats = Ho * Ho >= 16 ? stats : nullptr;          // a statistics block must lie inside one sample: 64 pixels, or 16 on the 4 x 4 maps
    g.stats_px = Ho * Ho >= 64 ? 64 : 16;
    return g;
}

// GroupNorm of the 16-bit tier: the one-pass kernel when every part of the input carries its statistics slab, the two-pass ones otherwise
int un_groupnorm16(UMap in, UMap in2, int c1, const float* gw, const float* gb, const float* ss, int silu, h16_t* y16, float* y32, int B, int HW,
                   int C, hipStream_t s) {
    static const bool fused = env_switch_on("DMAD_GN_FUSED");     // A/B switch
    if (fused && in.h && in.st && (!in2.h || in2.st) && HW >= 16 &&
        launch_groupnorm16_apply(in.h, in.st, in2.h, in2.st, c1, gw, gb, ss, silu, y16, y32, B, HW, C, s) == 0)
        return 0;
    return launch_groupnorm_nhwc(in.f, gw, gb, ss, silu, y32, B, HW, C, s, in2.f, c1, y16, in.h, in2.h);
}

bool unet_apply_h16(dmad_engine* e, const dmad_engine::UnOp& o, UMap in, int B, int& H, float* dstf, h16_t* dsth, float* dstst, int& rot, hipStream_t s,
                    UMap* result, UMap in2 = UMap{nullptr, nullptr, nullptr}, int c1 = 0) {
    h16_t* SK16 = (h16_t*)e->un_buf[5];        // the skip conv's output, f16 (the fp32 tier's buffer, reused)
    h16_t *T1h = e->un_t1h, *T2h = e->un_t2h, *ATTh = e->un_atth;
    float* outf = dstf;
    h16_t* outh = dsth;
    float* outst = dstst;
    if (!outf) {
        int r = rot; rot = (rot + 1) % 3;
        if (e->un_buf[r] == in.f) { r = rot; rot = (rot + 1) % 3; }
        outf = e->un_buf[r]; outh = e->un_buf16[r]; outst = e->un_st_buf[r];
    }
    int Hout = H;
    const UMap none{nullptr, nullptr, nullptr};
    if (o.kind == 1) {                      // ResBlock._forward, unet.py:186-199
        if (in2.f && o.cin == o.cout) { fail(DMAD_ERR_STATE, "a concatenated input needs the ResBlock's skip conv"); return false; }
        // GroupNorm reads the f16 maps (statistics from the producing GEMM's epilogue where there is one); the in_layers conv writes f16 only
        if (un_groupnorm16(in, in2, c1, o.gn1w, o.gn1b, nullptr, 1, T1h, nullptr, B, H * H, o.cin, s)) { gn_fail(H * H, o.cin); return false; }
        launch_gemm_h16(un_h16_args(o.w1h, o.b1, T1h, nullptr, T2h, o.cout, o.cin, 9, B, H, 1, nullptr, e->un_st_t2), s);
        const UMap t2{nullptr, T2h, H * H >= 16 ? e->un_st_t2 : nullptr};
        if (un_groupnorm16(t2, none, 0, o.gn2w, o.gn2b, e->un_ss_cur + o.ss_off, 1, T1h, nullptr, B, H * H, o.cout, s)) { gn_fail(H * H, o.cout); return false; }
        const h16_t* skip = in.h;
        if (o.cin != o.cout) {
            GemmH16Args g = un_h16_args(o.skwh, o.skb, in.h, nullptr, SK16, o.cout, o.cin, 1, B, H, 1, nullptr);
            if (in2.f) { g.ldx = c1; g.X2 = in2.h; g.ksplit = c1; g.ldx2 = o.cin - c1; }
            launch_gemm_h16(g, s);
            skip = SK16;
        }
        launch_gemm_h16(un_h16_args(o.w2h, o.b2, T1h, nullptr, outh, o.cout, o.cout, 9, B, H, 1, skip, outst), s);
    } else if (o.kind == 2) {               // AttentionBlock._forward + QKVAttention, unet.py:225-258
        const int C = o.cin, T = H * H;
        if (un_groupnorm16(in, none, 0, o.gn1w, o.gn1b, nullptr, 0, T1h, nullptr, B, T, C, s)) { gn_fail(T, C); return false; }
        if ((long)T * C > 256l * 256) { fail(DMAD_ERR_STATE, "UNet attention: %d tokens x %d channels exceed the f16 qkv buffer", T, C); return false; }
        launch_gemm_h16(un_h16_args(o.w1h, o.b1, T1h, nullptr, e->un_qkvh, 3 * C, C, 1, B, H, 1, nullptr), s);      // qkv straight to f16
        if (int rc = launch_qkv_attention_h16(e->un_qkvh, ATTh, B, T, kUnHeads, s)) { fail(rc > 0 ? DMAD_ERR_HIP : DMAD_ERR_STATE, "UNet attention (T = %d): %s", T, rc > 0 ? hipGetErrorString((hipError_t)rc) : "unsupported map size"); return false; }
        launch_gemm_h16(un_h16_args(o.w2h, o.b2, ATTh, nullptr, outh, C, C, 1, B, H, 1, in.h, outst), s);
    } else if (o.kind == 3) {               // Downsample: conv 3x3 stride 2, unet.py:82-111
        launch_gemm_h16(un_h16_args(o.w1h, o.b1, in.h, nullptr, outh, o.cout, o.cin, 9, B, H, 2, nullptr, outst), s);
        H /= 2;
        Hout = H;
    } else if (o.kind == 4) {               // Upsample: nearest x2 + conv 3x3, unet.py:49-79
        H *= 2;
        Hout = H;
        GemmH16Args g = un_h16_args(o.w1h, o.b1, in.h, nullptr, outh, o.cout, o.cin, 9, B, H, 1, nullptr, outst);
        g.up2 = 1;                              // the conv reads the half-resolution map through the upsampling where the kernel can
        if (!gemm_h16_fuses_up2(g)) {
            launch_upsample2x_nhwc_h16(in.h, e->un_uph, B, H / 2, H / 2, o.cin, s);
            g.up2 = 0;
            g.X = e->un_uph;
        }
        launch_gemm_h16(g, s);
    } else {                                // input conv 1 -> 128 (direct kernel, fp32 arithmetic): the f16 map and its statistics only
        if (launch_conv1ch_3x3(in.f, o.w1, o.b1, nullptr, B, o.cout, s, outh, (o.cout & 3) ? nullptr : outst)) { fail(DMAD_ERR_STATE, "input conv: %d output channels > 128", o.cout); return false; }
        if (o.cout & 3) outst = nullptr;
    }
    *result = UMap{outf, outh, Hout * Hout >= 16 ? outst : nullptr};
    return true;
}

// eps = UNetModel.forward(x, t * ones)  (unet.py:453-477): x, eps [B][32][32]
// h16 = 2: the split-f16 middle tier (fp32 pipeline, every conv on split-f16 operands: fp32-grade at several times the fp32 matrix rate).
// h16 < 0: the tier of the map-returning entry points (dmad_unet_eps / dmad_unet_p_sample / dmad_spec_query_logits): the 16-bit tier in
// DMAD_MODE_FAST (and in DMAD_MODE_EXACT_VOTES when dmad_set_waveform_tier chose the 16-bit tier), in DMAD_MODE_EXACT_VOTES otherwise the
// tier dmad_set_waveform_tier selects — the split-f16 tier by default (fp32-grade, 2.2 x the fp32 rate), the exact-fp32 UNet on request
// and in DMAD_MODE_FP32 — only the spec-domain vote loop has a recheck, so it alone runs the 16-bit tier by default (it passes h16 = 1);
// 0 / 1 / 2: explicit
// tape (exact-fp32 tier only, B <= unvjpB): every module writes its output (and a ResBlock its conv1 output, an AttentionBlock its qkv) to
// its tape slot instead of the work buffers — the same launches, the same bits (dmad_unet_eps_vjp's forward)
int unet_eps(dmad_engine* e, const float* x, int t, int B, float* eps, hipStream_t s, int h16 = -1, const dmad_engine::UnTape* tape = nullptr) {
    CHK(need_unet(e)); CHK(need_batch(e, B));
    if (t < 0) return fail(DMAD_ERR_INVALID, "diffusion step %d < 0", t);
    CHK(unet_prepare_step(e, t, s));
    if (h16 < 0) {      // the map-returning surfaces follow dmad_set_waveform_tier like the waveform-returning ones: split-f16 by default on exact-vote engines
        if (e->un_h16 && (e->mode == DMAD_MODE_FAST || (e->mode == DMAD_MODE_EXACT_VOTES && e->wave_tier == PATH_DEFAULT))) h16 = 1;
        else if (e->un_x3 && e->mode == DMAD_MODE_EXACT_VOTES && e->wave_tier == PATH_X3) h16 = 2;
        else h16 = 0;
    }
    if (h16 == 1 && !e->un_h16) return fail(DMAD_ERR_STATE, "this engine has no 16-bit UNet tier (DMAD_FP32 precision)");
    if (h16 == 1) {
        int H = 32, rot = 0;
        UMap h{x, nullptr, nullptr};
        std::vector<const float*> hs_st(e->un_hs.size(), nullptr);      // the statistics slab each saved map ended up with (16-pixel blocks on the 4x4 maps)
        for (const auto& r : e->un_ops) {
            const int i = r.save, top = r.top;                  // th.cat([h, hs.pop()], dim=1): h carries c1 channels, the saved map the rest
            const UMap hs = top >= 0 ? UMap{e->un_hs[top], e->un_hs16[top], hs_st[top]} : UMap{nullptr, nullptr, nullptr};
            if (!unet_apply_h16(e, r, h, B, H, i >= 0 ? e->un_hs[i] : nullptr, i >= 0 ? e->un_hs16[i] : nullptr, i >= 0 ? e->un_st_hs[i] : nullptr, rot, s, &h, hs,
                                top >= 0 ? r.cin - e->un_hs_ch[top] : 0))
                return DMAD_ERR_STATE;
            if (i >= 0) hs_st[i] = h.st;
        }
        if (un_groupnorm16(h, UMap{nullptr, nullptr, nullptr}, 0, e->un_outgw, e->un_outgb, nullptr, 1, e->un_t1h, nullptr, B, 1024, kUnMC, s)) { gn_fail(1024, kUnMC); return DMAD_ERR_STATE; }
        launch_conv3x3_c128_to1_h16(e->un_t1h, e->un_outw, e->un_outb, eps, B, s);       // (operands f16, fp32 accumulate, like the tier's GEMMs)
        LASTCHK();
        return 0;
    }
    const bool x3 = h16 == 2;
    if (x3 && !e->un_x3) return fail(DMAD_ERR_STATE, "this engine has no split-f16 UNet tier (it needs DMAD_EXACT precision)");
    if (tape && h16 != 0) return fail(DMAD_ERR_STATE, "the UNet tape belongs to the exact-fp32 tier");
    int H = 32, rot = 0;
    const std::vector<float*>& hsp = tape ? tape->hs : e->un_hs;   // where the saved maps land: un_hs, or their tape slots
    const float* h = x;
    for (size_t k = 0; k < e->un_ops.size(); ++k) {             // k: the tape's slot
        const auto& r = e->un_ops[k];
        const int top = r.top;                                  // th.cat([h, hs.pop()], dim=1): h carries c1 channels, the saved map the rest
        h = unet_apply(e, r, h, B, H, tape ? tape->out[k] : r.save >= 0 ? e->un_hs[r.save] : nullptr, rot, s, top >= 0 ? hsp[top] : nullptr,
                       top >= 0 ? r.cin - e->un_hs_ch[top] : 0, x3, tape ? tape->t2[k] : nullptr, tape ? tape->qkv[k] : nullptr);
        if (!h) return DMAD_ERR_STATE;
    }
    if (launch_groupnorm_nhwc(h, e->un_outgw, e->un_outgb, nullptr, 1, e->un_buf[3], B, 1024, kUnMC, s)) { gn_fail(1024, kUnMC); return DMAD_ERR_STATE; }
    static_assert(kUnMC == 128, "launch_conv3x3_c128_to1 is the 128-channel output layer");
    launch_conv3x3_c128_to1(e->un_buf[3], e->un_outw, e->un_outb, eps, B, s);       // (the 128 -> 1 output conv: exact fp32 on every tier but the 16-bit one)
    LASTCHK();
    return 0;
}

// ---- the UNet's vector-Jacobian product (dmad_unet_eps_vjp) ----------------------------------------------------------------
// The weight image of a dense conv's data gradient, packed on the device: w [taps][co][ci] -> wT [taps - 1 - tap][ci][co] (the 3x3 taps
// flipped; a 1x1 layer: the transpose)
void un_pack_wT(const float* w, float* wT, int taps, long ci, long co, hipStream_t s) {
    launch_unvjp_pack(w, wT, taps, (int)ci, (int)co, taps > 1 ? co * ci : 0, 1, ci, taps > 1 ? 1 : 0, s);
}

// The data gradient of one dense NHWC conv of the UNet (3x3 zero padding 1 / 1x1; H: the conv's input resolution) on its packed image
// (un_pack_wT): g [B][Ho][Ho][co] -> gx [B][H][H][ci].  stride 2 (Downsample): the stride-1 conv of the zero-dilated gradient (work:
// [B][H][H][co]).  up (Upsample = interpolate x2 + conv at 2H; g at 2H): the conv's gradient at 2H (work: [B][2H][2H][ci]), then the 2x2
// sums.  acc (optional, [B][H][H][ci]) joins the result in the GEMM's epilogue, with `up` in the 2x2 sum's.
int un_conv_dgrad(const float* wT, const float* g, float* gx, int ci, int co, int taps, int B, int H, int stride, bool up, const float* acc,
                  float* work, hipStream_t s) {
    const float* gin = g;
    if (!up && stride == 2) { launch_dilate2x_nhwc(g, work, B, H / 2, co, s); gin = work; }
    if (launch_gemm_f32(nhwc_conv_args(wT, nullptr, nullptr, gin, up ? work : gx, ci, co, taps, B, up ? 2 * H : H, 1, up ? nullptr : acc), s) != 0)
        return fail(DMAD_ERR_STATE, "UNet VJP: no GEMM for M = %d, K = %d, taps = %d", ci, co, taps);
    if (up) launch_upsample2x_bwd_nhwc(work, acc, gx, B, H, ci, s);
    return 0;
}

// One pass (B <= unvjpB): the forward with its tape, then the modules in reverse.  G[0] / G[1] carry the gradient of the current module's
// output / input (ping-pong); G[2..5] are the per-module scratch maps (G[2] conv2^T / proj^T / the dilated map / the upsampled gradient,
// G[3] GroupNorm2^T / the attention gradient, G[4] conv1^T / qkv^T, G[5] the skip conv^T).
// affine (the reverse VP-SDE chain): g_x = alpha * g_eps - gamma * (d eps / d x)^T g_eps, in the input conv backward's epilogue
int unet_vjp_pass(dmad_engine* e, const float* x, int t, int B, const float* g_eps, float* g_x, float* eps, hipStream_t s,
                  bool affine = false, float alpha = 1.f, float gamma = 0.f) {
    CHK(unet_eps(e, x, t, B, eps, s, 0, &e->un_tape));
    const std::vector<dmad_engine::UnOp>& ops = e->un_ops;
    const size_t W = (size_t)e->unvjpB * 1024 * 384;
    float* G[6];
    for (int i = 0; i < 6; ++i) G[i] = e->unvjp_work + i * W;
    const auto& tp = e->un_tape;
    auto gnb = [&](const float* xin, const float* xin2, int c1, const float* gw, const float* gb, const float* ss, int silu, const float* gy,
                   const float* add, const float* add2, float* gx, float* gx2, int HW, int C) -> int {
        if (launch_groupnorm_bwd(xin, xin2, c1, gw, gb, ss, silu, gy, add, add2, gx, gx2, B, HW, C, s)) return fail(DMAD_ERR_STATE, "UNet VJP: GroupNorm backward of a %d-channel map", C);
        return 0;
    };
    // out.2 (128 -> 1) backward: a 1 -> 128 conv of g_eps with the flipped image; out.0 + SiLU backward into G[0]
    if (launch_conv1ch_3x3(g_eps, e->un_outT, e->unvjp_zero, G[2], B, kUnMC, s)) return fail(DMAD_ERR_STATE, "UNet VJP: output conv backward");
    CHK(gnb(tp.out.back(), nullptr, 0, e->un_outgw, e->un_outgb, nullptr, 1, G[2], nullptr, nullptr, G[0], nullptr, 1024, kUnMC));
    float *cur = G[0], *nxt = G[1];
    for (int k = (int)ops.size() - 1; k >= 0; --k) {
        const auto& o = ops[k];
        const int H = ops[k].H, top = ops[k].top;
        const float* in = k ? tp.out[k - 1] : x;
        const float* in2 = top >= 0 ? tp.hs[top] : nullptr;
        const int c1 = top >= 0 ? o.cin - e->un_hs_ch[top] : 0;
        float* gin2 = top >= 0 ? e->unvjp_ghs_at[top] : nullptr;
        const float* acc = ops[k].acc >= 0 ? e->unvjp_ghs_at[ops[k].acc] : nullptr;
        if (o.kind == 1) {                      // ResBlock: skip(in) + conv2(SiLU(GN2(conv1(SiLU(GN1(in)))) * (1 + scale) + shift))
            CHK(un_conv_dgrad(o.w2T, cur, G[2], o.cout, o.cout, 9, B, H, 1, false, nullptr, nullptr, s));
            CHK(gnb(tp.t2[k], nullptr, 0, o.gn2w, o.gn2b, e->un_ss_cur + o.ss_off, 1, G[2], nullptr, nullptr, G[3], nullptr, H * H, o.cout));
            CHK(un_conv_dgrad(o.w1T, G[3], G[4], o.cin, o.cout, 9, B, H, 1, false, nullptr, nullptr, s));
            const float *add = cur, *add2 = acc;
            if (o.cin != o.cout) {              // the 1x1 skip conv's gradient, the consumer's saved-map gradient summed in its epilogue
                CHK(un_conv_dgrad(o.skwT, cur, G[5], o.cin, o.cout, 1, B, H, 1, false, acc, nullptr, s));
                add = G[5]; add2 = nullptr;
            }
            CHK(gnb(in, in2, c1, o.gn1w, o.gn1b, nullptr, 1, G[4], add, add2, nxt, gin2, H * H, o.cin));
        } else if (o.kind == 2) {               // AttentionBlock: in + proj_out(attention(qkv(GN(in))))
            const int T = H * H, C = o.cin;
            CHK(un_conv_dgrad(o.w2T, cur, G[2], C, C, 1, B, H, 1, false, nullptr, nullptr, s));
            if (int rc = launch_qkv_attention_bwd(tp.qkv[k], G[2], G[3], B, T, kUnHeads, s)) return fail(rc > 0 ? DMAD_ERR_HIP : DMAD_ERR_STATE, "UNet VJP: attention backward (T = %d)", T);
            CHK(un_conv_dgrad(o.w1T, G[3], G[4], C, 3 * C, 1, B, H, 1, false, nullptr, nullptr, s));
            CHK(gnb(in, nullptr, 0, o.gn1w, o.gn1b, nullptr, 0, G[4], cur, acc, nxt, nullptr, T, C));
        } else if (o.kind == 3) {               // Downsample (3x3, stride 2): the stride-1 conv of the zero-dilated gradient
            CHK(un_conv_dgrad(o.w1T, cur, nxt, o.cin, o.cout, 9, B, H, 2, false, acc, G[2], s));
        } else if (o.kind == 4) {               // Upsample: the conv's gradient at 2H, then the 2x2 sums
            CHK(un_conv_dgrad(o.w1T, cur, nxt, o.cin, o.cout, 9, B, H, 1, true, acc, G[2], s));
        } else {                                // conv_in (1 -> 128): a 128 -> 1 conv of the gradient with the flipped image
            launch_conv3x3_c128_to1(cur, o.w1T, e->unvjp_zero, g_x, B, s, affine ? g_eps : nullptr, alpha, gamma);
        }
        std::swap(cur, nxt);
    }
    LASTCHK();
    return 0;
}

int unet_vjp(dmad_engine* e, const float* x, int t, int B, const float* g_eps, float* g_x, float* eps, hipStream_t s) {
    CHK(need_unet(e));
    if (!e->f32) return fail(DMAD_ERR_STATE, "the UNet VJP runs on the exact-fp32 UNet tier: it needs a DMAD_FP32 or DMAD_EXACT engine");
    if (!e->unvjpB) return fail(DMAD_ERR_STATE, "no UNet VJP workspace: call dmad_reserve_unet_vjp first");
    CHK(need_batch(e, B));
    if (t < 0) return fail(DMAD_ERR_INVALID, "diffusion step %d < 0", t);
    return for_passes(B, e->unvjpB, [&](int64_t b0, int bb) {
        return unet_vjp_pass(e, x + b0 * 1024, t, bb, g_eps + b0 * 1024, g_x + b0 * 1024, eps ? eps + b0 * 1024 : e->un_eps, s);
    });
}

int ensure_embed(dmad_engine* e, int t, hipStream_t s) {
    if (e->emb_t == t) return 0;
    launch_embed_table((float)t, e->fc1w, e->fc1b, e->fc2w, e->fc2b, e->fctw, e->fctb, e->emb_table, e->emb2, e->bf16 ? e->b2 : nullptr,
                       e->bf16 ? e->epi_c : nullptr, e->NL, s);
    e->emb_t = t;
    return 0;
}

// The padding invariant of the zero-padded fp32 maps ([clips][LP][ld], a clip in rows [kPad, kPad + len)): a dilated tap reads up to
// kPad rows past either end of a clip and must find zeros there.  Rows outside [kPad, kPad + clip_len) are never written; rows
// [kPad + len, kPad + *dirty) hold what the longest call since the map was last clean left there, so a shorter call zeroes that band
// first, in every clip of the map, on its own stream.  A run of calls at one length (every fixed-length export) clears nothing.
void clean_pad(float* map, int* dirty, int len, size_t clips, size_t LP, size_t ld, hipStream_t s) {
    if (len < *dirty) launch_zero_band(map, (long)(LP * ld), (long)((kPad + len) * ld), (long)((*dirty - len) * ld), (long)clips, s);
    *dirty = len;
}

// exact32: evaluate on the exact-fp32 path (the only one of a DMAD_FP32 engine; DMAD_MODE_FP32 and the recheck pass of a
// DMAD_EXACT engine); batches larger than the fp32 workspace are walked in chunks of maxB32 clips
// save != nullptr (the VJP's forward pass; B <= maxB32, fp32 path): layer n reads its residual stream from slot n of `save`
// ([NL][vjpB][LP][256]) and writes the next one to slot n + 1 instead of the A / B ping-pong — the same launches, the same bits
// len != 0 (the any-length exports, fp32 path only): clips of len <= clip_len samples, rows [kPad, kPad + len) of the same maps
int wavenet_eps(dmad_engine* e, const float* x_t, int t, int B, float* eps, hipStream_t s, int path = PATH_DEFAULT, float* save = nullptr,
                int len = 0) {
    CHK(need_wavenet(e)); CHK(need_batch(e, B));
    if (t < 0) return fail(DMAD_ERR_INVALID, "diffusion step %d < 0", t);
    CHK(ensure_embed(e, t, s));
    const int L = len ? len : e->L, LP = e->LP, NL = e->NL;
    const bool use32 = !e->bf16 || (e->f32 && (path != PATH_DEFAULT || e->mode == DMAD_MODE_FP32));
    const bool x3 = use32 && path == PATH_X3 && e->wdil_x3;     // fp32 pipeline on split-f16 operands (three MFMAs per product)
    if (use32 && B > e->maxB32)
        return for_passes(B, e->maxB32, [&](int64_t b0, int bb) { return wavenet_eps(e, x_t + b0 * L, t, bb, eps + b0 * L, s, x3 ? PATH_X3 : PATH_FP32, nullptr, len); });
    if (!use32) {
        launch_wn_init_bf16(x_t, e->init_w, e->init_b, e->emb_table, e->hA, B, L, LP, e->f16, s);
        for (int n = 0; n < NL; ++n) {
            WnLayerArgs a{};
            a.hin = (n & 1) ? e->hB : e->hA;
            a.hout = (n & 1) ? e->hA : e->hB;
            a.gout = e->gstore + (size_t)n * B * L * kC;
            a.w1p = e->w1p + (size_t)n * 24 * 512 * 32;
            a.w2p = e->w2p + (size_t)n * 8 * 256 * 32;
            a.b1 = e->b1p + (size_t)n * 512;
            a.epi_c = e->epi_c + (size_t)n * 256;
            a.dilation = 1 << (n % e->cfg.dilation_cycle);
            a.L = L; a.LP = LP; a.last = (n == NL - 1); a.npos = (long)B * L;
            const bool timed = e->prof_on && !a.last && e->prof_used + 2 <= e->prof_ev.size();
            if (timed) (void)hipEventRecord(e->prof_ev[e->prof_used++], s);
            launch_wn_layer_bf16_p(a, B, e->f16, s);
            if (timed) (void)hipEventRecord(e->prof_ev[e->prof_used++], s);
        }
        WnFinalArgs f{};
        f.g = e->gstore; f.wsp = e->wsp; f.wf0p = e->wf0p; f.bskip_sum = e->bskip_sum; f.bf0 = e->bf0; f.wz = e->wz;
        f.eps = eps; f.bz = e->bz; f.skip_scale = (float)sqrt(1.0 / NL); f.NL = NL; f.B = B; f.L = L;
        const bool timed_f = e->prof_on && e->prof_used_f + 2 <= e->prof_ev_f.size();
        if (timed_f) (void)hipEventRecord(e->prof_ev_f[e->prof_used_f++], s);
        launch_wn_final_bf16_p(f, e->f16, s);
        if (timed_f) (void)hipEventRecord(e->prof_ev_f[e->prof_used_f++], s);
    } else {
        const long N = (long)B * L;
        const size_t sslot = (size_t)e->vjpB * LP * kC;           // one saved stream (VJP)
        if (save) clean_pad(save, &e->dirty_save, L, (size_t)NL * e->vjpB, LP, kC, s);
        else { clean_pad(e->hA32, &e->dirty_hA32, L, e->maxB32, LP, kC, s); clean_pad(e->hB32, &e->dirty_hB32, L, e->maxB32, LP, kC, s); }
        launch_wn_init_f32(x_t, e->init_w, e->init_b, e->emb_table, save ? save : e->hA32, B, L, LP, s, x3, x3 && e->diag[4]);
        const size_t slab = (size_t)e->maxB32 * e->L * 256;       // one gate-output slab per layer
        for (int n = 0; n < NL; ++n) {
            float* hin = save ? save + n * sslot : (n & 1) ? e->hB32 : e->hA32;
            float* hout = save ? save + (n + 1) * sslot : (n & 1) ? e->hA32 : e->hB32;
            const int d = 1 << (n % e->cfg.dilation_cycle);
            const bool last = n == NL - 1;
            float* gout = e->gstore32 + (size_t)n * slab;
            GemmF32Args g = wn_conv_args((x3 ? e->wdil_x3 : e->wdil) + (size_t)n * 3 * 512 * 256, hin + (size_t)kPad * kC, gout, e->bdil + (size_t)n * 512,
                                         512, 256, 3, N, L, (long)LP * kC, kC, (long)d * kC);
            g.x3 = x3; g.diag = x3 ? e->diag[0] : 0;
            g.epi = 1;                           // tanh * sigmoid in the epilogue: H never goes to HBM
            launch_gemm_f32(g, s);
            if (last) continue;                  // the last layer's residual output is never consumed (WaveNet.py:131-135)
            // res conv with the residual update in its epilogue; the skip convs run as one GEMM after the loop
            GemmF32Args u = plain_gemm((x3 ? e->wrs_x3 : e->wrs) + (size_t)n * 512 * 256, gout, nullptr, nullptr, e->brs + (size_t)n * 512, 256, 256,
                                       N, 256, 256, 0);
            u.epi = 2; u.res_rows = 256; u.first = 0; u.L = L; u.LP = LP;
            u.hin = hin; u.hout = hout; u.skip = nullptr; u.emb_next = e->emb_table + (size_t)(n + 1) * 256;
            u.x3 = x3; u.diag = x3 ? e->diag[1] : 0;
            launch_gemm_f32(u, s);
        }
        {   // skip = sum_n W_skip_n g_n + sum_n b_skip_n: taps = layers, tap stride = one slab (taps are centred on NL / 2)
            GemmF32Args k = wn_conv_args(x3 ? e->wskip_x3 : e->wskip32, e->gstore32 + (size_t)(NL >> 1) * slab, e->skip32, e->bskip32, 256, 256, NL, N, N, 0,
                                         256, (long)slab);
            k.x3 = x3; k.diag = x3 ? e->diag[2] : 0;
            launch_gemm_f32(k, s);
        }
        launch_scale(e->skip32, (float)sqrt(1.0 / NL), e->g32, N * 256, s, x3);
        GemmF32Args f = plain_gemm(x3 ? e->wf0_x3 : e->wf0, e->g32, e->H32, nullptr, e->bf0, 256, 256, N, 256, 256, 1);
        f.x3 = x3; f.diag = x3 ? e->diag[3] : 0;
        launch_gemm_f32(f, s);
        launch_dot256(e->H32, e->wz, e->bz, eps, N, s);
    }
    LASTCHK();
    return 0;
}

// One pass of dmad_wavenet_eps_vjp (B <= vjpB): forward-save, then the backward layer by layer.
//   G = three zero-padded [vjpB][LP][256] maps: region 0 g_s (the gradient of the skip sum, every layer's g_skip), regions 1 / 2 the
//   gradient of the residual stream ping-pong.  The gate-gradient GEMM contracts K = 512 over two taps — tap 0 = region 0 through
//   W_skip^T, tap 1 = region r through sqrt(1/2) W_res^T — by reading region r with a tap stride of r regions.
// affine (the reverse VP-SDE chain): g_x = alpha * g_eps - gamma * (d eps / d x_t)^T g_eps, in the init-conv backward's epilogue
int wavenet_vjp_pass(dmad_engine* e, const float* x_t, int t, int B, const float* g_eps, float* g_x, float* eps, hipStream_t s,
                     bool affine = false, float alpha = 1.f, float gamma = 0.f, int len = 0) {
    const int L = len ? len : e->L, LP = e->LP, NL = e->NL;
    const long N = (long)B * L;
    const size_t RS = (size_t)e->vjpB * LP * kC, sslot = RS;
    CHK(wavenet_eps(e, x_t, t, B, eps, s, PATH_FP32, e->vjp_save, len));
    clean_pad(e->vjp_G, &e->dirty_G, L, 3 * (size_t)e->vjpB, LP, kC, s);
    clean_pad(e->vjp_gH, &e->dirty_gH, L, e->vjpB, LP, 512, s);
    // final block: g_y = [y > 0] wz g_eps (y = relu(f0), kept in H32), g_s = sqrt(1/NL) W_f0^T g_y (scale folded into the image)
    launch_vjp_final(e->H32, e->wz, g_eps, e->vjp_gg, N, s);
    GemmF32Args f = plain_gemm(e->vjp_wf0T, e->vjp_gg, nullptr, nullptr, nullptr, 256, 256, N, 256, 256, 0);
    f.epi = 4; f.L = L; f.LP = LP; f.hin = nullptr; f.hout = e->vjp_G;
    CHK(launch_gemm_f32(f, s) ? fail(DMAD_ERR_INVALID, "VJP: no kernel for the f0 backward") : 0);
    for (int n = NL - 1; n >= 0; --n) {
        const int d = 1 << (n % e->cfg.dilation_cycle);
        const bool last = n == NL - 1;
        const int r_out = 1 + ((NL - 2 - n) & 1), r_in = 1 + ((NL - 1 - n) & 1);   // regions of g_h(n+1) (input) and g_h(n) (output)
        float* g_hout = e->vjp_G + (size_t)r_out * RS;
        float* g_hin = e->vjp_G + (size_t)r_in * RS;
        // g_gate = W_skip^T g_s + sqrt(1/2) W_res^T g_h(n+1)   (the last layer: the first term alone)
        const GemmF32Args gg = wn_conv_args(e->vjp_wgT + (size_t)n * 2 * 256 * 256, (last ? e->vjp_G : g_hout) + (size_t)kPad * kC, e->vjp_gg, nullptr, 256, 256,
                                            last ? 1 : 2, N, L, (long)LP * kC, kC, last ? 0 : (long)r_out * (long)RS);
        CHK(launch_gemm_f32(gg, s) ? fail(DMAD_ERR_INVALID, "VJP: no kernel for the gate gradient") : 0);
        // g_H from the recomputed H (epi 3), into the zero-padded [B][LP][512] map
        GemmF32Args g3 = wn_conv_args(e->wdil + (size_t)n * 3 * 512 * 256, e->vjp_save + n * sslot + (size_t)kPad * kC, nullptr, e->bdil + (size_t)n * 512, 512,
                                      256, 3, N, L, (long)LP * kC, kC, (long)d * kC);
        g3.epi = 3; g3.L = L; g3.LP = LP; g3.hin = e->vjp_gg; g3.hout = e->vjp_gH;
        CHK(launch_gemm_f32(g3, s) ? fail(DMAD_ERR_INVALID, "VJP: no kernel for the gate backward") : 0);
        // g_h(n) = sqrt(1/2) g_h(n+1) + transposed dilated conv of g_H (taps flipped in the image), epi 4
        GemmF32Args g4 = wn_conv_args(e->vjp_wdilT + (size_t)n * 3 * 256 * 512, e->vjp_gH + (size_t)kPad * 512, nullptr, nullptr, 256, 512, 3, N, L,
                                      (long)LP * 512, 512, (long)d * 512);
        g4.epi = 4; g4.L = L; g4.LP = LP; g4.hin = last ? nullptr : g_hout; g4.hout = g_hin;
        CHK(launch_gemm_f32(g4, s) ? fail(DMAD_ERR_INVALID, "VJP: no kernel for the transposed dilated conv") : 0);
    }
    launch_vjp_init(x_t, e->init_w, e->init_b, e->vjp_G + (size_t)(1 + ((NL - 1) & 1)) * RS, g_x, B, L, LP, s, affine ? g_eps : nullptr, alpha, gamma);
    LASTCHK();
    return 0;
}

int wavenet_vjp(dmad_engine* e, const float* x_t, int t, int B, const float* g_eps, float* g_x, float* eps, hipStream_t s, int len = 0) {
    if (!e->f32) return fail(DMAD_ERR_STATE, "the WaveNet VJP runs on the exact-fp32 path: a DMAD_BF16 engine holds no fp32 weights");
    CHK(need_wavenet(e));
    if (!e->vjpB) return fail(DMAD_ERR_STATE, "no VJP workspace: call dmad_reserve_vjp first");
    CHK(need_batch(e, B));
    if (t < 0) return fail(DMAD_ERR_INVALID, "diffusion step %d < 0", t);
    const size_t L = len ? len : e->L;
    return for_passes(B, e->vjpB, [&](int64_t b0, int bb) {
        return wavenet_vjp_pass(e, x_t + b0 * L, t, bb, g_eps + b0 * L, g_x + b0 * L, (eps ? eps : e->eps) + b0 * L, s, false, 1.f, 0.f, len);
    });
}

// the mel front-end behind its padding: the B padded rows in e->mel_xp -> spec
int mel_db_padded(dmad_engine* e, int B, float* spec, hipStream_t s, int to_db = 1) {
    const long rows = (long)B * 32;
    GemmF32Args g{};
    g.A = e->dftA; g.X = e->mel_xp; g.C = e->dftD; g.scale = nullptr; g.shift = nullptr;
    g.M = kDftM; g.K = 2048; g.taps = 1; g.ldc = kDftLd; g.relu = 0; g.N = rows; g.mode = 0;
    g.rows_per_batch = 32; g.batch_stride = e->LPm; g.row_stride = 512; g.tap_stride = 0;
    launch_gemm_f32(g, s);
    launch_mel_power(e->dftD, e->melP, kDftLd, kMelLd, rows, s);
    launch_gemm_f32(plain_gemm(e->fbA, e->melP, e->melM, nullptr, nullptr, 32, kMelLd, rows, 32, kMelLd, 0), s);
    launch_mel_db(e->melM, spec, B, to_db, s);
    LASTCHK();
    return 0;
}

int mel_db(dmad_engine* e, const float* x, int B, float* spec, hipStream_t s, int to_db = 1) {
    CHK(need_with_classifier(e)); CHK(need_batch(e, B));
    launch_mel_pad(x, e->mel_xp, B, e->L, e->LPm, s);
    return mel_db_padded(e, B, spec, s, to_db);
}

// ---------------------------------------------------------------------------------------------------------------
// Classifier-side vector-Jacobian products: the input VJPs of ResNeXt29, VGG19_bn (§18) and WideResNet-28-10 (§21) on
// their fp32 forwards — one pass function per network, one tape layout, driver and tape reader for all three (cls_vjp, cls_vjp_tape) —
// the mel front-end VJP (§14) and the masking loss on its maps (§20); the VGG19_bn forward and the classifier dispatch sit here too.
// Every VJP recomputes its forward.  ResNeXt29's and the mel VJP's GEMMs run without split-K, VGG19_bn's and WideResNet's with the split
// count of a max_batch launch, and every small kernel reduces in a fixed order: the gradients are bit-reproducible and do not depend on
// the batch.
// ---------------------------------------------------------------------------------------------------------------
// floats per spectrogram of the tape's slots, in forward order.  ResNeXt29, 28 slots: conv1's output, then per bottleneck its post-ReLU T1
// (input resolution), T2 and block output Y (output resolution)
std::vector<size_t> rx_tape_layout(const dmad_engine* e) {
    std::vector<size_t> f{(size_t)1024 * 64};
    size_t H = 32, Hi;
    for (const auto& b : e->rx) { Hi = H; H = (H - 1) / b.stride + 1; f.insert(f.end(), {Hi * Hi * b.D, H * H * b.D, H * H * b.cout}); }
    return f;
}
// VGG19_bn, 18 slots: the 16 post-ReLU conv maps, then the two post-ReLU FC vectors (311 296 floats in all)
std::vector<size_t> vgg_tape_layout() {
    std::vector<size_t> f;
    size_t H = 32;
    for (int v : kVggCfg) { if (v < 0) H >>= 1; else f.push_back(H * H * v); }
    f.insert(f.end(), {4096, 4096});
    return f;
}
// WideResNet, 25 slots: o (input resolution) and h (output resolution) of blocks 0..11, then the final post-ReLU map
std::vector<size_t> wrn_tape_layout(const dmad_engine* e) {
    std::vector<size_t> f;
    size_t H = 32;
    for (const auto& b : e->wrn) { f.push_back(H * H * b.cin); H = (H - 1) / b.stride + 1; f.push_back(H * H * b.cout); }
    f.push_back(H * H * 640);
    return f;
}
// DenseNet, 51 slots: the three streams at their pitches (the inputs every pre-activation decision is recomputed from), then the 48
// post-ReLU h maps; 322 048 + 1 032 192 floats per spectrogram
std::vector<size_t> dn_tape_layout() {
    std::vector<size_t> f;
    for (int k = 0; k < 3; ++k) f.push_back((size_t)kDnH[k] * kDnH[k] * kDnPitch[k]);
    for (int l = 0; l < 48; ++l) f.push_back((size_t)kDnH[l / 16] * kDnH[l / 16] * 48);
    return f;
}
// the engine's classifier: the slots' offsets, the tape's size (dmad_reserve_*_vjp) and the reader's bounds (dmad_*_vjp_tape) follow from this list
std::vector<size_t> cls_tape_layout(const dmad_engine* e) {
    return e->cls_kind == 1 ? rx_tape_layout(e) : e->cls_kind == 2 ? wrn_tape_layout(e) : e->cls_kind == 3 ? dn_tape_layout() : vgg_tape_layout();
}
constexpr int kDftKT = 2064;             // K of the DFT^T GEMM: the 2050 re / im rows padded to a multiple of 16

// floats per spectrogram of the six gradient work maps of rx_vjp_pass: block in / out gradients (32 x 32 x 256 at most), g_T2, its
// zero-dilation and g_T1 (32 x 32 x 1024 at most: stage 2's first bottleneck), the shortcut gradient (64 K) and its dilation (256 K)
const size_t kRxWork[6] = {262144, 262144, 1048576, 1048576, 1048576, 327680};

// The weight image of a ResNeXt29 conv's data gradient with the eval-mode BN scale folded in: a 1x1 layer w [M][K] -> wT [K][ldt] (ldt >= M,
// the rows beyond M zero: the K padding of the gradient GEMM); the grouped 3x3 (8 groups of G = M = K) [g][tap][m][k] -> [g][8 - tap][k][m]
void rx_pack_wT(const float* w, const float* scale, float* wT, int M, int K, int taps, int ldt, hipStream_t s) {
    if (taps == 9) launch_cvjp_pack_grouped(w, scale, wT, M, s);
    else launch_cvjp_transpose(w, M, K, K, scale, wT, ldt, s);
}

// The data gradient of one ResNeXt29 conv on its packed image (rx_pack_wT): g [B][Ho][Ho][groups * K] -> gx [B][Hin][Hin][groups * M] (M: the
// gradient's channels per group = the conv's input channels, K: the conv's output channels per group, padded for a 1x1 image with ldt > M),
// no split-K.  Stride 2: the grouped 3x3 runs at Hin = 2 Ho on the zero-dilated gradient (work: [B][Hin][Hin][groups * K]); the 1x1
// shortcut runs at Ho (work: [B][Ho][Ho][M]) and is scattered into the even pixels of gx.  res (optional, gx's shape; not with the
// stride-2 1x1) is added in the GEMM's epilogue.  slab (optional; dense convs): the split-K workspace with n_ref = max_batch x the GEMM's
// pixels, as the forward passes them (WideResNet); without it the launch is ResNeXt29's, bit for bit.
int rx_conv_dgrad(const float* wT, const float* g, float* gx, int M, int K, int taps, int groups, int B, int Ho, int stride, float* work,
                  const float* res, hipStream_t s, float* slab = nullptr, long slab_floats = 0, int maxB = 0) {
    const bool dil_in = stride == 2 && taps == 9, dil_out = stride == 2 && taps == 1;
    if (dil_in) launch_dilate2x_nhwc(g, work, B, Ho, groups * K, s);
    const int H = dil_in ? 2 * Ho : Ho;
    const GemmF32Args a = nhwc_conv_args(wT, nullptr, nullptr, dil_in ? work : g, dil_out ? work : gx, M, K, taps, B, H, 1, dil_out ? nullptr : res, 0, groups,
                                         groups * K, groups * M);
    if (launch_gemm_f32(a, s, slab, slab_floats, (long)maxB * H * H) != 0)
        return fail(DMAD_ERR_STATE, "classifier VJP: no GEMM for M = %d, K = %d, taps = %d", M, K, taps);
    if (dil_out) launch_dilate2x_nhwc(work, gx, B, Ho, M, s);
    return 0;
}

// g_spec = (d logits / d spec)^T g_logits of classify_resnext; logits: the forward it recomputes (B <= cvjpB)
int rx_vjp_pass(dmad_engine* e, const float* spec, int B, const float* g_logits, float* g_spec, float* logits, hipStream_t s) {
    const dmad_engine::TapeSlot* tp = e->cvjp_slot.data();          // slot 0: conv1's output, 3 i + 1 / + 2 / + 3: T1 / T2 / Y of bottleneck i
    CHK(classify_resnext(e, spec, B, logits, s, tp));
    float* G[6];
    G[0] = e->cvjp_work;
    for (int k = 1; k < 6; ++k) G[k] = G[k - 1] + kRxWork[k - 1] * e->cvjpB;
    float *gT = G[2], *gD = G[3], *gU = G[4], *gS = G[5], *gSd = G[5] + 65536l * e->cvjpB;
    // head: FC, 8 x 8 average pool and the last block's ReLU in one kernel
    launch_rx_head_bwd(g_logits, e->rxfcw, tp[27].p, G[0], B, e->cfg.num_classes, 64, 1024, s);
    float *cur = G[0], *nxt = G[1];
    int H = 8;
    for (int i = 8; i >= 0; --i) {
        const dmad_engine::RxBlock& b = e->rx[i];
        const int Ho = H, Hin = Ho * b.stride, Gc = b.D / 8;
        if (i < 8) launch_relu_mask(cur, tp[3 * i + 3].p, cur, (long)B * Ho * Ho * b.cout, s);     // the block output's ReLU
        CHK(rx_conv_dgrad(b.expand.wT, cur, gT, b.D, b.cout, 1, 1, B, Ho, 1, nullptr, nullptr, s));     // conv_expand (1x1) + bn_expand
        launch_relu_mask(gT, tp[3 * i + 2].p, gT, (long)B * Ho * Ho * b.D, s);
        CHK(rx_conv_dgrad(b.conv.wT, gT, gU, Gc, Gc, 9, 8, B, Ho, b.stride, gD, nullptr, s));          // grouped 3x3 (stride) + bn
        launch_relu_mask(gU, tp[3 * i + 1].p, gU, (long)B * Hin * Hin * b.D, s);
        const float* res = cur;                                                              // identity shortcut
        if (b.has_short) {                                                                   // 1x1 (stride) + bn at the output resolution,
            float* gsc = b.stride == 2 ? gSd : gS;                                           // scattered into the even pixels
            CHK(rx_conv_dgrad(b.shortc.wT, cur, gsc, b.cin, b.cout, 1, 1, B, Ho, b.stride, gS, nullptr, s));
            res = gsc;
        }
        CHK(rx_conv_dgrad(b.reduce.wT, gU, nxt, b.cin, b.D, 1, 1, B, Hin, 1, nullptr, res, s));       // conv_reduce (1x1) + bn, + shortcut
        std::swap(cur, nxt);
        H = Hin;
    }
    launch_rx_conv1_bwd(cur, tp[0].p, e->rxconv1.w, e->rxconv1.scale, g_spec, B, s);            // conv1's ReLU, bn and 1 <- 64 3x3 conv
    LASTCHK();
    return 0;
}

// first call: the transposed filterbank / DFT images and the gradient maps of up to 64 clips per pass
int mel_vjp_prepare(dmad_engine* e) {
    if (e->melvjpB) return 0;
    const int vB = e->maxB < 64 ? e->maxB : 64;
    const size_t rows = (size_t)vB * 32;
    CHK(e->alloc(&e->mel_fbT, (size_t)kMelLd * 32));
    CHK(e->alloc(&e->mel_dftAT, (size_t)2048 * kDftKT));
    launch_cvjp_transpose(e->fbA, 32, kMelLd, kMelLd, nullptr, e->mel_fbT, 32, nullptr);
    launch_cvjp_transpose(e->dftA, kDftM, 2048, 2048, nullptr, e->mel_dftAT, kDftKT, nullptr);
    HIPCHK(hipGetLastError());
    CHK(e->alloc(&e->melvjp_gM, rows * 32));
    CHK(e->alloc(&e->melvjp_gP, rows * kMelLd));
    CHK(e->alloc(&e->melvjp_gD, rows * kDftKT));
    CHK(e->alloc(&e->melvjp_gF, rows * 2048));
    HIPCHK(hipDeviceSynchronize());
    e->melvjpB = vB;
    return 0;
}

// g_x = (d melDB / d x)^T g_spec of mel_db (B <= melvjpB); spec: the forward it recomputes
int mel_vjp_pass(dmad_engine* e, const float* x, int B, const float* g_spec, float* g_x, float* spec, hipStream_t s) {
    CHK(mel_db(e, x, B, spec, s));                                          // leaves the DFT (dftD) and the mel power (melM) resident
    const long rows = (long)B * 32;
    auto gemm = [&](const GemmF32Args& g) -> int {
        if (launch_gemm_f32(g, s) != 0) return fail(DMAD_ERR_STATE, "mel VJP: no GEMM for M = %d, K = %d", g.M, g.K);
        return 0;
    };
    launch_mel_db_bwd(g_spec, e->melM, e->melvjp_gM, B, s);                                                        // dB
    CHK(gemm(plain_gemm(e->mel_fbT, e->melvjp_gM, e->melvjp_gP, nullptr, nullptr, kMelLd, 32, rows, kMelLd, 32, 0)));   // filterbank
    launch_mel_power_bwd(e->dftD, kDftLd, e->melvjp_gP, kMelLd, e->melvjp_gD, kDftKT, rows, s);                   // |.|^2
    CHK(gemm(plain_gemm(e->mel_dftAT, e->melvjp_gD, e->melvjp_gF, nullptr, nullptr, 2048, kDftKT, rows, 2048, kDftKT, 0)));   // DFT
    launch_mel_ola_bwd(e->melvjp_gF, g_x, B, e->L, s);                                                              // framing
    LASTCHK();
    return 0;
}

int mel_db_vjp(dmad_engine* e, const float* x, int B, const float* g_spec, float* g_x, float* spec, hipStream_t s) {
    CHK(need_with_classifier(e)); CHK(need_batch(e, B));
    CHK(mel_vjp_prepare(e));
    return for_passes(B, e->melvjpB, [&](int64_t b0, int bb) {
        return mel_vjp_pass(e, x + b0 * e->L, bb, g_spec + b0 * 1024, g_x + b0 * e->L, spec ? spec + b0 * 1024 : e->spec, s);
    });
}

// Masking loss of the imperceptible attack and its gradient, or the attack's update (masking.h), in passes of melvjpB clips
// on the mel front-end's DFT map and the mel VJP's gradient maps; melvjp_gM holds the per-frame hinge sums
int masking(dmad_engine* e, const float* delta, int B, const float* theta, const float* psd_scale, float* g_delta, float* loss, float* psd,
            const MaskingStep* step, hipStream_t s) {
    CHK(need_with_classifier(e)); CHK(need_batch(e, B));
    const int F = masking_frames(e->L);
    if (F < 1) return fail(DMAD_ERR_STATE, "masking loss: clip_len %d < the %d-sample window", e->L, kMaskWin);
    if (F > kMaskMaxFrames || (e->L & 3)) return fail(DMAD_ERR_STATE, "masking loss: clip_len %d gives %d frames (at most %d, clip_len a multiple of 4)", e->L, F, kMaskMaxFrames);
    CHK(mel_vjp_prepare(e));
    const MaskingWork w{e->dftA, e->mel_dftAT, e->dftD, e->melvjp_gD, e->melvjp_gF, e->melvjp_gM, kDftLd, kDftKT};
    const size_t L = e->L, TF = (size_t)kMaskBins * F;
    return for_passes(B, e->melvjpB, [&](int64_t b0, int bb) {
        MaskingStep st{};
        if (step) st = MaskingStep{step->x + b0 * L, step->delta + b0 * L, step->g_net + b0 * L, step->alpha + b0, step->signed_lr};
        if (masking_pass(w, delta + b0 * L, bb, (int)L, theta + b0 * TF, psd_scale + b0, loss + b0, psd ? psd + b0 * TF : nullptr,
                         step ? nullptr : g_delta + b0 * L, step ? &st : nullptr, s) != 0)
            return fail(DMAD_ERR_STATE, "masking loss: no GEMM for %d frame rows", bb * F);
        LASTCHK();
        return 0;
    });
}

// h16 = 1: the classifier's 16-bit tier where one is resident (ResNeXt29 on engines with a 16-bit side) — the fast mode's; 2: its
// split-f16 tier (exact-vote engines) — tier 1 of the exact-vote loops; every other caller (dmad_classify, the recheck tiers) gets the
// fp32 matrix cores
// VGG19_bn on the fp32 matrix cores.  tape (the VJP's forward): conv li writes its post-ReLU map into the tape's slot li and the first two Linear
// layers their post-ReLU vectors into slots 16 and 17 in place of act0 / act1 — the same launches with the same n_ref, so the same bits —
// and only the pooled maps pass through act0
int classify_vgg(dmad_engine* e, const float* spec, int B, float* logits, hipStream_t s, const dmad_engine::TapeSlot* tape = nullptr) {
    auto spare = [&](const float* in) { return in == e->act0 ? e->act1 : e->act0; };      // the work map `in` does not occupy
    float* cur = tape ? tape[0].p : e->act0;
    launch_vgg_conv1(spec, e->vconv1w, e->vscale[0], e->vshift[0], cur, B, s);
    int H = 32, cin = 64, li = 1;
    for (int i = 1; i < kVggCfgLen; ++i) {
        const int v = kVggCfg[i];
        float* nxt = (tape && v > 0) ? tape[li].p : spare(cur);
        if (v < 0) {
            launch_maxpool2_nhwc(cur, nxt, B, H, H, cin, s);
            H >>= 1;
        } else {
            launch_gemm_f32(nhwc_conv_args(e->vconvw[li], e->vscale[li], e->vshift[li], cur, nxt, v, cin, 9, B, H, 0, nullptr, 1, 0, 0), s, e->slab,
                            e->slab_floats, (long)e->maxB * H * H);      // (stride and ldx 0: the kernel's defaults, 1 and Cin)
            cin = v;
            ++li;
        }
        cur = nxt;
    }
    const int fin[3] = {512, 4096, 4096}, fout[3] = {4096, 4096, e->cfg.num_classes};
    for (int j = 0; j < 3; ++j) {
        float* dst = (j == 2) ? logits : tape ? tape[16 + j].p : spare(cur);
        launch_gemm_f32(plain_gemm(e->vfcw[j], cur, dst, nullptr, e->vfcb[j], fout[j], fin[j], B, fout[j], fin[j], j < 2), s, e->slab,
                        e->slab_floats, (long)e->maxB);
        cur = dst;
    }
    LASTCHK();
    return 0;
}

int classify(dmad_engine* e, const float* spec, int B, float* logits, hipStream_t s, int h16 = 0) {
    CHK(need_classifier(e)); CHK(need_batch(e, B));
    if (e->cls_kind == 1) return (h16 == 1 && e->rx_h16) ? classify_resnext_h16(e, spec, B, logits, s)
                                 : (h16 == 2 && e->rx_x3) ? classify_resnext_x3(e, spec, B, logits, s) : classify_resnext(e, spec, B, logits, s);
    if (e->cls_kind == 2) return classify_wrn(e, spec, B, logits, s);      // every tier falls to fp32, as for VGG19_bn
    if (e->cls_kind == 3) return classify_dn(e, spec, B, logits, s);       // likewise
    return classify_vgg(e, spec, B, logits, s);
}

constexpr size_t kVggWork = 65536;       // floats per spectrogram of one gradient ping-pong map: 32 x 32 x 64, the largest map

// The data gradient of a dense VGG19_bn 3x3 conv on its packed image (launch_cvjp_pack_dense): g [B][H][H][M] -> gx [B][H][H][K], the
// forward's GEMM with M and K exchanged.  slab / n_ref as the forward passes them: the split count follows from the layer and the
// engine's max_batch, never from B
int vgg_conv_dgrad(const float* wT, const float* g, float* gx, int M, int K, int B, int H, float* slab, long slab_floats, long n_ref, hipStream_t s) {
    if (launch_gemm_f32(nhwc_conv_args(wT, nullptr, nullptr, g, gx, K, M, 9, B, H, 1, nullptr), s, slab, slab_floats, n_ref) != 0)
        return fail(DMAD_ERR_STATE, "VGG19_bn VJP: no GEMM for M = %d, K = %d", K, M);
    return 0;
}

// g_spec = (d logits / d spec)^T g_logits of classify_vgg; logits: the forward it recomputes (B <= cvjpB)
int vgg_vjp_pass(dmad_engine* e, const float* spec, int B, const float* g_logits, float* g_spec, float* logits, hipStream_t s) {
    const dmad_engine::TapeSlot* tp = e->cvjp_slot.data();          // slots 0..15: the conv maps, 16 / 17: the FC vectors
    CHK(classify_vgg(e, spec, B, logits, s, tp));
    float *cur = e->cvjp_work, *nxt = e->cvjp_work + kVggWork * e->cvjpB;
    auto rows = [&](const float* wT, const float* g, float* out, int M, int K) -> int {      // out [B][M] = g [B][K] wT[M][K]^T
        if (launch_gemm_f32(plain_gemm(wT, g, out, nullptr, nullptr, M, K, B, M, K, 0), s, e->slab, e->slab_floats, (long)e->maxB) != 0)
            return fail(DMAD_ERR_STATE, "VGG19_bn VJP: no GEMM for M = %d, K = %d", M, K);
        return 0;
    };
    // classifier.6 (num_classes reduction elements, k ascending) with classifier.4's ReLU, then classifier.3 / .0 on their transposed images
    launch_rx_head_bwd(g_logits, e->vfcw[2], tp[17].p, cur, B, e->cfg.num_classes, 1, 4096, s);
    CHK(rows(e->vfcwT[1], cur, nxt, 4096, 4096));
    launch_relu_mask(nxt, tp[16].p, nxt, (long)B * 4096, s);
    CHK(rows(e->vfcwT[0], nxt, cur, 512, 4096));                                             // the gradient at the last pool's output
    int H = 1, li = 16;
    bool masked = false;                 // cur is the gradient at a ReLU's input (after a pool) / at its output (after a conv)
    for (int i = kVggCfgLen - 1; i >= 1; --i) {
        const int v = kVggCfg[i];
        if (v < 0) {                     // the pool and the ReLU of conv li - 1 in front of it
            H <<= 1;
            launch_vgg_pool_relu_bwd(cur, tp[li - 1].p, nxt, B, H, kVggCfg[i - 1], s);
            masked = true;
        } else {                         // conv li - 1 (its input: conv li - 2's map, or a pooled one) with its BN scale
            --li;
            if (!masked) launch_relu_mask(cur, tp[li].p, cur, (long)B * H * H * v, s);
            const int cin = kVggCfg[i - 1] > 0 ? kVggCfg[i - 1] : kVggCfg[i - 2];
            CHK(vgg_conv_dgrad(e->vconvwT[li], cur, nxt, v, cin, B, H, e->slab, e->slab_floats, (long)e->maxB * H * H, s));
            masked = false;
        }
        std::swap(cur, nxt);
    }
    launch_rx_conv1_bwd(cur, tp[0].p, e->vconv1w, e->vscale[0], g_spec, B, s);               // conv 0's ReLU, bn and 1 <- 64 3x3 conv
    LASTCHK();
    return 0;
}

// floats per spectrogram of the gradient work maps of wrn_vjp_pass: the block out / in gradients, g_h, its zero-dilation (stage 2's first
// block: 32 x 32 x 320), g_o, the shortcut's gradient at the output resolution (16 x 16 x 160 at most) and at the input resolution
const size_t kWrnWork[7] = {kWrnMap, kWrnMap, kWrnMap, 2 * kWrnMap, kWrnMap, kWrnMap / 4, kWrnMap};

// g_spec = (d logits / d spec)^T g_logits of classify_wrn; logits: the forward it recomputes (B <= cvjpB)
int wrn_vjp_pass(dmad_engine* e, const float* spec, int B, const float* g_logits, float* g_spec, float* logits, hipStream_t s) {
    const dmad_engine::TapeSlot* tp = e->cvjp_slot.data();          // slots 2 i / 2 i + 1: o / h of block i, 24: the final map
    CHK(classify_wrn(e, spec, B, logits, s, tp));
    float* G[7];
    G[0] = e->cvjp_work;
    for (int k = 1; k < 7; ++k) G[k] = G[k - 1] + kWrnWork[k - 1] * e->cvjpB;
    float *cur = G[0], *nxt = G[1], *gh = G[2], *gD = G[3], *go = G[4], *gS = G[5], *gSd = G[6];
    // head: FC^T (on the image that carries the final bn's scale), the 8 x 8 average pool and the last ReLU's mask: the gradient at block 11's output
    launch_rx_head_bwd(g_logits, e->wrn_fcws, tp[24].p, cur, B, e->cfg.num_classes, 64, 640, s);
    int H = 8;
    for (int i = 11; i >= 0; --i) {
        const dmad_engine::WrnBlock& b = e->wrn[i];
        const int Ho = H, Hin = Ho * b.stride;
        CHK(rx_conv_dgrad(b.w2T, cur, gh, b.cout, b.cout, 9, 1, B, Ho, 1, nullptr, nullptr, s, e->slab, e->slab_floats, e->maxB));       // conv2
        launch_relu_mask(gh, tp[2 * i + 1].p, gh, (long)B * Ho * Ho * b.cout, s);                                                                // relu2 (bn2's scale is in w1T)
        const float* gsc = nullptr;
        if (b.wsT) {                                                                                                                     // the 1x1 shortcut of the activated input
            float* out = b.stride == 2 ? gSd : gS;
            CHK(rx_conv_dgrad(b.wsT, cur, out, b.cin, b.cout, 1, 1, B, Ho, b.stride, gS, nullptr, s, e->slab, e->slab_floats, e->maxB));
            gsc = out;
        }
        CHK(rx_conv_dgrad(b.w1T, gh, go, b.cin, b.cout, 9, 1, B, Ho, b.stride, gD, gsc, s, e->slab, e->slab_floats, e->maxB));            // conv1 (stride) + the shortcut's
        launch_wrn_preact_bwd(go, tp[2 * i].p, b.s1, b.wsT ? nullptr : cur, nxt, (long)B * Hin * Hin, b.cin, s);                             // relu1, bn1, + the identity shortcut
        std::swap(cur, nxt);
        H = Hin;
    }
    launch_wrn_stem_bwd(cur, e->wrn_stem, g_spec, B, s);
    LASTCHK();
    return 0;
}

// floats per spectrogram of the gradient work maps of dn_vjp_pass: one gradient stream per resolution (the streams' pitches) and g_h
const size_t kDnWork[4] = {(size_t)1024 * 216, (size_t)256 * 304, (size_t)64 * 344, (size_t)1024 * 48};

// g_spec = (d logits / d spec)^T g_logits of classify_dn; logits: the forward it recomputes (B <= cvjpB).  The head's backward fills the
// last gradient stream; per layer, last to first: the transposed 3x3 of the layer's own 12-channel slice (complete by then: only later
// layers add to it) masked by h and scaled by bn2 -> g_h, then the transposed 1x1 masked by the recomputed bn1 decision and scaled by
// bn1, ADDED into channels [0, cin) of the same gradient stream — so a channel collects its terms in layer order, last to first; a
// transition's backward (pool, transposed 1x1, pre-activation) writes the whole previous gradient stream once.  100 launches.
int dn_vjp_pass(dmad_engine* e, const float* spec, int B, const float* g_logits, float* g_spec, float* logits, hipStream_t s) {
    const dmad_engine::TapeSlot* tp = e->cvjp_slot.data();          // slots 0..2: the streams, 3 + l: h of layer l
    CHK(classify_dn(e, spec, B, logits, s, tp));
    float* G[4];
    G[0] = e->cvjp_work;
    for (int k = 1; k < 4; ++k) G[k] = G[k - 1] + kDnWork[k - 1] * e->cvjpB;
    float* gh = G[3];
    launch_dn_head_bwd(g_logits, e->dn_fcws, tp[2].p, kDnPitch[2], e->dn_bns, e->dn_bnb, G[2], kDnPitch[2], B, 64, 342, e->cfg.num_classes, s);
    for (int blk = 2; blk >= 0; --blk) {
        const int H = kDnH[blk], ld = kDnPitch[blk];
        const long n_px = (long)B * H * H;
        for (int l = 16 * blk + 15; l >= 16 * blk; --l) {
            const dmad_engine::DnLayer& L = e->dn[l];
            launch_dn_growth_bwd(L.w2T, G[blk], ld, L.cin, tp[3 + l].p, L.s2, gh, B, H, s);
            launch_dn_pw(dn_pw_bwd(L.w1T, L.cin, 48, gh, 48, n_px, 0, H, tp[blk].p, ld, L.s1, L.b1, G[blk], ld, 1), true, s);
        }
        if (blk > 0) {
            const dmad_engine::DnTrans& T = e->dnT[blk - 1];
            const int Hp = kDnH[blk - 1], ldp = kDnPitch[blk - 1];
            launch_dn_pw(dn_pw_bwd(T.wT, T.cin, T.cout, G[blk], ld, (long)B * Hp * Hp, 1, Hp, tp[blk - 1].p, ldp, T.s, T.b, G[blk - 1], ldp, 0), true, s);
        }
    }
    launch_dn_stem_bwd(G[0], kDnPitch[0], e->dn_stem, g_spec, B, s);
    LASTCHK();
    return 0;
}

// dmad_dn_vjp_tape: post-ReLU map `index` (0..98, forward order) as the forward decided it.  An h map is copied from its slot; an o map, a
// transition's and the final map are recomputed from the stream by dn_preact, the function the forward's staging applied
int dn_vjp_tape(dmad_engine* e, int index, int B, float* out, hipStream_t s) {
    if (!e || !out) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(need_kind(e, 3));
    if (index < 0 || index > 98) return fail(DMAD_ERR_INVALID, "tape map %d outside [0, 98]", index);
    if (B < 1 || B > e->cvjp_lastB) return fail(DMAD_ERR_STATE, "the tape holds %d rows of a one-pass dmad_dn_vjp call, not %d", e->cvjp_lastB, B);
    const int blk = index / 33, j = index % 33, H = kDnH[blk];
    const long n_px = (long)B * H * H;
    const float* S = e->cvjp_slot[blk].p;
    if (index == 98 || j == 32) {
        const float* sc = index == 98 ? e->dn_bns : e->dnT[blk].s;
        const float* sh = index == 98 ? e->dn_bnb : e->dnT[blk].b;
        launch_dn_preact_map(S, kDnPitch[blk], sc, sh, out, n_px, kDnWidth[blk], s);
    } else if (j & 1) {
        HIPCHK(hipMemcpyAsync(out, e->cvjp_slot[3 + 16 * blk + j / 2].p, (size_t)n_px * 48 * sizeof(float), hipMemcpyDeviceToDevice, s));
    } else {
        const dmad_engine::DnLayer& L = e->dn[16 * blk + j / 2];
        launch_dn_preact_map(S, kDnPitch[blk], L.s1, L.b1, out, n_px, L.cin, s);
    }
    LASTCHK();
    return 0;
}

// dmad_classify_vjp / dmad_vgg_vjp / dmad_wrn_vjp / dmad_dn_vjp: the VJP of classifier `kind` in passes of the reservation; lastB remembers a one-pass call
// for the tape reader
int cls_vjp(dmad_engine* e, int kind, const float* spec, int B, const float* g_logits, float* g_spec, float* logits, hipStream_t s) {
    if (!e || !spec || !g_logits || !g_spec) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(need_kind(e, kind));
    if (!e->cvjpB) return fail(DMAD_ERR_STATE, "no %s VJP workspace: call %s first", kCls[kind].vjp_of, kCls[kind].reserve);
    CHK(need_batch(e, B));
    const int nc = e->cfg.num_classes;
    const auto pass = kind == 1 ? rx_vjp_pass : kind == 2 ? wrn_vjp_pass : kind == 3 ? dn_vjp_pass : vgg_vjp_pass;
    e->cvjp_lastB = 0;
    CHK(for_passes(B, e->cvjpB, [&](int64_t b0, int bb) {
        return pass(e, spec + b0 * 1024, bb, g_logits + b0 * nc, g_spec + b0 * 1024, logits ? logits + b0 * nc : e->logits, s);
    }));
    if (B <= e->cvjpB) e->cvjp_lastB = B;
    return 0;
}

// dmad_vgg_vjp_tape / dmad_wrn_vjp_tape: slot `index` of the tape a one-pass call left, B rows
int cls_vjp_tape(dmad_engine* e, int kind, int index, int B, float* out, hipStream_t s) {
    if (!e || !out) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(need_kind(e, kind));
    const int slots = (int)cls_tape_layout(e).size();
    if (index < 0 || index >= slots) return fail(DMAD_ERR_INVALID, "tape map %d outside [0, %d]", index, slots - 1);
    if (B < 1 || B > e->cvjp_lastB) return fail(DMAD_ERR_STATE, "the tape holds %d rows of a one-pass %s call, not %d", e->cvjp_lastB, kCls[kind].vjp, B);
    const dmad_engine::TapeSlot& t = e->cvjp_slot[index];
    HIPCHK(hipMemcpyAsync(out, t.p, (size_t)B * t.floats * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

// the reservation of classifier `kind`'s VJP: its tape and `work` floats of gradient maps per spectrogram; pack(): its backward images
template <class Pack>
int reserve_cls_vjp(dmad_engine* e, int max_batch, int kind, size_t work, Pack pack) {
    return reserve_vjp(
        e, max_batch, &dmad_engine::maxB, &dmad_engine::cvjpB, [&] { return need_kind(e, kind); },
        [&] { return std::vector<float**>{&e->cvjp_tape, &e->cvjp_work}; },
        [&]() -> int {
            e->cvjp_lastB = 0;               // the tape a reader could ask for is gone
            e->cvjp_slot.clear();
            return pack();
        },
        [&](int vB) -> int {
            const std::vector<size_t> lay = cls_tape_layout(e);
            size_t tape = 0;
            for (size_t f : lay) tape += f;
            CHK(e->alloc(&e->cvjp_tape, (size_t)vB * tape));
            CHK(e->alloc(&e->cvjp_work, (size_t)vB * work));
            float* at = e->cvjp_tape;
            for (size_t f : lay) { e->cvjp_slot.push_back({at, f}); at += f * vB; }
            return 0;
        });
}

// the exact-vote loops refuse a WideResNet or DenseNet engine: no recheck bound has been measured for these classifiers
int need_vote_bound(const dmad_engine* e) {
    if (e->cls_final && (e->cls_kind == 2 || e->cls_kind == 3) && e->mode == DMAD_MODE_EXACT_VOTES)
        return fail(DMAD_ERR_STATE, "no recheck bound has been measured for %s: the exact-vote loops refuse it (DMAD_MODE_FAST and DMAD_MODE_FP32 serve it)",
                    kCls[e->cls_kind].net);
    return 0;
}

// WaveNet path of the entry points that hand waveforms (or logits of purified waveforms) back — dmad_wavenet_eps, dmad_one_shot,
// dmad_ddpm_step / _purify, dmad_query_logits: the mode's own path, except that an exact-vote engine in DMAD_MODE_EXACT_VOTES serves
// them on the tier dmad_set_waveform_tier selected (default: the split-f16 tier, fp32-grade) — only the vote loop has a recheck
inline int wave_path(const dmad_engine* e) {
    if (!(e->bf16 && e->f32) || e->mode != DMAD_MODE_EXACT_VOTES) return PATH_DEFAULT;
    return e->wave_tier;
}

// the classifier tier of a vote loop's FIRST pass (and of the mode-default paths): the 16-bit tier (ResNeXt29) in DMAD_MODE_FAST only.
// Round 5, measured on the calibrated stand-in (profiles/r05b_resnext29_error_attribution.json): the f16 classifier's leader-difference
// error is 0.08-0.16 against 0.016-0.030 for the f16 WaveNet in front of the fp32 classifier — a bound that covered it would send a
// quarter of the samples to the recheck tiers, so the exact-vote mode keeps the classifier on the fp32 matrix cores in every tier.
// It runs the classifier's SPLIT-F16 tier there (fp32-grade: its error, ~1e-4, disappears under the WaveNet's): a third of the fp32 tier's time.
inline int cls_tier(const dmad_engine* e) {
    if (e->mode == DMAD_MODE_FAST) return e->rx_h16 ? 1 : 0;
    return (e->mode == DMAD_MODE_EXACT_VOTES && e->rx_x3 && e->cls_kind == 1) ? 2 : 0;
}

// ... and of a recheck tier: the split-f16 WaveNet tier is paired with the classifier's split-f16 tier (ResNeXt29; both fp32-grade, their
// errors add up to ~3e-4 under tau2 = 1e-3 — the fp32 ResNeXt29 at recheck batch sizes cost 0.8 ms per sample, 45 % on top of the
// WaveNet's), the exact-fp32 WaveNet tier with the fp32 classifier: what reaches tier 3 is the fp32 path bit for bit
inline int cls_tier_of_path(const dmad_engine* e, int path) { return (path == PATH_X3 && e->rx_x3 && e->cls_kind == 1) ? 2 : 0; }

// dmad_set_{,spec_}recheck_margin{,2}: the first pass's bound (tier 1) must be >= 0; the middle tier's (tier 2) must not be NaN,
// < 0 turns that tier off (the queued samples go straight to the exact-fp32 tier)
int set_recheck_bound(dmad_engine* e, bool spec, int tier, float tau) {
    if (!e) return fail(DMAD_ERR_INVALID, "null engine");
    if (tier == 1 && !(tau >= 0.f)) return fail(DMAD_ERR_INVALID, "recheck margin must be >= 0");
    if (tau != tau) return fail(DMAD_ERR_INVALID, "recheck margin is NaN");
    RecheckTiers& rt = spec ? e->spec_rt : e->wave_rt;
    (tier == 1 ? rt.tau1 : rt.tau2) = tau;
    return 0;
}

int read_recheck_stats(dmad_engine* e, bool spec, int64_t* samples, int64_t* rechecked, int64_t* rechecked_fp32, int32_t reset) {
    if (!e) return fail(DMAD_ERR_INVALID, "null engine");
    RecheckTiers& rt = spec ? e->spec_rt : e->wave_rt;
    if (samples) *samples = rt.samples;
    if (rechecked) *rechecked = rt.rechecked;
    if (rechecked_fp32) *rechecked_fp32 = rt.rechecked_fp32;
    if (reset) rt.samples = rt.rechecked = rt.rechecked_fp32 = 0;
    return 0;
}

// M5: checks the geometry against what m5.hip serves and packs the weight images of both directions into one buffer
int finalize_m5(dmad_engine* e) {
    auto find = [&](const char* name) -> const HostW* {
        auto it = e->hw.find(name);
        if (it == e->hw.end()) { fail(DMAD_ERR_STATE, "weight '%s' was not loaded", name); return nullptr; }
        return &it->second;
    };
    const HostW* c1 = find("m5.conv1.w");
    const HostW* st = find("m5.stride");
    const HostW* fw = find("m5.fc.w");
    if (!c1 || !st || !fw) return DMAD_ERR_STATE;
    if (c1->shape.size() != 3) return fail(DMAD_ERR_SHAPE, "M5: conv1.weight must be [n_channel][n_input][first_kernel_size]");
    if (c1->shape[1] != 1) return fail(DMAD_ERR_SHAPE, "M5: n_input = %lld is not supported (only 1)", (long long)c1->shape[1]);
    if (c1->shape[0] != kM5Ch) return fail(DMAD_ERR_SHAPE, "M5: n_channel = %lld is not supported (only %d)", (long long)c1->shape[0], kM5Ch);
    if (st->v[0] != (float)kM5Stride) return fail(DMAD_ERR_SHAPE, "M5: stride = %g is not supported (only %d)", st->v[0], kM5Stride);
    const int K1 = (int)c1->shape[2];
    if (K1 != 80 && K1 != 160) return fail(DMAD_ERR_SHAPE, "M5: first_kernel_size = %d is not supported (80 or 160)", K1);
    if (fw->shape.size() != 2 || fw->shape[1] != 2 * kM5Ch) return fail(DMAD_ERR_SHAPE, "M5: fc1.weight must be [n_output][%d] (n_channel = %d)", 2 * kM5Ch, kM5Ch);
    const int NO = (int)fw->shape[0];
    if (NO > kM5MaxOut) return fail(DMAD_ERR_SHAPE, "M5: n_output = %d is not supported (at most %d)", NO, kM5MaxOut);
    if (const char* m = m5_geometry(e->L, K1, NO, &e->m5g)) return fail(DMAD_ERR_SHAPE, "M5: %s (clip_len %d, first_kernel_size %d, n_output %d)", m, e->L, K1, NO);
    const int cin[4] = {1, 32, 32, 64}, cout[4] = {32, 32, 64, 64};
    std::vector<float> img;
    size_t off[18];
    int n = 0;
    auto put = [&](size_t count) { off[n++] = img.size(); img.resize(img.size() + ((count + 3) & ~(size_t)3), 0.f); return img.data() + off[n - 1]; };
    {
        float* t = put((size_t)K1 * kM5Ch);                  // [k][c]
        for (int c = 0; c < kM5Ch; ++c) for (int k = 0; k < K1; ++k) t[k * kM5Ch + c] = c1->v[(size_t)c * K1 + k];
        t = put((size_t)K1 * kM5Ch);                         // [c][k]
        memcpy(t, c1->v.data(), (size_t)K1 * kM5Ch * sizeof(float));
    }
    for (int l = 1; l < 4; ++l) {
        char name[32];
        snprintf(name, sizeof name, "m5.conv%d.w", l + 1);
        const HostW* w = e->get(name, {cout[l], cin[l], 3});
        if (!w) return DMAD_ERR_SHAPE;
        float* f = put((size_t)cout[l] * cin[l] * 3);        // [ci][tap][co]
        for (int co = 0; co < cout[l]; ++co) for (int ci = 0; ci < cin[l]; ++ci) for (int t = 0; t < 3; ++t)
            f[((size_t)ci * 3 + t) * cout[l] + co] = w->v[((size_t)co * cin[l] + ci) * 3 + t];
        float* b = put((size_t)cout[l] * cin[l] * 3);        // [co][tap][ci]
        for (int co = 0; co < cout[l]; ++co) for (int ci = 0; ci < cin[l]; ++ci) for (int t = 0; t < 3; ++t)
            b[((size_t)co * 3 + t) * cin[l] + ci] = w->v[((size_t)co * cin[l] + ci) * 3 + t];
    }
    for (int l = 0; l < 4; ++l)
        for (int k = 0; k < 2; ++k) {
            char name[32];
            snprintf(name, sizeof name, k ? "m5.shift%d" : "m5.scale%d", l + 1);
            const HostW* w = e->get(name, {cout[l]});
            if (!w) return DMAD_ERR_SHAPE;
            memcpy(put((size_t)cout[l]), w->v.data(), (size_t)cout[l] * sizeof(float));
        }
    memcpy(put(fw->v.size()), fw->v.data(), fw->v.size() * sizeof(float));
    const HostW* fb = e->get("m5.fc.b", {NO});
    if (!fb) return DMAD_ERR_SHAPE;
    memcpy(put((size_t)NO), fb->v.data(), (size_t)NO * sizeof(float));
    CHK(e->upload(&e->m5_buf, img));
    const float* d = e->m5_buf;
    M5Weights& W = e->m5w;
    n = 0;
    W.w1t = d + off[n++]; W.w1c = d + off[n++];
    for (int l = 0; l < 3; ++l) { W.wf[l] = d + off[n++]; W.wb[l] = d + off[n++]; }
    for (int l = 0; l < 4; ++l) { W.scale[l] = d + off[n++]; W.shift[l] = d + off[n++]; }
    W.fcw = d + off[n++]; W.fcb = d + off[n++];
    return need_kernels(KF_M5);
}

// KWS: checks the geometry against what kws.hip serves and packs the weight images of both directions into one buffer
int finalize_kws(dmad_engine* e) {
    auto find = [&](const char* name) -> const HostW* {
        auto it = e->hw.find(name);
        if (it == e->hw.end()) { fail(DMAD_ERR_STATE, "weight '%s' was not loaded", name); return nullptr; }
        return &it->second;
    };
    auto is = [](const HostW* w, std::initializer_list<int64_t> shape) { return w->shape == std::vector<int64_t>(shape); };
    const char* P = "kws.CRNN_model.";
    const HostW* dw = find("kws.CRNN_model.sepconv.0.weight");
    const HostW* pw = find("kws.CRNN_model.sepconv.1.weight");
    const HostW* hh = find("kws.CRNN_model.gru.weight_hh_l0");
    const HostW* uw = find("kws.apply_attn.U.weight");
    const HostW* st = find("kws.stride");
    const HostW* ks = find("kws.kernel_size");
    if (!dw || !pw || !hh || !uw || !st || !ks) return DMAD_ERR_STATE;
    if (dw->shape.size() != 3 || pw->shape.size() != 3) return fail(DMAD_ERR_SHAPE, "KWS: sepconv weights must be Conv1d weights [out][in / groups][k]");
    if (dw->shape[0] != kKwsIn || dw->shape[1] != 1) return fail(DMAD_ERR_SHAPE, "KWS: in_size = %lld is not supported (only %d, depthwise)", (long long)dw->shape[0], kKwsIn);
    if (st->v.size() != 2 || st->v[0] != 8.f || st->v[1] != 2.f)
        return fail(DMAD_ERR_SHAPE, "KWS: stride = (%g, %g) is not supported (only (8, 2))", st->v.size() > 0 ? st->v[0] : 0.f, st->v.size() > 1 ? st->v[1] : 0.f);
    if (ks->v.size() != 2 || ks->v[0] != 20.f || ks->v[1] != (float)kKwsK || dw->shape[2] != kKwsK || !is(pw, {pw->shape[0], kKwsIn, 1}))
        return fail(DMAD_ERR_SHAPE, "KWS: kernel_size = (%g, %g) is not supported (only (20, %d): a 5-tap depthwise conv, one pointwise group)",
                    ks->v.size() > 0 ? ks->v[0] : 0.f, ks->v.size() > 1 ? ks->v[1] : 0.f, kKwsK);
    if (pw->shape[0] != kKwsH || !is(hh, {kKwsG, kKwsH}))
        return fail(DMAD_ERR_SHAPE, "KWS: hidden_size = %lld is not supported (only %d)", (long long)pw->shape[0], kKwsH);
    if (!e->hw.count("kws.CRNN_model.gru.weight_ih_l1") || e->hw.count("kws.CRNN_model.gru.weight_ih_l2"))
        return fail(DMAD_ERR_SHAPE, "KWS: gru_num_layers is not supported (only 2)");
    if (!e->hw.count("kws.CRNN_model.gru.weight_ih_l0_reverse")) return fail(DMAD_ERR_SHAPE, "KWS: num_dirs = 1 is not supported (only a bidirectional GRU)");
    if (!is(uw, {kKwsOut, 2 * kKwsH})) return fail(DMAD_ERR_SHAPE, "KWS: num_classes = %lld is not supported (only %d)", uw->shape.empty() ? 0ll : (long long)uw->shape[0], kKwsOut);
    std::vector<float> img;
    size_t off[24];
    int n = 0;
    auto put = [&](size_t count) { off[n++] = img.size(); img.resize(img.size() + ((count + 3) & ~(size_t)3), 0.f); return img.data() + off[n - 1]; };
    auto copy = [&](const std::string& name, std::initializer_list<int64_t> shape) -> int {
        const HostW* w = e->get(name, shape);
        if (!w) return DMAD_ERR_SHAPE;
        memcpy(put(w->v.size()), w->v.data(), w->v.size() * sizeof(float));
        return 0;
    };
    // rows x cols -> cols x rows
    auto transposed = [&](const float* src, int rows, int cols) {
        float* t = put((size_t)rows * cols);
        for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) t[(size_t)c * rows + r] = src[(size_t)r * cols + c];
    };
    CHK(copy(std::string(P) + "sepconv.0.weight", {kKwsIn, 1, kKwsK}));
    CHK(copy(std::string(P) + "sepconv.0.bias", {kKwsIn}));
    transposed(pw->v.data(), kKwsH, kKwsIn);
    CHK(copy(std::string(P) + "sepconv.1.weight", {kKwsH, kKwsIn, 1}));
    CHK(copy(std::string(P) + "sepconv.1.bias", {kKwsH}));
    for (int l = 0; l < 2; ++l) {                          // the two directions of a layer side by side: row = direction * 192 + gate row
        const int K = l ? 2 * kKwsH : kKwsH;
        std::vector<float> cat[4];
        const char* kind[4] = {"weight_ih", "bias_ih", "weight_hh", "bias_hh"};
        for (int k = 0; k < 4; ++k)
            for (int d = 0; d < 2; ++d) {
                char name[96];
                snprintf(name, sizeof name, "%sgru.%s_l%d%s", P, kind[k], l, d ? "_reverse" : "");
                const HostW* w = k == 0 ? e->get(name, {kKwsG, K}) : k == 2 ? e->get(name, {kKwsG, kKwsH}) : e->get(name, {kKwsG});
                if (!w) return DMAD_ERR_SHAPE;
                cat[k].insert(cat[k].end(), w->v.begin(), w->v.end());
            }
        transposed(cat[0].data(), 2 * kKwsG, K);
        memcpy(put(cat[0].size()), cat[0].data(), cat[0].size() * sizeof(float));
        memcpy(put(cat[1].size()), cat[1].data(), cat[1].size() * sizeof(float));
        transposed(cat[2].data(), 2 * kKwsG, kKwsH);
        memcpy(put(cat[2].size()), cat[2].data(), cat[2].size() * sizeof(float));
        memcpy(put(cat[3].size()), cat[3].data(), cat[3].size() * sizeof(float));
    }
    const HostW* wx = e->get("kws.attn_layer.Wx_b.weight", {2 * kKwsH, 2 * kKwsH});
    if (!wx) return DMAD_ERR_SHAPE;
    transposed(wx->v.data(), 2 * kKwsH, 2 * kKwsH);
    CHK(copy("kws.attn_layer.Wx_b.weight", {2 * kKwsH, 2 * kKwsH}));
    CHK(copy("kws.attn_layer.Wx_b.bias", {2 * kKwsH}));
    CHK(copy("kws.attn_layer.Vt.weight", {1, 2 * kKwsH}));
    CHK(copy("kws.apply_attn.U.weight", {kKwsOut, 2 * kKwsH}));
    CHK(e->upload(&e->kws_buf, img));
    const float* d = e->kws_buf;
    KwsWeights& W = e->kwsw;
    n = 0;
    W.dw = d + off[n++]; W.dwb = d + off[n++]; W.pwT = d + off[n++]; W.pw = d + off[n++]; W.pwb = d + off[n++];
    for (int l = 0; l < 2; ++l) {
        W.wihT[l] = d + off[n++]; W.wih[l] = d + off[n++]; W.bih[l] = d + off[n++];
        W.whhT[l] = d + off[n++]; W.whh[l] = d + off[n++]; W.bhh[l] = d + off[n++];
    }
    W.wxT = d + off[n++]; W.wx = d + off[n++]; W.wxb = d + off[n++]; W.vt = d + off[n++]; W.u = d + off[n++];
    return need_kernels(KF_KWS);
}

}  // namespace

extern "C" {

const char* dmad_last_error(void) { return g_err.c_str(); }
const char* dmad_version(void) { return "dmad-hip 0.5.1 (gfx950)"; }
const char* dmad_last_warning(void) { return g_warn.c_str(); }

int dmad_create(const dmad_config* cfg, dmad_engine** out) {
    if (!cfg || !out) return fail(DMAD_ERR_INVALID, "null argument");
    if (cfg->struct_size != (int32_t)sizeof(dmad_config))       // a caller built against another revision of dmad.h
        return fail(DMAD_ERR_INVALID, "dmad_config.struct_size is %d, this library's dmad_config has %d bytes (%s)", cfg->struct_size,
                    (int)sizeof(dmad_config), dmad_version());
    if (cfg->res_channels != 256 || cfg->skip_channels != 256)
        return fail(DMAD_ERR_INVALID, "only res_channels = skip_channels = 256 is supported (got %d/%d)", cfg->res_channels, cfg->skip_channels);
    if (cfg->embed_dim_in != 128 || cfg->embed_dim_mid != 512 || cfg->embed_dim_out != 512)
        return fail(DMAD_ERR_INVALID, "only step-embedding dims 128/512/512 are supported");
    if (cfg->num_res_layers < 1 || cfg->num_res_layers > 64) return fail(DMAD_ERR_INVALID, "num_res_layers %d outside [1,64]", cfg->num_res_layers);
    if (cfg->dilation_cycle < 1 || cfg->dilation_cycle > 12) return fail(DMAD_ERR_INVALID, "dilation_cycle %d outside [1,12]", cfg->dilation_cycle);
    if (cfg->clip_len < 128 || cfg->clip_len % 128) return fail(DMAD_ERR_INVALID, "clip_len %d must be a positive multiple of 128", cfg->clip_len);
    if (cfg->with_classifier && cfg->clip_len != 16000) return fail(DMAD_ERR_INVALID, "the mel front-end needs clip_len = 16000");
    if (cfg->max_batch < 1) return fail(DMAD_ERR_INVALID, "max_batch must be >= 1");
    if (cfg->precision != DMAD_BF16 && cfg->precision != DMAD_FP32 && cfg->precision != DMAD_EXACT)
        return fail(DMAD_ERR_INVALID, "unknown precision %d", cfg->precision);
    if (cfg->recheck_batch < 0) return fail(DMAD_ERR_INVALID, "recheck_batch %d < 0", cfg->recheck_batch);
    if (cfg->half_type != DMAD_HALF_BF16 && cfg->half_type != DMAD_HALF_F16) return fail(DMAD_ERR_INVALID, "unknown half_type %d", cfg->half_type);
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(DMAD_ERR_HIP, "no HIP device visible");
    dmad_engine* e = new dmad_engine();
    e->cfg = *cfg;
    e->L = cfg->clip_len; e->LP = cfg->clip_len + 2 * kPad; e->NL = cfg->num_res_layers; e->maxB = cfg->max_batch;
    e->LPm = cfg->clip_len + 2048;
    e->bf16 = cfg->precision != DMAD_FP32;
    e->f32 = cfg->precision != DMAD_BF16;
    e->f16 = cfg->half_type == DMAD_HALF_F16;
    e->maxB32 = cfg->precision == DMAD_FP32 ? cfg->max_batch : (cfg->recheck_batch > 0 ? cfg->recheck_batch : 32);
    if (e->maxB32 > cfg->max_batch) e->maxB32 = cfg->max_batch;
    e->mode = cfg->precision == DMAD_EXACT ? DMAD_MODE_EXACT_VOTES : (cfg->precision == DMAD_FP32 ? DMAD_MODE_FP32 : DMAD_MODE_FAST);
    e->wave_rt.tau1 = cfg->half_type == DMAD_HALF_F16 ? 0.034f : 0.30f;  // measured logit-difference error (against the leader) of the 16-bit path x 1.4 (see dmad.h)
    e->wave_rt.tau2 = 1e-3f;                // the same for the split-f16 tier (dmad_set_recheck_margin2)
    e->un_h16 = cfg->precision != DMAD_FP32;    // engines with a 16-bit side also get the UNet's f16 tier (once UNet weights are loaded)
    e->rx_h16 = cfg->precision != DMAD_FP32;    // ... and ResNeXt29's (once its weights are loaded)
    if (!env_switch_on("DMAD_RX_H16")) e->rx_h16 = false;      // A/B switch: ResNeXt29 on the fp32 matrix cores in every tier
    e->rx_x3 = cfg->precision == DMAD_EXACT;    // ... and its split-f16 tier
    if (!env_switch_on("DMAD_RX_X3")) e->rx_x3 = false;        // A/B switch
    e->spec_rt.tau1 = 0.13f;                // spec-domain vote loop: measured logit-difference error of the f16 UNet chain x headroom (see dmad.h)
    e->spec_rt.tau2 = 5e-4f;                // ... of the chain on the split-f16 tier (measured 2.3e-4)
    e->un_x3 = cfg->precision == DMAD_EXACT;    // exact-vote engines also hold the UNet's split-f16 middle tier
    const bool wn = cfg->with_wavenet != 0;
    if (e->bf16 && !wn_final_p_supported(cfg->num_res_layers)) {
        delete e;
        return fail(DMAD_ERR_INVALID, "bf16 path does not support num_res_layers = %d", cfg->num_res_layers);
    }
    const size_t B = e->maxB, L = e->L, LP = e->LP, NL = e->NL, B32 = e->maxB32;
    int r = 0;
    do {
        if ((r = need_kernels(KF_GEMM_F32))) break;
        if ((r = e->alloc(&e->xt, B * L))) break;
        if ((r = e->alloc(&e->eps, B * L))) break;
        if ((r = e->alloc(&e->x0, B * L))) break;
        if ((r = e->alloc(&e->znoise, B * L))) break;
        if (e->bf16 && wn) {
            if ((r = e->alloc(&e->hA, B * LP * kC, true))) break;
            if ((r = e->alloc(&e->hB, B * LP * kC, true))) break;
            if ((r = e->alloc(&e->gstore, NL * B * L * kC))) break;
            if ((r = need_kernels(KF_WN_LAYER | KF_WN_FINAL))) break;
        }
        if (e->f32 && wn) {
            if ((r = e->alloc(&e->hA32, B32 * LP * kC, true))) break;
            if ((r = e->alloc(&e->hB32, B32 * LP * kC, true))) break;
            if ((r = e->alloc(&e->H32, B32 * L * 512))) break;
            if ((r = e->alloc(&e->g32, B32 * L * 256))) break;
            if ((r = e->alloc(&e->skip32, B32 * L * 256))) break;
            if (e->bf16 && (r = need_kernels(KF_GEMM_X3))) break;
        }
        if (e->bf16 && e->f32) {             // recheck queue of the exact-vote mode
            e->rc_cap = 1l << 20;
            if (const char* q = getenv("DMAD_RECHECK_QUEUE")) {     // tests: a small queue exercises the mid-call drain
                const long v = atol(q);
                if (v >= 1 && v < e->rc_cap) e->rc_cap = v;
            }
            if (e->rc_cap < (long)e->maxB) e->rc_cap = e->maxB;    // one batch always fits: the drain condition needs no more
            if ((r = e->alloc(&e->rc_list, (size_t)e->rc_cap))) break;
            if ((r = e->alloc(&e->rc_list2, (size_t)e->rc_cap))) break;
            if ((r = e->alloc(&e->rc_n, 1, true))) break;
            hipError_t he = hipHostMalloc((void**)&e->rc_n_host, sizeof(unsigned long long), hipHostMallocDefault);
            if (he != hipSuccess) { r = fail(DMAD_ERR_HIP, "hipHostMalloc failed: %s", hipGetErrorString(he)); break; }
        }
        if (cfg->with_classifier) {
            if ((r = e->alloc(&e->mel_xp, B * e->LPm))) break;
            if ((r = e->alloc(&e->dftD, B * 32 * kDftLd))) break;
            if ((r = e->alloc(&e->melP, B * 32 * kMelLd))) break;
            if ((r = e->alloc(&e->melM, B * 32 * 32))) break;
            if ((r = e->alloc(&e->spec, B * 1024))) break;
            if ((r = e->alloc(&e->act0, B * 1024 * 64))) break;
            if ((r = e->alloc(&e->act1, B * 1024 * 64))) break;
            if ((r = e->alloc(&e->logits, B * cfg->num_classes))) break;
            e->slab_floats = 8l << 20;           // 32 MiB split-K workspace (largest user: 16 x [B*4][512])
            if (e->slab_floats < (long)B * 16 * 4096) e->slab_floats = (long)B * 16 * 4096;
            if ((r = e->alloc(&e->slab, (size_t)e->slab_floats))) break;
            if ((r = init_mel_constants(e))) break;
        }
    } while (0);
    if (r) { dmad_destroy(e); return r; }
    *out = e;
    return 0;
}

void dmad_destroy(dmad_engine* e) {
    if (!e) return;
    for (hipEvent_t ev : e->prof_ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->prof_ev_f) (void)hipEventDestroy(ev);
    if (e->rc_n_host) (void)hipHostFree(e->rc_n_host);
    for (auto& a : e->allocs) (void)hipFree(a.first);
    delete e;
}

int64_t dmad_device_bytes(const dmad_engine* e) { return e ? e->bytes : 0; }

int dmad_profile_layers(dmad_engine* e, int32_t max_launches) {
    if (!e || max_launches < 0) return fail(DMAD_ERR_INVALID, "bad argument");
    e->prof_used = e->prof_used_f = 0;
    e->prof_on = max_launches > 0;
    while (e->prof_ev.size() < (size_t)max_launches * 2) {
        hipEvent_t ev;
        HIPCHK(hipEventCreate(&ev));
        e->prof_ev.push_back(ev);
    }
    const size_t nf = ((size_t)max_launches + e->NL - 1) / (e->NL > 1 ? e->NL - 1 : 1) + 1;   // one final launch per NL-1 timed layer launches
    while (e->prof_ev_f.size() < nf * 2) {
        hipEvent_t ev;
        HIPCHK(hipEventCreate(&ev));
        e->prof_ev_f.push_back(ev);
    }
    return 0;
}

static int prof_sum(std::vector<hipEvent_t>& evs, size_t used, float* total_ms, int32_t* launches) {
    double tot = 0.0;
    const size_t pairs = used / 2;
    if (pairs) HIPCHK(hipEventSynchronize(evs[used - 1]));
    for (size_t i = 0; i < pairs; ++i) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, evs[2 * i], evs[2 * i + 1]));
        tot += ms;
    }
    *total_ms = (float)tot;
    *launches = (int32_t)pairs;
    return 0;
}

int dmad_profile_read(dmad_engine* e, float* total_ms, int32_t* launches) {
    if (!e || !total_ms || !launches) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(prof_sum(e->prof_ev, e->prof_used, total_ms, launches));
    e->prof_used = 0;
    e->prof_on = false;
    return 0;
}

int dmad_profile_read_final(dmad_engine* e, float* total_ms, int32_t* launches) {
    if (!e || !total_ms || !launches) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(prof_sum(e->prof_ev_f, e->prof_used_f, total_ms, launches));
    e->prof_used_f = 0;
    return 0;
}

int dmad_load_weight(dmad_engine* e, const char* name, const float* host, const int64_t* shape, int32_t ndim) {
    if (!e || !name || !host || !shape || ndim < 1 || ndim > 4) return fail(DMAD_ERR_INVALID, "bad argument to dmad_load_weight");
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 1) return fail(DMAD_ERR_INVALID, "weight '%s': non-positive dimension", name);
        n *= shape[i];
    }
    HostW& h = e->hw[name];
    h.v.assign(host, host + n);
    h.shape.assign(shape, shape + ndim);
    return 0;
}

int dmad_finalize_weights(dmad_engine* e) {
    if (!e) return fail(DMAD_ERR_INVALID, "null engine");
    // finalises whichever part (WaveNet, classifier) has its weights loaded and is not packed yet
    bool did = false;
    if (!e->wn_final && e->hw.count("init.w")) {
        if (!e->cfg.with_wavenet) return fail(DMAD_ERR_STATE, "engine was created with with_wavenet = 0: it has no WaveNet workspace");
        CHK(finalize_wavenet(e));
        e->wn_final = true; did = true;
    }
    if (e->cfg.with_classifier && !e->cls_final && e->hw.count("vgg.conv0.w")) {
        CHK(finalize_classifier(e));
        e->cls_final = true; e->cls_kind = 0; did = true;
    } else if (e->cfg.with_classifier && !e->cls_final && e->hw.count("rx.conv1.w")) {
        CHK(finalize_resnext(e));
        e->cls_final = true; e->cls_kind = 1; did = true;
    } else if (e->cfg.with_classifier && !e->cls_final && e->hw.count("wrn.conv1.w")) {
        if (int r = finalize_wrn(e)) {       // a refused set leaves nothing behind, like a refused M5 set
            for (auto it = e->hw.begin(); it != e->hw.end();) it = it->first.compare(0, 4, "wrn.") == 0 ? e->hw.erase(it) : std::next(it);
            return r;
        }
        e->cls_final = true; e->cls_kind = 2; did = true;
    } else if (e->cfg.with_classifier && !e->cls_final && e->hw.count("dn.conv1.w")) {
        if (int r = finalize_dn(e)) {        // likewise
            for (auto it = e->hw.begin(); it != e->hw.end();) it = it->first.compare(0, 3, "dn.") == 0 ? e->hw.erase(it) : std::next(it);
            return r;
        }
        e->cls_final = true; e->cls_kind = 3; did = true;
    }
    if (!e->un_final && e->hw.count("un.time_embed.0.weight")) {
        if (!e->slab) {                     // engines created without a classifier have no split-K workspace yet
            e->slab_floats = 8l << 20;
            CHK(e->alloc(&e->slab, (size_t)e->slab_floats));
        }
        CHK(finalize_unet(e));
        e->un_final = true; did = true;
    }
    if (!e->m5_final && e->hw.count("m5.conv1.w")) {
        if (int r = finalize_m5(e)) {        // a refused set leaves nothing behind: the next finalise (of any part) must not retry it
            for (auto it = e->hw.begin(); it != e->hw.end();) it = it->first.compare(0, 3, "m5.") == 0 ? e->hw.erase(it) : std::next(it);
            return r;
        }
        e->m5_final = true; did = true;
    }
    if (!e->kws_final && e->hw.count("kws.CRNN_model.sepconv.0.weight")) {
        if (int r = finalize_kws(e)) {       // a refused set leaves nothing behind, like a refused M5 set
            for (auto it = e->hw.begin(); it != e->hw.end();) it = it->first.compare(0, 4, "kws.") == 0 ? e->hw.erase(it) : std::next(it);
            return r;
        }
        e->kws_final = true; did = true;
    }
    if (!did) return fail(DMAD_ERR_STATE, "nothing to finalise: no complete weight set was loaded");
    e->hw.clear();
    g_warn = e->warn;                       // dmad_last_warning(): empty unless this call found something to say
    e->warn.clear();
    return 0;
}

int dmad_wavenet_eps(dmad_engine* e, const float* x_t, int32_t t, int32_t B, float* eps, dmad_stream s) {
    if (!e || !x_t || !eps) return fail(DMAD_ERR_INVALID, "null argument");
    return wavenet_eps(e, x_t, t, B, eps, (hipStream_t)s, wave_path(e));
}

int dmad_one_shot(dmad_engine* e, const float* x_t, int32_t t, float c_a, float c_b, int32_t B, float* x0, dmad_stream s) {
    if (!e || !x_t || !x0) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(wavenet_eps(e, x_t, t, B, e->eps, (hipStream_t)s, wave_path(e)));
    launch_lincomb(0, x_t, e->eps, nullptr, c_a, c_b, 0.f, x0, (long)B * e->L, (hipStream_t)s);
    LASTCHK();
    return 0;
}

}  // extern "C"

namespace {
// the preconditions of the any-length exports (dmad_*_len), which run the exact-fp32 path whatever the engine's mode; checked ahead of
// the array pointers, so that an empty array (a null pointer from most hosts) is reported as the len = 0 it is
int need_len(const dmad_engine* e, const char* who, int len) {
    if (!e->f32) return fail(DMAD_ERR_STATE, "%s runs on the exact-fp32 path: a DMAD_BF16 engine holds no fp32 weights", who);
    if (len < 1 || len > e->L) return fail(DMAD_ERR_SHAPE, "%s: len %d outside [1, clip_len=%d]", who, len, e->L);
    return 0;
}

// dmad_ddpm_step / dmad_diffuse (len == 0: clip_len, on `path`) and their any-length forms; len == clip_len makes the fixed-length launches
int ddpm_step(dmad_engine* e, float* x, int t, float c_eps, float c_div, float c_sig, const float* z, uint64_t seed, uint64_t sample0, int B,
              hipStream_t s, int path, int len) {
    CHK(wavenet_eps(e, x, t, B, e->eps, s, path, nullptr, len));
    if (len && len != e->L) {
        launch_sched_len(2, x, e->eps, z, c_eps, c_div, c_sig, c_sig != 0.f, seed, sample0, 1u + (uint32_t)t, x, B, len, s);
        LASTCHK();
        return 0;
    }
    const float* zz = nullptr;
    if (c_sig != 0.f) {
        zz = z;
        if (!zz) {
            launch_philox_normal(seed, sample0, 1u + (uint32_t)t, e->znoise, B, e->L, s);
            zz = e->znoise;
        }
    }
    launch_lincomb(2, x, e->eps, zz, c_eps, c_div, c_sig, x, (long)B * e->L, s);
    LASTCHK();
    return 0;
}

int diffuse(dmad_engine* e, const float* x0, float c_a, float c_b, const float* z, uint64_t seed, uint64_t sample0, int B, float* x_t,
            hipStream_t s, int len) {
    CHK(need_batch(e, B));
    if (len && len != e->L) {
        launch_sched_len(1, x0, nullptr, z, c_a, c_b, 0.f, true, seed, sample0, 0xD1FFu, x_t, B, len, s);
        LASTCHK();
        return 0;
    }
    const float* zz = z;
    if (!zz) {
        launch_philox_normal(seed, sample0, 0xD1FFu, e->znoise, B, e->L, s);
        zz = e->znoise;
    }
    launch_lincomb(1, x0, nullptr, zz, c_a, c_b, 0.f, x_t, (long)B * e->L, s);
    LASTCHK();
    return 0;
}
}  // namespace

extern "C" {

int dmad_ddpm_step(dmad_engine* e, float* x, int32_t t, float c_eps, float c_div, float c_sig, const float* z, uint64_t seed,
                   uint64_t sample0, int32_t B, dmad_stream s) {
    if (!e || !x) return fail(DMAD_ERR_INVALID, "null argument");
    return ddpm_step(e, x, t, c_eps, c_div, c_sig, z, seed, sample0, B, (hipStream_t)s, wave_path(e), 0);
}

int dmad_ddpm_step_len(dmad_engine* e, float* x, int32_t t, float c_eps, float c_div, float c_sig, const float* z, uint64_t seed,
                       uint64_t sample0, int32_t B, int32_t len, dmad_stream s) {
    if (!e) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(need_len(e, "dmad_ddpm_step_len", len));
    if (!x) return fail(DMAD_ERR_INVALID, "null argument");
    return ddpm_step(e, x, t, c_eps, c_div, c_sig, z, seed, sample0, B, (hipStream_t)s, PATH_FP32, len);
}

int dmad_diffuse_len(dmad_engine* e, const float* x0, float c_a, float c_b, const float* z, uint64_t seed, uint64_t sample0, int32_t B,
                     int32_t len, float* x_t, dmad_stream s) {
    if (!e) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(need_len(e, "dmad_diffuse_len", len));
    if (!x0 || !x_t) return fail(DMAD_ERR_INVALID, "null argument");
    return diffuse(e, x0, c_a, c_b, z, seed, sample0, B, x_t, (hipStream_t)s, len);
}

int dmad_ddpm_purify_len(dmad_engine* e, const float* x0, int32_t t_star, float c_a, float c_b, const float* c_eps, const float* c_div,
                         const float* c_sig, uint64_t seed, uint64_t sample0, int32_t B, int32_t len, float* out, dmad_stream s) {
    if (!e) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(need_len(e, "dmad_ddpm_purify_len", len));
    if (!x0 || !out || !c_eps || !c_div || !c_sig) return fail(DMAD_ERR_INVALID, "null argument");
    if (t_star < 1) return fail(DMAD_ERR_INVALID, "t_star %d < 1", t_star);
    CHK(dmad_diffuse_len(e, x0, c_a, c_b, nullptr, seed, sample0, B, len, out, s));
    for (int t = t_star - 1; t >= 0; --t)
        CHK(dmad_ddpm_step_len(e, out, t, c_eps[t], c_div[t], t > 0 ? c_sig[t] : 0.f, nullptr, seed, sample0, B, len, s));
    return 0;
}

int dmad_wavenet_eps_len(dmad_engine* e, const float* x_t, int32_t t, int32_t B, int32_t len, float* eps, dmad_stream s) {
    if (!e) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(need_len(e, "dmad_wavenet_eps_len", len));
    if (!x_t || !eps) return fail(DMAD_ERR_INVALID, "null argument");
    return wavenet_eps(e, x_t, t, B, eps, (hipStream_t)s, PATH_FP32, nullptr, len);
}

int dmad_wavenet_eps_vjp_len(dmad_engine* e, const float* x_t, int32_t t, int32_t B, int32_t len, const float* g_eps, float* g_x, float* eps,
                             dmad_stream s) {
    if (!e) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(need_len(e, "dmad_wavenet_eps_vjp_len", len));
    if (!x_t || !g_eps || !g_x) return fail(DMAD_ERR_INVALID, "null argument");
    return wavenet_vjp(e, x_t, t, B, g_eps, g_x, eps, (hipStream_t)s, len);
}

int dmad_philox_normal_len(dmad_engine* e, uint64_t seed, uint64_t sample0, uint32_t stream, int32_t B, int32_t len, float* z, dmad_stream s) {
    if (!e) return fail(DMAD_ERR_INVALID, "bad argument");
    CHK(need_len(e, "dmad_philox_normal_len", len));
    if (!z || B < 1) return fail(DMAD_ERR_INVALID, "bad argument");
    if (len == e->L) launch_philox_normal(seed, sample0, stream, z, B, e->L, (hipStream_t)s);
    else launch_philox_normal_len(seed, sample0, stream, z, B, len, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_diffuse(dmad_engine* e, const float* x0, float c_a, float c_b, const float* z, uint64_t seed, uint64_t sample0,
                 int32_t B, float* x_t, dmad_stream s) {
    if (!e || !x0 || !x_t) return fail(DMAD_ERR_INVALID, "null argument");
    return diffuse(e, x0, c_a, c_b, z, seed, sample0, B, x_t, (hipStream_t)s, 0);
}

int dmad_unet_eps(dmad_engine* e, const float* x_t, int32_t t, int32_t B, float* eps, dmad_stream s) {
    if (!e || !x_t || !eps) return fail(DMAD_ERR_INVALID, "null argument");
    return unet_eps(e, x_t, t, B, eps, (hipStream_t)s);
}

int dmad_unet_eps_tier(dmad_engine* e, const float* x_t, int32_t t, int32_t B, int32_t tier, float* eps, dmad_stream s) {
    if (!e || !x_t || !eps) return fail(DMAD_ERR_INVALID, "null argument");
    if (tier != 0 && tier != 1 && tier != 2) return fail(DMAD_ERR_INVALID, "unknown UNet tier %d (0 exact fp32, 1 16-bit, 2 split-f16)", tier);
    return unet_eps(e, x_t, t, B, eps, (hipStream_t)s, tier);
}

int dmad_unet_p_sample(dmad_engine* e, float* x, int32_t t, float c_a, float c_b, float c_1, float c_2, float c_sig, const float* z,
                       uint64_t seed, uint64_t sample0, int32_t B, float* x0_out, dmad_stream s) {
    if (!e || !x) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(unet_eps(e, x, t, B, e->un_eps, (hipStream_t)s));
    const float* zz = nullptr;
    if (c_sig != 0.f) {
        zz = z;
        if (!zz) {
            launch_philox_normal(seed, sample0, 0x0E70u + (uint32_t)t, e->znoise, B, 1024, (hipStream_t)s);
            zz = e->znoise;
        }
    }
    launch_unet_p_sample(x, e->un_eps, zz, c_a, c_b, c_1, c_2, c_sig, x, x0_out, (long)B * 1024, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_ddpm_purify(dmad_engine* e, const float* x0, int32_t t_star, float c_a, float c_b, const float* c_eps, const float* c_div,
                     const float* c_sig, uint64_t seed, uint64_t sample0, int32_t B, float* out, dmad_stream s) {
    if (!e || !x0 || !out || !c_eps || !c_div || !c_sig) return fail(DMAD_ERR_INVALID, "null argument");
    if (t_star < 1) return fail(DMAD_ERR_INVALID, "t_star %d < 1", t_star);
    CHK(dmad_diffuse(e, x0, c_a, c_b, nullptr, seed, sample0, B, out, s));
    for (int t = t_star - 1; t >= 0; --t)
        CHK(dmad_ddpm_step(e, out, t, c_eps[t], c_div[t], t > 0 ? c_sig[t] : 0.f, nullptr, seed, sample0, B, s));
    return 0;
}

}  // extern "C"

namespace {

// The reverse VP-SDE chain of dmad_vpsde_purify and dmad_spec_vpsde_purify on rows of `width` floats, in passes of up to max_batch
// rows: the diffusion draw (Philox stream stream_diffuse), then per Euler step n eps_fn(x, k, bb) -- the domain's eps-network into
// `eps` -- and the update (stream stream_step0 + n).  z / traj hold n_steps + 1 slots of B rows: slot 0 the diffusion, n + 1 step n.
template <class Eps>
int vpsde_chain(dmad_engine* e, int width, uint32_t stream_diffuse, uint32_t stream_step0, const float* eps, Eps eps_fn, const float* x0,
                int B, int n_steps, float c_a, float c_b, const int32_t* k, const float* h, const float* hb, const float* q, const float* gs,
                const float* z, uint64_t seed, uint64_t sample0, float* out, float* traj, hipStream_t st) {
    const size_t L = width, slot = (size_t)B * L;
    for (int b0 = 0; b0 < B; b0 += e->maxB) {                  // a pass: the whole chain for up to max_batch rows
        const int bb = B - b0 < e->maxB ? B - b0 : e->maxB;
        float* x = out + b0 * L;
        const uint64_t s0 = sample0 + (uint64_t)b0;
        launch_vpsde_step(x0 + b0 * L, nullptr, z ? z + b0 * L : nullptr, c_a, c_b, 0.f, 0.f, seed, s0, stream_diffuse, x,
                          traj ? traj + b0 * L : nullptr, bb, width, st);
        for (int n = 0; n < n_steps; ++n) {
            CHK(eps_fn(x, k[n], bb));
            launch_vpsde_step(x, eps, z ? z + (n + 1) * slot + b0 * L : nullptr, hb[n], q[n], h[n], gs[n], seed, s0,
                              stream_step0 + (uint32_t)n, x, traj ? traj + (n + 1) * slot + b0 * L : nullptr, bb, width, st);
        }
    }
    LASTCHK();
    return 0;
}

// The reverse walk over the trajectory of vpsde_chain, in passes of the domain's VJP reservation (per_pass rows; g2 is its two
// gradient buffers): vjp_fn(x, k, bb, g, dst, alpha, gamma) is one affine VJP pass of the eps-network, dst = alpha g - gamma J^T g.
template <class Vjp>
int vpsde_chain_vjp(int width, int per_pass, float* g2, Vjp vjp_fn, const float* traj, int B, int n_steps, float c_a, const int32_t* k,
                    const float* h, const float* hb, const float* q, const float* g_out, float* g_x0) {
    const size_t L = width, slot = (size_t)B * L;
    for (int b0 = 0; b0 < B; b0 += per_pass) {                 // a pass of the reservation: the whole reverse walk
        const int bb = B - b0 < per_pass ? B - b0 : per_pass;
        const float* g = g_out + b0 * L;
        for (int n = n_steps - 1; n >= 0; --n) {
            // g <- (1 + h hb) g - (h q) J_n^T g, J_n = d eps / d x at traj[n]; the last step (n = 0) folds in d x_0 / d x0 = c_a
            double alpha = 1.0 + (double)h[n] * (double)hb[n], gamma = (double)h[n] * (double)q[n];
            if (n == 0) { alpha *= c_a; gamma *= c_a; }
            float* dst = n == 0 ? g_x0 + b0 * L : g2 + (size_t)((n_steps - 1 - n) & 1) * per_pass * L;
            CHK(vjp_fn(traj + n * slot + b0 * L, k[n], bb, g, dst, (float)alpha, (float)gamma));
            g = dst;
        }
    }
    return 0;
}

}  // namespace

extern "C" {

int dmad_vpsde_purify(dmad_engine* e, const float* x0, int32_t B, int32_t n_steps, float c_a, float c_b, const int32_t* k, const float* h,
                      const float* hb, const float* q, const float* gs, const float* z, uint64_t seed, uint64_t sample0, int32_t path, float* out,
                      float* traj, dmad_stream s) {
    if (!e || !x0 || !out || !k || !h || !hb || !q || !gs) return fail(DMAD_ERR_INVALID, "null argument");
    if (n_steps < 1) return fail(DMAD_ERR_INVALID, "n_steps %d < 1", n_steps);
    if (B < 1) return fail(DMAD_ERR_INVALID, "batch %d < 1", B);
    if (path != 0 && path != 1) return fail(DMAD_ERR_INVALID, "unknown path %d (0 the mode's default, 1 exact fp32)", path);
    if (path == 1 && !e->f32) return fail(DMAD_ERR_STATE, "path 1 is the exact-fp32 path: a DMAD_BF16 engine holds no fp32 weights");
    CHK(need_wavenet(e));
    for (int n = 0; n < n_steps; ++n)
        if (k[n] < 0) return fail(DMAD_ERR_INVALID, "step %d: k = %d < 0", n, k[n]);
    const int wp = path == 1 ? PATH_FP32 : wave_path(e);
    const hipStream_t st = (hipStream_t)s;
    auto eps = [=](const float* x, int kn, int bb) { return wavenet_eps(e, x, kn, bb, e->eps, st, wp); };
    return vpsde_chain(e, e->L, kVpsdeStreamDiffuse, kVpsdeStreamStep0, e->eps, eps, x0, B, n_steps, c_a, c_b, k, h, hb, q, gs, z, seed,
                       sample0, out, traj, st);
}

int dmad_vpsde_purify_vjp(dmad_engine* e, const float* traj, int32_t B, int32_t n_steps, float c_a, const int32_t* k, const float* h,
                          const float* hb, const float* q, const float* g_out, float* g_x0, dmad_stream s) {
    if (!e || !traj || !k || !h || !hb || !q || !g_out || !g_x0) return fail(DMAD_ERR_INVALID, "null argument");
    if (g_out == g_x0) return fail(DMAD_ERR_INVALID, "g_out and g_x0 must not alias");
    if (n_steps < 1) return fail(DMAD_ERR_INVALID, "n_steps %d < 1", n_steps);
    if (!e->f32) return fail(DMAD_ERR_STATE, "the WaveNet VJP runs on the exact-fp32 path: a DMAD_BF16 engine holds no fp32 weights");
    CHK(need_wavenet(e));
    if (!e->vjpB) return fail(DMAD_ERR_STATE, "no VJP workspace: call dmad_reserve_vjp first");
    CHK(need_batch(e, B));
    for (int n = 0; n < n_steps; ++n)
        if (k[n] < 0) return fail(DMAD_ERR_INVALID, "step %d: k = %d < 0", n, k[n]);
    auto vjp = [=](const float* x, int kn, int bb, const float* g, float* dst, float alpha, float gamma) {
        return wavenet_vjp_pass(e, x, kn, bb, g, dst, e->eps, (hipStream_t)s, true, alpha, gamma);
    };
    return vpsde_chain_vjp(e->L, e->vjpB, e->vjp_g2, vjp, traj, B, n_steps, c_a, k, h, hb, q, g_out, g_x0);
}

int dmad_spec_vpsde_purify(dmad_engine* e, const float* x0, int32_t B, int32_t n_steps, float c_a, float c_b, const int32_t* k, const float* h,
                           const float* hb, const float* q, const float* gs, const float* z, uint64_t seed, uint64_t sample0, int32_t path,
                           float* out, float* traj, dmad_stream s) {
    if (!e || !x0 || !out || !k || !h || !hb || !q || !gs) return fail(DMAD_ERR_INVALID, "null argument");
    if (n_steps < 1) return fail(DMAD_ERR_INVALID, "n_steps %d < 1", n_steps);
    if (B < 1) return fail(DMAD_ERR_INVALID, "batch %d < 1", B);
    if (path != 0 && path != 1) return fail(DMAD_ERR_INVALID, "unknown path %d (0 the mode's UNet map tier, 1 exact fp32)", path);
    if (path == 1 && !e->f32) return fail(DMAD_ERR_STATE, "path 1 is the exact-fp32 UNet tier: a DMAD_BF16 engine holds no fp32 weights");
    CHK(need_unet(e));
    for (int n = 0; n < n_steps; ++n)
        if (k[n] < 0 || k[n] > kUnSsSteps) return fail(DMAD_ERR_INVALID, "step %d: k = %d outside [0, %d]", n, k[n], kUnSsSteps);
    const int tier = path == 1 ? 0 : -1;
    const hipStream_t st = (hipStream_t)s;
    auto eps = [=](const float* x, int kn, int bb) { return unet_eps(e, x, kn, bb, e->un_eps, st, tier); };
    return vpsde_chain(e, 1024, kSpecVpsdeStreamDiffuse, kSpecVpsdeStreamStep0, e->un_eps, eps, x0, B, n_steps, c_a, c_b, k, h, hb, q, gs, z,
                       seed, sample0, out, traj, st);
}

int dmad_spec_vpsde_purify_vjp(dmad_engine* e, const float* traj, int32_t B, int32_t n_steps, float c_a, const int32_t* k, const float* h,
                               const float* hb, const float* q, const float* g_out, float* g_x0, dmad_stream s) {
    if (!e || !traj || !k || !h || !hb || !q || !g_out || !g_x0) return fail(DMAD_ERR_INVALID, "null argument");
    if (g_out == g_x0) return fail(DMAD_ERR_INVALID, "g_out and g_x0 must not alias");
    if (n_steps < 1) return fail(DMAD_ERR_INVALID, "n_steps %d < 1", n_steps);
    if (!e->f32) return fail(DMAD_ERR_STATE, "the UNet VJP runs on the exact-fp32 UNet tier: it needs a DMAD_FP32 or DMAD_EXACT engine");
    CHK(need_unet(e));
    if (!e->unvjpB) return fail(DMAD_ERR_STATE, "no UNet VJP workspace: call dmad_reserve_unet_vjp first");
    CHK(need_batch(e, B));
    for (int n = 0; n < n_steps; ++n)
        if (k[n] < 0 || k[n] > kUnSsSteps) return fail(DMAD_ERR_INVALID, "step %d: k = %d outside [0, %d]", n, k[n], kUnSsSteps);
    auto vjp = [=](const float* x, int kn, int bb, const float* g, float* dst, float alpha, float gamma) {
        return unet_vjp_pass(e, x, kn, bb, g, dst, e->un_eps, (hipStream_t)s, true, alpha, gamma);
    };
    return vpsde_chain_vjp(1024, e->unvjpB, e->unvjp_g2, vjp, traj, B, n_steps, c_a, k, h, hb, q, g_out, g_x0);
}

int dmad_mel_db(dmad_engine* e, const float* x, int32_t B, float* spec, dmad_stream s) {
    if (!e || !x || !spec) return fail(DMAD_ERR_INVALID, "null argument");
    return mel_db(e, x, B, spec, (hipStream_t)s);
}

int dmad_mel_power(dmad_engine* e, const float* x, int32_t B, float* mel, dmad_stream s) {
    if (!e || !x || !mel) return fail(DMAD_ERR_INVALID, "null argument");
    return mel_db(e, x, B, mel, (hipStream_t)s, 0);
}

int dmad_power_to_db(dmad_engine* e, const float* x, int64_t n, float* y, dmad_stream s) {
    if (!e || !x || !y || n < 0) return fail(DMAD_ERR_INVALID, "bad argument");
    if (n) launch_power_to_db(x, y, (long)n, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_classify(dmad_engine* e, const float* spec, int32_t B, float* logits, dmad_stream s) {
    if (!e || !spec || !logits) return fail(DMAD_ERR_INVALID, "null argument");
    return classify(e, spec, B, logits, (hipStream_t)s);
}

int dmad_classify_tier(dmad_engine* e, const float* spec, int32_t B, int32_t tier, float* logits, dmad_stream s) {
    if (!e || !spec || !logits) return fail(DMAD_ERR_INVALID, "null argument");
    if (tier != 0 && tier != 1 && tier != 2) return fail(DMAD_ERR_INVALID, "unknown classifier tier %d (0 fp32, 1 16-bit, 2 split-f16)", tier);
    return classify(e, spec, B, logits, (hipStream_t)s, tier);
}

int dmad_conv_h16(const uint16_t* x, const uint16_t* x2, int32_t ksplit, const uint16_t* w, const float* bias, const uint16_t* res16,
                  int32_t B, int32_t H, int32_t M, int32_t K, int32_t taps, int32_t stride, int32_t groups, int32_t relu,
                  float* out32, uint16_t* out16, dmad_stream s) {
    if (!x || !w || (!out32 && !out16)) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || H < 1 || M < 1 || K < 1 || groups < 1 || (stride != 1 && stride != 2)) return fail(DMAD_ERR_INVALID, "bad geometry");
    CHK(need_kernels(KF_GEMM_H16));
    const int Ho = (H - 1) / stride + 1;
    GemmH16Args g{};
    g.A = w; g.X = x; g.C = out32; g.C16 = out16; g.shift = bias; g.res16 = res16; g.M = M; g.K = K; g.taps = taps; g.ldc = groups * M;
    g.N = (long)B * Ho * Ho; g.H = H; g.W = H; g.ldx = x2 ? ksplit : groups * K; g.stride = stride; g.relu = relu; g.groups = groups;
    if (x2) { g.X2 = x2; g.ksplit = ksplit; g.ldx2 = K - ksplit; }
    launch_gemm_h16(g, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_conv_h16_up2(const uint16_t* x_half, const uint16_t* w, const float* bias, const uint16_t* res16, int32_t B, int32_t H, int32_t M, int32_t K,
                      float* out32, uint16_t* out16, float* stats, dmad_stream s) {
    if (!x_half || !w || (!out32 && !out16)) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || H < 2 || (H & 1) || M < 1 || K < 1) return fail(DMAD_ERR_INVALID, "bad geometry");
    CHK(need_kernels(KF_GEMM_H16));
    GemmH16Args g{};
    g.A = w; g.X = x_half; g.C = out32; g.C16 = out16; g.shift = bias; g.res16 = res16; g.M = M; g.K = K; g.taps = 9; g.ldc = M;
    g.N = (long)B * H * H; g.H = H; g.W = H; g.ldx = K; g.stride = 1; g.up2 = 1;
    if (stats) { g.stats = stats; g.stats_px = 64; }
    if (!gemm_h16_fuses_up2(g)) return fail(DMAD_ERR_STATE, "this shape is not served by the form that fuses the upsampling (the caller materialises the x2 map)");
    launch_gemm_h16(g, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_split_f16(const float* x, int64_t n, float* y, dmad_stream s) {
    if (!x || !y || n < 0 || (n & 3)) return fail(DMAD_ERR_INVALID, "bad argument (n must be a multiple of 4)");
    if (n) launch_scale(x, 1.f, y, (long)n, (hipStream_t)s, true);
    LASTCHK();
    return 0;
}

int dmad_conv_x3(const float* x, const float* x2, int32_t ksplit, const float* w, const float* bias, const float* res, int32_t B, int32_t H,
                 int32_t M, int32_t K, int32_t taps, int32_t stride, int32_t groups, int32_t relu, int32_t out_split, int32_t res_split, float* out,
                 dmad_stream s) {
    if (!x || !w || !out) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || H < 1 || M < 1 || K < 1 || groups < 1 || (stride != 1 && stride != 2) || (groups > 1 && x2)) return fail(DMAD_ERR_INVALID, "bad geometry");
    CHK(need_kernels(KF_GEMM_X3));
    GemmF32Args g = nhwc_conv_args(w, nullptr, bias, x, out, M, K, taps, B, H, stride, res, relu, groups, x2 ? ksplit : groups * K, groups * M);
    g.x3 = 1; g.out_split = out_split; g.res_split = res_split;
    if (x2) { g.X2 = x2; g.ksplit = ksplit; g.ldx2 = K - ksplit; }
    launch_gemm_f32(g, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_conv_h16_stats(const uint16_t* x, const uint16_t* w, const float* bias, const uint16_t* res16, int32_t B, int32_t H, int32_t M, int32_t K,
                        int32_t taps, int32_t stride, uint16_t* out16, float* stats, dmad_stream s) {
    if (!x || !w || !out16 || !stats) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || H < 1 || M < 1 || K < 1 || (stride != 1 && stride != 2)) return fail(DMAD_ERR_INVALID, "bad geometry");
    CHK(need_kernels(KF_GEMM_H16));
    const int Ho = (H - 1) / stride + 1;
    if (Ho * Ho != 16 && (Ho * Ho) % 64) return fail(DMAD_ERR_INVALID, "statistics blocks need maps of 16 or a multiple of 64 pixels");
    GemmH16Args g{};
    g.A = w; g.X = x; g.C16 = out16; g.shift = bias; g.res16 = res16; g.M = M; g.K = K; g.taps = taps; g.ldc = M;
    g.N = (long)B * Ho * Ho; g.H = H; g.W = H; g.ldx = K; g.stride = stride; g.stats = stats; g.stats_px = Ho * Ho >= 64 ? 64 : 16;
    launch_gemm_h16(g, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_groupnorm16_apply(const uint16_t* x, const float* st, const uint16_t* x2, const float* st2, int32_t c1, const float* gamma,
                           const float* beta, const float* ss, int32_t silu, int32_t B, int32_t HW, int32_t C, uint16_t* y16, float* y32,
                           dmad_stream s) {
    if (!x || !st || !gamma || !beta || (!y16 && !y32)) return fail(DMAD_ERR_INVALID, "null argument");
    if (launch_groupnorm16_apply(x, st, x2, st2, c1, gamma, beta, ss, silu, y16, y32, B, HW, C, (hipStream_t)s))
        return fail(DMAD_ERR_INVALID, "no one-pass GroupNorm for a %d-pixel x %d-channel map", HW, C);
    LASTCHK();
    return 0;
}

int dmad_qkv_attention_h16(const uint16_t* qkv16, int32_t B, int32_t T, int32_t heads, uint16_t* out16, dmad_stream s) {
    if (!qkv16 || !out16) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || B > 65535 || heads < 1) return fail(DMAD_ERR_INVALID, "bad geometry");
    if (int rc = launch_qkv_attention_h16(qkv16, out16, B, T, heads, (hipStream_t)s))
        return fail(rc > 0 ? DMAD_ERR_HIP : DMAD_ERR_INVALID, "f16 attention (T = %d): %s", T, rc > 0 ? hipGetErrorString((hipError_t)rc) : "unsupported map size");
    LASTCHK();
    return 0;
}

int dmad_groupnorm16(const uint16_t* x16, const uint16_t* x2_16, int32_t c1, const float* gamma, const float* beta, const float* ss,
                     int32_t silu, int32_t B, int32_t HW, int32_t C, uint16_t* y16, float* y32, dmad_stream s) {
    if (!x16 || !gamma || !beta || (!y16 == !y32)) return fail(DMAD_ERR_INVALID, "null argument (exactly one of y16 / y32)");
    if (launch_groupnorm_nhwc(nullptr, gamma, beta, ss, silu, y32, B, HW, C, (hipStream_t)s, nullptr, x2_16 ? c1 : 0, y16, x16, x2_16))
        return fail(DMAD_ERR_INVALID, "no two-pass f16 GroupNorm for a %d-pixel x %d-channel map (c1 = %d)", HW, C, c1);
    LASTCHK();
    return 0;
}

int dmad_conv1ch_3x3(const float* in, const float* w, const float* bias, int32_t B, int32_t Cout, float* out32, uint16_t* out16, float* stats,
                     dmad_stream s) {
    if (!in || !w || !bias || (!out32 && !out16)) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || Cout < 1) return fail(DMAD_ERR_INVALID, "bad geometry");
    if (launch_conv1ch_3x3(in, w, bias, out32, B, Cout, (hipStream_t)s, out16, stats))
        return fail(DMAD_ERR_INVALID, "no 1-channel 3x3 conv for %d output channels%s", Cout, stats ? " with statistics (Cout <= 128, a multiple of 4)" : " (Cout <= 128)");
    LASTCHK();
    return 0;
}

int dmad_conv3x3_c128_to1(const float* in, const float* w, const float* bias, int32_t B, const float* g_in, float alpha, float gamma,
                          float* out, dmad_stream s) {
    if (!in || !w || !bias || !out) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || g_in == out) return fail(DMAD_ERR_INVALID, "bad geometry (g_in and out are two buffers)");
    launch_conv3x3_c128_to1(in, w, bias, out, B, (hipStream_t)s, g_in, alpha, gamma);
    LASTCHK();
    return 0;
}

int dmad_conv3x3_c128_to1_h16(const uint16_t* in16, const float* w, const float* bias, int32_t B, float* out, dmad_stream s) {
    if (!in16 || !w || !bias || !out) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "bad geometry");
    launch_conv3x3_c128_to1_h16(in16, w, bias, out, B, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_upsample2x(const void* in, int32_t B, int32_t H, int32_t C, int32_t is_f16, void* out, dmad_stream s) {
    if (!in || !out || in == out) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || H < 1 || C < 1 || (C % (is_f16 ? 8 : 4))) return fail(DMAD_ERR_INVALID, "bad geometry (C a multiple of %d)", is_f16 ? 8 : 4);
    if (is_f16) launch_upsample2x_nhwc_h16((const h16_t*)in, (h16_t*)out, B, H, H, C, (hipStream_t)s);
    else launch_upsample2x_nhwc((const float*)in, (float*)out, B, H, H, C, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_conv_f32(const float* x, const float* x2, int32_t ksplit, const float* w, const float* scale, const float* shift, const float* res,
                  int32_t B, int32_t H, int32_t M, int32_t K, int32_t taps, int32_t stride, int32_t groups, int32_t relu, float* slab,
                  int64_t slab_floats, int64_t n_ref, float* out, int32_t* choice, dmad_stream s) {
    if (!x || !w || !out) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || H < 0 || M < 1 || K < 16 || (K % 16) || groups < 1 || groups > 65535 || (stride != 1 && stride != 2) || (taps != 1 && taps != 9))
        return fail(DMAD_ERR_INVALID, "bad geometry (K a multiple of 16, taps 1 or 9, stride 1 or 2)");
    if (H == 0 && (taps != 1 || stride != 1 || groups != 1 || x2)) return fail(DMAD_ERR_INVALID, "the row form (H = 0) is a plain GEMM: one tap, one group, one input");
    if (x2 && groups > 1) return fail(DMAD_ERR_INVALID, "two-part input serves dense convs only");
    if (slab_floats < 0 || n_ref < 0 || (slab && slab_floats < 1)) return fail(DMAD_ERR_INVALID, "bad split-K workspace");
    CHK(need_kernels(KF_GEMM_F32));
    GemmF32Args g{};
    if (H == 0) {
        g = plain_gemm(w, x, out, scale, shift, M, K, B, M, K, relu);
        g.res = res;
    } else {
        g = nhwc_conv_args(w, scale, shift, x, out, M, K, taps, B, H, stride, res, relu, groups, x2 ? ksplit : groups * K, groups * M);
        if (x2) { g.X2 = x2; g.ksplit = ksplit; g.ldx2 = K - ksplit; }
    }
    if (launch_gemm_f32(g, (hipStream_t)s, slab, (long)slab_floats, (long)n_ref) != 0) {
        gemm_take_bad_shapes();
        return fail(DMAD_ERR_INVALID, "no fp32 GEMM serves this shape");
    }
    if (choice) { const GemmF32Choice c = gemm_f32_last_choice(); choice[0] = c.bm; choice[1] = c.narrow; choice[2] = c.two; choice[3] = c.splits; }
    LASTCHK();
    return 0;
}

int dmad_conv_f32_vjp(const float* g_y, const float* w, const float* scale, const float* mask_y, const float* acc, int32_t B, int32_t H,
                      int32_t M, int32_t K, int32_t taps, int32_t stride, int32_t groups, int32_t form, int32_t ldt, float* wT, float* gm,
                      float* work, float* g_x, dmad_stream s) {
    if (!g_y || !w || !wT || !g_x) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || H < 1 || M < 16 || K < 4 || (M % 16) || (K % 4) || (stride != 1 && stride != 2) || (taps != 1 && taps != 9) || form < 0 || form > 4)
        return fail(DMAD_ERR_INVALID, "bad geometry (M a multiple of 16, K of 4, taps 1 or 9, stride 1 or 2, form 0 - 4)");
    if (stride == 2 && (H & 1)) return fail(DMAD_ERR_INVALID, "a stride-2 gradient is dilated to an even map: H = %d", H);
    if ((stride == 2 || form == 1) && !work) return fail(DMAD_ERR_INVALID, "this form needs the work map");
    CHK(need_kernels(KF_GEMM_F32));
    const hipStream_t st = (hipStream_t)s;
    const int Ho = form == 1 ? 2 * H : (H - 1) / stride + 1;
    if (form == 4) {                             // WideResNet's form: a dense 3x3 / 1x1 at stride 1 or 2, scale optional
        if (groups != 1 || ldt || (taps == 1 && stride == 2 && acc))
            return fail(DMAD_ERR_INVALID, "WideResNet's form: dense, no padded pitch, no acc with the stride-2 1x1");
        const float* g = g_y;
        if (mask_y) {
            if (!gm) return fail(DMAD_ERR_INVALID, "the ReLU mask needs its output map");
            launch_relu_mask(g_y, mask_y, gm, (long)B * Ho * Ho * M, st);
            g = gm;
        }
        if (taps == 9) launch_cvjp_pack_dense(w, scale, wT, M, K, st);
        else launch_cvjp_transpose(w, M, K, K, scale, wT, M, st);
        CHK(rx_conv_dgrad(wT, g, g_x, K, M, taps, 1, B, Ho, stride, work, acc, st));
    } else if (form == 3) {                      // VGG19_bn's form
        if (taps != 9 || stride != 1 || groups != 1 || !scale || ldt || acc || (K % 16))
            return fail(DMAD_ERR_INVALID, "VGG19_bn's form: a dense 3x3 with stride 1, a scale, K a multiple of 16, no acc and no padded pitch");
        const float* g = g_y;
        if (mask_y) {
            if (!gm) return fail(DMAD_ERR_INVALID, "the ReLU mask needs its output map");
            launch_relu_mask(g_y, mask_y, gm, (long)B * H * H * M, st);
            g = gm;
        }
        launch_cvjp_pack_dense(w, scale, wT, M, K, st);
        CHK(vgg_conv_dgrad(wT, g, g_x, M, K, B, H, nullptr, 0, 0, st));
    } else if (form < 2) {                       // the UNet's forms
        if (groups != 1 || scale || mask_y || gm || ldt || (form == 1 && (taps != 9 || stride != 1)))
            return fail(DMAD_ERR_INVALID, "the UNet's forms are dense, unscaled and unmasked (Upsample: 3x3, stride 1)");
        un_pack_wT(w, wT, taps, K, M, st);
        CHK(un_conv_dgrad(wT, g_y, g_x, K, M, taps, B, H, stride, form == 1, acc, work, st));
    } else {                                     // ResNeXt29's forms
        if (taps == 1 ? (groups != 1 || (ldt && (ldt < M || (ldt % 16))) || (stride == 2 && acc)) : (groups != 8 || M != K || ldt || !scale))
            return fail(DMAD_ERR_INVALID, "ResNeXt29's forms: a dense 1x1 (ldt 0 or a multiple of 16 >= M; no acc with stride 2) or the 8-group 3x3 with M = K and a scale");
        const int kp = taps == 1 && ldt ? ldt : M;                       // the gradient's channel pitch (padded with the image's rows)
        const float* g = g_y;
        if (mask_y) {
            const long n = (long)B * Ho * Ho * groups * kp;
            if (!gm || kp != M || (n & 3)) return fail(DMAD_ERR_INVALID, "the ReLU mask needs its output map, an unpadded gradient and a multiple of 4 values");
            launch_relu_mask(g_y, mask_y, gm, n, st);
            g = gm;
        }
        rx_pack_wT(w, scale, wT, M, K, taps, kp, st);
        CHK(rx_conv_dgrad(wT, g, g_x, K, kp, taps, groups, B, Ho, stride, work, acc, st));
    }
    LASTCHK();
    return 0;
}

int dmad_groupnorm_f32(const float* x, const float* x2, int32_t c1, const float* gamma, const float* beta, const float* ss, int32_t silu,
                       int32_t B, int32_t HW, int32_t C, int32_t split, float* y, dmad_stream s) {
    if (!x || !gamma || !beta || !y) return fail(DMAD_ERR_INVALID, "null argument");
    if (launch_groupnorm_nhwc(x, gamma, beta, ss, silu, y, B, HW, C, (hipStream_t)s, x2, x2 ? c1 : 0, nullptr, nullptr, nullptr, split ? 1 : 0))
        return fail(DMAD_ERR_INVALID, "no fp32 GroupNorm for a %d-pixel x %d-channel map (c1 = %d)", HW, C, c1);
    LASTCHK();
    return 0;
}

int dmad_groupnorm_bwd(const float* x, const float* x2, int32_t c1, const float* gamma, const float* beta, const float* ss, int32_t silu,
                       const float* gy, const float* add, const float* add2, int32_t B, int32_t HW, int32_t C, float* gx, float* gx2,
                       dmad_stream s) {
    if (!x || !gamma || !beta || !gy || !gx) return fail(DMAD_ERR_INVALID, "null argument");
    if (launch_groupnorm_bwd(x, x2, x2 ? c1 : 0, gamma, beta, ss, silu, gy, add, add2, gx, gx2, B, HW, C, (hipStream_t)s))
        return fail(DMAD_ERR_INVALID, "no GroupNorm backward for a %d-pixel x %d-channel map (c1 = %d)", HW, C, c1);
    LASTCHK();
    return 0;
}

int dmad_qkv_attention_f32(const float* qkv, int32_t B, int32_t T, int32_t heads, int32_t split, float* out, dmad_stream s) {
    if (!qkv || !out) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || heads < 1) return fail(DMAD_ERR_INVALID, "bad geometry");
    if (int rc = launch_qkv_attention(qkv, out, B, T, heads, (hipStream_t)s, nullptr, split ? 1 : 0))
        return fail(rc > 0 ? DMAD_ERR_HIP : DMAD_ERR_INVALID, "attention (T = %d): %s", T, rc > 0 ? hipGetErrorString((hipError_t)rc) : "unsupported map size");
    LASTCHK();
    return 0;
}

int dmad_qkv_attention_bwd(const float* qkv, const float* go, int32_t B, int32_t T, int32_t heads, float* gqkv, dmad_stream s) {
    if (!qkv || !go || !gqkv) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || heads < 1) return fail(DMAD_ERR_INVALID, "bad geometry");
    CHK(need_kernels(KF_UNET_ATT_BWD));
    if (int rc = launch_qkv_attention_bwd(qkv, go, gqkv, B, T, heads, (hipStream_t)s))
        return fail(rc > 0 ? DMAD_ERR_HIP : DMAD_ERR_INVALID, "attention backward (T = %d): unsupported map size", T);
    LASTCHK();
    return 0;
}

int dmad_rx_head_bwd(const float* g_logits, const float* W, const float* y, int32_t B, int32_t ncls, int32_t HW, int32_t C, float* gz, dmad_stream s) {
    if (!g_logits || !W || !y || !gz) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || ncls < 1 || HW < 1 || C < 1) return fail(DMAD_ERR_INVALID, "bad geometry");
    launch_rx_head_bwd(g_logits, W, y, gz, B, ncls, HW, C, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_rx_conv1_bwd(const float* g, const float* a, const float* w, const float* scale, int32_t B, float* gspec, dmad_stream s) {
    if (!g || !a || !w || !scale || !gspec) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "bad geometry");
    launch_rx_conv1_bwd(g, a, w, scale, gspec, B, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_vote(dmad_engine* e, const float* logits, int32_t B, int64_t* counts, dmad_stream s) {
    if (!e || !logits || !counts || B < 1) return fail(DMAD_ERR_INVALID, "bad argument to dmad_vote");
    launch_vote(logits, B, e->cfg.num_classes, (unsigned long long*)counts, nullptr, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_set_mode(dmad_engine* e, int32_t mode) {
    if (!e) return fail(DMAD_ERR_INVALID, "null engine");
    if (!(e->bf16 && e->f32)) {
        const int only = e->bf16 ? DMAD_MODE_FAST : DMAD_MODE_FP32;
        if (mode == only) return 0;
        return fail(DMAD_ERR_STATE, "mode %d needs a DMAD_EXACT engine (this one has only its %s path)", mode, e->bf16 ? "bf16" : "fp32");
    }
    if (mode != DMAD_MODE_FAST && mode != DMAD_MODE_EXACT_VOTES && mode != DMAD_MODE_FP32) return fail(DMAD_ERR_INVALID, "unknown mode %d", mode);
    e->mode = mode;
    return 0;
}

int dmad_set_waveform_tier(dmad_engine* e, int32_t tier) {
    if (!e) return fail(DMAD_ERR_INVALID, "null engine");
    if (tier != PATH_DEFAULT && tier != PATH_FP32 && tier != PATH_X3) return fail(DMAD_ERR_INVALID, "unknown waveform tier %d (0 16-bit, 1 fp32, 2 split-f16)", tier);
    if (!(e->bf16 && e->f32)) {
        if (tier == PATH_DEFAULT) return 0;
        return fail(DMAD_ERR_STATE, "waveform tiers need a DMAD_EXACT engine (this one has only its %s path)", e->bf16 ? "16-bit" : "fp32");
    }
    e->wave_tier = tier;
    return 0;
}

int dmad_set_recheck_margin(dmad_engine* e, float tau) { return set_recheck_bound(e, false, 1, tau); }
int dmad_set_recheck_margin2(dmad_engine* e, float tau2) { return set_recheck_bound(e, false, 2, tau2); }
int dmad_set_spec_recheck_margin(dmad_engine* e, float tau) { return set_recheck_bound(e, true, 1, tau); }
int dmad_set_spec_recheck_margin2(dmad_engine* e, float tau2) { return set_recheck_bound(e, true, 2, tau2); }

int dmad_recheck_stats(dmad_engine* e, int64_t* samples, int64_t* rechecked, int64_t* rechecked_fp32, int32_t reset) {
    return read_recheck_stats(e, false, samples, rechecked, rechecked_fp32, reset);
}
int dmad_spec_recheck_stats(dmad_engine* e, int64_t* samples, int64_t* rechecked, int32_t reset) {
    return read_recheck_stats(e, true, samples, rechecked, nullptr, reset);
}
int dmad_spec_recheck_stats2(dmad_engine* e, int64_t* samples, int64_t* rechecked, int64_t* rechecked_fp32, int32_t reset) {
    return read_recheck_stats(e, true, samples, rechecked, rechecked_fp32, reset);
}

int dmad_reserve_vjp(dmad_engine* e, int32_t max_batch) {
    return reserve_vjp(
        e, max_batch, &dmad_engine::maxB32, &dmad_engine::vjpB,
        [&]() -> int {
            if (!e->f32) return fail(DMAD_ERR_STATE, "the WaveNet VJP runs on the exact-fp32 path: a DMAD_BF16 engine holds no fp32 weights");
            return need_wavenet(e);
        },
        [&] { return std::vector<float**>{&e->vjp_save, &e->vjp_gH, &e->vjp_G, &e->vjp_gg, &e->vjp_g2}; },
        [&]() -> int {                      // one kernel packs all three images: it runs again while any of them was missing
            const size_t NL = e->NL;
            const bool missing = !e->vjp_wdilT || !e->vjp_wgT || !e->vjp_wf0T;
            CHK(pack_once(e, &e->vjp_wdilT, NL * 3 * 256 * 512, [] {}));
            CHK(pack_once(e, &e->vjp_wgT, NL * 2 * 256 * 256, [] {}));
            CHK(pack_once(e, &e->vjp_wf0T, 256 * 256, [] {}));
            if (missing) launch_vjp_pack(e->wdil, e->wrs, e->wf0, e->vjp_wdilT, e->vjp_wgT, e->vjp_wf0T, e->NL, nullptr);
            return 0;
        },
        [&](int vB) -> int {
            const size_t LP = e->LP, NL = e->NL;
            // zeroed: the padding rows of the saved streams and of the gradient maps are read as the convs' zero padding and never written
            // (rows a longer clip wrote are cleared before a shorter one reads them: clean_pad)
            CHK(e->alloc(&e->vjp_save, NL * vB * LP * kC, true));
            CHK(e->alloc(&e->vjp_gH, (size_t)vB * LP * 512, true));
            CHK(e->alloc(&e->vjp_G, 3 * (size_t)vB * LP * kC, true));
            CHK(e->alloc(&e->vjp_gg, (size_t)vB * e->L * kC));
            CHK(e->alloc(&e->vjp_g2, 2 * (size_t)vB * e->L));
            e->dirty_save = e->dirty_G = e->dirty_gH = 0;
            return 0;
        });
}

int dmad_wavenet_eps_vjp(dmad_engine* e, const float* x_t, int32_t t, int32_t B, const float* g_eps, float* g_x, float* eps, dmad_stream s) {
    if (!e || !x_t || !g_eps || !g_x) return fail(DMAD_ERR_INVALID, "null argument");
    return wavenet_vjp(e, x_t, t, B, g_eps, g_x, eps, (hipStream_t)s);
}

int dmad_reserve_unet_vjp(dmad_engine* e, int32_t max_batch) {
    return reserve_vjp(
        e, max_batch, &dmad_engine::maxB32, &dmad_engine::unvjpB,
        [&]() -> int {
            CHK(need_unet(e));
            return e->f32 ? 0 : fail(DMAD_ERR_STATE, "the UNet VJP runs on the exact-fp32 UNet tier: it needs a DMAD_FP32 or DMAD_EXACT engine");
        },
        [&] { return std::vector<float**>{&e->unvjp_tape, &e->unvjp_ghs, &e->unvjp_work, &e->unvjp_g2}; },
        [&]() -> int {                      // transposed weight images, packed on the device from the resident fp32 images
            if (!e->unvjp_zero) CHK(e->alloc(&e->unvjp_zero, kUnMC, true));
            for (auto& o : e->un_ops) {
                const long ci = o.cin, co = o.cout;
                if (o.kind == 0) {          // [co][9] -> [9][co], taps flipped (the 128 -> 1 conv's image)
                    CHK(pack_once(e, &o.w1T, 9 * co, [&] { launch_unvjp_pack(o.w1, o.w1T, 9, (int)co, 1, 1, 9, 0, 1, nullptr); }));
                } else if (o.kind == 2) {   // qkv [3C][C] -> [C][3C], proj_out [C][C] -> transposed
                    CHK(pack_once(e, &o.w1T, 3 * ci * ci, [&] { un_pack_wT(o.w1, o.w1T, 1, ci, 3 * ci, nullptr); }));
                    CHK(pack_once(e, &o.w2T, ci * ci, [&] { un_pack_wT(o.w2, o.w2T, 1, ci, ci, nullptr); }));
                } else {                    // 3x3 [tap][co][ci] -> [8 - tap][ci][co]
                    CHK(pack_once(e, &o.w1T, 9 * ci * co, [&] { un_pack_wT(o.w1, o.w1T, 9, ci, co, nullptr); }));
                    if (o.kind == 1) CHK(pack_once(e, &o.w2T, 9 * co * co, [&] { un_pack_wT(o.w2, o.w2T, 9, co, co, nullptr); }));
                    if (o.kind == 1 && ci != co) CHK(pack_once(e, &o.skwT, ci * co, [&] { un_pack_wT(o.skw, o.skwT, 1, ci, co, nullptr); }));
                }
            }
            CHK(pack_once(e, &e->un_outT, 9 * kUnMC, [&] { launch_unvjp_pack(e->un_outw, e->un_outT, kUnMC, 9, 1, 1, kUnMC, 0, 2, nullptr); }));   // [9][128] -> [128][9], flipped
            HIPCHK(hipGetLastError());
            return need_kernels(KF_UNET_ATT_BWD);
        },
        [&](int vB) -> int {
            // tape slots and saved-map gradients, in floats per spectrogram
            std::vector<size_t> out_off, t2_off, qkv_off, ghs_off;
            size_t tape = 0, ghs = 0;
            for (const auto& o : e->un_ops) {
                const size_t px = (size_t)o.H * o.H, opx = o.kind == 3 ? px / 4 : o.kind == 4 ? px * 4 : px;
                t2_off.push_back(o.kind == 1 ? tape : SIZE_MAX); if (o.kind == 1) tape += px * o.cout;
                qkv_off.push_back(o.kind == 2 ? tape : SIZE_MAX); if (o.kind == 2) tape += px * 3 * o.cin;
                out_off.push_back(tape); tape += opx * o.cout;
            }
            for (size_t i = 0; i < e->un_hs_ch.size(); ++i) { ghs_off.push_back(ghs); ghs += (size_t)e->un_hs_hw[i] * e->un_hs_ch[i]; }
            CHK(e->alloc(&e->unvjp_tape, (size_t)vB * tape));
            CHK(e->alloc(&e->unvjp_ghs, (size_t)vB * ghs));
            CHK(e->alloc(&e->unvjp_work, 6 * (size_t)vB * 1024 * 384));
            CHK(e->alloc(&e->unvjp_g2, 2 * (size_t)vB * 1024));
            auto at = [&](size_t off) { return off == SIZE_MAX ? nullptr : e->unvjp_tape + off * vB; };
            e->un_tape = dmad_engine::UnTape{};
            for (size_t k = 0; k < out_off.size(); ++k) {
                e->un_tape.out.push_back(at(out_off[k])); e->un_tape.t2.push_back(at(t2_off[k])); e->un_tape.qkv.push_back(at(qkv_off[k]));
                if (e->un_ops[k].save >= 0) e->un_tape.hs.push_back(e->un_tape.out[k]);
            }
            e->unvjp_ghs_at.clear();
            for (size_t off : ghs_off) e->unvjp_ghs_at.push_back(e->unvjp_ghs + off * vB);
            return 0;
        });
}

int dmad_unet_eps_vjp(dmad_engine* e, const float* x_t, int32_t t, int32_t B, const float* g_eps, float* g_x, float* eps, dmad_stream s) {
    if (!e || !x_t || !g_eps || !g_x) return fail(DMAD_ERR_INVALID, "null argument");
    return unet_vjp(e, x_t, t, B, g_eps, g_x, eps, (hipStream_t)s);
}

int dmad_reserve_classifier_vjp(dmad_engine* e, int32_t max_batch) {
    // transposed images with the BN scale folded in, packed on the device from the fp32 images: reduce [D][cin] -> [cin][D], the grouped 3x3
    // [g][tap][m][k] -> [g][8 - tap][k][m], expand [cout][D] -> [D][cout], the shortcut [cout][cin] -> [cin][cout]
    return reserve_cls_vjp(e, max_batch, 1, std::accumulate(std::begin(kRxWork), std::end(kRxWork), (size_t)0), [&]() -> int {
        for (dmad_engine::RxBlock& b : e->rx) {
            const int G = b.D / 8;
            CHK(pack_once(e, &b.reduce.wT, (size_t)b.cin * b.D, [&] { rx_pack_wT(b.reduce.w, b.reduce.scale, b.reduce.wT, b.D, b.cin, 1, b.D, nullptr); }));
            CHK(pack_once(e, &b.conv.wT, (size_t)8 * 9 * G * G, [&] { rx_pack_wT(b.conv.w, b.conv.scale, b.conv.wT, G, G, 9, 0, nullptr); }));
            CHK(pack_once(e, &b.expand.wT, (size_t)b.D * b.cout, [&] { rx_pack_wT(b.expand.w, b.expand.scale, b.expand.wT, b.cout, b.D, 1, b.cout, nullptr); }));
            if (b.has_short)
                CHK(pack_once(e, &b.shortc.wT, (size_t)b.cin * b.cout, [&] { rx_pack_wT(b.shortc.w, b.shortc.scale, b.shortc.wT, b.cout, b.cin, 1, b.cout, nullptr); }));
        }
        return 0;
    });
}

int dmad_classify_vjp(dmad_engine* e, const float* spec, int32_t B, const float* g_logits, float* g_spec, float* logits, dmad_stream s) {
    return cls_vjp(e, 1, spec, B, g_logits, g_spec, logits, (hipStream_t)s);
}

int dmad_reserve_vgg_vjp(dmad_engine* e, int32_t max_batch) {
    return reserve_cls_vjp(e, max_batch, 0, 2 * kVggWork, [&]() -> int {
        int cin = 64, li = 1;
        for (int i = 1; i < kVggCfgLen; ++i) {
            const int v = kVggCfg[i];
            if (v < 0) continue;
            // [tap][v][cin] -> [8 - tap][cin][v] * scale[v]
            CHK(pack_once(e, &e->vconvwT[li], (size_t)9 * cin * v, [&] { launch_cvjp_pack_dense(e->vconvw[li], e->vscale[li], e->vconvwT[li], v, cin, nullptr); }));
            cin = v;
            ++li;
        }
        // classifier.3 [4096][4096] -> transposed, classifier.0 [4096][512] -> [512][4096]
        CHK(pack_once(e, &e->vfcwT[1], (size_t)4096 * 4096, [&] { launch_cvjp_transpose(e->vfcw[1], 4096, 4096, 4096, nullptr, e->vfcwT[1], 4096, nullptr); }));
        CHK(pack_once(e, &e->vfcwT[0], (size_t)512 * 4096, [&] { launch_cvjp_transpose(e->vfcw[0], 4096, 512, 512, nullptr, e->vfcwT[0], 4096, nullptr); }));
        return 0;
    });
}

int dmad_vgg_vjp(dmad_engine* e, const float* spec, int32_t B, const float* g_logits, float* g_spec, float* logits, dmad_stream s) {
    return cls_vjp(e, 0, spec, B, g_logits, g_spec, logits, (hipStream_t)s);
}

int dmad_vgg_vjp_tape(dmad_engine* e, int32_t index, int32_t B, float* out, dmad_stream s) { return cls_vjp_tape(e, 0, index, B, out, (hipStream_t)s); }

int dmad_vgg_pool_relu_bwd(const float* g, const float* y, int32_t B, int32_t H, int32_t C, float* gpre, dmad_stream s) {
    if (!g || !y || !gpre) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || H < 2 || (H & 1) || C < 4 || (C & 3)) return fail(DMAD_ERR_INVALID, "bad geometry (H even, C a multiple of 4)");
    launch_vgg_pool_relu_bwd(g, y, gpre, B, H, C, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_reserve_wrn_vjp(dmad_engine* e, int32_t max_batch) {
    // the 3x3 convs tap-flipped and transposed (conv1's with bn2's scale folded in, conv2's plain), the 1x1 shortcuts [cout][cin] -> [cin][cout]
    return reserve_cls_vjp(e, max_batch, 2, std::accumulate(std::begin(kWrnWork), std::end(kWrnWork), (size_t)0), [&]() -> int {
        for (dmad_engine::WrnBlock& b : e->wrn) {
            CHK(pack_once(e, &b.w1T, (size_t)9 * b.cin * b.cout, [&] { launch_cvjp_pack_dense(b.w1, b.s2, b.w1T, b.cout, b.cin, nullptr); }));
            CHK(pack_once(e, &b.w2T, (size_t)9 * b.cout * b.cout, [&] { launch_cvjp_pack_dense(b.w2, nullptr, b.w2T, b.cout, b.cout, nullptr); }));
            if (b.ws) CHK(pack_once(e, &b.wsT, (size_t)b.cin * b.cout, [&] { launch_cvjp_transpose(b.ws, b.cout, b.cin, b.cin, nullptr, b.wsT, b.cout, nullptr); }));
        }
        return 0;
    });
}

int dmad_wrn_vjp(dmad_engine* e, const float* spec, int32_t B, const float* g_logits, float* g_spec, float* logits, dmad_stream s) {
    return cls_vjp(e, 2, spec, B, g_logits, g_spec, logits, (hipStream_t)s);
}

int dmad_wrn_vjp_tape(dmad_engine* e, int32_t index, int32_t B, float* out, dmad_stream s) { return cls_vjp_tape(e, 2, index, B, out, (hipStream_t)s); }

int dmad_wrn_preact(const float* x, const float* scale, const float* shift, int64_t n_px, int32_t C, float* out, dmad_stream s) {
    if (!x || !scale || !shift || !out) return fail(DMAD_ERR_INVALID, "null argument");
    if (n_px < 1 || C < 4 || (C & 3)) return fail(DMAD_ERR_INVALID, "bad geometry (C a multiple of 4)");
    launch_wrn_preact(x, scale, shift, out, (long)n_px, C, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_wrn_preact_bwd(const float* g, const float* o, const float* scale, const float* res, int64_t n_px, int32_t C, float* gx, dmad_stream s) {
    if (!g || !o || !scale || !gx) return fail(DMAD_ERR_INVALID, "null argument");
    if (n_px < 1 || C < 4 || (C & 3)) return fail(DMAD_ERR_INVALID, "bad geometry (C a multiple of 4)");
    launch_wrn_preact_bwd(g, o, scale, res, gx, (long)n_px, C, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_wrn_stem(const float* spec, const float* w, int32_t B, float* out, dmad_stream s) {
    if (!spec || !w || !out) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "bad geometry");
    launch_wrn_stem(spec, w, out, B, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_wrn_stem_bwd(const float* g, const float* w, int32_t B, float* gspec, dmad_stream s) {
    if (!g || !w || !gspec) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "bad geometry");
    launch_wrn_stem_bwd(g, w, gspec, B, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_reserve_dn_vjp(dmad_engine* e, int32_t max_batch) {
    if (!e) return fail(DMAD_ERR_INVALID, "null engine");
    // the backward images are built with the forward's at dmad_finalize_weights: nothing to pack
    return reserve_cls_vjp(e, max_batch, 3, std::accumulate(std::begin(kDnWork), std::end(kDnWork), (size_t)0), [&]() -> int { return 0; });
}

int dmad_dn_vjp(dmad_engine* e, const float* spec, int32_t B, const float* g_logits, float* g_spec, float* logits, dmad_stream s) {
    return cls_vjp(e, 3, spec, B, g_logits, g_spec, logits, (hipStream_t)s);
}

int dmad_dn_vjp_tape(dmad_engine* e, int32_t index, int32_t B, float* out, dmad_stream s) { return dn_vjp_tape(e, index, B, out, (hipStream_t)s); }

// the kernel hooks of densenet.hip: the geometry every access relies on is checked here
int dmad_dn_pw(const float* A, int32_t M, int32_t K, const float* x, int32_t ldx, int64_t n_px, const float* s_in, const float* b_in, const float* s_out,
               const float* b_out, float* out, int32_t ldo, dmad_stream s) {
    if (!A || !x || !s_in || !b_in || !out || (!s_out != !b_out)) return fail(DMAD_ERR_INVALID, "null argument");
    if (n_px < 1 || M < 1 || K < 2 || (K & 1) || (ldx & 1) || ldx < K || ldo < M) return fail(DMAD_ERR_INVALID, "bad geometry (K and the input pitch even, pitches >= widths)");
    launch_dn_pw(dn_pw_fwd(A, M, K, x, ldx, (long)n_px, s_in, b_in, s_out, b_out, out, ldo), false, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_dn_pw_bwd(const float* A, int32_t M, int32_t K, const float* g, int32_t ldg, int64_t n_px, int32_t pool, int32_t H, const float* x, int32_t ldx,
                   const float* s1, const float* b1, float* out, int32_t ldo, int32_t add, dmad_stream s) {
    if (!A || !g || !x || !s1 || !b1 || !out) return fail(DMAD_ERR_INVALID, "null argument");
    if (n_px < 1 || M < 1 || K < 2 || (K & 1) || (ldg & 1) || ldg < K || ldx < M || ldo < M) return fail(DMAD_ERR_INVALID, "bad geometry (K and the gradient's pitch even, pitches >= widths)");
    if (pool && (H < 2 || (H & 1) || n_px % ((int64_t)H * H))) return fail(DMAD_ERR_INVALID, "the pooled form takes whole H x H maps, H even");
    launch_dn_pw(dn_pw_bwd(A, M, K, g, ldg, (long)n_px, pool ? 1 : 0, H, x, ldx, s1, b1, out, ldo, add ? 1 : 0), true, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dn_growth_geometry(int B, int H, int ld, int off) {
    if (B < 1 || (H != 8 && H != 16 && H != 32) || (ld & 1) || (off & 1) || off < 0 || off + 12 > ld)
        return fail(DMAD_ERR_INVALID, "bad geometry (H 8, 16 or 32; pitch and offset even; offset + 12 <= pitch)");
    return 0;
}

int dmad_dn_growth(const float* A, const float* h, int32_t B, int32_t H, float* stream, int32_t ld, int32_t off, dmad_stream s) {
    if (!A || !h || !stream) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(dn_growth_geometry(B, H, ld, off));
    launch_dn_growth(A, h, stream, ld, off, B, H, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_dn_growth_bwd(const float* A, const float* g, int32_t ld, int32_t off, const float* h, const float* s2, int32_t B, int32_t H, float* gh,
                       dmad_stream s) {
    if (!A || !g || !h || !s2 || !gh) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(dn_growth_geometry(B, H, ld, off));
    launch_dn_growth_bwd(A, g, ld, off, h, s2, gh, B, H, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_dn_stem(const float* spec, const float* w, int32_t B, float* stream, int32_t ld, dmad_stream s) {
    if (!spec || !w || !stream) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || ld < 24 || (ld & 3)) return fail(DMAD_ERR_INVALID, "bad geometry (pitch a multiple of 4, >= 24)");
    launch_dn_stem(spec, w, stream, ld, B, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_dn_stem_bwd(const float* g, int32_t ld, const float* w, int32_t B, float* gspec, dmad_stream s) {
    if (!g || !w || !gspec) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || ld < 24 || (ld & 3)) return fail(DMAD_ERR_INVALID, "bad geometry (pitch a multiple of 4, >= 24)");
    launch_dn_stem_bwd(g, ld, w, gspec, B, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_dn_pool(const float* t, int32_t ldt, int32_t B, int32_t H, int32_t C, float* out, int32_t ldo, dmad_stream s) {
    if (!t || !out) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || H < 2 || (H & 1) || C < 1 || ldt < C || ldo < C) return fail(DMAD_ERR_INVALID, "bad geometry (H even, pitches >= C)");
    launch_dn_pool(t, ldt, out, ldo, B, H, C, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_dn_preact(const float* x, int32_t ldx, const float* scale, const float* shift, int64_t n_px, int32_t C, float* out, dmad_stream s) {
    if (!x || !scale || !shift || !out) return fail(DMAD_ERR_INVALID, "null argument");
    if (n_px < 1 || C < 1 || ldx < C) return fail(DMAD_ERR_INVALID, "bad geometry (pitch >= C)");
    launch_dn_preact_map(x, ldx, scale, shift, out, (long)n_px, C, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_dn_head(const float* x, int32_t ldx, const float* bns, const float* bnb, const float* fcw, const float* fcb, int32_t B, int32_t HW, int32_t C,
                 int32_t ncls, float* logits, dmad_stream s) {
    if (!x || !bns || !bnb || !fcw || !fcb || !logits) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || HW < 1 || (HW & (HW - 1)) || C < 1 || C > 384 || ldx < C || ncls < 1) return fail(DMAD_ERR_INVALID, "bad geometry (HW a power of two, C <= 384)");
    launch_dn_head(x, ldx, bns, bnb, fcw, fcb, logits, B, HW, C, ncls, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_dn_head_bwd(const float* g_logits, const float* fcws, const float* x, int32_t ldx, const float* bns, const float* bnb, int32_t B, int32_t HW,
                     int32_t C, int32_t ncls, float* g, int32_t ldg, dmad_stream s) {
    if (!g_logits || !fcws || !x || !bns || !bnb || !g) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || HW < 1 || (HW & (HW - 1)) || C < 1 || ldx < C || ldg < C || ncls < 1) return fail(DMAD_ERR_INVALID, "bad geometry (HW a power of two, pitches >= C)");
    launch_dn_head_bwd(g_logits, fcws, x, ldx, bns, bnb, g, ldg, B, HW, C, ncls, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_mel_db_vjp(dmad_engine* e, const float* x, int32_t B, const float* g_spec, float* g_x, float* spec, dmad_stream s) {
    if (!e || !x || !g_spec || !g_x) return fail(DMAD_ERR_INVALID, "null argument");
    return mel_db_vjp(e, x, B, g_spec, g_x, spec, (hipStream_t)s);
}

int dmad_masking_loss_vjp(dmad_engine* e, const float* delta, int32_t B, const float* theta, const float* psd_scale, float* g_delta, float* loss,
                          float* psd, dmad_stream s) {
    if (!e || !delta || !theta || !psd_scale || !g_delta || !loss) return fail(DMAD_ERR_INVALID, "null argument");
    return masking(e, delta, B, theta, psd_scale, g_delta, loss, psd, nullptr, (hipStream_t)s);
}

int dmad_masking_step(dmad_engine* e, const float* x, float* delta, const float* g_net, const float* alpha, float signed_lr, int32_t B,
                      const float* theta, const float* psd_scale, float* loss, dmad_stream s) {
    if (!e || !x || !delta || !g_net || !alpha || !theta || !psd_scale || !loss) return fail(DMAD_ERR_INVALID, "null argument");
    const MaskingStep st{x, delta, g_net, alpha, signed_lr};
    return masking(e, delta, B, theta, psd_scale, nullptr, loss, nullptr, &st, (hipStream_t)s);
}

int dmad_wavenet_eps_path(dmad_engine* e, const float* x_t, int32_t t, int32_t B, int32_t path, float* eps, dmad_stream s) {
    if (!e || !x_t || !eps) return fail(DMAD_ERR_INVALID, "null argument");
    CHK(need_path(e, path));
    return wavenet_eps(e, x_t, t, B, eps, (hipStream_t)s, path);
}

int dmad_debug_rounding(dmad_engine* e, const int32_t masks[5]) {
    if (!e || !masks) return fail(DMAD_ERR_INVALID, "null argument");
    if (!(e->bf16 && e->f32)) return fail(DMAD_ERR_STATE, "dmad_debug_rounding needs a DMAD_EXACT engine (it acts on the split-f16 tier)");
    for (int i = 0; i < 5; ++i) {
        if (masks[i] < 0 || masks[i] > 7) return fail(DMAD_ERR_INVALID, "mask %d = %d outside [0, 7]", i, masks[i]);
        e->diag[i] = masks[i];
    }
    return 0;
}

}  // extern "C"

namespace {

long read_queue_length(dmad_engine* e, hipStream_t st, int* rc) {
    *rc = 0;
    if (hipMemcpyAsync(e->rc_n_host, e->rc_n, sizeof(unsigned long long), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemsetAsync(e->rc_n, 0, sizeof(unsigned long long), st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        *rc = fail(DMAD_ERR_HIP, "reading the recheck queue length failed");
        return 0;
    }
    const long n = (long)*e->rc_n_host;
    if (n > e->rc_cap) *rc = fail(DMAD_ERR_STATE, "recheck queue overflow (%ld > %ld)", n, e->rc_cap);
    return n;
}

enum { TIER_SPLIT = 2, TIER_FP32 = 3 };    // the recheck tiers of vote_loop

// The vote loop of dmad_smooth_votes and dmad_spec_smooth_votes.  first(done, B, &lg) runs samples sample0 + done .. + B on the
// loop's first pass and points lg at their logits; with an engine without classifier nothing votes.  Without `recheck` every
// sample votes there.  With it (the exact-vote mode) a sample whose top-2 margin is below rt.tau1 is queued instead, and the queue
// drains at the end, or mid-call when the next batch could overflow it: rows(idx, B, tier) re-runs listed samples from the same
// Philox keys on TIER_SPLIT / TIER_FP32 into e->logits (and scatters the loop's outputs), in chunks of up to `chunk`.  The
// split-f16 tier (`mid` and rt.tau2 >= 0) settles every sample whose margin there is at least rt.tau2; the rest, or every queued
// sample without that tier, goes to the exact-fp32 tier.  A re-run row of the loop's outputs carries the last tier's result.
template <class First, class Rows>
int vote_loop(dmad_engine* e, RecheckTiers& rt, bool recheck, bool mid, int chunk, int64_t n, int batch, uint64_t sample0,
              int64_t* counts, First first, Rows rows, hipStream_t st) {
    const int C = e->cfg.num_classes;
    unsigned long long* cnt = (unsigned long long*)counts;
    // one recheck tier over list[0..nq): tau >= 0 queues the rows whose margin is still below tau in `next`, tau < 0 votes every row
    auto pass = [&](const long long* list, long nq, int tier, float tau, long long* next) -> int {
        for (long done = 0; done < nq; done += chunk) {
            const int B = (int)(nq - done < chunk ? nq - done : chunk);
            const long long* idx = list + done;
            CHK(rows(idx, B, tier));
            if (tau >= 0.f) launch_vote_margin(e->logits, B, C, cnt, tau, 0, idx, next, e->rc_n, e->rc_cap, nullptr, st);
            else launch_vote(e->logits, B, C, cnt, nullptr, st);
        }
        return 0;
    };
    // two stream synchronisations at most: the queue lengths decide the launches
    auto drain = [&]() -> int {
        int rc = 0;
        const long n1 = read_queue_length(e, st, &rc);
        if (rc) return rc;
        rt.rechecked += n1;
        if (n1 == 0) return 0;
        if (mid && rt.tau2 >= 0.f) {
            CHK(pass(e->rc_list, n1, TIER_SPLIT, rt.tau2, e->rc_list2));
            const long n2 = read_queue_length(e, st, &rc);
            if (rc) return rc;
            rt.rechecked_fp32 += n2;
            if (n2) CHK(pass(e->rc_list2, n2, TIER_FP32, -1.f, nullptr));
        } else {
            rt.rechecked_fp32 += n1;
            CHK(pass(e->rc_list, n1, TIER_FP32, -1.f, nullptr));
        }
        return 0;
    };
    // an earlier call that failed between queueing and draining must not leave its indices to this one
    if (recheck) HIPCHK(hipMemsetAsync(e->rc_n, 0, sizeof(unsigned long long), st));
    int64_t queued_from = 0;               // first sample (relative) of the current recheck segment
    for (int64_t done = 0; done < n; done += batch) {
        const int B = (int)((n - done < batch) ? (n - done) : batch);
        const float* lg = nullptr;
        CHK(first(done, B, &lg));
        if (!e->cfg.with_classifier) continue;
        if (recheck) {
            launch_vote_margin(lg, B, C, cnt, rt.tau1, (long long)(sample0 + (uint64_t)done), nullptr, e->rc_list, e->rc_n, e->rc_cap, nullptr, st);
            // the queue holds at most rc_cap indices: drain it before the samples voted since the last drain could overflow it
            if (done + B - queued_from + batch > e->rc_cap && done + B < n) {
                CHK(drain());
                queued_from = done + B;
            }
        } else {
            launch_vote(lg, B, C, cnt, nullptr, st);
        }
    }
    if (recheck && n > 0) CHK(drain());
    if (e->cfg.with_classifier) rt.samples += n;
    LASTCHK();
    return 0;
}

struct WaveJob {
    const float* clip; const float* delta; float sigma, scale; int t; float c_a, c_b; uint64_t seed, sample0;
    float* x0_out;                         // listed rows' x0 is also scattered here (dmad_smooth_votes' recheck)
};
// One batch of the waveform chain: noise -> WaveNet on `path` -> x0 (into x0_dst) -> mel dB -> logits (into logits_dst; nullptr:
// none).  Rows are samples s0 + b, or idx[b] when an index list is given.  The classifier tier: the mode's on the default path (a
// vote loop's first pass), the one paired with the WaveNet tier on an explicit path.
int wave_rows(dmad_engine* e, const WaveJob& j, uint64_t s0, const long long* idx, int B, int path, float* x0_dst, float* logits_dst,
              hipStream_t st) {
    const int L = e->L;
    if (idx) launch_mc_noise_scale_idx(j.clip, j.delta, j.sigma, j.scale, j.seed, j.sample0, idx, e->xt, B, L, st);
    else launch_mc_noise_scale(j.clip, j.delta ? j.delta + (s0 - j.sample0) * L : nullptr, j.sigma, j.scale, j.seed, s0, e->xt, B, L, st);
    CHK(wavenet_eps(e, e->xt, j.t, B, e->eps, st, path));
    launch_lincomb(0, e->xt, e->eps, nullptr, j.c_a, j.c_b, 0.f, x0_dst, (long)B * L, st);
    if (idx && j.x0_out) launch_scatter_rows(x0_dst, idx, (long long)j.sample0, j.x0_out, B, L, st);
    if (!logits_dst) return 0;
    CHK(mel_db(e, x0_dst, B, e->spec, st));
    return classify(e, e->spec, B, logits_dst, st, path == PATH_DEFAULT ? cls_tier(e) : cls_tier_of_path(e, path));
}

}  // namespace

extern "C" {

int dmad_eval_samples(dmad_engine* e, const float* clip, float sigma, float sqrt_alpha_bar_star, int32_t t, float c_a, float c_b,
                      uint64_t seed, uint64_t sample0, const float* delta, const int64_t* idx, int64_t n, int32_t path, float* logits_out,
                      float* x0_out, dmad_stream s) {
    if (!e || !clip || !idx || (!logits_out && !x0_out)) return fail(DMAD_ERR_INVALID, "null argument");
    if (n < 0) return fail(DMAD_ERR_INVALID, "n < 0");
    CHK(need_path(e, path));
    if (logits_out) { CHK(need_with_classifier(e)); CHK(need_vote_bound(e)); }
    const WaveJob job{clip, delta, sigma, sqrt_alpha_bar_star, t, c_a, c_b, seed, sample0, nullptr};
    CHK(for_passes(n, path == PATH_DEFAULT ? e->maxB : e->maxB32, [&](int64_t done, int B) {
        return wave_rows(e, job, 0, (const long long*)idx + done, B, path, x0_out ? x0_out + done * e->L : e->x0,
                         logits_out ? logits_out + done * e->cfg.num_classes : nullptr, (hipStream_t)s);
    }));
    LASTCHK();
    return 0;
}

int dmad_smooth_votes(dmad_engine* e, const float* clip, float sigma, float sqrt_alpha_bar_star, int32_t t, float c_a,
                      float c_b, int64_t n, int32_t batch, uint64_t seed, uint64_t sample0, const float* delta, int64_t* counts,
                      float* logits_out, float* x0_out, dmad_stream s) {
    if (!e || !clip) return fail(DMAD_ERR_INVALID, "null argument");
    if (n < 0 || batch < 1 || batch > e->maxB) return fail(DMAD_ERR_STATE, "batch %d outside [1, max_batch=%d] or n < 0", batch, e->maxB);
    if (e->cfg.with_classifier && !counts) return fail(DMAD_ERR_INVALID, "counts must not be null");
    CHK(need_vote_bound(e));
    hipStream_t st = (hipStream_t)s;
    const int L = e->L, C = e->cfg.num_classes;
    const WaveJob job{clip, delta, sigma, sqrt_alpha_bar_star, t, c_a, c_b, seed, sample0, x0_out};
    // exact-vote mode: the queued samples re-run on the split-f16 WaveNet (~fp32 accuracy at several times the fp32 matrix rate),
    // those still inside tau2 there on the exact-fp32 WaveNet
    const bool recheck = e->bf16 && e->f32 && e->mode == DMAD_MODE_EXACT_VOTES && e->cfg.with_classifier;
    auto first = [&](int64_t done, int B, const float** lg) -> int {
        float* out = logits_out ? logits_out + done * C : e->logits;
        *lg = out;
        return wave_rows(e, job, sample0 + (uint64_t)done, nullptr, B, PATH_DEFAULT, x0_out ? x0_out + done * L : e->x0,
                         e->cfg.with_classifier ? out : nullptr, st);
    };
    auto rows = [&](const long long* idx, int B, int tier) -> int {
        CHK(wave_rows(e, job, 0, idx, B, tier == TIER_SPLIT ? PATH_X3 : PATH_FP32, e->x0, e->logits, st));
        if (logits_out) launch_scatter_rows(e->logits, idx, (long long)sample0, logits_out, B, C, st);
        return 0;
    };
    return vote_loop(e, e->wave_rt, recheck, e->wdil_x3 != nullptr, e->maxB32, n, batch, sample0, counts, first, rows, st);
}

int dmad_rs_smooth_votes(dmad_engine* e, const float* clip, float sigma, int64_t n, int32_t batch, uint64_t seed, uint64_t sample0,
                         const float* delta, int64_t* counts, float* logits_out, dmad_stream s) {
    if (!e || !clip) return fail(DMAD_ERR_INVALID, "dmad_rs_smooth_votes: null argument");
    if (!counts) return fail(DMAD_ERR_INVALID, "dmad_rs_smooth_votes: counts must not be null");
    if (n < 0) return fail(DMAD_ERR_INVALID, "dmad_rs_smooth_votes: n < 0");
    CHK(need_classifier(e));
    CHK(need_batch(e, batch));
    if (((uintptr_t)clip | (uintptr_t)delta) & 15)
        return fail(DMAD_ERR_INVALID, "dmad_rs_smooth_votes: clip and delta must be 16-byte aligned (they are read as float4)");
    hipStream_t st = (hipStream_t)s;
    const int L = e->L, C = e->cfg.num_classes;
    // the noisy rows go straight into the mel front-end's padded layout; the classifier runs its fp32 tier whatever the engine's
    // precision and mode (dmad_classify's tier), so every sample votes in the first pass and no recheck bound is involved
    auto first = [&](int64_t done, int B, const float** lg) -> int {
        float* out = logits_out ? logits_out + done * C : e->logits;
        *lg = out;
        launch_mel_pad_noise(clip, delta ? delta + done * L : nullptr, sigma, seed, sample0 + (uint64_t)done, e->mel_xp, B, L, e->LPm, st);
        CHK(mel_db_padded(e, B, e->spec, st));
        return classify(e, e->spec, B, out, st);
    };
    auto rows = [](const long long*, int, int) -> int { return 0; };       // never called: nothing is queued without a recheck
    RecheckTiers none;                                                     // ... and the exact-vote statistics are not this loop's
    return vote_loop(e, none, false, false, e->maxB, n, batch, sample0, counts, first, rows, st);
}

}  // extern "C"

namespace {

struct SpecJob {
    const float* clip; float sigma; int t_star; float q_a, q_b; const float *c_a, *c_b, *c_1, *c_2, *c_sig; float mel_lo, mel_hi;
    uint64_t seed;
};
// One batch of the spec-domain chain (include/dmad.h, dmad_spec_smooth_votes): rows are samples s0 + b, or idx[b] when an index
// list is given (the recheck pass).  h16: -1 the mode's UNet tier, 0 exact fp32, 1 the 16-bit tier.  The purified dB spectrograms
// land in sp, the logits in lg.
// the chain behind its noisy waveforms: e->xt [B][L] -> purified dB spectrograms sp, logits lg.  cls16: the classifier tier (vote loops' first
// pass: the 16-bit tier where one is resident; every other caller: fp32)
int spec_chain_from_xt(dmad_engine* e, const SpecJob& j, uint64_t s0, const long long* idx, int B, int h16, int cls16, float* sp, float* lg, hipStream_t st) {
    CHK(mel_db(e, e->xt, B, e->spec, st));
    launch_philox_normal(j.seed, s0, 0x5BECu, e->znoise, B, 1024, st, idx);
    float* x = e->x0;                                                                   // [B][32][32] chain state
    launch_spec_diffuse(e->spec, e->znoise, j.mel_lo, j.mel_hi, j.q_a, j.q_b, x, (long)B * 1024, st);
    for (int t = j.t_star; t >= 0; --t) {
        CHK(unet_eps(e, x, t, B, e->un_eps, st, h16));
        const float sig = t > 0 ? j.c_sig[t] : 0.f;
        if (sig != 0.f) launch_philox_normal(j.seed, s0, 0x0E70u + (uint32_t)t, e->znoise, B, 1024, st, idx);
        launch_unet_p_sample(x, e->un_eps, sig != 0.f ? e->znoise : nullptr, j.c_a[t], j.c_b[t], j.c_1[t], j.c_2[t], sig, x, nullptr, (long)B * 1024, st);
    }
    launch_spec_unstandardize(x, j.mel_lo, j.mel_hi, sp, (long)B * 1024, st);
    CHK(classify(e, sp, B, lg, st, cls16));
    return 0;
}

int spec_chain(dmad_engine* e, const SpecJob& j, uint64_t s0, const long long* idx, int B, int h16, float* sp, float* lg, hipStream_t st) {
    const int L = e->L;
    if (idx) launch_mc_noise_scale_idx(j.clip, nullptr, j.sigma, 1.f, j.seed, 0, idx, e->xt, B, L, st);
    else launch_mc_noise_scale(j.clip, nullptr, j.sigma, 1.f, j.seed, s0, e->xt, B, L, st);      // no wave denoiser: no sqrt(alpha_bar*) scale
    return spec_chain_from_xt(e, j, s0, idx, B, h16, h16 == 1 ? cls_tier(e) : 0, sp, lg, st);      // the recheck tiers: the fp32 classifier
}

// The loop of the three query exports over the B * repeats query rows (row r = clip r % B, AcousticSystem's repeat layout), in passes of
// up to max_batch rows: the rows into e->xt, logits_of(nb, r0, lg) -- the export's defense and classifier -- and the optional decisions
template <class Logits>
int query_loop(dmad_engine* e, const float* x, int B, int repeats, float* logits, int32_t* decisions, hipStream_t st, Logits logits_of,
               int row_width = 0) {
    const int C = row_width ? row_width : e->cfg.num_classes;      // the M5 exports: n_output log-probabilities per row
    CHK(for_passes((int64_t)B * repeats, e->maxB, [&](int64_t r0, int nb) -> int {
        launch_repeat_rows(x, e->xt, B, (long)r0, nb, e->L, st);
        CHK(logits_of(nb, r0, logits + r0 * C));
        if (decisions) launch_vote(logits + r0 * C, nb, C, nullptr, decisions + r0, st);
        return 0;
    }));
    LASTCHK();
    return 0;
}

// purified waveforms -> mel dB -> the fp32 classifier, like AcousticSystem.forward's own call
int wave_logits(dmad_engine* e, const float* pur, int nb, float* lg, hipStream_t st) {
    CHK(mel_db(e, pur, nb, e->spec, st));
    return classify(e, e->spec, nb, lg, st);
}

// the purifier of dmad_query_logits / dmad_m5_query_logits on the nb rows of e->xt (rows r0 ...): where the purified rows are
int run_query_sampler(dmad_engine* e, int sampler, int t_star, float c_a, float c_b, const float* c_eps, const float* c_div, const float* c_sig,
                      uint64_t seed, uint64_t sample0, int64_t r0, int nb, hipStream_t st, const float** pur) {
    *pur = e->xt;
    if (sampler == 1) {
        CHK(dmad_ddpm_purify(e, e->xt, t_star, c_a, c_b, c_eps, c_div, c_sig, seed, sample0 + (uint64_t)r0, nb, e->x0, (dmad_stream)st));
        *pur = e->x0;
    } else if (sampler == 2) {
        CHK(wavenet_eps(e, e->xt, t_star - 1, nb, e->eps, st, wave_path(e)));
        launch_lincomb(0, e->xt, e->eps, nullptr, c_a, c_b, 0.f, e->x0, (long)nb * e->L, st);
        *pur = e->x0;
    }
    return 0;
}

int query_args(const void* e, const void* x, const void* logits, int B, int repeats, int sampler, int t_star, const float* c_eps,
               const float* c_div, const float* c_sig) {
    if (!e || !x || !logits) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || repeats < 1) return fail(DMAD_ERR_INVALID, "B and repeats must be >= 1");
    if (sampler < 0 || sampler > 2) return fail(DMAD_ERR_INVALID, "unknown sampler %d (0 none, 1 DDPM, 2 one-shot)", sampler);
    if (sampler && t_star < 1) return fail(DMAD_ERR_INVALID, "t_star %d < 1", t_star);
    if (sampler == 1 && (!c_eps || !c_div || !c_sig)) return fail(DMAD_ERR_INVALID, "the DDPM sampler needs its coefficient arrays");
    return 0;
}

}  // namespace

extern "C" {

int dmad_spec_smooth_votes(dmad_engine* e, const float* clip, float sigma, int32_t t_star, float q_a, float q_b, const float* c_a,
                           const float* c_b, const float* c_1, const float* c_2, const float* c_sig, float mel_lo, float mel_hi, int64_t n,
                           int32_t batch, uint64_t seed, uint64_t sample0, int64_t* counts, float* logits_out, float* spec_out, dmad_stream s) {
    if (!e || !clip || !counts || !c_a || !c_b || !c_1 || !c_2 || !c_sig) return fail(DMAD_ERR_INVALID, "null argument");
    if (!e->cfg.with_classifier || !e->cls_final) return fail(DMAD_ERR_STATE, "the spec-domain vote loop needs the mel front-end and a finalised classifier");
    CHK(need_vote_bound(e));
    CHK(need_unet(e));
    if (n < 0 || batch < 1 || batch > e->maxB) return fail(DMAD_ERR_STATE, "batch %d outside [1, max_batch=%d] or n < 0", batch, e->maxB);
    if (t_star < 0) return fail(DMAD_ERR_INVALID, "t_star %d < 0", t_star);
    if (!(mel_hi > mel_lo)) return fail(DMAD_ERR_INVALID, "empty mel range");
    hipStream_t st = (hipStream_t)s;
    const int C = e->cfg.num_classes;
    const SpecJob job{clip, sigma, t_star, q_a, q_b, c_a, c_b, c_1, c_2, c_sig, mel_lo, mel_hi, seed};
    // exact-vote mode of a DMAD_EXACT engine: the chain runs on the UNet's 16-bit tier; a queued sample re-runs its WHOLE chain from
    // the same Philox keys on the UNet's split-f16 tier (fp32-grade at several times the fp32 matrix rate), and on the exact-fp32
    // UNet if its margin there is still inside tau2
    const bool recheck = e->bf16 && e->f32 && e->un_h16 && e->mode == DMAD_MODE_EXACT_VOTES;
    auto first = [&](int64_t done, int B, const float** lg) -> int {
        float* out = logits_out ? logits_out + done * C : e->logits;
        *lg = out;
        return spec_chain(e, job, sample0 + (uint64_t)done, nullptr, B, (e->un_h16 && e->mode != DMAD_MODE_FP32) ? 1 : 0,
                          spec_out ? spec_out + done * 1024 : e->spec, out, st);
    };
    auto rows = [&](const long long* idx, int B, int tier) -> int {
        CHK(spec_chain(e, job, 0, idx, B, tier == TIER_SPLIT ? 2 : 0, e->spec, e->logits, st));
        if (spec_out) launch_scatter_rows(e->spec, idx, (long long)sample0, spec_out, B, 1024, st);
        if (logits_out) launch_scatter_rows(e->logits, idx, (long long)sample0, logits_out, B, C, st);
        return 0;
    };
    return vote_loop(e, e->spec_rt, recheck, e->un_x3, e->maxB, n, batch, sample0, counts, first, rows, st);
}

int dmad_spec_eval_samples(dmad_engine* e, const float* clip, float sigma, int32_t t_star, float q_a, float q_b, const float* c_a,
                           const float* c_b, const float* c_1, const float* c_2, const float* c_sig, float mel_lo, float mel_hi, uint64_t seed,
                           const int64_t* idx, int64_t n, int32_t tier, float* logits_out, float* spec_out, dmad_stream s) {
    if (!e || !clip || !idx || !c_a || !c_b || !c_1 || !c_2 || !c_sig || (!logits_out && !spec_out)) return fail(DMAD_ERR_INVALID, "null argument");
    if (!e->cfg.with_classifier || !e->cls_final) return fail(DMAD_ERR_STATE, "the spec-domain chain needs the mel front-end and a finalised classifier");
    CHK(need_vote_bound(e));
    CHK(need_unet(e));
    if (n < 0 || t_star < 0 || !(mel_hi > mel_lo)) return fail(DMAD_ERR_INVALID, "bad argument");
    if (tier != 0 && tier != 1 && tier != 2) return fail(DMAD_ERR_INVALID, "unknown UNet tier %d (0 exact fp32, 1 16-bit, 2 split-f16)", tier);
    if (tier == 1 && !e->un_h16) return fail(DMAD_ERR_STATE, "this engine has no 16-bit UNet tier (DMAD_FP32 precision)");
    if (tier == 2 && !e->un_x3) return fail(DMAD_ERR_STATE, "this engine has no split-f16 UNet tier (it needs DMAD_EXACT precision)");
    hipStream_t st = (hipStream_t)s;
    const int C = e->cfg.num_classes;
    const SpecJob job{clip, sigma, t_star, q_a, q_b, c_a, c_b, c_1, c_2, c_sig, mel_lo, mel_hi, seed};
    CHK(for_passes(n, e->maxB, [&](int64_t done, int B) {
        return spec_chain(e, job, 0, (const long long*)idx + done, B, tier, spec_out ? spec_out + done * 1024 : e->spec,
                          logits_out ? logits_out + done * C : e->logits, st);
    }));
    LASTCHK();
    return 0;
}

int dmad_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, int32_t sampler, int32_t t_star, float c_a, float c_b,
                      const float* c_eps, const float* c_div, const float* c_sig, uint64_t seed, uint64_t sample0, float* logits,
                      int32_t* decisions, dmad_stream s) {
    CHK(query_args(e, x, logits, B, repeats, sampler, t_star, c_eps, c_div, c_sig));
    CHK(need_with_classifier(e));
    hipStream_t st = (hipStream_t)s;
    return query_loop(e, x, B, repeats, logits, decisions, st, [&](int nb, int64_t r0, float* lg) -> int {
        const float* pur;
        CHK(run_query_sampler(e, sampler, t_star, c_a, c_b, c_eps, c_div, c_sig, seed, sample0, r0, nb, st, &pur));
        return wave_logits(e, pur, nb, lg, st);
    });
}

int dmad_spec_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, int32_t t_star, float q_a, float q_b, const float* c_a,
                           const float* c_b, const float* c_1, const float* c_2, const float* c_sig, float mel_lo, float mel_hi, uint64_t seed,
                           uint64_t sample0, float* logits, int32_t* decisions, dmad_stream s) {
    if (!e || !x || !logits || !c_a || !c_b || !c_1 || !c_2 || !c_sig) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || repeats < 1) return fail(DMAD_ERR_INVALID, "B and repeats must be >= 1");
    if (!e->cfg.with_classifier || !e->cls_final) return fail(DMAD_ERR_STATE, "the spec-domain query needs the mel front-end and a finalised classifier");
    CHK(need_unet(e));
    if (t_star < 0 || !(mel_hi > mel_lo)) return fail(DMAD_ERR_INVALID, "bad argument");
    hipStream_t st = (hipStream_t)s;
    const SpecJob job{nullptr, 0.f, t_star, q_a, q_b, c_a, c_b, c_1, c_2, c_sig, mel_lo, mel_hi, seed};
    return query_loop(e, x, B, repeats, logits, decisions, st, [&](int nb, int64_t r0, float* lg) {
        // the UNet tier of the map-returning surfaces (unet_eps, h16 = -1: on an exact-vote engine the dmad_set_waveform_tier tier, split-f16
        // by default), the fp32 classifier: like dmad_query_logits, a query hands logits back and has no recheck
        return spec_chain_from_xt(e, job, sample0 + (uint64_t)r0, nullptr, nb, -1, 0, e->spec, lg, st);
    });
}

// _NES.py:19-25 (noise = cat(noise, -noise), the zero probe in front, eval_input = noise * sigma + x), a chunk of rows at a time
int dmad_nes_probes(dmad_engine* e, const float* x, int32_t B, int32_t P, float sigma, int32_t with_origin, uint64_t seed, uint64_t draw0,
                    int64_t row0, int32_t rows, float* out, dmad_stream s) {
    if (!e || !x || !out) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || P < 2 || (P & 1)) return fail(DMAD_ERR_INVALID, "dmad_nes_probes: B %d must be >= 1 and P %d even and >= 2", B, P);
    if (with_origin != 0 && with_origin != 1) return fail(DMAD_ERR_INVALID, "dmad_nes_probes: with_origin must be 0 or 1");
    const int64_t total = (int64_t)B * (P + with_origin);
    if (row0 < 0 || rows < 1 || row0 + rows > total)
        return fail(DMAD_ERR_INVALID, "dmad_nes_probes: rows [%lld, %lld) are not inside the %lld query rows of %d clips", (long long)row0,
                    (long long)row0 + rows, (long long)total, B);
    launch_nes_probes(x, sigma, P / 2, with_origin, seed, draw0, DMAD_PHILOX_STREAM_NES, (long)row0, rows, out, e->L, (hipStream_t)s);
    LASTCHK();
    return 0;
}

// _NES.py:47,52,54 (grad = sum over draw batches of torch.mean(loss * noise, 1), / sigma / num_batches) without the noise tensor
int dmad_nes_grad(dmad_engine* e, const float* w, int32_t B, int32_t P, float scale, uint64_t seed, uint64_t draw0, int32_t accumulate,
                  float* grad, dmad_stream s) {
    if (!e || !w || !grad) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || P < 2 || (P & 1)) return fail(DMAD_ERR_INVALID, "dmad_nes_grad: B %d must be >= 1 and P %d even and >= 2", B, P);
    launch_nes_grad(w, P / 2, scale, seed, draw0, DMAD_PHILOX_STREAM_NES, accumulate != 0, grad, B, e->L, (hipStream_t)s);
    LASTCHK();
    return 0;
}

// the uniform twin of dmad_philox_normal: the draws of the swarm kernels below, for tests
int dmad_philox_uniform(dmad_engine* e, uint64_t seed, uint64_t sample0, uint32_t stream, int32_t B, float* out, dmad_stream s) {
    if (!e || !out || B < 1) return fail(DMAD_ERR_INVALID, "bad argument");
    launch_philox_uniform(seed, sample0, stream, out, B, e->L, (hipStream_t)s);
    LASTCHK();
    return 0;
}

// black_box_attack.py:371-391 (np.random.uniform positions and velocities, the carried best in front) and l.404 (the query rows)
int dmad_pso_init(dmad_engine* e, const float* x, const float* lower, const float* upper, int32_t B, int32_t P, const float* keep,
                  uint64_t seed, uint64_t draw0, float* pbest_loc, float* loc, float* vel, float* queries, dmad_stream s) {
    if (!e || !x || !lower || !upper || !pbest_loc || !loc || !vel || !queries) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || P < 1) return fail(DMAD_ERR_INVALID, "dmad_pso_init: B %d and P %d must be >= 1", B, P);
    launch_pso_init(x, lower, upper, keep, B, P, seed, draw0, DMAD_PHILOX_STREAM_PSO, pbest_loc, loc, vel, queries, e->L, (hipStream_t)s);
    LASTCHK();
    return 0;
}

// black_box_attack.py:474-484 (r1, r2, the velocity and position update, the clamp) and l.404 in one pass over the swarm
int dmad_pso_step(dmad_engine* e, const float* x, const float* lower, const float* upper, const float* pbest_loc, const float* gbest_loc,
                  int32_t B, int32_t P, float w, float c1, float c2, uint64_t seed, uint64_t draw0, float* loc, float* vel, float* queries,
                  dmad_stream s) {
    if (!e || !x || !lower || !upper || !pbest_loc || !gbest_loc || !loc || !vel || !queries) return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || P < 1) return fail(DMAD_ERR_INVALID, "dmad_pso_step: B %d and P %d must be >= 1", B, P);
    launch_pso_step(x, lower, upper, pbest_loc, gbest_loc, B, P, w, c1, c2, seed, draw0, DMAD_PHILOX_STREAM_PSO, loc, vel, queries, e->L,
                    (hipStream_t)s);
    LASTCHK();
    return 0;
}

// black_box_attack.py:420-437 (the personal and global bests) without the host loops
int dmad_pso_update_best(dmad_engine* e, const float* loss, const int64_t* predict, const float* loc, const int64_t* index, int32_t B,
                         int32_t P, float* pbests, float* pbest_loc, float* gbests, float* gbest_loc, int64_t* gbest_predict, dmad_stream s) {
    if (!e || !loss || !predict || !loc || !pbests || !pbest_loc || !gbests || !gbest_loc || !gbest_predict)
        return fail(DMAD_ERR_INVALID, "null argument");
    if (B < 1 || P < 1) return fail(DMAD_ERR_INVALID, "dmad_pso_update_best: B %d and P %d must be >= 1", B, P);
    launch_pso_update_best(loss, (const long long*)predict, loc, (const long long*)index, B, P, pbests, pbest_loc, gbests, gbest_loc,
                           (long long*)gbest_predict, e->L, (hipStream_t)s);
    LASTCHK();
    return 0;
}

// _KenanFFT.py:68 (torch.fft.rfft) and l.198 (the row maximum of |FFT|): one workgroup per clip
int dmad_wave_rfft(dmad_engine* e, const float* x, int32_t B, float* spec, float* maxmag, dmad_stream s) {
    if (!e || !x || !spec || !maxmag) return fail(DMAD_ERR_INVALID, "dmad_wave_rfft: null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "dmad_wave_rfft: B %d must be >= 1", B);
    CHK(need_wave_fft(e, "dmad_wave_rfft"));
    if (((uintptr_t)x | (uintptr_t)spec) & 7) return fail(DMAD_ERR_INVALID, "dmad_wave_rfft: x and spec must be 8-byte aligned");
    CHK(need_kernels(KF_WAVE_FFT));
    launch_wave_rfft(e->fft_plan, e->fft_tw, x, B, spec, maxmag, (hipStream_t)s);
    LASTCHK();
    return 0;
}

// _KenanFFT.py:72 (the masked assignment) and l.77 (torch.fft.irfft) in one launch
int dmad_wave_irfft_threshold(dmad_engine* e, const float* spec, const float* factor, int32_t B, float* out, int32_t* kept, dmad_stream s) {
    if (!e || !spec || !out || !kept) return fail(DMAD_ERR_INVALID, "dmad_wave_irfft_threshold: null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "dmad_wave_irfft_threshold: B %d must be >= 1", B);
    CHK(need_wave_fft(e, "dmad_wave_irfft_threshold"));
    if (((uintptr_t)spec | (uintptr_t)out) & 7) return fail(DMAD_ERR_INVALID, "dmad_wave_irfft_threshold: spec and out must be 8-byte aligned");
    CHK(need_kernels(KF_WAVE_FFT));
    launch_wave_irfft_threshold(e->fft_plan, e->fft_tw, spec, factor, B, out, kept, (hipStream_t)s);
    LASTCHK();
    return 0;
}

// _KenanFFT.py:233-243 (the per-clip loop of the bisection) without the host loop
int dmad_kenan_update(dmad_engine* e, const int64_t* pred, const int64_t* label, int32_t B, int32_t targeted, const float* perturbed,
                      float* best, float* fmin, float* fmax, float* factor, int32_t* succ, dmad_stream s) {
    if (!e || !pred || !label || !perturbed || !best || !fmin || !fmax || !factor || !succ)
        return fail(DMAD_ERR_INVALID, "dmad_kenan_update: null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "dmad_kenan_update: B %d must be >= 1", B);
    if (targeted != 0 && targeted != 1) return fail(DMAD_ERR_INVALID, "dmad_kenan_update: targeted must be 0 or 1");
    if (((uintptr_t)perturbed | (uintptr_t)best) & 15) return fail(DMAD_ERR_INVALID, "dmad_kenan_update: perturbed and best must be 16-byte aligned");
    launch_kenan_update((const long long*)pred, (const long long*)label, B, e->L, targeted, perturbed, best, fmin, fmax, factor, succ,
                        (hipStream_t)s);
    LASTCHK();
    return 0;
}

// time_defense.py:102-127 (AS: F.conv1d with a 1 / w kernel, zero padding) and l.130-157 (MS: F.pad zeros, unfold, torch.median)
int dmad_wave_smooth(dmad_engine* e, const float* x, int32_t B, int32_t kind, int32_t window, float* y, dmad_stream s) {
    if (!e || !x || !y) return fail(DMAD_ERR_INVALID, "dmad_wave_smooth: null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "dmad_wave_smooth: B %d must be >= 1", B);
    if (const char* m = wave_smooth_check(kind, window)) return fail(DMAD_ERR_INVALID, "dmad_wave_smooth: %s (kind %d, window %d)", m, kind, window);
    launch_wave_smooth(x, B, e->L, kind, window, y, (hipStream_t)s);
    LASTCHK();
    return 0;
}

// the mean is symmetric under zero padding: its VJP is the forward kernel on g_y; the median routes g_y[t] to the window position it came from
int dmad_wave_smooth_vjp(dmad_engine* e, const float* x, const float* g_y, int32_t B, int32_t kind, int32_t window, float* g_x, dmad_stream s) {
    if (!e || !g_y || !g_x || (kind == 1 && !x)) return fail(DMAD_ERR_INVALID, "dmad_wave_smooth_vjp: null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "dmad_wave_smooth_vjp: B %d must be >= 1", B);
    if (const char* m = wave_smooth_check(kind, window)) return fail(DMAD_ERR_INVALID, "dmad_wave_smooth_vjp: %s (kind %d, window %d)", m, kind, window);
    if (kind == 0) launch_wave_smooth(g_y, B, e->L, 0, window, g_x, (hipStream_t)s);
    else launch_wave_median_vjp(x, g_y, B, e->L, window, g_x, (hipStream_t)s);
    LASTCHK();
    return 0;
}

// frequency_defense.py:53-56 (torchaudio Resample down and up: F.conv1d of the padded clip with the sinc kernel, stride orig)
int dmad_wave_resample(dmad_engine* e, const float* x, int32_t B, int32_t L_in, const float* ker, int32_t phases, int32_t taps, int32_t stride,
                       int32_t width, int32_t L_out, float* y, dmad_stream s) {
    if (!e || !x || !y || !ker) return fail(DMAD_ERR_INVALID, "dmad_wave_resample: null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "dmad_wave_resample: B %d must be >= 1", B);
    if (const char* m = wave_resample_check(ker, L_in, phases, taps, stride, width, L_out)) return fail(DMAD_ERR_INVALID, "dmad_wave_resample: %s", m);
    launch_wave_resample(x, B, L_in, ker, phases, taps, stride, width, L_out, y, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_wave_resample_vjp(dmad_engine* e, const float* g_y, int32_t B, int32_t L_in, const float* ker, int32_t phases, int32_t taps,
                           int32_t stride, int32_t width, int32_t L_out, float* g_x, dmad_stream s) {
    if (!e || !g_y || !g_x || !ker) return fail(DMAD_ERR_INVALID, "dmad_wave_resample_vjp: null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "dmad_wave_resample_vjp: B %d must be >= 1", B);
    if (const char* m = wave_resample_check(ker, L_in, phases, taps, stride, width, L_out)) return fail(DMAD_ERR_INVALID, "dmad_wave_resample_vjp: %s", m);
    launch_wave_resample_vjp(g_y, B, L_in, ker, phases, taps, stride, width, L_out, g_x, (hipStream_t)s);
    LASTCHK();
    return 0;
}

// frequency_defense.py:85-98 / 125-139 (lfilter one clip at a time on the CPU, then clamp) as one launch, parallel along time
int dmad_wave_iir(dmad_engine* e, const float* x, int32_t B, const float* b, const float* a, int32_t order, float lo, float hi, float* y,
                  dmad_stream s) {
    if (!e || !x || !y || !b || !a) return fail(DMAD_ERR_INVALID, "dmad_wave_iir: null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "dmad_wave_iir: B %d must be >= 1", B);
    if (!(hi >= lo)) return fail(DMAD_ERR_INVALID, "dmad_wave_iir: empty clamp range");
    IirPlan plan;
    if (const char* m = iir_plan(b, a, order, e->L, &plan)) return fail(DMAD_ERR_INVALID, "dmad_wave_iir: %s (order %d)", m, order);
    HIPCHK((hipError_t)launch_wave_iir(plan, x, nullptr, B, e->L, lo, hi, 0, y, nullptr, (hipStream_t)s));
    LASTCHK();
    return 0;
}

// the adjoint of the clamped filter: the same kernel, backwards in time, on g_y masked by the recomputed unclamped forward
int dmad_wave_iir_vjp(dmad_engine* e, const float* x, const float* g_y, int32_t B, const float* b, const float* a, int32_t order, float lo,
                      float hi, float* g_x, float* y_or_null, dmad_stream s) {
    if (!e || !x || !g_y || !g_x || !b || !a) return fail(DMAD_ERR_INVALID, "dmad_wave_iir_vjp: null argument");
    if (B < 1 || B > e->maxB) return fail(DMAD_ERR_INVALID, "dmad_wave_iir_vjp: B %d outside [1, max_batch = %d]", B, e->maxB);
    if (!(hi >= lo)) return fail(DMAD_ERR_INVALID, "dmad_wave_iir_vjp: empty clamp range");
    IirPlan plan;
    if (const char* m = iir_plan(b, a, order, e->L, &plan)) return fail(DMAD_ERR_INVALID, "dmad_wave_iir_vjp: %s (order %d)", m, order);
    HIPCHK((hipError_t)launch_wave_iir(plan, x, nullptr, B, e->L, lo, hi, 0, y_or_null, e->eps, (hipStream_t)s));
    HIPCHK((hipError_t)launch_wave_iir(plan, g_y, e->eps, B, e->L, lo, hi, 1, g_x, nullptr, (hipStream_t)s));
    LASTCHK();
    return 0;
}

}  // extern "C"

namespace {

// one baseline defense on the nb rows of e->xt -> e->x0 (DS goes through e->eps)
int run_wave_defense(dmad_engine* e, const dmad_wave_defense* d, const IirPlan& plan, int nb, hipStream_t st) {
    const int L = e->L;
    switch (d->kind) {
    case DMAD_WAVE_AS: launch_wave_smooth(e->xt, nb, L, 0, d->window, e->x0, st); break;
    case DMAD_WAVE_MS: launch_wave_smooth(e->xt, nb, L, 1, d->window, e->x0, st); break;
    case DMAD_WAVE_DS:
        launch_wave_resample(e->xt, nb, L, d->down_ker, d->down_phases, d->down_taps, d->down_stride, d->down_width, d->down_len, e->eps, st);
        launch_wave_resample(e->eps, nb, d->down_len, d->up_ker, d->up_phases, d->up_taps, d->up_stride, d->up_width, L, e->x0, st);
        break;
    default: HIPCHK((hipError_t)launch_wave_iir(plan, e->xt, nullptr, nb, L, d->lo, d->hi, 0, e->x0, nullptr, st)); break;
    }
    return 0;
}

constexpr int64_t kM5RsRowsPerLaunch = 16384;      // samples (= workgroups) per launch of dmad_m5_rs_smooth_votes

int m5_launch(dmad_engine* e, const float* x, int B, float* logp, int32_t* cls, const float* g_logp, float* g_x, int layer, float* pooled,
              uint8_t* dec, hipStream_t st) {
    if ((uintptr_t)x & 15) return fail(DMAD_ERR_INVALID, "M5: x must be 16-byte aligned (the clip is read as float4)");
    launch_m5(e->m5w, e->m5g, x, B, logp, cls, g_logp, g_x, layer, pooled, dec, st);
    HIPCHK(hipGetLastError());
    return 0;
}

// the host-side checks of the three KWS exports, then the one launch they share
int kws_launch(dmad_engine* e, const char* who, const float* spec, int B, int T, float* logp, int32_t* cls, const float* g_logp, float* g_spec,
               int stage, float* tape, hipStream_t st) {
    if (B < 1) return fail(DMAD_ERR_INVALID, "%s: B must be >= 1", who);
    CHK(need_kws(e));
    KwsGeom g;
    if (const char* m = kws_geometry(T, &g)) return fail(DMAD_ERR_SHAPE, "%s: %s (T = %d)", who, m, T);
    launch_kws(e->kwsw, g, spec, B, logp, cls, g_logp, g_spec, stage, tape, st);
    HIPCHK(hipGetLastError());
    return 0;
}

constexpr int kKwsWaveRows = 512;           // rows of one pass of the wave exports: what the engine-owned spectrogram scratch holds (two
                                            // rounds of one-workgroup-per-row kws_kernel launches over the CUs; 64 rows left three quarters idle)
constexpr int kKwsWaveMinL = kMelHop * (kKwsMinT - 1), kKwsWaveMaxL = kMelHop * kKwsMaxT - 1;      // T = 1 + L / 200 in 5 .. kKwsMaxT

// the host-side checks of the three mel exports
int kws_mel_args(dmad_engine* e, const char* who, int B, int L) {
    if (B < 1) return fail(DMAD_ERR_INVALID, "%s: B must be >= 1", who);
    if (L < kMelMinL) return fail(DMAD_ERR_SHAPE, "%s: L = %d is below %d: the reflect padding mirrors %d samples", who, L, kMelMinL, kMelHop);
    return need_kws_mel(e);
}

// ... and of the wave and query exports: finalised weights, T inside what kws.hip serves, the constants and the scratch
int kws_wave_args(dmad_engine* e, const char* who, int B, int L, KwsGeom* g) {
    if (B < 1) return fail(DMAD_ERR_INVALID, "%s: B must be >= 1", who);
    CHK(need_kws(e));
    if (L < kKwsWaveMinL || L > kKwsWaveMaxL)
        return fail(DMAD_ERR_SHAPE, "%s: L = %d is outside %d .. %d (T = 1 + L / %d frames must lie in %d .. %d)", who, L, kKwsWaveMinL, kKwsWaveMaxL,
                    kMelHop, kKwsMinT, kKwsMaxT);
    if (const char* m = kws_geometry(1 + L / kMelHop, g)) return fail(DMAD_ERR_SHAPE, "%s: %s (L = %d)", who, m, L);
    CHK(need_kws_mel(e));
    if (!e->kws_spec) CHK(e->alloc(&e->kws_spec, (size_t)kKwsWaveRows * kKwsIn * kKwsMaxT));
    if (!e->kws_gspec) CHK(e->alloc(&e->kws_gspec, (size_t)kKwsWaveRows * kKwsIn * kKwsMaxT));
    return 0;
}

// waveforms x [B][L] -> the read frames of mel dB -> kws_kernel, in passes of kKwsWaveRows rows (rows are independent: the pass size
// cannot change a bit).  With g_logp also the waveform gradient: the KWS VJP, then the mel VJP on the read frames
int kws_wave_rows(dmad_engine* e, const KwsGeom& g, const float* x, int B, int L, float* logp, int32_t* cls, const float* g_logp, float* g_x,
                  hipStream_t st) {
    return for_passes(B, kKwsWaveRows, [&](int64_t r0, int nb) -> int {
        const float* xr = x + r0 * L;
        launch_kws_mel(e->kmel, xr, nb, L, g.T2, e->kws_spec, 1, st);
        launch_kws(e->kwsw, g, e->kws_spec, nb, logp ? logp + r0 * kKwsOut : nullptr, cls ? cls + r0 : nullptr,
                   g_logp ? g_logp + r0 * kKwsOut : nullptr, g_logp ? e->kws_gspec : nullptr, -1, nullptr, st);
        if (g_logp) launch_kws_mel_vjp(e->kmel, xr, e->kws_gspec, nb, L, g.T2, g_x + r0 * L, nullptr, st);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

}  // namespace

extern "C" {

// ---- the KWS mel front-end (kws_adaptive_attack_eval.py: MelSpectrogram(sample_rate=16000, n_mels=32), AmplitudeToDB('power'))

int dmad_kws_mel_power(dmad_engine* e, const float* x, int32_t B, int32_t L, float* out, dmad_stream s) {
    if (!e || !x || !out) return fail(DMAD_ERR_INVALID, "dmad_kws_mel_power: null argument");
    CHK(kws_mel_args(e, "dmad_kws_mel_power", B, L));
    launch_kws_mel(e->kmel, x, B, L, 0, out, 0, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return 0;
}

int dmad_kws_mel_db(dmad_engine* e, const float* x, int32_t B, int32_t L, float* out, dmad_stream s) {
    if (!e || !x || !out) return fail(DMAD_ERR_INVALID, "dmad_kws_mel_db: null argument");
    CHK(kws_mel_args(e, "dmad_kws_mel_db", B, L));
    launch_kws_mel(e->kmel, x, B, L, 0, out, 1, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return 0;
}

int dmad_kws_mel_db_vjp(dmad_engine* e, const float* x, int32_t B, int32_t L, const float* g_spec, float* g_x, float* spec, dmad_stream s) {
    if (!e || !x || !g_spec || !g_x) return fail(DMAD_ERR_INVALID, "dmad_kws_mel_db_vjp: null argument");
    CHK(kws_mel_args(e, "dmad_kws_mel_db_vjp", B, L));
    launch_kws_mel_vjp(e->kmel, x, g_spec, B, L, 0, g_x, spec, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return 0;
}

int dmad_kws_wave_logits(dmad_engine* e, const float* x, int32_t B, int32_t L, float* logp, int32_t* decisions, dmad_stream s) {
    if (!e || !x || !logp) return fail(DMAD_ERR_INVALID, "dmad_kws_wave_logits: null argument");
    KwsGeom g;
    CHK(kws_wave_args(e, "dmad_kws_wave_logits", B, L, &g));
    return kws_wave_rows(e, g, x, B, L, logp, decisions, nullptr, nullptr, (hipStream_t)s);
}

int dmad_kws_wave_vjp(dmad_engine* e, const float* x, int32_t B, int32_t L, const float* g_logp, float* g_x, float* logp, dmad_stream s) {
    if (!e || !x || !g_logp || !g_x) return fail(DMAD_ERR_INVALID, "dmad_kws_wave_vjp: null argument");
    KwsGeom g;
    CHK(kws_wave_args(e, "dmad_kws_wave_vjp", B, L, &g));
    return kws_wave_rows(e, g, x, B, L, logp, nullptr, g_logp, g_x, (hipStream_t)s);
}

int dmad_kws_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, int32_t sampler, int32_t t_star, float c_a, float c_b,
                          const float* c_eps, const float* c_div, const float* c_sig, uint64_t seed, uint64_t sample0, float* logits,
                          int32_t* decisions, dmad_stream s) {
    CHK(query_args(e, x, logits, B, repeats, sampler, t_star, c_eps, c_div, c_sig));
    KwsGeom g;
    CHK(kws_wave_args(e, "dmad_kws_query_logits", B, e->L, &g));
    if (sampler) CHK(need_wavenet(e));
    hipStream_t st = (hipStream_t)s;
    // the arg-max comes out of the KWS launch itself, so query_loop's vote is not asked for
    return query_loop(e, x, B, repeats, logits, nullptr, st, [&](int nb, int64_t r0, float* lg) -> int {
        const float* pur;
        CHK(run_query_sampler(e, sampler, t_star, c_a, c_b, c_eps, c_div, c_sig, seed, sample0, r0, nb, st, &pur));
        return kws_wave_rows(e, g, pur, nb, e->L, lg, decisions ? decisions + r0 : nullptr, nullptr, nullptr, st);
    }, kKwsOut);
}

int dmad_kws_defense_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, const dmad_wave_defense* d, float* logits,
                                  int32_t* decisions, dmad_stream s) {
    if (!e || !x || !logits || !d) return fail(DMAD_ERR_INVALID, "dmad_kws_defense_query_logits: null argument");
    if (B < 1 || repeats < 1) return fail(DMAD_ERR_INVALID, "dmad_kws_defense_query_logits: B and repeats must be >= 1");
    IirPlan plan;
    if (const char* m = wave_defense_check(d, e->L, &plan)) return fail(DMAD_ERR_INVALID, "dmad_kws_defense_query_logits: %s", m);
    KwsGeom g;
    CHK(kws_wave_args(e, "dmad_kws_defense_query_logits", B, e->L, &g));
    hipStream_t st = (hipStream_t)s;
    return query_loop(e, x, B, repeats, logits, nullptr, st, [&](int nb, int64_t r0, float* lg) -> int {
        CHK(run_wave_defense(e, d, plan, nb, st));
        return kws_wave_rows(e, g, e->x0, nb, e->L, lg, decisions ? decisions + r0 : nullptr, nullptr, nullptr, st);
    }, kKwsOut);
}

// ---- KWS (audio_models/RCNN_KWS/model.py:93-114): forward, input VJP and the tape hook

int dmad_kws_logits(dmad_engine* e, const float* spec, int32_t B, int32_t T, float* logp, int32_t* decisions, dmad_stream s) {
    if (!e || !spec || !logp) return fail(DMAD_ERR_INVALID, "dmad_kws_logits: null argument");
    return kws_launch(e, "dmad_kws_logits", spec, B, T, logp, decisions, nullptr, nullptr, -1, nullptr, (hipStream_t)s);
}

int dmad_kws_vjp(dmad_engine* e, const float* spec, int32_t B, int32_t T, const float* g_logp, float* g_spec, float* logp, dmad_stream s) {
    if (!e || !spec || !g_logp || !g_spec) return fail(DMAD_ERR_INVALID, "dmad_kws_vjp: null argument");
    return kws_launch(e, "dmad_kws_vjp", spec, B, T, logp, nullptr, g_logp, g_spec, -1, nullptr, (hipStream_t)s);
}

int dmad_kws_tape(dmad_engine* e, const float* spec, int32_t B, int32_t T, int32_t stage, float* out, dmad_stream s) {
    if (!e || !spec || !out) return fail(DMAD_ERR_INVALID, "dmad_kws_tape: null argument");
    if (stage < 0 || stage > 3) return fail(DMAD_ERR_INVALID, "dmad_kws_tape: stage must be in 0..3");
    return kws_launch(e, "dmad_kws_tape", spec, B, T, nullptr, nullptr, nullptr, nullptr, stage, out, (hipStream_t)s);
}

// adaptive_attack_eval.py:190-201 (AcousticSystem with a Time / FreqDomainDefense as its defender) behind the query layout of
// dmad_query_logits
int dmad_defense_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, const dmad_wave_defense* d, float* logits,
                              int32_t* decisions, dmad_stream s) {
    if (!e || !x || !logits || !d) return fail(DMAD_ERR_INVALID, "dmad_defense_query_logits: null argument");
    if (B < 1 || repeats < 1) return fail(DMAD_ERR_INVALID, "dmad_defense_query_logits: B and repeats must be >= 1");
    IirPlan plan;
    if (const char* m = wave_defense_check(d, e->L, &plan)) return fail(DMAD_ERR_INVALID, "dmad_defense_query_logits: %s", m);
    CHK(need_with_classifier(e));
    hipStream_t st = (hipStream_t)s;
    return query_loop(e, x, B, repeats, logits, decisions, st, [&](int nb, int64_t, float* lg) -> int {
        CHK(run_wave_defense(e, d, plan, nb, st));
        return wave_logits(e, e->x0, nb, lg, st);
    });
}

// ---- M5 (audio_models/M5/M5Net.py:21-38): forward, input VJP, tape hook and the two query exports

int dmad_m5_logits(dmad_engine* e, const float* x, int32_t B, float* logp, int32_t* decisions, dmad_stream s) {
    if (!e || !x || !logp) return fail(DMAD_ERR_INVALID, "dmad_m5_logits: null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "dmad_m5_logits: B must be >= 1");
    CHK(need_m5(e));
    return m5_launch(e, x, B, logp, decisions, nullptr, nullptr, 0, nullptr, nullptr, (hipStream_t)s);
}

int dmad_m5_vjp(dmad_engine* e, const float* x, int32_t B, const float* g_logp, float* g_x, float* logp, dmad_stream s) {
    if (!e || !x || !g_logp || !g_x) return fail(DMAD_ERR_INVALID, "dmad_m5_vjp: null argument");
    if (B < 1) return fail(DMAD_ERR_INVALID, "dmad_m5_vjp: B must be >= 1");
    CHK(need_m5(e));
    return m5_launch(e, x, B, logp, nullptr, g_logp, g_x, 0, nullptr, nullptr, (hipStream_t)s);
}

int dmad_m5_tape(dmad_engine* e, const float* x, int32_t B, int32_t layer, float* pooled, uint8_t* decisions, dmad_stream s) {
    if (!e || !x || !pooled || !decisions) return fail(DMAD_ERR_INVALID, "dmad_m5_tape: null argument");
    if (B < 1 || layer < 1 || layer > 4) return fail(DMAD_ERR_INVALID, "dmad_m5_tape: B must be >= 1 and layer in 1..4");
    CHK(need_m5(e));
    return m5_launch(e, x, B, nullptr, nullptr, nullptr, nullptr, layer, pooled, decisions, (hipStream_t)s);
}

int dmad_m5_rs_smooth_votes(dmad_engine* e, const float* clip, float sigma, int64_t n, uint64_t seed, uint64_t sample0, const float* delta,
                            int64_t* counts, float* logp_out, dmad_stream s) {
    if (!e || !clip) return fail(DMAD_ERR_INVALID, "dmad_m5_rs_smooth_votes: null argument");
    if (!counts) return fail(DMAD_ERR_INVALID, "dmad_m5_rs_smooth_votes: counts must not be null");
    if (n < 0) return fail(DMAD_ERR_INVALID, "dmad_m5_rs_smooth_votes: n < 0");
    CHK(need_m5(e));
    if (((uintptr_t)clip | (uintptr_t)delta) & 15)
        return fail(DMAD_ERR_INVALID, "dmad_m5_rs_smooth_votes: clip and delta must be 16-byte aligned (they are read as float4)");
    const int64_t L = e->L, NO = e->m5g.n_out;
    // one workgroup per sample; a launch's grid is capped, and a sample's bits depend on its index alone, not on where the cut falls
    CHK(for_passes(n, kM5RsRowsPerLaunch, [&](int64_t done, int rows) -> int {
        launch_m5_noisy(e->m5w, e->m5g, clip, delta ? delta + done * L : nullptr, sigma, seed, sample0 + (uint64_t)done, rows,
                        (unsigned long long*)counts, logp_out ? logp_out + done * NO : nullptr, (hipStream_t)s);
        return 0;
    }));
    HIPCHK(hipGetLastError());
    return 0;
}

int dmad_m5_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, int32_t sampler, int32_t t_star, float c_a, float c_b,
                         const float* c_eps, const float* c_div, const float* c_sig, uint64_t seed, uint64_t sample0, float* logits,
                         int32_t* decisions, dmad_stream s) {
    CHK(query_args(e, x, logits, B, repeats, sampler, t_star, c_eps, c_div, c_sig));
    CHK(need_m5(e));
    if (sampler) CHK(need_wavenet(e));
    hipStream_t st = (hipStream_t)s;
    const int NO = e->m5g.n_out;
    // the arg-max comes out of the M5 launch itself, so query_loop's vote is not asked for
    return query_loop(e, x, B, repeats, logits, nullptr, st, [&](int nb, int64_t r0, float* lg) -> int {
        const float* pur;
        CHK(run_query_sampler(e, sampler, t_star, c_a, c_b, c_eps, c_div, c_sig, seed, sample0, r0, nb, st, &pur));
        return m5_launch(e, pur, nb, lg, decisions ? decisions + r0 : nullptr, nullptr, nullptr, 0, nullptr, nullptr, st);
    }, NO);
}

int dmad_m5_defense_query_logits(dmad_engine* e, const float* x, int32_t B, int32_t repeats, const dmad_wave_defense* d, float* logits,
                                 int32_t* decisions, dmad_stream s) {
    if (!e || !x || !logits || !d) return fail(DMAD_ERR_INVALID, "dmad_m5_defense_query_logits: null argument");
    if (B < 1 || repeats < 1) return fail(DMAD_ERR_INVALID, "dmad_m5_defense_query_logits: B and repeats must be >= 1");
    IirPlan plan;
    if (const char* m = wave_defense_check(d, e->L, &plan)) return fail(DMAD_ERR_INVALID, "dmad_m5_defense_query_logits: %s", m);
    CHK(need_m5(e));
    hipStream_t st = (hipStream_t)s;
    return query_loop(e, x, B, repeats, logits, nullptr, st, [&](int nb, int64_t r0, float* lg) -> int {
        CHK(run_wave_defense(e, d, plan, nb, st));
        return m5_launch(e, e->x0, nb, lg, decisions ? decisions + r0 : nullptr, nullptr, nullptr, 0, nullptr, nullptr, st);
    }, e->m5g.n_out);
}

int dmad_philox_raw(dmad_engine* e, uint64_t seed, uint64_t sample, uint32_t stream, uint32_t nblocks, uint32_t* out, dmad_stream s) {
    if (!e || !out) return fail(DMAD_ERR_INVALID, "null argument");
    launch_philox_raw(seed, sample, stream, nblocks, out, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_philox_normal(dmad_engine* e, uint64_t seed, uint64_t sample0, uint32_t stream, int32_t B, float* z, dmad_stream s) {
    if (!e || !z || B < 1) return fail(DMAD_ERR_INVALID, "bad argument");
    launch_philox_normal(seed, sample0, stream, z, B, e->L, (hipStream_t)s);
    LASTCHK();
    return 0;
}

int dmad_time_layer(dmad_engine* e, int32_t layer, int32_t B, int32_t iters, float* ms_per_launch, dmad_stream s) {
    if (!e || !ms_per_launch || iters < 1) return fail(DMAD_ERR_INVALID, "bad argument");
    if (!e->wn_final || !e->bf16) return fail(DMAD_ERR_STATE, "dmad_time_layer needs a finalised bf16 engine");
    if (B < 1 || B > e->maxB || layer < 0 || layer >= e->NL) return fail(DMAD_ERR_STATE, "bad batch or layer");
    hipStream_t st = (hipStream_t)s;
    WnLayerArgs a{};
    a.hin = e->hA; a.hout = e->hB; a.gout = e->gstore + (size_t)layer * B * e->L * kC;
    a.w1p = e->w1p + (size_t)layer * 24 * 512 * 32; a.w2p = e->w2p + (size_t)layer * 8 * 256 * 32;
    a.b1 = e->b1p + (size_t)layer * 512; a.epi_c = e->epi_c + (size_t)layer * 256;
    a.dilation = 1 << (layer % e->cfg.dilation_cycle); a.L = e->L; a.LP = e->LP; a.last = 0; a.npos = (long)B * e->L;
    const char* ev = getenv("DMAD_LAYER_STAMPS");         // development only: per-phase cycle stamps (diagnostic build)
    const bool stamps = ev && atoi(ev) != 0;
    unsigned long long* dbg = nullptr;
    const size_t nblk = (size_t)B * (e->L / kTileT);
    if (stamps) {
        HIPCHK(hipMalloc((void**)&dbg, nblk * 8 * sizeof(unsigned long long)));
        a.dbg = dbg;
    }
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    launch_wn_layer_bf16_p(a, B, e->f16, st, stamps);
    HIPCHK(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) launch_wn_layer_bf16_p(a, B, e->f16, st, stamps);
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *ms_per_launch = ms / iters;
    if (dbg) {      // diagnostic: mean phase lengths in shader cycles (s_memtime), printed to stderr
        std::vector<unsigned long long> h(nblk * 8);
        HIPCHK(hipMemcpy(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost));
        double sum[9] = {0};
        for (size_t i = 0; i < 256 && i < nblk; ++i)   // per-workgroup phase sums over all its tiles
            for (int k = 0; k < 8; ++k) sum[k + 1] += (double)h[i * 8 + k];
        const size_t nwg = nblk < 256 ? nblk : 256;
        fprintf(stderr, "[dmad stamps] top-wait %.0f | gemm1 %.0f | gate0+barrier %.0f | gate||gemm2 %.0f | barrier %.0f | epilogue %.0f  (mean cycles per tile, %zu tiles); "
                "in-kernel clock %.3f GHz (shader cycles / 100 MHz ticks over the workgroups' lifetimes)\n",
                sum[1] / nblk, sum[2] / nblk, sum[3] / nblk, sum[4] / nblk, sum[5] / nblk, sum[8] / nblk, nblk,
                sum[7] > 0 ? sum[6] / sum[7] * 0.1 : 0.0);
        (void)nwg;
        (void)hipFree(dbg);
    }
    return 0;
}

}  // extern "C"
