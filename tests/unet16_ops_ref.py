"""References, bounds and CPU emulations shared by tests/test_gpu_unet16_ops.py (GPU) and tests/test_unet16_ops_cpu.py (no GPU): what sits
between the GEMMs of the UNet's 16-bit tier (f16 attention, two-pass f16 GroupNorm, the first and the last conv, the upsampling).  Plain
torch on the CPU; nothing here touches the HIP library.  The float64 references and the inputs are those of tests/f32_ops_ref.py."""
import math

import torch
import torch.nn.functional as F

from f32_ops_ref import ATT_CASES, F32_TOL, GN_MAPS, att_inputs, attention_ref, conv_ref, gn_inputs, groupnorm_ref, rel  # noqa: F401

U16 = 2.0 ** -11          # unit roundoff of f16 (11 significant bits)
LOG2E = 1.4426950408889634


# --------------------------------------------------------------------------------------------------------------- attention, f16
def _qkv_parts(qkv16, heads, dtype):
    B, T, _ = qkv16.shape
    q, k, v = qkv16.to(dtype).reshape(B, T, heads, 3, 64).permute(3, 0, 2, 1, 4)      # each [B][heads][T][64]
    return q, k, v


def _merge_heads(o):
    B, heads, T, _ = o.shape
    return o.permute(0, 2, 1, 3).reshape(B, T, heads * 64)


def attention_h16_bound(qkv16, heads):
    """Elementwise bound on |kernel - attention_ref(float64)| for qkv_attention_h16_kernel, from its roundings: the scores are exact f16
    products in fp32 sums (inside the F32_TOL term, like the fp32 row sum and the fp32 output accumulation); each softmax weight is rounded
    to f16 (relative 2^-11: 2^-11 * softmax(s) @ |v|), or, in and below the f16 subnormal range, absolutely (2^-25 per key and unit of
    max |v| of the head: T * 2^-25 * max|v|; the row sum is >= 1); the output is rounded to f16 (2^-11 * |ref|).  [B][T][heads * 64], float64."""
    B, T, _ = qkv16.shape
    ref = attention_ref(qkv16.double(), heads)
    q, k, v = _qkv_parts(qkv16, heads, torch.float64)
    s = (q @ k.transpose(-1, -2)) * 0.125
    p = torch.softmax(s, -1)
    pv = _merge_heads(p @ v.abs())
    vmax = v.abs().amax((2, 3), keepdim=True).expand(B, heads, T, 64)                # per sample and head
    return U16 * ref.abs() + U16 * pv + T * 2.0 ** -25 * _merge_heads(vmax) + F32_TOL * float(ref.abs().max())


def attention_h16_emulation(qkv16, heads, wrong=None):
    """The kernel's arithmetic on the CPU: q * 0.125 in f16 (exact), scores in fp32, p = exp2((s - m) * log2 e) in fp32, the row sum l over
    the unrounded p, (f16(p) @ v) / l in fp32, the result rounded to f16.  wrong: one of three deliberately wrong kernels —
    'swap_v' (the V rows of keys 5 and 6, one 16-key tile, swapped in the second product), 'sum_f16' (l taken over the f16-rounded
    weights and kept in their format: summed key by key in f16), 'drop_tile' (the second key tile of the first pair, keys 16..31, missing
    from the second product).  'sum_rounded' (l = the fp32 sum of f16(p)) is NOT wrong in the bound's sense: sum(f16(p) v) / sum(f16(p)) is
    a correctly normalised softmax whose weights carry one f16 rounding each, which the bound's first two terms cover to first order."""
    q, k, v = _qkv_parts(qkv16, heads, torch.float16)
    q = (q * torch.tensor(0.125, dtype=torch.float16)).float()
    k, v = k.float(), v.float()
    s = q @ k.transpose(-1, -2)
    m2 = s.max(-1, keepdim=True)[0] * LOG2E
    p = torch.exp2(s * LOG2E - m2)
    p16 = p.half().float()
    l = (p16 if wrong == 'sum_rounded' else p).sum(-1, keepdim=True)
    if wrong == 'sum_f16':
        acc = torch.zeros(p.shape[:-1], dtype=torch.float16)
        for j in range(p.shape[-1]):
            acc = acc + p[..., j].half()
        l = acc.float()[..., None]
    if wrong == 'swap_v':
        v = v.clone()
        v[:, :, [5, 6]] = v[:, :, [6, 5]]
    if wrong == 'drop_tile':
        p16 = p16.clone()
        p16[..., 16:32] = 0
    return _merge_heads((p16 @ v) / l).half()


# --------------------------------------------------------------------------------------------------- the last layer, 128 -> 1
def c128_to1_ref(x, w, bias, dtype=torch.float64):
    """x [B][1024][128], w [9][128] (tap-major), bias [1] -> [B][1024]: the 3x3 conv with zero padding on the 32 x 32 map."""
    B = x.shape[0]
    return conv_ref(x.reshape(B, 32, 32, 128), w.reshape(1, 9, 1, 128), shift=bias.reshape(1), dtype=dtype).reshape(B, 1024)


def c128_to1_bound(x16, w):
    """Per output pixel: 2^-21 * conv(|x|, |w|), the error of a weight split that really carries 22 significant bits (hi and lo of 11 each),
    + F32_TOL * max |ref|, the project's fp32-grade allowance for the fp32 accumulation.  The f16 inputs are exact."""
    ref = c128_to1_ref(x16, w, torch.zeros(1))
    return 2.0 ** -21 * c128_to1_ref(x16.abs(), w.abs(), torch.zeros(1)) + F32_TOL * float(ref.abs().max())


def split_weights(w, scaled):
    """What the two f16 parts of an fp32 weight add up to, in float64: hi = f16(w), lo = f16(w - hi) — or, scaled, lo = f16((w - hi) * 2^11)
    taken back by 2^-11 (the project's split format, csrc/dmad_common.h)."""
    w = w.float()
    hi = w.half().float()
    if scaled:
        lo = ((w - hi) * 2048.0).half().double() / 2048.0
    else:
        lo = (w - hi).half().double()
    return hi.double() + lo


def c128_to1_inputs(scale, B=3):
    g = torch.Generator().manual_seed(7100 + B)
    x16 = (torch.rand(B, 1024, 128, generator=g) * 2 - 1).half()
    w = (torch.rand(9, 128, generator=g) * 2 - 1) * scale
    bias = (torch.rand(1, generator=g) * 2 - 1) * scale
    return x16, w, bias


C128_SCALES = (0.1, 1e-3, 1e-4)


# ------------------------------------------------------------------------------------------------------ the first layer, 1 -> Cout
def conv1ch_ref(x, w, bias):
    """x [B][32][32], w [Cout][9], bias [Cout] -> [B][1024][Cout], float64."""
    Cout = w.shape[0]
    y = F.conv2d(x.double()[:, None], w.double().reshape(Cout, 1, 3, 3), bias.double(), padding=1)
    return y.permute(0, 2, 3, 1).reshape(x.shape[0], 1024, Cout)


def conv1ch_block_stats(out16):
    """The GroupNorm statistics slab of the f16-rounded outputs out16 [B][1024][Cout] in float64: per sample, pair of image rows (64 pixels)
    and 4-channel quad, (sum t, sum t^2) -> [B * 16][Cout / 4][2] (the layout groupnorm16_apply consumes), and sum |t| [B * 16][Cout / 4]."""
    B, _, Cout = out16.shape
    t = out16.double().reshape(B * 16, 64, Cout // 4, 4)
    return torch.stack([t.sum((1, 3)), (t * t).sum((1, 3))], -1), t.abs().sum((1, 3))


def conv1ch_inputs(B, Cout):
    g = torch.Generator().manual_seed(7200 + Cout)
    w = (torch.rand(Cout, 9, generator=g) * 2 - 1) * 0.5
    bias = torch.rand(Cout, generator=g) * 2 - 1
    x = torch.rand(3, 32, 32, generator=g) * 2 - 1
    x[0] = 0                                              # a single 1 at each corner and at the centre: every border tap on its own
    for (r, c) in ((0, 0), (0, 31), (31, 0), (31, 31), (16, 16)):
        x[0, r, c] = 1
    return x[:B].contiguous(), w, bias


# ------------------------------------------------------------------------------------------------------ two-pass f16 GroupNorm
# (HW, C, c1, scale-shift, SiLU, -): every map the UNet normalises, then the concatenated inputs with c1 = 256 (at C = 384 the group at
# channels 252 - 263 straddles the two parts), each with and without scale-shift and SiLU.  The tuple form is gn_inputs' own.
GN16_CASES = [(hw, c, c1, ss, silu, False) for (hw, c, c1) in [(hw, c, 0) for (hw, c) in GN_MAPS] + [(256, 384, 256), (1024, 384, 256), (64, 512, 256)]
              for ss in (False, True) for silu in (False, True)]


def gn16_inputs(case, B=3):
    """gn_inputs with the map rounded to f16 (returned as an f16 tensor)."""
    x, gamma, beta, ss, _, _, _ = gn_inputs(case, B)
    return x.half(), gamma, beta, ss


def measure_gn16_fp32_cpu_error():
    """The worst error (max |err| / max |ref|) of fp32 torch group_norm (+ scale-shift, + SiLU) on the CPU against float64, over GN16_CASES
    on their own f16-rounded inputs."""
    worst = 0.0
    for case in GN16_CASES:
        x16, gamma, beta, ss = gn16_inputs(case)
        y64 = groupnorm_ref(x16.double(), gamma.double(), beta.double(), None if ss is None else ss.double(), case[4])
        y32 = groupnorm_ref(x16.float(), gamma, beta, ss, case[4])
        worst = max(worst, rel(y32, y64))
    return worst


# The measured value (test_unet16_ops_cpu.test_gn16_fp32_cpu_reference_error reproduces it) and the bound derived from it as
# f32_ops_ref does: the kernel sums its partials sequentially where torch sums pairwise, and its SiLU is one v_exp and one v_rcp (1 ulp
# each) where torch calls libm — at most ~8 x the accumulated rounding.  The bound may not exceed the project's fp32-grade F32_TOL.
GN16_FWD_FP32_CPU_ERR = 3.69e-7
GN16_FWD_TOL = 8 * GN16_FWD_FP32_CPU_ERR
GN_ONE_PASS_TOL = 2e-4    # one-pass (epilogue statistics) against two-pass, * max(1, max |ref|): the bound the one-pass test already uses


def upsample2x_ref(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)
