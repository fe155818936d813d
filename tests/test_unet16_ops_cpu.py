"""The CPU half of the op-level tests of the UNet's 16-bit tier (tests/test_gpu_unet16_ops.py): dmad.h declares the new hooks, the
cross-compiled library exports them and dmad_hip._lib binds them; the derived attention bound holds for a faithful emulation of the kernel's
arithmetic and catches three wrong kernels; the 128 -> 1 conv's bound separates the unscaled weight split from the scaled one; and the
fp32-CPU-vs-float64 error behind the GroupNorm tolerance is measured here, so that the committed constant is reproducible."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_ops_ref as R  # noqa: E402
import unet16_ops_ref as U  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
LIB = os.path.join(PKG, 'libdmad_hip.so')
NAMES = ('dmad_qkv_attention_h16', 'dmad_groupnorm16', 'dmad_conv1ch_3x3', 'dmad_conv3x3_c128_to1', 'dmad_conv3x3_c128_to1_h16', 'dmad_upsample2x',
         'dmad_groupnorm_f32', 'dmad_qkv_attention_f32')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(LIB):
        subprocess.run(['make', '-C', os.path.join(PKG, 'csrc'), '-j4'], check=True)
    return ctypes.CDLL(LIB)


def test_header_declares_library_exports_and_lib_binds_the_hooks(lib):
    from dmad_hip import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dmad.h')).read(), flags=re.S)
    for name in NAMES:
        m = re.search(r'int\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
        res, args = _lib._SIGNATURES[name]
        assert res == ctypes.c_int and len(args) == len(m.group(1).split(',')), name        # one ctypes type per declared argument
        for a, t in zip(m.group(1).split(','), args):
            want = ctypes.c_void_p if ('*' in a or 'dmad_stream' in a) else ctypes.c_int64 if 'int64_t' in a else \
                ctypes.c_float if 'float' in a else ctypes.c_int32
            assert t == want, (name, a)
    for name in ('dmad_groupnorm_f32', 'dmad_qkv_attention_f32'):                          # the split-format output is asked for by argument
        assert re.search(r'int\s+%s\s*\([^)]*int32_t\s+split\b' % name, hdr), name


def _att_ratio(case, wrong=None):
    """max over the elements of |emulation - float64 reference| / bound."""
    q16 = R.att_inputs(case)[0].half()
    ref = R.attention_ref(q16.double(), case[1])
    err = (U.attention_h16_emulation(q16, case[1], wrong).double() - ref).abs()
    return float((err / U.attention_h16_bound(q16, case[1])).max())


def test_attention_emulation_within_the_bound():
    """The kernel's arithmetic, emulated on the CPU, stays inside the bound derived from its roundings on every case of the GPU test."""
    worst = max(_att_ratio(case) for case in R.ATT_CASES)
    print('attention_h16 emulation: worst err / bound = %.3f' % worst)
    assert worst < 1.0, worst
    q16 = R.att_inputs(R.ATT_CASES[0])[0].half()
    b, ref = U.attention_h16_bound(q16, 1), R.attention_ref(q16.double(), 1)
    assert float(b.mean()) < 1e-3 * float(ref.abs().max())                 # a bound of a few f16 roundings, not a tolerance in disguise


def test_attention_bound_catches_wrong_kernels():
    """Three deliberately wrong emulations leave the bound, so the GPU test would notice such a kernel: two V rows of one 16-key tile
    swapped (the regrouped V tile), the row sum kept in the weights' f16 format on a T = 256 row whose logits spread by ~30, the second
    key tile of a pair dropped at T = 64 (each MFMA contracts two key tiles)."""
    for T in (16, 64, 256):
        assert _att_ratio((T, 1, 1, False), 'swap_v') > 1.0, T
    spread256 = (256, 1, 1, True)
    q = R.att_inputs(spread256)[0].half().float()
    s = (q[0, 3, 0:64] @ q[0, :, 64:128].T) / 8
    assert 25 < float(s.max() - s.min()) < 45                              # the spread row
    assert _att_ratio(spread256) < 1.0
    assert _att_ratio(spread256, 'sum_f16') > 1.0
    assert _att_ratio((64, 1, 1, False), 'drop_tile') > 1.0
    assert _att_ratio((64, 4, 2, True), 'drop_tile') > 1.0


def _split_ratio(scale, scaled):
    """The split-only emulation of conv3x3_c128_to1_h16 (exact sums of the f16 inputs times hi + lo) against the bound: max err / bound."""
    x16, w, bias = U.c128_to1_inputs(scale)
    ref = U.c128_to1_ref(x16, w, bias)
    got = U.c128_to1_ref(x16, U.split_weights(w, scaled), bias)
    return float(((got - ref).abs() / U.c128_to1_bound(x16, w)).max())


def test_weight_split_unscaled_and_scaled():
    """hi = f16(w), lo = f16(w - hi): below |w| ~ 1e-3 lo is an f16 subnormal (spacing 2^-24) and no longer carries 11 more bits — the
    bound is violated at weight scale 1e-4.  With lo = f16((w - hi) * 2^11) (the project's split format) it holds at every scale."""
    for scale in U.C128_SCALES:
        print('weight scale %g: unscaled split err / bound = %.3g, scaled %.3g' % (scale, _split_ratio(scale, False), _split_ratio(scale, True)))
    assert _split_ratio(1e-4, False) > 1.0
    for scale in (0.1, 1e-3, 1e-4):
        assert _split_ratio(scale, True) < 1.0, scale


def test_block_statistics_reference():
    """conv1ch_block_stats on a map whose sums are known by hand: block = (sample, pair of image rows), quad = 4 channels."""
    t = torch.zeros(2, 1024, 8, dtype=torch.float16)
    t[1, 64 * 5 + 7, 4:8] = torch.tensor([1., -2., 3., 0.5], dtype=torch.float16)
    t[1, 64 * 5 + 63, 5] = 2
    st, sabs = U.conv1ch_block_stats(t)
    assert st.shape == (32, 2, 2) and sabs.shape == (32, 2)
    assert st[16 + 5, 1].tolist() == [4.5, 18.25] and float(sabs[16 + 5, 1]) == 8.5
    st[16 + 5, 1] = 0
    assert float(st.abs().sum()) == 0


def test_gn16_fp32_cpu_reference_error():
    """The measurement behind GN16_FWD_TOL: fp32 torch on the CPU against float64 on the GPU test's own f16-rounded inputs.  The committed
    constant is what this prints (an fp32 CPU build with another vector width may differ a little: within 0.5 - 1.25 x); 8 x it stays
    under the project's fp32-grade bound."""
    e = U.measure_gn16_fp32_cpu_error()
    print('fp32 CPU vs float64: GroupNorm forward on f16-rounded maps %.3e' % e)
    assert 0.5 * U.GN16_FWD_FP32_CPU_ERR <= e <= 1.25 * U.GN16_FWD_FP32_CPU_ERR, e
    assert U.GN16_FWD_TOL == 8 * U.GN16_FWD_FP32_CPU_ERR <= R.F32_TOL
    assert len(U.GN16_CASES) == 4 * (len(R.GN_MAPS) + 3) and sum(1 for c in U.GN16_CASES if c[2] == 256 and c[1] == 384) == 8
