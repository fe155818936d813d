"""The op-level fp32 tests' CPU half: dmad.h declares the hooks, the cross-compiled library exports them and dmad_hip._lib binds them;
the float64 reference helpers of tests/f32_ops_ref.py are themselves checked; and the fp32-CPU-vs-float64 errors behind the two
transcendental tolerances of tests/test_gpu_f32_ops.py are measured here, so that the committed constants are reproducible."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_ops_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
LIB = os.path.join(PKG, 'libdmad_hip.so')
NAMES = ('dmad_conv_f32', 'dmad_conv_f32_vjp', 'dmad_groupnorm_f32', 'dmad_groupnorm_bwd', 'dmad_qkv_attention_f32', 'dmad_qkv_attention_bwd',
         'dmad_rx_head_bwd', 'dmad_rx_conv1_bwd')


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
            want = ctypes.c_void_p if ('*' in a or 'dmad_stream' in a) else ctypes.c_int64 if 'int64_t' in a else ctypes.c_int32
            assert t == want, (name, a)


def test_attention_reference_against_sdpa():
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(2, 16, 4 * 192, generator=g, dtype=torch.float64)
    q, k, v = (t.permute(0, 2, 1, 3) for t in R.split_qkv(qkv, 4))
    want = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(2, 16, 256)      # its scale: 1 / sqrt(64) = 1/8
    assert float((R.attention_ref(qkv, 4) - want).abs().max()) < 1e-13


def test_weight_layouts_against_brute_force():
    g = torch.Generator().manual_seed(2)
    for groups, taps, stride in ((1, 9, 1), (2, 9, 2), (1, 1, 2), (2, 1, 1)):
        w, x = torch.randn(groups, taps, 3, 2, generator=g), torch.randn(2, 5, 5, groups * 2, generator=g)
        assert float((R.conv_ref(x, w, stride=stride) - R.conv_brute(x, w, stride)).abs().max()) < 1e-12
    w = torch.randn(9, 3, 2, generator=g)
    p = R.unvjp_pack_ref(w)
    assert all(p[t, k, m] == w[8 - t, m, k] for t in range(9) for k in range(2) for m in range(3))
    w1, sc = torch.randn(3, 5, generator=g), torch.rand(3, generator=g)
    tr = R.cvjp_transpose_ref(w1, sc, 4)
    assert all(tr[k, m] == (w1[m, k] * sc[m] if m < 3 else 0) for k in range(5) for m in range(4))
    wg, sg = torch.randn(8, 9, 2, 2, generator=g), torch.rand(16, generator=g)
    pg = R.cvjp_pack_grouped_ref(wg, sg)
    assert all(pg[q, t, k, m] == wg[q, 8 - t, m, k] * sg[q * 2 + m] for q in range(8) for t in range(9) for k in range(2) for m in range(2))
    # the data-gradient reference is the adjoint of the forward reference: <conv(x), g> == <x, dgrad(g)>
    wc, xc, gc = torch.randn(1, 9, 16, 4, generator=g), torch.randn(1, 4, 4, 4, generator=g), torch.randn(1, 2, 2, 16, generator=g)
    lhs = (R.conv_ref(xc, wc, stride=2) * gc.double()).sum()
    assert abs(float(lhs - (xc.double() * R.conv_dgrad_ref(gc, wc, 4, stride=2)).sum())) < 1e-10
    d = R.dilate2x_ref(torch.arange(8.).reshape(1, 2, 2, 2))
    assert d.shape == (1, 4, 4, 2) and float(d[0, 2, 2, 1]) == 7 and float(d.sum()) == 28 and float(d[0, 1].abs().sum()) == 0


def test_dispatch_calculator_against_hand_computed_cases():
    """launch_gemm_f32's rules by hand: 128-row tiles unless M <= 64 or fewer than 128 of them; the narrow tile under 256 workgroups of 64
    rows with >= 8 k-steps; two-part input always on its own 128-row instantiation; S = min(768 / wgs_ref, nks / 4) under 384 wgs_ref."""
    D = R.gemm_f32_dispatch
    assert D(15 * 1024, 128, 128, 9) == dict(bm=64, narrow=1, two=0, splits=1)        # 120 x 1 tiles of 128 < 128; 120 x 2 of 64 < 256
    assert D(16 * 1024, 128, 128, 9) == dict(bm=128, narrow=0, two=0, splits=1)       # 128 x 1
    assert D(3 * 1024, 512, 64, 1) == dict(bm=64, narrow=0, two=0, splits=1)          # 24 x 4 = 96 < 128, but 4 k-steps < 8
    assert D(4 * 1024, 512, 64, 1) == dict(bm=128, narrow=0, two=0, splits=1)         # 32 x 4 = 128
    assert D(70 * 1024, 64, 64, 9) == dict(bm=64, narrow=0, two=0, splits=1)          # M <= 64: 560 workgroups
    assert D(31 * 1024, 64, 64, 9) == dict(bm=64, narrow=1, two=0, splits=1)          # 248 < 256
    assert D(256, 128, 384, 1, two=True) == dict(bm=128, narrow=0, two=1, splits=1)
    assert D(15 * 256, 128, 128, 9, groups=4) == dict(bm=64, narrow=1, two=0, splits=1)   # 30 x 1 x 4 = 120 < 128; 30 x 2 x 4 = 240 < 256
    assert D(16 * 256, 128, 128, 9, groups=4) == dict(bm=128, narrow=0, two=0, splits=1)
    assert D(8, 512, 1024, 1, slab_floats=1 << 22, n_ref=64) == dict(bm=64, narrow=1, two=0, splits=16)   # wgs_ref 4: min(192, 64 / 4); 1 x 8 x 16 = 128 < 256
    assert D(8, 512, 1024, 1, slab_floats=1 << 22, n_ref=4) == dict(bm=64, narrow=1, two=0, splits=1)     # N > n_ref: one split
    assert D(96, 512, 512, 9, slab_floats=100000, n_ref=96) == dict(bm=64, narrow=1, two=0, splits=2)     # the slab holds 2 x 96 x 512 only
    assert R.dispatch_batches(1024, 128, 128, 9) == [1, 15, 16]
    assert R.dispatch_batches(1024, 512, 64, 1, extra=(2,)) == [1, 2, 3, 4]


def test_fp32_cpu_reference_errors():
    """The measurement behind GN_BWD_TOL / ATT_BWD_TOL: fp32 torch on the CPU against float64 on the GPU tests' own inputs.  The committed
    constants are what this prints (an fp32 CPU build with another vector width may differ a little: within 0.5 - 1.25 x), and 8 x them
    stays under a tenth of the whole-network VJP_TOL."""
    gn, att = R.measure_fp32_cpu_errors()
    print('fp32 CPU vs float64: GroupNorm backward %.3e, attention backward %.3e' % (gn, att))
    assert 0.5 * R.GN_BWD_FP32_CPU_ERR <= gn <= 1.25 * R.GN_BWD_FP32_CPU_ERR, gn
    assert 0.5 * R.ATT_BWD_FP32_CPU_ERR <= att <= 1.25 * R.ATT_BWD_FP32_CPU_ERR, att
    assert R.GN_BWD_TOL == 8 * R.GN_BWD_FP32_CPU_ERR <= 1e-5 and R.ATT_BWD_TOL == 8 * R.ATT_BWD_FP32_CPU_ERR <= 1e-5
    q, _ = R.att_inputs((64, 4, 2, True))
    s = (q[0, 3, 0:64] @ q[0, :, 64:128].T) / 8
    assert 25 < float(s.max() - s.min()) < 40                      # the row that exercises the max subtraction
