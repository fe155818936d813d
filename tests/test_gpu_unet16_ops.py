"""What sits between the GEMMs of the UNet's 16-bit tier, op by op through the test hooks of include/dmad.h, each against float64 torch on the
CPU: the f16 MFMA attention, the two-pass f16 GroupNorm, the first (1 -> C) and the last (128 -> 1) conv, the upsampling, and the
split-format outputs of the fp32 GroupNorm and attention.  The whole-network tests prove composition under a tolerance of 6e-3 after ~180
ops; these point at a kernel.  References, bounds and the measured constant behind the GroupNorm tolerance live in tests/unet16_ops_ref.py
(checked without a GPU by tests/test_unet16_ops_cpu.py)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_ops_ref as R  # noqa: E402
import unet16_ops_ref as U  # noqa: E402

pytestmark = pytest.mark.gpu


def _E():
    from dmad_hip import engine as E
    return E


def _cu(t):
    return None if t is None else t.cuda()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------ attention, f16
ATT16_CASES = [(T, heads, B, False) for T in (16, 64, 256) for heads in (1, 4) for B in (1, 3)] + [c for c in R.ATT_CASES if c[3]]


@pytest.mark.parametrize('case', ATT16_CASES, ids=lambda c: 'T%d_h%d_B%d_spread%d' % tuple(int(v) for v in c))
def test_qkv_attention_h16_vs_float64(case):
    """qkv_attention_h16_kernel<1|4|16> (T = 16: the one-tile path of the two-tile MFMA): every output element within the bound derived
    from the kernel's roundings (unet16_ops_ref.attention_h16_bound) of a float64 attention on the same f16 values; a sample's and a head's
    bits do not depend on the batch or on the other heads."""
    E = _E()
    T, heads, B, _ = case
    q16 = R.att_inputs(case)[0].half()
    ref = R.attention_ref(q16.double(), heads)
    bound = U.attention_h16_bound(q16, heads)
    out = E.qkv_attention_h16(q16.cuda(), heads)
    assert out.dtype == torch.float16 and tuple(out.shape) == (B, T, heads * 64)
    err = (out.cpu().double() - ref).abs()
    print('attention_h16 T=%d heads=%d B=%d: max err / bound = %.3f, max err / max|ref| = %.3e' %
          (T, heads, B, float((err / bound).max()), float(err.max()) / float(ref.abs().max())))
    assert bool((err <= bound).all()), float((err / bound).max())
    assert _same_bits(E.qkv_attention_h16(q16[B - 1:].cuda(), heads), out[B - 1:])
    if heads == 4:
        for h in range(4):
            one = E.qkv_attention_h16(q16[..., h * 192:(h + 1) * 192].contiguous().cuda(), 1)
            assert _same_bits(one, out[..., h * 64:(h + 1) * 64].contiguous()), h


def test_qkv_attention_h16_refuses_other_map_sizes():
    E = _E()
    for T in (8, 32, 128, 512):
        with pytest.raises(E.DmadError):
            E.qkv_attention_h16(torch.zeros(1, T, 192, device='cuda', dtype=torch.float16), 1)


# ---------------------------------------------------------------------------------------------------------- two-pass f16 GroupNorm
@pytest.mark.parametrize('case', U.GN16_CASES, ids=lambda c: 'HW%d_C%d_c1%d_ss%d_silu%d' % tuple(int(v) for v in c[:5]))
def test_groupnorm16_two_pass_vs_float64(case):
    """launch_groupnorm_nhwc on f16 maps (groupnorm16_stream_kernel: the form un_groupnorm16 falls back to without a statistics slab) on
    every map the UNet normalises and on concatenated inputs whose groups straddle the two parts, against float64 F.group_norm of the
    same f16 map.  The bound is 8 x the error of fp32 torch on the CPU on these inputs (unet16_ops_ref.GN16_FWD_TOL)."""
    E = _E()
    hw, C, c1, with_ss, silu, _ = case
    x16, gamma, beta, ss = U.gn16_inputs(case)
    y64 = R.groupnorm_ref(x16.double(), gamma.double(), beta.double(), None if ss is None else ss.double(), silu)
    xa, xb = (x16[..., :c1].contiguous(), x16[..., c1:].contiguous()) if c1 else (x16, None)
    kw = dict(silu=bool(silu), ss=_cu(ss))
    y32 = E.groupnorm16(xa.cuda(), gamma.cuda(), beta.cuda(), x2=_cu(xb), out32=True, **kw)
    y16 = E.groupnorm16(xa.cuda(), gamma.cuda(), beta.cuda(), x2=_cu(xb), **kw)
    err = R.rel(y32.cpu(), y64)
    print('groupnorm16 HW=%d C=%d c1=%d ss=%d silu=%d: err / max|ref| = %.3e (bound %.2e)' % (hw, C, c1, with_ss, silu, err, U.GN16_FWD_TOL))
    assert y32.dtype == torch.float32 and y16.dtype == torch.float16
    assert err < U.GN16_FWD_TOL, err
    assert _same_bits(y16, y32.half())
    x2_1 = None if xb is None else xb[1:2].cuda()
    assert _same_bits(E.groupnorm16(xa[1:2].cuda(), gamma.cuda(), beta.cuda(), x2=x2_1, out32=True, **kw), y32[1:2])
    assert _same_bits(E.groupnorm16(xa[1:2].cuda(), gamma.cuda(), beta.cuda(), x2=x2_1, **kw), y16[1:2])


def _one_pass_vs_two_pass(E, a16, st, seed):
    """groupnorm16_apply on (map, statistics slab) against the two-pass hook on the same f16 map [B][HW][C], with scale-shift and SiLU."""
    B, HW, C = a16.shape
    g = torch.Generator().manual_seed(seed)
    gamma, beta, ss = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5, torch.rand(2 * C, generator=g) - 0.5
    ref = R.groupnorm_ref(a16.cpu().double(), gamma.double(), beta.double(), ss.double(), True)
    tol = U.GN_ONE_PASS_TOL * max(1.0, float(ref.abs().max()))
    one32 = E.groupnorm16_apply(a16, st, gamma.cuda(), beta.cuda(), silu=True, ss=ss.cuda(), out32=True)
    two32 = E.groupnorm16(a16, gamma.cuda(), beta.cuda(), silu=True, ss=ss.cuda(), out32=True)
    d = float((one32 - two32).abs().max())
    print('one-pass vs two-pass GroupNorm HW=%d C=%d: max diff %.3e (bound %.3e); two-pass vs float64 %.3e' % (HW, C, d, tol, R.rel(two32.cpu(), ref)))
    assert d < tol, d
    one16 = E.groupnorm16_apply(a16, st, gamma.cuda(), beta.cuda(), silu=True, ss=ss.cuda())
    two16 = E.groupnorm16(a16, gamma.cuda(), beta.cuda(), silu=True, ss=ss.cuda())
    for y in (one16, two16):
        assert bool(((y.cpu().double() - ref).abs() < U.U16 * ref.abs() + tol).all())


@pytest.mark.parametrize('H,C', [(32, 128), (16, 256), (8, 256), (4, 256)])
def test_groupnorm16_two_pass_vs_one_pass(H, C):
    """The two forms of the tier's GroupNorm on one map per resolution: a conv GEMM's f16 output with the statistics its epilogue left
    (one-pass) against the two-pass kernel on the same map."""
    E = _E()
    g = torch.Generator().manual_seed(7300 + H)
    x = (torch.rand(3, H, H, 128, generator=g) * 2 - 1).half().cuda()
    w = ((torch.rand(1, 9, C, 128, generator=g) * 2 - 1) * 0.08).half().cuda()
    b = (torch.rand(C, generator=g) * 4 - 1).cuda()
    a16, st = E.conv_h16_stats(x, w, b)
    _one_pass_vs_two_pass(E, a16.reshape(3, H * H, C), st, 7400 + H)


def test_groupnorm16_refuses_what_no_kernel_serves():
    E = _E()
    z = lambda *s: torch.zeros(*s, device='cuda', dtype=torch.float16)
    f = lambda n: torch.ones(n, device='cuda')
    for C in (96, 640):
        with pytest.raises(E.DmadError):
            E.groupnorm16(z(1, 16, C), f(C), f(C))
    with pytest.raises(E.DmadError):
        E.groupnorm16(z(1, 16, 130), f(256), f(256), x2=z(1, 16, 126))                     # a split off the 4-channel grid


# -------------------------------------------------------------------------------------------------------------------- conv1ch_3x3
@pytest.mark.parametrize('B', (1, 3))
@pytest.mark.parametrize('Cout', (128, 64, 6))
def test_conv1ch_3x3_vs_float64(B, Cout):
    """The tier's first layer (also the output conv's backward in the UNet VJP): fp32 map against a float64 conv2d — image 0 is a single
    1 at each corner and at the centre —, the f16 twin = the rounded fp32 map, the GroupNorm statistics slab against float64 block sums
    of the f16 outputs within the worst-case fp32 bound for 256 sequential terms, and batch invariance."""
    E = _E()
    x, w, bias = U.conv1ch_inputs(B, Cout)
    ref = U.conv1ch_ref(x, w, bias)
    with_stats = Cout % 4 == 0
    o32, o16, st = E.conv1ch_3x3(x.cuda(), w.cuda(), bias.cuda(), want_stats=with_stats)
    err = R.rel(o32.cpu(), ref)
    print('conv1ch_3x3 B=%d Cout=%d: err / max|ref| = %.3e (bound %.1e)' % (B, Cout, err, R.F32_TOL))
    assert err < R.F32_TOL, err
    assert _same_bits(o16, o32.half())
    only16 = E.conv1ch_3x3(x.cuda(), w.cuda(), bias.cuda(), want32=False)[1]                # each output is optional
    assert _same_bits(only16, o16)
    if with_stats:
        want, sabs = U.conv1ch_block_stats(o16.cpu())
        e1, e2 = (st.cpu().double() - want)[..., 0].abs(), (st.cpu().double() - want)[..., 1].abs()
        b1, b2 = 256 * 2.0 ** -24 * sabs, 256 * 2.0 ** -24 * want[..., 1]
        print('  statistics: worst err / bound  sum %.3f  sum of squares %.3f' % (float((e1 / b1).max()), float((e2 / b2).max())))
        assert bool((e1 <= b1).all()) and bool((e2 <= b2).all())
    if B == 3:
        s32, s16, sst = E.conv1ch_3x3(x[2:3].cuda(), w.cuda(), bias.cuda(), want_stats=with_stats)
        assert _same_bits(s32, o32[2:3]) and _same_bits(s16, o16[2:3])
        assert not with_stats or _same_bits(sst, st[32:48])
    if Cout == 128:
        _one_pass_vs_two_pass(E, o16, st, 7500 + B)


def test_conv1ch_3x3_refusals():
    E = _E()
    x = torch.zeros(1, 32, 32, device='cuda')
    with pytest.raises(E.DmadError):
        E.conv1ch_3x3(x, torch.zeros(6, 9, device='cuda'), torch.zeros(6, device='cuda'), want_stats=True)      # quads of 4 channels
    with pytest.raises(E.DmadError):
        E.conv1ch_3x3(x, torch.zeros(129, 9, device='cuda'), torch.zeros(129, device='cuda'))                  # one thread per channel
    o32, _, _ = E.conv1ch_3x3(x + 1, torch.ones(4, 9, device='cuda'), torch.zeros(4, device='cuda'))           # a refusal leaves no debt behind
    assert float(o32[0, 33, 0]) == 9 and float(o32[0, 0, 3]) == 4


# -------------------------------------------------------------------------------------------------------- conv3x3_c128_to1, fp32
def _regions():
    yy, xx = torch.meshgrid(torch.arange(32), torch.arange(32), indexing='ij')
    by, bx = (yy == 0) | (yy == 31), (xx == 0) | (xx == 31)
    return {'corners': (by & bx).reshape(-1), 'edges': ((by | bx) & ~(by & bx)).reshape(-1), 'interior': (~(by | bx)).reshape(-1)}


@pytest.mark.parametrize('B', (1, 3))
def test_conv3x3_c128_to1_f32_vs_float64(B):
    """The last layer on the fp32 and split tiers, and its AFFINE form (the VP-SDE adjoint update): fp32-grade against float64 on the
    corners, the edges and the interior separately; batch-invariant bits; AFFINE = alpha * g_in - gamma * (the plain kernel's output)
    with each product and the difference rounded once."""
    E = _E()
    g = torch.Generator().manual_seed(7600)
    x = torch.rand(3, 1024, 128, generator=g) * 2 - 1
    w, bias = (torch.rand(9, 128, generator=g) * 2 - 1) * 0.1, torch.rand(1, generator=g) * 2 - 1
    g_in = torch.randn(3, 1024, generator=g)
    x, g_in = x[:B].contiguous(), g_in[:B].contiguous()
    ref = U.c128_to1_ref(x, w, bias)
    out = E.conv3x3_c128_to1(x.cuda(), w.cuda(), bias.cuda())
    assert R.rel(out.cpu(), ref) < R.F32_TOL
    for name, mask in _regions().items():
        e = R.rel(out.cpu()[:, mask], ref[:, mask])
        print('conv3x3_c128_to1 B=%d %s: err / max|ref| = %.3e (bound %.1e)' % (B, name, e, R.F32_TOL))
        assert e < R.F32_TOL, (name, e)
    assert _same_bits(E.conv3x3_c128_to1(x[B - 1:].cuda(), w.cuda(), bias.cuda()), out[B - 1:])
    alpha, gamma = 0.9873, 0.0421
    aff = E.conv3x3_c128_to1(x.cuda(), w.cuda(), bias.cuda(), g_in=g_in.cuda(), alpha=alpha, gamma=gamma)
    a32, g32 = torch.tensor(alpha, dtype=torch.float32), torch.tensor(gamma, dtype=torch.float32)
    assert _same_bits(aff.cpu(), (a32 * g_in) - (g32 * out.cpu()))
    ref_aff = a32.double() * g_in.double() - g32.double() * ref
    e = R.rel(aff.cpu(), ref_aff)
    print('conv3x3_c128_to1 B=%d AFFINE: err / max|ref| = %.3e' % (B, e))
    assert e < R.F32_TOL, e
    assert _same_bits(E.conv3x3_c128_to1(x[B - 1:].cuda(), w.cuda(), bias.cuda(), g_in=g_in[B - 1:].cuda(), alpha=alpha, gamma=gamma), aff[B - 1:])


# --------------------------------------------------------------------------------------------------------- conv3x3_c128_to1_h16
@pytest.mark.parametrize('B', (1, 3))
@pytest.mark.parametrize('scale', U.C128_SCALES, ids=lambda s: 'w%g' % s)
def test_conv3x3_c128_to1_h16_vs_float64(scale, B):
    """The 16-bit tier's last layer (MFMA, the fp32 weights split into two f16 parts): every pixel within the bound of a split that
    really carries 22 significant bits (unet16_ops_ref.c128_to1_bound), at weight scales down to 1e-4 — the reference UNet initialises
    this conv to zero, so trained weights here can be small —, and batch invariance."""
    E = _E()
    x16, w, bias = U.c128_to1_inputs(scale, B)
    ref = U.c128_to1_ref(x16, w, bias)
    bound = U.c128_to1_bound(x16, w)
    out = E.conv3x3_c128_to1(x16.cuda(), w.cuda(), bias.cuda())
    err = (out.cpu().double() - ref).abs()
    print('conv3x3_c128_to1_h16 B=%d weight scale %g: max err / bound = %.3f, max err / max|ref| = %.3e' %
          (B, scale, float((err / bound).max()), float(err.max()) / float(ref.abs().max())))
    assert bool((err <= bound).all()), float((err / bound).max())
    assert _same_bits(E.conv3x3_c128_to1(x16[B - 1:].cuda(), w.cuda(), bias.cuda()), out[B - 1:])


# ------------------------------------------------------------------------------------------------------------------- upsampling
@pytest.mark.parametrize('dtype', (torch.float32, torch.float16), ids=('f32', 'f16'))
def test_upsample2x_bit_equal(dtype):
    E = _E()
    g = torch.Generator().manual_seed(7700)
    for H in (2, 4, 16):
        for C in (128, 384):
            for B in (1, 3):
                x = torch.randn(B, H, H, C, generator=g).to(dtype)
                assert _same_bits(E.upsample2x(x.cuda()).cpu(), U.upsample2x_ref(x)), (H, C, B)
    with pytest.raises(E.DmadError):
        E.upsample2x(torch.zeros(1, 2, 2, 4 if dtype == torch.float16 else 6, device='cuda', dtype=dtype))


# ----------------------------------------------------------------------------------------------------------- split-format outputs
def test_split_format_outputs_of_the_fp32_groupnorm_and_attention():
    """The `split` argument the split-f16 middle tier uses: the output written in the split format is, bit for bit, the split of the
    plain output."""
    E = _E()
    for case in ((256, 128, 0, False, True, False), (64, 256, 0, True, True, False), (1024, 384, 256, True, False, False)):
        hw, C, c1, _, silu, _ = case
        x, gamma, beta, ss, _, _, _ = R.gn_inputs(case)
        xa, xb = (x[..., :c1].contiguous(), x[..., c1:].contiguous()) if c1 else (x, None)
        args = (xa.cuda(), gamma.cuda(), beta.cuda())
        plain = E.groupnorm_f32(*args, silu=bool(silu), ss=_cu(ss), x2=_cu(xb))
        sp = E.groupnorm_f32(*args, silu=bool(silu), ss=_cu(ss), x2=_cu(xb), split=True)
        assert torch.equal(sp.view(torch.int32), E.split_f16(plain).view(torch.int32)), case
        assert not torch.equal(sp.view(torch.int32), plain.view(torch.int32))
    for case in ((16, 4, 1, False), (64, 1, 3, False), (256, 4, 1, False)):
        qkv = R.att_inputs(case)[0].cuda()
        plain = E.qkv_attention_f32(qkv, case[1])
        sp = E.qkv_attention_f32(qkv, case[1], split=True)
        assert torch.equal(sp.view(torch.int32), E.split_f16(plain).view(torch.int32)), case
        assert not torch.equal(sp.view(torch.int32), plain.view(torch.int32))
