"""The exact-fp32 tier op by op (csrc/gemm_f32.hip's plain fp32 path, the GroupNorm / attention kernels and the backward-only kernels of
the vector-Jacobian products) through the test hooks of include/dmad.h, each against float64 torch on the CPU: F.conv2d, F.group_norm,
an explicit softmax attention, torch.autograd.grad for every backward.  The whole-network VJP tests prove composition; these point at a
kernel.  References, inputs and the measured fp32-CPU errors behind the two transcendental tolerances live in tests/f32_ops_ref.py."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _E():
    from dmad_hip import engine as E
    return E


def _cu(t):
    return None if t is None else t.cuda()


def _run_conv(case, x, w, scale, shift, res, sl, **kw):
    _, H, cin, cout, taps, stride, c1, with_res, relu, groups = case
    xs = x[sl]
    xa, xb = (xs[..., :c1], xs[..., c1:]) if c1 else (xs, None)
    return _E().conv_f32(_cu(xa), _cu(w), _cu(shift), scale=_cu(scale) if relu else None, stride=stride, groups=groups, relu=bool(relu),
                         res=None if res is None else _cu(res[sl]), x2=_cu(xb), **kw)


@pytest.mark.parametrize('case', R.CONV_CASES, ids=lambda c: 'B%d_H%d_%dto%d_t%d_s%d_c1%d_r%d_relu%d_g%d' % tuple(int(v) for v in c))
def test_conv_f32_vs_float64(case):
    """dmad_conv_f32 at batch sizes on both sides of every dispatch threshold of launch_gemm_f32 (computed from the launcher's rules):
    the launcher chose what the rules say, the result is fp32-grade against a float64 conv, and a sample's output has the same bits in
    every batch and every tile shape."""
    B0, H, cin, cout, taps, stride, c1, with_res, relu, groups = case
    Mg, Kg = cout // groups, cin // groups
    Ho = (H - 1) // stride + 1
    batches = R.dispatch_batches(Ho * Ho, Mg, Kg, taps, groups, bool(c1), extra=(B0,))
    Bmax = max(batches)
    x, w, scale, shift, res = R.conv_inputs(case, Bmax)
    solo = {}
    for b in sorted({0, Bmax - 1, min(1, Bmax - 1)}):
        solo[b], ch1 = _run_conv(case, x, w, scale, shift, res, slice(b, b + 1))
        assert ch1['splits'] == 1
    for B in batches:
        out, ch = _run_conv(case, x, w, scale, shift, res, slice(0, B))
        assert ch == R.gemm_f32_dispatch(B * Ho * Ho, Mg, Kg, taps, groups, bool(c1)), (B, ch)
        worst, top = 0.0, 0.0
        for b0 in range(0, B, 16):                      # the float64 reference in chunks of the batch
            sl = slice(b0, min(B, b0 + 16))
            ref = R.conv_ref(x[sl], w, scale if relu else None, shift, None if res is None else res[sl], stride, bool(relu))
            worst = max(worst, float((out[sl].cpu().double() - ref).abs().max()))
            top = max(top, float(ref.abs().max()))
        print('conv_f32 B=%d %s err/max|ref| = %.3e' % (B, ch, worst / top))
        assert worst / top < R.F32_TOL, (B, ch, worst / top)
        for b, o1 in solo.items():
            if b < B:
                assert torch.equal(out[b:b + 1], o1), (B, b, ch)            # batch- and tile-invariant bits


def test_conv_f32_reaches_every_dispatch_form():
    """Every form of launch_gemm_f32's plain path, named by the hook's report and not by assumption: the narrow 64 x 32 tile, the 64-row
    tile, the 128-row tile, the two-part instantiation, grouped launches (both tile heights), split-K with the reduce kernel."""
    E = _E()
    g = torch.Generator().manual_seed(1)
    mk = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).cuda()
    seen = {}
    _, seen['narrow'] = E.conv_f32(mk(1, 16, 16, 128), mk(1, 9, 128, 128) * 0.1)
    _, seen['bm64'] = E.conv_f32(mk(40, 32, 32, 64), mk(1, 9, 64, 64) * 0.1)
    _, seen['bm128'] = E.conv_f32(mk(16, 32, 32, 128), mk(1, 9, 128, 128) * 0.1)
    _, seen['two'] = E.conv_f32(mk(2, 16, 16, 256), mk(1, 1, 128, 384) * 0.1, x2=mk(2, 16, 16, 128))
    _, seen['grouped64'] = E.conv_f32(mk(2, 16, 16, 512), mk(4, 9, 128, 128) * 0.1, groups=4)
    _, seen['grouped128'] = E.conv_f32(mk(16, 16, 16, 512), mk(4, 9, 128, 128) * 0.1, groups=4)
    slab = torch.empty(1 << 22, device='cuda')
    _, seen['splitk'] = E.conv_f32(mk(8, 1024), mk(1, 1, 512, 1024) * 0.1, slab=slab, n_ref=64)
    assert seen['narrow'] == dict(bm=64, narrow=1, two=0, splits=1), seen
    assert seen['bm64'] == dict(bm=64, narrow=0, two=0, splits=1), seen
    assert seen['bm128'] == dict(bm=128, narrow=0, two=0, splits=1), seen
    assert seen['two'] == dict(bm=128, narrow=0, two=1, splits=1), seen
    assert seen['grouped64']['bm'] == 64 and seen['grouped128'] == dict(bm=128, narrow=0, two=0, splits=1), seen
    assert seen['splitk']['splits'] > 1, seen


ROW_CASES = [(10, 1024), (35, 1024), (64, 256), (512, 1024), (2048, 2064)]      # M, K: the FC heads' class counts, a 64-row GEMM, the mel DFT^T


@pytest.mark.parametrize('M,K', ROW_CASES)
def test_gemm_f32_rows_and_split_k(M, K):
    """The plain row form (Linear layers, the mel DFT) without and with the split-K slab: S > 1 by the hook's report and by the rules,
    fp32-grade against float64, and with one n_ref the same bits for every N <= n_ref; N > n_ref falls back to one split."""
    E = _E()
    g = torch.Generator().manual_seed(70 + M)
    n_ref = 96
    x = torch.rand(n_ref + 4, K, generator=g) * 2 - 1
    w = (torch.rand(1, 1, M, K, generator=g) * 2 - 1) * 0.1
    shift = torch.rand(M, generator=g) * 2 - 1
    res = torch.rand(n_ref + 4, M, generator=g) * 2 - 1
    ref = torch.relu(x.double() @ w[0, 0].double().T + shift.double() + res.double())
    top = float(ref.abs().max())
    slab = torch.empty(1 << 22, device='cuda')
    xc, wc, sc, rc = x.cuda(), w.cuda(), shift.cuda(), res.cuda()
    full, ch = E.conv_f32(xc[:n_ref], wc, sc, relu=True, res=rc[:n_ref], slab=slab, n_ref=n_ref)
    want = R.gemm_f32_dispatch(n_ref, M, K, 1, slab_floats=slab.numel(), n_ref=n_ref)
    assert ch == want and ch['splits'] > 1, (ch, want)
    assert float((full.cpu().double() - ref[:n_ref]).abs().max()) / top < R.F32_TOL
    for N in (1, 5, 33, 95):
        out, chn = E.conv_f32(xc[:N], wc, sc, relu=True, res=rc[:N], slab=slab, n_ref=n_ref)
        assert chn['splits'] == ch['splits'] and chn == R.gemm_f32_dispatch(N, M, K, 1, slab_floats=slab.numel(), n_ref=n_ref), (N, chn)
        assert torch.equal(out, full[:N]), N
    over, cho = E.conv_f32(xc, wc, sc, relu=True, res=rc, slab=slab, n_ref=n_ref)          # N > n_ref: one split
    assert cho['splits'] == 1
    plain, chp = E.conv_f32(xc, wc, sc, relu=True, res=rc)
    assert chp['splits'] == 1 and torch.equal(over, plain)
    assert float((plain.cpu().double() - ref).abs().max()) / top < R.F32_TOL
    one, _ = E.conv_f32(xc[7:8], wc, sc, relu=True, res=rc[7:8])
    assert torch.equal(one, plain[7:8])


def test_conv_f32_split_k_conv_form():
    """Split-K on a conv (a deep 4 x 4 layer, as the VGG tail runs it): S > 1, fp32-grade, batch-invariant bits under one n_ref."""
    E = _E()
    case = (6, 4, 512, 512, 9, 1, 0, 0, True, 1)
    x, w, scale, shift, _ = R.conv_inputs(case, 6)
    slab = torch.empty(1 << 22, device='cuda')
    full, ch = E.conv_f32(x.cuda(), w.cuda(), shift.cuda(), scale=scale.cuda(), relu=True, slab=slab, n_ref=6 * 16)
    assert ch == R.gemm_f32_dispatch(96, 512, 512, 9, slab_floats=slab.numel(), n_ref=96) and ch['splits'] > 1, ch
    ref = R.conv_ref(x, w, scale, shift, None, 1, True)
    assert R.rel(full.cpu(), ref) < R.F32_TOL
    for b in (0, 3, 5):
        one, c1 = E.conv_f32(x[b:b + 1].cuda(), w.cuda(), shift.cuda(), scale=scale.cuda(), relu=True, slab=slab, n_ref=96)
        assert c1['splits'] == ch['splits'] and torch.equal(one, full[b:b + 1])


# form, taps, stride, groups, M (forward out channels per group), K (in), H (forward input resolution), acc, scale, mask, ldt
DGRAD_CASES = [
    (0, 9, 1, 1, 256, 128, 16, False, False, False, 0), (0, 1, 1, 1, 128, 384, 16, True, False, False, 0),
    (0, 1, 1, 1, 768, 256, 8, False, False, False, 0), (0, 9, 2, 1, 128, 128, 16, True, False, False, 0),
    (1, 9, 1, 1, 256, 256, 8, True, False, False, 0), (1, 9, 1, 1, 128, 128, 4, False, False, False, 0),
    (2, 1, 1, 1, 256, 64, 16, False, True, True, 0), (2, 1, 1, 1, 64, 256, 16, True, True, False, 0),
    (2, 1, 1, 1, 48, 128, 8, False, True, False, 64), (2, 1, 2, 1, 512, 256, 16, False, True, True, 0),
    (2, 9, 1, 8, 32, 32, 16, False, True, True, 0), (2, 9, 2, 8, 64, 64, 16, False, True, True, 0),
]


@pytest.mark.parametrize('case', DGRAD_CASES, ids=lambda c: 'f%d_t%d_s%d_g%d_M%d_K%d_H%d_acc%d_sc%d_mask%d_ldt%d' % tuple(int(v) for v in c))
def test_conv_f32_vjp_vs_float64_autograd(case):
    """Every data-gradient form of the UNet's and ResNeXt29's VJPs through the engine's own sequence (pack -> dilate -> GEMM): the
    packed image, the masked and the dilated map and the 2x2 sums exactly, the gradient against float64 autograd, and a sample's bits
    the same at B = 1, 3, 8 and 33."""
    E = _E()
    form, taps, stride, groups, M, K, H, with_acc, with_scale, with_mask, ldt = case
    g = torch.Generator().manual_seed(8000 + sum(int(v) for v in case))
    Ho = 2 * H if form == 1 else (H - 1) // stride + 1
    kp = ldt if ldt else M
    BB = 33
    w = (torch.rand(groups, taps, M, K, generator=g) * 2 - 1) * 0.1
    scale = (torch.rand(groups * M, generator=g) + 0.5) if with_scale else None
    g_y = torch.rand(BB, Ho, Ho, groups * kp, generator=g) * 2 - 1            # (a padded image: the extra channels carry values too)
    acc = (torch.rand(BB, H, H, groups * K, generator=g) * 2 - 1) if with_acc else None
    mask = None
    if with_mask:                                                              # a saved activation with exact zeros and negative zeros
        mask = torch.relu(torch.randn(BB, Ho, Ho, groups * M, generator=g))
        mask.view(-1)[::7] = -0.0
        mask.view(-1)[3::11] = -1.5
    kw = dict(form=form, stride=stride, groups=groups, scale=_cu(scale), ldt=ldt)
    gx, wT, gm, work = E.conv_f32_vjp(g_y.cuda(), w.cuda(), H, mask_y=_cu(mask), acc=_cu(acc), **kw)
    # the pack kernels on their own: exactly the permuted / flipped / scaled image, padded rows zero
    if form < 2:
        want_wT = R.unvjp_pack_ref(w[0])
    elif taps == 9:
        want_wT = R.cvjp_pack_grouped_ref(w, scale)
    else:
        want_wT = R.cvjp_transpose_ref(w[0, 0], scale, kp)
        assert bool((wT[:, M:] == 0).all())
    assert torch.equal(wT.cpu(), want_wT)
    gin = g_y
    if with_mask:
        gin = torch.where(mask > 0, g_y, torch.zeros_like(g_y))
        assert torch.equal(gm.cpu(), gin)                                      # relu_mask: y > 0, never y >= 0 or the sign bit
    if form == 1:
        assert torch.equal(gx.cpu(), R.upsample2x_bwd_ref(work.cpu(), acc))    # the 2x2 sums in the kernel's order, + add
    elif stride == 2 and taps == 9:
        assert torch.equal(work.cpu(), R.dilate2x_ref(gin))
    elif stride == 2:
        assert torch.equal(gx.cpu(), R.dilate2x_ref(work.cpu()))
    worst = top = 0.0
    for b0 in range(0, BB, 11):
        sl = slice(b0, b0 + 11)
        ref = R.conv_dgrad_ref(g_y[sl], w, H, form, stride, scale, None if mask is None else mask[sl], None if acc is None else acc[sl])
        worst, top = max(worst, float((gx[sl].cpu().double() - ref).abs().max())), max(top, float(ref.abs().max()))
    print('conv_f32_vjp err/max|ref| = %.3e' % (worst / top))
    assert worst / top < R.F32_TOL, worst / top
    for B in (1, 3, 8):
        gb = E.conv_f32_vjp(g_y[:B].cuda(), w.cuda(), H, mask_y=None if mask is None else mask[:B].cuda(),
                            acc=None if acc is None else acc[:B].cuda(), **kw)[0]
        assert torch.equal(gb, gx[:B]), B
    last = E.conv_f32_vjp(g_y[32:].cuda(), w.cuda(), H, mask_y=None if mask is None else mask[32:].cuda(),
                          acc=None if acc is None else acc[32:].cuda(), **kw)[0]
    assert torch.equal(last, gx[32:])


@pytest.mark.parametrize('case', R.GN_CASES, ids=lambda c: 'HW%d_C%d_c1%d_ss%d_silu%d_add%d' % tuple(int(v) for v in c))
def test_groupnorm_f32_forward_and_backward(case):
    """launch_groupnorm_nhwc (fp32) and groupnorm_bwd_kernel on every map the UNet normalises and on concatenated inputs whose groups
    straddle the two parts, against float64 F.group_norm and its autograd; gx and gx2 separately.  The backward bound is 8 x the error
    of fp32 torch on the CPU on these inputs (f32_ops_ref.GN_BWD_TOL)."""
    E = _E()
    hw, C, c1, with_ss, silu, with_add = case
    x, gamma, beta, ss, gy, add, add2 = R.gn_inputs(case)
    y64, g64 = R.gn_fwd_bwd(x, gamma, beta, ss, silu, gy, torch.float64)
    xa, xb = (x[..., :c1].contiguous(), x[..., c1:].contiguous()) if c1 else (x, None)
    y = E.groupnorm_f32(xa.cuda(), gamma.cuda(), beta.cuda(), silu=bool(silu), ss=_cu(ss), x2=_cu(xb))
    ferr = R.rel(y.cpu(), y64)
    gx, gx2 = E.groupnorm_bwd(xa.cuda(), gamma.cuda(), beta.cuda(), gy.cuda(), silu=bool(silu), ss=_cu(ss), x2=_cu(xb), add=_cu(add), add2=_cu(add2))
    want = g64 + (add.double() + add2.double() if with_add else 0)
    top = float(g64.abs().max())
    e1 = float((gx.cpu().double() - want[..., :c1 if c1 else C]).abs().max()) / top
    e2 = float((gx2.cpu().double() - want[..., c1:]).abs().max()) / top if c1 else 0.0
    print('groupnorm fwd %.3e  gx %.3e  gx2 %.3e  (bounds %.1e / %.2e)' % (ferr, e1, e2, R.F32_TOL, R.GN_BWD_TOL))
    assert ferr < R.F32_TOL, ferr
    assert e1 < R.GN_BWD_TOL, e1
    assert e2 < R.GN_BWD_TOL, e2
    one = E.groupnorm_bwd(xa[2:3].cuda(), gamma.cuda(), beta.cuda(), gy[2:3].cuda(), silu=bool(silu), ss=_cu(ss), x2=None if xb is None else xb[2:3].cuda(),
                          add=None if add is None else add[2:3].cuda(), add2=None if add2 is None else add2[2:3].cuda())
    assert torch.equal(one[0], gx[2:3]) and (not c1 or torch.equal(one[1], gx2[2:3]))


def test_groupnorm_bwd_serves_any_c_multiple_of_32():
    """C = 96 (3 channels per group) with c1 = 40: a split inside a group, off the float4 grid — the backward serves it; the forward refuses it."""
    E = _E()
    g = torch.Generator().manual_seed(9)
    x = 3 + 0.5 * torch.randn(2, 64, 96, generator=g)
    gamma, beta, gy = 1 + 0.3 * torch.randn(96, generator=g), 0.3 * torch.randn(96, generator=g), torch.randn(2, 64, 96, generator=g)
    _, g64 = R.gn_fwd_bwd(x, gamma, beta, None, True, gy, torch.float64)
    gx, gx2 = E.groupnorm_bwd(x[..., :40].contiguous().cuda(), gamma.cuda(), beta.cuda(), gy.cuda(), silu=True, x2=x[..., 40:].contiguous().cuda())
    assert R.rel(torch.cat([gx, gx2], 2).cpu(), g64) < R.GN_BWD_TOL
    with pytest.raises(E.DmadError):
        E.groupnorm_f32(x.cuda(), gamma.cuda(), beta.cuda())


@pytest.mark.parametrize('case', R.ATT_CASES, ids=lambda c: 'T%d_h%d_B%d_spread%d' % tuple(int(v) for v in c))
def test_qkv_attention_f32_forward_and_backward(case):
    """launch_qkv_attention (fp32) and qkv_attention_bwd_kernel against an explicit float64 softmax attention (head-major split, 1/8
    scale) and its autograd; dq, dk and dv each against its own max |ref|.  The backward bound is 8 x the error of fp32 torch on the CPU
    on these inputs (f32_ops_ref.ATT_BWD_TOL)."""
    E = _E()
    T, heads, B, spread = case
    qkv, go = R.att_inputs(case)
    o64, g64 = R.att_fwd_bwd(qkv, go, heads, torch.float64)
    out = E.qkv_attention_f32(qkv.cuda(), heads)
    ferr = R.rel(out.cpu(), o64)
    gq = E.qkv_attention_bwd(qkv.cuda(), go.cuda(), heads)
    errs = [R.rel(a, r) for a, r in zip(R.split_qkv(gq.cpu(), heads), R.split_qkv(g64, heads))]
    print('attention fwd %.3e  dq %.3e dk %.3e dv %.3e  (bounds %.1e / %.2e)' % (ferr, *errs, R.F32_TOL, R.ATT_BWD_TOL))
    assert ferr < R.F32_TOL, ferr
    for name, e in zip(('dq', 'dk', 'dv'), errs):
        assert e < R.ATT_BWD_TOL, (name, e)
    assert torch.equal(E.qkv_attention_bwd(qkv[B - 1:].cuda(), go[B - 1:].cuda(), heads), gq[B - 1:])


def test_rx_head_and_conv1_bwd_vs_float64():
    """The two ends of ResNeXt29's backward walk: FC + average pool + last ReLU (M = 10 and 35 classes; a mask with exact zeros and
    negative zeros must agree with y > 0), and conv1's ReLU + BN + 1 <- 64 conv, against float64."""
    E = _E()
    g = torch.Generator().manual_seed(11)
    for ncls, B in ((10, 3), (35, 33)):
        gl, W = torch.randn(B, ncls, generator=g), torch.randn(ncls, 1024, generator=g) * 0.1
        y = torch.relu(torch.randn(B, 64, 1024, generator=g))
        y.view(-1)[::5] = -0.0
        y.view(-1)[2::9] = -2.0
        gz = E.rx_head_bwd(gl.cuda(), W.cuda(), y.cuda()).cpu()
        ref = (gl.double() @ W.double())[:, None, :] / 64 * (y > 0).double()
        assert bool((gz[~(y > 0)] == 0).all()) and bool((gz[y > 0] != 0).any())
        assert R.rel(gz, ref) < R.F32_TOL
        assert torch.equal(E.rx_head_bwd(gl[B - 1:].cuda(), W.cuda(), y[B - 1:].cuda()).cpu(), gz[B - 1:])
    for B in (1, 9):
        gg, a = torch.randn(B, 32, 32, 64, generator=g), torch.randn(B, 32, 32, 64, generator=g)
        a.view(-1)[::5] = -0.0
        w, scale = torch.randn(64, 9, generator=g) * 0.2, torch.rand(64, generator=g) + 0.5
        got = E.rx_conv1_bwd(gg.cuda(), a.cuda(), w.cuda(), scale.cuda()).cpu()
        spec = torch.zeros(B, 1, 32, 32, dtype=torch.float64, requires_grad=True)
        yy = torch.nn.functional.conv2d(spec, w.double().reshape(64, 1, 3, 3), padding=1) * scale.double().reshape(1, 64, 1, 1)
        ref, = torch.autograd.grad(yy, spec, torch.where(a > 0, gg, torch.zeros_like(gg)).double().permute(0, 3, 1, 2))
        assert R.rel(got, ref[:, 0]) < R.F32_TOL


def test_hooks_refuse_what_no_kernel_serves():
    """One assertion per refusal: a shape no kernel serves is an error, never a wrong answer."""
    E = _E()
    from dmad_hip import _lib
    lib = _lib.load()
    z = lambda *s: torch.zeros(*s, device='cuda')
    R_ = pytest.raises(E.DmadError)
    with R_: E.conv_f32(z(1, 4, 4, 24), z(1, 1, 128, 24))                                  # K % 16
    with R_: E.conv_f32(z(1, 4, 4, 16), z(1, 1, 64, 32), x2=z(1, 4, 4, 16))                # two-part input on the 64-row tile
    with R_: E.conv_f32(z(1, 4, 4, 24), z(1, 1, 128, 48), x2=z(1, 4, 4, 24))               # ksplit % 16
    with R_: E.conv_f32(z(1, 4, 4, 32), z(2, 1, 128, 64), x2=z(1, 4, 4, 32), groups=2)     # two-part input on a grouped conv
    with R_: E.conv_f32(z(1, 4, 4, 16), z(1, 1, 16, 16), stride=3)                         # stride
    with R_: E.conv_f32_vjp(z(1, 4, 4, 24), z(1, 1, 24, 16), 4)                            # M % 16 (the gradient GEMM's K)
    with R_: E.conv_f32_vjp(z(1, 3, 3, 16), z(1, 9, 16, 16), 5, stride=2)                  # stride 2 on an odd map
    with R_: E.conv_f32_vjp(z(1, 8, 8, 16), z(1, 1, 16, 16), 4, form=1)                    # Upsample is a 3x3
    with R_: E.conv_f32_vjp(z(1, 4, 4, 128), z(8, 9, 16, 32), 4, form=2, groups=8, scale=z(128))   # grouped pack needs M = K
    with R_: E.conv_f32_vjp(z(1, 4, 4, 40), z(1, 1, 32, 16), 4, form=2, ldt=40)            # padded pitch off the k-step
    with R_: E.conv_f32_vjp(z(1, 4, 4, 16), z(1, 1, 16, 16), 4, form=0, scale=z(16))       # the UNet's forms carry no scale
    with R_: E.groupnorm_f32(z(1, 16, 96), z(96), z(96))                                   # forward: C % 128
    with R_: E.groupnorm_f32(z(1, 4096, 512), z(512), z(512))                              # forward: more than 16 float4s per thread
    with R_: E.groupnorm_bwd(z(1, 16, 48), z(48), z(48), z(1, 16, 48))                     # backward: C % 32
    for T in (8, 32, 128, 512):
        with R_: E.qkv_attention_f32(z(1, T, 192), 1)
        with R_: E.qkv_attention_bwd(z(1, T, 192), z(1, T, 64), 1)
    p = ctypes.c_void_p(z(16).data_ptr())
    assert lib.dmad_rx_head_bwd(p, p, p, 0, 10, 64, 1024, p, None) != 0                   # B < 1
    assert lib.dmad_rx_conv1_bwd(p, p, p, p, 0, p, None) != 0
    assert lib.dmad_conv_f32(p, None, 0, p, None, None, None, 1, 0, 16, 16, 9, 1, 1, 0, None, 0, 0, p, None, None) != 0    # rows with 9 taps
    out, _ = E.conv_f32(torch.ones(1, 16, device='cuda'), torch.ones(1, 1, 16, 16, device='cuda'))     # ... and a refusal leaves no debt behind
    assert bool((out == 16).all())
