"""WideResNet-28-10 on the engine (dmad_classify's third classifier, dmad_reserve_wrn_vjp / dmad_wrn_vjp): its new kernels alone, the
GEMM shapes new to the project (160 rows: a partial last tile), the whole VJP against a decision-pinned float64 walk (tests/wrn_cases.py),
forward bits, determinism and batch independence, a finite difference, every engine precision with the reservation and the refusals, and
the module, the query path and the five drivers built on it."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_ops_ref as R  # noqa: E402
import vjp_reservation  # noqa: E402
import wrn_cases as W  # noqa: E402
from dmad_hip import synth  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wideresnet28_10.npz')


def _E():
    from dmad_hip import engine as E
    return E


@pytest.fixture(scope='module')
def sd():
    return synth.wideresnet28_10_state_dict(W.WRN_SEED)


@pytest.fixture(scope='module')
def eng(sd):
    E = _E()
    e = E.Engine(max_batch=8, precision=E.FP32, with_wavenet=False)
    e.load_wideresnet28_10(sd)
    yield e
    e.close()


def clips(ids):
    return torch.from_numpy(np.stack([synth.synthetic_clip(i).reshape(-1) for i in ids])).float()


def cotangent(B, seed):
    return torch.randn(B, 10, generator=torch.Generator().manual_seed(seed))


def ints(gen, shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


# ---- 1. the pre-activation forward and backward, exact --------------------------------------------------------------------------------
@pytest.mark.parametrize('B,H,C', [(3, 4, 160), (2, 2, 640)])
def test_preact_exact(B, H, C):
    """Small integers and power-of-two scales: every product and sum is exact, so the kernels must equal the float64 reference bit for
    bit.  C = 160 is 40 float4s per pixel (no divisor of a wave).  The saved map holds -0.0 and negative entries: both give 0."""
    E = _E()
    gen = torch.Generator().manual_seed(H * C)
    x, shift = ints(gen, (B, H, H, C)), ints(gen, (C,))
    scale = torch.tensor([0.5, 1.0, 2.0, -1.0, -0.25, 4.0])[torch.randint(0, 6, (C,), generator=gen)]
    got = E.wrn_preact(x.cuda(), scale.cuda(), shift.cuda()).cpu()
    ref = torch.relu(x.double() * scale.double() + shift.double())
    assert torch.equal(got.double(), ref) and 0.05 < float((got > 0).float().mean()) < 0.95
    assert torch.equal(E.wrn_preact(x[B - 1:].cuda(), scale.cuda(), shift.cuda()).cpu(), got[B - 1:])
    o = got.clone()
    o.view(-1)[::7] = -0.0
    o.view(-1)[3::11] = -1.5
    g, res = ints(gen, (B, H, H, C)) * 0.25, ints(gen, (B, H, H, C))
    for r in (None, res):
        gx = E.wrn_preact_bwd(g.cuda(), o.cuda(), scale.cuda(), None if r is None else r.cuda()).cpu()
        want = torch.where(o > 0, scale.double() * g.double(), torch.zeros((), dtype=torch.float64)) + (0 if r is None else r.double())
        assert torch.equal(gx.double(), want), r is None
        assert bool((gx[o <= 0] == (0 if r is None else r[o <= 0])).all())
        one = E.wrn_preact_bwd(g[B - 1:].cuda(), o[B - 1:].cuda(), scale.cuda(), None if r is None else r[B - 1:].cuda()).cpu()
        assert torch.equal(one, gx[B - 1:])


# ---- 2. the stem forward and backward, exact ------------------------------------------------------------------------------------------
def test_stem_exact():
    E = _E()
    gen = torch.Generator().manual_seed(16)
    B = 3
    spec, w, g = ints(gen, (B, 32, 32)), ints(gen, (16, 9)) * 0.25, ints(gen, (B, 32, 32, 16))
    x = spec.double().unsqueeze(1).requires_grad_(True)
    y = F.conv2d(x, w.double().reshape(16, 1, 3, 3), None, 1, 1)
    got = E.wrn_stem(spec.cuda(), w.cuda()).cpu()
    assert torch.equal(got.double(), y.detach().permute(0, 2, 3, 1))
    (gx,) = torch.autograd.grad(y, x, g.double().permute(0, 3, 1, 2))
    back = E.wrn_stem_bwd(g.cuda(), w.cuda()).cpu()
    assert torch.equal(back.double(), gx[:, 0]) and float(back.abs().max()) > 0
    assert torch.equal(E.wrn_stem(spec[B - 1:].cuda(), w.cuda()).cpu(), got[B - 1:])
    assert torch.equal(E.wrn_stem_bwd(g[B - 1:].cuda(), w.cuda()).cpu(), back[B - 1:])


# ---- 3. the GEMM shapes new to the project --------------------------------------------------------------------------------------------
def _conv_case(seed, B, H, M, K, taps):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, H, H, K, generator=gen) * 2 - 1
    w = (torch.rand(1, taps, M, K, generator=gen) * 2 - 1) * 0.1
    return gen, x, w


@pytest.mark.parametrize('B,H,M,K,taps,stride,epi,slab,bm', [
    (3, 4, 160, 16, 9, 1, True, False, 64),        # block 0's conv1: K = 16, three 64-row tiles, the last holds 32 rows
    (3, 4, 160, 160, 9, 1, True, False, 64),       # M = K = 160 with bn2 + ReLU
    (3, 4, 160, 160, 9, 1, False, True, 64),       # conv2 with the shortcut as its residual, split-K through the slab (n_ref = 8 samples)
    (8, 32, 160, 16, 9, 1, True, False, 128),      # enough rows for 128-row tiles: 128 + 32
    (3, 4, 320, 160, 9, 2, True, False, 64),       # 160 -> 320 at stride 2
    (3, 4, 320, 160, 1, 2, False, False, 64),      # the 1x1 stride-2 shortcut
])
def test_forward_gemm_shapes(B, H, M, K, taps, stride, epi, slab, bm):
    """M = 160 is no multiple of the 64- or 128-row tile: the partial last tile against float64 within the exact tier's bound, and the
    last sample alone with the same bits (the split count follows from n_ref, not from B)."""
    E = _E()
    gen, x, w = _conv_case(1000 + M + K + taps + stride + B, B, H, M, K, taps)
    Ho = (H - 1) // stride + 1
    scale = shift = res = None
    if epi:
        scale, shift = torch.rand(M, generator=gen) + 0.5, torch.rand(M, generator=gen) - 0.5
    else:
        res = torch.rand(B, Ho, Ho, M, generator=gen) * 2 - 1
    ws = torch.empty(1 << 20, device='cuda') if slab else None
    kw = dict(stride=stride, relu=epi, slab=ws, n_ref=8 * Ho * Ho if slab else 0)
    cu = lambda t: None if t is None else t.cuda()
    got, choice = E.conv_f32(x.cuda(), w.cuda(), shift=cu(shift), scale=cu(scale), res=cu(res), **kw)
    ref = R.conv_ref(x, w, scale=scale, shift=shift, res=res, stride=stride, relu=epi)
    err = R.rel(got.cpu(), ref)
    print('conv B=%d H=%d M=%d K=%d taps=%d stride=%d: err/max|ref| = %.3e, choice %s' % (B, H, M, K, taps, stride, err, choice))
    assert err < R.F32_TOL, err
    assert choice['bm'] == bm and (choice['splits'] > 1) == slab
    one, _ = E.conv_f32(x[B - 1:].cuda(), w.cuda(), shift=cu(shift), scale=cu(scale), res=None if res is None else res[B - 1:].cuda(), **kw)
    assert torch.equal(one, got[B - 1:])


@pytest.mark.parametrize('B,H,M,K,taps,stride,with_scale', [
    (3, 4, 160, 160, 9, 1, True),                  # conv1 of an identity block: bn2's scale in the image, the ReLU mask, the residual
    (3, 4, 160, 16, 9, 1, True),                   # block 0's conv1: a 16-channel gradient
    (3, 4, 160, 160, 9, 1, False),                 # conv2: the plain image
    (3, 4, 320, 160, 9, 2, True),                  # 320 <- 160 at stride 2, H = 4 -> 2: the zero-dilated gradient
    (3, 4, 320, 160, 1, 2, False),                 # the 1x1 stride-2 shortcut: scattered into the even pixels
    (3, 4, 160, 16, 1, 1, False),                  # block 0's 1x1 shortcut
])
def test_form4_vs_float64_autograd(B, H, M, K, taps, stride, with_scale):
    """dmad_conv_f32_vjp form 4 (pack -> mask -> dilate -> GEMM -> scatter): the packed image exactly, the gradient against float64
    F.conv2d autograd within the exact tier's bound, and the last sample alone with the same bits."""
    E = _E()
    gen, _, w = _conv_case(2000 + M + K + taps + stride, B, H, M, K, taps)
    Ho = (H - 1) // stride + 1
    g_y = torch.rand(B, Ho, Ho, M, generator=gen) * 2 - 1
    scale = torch.rand(M, generator=gen) + 0.5 if with_scale else None
    mask = acc = None
    if with_scale:
        mask = torch.relu(torch.randn(B, Ho, Ho, M, generator=gen))
        mask.view(-1)[::7] = -0.0
    if not (taps == 1 and stride == 2):
        acc = torch.rand(B, H, H, K, generator=gen) * 2 - 1
    cu = lambda t, s=slice(None): None if t is None else t[s].cuda()
    gx, wT, gm, _ = E.conv_f32_vjp(g_y.cuda(), w.cuda(), H, form=4, stride=stride, scale=cu(scale), mask_y=cu(mask), acc=cu(acc))
    ws = w[0] * scale[None, :, None] if with_scale else w[0]
    assert torch.equal(wT.cpu(), ws.flip(0).permute(0, 2, 1).contiguous())          # wT[taps - 1 - t][k][m] = w[t][m][k] * scale[m]
    if mask is not None:
        assert torch.equal(gm.cpu(), torch.where(mask > 0, g_y, torch.zeros_like(g_y)))
    ref = R.conv_dgrad_ref(g_y, w, H, form=2, stride=stride, scale=scale, mask_y=mask, acc=acc)
    err = R.rel(gx.cpu(), ref)
    print('form 4 M=%d K=%d taps=%d stride=%d: err/max|ref| = %.3e' % (M, K, taps, stride, err))
    assert err < R.F32_TOL, err
    last = slice(B - 1, B)
    one = E.conv_f32_vjp(g_y[last].cuda(), w.cuda(), H, form=4, stride=stride, scale=cu(scale), mask_y=cu(mask, last), acc=cu(acc, last))[0]
    assert torch.equal(one, gx[last])
    if taps == 1 and stride == 2:
        with pytest.raises(E.DmadError):
            E.conv_f32_vjp(g_y.cuda(), w.cuda(), H, form=4, stride=2, acc=torch.zeros(B, H, H, K).cuda())


# ---- 4. the whole VJP against the decision-pinned float64 walk ------------------------------------------------------------------------
def _tape(eng, B):
    return [eng.wrn_vjp_tape(k, B).cpu().permute(0, 3, 1, 2).contiguous() for k in range(25)]


@pytest.mark.parametrize('B,seed', [(2, 1), (3, 12)])
def test_wrn_vjp_against_pinned_float64(eng, sd, B, seed):
    """The engine's tape gives the ReLU decisions; the float64 walk pinned to them gives the gradient and the maps the engine must match,
    and the free float64 walk says how far from the kink every differing decision lies."""
    net = W.sd64(sd)
    x = W.specs(B, seed)
    eng.reserve_wrn_vjp(3)
    with torch.no_grad():
        free_logits, free = W.wrn_walk(net, x.double())
    for k in range(3):
        g = cotangent(B, 10 + k)
        got = eng.wrn_vjp(x.cuda(), g.cuda()).cpu()
        tape = _tape(eng, B)
        masks = [t > 0 for t in tape]
        ref, pin = W.pinned_vjp(net, x, g, masks)
        err = W.relmax(got, ref)
        print('wrn_vjp B=%d seed=%d k=%d relmax vs pinned float64 = %.3e' % (B, seed, k, err))
        assert err <= W.VJP_TOL, (k, err)
        if k:
            continue                                     # the tape does not depend on the cotangent: checked once per input
        worst, differing = 0.0, 0
        for j in range(25):
            e_j = W.relmax(tape[j], pin['maps'][j].detach())
            worst = max(worst, e_j)
            assert e_j <= W.FP32_TOL, (j, e_j)
            top = float(free['maps'][j].abs().max())
            d = masks[j] != free['masks'][j]
            differing += int(d.sum())
            assert bool((free['pre'][j].abs()[d] <= 2 * W.FP32_TOL * top).all()), (j, float(free['pre'][j].abs()[d].max()) / top)
        print('wrn_vjp B=%d seed=%d worst tape map error %.3e, %d decisions differ from the free float64 walk' % (B, seed, worst, differing))
        W.mask_conditions(masks)                         # non-vacuity, on the engine's own decisions


# ---- 5. forward bits ------------------------------------------------------------------------------------------------------------------
def test_forward_bits(eng):
    x = W.specs(5, 2).cuda()
    eng.reserve_wrn_vjp(5)
    _, lg = eng.wrn_vjp(x, cotangent(5, 2).cuda(), want_logits=True)
    tier0 = eng.classify_tier(x, 0)
    assert torch.equal(lg, tier0) and torch.equal(eng.classify(x), tier0)
    assert torch.equal(eng.classify_tier(x, 1), tier0) and torch.equal(eng.classify_tier(x, 2), tier0)      # every tier falls to fp32
    for j in (0, 4):
        assert torch.equal(eng.classify(x[j:j + 1]), tier0[j:j + 1]), j
    big = W.specs(11, 7).cuda()                            # more than max_batch = 8: chunked, the same bits
    whole = eng.classify(big)
    assert torch.equal(whole[8:], eng.classify(big[8:])) and torch.equal(whole[3:4], eng.classify(big[3:4]))
    with np.load(GOLDEN) as z:
        spec, ref = torch.from_numpy(z['spec_in']), z['logits']
    err = W.relmax(eng.classify(spec.cuda()).cpu().numpy(), ref)
    print('engine logits vs the reference fixture: relmax %.3e' % err)
    assert err < 2e-4, err


# ---- 6. determinism, batch independence, passes ---------------------------------------------------------------------------------------
def test_determinism_batch_independence_and_passes(eng, sd):
    E = _E()
    x, g = W.specs(7, 3).cuda(), cotangent(7, 3).cuda()
    eng.reserve_wrn_vjp(7)
    a, b = eng.wrn_vjp(x, g), eng.wrn_vjp(x, g)
    assert torch.equal(a, b)
    for j in (0, 4, 6):
        assert torch.equal(eng.wrn_vjp(x[j:j + 1], g[j:j + 1]), a[j:j + 1]), j
    with pytest.raises(E.DmadError, match='one-pass'):
        eng.wrn_vjp_tape(0, 2)                           # the last call held one row
    small = E.Engine(max_batch=8, precision=E.FP32, with_wavenet=False)      # a reservation cannot shrink: its own engine
    try:
        small.load_wideresnet28_10(sd)
        small.reserve_wrn_vjp(2)
        got, lg = small.wrn_vjp(x[:5], g[:5], want_logits=True)                # three passes, the last partial
        assert small.wrn_vjp_batch == 2
        with pytest.raises(E.DmadError, match='one-pass'):
            small.wrn_vjp_tape(0, 1)                     # more than one pass: no tape to read
        small.reserve_wrn_vjp(5)
        whole, lg5 = small.wrn_vjp(x[:5], g[:5], want_logits=True)
        assert torch.equal(got, whole) and torch.equal(lg, lg5)
        assert torch.equal(whole, a[:5])                 # ... and the same bits as under the other engine's reservation of 7
    finally:
        small.close()


# ---- 7. finite difference -------------------------------------------------------------------------------------------------------------
def test_finite_difference(eng, sd):
    """sum g (f(x + h d) - f(x - h d)) / 2h on the engine's own tier-0 forward against sum g_spec d, with the step and the tolerance of the
    VGG19_bn and ResNeXt29 tests (h = 1e-3, 2 %) and their directions, for their reasons: along d = sign of a gradient every pixel moves
    by h and the signal is |g_spec|_1, far above the quotient's absolute errors (crossed ReLU kinks, fp32 rounding of the logits over 2h);
    a Gaussian d leaves a signal of the size of |g_spec|_2 only.  One direction is the sign of the float64 gradient of the free walk (no
    engine in it), the other the sign of the engine's own gradient: a wrong g_spec gives a wrong pattern AND a wrong sum."""
    x, g = W.specs(2, 6), cotangent(2, 6)
    xr = x.double().requires_grad_(True)
    (g64,) = torch.autograd.grad((W.wrn_walk(W.sd64(sd), xr)[0] * g.double()).sum(), xr)
    x, g = x.cuda(), g.cuda()
    gx = eng.wrn_vjp(x, g).view(2, 1, 32, 32)
    own = torch.sign(gx)
    own[own == 0] = 1.0
    h = 1e-3
    for name, d in (('float64 sign', torch.sign(g64).float().cuda()), ('engine sign', own)):
        fd = ((eng.classify_tier(x + h * d, 0) - eng.classify_tier(x - h * d, 0)) * g).sum() / (2 * h)
        an = (gx * d).sum()
        print('finite difference along the %s: %.6e against %.6e' % (name, float(fd), float(an)))
        assert abs(float(fd) - float(an)) <= 2e-2 * abs(float(an)), (name, float(fd), float(an))


# ---- 8. every precision, reservations, refusals ---------------------------------------------------------------------------------------
_BITS = {}


@pytest.mark.parametrize('prec', ['FP32', 'EXACT', 'BF16'])
def test_every_precision_and_refusals(sd, prec):
    E = _E()
    kw = {'recheck_batch': 4} if prec == 'EXACT' else {}
    e = E.Engine(max_batch=4, precision=getattr(E, prec), with_wavenet=False, **kw)
    try:
        with pytest.raises(E.DmadError):
            e.reserve_wrn_vjp(2)                         # no classifier loaded yet
        e.load_wideresnet28_10(sd)
        assert e.has_classifier and e.classifier_kind == 'wideresnet28_10'
        e.wrn_vjp_batch = 1                              # past the host's on-demand reservation: the library's own refusal
        with pytest.raises(E.DmadError, match='dmad_reserve_wrn_vjp'):
            e.wrn_vjp(W.specs(1, 0).cuda(), cotangent(1, 0).cuda())
        e.wrn_vjp_batch = 0
        vjp_reservation.check(e, e.reserve_wrn_vjp, vjp_reservation.grow(e, e.reserve_wrn_vjp, (1, 2, 3), []))
        e.reserve_wrn_vjp(9)                             # capped at max_batch
        x, g = W.specs(3, 11).cuda(), cotangent(3, 11).cuda()
        gx, lg = e.wrn_vjp(x, g, want_logits=True)
        assert torch.equal(lg, e.classify_tier(x, 0)) and torch.equal(lg, e.classify(x))
        assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
        first = _BITS.setdefault('first', (gx.cpu(), lg.cpu()))                 # the fp32 images serve all three precisions: the same bits
        assert torch.equal(first[0], gx.cpu()) and torch.equal(first[1], lg.cpu())
        # the other classifiers' VJPs name the right export
        with pytest.raises(E.DmadError, match='dmad_wrn_vjp'):
            e.reserve_vgg_vjp(2)
        with pytest.raises(E.DmadError, match='dmad_wrn_vjp'):
            e.reserve_classifier_vjp(2)
        # the vote loops: no recheck bound has been measured for this classifier
        clip = clips([0])[0].cuda()
        coef = [[0.1, 0.2]] * 5
        if prec == 'EXACT':
            assert e.mode == E.MODE_EXACT_VOTES
            for call in (lambda: e.smooth_votes(clip, 0.5, 0.9, 3, 1.0, 0.1, 4),
                         lambda: e.eval_samples(clip, 0.5, 0.9, 3, 1.0, 0.1, torch.arange(2).cuda()),
                         lambda: e.spec_smooth_votes(clip, 0.5, 1, 0.9, 0.1, *coef, -80.0, 0.0, 4),
                         lambda: e.spec_eval_samples(clip, 0.5, 1, 0.9, 0.1, *coef, -80.0, 0.0, torch.arange(2).cuda(), 0)):
                with pytest.raises(E.DmadError, match='no recheck bound has been measured for WideResNet-28-10'):
                    call()
            with pytest.raises(E.DmadError, match='no recheck bound'):
                e.set_recheck_margin(0.5)                # no committed margin to inherit
            e.set_mode(E.MODE_FP32)
        with pytest.raises(E.DmadError, match='UNet weights are not finalised'):      # outside the exact-vote mode the loops go on (to the
            e.spec_smooth_votes(clip, 0.5, 1, 0.9, 0.1, *coef, -80.0, 0.0, 4)          # missing UNet here, refused before any launch)
    finally:
        e.close()


def test_other_engines_refuse_and_bad_geometry():
    E = _E()
    r = E.Engine(max_batch=4, precision=E.FP32, with_wavenet=False)
    try:
        bad = {k: v for k, v in E.fold_wideresnet_state_dict(synth.wideresnet28_10_state_dict(W.WRN_SEED)).items()}
        bad['wrn.b4.short.w'] = bad['wrn.b4.short.w'].T.copy()                   # [160, 320]: the right size, the wrong shape
        with pytest.raises(E.DmadError, match=r"\(-4\).*wrn.b4.short.w"):         # DMAD_ERR_SHAPE
            r._load(bad)
        r.load_vgg19_bn(synth.vgg19_bn_state_dict(4321))                         # the refused set left nothing behind
        with pytest.raises(E.DmadError, match='VGG19_bn'):
            r.reserve_wrn_vjp(2)
        r.wrn_vjp_batch = 2
        with pytest.raises(E.DmadError, match='dmad_vgg_vjp'):
            r.wrn_vjp(W.specs(1, 0).cuda(), cotangent(1, 0).cuda())
    finally:
        r.close()


# ---- 9. the module, the query path and the drivers ------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def wrn(eng, sd):
    from audio_models.ConvNets_SpeechCommands.models import create_model
    m = create_model('wideresnet28_10', 10, 1)
    m.load_state_dict(W.sd32(sd))
    return m.cuda().eval().bind_engine(eng)


def test_module_backends(eng, wrn, monkeypatch):
    from dmad_hip import autograd as ag
    x = W.specs(3, 12).cuda()
    with torch.no_grad():
        assert torch.equal(wrn(x), eng.classify(x))
        assert W.relmax(wrn.torch_forward(x).cpu(), eng.classify(x).cpu()) < 2e-4
    g = cotangent(3, 4).cuda()
    grads = {}
    try:
        for backend in ('hip', 'torch', 'auto'):
            wrn.grad_backend = backend
            if backend == 'auto':
                monkeypatch.setattr(ag, 'wrn_hip', lambda *a: (_ for _ in ()).throw(AssertionError('auto must not reach wrn_hip')))
            xg = x.clone().requires_grad_(True)
            (grads[backend],) = torch.autograd.grad((wrn(xg) * g).sum(), xg)
            wrn.zero_grad(set_to_none=True)
        assert torch.equal(grads['hip'].view(3, 32, 32), eng.wrn_vjp(x, g))
        assert all(p.grad is None for p in wrn.parameters())
        # the torch layers take their own ReLU decisions (two flips out of 4.6 million move this gradient by 3.5e-3 of its maximum), so
        # their gradient is not compared number by number: test_wrn_vjp_against_pinned_float64 is the check of the values
        assert all(bool(torch.isfinite(grads[k]).all()) and float(grads[k].abs().max()) > 0 for k in grads)
        print('hip vs torch layers: relmax %.3e' % W.relmax(grads['hip'].cpu(), grads['torch'].cpu()))
        xg = x.clone().requires_grad_(True)
        wrn.grad_backend = 'hip'
        monkeypatch.undo()
        with pytest.raises(_E().DmadError, match='first-order only'):
            torch.autograd.grad((wrn(xg) * g).sum(), xg, create_graph=True)
    finally:
        wrn.grad_backend = 'auto'


def test_query_is_one_call(eng, wrn, monkeypatch):
    """AcousticSystem.query with the mel front-end and the WideResNet on one engine: the one-call path (sampler 0), equal to the stages"""
    from acoustic_system import AcousticSystem
    from dmad_hip.transforms import MelSpectrogramDB
    system = AcousticSystem(classifier=wrn, transform=MelSpectrogramDB(eng), defender=None).eval()
    x = clips(range(3)).unsqueeze(1).cuda()
    assert system._engine_chain(True) == (eng, 0)
    monkeypatch.setattr(system, 'forward', lambda *a, **k: (_ for _ in ()).throw(AssertionError('query must not loop over forward')))
    logits, dec = system.query(x, 2)
    want = eng.classify(eng.mel_db(x))
    assert tuple(logits.shape) == (2, 3, 10) and torch.equal(logits[0], want) and torch.equal(logits[1], want)
    assert torch.equal(dec[0], want.argmax(1))
    # sampler 4: a baseline waveform defense on the engine in front of it (dmad_defense_query_logits)
    from transforms.time_defense import TimeDomainDefense
    den = TimeDomainDefense('AS', backend='hip', engine=eng)
    smooth = AcousticSystem(classifier=wrn, transform=MelSpectrogramDB(eng), defender=den).eval()
    assert smooth._engine_chain(True) == (eng, 4)
    monkeypatch.setattr(smooth, 'forward', lambda *a, **k: (_ for _ in ()).throw(AssertionError('query must not loop over forward')))
    logits4, _ = smooth.query(x, 1)
    want4 = eng.classify(eng.mel_db(eng.wave_smooth(x, 0, den.engine_defense(x)['window'])))
    assert torch.equal(logits4[0], want4) and not torch.equal(want4, want)


@pytest.fixture(scope='module')
def purifier_eng(sd):
    """one FP32 engine that holds the WideResNet beside the DiffWave purifier's synthetic WaveNet"""
    E = _E()
    e = E.Engine(max_batch=4, precision=E.FP32)
    e.load_wavenet(synth.wavenet_state_dict(1234))
    e.load_wideresnet28_10(sd)
    yield e
    e.close()


def _bound(sd, e):
    from audio_models.ConvNets_SpeechCommands.models import create_model
    m = create_model('wideresnet28_10', 10, 1)
    m.load_state_dict(W.sd32(sd))
    return m.cuda().eval().bind_engine(e)


def test_query_with_the_diffwave_purifier_is_one_call(purifier_eng, sd, monkeypatch):
    """sampler 1: DiffWave on device noise in front of mel dB -> WideResNet on one engine is ONE dmad_query_logits call (6 rows on
    max_batch 4: chunked inside it, the purifier and the classifier sharing the slab and the logits buffer), equal bit for bit to the
    staged computation ddpm_purify -> mel_db -> classify with the same Philox keys"""
    from acoustic_system import AcousticSystem
    from diffusion_models.diffwave_ddpm import DiffWave, WaveNetHIP
    from diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams
    from dmad_hip.transforms import MelSpectrogramDB
    e = purifier_eng
    wrn = _bound(sd, e)
    den = DiffWave(WaveNetHIP(e), calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG), reverse_timestep=2, seed=17)
    system = AcousticSystem(classifier=wrn, transform=MelSpectrogramDB(e), defender=den, defense_type='wave').eval()
    assert system._engine_chain(True) == (e, 1) and system._engine_chain(False) == (e, 0)
    x = clips([0, 5]).unsqueeze(1).cuda()
    B, R = 2, 3
    calls = []
    real = e.query_logits
    monkeypatch.setattr(e, 'query_logits', lambda *a, **k: (calls.append(a[1]), real(*a, **k))[1])
    monkeypatch.setattr(system, 'forward', lambda *a, **k: (_ for _ in ()).throw(AssertionError('query must not loop over forward')))
    den._draws = 100
    logits, dec = system.query(x, repeats=R)
    assert calls == [R] and den._draws == 100 + R * B and tuple(logits.shape) == (R, B, 10) and torch.equal(dec, logits.argmax(-1))
    ts, c_a, c_b, c_eps, c_div, c_sig = den.purify_coefficients()
    pur = e.ddpm_purify(x.repeat(R, 1, 1), ts, c_a, c_b, c_eps, c_div, c_sig, seed=17, sample0=100)
    staged = torch.cat([e.classify(e.mel_db(pur[i:i + 4])) for i in (0, 4)])
    assert torch.equal(logits.reshape(R * B, 10), staged)
    assert not torch.equal(logits[0], logits[1])                    # fresh noise per repeat
    one, _ = real(x[1:2], 1, 1, ts, c_a, c_b, c_eps, c_div, c_sig, seed=17, sample0=100 + 2 * B + 1)
    assert torch.equal(one, logits[2, 1:2])                         # row (2, 1) alone, by its key


def test_query_with_the_spec_purifier_is_one_call(sd, monkeypatch):
    """sampler 3: mel dB -> SpecPurifier (the engine's UNet) -> WideResNet on one engine is ONE dmad_spec_query_logits call (6 rows on
    max_batch 4).  The staged computation is dmad_spec_eval_samples on each clip alone (sigma = 0: the clip itself; the rows' Philox keys;
    the fp32 UNet tier), which hands back the purified spectrograms as well: the query's logits equal its logits bit for bit (a row's
    result does not depend on how the rows were batched: SpecPurifier's contract), and those equal the classifier run on the purified
    spectrograms by itself."""
    from acoustic_system import AcousticSystem
    from diffusion_models.improved_diffusion_ddpm import SpecPurifier, create_improved_diffusion
    from diffusion_models.Improved_Diffusion_Unconditional.improved_diffusion.sc09_spectrogram_dataset import MEL_LOWER_BOUND, MEL_UPPER_BOUND
    from dmad_hip.transforms import MelSpectrogramDB
    E = _E()
    e = E.Engine(max_batch=4, precision=E.FP32, with_wavenet=False)
    try:
        pur = create_improved_diffusion(None, reverse_timestep=3, state_dict=synth.unet_state_dict(31), engine=e)
        wrn = _bound(sd, e)
        den = SpecPurifier(pur, seed=23)
        system = AcousticSystem(classifier=wrn, transform=MelSpectrogramDB(e), defender=den, defense_type='spec').eval()
        assert system._engine_chain(True) == (e, 3) and system._engine_chain(False) == (e, 0)
        x = clips([1, 7]).unsqueeze(1).cuda()
        B, R = 2, 3
        calls = []
        real = e.spec_query_logits
        monkeypatch.setattr(e, 'spec_query_logits', lambda *a, **k: (calls.append(a[1]), real(*a, **k))[1])
        monkeypatch.setattr(system, 'forward', lambda *a, **k: (_ for _ in ()).throw(AssertionError('query must not loop over forward')))
        den._draws = 40
        logits, dec = system.query(x, repeats=R)
        assert calls == [R] and den._draws == 40 + R * B and tuple(logits.shape) == (R, B, 10)
        assert torch.equal(dec, logits.argmax(-1)) and bool(torch.isfinite(logits).all())
        assert not torch.equal(logits[0], logits[1])                # fresh noise per repeat
        coef = pur.purify_coefficients()
        for b in range(B):
            keys = torch.tensor([40 + r * B + b for r in range(R)]).cuda()
            lg, spec = e.spec_eval_samples(x[b], 0.0, *coef, MEL_LOWER_BOUND, MEL_UPPER_BOUND, keys, 0, seed=23, want_spec=True)
            assert torch.equal(lg, logits[:, b]), b
            assert torch.equal(e.classify(spec), lg), b
    finally:
        e.close()


@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory, sd):
    """ten one-clip classes and a pickled DataParallel(WideResNet) under the reference's module path"""
    import wave
    from audio_models.ConvNets_SpeechCommands.create_model import create_model  # noqa: F401  (makes `models` importable)
    from models.wideresnet import WideResNet
    from datasets.sc_dataset import SC09_CLASSES
    root = tmp_path_factory.mktemp('wrn')
    data = root / 'test'
    for i, c in enumerate(SC09_CLASSES[:10]):
        (data / c).mkdir(parents=True)
        pcm = (synth.synthetic_clip(i).reshape(-1) * 32767).astype('<i2')
        with wave.open(str(data / c / 'a.wav'), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(pcm.tobytes())
    ck = root / 'ConvNets_SpeechCommands'
    ck.mkdir()
    net = WideResNet(depth=28, widen_factor=10, dropRate=0, num_classes=10, in_channels=1)
    net.load_state_dict(W.sd32(sd))
    torch.save(torch.nn.DataParallel(net), str(ck / 'wideresnet28_10.pth'))
    return str(data), str(ck / 'wideresnet28_10.pth')


@pytest.mark.parametrize('driver,flags,over', [
    ('adaptive_attack_eval', ['--defense', 'None', '--max_iter_1', '2'], {}),
    ('black_box_attack_eval', ['--attack', 'FAKEBOB', '--defense', 'None'], dict(max_iter=2, samples_per_draw=4)),
    ('siren_attack_eval', ['--attack', 'SirenAttack', '--defense', 'None'], dict(max_epoch=1, max_iter=2, n_particles=3)),
    ('baseline_defense_eval', ['--attack', 'FAKEBOB', '--defense', 'AS', '--defense_backend', 'hip'], dict(max_iter=2, samples_per_draw=4)),
    ('imperceptible_attack_eval', ['--max_iter_1', '2', '--max_iter_2', '3'], {}),
])
def test_drivers_take_a_wideresnet_checkpoint(eng, checkpoint, driver, flags, over):
    import importlib
    from audio_models.ConvNets_SpeechCommands.create_model import create_model
    drv = importlib.import_module(driver)
    data, path = checkpoint
    args = drv.build_parser().parse_args(['--data_path', data, '--classifier_path', path, '--num_per_class', '1', '--batch_size', '4',
                                          '--dataload_workers_nums', '0', '--verbose', '0'] + flags)
    clf = create_model(args.classifier_path).cuda()
    assert type(clf).__name__ == 'WideResNet'
    clf.bind_engine(eng)
    out = drv.run(args, classifier=clf, log=lambda *a: None, **over)
    assert out['total'] == 10 and clf.grad_backend == 'hip'
    for k in ('clean_acc', 'denoised_acc', 'robust_acc'):
        assert np.isfinite(out[k]) and 0.0 <= out[k] <= 100.0, (driver, k, out[k])
