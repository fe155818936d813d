"""The VGG19_bn input VJP on the engine (dmad_reserve_vgg_vjp / dmad_vgg_vjp): its new kernels alone, the whole network against a
decision-pinned float64 reference (tests/vgg_vjp_cases.py), forward bits, determinism and batch independence, a finite difference,
every engine precision, the reservation and the refusals, and the module / driver switches built on it (VGG.grad_backend)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_ops_ref as R  # noqa: E402
import vgg_vjp_cases as V  # noqa: E402
import vjp_reservation  # noqa: E402
from dmad_hip import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def _E():
    from dmad_hip import engine as E
    return E


@pytest.fixture(scope='module')
def sd():
    return synth.vgg19_bn_state_dict(V.VGG_SEED)


@pytest.fixture(scope='module')
def eng(sd):
    E = _E()
    e = E.Engine(max_batch=8, precision=E.FP32, with_wavenet=False)
    e.load_vgg19_bn(sd)
    yield e
    e.close()


def clips(ids):
    return torch.from_numpy(np.stack([synth.synthetic_clip(i).reshape(-1) for i in ids])).float()


def cotangent(B, seed):
    return torch.randn(B, 10, generator=torch.Generator().manual_seed(seed))


# ---- 1. the new kernels alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,H,C', [(3, 4, 64), (2, 2, 512)])
def test_pool_relu_bwd_exact(B, H, C):
    """Small integers: the kernel's answer is exact, so it must equal the float64 reference bit for bit — the first maximum in scan order
    wins every tie, zero and negative windows hand back zeros (tests/test_vgg_vjp_cpu.py proves that the maps hold those cases)."""
    y, g = V.pool_case(B, H, C, seed=H)
    got = _E().vgg_pool_relu_bwd(g.cuda(), y.cuda()).cpu()
    ref = V.pool_relu_bwd_ref(g, y)
    assert torch.equal(got.double(), ref)
    won = V.windows(got.permute(0, 3, 1, 2)) != 0
    assert all(bool(won[..., p].any()) for p in range(4))
    assert torch.equal(_E().vgg_pool_relu_bwd(g[B - 1:].cuda(), y[B - 1:].cuda()).cpu(), got[B - 1:])


@pytest.mark.parametrize('B,H,C,with_mask', [(2, 4, 64, False), (2, 4, 64, True), (3, 2, 512, False), (3, 2, 512, True)])
def test_form3_vs_float64_autograd(B, H, C, with_mask):
    """dmad_conv_f32_vjp form 3 (pack -> mask -> GEMM): the packed image exactly, the masked gradient exactly, the gradient against float64
    F.conv2d autograd within the fp32 tier's bound, and a sample's bits the same alone."""
    E = _E()
    g = torch.Generator().manual_seed(300 + B * H + C + with_mask)
    w = (torch.rand(1, 9, C, C, generator=g) * 2 - 1) * 0.1                      # [1][tap][M][K]
    scale = torch.rand(C, generator=g) + 0.5
    g_y = torch.rand(B, H, H, C, generator=g) * 2 - 1
    mask = None
    if with_mask:
        mask = torch.relu(torch.randn(B, H, H, C, generator=g))
        mask.view(-1)[::7] = -0.0
        mask.view(-1)[3::11] = -1.5
    gx, wT, gm, _ = E.conv_f32_vjp(g_y.cuda(), w.cuda(), H, form=3, scale=scale.cuda(), mask_y=None if mask is None else mask.cuda())
    want_wT = (w[0] * scale[None, :, None]).flip(0).permute(0, 2, 1).contiguous()        # wT[8 - t][k][m] = w[t][m][k] * scale[m]
    assert torch.equal(wT.cpu(), want_wT)
    gin = g_y
    if with_mask:
        gin = torch.where(mask > 0, g_y, torch.zeros_like(g_y))
        assert torch.equal(gm.cpu(), gin)
    x = torch.zeros(B, C, H, H, dtype=torch.float64, requires_grad=True)
    w64 = w[0].double().permute(1, 2, 0).reshape(C, C, 3, 3)                             # [M][K][ky][kx]
    yy = F.conv2d(x, w64, padding=1) * scale.double().reshape(1, C, 1, 1)
    (ref,) = torch.autograd.grad(yy, x, gin.double().permute(0, 3, 1, 2))
    err = R.rel(gx.cpu(), ref.permute(0, 2, 3, 1))
    print('form 3 B=%d H=%d C=%d mask=%d err/max|ref| = %.3e' % (B, H, C, with_mask, err))
    assert err < R.F32_TOL, err
    one = E.conv_f32_vjp(g_y[B - 1:].cuda(), w.cuda(), H, form=3, scale=scale.cuda(), mask_y=None if mask is None else mask[B - 1:].cuda())[0]
    assert torch.equal(one, gx[B - 1:])
    with pytest.raises(E.DmadError):
        E.conv_f32_vjp(g_y.cuda(), w.cuda(), H, form=3)                                  # form 3 carries a scale


# ---- 2. the whole network against the decision-pinned float64 reference -----------------------------------------------------------
def _tape(eng, B):
    t = [eng.vgg_vjp_tape(k, B).cpu() for k in range(18)]
    return [m.permute(0, 3, 1, 2).contiguous() for m in t[:16]] + t[16:]


@pytest.mark.parametrize('B,seed', [(2, 1), (3, 12)])
def test_vgg_vjp_against_pinned_float64(eng, sd, B, seed):
    """The engine's tape gives the decisions (ReLU masks, pool arg-maxes); the float64 walk pinned to them gives the gradient and the maps
    the engine must match, and the free float64 walk says how far from a kink every differing decision lies."""
    net = V.sd64(sd)
    x = V.specs(B, seed)
    eng.reserve_vgg_vjp(3)
    free_logits, free = V.vgg_walk(net, x.double())
    pool_in = V.pool_input_index()
    for k in range(3):
        g = cotangent(B, 10 + k)
        got = eng.vgg_vjp(x.cuda(), g.cuda()).cpu()
        tape = _tape(eng, B)
        masks, args = V.tape_decisions(tape)
        ref, pin = V.pinned_vjp(net, x, g, (masks, args))
        err = V.relmax(got, ref)
        print('vgg_vjp B=%d seed=%d k=%d relmax vs pinned float64 = %.3e' % (B, seed, k, err))
        assert err <= V.VJP_TOL, (k, err)
        if k:
            continue                                     # the tape does not depend on the cotangent: checked once per input
        worst = 0.0
        for j in range(18):
            e_j = V.relmax(tape[j], pin['maps'][j].detach())
            worst = max(worst, e_j)
            assert e_j <= V.FP32_TOL, (j, e_j)
        differing = 0
        for j in range(18):                              # a ReLU's margin is |pre-activation|
            top = float(free['maps'][j].abs().max())
            d = masks[j] != free['masks'][j]
            differing += int(d.sum())
            assert bool((free['pre'][j].abs()[d] <= 2 * V.FP32_TOL * top).all()), ('relu', j, float(free['pre'][j].abs()[d].max()) / top)
        for p in range(5):                               # a pool window's margin is its top-2 gap
            top = float(free['maps'][pool_in[p]].abs().max())
            d = args[p] != free['args'][p]
            differing += int(d.sum())
            assert bool((free['gaps'][p][d] <= 2 * V.FP32_TOL * top).all()), ('pool', p, float(free['gaps'][p][d].max()) / top)
        print('vgg_vjp B=%d seed=%d worst tape map error %.3e, %d decisions differ from the free float64 walk' % (B, seed, worst, differing))
        for j in range(16):                              # non-vacuity, on the engine's own decisions
            frac = float(masks[j].double().mean())
            assert 0.05 < frac < 0.95, (j, frac)
            assert not torch.equal(masks[j][0], masks[j][1]), j
        for p in range(5):
            assert sorted(np.unique(args[p].numpy()).tolist()) == [0, 1, 2, 3], p


# ---- 3. forward bits ----------------------------------------------------------------------------------------------------------
def test_forward_logits_bitwise(eng):
    x = V.specs(5, 2).cuda()
    eng.reserve_vgg_vjp(5)
    _, lg = eng.vgg_vjp(x, cotangent(5, 2).cuda(), want_logits=True)
    assert torch.equal(lg, eng.classify_tier(x, 0))


# ---- 4. determinism, batch independence, passes -------------------------------------------------------------------------------------
def test_determinism_batch_independence_and_passes(eng, sd):
    E = _E()
    x, g = V.specs(7, 3).cuda(), cotangent(7, 3).cuda()
    eng.reserve_vgg_vjp(7)
    a, b = eng.vgg_vjp(x, g), eng.vgg_vjp(x, g)
    assert torch.equal(a, b)
    for j in (0, 4, 6):
        assert torch.equal(eng.vgg_vjp(x[j:j + 1], g[j:j + 1]), a[j:j + 1]), j
    with pytest.raises(E.DmadError):
        eng.vgg_vjp_tape(0, 2)                           # the last call held one row
    small = E.Engine(max_batch=8, precision=E.FP32, with_wavenet=False)      # a reservation cannot shrink: its own engine
    try:
        small.load_vgg19_bn(sd)
        small.reserve_vgg_vjp(2)
        got, lg = small.vgg_vjp(x[:5], g[:5], want_logits=True)                # three passes, the last partial
        assert small.vgg_vjp_batch == 2
        with pytest.raises(E.DmadError):
            small.vgg_vjp_tape(0, 1)                     # more than one pass: no tape to read
        small.reserve_vgg_vjp(5)
        whole, lg5 = small.vgg_vjp(x[:5], g[:5], want_logits=True)
        assert torch.equal(got, whole) and torch.equal(lg, lg5)
        assert torch.equal(whole, a[:5])                 # ... and the same bits as under the other engine's reservation of 7
    finally:
        small.close()


# ---- 5. finite difference -------------------------------------------------------------------------------------------------------
def test_finite_difference(eng, sd):
    """sum g (f(x + h d) - f(x - h d)) / 2h on the engine's own tier-0 forward against sum g_spec d; step and tolerance of the ResNeXt29
    test (h = 1e-3, 2 %).  The direction is d = sign of the float64 oracle gradient, the direction a sign-gradient attack steps along.
    A Gaussian d does not give a usable quotient on this network, on the CPU already: its signal sum g_spec d is of the size of |g_spec|_2
    (20.7 here) while the quotient's two errors are absolute — crossed ReLU / max-pool kinks (0.64, float64) and the fp32 rounding of
    logits up to 650 divided by 2h (0.49, fp32 torch) — so float64 is off by 3.1 % and fp32 torch by 5.4 % at h = 1e-3 (0.25 % / 16 %
    at 1e-4: no step serves both).  Along sign(g) every pixel moves by the same h and the signal is |g_spec|_1 (1058): float64 lands at
    0.15 % and fp32 torch at 0.18 %, a tenth of the bound.  A second direction does not come from the oracle: the sign of the engine's
    own gradient, a fixed +-1 pattern once computed, with the same signal (a wrong g_spec gives a wrong pattern AND a wrong sum, and the
    forward's quotient along it does not follow).  Random +-1 patterns are no alternative: four of them on the CPU gave a quotient error
    of 0.5 - 1.4 in fp32 torch against signals of 10 - 29, 2.5 - 8.6 %."""
    from oracle import dmad_oracle as orc
    x, g = V.specs(2, 6), cotangent(2, 6)
    xr = x.double().requires_grad_(True)
    (g64,) = torch.autograd.grad((orc.vgg19_bn_forward(V.sd64(sd), xr) * g.double()).sum(), xr)
    x, g = x.cuda(), g.cuda()
    gx = eng.vgg_vjp(x, g).view(2, 1, 32, 32)
    own = torch.sign(gx)
    own[own == 0] = 1.0
    h = 1e-3
    for name, d in (('oracle sign', torch.sign(g64).float().cuda()), ('engine sign', own)):
        fd = ((eng.classify_tier(x + h * d, 0) - eng.classify_tier(x - h * d, 0)) * g).sum() / (2 * h)
        an = (gx * d).sum()
        print('finite difference along the %s: %.6e against %.6e' % (name, float(fd), float(an)))
        assert abs(float(fd) - float(an)) <= 2e-2 * abs(float(an)), (name, float(fd), float(an))


# ---- 6. every precision, reservations, refusals -------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['FP32', 'EXACT', 'BF16'])
def test_every_precision_and_refusals(sd, prec):
    E = _E()
    kw = {'recheck_batch': 4} if prec == 'EXACT' else {}
    e = E.Engine(max_batch=4, precision=getattr(E, prec), with_wavenet=False, **kw)
    try:
        with pytest.raises(E.DmadError):
            e.reserve_vgg_vjp(2)                         # no classifier loaded yet
        e.load_vgg19_bn(sd)
        e.vgg_vjp_batch = 1                              # past the host's on-demand reservation: the library's own refusal
        with pytest.raises(E.DmadError, match='dmad_reserve_vgg_vjp'):
            e.vgg_vjp(V.specs(1, 0).cuda(), cotangent(1, 0).cuda())
        e.vgg_vjp_batch = 0
        vjp_reservation.check(e, e.reserve_vgg_vjp, vjp_reservation.grow(e, e.reserve_vgg_vjp, (1, 2, 3), []))
        e.reserve_vgg_vjp(9)                             # capped at max_batch
        x, g = V.specs(3, 11).cuda(), cotangent(3, 11).cuda()
        gx, lg = e.vgg_vjp(x, g, want_logits=True)
        assert torch.equal(lg, e.classify_tier(x, 0)) and bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    finally:
        e.close()


def test_resnext_engine_refuses():
    E = _E()
    r = E.Engine(max_batch=4, precision=E.FP32, with_wavenet=False)
    try:
        r.load_resnext29(synth.resnext29_state_dict(2929))
        with pytest.raises(E.DmadError, match='ResNeXt29'):
            r.reserve_vgg_vjp(2)
        r.vgg_vjp_batch = 2                              # past the host's on-demand reservation: the library's own refusal
        with pytest.raises(E.DmadError, match='ResNeXt29'):
            r.vgg_vjp(V.specs(1, 0).cuda(), cotangent(1, 0).cuda())
    finally:
        r.close()


# ---- 7. modules and the driver ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def vgg(eng, sd):
    from audio_models.ConvNets_SpeechCommands.models.vgg import vgg19_bn
    m = vgg19_bn(num_classes=10, in_channels=1)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.cuda().eval().bind_engine(eng)


def _ce_grad(vgg, mel, x, y):
    xg = x.clone().requires_grad_(True)
    loss = F.cross_entropy(vgg(mel(xg)), y)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    (g,) = torch.autograd.grad(loss, xg)
    torch.cuda.synchronize()
    return g, torch.cuda.max_memory_allocated()


def test_module_hip_backend_is_the_engine_vjp(eng, vgg, monkeypatch):
    from dmad_hip import autograd as ag
    from dmad_hip.transforms import MelSpectrogramDB
    x = clips([0, 1, 2, 3]).unsqueeze(1).cuda()
    y = torch.tensor([1, 3, 5, 7]).cuda()
    mel = MelSpectrogramDB(eng, grad_backend='hip')
    vgg.grad_backend = 'hip'
    try:
        g_h, peak_h = _ce_grad(vgg, mel, x, y)
        assert all(p.grad is None for p in vgg.parameters())
        # by hand: the cross-entropy's own gradient at the engine's tier-0 logits, then the two VJPs
        spec = eng.mel_db(x)
        lg = eng.classify_tier(spec, 0).requires_grad_(True)
        (g_lg,) = torch.autograd.grad(F.cross_entropy(lg, y), lg)
        by_hand = eng.mel_db_vjp(x, eng.vgg_vjp(spec, g_lg))
        assert torch.equal(g_h.reshape(by_hand.shape), by_hand)
        vgg.grad_backend = 'torch'
        g_t, peak_t = _ce_grad(vgg, mel, x, y)
        vgg.zero_grad(set_to_none=True)
        print('peak torch memory over the backward: hip %d B, torch %d B' % (peak_h, peak_t))
        assert peak_h < peak_t                            # no torch activation of the classifier is kept or made
        assert bool(torch.isfinite(g_t).all())
        vgg.grad_backend = 'auto'                        # 'auto' still runs the module's layers
        monkeypatch.setattr(ag, 'vgg_hip', lambda *a: (_ for _ in ()).throw(AssertionError('auto must not reach vgg_hip')))
        g_a, _ = _ce_grad(vgg, mel, x, y)
        assert torch.equal(g_a, g_t) or V.relmax(g_a.cpu(), g_t.cpu()) <= V.VJP_TOL      # MIOpen may pick another algorithm
    finally:
        vgg.grad_backend = 'auto'
        vgg.zero_grad(set_to_none=True)


def test_attack_and_driver_front(eng, vgg):
    import adaptive_attack_eval as drv
    from acoustic_system import AcousticSystem
    from dmad_hip.transforms import MelSpectrogramDB
    from robustness_eval.white_box_attack import AudioAttack
    vgg.grad_backend = 'hip'
    try:
        system = AcousticSystem(classifier=vgg, transform=MelSpectrogramDB(eng, grad_backend='hip'), defender=None).eval()
        x = clips(range(3)).unsqueeze(1).cuda()
        with torch.no_grad():
            y = system(x).argmax(1)
        runs = []
        for _ in range(2):
            att = AudioAttack(system, eps=65, max_iter_1=3, max_iter_2=0)
            x_adv, _ = att.generate(x, y, targeted=False)
            runs.append(x_adv)
        d = runs[0] - x
        assert float(d.abs().max()) <= 65 * 2 ** -15 + 1e-6 and float(runs[0].abs().max()) <= 1.0      # the linf ball and the box
        assert float(d.abs().max()) > 0
        assert torch.equal(runs[0], runs[1])
    finally:
        vgg.grad_backend = 'auto'
    clf, mel = drv.build_front(drv.build_parser().parse_args([]), classifier=vgg)
    try:
        assert clf is vgg and clf.grad_backend == 'hip' and mel.grad_backend == 'hip'
    finally:
        vgg.grad_backend = 'auto'
