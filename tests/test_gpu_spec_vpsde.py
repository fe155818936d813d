"""The reverse VP-SDE spectrogram purifier on the engine (dmad_spec_vpsde_purify / dmad_spec_vpsde_purify_vjp;
diffusion_models.improved_diffusion_sde.RevImprovedDiffusion), on the full-geometry synthetic UNet.

h q is 0.006-0.011 per step, so the eps term is about 1 % of the output and of the gradient: every accuracy check subtracts the chain's
linear part first — the chain with eps = 0 for outputs, c_a prod(1 + h beta/2) g_out for gradients — and measures the remainder
relative to its own max.  The CPU oracle chain runs oracle.unet_forward with the engine's Philox draws."""
import types

import numpy as np
import pytest
import torch

from dmad_hip import synth

pytestmark = pytest.mark.gpu

SEED = 5252


def relmax(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / np.abs(ref).max()


@pytest.fixture(scope='module')
def sde():
    from diffusion_models import improved_diffusion_sde
    return improved_diffusion_sde


@pytest.fixture(scope='module')
def orc():
    from oracle import dmad_oracle
    return dmad_oracle


@pytest.fixture(scope='module')
def sd():
    return synth.unet_state_dict(SEED)


def unet_engine(sd, precision, max_batch=8, **kw):
    from diffusion_models.improved_diffusion_ddpm import create_improved_diffusion
    from dmad_hip import engine as E
    e = E.Engine(max_batch=max_batch, precision=precision, with_wavenet=False, **kw)
    create_improved_diffusion(None, state_dict=sd, engine=e)
    return e


@pytest.fixture(scope='module')
def eng(sd):
    """exact-fp32 engine (max_batch 8) with the synthetic UNet and VGG19_bn."""
    from dmad_hip import engine as E
    e = unet_engine(sd, E.FP32)
    e.load_vgg19_bn(synth.vgg19_bn_state_dict(4321))
    yield e
    e.close()


def specs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, 32, 32, generator=g) * 1.6 - 0.8).float()


def spec_db(B, seed=0):
    return (specs(B, seed) * 40.0 - 40.0).cuda()             # mel-dB range of the standardisation


def make_args(t, **kw):
    a = dict(ddpm_path=None, t=t, score_type='guided_diffusion', sample_step=1, rand_t=False, t_delta=0, use_bm=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def draws(eng, sde, sch, B, seed, sample0):
    """The engine's Philox draws of a chain [S + 1, B, 1024] (slot 0 the diffusion draw)."""
    streams = [sde.SPEC_VPSDE_STREAM_DIFFUSE] + [sde.SPEC_VPSDE_STREAM_STEP0 + n for n in range(sch.steps)]
    return torch.stack([eng.philox_normal(seed, sample0, s, B)[:, :1024] for s in streams])


def oracle_chain(orc, sd, x0, sch, z, with_eps=True):
    """The chain on the CPU on oracle.unet_forward ([B, 1024] states), explicit draws z [S + 1, B, 1024]; differentiable in x0."""
    layout = synth.unet_layout()
    B = x0.shape[0]
    x = float(sch.c_a) * x0 + float(sch.c_b) * z[0]
    for n in range(sch.steps):
        drift = float(sch.hb[n]) * x
        if with_eps:
            eps = orc.unet_forward(sd, x.view(B, 1, 32, 32), torch.full((B,), int(sch.k[n])), layout).reshape(B, 1024)
            drift = drift - float(sch.q[n]) * eps
        x = x + drift * float(sch.h[n]) + float(sch.gs[n]) * z[n + 1]
    return x


@pytest.mark.parametrize('t', [2, 3])
def test_forward_against_oracle(eng, orc, sde, sd, t):
    sch = sde.spec_vpsde_schedule(t)
    B, S = 2, sch.steps
    x0 = specs(B, t).reshape(B, 1024)
    out, traj = eng.spec_vpsde_purify(x0.view(B, 32, 32).cuda(), sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs, seed=11,
                                      sample0=3, path=1, want_traj=True)
    z = draws(eng, sde, sch, B, 11, 3)
    zc = z.cpu()
    ref = oracle_chain(orc, sd, x0, sch, zc).double()
    lin = oracle_chain(orc, sd, x0.double(), sch, zc.double(), with_eps=False)
    got = out.reshape(B, 1024).cpu().double()
    assert float((ref - lin).abs().max()) > 1e-3 * float(lin.abs().max())          # the eps part is there to be measured
    assert relmax(got - lin, ref - lin) <= 1e-4, relmax(got - lin, ref - lin)
    # the trajectory: slot 0 the diffusion, slot S the output, every slot the oracle's state entering that step
    tr = traj.view(S + 1, B, 1024)
    assert torch.equal(tr[S], out.reshape(B, 1024))
    assert relmax(tr[0].cpu(), sch.c_a * x0.double() + sch.c_b * zc[0].double()) <= 1e-6
    for n in range(1, S):
        st = oracle_chain(orc, sd, x0, sde.VPSDESchedule(*(a[:n] for a in sch[:5]), sch.c_a, sch.c_b), zc)
        assert relmax(tr[n].cpu(), st) <= 1e-5, n
    # explicit draws are the Philox draws bit for bit; the FP32 engine's path 0 is its exact-fp32 tier
    a = (x0.view(B, 32, 32).cuda(), sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs)
    assert torch.equal(eng.spec_vpsde_purify(*a, z=z), out)
    assert torch.equal(eng.spec_vpsde_purify(*a, seed=11, sample0=3), out)


def test_exact_engine_tiers(sd, sde, orc):
    from dmad_hip import engine as E
    sch = sde.spec_vpsde_schedule(3)
    ex = unet_engine(sd, E.EXACT, max_batch=4, recheck_batch=4, with_classifier=False)
    try:
        x0 = specs(2, 8).cuda()
        z = draws(ex, sde, sch, 2, 4, 0)
        a = (x0, sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs)
        p0 = ex.spec_vpsde_purify(*a, z=z).reshape(2, 1024).cpu().double()
        p1 = ex.spec_vpsde_purify(*a, z=z, path=1).reshape(2, 1024).cpu().double()
    finally:
        ex.close()
    lin = oracle_chain(orc, sd, x0.reshape(2, 1024).cpu().double(), sch, z.cpu().double(), with_eps=False)
    assert relmax(p0 - lin, p1 - lin) <= 1e-4, relmax(p0 - lin, p1 - lin)
    assert not torch.equal(p0, p1)                                        # two tiers did run


@pytest.mark.parametrize('t', [2, 3])
def test_full_gradient_against_oracle(eng, orc, sde, sd, t):
    """'hip' through the standardisation (RevImprovedDiffusion) against CPU autograd of the oracle chain on the same draws."""
    den = sde.RevImprovedDiffusion(make_args(t), state_dict=sd, engine=eng, seed=29)
    s, w = spec_db(2, 9 + t), spec_db(2, 20 + t) / 40.0
    den._draws = 4
    sr = s.clone().requires_grad_(True)
    (g,) = torch.autograd.grad((den(sr) * w).sum(), sr)
    assert den._draws == 6
    sch = den.schedule()
    z = draws(eng, sde, sch, 2, 29, 4).cpu()
    sc = s.cpu().clone().requires_grad_(True)
    x = oracle_chain(orc, sd, orc.melspec_standardize(sc).reshape(2, 1024), sch, z)
    (gr,) = torch.autograd.grad((orc.melspec_inv_standardize(x).reshape(2, 1, 32, 32) * w.cpu()).sum(), sc)
    lin = sch.linear_gain() * w.cpu().double()
    gr, g = gr.double(), g.cpu().double()
    assert float((gr - lin).abs().max()) > 1e-3 * float(lin.abs().max())
    assert np.isfinite(g.numpy()).all() and relmax(g - lin, gr - lin) <= 1e-3, relmax(g - lin, gr - lin)


def test_full_gradient_directional_finite_difference(eng, sde):
    sch = sde.spec_vpsde_schedule(5)
    eng.reserve_unet_vjp(2)
    x0 = specs(1, 4).cuda()
    g_out = torch.randn(x0.shape, generator=torch.Generator().manual_seed(31)).cuda()
    a = (sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs)
    _, traj = eng.spec_vpsde_purify(x0, *a, seed=5, sample0=11, path=1, want_traj=True)
    g = eng.spec_vpsde_purify_vjp(traj, sch.c_a, sch.k, sch.h, sch.hb, sch.q, g_out).double()
    gain = sch.linear_gain()
    go = g_out[:, 0].double()
    rem = g - gain * go                                     # the eps part of the gradient: the direction that tests it
    v = (rem / rem.norm()).float().view(x0.shape)
    h = 1e-2

    def f(x):                                               # fixed Philox keys: the same draws at every evaluation
        return float((go * eng.spec_vpsde_purify(x, *a, seed=5, sample0=11, path=1).double()).sum())
    fd = (f(x0 + h * v) - f(x0 - h * v)) / (2 * h) - gain * float((go * v[:, 0].double()).sum())
    want = float((rem * v[:, 0].double()).sum())
    assert abs(fd - want) <= 0.01 * abs(want), (fd, want)


def test_hip_against_torch(eng, sde, sd):
    den = sde.RevImprovedDiffusion(make_args(3), state_dict=sd, engine=eng, seed=8)
    s, w = spec_db(3, 40), spec_db(3, 41) / 40.0
    res = {}
    for mode in ('none', 'hip', 'torch'):
        den.score_grad = mode
        den._draws = 0
        sr = s.clone().requires_grad_(True)
        out = den(sr)
        (g,) = torch.autograd.grad((out * w).sum(), sr)
        res[mode] = (out.detach().double().cpu(), g.double().cpu())
    part = res['hip'][1] - res['none'][1]
    assert float(part.abs().max()) > 1e-3 * float(res['none'][1].abs().max())
    d = float((res['hip'][1] - res['torch'][1]).abs().max()) / float(part.abs().max())
    assert d <= 1e-5, d
    assert relmax(res['torch'][0], res['hip'][0]) <= 1e-6


def test_deterministic_and_batch_independent(sd, sde):
    """Bits across calls, and a spectrogram alone == inside a batch when the sample keys match; B = 3 runs in Python chunks of 2 + 1
    (max_batch 2) for the forward and in library passes of 2 + 1 (reservation 2) for the gradient."""
    from dmad_hip import engine as E
    sch = sde.spec_vpsde_schedule(3)
    a = (sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs)
    x0 = specs(3, 12).cuda()
    g_out = torch.randn(x0.shape, generator=torch.Generator().manual_seed(3)).cuda()
    results = {}
    for mb in (2, 4):
        e = unet_engine(sd, E.FP32, max_batch=mb, with_classifier=False)
        try:
            e.reserve_unet_vjp(2)
            out, traj = e.spec_vpsde_purify(x0, *a, seed=1, sample0=20, path=1, want_traj=True)
            g = e.spec_vpsde_purify_vjp(traj, sch.c_a, sch.k, sch.h, sch.hb, sch.q, g_out)
            out2, traj2 = e.spec_vpsde_purify(x0, *a, seed=1, sample0=20, path=1, want_traj=True)
            assert torch.equal(out, out2) and torch.equal(traj, traj2)
            assert torch.equal(g, e.spec_vpsde_purify_vjp(traj2, sch.c_a, sch.k, sch.h, sch.hb, sch.q, g_out))
            for i in range(3):
                o1, t1 = e.spec_vpsde_purify(x0[i:i + 1], *a, seed=1, sample0=20 + i, path=1, want_traj=True)
                assert torch.equal(o1, out[i:i + 1]), i
                assert torch.equal(e.spec_vpsde_purify_vjp(t1, sch.c_a, sch.k, sch.h, sch.hb, sch.q, g_out[i:i + 1]), g[i:i + 1]), i
            results[mb] = (out, g)
        finally:
            e.close()
    # two engines of different max_batch are two GEMM configurations of the UNet's fp32 tier: close, not bit-equal
    assert relmax(results[2][0].cpu(), results[4][0].cpu()) <= 1e-6 and relmax(results[2][1].cpu(), results[4][1].cpu()) <= 1e-5
    assert bool(torch.isfinite(results[2][1]).all()) and float(results[2][1].abs().max()) > 0


def test_module_forward_modes(eng, sde, sd):
    """'hip' forwards with and without a gradient are bit-identical; 'none' runs the mode's tier and its gradient is the gain."""
    den = sde.RevImprovedDiffusion(make_args(3), state_dict=sd, engine=eng, seed=2)
    s = spec_db(2, 50)
    den._draws = 0
    with torch.no_grad():
        ref = den(s)
    den._draws = 0
    sr = s.clone().requires_grad_(True)
    out = den(sr)
    assert torch.equal(out.detach(), ref) and den._draws == 2
    den.score_grad = 'none'
    den._draws = 0
    sr = s.clone().requires_grad_(True)
    out = den(sr)
    w = spec_db(2, 51) / 40.0
    (g,) = torch.autograd.grad((out * w).sum(), sr)
    want = w * den.schedule().linear_gain()
    assert torch.allclose(g, want, rtol=1e-5, atol=1e-6 * float(want.abs().max()))
    assert not torch.equal(den(s), out.detach())                         # the next keys: other draws


def test_sample_step_and_rand_t(eng, sde, sd):
    den = sde.RevImprovedDiffusion(make_args(3, sample_step=2, rand_t=True, t_delta=2), state_dict=sd, engine=eng, seed=6)
    s = spec_db(2, 60)
    np.random.seed(123)
    sr = s.clone().requires_grad_(True)
    out = den(sr)
    assert out.shape == (4, 1, 32, 32) and den._draws == 4
    np.random.seed(123)
    levels = [3 + np.random.randint(-2, 2) for _ in range(2)]
    s1, s2 = den.schedule(levels[0]), den.schedule(levels[1])
    std = sde.melspec_standardize
    inv = sde.melspec_inv_standardize
    a = lambda sc: (sc.c_a, sc.c_b, sc.k, sc.h, sc.hb, sc.q, sc.gs)   # noqa: E731
    r1 = inv(eng.spec_vpsde_purify(std(s), *a(s1), seed=6, sample0=0, path=1))
    r2 = inv(eng.spec_vpsde_purify(r1, *a(s2), seed=6, sample0=2, path=1))   # round 2 purifies round 1's mel-dB output, next keys
    assert torch.equal(out[:2, 0].detach(), r1) and torch.equal(out[2:, 0].detach(), r2)
    (g,) = torch.autograd.grad(out.sum(), sr)
    assert bool(torch.isfinite(g).all())


def test_refusals(eng, sde, sd):
    from dmad_hip import engine as E
    from dmad_hip._lib import DmadError
    bf = unet_engine(sd, E.BF16, max_batch=2, with_classifier=False)
    try:
        with pytest.raises(DmadError, match="'none'"):
            sde.RevImprovedDiffusion(make_args(2), state_dict=sd, engine=bf, score_grad='hip')
        den = sde.RevImprovedDiffusion(make_args(2), state_dict=sd, engine=bf, score_grad='none')
        with torch.no_grad():
            assert bool(torch.isfinite(den(spec_db(1, 1))).all())
        sch = sde.spec_vpsde_schedule(2)
        with pytest.raises(DmadError, match='BF16'):
            bf.spec_vpsde_purify(specs(1).cuda(), sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs, path=1)
    finally:
        bf.close()
    s = spec_db(1, 2)
    for mode in ('none', 'hip'):
        den = sde.RevImprovedDiffusion(make_args(2), state_dict=sd, engine=eng, score_grad=mode)
        sr = s.clone().requires_grad_(True)
        with pytest.raises(DmadError, match='create_graph'):
            torch.autograd.grad(den(sr).sum(), sr, create_graph=True)
    for t in (0, 1001):
        with pytest.raises(ValueError):
            sde.RevImprovedDiffusion(make_args(t), state_dict=sd, engine=eng)(s)
    with pytest.raises(NotImplementedError, match='score type'):
        sde.RevImprovedDiffusion(make_args(2, score_type='ddpm'), state_dict=sd, engine=eng)(s)
    sch = sde.spec_vpsde_schedule(2)
    with pytest.raises(DmadError, match=r'outside \[0, 1000\]'):
        eng.spec_vpsde_purify(specs(1).cuda(), sch.c_a, sch.c_b, [1001, 0], sch.h, sch.hb, sch.q, sch.gs, path=1)
    fresh = unet_engine(sd, E.FP32, max_batch=2, with_classifier=False)
    try:
        _, traj = fresh.spec_vpsde_purify(specs(1).cuda(), sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs, path=1, want_traj=True)
        with pytest.raises(DmadError, match='dmad_reserve_unet_vjp'):
            fresh.spec_vpsde_purify_vjp(traj, sch.c_a, sch.k, sch.h, sch.hb, sch.q, specs(1).cuda())
    finally:
        fresh.close()


def test_spec_system_end_to_end(eng, sde, sd):
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.vgg import vgg19_bn
    from dmad_hip.transforms import MelSpectrogramDB
    net = vgg19_bn(num_classes=10, in_channels=1)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.vgg19_bn_state_dict(4321).items()})
    den = sde.RevImprovedDiffusion(make_args(2), state_dict=sd, engine=eng, seed=3)
    model = AcousticSystem(classifier=net.eval().cuda().bind_engine(eng), transform=MelSpectrogramDB(eng), defender=den, defense_type='spec')
    x = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in (2, 5)])).float().cuda()
    y = torch.tensor([1, 4]).cuda()
    grads = {}
    for mode in ('none', 'hip'):
        den.score_grad = mode
        den._draws = 0
        xg = x.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(torch.nn.functional.cross_entropy(model(xg), y), xg)
        grads[mode] = g.double().cpu()
    assert np.isfinite(grads['hip'].numpy()).all() and float(grads['hip'].abs().max()) > 0
    d = float((grads['hip'] - grads['none']).norm() / grads['none'].norm())
    assert d > 1e-3, d


def test_memory_of_the_full_gradient(sd, sde):
    """B = 4, t = 5: beyond the engine's fixed reservation, the allocator grows by the trajectory and a few maps, and the engine
    allocates nothing in the data path."""
    from dmad_hip import engine as E
    e = unet_engine(sd, E.FP32, max_batch=4, with_classifier=False)
    try:
        den = sde.RevImprovedDiffusion(make_args(5), state_dict=sd, engine=e, score_grad='hip')
        e.reserve_unet_vjp(4)
        s = spec_db(4, 70)
        before = e.device_bytes()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        sr = s.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(den(sr).sum(), sr)
        torch.cuda.synchronize()
        growth = torch.cuda.max_memory_allocated() - base
        assert e.device_bytes() == before
        assert bool(torch.isfinite(g).all())
        traj = (5 + 1) * 4 * 1024 * 4
        assert growth <= traj + 2 ** 20, growth
    finally:
        e.close()
