"""The reverse VP-SDE purifier on the engine (dmad_vpsde_purify / dmad_vpsde_purify_vjp; diffusion_models.diffwave_sde.RevDiffWave).

At small t the eps term is about 1 % of the output and of the gradient (h q ~ 0.01 per step), so a whole-tensor comparison would pass
with a wrong eps part.  Every accuracy check here subtracts the chain's linear part first — the chain with eps = 0 (x0 and the draws
through c_a, c_b, prod(1 + h beta/2) and gs) for outputs, c_a prod(1 + h beta/2) g_out for gradients — and measures the remainder
relative to its own max."""
import json
import types

import numpy as np
import pytest
import torch

from dmad_hip import synth

pytestmark = pytest.mark.gpu

TOL = 1e-4


def relmax(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / np.abs(ref).max()


def kink_free(sd):
    """The final block's ReLU kept away from its kink (as in tests/test_gpu_wavenet_vjp.py): bias +16 / -16 on even / odd channels."""
    out = dict(sd)
    b = np.asarray(sd['final_conv.0.conv.bias'])
    out['final_conv.0.conv.bias'] = np.where(np.arange(b.shape[0]) % 2 == 0, 16.0, -16.0).astype(b.dtype)
    return out


def clips(idx, scale=0.8):
    return torch.from_numpy(np.stack([synth.synthetic_clip(i)[0] for i in idx])) * scale          # [B, 16000]


SMALL = dict(synth.WAVENET_CONFIG, num_res_layers=5, dilation_cycle=4)


@pytest.fixture(scope='module')
def sde():
    from diffusion_models import diffwave_sde
    return diffwave_sde


@pytest.fixture(scope='module')
def orc():
    from oracle import dmad_oracle
    return dmad_oracle


@pytest.fixture(scope='module')
def small_sd():
    return kink_free(synth.wavenet_state_dict(77, SMALL))


@pytest.fixture(scope='module')
def small_fp32(small_sd):
    from dmad_hip import engine as E
    eng = E.Engine(wavenet_config=SMALL, max_batch=4, precision=E.FP32, with_classifier=False)
    eng.load_wavenet(small_sd)
    yield eng
    eng.close()


def f64_chain(orc, sd, x0, sch, z, nl, cyc, with_eps=True):
    """The chain in float64 on the CPU on oracle.wavenet_forward, with explicit draws z [S + 1, B, L]; differentiable in x0."""
    w = {k: v.double() for k, v in orc.folded_weights(sd, nl).items()}
    x = float(sch.c_a) * x0 + float(sch.c_b) * z[0]
    for n in range(sch.steps):
        drift = float(sch.hb[n]) * x
        if with_eps:
            steps = float(sch.k[n]) * torch.ones((x.shape[0], 1), dtype=torch.float64)
            drift = drift - float(sch.q[n]) * orc.wavenet_forward(w, x.unsqueeze(1), steps, nl, cyc)[:, 0]
        x = x + drift * float(sch.h[n]) + float(sch.gs[n]) * z[n + 1]
    return x


def draws(sch, B, seed):
    return torch.randn((sch.steps + 1, B, 16000), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('t', [2, 15])
def test_forward_against_float64(orc, sde, small_sd, small_fp32, t):
    sch = sde.vpsde_schedule(t)
    x0, z = clips([0, 7]), draws(sch, 2, 100 + t)
    got = small_fp32.vpsde_purify(x0.cuda(), sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs, z=z.cuda(), path=1).cpu().double()
    x64, z64 = x0.double(), z.double()
    ref = f64_chain(orc, small_sd, x64, sch, z64, 5, 4)
    lin = f64_chain(orc, small_sd, x64, sch, z64, 5, 4, with_eps=False)
    assert float((ref - lin).abs().max()) > 1e-3 * float(lin.abs().max())          # the eps part is there to be measured
    assert relmax(got - lin, ref - lin) <= TOL, relmax(got - lin, ref - lin)


def test_forward_tiers_and_trajectory(orc, sde, small_sd, small_fp32):
    from dmad_hip import engine as E
    sch = sde.vpsde_schedule(5)
    x0, z = clips([1, 2, 3]), draws(sch, 3, 5)
    a = (x0.cuda(), sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs)
    # FP32 engine: the trajectory call is the inference call bit for bit, and its slots are the chain's states
    plain = small_fp32.vpsde_purify(*a, seed=9, sample0=4)
    out, traj = small_fp32.vpsde_purify(*a, seed=9, sample0=4, path=1, want_traj=True)
    assert torch.equal(out, plain)
    S = sch.steps
    assert torch.equal(traj.view(S + 1, 3, -1)[S], out)                  # one chunk: [S + 1][B][L]
    # EXACT engine: the default (split-f16) tier within 1e-4 of its exact-fp32 path, eps part only
    ex = E.Engine(wavenet_config=SMALL, max_batch=4, precision=E.EXACT, recheck_batch=4, with_classifier=False)
    ex.load_wavenet(small_sd)
    zc = z.cuda()
    p0 = ex.vpsde_purify(*a, z=zc).cpu().double()
    p1 = ex.vpsde_purify(*a, z=zc, path=1).cpu().double()
    ex.close()
    lin = f64_chain(orc, small_sd, x0.double(), sch, z.double(), 5, 4, with_eps=False)
    assert relmax(p0 - lin, p1 - lin) <= TOL, relmax(p0 - lin, p1 - lin)
    assert not torch.equal(p0, p1)                                        # two tiers did run


@pytest.mark.parametrize('t', [2, 15])
def test_full_gradient_against_float64(orc, sde, small_sd, small_fp32, t):
    sch = sde.vpsde_schedule(t)
    x0, z = clips([3, 6]), draws(sch, 2, 200 + t)
    g_out = torch.randn(x0.shape, generator=torch.Generator().manual_seed(t))
    eng = small_fp32
    eng.reserve_vjp(2)
    _, traj = eng.vpsde_purify(x0.cuda(), sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs, z=z.cuda(), path=1, want_traj=True)
    got = eng.vpsde_purify_vjp(traj, sch.c_a, sch.k, sch.h, sch.hb, sch.q, g_out.cuda()).cpu().double()
    x64 = x0.double().requires_grad_(True)
    (ref,) = torch.autograd.grad(f64_chain(orc, small_sd, x64, sch, z.double(), 5, 4), x64, g_out.double())
    lin = sch.linear_gain() * g_out.double()
    assert float((ref - lin).abs().max()) > 1e-3 * float(lin.abs().max())
    assert np.isfinite(got.numpy()).all() and relmax(got - lin, ref - lin) <= TOL, relmax(got - lin, ref - lin)


def test_full_gradient_directional_finite_difference(sde, small_fp32):
    sch = sde.vpsde_schedule(15)
    eng = small_fp32
    eng.reserve_vjp(2)
    x0 = clips([4]).cuda()
    g_out = torch.randn(x0.shape, generator=torch.Generator().manual_seed(31)).cuda()
    a = (sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs)
    _, traj = eng.vpsde_purify(x0, *a, seed=5, sample0=11, path=1, want_traj=True)
    g = eng.vpsde_purify_vjp(traj, sch.c_a, sch.k, sch.h, sch.hb, sch.q, g_out).double()
    gain = sch.linear_gain()
    rem = g - gain * g_out.double()                         # the eps part of the gradient: the direction that tests it
    v = (rem / rem.norm()).float()
    eps = 1e-2

    def f(x):                                               # fixed Philox keys: the same draws at every evaluation
        return float((g_out.double() * eng.vpsde_purify(x, *a, seed=5, sample0=11, path=1).double()).sum())
    fd = (f(x0 + eps * v) - f(x0 - eps * v)) / (2 * eps) - gain * float((g_out.double() * v.double()).sum())
    want = float((rem * v.double()).sum())
    assert abs(fd - want) <= 0.01 * abs(want), (fd, want)


def test_reproducible_and_batch_independent(sde, small_sd):
    """Bits across repeated calls, and clip b alone == clip b inside [a, b, c] when the sample keys match; B = 3 runs in Python chunks
    of 2 + 1 (max_batch 2) for the forward and in library passes of 2 + 1 (reservation 2) for the gradient."""
    from dmad_hip import engine as E
    sch = sde.vpsde_schedule(10)
    a = (sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs)
    x0 = clips([0, 5, 9]).cuda()
    g_out = torch.randn(x0.shape, generator=torch.Generator().manual_seed(3)).cuda()
    results = {}
    for mb in (2, 4):
        eng = E.Engine(wavenet_config=SMALL, max_batch=mb, precision=E.FP32, with_classifier=False)
        eng.load_wavenet(small_sd)
        eng.reserve_vjp(2)
        out, traj = eng.vpsde_purify(x0, *a, seed=1, sample0=20, path=1, want_traj=True)
        g = eng.vpsde_purify_vjp(traj, sch.c_a, sch.k, sch.h, sch.hb, sch.q, g_out)
        out2, traj2 = eng.vpsde_purify(x0, *a, seed=1, sample0=20, path=1, want_traj=True)
        assert torch.equal(out, out2) and torch.equal(traj, traj2)
        assert torch.equal(g, eng.vpsde_purify_vjp(traj2, sch.c_a, sch.k, sch.h, sch.hb, sch.q, g_out))
        for i in range(3):
            o1, t1 = eng.vpsde_purify(x0[i:i + 1], *a, seed=1, sample0=20 + i, path=1, want_traj=True)
            assert torch.equal(o1, out[i:i + 1]), i
            assert torch.equal(eng.vpsde_purify_vjp(t1, sch.c_a, sch.k, sch.h, sch.hb, sch.q, g_out[i:i + 1]), g[i:i + 1]), i
        results[mb] = (out, g)
        eng.close()
    assert torch.equal(results[2][0], results[4][0]) and torch.equal(results[2][1], results[4][1])
    assert bool(torch.isfinite(results[2][1]).all()) and float(results[2][1].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- the module
def make_args(cfg_path, t, **kw):
    a = dict(ddpm_path=None, ddpm_config=cfg_path, t=t, score_type='guided_diffusion', sample_step=1, rand_t=False, t_delta=0, use_bm=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


@pytest.fixture(scope='module')
def small_cfg(tmp_path_factory):
    p = tmp_path_factory.mktemp('vpsde') / 'config.json'
    p.write_text(json.dumps({'diffusion_config': synth.DIFFUSION_CONFIG, 'wavenet_config': SMALL}))
    return str(p)


def test_none_mode_gradient_and_forward(sde, small_sd, small_fp32, small_cfg):
    den = sde.RevDiffWave(make_args(small_cfg, 15), state_dict=small_sd, engine=small_fp32, seed=4)
    x = clips([1, 8]).unsqueeze(1).cuda()
    with torch.no_grad():
        den._draws = 0
        ref = den(x)
    den._draws = 0
    xg = x.clone().requires_grad_(True)
    out = den(xg)
    assert torch.equal(out.detach(), ref)
    g_out = torch.randn(out.shape, generator=torch.Generator().manual_seed(2)).cuda()
    (g,) = torch.autograd.grad(out, xg, g_out)
    gain = den.schedule().linear_gain()
    assert torch.allclose(g, g_out * gain, rtol=2e-7, atol=0)
    # a different clip batch position and a fresh sample key give different noise: the forward does draw
    assert not torch.equal(den(x), ref)


def test_sample_step_and_rand_t(sde, small_sd, small_fp32, small_cfg):
    args = make_args(small_cfg, 5, sample_step=2, rand_t=True, t_delta=2)
    den = sde.RevDiffWave(args, state_dict=small_sd, engine=small_fp32, seed=6)
    x = clips([2, 3]).unsqueeze(1).cuda()
    np.random.seed(123)
    xg = x.clone().requires_grad_(True)
    out = den(xg)
    assert out.shape == (4, 1, 16000)
    np.random.seed(123)
    levels = [5 + np.random.randint(-2, 2) for _ in range(2)]
    s1, s2 = den.schedule(levels[0]), den.schedule(levels[1])
    eng, a = small_fp32, lambda s: (s.c_a, s.c_b, s.k, s.h, s.hb, s.q, s.gs)
    r1 = eng.vpsde_purify(x, *a(s1), seed=6, sample0=0)
    r2 = eng.vpsde_purify(r1, *a(s2), seed=6, sample0=2)               # round 2 purifies round 1's output with the next keys
    assert torch.equal(out[:2, 0].detach(), r1) and torch.equal(out[2:, 0].detach(), r2)
    w1, w2 = torch.randn_like(x), torch.randn_like(x)
    (g,) = torch.autograd.grad((out[:2] * w1).sum() + (out[2:] * w2).sum(), xg)
    want = s1.linear_gain() * (w1 + s2.linear_gain() * w2)
    assert torch.allclose(g, want, rtol=1e-6, atol=1e-6 * float(want.abs().max()))


def test_refusals(sde, small_sd, small_fp32, small_cfg):
    from dmad_hip import engine as E
    from dmad_hip._lib import DmadError
    bf = E.Engine(wavenet_config=SMALL, max_batch=2, precision=E.BF16, with_classifier=False)
    bf.load_wavenet(small_sd)
    with pytest.raises(DmadError, match='BF16'):
        sde.RevDiffWave(make_args(small_cfg, 2), state_dict=small_sd, engine=bf, score_grad='hip')
    sch = sde.vpsde_schedule(2)
    with pytest.raises(DmadError, match='BF16'):
        bf.vpsde_purify(clips([0]).cuda(), sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs, path=1)
    bf.close()
    x = clips([0]).unsqueeze(1).cuda()
    for mode in ('none', 'hip'):
        den = sde.RevDiffWave(make_args(small_cfg, 2), state_dict=small_sd, engine=small_fp32, score_grad=mode)
        xg = x.clone().requires_grad_(True)
        out = den(xg)
        with pytest.raises(DmadError, match='create_graph'):
            torch.autograd.grad(out.sum(), xg, create_graph=True)
    den = sde.RevDiffWave(make_args(small_cfg, 2, score_type='ddpm'), state_dict=small_sd, engine=small_fp32)
    with pytest.raises(NotImplementedError, match='score type'):
        den(x)
    with pytest.raises(ValueError):
        den.score_grad = 'cuda'


def test_memory_of_the_full_gradient(sde, small_sd, small_cfg):
    """B = 4, t = 5 on the full 36 x 12 geometry: beyond the engine's fixed reservation, the allocator grows by the trajectory and the
    outputs only (a few MB), and the engine allocates nothing in the data path."""
    from dmad_hip import engine as E
    sd = kink_free(synth.wavenet_state_dict(1234))
    eng = E.Engine(max_batch=4, precision=E.FP32, with_classifier=False)
    eng.load_wavenet(sd)
    cfg = small_cfg.replace('config.json', 'full.json')
    with open(cfg, 'w') as f:
        json.dump({'diffusion_config': synth.DIFFUSION_CONFIG, 'wavenet_config': synth.WAVENET_CONFIG}, f)
    den = sde.RevDiffWave(make_args(cfg, 5), state_dict=sd, engine=eng, score_grad='hip')
    eng.reserve_vjp(4)
    x = clips([0, 1, 2, 3]).unsqueeze(1).cuda()
    before = eng.device_bytes()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    xg = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(den(xg).sum(), xg)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    assert eng.device_bytes() == before
    assert bool(torch.isfinite(g).all())
    traj = (5 + 1) * 4 * 16000 * 4
    assert growth <= traj + 4 * 2**20, growth
    eng.close()


@pytest.fixture(scope='module')
def full_system_parts():
    from dmad_hip import engine as E
    sd = kink_free(synth.wavenet_state_dict(1234))
    eng = E.Engine(max_batch=4, precision=E.FP32)
    eng.load_wavenet(sd)
    eng.load_vgg19_bn(synth.vgg19_bn_state_dict(4321))
    yield eng, sd
    eng.close()


def test_system_hip_against_torch(sde, full_system_parts, tmp_path):
    """AcousticSystem(VGG19_bn stand-in, MelSpectrogramDB, RevDiffWave) with a CE loss on the full geometry: the HIP full gradient
    against the torch composition, measured on the part the eps-network contributes (g - g_none)."""
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.vgg import vgg19_bn
    from dmad_hip.transforms import MelSpectrogramDB
    eng, sd = full_system_parts
    cfg = tmp_path / 'config.json'
    cfg.write_text(json.dumps({'diffusion_config': synth.DIFFUSION_CONFIG, 'wavenet_config': synth.WAVENET_CONFIG}))
    den = sde.RevDiffWave(make_args(str(cfg), 2), state_dict=sd, engine=eng, seed=3)
    net = vgg19_bn(num_classes=10, in_channels=1)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.vgg19_bn_state_dict(4321).items()})
    model = AcousticSystem(classifier=net.eval().cuda().bind_engine(eng), transform=MelSpectrogramDB(eng), defender=den, defense_type='wave')
    x = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in (0, 5, 2)])).cuda()
    y = torch.tensor([1, 4, 7]).cuda()
    grads = {}
    for mode in ('none', 'hip', 'torch'):
        den.score_grad = mode
        den._draws = 0
        xg = x.clone().requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(model(xg), y)
        (g,) = torch.autograd.grad(loss, xg)
        grads[mode] = g.detach().double().cpu()
        del loss, g, xg
    d_hip = (grads['hip'] - grads['none']).norm()
    assert np.isfinite(grads['hip'].numpy()).all()
    # non-vacuity: the eps-network's part of the gradient is far above fp32 noise (1e-6): threshold 1e-3 of the whole
    assert d_hip / grads['none'].norm() > 1e-3, float(d_hip / grads['none'].norm())
    assert (grads['hip'] - grads['torch']).norm() <= 1e-2 * d_hip, (float((grads['hip'] - grads['torch']).norm()), float(d_hip))
