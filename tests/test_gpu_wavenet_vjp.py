"""The eps-network's vector-Jacobian product on the engine (dmad_wavenet_eps_vjp; WaveNetHIP(..., grad_backend='hip')):
against float64 CPU autograd of the oracle restatement, against a directional finite difference of the engine's own fp32 path,
bit-level properties (eps output, determinism, batch independence), through the whole defended system against the torch
restatement (values and memory), and its refusals."""
import numpy as np
import pytest
import torch

import vjp_reservation
from dmad_hip import synth

pytestmark = pytest.mark.gpu

VJP_TOL = 1e-4          # g_x against float64 autograd, relative to max |g_x|


def relmax(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / np.abs(ref).max()


@pytest.fixture(scope='module')
def orc():
    from oracle import dmad_oracle
    return dmad_oracle


def kink_free(sd):
    """The synthetic weights with the final block's ReLU (f0) kept away from its kink: bias +16 on even, -16 on odd channels, ten
    times the largest |W_f0 s| these inputs produce (1.7).  At a kink the gradient jumps, and an fp32 pre-activation within ~1e-7
    of zero lands on the other side than float64's: with the stock biases two such units of the 5-layer case make ANY fp32
    gradient (the CPU fp32 oracle's too) differ from float64's by 2.4 % of max |g_x|.  With these biases the mask is half zeros,
    half ones and well defined."""
    out = dict(sd)
    b = np.asarray(sd['final_conv.0.conv.bias'])
    out['final_conv.0.conv.bias'] = np.where(np.arange(b.shape[0]) % 2 == 0, 16.0, -16.0).astype(b.dtype)
    return out


@pytest.fixture(scope='module')
def full_sd():
    return kink_free(synth.wavenet_state_dict(1234))


@pytest.fixture(scope='module')
def fp32_engine(full_sd):
    """Full 36 x 12 geometry, exact-fp32 engine with the synthetic VGG19_bn (the system test)."""
    from dmad_hip import engine as E
    eng = E.Engine(max_batch=4, precision=E.FP32)
    eng.load_wavenet(full_sd)
    eng.load_vgg19_bn(synth.vgg19_bn_state_dict(4321))
    yield eng
    eng.close()


def clips(idx, scale=0.8):
    return torch.from_numpy(np.stack([synth.synthetic_clip(i)[0] for i in idx])) * scale          # [B, 16000]


def f64_vjp(orc, sd, x, t, g_eps, nl, cyc):
    """(d eps / d x)^T g_eps of oracle.wavenet_forward in float64 on the CPU."""
    w = {k: v.double() for k, v in orc.folded_weights(sd, nl).items()}
    x64 = x.double().unsqueeze(1).requires_grad_(True)
    eps = orc.wavenet_forward(w, x64, float(t) * torch.ones((x.shape[0], 1), dtype=torch.float64), nl, cyc)
    (g,) = torch.autograd.grad(eps, x64, g_eps.double().unsqueeze(1))
    return g[:, 0].numpy()


def test_vjp_against_float64_small_geometry(orc):
    from dmad_hip import engine as E
    cfg = dict(synth.WAVENET_CONFIG)
    cfg.update(num_res_layers=5, dilation_cycle=4)
    sd = kink_free(synth.wavenet_state_dict(77, cfg))
    eng = E.Engine(wavenet_config=cfg, max_batch=3, precision=E.FP32, with_classifier=False)
    eng.load_wavenet(sd)
    vjp_reservation.check(eng, eng.reserve_vjp, vjp_reservation.grow(eng, eng.reserve_vjp, (1, 2, 3), []))
    eng.reserve_vjp(3)
    x = clips([0, 7])
    g_eps = torch.randn(x.shape, generator=torch.Generator().manual_seed(11))
    got = eng.wavenet_eps_vjp(x.cuda(), 12, g_eps.cuda()).cpu().numpy()
    ref = f64_vjp(orc, sd, x, 12, g_eps, 5, 4)
    eng.close()
    assert np.isfinite(got).all() and relmax(got, ref) <= VJP_TOL, relmax(got, ref)


def test_vjp_against_float64_full_geometry(orc, full_sd, fp32_engine):
    eng = fp32_engine
    eng.reserve_vjp(4)
    x = clips([3])
    g_eps = torch.randn(x.shape, generator=torch.Generator().manual_seed(12))
    got = eng.wavenet_eps_vjp(x.cuda(), 40, g_eps.cuda()).cpu().numpy()
    ref = f64_vjp(orc, full_sd, x, 40, g_eps, 36, 12)
    assert np.isfinite(got).all() and relmax(got, ref) <= VJP_TOL, relmax(got, ref)


def test_vjp_directional_finite_difference(fp32_engine):
    eng = fp32_engine
    eng.reserve_vjp(4)
    x = clips([5]).cuda()
    g_eps = torch.randn(x.shape, generator=torch.Generator().manual_seed(13)).cuda()
    gx = eng.wavenet_eps_vjp(x, 40, g_eps)
    v = gx / gx.norm()
    h = 1e-2

    def f(xx):
        return float((g_eps.double() * eng.wavenet_eps(xx, 40).double()).sum())
    fd = (f(x + h * v) - f(x - h * v)) / (2 * h)
    want = float((gx.double() * v.double()).sum())
    assert abs(fd - want) <= 0.01 * abs(want), (fd, want)


def test_vjp_eps_output_determinism_and_batch_independence(full_sd):
    from dmad_hip import engine as E
    eng = E.Engine(max_batch=4, precision=E.EXACT, recheck_batch=4, with_classifier=False)
    eng.load_wavenet(full_sd)
    eng.reserve_vjp(2)                                          # B = 3 below runs as passes of 2 + 1 clips
    x = clips([0, 4, 9]).cuda()
    g_eps = torch.randn(x.shape, generator=torch.Generator().manual_seed(14)).cuda()
    gx, eps = eng.wavenet_eps_vjp(x, 40, g_eps, want_eps=True)
    assert torch.equal(eps, eng.wavenet_eps_path(x, 40, E.WAVE_FP32))
    assert torch.equal(gx, eng.wavenet_eps_vjp(x, 40, g_eps))
    for i in range(3):
        assert torch.equal(gx[i:i + 1], eng.wavenet_eps_vjp(x[i:i + 1], 40, g_eps[i:i + 1])), i
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    eng.close()


def _system(eng, sd, backend):
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.vgg import vgg19_bn
    from diffusion_models.diffwave_ddpm import DiffWave, WaveNetHIP
    from dmad_hip.transforms import MelSpectrogramDB
    from oracle import dmad_oracle as orc
    hp = orc.calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG)
    den = DiffWave(WaveNetHIP(eng, state_dict=sd, grad_backend=backend), hp, reverse_timestep=2, noise_source='device', seed=3)
    net = vgg19_bn(num_classes=10, in_channels=1)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.vgg19_bn_state_dict(4321).items()})
    net = net.eval().cuda().bind_engine(eng)
    return AcousticSystem(classifier=net, transform=MelSpectrogramDB(eng), defender=den, defense_type='wave'), den


def test_vjp_through_the_system_matches_torch_branch(fp32_engine, full_sd):
    eng = fp32_engine
    eng.reserve_vjp(4)
    model, den = _system(eng, full_sd, 'torch')
    x = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in (0, 5, 2, 8)])).cuda()           # [4, 1, 16000]
    grads, growth = {}, {}
    for backend in ('torch', 'hip'):
        den.model.grad_backend = backend
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        den._draws = 0                                          # the same Philox keys on both branches
        xg = x.clone().requires_grad_(True)
        out = model(xg)
        (g,) = torch.autograd.grad(out[:, 3].sum(), xg)
        torch.cuda.synchronize()
        growth[backend] = torch.cuda.max_memory_allocated() - base
        grads[backend] = g.detach().cpu().numpy()
        del out, g, xg
    assert np.isfinite(grads['hip']).all() and np.abs(grads['hip']).max() > 0
    assert relmax(grads['hip'], grads['torch']) <= 1e-3, relmax(grads['hip'], grads['torch'])
    assert growth['hip'] <= 0.05 * growth['torch'], growth


def test_vjp_without_state_dict(fp32_engine):
    """WaveNetHIP(engine) holds no weights for the torch restatement: with grad_backend='hip' it has a gradient, and EOT with
    use_grad=True (reference _EOT.py:36-66) runs on it."""
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.vgg import vgg19_bn
    from diffusion_models.diffwave_ddpm import DiffWave, WaveNetHIP
    from dmad_hip.transforms import MelSpectrogramDB
    from oracle import dmad_oracle as orc
    from robustness_eval._EOT import EOT
    from robustness_eval._utils import resolve_loss
    eng = fp32_engine
    wn = WaveNetHIP(eng, grad_backend='hip')
    x = clips([1, 6]).unsqueeze(1).cuda().requires_grad_(True)
    eps = wn((x, 40 * torch.ones(2, 1)))
    assert eps.shape == x.shape and eps.requires_grad
    (g,) = torch.autograd.grad((eps * eps).sum(), x)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    hp = orc.calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG)
    den = DiffWave(wn, hp, reverse_timestep=2, noise_source='device', seed=3)
    net = vgg19_bn(num_classes=10, in_channels=1)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.vgg19_bn_state_dict(4321).items()})
    model = AcousticSystem(classifier=net.eval().cuda().bind_engine(eng), transform=MelSpectrogramDB(eng), defender=den, defense_type='wave')
    loss_fn, _ = resolve_loss('Margin', False, 0., 'SCR', None, False)
    scores, loss, grad, decisions = EOT(model, loss_fn, EOT_size=2, EOT_batch_size=1, use_grad=True)(x.detach(), torch.tensor([0, 6]).cuda())
    assert grad.shape == x.shape and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0 and scores.shape == (2, 10)


def test_vjp_refusals(fp32_engine, full_sd):
    from diffusion_models.diffwave_ddpm import WaveNetHIP
    from dmad_hip import engine as E
    from dmad_hip._lib import DmadError
    cfg = dict(synth.WAVENET_CONFIG)
    cfg.update(num_res_layers=5, dilation_cycle=4)
    sd = synth.wavenet_state_dict(77, cfg)
    x = clips([0]).cuda()
    # a 16-bit engine holds no fp32 weights: refused by the C library, and by the autograd branch
    bf = E.Engine(wavenet_config=cfg, max_batch=2, precision=E.BF16, with_classifier=False)
    bf.load_wavenet(sd)
    with pytest.raises(DmadError, match='BF16'):
        bf.reserve_vjp(1)
    with pytest.raises(DmadError):
        WaveNetHIP(bf, grad_backend='hip')((x.unsqueeze(1).requires_grad_(True), 3 * torch.ones(1, 1)))
    bf.close()
    # no reservation: refused by the C library
    f32 = E.Engine(wavenet_config=cfg, max_batch=2, precision=E.FP32, with_classifier=False)
    f32.load_wavenet(sd)
    with pytest.raises(DmadError, match='dmad_reserve_vjp'):
        f32.wavenet_eps_vjp(x, 3, torch.ones_like(x))
    f32.close()
    # CPU tensors
    fp32_engine.reserve_vjp(1)
    with pytest.raises(DmadError):
        fp32_engine.wavenet_eps_vjp(x.cpu(), 3, torch.ones(1, 16000))
    wn = WaveNetHIP(fp32_engine, grad_backend='hip')
    with pytest.raises(DmadError):
        wn((x.cpu().unsqueeze(1).requires_grad_(True), 3 * torch.ones(1, 1)))
    # first-order only
    xg = x.unsqueeze(1).clone().requires_grad_(True)
    eps = wn((xg, 3 * torch.ones(1, 1)))
    with pytest.raises(DmadError, match='create_graph'):
        torch.autograd.grad(eps.sum(), xg, create_graph=True)
    with pytest.raises(ValueError):
        wn.grad_backend = 'cuda'
