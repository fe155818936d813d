"""The UNet's vector-Jacobian product on the engine (dmad_unet_eps_vjp; UNetModel.grad_backend; the SpecPurifier gradient branch):
against CPU autograd of the oracle restatement, against a directional finite difference of the engine's own fp32 tier, bit-level
properties (eps output, determinism, batch independence, passes), the purifier chain and the defended spec-domain system."""
import numpy as np
import pytest
import torch

import vjp_reservation
from dmad_hip import synth

pytestmark = pytest.mark.gpu

VJP_TOL = 1e-4          # g_x against CPU autograd of the oracle, relative to max |g_x|
SEED = 5252


def relmax(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / np.abs(ref).max()


@pytest.fixture(scope='module')
def orc():
    from oracle import dmad_oracle
    return dmad_oracle


@pytest.fixture(scope='module')
def sd():
    return synth.unet_state_dict(SEED)


@pytest.fixture(scope='module')
def eng(sd):
    """exact-fp32 engine (max_batch 8) with the synthetic UNet and VGG19_bn, no WaveNet."""
    from diffusion_models.improved_diffusion_ddpm import create_improved_diffusion
    from dmad_hip import engine as E
    e = E.Engine(max_batch=8, precision=E.FP32, with_wavenet=False)
    e.load_vgg19_bn(synth.vgg19_bn_state_dict(4321))
    e.pur = create_improved_diffusion(None, reverse_timestep=3, state_dict=sd, engine=e)
    yield e
    e.close()


def specs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, 32, 32, generator=g) * 1.6 - 0.8).float()


def oracle_vjp(orc, sd, x, t, g):
    layout = synth.unet_layout()
    xc = x.detach().cpu().clone().requires_grad_(True)
    eps = orc.unet_forward(sd, xc, torch.full((x.shape[0],), t), layout)
    (gx,) = torch.autograd.grad((eps * g.cpu()).sum(), xc)
    return gx.numpy()


@pytest.mark.parametrize('t', [0, 25, 500])
def test_unet_vjp_against_oracle(eng, orc, sd, t):
    x, g = specs(2, t).cuda(), specs(2, 100 + t).cuda()
    eng.reserve_unet_vjp(2)
    gx, eps = eng.unet_eps_vjp(x, t, g, want_eps=True)
    assert torch.equal(eps, eng.unet_eps(x, t, tier=0))
    ref = oracle_vjp(orc, sd, x, t, g)[:, 0]
    assert relmax(gx.cpu().numpy(), ref) <= VJP_TOL, relmax(gx.cpu().numpy(), ref)


def test_unet_vjp_finite_difference(eng):
    x, g, v = specs(2, 1).cuda(), specs(2, 2).cuda(), specs(2, 3).cuda()
    eng.reserve_unet_vjp(2)
    gx = eng.unet_eps_vjp(x, 25, g)
    f = lambda z: float((eng.unet_eps(z, 25, tier=0).double() * g[:, 0].double()).sum())
    h = 5e-3
    fd = (f(x + h * v) - f(x - h * v)) / (2 * h)
    an = float((gx.double() * v[:, 0].double()).sum())
    assert abs(fd - an) <= 0.01 * abs(an), (fd, an)


def test_unet_vjp_deterministic_and_batch_independent(sd):
    from diffusion_models.improved_diffusion_ddpm import create_improved_diffusion
    from dmad_hip import engine as E
    e = E.Engine(max_batch=5, precision=E.FP32, with_classifier=False, with_wavenet=False)
    try:
        create_improved_diffusion(None, reverse_timestep=3, state_dict=sd, engine=e)
        grown = vjp_reservation.grow(e, e.reserve_unet_vjp, (1, 2), [])      # dmad_device_bytes after reserve(1), (2) and, at the end, (3)
        e.reserve_unet_vjp(2)                   # B = 5 runs in passes of 2
        x, g = specs(5, 7).cuda(), specs(5, 8).cuda()
        a = e.unet_eps_vjp(x, 40, g)
        assert torch.equal(a, e.unet_eps_vjp(x, 40, g))
        for r in range(5):
            assert torch.equal(e.unet_eps_vjp(x[r:r + 1].contiguous(), 40, g[r:r + 1].contiguous()), a[r:r + 1]), r
        e.reserve_unet_vjp(1)                   # a smaller reservation keeps the present one
        assert e.unet_eps_vjp(x, 40, g).equal(a)
        vjp_reservation.check(e, e.reserve_unet_vjp, vjp_reservation.grow(e, e.reserve_unet_vjp, (3,), grown))
    finally:
        e.close()


def test_unet_vjp_refusals(sd):
    from diffusion_models.improved_diffusion_ddpm import create_improved_diffusion
    from dmad_hip import engine as E
    from dmad_hip._lib import DmadError
    e = E.Engine(max_batch=2, precision=E.FP32, with_classifier=False, with_wavenet=False)
    try:
        with pytest.raises(DmadError):
            e.reserve_unet_vjp(2)               # no UNet weights finalised
        pur = create_improved_diffusion(None, reverse_timestep=3, state_dict=sd, engine=e)
        x, g = specs(2).cuda(), specs(2, 1).cuda()
        with pytest.raises(DmadError, match='dmad_reserve_unet_vjp'):
            e.unet_eps_vjp(x, 3, g)             # no reservation
        e.reserve_unet_vjp(2)
        with pytest.raises(DmadError):
            e.unet_eps_vjp(x, 3, g[:1])         # shapes disagree
        with pytest.raises((DmadError, AssertionError)):
            e.unet_eps_vjp(x[:, :, :16], 3, g[:, :, :16])
        with pytest.raises(DmadError):
            e.unet_eps_vjp(x.cpu(), 3, g.cpu())
        xr = x.clone().requires_grad_(True)
        eps = pur.model(xr, torch.full((2,), 3))
        (gx,) = torch.autograd.grad(eps.sum(), xr, create_graph=False)
        assert bool(torch.isfinite(gx).all())
        with pytest.raises(DmadError, match='first-order'):
            torch.autograd.grad(pur.model(xr, torch.full((2,), 3)).sum(), xr, create_graph=True)
        with pytest.raises(NotImplementedError):
            pur.model(xr, torch.tensor([3, 4]))  # per-row timesteps keep their error
    finally:
        e.close()


def test_unet_model_autograd_equals_vjp(eng):
    x, g = specs(3, 11).cuda(), specs(3, 12).cuda()
    xr = x.clone().requires_grad_(True)
    eps = eng.pur.model(xr, torch.full((3,), 7))
    assert eps.shape == (3, 1, 32, 32) and torch.equal(eps.detach(), eng.unet_eps(x, 7, tier=0).unsqueeze(1))
    (ga,) = torch.autograd.grad((eps * g).sum(), xr)
    assert torch.equal(ga[:, 0], eng.unet_eps_vjp(x, 7, g))


def spec_db(B, seed=0):
    return (specs(B, seed) * 40.0 - 40.0).cuda()             # mel-dB range of the standardisation (-100 .. 38)


def test_spec_purifier_grad_branch_forward_values(eng):
    from diffusion_models.improved_diffusion_ddpm import SpecPurifier
    den = SpecPurifier(eng.pur, seed=17)
    s = spec_db(3, 5)
    den._draws = 11
    ref = den(s)
    assert den._draws == 14
    den._draws = 11
    got = den(s.clone().requires_grad_(True))
    assert den._draws == 14 and got.requires_grad
    assert relmax(got.detach().cpu().numpy(), ref.cpu().numpy()) <= 1e-5


def test_spec_purifier_chain_gradient_against_oracle(eng, orc, sd):
    from diffusion_models.improved_diffusion_ddpm import SpecPurifier
    den = SpecPurifier(eng.pur, seed=29)
    s = spec_db(1, 9)
    den._draws = 4
    sr = s.clone().requires_grad_(True)
    w = spec_db(1, 10)
    (g,) = torch.autograd.grad((den(sr) * w).sum(), sr)
    # the oracle chain on the CPU with the same draws
    gd, layout = orc.GaussianDiffusionOracle(1000), synth.unet_layout()
    zq = eng.philox_normal(29, 4, 0x5BEC, 1)[:, :1024].reshape(1, 1, 32, 32).cpu()
    zs = {t: eng.philox_normal(29, 4, 0x0E70 + t, 1)[:, :1024].reshape(1, 1, 32, 32).cpu() for t in range(1, 4)}
    sc = s.cpu().clone().requires_grad_(True)
    x = gd.q_sample(orc.melspec_standardize(sc), 3, zq)
    model = lambda v, t: orc.unet_forward(sd, v, torch.full((1,), t), layout)
    for t in range(3, -1, -1):
        x, _ = gd.p_sample(model, x, t, zs.get(t))
    (gr,) = torch.autograd.grad((orc.melspec_inv_standardize(x) * w.cpu()).sum(), sc)
    assert relmax(g.cpu().numpy(), gr.numpy()) <= 1e-3, relmax(g.cpu().numpy(), gr.numpy())


def test_spec_system_end_to_end(eng):
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.vgg import vgg19_bn
    from diffusion_models.improved_diffusion_ddpm import SpecPurifier
    from dmad_hip.transforms import MelSpectrogramDB
    net = vgg19_bn(num_classes=10, in_channels=1)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.vgg19_bn_state_dict(4321).items()})
    den = SpecPurifier(eng.pur, seed=3)
    model = AcousticSystem(classifier=net.eval().cuda().bind_engine(eng), transform=MelSpectrogramDB(eng), defender=den, defense_type='spec')
    x0 = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in (2, 5)])).float().cuda()
    y = torch.tensor([1, 4]).cuda()
    x = x0.clone().requires_grad_(True)
    den._draws = 0
    torch.nn.functional.cross_entropy(model(x), y, reduction='sum').backward()
    g = x.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0

    def loss(z):
        den._draws = 0
        with torch.no_grad():
            return float(torch.nn.functional.cross_entropy(model(z).double(), y, reduction='sum'))
    v = g / g.norm()                          # along the gradient: d loss / d h = |g|; steps small against the mel-dB curvature
    an = float(g.norm())
    fds = [(loss(x0 + h * v) - loss(x0 - h * v)) / (2 * h) for h in (1e-4, 3e-5)]
    assert min(abs(fd - an) for fd in fds) <= 0.02 * abs(an), (fds, an)


def test_spec_purifier_memory(eng):
    from diffusion_models.improved_diffusion_ddpm import SpecPurifier
    eng.reserve_unet_vjp(8)
    den = SpecPurifier(eng.pur, seed=1)
    s = spec_db(8, 21).requires_grad_(True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    (den(s) * s.detach()).sum().backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    assert bool(torch.isfinite(s.grad).all()) and growth < 64 * 2 ** 20, growth
