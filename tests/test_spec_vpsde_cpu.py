"""The reverse VP-SDE spectrogram purifier without a GPU: the float32 step schedule of diffusion_models.improved_diffusion_sde (pinned
against a table and an independent restatement of torchsde's fixed-step loop at its default dt), the module's reference surface
without torchsde, and the C ABI of dmad_spec_vpsde_purify / dmad_spec_vpsde_purify_vjp (header, exports, bindings)."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
LIB = os.path.join(PKG, 'libdmad_hip.so')
NAMES = ('dmad_spec_vpsde_purify', 'dmad_spec_vpsde_purify_vjp')
B0, B1, N = 0.1, 20.0, 1000

# k of every Euler step of sdeint(ts = linspace(1 - t/1000, 1 - 1e-5, 2), dt = 1e-3) in float32: repeats at t = 5, 10, 25, 30, 200,
# a first k of t at t = 100 (and 1000), and only t = 1, 2 end at k = 0
TABLE = {
    1: [0],
    2: [1, 0],
    3: [3, 2, 1],
    5: [4, 4, 3, 2, 1],
    10: [9, 9] + list(range(8, 0, -1)),
    25: [24, 23, 23] + list(range(22, 0, -1)),
    30: [29, 28, 27, 27] + list(range(26, 0, -1)),
    100: list(range(100, 0, -1)),
    200: [199, 199] + list(range(198, 0, -1)),
}


def restated_loop(t, dt=1e-3):
    """torchsde's fixed-step loop as it behaves, restated in numpy float32: next_t = min(curr_t + dt, ts[-1]); drift and diffusion
    at curr_t; the UNet's step index long((1 - curr_t) * 1000).  -> [(k, curr_t, h)]."""
    f = np.float32
    curr, end = f(1 - t / 1000), f(1 - 1e-5)
    out = []
    while curr < end:
        nxt = min(f(curr + f(dt)), end)
        out.append((int(f(f(1) - curr) * f(N)), curr, f(nxt - curr)))
        curr = nxt
    return out


@pytest.fixture(scope='module')
def sde():
    from diffusion_models import improved_diffusion_sde
    return improved_diffusion_sde


@pytest.mark.parametrize('t', sorted(TABLE) + [1000])
def test_schedule_step_indices(sde, t):
    sch = sde.spec_vpsde_schedule(t)
    loop = restated_loop(t)
    assert sch.k.tolist() == [k for k, _, _ in loop]
    if t in TABLE:
        assert sch.k.tolist() == TABLE[t]
    assert sch.steps == t
    assert sch.h.tolist() == [float(h) for _, _, h in loop]
    assert abs(float(sch.h[-1]) - 0.00099) < 1e-5
    assert sch.k.dtype == np.int32 and sch.h.dtype == sch.hb.dtype == sch.q.dtype == sch.gs.dtype == np.float32
    assert (sch.gs > 0).all()                           # no scale factor: every step draws, the last one included
    assert (sch.k[-1] == 0) == (t <= 2)
    if t == 1000:
        assert sch.k[0] == 1000 and sch.k.max() == 1000 and len(set(sch.k.tolist())) < t      # k = N is legal; repeats and skips


@pytest.mark.parametrize('t', [1, 2, 3, 5, 25, 200])
def test_schedule_coefficients_against_float64(sde, t):
    sch = sde.spec_vpsde_schedule(t)
    for n, (k, curr, h) in enumerate(restated_loop(t)):
        tt = 1.0 - np.float64(curr)
        beta = B0 + tt * (B1 - B0)
        abar = np.exp(-0.5 * (B1 - B0) * tt ** 2 - B0 * tt)
        assert sch.h[n] == np.float32(h)
        assert np.isclose(sch.hb[n], beta / 2, rtol=2e-6), n
        assert np.isclose(sch.q[n], beta / np.sqrt(1 - abar), rtol=2e-6), n
        assert np.isclose(sch.gs[n], np.sqrt(beta) * np.sqrt(np.float64(h)), rtol=2e-6, atol=0), n
        assert 0.006 <= float(sch.h[n]) * float(sch.q[n]) <= 0.0115, n
    betas = torch.linspace(B0 / N, B1 / N, N)                              # RevVPSDE.discrete_betas: the initial diffusion's table
    a = torch.cumprod(1 - betas, dim=0).double().numpy()
    assert np.isclose(sch.c_a, np.sqrt(a[t - 1]), rtol=1e-7) and np.isclose(sch.c_b, np.sqrt(1 - a[t - 1]), rtol=1e-6)
    assert np.isclose(sch.linear_gain(), sch.c_a * np.prod(1 + sch.h.astype(np.float64) * sch.hb), rtol=1e-12)
    # rand_t moves the diffusion level only; the integration range stays at t
    moved = sde.spec_vpsde_schedule(t, t_diffuse=t + 1)
    assert moved.k.tolist() == sch.k.tolist() and moved.h.tolist() == sch.h.tolist() and moved.gs.tolist() == sch.gs.tolist()
    assert np.isclose(moved.c_a, np.sqrt(a[t])) and moved.c_a != sch.c_a and moved.c_b != sch.c_b


def test_schedule_refusals(sde):
    for bad in (0, -3, 1001):
        with pytest.raises(ValueError):
            sde.spec_vpsde_schedule(bad)
        with pytest.raises(ValueError):
            sde.spec_vpsde_schedule(5, t_diffuse=bad)
    sde.spec_vpsde_schedule(1000, t_diffuse=1000)


def test_module_surface_without_torchsde(sde):
    assert 'torchsde' not in sys.modules
    for path in (sde.__file__, os.path.join(os.path.dirname(sde.__file__), '_rev_vpsde.py')):     # the module and the shared host module
        assert not re.search(r'^\s*(import|from)\s+torchsde', open(path).read(), flags=re.M), path
    p = inspect.signature(sde.RevVPSDE.__init__).parameters
    assert [(n, p[n].default) for n in list(p)[1:]] == [
        ('model', inspect.Parameter.empty), ('score_type', 'guided_diffusion'), ('beta_min', 0.1), ('beta_max', 20), ('N', 1000),
        ('img_shape', (1, 32, 32)), ('model_kwargs', None)]
    p = inspect.signature(sde.RevImprovedDiffusion.__init__).parameters
    assert list(p)[1:4] == ['args', 'config', 'device'] and p['config'].default is None and p['device'].default is None
    assert p['score_grad'].default == 'hip'
    for name in ('_scale_timesteps', 'vpsde_fn', 'rvpsde_fn', 'f', 'g'):
        assert callable(getattr(sde.RevVPSDE, name)), name
    for name in ('image_editing_sample', 'forward'):
        assert callable(getattr(sde.RevImprovedDiffusion, name)), name
    assert callable(sde._extract_into_tensor)


def test_revvpsde_attributes_and_diffusion(sde):
    """The reference's attributes, g(t, x) against the schedule's noise scale, and the score_type refusal of the drift."""
    v = sde.RevVPSDE(model=None, score_type='ddpm')
    assert v.noise_type == 'diagonal' and v.sde_type == 'ito'
    assert torch.equal(v.discrete_betas, torch.linspace(0.1 / 1000, 20 / 1000, 1000))
    assert torch.equal(v.alphas_cumprod, torch.cumprod(1. - v.discrete_betas, 0))
    tt = torch.tensor([0.3])
    assert torch.allclose(v.alphas_cumprod_cont(tt), torch.exp(-0.5 * 19.9 * tt ** 2 - 0.1 * tt))
    assert torch.allclose(v.sqrt_1m_alphas_cumprod_neg_recip_cont(tt), -1. / torch.sqrt(1. - v.alphas_cumprod_cont(tt)))
    x = torch.zeros(2, 1024)
    sch = sde.spec_vpsde_schedule(25)
    curr = torch.linspace(1 - 25 / 1000, 1 - 1e-5, 2)[0]
    end = torch.tensor(1 - 1e-5, dtype=torch.float32)
    for n in range(sch.steps):
        g = v.g(curr.reshape(1), x)
        assert g.shape == x.shape
        want = float(sch.gs[n]) / float(np.sqrt(np.float64(sch.h[n])))
        assert np.isclose(float(g[0, 0]), want, rtol=1e-6), n
        curr = min(curr + 1e-3, end)
    with pytest.raises(NotImplementedError, match='score type'):
        v.f(torch.tensor([0.95]), x)
    assert int(v._scale_timesteps(torch.tensor([1.0]))[0]) == 1000 and int(v._scale_timesteps(torch.tensor([0.0]))[0]) == 0
    assert int(v._scale_timesteps(torch.tensor([0.025]))[0]) == 25


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(LIB):
        subprocess.run(['make', '-C', os.path.join(PKG, 'csrc'), '-j4'], check=True)
    return ctypes.CDLL(LIB)


def _arg_types(decl):
    return [re.sub(r'\s+', ' ', a.strip().rsplit(' ', 1)[0].replace('*', ' *')).strip() for a in decl.split(',')]


def test_header_declares_the_spec_vpsde_chain():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dmad.h')).read(), flags=re.S)
    m = re.search(r'int\s+dmad_spec_vpsde_purify\s*\(([^)]*)\)\s*;', hdr)
    assert m
    assert _arg_types(m.group(1)) == [
        'dmad_engine *', 'const float *', 'int32_t', 'int32_t', 'float', 'float', 'const int32_t *', 'const float *', 'const float *',
        'const float *', 'const float *', 'const float *', 'uint64_t', 'uint64_t', 'int32_t', 'float *', 'float *', 'dmad_stream']
    m = re.search(r'int\s+dmad_spec_vpsde_purify_vjp\s*\(([^)]*)\)\s*;', hdr)
    assert m
    assert _arg_types(m.group(1)) == [
        'dmad_engine *', 'const float *', 'int32_t', 'int32_t', 'float', 'const int32_t *', 'const float *', 'const float *',
        'const float *', 'const float *', 'float *', 'dmad_stream']


def test_library_exports_the_spec_vpsde_chain(lib):
    for name in NAMES:
        assert hasattr(lib, name), name


def test_lib_binds_the_spec_vpsde_chain():
    from dmad_hip import _lib
    for name in NAMES:
        assert name in _lib.EXPORTS
    P, i32, f32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_uint64
    assert _lib._SIGNATURES['dmad_spec_vpsde_purify'] == (ctypes.c_int, [P, P, i32, i32, f32, f32, P, P, P, P, P, P, u64, u64, i32, P, P, P])
    assert _lib._SIGNATURES['dmad_spec_vpsde_purify_vjp'] == (ctypes.c_int, [P, P, i32, i32, f32, P, P, P, P, P, P, P])


def test_philox_streams_do_not_overlap(sde):
    """The new streams sit above every other stream the library keys: 0, 1 + t, 0x5BEC, 0x0E70 + t (t <= 1000), 0xD1FF and
    0x5DE00000 + n (n < 0x100000)."""
    from diffusion_models import diffwave_sde
    lo, hi = sde.SPEC_VPSDE_STREAM_DIFFUSE, sde.SPEC_VPSDE_STREAM_STEP0 + 1000
    assert lo == 0x5DF00000 and sde.SPEC_VPSDE_STREAM_STEP0 == 0x5DF00001
    assert lo > diffwave_sde.VPSDE_STREAM_STEP0 + 0xFFFFE and lo > 0x0E70 + 1000 and hi < 0xFFFFFFFF
    src = open(os.path.join(PKG, 'csrc', 'dmad_api.hip')).read()
    assert re.search(r'kSpecVpsdeStreamDiffuse\s*=\s*0x5DF00000u,\s*kSpecVpsdeStreamStep0\s*=\s*0x5DF00001u', src)
