"""The reverse VP-SDE purifier without a GPU: the float32 step schedule of diffusion_models.diffwave_sde (pinned against a table and
an independent restatement of torchsde's fixed-step loop), the module's reference surface without torchsde, and the C ABI of
dmad_vpsde_purify / dmad_vpsde_purify_vjp (header, exports, bindings)."""
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
NAMES = ('dmad_vpsde_purify', 'dmad_vpsde_purify_vjp')

# k of every Euler step of sdeint(ts = linspace(1 - t/200, 1 - 1e-5, 2), dt = 1/200) in float32: off by one at t = 10, repeated at
# t = 15 and 30, and the last step has k > 0 (so it draws noise) from t = 10 on
TABLE = {
    1: [0],
    2: [1, 0],
    3: [2, 1, 0],
    5: [4, 3, 2, 1, 0],
    10: [10, 9, 8, 7, 6, 5, 4, 3, 2, 1],
    15: [14, 13, 13] + list(range(12, 0, -1)),
    30: [29, 28, 27, 26, 26] + list(range(25, 0, -1)),
}


def restated_loop(t, T=200, N=200):
    """torchsde 0.2's fixed-step loop as it behaves, restated in numpy float32: next_t = min(curr_t + dt, ts[-1]); the drift and
    diffusion are evaluated at curr_t; RevVPSDE takes the step index as long((1 - curr_t) * N).  -> [(k, curr_t, h)]."""
    f = np.float32
    curr, end, dt = f(1 - t / T), f(1 - 1e-5), f(1. / T)
    out = []
    while curr < end:
        nxt = min(f(curr + dt), end)
        out.append((int(f(f(1) - curr) * f(N)), curr, f(nxt - curr)))
        curr = nxt
    return out


@pytest.fixture(scope='module')
def sde():
    from diffusion_models import diffwave_sde
    return diffwave_sde


@pytest.mark.parametrize('t', sorted(TABLE))
def test_schedule_step_indices(sde, t):
    sch = sde.vpsde_schedule(t)
    loop = restated_loop(t)
    assert sch.k.tolist() == TABLE[t] == [k for k, _, _ in loop]
    assert sch.h.tolist() == [float(h) for _, _, h in loop]
    assert abs(float(sch.h[-1]) - 0.00499) < 1e-5
    assert sch.k.dtype == np.int32 and sch.h.dtype == sch.hb.dtype == sch.q.dtype == sch.gs.dtype == np.float32
    # gs == 0 exactly where k == 0 (the reference's scale_factor = 0), and only there
    assert [float(g) == 0.0 for g in sch.gs] == [k == 0 for k in sch.k]
    assert (sch.gs[-1] > 0) == (t >= 10)


@pytest.mark.parametrize('t', [2, 5, 15, 30])
def test_schedule_coefficients_against_float64(sde, t):
    T = N = 200
    b0, b1 = 0.0001 * T, 0.02 * T
    betas = torch.linspace(b0 / N, b1 / N, N)                            # the RevVPSDE's float32 table ...
    ac = torch.cumprod(1. - betas, dim=0).double().numpy()              # ... its cumulative product, used in float64 from here
    sch = sde.vpsde_schedule(t, T, N, betas)
    for n, (k, curr, h) in enumerate(restated_loop(t)):
        tt = 1.0 - np.float64(curr)
        beta = b0 + (tt * N - 1) / (N - 1) * (b1 - b0)
        assert np.isclose(sch.h[n], np.float64(h), rtol=0, atol=0)
        assert np.isclose(sch.hb[n], beta / 2, rtol=2e-6), n
        assert np.isclose(sch.q[n], beta / np.sqrt(1 - ac[k]), rtol=2e-6), n
        scale = np.sqrt(1 - ac[k - 1]) / np.sqrt(1 - ac[k]) if k > 0 else 0.0
        assert np.isclose(sch.gs[n], scale * np.sqrt(beta) * np.sqrt(np.float64(h)), rtol=2e-6, atol=0), n
    a = torch.cumprod(1 - betas, dim=0).double().numpy()
    assert np.isclose(sch.c_a, np.sqrt(a[t - 1]), rtol=1e-7) and np.isclose(sch.c_b, np.sqrt(1 - a[t - 1]), rtol=1e-6)
    assert np.isclose(sch.linear_gain(), sch.c_a * np.prod(1 + sch.h.astype(np.float64) * sch.hb), rtol=1e-12)
    # rand_t moves the diffusion level only; the integration range stays at t
    moved = sde.vpsde_schedule(t, T, N, betas, t_diffuse=t + 1)
    assert moved.k.tolist() == sch.k.tolist() and np.isclose(moved.c_a, np.sqrt(a[t])) and moved.c_a != sch.c_a


def test_module_surface_without_torchsde(sde):
    assert 'torchsde' not in sys.modules
    for path in (sde.__file__, os.path.join(os.path.dirname(sde.__file__), '_rev_vpsde.py')):     # the module and the shared host module
        assert not re.search(r'^\s*(import|from)\s+torchsde', open(path).read(), flags=re.M), path
    p = inspect.signature(sde.RevVPSDE.__init__).parameters
    assert [(n, p[n].default) for n in list(p)[1:]] == [
        ('model', inspect.Parameter.empty), ('score_type', 'ddpm'), ('beta_min', 0.02), ('beta_max', 4), ('N', 200),
        ('audio_shape', (1, 16000)), ('model_kwargs', None)]
    p = inspect.signature(sde.RevDiffWave.__init__).parameters
    assert list(p)[1:3] == ['args', 'device'] and p['device'].default is None
    for name in ('_scale_timesteps', 'vpsde_fn', 'rvpsde_fn', 'f', 'g'):
        assert callable(getattr(sde.RevVPSDE, name)), name
    for name in ('audio_editing_sample', 'forward'):
        assert callable(getattr(sde.RevDiffWave, name)), name


def test_revvpsde_attributes_and_diffusion(sde):
    """The reference's attributes, g(t, x) against the schedule's noise scale, and the score_type refusal of the drift — all without
    a model (the drift refuses before it would call one)."""
    sdeo = sde.RevVPSDE(model=None, score_type='ddpm', beta_min=0.02, beta_max=4, N=200)
    assert sdeo.noise_type == 'diagonal' and sdeo.sde_type == 'ito'
    assert torch.equal(sdeo.discrete_betas, torch.linspace(0.02 / 200, 4 / 200, 200))
    assert torch.equal(sdeo.sqrt_1m_alphas_cumprod, torch.sqrt(1. - torch.cumprod(1. - sdeo.discrete_betas, 0)))
    x = torch.zeros(2, 16000)
    sch = sde.vpsde_schedule(15)
    curr = torch.linspace(1 - 15 / 200, 1 - 1e-5, 2)[0]
    for n in range(3):
        g = sdeo.g(curr.reshape(1), x)
        assert g.shape == x.shape
        want = float(sch.gs[n]) / float(torch.sqrt(torch.tensor(sch.h[n])))
        assert np.isclose(float(g[0, 0]), want, rtol=1e-6), n
        curr = min(curr + 1. / 200, torch.tensor(1 - 1e-5, dtype=torch.float32))
    assert float(sdeo.g(torch.tensor([1 - 1e-5 - 0.004]), x)[0, 0]) == 0.0          # k = 0: no noise
    with pytest.raises(NotImplementedError, match='score type'):
        sdeo.f(torch.tensor([0.95]), x)
    assert int(sdeo._scale_timesteps(torch.tensor([0.07]))[0]) == 14


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(LIB):
        subprocess.run(['make', '-C', os.path.join(PKG, 'csrc'), '-j4'], check=True)
    return ctypes.CDLL(LIB)


def _arg_types(decl):
    return [re.sub(r'\s+', ' ', a.strip().rsplit(' ', 1)[0].replace('*', ' *')).strip() for a in decl.split(',')]


def test_header_declares_the_vpsde_chain():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dmad.h')).read(), flags=re.S)
    m = re.search(r'int\s+dmad_vpsde_purify\s*\(([^)]*)\)\s*;', hdr)
    assert m
    assert _arg_types(m.group(1)) == [
        'dmad_engine *', 'const float *', 'int32_t', 'int32_t', 'float', 'float', 'const int32_t *', 'const float *', 'const float *',
        'const float *', 'const float *', 'const float *', 'uint64_t', 'uint64_t', 'int32_t', 'float *', 'float *', 'dmad_stream']
    m = re.search(r'int\s+dmad_vpsde_purify_vjp\s*\(([^)]*)\)\s*;', hdr)
    assert m
    assert _arg_types(m.group(1)) == [
        'dmad_engine *', 'const float *', 'int32_t', 'int32_t', 'float', 'const int32_t *', 'const float *', 'const float *',
        'const float *', 'const float *', 'float *', 'dmad_stream']


def test_library_exports_the_vpsde_chain(lib):
    for name in NAMES:
        assert hasattr(lib, name), name


def test_lib_binds_the_vpsde_chain():
    from dmad_hip import _lib
    for name in NAMES:
        assert name in _lib.EXPORTS
    P, i32, f32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_uint64
    assert _lib._SIGNATURES['dmad_vpsde_purify'] == (ctypes.c_int, [P, P, i32, i32, f32, f32, P, P, P, P, P, P, u64, u64, i32, P, P, P])
    assert _lib._SIGNATURES['dmad_vpsde_purify_vjp'] == (ctypes.c_int, [P, P, i32, i32, f32, P, P, P, P, P, P, P])
