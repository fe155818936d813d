"""The any-length exact-fp32 DiffWave path, the part that needs no GPU: the fixture check of tests/wavenet_len_cases.py (every case's
fp32 CPU oracle within the GPU file's tolerances of the float64 one, so that no ReLU kink decides a GPU test), the keyword-spotting
driver's flags, the routing of a DiffWave built with any_length=True on a scripted engine (other lengths go to the `_len` calls,
clip_len to today's), the surfaces that refuse other lengths before any library call, the engine methods' passes on a scripted library
(rows at a pitch of len), and the C ABI of the six exports."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import wavenet_len_cases as wc
from dmad_hip import synth
from dmad_hip._lib import DmadError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
LIB = os.path.join(PKG, 'libdmad_hip.so')
# name -> (twin, position of `len` among the arguments: right after B)
NEW_EXPORTS = {'dmad_wavenet_eps_len': ('dmad_wavenet_eps_path', 4), 'dmad_wavenet_eps_vjp_len': ('dmad_wavenet_eps_vjp', 4),
               'dmad_philox_normal_len': ('dmad_philox_normal', 5), 'dmad_diffuse_len': ('dmad_diffuse', 8),
               'dmad_ddpm_step_len': ('dmad_ddpm_step', 10), 'dmad_ddpm_purify_len': ('dmad_ddpm_purify', 11)}
CLIP = 2048


# ---- 1. the fixture check ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', wc.ALL_CASES, ids=wc.case_id)
def test_fp32_oracle_is_within_the_tolerances_of_float64(case):
    eps64, g64 = wc.reference(case)
    eps32, g32 = wc.reference(case, torch.float32)
    e_eps, e_g = wc.relmax(eps32, eps64), wc.relmax(g32, g64)
    print('%s: fp32 CPU oracle vs float64: eps %.2e (FP32_TOL %.0e), g_x %.2e (VJP_TOL %.0e)' % (wc.case_id(case), e_eps, wc.FP32_TOL, e_g, wc.VJP_TOL))
    assert eps64.shape == g64.shape == (case[1], case[2])
    assert e_eps <= wc.FP32_TOL and e_g <= wc.VJP_TOL


# ---- 2. the driver's flags --------------------------------------------------------------------------------------------------------------
def driver_args(*flags):
    import kws_adaptive_attack_eval as drv
    return drv, drv.build_parser().parse_args(list(flags))


def test_driver_flags():
    drv, args = driver_args('--defense', 'Diffusion')
    assert (args.clip_len, args.max_clip_len, args.attack, args.batch_size) == (0, 32000, 'CW', 1)
    drv.check_supported(args)                                                       # the native-length Diffusion row runs
    drv.check_supported(driver_args('--defense', 'Diffusion', '--max_clip_len', '9088')[1])
    drv.check_supported(driver_args('--defense', 'Diffusion', '--clip_len', '16000')[1])
    for bad in ('1000', '0', '-128'):
        with pytest.raises(ValueError, match='--max_clip_len'):
            drv.check_supported(driver_args('--defense', 'Diffusion', '--max_clip_len', bad)[1])
    for flags, names in ((('--attack', 'FAKEBOB'), '--clip_len'), (('--attack', 'SirenAttack'), '--clip_len'),
                         (('--attack', 'FAKEBOB', '--defense', 'Diffusion'), '--clip_len'), (('--attack', 'SirenAttack', '--defense', 'LPF'), '--clip_len'),
                         (('--defense', 'AS'), '--clip_len'), (('--defense', 'MS'), '--clip_len'), (('--defense', 'DS'), '--clip_len'),
                         (('--defense', 'LPF'), '--clip_len'), (('--defense', 'BPF'), '--clip_len'), (('--batch_size', '4'), '--clip_len'),
                         (('--batch_size', '4', '--defense', 'Diffusion'), '--clip_len'),
                         (('--clip_len', '8192', '--defense', 'Diffusion'), '--clip_len 16000')):
        with pytest.raises(NotImplementedError, match=names):
            drv.check_supported(driver_args(*flags)[1])
    with pytest.raises(ValueError, match='--max_clip_len 9088'):                    # a longer clip names the flag
        drv.MaxClipLen(lambda x: x, 9088)(torch.zeros(1, 1, 9089))
    assert drv.MaxClipLen(lambda x: x + 1, 9088)(torch.zeros(1, 1, 9088)).sum() == 9088


# ---- 3. routing and refusals on a scripted engine ---------------------------------------------------------------------------------------
class Dev(torch.Tensor):
    """a host tensor that says it lives on the device"""
    @property
    def is_cuda(self):
        return True


class ScriptedEngine:
    """clip_len 2048; records the name of every engine call and answers with zeros of the right shape"""
    L, precision, num_res_layers = CLIP, 1, 5

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(x, *a, **k):
            self.calls.append(name)
            if name == 'philox_normal':
                return torch.zeros(a[2], k.get('length') or self.L)
            x = x[:, 0] if x.dim() == 3 else x
            return x if name.startswith('ddpm_step') else torch.zeros_like(x)
        return call


def diffwave(eng, any_length=True, **kw):
    from diffusion_models.diffwave_ddpm import DiffWave, WaveNetHIP
    from oracle import dmad_oracle as orc
    hp = orc.calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG)
    return DiffWave(WaveNetHIP(eng, any_length=any_length), hp, reverse_timestep=2, **kw)


def test_routing_by_length():
    eng = ScriptedEngine()
    den = diffwave(eng)
    short, whole = torch.zeros(2, 1, 1021), torch.zeros(2, 1, CLIP)
    for x, sfx in ((short, '_len'), (whole, '')):
        eng.calls.clear()
        assert den(x).shape == x.shape and eng.calls == ['ddpm_purify' + sfx]
        eng.calls.clear()
        assert den._diffusion(x).shape == x.shape and den._reverse(x).shape == x.shape
        assert den.compute_eps_t(x, 1).shape == x.shape and den.compute_coefficients(x, 1)[1].shape == x.shape
        assert den.model((x, torch.ones(2, 1))).shape == x.shape
        assert eng.calls == ['diffuse' + sfx] + ['ddpm_step' + sfx] * 2 + ['wavenet_eps' + sfx] * 3
    eng.calls.clear()
    cpu_noise = diffwave(eng, noise_source='torch_cpu')
    assert cpu_noise(short).shape == short.shape and eng.calls == ['diffuse_len', 'ddpm_step_len', 'ddpm_step_len']
    # without any_length a model keeps today's calls whatever the length (the engine refuses)
    eng.calls.clear()
    diffwave(eng, any_length=False)(short)
    assert eng.calls == ['ddpm_purify']


def test_refusing_surfaces_raise_before_any_library_call():
    from acoustic_system import AcousticSystem
    from diffusion_models.diffwave_ddpm import ReffWave
    from diffusion_models.diffwave_sde import RevDiffWave
    from robustness_eval.certified_robust import RobustCertificate
    eng = ScriptedEngine()
    den = diffwave(eng)
    reff = ReffWave(den.model, den.diffusion_hyperparams, reverse_timestep=2, num_re=1)
    rev = RevDiffWave.__new__(RevDiffWave)
    torch.nn.Module.__init__(rev)
    rev.model, rev.device = den, torch.device('cpu')
    system = AcousticSystem(classifier=torch.nn.Identity(), transform=None, defender=den)
    system._engine_chain = lambda defend, L=None: (eng, 1)                          # the one-call query chain with the DiffWave sampler
    cert = RobustCertificate(torch.nn.Identity(), None, den, seed=1, shard=False)
    x = torch.zeros(1, 1, 1021)
    surfaces = {'one_shot_denoise': lambda: den.one_shot_denoise(x), 'two_shot_denoise': lambda: den.two_shot_denoise(x),
                'fast_reverse': lambda: den.fast_reverse(x), 'ReffWave.forward': lambda: reff(x), 'ReffWave.diffusion': lambda: reff.diffusion(x),
                'ReffWave.one_shot_denoise': lambda: reff.one_shot_denoise(x), 'VP-SDE': lambda: rev(x),
                'query': lambda: system.query(x.as_subclass(Dev), 2), 'vote loop': lambda: cert.smooth_predict(x, 4, 0.25)}
    for name, call in surfaces.items():
        with pytest.raises(NotImplementedError, match=r'(?s)clip_len \(2048 samples\) only, not at 1021.*DiffWave\.forward.*_diffusion.*_reverse.*compute_eps_t'
                                                      r'.*compute_coefficients.*model\(\(x, t\)\).*any_length=True') as info:
            call()
        assert name.split('.')[0].split(' ')[0].lower() in str(info.value).lower(), (name, str(info.value))
    assert eng.calls == []
    # the same surfaces at clip_len reach the engine
    den.one_shot_denoise(torch.zeros(1, 1, CLIP))
    assert eng.calls == ['one_shot']


def test_engine_methods_walk_passes_at_a_pitch_of_len(monkeypatch):
    """Engine.*_len on a scripted library (as tests/test_engine_plumbing_cpu.py does for the fixed-length methods): B = 9 rows of 1021
    floats on max_batch 4 are three calls of 4, 4 and 1 rows, every per-row pointer advanced by rows * 1021 * 4 bytes, the Philox key by
    the rows, and `len` = 1021 right after the row count."""
    from dmad_hip import engine as E

    class Stream:
        cuda_stream = 0

    class Lib:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def export(*args):
                self.calls.append((name, [a.value if isinstance(a, ctypes.c_void_p) else a for a in args]))
                return 0
            return export
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a, **k: Stream())
    e = E.Engine.__new__(E.Engine)
    e.lib, e._h, e.L, e.max_batch, e.device = Lib(), None, CLIP, 4, torch.device('cpu')
    B, n, row = 9, 1021, 1021 * 4
    x, g, z = (torch.zeros(B, n).as_subclass(Dev) for _ in range(3))

    def calls(name, fn):
        e.lib.calls.clear()
        out = fn()
        assert [c[0] for c in e.lib.calls] == [name] * 3, name
        return out, [c[1] for c in e.lib.calls]
    # (export, call, index of B, index of the key or None, {argument index: per-row tensor}, index of the output or None)
    out, got = calls('dmad_wavenet_eps_len', lambda: e.wavenet_eps_len(x.view(B, 1, n), 3))
    table = [(got, 3, None, {1: x, 5: out})]
    (gx, eps), got = calls('dmad_wavenet_eps_vjp_len', lambda: e.wavenet_eps_vjp_len(x, 3, g, want_eps=True))
    table.append((got, 3, None, {1: x, 5: g, 6: gx, 7: eps}))
    out, got = calls('dmad_diffuse_len', lambda: e.diffuse_len(x, .5, .25, z, seed=11, sample0=7))
    table.append((got, 7, 6, {1: x, 4: z, 9: out}))
    _, got = calls('dmad_ddpm_step_len', lambda: e.ddpm_step_len(x, 3, .1, .2, .3, z, seed=11, sample0=7))
    table.append((got, 9, 8, {1: x, 6: z}))
    out, got = calls('dmad_ddpm_purify_len', lambda: e.ddpm_purify_len(x, 2, .5, .25, [.1, .2], [.3, .4], [.5, .6], seed=11, sample0=7))
    table.append((got, 10, 9, {1: x, 12: out}))
    for got, at_b, at_key, rows in table:
        for (s, cnt), args in zip(((0, 4), (4, 4), (8, 1)), got):
            assert args[at_b] == cnt and args[at_b + 1] == n
            assert at_key is None or args[at_key] == 7 + s
            for i, t in rows.items():
                assert tuple(t.shape) == (B, n) and args[i] == t.data_ptr() + s * row, (i, s)
    e.lib.calls.clear()
    zs = e.philox_normal(1, 2, 3, 5, length=7)
    assert tuple(zs.shape) == (5, 7) and e.lib.calls == [('dmad_philox_normal_len', [None, 1, 2, 3, 5, 7, zs.data_ptr(), None])]
    with pytest.raises(DmadError, match='does not match'):
        e.wavenet_eps_vjp_len(x, 3, g[:, :5])
    with pytest.raises(DmadError, match='GPU'):
        e.wavenet_eps_len(torch.zeros(1, 5), 3)


# ---- 4. the C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def built_lib():
    if not os.path.exists(LIB):
        subprocess.run(['make', '-C', os.path.join(PKG, 'csrc'), '-j4'], check=True)
    return ctypes.CDLL(LIB)


def test_len_exports(built_lib):
    from dmad_hip import _lib
    from dmad_hip.engine import Engine
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dmad.h')).read(), flags=re.S)

    def params(name):
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, name
        return [re.sub(r'\s+', ' ', p.strip()) for p in m.group(1).split(',')]
    for name, (twin, at) in NEW_EXPORTS.items():
        assert hasattr(built_lib, name) and name in _lib.EXPORTS, name
        mine, theirs = params(name), params(twin)
        if twin == 'dmad_wavenet_eps_path':                                         # the twin's `path` argument is fixed to 1
            theirs.remove('int32_t path')
        assert mine[at] == 'int32_t len' and mine[at - 1] == 'int32_t B' and mine[:at] + mine[at + 1:] == theirs, (name, mine, theirs)
        sig, tsig = _lib._SIGNATURES[name], _lib._SIGNATURES[twin]
        targs = list(tsig[1])
        if twin == 'dmad_wavenet_eps_path':
            del targs[4]
        assert sig[0] is ctypes.c_int and sig[1][at] is ctypes.c_int32 and sig[1][:at] + sig[1][at + 1:] == targs, name
    for name in ('wavenet_eps_len', 'wavenet_eps_vjp_len', 'diffuse_len', 'ddpm_step_len', 'ddpm_purify_len'):
        assert callable(getattr(Engine, name)), name
