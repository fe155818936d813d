"""The imperceptible attack (Qin-I), the part that needs no GPU: the host PsychoacousticMasker and stage 2 of AudioAttack on its torch
branch against tests/golden/qin.npz (recorded from the reference by tests/golden/make_golden_qin.py), the float64 walk of
tests/qin_ref.py against torch.autograd, the C ABI and its binding, the refusals and the drivers' flags.

What the fixture pins of the masker, quirks of the reference included: the STFT is taken of float32 frames and rounded to complex64;
the PSD is 20 log10 |sqrt(8/3) S / 2048| clipped at -200 and normalised to a maximum of 96; maskers are strict local maxima (edges
never), smoothed with both neighbours in the power domain; the ATH is -inf outside 20 Hz ... 20 kHz and filters BEFORE the bark
distance does; the bark loop reads the bark scale at the position in the masker list, not at the bin, and advances i_prev by one when
it drops the earlier masker (the crafted case tells the two apart); the spread function has two slopes, max(masker - 40, 0) on the
upper one; the global threshold adds the ATH in the power domain.

Measured on the build machine (CPU, one torch thread and the default thread count):
  * masker sets: equal on all 3 x 28 frames; threshold against the fixture (stored as float32): max |diff| 3.8e-6 dB, the float32
    rounding of the stored values; bound THRESHOLD_TOL = 1e-4 dB (the issue's, from float32 / float64 restatements agreeing to 8e-5 dB);
  * stage 2, torch branch against the fixture trace: loss_theta max relative deviation 0 and x_imperceptible max |diff| 0, with one
    torch thread (as the recorder ran) and with the default thread count: the branch is the reference's operators in the reference's
    order, and the FFT and the model's small matmul do not depend on the thread count.  The bounds are 4x the measured deviation,
    LOSS_RTOL = X_ATOL = 4 * 0 = 0: the trace and the clips are compared for equality."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import qin_ref
from dmad_hip import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
LIB = os.path.join(PKG, 'libdmad_hip.so')
NEW_EXPORTS = ('dmad_masking_loss_vjp', 'dmad_masking_step')
THRESHOLD_TOL = 1e-4                    # dB
LOSS_RTOL = 4 * 0.0
X_ATOL = 4 * 0.0


@pytest.fixture(scope='module')
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, 'qin.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def masker():
    from robustness_eval.white_box_attack import PsychoacousticMasker
    return PsychoacousticMasker()


def clip(i):
    return np.asarray(synth.synthetic_clip(i), np.float32).reshape(-1)


def test_masker_surface(masker):
    from robustness_eval.white_box_attack import PsychoacousticMasker
    m = PsychoacousticMasker(1024, 256, 8000)
    assert (m.window_size, m.hop_size, m.sample_rate) == (1024, 256, 8000)
    assert (masker.window_size, masker.hop_size, masker.sample_rate) == (2048, 512, 16000)
    assert masker.fft_frequencies.shape == masker.bark.shape == masker.absolute_threshold_hearing.shape == (1025,)
    ath = masker.absolute_threshold_hearing
    assert np.isneginf(ath[:3]).all() and np.isfinite(ath[3:]).all()          # 0, 7.8 and 15.6 Hz lie below 20 Hz
    t, p = masker.calculate_threshold_and_psd_maximum(np.zeros(16000, np.float32))
    assert t.shape == (1025, 28) and p == -200.0                              # silence: no maskers, the threshold is the ATH
    assert np.isneginf(t[:3]).all() and np.allclose(t[3:, 0], ath[3:])
    src = open(os.path.join(PKG, 'robustness_eval', 'white_box_attack.py')).read()
    assert not re.search(r'^\s*(import|from)\s+librosa', src, flags=re.M)            # numpy and scipy only


def test_masker_against_the_reference(fx, masker):
    worst = 0.0
    for i in fx['clip_ids']:
        x = clip(int(i))
        threshold, psd_max = masker.calculate_threshold_and_psd_maximum(x)
        assert threshold.shape == (1025, 28) and threshold.dtype == np.float64
        assert abs(float(psd_max) - float(fx['psd_max'][i])) <= 1e-9
        psd, _ = masker.power_spectral_density(x)
        assert psd.max() == 96.0
        for f in range(28):
            bins = masker.filter_maskers(*masker.find_maskers(psd[:, f]))[1]
            want = fx['masker_bins'][i, f]
            assert bins.tolist() == want[want >= 0].tolist(), (i, f)
        worst = max(worst, float(np.abs(threshold - fx['threshold'][i]).max()))
    print('threshold: max |diff| to the fixture %.3g dB' % worst)
    assert worst <= THRESHOLD_TOL


def test_filter_maskers_reads_bark_by_position(fx, masker):
    kept = masker.filter_maskers(fx['crafted_maskers'], fx['crafted_idx'])[1]
    assert kept.tolist() == fx['crafted_kept'].tolist() == [101]
    assert fx['crafted_by_bin'].tolist() == [101, 400]                        # what a bark scale read at the bins would keep
    # the ATH filter comes first: a masker below it neither survives nor shields its neighbour
    m, idx = masker.filter_maskers(np.array([-50.0, 60.0]), np.array([100, 101]))
    assert idx.tolist() == [101] and m.tolist() == [60.0]


def test_find_maskers_strict_maxima():
    from robustness_eval.white_box_attack import PsychoacousticMasker
    v = np.array([5.0, 1.0, 3.0, 3.0, 1.0, 4.0, 2.0, 9.0])                    # an edge, a plateau, one strict maximum, an edge
    m, idx = PsychoacousticMasker.find_maskers(v)
    assert idx.tolist() == [5]
    assert abs(m[0] - 10 * np.log10(10 ** 0.1 + 10 ** 0.4 + 10 ** 0.2)) < 1e-12


class StridedAverageLinear(torch.nn.Module):
    """the model of make_golden_qin.py"""

    def __init__(self, weight):
        super().__init__()
        self.weight = torch.nn.Parameter(weight, requires_grad=False)

    def forward(self, x):
        F = self.weight.shape[1]
        return x[:, 0].reshape(x.shape[0], -1, F).mean(1) @ self.weight.t()


def _attack(fx, masker, **kw):
    from robustness_eval.white_box_attack import AudioAttack
    s = json.loads(str(fx['settings']))
    k = dict(s['stage_1'], **s['stage_2'])
    k.update(kw)
    return AudioAttack(StridedAverageLinear(torch.from_numpy(fx['weight'])).eval(), masker=masker, eot_attack_size=1, eot_defense_size=1, verbose=0,
                       masking_backend='torch', **k)


def test_stage_2_torch_branch_against_the_reference(fx, masker):
    att = _attack(fx, masker)
    x = torch.from_numpy(np.stack([synth.synthetic_clip(int(i)) for i in fx['clip_ids']])).float()
    att._targeted = True
    att.trace = []
    x_imp, success = att.stage_2(x, torch.from_numpy(fx['x_adv']), torch.from_numpy(fx['y']))
    assert len(att.trace) == fx['loss_theta'].shape[0] == 12
    assert [t['prediction'] for t in att.trace] == fx['prediction'].tolist()
    assert np.array_equal(np.array([t['alpha'] for t in att.trace], np.float32), fx['alpha'])
    d = np.diff(fx['alpha'], axis=0)
    assert (d > 0).any() and (d < 0).any()                                    # the fixture raises and lowers alpha
    assert success == fx['success_2'].tolist()
    loss = np.array([t['loss_theta'] for t in att.trace])
    dev_loss = float((np.abs(loss - fx['loss_theta']) / fx['loss_theta']).max())
    dev_x = float(np.abs(x_imp.numpy() - fx['x_imperceptible']).max())
    print('stage 2 torch branch against the fixture: loss_theta max relative deviation %.3g, x_imperceptible max |diff| %.3g' % (dev_loss, dev_x))
    assert dev_loss <= LOSS_RTOL and dev_x <= X_ATOL
    assert x_imp.shape == x.shape and not x_imp.requires_grad


def test_stage_2_early_stop_and_generate(fx, masker, capsys):
    """loss_theta_min above every loss: every example stops at the first iteration; generate returns both success lists"""
    att = _attack(fx, masker, loss_theta_min=1e9, max_iter_1=2, max_iter_2=5)
    att.trace = []
    x = torch.from_numpy(np.stack([synth.synthetic_clip(int(i)) for i in fx['clip_ids']])).float()
    x_adv, (s1, s2) = att.generate(x, torch.from_numpy(fx['y']), targeted=True)
    assert len(att.trace) == 1 and len(s1) == len(s2) == 3 and x_adv.shape == x.shape
    assert att.masking_backend == 'torch' and att._window_size == 2048 and att._hop_size == 512


def test_walk_against_autograd_in_float64():
    B, L = 2, 2048 + 3 * 512 + 100                                           # 4 frames and a tail no frame reads
    rng = np.random.RandomState(0)
    delta = rng.randn(B, L) * 1e-3
    theta = rng.rand(B, 1025, 4) * 40.0
    psd_max = np.array([3.0, 0.5])
    d = torch.from_numpy(delta).requires_grad_(True)                          # the reference's operators, every one in float64
    stft = torch.view_as_real(torch.stft(d, n_fft=2048, hop_length=512, win_length=2048, center=False,
                                         window=torch.hann_window(2048, dtype=torch.float64), return_complex=True))
    mag = torch.sqrt(torch.sum(torch.square(float(np.sqrt(8.0 / 3.0)) * stft / 2048), -1))
    psd = pow(10.0, 9.6) / torch.from_numpy(psd_max).reshape(-1, 1, 1) * torch.square(mag)
    loss = torch.mean(torch.relu(psd - torch.from_numpy(theta)), dim=(1, 2))
    (g,) = torch.autograd.grad(loss.sum(), d)
    g, loss = g[:, None], loss.detach()
    assert g.dtype == torch.float64 and g.shape == (B, 1, L)
    w = qin_ref.masking_walk(delta, theta, 10 ** 9.6 / psd_max)
    assert 0.05 < w['mask'].mean() < 0.95
    assert np.abs(w['loss'] - loss.numpy()).max() <= 1e-12 * np.abs(w['loss']).max()
    assert np.abs(w['g'] - g[:, 0].numpy()).max() <= 1e-11 * np.abs(w['g']).max()
    assert (w['g'][:, 2048 + 3 * 512:] == 0).all() and (g[:, 0, 2048 + 3 * 512:] == 0).all()
    pinned = qin_ref.masking_walk(delta, theta, 10 ** 9.6 / psd_max, mask=np.ones_like(w['mask']))     # a pinned mask is obeyed
    assert np.abs(pinned['loss'] - (w['psd'] - theta).mean(axis=(1, 2))).max() <= 1e-12
    x = rng.rand(B, L) * 2 - 1
    up = qin_ref.step_ref(x, delta, w['g'], [0.5, 2.0], -0.25, w['g'])
    assert np.abs(x + up).max() <= 1.0 + 1e-15


@pytest.fixture(scope='module')
def built_lib():
    if not os.path.exists(LIB):
        subprocess.run(['make', '-C', os.path.join(PKG, 'csrc'), '-j4'], check=True)
    return ctypes.CDLL(LIB)


def test_masking_exports(built_lib):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dmad.h')).read(), flags=re.S)
    from dmad_hip import _lib
    from dmad_hip.engine import Engine
    for name in NEW_EXPORTS:
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr), name
        assert hasattr(built_lib, name), name
        assert name in _lib.EXPORTS, name
    assert len(_lib._SIGNATURES['dmad_masking_loss_vjp'][1]) == 9 and len(_lib._SIGNATURES['dmad_masking_step'][1]) == 11
    assert _lib._SIGNATURES['dmad_masking_step'][1][5] is ctypes.c_float
    assert callable(Engine.masking_loss_vjp) and callable(Engine.masking_step)


def test_backend_refusals(fx, masker):
    from dmad_hip._lib import DmadError
    from robustness_eval.white_box_attack import AudioAttack, MASKING_BACKENDS
    assert MASKING_BACKENDS == ('hip', 'torch')
    model = StridedAverageLinear(torch.from_numpy(fx['weight']))
    with pytest.raises(ValueError):
        AudioAttack(model, masker=masker, eot_attack_size=1, eot_defense_size=1, masking_backend='cuda')
    att = AudioAttack(model, masker=masker, max_iter_1=1, max_iter_2=2, eot_attack_size=1, eot_defense_size=1, verbose=0)
    assert att.masking_backend == 'hip'
    x = torch.zeros(1, 1, 16000)
    seen = []
    att.stage_1 = lambda *a: seen.append(a)
    with pytest.raises(DmadError, match='no CPU path'):                       # no engine behind the model, and before stage 1 runs
        att.generate(x, torch.tensor([0]))
    model.classifier = type('C', (), {})()
    model.classifier.__dict__['engine'] = object()
    with pytest.raises(DmadError, match='no CPU path'):                       # an engine, but the clips are on the CPU
        att.generate(x, torch.tensor([0]))
    with pytest.raises(DmadError, match='no CPU path'):
        att.stage_2(x, x, torch.tensor([0]))
    assert not seen
    for bad in (None, object()):                                              # max_iter_2 > 0 without a masker: as before
        with pytest.raises(NotImplementedError):
            AudioAttack(model, masker=bad, max_iter_2=5, eot_attack_size=1, eot_defense_size=1).generate(x, torch.tensor([0]))


def test_driver_flags_and_refusals():
    import adaptive_attack_eval
    import baseline_defense_eval
    import black_box_attack_eval
    import imperceptible_attack_eval as drv
    import siren_attack_eval
    args = drv.build_parser().parse_args([])
    assert args.attack == 'Qin-I' and args.max_iter_2 == 4000 and args.masking_backend == 'hip' and args.defense == 'None'
    assert (args.eps, args.bound_norm, args.max_iter_1, args.batch_size, args.eot_attack_size, args.eot_defense_size) == (65, 'linf', 10, 20, 1, 1)
    for d in ('None', 'Diffusion', 'Diffusion-Spec'):
        drv.check_supported(drv.build_parser().parse_args(['--defense', d, '--masking_backend', 'torch']))
    owner = {'CW': 'adaptive_attack_eval.py', 'FAKEBOB': 'black_box_attack_eval.py', 'SirenAttack': 'siren_attack_eval.py'}
    for a, o in owner.items():
        with pytest.raises(NotImplementedError, match=r'--attack %s.*%s' % (a, o.replace('.', r'\.'))):
            drv.check_supported(drv.build_parser().parse_args(['--attack', a]))
    with pytest.raises(NotImplementedError, match='Kenansville'):
        drv.check_supported(drv.build_parser().parse_args(['--attack', 'Kenansville']))
    for d in ('AS', 'BPF', 'FeCo', 'DefenseGAN'):
        with pytest.raises(NotImplementedError, match=d):
            drv.check_supported(drv.build_parser().parse_args(['--defense', d]))
    with pytest.raises(NotImplementedError, match='max_iter_2'):
        drv.check_supported(drv.build_parser().parse_args(['--max_iter_2', '0']))
    # the four older drivers keep refusing Qin-I and stage 2, and name this driver
    for other, extra in ((adaptive_attack_eval, []), (baseline_defense_eval, ['--defense', 'AS']), (black_box_attack_eval, []),
                         (siren_attack_eval, [])):
        with pytest.raises(NotImplementedError, match=r'Qin-I.*imperceptible_attack_eval\.py') as ei:
            other.check_supported(other.build_parser().parse_args(['--attack', 'Qin-I'] + extra))
        assert 'Qin-I are not provided' not in str(ei.value) and 'does not provide' not in str(ei.value)
    for other, extra in ((adaptive_attack_eval, []), (baseline_defense_eval, ['--defense', 'AS'])):
        with pytest.raises(NotImplementedError, match=r'max_iter_2.*imperceptible_attack_eval\.py'):
            other.check_supported(other.build_parser().parse_args(['--attack', 'CW', '--max_iter_2', '3'] + extra))
