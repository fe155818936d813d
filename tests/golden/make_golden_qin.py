#!/usr/bin/env python3
"""BUILD-CONTAINER-ONLY generator of tests/golden/qin.npz: the imported reference's `PsychoacousticMasker` (white_box_attack.py l.38-275)
and a short run of stage 2 of its `AudioAttack` (l.470-706) on the CPU, against the small deterministic model of make_golden_fakebob.py
— a fixed-seed linear map of a strided average of the clip to 10 classes, its weights stored in the fixture.

Masker: calculate_threshold_and_psd_maximum on dmad_hip.synth.synthetic_clip(0..2) -> threshold [3, 1025, 28] (stored as float32: at
most 96 dB in magnitude, so the rounding is below 4e-6 dB, inside the 1e-4 dB the test allows), psd_max, and per frame the bins of
the maskers that survive filter_maskers (padded with -1).  One crafted call of filter_maskers, maskers 50 / 60 / 55 dB at bins 100,
101 and 400: the reference reads the bark scale at the POSITION in the masker list (0, 1, 2: all within 0.5 bark), so it keeps bin
101 only, where a bark scale read at the bins would keep 101 and 400.  The recorder computes both and asserts that they differ.

Stage 2: 3 clips, a targeted attack (the sign with which alpha * g_theta LOWERS the masking loss), max_iter_2 = 12,
num_iter_increase_alpha = 2, num_iter_decrease_alpha = 3, started from the result of the reference's own stage 1 (10 iterations,
eps 65).  Recorded per iteration (taken by wrapping _loss_gradient_masking_threshold, the reference is not edited: the wrapper reads
`alpha` and `prediction` from the calling frame) loss_theta, alpha and the predictions, then x_imperceptible and the success list.
Stage 1 reaches every target of this linear model and stage 2's network gradient keeps it there, so alpha would only ever be raised:
stage 2 therefore aims clip 1 at the NEXT class (RETARGET).  It starts as a miss, its alpha is lowered at iterations 3 and 6, the
summed network gradient (the reference never zeroes delta.grad in stage 2) carries it over at iteration 7, its alpha is raised at 8
and 10, and its best-so-far clip is replaced once (iteration 8).  That alpha is raised and lowered at least once each is asserted.
(A smaller stage-1 bound is no way to a miss: its saturated, 64-periodic delta has STFT bins that are exactly 0, where the reference's
sqrt gives a NaN gradient.)

Harness shims, all of them here: the reference's robustness_eval has no __init__.py, so it is mounted as a package of its own; a stub
`librosa` whose core.stft(center=False) is the rfft of the Hann-windowed float32 frames rounded to complex64 (what librosa computes:
float64 window times float32 frame, transformed, stored in the complex type of the input); torch.stft gets return_complex=True and
returns the real view the reference was written against.

Usage:  python tests/golden/make_golden_qin.py
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (path setup only)

N_CLIPS, L, FEATURES, CLASSES = 3, 16000, 64, 10
MODEL_SEED, MODEL_GAIN = 77, 400.0
TARGET_SHIFT = (3, 5, 7)                      # target of clip i = (the model's class + TARGET_SHIFT[i]) % 10
STAGE_1 = dict(eps=65.0, norm='linf', learning_rate_1=13.0, max_iter_1=10)
STAGE_2 = dict(alpha=0.05, learning_rate_2=1.0, max_iter_2=12,
               num_iter_increase_alpha=2, num_iter_decrease_alpha=3, loss_theta_min=0.05)
RETARGET = (0, 1, 0)                          # stage 2 aims clip 1 at another class than stage 1 reached
CRAFTED = dict(maskers=[50.0, 60.0, 55.0], masker_idx=[100, 101, 400])


class StridedAverageLinear(torch.nn.Module):
    """[n, 1, L] -> [n, 10]: feature f is the mean of the samples f, f + F, f + 2F, ...; logits = features @ W^T."""

    def __init__(self, weight):
        super().__init__()
        self.weight = torch.nn.Parameter(weight, requires_grad=False)

    def forward(self, x):
        F = self.weight.shape[1]
        return x[:, 0].reshape(x.shape[0], -1, F).mean(1) @ self.weight.t()


def model_weight():
    return torch.randn(CLASSES, FEATURES, generator=torch.Generator().manual_seed(MODEL_SEED)) * MODEL_GAIN


def stub_stft(y, n_fft, hop_length, win_length, window, center):
    assert not center and win_length == n_fft and y.dtype == np.float32 and y.ndim == 1
    n_frames = (len(y) - n_fft) // hop_length + 1
    out = np.empty((n_fft // 2 + 1, n_frames), dtype=np.complex64)
    for t in range(n_frames):
        out[:, t] = np.fft.rfft(window * y[t * hop_length:t * hop_length + n_fft])
    return out


def reference_module():
    pkg = types.ModuleType('robustness_eval')
    pkg.__path__ = [os.path.join(mg.REF, 'robustness_eval')]
    sys.modules['robustness_eval'] = pkg
    librosa = types.ModuleType('librosa')
    librosa.core = types.ModuleType('librosa.core')
    librosa.core.stft = stub_stft
    sys.modules['librosa'], sys.modules['librosa.core'] = librosa, librosa.core
    mod = importlib.import_module('robustness_eval.white_box_attack')
    assert mod.__file__.startswith(mg.REF)
    real_stft = torch.stft

    class _Torch:                              # the module's own `torch`: everything as it is, stft with the old return convention
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def stft(*a, **k):
            return torch.view_as_real(real_stft(*a, return_complex=True, **k))
    mod.torch = _Torch()
    return mod


def bark_by_bin(masker, maskers, idx):
    """filter_maskers' bark loop with the bark scale read at the maskers' bins: what the reference does NOT do"""
    keep = np.ones(len(idx), dtype=bool)
    prev = 0
    for i in range(1, len(idx)):
        if masker.bark[idx[i]] - masker.bark[idx[prev]] < 0.5:
            if maskers[prev] < maskers[i]:
                keep[prev] = False
                prev = prev + 1
            else:
                keep[i] = False
        else:
            prev = i
    return idx[keep]


def main():
    torch.set_num_threads(1)
    from dmad_hip import synth
    ref = reference_module()
    masker = ref.PsychoacousticMasker()
    clips = np.stack([synth.synthetic_clip(i) for i in range(N_CLIPS)]).astype(np.float32)           # [3, 1, L]

    thresholds, psd_max, sets = [], [], []
    for c in clips[:, 0]:
        t, m = masker.calculate_threshold_and_psd_maximum(c)
        thresholds.append(t)
        psd_max.append(m)
        psd, _ = masker.power_spectral_density(c)
        sets.append([masker.filter_maskers(*masker.find_maskers(psd[:, f]))[1] for f in range(psd.shape[1])])
    width = max(len(s) for per in sets for s in per)
    masker_bins = np.full((N_CLIPS, thresholds[0].shape[1], width), -1, np.int32)
    for i, per in enumerate(sets):
        for f, s in enumerate(per):
            masker_bins[i, f, :len(s)] = s
    thresholds = np.array(thresholds)
    assert np.isfinite(thresholds).all() and np.abs(thresholds).max() < 128

    cm, ci = np.array(CRAFTED['maskers']), np.array(CRAFTED['masker_idx'])
    assert (cm > masker.absolute_threshold_hearing[ci]).all()
    kept = masker.filter_maskers(cm, ci)[1]
    by_bin = bark_by_bin(masker, cm, ci)
    assert kept.tolist() != by_bin.tolist(), 'the crafted case does not tell position-indexed from bin-indexed bark'
    print('crafted filter_maskers: reference keeps', kept.tolist(), '- bark read at the bins would keep', by_bin.tolist())

    W = model_weight()
    model = StridedAverageLinear(W).eval()
    x = torch.from_numpy(clips)
    with torch.no_grad():
        clean = model(x).argmax(1)
    y = (clean + torch.tensor(TARGET_SHIFT)) % CLASSES
    att = ref.AudioAttack(model, masker=masker, eot_attack_size=1, eot_defense_size=1, verbose=0, **STAGE_1, **STAGE_2)
    att._targeted = True
    x_adv, success_1 = att.stage_1(x, y)
    x_adv = x_adv.detach()
    y = (y + torch.tensor(RETARGET)) % CLASSES
    trace = []
    inner = att._loss_gradient_masking_threshold

    def wrapped(*a, **k):
        caller = sys._getframe(1).f_locals
        g, loss = inner(*a, **k)
        trace.append((loss.numpy().astype(np.float64).copy(), caller['alpha'].reshape(-1).numpy().copy(),
                      caller['prediction'].reshape(-1).numpy().copy()))
        return g, loss
    att._loss_gradient_masking_threshold = wrapped
    x_imp, success_2 = att.stage_2(x, x_adv, y)
    loss_theta = np.array([t[0] for t in trace])
    alpha = np.array([t[1] for t in trace])
    prediction = np.array([t[2] for t in trace])
    print('stage 1 success', success_1, 'stage 2 success', success_2, 'iterations', len(trace))
    print('loss_theta\n', loss_theta, '\nalpha\n', alpha, '\nprediction\n', prediction, '\ny', y.tolist())
    assert len(trace) == STAGE_2['max_iter_2'], 'stage 2 stopped early'
    d = np.diff(alpha, axis=0)
    assert (d > 0).any() and (d < 0).any(), 'alpha must be raised and lowered at least once: choose other settings'
    np.savez_compressed(os.path.join(HERE, 'qin.npz'), weight=W.numpy(), clip_ids=np.arange(N_CLIPS), y=y.numpy(),
                        threshold=thresholds.astype(np.float32), psd_max=np.array(psd_max, np.float64), masker_bins=masker_bins,
                        crafted_maskers=cm, crafted_idx=ci, crafted_kept=kept, crafted_by_bin=by_bin,
                        x_adv=x_adv.numpy(), success_1=np.array(success_1), loss_theta=loss_theta, alpha=alpha, prediction=prediction,
                        x_imperceptible=x_imp.detach().numpy(), success_2=np.array(success_2), model_seed=np.array(MODEL_SEED),
                        settings=np.array(json.dumps(dict(stage_1=STAGE_1, stage_2=STAGE_2, target_shift=TARGET_SHIFT, retarget=RETARGET), sort_keys=True)))
    print('qin.npz: %d bytes' % os.path.getsize(os.path.join(HERE, 'qin.npz')))


if __name__ == '__main__':
    main()
