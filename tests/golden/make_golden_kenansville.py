#!/usr/bin/env python3
"""BUILD-CONTAINER-ONLY generator of tests/golden/kenansville.npz: a short run of the imported reference's
`robustness_eval.black_box_attack.Kenansville(atk_name='fft')` (l.584-663, and _KenanFFT.py's atk_bst_fft l.180-247) on the CPU, against
the small deterministic model of make_golden_fakebob.py / make_golden_siren.py -- a fixed-seed linear map of a strided average of the
clip to 10 classes.  The fixture stores the seed, the gain and the shape of its weights with a corner and the sum of them as a check, not
the 640 KB of weights: tests/kenansville_cases.py rebuilds them as model_weight() does.

The model keeps the class StridedAverageLinear of those fixtures with 16000 features instead of 64: a linear map of the raw clip.  With
64 features the strided average passes only the multiples of 250 Hz (with 3200, of 5 Hz), where the synthetic clips have nothing but
their noise floor: once a factor cuts that floor the logits are 1e-6 of rounding noise and the arg-max is decided by the summation
order of torch's mean, which a fixture cannot pin across thread counts and devices.  With every sample a feature each surviving bin
reaches the logits, and the smallest top-2 margin over the run is 1.7e-3 of the sum of the absolute products behind a logit, four orders
of magnitude above fp32 rounding.

n = 3 clips of dmad_hip.synth.synthetic_clip (seeds 6, 31 and 1) in one batch, max_iter = 8, untargeted, every label the class the model
gives the clean clip: a small factor -- a nearly untouched clip -- fails, and the bisection has something to find.  Clips 6 and 31 fail
and succeed in turn (01111011 and 01001110); clip 1 keeps its clean class at every factor up to 511 / 512 of its largest bin (found by
trying the seeds 0 .. 39: 1, 5, 14, 28, 32 and 39 do).  The seeds are also chosen so that no factor the run visits comes closer to any
|FFT| bin of its clip than 1000 times the fp32 error of torch.fft (printed below), so that an fp32 transform with another rounding
takes the same decisions: tests/test_gpu_kenansville.py asserts it.
Asserted here, so that the fixture judges every statement of the loop:
  * both bisection branches occur (a success lowers the upper bound, a failure raises the lower one);
  * some clip succeeds in one iteration and fails in a later one, so its kept clip is not the last perturbed one;
  * both final states of `succ` occur: one clip never succeeds and comes back as its input, bit for bit.

Recorded: adver_x, succ, and per iteration the factors and the predictions (taken by wrapping the model, the reference is not edited:
the wrapper reads `_attack_factor` from the calling frame).

Harness shims, all of them here: the reference's robustness_eval has no __init__.py, so it is mounted as a package of its own;
_Kenan / _ssa_core are stubbed when they do not import (the SSA form is not run); numpy.infty (removed in numpy 2) is given back as
numpy.inf.

Usage:  python tests/golden/make_golden_kenansville.py
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
from make_golden_siren import StridedAverageLinear  # noqa: E402

N_CLIPS, L, FEATURES, CLASSES = 3, 16000, 16000, 10
MODEL_SEED, MODEL_GAIN = 77, 400.0
CLIP_IDS = (6, 31, 1)                        # seeds of synth.synthetic_clip
SETTINGS = dict(atk_name='fft', max_iter=8, raster_width=100, early_stop=False, targeted=False, verbose=0, BITS=16, batch_size=N_CLIPS)


def model_weight():
    return torch.randn(CLASSES, FEATURES, generator=torch.Generator().manual_seed(MODEL_SEED)) * MODEL_GAIN


def reference_kenansville():
    pkg = types.ModuleType('robustness_eval')
    pkg.__path__ = [os.path.join(mg.REF, 'robustness_eval')]
    sys.modules['robustness_eval'] = pkg
    if not hasattr(np, 'infty'):
        np.infty = np.inf
    for name in ('robustness_eval._ssa_core', 'robustness_eval._Kenan'):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].ssa = sys.modules[name].inv_ssa = sys.modules[name].atk_bst = None
    mod = importlib.import_module('robustness_eval.black_box_attack')
    assert mod.__file__.startswith(mg.REF) and sys.modules['robustness_eval._KenanFFT'].__file__.startswith(mg.REF)
    return mod.Kenansville


class Recorder(torch.nn.Module):
    """The model, and what the attack's loop held when it asked: the factors (from the calling frame) and the arg-max of the answer."""

    def __init__(self, model):
        super().__init__()
        self.model, self.factors, self.preds, self.margin = model, [], [], float('inf')

    def forward(self, x):
        out = self.model(x)
        top = out.topk(2, 1).values
        scale = (x[:, 0].abs() @ self.model.weight.abs().t()).max(1).values            # sum of |products| behind a logit
        self.margin = min(self.margin, float(((top[:, 0] - top[:, 1]) / scale).min()))
        frame = sys._getframe(1)
        while '_attack_factor' not in frame.f_locals:                # up through torch's call wrappers to atk_bst_fft
            frame = frame.f_back
        self.factors.append(frame.f_locals['_attack_factor'].numpy().copy())
        self.preds.append(out.max(1)[1].numpy().copy())
        return out


def main():
    torch.set_num_threads(1)
    from dmad_hip import synth
    Kenansville = reference_kenansville()
    W = model_weight()
    model = StridedAverageLinear(W).eval()
    x = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in CLIP_IDS])).float()
    with torch.no_grad():
        clean = model(x).argmax(1)
    y = clean.clone()
    rec = Recorder(model).eval()
    att = Kenansville(rec, **SETTINGS)
    with torch.no_grad():
        adver_x, succ = att.generate(x, y, targeted=False)
    factors, preds = np.stack(rec.factors), np.stack(rec.preds)
    T = SETTINGS['max_iter']
    assert factors.shape == preds.shape == (T, N_CLIPS) and factors.dtype == np.float32
    won = preds != y.numpy()[None, :]
    print('labels', y.tolist())
    print('predictions\n', preds, '\nwon\n', won.astype(int), '\nfactors\n', factors, '\nsucc', succ)
    assert won.any() and (~won).any(), 'one bisection branch never ran'
    later_fail = [i for i in range(N_CLIPS) if any(won[t, i] and (~won[t + 1:, i]).any() for t in range(T))]
    assert later_fail, 'no clip succeeds and fails later: choose other labels'
    assert any(succ) and not all(succ), 'one final state of succ is missing: choose other labels'
    X = np.fft.rfft(x[:, 0].double().numpy(), axis=1)
    fp32 = np.abs(torch.fft.rfft(x[:, 0], dim=1).numpy() - X).max(1)
    gap = np.array([np.abs(np.abs(X) - factors[t].astype(np.float64)[:, None]).min(1) / fp32 for t in range(T)])
    print('closest bin to a visited factor, in fp32 errors of torch.fft:', gap.min(0))
    assert gap.min() > 1000
    print('smallest top-2 margin, as a share of the sum of absolute products: %.2e' % rec.margin)
    assert rec.margin > 1e-3
    for i in range(N_CLIPS):
        assert bool(succ[i]) == bool(won[:, i].any())
        if not succ[i]:
            assert torch.equal(adver_x[i], x[i])
    path = os.path.join(HERE, 'kenansville.npz')
    np.savez_compressed(path, model_gain=np.array(MODEL_GAIN), model_shape=np.array([CLASSES, FEATURES]), weight_corner=W[:, :8].numpy(),
                        weight_sum=np.array(float(W.double().sum())), clip_ids=np.array(CLIP_IDS), y=y.numpy(),
                        adver_x=adver_x.numpy(), succ=np.array(succ), factors=factors, preds=preds, later_fail=np.array(later_fail),
                        model_seed=np.array(MODEL_SEED), settings=np.array(json.dumps(SETTINGS, sort_keys=True)))
    assert os.path.getsize(path) < 1 << 20, 'a committed fixture stays under 1 MiB'


if __name__ == '__main__':
    main()
