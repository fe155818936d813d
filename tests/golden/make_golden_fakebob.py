#!/usr/bin/env python3
"""BUILD-CONTAINER-ONLY generator of tests/golden/fakebob.npz: a short run of the imported reference's
`robustness_eval.black_box_attack.FAKEBOB` (l.13-219) on the CPU, under torch.manual_seed, against a small deterministic model
defined here — a fixed-seed linear map of a strided average of the clip to 10 classes, its weights stored in the fixture.

n = 3 clips of dmad_hip.synth.synthetic_clip, samples_per_draw = 8, max_iter = 12, plateau_length = 3, stop_early_iter = 5, and step
sizes at which a step-size cut (plateau) and a removal by the convergence test (stop_early) both happen while a clip is still being
attacked: without them the fixture would exercise neither the shared loss history nor the index bookkeeping of the removal.  Both
events are asserted and the iteration at which each first shows is recorded.  An untargeted attack on a linear model raises the
loss at every step, and the convergence test removes every clip whose loss did not fall; a clip survives it only where the step is
small against the probes (max_lr 5e-6, min_lr 1e-6 against sigma 1e-3), so that the second-order term of the mean probe loss decides.
With these values clips 0 and 2 leave at the test of iteration 5 and clip 1 moves to position 0, where the next test compares it with
the loss remembered for clip 0.

Recorded: adver_x, success, and per iteration (taken by wrapping get_grad, the reference is not edited: the wrapper reads `lr` and
`consider_index` from the calling frame) adver_loss, y_pred, lr and consider_index, padded to n columns with NaN / -1.

Harness shims, all of them here: the reference's robustness_eval has no __init__.py, so it is mounted as a package of its own;
_Kenan / _KenanFFT are stubbed when they do not import; numpy.infty (removed in numpy 2) is given back as numpy.inf.

Usage:  python tests/golden/make_golden_fakebob.py
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
MODEL_SEED, MODEL_GAIN, TORCH_SEED = 77, 400.0, 1
SETTINGS = dict(task='SCR', targeted=False, confidence=0.5, epsilon=0.002, max_iter=12, max_lr=5e-6, min_lr=1e-6, samples_per_draw=8,
                samples_per_draw_batch_size=8, sigma=1e-3, momentum=0.9, plateau_length=3, plateau_drop=2., stop_early=True,
                stop_early_iter=5, batch_size=N_CLIPS, EOT_size=1, EOT_batch_size=1, verbose=0)


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


def reference_fakebob():
    pkg = types.ModuleType('robustness_eval')
    pkg.__path__ = [os.path.join(mg.REF, 'robustness_eval')]
    sys.modules['robustness_eval'] = pkg
    for name in ('robustness_eval._Kenan', 'robustness_eval._KenanFFT'):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].atk_bst = sys.modules[name].atk_bst_fft = None
    if not hasattr(np, 'infty'):
        np.infty = np.inf
    mod = importlib.import_module('robustness_eval.black_box_attack')
    assert mod.__file__.startswith(mg.REF)
    return mod.FAKEBOB


def main():
    torch.set_num_threads(1)
    from dmad_hip import synth
    FAKEBOB = reference_fakebob()
    W = model_weight()
    model = StridedAverageLinear(W).eval()
    x = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in range(N_CLIPS)])).float()
    with torch.no_grad():
        clean = model(x).argmax(1)
    y = clean.clone()
    y[2] = (clean[2] + 3) % CLASSES          # clip 2 carries a label the model does not give it: `success` from the first probe on
    att = FAKEBOB(model, **SETTINGS)
    trace = []
    inner = att.get_grad

    def get_grad(xb, yb):
        caller = sys._getframe(1).f_locals
        out = inner(xb, yb)
        trace.append((list(caller['consider_index']), list(caller['lr']), out[2].numpy().copy(), np.array(out[4]).copy()))
        return out
    att.get_grad = get_grad
    torch.manual_seed(TORCH_SEED)
    adver_x, success = att.generate(x, y, targeted=False)

    T = len(trace)
    consider = np.full((T, N_CLIPS), -1, np.int64)
    lr = np.full((T, N_CLIPS), np.nan, np.float64)
    adver_loss = np.full((T, N_CLIPS), np.nan, np.float32)
    y_pred = np.full((T, N_CLIPS), -1, np.int64)
    for t, (ci, l, al, yp) in enumerate(trace):
        k = len(ci)
        consider[t, :k], lr[t, :k], adver_loss[t, :k], y_pred[t, :k] = ci, l, al, yp
    live = (consider >= 0).sum(1)
    cut = [t for t in range(T) if np.nanmin(lr[t]) < SETTINGS['max_lr']]
    removed = [t for t in range(1, T) if live[t] < live[t - 1]]
    assert cut, 'no plateau drop happened: choose other step sizes'
    assert removed and live[removed[0]] >= 1, 'no stop_early removal with a survivor happened: choose other step sizes'
    assert removed[0] < T - 1, 'the run ends with the removal: the bookkeeping after it is not exercised'
    print('iterations %d, live %s, first step-size cut seen at %d, first removal seen at %d, success %s' % (T, live.tolist(), cut[0], removed[0], success))
    print('adver_loss', adver_loss)
    np.savez_compressed(os.path.join(HERE, 'fakebob.npz'), weight=W.numpy(), clip_ids=np.arange(N_CLIPS), y=y.numpy(),
                        adver_x=adver_x.numpy(), success=np.array(success), consider_index=consider, lr=lr, adver_loss=adver_loss,
                        y_pred=y_pred, plateau_drop_iter=np.array(cut[0]), stop_early_iter_seen=np.array(removed[0]),
                        torch_seed=np.array(TORCH_SEED), model_seed=np.array(MODEL_SEED),
                        settings=np.array(json.dumps(SETTINGS, sort_keys=True)))


if __name__ == '__main__':
    main()
