#!/usr/bin/env python3
"""BUILD-CONTAINER-ONLY generator of tests/golden/siren.npz: a short run of the imported reference's
`robustness_eval.black_box_attack.SirenAttack` (l.313-580) on the CPU, under np.random.seed, against the small deterministic model of
make_golden_fakebob.py — a fixed-seed linear map of a strided average of the clip to 10 classes, its weights stored in the fixture.

n = 3 clips of dmad_hip.synth.synthetic_clip, n_particles = 4, max_epoch = 3, max_iter = 4, abort_early_iter = 2, abort_early_epoch = 2.
The labels are classes the model does NOT give the clips: the loss is the cross-entropy of that label (resolve_loss returns it for
task 'SCR' whatever is asked for), so it is large, positive and different for every particle, and the swarm has something to lower.
epsilon is 5e-6: at the driver's 0.002 this swarm lowers the loss by several percent per move and the 0.01 % convergence test never
fires in a run this short; at 5e-6 two moves gain about that much, and (numpy seed 3) the test fires in the second epoch at iteration 3
and in the third at iteration 1, while the first epoch runs to its end.
Three events are asserted, and the evaluation at which each first shows is recorded:
  * a global best that improves after the first evaluation of an epoch (the swarm moves, and the move is scored);
  * an inner "Converge" break (an epoch of fewer than max_iter + 1 evaluations);
  * a second epoch, which starts from the carried best: its first evaluation cannot raise any global best.

Recorded: adver_x, success, and per evaluation (taken by wrapping delete_found, the reference is not edited: the wrapper reads `epoch`
and `iter` from the calling frame) the gbests of the working clips, consider_index, epoch and iteration, padded to n columns with
NaN / -1.  Also one direct call of the reference's delete_found on crafted inputs with two negative entries among five, inputs and
outputs.

Harness shims, all of them here: the reference's robustness_eval has no __init__.py, so it is mounted as a package of its own;
_Kenan / _KenanFFT are stubbed when they do not import; numpy.infty (removed in numpy 2) is given back as numpy.inf.

Usage:  python tests/golden/make_golden_siren.py
"""
import contextlib
import importlib
import io
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
MODEL_SEED, MODEL_GAIN, NUMPY_SEED = 77, 400.0, 3
LABEL_SHIFT = (3, 5, 7)                       # label of clip i = (the model's class + LABEL_SHIFT[i]) % 10
SETTINGS = dict(task='SCR', targeted=False, confidence=0., epsilon=5e-6, max_epoch=3, max_iter=4, c1=1.4961, c2=1.4961, n_particles=4,
                w_init=0.9, w_end=0.1, batch_size=N_CLIPS, EOT_size=1, EOT_batch_size=1, verbose=0, abort_early=True, abort_early_iter=2,
                abort_early_epoch=2)


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


def reference_siren():
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
    return mod.SirenAttack


def crafted_delete_found(SirenAttack):
    """One direct call of the reference's delete_found: five working clips, the second and the fourth found."""
    gen = torch.Generator().manual_seed(11)
    P, N = 2, 8
    gbests = torch.tensor([0.5, -0.1, 2.0, -3.0, 0.0])
    args = dict(x_batch=torch.randn(5, 1, N, generator=gen), y_batch=torch.tensor([4, 1, 0, 9, 2]), lower=-torch.rand(5, 1, N, generator=gen),
                upper=torch.rand(5, 1, N, generator=gen), pbest_locations=torch.randn(5, P, 1, N, generator=gen),
                locations=torch.randn(5, P, 1, N, generator=gen), volicities=torch.randn(5, P, 1, N, generator=gen),
                pbests=torch.rand(5, P, generator=gen))
    consider_index = [0, 2, 3, 5, 7]
    out = SirenAttack(None).delete_found(gbests, *args.values(), consider_index)
    rec = {'df_gbests': gbests.numpy(), 'df_consider_index': np.array(consider_index), 'df_out_consider_index': np.array(out[8])}
    for (name, t), o in zip(args.items(), out[:8]):
        rec['df_' + name] = t.numpy()
        rec['df_out_' + name] = o.numpy()
    assert rec['df_out_consider_index'].tolist() == [0, 3, 7]
    return rec


def main():
    torch.set_num_threads(1)
    from dmad_hip import synth
    SirenAttack = reference_siren()
    W = model_weight()
    model = StridedAverageLinear(W).eval()
    x = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in range(N_CLIPS)])).float()
    with torch.no_grad():
        clean = model(x).argmax(1)
    y = (clean + torch.tensor(LABEL_SHIFT)) % CLASSES
    att = SirenAttack(model, **SETTINGS)
    trace = []
    inner = att.delete_found

    def delete_found(gbests, *rest):
        caller = sys._getframe(1).f_locals
        trace.append((gbests.numpy().copy(), list(rest[-1]), int(caller['epoch']), int(caller['iter'])))
        return inner(gbests, *rest)
    att.delete_found = delete_found
    np.random.seed(NUMPY_SEED)
    said = io.StringIO()
    with contextlib.redirect_stdout(said):
        adver_x, success = att.generate(x, y, targeted=False)

    T = len(trace)
    gbests = np.full((T, N_CLIPS), np.nan, np.float32)
    consider = np.full((T, N_CLIPS), -1, np.int64)
    epoch, it = np.zeros(T, np.int64), np.zeros(T, np.int64)
    for t, (g, ci, ep, i) in enumerate(trace):
        gbests[t, :len(ci)], consider[t, :len(ci)], epoch[t], it[t] = g, ci, ep, i
    improved = [t for t in range(1, T) if it[t] > 0 and (gbests[t] < gbests[t - 1]).any()]
    per_epoch = [int((epoch == e).sum()) for e in range(int(epoch.max()) + 1)]
    short = [e for e, c in enumerate(per_epoch) if c < SETTINGS['max_iter'] + 1]
    second = [t for t in range(T) if epoch[t] == 1]
    assert improved, 'no global best improved after the first evaluation of an epoch: choose another seed'
    assert short and 'Converge, Break Inner Loop' in said.getvalue(), 'no inner convergence break happened: choose another seed'
    assert second and it[second[0]] == 0 and (gbests[second[0]] <= gbests[second[0] - 1]).all(), 'no second epoch from the carried best'
    assert (gbests > 0).all() and not any(success), 'cross-entropy is never negative'
    converge_at = int(np.nonzero(epoch == short[0])[0][-1])
    print('evaluations %d, per epoch %s, first improvement after a move at %d, inner break after %d, second epoch starts at %d' % (
        T, per_epoch, improved[0], converge_at, second[0]))
    print('gbests', gbests)
    np.savez_compressed(os.path.join(HERE, 'siren.npz'), weight=W.numpy(), clip_ids=np.arange(N_CLIPS), y=y.numpy(),
                        adver_x=adver_x.numpy(), success=np.array(success), gbests=gbests, consider_index=consider, epoch=epoch, iteration=it,
                        improved_at=np.array(improved[0]), converge_at=np.array(converge_at), second_epoch_at=np.array(second[0]),
                        numpy_seed=np.array(NUMPY_SEED), model_seed=np.array(MODEL_SEED),
                        settings=np.array(json.dumps(SETTINGS, sort_keys=True)), **crafted_delete_found(SirenAttack))


if __name__ == '__main__':
    main()
