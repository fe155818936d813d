"""CPU tests of SirenAttack: the C ABI of the particle-swarm kernels and its binding, SirenAttack(noise_source='numpy') against the
fixture recorded from the reference (tests/golden/siren.npz, made by tests/golden/make_golden_siren.py), the mirror's delete_found
against the reference's, the opt-in margin loss, the refusals, and the flags of siren_attack_eval.py."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
LIB = os.path.join(PKG, 'libdmad_hip.so')
NEW_EXPORTS = {'dmad_philox_uniform': 7, 'dmad_pso_init': 14, 'dmad_pso_step': 17, 'dmad_pso_update_best': 13}   # name -> arguments


@pytest.fixture(scope='module')
def built_lib():
    if not os.path.exists(LIB):
        subprocess.run(['make', '-C', os.path.join(PKG, 'csrc'), '-j4'], check=True)
    return ctypes.CDLL(LIB)


def test_pso_exports(built_lib):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dmad.h')).read(), flags=re.S)
    from dmad_hip import _lib, engine
    for name, nargs in NEW_EXPORTS.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, hdr)
        assert m and len(m.group(1).split(',')) == nargs, name
        assert hasattr(built_lib, name), name
        assert name in _lib.EXPORTS and len(_lib._SIGNATURES[name][1]) == nargs, name
    m = re.search(r'#define\s+DMAD_PHILOX_STREAM_PSO\s+(0x[0-9A-Fa-f]+)u', hdr)
    assert m and int(m.group(1), 16) == engine.PSO_STREAM == 0x50530000
    for method in ('philox_uniform', 'pso_init', 'pso_step', 'pso_update_best'):
        assert callable(getattr(engine.Engine, method)), method


class StridedAverageLinear(torch.nn.Module):
    """The fixture's model: feature f is the mean of the samples f, f + F, f + 2F, ...; logits = features @ W^T."""

    def __init__(self, weight):
        super().__init__()
        self.weight = torch.nn.Parameter(weight, requires_grad=False)

    def forward(self, x):
        F = self.weight.shape[1]
        return x[:, 0].reshape(x.shape[0], -1, F).mean(1) @ self.weight.t()


@pytest.fixture(scope='module')
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, 'siren.npz')) as z:
        return {k: z[k] for k in z.files}


def test_siren_against_the_reference_fixture(golden, capsys):
    from dmad_hip import synth
    from robustness_eval.black_box_attack import SirenAttack
    g = golden
    settings = json.loads(str(g['settings']))
    assert (settings['n_particles'], settings['max_epoch'], settings['max_iter'], settings['abort_early_iter']) == (4, 3, 4, 2)
    # the fixture holds an improvement after a move, an inner convergence break and a second epoch (asserted by its maker)
    T = g['gbests'].shape[0]
    assert 0 < int(g['improved_at']) and int(g['second_epoch_at']) == 5 and T < 3 * 5
    model = StridedAverageLinear(torch.from_numpy(g['weight'])).eval()
    x = torch.from_numpy(np.stack([synth.synthetic_clip(int(i)) for i in g['clip_ids']])).float()
    assert x.shape == (3, 1, 16000)
    y = torch.from_numpy(g['y'])
    att = SirenAttack(model, noise_source='numpy', **settings)
    assert att.loss_name == 'reference'
    trace, inner = [], att.delete_found

    def delete_found(gbests, *rest):                         # the maker's wrapper, on the mirror
        trace.append((gbests.numpy().copy(), list(rest[-1])))
        return inner(gbests, *rest)
    att.delete_found = delete_found
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                 # as the maker ran: the same reduction order inside torch
    try:
        np.random.seed(int(g['numpy_seed']))
        adver_x, success = att.generate(x, y, targeted=False)
    finally:
        torch.set_num_threads(threads)
    assert success == g['success'].tolist() == [False] * 3
    assert len(trace) == T
    for t, (gb, ci) in enumerate(trace):
        k = int((g['consider_index'][t] >= 0).sum())
        assert ci == g['consider_index'][t, :k].tolist(), t
        err = np.abs(gb.astype(np.float64) - g['gbests'][t, :k].astype(np.float64)).max()
        assert err <= 1e-6, (t, err)
    assert capsys.readouterr().out.count('Converge, Break Inner Loop') == 2
    assert adver_x.shape == x.shape
    assert float((adver_x - torch.from_numpy(g['adver_x'])).abs().max()) <= 1e-6


def test_delete_found_against_the_reference_call(golden):
    from robustness_eval.black_box_attack import SirenAttack
    g = golden
    names = ('x_batch', 'y_batch', 'lower', 'upper', 'pbest_locations', 'locations', 'volicities', 'pbests')
    assert int((g['df_gbests'] < 0).sum()) == 2 and g['df_gbests'].shape == (5,)
    out = SirenAttack(None).delete_found(torch.from_numpy(g['df_gbests']), *[torch.from_numpy(g['df_' + n]) for n in names],
                                         g['df_consider_index'].tolist())
    assert len(out) == 9 and out[8] == g['df_out_consider_index'].tolist()
    for n, o in zip(names, out):
        want = torch.from_numpy(g['df_out_' + n])
        assert o.dtype == want.dtype and torch.equal(o, want), n
    gone = SirenAttack(None).delete_found(torch.tensor([-1.0, -2.0]), *[torch.from_numpy(g['df_' + n])[:2] for n in names], [4, 6])
    assert gone[8] == [] and all(o is None for o in gone[:8])


def test_margin_loss_against_the_formula():
    """score_real + confidence - max other score, per row, in float64; the sign flipped when targeted."""
    from robustness_eval._utils import MarginLoss
    scores = torch.tensor([[2.0, -1.0, 0.5, 1.5],           # the label leads by 0.5
                           [0.25, 3.0, -2.0, 3.0],          # a tie between the label and another class
                           [-5.0, -7.0, -6.0, -9.0],        # all scores negative, label last among them
                           [1.0, 4.0, 2.0, -3.0]], dtype=torch.float64)            # misclassified: another class leads by 2
    label = torch.tensor([0, 1, 3, 2])
    conf = 0.125
    want = []
    for row, l in zip(scores.tolist(), label.tolist()):
        want.append(row[l] + conf - max(v for j, v in enumerate(row) if j != l))
    assert want == [0.625, 0.125, -3.875, -1.875]
    got = MarginLoss(False, conf)(scores, label)
    assert got.dtype == torch.float64 and got.tolist() == want
    assert MarginLoss(True, conf)(scores, label).tolist() == [2 * conf - w for w in want]
    assert (MarginLoss(False, 0.)(scores, label) < 0).tolist() == [False, False, True, True]


def test_margin_loss_makes_the_removal_live():
    """With loss='margin' a misclassified clip has a negative loss at its first evaluation: it leaves the working batch and `success`
    is True for it; with the default loss nothing ever leaves."""
    from robustness_eval.black_box_attack import SirenAttack
    model = StridedAverageLinear(torch.randn(10, 64, generator=torch.Generator().manual_seed(0)) * 100).eval()
    x = torch.rand(3, 1, 128, generator=torch.Generator().manual_seed(1)) - 0.5
    with torch.no_grad():
        top2 = model(x).topk(2, 1).indices
    y = top2[:, 0].clone()
    y[1] = top2[1, 1]                                        # clip 1 is mislabelled
    kw = dict(task='SCR', max_epoch=1, max_iter=2, n_particles=3, batch_size=3, verbose=0, epsilon=1e-7)
    seen = []
    att = SirenAttack(model, loss='margin', **kw)
    inner = att.delete_found
    att.delete_found = lambda *a: (seen.append(list(a[-1])), inner(*a))[1]
    np.random.seed(0)
    adver_x, success = att.generate(x, y)
    assert success == [False, True, False] and seen[0] == [0, 1, 2] and seen[1:] == [[0, 2]] * 2
    assert adver_x.shape == x.shape and float((adver_x - x).abs().max()) <= 1e-7 + 2.0 ** -24
    np.random.seed(0)
    assert SirenAttack(model, **kw).generate(x, y)[1] == [False] * 3


def test_refusals():
    from dmad_hip._lib import DmadError
    from robustness_eval.black_box_attack import SirenAttack
    model = StridedAverageLinear(torch.zeros(10, 64))
    with pytest.raises(ValueError):
        SirenAttack(model, noise_source='torch')
    with pytest.raises(ValueError):
        SirenAttack(model, loss='Entropy')
    with pytest.raises(DmadError):
        SirenAttack(model, noise_source='device')
    att = SirenAttack(model)
    assert (att.noise_source, att.loss_name, att.seed, att._draws, att.engine) == ('numpy', 'reference', 0, 0, None)
    assert (att.epsilon, att.max_epoch, att.max_iter, att.n_particles, att.c1, att.c2, att.w_init, att.w_end, att.confidence) == \
        (0.002, 300, 30, 25, 1.4961, 1.4961, 0.9, 0.1, 0.)
    assert (att.task, att.batch_size, att.abort_early, att.abort_early_iter, att.abort_early_epoch) == ('CSI', 1, True, 10, 10)
    x, y = torch.zeros(1, 1, 64), torch.tensor([0])
    with pytest.raises(NotImplementedError):
        SirenAttack(model, task='SV').generate(x, y)
    with pytest.raises(NotImplementedError):
        SirenAttack(model, task='SV', threshold=0.5).generate(x, y)          # a threshold, but no loss for the task
    with pytest.raises(NotImplementedError):
        SirenAttack(model, task='SV', threshold=0.5, loss='margin').generate(x, y)


REFERENCE_FLAGS = {
    'data_path': 'datasets/speech_commands/test', 'classifier_model': 'resnext29_8_64', 'classifier_type': 'vanilla',
    'classifier_input': 'mel32', 'num_per_class': 10, 'ddpm_config': 'configs/config.json',
    'ddpm_path': 'diffusion_models/DiffWave_Unconditional/exp/ch256_T200_betaT0.02/logs/checkpoint/1000000.pkl', 'sample_step': 1, 't': 1,
    't_delta': 15, 'rand_t': False, 'diffusion_type': 'ddpm', 'score_type': 'guided_diffusion', 'use_bm': False, 'attack': 'CW',
    'defense': 'None', 'bound_norm': 'linf', 'eps': 65, 'max_iter_1': 10, 'max_iter_2': 0, 'eot_attack_size': 1, 'eot_defense_size': 1,
    'verbose': 1, 'dataload_workers_nums': 8, 'batch_size': 20, 'gpu': 0, 'save_path': None,
}


def test_driver_flags_and_refusals():
    import siren_attack_eval as drv
    args = drv.build_parser().parse_args([])
    for k, v in REFERENCE_FLAGS.items():
        assert getattr(args, k) == v, k
    assert args.swarm_noise == 'device' and args.seed == 0 and args.siren_loss == 'reference'
    assert drv.ATTACKER_CONSTANTS == dict(epsilon=0.002, max_epoch=300, max_iter=30, n_particles=25)
    for d in ('None', 'Diffusion', 'Diffusion-Spec'):
        drv.check_supported(drv.build_parser().parse_args(['--attack', 'SirenAttack', '--defense', d, '--swarm_noise', 'numpy', '--seed', '3',
                                                           '--siren_loss', 'margin']))
    for a in ('CW', 'Qin-I', 'Kenansville', 'FAKEBOB'):
        with pytest.raises(NotImplementedError, match=a):
            drv.check_supported(drv.build_parser().parse_args(['--attack', a]))
    with pytest.raises(NotImplementedError, match='DefenseGAN'):
        drv.check_supported(drv.build_parser().parse_args(['--attack', 'SirenAttack', '--defense', 'DefenseGAN']))
    with pytest.raises(NotImplementedError):
        drv.run(drv.build_parser().parse_args([]))                        # the default attack is the white-box driver's
    # the two other drivers keep refusing SirenAttack, and say where it runs
    import adaptive_attack_eval
    import black_box_attack_eval
    for other in (adaptive_attack_eval, black_box_attack_eval):
        with pytest.raises(NotImplementedError, match=r'SirenAttack.*siren_attack_eval\.py'):
            other.check_supported(other.build_parser().parse_args(['--attack', 'SirenAttack']))
