"""CPU tests of the white-box attack driver and the classifier-side VJP surface: the C ABI and its binding, the grad_backend switches of
CifarResNeXt and MelSpectrogramDB, AudioAttack stage 1 against an independent restatement of its loop on a small CPU model, the EOT
gradient path, the refusals, and the driver's flags."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
LIB = os.path.join(PKG, 'libdmad_hip.so')
NEW_EXPORTS = ('dmad_reserve_classifier_vjp', 'dmad_classify_vjp', 'dmad_mel_db_vjp')


@pytest.fixture(scope='module')
def built_lib():
    if not os.path.exists(LIB):
        subprocess.run(['make', '-C', os.path.join(PKG, 'csrc'), '-j4'], check=True)
    return ctypes.CDLL(LIB)


def test_classifier_vjp_exports(built_lib):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dmad.h')).read(), flags=re.S)
    from dmad_hip import _lib
    for name in NEW_EXPORTS:
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr), name
        assert hasattr(built_lib, name), name
        assert name in _lib.EXPORTS, name
    assert len(_lib._SIGNATURES['dmad_classify_vjp'][1]) == 7 and len(_lib._SIGNATURES['dmad_mel_db_vjp'][1]) == 7


def test_resnext_grad_backend(monkeypatch):
    from audio_models.ConvNets_SpeechCommands.models.resnext import CifarResNeXt
    from dmad_hip import autograd as ag
    m = CifarResNeXt(nlabels=10, in_channels=1).eval()
    assert m.grad_backend == 'auto'
    with pytest.raises(ValueError):
        m.grad_backend = 'cuda'
    assert m.grad_backend == 'auto'
    called = []
    monkeypatch.setattr(ag, 'resnext_hip', lambda eng, x: called.append(eng) or 'hip')
    m.__dict__['engine'] = 'ENGINE'
    x = torch.zeros(2, 1, 32, 32, requires_grad=True)
    for backend in ('auto', 'torch'):                   # the torch branch: the module's own layers (no CPU path -> refused there)
        m.grad_backend = backend
        with pytest.raises(NotImplementedError, match='no CPU path'):
            m(x)
    assert not called
    m.grad_backend = 'hip'
    assert m(x) == 'hip' and called == ['ENGINE']


def test_mel_grad_backend(monkeypatch):
    from dmad_hip import autograd as ag
    from dmad_hip.transforms import MelSpectrogramDB
    with pytest.raises(ValueError):
        MelSpectrogramDB('ENGINE', grad_backend='gpu')
    t = MelSpectrogramDB('ENGINE')
    assert t.grad_backend == 'auto'
    monkeypatch.setattr(ag, 'mel_db', lambda x: 'torch')
    monkeypatch.setattr(ag, 'mel_db_hip', lambda eng, x: 'hip:' + eng)
    x = torch.zeros(1, 1, 16000, requires_grad=True)
    assert t(x) == 'torch'
    assert MelSpectrogramDB('ENGINE', grad_backend='torch')(x) == 'torch'
    assert MelSpectrogramDB('ENGINE', grad_backend='hip')(x) == 'hip:ENGINE'


class _Tiny(torch.nn.Module):
    """[n, 1, L] -> [n, 10] linear model that records every input it sees."""

    def __init__(self, L, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = torch.nn.Parameter(torch.randn(10, L, generator=g) * 0.5)
        self.seen = []

    def forward(self, x):
        self.seen.append(x.detach().clone())
        return x[:, 0] @ self.w.t()


def _restated_stage_1(model, x, y, eps, lr, norm, targeted, iters, every, factor):
    """Stage 1 written out independently: batched projections, per-example bounds as a float64 vector."""
    s = 2.0 ** -15
    n = x.shape[0]
    e = torch.full((n,), eps * s, dtype=torch.float64)
    step = lr * s
    d = torch.zeros_like(x)
    best = [None] * n
    for i in range(iters + 1):
        xp = (x + d).requires_grad_(True)
        out = model(xp)
        ok = (out.argmax(1) == y) if targeted else (out.argmax(1) != y)
        for j in torch.nonzero(ok).view(-1).tolist():
            best[j] = (x[j] + d[j]).clone()
        if i > 0 and i % every == 0:
            for j in torch.nonzero(ok).view(-1).tolist():
                nj = float(d[j].abs().max()) if norm == 'linf' else float(torch.norm(d[j], dim=(1,)))
                e[j] = min(float(e[j]), nj) * factor
        if i == iters:
            break
        (g,) = torch.autograd.grad(torch.nn.functional.cross_entropy(out, y), xp)
        d = d - step * g.sign() if targeted else d + step * g.sign()
        e32 = e.float()[:, None, None]
        if norm == 'linf':
            d = torch.max(torch.min(d, e32), -e32)
        else:
            nrm = torch.stack([torch.norm(d[j:j + 1], dim=(1, 2))[0] for j in range(n)])[:, None, None]
            d = d * torch.min(torch.ones_like(nrm), e32 / nrm)
        d = (x + d).clamp(-1, 1) - x
    ok = [b is not None for b in best]
    final = x + d
    return torch.stack([best[j] if ok[j] else final[j] for j in range(n)]), ok


@pytest.mark.parametrize('norm', ['linf', 'l2'])
@pytest.mark.parametrize('targeted', [False, True])
def test_stage_1_against_restatement(norm, targeted):
    from robustness_eval.white_box_attack import AudioAttack
    L, n = 64, 6
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(n, 1, L, generator=g) * 1.8 - 0.9).float()
    x[0, 0, :4] = 0.999                                  # the [-1, 1] box binds
    y = torch.tensor([0, 1, 2, 3, 4, 5]) if not targeted else torch.tensor([7, 7, 3, 3, 1, 1])
    eps = 1500.0 if norm == 'linf' else 9000.0
    lr = eps / 5 if norm == 'linf' else eps / 50
    m1, m2 = _Tiny(L, 11), _Tiny(L, 11)
    att = AudioAttack(m1, eps=eps, norm=norm, learning_rate_1=lr, max_iter_1=12, max_iter_2=0, eot_attack_size=1, eot_defense_size=1,
                      verbose=0)
    x_adv, (succ, second) = att.generate(x, y, targeted=targeted)
    ref_adv, ref_succ = _restated_stage_1(m2, x, y, eps, lr, norm, targeted, 12, 10, 0.8)
    assert second is None and succ == ref_succ
    assert any(succ) and len(m1.seen) == len(m2.seen) == 13
    for a, b in zip(m1.seen, m2.seen):                   # the delta trajectory, iteration by iteration
        torch.testing.assert_close(a, b, rtol=0, atol=1e-6)
    torch.testing.assert_close(x_adv, ref_adv, rtol=0, atol=1e-6)
    assert x_adv.shape == x.shape and float(x_adv.abs().max()) <= 1.0
    d = x_adv - x
    if norm == 'linf':
        assert float(d.abs().max()) <= eps * 2 ** -15 + 1e-6          # + the rounding of (x + d) - x
    else:
        assert float(torch.norm(d, dim=(1, 2)).max()) <= eps * 2 ** -15 * (1 + 1e-5)


def test_stage_1_eot_gradient_path():
    from robustness_eval.white_box_attack import AudioAttack
    L, n = 32, 3
    x = (torch.rand(n, 1, L, generator=torch.Generator().manual_seed(1)) - 0.5).float()
    m = _Tiny(L, 5)
    att = AudioAttack(m, eps=2000, norm='linf', learning_rate_1=400, max_iter_1=3, max_iter_2=0, eot_attack_size=2, eot_defense_size=1,
                      verbose=0)
    x_adv, (succ, _) = att.generate(x, torch.tensor([0, 1, 2]), targeted=False)
    assert x_adv.shape == x.shape and len(succ) == n
    assert float((m.seen[-1] - x).abs().max()) > 0       # the EOT gradient moved delta
    att2 = AudioAttack(_Tiny(L, 5), eps=2000, norm='linf', learning_rate_1=400, max_iter_1=3, max_iter_2=0, eot_attack_size=2,
                       eot_defense_size=2, verbose=0)
    att2.generate(x, torch.tensor([0, 1, 2]), targeted=False)


def test_attack_refusals():
    from robustness_eval.white_box_attack import AudioAttack, lp_norm, project_to_norm_ball
    m = _Tiny(8, 0)
    with pytest.raises(NotImplementedError):
        AudioAttack(m, norm='l1', eot_attack_size=1, eot_defense_size=1)
    with pytest.raises(NotImplementedError):
        AudioAttack(m, max_iter_2=5, eot_attack_size=1, eot_defense_size=1).generate(torch.zeros(1, 1, 8), torch.tensor([0]))
    with pytest.raises(NotImplementedError):
        AudioAttack(m, masker=object(), max_iter_2=5, eot_attack_size=1, eot_defense_size=1).generate(torch.zeros(1, 1, 8), torch.tensor([0]))
    x_adv, (succ, second) = AudioAttack(m, masker=object(), max_iter_1=2, max_iter_2=0, eot_attack_size=1, eot_defense_size=1,
                                        verbose=0).generate(torch.zeros(1, 1, 8), torch.tensor([0]))   # a masker alone: stage 1 runs
    assert x_adv.shape == (1, 1, 8) and len(succ) == 1 and second is None
    with pytest.raises(NotImplementedError):
        lp_norm(torch.zeros(2, 3), 'l1')
    with pytest.raises(NotImplementedError):
        project_to_norm_ball(torch.zeros(1, 1, 3), 'l1', 1.0)
    assert float(lp_norm(torch.tensor([[3.0, -4.0]]), 'l2')) == 5.0 and float(lp_norm(torch.tensor([[3.0, -4.0]]), 'linf')) == 4.0


REFERENCE_FLAGS = {
    'data_path': 'datasets/speech_commands/test', 'classifier_model': 'resnext29_8_64', 'classifier_type': 'vanilla',
    'classifier_input': 'mel32', 'num_per_class': 10, 'ddpm_config': 'configs/config.json',
    'ddpm_path': 'diffusion_models/DiffWave_Unconditional/exp/ch256_T200_betaT0.02/logs/checkpoint/1000000.pkl', 'sample_step': 1, 't': 1,
    't_delta': 15, 'rand_t': False, 'diffusion_type': 'ddpm', 'score_type': 'guided_diffusion', 'use_bm': False, 'attack': 'CW',
    'defense': 'None', 'bound_norm': 'linf', 'eps': 65, 'max_iter_1': 10, 'max_iter_2': 0, 'eot_attack_size': 1, 'eot_defense_size': 1,
    'verbose': 1, 'dataload_workers_nums': 8, 'batch_size': 20, 'gpu': 0, 'save_path': None,
}


def test_driver_flags_and_refusals():
    import adaptive_attack_eval as drv
    args = drv.build_parser().parse_args([])
    for k, v in REFERENCE_FLAGS.items():
        assert getattr(args, k) == v, k
    assert args.classifier_path.endswith('jacobian_reg_resnext29_8_64_sgd_plateau_bs96_lr1.0e-02_wd1.0e-02/reg=1e-08-best-robust-acc.pth')
    assert args.grad_backend == 'hip' and args.score_grad is None
    drv.check_supported(args)
    for d in ('Diffusion', 'Diffusion-Spec'):
        drv.check_supported(drv.build_parser().parse_args(['--defense', d]))
    for a in ('Qin-I', 'Kenansville', 'FAKEBOB', 'SirenAttack'):
        with pytest.raises(NotImplementedError, match=a):
            drv.check_supported(drv.build_parser().parse_args(['--attack', a]))
    for d in ('AS', 'MS', 'DS', 'LPF', 'BPF', 'FeCo', 'DefenseGAN'):
        with pytest.raises(NotImplementedError, match=d):
            drv.check_supported(drv.build_parser().parse_args(['--defense', d]))
    with pytest.raises(NotImplementedError):
        drv.check_supported(drv.build_parser().parse_args(['--max_iter_2', '3']))
    with pytest.raises(NotImplementedError):
        drv.check_supported(drv.build_parser().parse_args(['--defense', 'Diffusion-Spec', '--save_path', 'x']))
