"""CPU tests of the VGG19_bn VJP surface: the C ABI and its binding, VGG.grad_backend and its routing on a scripted engine, and the
float64 references of tests/test_gpu_vgg_vjp.py (tests/vgg_vjp_cases.py) against plain float64 autograd."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vgg_vjp_cases as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
LIB = os.path.join(PKG, 'libdmad_hip.so')
NEW_EXPORTS = ('dmad_reserve_vgg_vjp', 'dmad_vgg_vjp', 'dmad_vgg_vjp_tape', 'dmad_vgg_pool_relu_bwd')


@pytest.fixture(scope='module')
def built_lib():
    if not os.path.exists(LIB):
        subprocess.run(['make', '-C', os.path.join(PKG, 'csrc'), '-j4'], check=True)
    return ctypes.CDLL(LIB)


def test_vgg_vjp_exports(built_lib):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dmad.h')).read(), flags=re.S)
    from dmad_hip import _lib
    for name in NEW_EXPORTS:
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr), name
        assert hasattr(built_lib, name), name
        assert name in _lib.EXPORTS, name
    sig = _lib._SIGNATURES
    assert sig['dmad_vgg_vjp'] == sig['dmad_classify_vjp'] and sig['dmad_reserve_vgg_vjp'] == sig['dmad_reserve_classifier_vjp']
    assert len(sig['dmad_vgg_vjp_tape'][1]) == 5 and len(sig['dmad_vgg_pool_relu_bwd'][1]) == 7
    from dmad_hip import engine as E
    for name in ('reserve_vgg_vjp', 'vgg_vjp', 'vgg_vjp_tape'):
        assert callable(getattr(E.Engine, name)), name
    assert len(E.VGG_TAPE_MAPS) == 16 and sum(h * h * c for h, c in E.VGG_TAPE_MAPS) + 2 * 4096 == 311296


def test_vgg_grad_backend(monkeypatch):
    from audio_models.ConvNets_SpeechCommands.models.vgg import vgg19_bn
    from dmad_hip import autograd as ag
    m = vgg19_bn(num_classes=10, in_channels=1).eval()
    assert m.GRAD_BACKENDS == ('auto', 'torch', 'hip') and m.grad_backend == 'auto'
    with pytest.raises(ValueError):
        m.grad_backend = 'cuda'
    assert m.grad_backend == 'auto'
    called = []
    monkeypatch.setattr(ag, 'vgg_hip', lambda eng, x: called.append(eng) or 'hip')
    m.__dict__['engine'] = 'ENGINE'
    x = torch.zeros(2, 1, 32, 32, requires_grad=True)
    for backend in ('auto', 'torch'):                   # the torch branch: the module's own layers (no CPU path -> refused there)
        m.grad_backend = backend
        assert m.grad_backend == backend
        with pytest.raises(NotImplementedError, match='no CPU path'):
            m(x)
    assert not called
    m.grad_backend = 'hip'
    assert m.grad_backend == 'hip'
    assert m(x) == 'hip' and called == ['ENGINE']
    with torch.no_grad():                               # no gradient asked for: not the VJP's Function
        monkeypatch.setitem(m.__dict__, 'engine', type('Eng', (), {'classify': staticmethod(lambda x: 'classify')})())
        assert m(x) == 'classify' and called == ['ENGINE']


def test_vgg_hip_function_on_a_scripted_engine():
    """VGGHIP saves only the input, its forward is classify_tier(., 0) and its backward one vgg_vjp call, after growing the reservation"""
    from dmad_hip import autograd as ag

    class Eng:
        max_batch, vgg_vjp_batch, log = 8, 0, []

        def classify_tier(self, spec, tier):
            self.log.append(('classify_tier', tier))
            return spec.reshape(spec.shape[0], -1)[:, :10] * 2.0

        def reserve_vgg_vjp(self, n):
            self.log.append(('reserve', n))
            self.vgg_vjp_batch = n

        def vgg_vjp(self, spec, g):
            self.log.append(('vgg_vjp', tuple(g.shape)))
            return torch.full((spec.shape[0], 32, 32), 3.0)

    eng = Eng()
    monkey = pytest.MonkeyPatch()
    monkey.setattr(ag, '_require_cuda', lambda t: None)
    try:
        x = torch.zeros(3, 1, 32, 32, requires_grad=True)
        out = ag.vgg_hip(eng, x)
        (gx,) = torch.autograd.grad(out.sum(), x)
        (gx2,) = torch.autograd.grad(ag.vgg_hip(eng, x).sum(), x)
    finally:
        monkey.undo()
    assert eng.log == [('classify_tier', 0), ('reserve', 3), ('vgg_vjp', (3, 10)), ('classify_tier', 0), ('vgg_vjp', (3, 10))]
    assert tuple(gx.shape) == (3, 1, 32, 32) and bool((gx == 3.0).all()) and torch.equal(gx, gx2)


@pytest.mark.parametrize('B,H,C', [(3, 4, 64), (2, 2, 512)])
def test_pool_relu_bwd_reference(B, H, C):
    """The pool + ReLU backward reference against float64 autograd of max_pool2d(relu(.)) wherever autograd's answer is defined by the
    rule (no tie at the maximum), the tie rule where it is not, and the case's own coverage."""
    y, g = V.pool_case(B, H, C, seed=H)
    ref = V.pool_relu_bwd_ref(g, y)
    w = V.windows(y.permute(0, 3, 1, 2))
    rw = V.windows(ref.permute(0, 3, 1, 2))
    top = w.max(-1, keepdim=True).values
    ties = (w == top).sum(-1)
    # torch's own backward on the post-ReLU map (the kernel's input): y = relu(pre) with pre = y where y > 0
    pre = y.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    (auto,) = torch.autograd.grad(F.max_pool2d(torch.relu(pre), 2, 2), pre, g.double().permute(0, 3, 1, 2))
    single = (ties == 1).unsqueeze(-1).expand_as(w)
    assert torch.equal(rw[single], V.windows(auto)[single])
    # the rule, window by window: everything to the first maximum if it is > 0, zeros elsewhere
    a = V.first_max(w)
    gg = g.double().permute(0, 3, 1, 2)
    assert torch.equal(rw.gather(-1, a.unsqueeze(-1)).squeeze(-1), torch.where(top.squeeze(-1) > 0, gg, torch.zeros_like(gg)))
    assert bool(((rw != 0).sum(-1) <= 1).all())
    assert bool((rw.sum(-1)[top.squeeze(-1) <= 0] == 0).all())
    # coverage: a positive tie in every pair of positions won by the earlier one, zero and negative windows, every position wins
    pos = top.squeeze(-1) > 0
    for p in range(4):
        assert bool(((a == p) & pos & (ties == 1)).any()), p
        for q in range(p + 1, 4):
            tie_pq = (w[..., p] == top.squeeze(-1)) & (w[..., q] == top.squeeze(-1)) & (ties == 2) & pos
            assert bool(tie_pq.any()), (p, q)
            assert bool((a[tie_pq] == p).all()) and bool((rw[..., q][tie_pq] == 0).all()) and bool((rw[..., p][tie_pq] != 0).all())
    assert bool((w == 0).all(-1).any()) and bool((top.squeeze(-1) < 0).any()) and bool(((top.squeeze(-1) == 0) & (w < 0).any(-1)).any())
    assert bool((ties == 4).any()) and bool((ties == 3).any())


@pytest.fixture(scope='module')
def net():
    from dmad_hip import synth
    return V.sd64(synth.vgg19_bn_state_dict(V.VGG_SEED))


@pytest.mark.parametrize('B,seed', [(2, 1), (3, 12)])
def test_pinned_walk_is_self_consistent(net, B, seed):
    """Pinned to its own float64 decisions the walk is the oracle's VGG19_bn: same logits, and its VJP equals torch.autograd.grad of
    oracle.dmad_oracle.vgg19_bn_forward to 1e-12.  The decisions read back from the free walk's maps (as the GPU test reads them from
    the engine's tape) are the free walk's own."""
    from oracle import dmad_oracle as orc
    x = V.specs(B, seed).double()
    logits, rec = V.vgg_walk(net, x)
    ref = orc.vgg19_bn_forward(net, x)
    assert V.relmax(logits, ref) <= 1e-12
    masks, args = V.tape_decisions(rec['maps'])
    assert all(torch.equal(a, b) for a, b in zip(masks, rec['masks'])) and all(torch.equal(a, b) for a, b in zip(args, rec['args']))
    assert len(masks) == 18 and len(args) == 5 and V.pool_input_index() == [1, 3, 7, 11, 15]
    for k in range(3):
        g = torch.randn(B, 10, generator=torch.Generator().manual_seed(10 + k))
        xr = x.clone().requires_grad_(True)
        (want,) = torch.autograd.grad((orc.vgg19_bn_forward(net, xr) * g.double()).sum(), xr)
        got, prec = V.pinned_vjp(net, x, g, (masks, args))
        assert V.relmax(got, want[:, 0]) <= 1e-12, k
        assert all(torch.equal(a, b) for a, b in zip(prec['maps'], rec['maps']))


def test_pinned_walk_follows_the_given_decisions(net):
    """A pinned decision is obeyed, not recomputed: with one ReLU unit switched and one pool window moved to another entry the walk's map
    and its VJP change."""
    x = V.specs(2, 1).double()
    _, rec = V.vgg_walk(net, x)
    masks = [m.clone() for m in rec['masks']]
    args = [a.clone() for a in rec['args']]
    on = rec['masks'][3].nonzero()[0]
    masks[3][tuple(on)] = False
    args[0][0, 0, 0, 0] = (args[0][0, 0, 0, 0] + 1) % 4
    g = torch.randn(2, 10, generator=torch.Generator().manual_seed(3))
    base, _ = V.pinned_vjp(net, x, g, (rec['masks'], rec['args']))
    moved, prec = V.pinned_vjp(net, x, g, (masks, args))
    assert float(prec['maps'][3][tuple(on)].detach()) == 0.0 and float(rec['maps'][3][tuple(on)]) > 0.0
    assert not torch.equal(base, moved)
    assert torch.equal(prec['args'][0], args[0]) and torch.equal(prec['masks'][3], masks[3])


def test_stand_in_is_not_vacuous(net):
    """On the GPU test's inputs the committed stand-in's decisions vary: between 5 % and 95 % of every conv layer's units are on, the
    masks differ between batch rows, and all four window positions win in every pool layer."""
    for B, seed in ((2, 1), (3, 12)):
        _, rec = V.vgg_walk(net, V.specs(B, seed).double())
        for k in range(16):
            frac = float(rec['masks'][k].double().mean())
            assert 0.05 < frac < 0.95, (seed, k, frac)
            assert not torch.equal(rec['masks'][k][0], rec['masks'][k][1]), (seed, k)
        for j, a in enumerate(rec['args']):
            assert sorted(np.unique(a.numpy()).tolist()) == [0, 1, 2, 3], (seed, j)
