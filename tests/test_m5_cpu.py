"""M5 on the engine, the part that needs no GPU: the float64 references of tests/test_gpu_m5.py (m5_walk, the pool routing rule) against
the oracle and plain autograd, the BatchNorm fold, the structural zeros of the input gradient, the host semantics of the module and the
drivers, and the conditions the GPU tests rely on, checked here with the torch module."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import m5_cases as mc
from dmad_hip import engine as E
from oracle import dmad_oracle as orc

CASES = {'k160': mc.real_sd, 'k80': mc.synth_sd}


@pytest.fixture(scope='module', params=sorted(CASES))
def case(request):
    sd = CASES[request.param]()
    x = mc.clips(2).double()
    logp, rec = mc.m5_walk(mc.sd_t(sd), x)
    return request.param, sd, x, logp, rec


def test_walk_equals_oracle(case):
    _, sd, x, logp, rec = case
    ref = orc.m5_forward(mc.sd_t(sd), x)
    assert (logp - ref).abs().max().item() < 1e-12
    k1 = np.asarray(sd['conv1.weight']).shape[2]
    t1 = ((mc.L - k1) // 16 + 1) // 4
    assert [tuple(p.shape[1:]) for p in rec['pooled']] == [(32, t1), (32, 61), (64, 14), (64, 3)]
    assert [p.shape[-1] % 4 for p in rec['pre']] == {160: [3, 1, 3, 0], 80: [0, 3, 3, 0]}[k1]       # 991, 245, 59, 12 / 996, 247, 59, 12 frames
    for d in rec['dec']:                                                          # both ReLU states occur in every block
        assert 0 < (d >> 2).float().mean().item() < 1


def test_pinned_walk_equals_autograd(case):
    _, sd, x, logp, rec = case
    sd64 = mc.sd_t(sd)
    g = torch.randn(logp.shape, generator=torch.Generator().manual_seed(2)).double()
    xr = x.clone().requires_grad_(True)
    (ref,) = torch.autograd.grad((orc.m5_forward(sd64, xr) * g).sum(), xr)
    got, rec2 = mc.pinned_vjp(sd64, x, g, rec['dec'])
    assert (got - ref[:, 0]).abs().max().item() <= 1e-12 * ref.abs().max().item()
    assert all(torch.equal(a, b) for a, b in zip(rec['dec'], rec2['dec']))


def test_structural_zeros(case):
    """pool4 keeps conv4 frames 0-11, hence conv1 frames <= 935, hence samples <= 16 * 935 + k1 - 1: the gradient beyond is exactly 0"""
    _, sd, x, logp, rec = case
    k1 = np.asarray(sd['conv1.weight']).shape[2]
    first_zero = 16 * 935 + k1
    assert first_zero == {160: 15120, 80: 15040}[k1]
    g = torch.randn(logp.shape, generator=torch.Generator().manual_seed(3)).double()
    gx, _ = mc.pinned_vjp(mc.sd_t(sd), x, g, rec['dec'])
    assert (gx[:, first_zero:] == 0).all() and (gx[:, :first_zero] != 0).any(1).all()


def test_fold_against_unfolded_batchnorm(case):
    _, sd, x, _, rec = case
    f = E.fold_m5_state_dict(sd)
    assert f['m5.stride'].tolist() == [16.0] and all(v.dtype == np.float32 for v in f.values())
    sd64 = mc.sd_t(sd)
    h = x
    for i in (1, 2, 3, 4):
        conv = F.conv1d(h, sd64['conv%d.weight' % i], None, stride=16 if i == 1 else 1)              # no bias: it lives in the shift
        got = conv * torch.from_numpy(f['m5.scale%d' % i]).double()[None, :, None] + torch.from_numpy(f['m5.shift%d' % i]).double()[None, :, None]
        assert np.array_equal(f['m5.conv%d.w' % i], np.asarray(sd['conv%d.weight' % i], np.float32))
        ref = rec['pre'][i - 1]
        assert (got - ref).abs().max().item() <= mc.FP32_TOL * ref.abs().max().item()
        h = rec['pooled'][i - 1]


def test_pool_routing_reference():
    pre, g = mc.pool_case(seed=4)
    n = g.shape[1]
    out = mc.pool_route_ref(pre, g)
    w = pre[:, :4 * n].reshape(-1, n, 4)
    o = out[:, :4 * n].reshape(-1, n, 4)
    assert (out[:, 4 * n:] == 0).all()                                    # remainder frames, though they hold the largest values
    assert ((o != 0).sum(-1) <= 1).all()
    # the special windows of channel 0, in pool_case's order: six pair ties -> the earlier position
    assert [int(o[0, i].nonzero()[0]) for i in range(6)] == [0, 0, 0, 1, 1, 2]
    assert [int(o[0, i].nonzero()[0]) for i in range(6, 10)] == [0, 1, 0, 0]          # ties of three (twice, once split) and four
    assert [int(o[0, i].nonzero()[0]) for i in range(10, 14)] == [0, 1, 2, 3]          # a single maximum at each position
    assert (o[0, 14:17] == 0).all()                                        # all-zero, all-negative, zero above negatives: ReLU'(0) = 0
    # against autograd of relu -> max_pool1d wherever torch's own rule is defined the same way (it is: first maximum, ReLU'(0) = 0)
    p = pre.double().clone().requires_grad_(True)
    (ref,) = torch.autograd.grad((F.max_pool1d(torch.relu(p).unsqueeze(0), 4)[0] * g.double()).sum(), p)
    assert torch.equal(ref, out)
    assert (w.max(-1).values > 0).sum() == (o != 0).any(-1).sum()


def test_walk_routes_like_the_reference():
    """m5_walk's decisions on an integer map are pool_route_ref's"""
    pre, g = mc.pool_case(seed=5, C=32)
    n = g.shape[1]
    r = torch.relu(pre[:, :4 * n].reshape(32, n, 4))
    a, on = mc.first_max(r), r.max(-1).values > 0
    routed = (F.one_hot(a, 4) * (on * 1.0).unsqueeze(-1) * g.unsqueeze(-1)).reshape(32, 4 * n).double()
    assert torch.equal(routed, mc.pool_route_ref(pre, g)[:, :4 * n])


# ---- host semantics ---------------------------------------------------------------------------------------------------------------
def test_grad_backend_validation_and_default_module():
    from audio_models.M5.M5Net import M5
    m = M5(first_kernel_size=160, n_output=10)
    assert m.grad_backend == 'auto' and M5.GRAD_BACKENDS == ('auto', 'torch', 'hip')
    m.grad_backend = 'hip'
    assert m.grad_backend == 'hip'
    with pytest.raises(ValueError):
        m.grad_backend = 'cuda'
    assert not hasattr(m, 'bind_engine')                    # RobustCertificate / build_front bind whatever has it
    assert 'engine' not in m.__dict__ and hasattr(m, 'use_engine')
    x = mc.clips(1)
    sd = mc.real_sd()
    mod = mc.module(sd)
    assert torch.allclose(mod(x), orc.m5_forward(mc.sd_t(sd, torch.float32), x), atol=1e-5)      # a default M5 is the torch module it was
    import copy
    mod.__dict__['engine'] = object()
    assert 'engine' not in copy.deepcopy(mod).__dict__      # a copy is unbound


def test_build_front_and_refusals(monkeypatch):
    import adaptive_attack_eval as drv
    from audio_models.M5.M5Net import M5
    mod = mc.module(mc.real_sd())
    used = []
    monkeypatch.setattr(M5, 'cuda', lambda self, *a: self)
    monkeypatch.setattr(M5, 'use_engine', lambda self, engine=None: used.append(engine) or self)
    args = drv.build_parser().parse_args(['--grad_backend', 'torch'])
    clf, tr = drv.build_front(args, classifier=mod)
    assert clf is mod and tr is None and used == [None] and mod.grad_backend == 'torch'
    args = drv.build_parser().parse_args(['--defense', 'Diffusion-Spec'])
    for fn in (lambda: drv.check_classifier_defense(args, mod), lambda: drv.build_system(args, classifier=mod),
               lambda: drv.build_front(args, classifier=mod)):
        with pytest.raises(NotImplementedError, match='spectrogram'):
            fn()
    drv.check_classifier_defense(drv.build_parser().parse_args(['--defense', 'Diffusion']), mod)
    drv.check_classifier_defense(args, torch.nn.Linear(2, 2))           # any other classifier: not this check's business


def test_abi_names_m5_exports():
    from dmad_hip import _lib
    for n in ('dmad_m5_logits', 'dmad_m5_vjp', 'dmad_m5_tape', 'dmad_m5_query_logits', 'dmad_m5_defense_query_logits'):
        assert n in _lib.EXPORTS


# ---- conditions the GPU tests rely on, checked with the torch module ------------------------------------------------------------------
def test_fp32_and_float64_walks_take_the_same_decisions():
    sd = mc.real_sd()
    x = mc.clips(16)
    _, r64 = mc.m5_walk(mc.sd_t(sd), x.double())
    _, r32 = mc.m5_walk(mc.sd_t(sd, torch.float32), x)
    assert all(torch.equal(a, b) for a, b in zip(r64['dec'], r32['dec']))
    g = torch.randn(16, 10, generator=torch.Generator().manual_seed(6))
    g64, _ = mc.pinned_vjp(mc.sd_t(sd), x, g, r64['dec'])
    xr = x.clone().requires_grad_(True)
    (g32,) = torch.autograd.grad((mc.module(sd)(xr) * g).sum(), xr)
    err = ((g32[:, 0].double() - g64).abs().amax(1) / g64.abs().amax(1)).max().item()
    assert err < mc.VJP_TOL / 10, err                       # measured 4.5e-6


def test_attack_condition_on_the_torch_module():
    """The attack of test_gpu_m5.py (AudioAttack eps 65, lr 13, 10 iterations, untargeted, labels = clean predictions) as plain torch
    sign-gradient steps on the module: it flips all 8 clips and raises the mean loss (0.39 -> 4.6)."""
    mod = mc.module(mc.real_sd())
    x = mc.clips(8)
    with torch.no_grad():
        y = mod(x).argmax(1)
        loss0 = F.cross_entropy(mod(x), y).item()
    eps, lr = 65 / 2 ** 15, 13 / 2 ** 15
    delta = torch.zeros_like(x)
    for _ in range(10):
        d = delta.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(F.cross_entropy(mod(x + d), y), d)
        delta = (delta + lr * g.sign()).clamp(-eps, eps)
    with torch.no_grad():
        out = mod(x + delta)
    assert (out.argmax(1) != y).all()
    assert loss0 < 1.0 and F.cross_entropy(out, y).item() > 2.0, (loss0, F.cross_entropy(out, y).item())
