"""The device-side particle swarm (dmad_philox_uniform / dmad_pso_init / dmad_pso_step / dmad_pso_update_best), SirenAttack(noise_source=
'device') on a plain callable and on the engine's own query chain, and the SirenAttack driver.

Keying under test: the draws of particle p of clip b in one swarm event are the rows eng.philox_uniform(seed, draw0 + b*P + p,
PSO_STREAM + k, 1) returns, k = 0 position, 1 velocity, 2 r1, 3 r2; the kernels and that test hook must produce the same bits for the
same key, and the hook itself is checked against the raw Philox words.

Error bounds (none of them taken from the code under test), with u = 2^-24 and every operand an fp32 value:
  * a position is clamp(fl(lower + fl(fl(upper - lower) * u_pos))): three roundings on terms no larger than |lower| + |upper - lower|,
    so it is within 4u (|lower| + |upper - lower|) of the float64 value (the fourth u is headroom for the higher-order terms; the clamp
    cannot widen a distance);
  * a velocity is fl(-d + fl(2d * u_vel)) with d = fl|lower - upper|: three roundings on terms no larger than 3d -> 4u * 3d;
  * a moved velocity is a sum of three terms, each the product of at most five rounded values (r, c r, the difference, the product, the
    partial sums): within 8u (|w v| + |c1 r1 (pbest - loc)| + |c2 r2 (gbest - loc)|);
  * the position after a move and the query rows are single fp32 operations on the returned velocity: bit for bit."""
import os
import wave

import numpy as np
import pytest
import torch

from dmad_hip import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SEED = 0x51EE7
EPS = 0.002
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def clips(ids, gain=1.0):
    return torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in ids])).float().mul(gain).cuda()       # [n, 1, L]


def bounds(x, eps=EPS):
    return torch.clamp(-1 - x, min=-eps), torch.clamp(1 - x, max=eps)


@pytest.fixture(scope='module')
def eng():
    from dmad_hip import engine as E
    e = E.Engine(max_batch=8, precision=E.FP32, with_classifier=False, with_wavenet=False)
    yield e
    e.close()


@pytest.fixture(scope='module')
def swarm():
    """B = 3 clips at gain 0.8, the second rescaled to a peak of +0.9995: its upper bound is 0.0005 < epsilon there."""
    x = clips(range(3), 0.8)
    flat = x[1].flatten()
    x[1] = x[1] * (0.9995 / flat[flat.abs().argmax()])
    lower, upper = bounds(x)
    assert float(x.max()) < 1 and bool((upper < EPS).any()) and bool((upper[0] == EPS).all())
    return x, lower, upper


def uniforms(eng, draw0, k, B, P):
    from dmad_hip.engine import PSO_STREAM
    return eng.philox_uniform(SEED, draw0, PSO_STREAM + k, B * P).view(B, P, eng.L)


def test_philox_uniform_against_the_raw_words(eng):
    from dmad_hip.engine import NES_STREAM, PSO_STREAM
    for seed, sample in ((SEED, 0), (2 ** 40 + 7, 2 ** 33 + 5)):
        for stream in (PSO_STREAM + 2, NES_STREAM):
            words = eng.philox_raw(seed, sample, stream, eng.L // 4).cpu().numpy().view(np.uint32)
            want = ((words >> 8).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
            assert want.dtype == np.float32
            got = eng.philox_uniform(seed, sample, stream, 1)
            assert got.shape == (1, eng.L) and np.array_equal(got[0].cpu().numpy().view(np.uint32), want.view(np.uint32)), (seed, stream)
            two = eng.philox_uniform(seed, sample - 1 if sample else 0, stream, 2)
            assert torch.equal(two[1 if sample else 0], got[0])
    assert 0.0 < float(got.min()) and float(got.max()) <= 1.0 and abs(float(got.mean()) - 0.5) < 0.02


def init_reference(eng, x, lower, upper, P, draw0):
    """float64 (positions, their bound, velocities, their bound), each [B, P, L], from philox_uniform's rows"""
    B = x.shape[0]
    lo, up = lower[:, 0].double()[:, None], upper[:, 0].double()[:, None]
    pos = torch.min(torch.max(lo + (up - lo) * uniforms(eng, draw0, 0, B, P).double(), lo), up)
    d = (lo - up).abs()
    vel = -d + 2 * d * uniforms(eng, draw0, 1, B, P).double()
    return pos, 4 * U * (lo.abs() + (up - lo).abs()), vel, 4 * U * 3 * d


@pytest.mark.parametrize('B,P', [(3, 5), (2, 25)])
def test_init(eng, swarm, B, P):
    x, lower, upper = (t[:B] for t in swarm)
    L, draw0 = eng.L, 4321
    pbest_loc, loc, vel, queries = eng.pso_init(x, lower, upper, P, SEED, draw0)
    assert pbest_loc.shape == loc.shape == vel.shape == queries.shape == (B * P, L)
    pb = pbest_loc.view(B, P, L)
    assert bool((pb >= lower).all()) and bool((pb <= upper).all())                 # inside the bounds, exactly
    pos, pos_bound, v, v_bound = init_reference(eng, x, lower, upper, P, draw0)
    assert bool(((pb.double() - pos).abs() <= pos_bound).all()), float(((pb.double() - pos).abs() - pos_bound).max())
    assert bool(((vel.view(B, P, L).double() - v).abs() <= v_bound).all()), float(((vel.view(B, P, L).double() - v).abs() - v_bound).max())
    assert float(v.abs().max()) > 1e-3 and float(pos.std()) > 1e-4                 # the draws do spread
    assert torch.equal(loc, pbest_loc)
    assert torch.equal(queries.view(B, P, L), pb + x)
    assert not torch.equal(pb[0, 0], pb[0, 1]) and not torch.equal(pb[0, 1], pb[1, 1])
    for b in range(B):                                                             # a clip alone, at its own keys
        alone = eng.pso_init(x[b:b + 1], lower[b:b + 1], upper[b:b + 1], P, SEED, draw0 + b * P)
        for a, full in zip(alone, (pbest_loc, loc, vel, queries)):
            assert torch.equal(a, full[b * P:(b + 1) * P]), b


def test_init_keep_and_in_place(eng, swarm):
    from dmad_hip._lib import DmadError
    x, lower, upper = swarm
    B, P, L, draw0 = 3, 5, eng.L, 99
    plain = eng.pso_init(x, lower, upper, P, SEED, draw0)
    keep = (0.25 * lower + 0.5 * upper).contiguous()
    state = [torch.full((B * P, L), 7.0, device='cuda') for _ in range(4)]
    kept = eng.pso_init(x, lower, upper, P, SEED, draw0, keep, *state)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(kept, state))          # written in place
    for name, a, b in zip(('pbest_loc', 'loc', 'vel', 'queries'), kept, plain):
        a, b = a.view(B, P, L), b.view(B, P, L)
        assert torch.equal(a[:, 1:], b[:, 1:]), name
        if name == 'vel':
            assert torch.equal(a[:, 0], b[:, 0])                                   # the velocity key of particle 0 is still used
        elif name == 'queries':
            assert torch.equal(a[:, 0], keep[:, 0] + x[:, 0])
        else:
            assert torch.equal(a[:, 0], keep[:, 0])
    with pytest.raises(DmadError):
        eng.pso_init(x, lower, upper, 0, SEED, draw0)
    with pytest.raises(DmadError):
        eng.pso_init(x.cpu(), lower.cpu(), upper.cpu(), P, SEED, draw0)


def test_step(eng, swarm):
    x, lower, upper = swarm
    B, P, L = 3, 5, eng.L
    w, c1, c2, draw1 = 0.58, 1.4961, 1.4961, 777
    pbest_loc = eng.pso_init(x, lower, upper, P, SEED, 10)[0]                      # personal bests away from the positions
    _, loc0, vel0, _ = eng.pso_init(x, lower, upper, P, SEED, 10 + B * P)
    gbest = pbest_loc.view(B, P, L)[:, 2].clone()                                  # [B, L]
    loc, vel, queries = eng.pso_step(x, lower, upper, pbest_loc, gbest, P, w, c1, c2, SEED, draw1, loc0.clone(), vel0.clone())
    tiny = torch.tensor(1e-5, dtype=torch.float32, device='cuda')
    r1, r2 = uniforms(eng, draw1, 2, B, P) + tiny, uniforms(eng, draw1, 3, B, P) + tiny
    assert r1.dtype == torch.float32
    wf, c1f, c2f = (float(np.float32(v)) for v in (w, c1, c2))
    l0, v0, pb = loc0.view(B, P, L).double(), vel0.view(B, P, L).double(), pbest_loc.view(B, P, L).double()
    t0, t1, t2 = wf * v0, c1f * r1.double() * (pb - l0), c2f * r2.double() * (gbest.double()[:, None] - l0)
    bound = 8 * U * (t0.abs() + t1.abs() + t2.abs())
    err = (vel.view(B, P, L).double() - (t0 + t1 + t2)).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    assert float(t1.abs().max()) > 1e-4 and float(t2.abs().max()) > 1e-4           # both attractions pull
    moved = torch.min(torch.max(loc0.view(B, P, L) + vel.view(B, P, L), lower), upper)
    assert torch.equal(loc.view(B, P, L), moved)
    assert torch.equal(queries.view(B, P, L), loc.view(B, P, L) + x)
    assert bool((loc.view(B, P, L) >= lower).all()) and bool((loc.view(B, P, L) <= upper).all())
    assert bool((loc.view(B, P, L) == upper).any()) or bool((loc.view(B, P, L) == lower).any())      # the clamp does act
    again = eng.pso_step(x, lower, upper, pbest_loc, gbest, P, w, c1, c2, SEED, draw1, loc0.clone(), vel0.clone())
    for a, b in zip(again, (loc, vel, queries)):                                   # bit-reproducible
        assert torch.equal(a, b)
    for b in range(B):                                                             # a clip alone, at its own keys
        rows = slice(b * P, (b + 1) * P)
        alone = eng.pso_step(x[b:b + 1], lower[b:b + 1], upper[b:b + 1], pbest_loc[rows].clone(), gbest[b:b + 1], P, w, c1, c2, SEED,
                             draw1 + b * P, loc0[rows].clone(), vel0[rows].clone())
        for a, full in zip(alone, (loc, vel, queries)):
            assert torch.equal(a, full[rows]), b
    other = eng.pso_step(x, lower, upper, pbest_loc, gbest, P, w, c1, c2, SEED, draw1 + B * P, loc0.clone(), vel0.clone())
    assert not torch.equal(other[1], vel)                                          # other keys, another move


def restated_update_best(loss, predict, loc, pbests, pbest_loc, gbests, gbest_loc, gbest_predict, consider_index):
    """black_box_attack.py:420-437, loop for loop, on copies; loc and pbest_loc [B, P, L]"""
    pbests, pbest_loc, gbests, gbest_loc, gbest_predict = (t.clone() for t in (pbests, pbest_loc, gbests, gbest_loc, gbest_predict))
    update_index = torch.where(loss < pbests)
    for ii, jj in zip(update_index[0].tolist(), update_index[1].tolist()):
        pbests[ii, jj] = loss[ii, jj]
        pbest_loc[ii, jj] = loc[ii, jj]
    gbest_index = torch.argmin(pbests, 1)
    for kk in range(gbest_index.shape[0]):
        index = consider_index[kk]
        if pbests[kk, gbest_index[kk]] < gbests[index]:
            gbests[index] = pbests[kk, gbest_index[kk]]
            gbest_loc[index] = pbest_loc[kk, gbest_index[kk]]
            gbest_predict[index] = predict[kk, gbest_index[kk]]
    return pbests, pbest_loc, gbests, gbest_loc, gbest_predict


CRAFTED = dict(                                 # three working clips of P = 5
    pbests=[[1.0, 0.8, np.inf, 2.0, 0.9], [0.3, 0.4, 0.5, 0.6, 0.7], [np.inf] * 5],
    # clip 0: particles 0 and 1 both fall to 0.5 (a tie: the first wins), particle 2 takes its first value, a NaN changes nothing;
    # clip 1: nothing improves (an equal loss is no improvement);  clip 2: NaN losses beside a tie of particles 3 and 4
    loss=[[0.5, 0.5, 3.0, np.nan, 0.95], [0.3, 0.5, 0.6, 0.7, 0.8], [np.nan, 2.0, np.nan, 1.0, 1.0]],
    predict=[[1, 2, 3, 4, 5], [6, 7, 8, 9, 0], [3, 1, 4, 1, 5]])


@pytest.mark.parametrize('working,consider_index,n_all,gbests0', [
    ((0, 1, 2), None, 3, [0.6, 0.3, np.inf]),                 # clip 1's global best equals its best personal best: untouched
    ((0, 2), [3, 1], 4, [0.11, np.inf, 0.22, 0.6]),           # two working clips out of four, which own rows 3 and 1
    ((2, 1), [0, 2], 3, [0.5, 0.7, 0.1])])                    # a global best that does not improve although the personal ones do
def test_update_best_against_the_restatement(eng, working, consider_index, n_all, gbests0):
    L, P, B = eng.L, 5, len(working)
    gen = torch.Generator().manual_seed(5)
    pick = lambda key, dtype: torch.tensor([CRAFTED[key][c] for c in working], dtype=dtype).cuda()
    loss, pbests, predict = pick('loss', torch.float32), pick('pbests', torch.float32), pick('predict', torch.int64)
    loc, pbest_loc = torch.randn(B * P, L, generator=gen).cuda(), torch.randn(B * P, L, generator=gen).cuda()
    gbests, gbest_loc = torch.tensor(gbests0, dtype=torch.float32).cuda(), torch.randn(n_all, 1, L, generator=gen).cuda()
    gbest_predict = torch.arange(100, 100 + n_all).cuda()
    want = restated_update_best(loss, predict, loc.view(B, P, L), pbests, pbest_loc.view(B, P, L), gbests, gbest_loc[:, 0], gbest_predict,
                                consider_index or list(range(B)))
    before = [t.clone() for t in (pbests, pbest_loc, gbests, gbest_loc, gbest_predict)]
    index = None if consider_index is None else torch.tensor(consider_index).cuda()
    got = eng.pso_update_best(loss, predict, loc, pbests, pbest_loc, gbests, gbest_loc, gbest_predict, index)
    for g, t in zip(got, (pbests, pbest_loc, gbests, gbest_loc, gbest_predict)):
        assert g.data_ptr() == t.data_ptr()                                        # updated in place
    for name, g, w in zip(('pbests', 'pbest_loc', 'gbests', 'gbest_loc', 'gbest_predict'), got, want):
        assert torch.equal(g.reshape(w.shape), w), name
    changed = [not torch.equal(a, b) for a, b in zip(before, got)]
    if consider_index is None:
        assert all(changed)
        rows = slice(P, 2 * P)                                                     # clip 1: nothing improved, nothing touched
        assert torch.equal(pbest_loc[rows], before[1][rows]) and torch.equal(gbest_loc[1], before[3][1]) and int(gbest_predict[1]) == 101
        assert torch.equal(gbests.cpu(), torch.tensor([0.5, 0.3, 1.0])) and gbest_predict.tolist() == [1, 101, 1]
        assert torch.equal(gbest_loc[0, 0], loc[0]) and torch.equal(gbest_loc[2, 0], loc[2 * P + 3])
    elif consider_index == [3, 1]:
        assert torch.equal(gbests.cpu(), torch.tensor([0.11, 1.0, 0.22, 0.5])) and gbest_predict.tolist() == [100, 1, 102, 1]
        assert torch.equal(gbest_loc[0], before[3][0]) and torch.equal(gbest_loc[2], before[3][2])
    else:
        assert changed == [True, True, False, False, False]


class RowwiseStridedAverageLinear(torch.nn.Module):
    """The model of tests/golden/siren.npz on the GPU, evaluated a row at a time: every row goes through kernels of one fixed shape, so
    its logits cannot depend on how the rows are batched."""

    def __init__(self, weight):
        super().__init__()
        self.weight = torch.nn.Parameter(weight, requires_grad=False)

    def forward(self, x):
        F = self.weight.shape[1]
        return torch.cat([x[i:i + 1, 0].reshape(1, -1, F).mean(1) @ self.weight.t() for i in range(x.shape[0])])


def restated_siren(eng, model, x, y, P, max_epoch, max_iter, att, draw0):
    """black_box_attack.py:344-498 in torch fp32 (no clip leaves, no convergence test fires), with the reference's np.random arrays
    replaced by philox_uniform's rows at the documented keys.  -> (gbests per evaluation, gbest_location, the draw counter)"""
    n, _, L = x.shape
    lower, upper = bounds(x, att.epsilon)
    lo, up = lower.unsqueeze(1), upper.unsqueeze(1)                                # [n, 1, 1, L]
    rows = torch.arange(n, device=x.device)
    tiny = torch.tensor(1e-5, dtype=torch.float32, device=x.device)
    draws, trace = draw0, []
    gbests, gbest_loc = torch.full((n,), np.inf, device=x.device), torch.zeros_like(x)
    for epoch in range(max_epoch):
        pos = torch.min(torch.max(lo + (up - lo) * uniforms(eng, draws, 0, n, P).unsqueeze(2), lo), up)
        if epoch == 0:
            pbests = torch.full((n, P), np.inf, device=x.device)
        else:
            best = pbests.argmin(1)
            pos[:, 0] = pbest_loc[rows, best]
            pbests = torch.cat((pbests[rows, best].unsqueeze(1), torch.full((n, P - 1), np.inf, device=x.device)), 1)
        pbest_loc, loc = pos.clone(), pos.clone()
        d = (lo - up).abs()
        vel = -d + (2 * d) * uniforms(eng, draws, 1, n, P).unsqueeze(2)
        draws += n * P
        for it in range(max_iter + 1):
            logits = model((loc + x.unsqueeze(1)).view(-1, 1, L))
            loss = torch.nn.functional.cross_entropy(logits, y.repeat_interleave(P), reduction='none').view(n, P)
            better = loss < pbests
            pbests = torch.where(better, loss, pbests)
            pbest_loc[better] = loc[better]
            best = pbests.argmin(1)
            gain = pbests[rows, best] < gbests
            gbests = torch.where(gain, pbests[rows, best], gbests)
            gbest_loc[gain] = pbest_loc[rows, best][gain]
            trace.append(gbests.clone())
            if it < max_iter:
                w = att._inertia(it)
                r1, r2 = uniforms(eng, draws, 2, n, P).unsqueeze(2) + tiny, uniforms(eng, draws, 3, n, P).unsqueeze(2) + tiny
                vel = w * vel + att.c1 * r1 * (pbest_loc - loc) + att.c2 * r2 * (gbest_loc.unsqueeze(1) - loc)
                loc = torch.min(torch.max(loc + vel, lo), up)
                draws += n * P
    return trace, gbest_loc, draws


def test_siren_device_on_a_plain_callable(eng):
    from robustness_eval.black_box_attack import SirenAttack
    with np.load(os.path.join(GOLDEN, 'siren.npz')) as z:
        model = RowwiseStridedAverageLinear(torch.from_numpy(z['weight'])).cuda().eval()
        x, y = clips([int(i) for i in z['clip_ids']]), torch.from_numpy(z['y']).cuda()
    n, P, max_epoch, max_iter = 3, 4, 2, 3
    att = SirenAttack(model, task='SCR', epsilon=EPS, max_epoch=max_epoch, max_iter=max_iter, n_particles=P, batch_size=n, verbose=0,
                      noise_source='device', seed=SEED, engine=eng)
    assert att.engine is eng and att._draws == 0
    seen, inits = [], []
    update, init = eng.pso_update_best, eng.pso_init
    eng.pso_update_best = lambda *a, **k: (update(*a, **k), seen.append((a[5].clone(), a[6].clone())))[0]
    eng.pso_init = lambda *a, **k: (inits.append(a[5]), init(*a, **k))[1]           # draw0 of every epoch
    try:
        adver_x, success = att.generate(x, y, targeted=False)
        per_epoch = n * P * (1 + max_iter)                                         # one initialisation and max_iter moves
        assert att._draws == max_epoch * per_epoch and inits == [0, per_epoch]
        trace, gbest_loc, draws = restated_siren(eng, model, x, y, P, max_epoch, max_iter, att, 0)
        assert draws == att._draws and len(seen) == len(trace) == max_epoch * (max_iter + 1)
        for t, ((gb, _), want) in enumerate(zip(seen, trace)):
            assert float((gb.double() - want.double()).abs().max()) <= 1e-6, t
        assert float(trace[-1].min()) > 0 and bool((trace[-1] < trace[0]).any())   # positive losses, and the swarm lowers one
        lower, upper = bounds(x)
        final = seen[-1][1]
        assert bool((final >= lower).all()) and bool((final <= upper).all())
        assert torch.equal(adver_x, final + x) and success == [False] * n
        att.generate(x, y, targeted=False)                                         # a second call goes on with other keys
        assert att._draws == 2 * max_epoch * per_epoch and inits == [0, per_epoch, 2 * per_epoch, 3 * per_epoch]
        assert not torch.equal(seen[len(trace)][0], seen[0][0])
    finally:
        del eng.pso_update_best, eng.pso_init


@pytest.fixture(scope='module')
def chain():
    """A classifier engine with the calibrated synthetic ResNeXt29, and AcousticSystem(no defender) on it."""
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.resnext import CifarResNeXt
    from dmad_hip import engine as E
    from dmad_hip.transforms import MelSpectrogramDB
    sd = synth.resnext29_state_dict(2929)
    e = E.Engine(max_batch=8, precision=E.FP32, with_wavenet=False)
    e.load_resnext29(sd)
    rx = CifarResNeXt(nlabels=10, in_channels=1)
    rx.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    rx = rx.cuda().eval().bind_engine(e)
    system = AcousticSystem(classifier=rx, transform=MelSpectrogramDB(e), defender=None).eval()
    assert system._engine_chain(True) == (e, 0)
    yield e, sd, system
    e.close()


def test_siren_device_on_the_engine_chain(chain):
    from robustness_eval.black_box_attack import SirenAttack
    e, _, system = chain
    x = clips([0, 5])
    with torch.no_grad():
        clean = system(x)
    # labels: the runner-up class.  The stand-in is so sure of its own prediction that the fp32 cross-entropy against it is exactly 0 for
    # every particle, which says nothing; against the runner-up the loss is the top-2 margin, which every particle moves
    y = clean.topk(2, 1).indices[:, 1]
    P = 5
    att = SirenAttack(system, task='SCR', epsilon=EPS, max_epoch=2, max_iter=2, n_particles=P, batch_size=2, verbose=0, noise_source='device',
                      seed=SEED)
    assert att.engine is e                                                         # found through model.classifier
    seen = []
    update = e.pso_update_best
    e.pso_update_best = lambda *a, **k: (update(*a, **k), seen.append((a[0].clone(), a[5].clone())))[0]
    try:
        adver_x, success = att.generate(x, y, targeted=False)
    finally:
        del e.pso_update_best
    assert len(seen) == 2 * 3 and att._draws == 2 * 2 * P * 3
    for loss, _ in seen:
        assert loss.shape == (2, P) and all(row.unique().numel() > 1 for row in loss), 'the particles of a clip have one loss'
    for (_, a), (_, b) in zip(seen, seen[1:]):
        assert bool((b <= a).all())                                                # a global best never rises
    gbests = seen[-1][1]
    assert bool((gbests > 0).all()) and success == [False, False]
    lower, upper = bounds(x)
    assert bool((adver_x - x >= lower - 2 * U).all()) and bool((adver_x - x <= upper + 2 * U).all()) and float(adver_x.abs().max()) <= 1.0
    # the reported best IS the loss of the returned clip: its query row was fl(location + x), and a row's logits do not depend on the batch
    logits, _ = system.query(adver_x, 1)
    assert torch.equal(torch.nn.functional.cross_entropy(logits[0], y, reduction='none'), gbests)


def test_margin_loss_removes_a_found_clip(chain):
    from robustness_eval.black_box_attack import SirenAttack
    e, _, system = chain
    x = clips([0, 5, 7])
    with torch.no_grad():
        top2 = system(x).topk(2, 1).indices
    y = top2[:, 0].clone()
    y[1] = top2[1, 1]                                                              # clip 1 is mislabelled: its margin is negative at once
    P = 3
    att = SirenAttack(system, task='SCR', epsilon=EPS, max_epoch=1, max_iter=2, n_particles=P, batch_size=3, verbose=0, noise_source='device',
                      seed=SEED, loss='margin')
    steps, updates = [], []
    step, update = e.pso_step, e.pso_update_best
    e.pso_step = lambda *a, **k: (steps.append((a[0].shape[0], a[3].shape[0], a[4].shape[0], a[11].shape[0], a[12].shape[0])), step(*a, **k))[1]
    e.pso_update_best = lambda *a, **k: (updates.append((tuple(a[0].shape), a[2].shape[0], None if a[8] is None else a[8].tolist())),
                                         update(*a, **k))[1]
    try:
        adver_x, success = att.generate(x, y, targeted=False)
    finally:
        del e.pso_step, e.pso_update_best
    assert success[1] is True and success[0] is False and success[2] is False
    assert updates == [((3, P), 3 * P, None), ((2, P), 2 * P, [0, 2]), ((2, P), 2 * P, [0, 2])]
    assert steps == [(2, 2 * P, 2, 2 * P, 2 * P)] * 2                              # x, pbest_loc, gbest_loc, loc, vel of the two clips left
    assert att._draws == 3 * P + 2 * 2 * P
    assert adver_x.shape == x.shape
    with torch.no_grad():
        assert int(system(adver_x[1:2]).argmax(1)) != int(y[1])                     # "success": the returned clip is not classified as y


def test_driver_run(tmp_path, chain, monkeypatch):
    import siren_attack_eval as drv
    from robustness_eval.black_box_attack import SirenAttack
    from audio_models.ConvNets_SpeechCommands.create_model import create_model
    from models.resnext import CifarResNeXt                  # the module path of the reference's pickled checkpoints
    from datasets.sc_dataset import SC09_CLASSES
    e, sd, _ = chain
    data = tmp_path / 'test'
    for i, c in enumerate(SC09_CLASSES[:10]):
        (data / c).mkdir(parents=True)
        pcm = (synth.synthetic_clip(i).reshape(-1) * 32767).astype('<i2')
        with wave.open(str(data / c / 'a.wav'), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(pcm.tobytes())
    ck = tmp_path / 'ConvNets_SpeechCommands'
    ck.mkdir()
    rx = CifarResNeXt(nlabels=10, in_channels=1)
    rx.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    torch.save(torch.nn.DataParallel(rx), str(ck / 'resnext29.pth'))
    args = drv.build_parser().parse_args(['--data_path', str(data), '--classifier_path', str(ck / 'resnext29.pth'), '--attack', 'SirenAttack',
                                          '--defense', 'None', '--num_per_class', '1', '--batch_size', '4', '--dataload_workers_nums', '0',
                                          '--verbose', '0'])
    assert args.swarm_noise == 'device' and args.siren_loss == 'reference'
    clf = create_model(args.classifier_path).cuda()
    clf.bind_engine(e)
    lines, made = [], []
    attacker = SirenAttack.generate
    monkeypatch.setattr(SirenAttack, 'generate', lambda self, **k: (made.append((self, self._draws)), attacker(self, **k))[1])
    out = drv.run(args, classifier=clf, log=lambda *a: lines.append(' '.join(str(v) for v in a)), max_epoch=1, max_iter=2, n_particles=3)
    assert out['total'] == 10
    # three batches (4 + 4 + 2 clips), one attacker, one initialisation and two moves of n * 3 keys each: the counter goes on
    assert len({id(a) for a, _ in made}) == 1 and [d for _, d in made] == [0, 36, 72] and made[0][0]._draws == 90
    for k in ('clean_acc', 'denoised_acc', 'robust_acc'):
        assert np.isfinite(out[k]) and 0.0 <= out[k] <= 100.0, (k, out[k])
    assert out['robust_acc'] == 100.0                                              # the reference's loss never reports a success
    assert [l.split(':')[0] for l in lines[-3:]] == ['original clean test accuracy', 'denoised clean test accuracy', 'CW robust test accuracy']
