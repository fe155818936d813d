"""The device-side NES estimate (dmad_nes_probes / dmad_nes_grad), NES(noise_source='device') on a plain callable and on the engine's
own query chain, FAKEBOB on top of it, and the black-box driver.

Keying under test: direction j (0 <= j < H = P/2) of clip b is the row eng.philox_normal(seed, draw0 + b*H + j, NES_STREAM, 1) returns;
the two kernels and that test hook must produce the same bits for the same key.

Error bounds (none of them taken from the code under test):
  * a probe element is fl(x + fl(sigma * u)) with |x| <= 0.8 and |sigma * u| < 0.01: every rounded value is below 1 in magnitude, so each
    of the two roundings is at most 2^-24 and the element is within 2^-23 of x + sigma * u;
  * an estimate element is a sequential fp32 sum over j of rounded products of a rounded difference, times a rounded scale: H + 2
    roundings on every term, so |err| <= 2 * gamma * scale * sum_j |(w_j - w_{H+j}) u_j| with gamma = (H + 2) * 2^-24 (the factor 2
    covers the higher-order terms of (1 + 2^-24)^(H+2) - 1 for every H used here);
  * accumulating onto an earlier estimate adds one rounding of the sum: 2^-24 * |sum|."""
import os
import wave

import numpy as np
import pytest
import torch

from dmad_hip import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SEED = 0xFAB0B
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def clips(ids, gain=1.0):
    return torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in ids])).float().mul(gain).cuda()       # [n, 1, L]


@pytest.fixture(scope='module')
def eng():
    from dmad_hip import engine as E
    e = E.Engine(max_batch=8, precision=E.FP32, with_classifier=False, with_wavenet=False)
    yield e
    e.close()


def directions(eng, draw0, B, H):
    from dmad_hip.engine import NES_STREAM
    return eng.philox_normal(SEED, draw0, NES_STREAM, B * H).view(B, H, eng.L)


def expected_rows(x, u, sigma, with_origin):
    """float64 [B, P + with_origin, L] of the reference's layout (_NES.py:19-25)"""
    x64, su = x.double(), float(np.float32(sigma)) * u.double()
    parts = ([x64] if with_origin else []) + [x64 + su, x64 - su]
    return torch.cat(parts, 1)


@pytest.mark.parametrize('with_origin', [True, False])
def test_probes(eng, with_origin):
    from dmad_hip._lib import DmadError
    B, P, sigma, draw0 = 3, 6, 1e-3, 12345
    H, per_clip = P // 2, P + int(with_origin)
    x = clips(range(B), 0.8)
    assert float(x.abs().max()) <= 0.8
    u = directions(eng, draw0, B, H)
    assert float(u.abs().max()) * sigma < 0.01
    rows = eng.nes_probes(x, P, sigma, with_origin, SEED, draw0)
    assert rows.shape == (B * per_clip, eng.L)
    got = rows.view(B, per_clip, eng.L)
    if with_origin:
        assert torch.equal(got[:, 0], x[:, 0])
    want = expected_rows(x, u, sigma, with_origin)
    assert float((got.double() - want).abs().max()) <= 2 * U
    plus, minus = got[:, per_clip - P:per_clip - H].double(), got[:, per_clip - H:].double()
    assert float((plus + minus - 2 * x.double()).abs().max()) <= 2 * U
    assert float((plus - minus).abs().max()) > 1e-4                     # the probes do move
    for step in (1, 4, 7):                                              # a row depends on its global index alone
        parts = [eng.nes_probes(x, P, sigma, with_origin, SEED, draw0, r0, min(step, B * per_clip - r0)) for r0 in range(0, B * per_clip, step)]
        assert torch.equal(torch.cat(parts), rows), step
    for bad in (dict(P=5), dict(P=0), dict(row0=B * per_clip - 1, rows=2), dict(row0=-1, rows=1)):
        kw = dict(P=P, row0=0, rows=1)
        kw.update(bad)
        with pytest.raises(DmadError):
            eng.nes_probes(x, kw['P'], sigma, with_origin, SEED, draw0, kw['row0'], kw['rows'])


def test_probes_key_arithmetic_at_driver_width(eng):
    B, P, sigma, draw0 = 2, 200, 1e-3, 7
    x = clips([3, 4], 0.8)
    u = directions(eng, draw0, B, P // 2)
    got = eng.nes_probes(x, P, sigma, True, SEED, draw0).view(B, P + 1, eng.L)
    assert float((got.double() - expected_rows(x, u, sigma, True)).abs().max()) <= 2 * U
    assert not torch.equal(got[0, 1], got[1, 1])


def grad_reference(eng, w, P, scale, draw0):
    """(float64 value, a-priori elementwise bound) of scale * sum_j (w_j - w_{H+j}) u_j"""
    B, H = w.shape[0], P // 2
    u = directions(eng, draw0, B, H).double()
    d = (w[:, :H].double() - w[:, H:].double())[:, :, None]
    gamma = (H + 2) * U
    return scale * (d * u).sum(1), 2 * gamma * scale * (d * u).abs().sum(1)


@pytest.mark.parametrize('B,P', [(3, 6), (2, 200)])
def test_grad_against_float64(eng, B, P):
    H = P // 2
    gen = torch.Generator().manual_seed(P)
    w1, w2 = torch.randn(B, P, generator=gen).cuda(), torch.randn(B, P, generator=gen).cuda()
    scale = float(np.float32(1.0 / (P * 1e-3 * 2)))
    d1, d2 = 900, 900 + B * H
    g1 = eng.nes_grad(w1, P, scale, SEED, d1)
    r1, b1 = grad_reference(eng, w1, P, scale, d1)
    assert g1.shape == (B, eng.L) and float(g1.abs().max()) > 0
    assert bool(((g1.double() - r1).abs() <= b1).all()), float(((g1.double() - r1).abs() - b1).max())
    assert torch.equal(eng.nes_grad(w1, P, scale, SEED, d1), g1)                      # bit-reproducible
    for b in range(B):                                                               # a clip's row does not depend on the batch
        assert torch.equal(eng.nes_grad(w1[b:b + 1], P, scale, SEED, d1 + b * H)[0], g1[b]), b
    acc = g1.clone()
    out = eng.nes_grad(w2, P, scale, SEED, d2, grad=acc)                              # a second draw batch, accumulated in place
    assert out.data_ptr() == acc.data_ptr()
    r2, b2 = grad_reference(eng, w2, P, scale, d2)
    bound = (b1 + b2) * (1 + U) + U * (r1 + r2).abs()
    assert bool(((acc.double() - (r1 + r2)).abs() <= bound).all())
    assert not torch.equal(acc, g1)
    from dmad_hip._lib import DmadError
    with pytest.raises(DmadError):
        eng.nes_grad(w1[:, :P - 1], P - 1, scale, SEED, d1)


class RowwiseStridedAverageLinear(torch.nn.Module):
    """The model of tests/golden/fakebob.npz on the GPU, evaluated a row at a time: every row goes through kernels of one fixed shape, so
    its logits cannot depend on how the rows are batched."""

    def __init__(self, weight):
        super().__init__()
        self.weight = torch.nn.Parameter(weight, requires_grad=False)

    def forward(self, x):
        F = self.weight.shape[1]
        return torch.cat([x[i:i + 1, 0].reshape(1, -1, F).mean(1) @ self.weight.t() for i in range(x.shape[0])])


def restated_nes(eng, model, x, y, samples, batch, sigma, draw0):
    """_NES.py:15-55 (EOT 1-1) with the sums in float64.  The queries are formed in fp32 as the reference forms them (`noise * sigma + x`);
    u comes from eng.philox_normal at the documented keys."""
    n, _, L = x.shape
    H, draws = batch // 2, samples // batch
    grad = bound = mean_loss = None
    for i in range(draws):
        u = directions(eng, draw0 + i * n * H, n, H).view(n, H, 1, L)
        noise = torch.cat((u, -u), 1)
        if i == 0:
            noise = torch.cat((torch.zeros_like(x).unsqueeze(1), noise), 1)
        per_clip = noise.shape[1]
        logits = model((noise * sigma + x.unsqueeze(1)).view(-1, 1, L))
        loss = torch.nn.functional.cross_entropy(logits, y.repeat_interleave(per_clip), reduction='none').view(n, per_clip).double()
        if i == 0:
            adver_loss, adver_score, predict = loss[:, 0], logits.view(n, per_clip, -1)[:, 0], logits.view(n, per_clip, -1)[:, 0].argmax(1)
            loss = loss[:, 1:]
        d = (loss[:, :H] - loss[:, H:])[:, :, None]
        u64 = u[:, :, 0].double()
        scale = 1.0 / (batch * sigma * draws)
        g = scale * (d * u64).sum(1)
        # the kernel bound, plus the estimate's sensitivity to the 1e-6 the losses may be off by, plus the rounding of scale to fp32
        b = 2 * (H + 2) * U * scale * (d * u64).abs().sum(1) + scale * 2e-6 * u64.abs().sum(1) + U * g.abs()
        if grad is None:
            grad, bound, mean_loss = g, b, loss.mean(1)
        else:
            grad, bound, mean_loss = grad + g, (bound + b) * (1 + U) + U * (grad + g).abs(), mean_loss + loss.mean(1)
    return mean_loss / draws, grad.view(n, 1, L), bound.view(n, 1, L), adver_loss, adver_score, predict


def test_nes_device_on_a_plain_callable(eng):
    from robustness_eval._EOT import EOT
    from robustness_eval._NES import NES
    from robustness_eval._utils import resolve_loss
    with np.load(os.path.join(GOLDEN, 'fakebob.npz')) as z:
        model = RowwiseStridedAverageLinear(torch.from_numpy(z['weight'])).cuda().eval()
    x = clips(range(3))
    with torch.no_grad():
        y = model(x).argmax(1)
    loss_fn, _ = resolve_loss('Margin', False, 0.5, 'SCR', None, False)
    samples, batch, sigma, draw0 = 16, 8, 1e-3, 1000                                 # two draw batches

    def run(probe_rows):
        nes = NES(samples, batch, sigma, EOT(model, loss_fn, 1, 1, False), noise_source='device', seed=SEED, probe_rows=probe_rows, engine=eng)
        nes._draws = draw0
        out = nes(x, y)
        assert nes._draws == draw0 + 2 * 3 * (batch // 2)
        return out
    mean_loss, grad, adver_loss, adver_score, predict = run(None)
    r_mean, r_grad, r_bound, r_adver, r_score, r_predict = restated_nes(eng, model, x, y, samples, batch, sigma, draw0)
    assert grad.shape == x.shape and mean_loss.shape == adver_loss.shape == (3,) and adver_score.shape == (3, 10)
    assert float((mean_loss.double() - r_mean).abs().max()) <= 1e-6
    assert float((adver_loss.double() - r_adver).abs().max()) <= 1e-6
    assert float((adver_score.double() - r_score.double()).abs().max()) <= 1e-6
    assert predict.tolist() == r_predict.tolist() == y.tolist()
    assert float(r_grad.abs().max()) > 0
    assert bool(((grad.double() - r_grad).abs() <= r_bound).all()), float(((grad.double() - r_grad).abs() - r_bound).max())
    for a, b in zip(run(5), (mean_loss, grad, adver_loss, adver_score)):              # chunks of 5 query rows: the same bits
        assert torch.equal(a, b)
    assert run(5)[4].tolist() == predict.tolist()


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


def test_nes_device_on_the_engine_chain(chain):
    from robustness_eval._EOT import EOT
    from robustness_eval._NES import NES
    from robustness_eval._utils import resolve_loss
    from robustness_eval.black_box_attack import FAKEBOB
    e, _, system = chain
    x = clips([0, 5])
    with torch.no_grad():
        clean = system(x)
    # labels: the runner-up class.  The stand-in is so sure of its own prediction that the fp32 cross-entropy against it is exactly 0 for
    # every probe, which says nothing; against the runner-up the loss is the top-2 margin, which every probe moves
    pred, y = clean.argmax(1), clean.topk(2, 1).indices[:, 1]
    loss_fn, _ = resolve_loss('Margin', False, 0.5, 'SCR', None, False)
    P, sigma, draw0 = 8, 1e-3, 40
    nes = NES(P, P, sigma, EOT(system, loss_fn, 1, 1, False), noise_source='device', seed=SEED, probe_rows=5)
    assert nes.engine is e                                                           # found through EOT_wrapper.model.classifier
    loss, scores, decisions = nes._probe_device(x, y, True, draw0)
    rows = e.nes_probes(x, P, sigma, True, SEED, draw0)
    logits, dec = system.query(rows.view(-1, 1, e.L), 1)
    assert torch.equal(scores, logits[0].view(2, P + 1, -1))                         # dmad_query_logits rows are batch-independent
    assert [int(d[0]) for d in decisions] == dec[0].tolist()
    assert loss.unique().numel() > 1, 'every probe has the same loss: the probes did not reach the classifier'
    nes._draws = draw0
    mean_loss, grad, adver_loss, adver_score, predict = nes(x, y)
    assert torch.equal(adver_score, logits[0].view(2, P + 1, -1)[:, 0]) and torch.equal(adver_loss, loss[:, 0])
    assert grad.shape == x.shape and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    assert predict.tolist() == pred.tolist()

    eps = 0.002
    att = FAKEBOB(system, task='SCR', epsilon=eps, max_iter=4, samples_per_draw=8, samples_per_draw_batch_size=8, max_lr=5e-4, min_lr=1e-4,
                  batch_size=2, verbose=0, noise_source='device', seed=SEED)
    adver_x, success = att.generate(x, y, targeted=False)
    assert adver_x.shape == x.shape and len(success) == 2 and all(isinstance(s, bool) for s in success)
    # within epsilon of x: inside the fp32 bounds the attack clips to, exactly
    assert bool((adver_x <= torch.clamp(x + eps, max=1)).all()) and bool((adver_x >= torch.clamp(x - eps, min=-1)).all())
    assert float(adver_x.abs().max()) <= 1.0
    nes = att.NES_wrapper
    assert nes._draws == 5 * 2 * 4                                                    # max_iter + 1 estimates of n * H draws
    # a second call (the driver makes one per batch of clips) goes on with the counter: other keys, so other directions
    seen = []
    probes = e.nes_probes
    e.nes_probes = lambda *a, **k: (seen.append(a[5]), probes(*a, **k))[1]            # draw0 of every chunk
    try:
        att.generate(x, y, targeted=False)
    finally:
        del e.nes_probes
    assert att.NES_wrapper is nes and nes._draws == 2 * 5 * 2 * 4
    assert sorted(set(seen)) == [40 + 8 * k for k in range(5)]


def test_driver_run(tmp_path, chain, monkeypatch):
    import black_box_attack_eval as drv
    from robustness_eval.black_box_attack import FAKEBOB
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
    args = drv.build_parser().parse_args(['--data_path', str(data), '--classifier_path', str(ck / 'resnext29.pth'), '--attack', 'FAKEBOB',
                                          '--defense', 'None', '--num_per_class', '1', '--batch_size', '4', '--dataload_workers_nums', '0',
                                          '--verbose', '0', '--save_path', str(tmp_path / 'saved')])
    assert args.nes_noise == 'device'
    clf = create_model(args.classifier_path).cuda()
    clf.bind_engine(e)
    lines = []
    made = []
    attacker = FAKEBOB.generate
    monkeypatch.setattr(FAKEBOB, 'generate', lambda self, **k: (made.append((self, self.NES_wrapper and self.NES_wrapper._draws)), attacker(self, **k))[1])
    out = drv.run(args, classifier=clf, log=lambda *a: lines.append(' '.join(str(v) for v in a)), max_iter=2, samples_per_draw=4)
    assert out['total'] == 10
    # three batches (4 + 4 + 2 clips), one attacker, 3 estimates of n * 2 draws each: the counter goes on from batch to batch
    assert len({id(a) for a, _ in made}) == 1 and [d for _, d in made] == [None, 24, 48] and made[0][0].NES_wrapper._draws == 60
    assert len(list((tmp_path / 'saved' / 'adv').glob('*_adv.wav'))) == 10 and len(list((tmp_path / 'saved' / 'clean').glob('*_clean.wav'))) == 10
    for k in ('clean_acc', 'denoised_acc', 'robust_acc'):
        assert np.isfinite(out[k]) and 0.0 <= out[k] <= 100.0, (k, out[k])
    assert [l.split(':')[0] for l in lines[-3:]] == ['original clean test accuracy', 'denoised clean test accuracy', 'CW robust test accuracy']
