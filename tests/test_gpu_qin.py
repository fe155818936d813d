"""The masking loss of the imperceptible attack on the engine (dmad_masking_loss_vjp, dmad_masking_step) against the float64
walk of tests/qin_ref.py, its edges, its determinism, and stage 2 of AudioAttack on both masking backends with the driver on top.

Inputs: delta = (65 / 32768) * random signs (seed b for row b) on synthetic_clip(0..3), theta and psd_scale from the host masker and
rounded to float32 (the float64 walk reads the same float32 values).  In float64 alone these give 22 - 34 % of the 28 700 bins per clip
above their threshold, 0 - 3 of them within 1e-4 of it and none within 1e-5.

Bounds.  TOL = 1e-4 is MEL_TOL of test_gpu_classifier_vjp.py: the same two fp32 GEMMs behind a milder nonlinearity (a square in place
of 1 / M); psd relative to its per-clip maximum, g_delta relative to max |g| per clip with the hinge mask PINNED to the engine's own
psd > theta (a bin within rounding of its threshold may fall on either side; the engine's mask may differ from the float64 one only at
bins whose float64 margin |psd / theta - 1| is below 1e-4, at most 0.1 % of a clip's bins), the loss relative to its value.
masking_step against masking_loss_vjp followed by the update in float64 on the engine's own g_theta: STEP_TOL = 1e-6 absolute (values
bounded by 2, four fp32 roundings of 2^-24 relative each).  Stage 2 on the engine against the torch branch on the same GPU: decisions
and alpha equal, the clips within ATTACK_TOL = 4 * STEP_TOL * 12 iterations = 4.8e-5 (iterating amplifies fp32 differences; measured on
the MI355X: 9.9e-6, with all three clips successes of both stages and loss_theta falling from 28 - 56 to 0.4 - 1.0)."""
import json
import wave

import numpy as np
import pytest
import torch

import qin_ref
from dmad_hip import synth

pytestmark = pytest.mark.gpu

TOL = 1e-4
STEP_TOL = 1e-6
ITERS_2 = 12
ATTACK_TOL = 4 * STEP_TOL * ITERS_2
L, F, K = 16000, 28, 1025
FIRST_UNREAD = 512 * (F - 1) + 2048          # 15 872
RX_SEED = 2929


def clips(ids):
    return torch.from_numpy(np.stack([synth.synthetic_clip(i).reshape(-1) for i in ids])).float()


@pytest.fixture(scope='module')
def eng():
    from dmad_hip import engine as E
    e = E.Engine(max_batch=65, precision=E.FP32, with_wavenet=False)
    e.load_resnext29(synth.resnext29_state_dict(RX_SEED))
    yield e
    e.close()


@pytest.fixture(scope='module')
def host():
    """clips 0..3, their float32 theta / psd_scale from the host masker, the sign perturbations and the float64 walk; computed once"""
    from robustness_eval.white_box_attack import PsychoacousticMasker
    m = PsychoacousticMasker()
    x = clips(range(4))
    pairs = [m.calculate_threshold_and_psd_maximum(c.numpy()) for c in x]
    theta = (10 ** (np.array([t for t, _ in pairs]) * 0.1)).astype(np.float32)
    scale = (10 ** 9.6 / 10 ** (np.array([p for _, p in pairs]) * 0.1)).astype(np.float32)
    delta = qin_ref.sign_delta(4)
    walk = qin_ref.masking_walk(delta, theta, scale)
    for k in ('psd', 'mask', 'loss', 'g'):
        walk[k].setflags(write=False)
    return dict(x=x, theta=theta, scale=scale, delta=delta, walk=walk, masker=m)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('rows', [[0], [1, 2, 3]], ids=['B1', 'B3'])
def test_against_float64(eng, host, rows):
    w = host['walk']
    g, loss, psd = eng.masking_loss_vjp(dev(host['delta'][rows]), dev(host['theta'][rows]), dev(host['scale'][rows]), want_psd=True)
    g, loss, psd = g.cpu().numpy().astype(np.float64), loss.cpu().numpy().astype(np.float64), psd.cpu().numpy().astype(np.float64)
    assert g.shape == (len(rows), L) and psd.shape == (len(rows), K, F)
    mask = psd > host['theta'][rows].astype(np.float64)
    pinned = qin_ref.masking_walk(host['delta'][rows], host['theta'][rows], host['scale'][rows], mask=mask)
    for j, r in enumerate(rows):
        e_psd = np.abs(psd[j] - w['psd'][r]).max() / w['psd'][r].max()
        e_g = np.abs(g[j] - pinned['g'][j]).max() / np.abs(pinned['g'][j]).max()
        e_loss = abs(loss[j] - w['loss'][r]) / w['loss'][r]
        flips = mask[j] != w['mask'][r]
        margin = np.abs(w['psd'][r] / host['theta'][r].astype(np.float64) - 1.0)
        print('clip %d: psd %.3g  g_delta %.3g  loss %.3g (rel.); active %.1f %%, mask flips %d, bins within 1e-4 of theta %d'
              % (r, e_psd, e_g, e_loss, 100 * mask[j].mean(), flips.sum(), (margin < TOL).sum()))
        assert e_psd <= TOL and e_g <= TOL and e_loss <= TOL
        assert 0.05 < mask[j].mean() < 0.95
        assert (margin[flips] < TOL).all() and flips.mean() <= 1e-3
    assert (g[:, FIRST_UNREAD:] == 0).all() and (g[:, :FIRST_UNREAD] != 0).any(1).all()


def test_pass_boundary(eng, host):
    """65 clips: one pass of 64 and one of 1; row b is clip b % 4, and every row's loss is its clip's"""
    rows = [b % 4 for b in range(65)]
    g, loss = eng.masking_loss_vjp(dev(host['delta'][rows]), dev(host['theta'][rows]), dev(host['scale'][rows]))
    one = [eng.masking_loss_vjp(dev(host['delta'][[r]]), dev(host['theta'][[r]]), dev(host['scale'][[r]])) for r in range(4)]
    ref = host['walk']['loss']
    lo = loss.cpu().numpy().astype(np.float64)
    assert (np.abs(lo - ref[rows]) / ref[rows]).max() <= TOL
    for b in (0, 3, 63, 64):
        assert torch.equal(loss[b], one[rows[b]][1][0]) and torch.equal(g[b], one[rows[b]][0][0])


def test_edges(eng, host):
    delta = host['delta'][:3].copy()
    delta[1] = 0.0                                                     # a row of zeros: loss 0 and a gradient of exactly 0
    g, loss = eng.masking_loss_vjp(dev(delta), dev(host['theta'][:3]), dev(host['scale'][:3]))
    assert float(loss[1]) == 0.0 and (g[1] == 0).all()
    assert (g[:, FIRST_UNREAD:] == 0).all() and float(loss[0]) > 0 and float(loss[2]) > 0
    # an all-zero clip: psd_max = -200 dB, so psd_scale = 10^29.6; no maskers, so theta is the ATH (0 in bins 0 - 2)
    t, p = host['masker'].calculate_threshold_and_psd_maximum(np.zeros(L, np.float32))
    theta = (10 ** (t * 0.1)).astype(np.float32)[None]
    scale = np.array([10 ** 9.6 / 10 ** (p * 0.1)], np.float32)
    assert np.isfinite(theta).all() and np.isfinite(scale).all() and (theta[0, :3] == 0).all()
    g, loss = eng.masking_loss_vjp(dev(host['delta'][:1]), dev(theta), dev(scale))
    assert torch.isfinite(loss).all() and torch.isfinite(g).all() and float(loss) > 0 and float(g.abs().max()) > 0


def test_determinism_and_batch_independence(eng, host):
    rows = [0, 1, 2, 3, 2, 0, 1]
    d, t, s = dev(host['delta'][rows]), dev(host['theta'][rows]), dev(host['scale'][rows])
    a, b = eng.masking_loss_vjp(d, t, s, want_psd=True), eng.masking_loss_vjp(d, t, s, want_psd=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert torch.equal(a[0][2], a[0][4]) and torch.equal(a[1][0], a[1][5])              # the same clip in another row
    for j in (0, 3, 6):
        one = eng.masking_loss_vjp(d[j:j + 1], t[j:j + 1], s[j:j + 1], want_psd=True)
        assert all(torch.equal(u[0], v[j]) for u, v in zip(one, a))


@pytest.mark.parametrize('signed_lr', [-2.0 ** -15, 2.0 ** -15], ids=['targeted', 'untargeted'])
def test_masking_step(eng, host, signed_lr):
    B = 3
    x = host['x'][:B].clone()
    x[0, :8] = 0.99999                                                 # the box binds: delta + step pushes these samples past 1
    x[2, 100:104] = -0.99999
    delta = host['delta'][:B].copy()
    delta[0, :8], delta[2, 100:104] = 2e-3, -2e-3
    g_net = np.random.RandomState(7).randn(B, L).astype(np.float32) * 0.5
    g_net[0, :8] = 40.0 * np.sign(signed_lr)                           # towards +1 whatever the sign of the step
    g_net[2, 100:104] = -40.0 * np.sign(signed_lr)
    alpha = np.array([0.05, 0.5, 3.0], np.float32)                     # per clip
    th, sc = dev(host['theta'][:B]), dev(host['scale'][:B])
    g_theta, loss_ref = eng.masking_loss_vjp(dev(delta), th, sc)
    d = dev(delta).unsqueeze(1)                                        # [B, 1, L], updated in place
    ptr = d.data_ptr()
    loss = eng.masking_step(dev(x.numpy()).unsqueeze(1), d, dev(g_net), dev(alpha), signed_lr, th, sc)
    assert d.data_ptr() == ptr and torch.equal(loss, loss_ref)
    want = qin_ref.step_ref(x.numpy(), delta, g_net, alpha, signed_lr, g_theta.cpu().numpy())
    got = d[:, 0].cpu().numpy().astype(np.float64)
    err = np.abs(got - want).max()
    hit = np.abs(np.abs(x.numpy().astype(np.float64) + got) - 1.0) < 1e-7
    print('masking_step: max |diff| %.3g, %d samples on the box' % (err, hit.sum()))
    assert err <= STEP_TOL
    assert hit[0, :8].all() and hit[2, 100:104].all()
    assert np.abs(got - delta).max() > 1e-4                            # it moved


def test_refusals(eng, host):
    from dmad_hip import engine as E
    from dmad_hip._lib import DmadError
    d, t, s = dev(host['delta'][:1]), dev(host['theta'][:1]), dev(host['scale'][:1])
    with pytest.raises(DmadError):
        eng.masking_loss_vjp(d, t[:, :, :27].contiguous(), s)
    with pytest.raises(DmadError, match='no CPU path'):
        eng.masking_loss_vjp(d.cpu(), t, s)
    with pytest.raises(DmadError):
        eng.masking_step(d, d.double(), d, s, 1.0, t, s)              # delta is updated in place: float32 only
    import ctypes
    null = ctypes.c_void_p(None)
    assert eng.lib.dmad_masking_loss_vjp(eng._h, null, 1, null, null, null, null, null, null) != 0
    assert eng.lib.dmad_masking_loss_vjp(eng._h, ctypes.c_void_p(d.data_ptr()), 66, ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(s.data_ptr()),
                                         ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(s.data_ptr()), null, null) != 0     # B > max_batch
    bare = E.Engine(max_batch=2, precision=E.FP32, with_classifier=False, with_wavenet=False)     # no mel constants
    with pytest.raises(DmadError, match='with_classifier'):
        bare.masking_loss_vjp(d, t, s)
    bare.close()
    # clip_len < 2048 cannot be reached through an engine with mel constants: dmad_create gives those to clip_len = 16000 only


@pytest.fixture(scope='module')
def system():
    """AcousticSystem(ResNeXt29, mel dB, None) on an engine of its own.  The classifier is the stand-in of test_gpu_classifier_vjp.py
    (kink_free): every ReLU kept away from its kink on the three clips and the head scaled to logits of a few units.  The calibrated
    synthetic net as it is gives all three clips one class with logit gaps of several hundred, which ten steps at eps 65 do not close,
    and a saturated softmax; and a net whose ReLUs sit within rounding of zero turns the 1e-7 differences between the two masking
    backends into jumps of its own gradient, which is no property of the masking code."""
    import test_gpu_classifier_vjp as cv
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.resnext import CifarResNeXt
    from dmad_hip import engine as E
    from dmad_hip.transforms import MelSpectrogramDB
    from oracle import dmad_oracle as orc
    sd = cv.kink_free(synth.resnext29_state_dict(RX_SEED), orc.mel_db(clips(range(3)).unsqueeze(1)).double())
    e = E.Engine(max_batch=4, precision=E.FP32, with_wavenet=False)
    e.load_resnext29(sd)
    rx = CifarResNeXt(nlabels=10, in_channels=1)
    rx.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    rx = rx.cuda().eval()
    rx.bind_engine(e)
    rx.grad_backend = 'hip'
    e.reserve_classifier_vjp(3)
    yield AcousticSystem(classifier=rx, transform=MelSpectrogramDB(e, grad_backend='hip'), defender=None).eval()
    e.close()


def _attack(system, masker, backend):
    from robustness_eval.white_box_attack import AudioAttack
    att = AudioAttack(system, masker=masker, eps=65, norm='linf', learning_rate_1=13, max_iter_1=10, max_iter_2=ITERS_2, num_iter_increase_alpha=2,
                      num_iter_decrease_alpha=3, eot_attack_size=1, eot_defense_size=1, verbose=0, masking_backend=backend)
    att.trace = []
    return att


def test_attack_hip_against_torch(eng, host, system):
    """--defense None, 3 clips, 10 + 12 iterations, the driver's eps 65 and step eps / 5, targeted.  The targets are the classes an UNTARGETED stage 1 of the same settings
    drives the clips into (the runner-up of the clean logits where it moves none): classes ten sign steps can reach, so that stage 2
    starts from hits with a perturbation that is not zero (on delta = 0 every STFT bin is exactly 0, where the torch branch's sqrt
    gives a NaN gradient and the engine 0: module docstring of white_box_attack.py).  Targeted is the sign with which alpha * g_theta
    lowers the masking loss.  Measured on the MI355X: clips max |diff| 9.9e-6 (per clip 1.3e-6, 5.3e-6, 9.9e-6) against
    ATTACK_TOL = 4.8e-5; loss_theta of the two traces within 5.1e-4 relative."""
    x = host['x'][:3].unsqueeze(1).cuda()
    with torch.no_grad():
        top = system(x).topk(2, dim=1).indices
    probe = _attack(system, host['masker'], 'hip')
    probe._targeted = False
    x_u = probe.stage_1(x, top[:, 0])[0]
    with torch.no_grad():
        reached = system(x_u).argmax(1)
    y = torch.where(reached != top[:, 0], reached, top[:, 1])
    hip = _attack(system, host['masker'], 'hip')
    x_hip, (s1, s2) = hip.generate(x, y, targeted=True)
    assert x_hip.shape == x.shape and len(s1) == len(s2) == 3 and len(hip.trace) == ITERS_2 and float(x_hip.abs().max()) <= 1.0
    first = _attack(system, host['masker'], 'hip')
    first._targeted = True
    x_1, _ = first.stage_1(x, y)                                                  # stage 1 alone: the clips stage 2 started from
    th, sc = dev(host['theta'][:3]), dev(host['scale'][:3])
    before = eng.masking_loss_vjp(x_1 - x, th, sc)[1].tolist()
    after = eng.masking_loss_vjp(x_hip - x, th, sc)[1].tolist()
    print('targets', y.tolist(), 'clean', top[:, 0].tolist(), 'alpha', hip.trace[-1]['alpha'], 'predictions', [t['prediction'] for t in hip.trace])
    print('stage 2 on the engine: success', s1, s2, 'loss_theta of the stage-1 clips', before, 'of the returned clips', after)
    assert any(s2) and all(a <= b for a, b, ok in zip(after, before, s2) if ok)
    with torch.no_grad():
        pred = system(x_hip).argmax(1)
    assert all(int(p) == int(t) for p, t, ok in zip(pred, y, s2) if ok)
    tor = _attack(system, host['masker'], 'torch')
    x_tor, (t1, t2) = tor.generate(x, y, targeted=True)
    assert (s1, s2) == (t1, t2)
    assert [t['prediction'] for t in hip.trace] == [t['prediction'] for t in tor.trace]
    assert [t['alpha'] for t in hip.trace] == [t['alpha'] for t in tor.trace]
    dev_x = float((x_hip - x_tor).abs().max())
    print('per clip max |diff|', (x_hip - x_tor).abs().amax(dim=(1, 2)).tolist())
    lh, lt = np.array([t['loss_theta'] for t in hip.trace]), np.array([t['loss_theta'] for t in tor.trace])
    print('engine against torch branch after %d iterations: clips max |diff| %.3g, loss_theta max relative deviation %.3g'
          % (ITERS_2, dev_x, float((np.abs(lh - lt) / lt).max())))
    assert dev_x <= ATTACK_TOL


def test_driver_main(tmp_path, eng):
    import imperceptible_attack_eval as drv
    from audio_models.ConvNets_SpeechCommands.create_model import create_model
    from models.resnext import CifarResNeXt                  # the module path of the reference's pickled checkpoints
    from datasets.sc_dataset import SC09_CLASSES
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
    rx.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.resnext29_state_dict(RX_SEED).items()})
    torch.save(torch.nn.DataParallel(rx), str(ck / 'resnext29.pth'))
    clf = create_model(str(ck / 'resnext29.pth')).cuda()
    clf.bind_engine(eng)
    lines = []
    out = drv.main(['--data_path', str(data), '--classifier_path', str(ck / 'resnext29.pth'), '--max_iter_1', '2', '--max_iter_2', '3',
                    '--num_per_class', '1', '--batch_size', '4', '--dataload_workers_nums', '0', '--verbose', '0'],
                   classifier=clf, log=lambda *a: lines.append(' '.join(str(v) for v in a)))
    assert out['total'] == 10 and 0 <= out['imperceptible_success'] <= 10
    assert any(l.startswith('attack: Qin-I with linf_eps=65 & iter=2+3') and 'masking=hip' in l for l in lines)
    assert lines[-1] == 'Imperceptible attack success rate: {:.4f}%'.format(out['imperceptible_rate'])
    for k in ('clean_acc', 'denoised_acc', 'robust_acc', 'imperceptible_rate'):
        assert np.isfinite(out[k]) and 0.0 <= out[k] <= 100.0, (k, out[k])
    assert json.dumps(out)
