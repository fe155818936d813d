"""Kenansville(fft_backend='device') on the engine against fft_backend='torch' (the reference's operators, pinned bit for bit by
tests/golden/kenansville.npz in test_kenansville_cpu.py) on the fixture's clips, model and max_iter; one engine system (the synthetic
VGG19_bn behind the mel front-end) on the one-call query path; and the driver's run().

Tolerance, as in test_gpu_wave_fft.py: 4 x the measured fp32 error of CPU torch.fft against float64 on the same clips, relative to the
clip's largest |X| (factors) or |x| (clips).  The bisection is far from any bin at its eighth halving: the first test asserts, in float64
on the CPU, that no bin of the fixture's clips lies within that tolerance of any factor the fixture visits, so both backends must take
the same decisions."""
import json
import os
import wave

import numpy as np
import pytest
import torch

from dmad_hip import synth
from kenansville_cases import StridedAverageLinear, fixture_weight, stop_after_a_gpu_fault  # noqa: F401  (an autouse fixture)

pytestmark = pytest.mark.gpu
MARGIN = 4.0


@pytest.fixture(scope='module')
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, 'kenansville.npz')) as z:
        return {k: z[k] for k in z.files}


def test_device_backend_against_the_torch_backend(golden):
    from dmad_hip import engine as E
    from robustness_eval.black_box_attack import Kenansville
    g = golden
    settings = json.loads(str(g['settings']))
    T = settings['max_iter']
    x = torch.from_numpy(np.stack([synth.synthetic_clip(int(i)) for i in g['clip_ids']])).float()
    y = torch.from_numpy(g['y'])
    L = x.shape[-1]
    # float64 on the CPU: the tolerance, and that no bin is within it of a visited factor
    x64 = x[:, 0].double().numpy()
    X = np.fft.rfft(x64, axis=1)
    mag, peak, xpeak = np.abs(X), np.abs(X).max(1), np.abs(x64).max(1)
    X32 = torch.fft.rfft(x[:, 0], dim=1)
    fwd = float((np.abs(X32.numpy().astype(np.complex128) - X).max(1) / peak).max())
    inv = 0.0
    for t in range(T):
        f = g['factors'][t].astype(np.float64)[:, None]
        gap = np.abs(mag - f).min(1) / peak
        assert (gap > 2 * MARGIN * fwd).all(), (t, gap, fwd)                   # twice: the device's factor may itself be off by the tolerance
        keep = mag >= f
        want = np.fft.irfft(np.where(keep, X, 0), n=L, axis=1)
        y32 = torch.fft.irfft(torch.where(torch.from_numpy(keep), X32, torch.zeros_like(X32)), n=L, dim=1).numpy().astype(np.float64)
        inv = max(inv, float((np.abs(y32 - want).max(1) / xpeak).max()))
    print('torch fp32 against float64 on the fixture clips: forward %.3e of max|X|, thresholded inverse %.3e of max|x|' % (fwd, inv))

    model = StridedAverageLinear(fixture_weight(g)).eval()
    ref = Kenansville(model, fft_backend='torch', **settings)
    ref.trace = []
    want_x, want_succ = ref.generate(x, y, targeted=False)
    assert want_succ == g['succ'].tolist()

    e = E.Engine(clip_len=L, max_batch=1, precision=E.FP32, with_classifier=False, with_wavenet=False)
    try:
        calls = {'rfft': 0, 'irfft': 0, 'update': 0}
        for name, key in (('wave_rfft', 'rfft'), ('wave_irfft_threshold', 'irfft'), ('kenan_update', 'update')):
            inner = getattr(e, name)
            setattr(e, name, lambda *a, _inner=inner, _key=key, **k: (calls.__setitem__(_key, calls[_key] + 1), _inner(*a, **k))[1])
        att = Kenansville(model.cuda(), fft_backend='device', engine=e, **settings)
        att.trace = []
        got_x, got_succ = att.generate(x.cuda(), y.cuda(), targeted=False)
        assert calls == {'rfft': 1, 'irfft': T, 'update': T}                   # one forward transform per batch
    finally:
        e.close()
    assert got_succ == want_succ == [True, True, False]
    assert len(att.trace) == len(ref.trace) == T
    worst_f = 0.0
    for t, ((fd, pd), (fr, pr)) in enumerate(zip(att.trace, ref.trace)):
        assert pd.cpu().tolist() == pr.tolist() == g['preds'][t].tolist(), t
        df = np.abs(fd.cpu().double().numpy() - fr.double().numpy()) / peak
        worst_f = max(worst_f, float(df.max()))
        assert (df <= MARGIN * fwd).all(), (t, df, fwd)
    dx = np.abs(got_x.cpu().double().numpy() - want_x.double().numpy())[:, 0].max(1) / xpeak
    print('device against torch: factors %.3e of max|X| (allowed %.3e), clips %.3e of max|x| (allowed %.3e)' % (worst_f, MARGIN * fwd, dx.max(), MARGIN * inv))
    assert (dx <= MARGIN * inv).all(), (dx, inv)
    assert got_x.shape == x.shape and torch.equal(got_x[2].cpu(), x[2])       # the clip that never succeeds: the input's bits


@pytest.fixture(scope='module')
def chain():
    """A classifier engine with the synthetic VGG19_bn, and AcousticSystem(no defender) on it."""
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.vgg import vgg19_bn
    from dmad_hip import engine as E
    from dmad_hip.transforms import MelSpectrogramDB
    sd = synth.vgg19_bn_state_dict(4321)
    e = E.Engine(max_batch=8, precision=E.FP32, with_wavenet=False)
    e.load_vgg19_bn(sd)
    net = vgg19_bn(num_classes=10, in_channels=1)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    net = net.cuda().eval().bind_engine(e)
    system = AcousticSystem(classifier=net, transform=MelSpectrogramDB(e), defender=None).eval()
    assert system._engine_chain(True) == (e, 0)
    yield e, sd, system
    e.close()


def test_device_backend_on_the_engine_chain(chain):
    from robustness_eval.black_box_attack import Kenansville
    e, _, system = chain
    x = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in (0, 5)])).float().cuda()
    with torch.no_grad():
        y = system(x).argmax(1)
    att = Kenansville(system, max_iter=3, batch_size=2, verbose=0, fft_backend='device')
    assert att.engine is e                                                     # found through model.classifier
    att.trace = []
    queries = []
    inner = e.query_logits
    e.query_logits = lambda xq, *a, **k: (queries.append(tuple(xq.shape)), inner(xq, *a, **k))[1]
    try:
        adver_x, succ = att.generate(x, y, targeted=False)
    finally:
        del e.query_logits
    assert queries == [(2, 1, 16000)] * 3                                      # the one-call path, once per iteration
    assert adver_x.shape == x.shape and len(succ) == 2 and len(att.trace) == 3
    won = torch.stack([p != y for _, p in att.trace])                          # [3, 2]
    assert succ == won.any(0).tolist()
    for i in range(2):
        if not succ[i]:
            assert torch.equal(adver_x[i], x[i])                               # a failed clip comes back as the input's bits
        else:                                                                  # the kept clip is the one of the last success: it is misclassified
            with torch.no_grad():
                assert int(system.query(adver_x[i:i + 1], 1)[0][0].argmax(1)) != int(y[i])
    # the first factor is half of the row maximum of |FFT|
    _, maxmag = e.wave_rfft(x)
    assert torch.equal(att.trace[0][0], maxmag / 2)


def test_driver_run(tmp_path, chain, monkeypatch):
    import kenansville_attack_eval as drv
    from audio_models.ConvNets_SpeechCommands.create_model import create_model
    from models.vgg import vgg19_bn                            # the module path of the reference's pickled checkpoints
    from datasets.sc_dataset import SC09_CLASSES
    from robustness_eval.black_box_attack import Kenansville
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
    net = vgg19_bn(num_classes=10, in_channels=1)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    torch.save(torch.nn.DataParallel(net), str(ck / 'vgg19_bn.pth'))
    args = drv.build_parser().parse_args(['--data_path', str(data), '--classifier_path', str(ck / 'vgg19_bn.pth'), '--attack', 'Kenansville',
                                          '--defense', 'None', '--num_per_class', '1', '--batch_size', '4', '--dataload_workers_nums', '0',
                                          '--verbose', '0'])
    assert args.kenan_method == 'fft' and args.kenan_backend == 'device'
    clf = create_model(args.classifier_path).cuda()
    clf.bind_engine(e)
    lines, made = [], []
    attacker = Kenansville.generate
    monkeypatch.setattr(Kenansville, 'generate', lambda self, **k: (made.append(self), attacker(self, **k))[1])
    out = drv.run(args, classifier=clf, log=lambda *a: lines.append(' '.join(str(v) for v in a)), max_iter=3)
    assert out['total'] == 10
    assert len(made) == 3 and len({id(a) for a in made}) == 1                  # three batches (4 + 4 + 2 clips), one attacker
    assert (made[0].max_iter, made[0].fft_backend, made[0].engine) == (3, 'device', e)
    for k in ('clean_acc', 'denoised_acc', 'robust_acc'):
        assert np.isfinite(out[k]) and 0.0 <= out[k] <= 100.0, (k, out[k])
    assert any(l.startswith('attack: Kenansville with method=fft & iter=3 & backend=device') for l in lines)
    assert [l.split(':')[0] for l in lines[-3:]] == ['original clean test accuracy', 'denoised clean test accuracy', 'CW robust test accuracy']
