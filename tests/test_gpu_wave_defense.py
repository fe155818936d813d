"""The baseline waveform defenses on the engine (csrc/wave_defense.hip, dmad_wave_* and dmad_defense_query_logits) against the 'host'
backend in float64: every op forward and VJP, the IIR kernel's segment edges, the clamp's mask, the adjoint identity, the refusals, the
one-call query path of AcousticSystem and the driver.  Bounds: MS is exact; AS and DS are 4u sum|terms| from a float64 evaluation of the
sum of absolute products; the IIR filters get 8 x the error of a sequential fp32 run of the same filter on the same inputs
(wave_defense_cases.iir_fp32_error, recorded in test_wave_defense_cpu.py)."""
import functools
import wave

import numpy as np
import pytest
import torch

import wave_defense_cases as wc
from dmad_hip import synth
from transforms import _wave_design as wd

pytestmark = pytest.mark.gpu
U, L = wc.U, wc.L
ROWS = {1: [0], 3: [0, 9, 10], 11: list(range(11))}          # rows of clips(11): 9 has the zero tail, 10 is all zero
INF = float('inf')


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault():
    """A failed assertion is one test's business; a HIP error after a test is the device's: nothing more is started on it."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:      # noqa: BLE001
        pytest.exit('HIP error after a test, stopping the session: %s' % e, returncode=3)


@pytest.fixture(scope='module')
def eng():
    from dmad_hip import engine as E
    e = E.Engine(max_batch=8, precision=E.FP32, with_classifier=False, with_wavenet=False)
    yield e
    e.close()


def t64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


def host64(a):
    return a.detach().cpu().double().numpy()


def vjp64(fn, x, g):
    x = t64(x).requires_grad_(True)
    return torch.autograd.grad(fn(x), x, t64(g))[0].numpy()


def resamplers():
    dk, dw, do, dn = wd.sinc_resample_kernel(16000, 8000)
    uk, uw, uo, un = wd.sinc_resample_kernel(8000, 16000)
    return (dk, dw, do, 8000), (uk, uw, uo, 16000)


@functools.lru_cache(maxsize=None)
def reference(op):
    """(forward, forward bound, VJP, VJP bound) of op on clips(11) / grads(11), float64, computed once."""
    x, g = wc.clips(11), wc.grads(11)
    if op == 'AS':
        f = lambda v: wd.host_mean(v, 3)                                                                     # noqa: E731
        return f(t64(x)).numpy(), 4 * U * f(t64(np.abs(x))).numpy(), vjp64(f, x, g), 4 * U * f(t64(np.abs(g))).numpy()
    if op in ('DOWN', 'UP'):
        k, w, o, lout = resamplers()[op == 'UP']
        xin, gin = (x, g[:, :lout]) if op == 'DOWN' else (x[:, :8000], g)
        f = lambda v: wd.host_resample(v, k, w, o, lout)                                                     # noqa: E731
        fa = lambda v: wd.host_resample(v, np.abs(k), w, o, lout)                                            # noqa: E731
        return f(t64(xin)).numpy(), 4 * U * fa(t64(np.abs(xin))).numpy(), vjp64(f, xin, gin), 4 * U * vjp64(fa, xin, np.abs(gin))
    b, a = wc.filters()[op]
    return (wc.lfilter64(b, a, x), wc.iir_fp32_error(op, 'forward') * 8, wc.lfilter64(b, a, g[:, ::-1])[:, ::-1],
            wc.iir_fp32_error(op, 'adjoint') * 8)


def run_op(eng, op, x, g):
    """(forward, VJP) of op on the engine for device rows x and output gradients g."""
    if op == 'AS':
        return eng.wave_smooth(x, 0, 3), eng.wave_smooth_vjp(x, g, 0, 3)
    if op in ('DOWN', 'UP'):
        k, w, o, lout = resamplers()[op == 'UP']
        xin, gin = (x, g[:, :lout]) if op == 'DOWN' else (x[:, :8000], g)
        return eng.wave_resample(xin, k, o, w, lout), eng.wave_resample_vjp(gin, xin.shape[1], k, o, w)
    b, a = wc.filters()[op]
    return eng.wave_iir(x, b, a), eng.wave_iir_vjp(x, g, b, a)


@pytest.mark.parametrize('B', [1, 3, 11])
@pytest.mark.parametrize('op', ['AS', 'DOWN', 'UP', 'LPF', 'BPF', 'order1', 'order8'])
def test_op_against_float64(eng, op, B):
    rows = ROWS[B]
    x, g = dev(wc.clips(11)[rows]), dev(wc.grads(11)[rows])
    y, gx = run_op(eng, op, x, g)
    ry, by, rg, bg = reference(op)
    for name, got, ref, bound in (('forward', y, ry, by), ('vjp', gx, rg, bg)):
        ref, bound = ref[rows], (bound[rows] if isinstance(bound, np.ndarray) else bound)
        err = np.abs(host64(got) - ref)
        print('%s %s B=%d: max err %.3e, max err / bound %.3f, peak %.3e' % (op, name, B, err.max(), (err / (bound + 1e-300)).max(),
                                                                            np.abs(ref).max()))
        assert got.shape == ref.shape and np.all(err <= bound), (op, name, float(err.max()))
    assert bool((y[rows.index(10)] == 0).all()) if 10 in rows else True              # the all-zero clip stays zero
    if B == 11:                                                                       # a row does not depend on its batch or its chunk
        y1, g1 = run_op(eng, op, x[:1], g[:1])
        assert torch.equal(y1[0], y[0]) and torch.equal(g1[0], gx[0])
        y9, g9 = run_op(eng, op, x[9:10], g[9:10])                                    # row 9 sits in the second max_batch chunk
        assert torch.equal(y9[0], y[9]) and torch.equal(g9[0], gx[9])


def median_rule(x, g, w):
    """(y, g_x) of the zero-padded median in numpy with the stated tie rule: the LOWEST window position that holds the median value
    receives the gradient; a padding position receives nothing.  g must be exactly summable."""
    p = (w - 1) // 2
    B, n = x.shape
    xp = np.pad(x, ((0, 0), (p, p)))
    win = np.lib.stride_tricks.sliding_window_view(xp, w, axis=1)                     # [B, n, w]
    med = np.sort(win, axis=2)[:, :, p]
    src = np.argmax(win == med[:, :, None], axis=2)                                   # the first position that holds it
    pos = np.arange(n)[None, :] + src - p                                             # its index in x (outside [0, n): padding)
    gx = np.zeros((B, n), np.float64)
    ok = (pos >= 0) & (pos < n)
    for b in range(B):
        np.add.at(gx[b], pos[b][ok[b]], g[b][ok[b]].astype(np.float64))
    return med, gx


@pytest.mark.parametrize('w', [3, 9])
@pytest.mark.parametrize('B', [1, 3, 11])
def test_median(eng, B, w):
    rows = ROWS[B]
    x = wc.clips(11)[rows]
    g = np.random.default_rng(7).integers(-8, 9, size=x.shape).astype(np.float32) / 8            # sums of <= 9 of these are exact in fp32
    y = eng.wave_smooth(dev(x), 1, w)
    gx = eng.wave_smooth_vjp(dev(x), dev(g), 1, w)
    med, rule = median_rule(x, g, w)
    assert np.array_equal(y.cpu().numpy(), wd.host_median(torch.from_numpy(x.copy()), w).numpy())      # torch.median of an odd window: exact
    assert np.array_equal(y.cpu().numpy(), med)
    assert np.array_equal(host64(gx), rule)                                           # zero tail and zero clip included: the tie rule
    if B == 11:
        assert torch.equal(eng.wave_smooth(dev(x[:1]), 1, w)[0], y[0]) and torch.equal(eng.wave_smooth_vjp(dev(x[:1]), dev(g[:1]), 1, w)[0], gx[0])


def test_median_gradient_equals_autograd_without_ties(eng):
    x = np.random.default_rng(11).standard_normal((3, L)).astype(np.float32)
    for w in (3, 5, 7, 9):
        win = np.lib.stride_tricks.sliding_window_view(np.pad(x, ((0, 0), (w // 2, w // 2))), w, axis=1)
        s = np.sort(win, axis=2)
        assert np.all(s[:, w:-w, 1:] != s[:, w:-w, :-1])                               # tie-free away from the padded edges
        g = np.random.default_rng(w).integers(-8, 9, size=x.shape).astype(np.float32) / 8
        xt = torch.from_numpy(x.copy()).requires_grad_(True)
        ref, = torch.autograd.grad(wd.host_median(xt, w), xt, torch.from_numpy(g))
        got = eng.wave_smooth_vjp(dev(x), dev(g), 1, w).cpu()
        # the padded edges hold several zeros (ties among padding): compare where every window that contains s is tie-free
        assert torch.equal(got[:, 2 * w:-2 * w], ref[:, 2 * w:-2 * w])
        assert np.array_equal(host64(got), median_rule(x, g, w)[1])


@pytest.mark.parametrize('name', ['BPF', 'order8', 'LPF'])
def test_iir_impulses_across_segments(eng, name):
    """An impulse at sample 0, in the last sample of segment 0 and in the first of segment 1: a wrong carry shows in all that follows."""
    b, a = wc.filters()[name]
    x = np.zeros((3, L), np.float32)
    x[0, 0] = x[1, wc.SEG - 1] = x[2, wc.SEG] = 1.0
    ref = wc.lfilter64(b, a, x)
    bound = 8 * np.abs(wc.lfilter32_sequential(b, a, x).astype(np.float64) - ref).max()
    err = np.abs(host64(eng.wave_iir(dev(x), b, a)) - ref)
    print('impulse %s: max err %.3e, bound %.3e, peak %.3e' % (name, err.max(), bound, np.abs(ref).max()))
    assert bound > 0 and err.max() <= bound
    g = eng.wave_iir_vjp(dev(x), dev(x), b, a)                                        # the adjoint of an impulse: the flipped response
    refg = wc.lfilter64(b, a, x[:, ::-1])[:, ::-1]
    assert np.abs(host64(g) - refg).max() <= bound


def test_iir_normalises_by_a0(eng):
    b, a = wc.filters()['BPF']
    x, g = dev(wc.clips(11)[:3]), dev(wc.grads(11)[:3])
    assert torch.equal(eng.wave_iir(x, b * 2, a * 2), eng.wave_iir(x, b, a))
    assert torch.equal(eng.wave_iir_vjp(x, g, b * 2, a * 2), eng.wave_iir_vjp(x, g, b, a))


def test_iir_clamp_and_masked_adjoint(eng):
    b, a = wc.filters()['LPF']
    x = wc.clips(11)[:3].copy()
    x *= 1.1 / np.abs(x).max(axis=1, keepdims=True)                                   # peak 1.1 (0.9 * 1.1 <= 1: the [-1, 1] range of LPF)
    g = wc.grads(11)[:3]
    u = wc.lfilter64(b, a, x)
    fb, ab = 8 * wc.iir_fp32_error('LPF', 'forward') * 1.1 / 0.5, 8 * wc.iir_fp32_error('LPF', 'adjoint')     # the yardstick clips peak at 0.5
    assert int((np.abs(u) > 1 + fb).sum()) >= 10, 'the float64 reference must clamp at least 10 samples'
    near = np.abs(np.abs(u) - 1) <= fb
    assert near.mean() <= 0.01
    gx, y = eng.wave_iir_vjp(dev(x), dev(g), b, a, -1.0, 1.0, want_y=True)
    assert torch.equal(y, eng.wave_iir(dev(x), b, a, -1.0, 1.0))
    yh = host64(y)
    assert np.abs(yh).max() == 1.0 and np.all(np.abs(yh - np.clip(u, -1, 1)) <= fb)
    assert np.all(np.abs(yh[np.abs(u) > 1 + fb]) == 1.0)
    m = np.where(near, np.abs(yh) < 1, np.abs(u) <= 1)                                # inside the bound of +-1 the kernel's own decision counts
    ref = wc.lfilter64(b, a, (g * m)[:, ::-1])[:, ::-1]
    assert np.abs(host64(gx) - ref).max() <= ab
    assert np.abs(ref - wc.lfilter64(b, a, g[:, ::-1])[:, ::-1]).max() > 100 * ab     # the mask matters


@pytest.mark.parametrize('op', ['AS', 'MS', 'DOWN', 'UP', 'LPF', 'BPF'])
def test_adjoint_identity(eng, op):
    """<A x, g> = <x, A^T g> in float64 accumulation, within the summed bounds of both sides, for random x and g."""
    rng = np.random.default_rng(3)
    x, g = rng.standard_normal((3, L)).astype(np.float32) * 0.3, rng.standard_normal((3, L)).astype(np.float32)
    if op == 'MS':
        g = np.round(g * 8) / 8
        y, gx = eng.wave_smooth(dev(x), 1, 3), eng.wave_smooth_vjp(dev(x), dev(g), 1, 3)
        gy, xin, slack = g, x, 0.0                                                    # y[t] = x[src(t)] and the routed sums are exact
    else:
        y, gx = run_op(eng, op, dev(x), dev(g))
        gy, xin = (g[:, :y.shape[1]], x[:, :gx.shape[1]])
        if op in ('LPF', 'BPF'):
            bf = ba = None
            b, a = wc.filters()[op]
            bf = 8 * np.abs(wc.lfilter32_sequential(b, a, x).astype(np.float64) - wc.lfilter64(b, a, x)).max()
            ba = 8 * np.abs(wc.lfilter32_sequential(b, a, g[:, ::-1]).astype(np.float64) - wc.lfilter64(b, a, g[:, ::-1])).max()
            slack = bf * np.abs(gy).sum() + ba * np.abs(xin).sum()
        else:
            k = {'AS': np.full((1, 3), np.float32(1) / np.float32(3)), 'DOWN': resamplers()[0][0], 'UP': resamplers()[1][0]}[op]
            slack = 2 * 4 * U * float(np.abs(k).max()) * k.shape[1] * float(np.abs(gy).max()) * np.abs(xin).sum()
    lhs, rhs = float((host64(y) * gy).sum()), float((xin.astype(np.float64) * host64(gx)).sum())
    print('adjoint %s: <Ax,g> %.9e  <x,ATg> %.9e  diff %.3e  slack %.3e' % (op, lhs, rhs, abs(lhs - rhs), slack))
    assert abs(lhs - rhs) <= slack + 1e-12 * abs(lhs) and abs(lhs) > 1e-3


def test_refusals(eng):
    from dmad_hip._lib import DmadError, DmadWaveDefense, check
    import ctypes as C
    x = dev(wc.clips(11)[:2])
    b, a = wc.filters()['BPF']
    with pytest.raises(DmadError, match='dmad_wave_smooth: window must be odd'):
        eng.wave_smooth(x, 0, 4)
    with pytest.raises(DmadError, match='dmad_wave_smooth: median window must be 3, 5, 7 or 9'):
        eng.wave_smooth(x, 1, 11)
    with pytest.raises(DmadError, match='dmad_wave_smooth_vjp: mean window above 63'):
        eng.wave_smooth_vjp(x, x, 0, 65)
    with pytest.raises(DmadError, match=r'dmad_wave_iir: order outside \[1, 8\]'):
        eng.wave_iir(x, np.ones(10, np.float32), np.ones(10, np.float32))
    with pytest.raises(DmadError, match=r'dmad_wave_iir_vjp: a\[0\] must be finite and non-zero'):
        eng.wave_iir_vjp(x, x, b, a * np.array([0] + [1] * 6, np.float32))
    with pytest.raises(DmadError, match='dmad_wave_resample: phases \\* taps above 256'):
        eng.wave_resample(x, np.ones((2, 200), np.float32), 1, 7, L)
    with pytest.raises(DmadError, match='dmad_wave_iir: null argument'):
        check(eng.lib.dmad_wave_iir(eng._h, None, 2, None, None, 6, -1.0, 1.0, None, None))
    d = DmadWaveDefense(kind=0, window=3)
    d.struct_size -= 4
    with pytest.raises(DmadError, match='dmad_defense_query_logits: dmad_wave_defense.struct_size'):
        check(eng.lib.dmad_defense_query_logits(eng._h, C.c_void_p(x.data_ptr()), 2, 1, C.byref(d), C.c_void_p(x.data_ptr()), None, None))
    with pytest.raises(DmadError, match='with_classifier = 0'):
        eng.defense_query_logits(x, 1, dict(kind='AS', window=3))


@pytest.fixture(scope='module')
def chain():
    """A classifier engine with the calibrated synthetic ResNeXt29 (as in test_gpu_nes.py)."""
    from audio_models.ConvNets_SpeechCommands.models.resnext import CifarResNeXt
    from dmad_hip import engine as E
    sd = synth.resnext29_state_dict(2929)
    e = E.Engine(max_batch=8, precision=E.FP32, with_wavenet=False)
    e.load_resnext29(sd)
    rx = CifarResNeXt(nlabels=10, in_channels=1)
    rx.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    rx = rx.cuda().eval().bind_engine(e)
    yield e, sd, rx
    e.close()


def make_system(kind, e, rx, backend):
    from acoustic_system import AcousticSystem
    from dmad_hip.transforms import MelSpectrogramDB
    from transforms.frequency_defense import FreqDomainDefense
    from transforms.time_defense import TimeDomainDefense
    cls = TimeDomainDefense if kind in ('AS', 'MS') else FreqDomainDefense
    return AcousticSystem(classifier=rx, transform=MelSpectrogramDB(e), defender=cls(kind, backend=backend, engine=e if backend == 'hip' else None)).eval()


@pytest.mark.parametrize('kind', ['AS', 'MS', 'DS', 'LPF', 'BPF'])
def test_query_takes_the_one_call_path(chain, kind, monkeypatch):
    e, _, rx = chain
    x = dev(wc.clips(11)[[0, 5, 9]]).unsqueeze(1)
    system = make_system(kind, e, rx, 'hip')
    assert system._engine_chain(True) == (e, 4) and system._engine_chain(False) == (e, 0)
    calls = []
    real = e.defense_query_logits
    monkeypatch.setattr(e, 'defense_query_logits', lambda *a, **k: (calls.append(a[1]), real(*a, **k))[1])
    monkeypatch.setattr(type(system), 'forward', lambda *a, **k: pytest.fail('query() fell back to forward()'))
    logits, dec = system.query(x, repeats=2)
    monkeypatch.undo()
    assert calls == [2] and logits.shape == (2, 3, 10) and dec.shape == (2, 3)
    with torch.no_grad():
        ref = system(x.repeat(2, 1, 1)).view(2, 3, -1)
    # both run defense -> mel dB -> fp32 classifier on the same kernels and a row does not depend on its batch: the comparison of
    # test_gpu_nes.py between a query and the rows of another batching, torch.equal
    assert torch.equal(logits, ref) and torch.equal(dec, ref.argmax(-1))
    assert not torch.equal(logits[0], system(x, False))                              # the defense did something
    host = make_system(kind, e, rx, 'host')
    assert host._engine_chain(True) == (None, 0)
    seen = []
    fwd = type(host).forward
    monkeypatch.setattr(type(host), 'forward', lambda self, *a, **k: (seen.append(1), fwd(self, *a, **k))[1])
    hl, hd = host.query(x, repeats=2)
    assert seen == [1] and hl.shape == (2, 3, 10) and bool(torch.isfinite(hl).all())


def test_driver_run(tmp_path, chain):
    import baseline_defense_eval as drv
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
    clf = create_model(str(ck / 'resnext29.pth')).cuda()
    clf.bind_engine(e)
    common = ['--data_path', str(data), '--classifier_path', str(ck / 'resnext29.pth'), '--num_per_class', '1', '--batch_size', '4',
              '--dataload_workers_nums', '0', '--verbose', '0']
    for flags, over in ((['--attack', 'CW', '--defense', 'BPF', '--max_iter_1', '2'], {}),
                        (['--attack', 'FAKEBOB', '--defense', 'AS'], dict(max_iter=2, samples_per_draw=4))):
        out = {}
        for backend in ('hip', 'host'):
            lines = []
            args = drv.build_parser().parse_args(common + flags + ['--defense_backend', backend])
            out[backend] = drv.run(args, classifier=clf, log=lambda *a: lines.append(' '.join(str(v) for v in a)), **over)
            assert out[backend]['total'] == 10
            for k in ('clean_acc', 'denoised_acc', 'robust_acc'):
                assert np.isfinite(out[backend][k]) and 0.0 <= out[backend][k] <= 100.0, (k, out[backend][k])
            assert any(l.startswith('defense: %s' % {'BPF': 'Band_Pass_Filter', 'AS': 'Average_Smoothing'}[args.defense]) for l in lines)
        assert out['hip']['clean_acc'] == out['host']['clean_acc'] and out['hip']['denoised_acc'] == out['host']['denoised_acc']
