"""The whole-clip real FFT pair and the Kenansville bisection kernel on the engine (csrc/wave_fft.hip: dmad_wave_rfft,
dmad_wave_irfft_threshold, dmad_kenan_update) against numpy in float64, on engines without a WaveNet and without a classifier.

Lengths: the smallest at which each stage kind can go wrong -- 128 (M = 4*4*4, radix 4 only), 256 (the radix-2 stage), 640 (one radix-5
stage), 3200 (two radix-5 stages) --, 16000 (the workload's length, less than 64 KiB of LDS) and 32000 (more than 64 KiB: the dynamic-LDS
attribute, radix 2 and radix 5 together).  Inputs: three random rows and two synthetic clips per length.

Tolerance: per length the test measures the error of CPU torch.fft in fp32 against float64 on the same rows, relative to the row's
largest |X| (forward) or |x| (inverse), and allows the engine 4 times that, the project's margin for an fp32 kernel against its fp32
restatement.  Both figures are printed.  Threshold decisions: a bin whose float64 magnitude is within the forward tolerance of the factor
may fall on either side; such bins (at most 1 % of a row's) are left out of `kept`, and the output comparison is widened by exactly their
largest possible contribution, 2 |X_k| / L each."""
import functools

import numpy as np
import pytest
import torch

from dmad_hip import synth
from kenansville_cases import stop_after_a_gpu_fault  # noqa: F401  (an autouse fixture)

pytestmark = pytest.mark.gpu
LENGTHS = [128, 256, 640, 3200, 16000, 32000]
FRACTIONS = [0.5, 0.1, 0.01, 0.001, 1e-4]
MARGIN = 4.0


_ENGINES = {}


@pytest.fixture(scope='module')
def engines():
    """engine(L): one FP32 engine per clip length, max_batch 1 (nothing of the FFT pair is sized by it), no WaveNet, no classifier"""
    from dmad_hip import engine as E

    def get(L, precision=E.FP32):
        if (L, precision) not in _ENGINES:
            _ENGINES[(L, precision)] = E.Engine(clip_len=L, max_batch=1, precision=precision, with_classifier=False, with_wavenet=False)
        return _ENGINES[(L, precision)]
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


@functools.lru_cache(maxsize=None)
def rows(L):
    """fp32 [5, L]: three random rows, two synthetic clips"""
    rng = np.random.default_rng(1000 + L)
    x = [0.3 * rng.standard_normal(L) for _ in range(3)] + [synth.synthetic_clip(s, length=L).reshape(-1) for s in (0, 2)]
    x = np.stack(x).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(L):
    """float64 spectrum of rows(L), and the measured fp32 error of CPU torch.fft relative to the row's peak: forward and round trip"""
    x = rows(L)
    X = np.fft.rfft(x.astype(np.float64), axis=1)
    peak = np.abs(X).max(1)
    xt = torch.from_numpy(x.copy())
    X32 = torch.fft.rfft(xt, dim=1)
    fwd = float((np.abs(X32.numpy().astype(np.complex128) - X).max(1) / peak).max())
    back = torch.fft.irfft(X32, n=L, dim=1).numpy().astype(np.float64)
    inv = float((np.abs(back - x).max(1) / np.abs(x).max(1)).max())
    return X, peak, fwd, inv


def cplx(spec):
    s = spec.detach().cpu().double().numpy()
    return s[..., 0] + 1j * s[..., 1]


@pytest.mark.parametrize('L', LENGTHS)
def test_rfft_and_round_trip_against_float64(engines, L):
    e = engines(L)
    x = rows(L)
    X, peak, fwd, inv = reference(L)
    spec, maxmag = e.wave_rfft(torch.from_numpy(x.copy()).cuda())
    assert spec.shape == (5, L // 2 + 1, 2) and maxmag.shape == (5,) and spec.dtype == maxmag.dtype == torch.float32
    got = cplx(spec)
    err = float((np.abs(got - X).max(1) / peak).max())
    err_max = float((np.abs(maxmag.cpu().double().numpy() - peak) / peak).max())
    out, kept = e.wave_irfft_threshold(spec)
    err_inv = float((np.abs(out.cpu().double().numpy() - x).max(1) / np.abs(x).max(1)).max())
    print('L %d forward: torch fp32 %.3e, engine %.3e (maxmag %.3e); round trip: torch fp32 %.3e, engine %.3e' % (L, fwd, err, err_max, inv, err_inv))
    assert bool((spec[:, 0, 1] == 0).all()) and bool((spec[:, -1, 1] == 0).all())           # DC and Nyquist are real
    assert err <= MARGIN * fwd, (L, err, fwd)
    assert err_max <= MARGIN * fwd, (L, err_max, fwd)
    assert err_inv <= MARGIN * inv, (L, err_inv, inv)
    assert kept.dtype == torch.int32 and kept.tolist() == [L // 2 + 1] * 5                 # a null factor keeps every bin


@pytest.mark.parametrize('L', LENGTHS)
def test_threshold_against_the_float64_walk(engines, L):
    e = engines(L)
    x = rows(L)
    X, peak, fwd, _ = reference(L)
    mag = np.abs(X)
    xpeak = np.abs(x).max(1)
    spec, _ = e.wave_rfft(torch.from_numpy(x.copy()).cuda())
    nbins = L // 2 + 1
    X32 = torch.fft.rfft(torch.from_numpy(x.copy()), dim=1)
    walk, worst_torch = [], 0.0
    for c in FRACTIONS:
        f = (c * peak).astype(np.float32)
        f64 = f.astype(np.float64)[:, None]
        near = np.abs(mag - f64) <= MARGIN * fwd * peak[:, None]              # either side is right for these
        assert near.sum(1).max() <= 0.01 * nbins, (L, c, near.sum(1))
        keep = (mag >= f64) & ~near
        want = np.fft.irfft(np.where(keep, X, 0), n=L, axis=1)
        # the fp32 error of torch.fft on the same walk (same mask), relative to the row's peak sample
        y32 = torch.fft.irfft(torch.where(torch.from_numpy(keep), X32, torch.zeros_like(X32)), n=L, dim=1).numpy().astype(np.float64)
        worst_torch = max(worst_torch, float((np.abs(y32 - want).max(1) / xpeak).max()))
        walk.append((c, f, near, keep, want))
    worst = 0.0
    for c, f, near, keep, want in walk:
        slack = 2.0 * np.where(near, mag, 0).sum(1) / L                        # what the left-out bins can add to a sample
        out, kept = e.wave_irfft_threshold(spec, torch.from_numpy(f).cuda())
        diff = np.abs(out.cpu().double().numpy() - want).max(1)
        g_err = float(((diff - slack).clip(min=0) / xpeak).max())
        worst = max(worst, g_err)
        print('L %d factor %g: engine %.3e beyond the %s left-out bins; kept %s' % (L, c, g_err, near.sum(1).tolist(), kept.tolist()))
        k = kept.cpu().numpy()
        assert ((k >= keep.sum(1)) & (k <= keep.sum(1) + near.sum(1))).all(), (L, c, k, keep.sum(1), near.sum(1))
        assert g_err <= MARGIN * worst_torch, (L, c, g_err, worst_torch)
    print('L %d threshold pass: torch fp32 %.3e, engine %.3e' % (L, worst_torch, worst))


@pytest.mark.parametrize('L', [128, 16000, 32000])
def test_bits_do_not_depend_on_the_batch_or_the_call(engines, L):
    e = engines(L)
    x = torch.from_numpy(rows(L).copy()).cuda()
    _, peak, _, _ = reference(L)
    f = torch.from_numpy((0.01 * peak).astype(np.float32)).cuda()
    spec, maxmag = e.wave_rfft(x)
    out, kept = e.wave_irfft_threshold(spec, f)
    spec2, maxmag2 = e.wave_rfft(x)
    out2, kept2 = e.wave_irfft_threshold(spec2, f)
    assert torch.equal(spec, spec2) and torch.equal(maxmag, maxmag2) and torch.equal(out, out2) and torch.equal(kept, kept2)
    for b in (0, 3, 4):
        s1, m1 = e.wave_rfft(x[b:b + 1])
        o1, k1 = e.wave_irfft_threshold(s1, f[b:b + 1])
        assert torch.equal(s1[0], spec[b]) and torch.equal(m1[0], maxmag[b]) and torch.equal(o1[0], out[b]) and int(k1[0]) == int(kept[b]), (L, b)
    # factor 0 cuts nothing: the plain inverse, bit for bit
    o0, k0 = e.wave_irfft_threshold(spec, torch.zeros_like(f))
    on, kn = e.wave_irfft_threshold(spec)
    assert torch.equal(o0, on) and torch.equal(k0, kn)
    # caller-owned outputs are written in place
    o_own, k_own = torch.empty_like(out), torch.empty_like(kept)
    o_ret, k_ret = e.wave_irfft_threshold(spec, f, o_own, k_own)
    assert o_ret is o_own and k_ret is k_own and torch.equal(o_own, out) and torch.equal(k_own, kept)


def test_every_precision_serves_the_pair(engines):
    from dmad_hip import engine as E
    x = torch.from_numpy(rows(640).copy()).cuda()
    base = engines(640).wave_rfft(x)
    for precision in (E.BF16, E.EXACT):
        spec, maxmag = engines(640, precision).wave_rfft(x)
        assert torch.equal(spec, base[0]) and torch.equal(maxmag, base[1])


def torch_update(pred, label, targeted, perturbed, best, lo, hi, factor, succ):
    """the torch fp32 statements of the attack's per-clip loop, on the CPU"""
    best, lo, hi, factor, succ = best.clone(), lo.clone(), hi.clone(), factor.clone(), succ.clone()
    for i in range(pred.shape[0]):
        if (label[i] != pred[i] and not targeted) or (label[i] == pred[i] and targeted):
            best[i, ...] = perturbed[i, ...]
            hi[i] = factor[i]
            factor[i] = ((lo[i] + hi[i]) / 2).abs()
            succ[i] = 1
        else:
            lo[i] = factor[i]
            factor[i] = ((lo[i] + hi[i]) / 2).abs()
    return best, lo, hi, factor, succ


@pytest.mark.parametrize('targeted', [False, True])
def test_kenan_update_bit_for_bit(engines, targeted):
    L = 640
    e = engines(L)
    gen = torch.Generator().manual_seed(5)
    B = 6
    label = torch.tensor([3, 3, 7, 0, 9, 2])
    pred = torch.tensor([3, 4, 7, 1, 9, 5])               # rows 0, 2, 4 agree with the label, rows 1, 3, 5 do not
    perturbed = torch.randn(B, L, generator=gen)
    best = torch.randn(B, L, generator=gen)
    lo = torch.rand(B, generator=gen) * 3
    hi = lo + torch.rand(B, generator=gen) * 500 + 1e-3
    factor = lo + (hi - lo) * torch.rand(B, generator=gen)
    lo[5], hi[5], factor[5] = -7.0, 2.0, -1.5             # a negative midpoint: the abs() acts
    succ = torch.tensor([0, 0, 1, 1, 0, 0], dtype=torch.int32)      # rows 2 and 3 succeeded earlier: whichever fails now keeps best and succ
    want = torch_update(pred, label, targeted, perturbed, best, lo, hi, factor, succ)
    won = (pred == label) if targeted else (pred != label)
    assert won.tolist() == ([True, False] * 3 if targeted else [False, True] * 3)
    dev = [t.clone().cuda() for t in (best, lo, hi, factor, succ)]
    got = e.kenan_update(pred.cuda(), label.cuda(), targeted, perturbed.cuda(), *dev)
    for name, g, w, d in zip(('best', 'fmin', 'fmax', 'factor', 'succ'), got, want, dev):
        assert g is d, name                                # updated in place
        assert torch.equal(g.cpu(), w), name
    kept_row = 2 if not targeted else 3                   # succeeded earlier, fails now
    assert not bool(won[kept_row]) and torch.equal(got[0][kept_row].cpu(), best[kept_row]) and int(got[4][kept_row]) == 1
    assert float(got[3][5]) >= 0
    # a second step from the updated state, as the attack's loop takes it
    want2 = torch_update(pred, label, targeted, perturbed, *want)
    got2 = e.kenan_update(pred.cuda(), label.cuda(), targeted, perturbed.cuda(), *dev)
    for name, g, w in zip(('best', 'fmin', 'fmax', 'factor', 'succ'), got2, want2):
        assert torch.equal(g.cpu(), w), name


def test_refusals(engines):
    from dmad_hip import engine as E
    from dmad_hip._lib import DmadError
    e = engines(640)
    x = torch.from_numpy(rows(640).copy())
    with pytest.raises(DmadError, match='must live on the GPU'):
        e.wave_rfft(x)
    with pytest.raises(AssertionError, match=r'expected \[B,640\]'):
        e.wave_rfft(x[:, :512].cuda())
    spec, _ = e.wave_rfft(x.cuda())
    with pytest.raises(DmadError, match='must live on the GPU'):
        e.wave_irfft_threshold(spec.cpu())
    with pytest.raises(AssertionError, match=r'expected spec \[B,321,2\]'):
        e.wave_irfft_threshold(spec[:, :320])
    with pytest.raises(AssertionError, match='factor'):
        e.wave_irfft_threshold(spec, torch.zeros(4, device='cuda'))
    with pytest.raises(DmadError, match='must live on the GPU'):
        e.kenan_update(torch.zeros(5, dtype=torch.long), torch.zeros(5, dtype=torch.long), False, x.cuda(), x.cuda().clone(),
                       *(torch.zeros(5, device='cuda') for _ in range(3)), torch.zeros(5, device='cuda', dtype=torch.int32))
    odd = E.Engine(clip_len=384, max_batch=1, precision=E.FP32, with_classifier=False, with_wavenet=False)       # M = 192 = 2^6 * 3
    try:
        with pytest.raises(DmadError, match=r"clip_len 384.*radices 4, 2 and 5.*fft_backend='torch'"):
            odd.wave_rfft(torch.zeros(1, 384, device='cuda'))
        with pytest.raises(DmadError, match=r"clip_len 384.*fft_backend='torch'"):
            odd.wave_irfft_threshold(torch.zeros(1, 193, 2, device='cuda'))
    finally:
        odd.close()
