"""The plain randomized-smoothing loop as one engine call (dmad_rs_smooth_votes, dmad_m5_rs_smooth_votes; RobustCertificate with
denoiser=None).  The reference of every comparison is built from exports that predate the fused route only: x = clip + sigma *
philox_normal(seed, sample0, 0, n), then mel_db -> classify, or m5_logits, and the first maximum of each row.  The fused route
must give those logits bit for bit, hence those counts."""
import json
import os
import wave

import numpy as np
import pytest
import torch

import m5_cases as mc
from dmad_hip import synth

pytestmark = pytest.mark.gpu

MAXB = 6
M5_ROWS_PER_LAUNCH = 16384           # kM5RsRowsPerLaunch of csrc/dmad_api.hip
# (n, batch, sample0, sigma): one sample, a full pass, a partial last pass, passes of one row; both halves of the 64-bit sample index
SHAPES = [(1, None, 0, 0.25), (MAXB, None, 5, 1.0), (2 * MAXB + 3, None, 2 ** 32 + 7, 0.25), (2 * MAXB + 3, 1, 0, 1.0), (MAXB + 1, 4, 5, 0.25)]
SEED = 11
# RobustCertificate's non-vacuity condition (the host loop's counts cover >= 3 classes) was measured on the host loop alone (_fused_rs
# forced off; seed 3, 64 samples, batch_size 16) over synthetic clips 0-3 and sigma 0.25 / 0.5 / 1.0.  Both nets vote for two classes
# at sigma 0.25 (clip 3 on VGG19_bn: three) and at sigma 1.0, and for three to six at sigma 0.5.  Chosen: synthetic clip 0 at sigma 0.5
# for both: VGG19_bn (synth seed 4321) gives [31, 0, 0, 6, 0, 0, 12, 15, 0, 0], M5 (the trained k = 160 checkpoint)
# [14, 1, 0, 0, 2, 5, 0, 0, 0, 42]
RC_CASE = {'vgg': (0, 0.5), 'm5': (0, 0.5)}

CLASSIFIERS = {'vgg19_bn': (synth.vgg19_bn_state_dict, 'load_vgg19_bn'), 'resnext29': (synth.resnext29_state_dict, 'load_resnext29'),
               'wideresnet28_10': (synth.wideresnet28_10_state_dict, 'load_wideresnet28_10'),
               'densenet_bc_100_12': (synth.densenet_bc_100_12_state_dict, 'load_densenet_bc_100_12')}


def _E():
    from dmad_hip import engine as E
    return E


def new_engine(kind=None, precision='FP32', m5_sd=None, max_batch=MAXB, **kw):
    E = _E()
    if precision == 'EXACT':
        kw.setdefault('recheck_batch', 4)
    e = E.Engine(max_batch=max_batch, precision=getattr(E, precision), with_wavenet=False, **kw)
    if kind is not None:
        sd, loader = CLASSIFIERS[kind]
        getattr(e, loader)(sd())
    if m5_sd is not None:
        e.load_m5(m5_sd)
    return e


def clip_of(i):
    return torch.from_numpy(synth.synthetic_clip(i)).float().reshape(-1).cuda()


def noisy(e, clip, sigma, seed, sample0, n, delta=None):
    """the host loop's inputs [n, L]: clip + delta, or clip + sigma * the Philox normals"""
    return clip.reshape(1, -1) + (delta.reshape(n, -1) if delta is not None else sigma * e.philox_normal(seed, sample0, 0, n))


def ref_mel(e, clip, sigma, seed, sample0, n, delta=None):
    lg = e.classify(e.mel_db(noisy(e, clip, sigma, seed, sample0, n, delta)))
    return lg, torch.bincount(mc.first_max(lg), minlength=lg.shape[1])


def ref_m5(e, clip, sigma, seed, sample0, n, delta=None):
    lp = e.m5_logits(noisy(e, clip, sigma, seed, sample0, n, delta))
    return lp, torch.bincount(mc.first_max(lp), minlength=lp.shape[1])


def fused(e, kind, clip, sigma, n, batch=None, **kw):
    if kind == 'm5':
        return e.m5_rs_smooth_votes(clip, sigma, n, **kw)
    return e.rs_smooth_votes(clip, sigma, n, batch=batch, **kw)


@pytest.fixture(scope='module')
def vgg():
    e = new_engine('vgg19_bn')
    yield e
    e.close()


@pytest.fixture(scope='module', params=['FP32', 'EXACT'])
def resnext(request):
    e = new_engine('resnext29', request.param)
    yield e
    e.close()


@pytest.fixture(scope='module', params=['k160', 'k80'])
def m5(request):
    """both m5_cases nets: K1 = 160 / 10 classes (the trained checkpoint) and K1 = 80 / 35 classes; no classifier, no WaveNet"""
    e = new_engine(m5_sd={'k160': mc.real_sd, 'k80': mc.synth_sd}[request.param](), with_classifier=False)
    yield e
    e.close()


def check_bits(e, kind, ref, shape, clip):
    n, batch, sample0, sigma = shape
    lg_ref, c_ref = ref(e, clip, sigma, SEED, sample0, n)
    counts, lg = fused(e, kind, clip, sigma, n, batch=batch, seed=SEED, sample0=sample0, want_logits=True)
    assert torch.equal(lg, lg_ref), (lg - lg_ref).abs().max().item()
    assert counts.dtype == torch.int64 and counts.tolist() == c_ref.tolist() and int(counts.sum()) == n


# ---- 1. bits against the unfused exports ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES)
def test_bits_vgg19_bn(vgg, shape):
    check_bits(vgg, 'mel', ref_mel, shape, clip_of(0))


@pytest.mark.parametrize('shape', SHAPES)
def test_bits_resnext29(resnext, shape):
    """on the EXACT engine (exact-vote mode) the route must stay on the fp32 tier: dmad_classify's logits, not the 16-bit tier's"""
    E = _E()
    clip = clip_of(1)
    if resnext.precision == E.EXACT:
        assert resnext.mode == E.MODE_EXACT_VOTES
        n, _, sample0, sigma = shape
        spec = resnext.mel_db(noisy(resnext, clip, sigma, SEED, sample0, n))
        assert not torch.equal(resnext.classify_tier(spec, 1), resnext.classify(spec))         # the tiers are told apart by their bits
    check_bits(resnext, 'mel', ref_mel, shape, clip)


@pytest.mark.parametrize('kind', ['wideresnet28_10', 'densenet_bc_100_12'])
def test_bits_unbounded_classifiers_in_the_exact_vote_mode(kind):
    """no recheck bound has been measured for these two, and the other vote loops refuse them in the exact-vote mode; this route
    involves no bound and serves them"""
    E = _E()
    e = new_engine(kind, 'EXACT')
    try:
        assert e.mode == E.MODE_EXACT_VOTES
        clip = clip_of(2)
        with pytest.raises(E.DmadError, match='no recheck bound'):
            e.smooth_votes(clip, 0.5, 0.9, 3, 1.0, 0.1, 4)
        check_bits(e, 'mel', ref_mel, (MAXB + 1, None, 5, 0.25), clip)
    finally:
        e.close()


@pytest.mark.parametrize('shape', SHAPES)
def test_bits_m5(m5, shape):
    check_bits(m5, 'm5', ref_m5, shape, clip_of(3))


# ---- 2. the caller's noise --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['mel', 'm5'])
def test_delta_path(vgg, m5, kind):
    e, ref = (vgg, ref_mel) if kind == 'mel' else (m5, ref_m5)
    clip, n, n1, s0 = clip_of(4), MAXB + 5, 4, 9
    delta = torch.normal(0, 0.5, size=(n, 1, 16000), generator=torch.Generator().manual_seed(5)).cuda()
    lg_ref, c_ref = ref(e, clip, 0.5, 0, 0, n, delta=delta)
    assert not torch.equal(lg_ref, ref(e, clip, 0.5, SEED, s0, n)[0])                        # ... and is not the device noise
    counts, a = fused(e, kind, clip, 0.5, n1, seed=SEED, sample0=s0, delta=delta[:n1], want_logits=True)
    counts, b = fused(e, kind, clip, 0.5, n - n1, seed=SEED, sample0=s0 + n1, delta=delta[n1:], want_logits=True, counts=counts)
    assert torch.equal(torch.cat([a, b]), lg_ref) and counts.tolist() == c_ref.tolist()


# ---- 3. accumulation, sharding, batch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['mel', 'm5'])
def test_accumulation_sharding_and_batch(vgg, m5, kind):
    e, ref = (vgg, ref_mel) if kind == 'mel' else (m5, ref_m5)
    clip, n, n1, s0, sigma = clip_of(5), 2 * MAXB + 3, 5, 2 ** 32 - 3, 1.0                      # the shard boundary crosses 2^32
    whole, _ = fused(e, kind, clip, sigma, n, batch=4, seed=SEED, sample0=s0)
    assert whole.tolist() == ref(e, clip, sigma, SEED, s0, n)[1].tolist()
    start = torch.arange(1, whole.numel() + 1, dtype=torch.int64, device='cuda')
    acc, _ = fused(e, kind, clip, sigma, n1, batch=4, seed=SEED, sample0=s0, counts=start.clone())       # n1 is no multiple of batch
    assert acc.tolist() != start.tolist() and int(acc.sum()) == int(start.sum()) + n1
    acc, _ = fused(e, kind, clip, sigma, n - n1, batch=4, seed=SEED, sample0=s0 + n1, counts=acc)
    assert (acc - start).tolist() == whole.tolist()
    for batch in (1, 3, MAXB, None):
        assert fused(e, kind, clip, sigma, n, batch=batch, seed=SEED, sample0=s0)[0].tolist() == whole.tolist()


def test_m5_rows_per_launch(m5):
    """n above the rows of one launch: the counts are those of two calls cut elsewhere, and the rows behind the cut are the reference's"""
    clip, n, cut, tail = clip_of(0), M5_ROWS_PER_LAUNCH + 5, 9000, 8
    counts, lp = m5.m5_rs_smooth_votes(clip, 0.25, n, seed=SEED, sample0=3, want_logits=True)
    assert int(counts.sum()) == n and counts.tolist() == torch.bincount(mc.first_max(lp), minlength=lp.shape[1]).tolist()
    parts, _ = m5.m5_rs_smooth_votes(clip, 0.25, cut, seed=SEED, sample0=3)
    parts, _ = m5.m5_rs_smooth_votes(clip, 0.25, n - cut, seed=SEED, sample0=3 + cut, counts=parts)
    assert parts.tolist() == counts.tolist()
    lp_ref, _ = ref_m5(m5, clip, 0.25, SEED, 3 + n - tail, tail)                               # rows on both sides of the launch boundary
    assert torch.equal(lp[n - tail:], lp_ref)


# ---- 4. RobustCertificate ---------------------------------------------------------------------------------------------------------------
def vgg_module(e):
    from audio_models.ConvNets_SpeechCommands.models.vgg import vgg19_bn
    net = vgg19_bn(num_classes=10, in_channels=1)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.vgg19_bn_state_dict(4321).items()})
    return net.eval().bind_engine(e)


def certificate(kind, vgg, m5_real, **kw):
    from dmad_hip.transforms import MelSpectrogramDB
    from robustness_eval.certified_robust import RobustCertificate
    if kind == 'vgg':
        return RobustCertificate(classifier=vgg_module(vgg), transform=MelSpectrogramDB(vgg), denoiser=None, **kw), vgg
    net = mc.module(mc.real_sd()).cuda().use_engine(m5_real)
    return RobustCertificate(classifier=net, transform=None, denoiser=None, **kw), m5_real


@pytest.fixture(scope='module')
def m5_real():
    e = new_engine(m5_sd=mc.real_sd(), with_classifier=False)
    yield e
    e.close()


def counted(monkeypatch, e, name):
    calls, inner = [], getattr(e, name)
    monkeypatch.setattr(e, name, lambda *a, **k: calls.append((a[2], k.get('sample0'))) or inner(*a, **k))
    return calls


@pytest.mark.parametrize('kind', ['vgg', 'm5'])
def test_certificate_counts_equal_the_host_loop(vgg, m5_real, kind, monkeypatch):
    """smooth_predict(denoiser=None) on the fused route against the same object forced onto _generic_votes, same seed, batch_size 4 and
    16, device noise and the torch_cpu stream.  Non-vacuity: the host loop alone must vote for at least 3 classes (RC_CASE: synthetic clip 0 at
    sigma 0.5 for both nets, where it was measured to vote for 4 and 5)."""
    from robustness_eval.certified_robust import RobustCertificate
    ci, sigma = RC_CASE[kind]
    x = clip_of(ci).reshape(1, -1)
    for batch_size in (4, 16):
        rc, e = certificate(kind, vgg, m5_real, seed=3)
        calls = counted(monkeypatch, e, 'm5_rs_smooth_votes' if kind == 'm5' else 'rs_smooth_votes')
        got = rc.smooth_predict(x, num_sampling=64, sigma=sigma, batch_size=batch_size)
        assert calls == [(64, 0)] and rc._last is None                                         # one call for the whole loop
        monkeypatch.undo()
        host, _ = certificate(kind, vgg, m5_real, seed=3)
        monkeypatch.setattr(RobustCertificate, '_fused_rs', lambda self: None)
        want = host.smooth_predict(x, num_sampling=64, sigma=sigma, batch_size=batch_size)
        print('%s sigma %g batch_size %d: host loop counts %s' % (kind, sigma, batch_size, want.tolist()))
        assert int((want > 0).sum()) >= 3, want.tolist()
        assert got.tolist() == want.tolist() and got.dtype == want.dtype and got.device == want.device
        # the reference's CPU stream, fed batch by batch as delta
        torch.manual_seed(8)
        want = RobustCertificate(host.classifier, host.transform, None, noise_source='torch_cpu').smooth_predict(x, 37, sigma, batch_size)
        monkeypatch.undo()
        torch.manual_seed(8)
        got = RobustCertificate(rc.classifier, rc.transform, None, noise_source='torch_cpu').smooth_predict(x, 37, sigma, batch_size)
        assert got.tolist() == want.tolist() and int(got.sum()) == 37


@pytest.mark.parametrize('kind', ['vgg', 'm5'])
def test_certify_equal_on_both_routes(vgg, m5_real, kind, monkeypatch):
    from robustness_eval.certified_robust import RobustCertificate
    sigma = RC_CASE[kind][1]
    x = torch.stack([clip_of(0), clip_of(1)]).reshape(2, 1, -1)
    y = torch.tensor([1, 2]).cuda()
    rc, _ = certificate(kind, vgg, m5_real, seed=5)
    got = rc.certify(x, y, sigma=sigma, n_0=20, n=100, batch_size=16)
    host, _ = certificate(kind, vgg, m5_real, seed=5)
    monkeypatch.setattr(RobustCertificate, '_fused_rs', lambda self: None)
    want = host.certify(x, y, sigma=sigma, n_0=20, n=100, batch_size=16)
    assert got[0].tolist() == want[0].tolist() and torch.equal(got[1], want[1])


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------------------
def test_driver_randsmooth_goes_through_the_fused_route(vgg, tmp_path, monkeypatch):
    import certified_robustness_eval as drv
    from datasets.sc_dataset import SC09_CLASSES
    E = _E()
    data = tmp_path / 'test'
    for ci, c in enumerate(SC09_CLASSES):
        (data / c).mkdir(parents=True)
        if ci < 3:
            with wave.open(str(data / c / 'a.wav'), 'wb') as w:
                w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
                w.writeframes(np.clip(np.round(synth.synthetic_clip(ci)[0] * 32768.0), -32768, 32767).astype('<i2').tobytes())
    precision = E._PRECISIONS[os.environ.get('DMAD_PRECISION', 'exact').lower()]
    monkeypatch.setitem(E._ENGINES, (torch.cuda.current_device(), precision), vgg)             # what MelSpectrogramDB() hands out
    calls = counted(monkeypatch, vgg, 'rs_smooth_votes')
    args = drv.build_parser().parse_args(['--data_path', str(data), '--num_per_class', '1', '--defense_method', 'randsmooth', '--sigma', '0.5',
                                          '--num_sampling', '64', '--dataload_workers_nums', '0', '--save_path', str(tmp_path / 'records')])
    torch.manual_seed(3)
    recs = drv.run(args, classifier=vgg_module(vgg), log=lambda *_: None)
    assert json.load(open(tmp_path / 'records' / 'sigma=0.5' / 'sigma=0.5_N=64.json')) == recs and len(recs) == 3
    assert [r['y_true'] for r in recs] == [0, 1, 2] and all((r['y_pred'] == -1) == (r['certified_radius'] == 0) for r in recs)
    assert calls == [(100, 0), (64, 0)] * 3                                                 # n_0 then n, one call each, per clip


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(vgg, m5_real):
    E = _E()
    import ctypes as C
    clip = clip_of(0)
    counts = torch.zeros(10, dtype=torch.int64, device='cuda')
    p, s = (lambda t: C.c_void_p(t.data_ptr())), C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(rc, code, text):
        assert rc == code and text in vgg.lib.dmad_last_error().decode(), (rc, vgg.lib.dmad_last_error())

    rs, m5rs = vgg.lib.dmad_rs_smooth_votes, vgg.lib.dmad_m5_rs_smooth_votes
    refused(rs(vgg._h, p(clip), 0.5, 4, MAXB + 1, 0, 0, None, p(counts), None, s), -2, 'batch %d outside [1, max_batch=%d]' % (MAXB + 1, MAXB))
    refused(rs(vgg._h, p(clip), 0.5, 4, 0, 0, 0, None, p(counts), None, s), -2, 'batch 0 outside')
    refused(rs(vgg._h, p(clip), 0.5, -1, 2, 0, 0, None, p(counts), None, s), -1, 'n < 0')
    refused(rs(vgg._h, p(clip), 0.5, 4, 2, 0, 0, None, None, None, s), -1, 'counts must not be null')
    refused(rs(vgg._h, None, 0.5, 4, 2, 0, 0, None, p(counts), None, s), -1, 'null argument')
    refused(rs(vgg._h, C.c_void_p(clip.data_ptr() + 4), 0.5, 4, 2, 0, 0, None, p(counts), None, s), -1, '16-byte aligned')
    refused(m5rs(vgg._h, p(clip), 0.5, 4, 0, 0, None, p(counts), None, s), -2, 'M5 weights are not finalised')       # no M5 here
    refused(m5rs(m5_real._h, p(clip), 0.5, -1, 0, 0, None, p(counts), None, s), -1, 'n < 0')
    refused(m5rs(m5_real._h, p(clip), 0.5, 4, 0, 0, None, None, None, s), -1, 'counts must not be null')
    refused(m5rs(m5_real._h, C.c_void_p(clip.data_ptr() + 4), 0.5, 4, 0, 0, None, p(counts), None, s), -1, '16-byte aligned')
    refused(rs(m5_real._h, p(clip), 0.5, 4, 2, 0, 0, None, p(counts), None, s), -2, 'with_classifier = 0')           # no classifier there
    with pytest.raises(E.DmadError, match='with_classifier = 0'):
        m5_real.rs_smooth_votes(clip, 0.5, 4)
    with pytest.raises(E.DmadError, match='M5 weights are not finalised'):
        vgg.m5_rs_smooth_votes(clip, 0.5, 4)
    empty = new_engine()                                     # the mel front-end, but no classifier weights yet
    try:
        with pytest.raises(E.DmadError, match='classifier weights are not finalised'):
            empty.rs_smooth_votes(clip, 0.5, 4)
    finally:
        empty.close()
    torch.cuda.synchronize()
    assert counts.tolist() == [0] * 10                       # nothing was launched
    assert vgg.rs_smooth_votes(clip, 0.5, 0)[0].tolist() == [0] * 10 and m5_real.m5_rs_smooth_votes(clip, 0.5, 0)[0].tolist() == [0] * 10
