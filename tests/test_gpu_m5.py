"""M5 on the engine (csrc/m5.hip, dmad_m5_*) against float64: the forward on the trained kernel_size = 160 weights and on the synthetic
k = 80 / 35-class net, the tape, the input VJP against the float64 walk pinned to the engine's own decisions (tests/m5_cases.py), the
bit-reproducibility rules, every precision and refusal, the one-call query path of AcousticSystem, the module and the attack, the
drivers and the memory of a gradient.  Clips are full length (16000 samples): all four pool remainders occur there."""
import json
import types
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import m5_cases as mc
from dmad_hip import synth

pytestmark = pytest.mark.gpu

CASES = {'k160': mc.real_sd, 'k80': mc.synth_sd}


def new_engine(sd=None, max_batch=8, precision=None, **kw):
    from dmad_hip import engine as E
    e = E.Engine(max_batch=max_batch, precision=E.FP32 if precision is None else precision, with_wavenet=kw.pop('with_wavenet', False), **kw)
    if sd is not None:
        e.load_m5(sd)
    return e


@pytest.fixture(scope='module', params=sorted(CASES))
def case(request):
    """(name, state dict, engine, clips 0-4 [5,1,L] on the host, their free float64 walk)"""
    sd = CASES[request.param]()
    x = mc.clips(5)
    logp64, rec64 = mc.m5_walk(mc.sd_t(sd), x.double())
    e = new_engine(sd)
    yield request.param, sd, e, x, logp64, rec64
    e.close()


@pytest.fixture(scope='module')
def real():
    sd = mc.real_sd()
    e = new_engine(sd)
    yield sd, e
    e.close()


def bound_module(sd, e, grad_backend='hip'):
    m = mc.module(sd).cuda().use_engine(e)
    m.grad_backend = grad_backend
    return m


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------------
def test_forward_golden(real):
    _, e = real
    x, ref = mc.golden_clips()
    got, dec = e.m5_logits(x.cuda(), want_decisions=True)
    err = (got.cpu() - ref).abs().max().item()
    print('golden |err| %.3e' % err)
    assert err < 1e-4
    assert dec.cpu().tolist() == ref.argmax(1).tolist() == got.argmax(1).cpu().tolist()


def test_forward_vs_float64(case):
    name, _, e, x, logp64, _ = case
    got, dec = e.m5_logits(x.cuda(), want_decisions=True)
    err = (got.cpu().double() - logp64).abs().max().item() / logp64.abs().max().item()
    print(name, 'logp rel err %.3e' % err)
    assert err < mc.FP32_TOL
    assert dec.cpu().tolist() == logp64.argmax(1).tolist()
    assert got.shape == (5, e.m5_classes) and e.m5_classes == {'k160': 10, 'k80': 35}[name]


# ---- 2. tape ----------------------------------------------------------------------------------------------------------------------------
def test_tape(case):
    name, _, e, x, _, rec64 = case
    for layer in (1, 2, 3, 4):
        pooled, dec = e.m5_tape(x.cuda(), layer)
        ref = rec64['pooled'][layer - 1]
        assert tuple(pooled.shape) == tuple(ref.shape) == tuple(dec.shape) and dec.dtype == torch.uint8
        err = (pooled.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
        n, dist, top = mc.kink_distance(rec64, layer - 1, dec)
        print(name, 'layer', layer, 'pooled rel err %.3e, %d decisions differ, farthest %.3e of max |pre| %.3e' % (err, n, dist, top))
        assert err < mc.FP32_TOL
        assert dist <= 2 * mc.FP32_TOL * top             # two values swap order only if each is off by at most the tier's bound
        assert int(dec.max()) <= 7


# ---- 3. VJP -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [2, 3])
def test_vjp_vs_pinned_float64(case, B):
    name, sd, e, x, _, _ = case
    x = x[5 - B:]
    xc = x.cuda()
    g = torch.randn(B, e.m5_classes, generator=torch.Generator().manual_seed(10 + B))
    decs = [e.m5_tape(xc, layer)[1].cpu() for layer in (1, 2, 3, 4)]
    gx = e.m5_vjp(xc, g.cuda()).cpu()
    ref, _ = mc.pinned_vjp(mc.sd_t(sd), x, g, decs)
    assert gx.shape == ref.shape == (B, mc.L)
    err = (gx.double() - ref).abs().amax(1) / ref.abs().amax(1)
    print(name, 'B', B, 'vjp rel err per clip', ['%.2e' % v for v in err.tolist()])
    assert (ref.abs().amax(1) > 0).all() and (err < mc.VJP_TOL).all()          # no clip is left out
    zero = ref == 0
    k1 = np.asarray(sd['conv1.weight']).shape[2]
    assert zero[:, 16 * 935 + k1:].all() and zero.sum() > 0
    assert (gx[zero] == 0).all()


def test_vjp_vs_torch_autograd(real):
    sd, e = real
    x = mc.clips(2, first=5)
    g = torch.randn(2, 10, generator=torch.Generator().manual_seed(4))
    mod = mc.module(sd).cuda()
    xr = x.cuda().requires_grad_(True)
    (ref,) = torch.autograd.grad((mod(xr) * g.cuda()).sum(), xr)
    gx = e.m5_vjp(x.cuda(), g.cuda())
    err = (gx - ref[:, 0]).abs().amax(1) / ref[:, 0].abs().amax(1)
    print('vs fp32 autograd', err.tolist())
    assert (err < mc.VJP_TOL).all()


# ---- 4. bits ------------------------------------------------------------------------------------------------------------------------------
def test_bits(case):
    _, sd, e, x, _, _ = case
    xc = x.cuda()
    g = torch.randn(5, e.m5_classes, generator=torch.Generator().manual_seed(5)).cuda()
    lp, (gx, lp2) = e.m5_logits(xc), e.m5_vjp(xc, g, want_logits=True)
    assert torch.equal(lp, e.m5_logits(xc)) and torch.equal(gx, e.m5_vjp(xc, g))         # two calls
    assert torch.equal(lp, lp2)                                                            # the VJP's log-probs are m5_logits'
    for b in (0, 3):                                                                       # clip b alone = row b of the batch
        assert torch.equal(e.m5_logits(xc[b:b + 1]), lp[b:b + 1])
        assert torch.equal(e.m5_vjp(xc[b:b + 1], g[b:b + 1]), gx[b:b + 1])
    small = new_engine(sd, max_batch=2)                                                    # B = 5 in passes of 2 = one pass of 5
    try:
        assert torch.equal(small.m5_logits(xc), lp) and torch.equal(small.m5_vjp(xc, g), gx)
    finally:
        small.close()


# ---- 5. precisions and refusals -----------------------------------------------------------------------------------------------------------
def test_every_precision_same_bits(real):
    from dmad_hip import engine as E
    sd, e = real
    x = mc.clips(2).cuda()
    g = torch.randn(2, 10, generator=torch.Generator().manual_seed(6)).cuda()
    lp, gx = e.m5_logits(x), e.m5_vjp(x, g)
    for prec in (E.EXACT, E.BF16):
        other = new_engine(sd, max_batch=2, precision=prec)
        try:
            assert torch.equal(other.m5_logits(x), lp) and torch.equal(other.m5_vjp(x, g), gx)
        finally:
            other.close()


def test_refusals(real):
    from dmad_hip._lib import DmadError
    from dmad_hip.autograd import m5_hip
    sd, e = real
    x = mc.clips(2).cuda()
    empty = new_engine()
    try:
        for call in (lambda: empty.m5_logits(x), lambda: empty.m5_vjp(x, torch.zeros(2, 10).cuda()), lambda: empty.m5_tape(x, 1),
                     lambda: empty.m5_query_logits(x, 1), lambda: empty.m5_defense_query_logits(x, 1, dict(kind='AS', window=3))):
            with pytest.raises(DmadError, match=r'\(-2\).*M5 weights are not finalised'):          # DMAD_ERR_STATE
                call()
        # wrong geometry: DMAD_ERR_SHAPE (-4), the message names the field
        bad = dict(sd)
        bad['conv1.weight'] = np.asarray(sd['conv1.weight'])[:, :, :96]
        with pytest.raises(DmadError, match=r'\(-4\).*first_kernel_size'):
            empty.load_m5(bad)
        assert not empty.has_m5
        with pytest.raises(DmadError, match=r'\(-4\).*stride'):
            empty.load_m5(sd, stride=8)
        wide = synth.m5_state_dict(3, 80, 65)
        with pytest.raises(DmadError, match=r'\(-4\).*n_output'):
            empty.load_m5(wide)
        two = synth.m5_state_dict(3, 80, 35)
        two['conv1.weight'] = np.repeat(two['conv1.weight'], 2, axis=1)
        with pytest.raises(DmadError, match=r'\(-4\).*n_input'):
            empty.load_m5(two)
        with pytest.raises(DmadError, match=r'\(-4\).*n_channel'):
            empty.load_m5(synth.m5_state_dict(3, 80, 35, n_channel=16))
        # a refused set leaves nothing behind: the next finalise, of another part, does not retry it
        other = new_engine(max_batch=2)
        try:
            with pytest.raises(DmadError, match=r'\(-4\).*n_channel'):
                other.load_m5(synth.m5_state_dict(3, 80, 35, n_channel=16))
            other.load_vgg19_bn(synth.vgg19_bn_state_dict(4321))
            assert other.has_classifier and not other.has_m5
            other.load_m5(sd)
            assert torch.equal(other.m5_logits(x), e.m5_logits(x))
        finally:
            other.close()
        # the engine's clip length: too short for first_kernel_size, too short for the four pools, too long for the LDS of one CU
        for clip_len, k1, why in ((128, 160, 'at least first_kernel_size'), (1024, 80, 'too short'), (32000, 160, 'too long')):
            odd = new_engine(max_batch=2, clip_len=clip_len, with_classifier=False)
            try:
                with pytest.raises(DmadError, match=r'\(-4\).*clip_len.*' + why):
                    odd.load_m5(sd if k1 == 160 else mc.synth_sd())
                assert not odd.has_m5
            finally:
                odd.close()
        empty.load_m5(sd)                                  # the refused sets left nothing behind
        assert torch.equal(empty.m5_logits(x), e.m5_logits(x))
        with pytest.raises(DmadError, match='with_classifier|classifier weights are not finalised'):
            empty.classify(torch.zeros(1, 1, 32, 32).cuda())          # dmad_classify on an M5-only engine fails as before
    finally:
        empty.close()
    # a second, different M5 is refused by bind; the same one is accepted
    e.bind('m5', sd, e.load_m5)
    with pytest.raises(DmadError, match='different m5 weights'):
        e.bind('m5', mc.synth_sd(), e.load_m5)
    with pytest.raises(DmadError, match='different m5 weights'):
        mc.module(mc.synth_sd()).cuda().use_engine(e)
    # create_graph=True
    xr = x.clone().requires_grad_(True)
    out = m5_hip(e, xr)
    with pytest.raises(DmadError, match='first-order only'):
        torch.autograd.grad(out.sum(), xr, create_graph=True)
    with pytest.raises(DmadError, match=r'\(-2\).*WaveNet'):
        e.m5_query_logits(x, 1, sampler=2, t_star=1, c_a=1.0, c_b=0.0)   # no WaveNet in this engine


def test_vgg_and_m5_in_one_engine(real):
    sd, e = real
    both = new_engine(sd, max_batch=2)
    try:
        vsd = synth.vgg19_bn_state_dict(4321)
        both.load_vgg19_bn(vsd)
        only = new_engine(max_batch=2)
        only.load_vgg19_bn(vsd)
        x = mc.clips(2).cuda()
        spec = only.mel_db(x)
        assert torch.equal(both.classify(both.mel_db(x)), only.classify(spec))
        assert torch.equal(both.m5_logits(x), e.m5_logits(x))
        assert both.has_classifier and both.has_m5 and both.classifier_kind == 'vgg19_bn'
        only.close()
    finally:
        both.close()


# ---- 6. query path ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def wave_engine():
    """FP32 engine with the synthetic WaveNet and the real M5"""
    from dmad_hip import engine as E
    e = E.Engine(max_batch=4, precision=E.FP32)
    e.load_wavenet(synth.wavenet_state_dict(1234))
    sd = mc.real_sd()
    e.load_m5(sd)
    yield e, sd
    e.close()


def counted(monkeypatch, e, name):
    calls = []
    real_fn = getattr(e, name)
    monkeypatch.setattr(e, name, lambda *a, **k: (calls.append(a[1]), real_fn(*a, **k))[1])
    return calls


def test_query_path(wave_engine, monkeypatch):
    from acoustic_system import AcousticSystem
    from diffusion_models.diffwave_ddpm import DiffWave, WaveNetHIP
    from diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams
    from transforms.time_defense import TimeDomainDefense
    e, sd = wave_engine
    m5 = bound_module(sd, e)
    x = mc.clips(2).cuda()
    B, R = 2, 3
    # sampler 0
    plain = AcousticSystem(classifier=m5, transform=None, defender=None).eval()
    assert plain._engine_chain(True) == (e, 0)
    calls = counted(monkeypatch, e, 'm5_query_logits')
    monkeypatch.setattr(AcousticSystem, 'forward', lambda *a, **k: pytest.fail('query() fell back to forward()'))
    logits, dec = plain.query(x, repeats=R)
    assert calls == [R] and logits.shape == (R, B, 10) and dec.shape == (R, B) and dec.dtype == torch.int64
    assert torch.equal(logits.reshape(R * B, 10), e.m5_logits(x.repeat(R, 1, 1))) and torch.equal(dec, logits.argmax(-1))
    # sampler 1: DiffWave on device noise, t* = 2
    den = DiffWave(WaveNetHIP(e), calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG), reverse_timestep=2, seed=17)
    system = AcousticSystem(classifier=m5, transform=None, defender=den, defense_type='wave').eval()
    assert system._engine_chain(True) == (e, 1) and system._engine_chain(False) == (e, 0)
    den._draws = 100
    del calls[:]
    logits, dec = system.query(x, repeats=R)                       # 6 rows > max_batch 4: chunked inside the call
    assert calls == [R] and den._draws == 100 + R * B and logits.shape == (R, B, 10)
    ts, c_a, c_b, c_eps, c_div, c_sig = den.purify_coefficients()
    pur = e.ddpm_purify(x.repeat(R, 1, 1), ts, c_a, c_b, c_eps, c_div, c_sig, seed=17, sample0=100)
    assert torch.equal(logits.reshape(R * B, 10), e.m5_logits(pur)) and torch.equal(dec, logits.argmax(-1))
    assert not torch.equal(logits[0], logits[1])                    # fresh noise per repeat
    one, _ = e.m5_query_logits(x[1:2], 1, 1, ts, c_a, c_b, c_eps, c_div, c_sig, seed=17, sample0=100 + 2 * B + 1)
    assert torch.equal(one, logits[2, 1:2])                         # row (2, 1) alone, by its key
    # a baseline defense on backend 'hip'
    smooth = AcousticSystem(classifier=m5, transform=None, defender=TimeDomainDefense('AS', backend='hip', engine=e)).eval()
    assert smooth._engine_chain(True) == (e, 4)
    dcalls = counted(monkeypatch, e, 'm5_defense_query_logits')
    dl, dd = smooth.query(x, repeats=2)
    assert dcalls == [2] and dl.shape == (2, B, 10)
    y = e.wave_smooth(x, 0, smooth.defender.engine_defense(x)['window'])
    assert torch.equal(dl[0], e.m5_logits(y)) and torch.equal(dl[0], dl[1]) and torch.equal(dd, dl.argmax(-1))
    assert not torch.equal(dl[0], e.m5_logits(x))                   # the defense did something
    monkeypatch.undo()
    # a default (unbound) M5 keeps the forward loop
    loose = AcousticSystem(classifier=mc.module(sd).cuda(), transform=None, defender=None).eval()
    assert loose._engine_chain(True) == (None, 0)
    ll, _ = loose.query(x, repeats=2)
    assert ll.shape == (2, B, 10) and (ll[0] - e.m5_logits(x)).abs().max().item() < 1e-4


# ---- 7. module and attack ---------------------------------------------------------------------------------------------------------------
def test_module_gradient(real):
    from acoustic_system import AcousticSystem
    sd, e = real
    x = mc.clips(3).cuda()
    grads = {}
    for backend in ('hip', 'torch'):
        system = AcousticSystem(bound_module(sd, e, backend), None, None).eval()
        xr = x.clone().requires_grad_(True)
        out = system(xr)
        y = out.detach().argmax(1)
        (grads[backend],) = torch.autograd.grad(F.cross_entropy(out, y), xr)
        if backend == 'hip':
            assert torch.equal(out.detach(), e.m5_logits(x))
            lp = e.m5_logits(x).requires_grad_(True)         # the cotangent autograd hands the VJP: softmax(logp) - onehot, over 3 clips
            (cot,) = torch.autograd.grad(F.cross_entropy(lp, y), lp)
            assert torch.allclose(cot, (torch.softmax(lp.detach(), 1) - F.one_hot(y, 10).float()) / 3, atol=1e-7)
            assert torch.equal(grads['hip'][:, 0], e.m5_vjp(x, cot))
    err = (grads['hip'] - grads['torch']).abs().amax((1, 2)) / grads['torch'].abs().amax((1, 2))
    assert (err < mc.VJP_TOL).all(), err
    with torch.no_grad():                                   # without a gradient the forward is the engine's
        assert torch.equal(AcousticSystem(bound_module(sd, e), None, None).eval()(x), e.m5_logits(x))
    m = bound_module(sd, e).train()                         # training mode: the layers
    assert m(x).shape == (3, 10) and m.bn1.num_batches_tracked.item() > 0


def test_attack(real):
    from acoustic_system import AcousticSystem
    from robustness_eval.white_box_attack import AudioAttack
    sd, e = real
    system = AcousticSystem(bound_module(sd, e), None, None).eval()
    x = mc.clips(8).cuda()
    y = e.m5_logits(x).argmax(1)
    loss0 = F.cross_entropy(e.m5_logits(x), y).item()
    attack = AudioAttack(model=system, eps=65, norm='linf', max_iter_1=10, max_iter_2=0, learning_rate_1=13, eot_attack_size=1,
                         eot_defense_size=1, verbose=0)
    x_adv, (success, _) = attack.generate(x=x, y=y, targeted=False)
    assert (x_adv - x).abs().max().item() <= 65 * 2 ** -15 + 1e-6
    out = e.m5_logits(x_adv)
    assert success == (out.argmax(1) != y).tolist()
    loss1 = F.cross_entropy(out, y).item()
    print('attack: %d of 8 flipped, mean loss %.3f -> %.3f' % (sum(success), loss0, loss1))
    assert loss1 > loss0


def test_gradient_through_revdiffwave(wave_engine, tmp_path):
    from acoustic_system import AcousticSystem
    from diffusion_models.diffwave_sde import RevDiffWave
    e, sd = wave_engine
    cfg = tmp_path / 'config.json'
    cfg.write_text(json.dumps({'diffusion_config': synth.DIFFUSION_CONFIG, 'wavenet_config': synth.WAVENET_CONFIG}))
    args = types.SimpleNamespace(ddpm_path=None, ddpm_config=str(cfg), t=1, score_type='guided_diffusion', sample_step=1, rand_t=False,
                                 t_delta=0, use_bm=False)
    den = RevDiffWave(args, state_dict=synth.wavenet_state_dict(1234), engine=e, score_grad='hip', seed=3)
    x = mc.clips(3).cuda()
    grads = {}
    for backend in ('hip', 'torch'):
        system = AcousticSystem(bound_module(sd, e, backend), None, den, defense_type='wave').eval()
        den._draws = 0
        xr = x.clone().requires_grad_(True)
        out = system(xr)
        (grads[backend],) = torch.autograd.grad(F.cross_entropy(out, out.detach().argmax(1)), xr)
    err = (grads['hip'] - grads['torch']).abs().amax((1, 2)) / grads['torch'].abs().amax((1, 2))
    print('through RevDiffWave', err.tolist())
    assert (err < mc.VJP_TOL).all()


# ---- 8. drivers ---------------------------------------------------------------------------------------------------------------------------
def test_drivers(wave_engine, tmp_path):
    import adaptive_attack_eval as white
    import baseline_defense_eval as base
    import black_box_attack_eval as fakebob
    import siren_attack_eval as siren
    from audio_models.ConvNets_SpeechCommands.create_model import create_model
    from datasets.sc_dataset import SC09_CLASSES
    from diffusion_models.diffwave_sde import RevDiffWave
    from M5Net import M5                                       # the module path of the reference's pickled M5 checkpoints
    e, sd = wave_engine
    data = tmp_path / 'test'
    for i, c in enumerate(SC09_CLASSES[:10]):
        (data / c).mkdir(parents=True)
        pcm = (synth.synthetic_clip(i).reshape(-1) * 32767).astype('<i2')
        with wave.open(str(data / c / 'a.wav'), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(pcm.tobytes())
    m = M5(n_input=1, first_kernel_size=160, n_output=10)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    ck = tmp_path / 'm5_k160.pth'
    torch.save(m, str(ck))
    cfg = tmp_path / 'config.json'
    cfg.write_text(json.dumps({'diffusion_config': synth.DIFFUSION_CONFIG, 'wavenet_config': synth.WAVENET_CONFIG}))
    common = ['--data_path', str(data), '--classifier_path', str(ck), '--num_per_class', '1', '--batch_size', '4',
              '--dataload_workers_nums', '0', '--verbose', '0']

    def classifier():
        clf = create_model(str(ck)).cuda()
        assert type(clf).__name__ == 'M5' and 'engine' not in clf.__dict__
        return clf.use_engine(e)

    def check(out):
        assert out['total'] == 10
        for k in ('clean_acc', 'denoised_acc', 'robust_acc'):
            assert np.isfinite(out[k]) and 0 <= out[k] <= 100

    quiet = lambda *a: None                                   # noqa: E731
    for defense in ('None', 'Diffusion'):
        args = white.build_parser().parse_args(common + ['--defense', defense, '--t', '1', '--max_iter_1', '2', '--score_grad', 'hip'])
        den = None
        if defense == 'Diffusion':
            dargs = types.SimpleNamespace(ddpm_path=None, ddpm_config=str(cfg), t=1, score_type='guided_diffusion', sample_step=1,
                                          rand_t=False, t_delta=0, use_bm=False)
            den = RevDiffWave(dargs, state_dict=synth.wavenet_state_dict(1234), engine=e, score_grad='hip', seed=1)
        clf = classifier()
        check(white.run(args, classifier=clf, defender=den, log=quiet))
        assert clf.grad_backend == 'hip'
    args = fakebob.build_parser().parse_args(common + ['--attack', 'FAKEBOB', '--defense', 'None'])
    assert args.nes_noise == 'device'
    check(fakebob.run(args, classifier=classifier(), log=quiet, max_iter=2, samples_per_draw=4))
    args = siren.build_parser().parse_args(common + ['--attack', 'SirenAttack', '--defense', 'None'])
    assert args.swarm_noise == 'device'
    check(siren.run(args, classifier=classifier(), log=quiet, max_epoch=1, max_iter=2, n_particles=3))
    args = base.build_parser().parse_args(common + ['--attack', 'CW', '--defense', 'AS', '--max_iter_1', '2', '--defense_backend', 'hip'])
    check(base.run(args, classifier=classifier(), log=quiet))
    with pytest.raises(NotImplementedError, match='spectrogram'):
        white.run(white.build_parser().parse_args(common + ['--defense', 'Diffusion-Spec']), classifier=classifier(), log=quiet)


# ---- 9. memory ------------------------------------------------------------------------------------------------------------------------------
def test_vjp_memory():
    sd = mc.real_sd()
    e = new_engine(sd, max_batch=64)
    try:
        B = 64
        x = torch.randn(B, 1, mc.L, device='cuda') * 0.1
        g = torch.randn(B, 10, device='cuda')
        e.m5_vjp(x[:2], g[:2])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        gx = e.m5_vjp(x, g)
        torch.cuda.synchronize()
        grew = torch.cuda.max_memory_allocated() - base
        print('m5_vjp at B = 64 allocates %d bytes' % grew)
        assert gx.shape == (B, mc.L)
        assert grew <= 2 * B * mc.L * 4 + (1 << 20)        # the returned gradient plus one contiguous copy of the input
        mod = mc.module(sd).cuda()
        xr = x.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.autograd.grad((mod(xr) * g).sum(), xr)
        torch.cuda.synchronize()
        layers = torch.cuda.max_memory_allocated() - base
        print('the torch layers allocate %d bytes' % layers)
        assert layers >= 2 * B * 32 * 991 * 4                # at least the conv1 and BatchNorm outputs: about 4x the engine's bound
    finally:
        e.close()
