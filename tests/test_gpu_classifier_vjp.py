"""The classifier-side vector-Jacobian products on the engine (dmad_classify_vjp: ResNeXt29 on its fp32 tier; dmad_mel_db_vjp: the
dB mel front-end), their autograd Functions and module switches (CifarResNeXt.grad_backend, MelSpectrogramDB(grad_backend=)), and
the white-box attack driver built on them (AudioAttack stage 1, adaptive_attack_eval.run)."""
import json
import types

import numpy as np
import pytest
import torch

import vjp_reservation
from dmad_hip import synth

pytestmark = pytest.mark.gpu

VJP_TOL = 1e-4          # relative to max |g|: the tolerance of the UNet VJP test
# The mel VJP against float64: the same fp32 pipeline in torch on the CPU (fp32 stft / matmul / log10 and their autograd) lands at
# 5e-6 relative to max |g_x| on these clips; the 1/M factor of the dB stage takes the fp32 DFT's absolute error into near-silent bins
# at full weight, so the engine's GEMM accumulation order may differ by a small multiple of that.  1e-4 keeps a 20x margin.
MEL_TOL = 1e-4
RX_SEED = 2929


def relmax(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / np.abs(ref).max()


@pytest.fixture(scope='module')
def orc():
    from oracle import dmad_oracle
    return dmad_oracle


def kink_free(sd, inputs):
    """The calibrated stand-in with every ReLU kept away from its kink on the tests' inputs, its masks still depending on channel, pixel
    and batch row.  Layer by layer (float64, eval-mode BN), each channel's BN bias puts the channel's zero in the middle of the widest gap
    between its sorted pre-activations over all inputs and pixels, searched between the 25th and the 75th percentile: at least a quarter
    of the channel's units is on and a quarter off, and no unit lies within half that gap of zero (at least 3e-5 of the channel's largest
    magnitude on these inputs, far above fp32 rounding).  Without it, a ReLU net evaluated in two fp32 orders (engine, MIOpen, fp32
    against float64) flips the odd pre-activation within rounding of zero, and a flip in stage 3 moves the input gradient by up to 1e-2
    of its max over that unit's receptive field — a property of the comparison, not of either gradient.  The head is rescaled to logits
    of a few units (an unsaturated softmax)."""
    import torch.nn.functional as F
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    T = lambda k: torch.from_numpy(np.asarray(out[k])).double()

    def affine(h, p):
        sc = T(p + '.weight') / torch.sqrt(T(p + '.running_var') + 1e-5)
        return h * sc[:, None, None] - (T(p + '.running_mean') * sc)[:, None, None]

    def place(pre, p):
        C = pre.shape[1]
        v = pre.transpose(0, 1).reshape(C, -1).sort(dim=1).values
        n = v.shape[1]
        lo, hi = n // 4, (3 * n) // 4
        k = (v[:, lo + 1:hi + 1] - v[:, lo:hi]).argmax(1) + lo
        c = torch.arange(C)
        mid = 0.5 * (v[c, k] + v[c, k + 1])
        out[p + '.bias'] = (-mid).numpy().astype(np.float32)
        return torch.relu(pre - mid[:, None, None])

    h = place(affine(F.conv2d(inputs, T('conv_1_3x3.weight'), None, 1, 1), 'bn_1'), 'bn_1')
    for st in (1, 2, 3):
        for k in range(3):
            p = 'stage_%d.stage_%d_bottleneck_%d.' % (st, st, k)
            stride = 2 if (k == 0 and st > 1) else 1
            b = place(affine(F.conv2d(h, T(p + 'conv_reduce.weight')), p + 'bn_reduce'), p + 'bn_reduce')
            b = place(affine(F.conv2d(b, T(p + 'conv_conv.weight'), None, stride, 1, 1, 8), p + 'bn'), p + 'bn')
            e = affine(F.conv2d(b, T(p + 'conv_expand.weight')), p + 'bn_expand')
            r = h
            if p + 'shortcut.shortcut_conv.weight' in out:
                ps = p + 'shortcut.shortcut_bn'
                r = affine(F.conv2d(h, T(p + 'shortcut.shortcut_conv.weight'), None, stride), ps) + T(ps + '.bias')[:, None, None]
            h = place(r + e, p + 'bn_expand')
    z = h.mean(dim=(2, 3)) @ T('classifier.weight').t()
    out['classifier.weight'] = (np.asarray(out['classifier.weight']) * (4.0 / float(z.abs().max()))).astype(np.float32)
    return out


def calibration_inputs(orc):
    """every spectrogram the ResNeXt29 tests evaluate: their random maps and the mel spectrograms of their clips"""
    return [specs(2, 1), specs(3, 12), specs(5, 2), specs(7, 3), specs(2, 6), specs(3, 11), orc.mel_db(clips(range(10)).unsqueeze(1))]


@pytest.fixture(scope='module')
def sd(orc):
    return kink_free(synth.resnext29_state_dict(RX_SEED), torch.cat(calibration_inputs(orc)).double())


@pytest.fixture(scope='module')
def eng(sd):
    from dmad_hip import engine as E
    e = E.Engine(max_batch=8, precision=E.FP32, with_wavenet=False)
    e.load_resnext29(sd)
    yield e
    e.close()


def specs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, 32, 32, generator=g) * 60.0 - 70.0).float()      # the dB range of the mel front-end


def clips(ids):
    return torch.from_numpy(np.stack([synth.synthetic_clip(i).reshape(-1) for i in ids])).float()


def oracle_vjp(orc, sd, spec, g):
    sd64 = {k: torch.from_numpy(np.asarray(v)).double() if np.asarray(v).dtype.kind == 'f' else torch.from_numpy(np.asarray(v))
            for k, v in sd.items()}
    x = spec.detach().cpu().double().requires_grad_(True)
    (gx,) = torch.autograd.grad((orc.resnext29_forward(sd64, x) * g.cpu().double()).sum(), x)
    return gx.numpy()


def mel_f64(orc, x):
    """float64 restatement of mel_db: stft (center, constant padding), |.|^2, slaney filterbank, 10 log10(clamp(., 1e-10))."""
    win = torch.hann_window(2048, periodic=True, dtype=torch.float64)
    s = torch.stft(x.reshape(x.shape[0], -1), 2048, 512, 2048, win, center=True, pad_mode='constant', normalized=False, onesided=True,
                   return_complex=True)
    p = s.real ** 2 + s.imag ** 2
    fb = torch.from_numpy(np.asarray(orc.mel_filterbank(1025, 0.0, 8000.0, 32, 16000), np.float64))
    mel = torch.matmul(p.transpose(1, 2), fb).transpose(1, 2)
    return (10.0 * torch.log10(torch.clamp(mel, min=1e-10))).unsqueeze(1)


def test_classify_vjp_against_oracle(eng, orc, sd):
    eng.reserve_classifier_vjp(3)
    for x in (specs(2, 1).cuda(), specs(3, 12).cuda()):      # two inputs in turn: the tape of the second call is its own
        for k in range(3):
            g = torch.randn(x.shape[0], 10, generator=torch.Generator().manual_seed(10 + k)).cuda()
            got = eng.classify_vjp(x, g)
            err = relmax(got.cpu(), oracle_vjp(orc, sd, x, g)[:, 0])
            assert err <= VJP_TOL, (x.shape[0], k, err)


def test_stand_in_masks_vary(orc, sd):
    """kink_free keeps the masks position-dependent: every layer's ReLU mask differs between pixels of a channel and between batch rows"""
    import torch.nn.functional as F
    T = {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items() if np.asarray(v).dtype.kind == 'f'}
    bn = lambda h, p: F.batch_norm(h, T[p + '.running_mean'], T[p + '.running_var'], T[p + '.weight'], T[p + '.bias'], False, 0.0, 1e-5)
    x = specs(3, 12).double()
    pre = bn(F.conv2d(x, T['conv_1_3x3.weight'], None, 1, 1), 'bn_1')
    on = (pre > 0).double()
    per_channel = on.mean(dim=(0, 2, 3))
    assert float(per_channel.min()) > 0.05 and float(per_channel.max()) < 0.95
    assert not torch.equal(on[0], on[1])


def test_mel_vjp_against_f64(eng, orc):
    x = clips([0, 1, 2]).unsqueeze(1)
    g = torch.randn(3, 1, 32, 32, generator=torch.Generator().manual_seed(4))
    x64 = x.double().requires_grad_(True)
    (ref,) = torch.autograd.grad((mel_f64(orc, x64) * g.double()).sum(), x64)
    got = eng.mel_db_vjp(x.cuda(), g.cuda())
    err = relmax(got.cpu(), ref[:, 0])
    assert err <= MEL_TOL, err
    # clips as fix_length leaves them: the second half exactly zero, and an all-zero clip.  Frame fr reads samples [512 fr - 1024,
    # 512 fr + 1024) (reflect padding mirrors zeros into zeros), so frames >= 18 are silent, their mel power is exactly 0 and the
    # clamp(min=1e-10) branch of the dB stage decides the gradient: no gradient, not 10 / (ln 10 * 0).  Samples from 10240 on are read
    # by silent frames only.  The cotangent covers the bins above -40 dB (as the finite-difference test) plus the silent ones, so that
    # max |g_x| is not set by a near-silent bin of the two frames that straddle the edge.
    # A third clip keeps a tail of 1e-9 instead of zeros: mel powers of ~1e-15, above 0 and below the clamp, where the rule is
    # "M >= 1e-10 passes the gradient" and not "M > 0" (which would hand back g * 10 / (ln 10 * 1e-15)).
    z = clips([0, 1, 2]).unsqueeze(1)
    z[0, :, 8000:] = 0.0
    z[1] = 0.0
    z[2, :, 8000:] = 1e-9 * torch.randn(1, 8000, generator=torch.Generator().manual_seed(15))
    spec = eng.mel_db(z.cuda()).cpu()
    assert bool((spec[0, :, :, 18:] < -99.9).all()) and bool((spec[1] < -99.9).all())            # clamp(min=1e-10): -100 dB
    assert bool((spec[2, :, :, 18:] < -99.9).all()) and bool((eng.mel_power(z[2:].cuda()) > 0).all())
    gz = torch.randn(3, 1, 32, 32, generator=torch.Generator().manual_seed(14)) * ((spec > -40.0) | (spec < -99.9)).float()
    assert float(gz[:, :, :, 18:].abs().min()) > 0                       # the silent bins do carry a cotangent
    z64 = z.double().requires_grad_(True)
    (refz,) = torch.autograd.grad((mel_f64(orc, z64) * gz.double()).sum(), z64)
    gotz = eng.mel_db_vjp(z.cuda(), gz.cuda()).cpu()
    assert bool(torch.isfinite(gotz).all())
    assert bool((gotz[0].reshape(-1)[10240:] == 0).all()) and bool((gotz[1] == 0).all()) and bool((gotz[2].reshape(-1)[10240:] == 0).all())
    assert bool((refz[0].reshape(-1)[10240:] == 0).all()) and bool((refz[1] == 0).all()) and bool((refz[2].reshape(-1)[10240:] == 0).all())
    for j in (0, 2):
        errz = relmax(gotz[j].reshape(-1), refz[j].reshape(-1))
        assert errz <= MEL_TOL, (j, errz)


def test_forward_outputs_bitwise(eng):
    x = specs(5, 2).cuda()
    g = torch.randn(5, 10, generator=torch.Generator().manual_seed(2)).cuda()
    eng.reserve_classifier_vjp(5)
    _, lg = eng.classify_vjp(x, g, want_logits=True)
    assert torch.equal(lg, eng.classify_tier(x, 0))
    w = clips([3, 4]).unsqueeze(1).cuda()
    _, sp = eng.mel_db_vjp(w, torch.randn(2, 1, 32, 32).cuda(), want_spec=True)
    assert torch.equal(sp, eng.mel_db(w))


def test_determinism_and_batch_independence(eng):
    x = specs(7, 3).cuda()
    g = torch.randn(7, 10, generator=torch.Generator().manual_seed(3)).cuda()
    eng.reserve_classifier_vjp(7)
    a, b = eng.classify_vjp(x, g), eng.classify_vjp(x, g)
    assert torch.equal(a, b)
    for j in (0, 4, 6):
        assert torch.equal(eng.classify_vjp(x[j:j + 1], g[j:j + 1]), a[j:j + 1])
    w = clips(range(7)).unsqueeze(1).cuda()
    gs = torch.randn(7, 1, 32, 32, generator=torch.Generator().manual_seed(5)).cuda()
    m1, m2 = eng.mel_db_vjp(w, gs), eng.mel_db_vjp(w, gs)
    assert torch.equal(m1, m2)
    for j in (0, 5):
        assert torch.equal(eng.mel_db_vjp(w[j:j + 1], gs[j:j + 1]), m1[j:j + 1])


def test_two_passes_equal_one_pass(sd):
    """B = 2 on a reservation of 1 (two passes of one row) and on a reservation of 2 (one pass): the same bits.  Its own engine: a
    reservation cannot shrink."""
    from dmad_hip import engine as E
    e = E.Engine(max_batch=2, precision=E.FP32, with_wavenet=False)
    e.load_resnext29(sd)
    x = specs(2, 6).cuda()
    g = torch.randn(2, 10, generator=torch.Generator().manual_seed(6)).cuda()
    e.reserve_classifier_vjp(1)
    g1, l1 = e.classify_vjp(x, g, want_logits=True)
    e.reserve_classifier_vjp(2)
    g2, l2 = e.classify_vjp(x, g, want_logits=True)
    assert torch.equal(g1, g2) and torch.equal(l1, l2)
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    e.close()


def test_finite_difference(eng):
    x = specs(2, 6).cuda()
    g = torch.randn(2, 10, generator=torch.Generator().manual_seed(6)).cuda()
    eng.reserve_classifier_vjp(2)
    gx = eng.classify_vjp(x, g).view(2, 1, 32, 32)
    d = torch.randn(2, 1, 32, 32, generator=torch.Generator().manual_seed(7)).cuda()
    # h: below it the fp32 rounding of the logit differences dominates (2 % at h = 1e-4), above it the step crosses kinks (0.3 % at
    # h = 1e-3 in float64 on the CPU, 14 % at 1e-2)
    h = 1e-3
    fd = ((eng.classify_tier(x + h * d, 0) - eng.classify_tier(x - h * d, 0)) * g).sum() / (2 * h)
    an = (gx * d).sum()
    assert abs(float(fd) - float(an)) <= 2e-2 * abs(float(an)), (float(fd), float(an))
    w = clips([5]).unsqueeze(1).cuda()
    # bins above -40 dB only: in near-silent bins the step crosses the log's curvature (second-order terms of the 1/M factor)
    gs = torch.randn(1, 1, 32, 32, generator=torch.Generator().manual_seed(8)).cuda() * (eng.mel_db(w) > -40.0).float()
    gw = eng.mel_db_vjp(w, gs).view(1, 1, -1)
    dw = torch.randn(1, 1, 16000, generator=torch.Generator().manual_seed(9)).cuda() * 1e-4
    fdm = ((eng.mel_db(w + dw) - eng.mel_db(w - dw)) * gs).sum() / 2
    anm = (gw * dw).sum()
    assert abs(float(fdm) - float(anm)) <= 5e-2 * abs(float(anm)), (float(fdm), float(anm))


@pytest.mark.parametrize('prec', ['FP32', 'EXACT', 'BF16'])
def test_every_precision_and_refusals(sd, prec):
    from dmad_hip import engine as E
    from dmad_hip._lib import DmadError
    kw = {'recheck_batch': 4} if prec == 'EXACT' else {}
    e = E.Engine(max_batch=4, precision=getattr(E, prec), with_wavenet=False, **kw)
    with pytest.raises(DmadError):
        e.reserve_classifier_vjp(2)                      # no classifier loaded yet
    e.load_resnext29(sd)
    vjp_reservation.check(e, e.reserve_classifier_vjp, vjp_reservation.grow(e, e.reserve_classifier_vjp, (1, 2, 3), []))
    e.reserve_classifier_vjp(4)
    x = specs(3, 11).cuda()
    g = torch.randn(3, 10, generator=torch.Generator().manual_seed(11)).cuda()
    gx, lg = e.classify_vjp(x, g, want_logits=True)
    assert torch.equal(lg, e.classify_tier(x, 0)) and bool(torch.isfinite(gx).all())
    e.close()
    v = E.Engine(max_batch=4, precision=getattr(E, prec), with_wavenet=False, **kw)
    v.load_vgg19_bn(synth.vgg19_bn_state_dict(4321))
    with pytest.raises(DmadError, match='VGG19_bn'):
        v.reserve_classifier_vjp(2)
    with pytest.raises(DmadError):
        v.classify_vjp(x, g)
    v.close()


@pytest.fixture(scope='module')
def modules(eng, sd):
    from audio_models.ConvNets_SpeechCommands.models.resnext import CifarResNeXt
    rx = CifarResNeXt(nlabels=10, in_channels=1)
    rx.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    rx = rx.cuda().eval()
    rx.bind_engine(eng)
    return rx


def _ce_grad(rx, mel, x, y):
    xg = x.clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(rx(mel(xg)), y)
    (g,) = torch.autograd.grad(loss, xg)
    return g


def test_torch_branch_against_hip(eng, modules):
    from dmad_hip.transforms import MelSpectrogramDB
    rx = modules
    x = clips([0, 1, 2, 3]).unsqueeze(1).cuda()
    y = torch.tensor([1, 3, 5, 7]).cuda()
    rx.grad_backend = 'torch'
    g_t = _ce_grad(rx, MelSpectrogramDB(eng, grad_backend='torch'), x, y)
    rx.zero_grad(set_to_none=True)
    rx.grad_backend = 'hip'
    g_h = _ce_grad(rx, MelSpectrogramDB(eng, grad_backend='hip'), x, y)
    assert all(p.grad is None for p in rx.parameters())
    xg = x.clone().requires_grad_(True)
    torch.nn.functional.cross_entropy(rx(MelSpectrogramDB(eng, grad_backend='hip')(xg)), y).backward()
    assert all(p.grad is None for p in rx.parameters())   # 'hip' computes no weight gradient
    rx.grad_backend = 'auto'
    assert relmax(g_h.cpu(), g_t.cpu()) <= VJP_TOL


def test_attack_defense_none(eng, modules):
    from acoustic_system import AcousticSystem
    from dmad_hip.transforms import MelSpectrogramDB
    from robustness_eval.white_box_attack import AudioAttack
    rx = modules
    rx.grad_backend = 'hip'
    system = AcousticSystem(classifier=rx, transform=MelSpectrogramDB(eng, grad_backend='hip'), defender=None).eval()
    x = clips(range(8)).unsqueeze(1).cuda()
    with torch.no_grad():
        y = system(x).argmax(1)                          # clean predictions as labels: an untargeted attack has work to do
        loss0 = torch.nn.functional.cross_entropy(system(x), y, reduction='none')
    att = AudioAttack(system, eps=65, norm='linf', learning_rate_1=13, max_iter_1=10, max_iter_2=0, eot_attack_size=1, eot_defense_size=1,
                      verbose=0)
    x_adv, (succ, _) = att.generate(x, y, targeted=False)
    rx.grad_backend = 'auto'
    d = x_adv - x
    assert float(d.abs().max()) <= 65 * 2 ** -15 + 1e-6 and float(x_adv.abs().max()) <= 1.0     # + the rounding of (x + d) - x
    with torch.no_grad():
        pred = eng.classify(eng.mel_db(x_adv)).argmax(1)
        loss1 = torch.nn.functional.cross_entropy(system(x_adv), y, reduction='none')
    assert [bool(p != t) for p, t in zip(pred.tolist(), y.tolist())] == succ
    assert float(loss1.mean()) > float(loss0.mean())


def _diff_args(cfg, t):
    return types.SimpleNamespace(ddpm_path=None, ddpm_config=cfg, t=t, score_type='guided_diffusion', sample_step=1, rand_t=False, t_delta=0,
                                 use_bm=False)


@pytest.fixture(scope='module')
def wave_parts(tmp_path_factory, orc):
    """FP32 engine with the WaveNet and a ResNeXt29 stand-in made kink-free also on the mel spectrograms of the purified clips that
    test_attack_revdiffwave_gradient classifies; the purifier with its draws."""
    from dmad_hip import engine as E
    from diffusion_models.diffwave_sde import RevDiffWave
    cfg = tmp_path_factory.mktemp('cvjp') / 'config.json'
    cfg.write_text(json.dumps({'diffusion_config': synth.DIFFUSION_CONFIG, 'wavenet_config': synth.WAVENET_CONFIG}))
    wsd = synth.wavenet_state_dict(1234)
    e = E.Engine(max_batch=4, precision=E.FP32)
    e.load_wavenet(wsd)
    den = RevDiffWave(_diff_args(str(cfg), 1), state_dict=wsd, engine=e, score_grad='hip', seed=3)
    with torch.no_grad():
        den._draws = 0
        pur = den(clips([0, 1, 2]).unsqueeze(1).cuda()).reshape(3, 1, -1).cpu()
    rsd = kink_free(synth.resnext29_state_dict(RX_SEED), torch.cat(calibration_inputs(orc) + [orc.mel_db(pur)]).double())
    e.load_resnext29(rsd)
    yield e, wsd, str(cfg), rsd, den
    e.close()


def test_attack_revdiffwave_gradient(wave_parts):
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.resnext import CifarResNeXt
    from dmad_hip.transforms import MelSpectrogramDB
    e, wsd, cfg, rsd, den = wave_parts
    rx = CifarResNeXt(nlabels=10, in_channels=1)
    rx.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rsd.items()})
    rx = rx.cuda().eval().bind_engine(e)
    x = clips([0, 1, 2]).unsqueeze(1).cuda()
    y = torch.tensor([2, 4, 6]).cuda()
    grads = {}
    for backend in ('torch', 'hip'):
        rx.grad_backend = backend
        system = AcousticSystem(classifier=rx, transform=MelSpectrogramDB(e, grad_backend=backend), defender=den, defense_type='wave')
        den._draws = 0
        xg = x.clone().requires_grad_(True)
        (grads[backend],) = torch.autograd.grad(torch.nn.functional.cross_entropy(system(xg), y), xg)
    rx.grad_backend = 'auto'
    assert bool(torch.isfinite(grads['hip']).all())
    assert relmax(grads['hip'].cpu(), grads['torch'].cpu()) <= VJP_TOL


def test_driver_run(tmp_path, wave_parts):
    import wave
    import adaptive_attack_eval as drv
    from audio_models.ConvNets_SpeechCommands.create_model import create_model
    from models.resnext import CifarResNeXt                  # the module path of the reference's pickled checkpoints
    from datasets.sc_dataset import SC09_CLASSES
    from diffusion_models.diffwave_sde import RevDiffWave
    e, wsd, cfg, sd, _ = wave_parts
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
    for defense in ('None', 'Diffusion'):
        args = drv.build_parser().parse_args(['--data_path', str(data), '--classifier_path', str(ck / 'resnext29.pth'), '--defense', defense,
                                              '--t', '1', '--max_iter_1', '2', '--num_per_class', '1', '--batch_size', '4',
                                              '--dataload_workers_nums', '0', '--verbose', '0', '--score_grad', 'hip'])
        clf = create_model(args.classifier_path).cuda()
        clf.bind_engine(e)
        den = RevDiffWave(_diff_args(cfg, 1), state_dict=wsd, engine=e, score_grad='hip', seed=1) if defense == 'Diffusion' else None
        out = drv.run(args, classifier=clf, defender=den, log=lambda *a: None)
        assert out['total'] == 10
        for k in ('clean_acc', 'denoised_acc', 'robust_acc'):
            assert np.isfinite(out[k]) and 0.0 <= out[k] <= 100.0, (defense, k, out[k])
