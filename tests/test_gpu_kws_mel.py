"""The keyword spotter's mel front-end on the engine (csrc/kws_mel.hip, dmad_kws_mel_* / dmad_kws_wave_* / dmad_kws_*query_logits) against
the float64 matrix-form walk of tests/kws_mel_cases.py, which tests/test_kws_mel_cpu.py proves against torch.stft-based autograd: forward
and VJP on every length, the bit rules, the fused waveform -> log-probability route and its gradient, AcousticSystem's routing, the
refusals, and the attack driver on a small dataset.

Cases.  L = 800 (T = 5, the smallest row: both reflections inside one tile), 801, 999 | 1000 (the step T 5 -> 6), 1237 (a right fold of
163 samples), 6600, 16000 (the driver's length), the L whose T is one below, at and one above the kernel's frame tile of 8, and once the
cap L = 128 799 (T = 644) at B = 2.  Rows: noise * 0.1; 0.5 sin(2 pi 440 t) + 1e-3 noise (quiet bins, cancellation); silence, whose dB
must be exactly -100 and whose gradient exactly 0.

Tolerance.  The yardstick is the fp32 CPU run of the matrix-form walk against its float64 run on the same input (kws_mel_cases.case):
absolute in dB for the spectrogram, of the largest value for the mel power, of the gradient's maximum for g_x, and never less than one
ulp (2^-23) of the largest value.  The engine is allowed FACTOR = 4 x that, as in test_gpu_kws.py: the same precision, another summation
order (one chain of 400 terms per bin where the CPU's GEMM blocks), the device's log10.  For the waveform gradient of the fused route
the same yardstick is computed in the test from the fp32 module + fp32 walk against the float64 pair.

Margins, measured on the CPU with the float64 walk on these inputs (a break that stays inside the allowance is not caught): the
symmetric Hann window in place of the periodic one lands 470 to 1700 x outside the dB allowance and 200 to 770 x outside the gradient's;
the slaney scale in place of htk 4000 to 14000 x and 770 to 5400 x; a dropped fold of the reflected samples does not move the
spectrogram at all and lands 46 (L = 16000) to 770 x outside the gradient's allowance.  The engine's measured errors are in DESIGN
section 23."""
import os
import wave

import numpy as np
import pytest
import torch

import kws_cases as kc
import kws_mel_cases as mc

pytestmark = pytest.mark.gpu

FACTOR = 4.0
ULP = 2.0 ** -23
LENGTHS = mc.CASES + mc.TILE_CASES
FUSED = (800, 1237, 16000)


def new_engine(sd=None):
    from dmad_hip import engine as E
    e = E.Engine(max_batch=8, precision=E.FP32, with_wavenet=False, with_classifier=False)       # clip_len 16000: the query exports' L
    if sd is not None:
        e.load_kws(sd)
    return e


@pytest.fixture(scope='module')
def eng():
    e = new_engine(kc.state_dict())
    yield e
    e.close()


def module(dtype=torch.float32):
    from audio_models.RCNN_KWS.model import KWSModel
    net = KWSModel(in_size=32)
    net.load_state_dict(kc.state_dict())
    return net.to(dtype).eval()


def raw_vjp(e, x, g, want_spec=True):
    """dmad_kws_mel_db_vjp into buffers this test pre-fills with NaN: (g_x [B,L], spec [B,32,T])"""
    from dmad_hip import engine as E
    xw, gs = x.cuda().float().contiguous(), g.cuda().float().contiguous()
    B, L = xw.shape
    gx = torch.full_like(xw, float('nan'))
    sp = torch.full((B, 32, mc.frames_of(L)), float('nan'), device='cuda')
    E.check(e.lib.dmad_kws_mel_db_vjp(e._h, E._ptr(xw), B, L, E._ptr(gs), E._ptr(gx), E._ptr(sp) if want_spec else None, E._stream()))
    return gx, sp


def check_forward(e, L, B=3):
    x, g, ref, e_db, e_pow, e_g = mc.case(L, B)
    db, power = e.kws_mel_db(x.cuda()), e.kws_mel_power(x.cuda())
    assert tuple(db.shape) == tuple(power.shape) == (B, 32, mc.frames_of(L))
    err_db = (db.cpu().double() - ref['db']).abs().max().item()
    err_pow = (power.cpu().double() - ref['mel']).abs().max().item() / ref['mel'].abs().max().item()
    rows_db = [(db[i].cpu().double() - ref['db'][i]).abs().max().item() for i in range(B)]
    print('L = %d (T = %d): dB |err| %.3e of allowed %.3e (per row %s); power %.3e of allowed %.3e of its maximum'
          % (L, ref['T'], err_db, FACTOR * e_db, ' '.join('%.2e' % r for r in rows_db), err_pow, FACTOR * e_pow))
    assert err_db <= FACTOR * e_db and err_pow <= FACTOR * e_pow
    if B > 2:
        assert (db[2] == -100.0).all() and (power[2] == 0.0).all()                   # silence
    return x, db


def check_vjp(e, L, B=3):
    x, g, ref, e_db, e_pow, e_g = mc.case(L, B)
    gx, sp = raw_vjp(e, x, g)
    gmax = ref['g_x'].abs().max().item()
    err = (gx.cpu().double() - ref['g_x']).abs().max().item() / gmax
    print('L = %d (T = %d): gradient |err| %.3e of allowed %.3e of its maximum %.3g' % (L, ref['T'], err, FACTOR * e_g, gmax))
    assert not torch.isnan(gx).any() and not torch.isnan(sp).any()                    # every element was written over the NaN
    assert err <= FACTOR * e_g
    if B > 2:
        assert (gx[2] == 0.0).all()
    assert torch.equal(sp, e.kws_mel_db(x.cuda()))                                    # the VJP's spectrogram: the forward's bits
    assert torch.equal(e.kws_mel_db_vjp(x.cuda(), g.cuda()), gx)                      # the wrapper
    assert torch.equal(e.kws_mel_db_vjp(x.cuda()[:, None], g.cuda()[:, None]), gx)    # ... [B,1,L] and [B,1,32,T] in


# ---- 1. forward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', LENGTHS)
def test_forward_vs_walk(eng, L, monkeypatch):
    x, db = check_forward(eng, L)
    from dmad_hip import engine as E
    from shims.torchaudio import transforms as T
    monkeypatch.setattr(E, 'get_engine', lambda *a, **k: eng)                         # the shims run on the shared engine
    pair = torch.nn.Sequential(T.MelSpectrogram(sample_rate=16000, n_mels=32), T.AmplitudeToDB(stype='power'))
    out = pair(x.cuda()[:, None])
    assert tuple(out.shape) == (3, 1, 32, mc.frames_of(L)) and torch.equal(out[:, 0], db)
    from dmad_hip.transforms import KWSMelSpectrogramDB
    assert torch.equal(KWSMelSpectrogramDB(eng)(x.cuda()[:, None]), out)


# ---- 2. VJP -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', LENGTHS)
def test_vjp_vs_walk(eng, L):
    check_vjp(eng, L)


def test_forward_and_vjp_at_the_cap(eng):
    check_forward(eng, mc.CAP, B=2)
    check_vjp(eng, mc.CAP, B=2)


# ---- 3. bits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', (1237, 16000))
def test_bits(eng, L):
    x, g = mc.rows(L, 7)
    x, g = x.cuda(), g.cuda()
    db7, gx7 = eng.kws_mel_db(x), eng.kws_mel_db_vjp(x, g)
    db1, gx1 = eng.kws_mel_db(x[5:6].clone()), eng.kws_mel_db_vjp(x[5:6].clone(), g[5:6].clone())
    assert torch.equal(db1[0], db7[5]) and torch.equal(gx1[0], gx7[5])                # alone, and as row 5 of 7
    assert torch.equal(eng.kws_mel_db(x), db7) and torch.equal(eng.kws_mel_db_vjp(x, g), gx7)      # and in a second call
    assert not torch.equal(db7[5], db7[4])
    # frame f is the same in the clip cut to 200 (f + 2) samples, where no right fold touches it: another tile count, another place in
    # its tile, another length
    T = mc.frames_of(L)
    for f in sorted({0, 1, 3, 7, 8, 9, 15, 16, T - 3}):
        if f > T - 3:
            continue
        cut = eng.kws_mel_db(x[:, :200 * (f + 2)].contiguous())
        assert cut.shape[2] == f + 3 and torch.equal(cut[:, :, f], db7[:, :, f]), f
        assert torch.equal(cut[:, :, :f + 1], db7[:, :, :f + 1]), f


# ---- 4. the fused route -----------------------------------------------------------------------------------------------------------------
def wave_reference(L):
    """float64: module on the walk's dB, and back through the walk -> (logp [3,4], g_x [3,L], allowance of the gradient, of logp)"""
    x, _ = mc.rows(L)
    g = torch.randn(3, 4, generator=torch.Generator().manual_seed(L))
    out = {}
    for dtype in (torch.float64, torch.float32):
        db = mc.mel_walk(x, dtype=dtype)['db'].clone().requires_grad_(True)
        lp = module(dtype)(db[:, None], torch.zeros(4, 3, 64, dtype=dtype))
        (lp * g.to(dtype)).sum().backward()
        out[dtype] = lp.detach().double(), mc.mel_walk(x, db.grad, dtype=dtype)['g_x'].double()
    (lp64, gx64), (lp32, gx32) = out[torch.float64], out[torch.float32]
    gmax = gx64.abs().max().item()
    allow_g = FACTOR * max((gx32 - gx64).abs().max().item() / gmax, ULP)
    allow_lp = FACTOR * max((lp32 - lp64).abs().max().item(), ULP * lp64.abs().max().item())
    return x, g, lp64, gx64, allow_g, allow_lp


@pytest.mark.parametrize('L', FUSED)
def test_fused_route(eng, L):
    from dmad_hip import engine as E
    x, g, lp64, gx64, allow_g, allow_lp = wave_reference(L)
    xc, gc = x.cuda(), g.cuda()
    db = eng.kws_mel_db(xc)
    lp, dec = eng.kws_wave_logits(xc, want_decisions=True)
    assert torch.equal(lp, eng.kws_logits(db)) and dec.tolist() == lp.argmax(1).tolist()
    gx = torch.full_like(xc, float('nan'))
    lp2 = torch.full((3, 4), float('nan'), device='cuda')
    E.check(eng.lib.dmad_kws_wave_vjp(eng._h, E._ptr(xc), 3, L, E._ptr(gc), E._ptr(gx), E._ptr(lp2), E._stream()))
    assert not torch.isnan(gx).any()
    assert torch.equal(gx, eng.kws_mel_db_vjp(xc, eng.kws_vjp(db, gc)))               # the two-call route on all frames: the same bits
    assert torch.equal(lp2, lp) and torch.equal(eng.kws_wave_vjp(xc, gc), gx)
    gmax = gx64.abs().max().item()
    err_g, err_lp = (gx.cpu().double() - gx64).abs().max().item() / gmax, (lp.cpu().double() - lp64).abs().max().item()
    print('L = %d: logp |err| %.3e of allowed %.3e; waveform gradient %.3e of allowed %.3e of its maximum %.3g'
          % (L, err_lp, allow_lp, err_g, allow_g, gmax))
    assert err_g <= allow_g and err_lp <= allow_lp
    # rows in passes of 512 and alone: the same bits
    many = xc[:2].repeat(257, 1)
    lpm = eng.kws_wave_logits(many)
    assert torch.equal(lpm[512], lp[0]) and torch.equal(lpm[513], lp[1]) and torch.equal(lpm[1], lp[1])
    gm = eng.kws_wave_vjp(many, gc[:2].repeat(257, 1))
    assert torch.equal(gm[512], gx[0]) and torch.equal(gm[513], gx[1]) and torch.equal(gm[1], gx[1])


# ---- 5. under AcousticSystem ------------------------------------------------------------------------------------------------------------
def recorded(monkeypatch, e, names):
    calls = []
    for n in names:
        real = getattr(e, n)
        monkeypatch.setattr(e, n, (lambda real, n: lambda *a, **k: calls.append(n) or real(*a, **k))(real, n))
    return calls


def test_acoustic_system_fused_route(eng, monkeypatch):
    from acoustic_system import AcousticSystem
    from dmad_hip import engine as E
    from dmad_hip.transforms import KWSMelSpectrogramDB
    from shims.torchaudio import transforms as T
    L = 1237
    x, g, lp64, gx64, allow_g, allow_lp = wave_reference(L)
    net = module().cuda().use_engine(eng)
    front = KWSMelSpectrogramDB(eng, grad_backend='hip')
    system = AcousticSystem(classifier=net, transform=front, defender=None)
    expect = eng.kws_wave_logits(x.cuda())
    calls = recorded(monkeypatch, eng, ('kws_wave_logits', 'kws_wave_vjp', 'kws_logits', 'kws_vjp', 'kws_mel_db', 'kws_mel_db_vjp', 'kws_mel_power'))
    with torch.no_grad():
        out = system(x.cuda()[:, None])
    assert calls == ['kws_wave_logits'] and torch.equal(out, expect)                  # one call
    monkeypatch.setattr(E, 'get_engine', lambda *a, **k: eng)
    for pair in (torch.nn.Sequential(T.MelSpectrogram(sample_rate=16000, n_mels=32), T.AmplitudeToDB()),
                 types_compose([T.MelSpectrogram(sample_rate=16000, n_mels=32), T.AmplitudeToDB()])):
        del calls[:]
        with torch.no_grad():
            assert torch.equal(AcousticSystem(net, pair, None)(x.cuda()[:, None]), expect) and calls == ['kws_wave_logits']
    grads = {}
    for backend in ('hip', 'torch'):
        net.grad_backend = front.grad_backend = backend
        del calls[:]
        w = x.cuda()[:, None].requires_grad_(True)
        (system(w) * g.cuda()).sum().backward()
        assert calls == (['kws_wave_logits', 'kws_wave_vjp'] if backend == 'hip' else []), backend
        assert tuple(w.grad.shape) == (3, 1, L)
        grads[backend] = w.grad[:, 0].cpu().double()
    gmax = gx64.abs().max().item()
    err_hip, err_pair = (grads['hip'] - gx64).abs().max().item() / gmax, (grads['hip'] - grads['torch']).abs().max().item() / gmax
    print('waveform gradient under AcousticSystem: hip vs float64 %.3e, hip vs torch %.3e, allowed %.3e of its maximum' % (err_hip, err_pair, allow_g))
    assert err_hip <= allow_g and err_pair <= allow_g
    net.grad_backend = front.grad_backend = 'hip'
    # query(): no defender -> one call on the repeated rows, at any length
    del calls[:]
    logits, dec = system.query(x.cuda()[:, None], 2)
    assert calls == ['kws_wave_logits'] and tuple(logits.shape) == (2, 3, 4) and dec.dtype == torch.int64
    assert torch.equal(logits.reshape(6, 4), system(x.cuda()[:, None].repeat(2, 1, 1))) and torch.equal(dec, logits.argmax(-1))


def types_compose(ts):
    import adaptive_attack_eval as white_box
    c = white_box._Compose(ts)
    c.transforms = ts                                                                 # torchvision's Compose keeps its stages there
    return c


def test_acoustic_system_query_with_a_defense(eng, monkeypatch):
    from acoustic_system import AcousticSystem
    from dmad_hip.transforms import KWSMelSpectrogramDB
    from transforms.time_defense import TimeDomainDefense
    net = module().cuda().use_engine(eng)
    system = AcousticSystem(net, KWSMelSpectrogramDB(eng), TimeDomainDefense('AS', backend='hip', engine=eng))
    x = mc.rows(16000)[0][:2].cuda()[:, None]
    with torch.no_grad():
        expect = system(x.repeat(2, 1, 1))                                            # defense -> one fused call, row by row
    calls = recorded(monkeypatch, eng, ('kws_defense_query_logits', 'kws_query_logits', 'kws_wave_logits'))
    fallback = []
    monkeypatch.setattr(system, 'forward', lambda x, defend=True: fallback.append(tuple(x.shape)) or torch.zeros(x.shape[0], 4, device=x.device))
    logits, dec = system.query(x, 2)
    assert calls == ['kws_defense_query_logits'] and fallback == []                   # sampler 4: one call, no fallback to forward
    assert tuple(logits.shape) == (2, 2, 4) and torch.equal(dec, logits.argmax(-1))
    print('defense query vs forward: max |diff| %.3e' % (logits.reshape(4, 4) - expect).abs().max().item())
    assert torch.equal(logits.reshape(4, 4), expect)
    del calls[:]
    logits, _ = system.query(x[:, :, :8000].contiguous(), 2)                          # L != eng.L: the forward loop
    assert calls == [] and fallback == [(4, 1, 8000)] and tuple(logits.shape) == (2, 2, 4)


# ---- 6. refusals: host-side checks ------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    from dmad_hip._lib import DmadError
    from dmad_hip.autograd import kws_mel_db_hip, kws_wave_hip
    g4 = torch.zeros(2, 4).cuda()
    short = torch.zeros(2, 200).cuda()
    for call in (lambda: eng.kws_mel_db(short), lambda: eng.kws_mel_power(short), lambda: eng.kws_mel_db_vjp(short, torch.zeros(2, 32, 2).cuda())):
        with pytest.raises(DmadError, match=r'\(-4\).*L = 200'):                      # DMAD_ERR_SHAPE, names L
            call()
    assert tuple(eng.kws_mel_db(torch.zeros(2, 201).cuda()).shape) == (2, 32, 2)
    for L in (799, 128800):
        x = torch.zeros(2, L).cuda()
        for call in (lambda: eng.kws_wave_logits(x), lambda: eng.kws_wave_vjp(x, g4)):
            with pytest.raises(DmadError, match=r'\(-4\).*L = %d' % L):
                call()
    empty = new_engine()
    try:
        x = mc.rows(1237)[0].cuda()
        assert empty.device_bytes() < eng.device_bytes()
        before = empty.device_bytes()
        assert torch.equal(empty.kws_mel_db(x), eng.kws_mel_db(x))                    # the front-end needs no weights, on any engine
        assert empty.device_bytes() - before >= 4 * (400 * 402 * 2 + 32 * 201)        # ... and its constants are counted
        for call in (lambda: empty.kws_wave_logits(x), lambda: empty.kws_wave_vjp(x, torch.zeros(3, 4).cuda()),
                     lambda: empty.kws_query_logits(torch.zeros(1, 16000).cuda(), 2)):
            with pytest.raises(DmadError, match=r'\(-2\).*KWS weights are not finalised'):        # DMAD_ERR_STATE
                call()
    finally:
        empty.close()
    xr = mc.rows(1237)[0].cuda()[:, None].requires_grad_(True)
    for fn in (kws_mel_db_hip, kws_wave_hip):
        with pytest.raises(DmadError, match='first-order only'):
            torch.autograd.grad(fn(eng, xr).sum(), xr, create_graph=True)


# ---- 7. the driver ----------------------------------------------------------------------------------------------------------------------
def read_wav(path):
    with wave.open(path, 'rb') as w:
        return np.frombuffer(w.readframes(w.getnframes()), dtype='<i2').astype(np.float64) / 32767.0


def test_driver_cw_at_native_length(eng, tmp_path, monkeypatch):
    import kws_adaptive_attack_eval as drv
    root = mc.make_tree(str(tmp_path / 'data'), per_class=2)
    save = str(tmp_path / 'out')
    args = drv.build_parser().parse_args(['--data_path', root, '--attack', 'CW', '--defense', 'None', '--max_iter_1', '2', '--verbose', '0',
                                          '--save_path', save])
    calls = recorded(monkeypatch, eng, ('kws_wave_vjp', 'kws_wave_logits', 'kws_vjp', 'kws_mel_db_vjp'))
    lines = []
    out = drv.run(args, classifier=module(), engine=eng, log=lines.append)
    assert out['total'] == 8 and set(out) == {'total', 'clean_acc', 'denoised_acc', 'robust_acc'}
    assert out['clean_acc'] == out['denoised_acc'] and 0.0 <= out['robust_acc'] <= out['clean_acc'] <= 100.0
    assert calls.count('kws_wave_vjp') == 8 * 2 and 'kws_vjp' not in calls and 'kws_mel_db_vjp' not in calls
    assert any('CW robust test accuracy' in l for l in lines)
    lengths, moved = set(), 0
    for name in sorted(os.listdir(os.path.join(save, 'adv'))):
        if not name.endswith('_adv.wav'):
            continue
        adv = read_wav(os.path.join(save, 'adv', name))
        clean = read_wav(os.path.join(save, 'clean', name.replace('_adv.wav', '_clean.wav')))
        lengths.add(len(adv))
        assert len(adv) == len(clean) and np.abs(adv - clean).max() <= (args.eps + 2.0) / 32768.0, name       # eps, and a unit of each file's rounding
        moved += np.abs(adv - clean).max() > 0
    assert moved >= 4 and len(lengths) > 1 and all(1600 <= n <= 2400 for n in lengths)              # every clip at its own length


def test_driver_fakebob_against_a_defense(eng, tmp_path, monkeypatch):
    import kws_adaptive_attack_eval as drv
    root = mc.make_tree(str(tmp_path / 'data'), per_class=2)
    args = drv.build_parser().parse_args(['--data_path', root, '--clip_len', '16000', '--defense', 'AS', '--attack', 'FAKEBOB', '--verbose', '0',
                                          '--batch_size', '4'])
    calls = recorded(monkeypatch, eng, ('kws_defense_query_logits', 'kws_wave_logits'))
    out = drv.run(args, classifier=module(), engine=eng, log=lambda *a: None, max_iter=2, samples_per_draw=4)
    assert out['total'] == 8 and 0.0 <= out['robust_acc'] <= 100.0
    assert 'kws_defense_query_logits' in calls                                        # the probes went through the one-call query
