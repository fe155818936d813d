"""The attention-CRNN keyword spotter on the engine (csrc/kws.hip, dmad_kws_*) against the float64 walk of tests/kws_cases.py, which
tests/test_kws_cpu.py proves against the fixture recorded from the reference: the tape stage by stage, the forward and the input VJP on
the six recorded row lengths and at the cap, the exact zeros of the gradient, the bit-reproducibility rules, the module under
AcousticSystem, and the refusals.

Tolerance.  The yardstick is the reference module in fp32 on the CPU against its own float64 run on the same inputs, recorded per case in
the fixture (err_logp_<T>: absolute on logp; err_g_<T>: of the gradient's maximum).  The engine is allowed FACTOR = 4 x that: the same
precision with another summation order and the device's expf / tanhf.  A dropped bias, a swapped gate or a reversed direction lands
three orders of magnitude outside it.  Where no recorded value exists (the case at the cap, the stages, the waveform gradient) the same
yardstick is computed in the test: the fp32 CPU run of the same computation against float64, and never less than one ulp (2^-23) of the
quantity's largest value, below which no fp32 result can be asked to be.  The engine's measured errors are in DESIGN section 22."""
import functools

import pytest
import torch

import kws_cases as kc

pytestmark = pytest.mark.gpu

FACTOR = 4.0
ULP = 2.0 ** -23
CAP = 644
STAGES = ('x0', 'h0', 'h1', 'e')


def new_engine(sd=None):
    from dmad_hip import engine as E
    e = E.Engine(max_batch=8, precision=E.FP32, with_wavenet=False, with_classifier=False)
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


@functools.lru_cache(maxsize=None)
def case(T):
    """(spec [3,1,32,T], g [3,4], the float64 walk, the allowance on logp (absolute) and on the gradient (of its maximum)); computed once"""
    fx = kc.fixture()
    if T in kc.CASES:
        spec, g = torch.from_numpy(fx['spec_%d' % T].copy()), torch.from_numpy(fx['g_%d' % T].copy())
        ref = kc.kws_walk(kc.state_dict(), spec, g)
        return spec, g, ref, FACTOR * float(fx['err_logp_%d' % T]), FACTOR * float(fx['err_g_%d' % T])
    gen = torch.Generator().manual_seed(1000 + T)             # the cap: the recorder's input family, and the yardstick computed here
    spec, g = torch.randn(3, 1, 32, T, generator=gen) * 15 - 30, torch.randn(3, 4, generator=gen)
    ref = kc.kws_walk(kc.state_dict(), spec, g)
    x = spec.clone().requires_grad_(True)
    lp32 = module()(x)
    (lp32 * g).sum().backward()
    gmax = ref['g_spec'].abs().max().item()
    err_lp = max((lp32.detach().double() - ref['logp']).abs().max().item(), ULP * ref['logp'].abs().max().item())
    err_g = max((x.grad[:, 0].double() - ref['g_spec']).abs().max().item() / gmax, ULP)
    return spec, g, ref, FACTOR * err_lp, FACTOR * err_g


def raw_vjp(e, spec, g, want_logits=True):
    """dmad_kws_vjp into buffers this test pre-fills with NaN: (g_spec [B,32,T], logp [B,4])"""
    from dmad_hip import engine as E
    xs = spec.cuda().float().reshape(spec.shape[0], 32, -1).contiguous()
    gl = g.cuda().float().contiguous()
    gs = torch.full_like(xs, float('nan'))
    lp = torch.full((xs.shape[0], 4), float('nan'), device='cuda')
    E.check(e.lib.dmad_kws_vjp(e._h, E._ptr(xs), xs.shape[0], xs.shape[2], E._ptr(gl), E._ptr(gs), E._ptr(lp) if want_logits else None,
                               E._stream()))
    return gs, lp


# ---- 1. the tape, stage by stage --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', (21, 81))
def test_stages(eng, T):
    spec, _, ref, _, _ = case(T)
    own = kc.kws_walk(kc.state_dict(), spec, dtype=torch.float32)          # the walk's own fp32 error: the scale of each stage's allowance
    S = kc.steps(T)
    for i, name in enumerate(STAGES):
        got = eng.kws_tape(spec.cuda(), i).cpu().double()
        assert tuple(got.shape) == ((3, S, 64), (3, S, 128), (3, S, 128), (3, S))[i], name
        top = ref[name].abs().max().item()
        allow = FACTOR * max((own[name].double() - ref[name]).abs().max().item(), ULP * top)
        err = (got - ref[name]).abs().max().item()
        print('T = %d stage %d (%s): |err| %.3e of allowed %.3e (largest value %.3g)' % (T, i, name, err, allow, top))
        assert err <= allow, 'stage %d (%s)' % (i, name)


# ---- 2. forward and VJP against float64, the exact zeros --------------------------------------------------------------------------------
@pytest.mark.parametrize('T', kc.CASES + (CAP,))
def test_forward_and_vjp_vs_float64(eng, T):
    spec, g, ref, allow_lp, allow_g = case(T)
    logp, dec = eng.kws_logits(spec.cuda(), want_decisions=True)
    assert tuple(logp.shape) == (3, 4) and dec.dtype == torch.int32
    err_lp = (logp.cpu().double() - ref['logp']).abs().max().item()
    gs, lp2 = raw_vjp(eng, spec, g)
    gmax = ref['g_spec'].abs().max().item()
    err_g = (gs.cpu().double() - ref['g_spec']).abs().max().item() / gmax
    print('T = %d: logp |err| %.3e of allowed %.3e; gradient %.3e of allowed %.3e of its maximum %.3g'
          % (T, err_lp, allow_lp, err_g, allow_g, gmax))
    assert err_lp <= allow_lp
    assert err_g <= allow_g
    assert dec.cpu().tolist() == logp.argmax(1).cpu().tolist() == ref['logp'].argmax(1).tolist()
    assert torch.equal(lp2, logp)                                         # the VJP launch's own log-probabilities: the same bits
    # every element was written over the NaN, and outside frames 16 j .. 16 j + 4 with an exact +0.0
    m = torch.from_numpy(kc.support(T))
    out = gs.cpu()[:, :, ~m]
    assert not torch.isnan(gs).any()
    assert (out == 0).all() and not torch.signbit(out).any()
    assert (gs.cpu()[:, :, m].abs().amax(dim=(0, 1)) > 0).all()
    assert torch.equal(eng.kws_vjp(spec.cuda(), g.cuda()), gs)           # the wrapper, [B,1,32,T] in


# ---- 3. bits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', (37, 81))
def test_bits(eng, T):
    gen = torch.Generator().manual_seed(7 + T)
    spec = (torch.randn(7, 32, T, generator=gen) * 15 - 30).cuda()
    g = torch.randn(7, 4, generator=gen).cuda()
    lp7 = eng.kws_logits(spec)
    gs7, lpv7 = eng.kws_vjp(spec, g, want_logits=True)
    lp1 = eng.kws_logits(spec[5:6].clone())
    gs1, lpv1 = eng.kws_vjp(spec[5:6].clone(), g[5:6].clone(), want_logits=True)
    assert torch.equal(lp1[0], lp7[5]) and torch.equal(gs1[0], gs7[5])                # alone, and as row 5 of 7
    assert torch.equal(lpv1, lp1) and torch.equal(lpv7, lp7)                          # the VJP's log-probabilities are the forward's
    assert torch.equal(eng.kws_logits(spec), lp7) and torch.equal(eng.kws_vjp(spec, g), gs7)        # and in a second call
    assert not torch.equal(lp7[5], lp7[4])


# ---- 4. the public surface --------------------------------------------------------------------------------------------------------------
def frames(x):
    """a plain torch front-end: waveform [B,1,1312] -> [B,1,32,81], overlapping 32-sample frames scaled to a dB-like range"""
    return x.unfold(-1, 32, 16).transpose(2, 3) * 75 - 30


def test_module_under_acoustic_system(eng, monkeypatch):
    from acoustic_system import AcousticSystem
    net = module().cuda().use_engine(eng)
    assert net.engine is eng and 'engine' not in net.state_dict()
    system = AcousticSystem(classifier=net, transform=frames, defender=None)
    gen = torch.Generator().manual_seed(5)
    wave = torch.randn(3, 1, 1312, generator=gen) * 0.2             # below the int16 rescale of AcousticSystem
    g = torch.randn(3, 4, generator=gen)
    # float64 on the CPU, and the fp32 module's own error there: the yardstick
    w64 = wave.double().requires_grad_(True)
    lp64 = module(torch.float64)(frames(w64), torch.zeros(4, 3, 64, dtype=torch.float64))
    (lp64 * g.double()).sum().backward()
    w32 = wave.clone().requires_grad_(True)
    (module()(frames(w32)) * g).sum().backward()
    gmax = w64.grad.abs().max().item()
    allow = FACTOR * max((w32.grad.double() - w64.grad).abs().max().item() / gmax, ULP)
    calls = []
    real_logits, real_vjp = eng.kws_logits, eng.kws_vjp
    monkeypatch.setattr(eng, 'kws_logits', lambda *a, **k: calls.append('logits') or real_logits(*a, **k))
    monkeypatch.setattr(eng, 'kws_vjp', lambda *a, **k: calls.append('vjp') or real_vjp(*a, **k))
    with torch.no_grad():
        out = system(wave.cuda())
    assert calls == ['logits'] and tuple(out.shape) == (3, 4) and torch.equal(out, real_logits(frames(wave.cuda())))
    assert tuple(system(wave[:1].cuda()).shape) == (1, 4)
    grads = {}
    for backend in ('hip', 'torch', 'auto'):
        net.grad_backend = backend
        del calls[:]
        w = wave.cuda().requires_grad_(True)
        loss = (system(w) * g.cuda()).sum()
        loss.backward()
        assert calls == (['logits', 'vjp'] if backend == 'hip' else []), backend
        assert w.grad is not None and tuple(w.grad.shape) == (3, 1, 1312)
        grads[backend] = w.grad.cpu().double()
    err_hip = (grads['hip'] - w64.grad).abs().max().item() / gmax
    err_pair = (grads['hip'] - grads['torch']).abs().max().item() / gmax
    print('waveform gradient: hip vs float64 %.3e, hip vs torch %.3e, allowed %.3e of its maximum %.3g' % (err_hip, err_pair, allow, gmax))
    assert err_hip <= allow and err_pair <= allow
    # a caller's hidden state, and training mode, take the module's torch layers
    net.grad_backend = 'hip'
    del calls[:]
    with torch.no_grad():
        again = net(frames(wave.cuda()), torch.zeros(4, 3, 64).cuda())
        net.train()
        trained = net(frames(wave.cuda()))
        net.eval()
    assert calls == [] and (again - out).abs().max().item() < 1e-4 and (trained - out).abs().max().item() < 1e-4
    from dmad_hip._lib import DmadError
    from dmad_hip.autograd import kws_hip
    xr = frames(wave.cuda()).requires_grad_(True)
    with pytest.raises(DmadError, match='first-order only'):
        torch.autograd.grad(kws_hip(eng, xr).sum(), xr, create_graph=True)


# ---- 5. refusals: host-side checks, no launch --------------------------------------------------------------------------------------------
def test_refusals(eng):
    from dmad_hip._lib import DmadError
    sd = kc.state_dict()
    g = torch.zeros(2, 4).cuda()
    for T in (4, CAP + 1):
        x = torch.zeros(2, 32, T).cuda()
        for call in (lambda: eng.kws_logits(x), lambda: eng.kws_vjp(x, g), lambda: eng.kws_tape(x, 0)):
            with pytest.raises(DmadError, match=r'\(-4\).*T is'):                         # DMAD_ERR_SHAPE, names the field
                call()
    x = torch.zeros(2, 32, 81).cuda()
    with pytest.raises(DmadError, match='stage'):
        eng.kws_tape(x, 4)
    empty = new_engine()
    try:
        for call in (lambda: empty.kws_logits(x), lambda: empty.kws_vjp(x, g), lambda: empty.kws_tape(x, 0)):
            with pytest.raises(DmadError, match=r'\(-2\).*KWS weights are not finalised'):        # DMAD_ERR_STATE
                call()
        # wrong geometry: DMAD_ERR_SHAPE, the message names the field; a refused set leaves nothing behind
        from audio_models.RCNN_KWS.model import KWSModel
        for kw, field in ((dict(in_size=40), 'in_size'), (dict(in_size=32, hidden_size=32), 'hidden_size'),
                          (dict(in_size=32, num_classes=5), 'num_classes'), (dict(in_size=32, gru_num_layers=1), 'gru_num_layers')):
            with pytest.raises(DmadError, match=r'\(-4\).*' + field):
                empty.load_kws(KWSModel(**kw).state_dict())
            assert not empty.has_kws
        with pytest.raises(DmadError, match=r'\(-4\).*stride'):
            empty.load_kws(sd, stride=(8, 1))
        with pytest.raises(DmadError, match=r'\(-4\).*kernel_size'):
            empty.load_kws(sd, kernel_size=(40, 5))
        empty.load_kws(sd)
        x = torch.from_numpy(kc.fixture()['spec_21'].copy()).cuda()
        assert torch.equal(empty.kws_logits(x), eng.kws_logits(x))
    finally:
        empty.close()
    eng.bind('kws', sd, eng.load_kws)                                  # the same weights again: accepted; other ones: refused
    other = {k: v + 1 for k, v in sd.items()}
    with pytest.raises(DmadError, match='different kws weights'):
        eng.bind('kws', other, eng.load_kws)
