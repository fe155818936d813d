"""DenseNet-BC-100-12 on the engine (dmad_classify's fourth classifier, dmad_reserve_dn_vjp / dmad_dn_vjp): the kernels of csrc/densenet.hip
alone (small integers, bit for bit; random data against float64), forward bits, the whole VJP against a decision-pinned float64 walk
(tests/dn_cases.py) with tolerances taken from the same walk in float32 on the CPU, determinism and batch independence, a finite
difference, every engine precision with the reservation and the refusals, and the module, the query path and the five drivers built on it."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dn_cases as D  # noqa: E402
import vjp_reservation  # noqa: E402
from dmad_hip import synth  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'densenet_bc_100_12.npz')
EXACT_TIER = 1e-5            # the exact tier's bound of test_gpu_wrn.py's gemm_f32 cases, relative to the map's maximum
PITCH = {32: 216, 16: 304, 8: 344}
NAN = float('nan')


def _E():
    from dmad_hip import engine as E
    return E


@pytest.fixture(scope='module')
def sd():
    return synth.densenet_bc_100_12_state_dict(D.DN_SEED)


@pytest.fixture(scope='module')
def eng(sd):
    E = _E()
    e = E.Engine(max_batch=8, precision=E.FP32, with_wavenet=False)
    e.load_densenet_bc_100_12(sd)
    yield e
    e.close()


def clips(ids):
    return torch.from_numpy(np.stack([synth.synthetic_clip(i).reshape(-1) for i in ids])).float()


def cotangent(B, seed):
    return torch.randn(B, 10, generator=torch.Generator().manual_seed(seed))


def ints(gen, shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def pow2(gen, n):
    return torch.tensor([0.5, 1.0, 2.0, -1.0, -0.25, 4.0])[torch.randint(0, 6, (n,), generator=gen)]


def pre64(s, x, b):
    """the one pre-activation in float64: max(s x + b, 0), a NaN kept, -0.0 and negatives zeroed"""
    t = s.double() * x.double() + b.double()
    return torch.where(t > 0, t, torch.where(torch.isnan(t), t, torch.zeros((), dtype=torch.float64)))


def same(got, ref):
    return np.array_equal(got.double().numpy(), ref.double().numpy(), equal_nan=True)


# ---- 1. the kernels alone, exact ------------------------------------------------------------------------------------------------------
def test_preact_zeroes_negatives_and_keeps_nan():
    E = _E()
    x = torch.tensor([[-0.0, -1.5, 2.0, NAN, 0.0, 3.0, 77.0, NAN]])               # pitch 8, C = 6: the last two are never read
    one, zero = torch.ones(6), torch.zeros(6)
    got = E.dn_preact(x.cuda(), one.cuda(), zero.cuda()).cpu()
    assert tuple(got.shape) == (1, 6) and got[0, :3].tolist() == [0.0, 0.0, 2.0] and bool(torch.isnan(got[0, 3])) and got[0, 4:].tolist() == [0.0, 3.0]
    assert not bool(torch.signbit(got[0, 0])) and not bool(torch.signbit(got[0, 1]))     # -0.0 and negatives come out as +0.0


@pytest.mark.parametrize('epi', [False, True])
@pytest.mark.parametrize('cin,M', [(24, 48), (36, 48), (204, 48), (330, 48), (216, 108), (300, 150)])
@pytest.mark.parametrize('n_px', [64, 1000])
def test_pw_exact(n_px, cin, M, epi):
    """The bottleneck / transition 1x1 on small integers and power-of-two scales against float64: bit for bit.  The stream's channels
    behind cin hold NaN (330 -> K4 = 332 spans two of them): nothing behind the width may be read, zero weights would not save 0 x NaN.
    One input is NaN (its pixel's outputs must all be NaN), some are -0.0.  1000 pixels are no multiple of the 64-pixel tile; M = 150 ends
    in a partial 16-row tile."""
    E = _E()
    gen = torch.Generator().manual_seed(n_px + cin + M + epi)
    ld = cin + 10
    x = torch.full((n_px, ld), NAN)
    x[:, :cin] = ints(gen, (n_px, cin))
    x[::7, 3] = -0.0
    x[5, cin - 1] = NAN
    w, s_in, b_in = ints(gen, (M, cin), -2, 2), pow2(gen, cin), ints(gen, (cin,))
    s_out, b_out = (pow2(gen, M), ints(gen, (M,))) if epi else (None, None)
    got = E.dn_pw(x.cuda(), w.cuda(), s_in.cuda(), b_in.cuda(), None if s_out is None else s_out.cuda(), None if b_out is None else b_out.cuda()).cpu()
    o = pre64(s_in, x[:, :cin], b_in)
    ref = o @ w.double().t()
    if epi:
        ref = pre64(s_out, ref, b_out)
    assert tuple(got.shape) == (n_px, M) and same(got, ref)
    assert bool(torch.isnan(got[5]).all()) and int(torch.isnan(got).any(1).sum()) == 1
    assert 0.05 < float((o[:5] > 0).double().mean()) < 0.95


@pytest.mark.parametrize('last', [False, True])
@pytest.mark.parametrize('H', [8, 16, 32])
@pytest.mark.parametrize('B', [1, 3])
def test_growth_exact(B, H, last):
    """The 3x3 48 -> 12 conv into the first / last slice of a stream pre-filled with sentinels: the slice bit for bit, every other channel
    bit-unchanged.  dense3's first slice starts at channel 150, no multiple of 4."""
    E = _E()
    gen = torch.Generator().manual_seed(B * 100 + H + last)
    blk = {32: 0, 16: 1, 8: 2}[H]
    ld, off = PITCH[H], (D.BLOCKS[blk][2] - 12) if last else D.BLOCKS[blk][1]
    h, w = ints(gen, (B, H, H, 48)), ints(gen, (12, 48, 3, 3), -2, 2)
    stream = ints(gen, (B, H, H, ld), -9, 9)
    before = stream.clone()
    got = E.dn_growth(h.cuda(), w.cuda(), stream.cuda(), off).cpu()
    ref = F.conv2d(h.double().permute(0, 3, 1, 2), w.double(), None, 1, 1).permute(0, 2, 3, 1)
    assert same(got[..., off:off + 12], ref) and float(ref.abs().max()) > 0
    keep = torch.ones(ld, dtype=torch.bool)
    keep[off:off + 12] = False
    assert torch.equal(got[..., keep].view(torch.int32), before[..., keep].view(torch.int32))
    if B > 1:                                                         # the last spectrogram alone: the same bits
        alone = E.dn_growth(h[B - 1:].cuda(), w.cuda(), before[B - 1:].cuda(), off).cpu()
        assert torch.equal(alone, got[B - 1:])


@pytest.mark.parametrize('last', [False, True])
@pytest.mark.parametrize('H', [8, 16, 32])
@pytest.mark.parametrize('B', [1, 3])
def test_growth_bwd_exact(B, H, last):
    """The transposed 3x3 (12 -> 48, flipped taps) of a gradient stream's slice, masked by h (-0.0 and negatives give 0) and scaled by
    bn2.  Everything outside the slice is NaN: nothing else may be read."""
    E = _E()
    gen = torch.Generator().manual_seed(B * 100 + H + last + 7)
    blk = {32: 0, 16: 1, 8: 2}[H]
    ld, off = PITCH[H], (D.BLOCKS[blk][2] - 12) if last else D.BLOCKS[blk][1]
    g = torch.full((B, H, H, ld), NAN)
    g[..., off:off + 12] = ints(gen, (B, H, H, 12))
    h, w, s2 = ints(gen, (B, H, H, 48)), ints(gen, (12, 48, 3, 3), -2, 2), pow2(gen, 48)
    h.view(-1)[::5] = -0.0
    hh = h.double().permute(0, 3, 1, 2).requires_grad_(True)
    y = F.conv2d(hh, w.double(), None, 1, 1)
    (gh,) = torch.autograd.grad(y, hh, g[..., off:off + 12].double().permute(0, 3, 1, 2))
    ref = torch.where(h > 0, s2.double() * gh.permute(0, 2, 3, 1), torch.zeros((), dtype=torch.float64))
    got = E.dn_growth_bwd(g.cuda(), off, w.cuda(), h.cuda(), s2.cuda()).cpu()
    assert same(got, ref) and 0.05 < float((got != 0).double().mean()) < 0.95


@pytest.mark.parametrize('add', [True, False])
@pytest.mark.parametrize('n_px,M,K,pool_H', [(64, 24, 48, 0), (1000, 36, 48, 0), (1000, 330, 48, 0), (64, 204, 48, 0),
                                             (1024, 216, 108, 32), (512, 300, 150, 16)])
def test_pw_bwd_exact(n_px, M, K, pool_H, add):
    """The transposed 1x1 (K -> M), masked by the recomputed pre-activation decision and scaled by bn1, added into (or written to)
    channels [0, M) of the gradient stream: bit for bit, channels >= M bit-unchanged.  The transition's form reads the gradient of its
    2x2 average pool (a quarter of the pooled pixel's); K = 150 is padded to 152 in the staging.  Behind their widths g and x hold NaN."""
    E = _E()
    gen = torch.Generator().manual_seed(n_px + M + K + add)
    ld, ldg = M + 6, K + 2
    n_g = n_px // 4 if pool_H else n_px
    g = torch.full((n_g, ldg), NAN)
    g[:, :K] = ints(gen, (n_g, K))
    x = torch.full((n_px, ld), NAN)
    x[:, :M] = ints(gen, (n_px, M))
    w, s1, b1 = ints(gen, (K, M), -2, 2), pow2(gen, M), ints(gen, (M,))
    out = ints(gen, (n_px, ld), -9, 9)
    before = out.clone()
    got = E.dn_pw_bwd(g.cuda(), w.cuda(), x.cuda(), s1.cuda(), b1.cuda(), out.cuda(), add=add, pool_H=pool_H).cpu()
    gp = g[:, :K].double()
    if pool_H:
        Hh = pool_H // 2
        gp = 0.25 * gp.view(-1, Hh, Hh, K).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(n_px, K)
    v = torch.where(pre64(s1, x[:, :M], b1) > 0, s1.double() * (gp @ w.double()), torch.zeros((), dtype=torch.float64))
    ref = v + before[:, :M].double() if add else v
    assert same(got[:, :M], ref) and 0.05 < float((v != 0).double().mean()) < 0.95
    assert torch.equal(got[:, M:].view(torch.int32), before[:, M:].view(torch.int32))


def test_stem_pool_head_exact():
    E = _E()
    gen = torch.Generator().manual_seed(24)
    B = 2
    spec, w = ints(gen, (B, 32, 32)), ints(gen, (24, 9)) * 0.25
    stream = ints(gen, (B, 32, 32, 216), -9, 9)
    before = stream.clone()
    x = spec.double().unsqueeze(1).requires_grad_(True)
    y = F.conv2d(x, w.double().reshape(24, 1, 3, 3), None, 1, 1)
    got = E.dn_stem(spec.cuda(), w.cuda(), stream.cuda()).cpu()
    assert same(got[..., :24], y.detach().permute(0, 2, 3, 1)) and torch.equal(got[..., 24:], before[..., 24:])
    g = torch.full((B, 32, 32, 216), NAN)
    g[..., :24] = ints(gen, (B, 32, 32, 24))
    (gx,) = torch.autograd.grad(y, x, g[..., :24].double().permute(0, 3, 1, 2))
    back = E.dn_stem_bwd(g.cuda(), w.cuda()).cpu()
    assert same(back, gx[:, 0]) and float(back.abs().max()) > 0
    assert torch.equal(E.dn_stem_bwd(g[1:].cuda(), w.cuda()).cpu(), back[1:])
    # the 2x2 average pool of a transition's map (pitch 152, 150 channels) into a stream of pitch 344
    t = torch.full((B, 16, 16, 152), NAN)
    t[..., :150] = ints(gen, (B, 16, 16, 150))
    nxt = ints(gen, (B, 8, 8, 344), -9, 9)
    keep = nxt.clone()
    p = E.dn_pool(t.cuda(), 150, nxt.cuda()).cpu()
    assert same(p[..., :150], F.avg_pool2d(t[..., :150].double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)) and torch.equal(p[..., 150:], keep[..., 150:])
    # the head and its backward (342 channels at pitch 344)
    xs = torch.full((B, 64, 344), NAN)
    xs[..., :342] = ints(gen, (B, 64, 342))
    bns, bnb, fcw, fcb, gl = pow2(gen, 342), ints(gen, (342,)), ints(gen, (10, 342), -2, 2), ints(gen, (10,)), ints(gen, (B, 10))
    f = pre64(bns, xs[..., :342], bnb)
    lg = E.dn_head(xs.cuda(), bns.cuda(), bnb.cuda(), fcw.cuda(), fcb.cuda()).cpu()
    assert same(lg, f.mean(1) @ fcw.double().t() + fcb.double())
    hb = E.dn_head_bwd(gl.cuda(), fcw.cuda(), xs.cuda(), bns.cuda(), bnb.cuda(), 344).cpu()
    want = torch.where(f > 0, ((gl.double() @ fcw.double()) / 64)[:, None, :], torch.zeros((), dtype=torch.float64))
    assert same(hb[..., :342], want) and bool((hb[..., 342:] == 0).all())


# ---- 2. the same kernels on random fp32 data against float64 --------------------------------------------------------------------------
def test_kernels_random_vs_float64():
    E = _E()
    gen = torch.Generator().manual_seed(99)
    rnd = lambda *s: torch.rand(*s, generator=gen) * 2 - 1
    errs = {}
    for cin, M, epi in ((330, 48, True), (300, 150, False)):
        x, w, s_in, b_in, s_out, b_out = rnd(1000, cin + 2), rnd(M, cin) * 0.1, rnd(cin) + 1.5, rnd(cin), rnd(M) + 1.5, rnd(M)
        got = E.dn_pw(x.cuda(), w.cuda(), s_in.cuda(), b_in.cuda(), s_out.cuda() if epi else None, b_out.cuda() if epi else None).cpu()
        ref = pre64(s_in, x[:, :cin], b_in) @ w.double().t()
        errs['pw %d->%d' % (cin, M)] = D.relmax(got, pre64(s_out, ref, b_out) if epi else ref)
        g, out = rnd(1000, M), rnd(1000, cin + 2)
        v = torch.where(pre64(s_in, x[:, :cin], b_in) > 0, s_in.double() * (g.double() @ w.double()), torch.zeros((), dtype=torch.float64))
        want = out[:, :cin].double() + v
        back = E.dn_pw_bwd(g.cuda(), w.cuda(), x.cuda(), s_in.cuda(), b_in.cuda(), out.cuda()).cpu()
        errs['pw_bwd %d->%d' % (M, cin)] = D.relmax(back[:, :cin], want)
    B, H, off = 2, 16, 288
    h, w, s2 = rnd(B, H, H, 48), rnd(12, 48, 3, 3) * 0.1, rnd(48) + 1.5
    stream = rnd(B, H, H, 304)
    hh = h.double().permute(0, 3, 1, 2).requires_grad_(True)
    y = F.conv2d(hh, w.double(), None, 1, 1)
    got = E.dn_growth(h.cuda(), w.cuda(), stream.cuda(), off).cpu()
    errs['growth'] = D.relmax(got[..., off:off + 12], y.detach().permute(0, 2, 3, 1))
    (gh,) = torch.autograd.grad(y, hh, stream[..., off:off + 12].double().permute(0, 3, 1, 2))
    back = E.dn_growth_bwd(stream.cuda(), off, w.cuda(), h.cuda(), s2.cuda()).cpu()
    errs['growth_bwd'] = D.relmax(back, torch.where(h > 0, s2.double() * gh.permute(0, 2, 3, 1), torch.zeros((), dtype=torch.float64)))
    print('kernels vs float64, relmax: ' + ', '.join('%s %.2e' % kv for kv in errs.items()))
    assert all(e <= EXACT_TIER for e in errs.values()), errs


# ---- 3. forward bits ------------------------------------------------------------------------------------------------------------------
def test_forward_bits(eng):
    x = D.specs(5, 2).cuda()
    eng.reserve_dn_vjp(5)
    _, lg = eng.dn_vjp(x, cotangent(5, 2).cuda(), want_logits=True)
    tier0 = eng.classify_tier(x, 0)
    assert torch.equal(lg, tier0) and torch.equal(eng.classify(x), tier0)
    assert torch.equal(eng.classify_tier(x, 1), tier0) and torch.equal(eng.classify_tier(x, 2), tier0)      # every tier falls to fp32
    for j in (0, 4):
        assert torch.equal(eng.classify(x[j:j + 1]), tier0[j:j + 1]), j
    big = D.specs(11, 7).cuda()                            # more than max_batch = 8: chunked, the same bits
    whole = eng.classify(big)
    assert torch.equal(whole[8:], eng.classify(big[8:])) and torch.equal(whole[3:4], eng.classify(big[3:4]))
    with np.load(GOLDEN) as z:
        spec, ref = torch.from_numpy(z['spec_in']), z['logits']
    err = D.relmax(eng.classify(spec.cuda()).cpu().numpy(), ref)
    print('engine logits vs the reference fixture: relmax %.3e' % err)
    assert err < 2e-4, err


# ---- 4. the whole VJP, decisions pinned -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,seed', [(2, 1), (3, 12)])
def test_dn_vjp_against_pinned_float64(eng, sd, B, seed):
    """The engine's 99 post-ReLU maps and its gradient against the float64 walk pinned to the ENGINE's decisions.  The tolerances come from
    the reference computation, not the engine: the same pinned walk in float32 on the CPU has the error e32 against float64 (per map as a
    share of the map's maximum; for the gradient as a share of max |g|), and the engine — another legitimate fp32 summation order — must
    stay within 4 x e32.  A decision that differs from the free float64 walk must sit at a unit whose |pre-activation| is within 4 x its
    map's e32.  The figures of one MI355X run are in DESIGN §24."""
    x, g = D.specs(B, seed), cotangent(B, seed)
    eng.reserve_dn_vjp(B)
    gx, lg = eng.dn_vjp(x.cuda(), g.cuda(), want_logits=True)
    tape = [eng.dn_vjp_tape(j, B).permute(0, 3, 1, 2).cpu() for j in range(D.N_MAPS)]
    masks = [t > 0 for t in tape]
    D.mask_conditions(masks)                             # non-vacuity, on the engine's own decisions
    net64, net32 = D.sd64(sd), D.sd32(sd)
    with torch.no_grad():
        _, free = D.dn_walk(net64, x.double())
    g64, pin64 = D.pinned_vjp(net64, x, g, masks)
    g32, pin32 = D.pinned_vjp(net32, x, g, masks)
    worst, differing = (0.0, 0.0, -1), 0
    failures = []
    for j in range(D.N_MAPS):
        ref = pin64['maps'][j].detach()
        assert tape[j].shape == ref.shape, j
        top = float(ref.abs().max())
        e32 = float((pin32['maps'][j].detach().double() - ref).abs().max()) / top
        err = float((tape[j].double() - ref).abs().max()) / top
        if err > worst[0]:
            worst = (err, e32, j)
        if err > 4 * e32:
            failures.append((j, err, e32))
        d = masks[j] != free['masks'][j]
        differing += int(d.sum())
        ftop = float(free['maps'][j].abs().max())
        assert bool((free['pre'][j].abs()[d] <= 4 * e32 * ftop).all()), (j, float(free['pre'][j].abs()[d].max()) / ftop, e32)
    e32_g, err_g = D.relmax(g32, g64), D.relmax(gx.cpu(), g64)
    e32_l, err_l = D.relmax(pin32_logits(net32, x, masks), pin64_logits(net64, x, masks)), D.relmax(lg.cpu(), pin64_logits(net64, x, masks))
    print('dn_vjp B=%d seed=%d: worst tape map %d error %.3e (e32 %.3e); gradient error %.3e (e32 %.3e); logits error %.3e (e32 %.3e); '
          '%d decisions differ from the free float64 walk' % (B, seed, worst[2], worst[0], worst[1], err_g, e32_g, err_l, e32_l, differing))
    assert not failures, failures[:5]
    assert err_g <= 4 * e32_g, (err_g, e32_g)


def pin64_logits(net, x, masks):
    with torch.no_grad():
        return D.dn_walk(net, x.double(), masks)[0]


def pin32_logits(net, x, masks):
    with torch.no_grad():
        return D.dn_walk(net, x.float(), masks)[0]


# ---- 5. determinism, batch independence, passes ---------------------------------------------------------------------------------------
def test_determinism_batch_independence_and_passes(eng, sd):
    E = _E()
    x, g = D.specs(7, 3).cuda(), cotangent(7, 3).cuda()
    eng.reserve_dn_vjp(7)
    a, b = eng.dn_vjp(x, g), eng.dn_vjp(x, g)
    assert torch.equal(a, b)
    for j in (0, 4, 6):
        assert torch.equal(eng.dn_vjp(x[j:j + 1], g[j:j + 1]), a[j:j + 1]), j
    with pytest.raises(E.DmadError, match='one-pass'):
        eng.dn_vjp_tape(0, 2)                            # the last call held one row
    big, gb = D.specs(11, 7).cuda(), cotangent(11, 7).cuda()              # B = 11 on max_batch 8: chunked, the same bits
    whole = eng.dn_vjp(big, gb)
    assert torch.equal(whole[8:], eng.dn_vjp(big[8:], gb[8:])) and torch.equal(whole[3:4], eng.dn_vjp(big[3:4], gb[3:4]))
    small = E.Engine(max_batch=8, precision=E.FP32, with_wavenet=False)      # a reservation cannot shrink: its own engine
    try:
        small.load_densenet_bc_100_12(sd)
        small.reserve_dn_vjp(2)
        got, lg = small.dn_vjp(x[:5], g[:5], want_logits=True)                 # three passes, the last partial
        assert small.dn_vjp_batch == 2
        with pytest.raises(E.DmadError, match='one-pass'):
            small.dn_vjp_tape(0, 1)                      # more than one pass: no tape to read
        small.reserve_dn_vjp(5)
        whole, lg5 = small.dn_vjp(x[:5], g[:5], want_logits=True)
        assert torch.equal(got, whole) and torch.equal(lg, lg5)
        assert torch.equal(whole, a[:5])                 # ... and the same bits as under the other engine's reservation of 7
    finally:
        small.close()


# ---- 6. finite difference -------------------------------------------------------------------------------------------------------------
def test_finite_difference(eng, sd):
    """sum g (f(x + h d) - f(x - h d)) / 2h on the engine's own tier-0 forward against sum g_spec d, with the step, the tolerance and the
    directions of test_gpu_wrn.py::test_finite_difference (h = 1e-3, 2 %; the sign of the free float64 gradient and the sign of the
    engine's own)."""
    x, g = D.specs(2, 6), cotangent(2, 6)
    xr = x.double().requires_grad_(True)
    (g64,) = torch.autograd.grad((D.dn_walk(D.sd64(sd), xr)[0] * g.double()).sum(), xr)
    x, g = x.cuda(), g.cuda()
    gx = eng.dn_vjp(x, g).view(2, 1, 32, 32)
    own = torch.sign(gx)
    own[own == 0] = 1.0
    h = 1e-3
    for name, d in (('float64 sign', torch.sign(g64).float().cuda()), ('engine sign', own)):
        fd = ((eng.classify_tier(x + h * d, 0) - eng.classify_tier(x - h * d, 0)) * g).sum() / (2 * h)
        an = (gx * d).sum()
        print('finite difference along the %s: %.6e against %.6e' % (name, float(fd), float(an)))
        assert abs(float(fd) - float(an)) <= 2e-2 * abs(float(an)), (name, float(fd), float(an))


# ---- 7. every precision, reservations, refusals ---------------------------------------------------------------------------------------
_BITS = {}


@pytest.mark.parametrize('prec', ['FP32', 'EXACT', 'BF16'])
def test_every_precision_and_refusals(sd, prec):
    E = _E()
    kw = {'recheck_batch': 4} if prec == 'EXACT' else {}
    e = E.Engine(max_batch=4, precision=getattr(E, prec), with_wavenet=False, **kw)
    try:
        with pytest.raises(E.DmadError):
            e.reserve_dn_vjp(2)                          # no classifier loaded yet
        e.load_densenet_bc_100_12(sd)
        assert e.has_classifier and e.classifier_kind == 'densenet_bc_100_12'
        e.dn_vjp_batch = 1                               # past the host's on-demand reservation: the library's own refusal
        with pytest.raises(E.DmadError, match='dmad_reserve_dn_vjp'):
            e.dn_vjp(D.specs(1, 0).cuda(), cotangent(1, 0).cuda())
        e.dn_vjp_batch = 0
        vjp_reservation.check(e, e.reserve_dn_vjp, vjp_reservation.grow(e, e.reserve_dn_vjp, (1, 2, 3), []))
        e.reserve_dn_vjp(9)                              # capped at max_batch
        x, g = D.specs(3, 11).cuda(), cotangent(3, 11).cuda()
        gx, lg = e.dn_vjp(x, g, want_logits=True)
        assert torch.equal(lg, e.classify_tier(x, 0)) and torch.equal(lg, e.classify(x))
        assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
        first = _BITS.setdefault('first', (gx.cpu(), lg.cpu()))                 # the fp32 images serve all three precisions: the same bits
        assert torch.equal(first[0], gx.cpu()) and torch.equal(first[1], lg.cpu())
        # the other classifiers' VJPs name the right export
        for reserve in (e.reserve_vgg_vjp, e.reserve_classifier_vjp, e.reserve_wrn_vjp):
            with pytest.raises(E.DmadError, match='dmad_dn_vjp'):
                reserve(2)
        e.wrn_vjp_batch = 2
        with pytest.raises(E.DmadError, match='DenseNet-BC-100-12'):
            e.wrn_vjp(x, g)
        # the vote loops: no recheck bound has been measured for this classifier
        clip = clips([0])[0].cuda()
        coef = [[0.1, 0.2]] * 5
        if prec == 'EXACT':
            assert e.mode == E.MODE_EXACT_VOTES
            for call in (lambda: e.smooth_votes(clip, 0.5, 0.9, 3, 1.0, 0.1, 4),
                         lambda: e.eval_samples(clip, 0.5, 0.9, 3, 1.0, 0.1, torch.arange(2).cuda()),
                         lambda: e.spec_smooth_votes(clip, 0.5, 1, 0.9, 0.1, *coef, -80.0, 0.0, 4),
                         lambda: e.spec_eval_samples(clip, 0.5, 1, 0.9, 0.1, *coef, -80.0, 0.0, torch.arange(2).cuda(), 0)):
                with pytest.raises(E.DmadError, match='no recheck bound has been measured for DenseNet-BC-100-12'):
                    call()
            with pytest.raises(E.DmadError, match='no recheck bound'):
                e.set_recheck_margin(0.5)                # no committed margin to inherit
            e.set_mode(E.MODE_FP32)
        with pytest.raises(E.DmadError, match='UNet weights are not finalised'):      # outside the exact-vote mode the loops go on (to the
            e.spec_smooth_votes(clip, 0.5, 1, 0.9, 0.1, *coef, -80.0, 0.0, 4)          # missing UNet here, refused before any launch)
    finally:
        e.close()


def test_other_engines_refuse_and_bad_geometry(sd):
    E = _E()
    r = E.Engine(max_batch=4, precision=E.FP32, with_wavenet=False)
    try:
        bad = dict(E.fold_densenet_state_dict(sd))
        bad['dn.t1.conv.w'] = bad['dn.t1.conv.w'].T.copy()                       # [300, 150]: the right size, the wrong shape
        with pytest.raises(E.DmadError, match=r"\(-4\).*dn.t1.conv.w"):           # DMAD_ERR_SHAPE
            r._load(bad)
        r.load_vgg19_bn(synth.vgg19_bn_state_dict(4321))                         # the refused set left nothing behind
        with pytest.raises(E.DmadError, match='VGG19_bn'):
            r.reserve_dn_vjp(2)
        r.dn_vjp_batch = 2
        with pytest.raises(E.DmadError, match='dmad_vgg_vjp'):
            r.dn_vjp(D.specs(1, 0).cuda(), cotangent(1, 0).cuda())
    finally:
        r.close()
    from audio_models.ConvNets_SpeechCommands.models.densenet import DenseNet
    with pytest.raises(NotImplementedError, match='DenseNet-BC-100-12'):
        DenseNet(depth=40, num_classes=10, in_channels=1).cuda().eval().bind_engine()


# ---- 8. the module, the query path and the drivers ------------------------------------------------------------------------------------
def _bound(sd, e):
    from audio_models.ConvNets_SpeechCommands.models import DenseNet
    m = DenseNet(depth=100, growthRate=12, compressionRate=2, num_classes=10, in_channels=1)
    m.load_state_dict(D.sd32(sd))
    return m.cuda().eval().bind_engine(e)


@pytest.fixture(scope='module')
def dn(eng, sd):
    return _bound(sd, eng)


def test_module_backends(eng, dn, monkeypatch):
    from dmad_hip import autograd as ag
    x = D.specs(3, 12).cuda()
    with torch.no_grad():
        assert torch.equal(dn(x), eng.classify(x))
        assert D.relmax(dn.torch_forward(x).cpu(), eng.classify(x).cpu()) < 2e-4
    g = cotangent(3, 4).cuda()
    grads = {}
    try:
        for backend in ('hip', 'torch', 'auto'):
            dn.grad_backend = backend
            if backend == 'auto':
                monkeypatch.setattr(ag, 'dn_hip', lambda *a: (_ for _ in ()).throw(AssertionError('auto must not reach dn_hip')))
            xg = x.clone().requires_grad_(True)
            (grads[backend],) = torch.autograd.grad((dn(xg) * g).sum(), xg)
            dn.zero_grad(set_to_none=True)
        assert torch.equal(grads['hip'].view(3, 32, 32), eng.dn_vjp(x, g))
        assert all(p.grad is None for p in dn.parameters())
        # the torch layers take their own ReLU decisions, so their gradient is not compared number by number:
        # test_dn_vjp_against_pinned_float64 is the check of the values
        assert all(bool(torch.isfinite(grads[k]).all()) and float(grads[k].abs().max()) > 0 for k in grads)
        print('hip vs torch layers: relmax %.3e' % D.relmax(grads['hip'].cpu(), grads['torch'].cpu()))
        xg = x.clone().requires_grad_(True)
        dn.grad_backend = 'hip'
        monkeypatch.undo()
        with pytest.raises(_E().DmadError, match='first-order only'):
            torch.autograd.grad((dn(xg) * g).sum(), xg, create_graph=True)
    finally:
        dn.grad_backend = 'auto'


def test_query_is_one_call(eng, dn, monkeypatch):
    """AcousticSystem.query with the mel front-end and the DenseNet on one engine: the one-call path (sampler 0), equal to the stages; and
    sampler 4, a baseline waveform defense on the engine in front of it"""
    from acoustic_system import AcousticSystem
    from dmad_hip.transforms import MelSpectrogramDB
    system = AcousticSystem(classifier=dn, transform=MelSpectrogramDB(eng), defender=None).eval()
    x = clips(range(3)).unsqueeze(1).cuda()
    assert system._engine_chain(True) == (eng, 0)
    monkeypatch.setattr(system, 'forward', lambda *a, **k: (_ for _ in ()).throw(AssertionError('query must not loop over forward')))
    logits, dec = system.query(x, 2)
    want = eng.classify(eng.mel_db(x))
    assert tuple(logits.shape) == (2, 3, 10) and torch.equal(logits[0], want) and torch.equal(logits[1], want)
    assert torch.equal(dec[0], want.argmax(1))
    from transforms.time_defense import TimeDomainDefense
    den = TimeDomainDefense('AS', backend='hip', engine=eng)
    smooth = AcousticSystem(classifier=dn, transform=MelSpectrogramDB(eng), defender=den).eval()
    assert smooth._engine_chain(True) == (eng, 4)
    monkeypatch.setattr(smooth, 'forward', lambda *a, **k: (_ for _ in ()).throw(AssertionError('query must not loop over forward')))
    logits4, _ = smooth.query(x, 1)
    want4 = eng.classify(eng.mel_db(eng.wave_smooth(x, 0, den.engine_defense(x)['window'])))
    assert torch.equal(logits4[0], want4) and not torch.equal(want4, want)


def test_query_with_the_diffwave_purifier_is_one_call(sd, monkeypatch):
    """sampler 1: DiffWave on device noise in front of mel dB -> DenseNet on one engine is ONE dmad_query_logits call (6 rows on max_batch
    4), equal bit for bit to the staged computation ddpm_purify -> mel_db -> classify with the same Philox keys"""
    from acoustic_system import AcousticSystem
    from diffusion_models.diffwave_ddpm import DiffWave, WaveNetHIP
    from diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams
    from dmad_hip.transforms import MelSpectrogramDB
    E = _E()
    e = E.Engine(max_batch=4, precision=E.FP32)
    try:
        e.load_wavenet(synth.wavenet_state_dict(1234))
        e.load_densenet_bc_100_12(sd)
        net = _bound(sd, e)
        den = DiffWave(WaveNetHIP(e), calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG), reverse_timestep=2, seed=17)
        system = AcousticSystem(classifier=net, transform=MelSpectrogramDB(e), defender=den, defense_type='wave').eval()
        assert system._engine_chain(True) == (e, 1) and system._engine_chain(False) == (e, 0)
        x = clips([0, 5]).unsqueeze(1).cuda()
        B, R = 2, 3
        calls = []
        real = e.query_logits
        monkeypatch.setattr(e, 'query_logits', lambda *a, **k: (calls.append(a[1]), real(*a, **k))[1])
        monkeypatch.setattr(system, 'forward', lambda *a, **k: (_ for _ in ()).throw(AssertionError('query must not loop over forward')))
        den._draws = 100
        logits, dec = system.query(x, repeats=R)
        assert calls == [R] and den._draws == 100 + R * B and tuple(logits.shape) == (R, B, 10) and torch.equal(dec, logits.argmax(-1))
        ts, c_a, c_b, c_eps, c_div, c_sig = den.purify_coefficients()
        pur = e.ddpm_purify(x.repeat(R, 1, 1), ts, c_a, c_b, c_eps, c_div, c_sig, seed=17, sample0=100)
        staged = torch.cat([e.classify(e.mel_db(pur[i:i + 4])) for i in (0, 4)])
        assert torch.equal(logits.reshape(R * B, 10), staged)
        assert not torch.equal(logits[0], logits[1])                    # fresh noise per repeat
    finally:
        e.close()


def test_query_with_the_spec_purifier_is_one_call(sd, monkeypatch):
    """sampler 3: mel dB -> SpecPurifier (the engine's UNet) -> DenseNet on one engine is ONE dmad_spec_query_logits call (6 rows on
    max_batch 4), equal bit for bit to dmad_spec_eval_samples on each clip alone, whose purified spectrograms the classifier maps to the
    same logits by itself"""
    from acoustic_system import AcousticSystem
    from diffusion_models.improved_diffusion_ddpm import SpecPurifier, create_improved_diffusion
    from diffusion_models.Improved_Diffusion_Unconditional.improved_diffusion.sc09_spectrogram_dataset import MEL_LOWER_BOUND, MEL_UPPER_BOUND
    from dmad_hip.transforms import MelSpectrogramDB
    E = _E()
    e = E.Engine(max_batch=4, precision=E.FP32, with_wavenet=False)
    try:
        pur = create_improved_diffusion(None, reverse_timestep=3, state_dict=synth.unet_state_dict(31), engine=e)
        net = _bound(sd, e)
        den = SpecPurifier(pur, seed=23)
        system = AcousticSystem(classifier=net, transform=MelSpectrogramDB(e), defender=den, defense_type='spec').eval()
        assert system._engine_chain(True) == (e, 3) and system._engine_chain(False) == (e, 0)
        x = clips([1, 7]).unsqueeze(1).cuda()
        B, R = 2, 3
        calls = []
        real = e.spec_query_logits
        monkeypatch.setattr(e, 'spec_query_logits', lambda *a, **k: (calls.append(a[1]), real(*a, **k))[1])
        monkeypatch.setattr(system, 'forward', lambda *a, **k: (_ for _ in ()).throw(AssertionError('query must not loop over forward')))
        den._draws = 40
        logits, dec = system.query(x, repeats=R)
        assert calls == [R] and den._draws == 40 + R * B and tuple(logits.shape) == (R, B, 10)
        assert torch.equal(dec, logits.argmax(-1)) and bool(torch.isfinite(logits).all())
        assert not torch.equal(logits[0], logits[1])                # fresh noise per repeat
        coef = pur.purify_coefficients()
        for b in range(B):
            keys = torch.tensor([40 + r * B + b for r in range(R)]).cuda()
            lg, spec = e.spec_eval_samples(x[b], 0.0, *coef, MEL_LOWER_BOUND, MEL_UPPER_BOUND, keys, 0, seed=23, want_spec=True)
            assert torch.equal(lg, logits[:, b]), b
            assert torch.equal(e.classify(spec), lg), b
    finally:
        e.close()


@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory, sd):
    """ten one-clip classes and a pickled DataParallel(DenseNet) under the reference's module path"""
    import wave
    from audio_models.ConvNets_SpeechCommands.create_model import create_model  # noqa: F401  (makes `models` importable)
    from models.densenet import DenseNet
    from datasets.sc_dataset import SC09_CLASSES
    root = tmp_path_factory.mktemp('dn')
    data = root / 'test'
    for i, c in enumerate(SC09_CLASSES[:10]):
        (data / c).mkdir(parents=True)
        pcm = (synth.synthetic_clip(i).reshape(-1) * 32767).astype('<i2')
        with wave.open(str(data / c / 'a.wav'), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(pcm.tobytes())
    ck = root / 'ConvNets_SpeechCommands'
    ck.mkdir()
    net = DenseNet(depth=100, growthRate=12, compressionRate=2, num_classes=10, in_channels=1)
    net.load_state_dict(D.sd32(sd))
    torch.save(torch.nn.DataParallel(net), str(ck / 'densenet_bc_100_12.pth'))
    return str(data), str(ck / 'densenet_bc_100_12.pth')


@pytest.mark.parametrize('driver,flags,over', [
    ('adaptive_attack_eval', ['--defense', 'None', '--max_iter_1', '2'], {}),
    ('black_box_attack_eval', ['--attack', 'FAKEBOB', '--defense', 'None'], dict(max_iter=2, samples_per_draw=4)),
    ('siren_attack_eval', ['--attack', 'SirenAttack', '--defense', 'None'], dict(max_epoch=1, max_iter=2, n_particles=3)),
    ('baseline_defense_eval', ['--attack', 'FAKEBOB', '--defense', 'AS', '--defense_backend', 'hip'], dict(max_iter=2, samples_per_draw=4)),
    ('imperceptible_attack_eval', ['--max_iter_1', '2', '--max_iter_2', '3'], {}),
])
def test_drivers_take_a_densenet_checkpoint(eng, checkpoint, driver, flags, over):
    import importlib
    from audio_models.ConvNets_SpeechCommands.create_model import create_model
    drv = importlib.import_module(driver)
    data, path = checkpoint
    args = drv.build_parser().parse_args(['--data_path', data, '--classifier_path', path, '--num_per_class', '1', '--batch_size', '4',
                                          '--dataload_workers_nums', '0', '--verbose', '0'] + flags)
    clf = create_model(args.classifier_path).cuda()
    assert type(clf).__name__ == 'DenseNet'
    clf.bind_engine(eng)
    out = drv.run(args, classifier=clf, log=lambda *a: None, **over)
    assert out['total'] == 10 and clf.grad_backend == 'hip'
    for k in ('clean_acc', 'denoised_acc', 'robust_acc'):
        assert np.isfinite(out[k]) and 0.0 <= out[k] <= 100.0, (driver, k, out[k])
