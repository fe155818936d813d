"""The Python side of the C boundary (dmad_hip.engine) on a scripted library: no GPU, no libdmad_hip.so.

Every wrapper that walks a batch in passes of max_batch rows is driven with B = 9 on max_batch = 4 and the calls the library would
have received are compared with the tensors handed in and returned: row counts, pointer advance per pass, Philox key offsets, the
trajectory slices of the VP-SDE pair, optional outputs.  The one-call surfaces, the refusal texts and the folded weight arrays
(sha256 recorded from the parent of the commit that added this file, on which the whole file passed unchanged) are pinned the same
way.  Only public names are used; vgg_vjp_tape (it allocates on 'cuda') and the standalone op hooks (they load the real library) are
covered by the GPU suite."""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest
import torch

from dmad_hip import engine as E, synth
from dmad_hip._lib import DmadError

L, MB = 2048, 4                     # L = 2048: masking_frames() == 1, the smallest length the masking wrappers accept
GPU_TEXT = 'input must live on the GPU (the dmad engine has no CPU path)'


class Dev(torch.Tensor):
    """A host tensor that says it lives on the device; views, detach / contiguous / float and empty_like keep the subclass."""
    @property
    def is_cuda(self):
        return True


def dev(*shape, dtype=torch.float32):
    return (torch.arange(math.prod(shape)).reshape(shape) + 1).to(dtype).as_subclass(Dev)


class Lib:
    """Every export exists, records (name, args) and succeeds; `hook` may look at the arguments while the call is live."""
    def __init__(self, hook=None):
        self.calls, self.seen, self.hook = [], [], hook

    def __getattr__(self, name):
        def export(*args):
            self.calls.append((name, args))
            if self.hook is not None:
                self.seen.append(self.hook(name, args))
            return 0
        return export


@pytest.fixture
def eng(monkeypatch):
    class Stream:
        cuda_stream = 0
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a, **k: Stream())
    e = E.Engine.__new__(E.Engine)
    e.lib, e._h, e.L, e.max_batch, e.num_classes, e.device = Lib(), None, L, MB, 10, torch.device('cpu')
    e.has_m5, e.m5_classes, e.m5_maps, e.vgg_vjp_batch = True, 35, ((32, 30), (32, 5), (64, 1), (64, 1)), MB
    return e


def norm(a):
    """an argument as a comparable value: pointers as addresses, ctypes arrays as tuples"""
    if isinstance(a, C.c_void_p):
        return a.value
    if isinstance(a, C.Array):
        return tuple(a)
    if isinstance(a, C._Pointer):
        return C.addressof(a.contents)
    return a


def row_bytes(t):
    return t[0].numel() * t.element_size()


# ---------------------------------------------------------------------------------------------------------------- the table
# A case runs one wrapper on fresh [B, ...] tensors and returns (export, index of the row count, index of the key or None,
# {argument index: per-row tensor | (tensor, rows per clip) | None}); index 0 is the handle.  opt: ask for the optional outputs.
S_STEPS = 2
SCHED = dict(k=[5, 3], h=[.1, .2], hb=[.3, .4], q=[.5, .6], gs=[.7, .8])


def c_wavenet_eps(e, B, opt):
    x = dev(B, L)
    return 'dmad_wavenet_eps', 3, None, {1: x, 4: e.wavenet_eps(x, 3)}


def c_wavenet_eps_path(e, B, opt):
    x = dev(B, L)
    return 'dmad_wavenet_eps_path', 3, None, {1: x, 5: e.wavenet_eps_path(x, 3, 2)}


def _pair(r, opt):
    return r if opt else (r, None)


def c_wavenet_eps_vjp(e, B, opt):
    x, g = dev(B, L), dev(B, L)
    gx, eps = _pair(e.wavenet_eps_vjp(x, 3, g, want_eps=opt), opt)
    return 'dmad_wavenet_eps_vjp', 3, None, {1: x, 4: g, 5: gx, 6: eps}


def c_one_shot(e, B, opt):
    x = dev(B, L)
    return 'dmad_one_shot', 5, None, {1: x, 6: e.one_shot(x, 3, .5, .25)}


def c_ddpm_step(e, B, opt):
    x, z = dev(B, L), (dev(B, L) if opt else None)
    assert e.ddpm_step(x, 3, .1, .2, .3, z, seed=11, sample0=7) is x
    return 'dmad_ddpm_step', 9, 8, {1: x, 6: z}


def c_diffuse(e, B, opt):
    x, z = dev(B, L), (dev(B, L) if opt else None)
    return 'dmad_diffuse', 7, 6, {1: x, 4: z, 8: e.diffuse(x, .5, .25, z, seed=11, sample0=7)}


def c_ddpm_purify(e, B, opt):
    x = dev(B, L)
    return 'dmad_ddpm_purify', 10, 9, {1: x, 11: e.ddpm_purify(x, 2, .5, .25, [.1, .2], [.3, .4], [.5, .6], seed=11, sample0=7)}


def c_unet_eps(e, B, opt):
    x = dev(B, 32, 32)
    return 'dmad_unet_eps', 3, None, {1: x, 4: e.unet_eps(x, 3)}


def c_unet_eps_tier(e, B, opt):
    x = dev(B, 32, 32)
    return 'dmad_unet_eps_tier', 3, None, {1: x, 5: e.unet_eps(x, 3, tier=2)}


def c_unet_eps_vjp(e, B, opt):
    x, g = dev(B, 32, 32), dev(B, 32, 32)
    gx, eps = _pair(e.unet_eps_vjp(x, 3, g, want_eps=opt), opt)
    return 'dmad_unet_eps_vjp', 3, None, {1: x, 4: g, 5: gx, 6: eps}


def c_unet_p_sample(e, B, opt):
    x, z = dev(B, 32, 32), (dev(B, 32, 32) if opt else None)
    return 'dmad_unet_p_sample', 11, 10, {1: x, 8: z, 12: e.unet_p_sample(x, 3, .1, .2, .3, .4, .5, z, seed=11, sample0=7, want_x0=opt)}


def c_mel_db(e, B, opt):
    x = dev(B, L)
    return 'dmad_mel_db', 2, None, {1: x, 3: e.mel_db(x)}


def c_mel_power(e, B, opt):
    x = dev(B, L)
    return 'dmad_mel_power', 2, None, {1: x, 3: e.mel_power(x)}


def c_mel_db_vjp(e, B, opt):
    x, g = dev(B, L), dev(B, 32, 32)
    gx, sp = _pair(e.mel_db_vjp(x, g, want_spec=opt), opt)
    return 'dmad_mel_db_vjp', 2, None, {1: x, 3: g, 4: gx, 5: sp}


def c_classify(e, B, opt):
    x = dev(B, 1, 32, 32)
    return 'dmad_classify', 2, None, {1: x, 3: e.classify(x)}


def c_classify_tier(e, B, opt):
    x = dev(B, 1, 32, 32)
    return 'dmad_classify_tier', 2, None, {1: x, 4: e.classify_tier(x, 2)}


def c_classify_vjp(e, B, opt):
    x, g = dev(B, 32, 32), dev(B, 10)
    gs, lg = _pair(e.classify_vjp(x, g, want_logits=opt), opt)
    return 'dmad_classify_vjp', 2, None, {1: x, 3: g, 4: gs, 5: lg}


def c_vgg_vjp(e, B, opt):
    x, g = dev(B, 32, 32), dev(B, 10)
    gs, lg = _pair(e.vgg_vjp(x, g, want_logits=opt), opt)
    return 'dmad_vgg_vjp', 2, None, {1: x, 3: g, 4: gs, 5: lg}


def c_masking_loss_vjp(e, B, opt):
    d, th, sc = dev(B, L), dev(B, 1025, 1), dev(B)
    r = e.masking_loss_vjp(d, th, sc, want_psd=opt)
    return 'dmad_masking_loss_vjp', 2, None, {1: d, 3: th, 4: sc, 5: r[0], 6: r[1], 7: r[2] if opt else None}


def c_masking_step(e, B, opt):
    x, d, gn, al, th, sc = dev(B, L), dev(B, L), dev(B, L), dev(B), dev(B, 1025, 1), dev(B)
    return 'dmad_masking_step', 6, None, {1: x, 2: d, 3: gn, 4: al, 7: th, 8: sc, 9: e.masking_step(x, d, gn, al, -.01, th, sc)}


def c_wave_smooth(e, B, opt):
    x = dev(B, L)
    return 'dmad_wave_smooth', 2, None, {1: x, 5: e.wave_smooth(x, 1, 7)}


def c_wave_smooth_vjp(e, B, opt):
    x, g = dev(B, L), dev(B, L)
    return 'dmad_wave_smooth_vjp', 3, None, {1: x, 2: g, 6: e.wave_smooth_vjp(x, g, 1, 7)}


KER = np.arange(6, dtype=np.float32).reshape(2, 3)


def c_wave_resample(e, B, opt):
    x = dev(B, 40)
    return 'dmad_wave_resample', 2, None, {1: x, 10: e.wave_resample(x, KER, 2, 3, 20)}


def c_wave_resample_vjp(e, B, opt):
    g = dev(B, 20)
    return 'dmad_wave_resample_vjp', 2, None, {1: g, 10: e.wave_resample_vjp(g, 40, KER, 2, 3)}


def c_wave_iir(e, B, opt):
    x = dev(B, L)
    return 'dmad_wave_iir', 2, None, {1: x, 8: e.wave_iir(x, [1., 2., 3.], [1., .5, .25], -1., 1.)}


def c_wave_iir_vjp(e, B, opt):
    x, g = dev(B, L), dev(B, L)
    gx, y = _pair(e.wave_iir_vjp(x, g, [1., 2., 3.], [1., .5, .25], -1., 1., want_y=opt), opt)
    return 'dmad_wave_iir_vjp', 3, None, {1: x, 2: g, 9: gx, 10: y}


def _c_vpsde(name, shape):
    def fwd(e, B, opt):
        x = dev(B, *shape)
        out, traj = _pair(getattr(e, name)(x, .5, .25, **SCHED, seed=11, sample0=7, path=1, want_traj=opt), opt)
        if opt:
            assert tuple(traj.shape) == ((S_STEPS + 1) * B, math.prod(shape)) and traj.dtype == torch.float32
        return 'dmad_' + name, 2, 13, {1: x, 11: None, 15: out, 16: (traj, S_STEPS + 1) if opt else None}

    def vjp(e, B, opt):
        traj, g = dev((S_STEPS + 1) * B, math.prod(shape)), dev(B, *shape)
        gx = getattr(e, name + '_vjp')(traj, .5, SCHED['k'], SCHED['h'], SCHED['hb'], SCHED['q'], g)
        return 'dmad_' + name + '_vjp', 2, None, {1: (traj, S_STEPS + 1), 9: g, 10: gx}
    fwd.__name__, vjp.__name__ = 'c_' + name, 'c_' + name + '_vjp'
    return [fwd, vjp]


CASES = [c_wavenet_eps, c_wavenet_eps_path, c_wavenet_eps_vjp, c_one_shot, c_ddpm_step, c_diffuse, c_ddpm_purify, c_unet_eps,
         c_unet_eps_tier, c_unet_eps_vjp, c_unet_p_sample, c_mel_db, c_mel_power, c_mel_db_vjp, c_classify, c_classify_tier,
         c_classify_vjp, c_vgg_vjp, c_masking_loss_vjp, c_masking_step, c_wave_smooth, c_wave_smooth_vjp, c_wave_resample,
         c_wave_resample_vjp, c_wave_iir, c_wave_iir_vjp] + _c_vpsde('vpsde_purify', (L,)) + _c_vpsde('spec_vpsde_purify', (32, 32))


@pytest.mark.parametrize('opt', [False, True], ids=['plain', 'optional'])
@pytest.mark.parametrize('B', [9, 4])
@pytest.mark.parametrize('case', CASES, ids=lambda c: c.__name__[2:])
def test_passes(eng, case, B, opt):
    """1. and 2.: the passes are 4 + 4 + 1 (one call at B = 4) of the expected export; every per-row pointer advances by the rows
    before the pass, an absent optional tensor is None in every pass, the key is sample0 + s, everything else never changes."""
    export, rows, key, ptrs = case(eng, B, opt)
    calls = eng.lib.calls
    assert [name for name, _ in calls] == [export] * len(calls)
    assert [args[rows] for _, args in calls] == ([4, 4, 1] if B == 9 else [4])
    rest0 = None
    for k, (_, args) in enumerate(calls):
        s = MB * k
        for i, t in ptrs.items():
            if t is None:
                assert norm(args[i]) is None, (i, k)
            else:
                t, per_clip = t if isinstance(t, tuple) else (t, 1)
                assert norm(args[i]) == t.data_ptr() + per_clip * s * row_bytes(t), (i, k)
        if key is not None:
            assert args[key] == 7 + s and type(args[key]) is int
        rest = [norm(a) for i, a in enumerate(args) if i not in ptrs and i not in (rows, key)]
        rest0 = rest if rest0 is None else rest0
        assert rest == rest0 and rest[0] is None and rest[-1] is None        # the handle in front, the stream at the end
    if key is not None and B == 9:
        assert [args[key] for _, args in calls] == [7, 11, 15]


@pytest.mark.parametrize('name,shape', [('vpsde_purify', (L,)), ('spec_vpsde_purify', (32, 32))])
def test_vpsde_explicit_noise_is_a_fresh_slice_per_pass(eng, name, shape):
    """3.: the floats at the z pointer during pass k are z[:, s:e] (read inside the call: the copy is freed afterwards)."""
    B, width = 9, math.prod(shape)
    z = dev(S_STEPS + 1, B, width)

    def read(export, args):
        n = (S_STEPS + 1) * args[2] * width
        return torch.tensor((C.c_float * n).from_address(args[11].value)[:])
    eng.lib = Lib(read)
    getattr(eng, name)(dev(B, *shape), .5, .25, **SCHED, z=z)
    assert len(eng.lib.seen) == 3
    for k, got in enumerate(eng.lib.seen):
        assert torch.equal(got, z[:, MB * k:MB * (k + 1)].reshape(-1))
    with pytest.raises(DmadError, match=r'z must be a CUDA tensor \[3, 9, %d\], not ' % width):
        getattr(eng, name)(dev(B, *shape), .5, .25, **SCHED, z=dev(S_STEPS + 1, B, width + 1))


# ---------------------------------------------------------------------------------------------------------------- one call
def _is(t, shape, dtype=torch.float32):
    return tuple(t.shape) == tuple(shape) and t.dtype == dtype


def test_one_call_surfaces(eng):
    """4.: one library call whatever B is, and the documented shapes and dtypes of what comes back."""
    B, R, e = 9, 3, eng
    x, clip, idx = dev(B, 1, L), dev(L), dev(5, dtype=torch.int64)
    c5 = [[.1, .2, .3]] * 5                   # t_star + 1 = 3 coefficients each
    iir = dict(kind='IIR', b=[1., 2.], a=[1., .5], lo=-1., hi=1.)
    ds = dict(kind='DS', down=(KER, 2, 3, 20), up=(KER, 1, 3))

    def once(export, call):
        e.lib = Lib()
        r = call()
        assert [n for n, _ in e.lib.calls] == [export], export
        return r

    out, dec = once('dmad_m5_logits', lambda: e.m5_logits(x, want_decisions=True))
    assert _is(out, (B, 35)) and _is(dec, (B,), torch.int32)
    gx, lp = once('dmad_m5_vjp', lambda: e.m5_vjp(x, dev(B, 35), want_logits=True))
    assert _is(gx, (B, L)) and _is(lp, (B, 35))
    pooled, d8 = once('dmad_m5_tape', lambda: e.m5_tape(x, 2))
    assert _is(pooled, (B, 32, 5)) and _is(d8, (B, 32, 5), torch.uint8)
    for export, width, call in (
            ('dmad_query_logits', 10, lambda: e.query_logits(x, R, 1, 2, .5, .25, [.1, .2], [.3, .4], [.5, .6], seed=1, sample0=7)),
            ('dmad_query_logits', 10, lambda: e.query_logits(x, R)),
            ('dmad_m5_query_logits', 35, lambda: e.m5_query_logits(x, R, 1, 2, .5, .25, [.1, .2], [.3, .4], [.5, .6], seed=1, sample0=7)),
            ('dmad_spec_query_logits', 10, lambda: e.spec_query_logits(x, R, 2, .5, .25, *c5, -80., 0.)),
            ('dmad_defense_query_logits', 10, lambda: e.defense_query_logits(x, R, dict(kind='AS', window=5))),
            ('dmad_defense_query_logits', 10, lambda: e.defense_query_logits(x, R, ds)),
            ('dmad_m5_defense_query_logits', 35, lambda: e.m5_defense_query_logits(x, R, iir))):
        logits, dec = once(export, call)
        assert _is(logits, (R * B, width)) and _is(dec, (R * B,), torch.int32), export
    assert e.lib.calls[0][1][2:4] == (B, R)
    counts, lg, x0 = once('dmad_smooth_votes', lambda: e.smooth_votes(clip, .5, .9, 3, .5, .25, 6, want_logits=True, want_x0=True))
    assert _is(counts, (10,), torch.int64) and _is(lg, (6, 10)) and _is(x0, (6, L))
    assert e.lib.calls[0][1][8] == MB                                    # batch defaults to, and is capped at, max_batch
    counts, lg, sp = once('dmad_spec_smooth_votes', lambda: e.spec_smooth_votes(clip, .5, 2, .5, .25, *c5, -80., 0., 6, batch=64,
                                                                                want_logits=True, want_spec=True))
    assert _is(counts, (10,), torch.int64) and _is(lg, (6, 10)) and _is(sp, (6, 1, 32, 32)) and e.lib.calls[0][1][14] == MB
    assert once('dmad_smooth_votes', lambda: e.smooth_votes(clip, .5, .9, 3, .5, .25, 6))[1:] == (None, None)
    lg, x0 = once('dmad_eval_samples', lambda: e.eval_samples(clip, .5, .9, 3, .5, .25, idx, path=2, delta=dev(5, L), want_x0=True))
    assert _is(lg, (5, 10)) and _is(x0, (5, L))
    lg, sp = once('dmad_spec_eval_samples', lambda: e.spec_eval_samples(clip, .5, 2, .5, .25, *c5, -80., 0., idx, tier=1, want_spec=True))
    assert _is(lg, (5, 10)) and _is(sp, (5, 1, 32, 32))
    assert _is(once('dmad_spec_eval_samples', lambda: e.spec_eval_samples(clip, .5, 2, .5, .25, *c5, -80., 0., idx, tier=1)), (5, 10))
    assert _is(once('dmad_nes_probes', lambda: e.nes_probes(x, 4, .01, True)), (B * 5, L))
    assert _is(once('dmad_nes_grad', lambda: e.nes_grad(dev(B, 4), 4, .5)), (B, L))
    P = 2
    st = once('dmad_pso_init', lambda: e.pso_init(x, x, x, P))
    assert len(st) == 4 and all(_is(t, (B * P, L)) for t in st)
    own = [dev(B * P, L) for _ in range(3)]
    loc, vel, q = once('dmad_pso_step', lambda: e.pso_step(x, x, x, own[0], x, P, .7, 1.4, 1.4, 1, 0, own[1], own[2]))
    assert loc is own[1] and vel is own[2] and _is(q, (B * P, L))
    best = once('dmad_pso_update_best', lambda: e.pso_update_best(dev(B, P), dev(B, P, dtype=torch.int64), own[1], dev(B, P), own[0], dev(B),
                                                                 dev(B, L), dev(B, dtype=torch.int64)))
    assert len(best) == 5
    assert _is(once('dmad_philox_uniform', lambda: e.philox_uniform(1, 2, 3, B)), (B, L))
    assert _is(once('dmad_philox_normal', lambda: e.philox_normal(1, 2, 3, B)), (B, L))
    assert e.lib.calls[0][1][1:5] == (1, 2, 3, B)
    assert _is(once('dmad_philox_raw', lambda: e.philox_raw(1, 2, 3, 5)), (20,), torch.int32)
    once('dmad_vote', lambda: e.vote(dev(B, 10), dev(10, dtype=torch.int64)))
    assert _is(once('dmad_power_to_db', lambda: e.power_to_db(dev(B, 1, 32, 32))), (B, 1, 32, 32))
    assert e.lib.calls[0][1][2] == B * 1024
    assert once('dmad_recheck_stats', lambda: e.recheck_stats(detail=True)) == (0, 0, 0)
    assert once('dmad_spec_recheck_stats2', lambda: e.spec_recheck_stats(reset=True)) == (0, 0)
    assert once('dmad_profile_read', e.profile_read) == (0.0, 0) and once('dmad_profile_read_final', e.profile_read_final) == (0.0, 0)
    for name, attr in (('vjp', 'vjp_batch'), ('unet_vjp', 'unet_vjp_batch'), ('classifier_vjp', 'classifier_vjp_batch'), ('vgg_vjp', 'vgg_vjp_batch')):
        setattr(e, attr, 0)
        once('dmad_reserve_' + name, lambda: getattr(e, 'reserve_' + name)(6))
        assert e.lib.calls[0][1] == (None, 6) and getattr(e, attr) == (MB if name == 'vgg_vjp' else 6)
        once('dmad_reserve_' + name, lambda: getattr(e, 'reserve_' + name)(2))
        assert getattr(e, attr) == (MB if name == 'vgg_vjp' else 6)               # a smaller request never shrinks the record


def test_query_coefficients_reach_the_library(eng):
    """the host coefficient arrays of the query / purify / vote surfaces: the values handed in, in the export's order"""
    x, f = dev(2, L), np.float32
    eng.query_logits(x, 1, 1, 2, .5, .25, [.1, .2], [.3, .4], [.5, .6])
    eng.m5_query_logits(x, 1, 0)
    eng.spec_query_logits(x, 1, 1, .5, .25, [1, 2], [3, 4], [5, 6], [7, 8], [9, 10], -80., 0.)
    eng.ddpm_purify(x, 2, .5, .25, [.1, .2], [.3, .4], [.5, .6])
    eng.vpsde_purify(x, .5, .25, **SCHED)
    eng.debug_rounding(1, 0, 1)
    q, m5, sq, dp, vp, dr = (args for _, args in eng.lib.calls)
    assert [tuple(a) for a in q[8:11]] == [(f(.1), f(.2)), (f(.3), f(.4)), (f(.5), f(.6))] and all(a._type_ is C.c_float for a in q[8:11])
    assert m5[8:11] == (None, None, None)
    assert [tuple(a) for a in sq[7:12]] == [(1., 2.), (3., 4.), (5., 6.), (7., 8.), (9., 10.)]
    assert [tuple(a) for a in dp[5:8]] == [tuple(a) for a in q[8:11]]
    assert tuple(vp[6]) == (5, 3) and vp[6]._type_ is C.c_int32
    assert [tuple(a) for a in vp[7:11]] == [tuple(f(v) for v in SCHED[n]) for n in ('h', 'hb', 'q', 'gs')]
    assert tuple(dr[1]) == (1, 0, 1, 0, 0)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_host_tensors_are_refused_with_the_same_text(eng):
    """5.: a plain host tensor raises DmadError with the one text at every site that raises it."""
    e, h = eng, torch.zeros
    x, sp, own = dev(2, L), dev(2, 32, 32), dev(4, L)
    for call in (lambda: e.wavenet_eps(h(2, L), 3),                                      # the waveform shaper
                 lambda: e.unet_eps(h(2, 32, 32), 3),                                    # the spectrogram shaper
                 lambda: e.wave_resample(h(2, 40), KER, 2, 3, 20),                        # the row shaper
                 lambda: e.classify(h(2, 1, 32, 32)), lambda: e.classify_tier(h(2, 1, 32, 32), 0),
                 lambda: e.power_to_db(h(2, 32)), lambda: e.nes_grad(h(2, 4), 4, .5),
                 lambda: e.masking_loss_vjp(x, h(2, 1025, 1), dev(2)), lambda: e.masking_loss_vjp(x, dev(2, 1025, 1), h(2)),
                 lambda: e.pso_step(x, x, x, h(4, L), x, 2, .7, 1.4, 1.4, 1, 0, own, own),  # a caller-owned state tensor
                 lambda: e.pso_update_best(h(2, 2), dev(2, 2, dtype=torch.int64), own, dev(2, 2), own, dev(2), x, dev(2, dtype=torch.int64))):
        with pytest.raises(DmadError) as err:
            call()
        assert str(err.value) == GPU_TEXT
    with pytest.raises(DmadError) as err:
        e.masking_step(x, h(2, L), x, dev(2), .01, dev(2, 1025, 1), dev(2))
    assert str(err.value) == 'delta is updated in place: it must be a contiguous float32 tensor on the GPU (the dmad engine has no CPU path)'
    assert e.lib.calls == []


def test_shape_refusals_keep_their_texts(eng):
    e = eng
    x, sp = dev(3, L), dev(3, 32, 32)
    for call, text in (
            (lambda: e.wavenet_eps_vjp(x, 3, dev(2, L)), 'g_eps has shape (2, %d), x_t (3, %d)' % (L, L)),
            (lambda: e.unet_eps_vjp(sp, 3, dev(2, 32, 32)), 'g_eps has shape (2, 32, 32), x_t (3, 32, 32)'),
            (lambda: e.classify_vjp(sp, dev(3, 9)), 'g_logits must be a CUDA tensor [3, 10], not (3, 9)'),
            (lambda: e.vgg_vjp(sp, torch.zeros(3, 10)), 'g_logits must be a CUDA tensor [3, 10], not (3, 10)'),
            (lambda: e.m5_vjp(x, dev(3, 10)), 'g must be a CUDA tensor [3, 35], not (3, 10)'),
            (lambda: e.mel_db_vjp(x, dev(2, 32, 32)), 'g_spec has 2 rows, x 3'),
            (lambda: e.wave_smooth_vjp(x, dev(2, L), 0, 5), 'g_y has 2 rows, x 3'),
            (lambda: e.wave_iir_vjp(x, dev(2, L), [1.], [1.]), 'g_y has 2 rows, x 3'),
            (lambda: e.vpsde_purify_vjp(dev(8, L), .5, SCHED['k'], SCHED['h'], SCHED['hb'], SCHED['q'], x),
             'traj must be the [(S + 1) * B, L] = [9, %d] trajectory of vpsde_purify, not (8, %d)' % (L, L)),
            (lambda: e.spec_vpsde_purify_vjp(dev(9, 1000), .5, SCHED['k'], SCHED['h'], SCHED['hb'], SCHED['q'], sp),
             'traj must be the [(S + 1) * B, 1024] = [9, 1024] trajectory of spec_vpsde_purify, not (9, 1000)'),
            (lambda: e.vpsde_purify(x, .5, .25, [5, 3], [.1], [.3, .4], [.5, .6], [.7, .8]),
             'the schedule arrays k / h / hb / q / gs must have one entry per Euler step (2)'),
            (lambda: e.spec_vpsde_purify_vjp(dev(3, 1024), .5, [], [], [], [], sp),
             'the schedule arrays k / h / hb / q / gs must have one entry per Euler step (0)'),
            (lambda: e.wave_iir(x, [1., 2., 3.], [1., .5]), 'expected 3 coefficients, got 2'),
            (lambda: e.defense_query_logits(x, 1, dict(kind='IIR', b=[1., 2.], a=[1.], lo=-1., hi=1.)), 'expected 2 coefficients, got 1'),
            (lambda: e.wave_resample(dev(3, 2, 40), KER, 2, 3, 20), 'x must be [B, 40], not (3, 2, 40)'),
            (lambda: e.masking_loss_vjp(x, dev(3, 1025, 2), dev(3)), 'theta must be [3, 1025, 1] and psd_scale [3], not (3, 1025, 2) and (3,)'),
            (lambda: e.masking_step(x, dev(3, L), x, dev(2), .01, dev(3, 1025, 1), dev(3)), 'x, g_net and alpha must hold 3 rows on the GPU'),
            (lambda: e.m5_tape(x, 5), 'layer must be 1..4, not 5')):
        with pytest.raises(DmadError) as err:
            call()
        assert str(err.value) == text
    assert e.lib.calls == []


# ---------------------------------------------------------------------------------------------------------------- folding
def _digest(arrays):
    h = hashlib.sha256()
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        h.update(k.encode()); h.update(str(a.dtype).encode()); h.update(str(a.shape).encode()); h.update(a.tobytes())
    return h.hexdigest()


FOLDED = {      # sha256 over (name, dtype, shape, bytes) of the folded arrays in sorted order, recorded before the fold functions were touched
    'wavenet': 'd9960fd8fa8c0aca57f80aa4bc35e242dfa812e499aa4891f8e4f44e5bf8dcbc',
    'vgg19_bn': '0c3f41178490fe8fbfcf5a9b4b13fae5b7f5b05b53aa42bacb7aa42f087d1135',
    'resnext29': '5be93ea39c9d30476e7d354c653ce590588608a53b225b11252cb070d12ed7aa',
    'm5': 'a4e951f3525f4af22255d3331455564c5a075630757cce69201245647c444d81',
    'unet': '15fd6fcd16b01b63f85c6b3c56a0e4cdb0ce5fcb2aab0345f4da4c38345c39d1',
}


@pytest.mark.parametrize('net', sorted(FOLDED))
def test_folded_arrays_are_byte_identical(eng, net):
    """6.: what reaches dmad_load_weight for the synthetic state dicts has not moved by a bit."""
    if net == 'unet':                   # no fold function: the arrays are taken where the loader hands them to the library
        got = {}

        def keep(export, args):
            if export == 'dmad_load_weight':
                shape = tuple(args[3][:args[4]])
                got[args[1].decode()] = np.frombuffer(C.string_at(args[2], 4 * math.prod(shape)), dtype=np.float32).reshape(shape)
        eng.lib, eng.has_unet = Lib(keep), False
        sd = synth.unet_state_dict()
        eng.load_unet(sd)
        assert eng.has_unet and eng.unet_owner == E.state_fingerprint(sd) and eng.lib.calls[-1][0] == 'dmad_last_warning'
        assert sorted(got) == sorted('un.' + k for k in sd)
    else:
        got = {'wavenet': lambda: E.fold_wavenet_state_dict(synth.wavenet_state_dict(), synth.WAVENET_CONFIG['num_res_layers']),
               'vgg19_bn': lambda: E.fold_vgg19_bn_state_dict(synth.vgg19_bn_state_dict()),
               'resnext29': lambda: E.fold_resnext29_state_dict(synth.resnext29_state_dict()),
               'm5': lambda: E.fold_m5_state_dict(synth.m5_state_dict())}[net]()
        assert all(a.dtype == np.float32 for a in got.values())
    assert _digest(got) == FOLDED[net]


def test_default_geometry_is_one_table():
    g = dict(E.Engine.geometry(None))
    assert g == dict(res_channels=256, skip_channels=256, num_res_layers=36, dilation_cycle=12, diffusion_step_embed_dim_in=128,
                     diffusion_step_embed_dim_mid=512, diffusion_step_embed_dim_out=512)
    assert dict(E.Engine.geometry(dict(num_res_layers=5, in_channels=1, bogus=3))) == dict(g, num_res_layers=5)
