"""The WaveNet eps-network's three fast tiers at the small shapes where their tile walks and tap reach branch: the 16-bit MFMA tier on bf16
and on f16 operands (wn_init_h16, wn_layer_p, wn_final_p), the split-f16 tier (gemm_f32.hip with x3) and the exact-fp32 tier, through
Engine.wavenet_eps / wavenet_eps_path alone.  Cases, references, bounds and the walk predictors live in tests/wavenet_tier_cases.py
(checked without a GPU by tests/test_wavenet_tiers_cpu.py).

1. every case on every tier against the float64 oracle: FP32_TOL, SPLIT_TOL, and for the 16-bit tiers M16 x E_q of the rounding model;
2. bits do not depend on the walk: a row alone (few tiles, another walk) has the bits it has in the batch; the batch reversed gives the
   reversed result; a B = 1 call after a full batch equals a fresh engine's first call (stale gate store, ping-pong and pad contents);
3. same kernels, same bits: the exact-vote engine's 16-bit tier against a 16-bit engine on f16 operands; the fp32 and split tiers walked
   in passes of 3, 3, 2 against the unchunked engine;
4. a changed sample changes no bit outside [p - R, p + R] of its clip ("reads no row it should not");
5. a NaN sample gives NaN exactly on that interval ("reads every row it should", and a NaN stays a NaN: dmad_common.h)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wavenet_tier_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu

PATH = {'f16': 0, 'fp32': 1, 'split': 2}            # wavenet_eps_path of the exact-vote engine


def new_engine(kind, case):
    """'bf16': precision BF16 (bf16 operands); 'exact': precision EXACT on f16 operands, its waveform tier set to the 16-bit one;
    'f16': precision BF16 on f16 operands; 'exact3': 'exact' with recheck_batch 3"""
    from dmad_hip import engine as E
    nl, L, _, max_batch = tc.CASES[case]
    kw = {'bf16': dict(precision=E.BF16), 'f16': dict(precision=E.BF16, half_type=E.HALF_F16),
          'exact': dict(precision=E.EXACT, half_type=E.HALF_F16), 'exact3': dict(precision=E.EXACT, half_type=E.HALF_F16, recheck_batch=3)}[kind]
    eng = E.Engine(wavenet_config=tc.wavenet_config(nl), clip_len=L, max_batch=max_batch, with_classifier=False, **kw)
    eng.load_wavenet(tc.state_dict(nl))
    if kind.startswith('exact'):
        eng.set_waveform_tier(E.WAVE_16BIT)
    return eng


@pytest.fixture(scope='module')
def engines():
    """(kind, case) -> the module's engine of that geometry, opened on first use, closed at teardown"""
    pool = {}

    def get(kind, case):
        key = (kind,) + tc.CASES[case][:2] + tc.CASES[case][3:]
        if key not in pool:
            pool[key] = new_engine(kind, case)
        return pool[key]
    yield get
    for eng in pool.values():
        eng.close()


def run(eng, tier, x):
    """eps [B, L] of the rows x (on the device) on `tier` of the engine that serves it"""
    return eng.wavenet_eps(x, tc.T_STEP) if tier == 'bf16' else eng.wavenet_eps_path(x, tc.T_STEP, PATH[tier])


def serving(engines, tier, case):
    return engines('bf16' if tier == 'bf16' else 'exact', case)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 0. the case list reaches every branch of the two walks on this device -------------------------------------------------------------
def test_cases_reach_every_walk_branch_on_this_device():
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    cover = tc.branch_coverage(cus)
    for name, cases in cover.items():
        print('%d CUs: %s: %s' % (cus, name, ', '.join(cases) or 'NO CASE'))
    missed = [name for name, cases in cover.items() if not cases]
    assert not missed, 'on %d compute units no case of wavenet_tier_cases reaches: %s' % (cus, '; '.join(missed))


# ---- 1. against the float64 oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tier', tc.TIERS)
@pytest.mark.parametrize('case', tc.ALL_CASES)
def test_eps_against_the_float64_oracle(case, tier, engines):
    nl, L, B, _ = tc.CASES[case]
    ref, bound = tc.reference(case), tc.tier_bound(case, tier)
    got = run(serving(engines, tier, case), tier, tc.inputs(case).cuda()).cpu().numpy()
    err = tc.relmax(got, ref)
    if tier in tc.M16:
        print('%s %s: eps vs float64 oracle %.3e, E_q %.3e, err / E_q = %.3f (m = %d, bound %.3e)' % (case, tier, err, tc.e_q(case, tier), err / tc.e_q(case, tier), tc.M16[tier], bound))
    else:
        print('%s %s: eps vs float64 oracle %.3e (bound %.0e)' % (case, tier, err, bound))
    assert got.shape == (B, L) and np.isfinite(got).all() and err <= bound


# ---- 2. bits do not depend on the walk --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', tc.SHAPE_CASES)
def test_bits_do_not_depend_on_the_walk(case, engines):
    nl, L, B, _ = tc.CASES[case]
    x = tc.inputs(case).cuda()
    fresh = {kind: new_engine(kind, case) for kind in ('bf16', 'exact')}
    try:
        for tier in tc.TIERS:
            eng = serving(engines, tier, case)
            whole = run(eng, tier, x)
            for b in sorted({0, B // 2, B - 1}):
                assert same_bits(run(eng, tier, x[b:b + 1].contiguous()), whole[b:b + 1]), (tier, 'row alone', b)
            if B > 1:
                assert same_bits(run(eng, tier, x.flip(0).contiguous()), whole.flip(0)), (tier, 'reversed')
            run(eng, tier, x)                                   # every buffer as full as this case makes it
            after = run(eng, tier, x[:1].contiguous())
            first = run(fresh['bf16' if tier == 'bf16' else 'exact'], tier, x[:1].contiguous())
            assert same_bits(after, first) and same_bits(after, whole[:1]), (tier, 'B = 1 after the full batch')
    finally:
        for eng in fresh.values():
            eng.close()


# ---- 3. same kernels, same bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', tc.ALL_CASES)
def test_exact_engines_16bit_tier_is_the_f16_engines(case, engines):
    x = tc.inputs(case).cuda()
    assert same_bits(run(engines('exact', case), 'f16', x), engines('f16', case).wavenet_eps(x, tc.T_STEP))


@pytest.mark.parametrize('case', tc.CHUNKED_CASES)
def test_passes_of_recheck_batch_give_the_unchunked_bits(case, engines):
    """for_passes over maxB32 = 3 at B = 8: passes of 3, 3 and 2 rows, every pointer advanced by the rows done"""
    x = tc.inputs(case).cuda()
    assert x.shape[0] == 8
    chunked = new_engine('exact3', case)
    try:
        for tier in ('fp32', 'split'):
            assert same_bits(run(chunked, tier, x), run(engines('exact', case), tier, x)), tier
    finally:
        chunked.close()


# ---- 4, 5. footprints -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', tc.FOOT_CASES)
def test_perturbation_footprint(case, engines):
    """One sample of clip 1 raised by FOOT_DELTA: outside [p - R, p + R] of clip 1, and in clips 0 and 2, every tier keeps its bits."""
    base_x = tc.inputs(case, tc.FOOT_B).cuda()
    for tier in tc.TIERS:
        eng = serving(engines, tier, case)
        base = run(eng, tier, base_x).view(torch.int32).cpu().numpy()
        for p in tc.foot_positions(case):
            got = run(eng, tier, tc.foot_inputs(case, p).cuda()).view(torch.int32).cpu().numpy()
            changed, inside = got != base, tc.foot_interval(case, p)
            assert not (changed & ~inside).any(), (tier, p, np.argwhere(changed & ~inside)[:8].tolist())
            assert changed[tc.FOOT_CLIP, p], (tier, p)          # the change is seen at all


@pytest.mark.parametrize('case', tc.FOOT_CASES)
def test_nan_footprint(case, engines):
    """One sample of clip 1 set to NaN: isnan(eps) is isnan of the float64 oracle, the interval [p - R, p + R] of clip 1, on every tier."""
    for p in tc.foot_positions(case):
        want = tc.oracle_nan_mask(case, p)
        assert np.array_equal(want, tc.foot_interval(case, p))
        x = tc.foot_inputs(case, p, float('nan')).cuda()
        for tier in tc.TIERS:
            got = torch.isnan(run(serving(engines, tier, case), tier, x)).cpu().numpy()
            assert np.array_equal(got, want), (tier, p, 'NaN missing at', np.argwhere(want & ~got)[:8].tolist(), 'NaN outside at', np.argwhere(got & ~want)[:8].tolist())
