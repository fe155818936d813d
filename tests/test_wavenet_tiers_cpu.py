"""The WaveNet tier tests at small shapes, the part that needs no GPU: that the references and bounds of tests/wavenet_tier_cases.py are
sound.  The two walk predictors visit every tile exactly once and find, on 256 compute units, the branches the case table names; the fp32
CPU oracle is within FP32_TOL of float64 on every case (no ReLU kink decides a GPU test); the rounding model without its roundings is the
oracle; 8 E_q stays below a quarter of the suite's 36-layer tolerances on every case; the float64 oracle's NaN footprint is exactly
[p - R, p + R] of the changed clip."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wavenet_tier_cases as tc  # noqa: E402


# ---- 1. the walk predictors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cus', [256, 304, 64, 8])
def test_walks_visit_every_tile_exactly_once(cus):
    for ntiles in range(1, 601):
        lw = tc.layer_walk(ntiles, cus)
        assert lw['grid'] == min(ntiles, cus) and len(lw['walks']) == lw['grid']
        assert sorted(t for w in lw['walks'] for t in w) == list(range(ntiles)), ('layer', ntiles)
        assert all(w == sorted(w) for w in lw['walks'])
        for npos in (ntiles * 256, ntiles * 256 - 128, ntiles * 256 - 255):
            fw = tc.final_walk(npos, cus)
            assert fw['ntiles'] == ntiles and sorted(t for w in fw['walks'] for t in w) == list(range(ntiles)), ('final', npos)
            assert 1 <= fw['last_rows'] <= 256 and 256 * (ntiles - 1) + fw['last_rows'] == npos


def test_case_table_on_256_compute_units():
    """what the module's table says of every shape case, from the predictors"""
    def walks(case, B=None):
        lw, fw = tc.case_walks(case, 256, B)
        return lw['kind'], lw['grid'], lw['max_tiles'], lw['idle'], fw['ntiles'], fw['max_tiles'], fw['last_rows']
    assert walks('one-tile') == ('plain', 1, 1, 0, 1, 1, 128)
    assert walks('two-clips-per-final-tile') == ('plain', 3, 1, 0, 2, 1, 128)
    assert walks('xcd-one-each') == ('xcd', 8, 1, 0, 4, 1, 256)
    assert walks('straddle') == ('plain', 9, 1, 0, 5, 1, 128)
    assert walks('xcd-small') == ('xcd', 24, 1, 0, 12, 1, 256)
    assert walks('deep-reach') == ('plain', 34, 1, 0, 17, 1, 256)
    assert walks('ragged-xcd') == ('xcd', 256, 2, 5, 129, 1, 256)
    assert walks('long-walk') == ('xcd', 256, 3, 0, 264, 2, 256)
    assert all(walks(c) == ('plain', 6, 1, 0, 3, 1, 256) for c in tc.LADDER)
    # ragged-xcd: chunk 33, step 32: the first workgroup of XCDs 0 - 6 walks two tiles; the last XCD's range [231, 258) is short and leaves five idle
    lw = tc.layer_walk(258, 256)
    assert [len(lw['walks'][b]) for b in range(8)] == [2] * 7 + [1] and lw['walks'][0] == [0, 32] and lw['walks'][7] == [231] and lw['walks'][8 * 27 + 7] == []
    # the solo calls of the batch-independence test take other branches than the batched ones
    assert walks('xcd-small', 1)[:2] == ('xcd', 8) and walks('ragged-xcd', 1)[:3] == ('plain', 86, 1) and walks('long-walk', 1)[:3] == ('plain', 66, 1)
    assert walks('xcd-one-each', 1)[:2] == ('plain', 1)


def test_branch_coverage_is_complete_on_256_and_names_what_another_device_misses():
    cover = tc.branch_coverage(256)
    assert set(cover) == set(tc.BRANCHES) and all(cover.values()), cover
    assert 'ragged-xcd' in cover['XCD walk with idle workgroups'] and 'long-walk' in cover['>= 3 layer tiles per workgroup']
    assert cover['npos < 256'] == ['one-tile'] and cover['>= 2 final tiles per workgroup'] == ['long-walk']
    missed = [name for name, cases in tc.branch_coverage(304).items() if not cases]
    assert 'XCD walk with idle workgroups' in missed and '>= 3 layer tiles per workgroup' in missed


# ---- 2. the references ------------------------------------------------------------------------------------------------------------------
def test_tolerances_are_the_suites_own():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_gpu_parity.py')).read()
    found = {k: float(v) for k, v in re.findall(r'^(FP32_TOL|F16_MAX_TOL|SPLIT_TOL) = ([0-9.e-]+)', src, flags=re.M)}
    found['BF16_MAX_TOL'] = float(re.search(r'^BF16_MAX_TOL, BF16_RMS_TOL = ([0-9.e-]+),', src, flags=re.M).group(1))
    assert found == {'FP32_TOL': tc.FP32_TOL, 'F16_MAX_TOL': tc.F16_MAX_TOL, 'SPLIT_TOL': tc.SPLIT_TOL, 'BF16_MAX_TOL': tc.BF16_MAX_TOL}
    assert all(m in (2, 4, 8) and m <= tc.M16_CAP for m in tc.M16.values())
    for fmt, m in tc.M16.items():           # the smallest power of two >= 2 x the measured ratio
        assert tc.MEASURED_RATIO[fmt] is not None and m >= 2 * tc.MEASURED_RATIO[fmt] and (m == 2 or m // 2 < 2 * tc.MEASURED_RATIO[fmt]), fmt


@pytest.mark.parametrize('case', tc.ALL_CASES)
def test_fp32_oracle_is_within_fp32_tol_of_float64(case):
    nl, L, B, _ = tc.CASES[case]
    r64 = tc.reference(case)
    err = tc.relmax(tc.reference(case, torch.float32), r64)
    print('%s: fp32 CPU oracle vs float64 %.2e (FP32_TOL %.0e), max |eps| %.3f' % (case, err, tc.FP32_TOL, np.abs(r64).max()))
    assert r64.shape == (B, L) and np.isfinite(r64).all() and err <= tc.FP32_TOL


@pytest.mark.parametrize('case', tc.ALL_CASES)
def test_rounding_model_and_its_bound(case):
    """Without its roundings the model is the oracle (its dilated-conv image is scaled and unscaled in fp32: 1e-7); with them, 8 E_q is
    below a quarter of the tolerance the suite holds the tier to after 36 layers."""
    x, r64 = tc.inputs(case), tc.reference(case)
    plain = tc.relmax(tc.model_forward(case, x, None, torch.float64).numpy(), r64)
    assert plain <= 1e-7, plain
    for fmt in ('f16', 'bf16'):
        q32, q64 = tc.model_errors(case, fmt)
        print('%s %s: Q32 vs R64 %.2e, Q64 vs R64 %.2e, 8 E_q %.2e (cap %.2e)' % (case, fmt, q32, q64, 8 * tc.e_q(case, fmt), tc.TIER_TOL[fmt] / 4))
        assert min(q32, q64) > 1e-6                             # the roundings act: the model is not the oracle
        assert tc.M16_CAP * tc.e_q(case, fmt) < tc.TIER_TOL[fmt] / 4
        assert tc.bound16(case, fmt) == tc.M16[fmt] * max(q32, q64) == tc.tier_bound(case, fmt)
    assert tc.tier_bound(case, 'fp32') == tc.FP32_TOL and tc.tier_bound(case, 'split') == tc.SPLIT_TOL


# ---- 3. the footprints ------------------------------------------------------------------------------------------------------------------
def test_reach_and_positions():
    assert [tc.reach(c) for c in tc.LADDER] == [2 ** n - 1 for n in range(1, 13)] + [4096] and tc.reach('deep-reach') == 4096
    assert tc.foot_positions('depth-1') == (0, 127, 128, 255) and tc.foot_positions('deep-reach') == (0, 127, 128, 1088, 2175)
    m = tc.foot_interval('depth-3', 127)
    assert m.shape == (3, 256) and not m[0].any() and not m[2].any() and np.flatnonzero(m[1]).tolist() == list(range(120, 135))
    assert np.flatnonzero(tc.foot_interval('depth-2', 0)[1]).tolist() == [0, 1, 2, 3]
    assert np.flatnonzero(tc.foot_interval('depth-2', 255)[1]).tolist() == [252, 253, 254, 255]
    x0, x1 = tc.inputs('depth-2', 3), tc.foot_inputs('depth-2', 128)
    assert (x0 != x1).nonzero().tolist() == [[1, 128]] and float(x1[1, 128] - x0[1, 128]) == pytest.approx(tc.FOOT_DELTA)
    assert torch.isnan(tc.foot_inputs('depth-2', 128, float('nan'))).nonzero().tolist() == [[1, 128]]


@pytest.mark.parametrize('case', tc.FOOT_CASES)
def test_float64_oracle_nan_footprint_is_the_interval(case):
    for p in tc.foot_positions(case):
        assert np.array_equal(tc.oracle_nan_mask(case, p), tc.foot_interval(case, p)), p
