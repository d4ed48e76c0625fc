"""The stage-2 seam cases (tests/stage2_cases.py) are what they claim to be -- checked on the oracle alone, without a GPU -- and the
reference the GPU tests compare with (the oracle evaluated in np.longdouble) is pinned against its float64 evaluation.

These are conditions on the INPUTS, not tolerances: if a change to ``helpers.synthetic_domain`` breaks one, the case has to be chosen
again (another seed, another NaN placement), never the condition relaxed."""
import numpy as np
import pytest

from lorenzcycletoolkit_amd import tables
from oracle import lec_oracle as o
from tests import stage2_cases as sc
from tests.helpers import SCALARS, compare

# float64 against extended evaluation of the oracle, in `compare`'s measure (each term's scale): measured 2.1e-13 at 160 levels and at
# 131 rows.  With this bar the GPU tests' 1e-9 keeps two orders of room over the reference's own rounding.
REFERENCE_BAR = 1e-11


def _nan_rows(b, field, t, k):
    return np.flatnonzero(np.isnan(b.f[field + "_ZA"][t, k])).tolist()


@pytest.mark.parametrize("case", sc.FIXED_IDS + (sc.MOVING_ID,))
def test_every_term_is_finite_and_none_is_zero(case):
    """No case degenerates into "no level left" (a term that integrates an empty array is 0.0) or into a NaN."""
    s, _ = sc.reference(case)
    for name in SCALARS:
        assert np.isfinite(s[name]).all(), (case, name)
        assert np.any(s[name] != 0.0), (case, name)


@pytest.mark.parametrize("case", sc.TALL_CLEAN_IDS + sc.TALL_NAN_IDS)
def test_tall_boxes_have_the_intended_height_on_the_intended_side_of_64(case):
    dom, limits, exp = sc.build(case)
    iw, ie, js, jn = tables.box_indices(dom.lat, dom.lon, *limits)
    assert jn - js + 1 == exp["height"] and ie - iw + 1 >= 2
    assert exp["kernel"] == ("small" if exp["height"] <= 64 else "general")
    assert o.make_box(dom, *limits).idx == (iw, ie, js, jn)         # the oracle selects the same box


def test_moving_boxes_have_the_intended_heights():
    """One buffer of 130 rows (general kernel) that holds a 64-row and a 2-row box: alone in a shard those take the small kernel."""
    dom, limits, exp = sc.build(sc.MOVING_ID)
    boxes = [tables.box_indices(dom.lat, dom.lon, *lim) for lim in limits]
    assert boxes == exp["boxes"]
    heights = [b[3] - b[2] + 1 for b in boxes]
    assert heights == exp["height"] == [130, 64, 65, 2, 100]
    assert max(heights) > 64 and exp["kernel"] == "general"
    assert heights[1] <= 64 and heights[3] <= 64


@pytest.mark.parametrize("case", sc.NAN_FIXED_IDS)
def test_nan_cases_really_lose_or_repair_levels(case):
    dom, limits, exp = sc.build(case)
    with np.errstate(invalid="ignore"):
        b = o.make_box(dom, *limits)
        _, lv = o.all_terms(b)
    assert exp["za_nan"] and (exp["repaired"] or exp["dropped"])
    for field, t, k, rows in exp["za_nan"]:             # before _handle_nans: NaN at the intended (level, latitude) places and only there
        assert _nan_rows(b, field, t, k) == rows, (field, t, k)
    for table, piece, t, k in exp["repaired"]:          # the piece is saved before _handle_nans, the table after
        assert np.isnan(lv[piece][t, k]) and np.isfinite(lv[table][t, k]), (table, piece, t, k)
    for table, k in exp["dropped"]:                     # absent from EVERY step's integral
        assert np.isnan(lv[table][:, k]).all(), (table, k)
        assert np.isfinite(lv[table]).sum(axis=1).min() >= 2, table         # ... and levels are left to integrate over


def test_moving_case_really_loses_and_repairs_levels():
    dom, limits, exp = sc.build(sc.MOVING_ID)
    dTdt = o.moving_dTdt(dom)
    tabs = {}
    with np.errstate(invalid="ignore"):
        for t in range(dom.time_s.size):
            sub = o.Domain(dom.tair[t:t + 1], dom.u[t:t + 1], dom.v[t:t + 1], dom.omega[t:t + 1], dom.geopt[t:t + 1], dom.lat, dom.lon,
                           dom.level, dom.time_s[t:t + 1])
            b = o.make_box(sub, *limits[t], dTdt=dTdt[t:t + 1], fixed=False)
            tabs[t] = (b, o.all_terms(b)[1])
    for field, t, k, rows in exp["za_nan"]:
        assert _nan_rows(tabs[t][0], field, 0, k) == rows, (field, t, k)
    for table, piece, t, k in exp["repaired"]:
        assert np.isnan(tabs[t][1][piece][0, k]) and np.isfinite(tabs[t][1][table][0, k]), (table, piece, t, k)
    for table, t, k in exp["dropped"]:                  # one BoxData per step: that step alone loses the level
        assert np.isnan(tabs[t][1][table][0, k]), (table, t, k)
        assert all(np.isfinite(tabs[s][1][table][0, k]) for s in tabs if s != t), (table, t, k)


@pytest.mark.parametrize("case", sc.MANY_CLEAN_IDS + (sc.MANY_NAN_ID,))
def test_many_level_cases_exercise_the_sigma_clamp_without_it_deciding_the_result(case):
    dom, limits, exp = sc.build(case)
    assert exp["clamp"] and dom.level.size >= 64
    with np.errstate(invalid="ignore"):
        share = float(np.mean(o.make_box(dom, *limits).sigma_AA == 0.03))
    assert 0.0 < share < 0.1, share


def test_extended_interpolation_follows_np_interp():
    """np.interp refuses np.longdouble, so the oracle interpolates such values itself (``_interp_wide``): on float64 data it must give
    np.interp's numbers -- gaps, nodes, both ends outside the valid range, one valid point."""
    rng = np.random.default_rng(5)
    p = np.linspace(10000.0, 100000.0, 23)
    for ok_idx in ([3, 4, 9, 15, 16, 20], [0, 22], [0, 1, 2, 21, 22], [7]):
        y = rng.standard_normal(len(ok_idx))
        want = np.interp(p, p[ok_idx], y, left=np.nan, right=np.nan)
        got = o._interp_wide(p.astype(np.longdouble), p[ok_idx].astype(np.longdouble), y.astype(np.longdouble))
        assert got.dtype == np.longdouble and np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.max(np.abs(got[ok].astype(np.float64) - want[ok])) <= 4 * np.finfo(np.float64).eps * np.max(np.abs(y))
        assert np.array_equal(got[ok_idx].astype(np.float64), y)


@pytest.mark.parametrize("case", sc.CLEAN_IDS)
def test_float64_oracle_lies_within_1e_11_of_the_extended_one(case):
    """Pins the reference of tests/test_gpu_stage2_edges.py: every term, budget, residual and level table of the float64 evaluation
    against the np.longdouble one."""
    dom, _, _ = sc.build(case)
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "np.longdouble is no wider than float64 on this platform"
    s64, l64 = sc.reference(case, extended=False)
    sld, lld = sc.reference(case, extended=True)
    worst = compare(s64, l64, sld, lld, REFERENCE_BAR, f"{case}: float64 vs extended oracle", time_s=dom.time_s)
    print(case, max(worst.values()))
