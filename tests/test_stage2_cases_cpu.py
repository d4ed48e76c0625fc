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


@pytest.mark.parametrize("case", sc.FIXED_IDS + sc.MOVING_IDS)
def test_every_term_is_finite_and_none_is_zero(case):
    """No case degenerates into "no level left" (a term that integrates an empty array is 0.0) or into a NaN."""
    s, _ = sc.reference(case)
    for name in SCALARS:
        assert np.isfinite(s[name]).all(), (case, name)
        assert np.any(s[name] != 0.0), (case, name)


@pytest.mark.parametrize("case", sc.TALL_CLEAN_IDS + sc.TALL_NAN_IDS + sc.AXES_FIXED_IDS)
def test_tall_boxes_have_the_intended_height_on_the_intended_side_of_64(case):
    dom, limits, exp = sc.build(case)
    iw, ie, js, jn = tables.box_indices(dom.lat, dom.lon, *limits)
    assert jn - js + 1 == exp["height"] and ie - iw + 1 >= 2
    assert exp["kernel"] == ("small" if exp["height"] <= 64 else "general")
    assert o.make_box(dom, *limits).idx == (iw, ie, js, jn)         # the oracle selects the same box


def test_moving_boxes_have_the_intended_heights(case=sc.MOVING_ID):
    """One buffer of 130 rows (general kernel) that holds a 64-row and a 2-row box: alone in a shard those take the small kernel."""
    dom, limits, exp = sc.build(case)
    boxes = [tables.box_indices(dom.lat, dom.lon, *lim) for lim in limits]
    assert boxes == exp["boxes"]
    assert [o.make_box(dom, *lim).idx for lim in limits] == boxes   # the oracle selects the same boxes
    assert len({b[2] for b in boxes}) == (5 if case == sc.AXES_MOVING_ID else 1)      # uneven latitudes: a start row, and tables, per box
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


def test_moving_case_really_loses_and_repairs_levels(case=sc.MOVING_ID):
    dom, limits, exp = sc.build(case)
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


@pytest.mark.parametrize("case", sc.MANY_CLEAN_IDS + (sc.MANY_NAN_ID, "axes_levels130", "axes_levels130_nan"))
def test_many_level_cases_exercise_the_sigma_clamp_without_it_deciding_the_result(case):
    dom, limits, exp = sc.build(case)
    assert exp["clamp"] and dom.level.size >= 64
    with np.errstate(invalid="ignore"):
        share = float(np.mean(o.make_box(dom, *limits).sigma_AA == 0.03))
    assert 0.0 < share < 0.1, share


def test_extended_interpolation_follows_np_interp(p=None):
    """np.interp refuses np.longdouble, so the oracle interpolates such values itself (``_interp_wide``): on float64 data it must give
    np.interp's numbers -- gaps, nodes, both ends outside the valid range, one valid point."""
    rng = np.random.default_rng(5)
    p = np.linspace(10000.0, 100000.0, 23) if p is None else p
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


# ---------------------------------------------------------------------------------------------------------------------------------
# the axes family: uneven latitudes and pressure levels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.AXES_FIXED_IDS + (sc.AXES_MOVING_ID,))
def test_axes_cases_have_no_two_neighbouring_intervals_alike(case):
    """Every interior latitude of the box(es) and every interior level: the intervals either side differ by 5 % of the longer one or
    more, recomputed here from the axes; nothing lies above the data's top level, 10 000 Pa."""
    dom, limits, exp = sc.build(case)
    boxes = [tables.box_indices(dom.lat, dom.lon, *lim) for lim in (limits if case == sc.AXES_MOVING_ID else [limits])]
    rel = lambda x: np.abs(np.diff(x, 2)) / np.maximum(np.diff(x)[1:], np.diff(x)[:-1])
    lat = min(rel(dom.lat[js:jn + 1]).min() for _, _, js, jn in boxes if jn - js >= 2)
    assert np.all(np.diff(dom.lat) > 0) and np.all(np.diff(dom.level) > 0) and dom.level[0] == 10000.0 and dom.level[-1] == 100000.0
    assert exp["asymmetry"]["lat"] == pytest.approx(lat, rel=1e-9) and exp["asymmetry"]["level"] == pytest.approx(rel(dom.level).min(), rel=1e-9)
    assert exp["asymmetry"]["lat"] >= 0.05 and exp["asymmetry"]["level"] >= 0.05, exp["asymmetry"]
    for iw, ie, js, jn in boxes:                        # one grid point inside the grid on every side
        assert iw == 1 and ie == dom.lon.size - 2 and js >= 1 and jn <= dom.lat.size - 2


def test_axes_moving_boxes_have_the_intended_heights_and_rows():
    test_moving_boxes_have_the_intended_heights(sc.AXES_MOVING_ID)


def test_axes_moving_case_really_loses_and_repairs_levels():
    test_moving_case_really_loses_and_repairs_levels(sc.AXES_MOVING_ID)


def test_extended_interpolation_follows_np_interp_on_uneven_pressures():
    p = sc.uneven_axis(10000.0, 100000.0, 23)
    assert sc.interval_asymmetry(p) >= 0.05
    test_extended_interpolation_follows_np_interp(p)


def test_even_cases_have_the_symmetry_the_axes_family_removes():
    assert sc.interval_asymmetry(sc.build("tall131")[0].lat) < 1e-12 and sc.interval_asymmetry(sc.build("levels129")[0].level) < 1e-12


# Plausible wrong forms of the oracle's functions: each is what a stage 2 that is right on even axes and wrong on uneven ones computes.
def _two_point(y, x, axis):
    """np.gradient with the interior taken as (f[i+1] - f[i-1]) / (x[i+1] - x[i-1]): the middle coefficient dropped."""
    g = np.moveaxis(np.array(np.gradient(y, x, axis=axis, edge_order=1)), axis, 0)
    f = np.moveaxis(np.asarray(y), axis, 0)
    h = (x[2:] - x[:-2]).reshape((-1,) + (1,) * (f.ndim - 1))
    g[1:-1] = (f[2:] - f[:-2]) / h
    return np.moveaxis(g, 0, axis)


def _mutant(kind):
    real_diff, real_trapz, real_fill = o.differentiate, o.trapz, o.interpolate_and_drop_nan_levels

    def diff_lat(y, x, axis):                           # the meridional derivatives of stage 2: axis 2 of [t, k, lat] arrays
        return _two_point(y, x, axis) if (axis == 2 and np.ndim(y) == 3) else real_diff(y, x, axis)

    def diff_level(y, x, axis):
        return _two_point(y, x, axis) if axis == 1 else real_diff(y, x, axis)

    def fill_by_index(f, p):                            # gaps interpolated in level index, not in pressure
        fc, kept = real_fill(f, np.arange(len(p), dtype=p.dtype))
        return fc, p[np.asarray(kept).astype(int)]

    def even_weights(which):                            # every interval of the trapezoid set to the mean interval
        def trapz(y, x, axis):
            if axis == which and len(x) > 2:
                x = np.linspace(x[0], x[-1], len(x))
            return real_trapz(y, x, axis)
        return trapz

    return {"d/dphi": ("differentiate", diff_lat), "d/dp": ("differentiate", diff_level), "gaps": ("interpolate_and_drop_nan_levels", fill_by_index),
            "trapz p": ("trapz", even_weights(1)), "trapz phi": ("trapz", even_weights(2))}[kind]


DP_TERMS = ("Az", "Ae", "Ca", "Ck", "BAz", "BAe", "Gz", "Ge")
MUTANTS = [(kind, case, even, terms) for kind, cases, terms in (
    ("d/dphi", (("axes_small", "tall63"), ("axes_tall131", "tall131")), ("Ca", "Ck")),
    ("d/dp", (("axes_small", "tall63"), ("axes_tall131", "tall131"), ("axes_levels130", "levels129")), DP_TERMS),
    ("gaps", (("axes_tall131_nan", "tall131_interior_T_row100"), ("axes_small_nan", "tall131_seam_omega"), ("axes_levels130_nan", "levels130_nan")), None),
    ("trapz p", (("axes_levels130", "levels129"),), tuple(SCALARS)),
    ("trapz phi", (("axes_tall131", "tall131"),), tuple(SCALARS))) for case, even in cases]
MUTANT_MOVES = 1e-6         # of the term's scale: 1000 x the GPU tests' bar of 1e-9


@pytest.mark.parametrize("kind,case,even,terms", MUTANTS, ids=[f"{m[0]}-{m[1]}" for m in MUTANTS])
def test_the_axes_cases_tell_a_wrong_stage_2_from_a_right_one(monkeypatch, kind, case, even, terms):
    """The float64 oracle once more with one function exchanged for a plausible wrong form: on the axes case every listed term moves by
    1e-6 of its scale or more -- a thousand times the GPU tests' bar -- and on the corresponding even-axis case nothing moves beyond the
    reference's own rounding (REFERENCE_BAR; an even-axis gap is one level deep there, where index and pressure give the same
    midpoint).  ``terms`` None: the terms whose tables the case names in ``repaired``."""
    from tests.helpers import as_f64, scale_err
    moved = {}
    for cid in (case, even):
        dom, limits, exp = sc.build(cid)
        base, _ = sc.reference(cid, extended=False)
        with monkeypatch.context() as m, np.errstate(invalid="ignore"):
            m.setattr(o, *_mutant(kind))
            wrong, _ = o.lec_fixed(as_f64(dom), *limits)
        moved[cid] = {k: scale_err(wrong[k], base[k]) for k in SCALARS}
    listed = terms if terms is not None else tuple(sorted({r[0] for r in sc.build(case)[2]["repaired"]}))
    print(kind, case, {k: f"{moved[case][k]:.1e}" for k in listed}, "| even:", even, f"{max(moved[even].values()):.1e}")
    assert listed and all(moved[case][k] >= MUTANT_MOVES for k in listed), {k: moved[case][k] for k in listed if not moved[case][k] >= MUTANT_MOVES}
    assert max(moved[even].values()) <= REFERENCE_BAR, moved[even]
    s, _ = sc.reference(case, extended=False)           # the oracle is itself again
    again, _ = o.lec_fixed(as_f64(sc.build(case)[0]), *sc.build(case)[1])
    assert all(np.array_equal(again[k], s[k]) for k in SCALARS)
