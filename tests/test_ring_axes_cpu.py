"""The cases of tests/ring_axes_cases.py, checked on the oracle and the restatements alone: the axes are as uneven as they claim, the
static-stability clamp is far from binding, the restatements of the sections and maps close on ``oracle.all_terms`` on every domain (ring
and open box), the references MOVE when np.gradient's interior is replaced by the plain centred difference on one axis -- a defect that
is invisible on the even axes of the sibling tests --, and the NaN case changes the terms at the steps it says.  No kernel is run here;
tests/test_gpu_ring_axes.py holds the kernels to these references.  Run with -s for the measured figures.

Measured: asymmetry of the band's latitudes 0.21 .. 0.25, of the levels 0.21 .. 0.25, of the time triples 0.56; least sigma_AA 0.42 ..
0.50; closures at most 3.8e-15 of scale; the mutant's shifts, for the entries of SHIFT_ENTRIES: latitude 2.2e-3 (Gz of the sections) ..
0.22 (Ca), level 2.8e-2 (Ge(n) row shares) .. 1.0 (Ge), time 0.52 .. 0.66; on ``ring_domain``'s own axes every shift is at most 3e-16."""
import contextlib

import numpy as np
import pytest

from oracle import lec_oracle as o
from tests import maps_restatement as mr
from tests import ring_axes_cases as ra
from tests import rowstats_cases as rc
from tests import rowstats_restatement as rs
from tests import sections_restatement as sr
from tests import spectrum_ge_restatement as gr
from tests import spectrum_nl_restatement as nr
from tests.helpers import as_f64
from tests.stage2_cases import interval_asymmetry

CLOSE = 1e-11                     # the project's closure bar, of the term's scale
SHIFT_FLOOR = 1e-4                # what the mutant must move every listed entry by: 1e5 x the GPU parity bar of 1e-9
REFERENCE_BAR = 1e-12             # the float64 record restatement against the extended one (tests/test_rowstats_cases_cpu.py)
N_WAVE = 8
ALL_CASES = [c + s for c in ra.CLEAN_IDS for s in ("", "_open")]
# axis: ({product: the terms that must move}, the row-share records that must move)
SHIFT_ENTRIES = {"latitude": ({"sections": ("Ca", "Ck", "Gz", "Ge"), "maps": ("Ca", "Ck", "Ge")}, ("S/L", "Ge(n)")),
                 "level": ({"sections": ("Az", "Ae", "Ca", "Ck", "Gz", "Ge"), "maps": ("Ae", "Ca", "Ck", "Ge")}, ("S/L", "Ge(n)")),
                 "time": ({"sections": ("Gz", "Ge"), "maps": ("Ge",)}, ("Ge(n)",))}


def _scale(ref, axes):
    a = np.where(np.isnan(ref), -np.inf, np.abs(ref)).max(axis=axes, keepdims=True)
    return np.where(np.isfinite(a), a, 1.0)


def _err(got, ref, axes):
    """max |got - ref| over the term's scale (its largest |value| over ``axes``), per term along axis 1; NaN at the same places."""
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref) / _scale(ref, axes)
    return np.nanmax(np.where(np.isnan(e), 0.0, e), axis=tuple(a for a in range(ref.ndim) if a != 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# the axes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ra.CLEAN_IDS)
def test_axes_are_uneven_and_band_local(name):
    dom, box, exp = ra.build(name)
    js, jn = box[2], box[3]
    a = exp["asymmetry"]
    print(f"{name}: asymmetry lat {a['lat']:.3f}, level {a['level']:.3f}, time {a['time']:.3f}")
    assert a["lat"] == interval_asymmetry(dom.lat[js:jn + 1]) >= 0.15 and a["level"] == interval_asymmetry(dom.level) >= 0.15
    assert a["time"] == rc.asymmetry(rc.gradient_triples(dom.time_s)) >= 0.3
    assert 0 < js and jn < dom.lat.size - 1 and exp["nyb"] == jn - js + 1
    # band-local against cube-global: np.gradient is one-sided at the band's edge rows and centred there on the cube's axis, so a kernel
    # that takes row js + jb's coefficients from the cube's axis is wrong at both edges
    one_sided = lambda x, i, k: np.array([-1.0, 1.0]) / (x[k] - x[i])
    cube = rc.gradient_triples(dom.lat)                                       # row j of the cube: cube[j - 1]
    for edge, (i, k) in ((js, (js, js + 1)), (jn, (jn - 1, jn))):
        assert abs(cube[edge - 1][1]) > 0.05 * np.abs(one_sided(dom.lat, i, k)).max()          # the cube's triple has a middle term there
    # ... and the interior triples of the band are those of the cube's rows js + 1 .. jn - 1, none alike
    band = rc.gradient_triples(dom.lat[js:jn + 1])
    assert np.array_equal(band, cube[js:jn - 1]) and len({tuple(t) for t in band}) == len(band)


@pytest.mark.parametrize("case_id", ALL_CASES)
def test_the_frame_is_nan_and_the_box_is_clean(case_id):
    dom, (iw, ie, js, jn), exp = ra.build(case_id)
    for n in ra.FIELDS:
        a = getattr(dom, n)
        inside = np.zeros(a.shape, dtype=bool)
        inside[:, :, js:jn + 1, iw:ie + 1] = True
        assert np.isnan(a[~inside]).all() and np.isfinite(a[inside]).all(), n
    assert exp["ring"] == (iw == 0 and ie == dom.lon.size - 1) and exp["nxb"] == ie - iw + 1


@pytest.mark.parametrize("case_id", ALL_CASES)
def test_clamp_does_not_bind(case_id):
    b, _ = ra.reference(case_id)
    print(f"{case_id}: least sigma_AA {b.sigma_AA.min():.3f}")
    assert b.sigma_AA.min() >= 0.3


# ---------------------------------------------------------------------------------------------------------------------------------
# closure on the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ALL_CASES + [ra.F32_ID + "_open"])
def test_restatements_close_on_the_oracle(case_id):
    b, r = ra.reference(case_id)
    ring = ra.build(case_id)[2]["ring"]
    scalars, _ = o.all_terms(b)
    sec = np.stack([np.asarray(scalars[t], dtype=np.float64) for t in sr.TERMS], axis=1)              # [T, 10]
    cw = sr.area_weights(b)
    e_sec = _err((r["Xc"] * cw).sum(axis=-1), sec, (0,))
    e_map = _err(mr.zonal_average(r["H"], b, ring), sec[:, [sr.TERMS.index(t) for t in mr.TERMS]], (0,))
    print(f"{case_id}: sections close on all_terms to {e_sec.max():.1e}, the maps' Hovmoeller to {e_map.max():.1e} of scale")
    assert e_sec.max() <= CLOSE and e_map.max() <= CLOSE


# ---------------------------------------------------------------------------------------------------------------------------------
# sensitivity: the centred-difference mutant
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def centred_difference_on(coords):
    """np.gradient with its interior replaced by (f[i+1] - f[i-1]) / (x[i+1] - x[i-1]) wherever it is called with one of the coordinate
    arrays ``coords``: np.gradient itself on an even axis, and np.gradient without its middle coefficient, with the outer two of a
    wrong size, on an uneven one."""
    real = np.gradient

    def wrong(y, *varargs, axis=None, edge_order=1):
        g = real(y, *varargs, axis=axis, edge_order=edge_order)
        if len(varargs) != 1 or np.ndim(varargs[0]) != 1 or not isinstance(axis, (int, np.integer)):
            return g
        x = np.asarray(varargs[0])
        if not any(x.shape == c.shape and np.array_equal(x, c) for c in coords):
            return g
        g = np.array(g)
        gm, ym = np.moveaxis(g, axis, 0), np.moveaxis(np.asarray(y), axis, 0)
        gm[1:-1] = (ym[2:] - ym[:-2]) / (x[2:] - x[:-2]).reshape((-1,) + (1,) * (ym.ndim - 1))
        return g

    np.gradient = wrong
    try:
        yield
    finally:
        np.gradient = real


def _products(case_id, dom=None):
    """What the GPU tests compare with, on the case's box: per-step sections, the maps' columns, the S/L and Ge(n) row shares."""
    d, box, exp = ra.build(case_id)
    d = as_f64(d if dom is None else dom)
    south, north = ra.limits_of(d, box)
    r = ra.restate(ra.oracle_box(case_id, dom), exp["ring"])
    with np.errstate(invalid="ignore"):
        return {"sections": r["X"], "maps": r["C"], "S/L": nr.row_shares(d, south, north, N_WAVE)[0], "Ge(n)": gr.row_shares_q(d, south, north, N_WAVE)}


def _shifts(case_id, axis, dom=None):
    d, box, _ = ra.build(case_id)
    d = d if dom is None else dom
    lat = np.asarray(d.lat[box[2]:box[3] + 1], dtype=np.float64)
    coords = {"latitude": [lat, np.deg2rad(lat)], "level": [np.asarray(d.level, dtype=np.float64)], "time": [np.asarray(d.time_s, dtype=np.float64)]}[axis]
    ref = _products(case_id, dom)
    with centred_difference_on(coords):
        got = _products(case_id, dom)
    out = {}
    for what, terms, axes in (("sections", sr.TERMS, (0, 2, 3)), ("maps", mr.TERMS, (0, 2, 3))):
        out[what] = dict(zip(terms, _err(got[what], ref[what], axes)))
    for what in ("S/L", "Ge(n)"):
        out[what] = float(np.abs(got[what] - ref[what]).max() / np.abs(ref[what]).max())
    return out


@pytest.mark.parametrize("axis", list(SHIFT_ENTRIES))
def test_the_references_see_a_centred_difference(axis):
    """On ``narrow`` every entry the mutant can reach moves by SHIFT_FLOOR of its scale or more; on ``ring_domain``'s own axes (printed,
    not asserted: it documents the blind spot) by nothing."""
    terms, records = SHIFT_ENTRIES[axis]
    s = _shifts("narrow", axis)
    blind = _shifts("narrow", axis, dom=ra.framed(ra.even("narrow"), ra.build("narrow")[1], True))
    fmt = lambda m: ", ".join(f"{k} {v:.1e}" for k, v in m.items())
    low = {}
    for what, names in terms.items():
        print(f"{axis} mutant, {what}: {fmt({k: s[what][k] for k in names})}   [even axes: {fmt({k: blind[what][k] for k in names})}]")
        low.update({f"{what} {k}": s[what][k] for k in names if not s[what][k] >= SHIFT_FLOOR})
    for what in records:
        print(f"{axis} mutant, {what} row shares: {s[what]:.1e}   [even axes: {blind[what]:.1e}]")
        if not s[what] >= SHIFT_FLOOR:
            low[what] = s[what]
    assert not low, (axis, low)


def test_the_mutant_is_np_gradient_on_an_even_axis():
    x, y = np.linspace(0.0, 3.0, 7), np.random.default_rng(0).standard_normal((7, 3))
    with centred_difference_on([x]):
        got = np.gradient(y, x, axis=0, edge_order=1)
    assert np.abs(got - np.gradient(y, x, axis=0, edge_order=1)).max() <= 1e-15 * np.abs(got).max()


# ---------------------------------------------------------------------------------------------------------------------------------
# the NaN case
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("suffix", ["", "_open"])
def test_nan_case_changes_each_term_at_its_own_steps(suffix):
    dom, box, exp = ra.build(ra.NAN_ID + suffix)
    plain = ra.build("narrow" + suffix)[0]
    for field, at in exp["plants"]:
        a, c = getattr(dom, field), getattr(plain, field)
        assert np.isnan(a[at]).all() and np.isfinite(c[at]).all()
        assert int(np.isnan(a).sum()) == int(np.isnan(c).sum()) + int(np.size(a[at]))          # the plants lie inside the box
    _, r = ra.reference(ra.NAN_ID + suffix)
    _, r0 = ra.reference("narrow" + suffix)
    assert np.isfinite(r["Xc"]).all() and np.isfinite(r["C"]).all() and np.isfinite(r["H"]).all()
    assert np.isnan(r["X"]).any()                          # ... while the sections themselves hold NaN levels: bridged or trimmed
    for what, terms, key in (("sections", sr.TERMS, "Xc"), ("maps", mr.TERMS, "C")):
        changed = {t: {s for s in range(ra.NT) if not np.array_equal(r[key][s, i], r0[key][s, i])} for i, t in enumerate(terms)}
        print(f"narrow_nan{suffix}, {what}: steps at which a term's columns differ from the clean case's {changed}")
        assert changed == {t: exp["changed"][t] for t in terms}, what
    assert len({frozenset(exp["changed"][t]) for t in mr.TERMS}) >= 5          # the per-term states of the level march do diverge


# ---------------------------------------------------------------------------------------------------------------------------------
# records: the float64 restatement against the extended one, in the measure of tests/test_rowstats_cases_cpu.py
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ra.RECORD_IDS)
def test_record_reference_against_itself(case_id):
    dom, boxes, kw, exp = ra.records_build(case_id)
    assert min(exp["asymmetry"].values()) > 0.05 and kw["kind"] == "ring" and kw["runs"] == ra.RECORD_RUNS
    r64, rld = ra.records_reference(case_id, False)[(0, 4)][0], ra.records_reference(case_id, True)[(0, 4)][0]
    assert np.isfinite(rld).all() and np.array_equal(r64[..., rs.EDGES], rld[..., rs.EDGES])
    m = float(rc.moment_error(r64, rld).max())
    mean = rc.mean_error(r64, rld, rc.row_max(dom, boxes[0]), dom.lon.size)
    print(f"{case_id}: float64 restatement within {m:.2e} of the extended one in slots 5..21, means {mean:.2f} of their bound")
    assert m <= REFERENCE_BAR and mean <= 1.0
