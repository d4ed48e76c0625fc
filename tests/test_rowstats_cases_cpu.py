"""The cases of tests/rowstats_cases.py and the restatement of tests/rowstats_restatement.py, checked on the CPU alone: the reference
against itself in float64, the slot definitions against the pinned oracle's level tables, every case against what it claims about the
kernels' control flow, and the cases' power to see the errors they exist for (deliberately wrong variants of the float64 restatement;
no altered kernel is built or run).  Run with -s for the coverage sets and the measured figures."""
import contextlib

import numpy as np
import pytest

from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests import rowstats_cases as rc
from tests import rowstats_restatement as rs
from tests.helpers import as_f64, as_longdouble, scale_err

# The float64 restatement against the extended-precision one, slots 5..21 in the measure of the GPU test (of the statistic's largest
# value over the case's rows): a CONDITION on the cases, a tenth of the GPU bar.  Measured worst over all cases: 6.4e-13 (ring-256-float32-noq).
REFERENCE_BAR = 1e-12
# The means of the float64 restatement cannot be asked for a tenth of THEIR bound: its trapezoid weights come from float64 radians,
# each rounded by up to 2^-53 |lambda|, and the bound assumes exact weights -- which is why every domain starts at longitude 0 and
# narrow boxes stay near it (rowstats_cases._domain, _step_boxes).  They are held to the bound itself.  Measured worst: 0.61.
REFERENCE_MEAN_BOUND = 1.0
# conditioning: the float64 shifted sums (shifted_records) against the extended-precision restatement at the R the cases use, in the
# measure of slots 5..21; the rule asks for less than a tenth of the 1e-11 bar.  {case: measured}
COND_MEASURED = {"cond-a": 4.3e-15, "cond-b": 7.7e-13, "cond-c": 6.2e-13}
SEES = 100 * rc.GPU_BAR           # what a wrong variant must exceed in some statistic of some case


def _each_box(case_id, extended):
    """(label, records, box, first step) of every box of a case: a fixed box once per cube, a per-step box per step, a track's per step."""
    dom, boxes, kw, _ = rc.build(case_id)
    ref = rc.reference(case_id, extended)
    for plant, r in (ref.items() if "plants" in kw else [(None, ref)]):
        d = dom if plant is None else rc.planted(dom, next(p for p in kw["plants"] if p[0] == plant))
        if kw["kind"] == "steps":
            at = 0
            for (steps, bs), tr in zip(kw["tracks"], r):
                for i, b in enumerate(bs):
                    yield f"track box {at}", tr[i:i + 1, :, :b[3] - b[2] + 1], b, rc.track_domain(d, steps), i
                    at += 1
        elif isinstance(r, dict):
            for c, recs in r.items():
                for b, rec in zip(boxes, recs):
                    yield f"{plant} {c} {b}", rec, b, rc.steps_of(d, *c), 0
        else:
            for t, b in enumerate(boxes):
                yield f"{plant} step {t}", r[t:t + 1, :, :b[3] - b[2] + 1], b, d, t


@pytest.mark.parametrize("family", sorted(rc.FAMILY_IDS))
def test_reference_against_itself(family):
    """reference(extended=False), the same functions in float64, lies within REFERENCE_BAR of reference(extended=True) for every case."""
    worst, worst_mean, where = 0.0, 0.0, None
    for case_id in rc.FAMILY_IDS[family]:
        got, ref = [], []
        for (what, r64, b, d, t), (_, rld, _, _, _) in zip(_each_box(case_id, False), _each_box(case_id, True)):
            got.append(r64.reshape(-1, rs.NSLOT)); ref.append(rld.reshape(-1, rs.NSLOT))
            n = r64.shape[0]
            worst_mean = max(worst_mean, rc.mean_error(r64, rld, rc.row_max(d, b, t, t + n), b[1] - b[0] + 1))
            assert np.array_equal(np.isnan(r64), np.isnan(rld)), (case_id, what)
            e = ~np.isnan(rld[..., rs.EDGES])
            assert np.array_equal(r64[..., rs.EDGES][e], rld[..., rs.EDGES][e]), (case_id, what)
        m = float(rc.moment_error(np.concatenate(got), np.concatenate(ref)).max())
        if m > worst:
            worst, where = m, case_id
    print(f"{family}: float64 restatement within {worst:.2e} of the extended one in slots 5..21 ({where}); means {worst_mean:.2f} of their bound")
    assert worst <= REFERENCE_BAR and worst_mean <= REFERENCE_MEAN_BOUND


# ---------------------------------------------------------------------------------------------------------------------------------
# the slot definitions against the oracle's level tables
# ---------------------------------------------------------------------------------------------------------------------------------
def _terms_from_records(rec, b):
    """A handful of the oracle's level tables recombined from records with plain NumPy: Ke and Kz, Ca's [v'T'] piece (Ca_1), Ge."""
    S = rs.SLOT
    aa = lambda X: o.area_average(X, b.rlats, b.coslats)
    sig = b.sigma_AA
    tae = rec[..., S["MT"]] - aa(rec[..., S["MT"]])[..., None]
    dphi = o.differentiate(tae * b.coslats[None, None, :], b.rlats, axis=2)
    return {"Ke": aa(rec[..., S["UU"]] + rec[..., S["VV"]]), "Kz": aa(rec[..., S["MU"]] ** 2 + rec[..., S["MV"]] ** 2),
            "Ca_1": aa(rec[..., S["VT"]] * dphi / (2 * o.RE * sig[..., None])), "Ge": aa(rec[..., S["QT"]]) / (o.CP_D * sig)}


def _oracle_tables(b):
    return {**{k: v for k, v in o.energy_contents(b)[1].items() if k in ("Ke", "Kz")}, "Ca_1": o.conversion_terms(b)[1]["Ca_1"],
            "Ge": o.generation_terms(b)[1]["Ge"]}


def _tie(what, rec, b):
    got, ref = _terms_from_records(rec, b), _oracle_tables(b)
    worst = {k: scale_err(np.asarray(got[k], dtype=np.float64), ref[k]) for k in ref}
    print(f"{what}: recombined level tables within {max(worst.values()):.2e} of the oracle's")
    assert max(worst.values()) <= REFERENCE_BAR, (what, worst)


def test_restatement_against_the_oracles_terms_fixed():
    case_id = "sweep-f64v2-s1-stencil"
    dom, boxes, _, _ = rc.build(case_id)
    i = next(i for i, b in enumerate(boxes) if b[1] - b[0] + 1 == 130)
    _tie("fixed", rc.reference(case_id)[(0, 4)][i], o.make_box(as_longdouble(dom), *rc.limits_of(dom, boxes[i])))


def test_restatement_against_the_oracles_terms_moving():
    case_id = "tile-float64-nb-even-nl10-narrow"
    dom, boxes, _, _ = rc.build(case_id)
    d, ref = as_longdouble(dom), rc.reference(case_id)
    dT = o.moving_dTdt(d)
    for t in (0, 7, len(boxes) - 1):
        sub = o.Domain(d.tair[t:t + 1], d.u[t:t + 1], d.v[t:t + 1], d.omega[t:t + 1], d.geopt[t:t + 1], d.lat, d.lon, d.level, d.time_s[t:t + 1])
        b = o.make_box(sub, *rc.limits_of(dom, boxes[t]), dTdt=dT[t:t + 1], fixed=False)
        _tie(f"moving step {t}", ref[t:t + 1, :, :boxes[t][3] - boxes[t][2] + 1], b)


def test_restatement_against_the_oracles_terms_ring():
    case_id = "ring-65-float64-stencil"
    dom, boxes, _, _ = rc.build(case_id)
    _tie("ring", rc.reference(case_id)[(0, 3)][0], rr.ring_box(as_longdouble(dom), dom.lat[boxes[0][2]], dom.lat[boxes[0][3]]))


# ---------------------------------------------------------------------------------------------------------------------------------
# every case is what it claims
# ---------------------------------------------------------------------------------------------------------------------------------
def _walk(vec, shift, nxb):
    """The trip loop of lec_rowsweep_kernel, lane by lane: (trips launched, [kind of each trip], trip and lane of the row's last element).
    Asserts that the lanes that take part cover every element once and that a middle trip lies strictly inside the row."""
    nvec = (nxb + vec - 1) // vec + (1 if vec > 1 else 0)
    ntrips = (nvec + 63) // 64
    e0_last = ((nxb - 1 + shift) // vec) * vec - shift
    mid_end = 1 if ntrips == 1 else min((nxb - 1 + shift) // (64 * vec), ntrips)
    kinds = ["edge"] + ["middle"] * max(mid_end - 1, 0) + ["edge"] * (ntrips - max(mid_end, 1))
    seen, last = np.zeros(nxb, dtype=int), None
    for it, kind in enumerate(kinds):
        for lane in range(64):
            e0 = it * 64 * vec - shift + lane * vec
            if kind == "edge" and e0 > e0_last:
                continue
            for e in range(e0, e0 + vec):
                if kind == "middle":
                    assert 1 <= e <= nxb - 2
                if 0 <= e < nxb:
                    seen[e] += 1
                    if e == nxb - 1:
                        last = (it, lane)
    assert np.all(seen == 1)
    return ntrips, kinds, last


def _classes(ntrips, kinds, last):
    return ("one" if ntrips == 1 else ("middle" if "middle" in kinds else "two")), {0: "0", 63: "63"}.get(last[1], "other")


def test_sweep_cases_are_what_they_claim_and_complete():
    """The restated launch rule against a lane-by-lane walk of the trip loop; every (form, shift) crosses every combination of {one
    trip, two trips, a middle trip} x {last element in lane 0, lane 63, elsewhere} that some width can reach, in the full set; every
    further mode crosses the three trip structures."""
    vecs = {"f64v2": 2, "f64v1": 1, "f32v4": 4, "f32v2": 2, "f32v2forced": 2, "f32v1": 1}
    seen = {}
    for case_id in rc.FAMILY_IDS["sweep"]:
        _, form, s, mode = case_id.split("-")
        dom, boxes, kw, exp = rc.build(case_id)
        assert dom.tair.dtype == (np.float64 if form.startswith("f64") else np.float32)
        assert kw["tuning"]["kernel"] == ("two_sweep" if mode == "twosweep" else "row_sweep") and rc.tables_uniform(dom.lon) == (mode not in ("table", "twosweep"))
        if mode == "twosweep":          # another kernel: only the row's alignment and widths carry over
            continue
        for b, e in zip(boxes, exp):
            assert e["vec"] == vecs[form] and e["shift"] == int(s[1:]) == (b[0] % e["vec"]) and b[0] >= 1 and b[1] <= dom.lon.size - 2
            ntrips, kinds, last = _walk(e["vec"], e["shift"], e["nxb"])
            assert (ntrips, last) == (e["ntrips"], (e["last_trip"], e["last_lane"])) and e["one_trip"] == (ntrips == 1)
            assert (e["trips"], e["lane"]) == _classes(ntrips, kinds, last)
            seen.setdefault((form, e["shift"], mode), set()).add((e["trips"], e["lane"]))
    for (form, shift, mode), got in sorted(seen.items()):
        if mode == "stencil":
            reach = {_classes(*_walk(vecs[form], shift, w)) for w in range(2, 64 * vecs[form] * 3 + vecs[form] + 2)}
            print(f"sweep {form} shift {shift}: {sorted(got)}")
            assert got == reach and {t for t, _ in got} == {"one", "two", "middle"} and {l for _, l in got} == {"0", "63", "other"}, (form, shift, reach - got)
        else:
            assert {t for t, _ in got} == {"one", "two", "middle"}, (form, shift, mode)
    assert {k[:2] for k in seen} == {(f, s) for f, v in vecs.items() for s in range(v)}
    assert {k[2] for k in seen} == set(rc.SWEEP_MODES)


def test_block_cases_are_what_they_claim_and_complete():
    seen = set()
    for case_id in rc.FAMILY_IDS["block"]:
        dom, boxes, kw, exp = rc.build(case_id)
        assert kw["tuning"]["kernel"] == "row_block" and boxes[0][3] - boxes[0][2] + 1 == 5 and dom.level.size == 3
        # what lec_rowstats asks of a row-block call (block_ok), or it quietly runs one wave per row instead: all terms with dT/dt from
        # the cube, a geopotential cube, at least two processed steps
        assert kw["with_q"] and kw["with_phi"] and not kw["dtdt"] and all(r[3] >= 2 for r in kw["runs"])
        for b, e in zip(boxes, exp):
            assert e["vec"] == 2 and e["shift"] == b[0] % 2
            ntrips, kinds, last = _walk(2, e["shift"], e["nxb"])
            assert (e["trips"], e["lane"]) == _classes(ntrips, kinds, last)
            seen.add((dom.tair.dtype.name, e["shape"], e["shift"], e["trips"]))
            p = e["partial"]
            assert p["j"] == (e["shape"] % 10 == 2) and p["k"] == ((e["shape"] // 10) % 10 == 2) and all(p["t"]) == (e["shape"] // 100 == 2)
    print(f"block: {len(seen)} (dtype, shape, shift, trips) combinations")
    assert seen == {(d, s, sh, t) for d in ("float64", "float32") for s in rc.BLOCK_SHAPES for sh in (0, 1) for t in ("one", "two", "middle")}


def test_tile_and_plane_cases_are_what_they_claim_and_complete():
    """Box tiles: the windowed and the non-windowed form x storage / dT/dt mode / longitudes x levels x (own walk, one walk) are all
    reached; the narrow calls cross every height, start-column residue, grid edge and partial row group, the two calls together every
    width.  Box planes: as the narrow tile calls, with boxes that fill and do not fill their slab."""
    narrow = lambda e: (e["heights"] == list(range(2, 10)) and e["residues"] == [0, 1, 2, 3] and e["width_residues"] == [0, 1, 2, 3]
                        and e["edges"] == ["east", "north", "south", "west"] and e["partial_row_group"] == [0, 1, 2, 3] and e["row_groups"] == 3)
    reached, walks = set(), set()
    for case_id in rc.FAMILY_IDS["tile"]:
        dom, boxes, kw, e = rc.build(case_id)
        if kw["kind"] == "steps":
            assert e["tracks"] == 3 and e["same_step"] and e["two_steps_away"] and e["track_ends"] >= 1
            assert max(b[1] - b[0] + 1 for b in boxes) <= 64          # (a step table of narrow boxes: the WINDOW form)
            continue
        assert all(0 <= b[0] <= b[1] < dom.lon.size and 0 <= b[2] <= b[3] < dom.lat.size for b in boxes) and len(boxes) == dom.tair.shape[0]
        nl = dom.level.size
        assert e["window"] == (max(e["widths"]) <= 64) == (not e["wide"]) == case_id.endswith("narrow")
        assert e["widths"] == sorted(set(rc.TILE_NARROW if e["window"] else rc.TILE_WIDE)) and (narrow(e) if e["window"] else e["heights"] == list(range(2, 10)))
        assert e["walks"][nl] == nl <= 21 and e["walks"][0] < nl and [t.get("tile_j", 0) for t in kw["tunings"]] == [0, nl]
        walks.add((nl, e["walks"][0]))
        reached |= {(dom.tair.dtype.name, kw["mode"], rc.tables_uniform(dom.lon), nl, e["window"], tj) for tj in (0, nl)}
    print(f"tile: {len(reached)} (dtype, mode, even longitudes, levels, window, tile_j) combinations; (levels, levels per wave) {sorted(walks)}")
    assert reached == {(d, m, u, nl, w, tj) for d, m in rc.TILE_KINDS for u in (True, False) for nl in rc.TILE_LEVELS for w in (True, False) for tj in (0, nl)}
    assert set(rc.TILE_NARROW) | set(rc.TILE_WIDE) == set(rc.TILE_WIDTHS) and max(rc.TILE_NARROW) == 64 < 70 == max(rc.TILE_WIDE)
    kinds, walks = set(), set()
    for case_id in rc.FAMILY_IDS["plane"]:
        dom, boxes, kw, e = rc.build(case_id)
        nl = dom.level.size
        assert e["widths"] == sorted(rc.PLANE_WIDTHS) and narrow(dict(e, heights=list(range(2, 10)))) and e["heights"] == sorted(set(rc.PLANE_HEIGHTS))
        assert e["fills_slab_rows"] == [False, True] and e["fills_slab_columns"] == [False, True] and not e["wide"] and not e["window"]
        assert e["walks"][nl] == nl <= 42 and e["walks"][0] < nl and [t.get("tile_j", 0) for t in kw["tunings"]] == [0, nl]
        kinds.add(dom.tair.dtype.name)
        walks.add((nl, e["walks"][0]))
    print(f"plane: {sorted(kinds)}; (levels, levels per wave) {sorted(walks)}")
    assert kinds == {"float64", "float32"} and {w[0] for w in walks} == set(rc.PLANE_LEVELS)
    # the two launch rules differ where a launch is large: 512 steps of 61 rows, 37 levels -- 19 levels per wave against 10
    assert rc.tile_walk(37, 512, 61, 0, "tile") == 19 and rc.tile_walk(37, 512, 61, 0, "plane") == 10
    assert {e: rc.build(c)[3]["boxes"]["window"] for c, e in (("axes-tile", 1), ("axes-tilewide", 0))} == {1: True, 0: False}


def test_ring_axes_nan_and_conditioning_cases_are_what_they_claim():
    ring = {(rc.build(c)[3][0]["vec"], rc.build(c)[3][0]["trips"], rc.build(c)[3][0]["mode"]) for c in rc.FAMILY_IDS["ring"]}
    print(f"ring: {sorted(ring)}")
    assert {r[0] for r in ring} == {1, 2, 4} and {r[1] for r in ring} == {"one", "two", "middle"} and {r[2] for r in ring} == set(rc.RING_MODES)
    for case_id in rc.FAMILY_IDS["axes"]:
        asym = rc.build(case_id)[3]["asymmetry"]
        print(f"{case_id}: least asymmetry of the coefficient triples {({k: round(v, 3) for k, v in asym.items()})}")
        assert min(asym.values()) > 0.05, (case_id, asym)
    for case_id in rc.FAMILY_IDS["nan"]:
        dom, boxes, kw, e = rc.build(case_id)
        assert len(kw["plants"]) == 10
        if kw["kind"] == "fixed":
            assert e["trips"] == "middle" and e["shift"] == 1
            iw, ie = boxes[0][:2]
            mid = kw["plants"][1][2][3] - iw
            assert 64 * e["vec"] - 1 <= mid < 128 * e["vec"] - 1            # box element of the middle plant: in trip 1
        for name, fi, (t, k, j, i) in kw["plants"]:
            bx = boxes[0] if kw["kind"] == "fixed" else boxes[2]      # the box of the row looked at reads the point
            assert bx[0] <= i <= bx[1] and bx[2] <= j <= bx[3] and 0 <= k < dom.level.size and 0 <= t < dom.tair.shape[0], (case_id, name)
    assert [[e["trips"] for e in rc.build(c)[3]] for c in rc.FAMILY_IDS["conditioning"]] == [["one", "two", "middle"]] * 3


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases can see the errors they exist for
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _oracle_with(name, fn):
    keep = getattr(o, name)
    setattr(o, name, fn)
    try:
        yield
    finally:
        setattr(o, name, keep)


def _sees(what, pairs):
    worst = max(float(rc.moment_error(got, ref).max()) for got, ref in pairs)
    print(f"{what}: {worst / rc.GPU_BAR:.3g} x the GPU bar")
    assert worst >= SEES, what


def test_sweep_sees_full_weight_at_the_last_element():
    wrong = lambda X, rlons, xlength: (o.trapz(X, rlons, axis=-1) + 0.5 * (rlons[-1] - rlons[-2]) * X[..., -1]) / xlength
    case_id = "sweep-f64v2-s0-stencil"
    dom, boxes, kw, _ = rc.build(case_id)
    ref = rc.reference(case_id)[(0, 4)]
    with _oracle_with("zonal_average", wrong):
        pairs = [(rc.fixed_records(dom, boxes[i], kw, (0, 4), extended=False), ref[i]) for i in (0, 10, len(boxes) - 1)]
    assert all(float(rc.moment_error(g, r).max()) >= SEES for g, r in pairs)         # every width sees it, the widest too
    _sees("sweep, full weight at the last element", pairs)


def _east_centred(d, limits, limits_wide, dTdt=None):
    """float64 records of a box whose d T / d lambda at the east column is a centred difference that reads the neighbour beyond the box
    (0 there: the frame zeroed): Q of the box widened by one column, cut back."""
    b = o.make_box(d, *limits, dTdt=dTdt)
    with np.errstate(invalid="ignore", divide="ignore"):          # (T = 0 in the zeroed frame column: its own Q is cut away)
        Q = o.make_box(d, *limits_wide, dTdt=dTdt).f["Q"][..., :-1]
    za = o.zonal_average(Q, b.rlons, b.xlength)
    b.f.update(Q=Q, Q_ZA=za, Q_ZE=Q - za[..., None])
    return np.asarray(rs.records_of_box(b), dtype=np.float64)


def _zero_frame(dom, box):
    d = as_f64(dom)
    m = np.zeros(d.tair.shape[2:], dtype=bool)
    m[box[2]:box[3] + 1, box[0]:box[1] + 1] = True
    return o.Domain(*[np.where(m, a, 0.0) for a in (d.tair, d.u, d.v, d.omega, d.geopt)], d.lat, d.lon, d.level, d.time_s)


def test_sweep_and_tile_see_a_centred_difference_at_the_east_column():
    case_id = "sweep-f64v2-s0-stencil"
    dom, boxes, _, _ = rc.build(case_id)
    pairs = []
    for i in (0, 10, len(boxes) - 1):
        b = boxes[i]
        pairs.append((_east_centred(_zero_frame(dom, b), rc.limits_of(dom, b), rc.limits_of(dom, (b[0], b[1] + 1, b[2], b[3]))), rc.reference(case_id)[(0, 4)][i]))
    _sees("sweep, centred d/dlon at the east column", pairs)
    case_id = "tile-float64-cube-even-nl10-narrow"
    dom, boxes, _, _ = rc.build(case_id)
    dT, pairs = rc.dtdt_cube(dom), []
    for t, b in enumerate(boxes):
        if b[1] + 1 < dom.lon.size and len(pairs) < 3:
            z = rc.steps_of(_zero_frame(dom, b), t, t + 1)
            got = _east_centred(z, rc.limits_of(dom, b), rc.limits_of(dom, (b[0], b[1] + 1, b[2], b[3])), dTdt=dT[t:t + 1])
            pairs.append((got, rc.reference(case_id)[t:t + 1, :, :b[3] - b[2] + 1]))
    _sees("tile, centred d/dlon at the east column", pairs)


def _swapped_gradient(axis_of_4d):
    """np.gradient with the two outer coefficients of every interior point given to the wrong neighbour (each keeps the sign of its
    side) along one axis of a 4-D field: a f[i-1] + b f[i] + c f[i+1] becomes -c f[i-1] + b f[i] - a f[i+1].  On an even axis a = -c
    and nothing changes."""
    def wrong(y, x, axis):
        if np.ndim(y) != 4 or axis != axis_of_4d:
            return np.gradient(y, x, axis=axis, edge_order=1)
        g = np.moveaxis(np.array(np.gradient(y, x, axis=axis, edge_order=1)), axis, 0)
        ym, c = np.moveaxis(y, axis, 0), rc.gradient_triples(x)
        sh = (-1,) + (1,) * (ym.ndim - 1)
        g[1:-1] = -c[:, 2].reshape(sh) * ym[:-2] + c[:, 1].reshape(sh) * ym[1:-1] - c[:, 0].reshape(sh) * ym[2:]
        return np.moveaxis(g, 0, axis)
    return wrong


@pytest.mark.parametrize("table, axis", [("lattab", 2), ("levtab", 1), ("tcoef", 0)])
def test_axes_see_swapped_coefficients(table, axis):
    """Each axes case sees the swap; on an even axis the swapped form IS np.gradient (checked: the sweep family does not see it)."""
    refs = {c: rc.reference(c) for c in rc.FAMILY_IDS["axes"] + ("sweep-f64v2-s0-stencil",)}       # before the oracle is altered
    with _oracle_with("differentiate", _swapped_gradient(axis)):
        for case_id in rc.FAMILY_IDS["axes"]:
            dom, boxes, kw, _ = rc.build(case_id)
            if kw["kind"] == "fixed":
                pairs = [(rc.fixed_records(dom, boxes[-1], kw, (0, 4), extended=False), refs[case_id][(0, 4)][-1])]
            else:       # (the moving framework's dT/dt is formed before the boxes: differentiate is patched for it too)
                pairs = [(rc.moving_records(dom, boxes, kw, extended=False), refs[case_id])]
            _sees(f"{case_id}, {table} swapped", pairs)
        dom, boxes, kw, _ = rc.build("sweep-f64v2-s0-stencil")
        even = rc.fixed_records(dom, boxes[-1], kw, (0, 4), extended=False)
    assert float(rc.moment_error(even, refs["sweep-f64v2-s0-stencil"][(0, 4)][-1]).max()) <= REFERENCE_BAR


def shifted_records(dom, box, shifted=True):
    """Slots 0..21 of one fixed box from the 20 weighted sums about a shift c (the row's first element; ``shifted`` False: about 0), in
    float64 NumPy: the formulas of lec_rowsweep.hip's header comment -- a = T - cT, b = u - cU, c = v - cV, d = w - cW, e = Phi - cP,
    f = Q;  [x'y'] = <xy> - <x><y>;  [v x'x'] = <c xx> - 2 <x><c x> + <x>^2 <c> + cV [x'x'] (its [vT'T'], and term by term [Ev] =
    [v u'u'] + [v v'v']);  [Kv] = 2[u][u'v'] + [u]^2[v] + 2[v][v'v'] + [v]^3.  Q is the oracle's (float64)."""
    b = o.make_box(as_f64(dom), *rc.limits_of(dom, box))
    dx = np.diff(b.rlons)
    w = np.zeros(b.rlons.size)
    w[:-1] += 0.5 * dx
    w[1:] += 0.5 * dx
    w = w / b.xlength
    S = lambda X: np.sum(w * X, axis=-1)
    X = [b.f[n] for n in ("tair", "u", "v", "omega", "geopt")]
    cs = [x[..., 0] if shifted else np.zeros(x.shape[:-1]) for x in X]
    a, bb, c, d, e = [x - s[..., None] for x, s in zip(X, cs)]
    f = b.f["Q"]
    cV, cW = cs[2], cs[3]
    ma, mb, mc, md, me, mf = S(a), S(bb), S(c), S(d), S(e), S(f)
    cov = lambda x, y, mx, my: S(x * y) - mx * my
    TT, UU, VV = cov(a, a, ma, ma), cov(bb, bb, mb, mb), cov(c, c, mc, mc)
    UV, WU, WV = cov(bb, c, mb, mc), cov(d, bb, md, mb), cov(d, c, md, mc)
    third = lambda y, my, cy, x, mx, xx: S(y * x * x) - 2 * mx * S(y * x) + mx * mx * my + cy * xx      # [(cy + y) x'x']
    mU, mV, mW = cs[1] + mb, cV + mc, cW + md
    cols = [cs[0] + ma, mU, mV, mW, cs[4] + me, mf, TT, UU, VV, cov(c, a, mc, ma), cov(d, a, md, ma), UV, WU, WV, cov(d, e, md, me), cov(f, a, mf, ma),
            third(c, mc, cV, a, ma, TT), third(d, md, cW, a, ma, TT),
            2 * mU * UV + mU * mU * mV + 2 * mV * VV + mV ** 3, 2 * mU * WU + mU * mU * mW + 2 * mV * WV + mV * mV * mW,
            third(c, mc, cV, bb, mb, UU) + third(c, mc, cV, c, mc, VV), third(d, md, cW, bb, mb, UU) + third(d, md, cW, c, mc, VV)]
    return np.stack(cols + [np.zeros_like(ma)] * 6, axis=-1)


def test_conditioning_strains_the_shift_and_R_follows_its_rule():
    """About 0 instead of about the first element the float64 sums miss the GPU bar by more than 100 x on this family (it strains the
    cancellation at all); about the first element they stay below a tenth of the bar at the chosen R -- the largest of 100, 30, 10 at which they do."""
    pairs0 = []
    for case_id in rc.FAMILY_IDS["conditioning"]:
        dom, boxes, _, _ = rc.build(case_id)
        ref = rc.reference(case_id)[(0, 4)]
        m = max(float(rc.moment_error(shifted_records(dom, b), r).max()) for b, r in zip(boxes, ref))
        print(f"{case_id}: float64 shifted sums within {m:.2e} (slots 5..21, of the largest value); R = {rc.build(case_id)[3][0]['R']}")
        assert m < 0.1 * rc.GPU_BAR and m <= 2 * COND_MEASURED[case_id], (case_id, m)
        pairs0 += [(shifted_records(dom, b, shifted=False), r) for b, r in zip(boxes, ref)]
    dom = rc.smooth_domain(0.01, 1, 100)                  # the next larger R of the rule's three does not pass (case b)
    m100 = max(float(rc.moment_error(shifted_records(dom, b), rs.row_records(dom, rc.limits_of(dom, b))).max()) for b in rc.build("cond-b")[1])
    print(f"cond-b at R = 100: {m100:.2e}")
    assert rc.COND_R == 30 and m100 >= 0.1 * rc.GPU_BAR
    _sees("conditioning, sums about 0", pairs0)
