"""Case builders for the seams of stage 2 (csrc/lec_reduce.hip)  --  TEST INFRASTRUCTURE ONLY; no GPU, no torch.

Stage 2's launch constants put these seams into its control flow:

* boxes of at most 64 latitude rows take ``lec_level_small_kernel``, taller ones ``lec_area_means_kernel`` + ``lec_level_terms_kernel``;
* the general kernel stages 64 rows plus one halo row either side per trip, so a box row 63 / 64 / 65 / 127 / 128 reads its
  neighbour across a trip, and a box whose height is no multiple of 64 ends in a partial trip;
* ``build_level_functions`` and the level-table epilogue of ``lec_vertical_kernel`` walk the levels 64 per pass, up to 160.

Every builder returns ``(dom, limits, expectations)``: a ``helpers.synthetic_domain`` (NaNs planted where the case says), the box as
geographic limits (west, east, south, north) -- a list of them, one per step, for the moving case -- and what the case claims about
itself, which tests/test_stage2_cases_cpu.py checks on the oracle alone.  The grids are thin (10 or 12 columns): stage 1 is not the
subject here.

``expectations`` keys (rows are BOX rows, levels and steps are indices):
  height    box rows (a list, one per step, for the moving case)        kernel   "small" | "general" (by the call's tallest box)
  za_nan    [(field, step, level, rows)]: the field's zonal mean is NaN at exactly these rows of that (step, level)
  repaired  [(table, piece, step, level)]: ``piece`` (saved before _handle_nans) is NaN there, ``table`` (saved after) is finite
  dropped   [(table, level)] (fixed) / [(table, step, level)] (moving): the level is absent from the integral -- of EVERY step in the
            fixed framework (dropna over [time, level]), of that step alone in the moving one
  clamp     True: the static-stability clamp must bind on some, and on fewer than a tenth, of the (step, level) pairs
  asymmetry (axes family) {"lat", "level"}: the least |hd - hs| / max(hs, hd) over the neighbouring intervals (hs, hd) of the box's
            interior latitudes (of every box of three rows or more, for the moving case) and of the interior levels

The ``axes`` family.  ``synthetic_domain`` puts every case above on ``linspace`` latitudes and levels, where np.gradient's middle
coefficient is 0 in every interior row and level, every interior row shares one coefficient triple, a one-level gap is repaired to the
midpoint whether one interpolates in pressure or in level index, and the trapezoid weights of the interior are all alike.  The
``axes_*`` cases replace ``dom.lat`` and ``dom.level`` after generation (the fields stay as generated: the oracle only sees values
on axes) by ``uneven_axis`` and cross the same seams again, with gaps two to five levels deep.

``build(case_id)`` caches: a case is built once per process and must not be written to.
"""
import functools

import numpy as np

from tests.helpers import synthetic_domain

FIELDS = ("tair", "u", "v", "omega", "geopt")

TALL_HEIGHTS = (63, 64, 65, 66, 127, 128, 129, 131)
TALL_NAN_CASES = ("seam_omega", "tail_omega_reaches_boundary", "interior_T_row100", "bottom_rows_64_65", "column", "wind_last_row")
MANY_LEVELS = (64, 65, 128, 129, 160)
MOVING_HEIGHTS = (130, 64, 65, 2, 100)


AXES_HEIGHTS = {"axes_small": 12, "axes_small64": 64, "axes_tall66": 66, "axes_tall131": 131}


def _kernel(height):
    return "small" if height <= 64 else "general"


def _limits(dom, iw, ie, js, jn):
    return (dom.lon[iw], dom.lon[ie], dom.lat[js], dom.lat[jn])


def tall_clean(height):
    """One fixed box of ``height`` rows (grid rows 2 .. height + 1 of height + 3), 5 levels, 3 steps, clean data."""
    dom = synthetic_domain(3, 5, height + 3, 12, seed=height, lat0=-70.0, lat1=-5.0)
    return dom, _limits(dom, 1, 10, 2, height + 1), {"height": height, "kernel": _kernel(height)}


def tall_nan(case):
    """One fixed box of 131 rows (grid rows 1 .. 131 of 134: trips of 64 + 64 + 3), 8 levels, 4 steps, NaNs by ``case``.  Rows below
    are box rows (grid row - 1); columns are grid columns, all inside the box (columns 1 .. 10)."""
    dom = synthetic_domain(4, 8, 134, 12, seed=7, lat0=-70.0, lat1=-5.0)
    nl = dom.level.size
    g = lambda a, b: slice(a + 1, b + 2)          # box rows a .. b inclusive -> grid rows
    r = lambda a, b: list(range(a, b + 1))
    exp = {"height": 131, "kernel": "general"}
    if case == "seam_omega":                      # BAz's bottom-top repair on both sides of the first seam and in the halo
        dom.omega[2, 4, g(63, 65), 3:6] = np.nan
        exp.update(za_nan=[("omega", 2, 4, r(63, 65))], repaired=[("Ce", "Ce_2", 2, 4), ("Cz", "Cz_2", 2, 4)], dropped=[])
    elif case == "tail_omega_reaches_boundary":   # the per-latitude repair reaches the bottom level, in the third (partial) trip
        dom.omega[2, nl - 2, g(128, 130), 3:6] = np.nan
        dom.omega[2, nl - 1, g(70, 71), 5:7] = np.nan
        exp.update(za_nan=[("omega", 2, nl - 2, r(128, 130)), ("omega", 2, nl - 1, r(70, 71))], repaired=[],
                   dropped=[("Ce", nl - 1), ("Ce", nl - 2), ("Cz", nl - 1)])
    elif case == "interior_T_row100":             # an interior T gap in a later trip
        dom.tair[3, 3, 100 + 1, 4] = np.nan
        exp.update(za_nan=[("tair", 3, 3, [100])], repaired=[("Ce", "Ce_2", 3, 3), ("Ca", "Ca_2", 3, 2), ("Ca", "Ca_2", 3, 4)], dropped=[])
    elif case == "bottom_rows_64_65":             # the bottom level dropped for the whole series
        dom.tair[1:3, nl - 1, g(64, 65), 2:5] = np.nan
        dom.omega[1:3, nl - 1, g(64, 65), 2:5] = np.nan
        exp.update(za_nan=[("tair", 1, nl - 1, r(64, 65)), ("omega", 2, nl - 1, r(64, 65))], repaired=[],
                   dropped=[("Az", nl - 1), ("Ae", nl - 1), ("Ce", nl - 1), ("Cz", nl - 1)])
    elif case == "column":                        # a column lost from level 5 to the ground across the second seam, every step
        for name in FIELDS:
            getattr(dom, name)[:, 5:, g(126, 129), 4:6] = np.nan
        exp.update(za_nan=[("u", 0, 5, r(126, 129)), ("tair", 3, nl - 1, r(126, 129)), ("geopt", 2, 6, r(126, 129))], repaired=[],
                   dropped=[(t, k) for t in ("Az", "Ae", "Kz", "Ke", "Ce", "Cz", "Ck") for k in (5, 6, 7)])
    elif case == "wind_last_row":                 # the north-edge row (it carries the north-south boundary pieces), in the last trip
        dom.u[:, 3, 130 + 1, 4] = np.nan
        exp.update(za_nan=[("u", 0, 3, [130]), ("u", 3, 3, [130])], repaired=[("Ck", "Ck_1", 0, 3), ("Ck", "Ck_4", 2, 2), ("Ck", "Ck_4", 2, 4)],
                   dropped=[])
    else:
        raise KeyError(case)
    return dom, _limits(dom, 1, 10, 1, 131), exp


def many_levels_clean(nl):
    """``nl`` levels on a 7 x 10 grid, 3 steps, the box one point inside the grid.  Seed: ``nl``, except at 64 levels, where the noise of
    most seeds (64 among them) leaves no (step, level) pair on the static-stability clamp -- seed 0 puts one there."""
    dom = synthetic_domain(3, nl, 7, 10, seed={64: 0}.get(nl, nl))
    return dom, _limits(dom, 1, 8, 1, 5), {"height": 5, "kernel": "small", "clamp": True}


def many_levels_nan():
    """130 levels: a top level NaN at one step (dropped for every step), an interior wind gap in the second pass of the level loops, a
    T gap at level 100, and the bottom level (third pass) NaN at one step.  Grid rows 3 / 2 are box rows 2 / 1."""
    dom = synthetic_domain(3, 130, 7, 10, seed=1)
    dom.v[1, 0, :, :] = np.nan
    dom.u[:, 70, 3, 4] = np.nan
    dom.tair[2, 100, 2, 5] = np.nan
    dom.omega[1, 129, 3, 3:5] = np.nan
    exp = {"height": 5, "kernel": "small", "clamp": True,
           "za_nan": [("v", 1, 0, [0, 1, 2, 3, 4]), ("u", 0, 70, [2]), ("u", 2, 70, [2]), ("tair", 2, 100, [1]), ("omega", 1, 129, [2])],
           "repaired": [("Ck", "Ck_1", 0, 70), ("Ck", "Ck_1", 2, 70), ("Ce", "Ce_2", 2, 100)],
           "dropped": [("Kz", 0), ("Ke", 0), ("Ck", 0), ("Ce", 129), ("Cz", 129)]}
    return dom, _limits(dom, 1, 8, 1, 5), exp


def moving_mixed_heights():
    """Per-step boxes of 130, 64, 65, 2 and 100 rows from grid row 2 of a 140 x 12 grid, 6 levels: one record buffer of 130 rows in which
    the lower boxes end inside a trip.  omega is NaN in the LAST row of step 2's 65-row box (box row 64: the first row of the second
    trip), T in the last row of step 4's 100-row box at the bottom level."""
    dom = synthetic_domain(5, 6, 140, 12, seed=3, lat0=-70.0, lat1=-1.0)
    dom.omega[2, 3, 66, 4] = np.nan
    dom.tair[4, 5, 101, 4] = np.nan
    boxes = [(1, 10, 2, 2 + h - 1) for h in MOVING_HEIGHTS]
    exp = {"height": list(MOVING_HEIGHTS), "kernel": "general", "boxes": boxes,
           "za_nan": [("omega", 2, 3, [64]), ("tair", 4, 5, [99])],
           "repaired": [("Ce", "Ce_2", 2, 3), ("Cz", "Cz_2", 2, 3)],
           "dropped": [("Az", 4, 5), ("Ae", 4, 5), ("Ce", 4, 5)]}
    return dom, [_limits(dom, *b) for b in boxes], exp


# ---------------------------------------------------------------------------------------------------------------------------------
# axes: uneven latitudes and pressure levels
# ---------------------------------------------------------------------------------------------------------------------------------
def uneven_axis(lo, hi, n):
    """``n`` ascending points from ``lo`` to ``hi`` whose intervals alternate between longer and shorter than the mean by 10 to 20 %, no
    two by the same share (the golden-ratio sequence): neighbouring intervals differ by 18 % of the longer one at the least, and every
    interior point has a coefficient triple of its own.  (The form lat + 0.2 step sin(j) of tests/rowstats_cases.py will not do at these
    heights: its neighbouring intervals differ by 0.18 step |sin j|, which is 0.2 % at j = 22 and 0.3 % at j = 44; geomspace gives 1.8 %
    at 130 levels.)"""
    j = np.arange(n - 1)
    h = 1.0 + 0.2 * (-1.0) ** j * (0.5 + 0.5 * ((j * 0.6180339887498949) % 1.0))
    x = lo + (hi - lo) * np.concatenate([[0.0], np.cumsum(h)]) / h.sum()
    x[-1] = hi
    return x


def interval_asymmetry(x):
    """min over the interior points of |hd - hs| / max(hs, hd), (hs, hd) the intervals either side: 0 on an even axis."""
    d = np.diff(np.asarray(x, dtype=np.float64))
    return float(np.min(np.abs(d[1:] - d[:-1]) / np.maximum(d[1:], d[:-1])))


def _uneven(dom):
    """``dom`` on uneven axes of the same extent (10 000 Pa, the data's pmin, stays the top level).  Levels: geomspace up to 12 of them
    (neighbouring intervals differ by 25 % at 9 levels, 37 % at 6), ``uneven_axis`` beyond."""
    nl = dom.level.size
    dom.lat = uneven_axis(dom.lat[0], dom.lat[-1], dom.lat.size)
    dom.level = np.geomspace(dom.level[0], dom.level[-1], nl) if nl <= 12 else uneven_axis(dom.level[0], dom.level[-1], nl)
    return dom


def _asymmetry(dom, boxes):
    return {"lat": min(interval_asymmetry(dom.lat[js:jn + 1]) for _, _, js, jn in boxes if jn - js >= 2), "level": interval_asymmetry(dom.level)}


def _axes_rows_domain(height, nt):
    """A box of ``height`` rows, one grid point inside a grid of height + 2 rows and 12 columns on every side (box row = grid row - 1),
    9 levels.  The 64-row box lies in a grid of 72 rows: its records are also run through the general kernels in a buffer of 70 rows,
    and a record buffer is no taller than the grid."""
    dom = _uneven(synthetic_domain(nt, 9, 72 if height == 64 else height + 2, 12, seed=height, lat0=-70.0, lat1=-5.0))
    box = (1, 10, 1, height)
    return dom, box, {"height": height, "kernel": _kernel(height), "asymmetry": _asymmetry(dom, [box])}


def axes_rows(case):
    """3 steps x 9 levels, clean: 12 rows (the small kernel, gr b and p b non-zero in every interior lane), 64 and 66 rows (the kernel
    switch from either side), 131 rows (the general kernel: another coefficient triple in every staged row, halo rows across both trip
    seams, a last trip of 3 rows)."""
    dom, box, exp = _axes_rows_domain(AXES_HEIGHTS[case], 3)
    return dom, _limits(dom, *box), exp


def axes_rows_nan(case):
    """``axes_small`` / ``axes_tall131`` with 4 steps and gaps two to five levels deep (9 levels: 0 .. 8), so that the weight of a repair
    is not 1/2 and depends on p.  Box rows (ra, rb, rc, rd) = (63..65, 100, 129, 10..11) at 131 rows, (5..7, 9, -, 2..3) at 12:
      (a) step 2: omega at rows ra (131 rows: either side of the first trip seam), levels 3 and 4 -- BAz's per-latitude repair, and the
          pieces of Ce, Cz and Ca;
      (b) step 0: one u point at row rb (131 rows: in the second trip), levels 4, 5, 6 -- Ck_1 there, and Ck_4 / Ck_5 (d[u]/dp) at
          levels 3 .. 7: a gap five levels deep in Ck;
      (c) step 3, 131 rows only: one T point at row rc (the last trip), levels 5 and 6 -- every piece with T there, Ca_2 (d T*/dp) at
          levels 4 .. 7;
      (d) step 1: omega at rows rd, levels 7 and 8, the two at the bottom -- lost to every step of Ce, Cz, Ca and Ck, whose integrals
          end at level 6 and lose two uneven intervals.  Step 1 on purpose: a first time shard of step 0 alone does not hold it."""
    tall = case == "axes_tall131_nan"
    dom, box, exp = _axes_rows_domain(131 if tall else 12, 4)
    ra, rb, rc, rd = ([63, 64, 65], 100, 129, [10, 11]) if tall else ([5, 6, 7], 9, None, [2, 3])
    g = lambda rows: slice(rows[0] + 1, rows[-1] + 2)          # box rows -> grid rows
    dom.omega[2, 3:5, g(ra), 3:6] = np.nan
    dom.u[0, 4:7, rb + 1, 4] = np.nan
    dom.omega[1, 7:9, g(rd), 2:5] = np.nan
    za = [("omega", 2, 3, ra), ("omega", 2, 4, ra), ("u", 0, 4, [rb]), ("u", 0, 5, [rb]), ("u", 0, 6, [rb]), ("omega", 1, 7, rd), ("omega", 1, 8, rd)]
    rep = [(t, t + "_2", 2, k) for t in ("Ce", "Cz", "Ca") for k in (3, 4)] + [("Ck", "Ck_1", 0, k) for k in (4, 5, 6)] + [("Ck", "Ck_4", 0, 3)]
    if tall:
        dom.tair[3, 5:7, rc + 1, 4] = np.nan
        za += [("tair", 3, 5, [rc]), ("tair", 3, 6, [rc])]
        rep += [("Ca", "Ca_2", 3, 4), ("Ca", "Ca_1", 3, 5), ("Ce", "Ce_2", 3, 5), ("Ce", "Ce_2", 3, 6)]
    exp.update(za_nan=za, repaired=rep, dropped=[(t, k) for t in ("Ce", "Cz", "Ca", "Ck") for k in (7, 8)])
    return dom, _limits(dom, *box), exp


AXES_LEVELS_SEED = 130          # on these levels every seed from 0 to 139 leaves 2.5 ... 8 % of the (step, level) pairs on the clamp: 5.4 % here


def _axes_levels_domain():
    dom = _uneven(synthetic_domain(3, 130, 7, 10, seed=AXES_LEVELS_SEED))
    box = (1, 8, 1, 5)
    return dom, box, {"height": 5, "kernel": "small", "clamp": True, "asymmetry": _asymmetry(dom, [box])}


def axes_levels130():
    """130 uneven levels on a 7 x 10 grid, 3 steps, clean: lv[4k], pa / pb / pc, c1k and the trapezoid in p for k >= 64 and k >= 128."""
    dom, box, exp = _axes_levels_domain()
    return dom, _limits(dom, *box), exp


def axes_levels130_nan():
    """130 uneven levels: a T gap at levels 100 and 101 (one point, step 2), a u gap at levels 63, 64, 65 (one point, every step: the
    repair scan's first pass ends inside it), the top level NaN at step 1 (dropped for every step).  Grid rows 3 / 2 are box rows
    2 / 1."""
    dom, box, exp = _axes_levels_domain()
    dom.v[1, 0, :, :] = np.nan
    dom.u[:, 63:66, 3, 4] = np.nan
    dom.tair[2, 100:102, 2, 5] = np.nan
    exp.update(za_nan=[("v", 1, 0, [0, 1, 2, 3, 4])] + [("u", t, k, [2]) for t in (0, 2) for k in (63, 64, 65)] + [("tair", 2, 100, [1]), ("tair", 2, 101, [1])],
               repaired=[("Ck", "Ck_1", t, k) for t in (0, 2) for k in (63, 64, 65)] + [("Ck", "Ck_4", 0, 62), ("Ck", "Ck_4", 0, 66)]
               + [("Ce", "Ce_2", 2, 100), ("Ce", "Ce_2", 2, 101), ("Ca", "Ca_2", 2, 99), ("Ca", "Ca_2", 2, 102)],
               dropped=[("Kz", 0), ("Ke", 0), ("Ck", 0)])
    return dom, _limits(dom, *box), exp


AXES_MOVING_STARTS = (2, 40, 7, 100, 21)


def axes_moving():
    """``moving_mixed_heights`` on uneven axes, the boxes of 130, 64, 65, 2 and 100 rows starting at grid rows 2, 40, 7, 100 and 21: every
    box has latitude tables of its own (on even latitudes boxes of one height share their gradient coefficients).  omega is NaN at levels
    2 and 3 (of 6) in the last row of step 2's 65-row box (box row 64, grid row 71: the first row of the second trip), T in the last row of
    step 4's 100-row box (grid row 120) at the bottom level.  Step 3's 2-row box has no interior row."""
    dom = _uneven(synthetic_domain(5, 6, 140, 12, seed=3, lat0=-70.0, lat1=-1.0))
    dom.omega[2, 2:4, 71, 4] = np.nan
    dom.tair[4, 5, 120, 4] = np.nan
    boxes = [(1, 10, j, j + h - 1) for j, h in zip(AXES_MOVING_STARTS, MOVING_HEIGHTS)]
    exp = {"height": list(MOVING_HEIGHTS), "kernel": "general", "boxes": boxes, "asymmetry": _asymmetry(dom, boxes),
           "za_nan": [("omega", 2, 2, [64]), ("omega", 2, 3, [64]), ("tair", 4, 5, [99])],
           "repaired": [(t, t + "_2", 2, k) for t in ("Ce", "Cz") for k in (2, 3)],
           "dropped": [("Az", 4, 5), ("Ae", 4, 5), ("Ce", 4, 5)]}
    return dom, [_limits(dom, *b) for b in boxes], exp


TALL_CLEAN_IDS = tuple(f"tall{h}" for h in TALL_HEIGHTS)
TALL_NAN_IDS = tuple(f"tall131_{c}" for c in TALL_NAN_CASES)
MANY_CLEAN_IDS = tuple(f"levels{n}" for n in MANY_LEVELS)
MANY_NAN_ID = "levels130_nan"
MOVING_ID = "moving_mixed_heights"
CLEAN_IDS = TALL_CLEAN_IDS + MANY_CLEAN_IDS
NAN_FIXED_IDS = TALL_NAN_IDS + (MANY_NAN_ID,)
AXES_ROWS_IDS = tuple(AXES_HEIGHTS)
AXES_CLEAN_IDS = AXES_ROWS_IDS + ("axes_levels130",)
AXES_NAN_IDS = ("axes_tall131_nan", "axes_small_nan", "axes_levels130_nan")
AXES_FIXED_IDS = AXES_CLEAN_IDS + AXES_NAN_IDS
AXES_MOVING_ID = "axes_moving"
MOVING_IDS = (MOVING_ID, AXES_MOVING_ID)
CLEAN_IDS = CLEAN_IDS + AXES_CLEAN_IDS
NAN_FIXED_IDS = NAN_FIXED_IDS + AXES_NAN_IDS
FIXED_IDS = TALL_CLEAN_IDS + TALL_NAN_IDS + MANY_CLEAN_IDS + (MANY_NAN_ID,) + AXES_FIXED_IDS

_BUILDERS = {**{f"tall{h}": functools.partial(tall_clean, h) for h in TALL_HEIGHTS},
             **{f"tall131_{c}": functools.partial(tall_nan, c) for c in TALL_NAN_CASES},
             **{f"levels{n}": functools.partial(many_levels_clean, n) for n in MANY_LEVELS},
             MANY_NAN_ID: many_levels_nan, MOVING_ID: moving_mixed_heights,
             **{c: functools.partial(axes_rows, c) for c in AXES_ROWS_IDS},
             **{c: functools.partial(axes_rows_nan, c) for c in ("axes_tall131_nan", "axes_small_nan")},
             "axes_levels130": axes_levels130, "axes_levels130_nan": axes_levels130_nan, AXES_MOVING_ID: axes_moving}


@functools.lru_cache(maxsize=None)
def build(case_id):
    """(dom, limits, expectations) of a case by id, built once per process: read-only."""
    return _BUILDERS[case_id]()


@functools.lru_cache(maxsize=None)
def reference(case_id, extended=True):
    """(scalars, level tables) of the oracle on a case, as float64, evaluated in np.longdouble (``extended``) or in float64: computed
    once per process and shared by the tests -- read-only."""
    from oracle import lec_oracle as o
    from tests.helpers import as_f64, as_longdouble
    dom, limits, _ = build(case_id)
    d = as_longdouble(dom) if extended else as_f64(dom)
    with np.errstate(invalid="ignore"):
        s, lv = o.lec_moving(d, limits) if case_id in MOVING_IDS else o.lec_fixed(d, *limits)
    f64 = lambda m: {k: np.asarray(v, dtype=np.float64) for k, v in m.items()}
    return f64(s), f64(lv)
