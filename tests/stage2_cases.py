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


TALL_CLEAN_IDS = tuple(f"tall{h}" for h in TALL_HEIGHTS)
TALL_NAN_IDS = tuple(f"tall131_{c}" for c in TALL_NAN_CASES)
MANY_CLEAN_IDS = tuple(f"levels{n}" for n in MANY_LEVELS)
MANY_NAN_ID = "levels130_nan"
MOVING_ID = "moving_mixed_heights"
CLEAN_IDS = TALL_CLEAN_IDS + MANY_CLEAN_IDS
NAN_FIXED_IDS = TALL_NAN_IDS + (MANY_NAN_ID,)
FIXED_IDS = TALL_CLEAN_IDS + TALL_NAN_IDS + MANY_CLEAN_IDS + (MANY_NAN_ID,)

_BUILDERS = {**{f"tall{h}": functools.partial(tall_clean, h) for h in TALL_HEIGHTS},
             **{f"tall131_{c}": functools.partial(tall_nan, c) for c in TALL_NAN_CASES},
             **{f"levels{n}": functools.partial(many_levels_clean, n) for n in MANY_LEVELS},
             MANY_NAN_ID: many_levels_nan, MOVING_ID: moving_mixed_heights}


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
        s, lv = o.lec_moving(d, limits) if case_id == MOVING_ID else o.lec_fixed(d, *limits)
    f64 = lambda m: {k: np.asarray(v, dtype=np.float64) for k, v in m.items()}
    return f64(s), f64(lv)
