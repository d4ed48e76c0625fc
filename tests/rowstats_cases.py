"""Case builders for the seams of stage 1 (csrc/lec_rowsweep_kernel.h, lec_rowblock.hip, lec_boxtile.hip, lec_boxplane.hip)  --  TEST
INFRASTRUCTURE ONLY; no GPU, no torch.

Every case holds the stage-1 kernels to tests/rowstats_restatement.py, the 28 interface statistics of a row evaluated in np.longdouble
from the oracle's own functions, at the smallest shapes at which a kernel family's control flow changes.  A case is a DOMAIN (clean
fields, shared by all cases of one (dtype, grid)) and a list of BOXES; a fixed-box case makes one call per box and run, a per-step case
one call with a box per step.  ``build(case_id)`` returns ``(dom, boxes, kw, expectations)``; ``reference(case_id, extended)`` the
records.  Both cache: built once per process, never written to.

The frame.  The GPU test hands the kernels fields that are NaN at every grid point outside the box (per-step boxes with T's time
neighbours read from the cube: outside the boxes of steps t - 1, t, t + 1; packed series: the slab beside the box; a ring: the
latitude rows outside the band).  The restatement differentiates the box-cropped arrays, so it never sees the frame; a kernel whose
edge trips let a value from outside the box into a statistic -- 0 x NaN is NaN -- does not come out finite.

Families (``kw["family"]``) and what ``expectations`` states, restated from the launch rules in a few lines of Python below:

  sweep   one wave per row (tuning kernel=row_sweep), one fixed box per call.  Per box: vec (elements per lane and trip, from dtype,
          nx and f32_vec), shift (iw % vec), nvec, ntrips, one_trip, mid_end, and trip / lane of the vector that holds the row's last
          element (e0_last); ``trips`` in {"one", "two", "middle"}, ``lane`` in {"0", "63", "other"}.
  block   lec_rowblock_kernel (tuning kernel=row_block, block_shape 212 / 222 / 122) on 5 box rows, 3 levels, 3 steps: partial blocks
          along every axis; the same per-box numbers as sweep (fp32: float2 at most).
  tile    lec_boxtile_kernel, a box per step on a cube, one call for boxes of at most 64 columns and one with wider boxes (``window``:
          whether the launch takes the kernel's WINDOW form): widths, heights, start-column residues mod 4, grid edges touched, row
          groups of 4, levels per wave (the launch's choice and one walk over all levels).
  plane   lec_boxplane_kernel, a box-packed series (slabs of at most 64 columns): as tile, plus boxes that fill / do not fill the slab.
  ring    lec_rowstats_ring at the row widths tests/test_gpu_ring.py names; modes 0, 2, 3.
  axes    uneven latitudes, pressure levels and time steps on sweep, block, tile and plane: every interior coefficient triple of the
          three axes asymmetric by more than 5 %.
  conditioning   rows that strain the shift of the single-sweep form (sweep kernel): no noise at all, and the box's west column -- the
          shift -- R row standard deviations away from the row, in T alone and in all five fields.
  nan     one NaN at a time INSIDE the box (``kw["plants"]``), on sweep (double2, float4), tile and plane: at the row's first, a
          middle-trip and last element, and in T one row, level and step away.  ``reference`` is then {plant: records}.
The tile family also holds ``steps-float64`` (lec_rowstats_steps: three tracks over one cube), the sweep family three cases of the
two-sweep cross-check kernel on table longitudes.
"""
import functools

import numpy as np

from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests import rowstats_restatement as rs
from tests.helpers import synthetic_domain

LANES = 64
GPU_BAR = 1e-11            # slots 5..21: of the statistic's largest value over the case's rows
EPS = 2.0 ** -53

# ---------------------------------------------------------------------------------------------------------------------------------
# the launch rule, restated (lec_rowstats.hip: aligned / aligned8; lec_rowsweep_kernel.h: launch_dtype, launch_one and the kernel)
# ---------------------------------------------------------------------------------------------------------------------------------


def vec_of(dtype, nx, f32_vec=0, family="sweep"):
    """Elements per lane and trip.  fp64: 2 when nx is even, else 1; fp32: 4 when nx % 4 == 0 and float2 is not forced (the row-block
    kernel has no float4 form), else 2 when nx is even, else 1.  (Cube bases are 16-byte aligned: torch allocations are.)"""
    if np.dtype(dtype) == np.float64:
        return 2 if nx % 2 == 0 else 1
    if nx % 4 == 0 and f32_vec != 2 and family != "block":
        return 4
    return 2 if nx % 2 == 0 else 1


def trips_of(vec, iw, nxb, nx):
    """What the one-wave-per-row kernels do with a row of ``nxb`` elements starting at column ``iw`` of rows of ``nx``."""
    shift = iw % vec if vec > 1 else 0                 # rowoff % VEC: every row pitch is a multiple of VEC when VEC > 1
    assert vec == 1 or nx % vec == 0
    nvec = (nxb + vec - 1) // vec + (1 if vec > 1 else 0)
    ntrips = (nvec + LANES - 1) // LANES
    mid_end = min((nxb - 1 + shift) // (LANES * vec), ntrips)
    e0_last = ((nxb - 1 + shift) // vec) * vec - shift
    vi = (e0_last + shift) // vec                       # the vector (lane of a trip) that holds the last element
    assert vi // LANES < ntrips                         # the launch's trips cover the row
    return dict(vec=vec, shift=shift, nxb=nxb, nvec=nvec, ntrips=ntrips, one_trip=ntrips == 1, mid_end=mid_end, e0_last=e0_last,
                last_trip=vi // LANES, last_lane=vi % LANES,
                trips="one" if ntrips == 1 else ("middle" if mid_end >= 2 else "two"),
                lane={0: "0", LANES - 1: "63"}.get(vi % LANES, "other"))


# (waves a launch aims for, longest walk it chooses by itself, longest walk a caller may ask for): launch_tiles in lec_boxtile.hip
# (kTargetWaves, kMaxLevels, kMaxLevels) and lec_launch_boxplane in lec_boxplane.hip (kTargetWaves, kWalk, kMaxLevels)
WALK_RULE = {"tile": (8192, 21, 21), "plane": (32768, 10, 42)}


def tile_walk(nl, t_count, nyb_max, tile_j, kernel):
    """Levels per wave of a box-tile / box-plane launch (``kernel``: "tile" | "plane"); tile_j < 1: the launch's own choice -- as many
    chunks as the target number of waves asks for, between walks of 5 levels and the kernel's longest own walk."""
    target, own, asked = WALK_RULE[kernel]
    assert tile_j <= asked
    if tile_j < 1:
        n_rb, jchunk = (nyb_max + 3) // 4, (t_count + 7) // 8
        want = -(-target // (8 * jchunk * n_rb))
        most, least = -(-nl // 5), -(-nl // own)
        tile_j = -(-nl // (least if want < least else min(want, most)))
    return min(tile_j, nl)


def full_widths(vec):
    return sorted({2, 3, 4, 5} | {w for m in (1, 2, 3) for w in range(63 * vec * m - vec - 1, 64 * vec * m + vec + 2)})


def reduced_widths(vec, shift):
    """Three widths on each side of every change: the launch's trip count (nvec passes a multiple of 64) and the trip of the row's last
    element (which is also where mid_end moves), for one, two and three trips."""
    w = {2, 3, 5}
    for m in (1, 2, 3):
        w0 = vec * (64 * m - 1) + 1 if vec > 1 else 64 * m + 1      # first width whose launch has m + 1 trips
        w1 = 64 * vec * m - shift + 1                               # first width whose last element lies in trip m
        w |= {w0 - 1, w0, w0 + 1, w1 - 1, w1, w1 + 1}
    return sorted(w)


# ---------------------------------------------------------------------------------------------------------------------------------
# domains
# ---------------------------------------------------------------------------------------------------------------------------------
AXES_LEVELS_HPA = (50, 100, 250, 300, 500, 650, 850, 925, 975)        # nine of the 37 ERA5 levels, no two neighbouring gaps alike
AXES_HOURS = (0.0, 1.0, 4.0, 6.0)                                     # 1-, 3-, 2-hour steps


def domain(dtype, nt, nl, ny, nx, lon="even", axes="even"):
    """The clean fields of a (dtype, grid): read-only.  ``lon`` "table": stretched longitudes (the kernels' wlon / glon tables);
    ``axes`` "uneven": latitudes, levels (nl must be 9) and time steps (nt must be 4) replaced after generation."""
    return _domain(np.dtype(dtype).name, nt, nl, ny, nx, lon, axes)


@functools.lru_cache(maxsize=None)
def _domain(dtype, nt, nl, ny, nx, lon, axes):
    # Longitudes 0, 1/8, 2/8, ... degrees: exactly representable and exactly evenly spaced, so the trapezoid weights of the extended-
    # precision restatement are the kernels' uniform weights to a fraction of an ulp, and near 0, where a float64 radian (the host
    # tables of the "table" form, the float64 restatement) is rounded by the least: the bound on the means assumes exact weights
    dom = synthetic_domain(nt, nl, ny, nx, seed=nx + 7 * ny + nl, dtype=np.dtype(dtype).type, lon0=0.0, lon1=0.125 * (nx - 1), nonuniform_lon=lon == "table")
    if axes == "uneven":
        assert nl == len(AXES_LEVELS_HPA) and nt == len(AXES_HOURS)
        step = dom.lat[1] - dom.lat[0]
        dom.lat = np.sort(dom.lat + 0.2 * step * np.sin(np.arange(ny)))
        dom.level = np.asarray(AXES_LEVELS_HPA, dtype=np.float64) * 100.0
        dom.time_s = np.asarray(AXES_HOURS) * 3600.0
    return dom


def steps_of(dom, h0, h1):
    """Steps [h0, h1) of a domain as a domain of its own (views)."""
    return o.Domain(dom.tair[h0:h1], dom.u[h0:h1], dom.v[h0:h1], dom.omega[h0:h1], dom.geopt[h0:h1], dom.lat, dom.lon, dom.level, dom.time_s[h0:h1])


def limits_of(dom, box):
    iw, ie, js, jn = box
    return (dom.lon[iw], dom.lon[ie], dom.lat[js], dom.lat[jn])


def dtdt_cube(dom):
    """A caller's dT/dt cube in the storage dtype: np.gradient of the stored T (as fp64) over the domain's time axis."""
    return np.ascontiguousarray(o.differentiate(dom.tair.astype(np.float64), dom.time_s, axis=0).astype(dom.tair.dtype))


def tables_uniform(lon):
    """The engine's choice between the even-longitude and the table formulation (tables.is_uniform)."""
    d = np.diff(np.asarray(lon, dtype=np.float64))
    return bool(np.all(np.abs(d - d[0]) <= 1e-12 * np.abs(d[0])))


def gradient_triples(x):
    """np.gradient's interior coefficients (a, b, c) of an axis: d f/dx [i] = a f[i-1] + b f[i] + c f[i+1]."""
    d = np.diff(np.asarray(x, dtype=np.float64))
    d1, d2 = d[:-1], d[1:]
    return np.stack([-d2 / (d1 * (d1 + d2)), (d2 - d1) / (d1 * d2), d1 / (d2 * (d1 + d2))], axis=1)


def asymmetry(triples):
    """min over the interior points of | |a| - |c| | / max(|a|, |c|): 0 on an even axis."""
    a, c = np.abs(triples[:, 0]), np.abs(triples[:, 2])
    return float(np.min(np.abs(a - c) / np.maximum(a, c)))


def axes_asymmetry(dom, boxes):
    """The least asymmetry of the coefficient triples the kernels are given: lattab (box-local latitudes, every box), levtab (alpha and
    gamma of S = -(T / theta) d theta / dp, i.e. np.gradient's outer coefficients times the Exner ratios) and tcoef."""
    ex = (dom.level / o.P0_PA) ** o.KAPPA
    g = gradient_triples(dom.level)
    lev = np.stack([g[:, 0] * ex[1:-1] / ex[:-2], g[:, 1], g[:, 2] * ex[1:-1] / ex[2:]], axis=1)
    lat = min(asymmetry(gradient_triples(dom.lat[b[2]:b[3] + 1])) for b in boxes if b[3] - b[2] >= 2)
    return {"lattab": lat, "levtab": asymmetry(lev), "levels": asymmetry(g), "tcoef": asymmetry(gradient_triples(dom.time_s))}


# ---------------------------------------------------------------------------------------------------------------------------------
# sweep
# ---------------------------------------------------------------------------------------------------------------------------------
# form: (dtype, nx, tuning f32_vec).  nx holds the widest row of the form's width set behind a start column of every residue, with a
# frame column either side
SWEEP_FORMS = {"f64v2": ("float64", 392, 0), "f64v1": ("float64", 197, 0), "f32v4": ("float32", 780, 0), "f32v2": ("float32", 390, 0),
               "f32v2forced": ("float32", 392, 2), "f32v1": ("float32", 197, 0)}
SWEEP_MODES = ("stencil", "noq", "cube", "table", "nophi")
# the two-sweep cross-check kernel (tuning kernel=two_sweep; deviations from the zonal mean, then products) on table longitudes: it
# shares no element arithmetic with the single-sweep kernels, but the same way of addressing a row's vectors
TWO_SWEEP_IDS = ("sweep-f64v2-s1-twosweep", "sweep-f32v4-s1-twosweep", "sweep-f64v1-s0-twosweep")
SWEEP_GRID = dict(nt=4, nl=3, ny=6)
SWEEP_ROWS = (1, 4)                  # box rows js .. jn: four rows, a frame row either side
# (h0, h1, t_begin, t_count): the cube holds steps [h0, h1) of the domain, the call processes [t_begin, t_begin + t_count) of the cube.
# Two steps: the first-step twin of the time stencil plus a one-step launch; four steps whole; steps 1, 2 of four: the launch's
# first step has a real predecessor and lec_qtime_kernel takes the row's own backward pieces
STENCIL_RUNS = ((0, 2, 0, 2), (0, 4, 0, 4), (0, 4, 1, 2))


def _start_column(vec, shift):
    return shift if shift >= 1 else vec          # iw % vec == shift, and at least one frame column west of the box


def sweep_ids():
    ids = []
    for form, (dtype, nx, fv) in SWEEP_FORMS.items():
        for shift in range(vec_of(dtype, nx, fv)):
            ids += [f"sweep-{form}-s{shift}-{mode}" for mode in SWEEP_MODES]
    return tuple(ids) + TWO_SWEEP_IDS


def _mode_kw(mode):
    return dict(with_q=mode != "noq", dtdt=mode == "cube", with_phi=mode != "nophi")


def _sweep(form, shift, mode):
    dtype, nx, fv = SWEEP_FORMS[form]
    vec = vec_of(dtype, nx, fv)
    dom = domain(dtype, nx=nx, lon="table" if mode in ("table", "twosweep") else "even", **SWEEP_GRID)
    iw = _start_column(vec, shift)
    widths = full_widths(vec) if mode == "stencil" else reduced_widths(vec, shift)
    boxes = [(iw, iw + w - 1) + SWEEP_ROWS for w in widths]
    assert all(b[1] <= nx - 2 for b in boxes)
    tuning = {"kernel": "two_sweep"} if mode == "twosweep" else {"kernel": "row_sweep", **({"f32_vec": 2} if fv else {})}
    kw = dict(family="sweep", kind="fixed", tuning=tuning, runs=STENCIL_RUNS if mode == "stencil" else ((0, 4, 0, 4),), **_mode_kw(mode))
    exp = [dict(trips_of(vec, b[0], b[1] - b[0] + 1, nx), form=form, uniform=mode not in ("table", "twosweep")) for b in boxes]
    return dom, boxes, kw, exp


# ---------------------------------------------------------------------------------------------------------------------------------
# block
# ---------------------------------------------------------------------------------------------------------------------------------
BLOCK_SHAPES = (212, 222, 122)
BLOCK_GRID = dict(nt=5, nl=3, ny=7, nx=392)
BLOCK_ROWS = (1, 5)                  # five box rows: a partial block of two latitudes
BLOCK_RUNS = ((0, 3, 0, 3), (0, 5, 1, 3))       # three steps whole (a partial block of two steps); a shard with a halo step either side


BLOCK_TABLE_IDS = ("block-float64-212-s1-table", "block-float32-222-s0-table")      # table longitudes: only on request (tuning), never AUTO


def block_ids():
    return tuple(f"block-{d}-{s}-s{shift}" for d in ("float64", "float32") for s in BLOCK_SHAPES for shift in (0, 1)) + BLOCK_TABLE_IDS


def _block(dtype, shape, shift, axes="even", widths=None, lon="even"):
    grid = dict(BLOCK_GRID, **({"nt": 4, "nl": 9} if axes == "uneven" else {}))
    dom = domain(dtype, axes=axes, lon=lon, **grid)
    vec = vec_of(dtype, grid["nx"], family="block")
    iw = _start_column(vec, shift)
    boxes = [(iw, iw + w - 1) + BLOCK_ROWS for w in (widths or reduced_widths(vec, shift))]
    kw = dict(family="block", kind="fixed", tuning={"kernel": "row_block", "block_shape": shape},
              runs=((0, 4, 0, 4), (0, 4, 1, 2)) if axes == "uneven" else BLOCK_RUNS, **_mode_kw("stencil"))
    bt, bk, bj = shape // 100, (shape // 10) % 10, shape % 10
    exp = [dict(trips_of(vec, b[0], b[1] - b[0] + 1, grid["nx"]), shape=shape,
                partial={"t": [r[3] % bt != 0 for r in kw["runs"]], "k": grid["nl"] % bk != 0, "j": 5 % bj != 0}) for b in boxes]
    return dom, boxes, kw, exp


# ---------------------------------------------------------------------------------------------------------------------------------
# tile and plane: a box per step
# ---------------------------------------------------------------------------------------------------------------------------------
TILE_WIDTHS = tuple(range(2, 19)) + tuple(range(30, 35)) + tuple(range(46, 51)) + tuple(range(62, 67)) + (70,)
# Two calls per kind: boxes of at most 64 columns (kCW: one column chunk; with Q the WINDOW form of lec_boxtile_kernel, which slides
# T(k-1), T(k), T(k+1) through registers down the level walk), and a call whose widest box has 70 (two column chunks, every pass
# loads its own T neighbours) -- the launch picks the form by the call's widest box
TILE_NARROW = tuple(w for w in TILE_WIDTHS if w <= 64)
TILE_WIDE = (62, 63, 64, 65, 66, 70, 5, 17, 33)
TILE_GRID = dict(ny=12, nx=74)
TILE_LEVELS = (10, 11, 21)
TILE_KINDS = (("float64", "cube"), ("float64", "nb"), ("float32", "nb"))      # dT/dt: a cube / per point from the cube's time neighbours
PLANE_WIDTHS = tuple(range(2, 13)) + tuple(range(59, 65))
PLANE_HEIGHTS = (2, 3, 4, 5, 7, 8, 9, 3)      # one short of, at and one past a multiple of 4
PLANE_GRID = dict(ny=11, nx=70)
PLANE_LEVELS = (10, 11, 20, 21)
PLANE_SLAB = (9, 64)                          # slab rows x columns: the tallest / widest box fills it


def tile_ids():
    return tuple(f"tile-{d}-{m}-{lon}-nl{nl}-{c}" for d, m in TILE_KINDS for lon in ("even", "table") for nl in TILE_LEVELS for c in ("narrow", "wide"))


def plane_ids():
    return tuple(f"plane-{d}-nl{nl}" for d in ("float64", "float32") for nl in PLANE_LEVELS)


def _step_boxes(widths, heights, ny, nx):
    """One box per step: widths in turn, heights in turn, the start column of every residue mod 4, and boxes on each grid edge.  Narrow
    boxes stay within 12 columns of longitude 0 and only boxes of 30 columns or more go to the east edge: with stretched longitudes the
    kernels are handed trapezoid weights the host formed from float64 radians (as the reference does), each off by up to
    2^-53 |lambda| / step of itself, which the bound on the means -- exact weights -- has room for only where |lambda| / step is of the
    order of the box's width."""
    boxes = []
    for t, w in enumerate(widths):
        h = heights[t % len(heights)]
        iw = {0: 0, 1: nx - w if w >= 30 else 1}.get(t % 5, min(1 + t % 4 + 4 * (t % 3), nx - w))
        js = {0: 0, 1: ny - h}.get(t % 7, min(1 + t % 2, ny - h))
        boxes.append((iw, iw + w - 1, js, js + h - 1))
    return boxes


def _step_exp(boxes, ny, nx, nl, kernel, slab=None):
    w, h = [b[1] - b[0] + 1 for b in boxes], [b[3] - b[2] + 1 for b in boxes]
    exp = dict(widths=sorted(set(w)), heights=sorted(set(h)), residues=sorted({b[0] % 4 for b in boxes}), width_residues=sorted({x % 4 for x in w}),
               edges=sorted({e for b in boxes for e, on in (("west", b[0] == 0), ("east", b[1] == nx - 1), ("south", b[2] == 0), ("north", b[3] == ny - 1)) if on}),
               row_groups=(max(h) + 3) // 4, partial_row_group=sorted({x % 4 for x in h}), wide=max(w) > 64,
               window=kernel == "tile" and max(w) <= 64,        # launch_tiles: mode != 0 && nxb_max <= kCW (every case here has Q)
               walks={tj: tile_walk(nl, len(boxes), max(h), tj, kernel) for tj in (0, nl)})
    if slab is not None:
        exp["fills_slab_rows"] = sorted({x == slab[0] for x in h})
        exp["fills_slab_columns"] = sorted({x == slab[1] for x in w})
    return exp


def _tile(dtype, mode, lon, nl, call="narrow", axes="even"):
    widths = {"narrow": TILE_NARROW, "wide": TILE_WIDE} if axes == "even" else {"narrow": (5, 17, 33, 64), "wide": (5, 17, 33, 70)}
    widths = widths[call]
    dom = domain(dtype, nt=len(widths), nl=nl, lon=lon, axes=axes, **TILE_GRID)
    boxes = _step_boxes(widths, tuple(range(2, 10)), **TILE_GRID)
    kw = dict(family="tile", kind="moving", mode=mode, tunings=[{"kernel": "box_tile"}, {"kernel": "box_tile", "tile_j": nl}])
    return dom, boxes, kw, _step_exp(boxes, nl=nl, kernel="tile", **TILE_GRID)


def _plane(dtype, nl, axes="even"):
    widths = PLANE_WIDTHS if axes == "even" else (5, 12, 61, 64)
    dom = domain(dtype, nt=len(widths), nl=nl, axes=axes, **PLANE_GRID)
    boxes = _step_boxes(widths, PLANE_HEIGHTS if axes == "even" else (9, 3, 4, 5), **PLANE_GRID)
    kw = dict(family="plane", kind="packed", slab=PLANE_SLAB, tunings=[{"kernel": "box_plane"}, {"kernel": "box_plane", "tile_j": nl}])
    return dom, boxes, kw, _step_exp(boxes, nl=nl, kernel="plane", slab=PLANE_SLAB, **PLANE_GRID)


def pack(a, boxes, slab, shift=0, fill=np.nan):
    """Box-packed form of a cube: step t holds box t of step t + shift (clamped to the cube) at the slab's origin, ``fill`` beside it."""
    out = np.full((len(boxes), a.shape[1]) + tuple(slab), fill, dtype=a.dtype)
    for t, (iw, ie, js, jn) in enumerate(boxes):
        out[t, :, :jn - js + 1, :ie - iw + 1] = a[min(max(t + shift, 0), a.shape[0] - 1), :, js:jn + 1, iw:ie + 1]
    return out


def cover(boxes, nt, ny, nx, reach):
    """bool [nt, ny, nx]: the points of step t that a box of steps t - reach .. t + reach covers (what the frame leaves)."""
    m = np.zeros((nt, ny, nx), dtype=bool)
    for t in range(nt):
        for s in range(max(t - reach, 0), min(t + reach, nt - 1) + 1):
            iw, ie, js, jn = boxes[s]
            m[t, js:jn + 1, iw:ie + 1] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# ring
# ---------------------------------------------------------------------------------------------------------------------------------
# (columns, storage, tuning f32_vec): the list of tests/test_gpu_ring.py (SHAPES), where it says which edge trip or vector form
# each width is for; tests/test_gpu_rowstats_records.py asserts the two lists are one
RING_SHAPES = ((7, "float64", 0), (8, "float64", 0), (64, "float64", 0), (65, "float64", 0), (128, "float64", 0), (129, "float64", 0),
               (130, "float64", 0), (256, "float32", 0), (260, "float32", 0), (258, "float32", 0), (257, "float32", 0), (260, "float32", 2))
RING_MODES = ("noq", "cube", "stencil")        # kernel modes 0, 2, 3
RING_GRID = dict(nt=3, nl=4, ny=7)
RING_ROWS = (1, 5)


def ring_ids():
    return tuple(f"ring-{nx}-{d}" + ("-f32vec2" if fv else "") + f"-{m}" for nx, d, fv in RING_SHAPES for m in RING_MODES)


@functools.lru_cache(maxsize=None)
def ring_dom(nx, dtype):
    return rr.ring_domain(RING_GRID["nt"], RING_GRID["nl"], RING_GRID["ny"], nx, seed=nx, dtype=np.dtype(dtype).type, lat0=-60.0, lat1=60.0)


def _ring(nx, dtype, fv, mode):
    dom = ring_dom(nx, dtype)
    boxes = [(0, nx - 1) + RING_ROWS]
    kw = dict(family="ring", kind="ring", tuning={"kernel": "row_sweep", **({"f32_vec": 2} if fv else {})}, runs=((0, 3, 0, 3),), **_mode_kw(mode))
    return dom, boxes, kw, [dict(trips_of(vec_of(dtype, nx, fv), 0, nx, nx), mode=mode)]


# ---------------------------------------------------------------------------------------------------------------------------------
# axes
# ---------------------------------------------------------------------------------------------------------------------------------
AXES_IDS = ("axes-sweep-float64", "axes-sweep-float32", "axes-block", "axes-tile", "axes-tilewide", "axes-plane")
AXES_SWEEP_WIDTHS = (5, 40, 131)


def _axes(what, dtype=None):
    if what == "sweep":
        nx = 392
        vec = vec_of(dtype, nx)
        dom = domain(dtype, nt=4, nl=9, ny=8, nx=nx, axes="uneven")
        boxes = [(1, w, 1, 6) for w in AXES_SWEEP_WIDTHS]
        kw = dict(family="axes", kind="fixed", tuning={"kernel": "row_sweep"}, runs=((0, 4, 0, 4), (0, 4, 1, 2)), **_mode_kw("stencil"))
        exp = [trips_of(vec, b[0], b[1] - b[0] + 1, nx) for b in boxes]
    elif what == "block":
        dom, boxes, kw, exp = _block("float64", 212, 1, axes="uneven", widths=AXES_SWEEP_WIDTHS)
    elif what in ("tile", "tilewide"):
        dom, boxes, kw, exp = _tile("float64", "nb", "even", 9, call="wide" if what == "tilewide" else "narrow", axes="uneven")
    else:
        dom, boxes, kw, exp = _plane("float64", 9, axes="uneven")
    kw = dict(kw, family="axes", runs_on=what)
    exp = {"boxes": exp, "asymmetry": axes_asymmetry(dom, boxes)}
    return dom, boxes, kw, exp


# ---------------------------------------------------------------------------------------------------------------------------------
# nan: one NaN at a time inside the box
# ---------------------------------------------------------------------------------------------------------------------------------
NAN_IDS = ("nan-sweep-f64v2", "nan-sweep-f32v4", "nan-tile", "nan-plane")
NAN_STEP_BOXES = tuple((2 + t, 41 + t, 1 + t % 2, 8 + t % 2) for t in range(5))      # 40 x 8 points, moving a column per step


def _plants(t, k, j, iw, ie, mid):
    """(name, field index (0 T, 1 u), (step, level, grid row, grid column)): the row looked at is (t, k, j).  Its first element is the
    shift of every sum, ``mid`` lies in a middle trip, the last element ends an edge trip; then T one row, level and step away."""
    return (("T_first", 0, (t, k, j, iw)), ("T_middle", 0, (t, k, j, mid)), ("T_last", 0, (t, k, j, ie)), ("u_first", 1, (t, k, j, iw)),
            ("T_row_below", 0, (t, k, j - 1, mid)), ("T_row_above", 0, (t, k, j + 1, mid)), ("T_level_above", 0, (t, k - 1, j, mid)),
            ("T_level_below", 0, (t, k + 1, j, mid)), ("T_step_before", 0, (t - 1, k, j, mid)), ("T_step_after", 0, (t + 1, k, j, mid)))


def planted(dom, plant):
    """``dom`` with the plant's one element NaN (a copy)."""
    f = [a.copy() for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    f[plant[1]][plant[2]] = np.nan
    return o.Domain(*f, dom.lat, dom.lon, dom.level, dom.time_s)


def _nan(what, form=None):
    if what == "sweep":
        dtype, nx, fv = SWEEP_FORMS[form]
        vec = vec_of(dtype, nx, fv)
        dom = domain(dtype, nx=nx, **SWEEP_GRID)
        box = (1, 64 * vec * 2 + 5) + SWEEP_ROWS                  # shift 1; three trips, the second a middle trip
        kw = dict(family="nan", kind="fixed", tuning={"kernel": "row_sweep"}, runs=((0, 4, 0, 4),), **_mode_kw("stencil"))
        kw["plants"] = _plants(1, 1, 2, box[0], box[1], box[0] + 64 * vec + 10)
        exp = dict(trips_of(vec, box[0], box[1] - box[0] + 1, nx), form=form)
        return dom, [box], kw, exp
    boxes = list(NAN_STEP_BOXES)
    if what == "tile":
        dom = domain("float64", nt=5, nl=10, **TILE_GRID)
        kw = dict(family="nan", kind="moving", mode="nb", tunings=[{"kernel": "box_tile"}])
    else:
        dom = domain("float64", nt=5, nl=10, **PLANE_GRID)
        kw = dict(family="nan", kind="packed", slab=PLANE_SLAB, tunings=[{"kernel": "box_plane"}])
    iw, ie, js, _ = boxes[2]
    kw["plants"] = _plants(2, 4, js + 3, iw, ie, iw + 20)
    return dom, boxes, kw, {"row": (2, 4, js + 3)}


# ---------------------------------------------------------------------------------------------------------------------------------
# steps: the boxes of several tracks over one cube (lec_rowstats_steps)
# ---------------------------------------------------------------------------------------------------------------------------------
STEPS_ID = "steps-float64"
# (cube steps of the track, its boxes): A every step 0..3; B every second step (its time neighbours lie two cube steps away); C two
# steps that A reads too, in the grid's corners.  Every track starts and ends inside the cube's series: six track ends
STEPS_TRACKS = (((0, 1, 2, 3), tuple((5 + t, 25 + t, 2, 7) for t in range(4))),
                ((0, 2, 4), tuple((20 + 2 * i, 64 + 2 * i, 1 + i, 9 + i) for i in range(3))),
                ((2, 3), ((0, 3, 0, 2), (70, 73, 9, 11))))


def _steps():
    dom = domain("float64", nt=5, nl=10, **TILE_GRID)
    table = [(s[i], s[max(i - 1, 0)], s[min(i + 1, len(s) - 1)]) for s, _ in STEPS_TRACKS for i in range(len(s))]
    boxes = [b for _, bs in STEPS_TRACKS for b in bs]
    kw = dict(family="tile", kind="steps", tuning={"kernel": "box_tile"}, table=table, tracks=STEPS_TRACKS)
    read = [r[0] for r in table]
    exp = dict(tracks=len(STEPS_TRACKS), same_step=sorted({s for s in read if read.count(s) > 1}), two_steps_away=any(abs(r[0] - r[1]) == 2 for r in table),
               track_ends=sum(r[0] == r[1] or r[0] == r[2] for r in table))
    return dom, boxes, kw, exp


def steps_cover(table, boxes, nt, ny, nx):
    """bool [nt, ny, nx]: the points of cube step s that a box reading s, or taking a time neighbour from s, covers."""
    m = np.zeros((nt, ny, nx), dtype=bool)
    for row, (iw, ie, js, jn) in zip(table, boxes):
        for s in row:
            m[s, js:jn + 1, iw:ie + 1] = True
    return m


def track_domain(dom, steps):
    """The sub-series of a track: the cube's steps it reads, as a series of their own."""
    i = list(steps)
    return o.Domain(dom.tair[i], dom.u[i], dom.v[i], dom.omega[i], dom.geopt[i], dom.lat, dom.lon, dom.level, dom.time_s[i])


# ---------------------------------------------------------------------------------------------------------------------------------
# conditioning: rows that strain the single-sweep form's shift
# ---------------------------------------------------------------------------------------------------------------------------------
COND_IDS = ("cond-a", "cond-b", "cond-c")
COND_WIDTHS = (100, 200, 300)               # one, two and three trips of double2
COND_NX = 392
# The chosen R, by the rule: the largest of 100, 30, 10 at which the float64 shifted sums (tests/test_rowstats_cases_cpu.py:
# shifted_records, NumPy from the formulas in lec_rowsweep.hip's header) stay below a tenth of the 1e-11 bar on cases b and c.
# Measured (slots 5..21, of the statistic's largest value): R = 100: 5.8e-12 (b), 4.5e-13 (c); R = 30: 7.7e-13 (b), 6.2e-13 (c).
COND_R = 30


@functools.lru_cache(maxsize=None)
def smooth_domain(noise, displaced, R=COND_R):
    """The smooth part of ``helpers.synthetic_domain`` on the sweep grid, with a zonal wave added to u and Phi, which have none there
    (a statistic that is 0 for every row has no scale to be judged by) and T's wave at half its amplitude, plus ``noise`` times that
    function's noise.  The eddy amplitude of a T row is then 0.5e-3 .. 2.7e-3 of its mean.  ``displaced``: how many of T, u, v, omega, Phi have the box's west column (column 1)
    displaced by R standard deviations of their row (over the widest box)."""
    nt, nl, ny, nx = SWEEP_GRID["nt"], SWEEP_GRID["nl"], SWEEP_GRID["ny"], COND_NX
    rng = np.random.default_rng(11)
    lat, lon = np.linspace(-60.0, -10.0, ny), 0.125 * np.arange(nx)
    level, time_s = np.linspace(10000.0, 100000.0, nl), np.arange(nt) * 21600.0
    phi, lam = np.deg2rad(lat)[None, None, :, None], np.deg2rad(lon)[None, None, None, :]
    p, tt, shp = level[None, :, None, None], (np.arange(nt) / nt)[:, None, None, None], (nt, nl, ny, nx)
    n = lambda amp: noise * amp * rng.standard_normal(shp)
    f = [288.0 * (p / 1e5) ** 0.19 + 10.0 * np.cos(2 * phi) * (p / 1e5) + 1.0 * np.sin(3 * lam + tt) + n(1.0),
         25.0 * np.cos(phi) * (1 - p / 1.2e5) + 0.5 * np.cos(5 * lam - tt) + n(5.0),
         3.0 * np.sin(2 * lam) * np.cos(phi) + 0.1 * np.cos(7 * lam) + n(3.0),
         0.05 * np.sin(3 * lam) * np.cos(phi) + n(0.1),
         o.G * 7000.0 * np.log(1e5 / p) + 100.0 * np.sin(4 * lam + tt) * np.cos(phi) + n(100.0)]
    f = [np.array(np.broadcast_to(a, shp)) for a in f]
    for a in f[:displaced]:
        a[..., 1] += R * a[..., 1:1 + max(COND_WIDTHS)].std(axis=-1)
    return o.Domain(*f, lat, lon, level, time_s)


def _cond(which):
    """a: no noise at all.  b: 1 % noise, the west column displaced by COND_R = 30 row standard deviations in T alone.  c: in all five
    fields.  R by the rule in the module's COND_R comment: at R = 30 the float64 shifted sums lie at 7.7e-13 (b) and 6.2e-13 (c) of the
    statistics' largest values (the measure of slots 5..21), below the tenth of the bar the rule asks for; at R = 100 case b is at
    5.8e-12.  Formed about 0 instead, the float64 sums of case a are off by 2.3e-9."""
    dom = smooth_domain(*{"a": (0.0, 0), "b": (0.01, 1), "c": (0.01, 5)}[which])
    boxes = [(1, w) + SWEEP_ROWS for w in COND_WIDTHS]
    kw = dict(family="conditioning", kind="fixed", tuning={"kernel": "row_sweep"}, runs=((0, 4, 0, 4),), **_mode_kw("stencil"))
    exp = [dict(trips_of(2, 1, w, COND_NX), R={"a": 0}.get(which, COND_R)) for w in COND_WIDTHS]
    return dom, boxes, kw, exp


# ---------------------------------------------------------------------------------------------------------------------------------
# build and reference
# ---------------------------------------------------------------------------------------------------------------------------------
FAMILY_IDS = {"sweep": sweep_ids(), "block": block_ids(), "tile": tile_ids() + (STEPS_ID,), "plane": plane_ids(), "ring": ring_ids(), "axes": AXES_IDS,
              "conditioning": COND_IDS, "nan": NAN_IDS}
ALL_IDS = tuple(i for ids in FAMILY_IDS.values() for i in ids)


@functools.lru_cache(maxsize=None)
def build(case_id):
    """(dom, boxes, call keywords, expectations) of a case by id, built once per process: read-only."""
    p = case_id.split("-")
    if p[0] == "sweep":
        return _sweep(p[1], int(p[2][1:]), p[3])
    if p[0] == "block":
        return _block(p[1], int(p[2]), int(p[3][1:]), lon=p[4] if len(p) > 4 else "even")
    if p[0] == "tile":
        return _tile(p[1], p[2], p[3], int(p[4][2:]), p[5])
    if p[0] == "steps":
        return _steps()
    if p[0] == "plane":
        return _plane(p[1], int(p[2][2:]))
    if p[0] == "ring":
        return _ring(int(p[1]), p[2], 2 if "f32vec2" in p else 0, p[-1])
    if p[0] == "axes":
        return _axes(p[1], p[2] if len(p) > 2 else None)
    if p[0] == "nan":
        return _nan(p[1], p[2] if len(p) > 2 else None)
    if p[0] == "cond":
        return _cond(p[1])
    raise KeyError(case_id)


def fixed_records(dom, box, kw, run, extended=True, ring=False):
    """Records [h1 - h0, nl, nyb, 28] of one box over the cube of a run (every step of the cube, processed or not)."""
    sub = steps_of(dom, run[0], run[1])
    args = dict(dTdt=dtdt_cube(sub) if kw["dtdt"] else None, with_q=kw["with_q"], with_phi=kw["with_phi"], extended=extended)
    if ring:
        return rs.row_records_ring(sub, dom.lat[box[2]], dom.lat[box[3]], **args)
    return rs.row_records(sub, limits_of(dom, box), **args)


def moving_records(dom, boxes, kw, extended=True):
    """Records [nt, nl, nyb_max, 28] of a box per step; dT/dt is np.gradient over the cube's time axis in every mode (the "cube" mode
    hands the kernel that cube, rounded to the storage dtype: fp64 there)."""
    dT = dtdt_cube(dom) if kw.get("mode") == "cube" else None
    return rs.row_records_moving(dom, [limits_of(dom, b) for b in boxes], dT, extended=extended)


def records_of(dom, boxes, kw, extended=True):
    """Per-step cases: the records [nt, nl, nyb_max, 28]; a step table: one such array per track, each from the track's own sub-series;
    fixed-box and ring cases: {(h0, h1): [records of box 0, box 1, ...]} by the cube a run holds."""
    if kw["kind"] in ("moving", "packed"):
        return moving_records(dom, boxes, kw, extended)
    if kw["kind"] == "steps":
        return [rs.row_records_moving(track_domain(dom, s), [limits_of(dom, b) for b in bs], extended=extended) for s, bs in kw["tracks"]]
    cubes = sorted({r[:2] for r in kw["runs"]})
    return {c: [fixed_records(dom, b, kw, c, extended, ring=kw["kind"] == "ring") for b in boxes] for c in cubes}


def reference(case_id, extended=True):
    return _reference(case_id, bool(extended))


@functools.lru_cache(maxsize=None)
def _reference(case_id, extended):
    """``reference``: ``records_of`` a case -- of a nan case: {plant name: records_of the planted domain}.  float64, evaluated in np.longdouble
    (``extended``) or float64: computed once per process and shared -- read-only."""
    dom, boxes, kw, _ = build(case_id)
    if "plants" in kw:
        return {pl[0]: records_of(planted(dom, pl), boxes, kw, extended) for pl in kw["plants"]}
    return records_of(dom, boxes, kw, extended)


# ---------------------------------------------------------------------------------------------------------------------------------
# the measure
# ---------------------------------------------------------------------------------------------------------------------------------
def row_max(dom, box, h0=0, h1=None):
    """max |X| over a row's box elements, [steps, nl, nyb, 5] for T, u, v, omega, Phi (the stored values as fp64; NaNs left out)."""
    iw, ie, js, jn = box
    a = [np.abs(f[h0:h1, :, js:jn + 1, iw:ie + 1].astype(np.float64)) for f in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    return np.stack([np.where(np.isnan(x), 0.0, x).max(axis=-1) for x in a], axis=-1)


def moment_error(got, ref):
    """Slots 5..21, per slot: max over rows |got - ref| / max over rows |ref| (rows on the leading axes).  inf where NaNs are not at
    the reference's places; a slot whose reference is 0 everywhere must be 0."""
    got, ref = np.asarray(got)[..., rs.MOMENTS].reshape(-1, 17), np.asarray(ref)[..., rs.MOMENTS].reshape(-1, 17)
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return np.full(17, np.inf)
    top = np.where(np.isnan(ref), 0.0, np.abs(ref)).max(axis=0)
    err = np.where(np.isnan(ref), 0.0, np.abs(got - ref)).max(axis=0)
    return np.where(top > 0, err / np.where(top > 0, top, 1.0), np.where(err > 0, np.inf, 0.0))


def mean_error(got, ref, xmax, nxb):
    """Slots 0..4: the largest |got - ref| / ((nxb + 4) 2^-53 max |X|) over the rows -- the classical bound of a weighted sum of nxb
    terms in any order plus the shift's subtraction and addition; <= 1 passes.  NaNs must sit at the reference's places (else inf)."""
    got, ref = np.asarray(got)[..., rs.MEANS], np.asarray(ref)[..., rs.MEANS]
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return float("inf")
    bound = (nxb + 4) * EPS * xmax
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, np.abs(got - ref) / bound, np.where(got == ref, 0.0, np.inf))
    return float(np.where(np.isnan(ref), 0.0, r).max())
