"""Case builders for the ring pass, the spectra, the sections and the maps on uneven axes and inner bands  --  TEST INFRASTRUCTURE ONLY;
no GPU, no torch.

Every GPU test of lec_rowstats_ring, lec_rowspec*, lec_level_spec*, lec_sections and lec_maps builds its domain with
``ring_restatement.ring_domain``: linspace latitudes and levels, 6-hourly steps, the band on the whole latitude axis.  There np.gradient's
middle coefficient is 0 at every interior point, every interior row, level and step shares one coefficient triple, and ``js = 0``.  The
domains here are ``ring_domain`` on uneven axes: the latitudes and time steps are replaced after generation (the fields stay as generated:
the restatements only see values on axes, as in ``stage2_cases._uneven``), the levels are handed to ``ring_domain`` -- T is generated
as a function of p, and relabelling the levels of a finished T profile makes the static stability negative at the closely spaced bottom
levels, where the 0.03 clamp then binds:

  latitudes  ``stage2_cases.uneven_axis(-70, 70, ny)``                      levels  ``rowstats_cases.AXES_LEVELS_HPA`` (9), or
  time       ``rowstats_cases.AXES_HOURS`` (4 steps: 1-, 3-, 2-hour steps)           ``uneven_axis(5000, 97500, 17)``
  longitudes the full ring of ``ring_domain``

  domain     cube (lat x lon)  band rows  levels  what it is for
  narrow     9 x 70            1 .. 7     9       the maps' 64-column wave seam (a ring of 70); the open box is columns 3 .. 67: 65 columns,
                                                  whose last lies alone in the second wave
  tall       68 x 16           1 .. 66    9       the second 64-row trip of lec_section_rows_kernel and lec_mapcol_coef_kernel, the tall path
                                                  of the level and level-spectrum kernels
  levels17   7 x 16            1 .. 5     17      kFoldBatch and the level march: two full batches of 8 levels plus one

The frame.  In every case the cube rows outside the band are NaN in all five fields, in the ``_open`` cases the columns outside the box
as well (the framing of tests/test_gpu_rowstats_records.py).  The restatements crop before they differentiate, so they never see the
frame; a kernel that reads a row or column outside the box does not come out finite.

``build(case_id)`` returns ``(dom, box, expectations)``: the framed domain, the box (iw, ie, js, jn) and what the case claims about
itself, which tests/test_ring_axes_cpu.py checks on the restatements alone.  Case ids: ``narrow``, ``tall``, ``levels17``, ``narrow_f32``
(fp32 storage), ``narrow_nan``, each also with ``_open``.  ``clean(name, dtype)`` is the unframed domain.  Both cache: built once per
process, never written to.

``narrow_nan`` is ``narrow`` plus three plants, [step, level, row, column]:
  u[1, 4:6, 4, 10]            a gap two levels deep across unequal intervals, in u only;
  omega[2, 7:9, 2:4, 20:23]   the two bottom levels: the integral ends at level 6;
  tair[3, 0, 5, 63]           the top level, in the last lane of the first wave (its d/dlon neighbours are columns 62 and 64); it reaches
                              Q at step 2 through dT/dt.
All column values stay finite, and every term changes at its own set of steps (``expectations["changed"]``): the six per-term states of
lec_mapcol_col_kernel's level march differ from one another.

The records cases (``records_build``) hold lec_rowstats_ring to tests/rowstats_restatement.py on ``narrow``, in the measure of
tests/rowstats_cases.py.  They live here and not in that module's ``axes`` family: its CPU test asks every case of the family to see
swapped time coefficients, which a run without Q (mode 0) cannot.
"""
import functools

import numpy as np

from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests import rowstats_cases as rc
from tests.stage2_cases import interval_asymmetry, uneven_axis

FIELDS = ("tair", "u", "v", "omega", "geopt")
LAT0, LAT1 = -70.0, 70.0
NT = len(rc.AXES_HOURS)
# name: (cube rows, ring columns, band rows (js, jn), levels, the open box's columns (iw, ie))
DOMAINS = {"narrow": (9, 70, (1, 7), 9, (3, 67)), "tall": (68, 16, (1, 66), 9, (2, 13)), "levels17": (7, 16, (1, 5), 17, (2, 13))}
CLEAN_IDS = tuple(DOMAINS)
NAN_ID = "narrow_nan"
F32_ID = "narrow_f32"
# (field, (step, levels, rows, columns)) of narrow_nan
NAN_PLANTS = (("u", (1, slice(4, 6), 4, 10)), ("omega", (2, slice(7, 9), slice(2, 4), slice(20, 23))), ("tair", (3, 0, 5, 63)))
# term: the steps at which its column values differ from the clean case's (sections and maps, ring and open box alike)
NAN_CHANGED = {"Az": {3}, "Ae": {3}, "Kz": {1}, "Ke": {1}, "Cz": {2, 3}, "Ca": {2, 3}, "Ck": {1, 2}, "Ce": {2, 3}, "Gz": {1, 2, 3}, "Ge": {1, 2, 3}}


def levels_of(name):
    nl = DOMAINS[name][3]
    return np.asarray(rc.AXES_LEVELS_HPA, dtype=np.float64) * 100.0 if nl == len(rc.AXES_LEVELS_HPA) else uneven_axis(5000.0, 97500.0, nl)


@functools.lru_cache(maxsize=None)
def _clean(name, dtype):
    ny, nx, _, nl, _ = DOMAINS[name]
    dom = rr.ring_domain(NT, nl, ny, nx, seed=nx + ny + nl, dtype=np.dtype(dtype).type, lat0=LAT0, lat1=LAT1, level=levels_of(name))
    dom.lat = uneven_axis(LAT0, LAT1, ny)
    dom.time_s = np.asarray(rc.AXES_HOURS) * 3600.0
    return dom


def clean(name, dtype=np.float64):
    """The unframed fields of a domain on its uneven axes: read-only."""
    return _clean(name, np.dtype(dtype).name)


def even(name):
    """``ring_domain`` of the same size on its own even axes (what the sibling tests run on): read-only."""
    ny, nx, _, nl, _ = DOMAINS[name]
    return _even(ny, nx, nl)


@functools.lru_cache(maxsize=None)
def _even(ny, nx, nl):
    return rr.ring_domain(NT, nl, ny, nx, seed=nx + ny + nl, lat0=LAT0, lat1=LAT1)


def framed(dom, box, ring):
    """A copy of ``dom`` that is NaN outside the band's rows -- and, for an open box, outside its columns -- in all five fields."""
    iw, ie, js, jn = box
    keep = np.zeros(dom.tair.shape[2:], dtype=bool)
    keep[js:jn + 1, :] = True
    if not ring:
        keep[:, :iw] = False
        keep[:, ie + 1:] = False
    f = [np.ascontiguousarray(np.where(keep, getattr(dom, n), np.nan).astype(getattr(dom, n).dtype)) for n in FIELDS]
    return o.Domain(*f, dom.lat, dom.lon, dom.level, dom.time_s)


def limits_of(dom, box):
    """(south, north) of a band; ``rowstats_cases.limits_of`` gives all four."""
    return float(dom.lat[box[2]]), float(dom.lat[box[3]])


def parse(case_id):
    """(domain name, storage dtype, NaN plants?, ring?) of a case id."""
    ring = not case_id.endswith("_open")
    base = case_id[:-len("_open")] if not ring else case_id
    name = base.split("_")[0]
    if name not in DOMAINS or base not in (name, name + "_nan", name + "_f32") or (base != name and name != "narrow"):
        raise KeyError(case_id)
    return name, np.float32 if base.endswith("_f32") else np.float64, base.endswith("_nan"), ring


@functools.lru_cache(maxsize=None)
def build(case_id):
    """(framed domain, box (iw, ie, js, jn), expectations) of a case by id, built once per process: read-only."""
    name, dtype, nans, ring = parse(case_id)
    ny, nx, (js, jn), nl, cols = DOMAINS[name]
    dom = clean(name, dtype)
    box = (0, nx - 1, js, jn) if ring else (cols[0], cols[1], js, jn)
    if nans:
        f = {n: getattr(dom, n).copy() for n in FIELDS}
        for field, at in NAN_PLANTS:
            f[field][at] = np.nan
        dom = o.Domain(*[f[n] for n in FIELDS], dom.lat, dom.lon, dom.level, dom.time_s)
    exp = {"ring": ring, "nyb": jn - js + 1, "nxb": box[1] - box[0] + 1,
           "asymmetry": {"lat": interval_asymmetry(dom.lat[js:jn + 1]), "level": interval_asymmetry(dom.level),
                         "time": rc.asymmetry(rc.gradient_triples(dom.time_s))}}
    if nans:
        exp["changed"] = NAN_CHANGED
        exp["plants"] = NAN_PLANTS
    return framed(dom, box, ring), box, exp


# ---------------------------------------------------------------------------------------------------------------------------------
# records: lec_rowstats_ring on uneven axes, in the measure of tests/rowstats_cases.py
# ---------------------------------------------------------------------------------------------------------------------------------
RECORD_IDS = tuple(f"ring_axes-narrow-{d}-{m}" for d in ("float64", "float32") for m in rc.RING_MODES)
# the whole series, and steps 1, 2 of the four: the launch's first step has a predecessor, and tcoef is read at the cube's step
RECORD_RUNS = ((0, 4, 0, 4), (0, 4, 1, 2))


@functools.lru_cache(maxsize=None)
def records_build(case_id):
    """(clean domain, boxes, call keywords, expectations) of a records case, in the form of ``rowstats_cases.build``: the GPU test frames
    the fields itself."""
    _, name, dtype, mode = case_id.split("-")
    ny, nx, (js, jn), nl, _ = DOMAINS[name]
    dom = clean(name, dtype)
    boxes = [(0, nx - 1, js, jn)]
    kw = dict(family="ring_axes", kind="ring", tuning={"kernel": "row_sweep"}, runs=RECORD_RUNS, **rc._mode_kw(mode))
    exp = {"boxes": [dict(rc.trips_of(rc.vec_of(dtype, nx), 0, nx, nx), mode=mode)], "asymmetry": rc.axes_asymmetry(dom, boxes)}
    return dom, boxes, kw, exp


@functools.lru_cache(maxsize=None)
def records_reference(case_id, extended=True):
    """``rowstats_cases.records_of`` a records case: {(h0, h1): [records of the band]}, computed once per process -- read-only."""
    dom, boxes, kw, _ = records_build(case_id)
    return rc.records_of(dom, boxes, kw, bool(extended))


# ---------------------------------------------------------------------------------------------------------------------------------
# references: the restatements on a case, computed once per process and shared by the tests -- read-only
# ---------------------------------------------------------------------------------------------------------------------------------
def oracle_box(case_id, dom=None):
    """The oracle's ``Box`` of a case (fp32 storage: the float32-rounded fields as fp64): ``ring_restatement.ring_box`` of the band, or
    ``oracle.make_box`` of the open box.  ``dom``: another domain on the case's box (a mutant run, the even twin)."""
    from tests.helpers import as_f64
    d, box, exp = build(case_id)
    d = as_f64(d if dom is None else dom)
    south, north = limits_of(d, box)
    with np.errstate(invalid="ignore"):
        if exp["ring"]:
            return rr.ring_box(d, south, north)
        return o.make_box(d, d.lon[box[0]], d.lon[box[1]], south, north)


def restate(b, ring):
    """The sections and maps of a ``Box``: X [T, 10, nl, ny], its columns Xc [T, 10, ny] and mean Xm; the maps' columns C [T, 6, ny, nxb],
    Hovmoeller H [T, 6, nxb] and mean M."""
    from tests import maps_restatement as mr
    from tests import sections_restatement as sr
    with np.errstate(invalid="ignore"):
        X = sr.sections(b)
        C = mr.columns(mr.maps(b, ring), b.level)
        return {"X": X, "Xc": sr.columns(X, b.level), "Xm": sr.time_mean(X), "C": C, "H": mr.hovmoller(C, sr.area_weights(b)), "M": mr.time_mean(C)}


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """(box, ``restate`` of it) of a case."""
    b = oracle_box(case_id)
    return b, restate(b, build(case_id)[2]["ring"])
