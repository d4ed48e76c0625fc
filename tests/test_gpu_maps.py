"""-f [--periodic] --maps on the GPU: ``lec_maps`` through ``LECEngine.compute(..., maps=True)`` / ``map_stage`` against the CPU restatement
(tests/maps_restatement.py), against the same run's sections and against its scalars.

Shapes.  T = 5.  The seams of the kernel lie along longitude (one wave per 64 columns) and level (the march down a column): rings of 16,
64, 65 and 130 columns, 65 rows once (a second 64-row trip of the factors kernel), 70 levels once, open boxes whose edges lie inside a
wave and past a trip (columns 3 .. 127 of 130) and on the small axis (2 .. 13 of 16); fp64 storage and fp32 storage once (the restatement
is fed the float32-rounded fields as fp64).

Bars.  1e-9 of the term's scale (its largest |value| in the case) for the per-step maps, the Hovmoeller and the time mean against the
restatement, for the zonal average of a map row against the run's own ``section_lat`` and for that of the Hovmoeller against its scalars:
the project's parity bar.  NaN patterns are the restatement's exactly; chunk independence and ``maps=False`` are bit for bit.
Measured on MI355X: map_steps 5.2e-14, map_lon 4.6e-14, map_mean 2.6e-14, closure on section_lat 4.5e-15, on the scalars 9.9e-15 (each
test prints its own figure).
Uneven axes, inner bands (js > 0, NaN rows and columns around the box) and NaNs in the other fields: tests/test_gpu_ring_axes.py."""
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib
from lorenzcycletoolkit_amd.constants import MAP_TERMS, SCALAR_TERMS, SECTION_TERMS
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import maps_restatement as mr
from tests import ring_restatement as rr
from tests import sections_restatement as sr
from tests.helpers import as_f64

DEV = "cuda:0"
NT = 5
TOL = 1e-9
SOUTH, NORTH = -60.0, 60.0
# (kind, nx, (iw, ie), rows, levels, storage)
CASES = [("ring", 16, None, 5, 5, np.float64), ("ring", 64, None, 5, 5, np.float64), ("ring", 65, None, 5, 5, np.float64),
         ("ring", 130, None, 5, 5, np.float64), ("ring", 16, None, 65, 5, np.float64), ("ring", 65, None, 5, 70, np.float64),
         ("open", 130, (3, 127), 5, 5, np.float64), ("open", 16, (2, 13), 5, 5, np.float64), ("open", 130, (3, 127), 5, 5, np.float32)]
IDS = [f"{k}-{nx}cols-{ny}rows-{nl}lev-{np.dtype(d).name}" for k, nx, _, ny, nl, d in CASES]

_cache = {}


def _dom(nx, ny, nl, dtype=np.float64):
    key = ("dom", nx, ny, nl, np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = rr.ring_domain(NT, nl, ny, nx, seed=nx + ny + nl, dtype=dtype, lat0=SOUTH, lat1=NORTH)
    return _cache[key]


def _box(cols, dom):
    """The oracle's Box of the case (whole latitude axis; the ring, or the columns ``cols`` as a limited area)."""
    d = as_f64(dom)
    with np.errstate(invalid="ignore"):
        if cols is None:
            return rr.ring_box(d, SOUTH, NORTH)
        return o.make_box(d, dom.lon[cols[0]], dom.lon[cols[1]], SOUTH, NORTH)


def _restate(b, ring):
    """(C [T, 6, ny, nxb], H [T, 6, nxb], M [6, ny, nxb]) of the restatement on the box ``b``."""
    with np.errstate(invalid="ignore"):
        C = mr.columns(mr.maps(b, ring), b.level)
        return C, mr.hovmoller(C, sr.area_weights(b)), mr.time_mean(C)


def _reference(kind, nx, cols, ny, nl, dtype):
    """(box, C, H, M), computed once per case and shared."""
    key = ("ref", kind, nx, cols, ny, nl, np.dtype(dtype).name)
    if key not in _cache:
        b = _box(cols, _dom(nx, ny, nl, dtype))
        _cache[key] = (b,) + _restate(b, cols is None)
    return _cache[key]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _fields(dom):
    return [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]


def _engine(cols, dom):
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    if cols is None:
        return eng, eng.prepare_boxes([(0, dom.lon.size - 1, 0, dom.lat.size - 1)], ring=True)
    return eng, eng.prepare_boxes([(cols[0], cols[1], 0, dom.lat.size - 1)])


def _scale(ref, axes):
    """The term's scale: its largest finite |value| over ``axes`` (1.0 where the term has none)."""
    a = np.where(np.isnan(ref), -np.inf, np.abs(ref)).max(axis=axes, keepdims=True)
    return np.where(np.isfinite(a), a, 1.0)


def _close(got, ref, axes, what):
    """|got - ref| <= TOL * the term's scale, the NaN patterns equal; returns the largest error over scale."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern"
    err = np.nanmax(np.abs(got - ref) / _scale(ref, axes)) if np.isfinite(ref).any() else 0.0
    print(f"{what}: max error / scale = {err:.3e}")
    assert err <= TOL, (what, err)
    return err


@pytest.mark.parametrize("kind, nx, cols, ny, nl, dtype", CASES, ids=IDS)
def test_maps_match_restatement_and_close(kind, nx, cols, ny, nl, dtype):
    dom = _dom(nx, ny, nl, dtype)
    b, C, H, M = _reference(kind, nx, cols, ny, nl, dtype)
    ring = cols is None
    eng, pb = _engine(cols, dom)
    res = eng.compute(*_fields(dom), pb, time_s=dom.time_s, maps=True, map_steps=True, sections=True)
    steps, lon, mean = res.map_steps.cpu().numpy(), res.map_lon.cpu().numpy(), res.map_mean.cpu().numpy()
    tag = f"{kind} {nx}x{ny}x{nl} {np.dtype(dtype).name}"
    nxb = nx if ring else cols[1] - cols[0] + 1
    assert steps.shape == (NT, 6, ny, nxb) and lon.shape == (NT, 6, nxb) and mean.shape == (6, ny, nxb)
    _close(steps, C, (0, 2, 3), tag + " map_steps")
    _close(lon, H, (0, 2), tag + " map_lon")
    _close(mean, M, (1, 2), tag + " map_mean")
    # closure on the same run's sections and scalars, with the box's own zonal average
    lat = res.section_lat.cpu().numpy()[:, [SECTION_TERMS.index(t) for t in MAP_TERMS]]
    _close(mr.zonal_average(steps, b, ring), lat, (0, 2), tag + " zonal average of map_steps against section_lat")
    own_sc = res.scalars.cpu().numpy()[:, [SCALAR_TERMS.index(t) for t in MAP_TERMS]]
    _close(mr.zonal_average(lon, b, ring), own_sc, (0,), tag + " zonal average of map_lon against the scalars")


NAN_CASES = {"interior level": dict(t=2, k=[2], row=2, cols=[7, 8]), "top level": dict(t=2, k=[0], row=2, cols=[7, 8]),
             "one point at every level": dict(t=2, k=[0, 1, 2, 3, 4], row=2, cols=[70])}


@pytest.mark.parametrize("kind", ["ring", "open"])
@pytest.mark.parametrize("case", list(NAN_CASES))
def test_nan_patterns_are_the_restatements(case, kind):
    nx, ny, nl = 130, 5, 5
    cols = None if kind == "ring" else (3, 127)
    c = NAN_CASES[case]
    base = _dom(nx, ny, nl)
    T = base.tair.copy()
    for k in c["k"]:
        T[c["t"], k, c["row"], c["cols"]] = np.nan
    dom = o.Domain(T, base.u, base.v, base.omega, base.geopt, base.lat, base.lon, base.level, base.time_s)
    Cr, Hr, Mr = _restate(_box(cols, dom), cols is None)
    eng, pb = _engine(cols, dom)
    res = eng.compute(*_fields(dom), pb, time_s=dom.time_s, maps=True, map_steps=True)
    steps = res.map_steps.cpu().numpy()
    _close(steps, Cr, (0, 2, 3), f"{kind} {case}: map_steps")
    _close(res.map_lon.cpu().numpy(), Hr, (0, 2), f"{kind} {case}: map_lon")
    _close(res.map_mean.cpu().numpy(), Mr, (1, 2), f"{kind} {case}: map_mean")
    ae = MAP_TERMS.index("Ae")                      # Ae reads T' of its own row and level only (sigma is clamped where it is NaN)
    if case == "one point at every level":          # a NaN point makes its whole row NaN at that level, through the zonal mean
        assert np.isnan(steps[c["t"], ae, c["row"]]).all() and np.isfinite(steps[c["t"], ae, [1, 3]]).all()
        assert np.isnan(res.map_lon.cpu().numpy()[c["t"], ae]).all()
    else:                                            # bridged or trimmed: the columns stay finite
        assert np.isfinite(steps[:, ae]).all()


def _records(dom, cols):
    """(engine, box, fields, rows, levraw) of the whole series."""
    eng, pb = _engine(cols, dom)
    f = _fields(dom)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    levraw = torch.empty((rows.shape[0], rows.shape[1], _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
    eng.level_stage(rows, pb, levraw)
    return eng, pb, f, rows, levraw


@pytest.mark.parametrize("kind", ["ring", "open"])
def test_chunk_independence_bit_for_bit(kind, monkeypatch):
    nx, ny, nl = 130, 5, 5
    cols = None if kind == "ring" else (3, 127)
    dom = _dom(nx, ny, nl)
    eng, pb, f, rows, levraw = _records(dom, cols)
    out = {}
    for name, chunk, cap in (("1", 1, None), ("2", 2, None), ("5", 5, None), ("cap", 5, 2)):
        if cap is not None:       # a byte cap that holds two steps of the column values and row factors: the chunk is cut in 2 + 2 + 1
            nxb = nx if cols is None else cols[1] - cols[0] + 1
            monkeypatch.setattr(LECEngine, "MAP_CHUNK_BYTES", cap * 8 * (6 * ny * nxb + nl * ny * _lib.LEC_MAPS_NCOEF))
        st = eng.map_begin(NT, pb, DEV)
        for a in range(0, NT, chunk):
            b = min(a + chunk, NT)
            eng.map_stage(*f[:4], rows[a:b], pb, levraw[a:b], st, a, time_s=dom.time_s, t_begin=a)
        if cap is not None:
            assert st["work"].shape[0] == cap
        res = eng.vertical_stage(levraw, pb)
        eng.map_finish(res, st)
        out[name] = (res.map_mean, res.map_lon)
        monkeypatch.undo()
    whole = eng.compute(*f, pb, time_s=dom.time_s, maps=True)
    kept = eng.compute(*f, pb, time_s=dom.time_s, maps=True, map_steps=True)
    out["compute"], out["map_steps"] = (whole.map_mean, whole.map_lon), (kept.map_mean, kept.map_lon)
    for name, got in out.items():
        for x, y, what in zip(got, out["5"], ("map_mean", "map_lon")):
            assert not torch.isnan(y).any()
            assert torch.equal(x, y), (name, what)


def test_without_maps_nothing_changes():
    dom = _dom(65, 5, 5)
    eng, pb = _engine(None, dom)
    for kw in (dict(time_s=dom.time_s), dict(time_s=dom.time_s, sections=True, wavenumbers=4)):
        plain, again = eng.compute(*_fields(dom), pb, **kw), eng.compute(*_fields(dom), pb, maps=False, **kw)
        with_maps = eng.compute(*_fields(dom), pb, maps=True, **kw)
        for f in dataclasses.fields(plain):
            a, b, c = getattr(plain, f.name), getattr(again, f.name), getattr(with_maps, f.name)
            if f.name.startswith("map_"):
                assert a is None and b is None, f.name
                continue
            assert (a is None) == (b is None) == (c is None), f.name
            if a is not None:
                assert torch.equal(a, b) and torch.equal(a, c), f.name
        assert with_maps.map_mean is not None and with_maps.map_lon is not None and with_maps.map_steps is None


def test_refused_in_words():
    dom = _dom(16, 5, 5)
    eng, pb = _engine((2, 13), dom)
    f = _fields(dom)
    box = (2, 13, 0, 4)
    with pytest.raises(ValueError, match="ONE fixed box"):
        eng.compute(*f, [box] * NT, time_s=dom.time_s, maps=True)
    with pytest.raises(ValueError, match="ONE fixed box"):
        eng.compute(*f, [box], time_s=dom.time_s, maps=True, per_step_boxes=True)
    with pytest.raises(ValueError, match="one process on one GPU"):
        eng.compute(*f, [box], time_s=dom.time_s, maps=True, merge_dropmask=lambda m: None)
    with pytest.raises(ValueError, match="one process on one GPU"):
        eng.compute(*f, [box], time_s=dom.time_s, maps=True, out=torch.empty((NT, LECEngine.packed_width(5)), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="dTdt cube is not supported"):
        eng.compute(*f, [box], time_s=dom.time_s, maps=True, dTdt=torch.zeros_like(f[0]))
    with pytest.raises(ValueError, match="maps need with_q"):
        eng.compute(*f, [box], time_s=dom.time_s, maps=True, with_q=False)
    with pytest.raises(ValueError, match="part of maps=True"):
        eng.compute(*f, [box], time_s=dom.time_s, map_steps=True)
    with pytest.raises(ValueError, match="at least 3 box columns"):
        eng.compute(*f, [(2, 3, 0, 4)], time_s=dom.time_s, maps=True)
