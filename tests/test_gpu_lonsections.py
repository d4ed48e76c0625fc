"""-f [--periodic] --lon-sections on the GPU: ``lec_lonsections`` through ``LECEngine.compute(..., lon_sections=True)`` /
``lonsection_stage`` against the CPU restatement (tests/lonsections_restatement.py), against the same run's latitude x pressure sections
and against its maps' Hovmoeller.

Shapes.  T = 5.  The seams of the kernel lie along longitude (one wave per 64 columns), along the rows (the march, and the factors
kernel's trips of 64) and along the levels (a wave's level has no neighbour at either end of the axis): rings of 16, 64, 65 and 130 columns
at 5 rows x 5 levels, 2 rows once (the first row is the last: both phi-neighbours are missing), 65 rows once, 2 levels once (both vertical
neighbours are missing at either level), 70 levels once, open boxes on columns 3 .. 127 of 130 and 2 .. 13 of 16, fp32 storage once (the
restatement is fed the float32-rounded fields as fp64).  Uneven axes and an inner band: the three domains of tests/ring_axes_cases.py.

Bars.  1e-9 of the term's scale (its largest |value| in the case) for the per-step sections and the time mean against the restatement,
for the box's zonal average against sum_j cw_j of the run's own ``section_steps`` and for the vertical trapezoid against its ``map_lon``:
the project's parity bar (tests/test_gpu_maps.py).  NaN patterns are the restatement's exactly; chunk independence and
``lon_sections=False`` are bit for bit.
Measured on MI355X: lonsection_steps 6.9e-13, lonsection_mean 4.2e-13 against the restatement (uneven axes: 9.4e-13, 6.8e-13); the zonal
average against sum_j cw_j section_steps 5.4e-15 (uneven axes 7.5e-15), the vertical trapezoid against map_lon 7.7e-16 (each test prints
its own figure)."""
import ctypes
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib
from lorenzcycletoolkit_amd.constants import MAP_TERMS, SECTION_TERMS
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import lonsections_restatement as lr
from tests import maps_restatement as mr
from tests import ring_axes_cases as ra
from tests import ring_restatement as rr
from tests import sections_restatement as sr
from tests import test_lonsections_cpu as cpu
from tests.helpers import as_f64

DEV = "cuda:0"
NT = 5
TOL = 1e-9
SOUTH, NORTH = -60.0, 60.0
SEC_IDX = [SECTION_TERMS.index(t) for t in MAP_TERMS]
# (kind, nx, (iw, ie), rows, levels, storage)
CASES = [("ring", 16, None, 5, 5, np.float64), ("ring", 64, None, 5, 5, np.float64), ("ring", 65, None, 5, 5, np.float64),
         ("ring", 130, None, 5, 5, np.float64), ("ring", 16, None, 2, 5, np.float64), ("ring", 16, None, 65, 5, np.float64),
         ("ring", 16, None, 5, 2, np.float64), ("ring", 65, None, 5, 70, np.float64),
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
    """(X [T, 6, nl, nxb], M [6, nl, nxb]) of the restatement on the box ``b``."""
    with np.errstate(invalid="ignore"):
        X = lr.lon_sections(mr.maps(b, ring), sr.area_weights(b))
        return X, lr.time_mean(X)


def _reference(kind, nx, cols, ny, nl, dtype):
    """(box, X, M), computed once per case and shared."""
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


def _closures(res, b, ring, tag):
    """Both closures of the issue on one run that also carries ``section_steps`` and ``map_lon``."""
    steps = res.lonsection_steps.cpu().numpy()
    cw = sr.area_weights(b)
    sec = res.section_steps.cpu().numpy()[:, SEC_IDX]                   # [T, 6, nl, nyb]
    S = np.zeros(sec.shape[:3])
    for j in range(sec.shape[3]):
        S = S + cw[j] * sec[..., j]
    _close(mr.zonal_average(steps, b, ring), S, (0, 2), tag + " zonal average of lonsection_steps against sum_j cw_j section_steps")
    _close(lr.columns(steps, b.level), res.map_lon.cpu().numpy(), (0, 2), tag + " vertical trapezoid of lonsection_steps against map_lon")


@pytest.mark.parametrize("kind, nx, cols, ny, nl, dtype", CASES, ids=IDS)
def test_lon_sections_match_restatement_and_close(kind, nx, cols, ny, nl, dtype):
    dom = _dom(nx, ny, nl, dtype)
    b, X, M = _reference(kind, nx, cols, ny, nl, dtype)
    ring = cols is None
    eng, pb = _engine(cols, dom)
    res = eng.compute(*_fields(dom), pb, time_s=dom.time_s, lon_sections=True, lon_section_steps=True, sections=True, section_steps=True,
                      maps=True)
    steps, mean = res.lonsection_steps.cpu().numpy(), res.lonsection_mean.cpu().numpy()
    tag = f"{kind} {nx}x{ny}x{nl} {np.dtype(dtype).name}"
    nxb = nx if ring else cols[1] - cols[0] + 1
    assert steps.shape == (NT, 6, nl, nxb) and mean.shape == (6, nl, nxb)
    assert np.isfinite(X).all()
    _close(steps, X, (0, 2, 3), tag + " lonsection_steps")
    _close(mean, M, (1, 2), tag + " lonsection_mean")
    _closures(res, b, ring, tag)


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
    Xr, Mr = _restate(_box(cols, dom), cols is None)
    eng, pb = _engine(cols, dom)
    res = eng.compute(*_fields(dom), pb, time_s=dom.time_s, lon_sections=True, lon_section_steps=True)
    steps = res.lonsection_steps.cpu().numpy()
    _close(steps, Xr, (0, 2, 3), f"{kind} {case}: lonsection_steps")
    _close(res.lonsection_mean.cpu().numpy(), Mr, (1, 2), f"{kind} {case}: lonsection_mean")
    ae = MAP_TERMS.index("Ae")                      # Ae reads T' of its own row and level only
    for k in c["k"]:                                # a NaN point makes its level NaN at EVERY column, through the row's zonal mean
        assert np.isnan(steps[c["t"], ae, k]).all()
    assert np.isfinite(steps[[0, 4], ae]).all()
    assert np.isnan(res.lonsection_mean.cpu().numpy()[ae, c["k"]]).all()


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
    nxb = nx if cols is None else cols[1] - cols[0] + 1
    out = {}
    for name, chunk, cap in (("1", 1, None), ("2", 2, None), ("5", 5, None), ("cap", 5, 2)):
        if cap is not None:       # a byte cap that holds two steps of the sections and row factors: the chunk is cut in 2 + 2 + 1
            monkeypatch.setattr(LECEngine, "MAP_CHUNK_BYTES", cap * 8 * (6 * nl * nxb + nl * ny * _lib.LEC_MAPS_NCOEF))
        st = eng.lonsection_begin(NT, pb, DEV)
        for a in range(0, NT, chunk):
            b = min(a + chunk, NT)
            eng.lonsection_stage(*f[:4], rows[a:b], pb, levraw[a:b], st, a, time_s=dom.time_s, t_begin=a)
        if cap is not None:
            assert st["work"].shape[0] == cap
        res = eng.vertical_stage(levraw, pb)
        eng.lonsection_finish(res, st)
        out[name] = res.lonsection_mean
        monkeypatch.undo()
    out["compute"] = eng.compute(*f, pb, time_s=dom.time_s, lon_sections=True).lonsection_mean
    kept = eng.compute(*f, pb, time_s=dom.time_s, lon_sections=True, lon_section_steps=True)
    out["lon_section_steps"] = kept.lonsection_mean
    assert not torch.isnan(out["5"]).any()
    for name, got in out.items():
        assert torch.equal(got, out["5"]), name


def test_flag_off_and_on_keep_every_other_bit():
    dom = _dom(65, 5, 5)
    eng, pb = _engine(None, dom)
    for kw in (dict(time_s=dom.time_s), dict(time_s=dom.time_s, sections=True, maps=True, wavenumbers=4)):
        plain, again = eng.compute(*_fields(dom), pb, **kw), eng.compute(*_fields(dom), pb, lon_sections=False, **kw)
        with_ls = eng.compute(*_fields(dom), pb, lon_sections=True, **kw)
        for f in dataclasses.fields(plain):
            a, b, c = getattr(plain, f.name), getattr(again, f.name), getattr(with_ls, f.name)
            if f.name.startswith("lonsection_"):
                assert a is None and b is None, f.name
                continue
            assert (a is None) == (b is None) == (c is None), f.name
            if a is not None:
                assert torch.equal(a, b) and torch.equal(a, c), f.name
        assert with_ls.lonsection_mean is not None and with_ls.lonsection_steps is None


@pytest.mark.parametrize("case_id", [n + s for n in ra.CLEAN_IDS for s in ("", "_open")])
def test_uneven_axes_and_inner_bands(case_id):
    """The three domains of tests/ring_axes_cases.py: uneven latitudes, levels (17 among them) and time steps, js > 0, NaN rows -- and for
    an open box NaN columns -- around the box."""
    dom, box, exp = ra.build(case_id)
    ring = exp["ring"]
    b = ra.oracle_box(case_id)
    X, M = _restate(b, ring)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    pb = eng.prepare_boxes([box], ring=True) if ring else eng.prepare_boxes([box])
    res = eng.compute(*[_dev(getattr(dom, n)) for n in ra.FIELDS], pb, time_s=dom.time_s, lon_sections=True, lon_section_steps=True,
                      sections=True, section_steps=True, maps=True)
    assert box[2] > 0 and np.isfinite(X).all()
    _close(res.lonsection_steps.cpu().numpy(), X, (0, 2, 3), case_id + " lonsection_steps")
    _close(res.lonsection_mean.cpu().numpy(), M, (1, 2), case_id + " lonsection_mean")
    _closures(res, b, ring, case_id)


def test_engine_refusals_in_words():
    dom = _dom(16, 5, 5)
    eng, pb = _engine((2, 13), dom)
    f = _fields(dom)
    box = (2, 13, 0, 4)
    kw = dict(time_s=dom.time_s, lon_sections=True)
    with pytest.raises(ValueError, match="ONE fixed box"):
        eng.compute(*f, [box] * NT, **kw)
    with pytest.raises(ValueError, match="ONE fixed box"):
        eng.compute(*f, [box], per_step_boxes=True, **kw)
    with pytest.raises(ValueError, match="one process on one GPU"):
        eng.compute(*f, [box], merge_dropmask=lambda m: None, **kw)
    with pytest.raises(ValueError, match="dTdt cube is not supported"):
        eng.compute(*f, [box], dTdt=torch.zeros_like(f[0]), **kw)
    with pytest.raises(ValueError, match="longitude-pressure sections need with_q"):
        eng.compute(*f, [box], with_q=False, **kw)
    with pytest.raises(ValueError, match="longitude-pressure sections need at least 3 box columns"):
        eng.compute(*f, [(2, 3, 0, 4)], **kw)
    from tests.helpers import synthetic_domain
    un = synthetic_domain(NT, 5, 5, 16, seed=1, nonuniform_lon=True)
    eng2 = LECEngine(un.lat, un.lon, un.level, device=DEV)
    with pytest.raises(ValueError, match="longitude-pressure sections need evenly spaced longitudes"):
        eng2.compute(*[_dev(a) for a in (un.tair, un.u, un.v, un.omega, un.geopt)], [box], **kw)


# -- the C call's refusals on real arguments: nothing is launched ---------------------------------------------------------------------
SENTINEL = -12345.0


def _real_args():
    """A valid ``lec_lonsections`` call with the scalars of ``test_lonsections_cpu.fixed_args`` on real device arrays; returns (args, the two
    outputs prefilled with SENTINEL, whatever must stay alive)."""
    proto = cpu.fixed_args()
    dom = rr.ring_domain(proto.nt, proto.nl, proto.ny, proto.nx, seed=3, lat0=SOUTH, lat1=NORTH)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    pb = eng.prepare_boxes([(proto.iw, proto.ie, proto.js, proto.jn)])
    f = _fields(dom)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    levraw = torch.empty((proto.nt, proto.nl, _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
    eng.level_stage(rows, pb, levraw)
    a, b = proto.t_begin, proto.t_begin + proto.t_count
    nyb, nxb = proto.jn - proto.js + 1, proto.ie - proto.iw + 1
    f64 = dict(dtype=torch.float64, device=DEV)
    keep = dict(f=f, rows=rows[a:b].contiguous(), levraw=levraw[a:b].contiguous(), tcoef=eng.time_coefs_device(dom.time_s), eng=eng, pb=pb,
                coef=torch.empty((proto.t_count, proto.nl, nyb, _lib.LEC_MAPS_NCOEF), **f64))
    sec = torch.full((proto.t_count, 6, proto.nl, nxb), SENTINEL, **f64)
    tot = torch.full((6, proto.nl, nxb), SENTINEL, **f64)
    p = lambda t: t.data_ptr()
    for name, t in (("tair_d", f[0]), ("u_d", f[1]), ("v_d", f[2]), ("omega_d", f[3]), ("rows_d", keep["rows"]), ("levraw_d", keep["levraw"]),
                    ("lattab2_d", pb.dev["lattab2"]), ("levtab2_d", eng._levtab2), ("lattab_d", pb.dev["lattab"]), ("levtab_d", eng._levtab),
                    ("tcoef_d", keep["tcoef"]), ("coef_d", keep["coef"]), ("lonsec_d", sec), ("lonsecsum_d", tot)):
        setattr(proto, name, p(t))
    proto.inv_hdeg = float(pb.bt.boxtab[0, 2])
    proto.stream = torch.cuda.current_stream(DEV).cuda_stream
    return proto, sec, tot, keep


def test_c_call_refusals_launch_nothing():
    lib = _lib.load()
    cases = [(f, c, 1) for f, c in cpu.FIXED_ARG] + [(f, c, 2) for f, c in cpu.FIXED_UNSUPPORTED]
    for field, change, code in cases:
        a, sec, tot, keep = _cache.get("cargs") or _cache.setdefault("cargs", _real_args())
        b = _lib.LonSectionsArgs.from_buffer_copy(a)
        change(b)
        with torch.cuda.device(DEV):
            assert lib.lec_lonsections(ctypes.byref(b)) == code, field
        msg = lib.lec_last_error()
        assert msg.startswith(b"lec_lonsections:") and field.encode() in msg, (field, msg)
        torch.cuda.synchronize()
        assert bool((sec == SENTINEL).all()) and bool((tot == SENTINEL).all()), field
    # ... and the arguments are otherwise valid: unchanged, the call runs and gives compute's numbers
    a, sec, tot, keep = _cache["cargs"]
    tot.zero_()
    with torch.cuda.device(DEV):
        assert lib.lec_lonsections(ctypes.byref(a)) == 0, lib.lec_last_error()
    torch.cuda.synchronize()
    assert not bool((sec == SENTINEL).any()) and bool(torch.isfinite(sec).all())
    s = sec[0].clone()
    for t in range(1, sec.shape[0]):
        s = s + sec[t]
    assert torch.equal(tot, s)
