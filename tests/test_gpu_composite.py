"""-t / -c --composites on the GPU: ``lec_composite`` through ``LECEngine.compute(..., per_step_boxes=True, composites=True)`` /
``composite_stage`` against the CPU restatement (tests/composite_restatement.py) and against the same run's scalars.

Shapes.  T = 5, every step's box at another place of a grid a few points larger than the box: step 0 touches the domain's west and south
edge, step 1 its east and north edge.  The seams of the kernel lie along longitude (one wave per 64 box columns), along the rows (the
factors kernel walks them in trips of 64) and along the levels (the march down a column): boxes of 5, 63, 64, 65 and 130 columns, 65 rows
once, 70 levels once.  Layouts: the box-packed series in fp64 (dT/dt as a cube) and in fp32 (tm / tp; the restatement is fed the
float32-rounded fields as fp64), the unpacked cube with a dT/dt cube once and with its own time neighbours once.

Bars.  1e-9 of the term's scale (its largest |value| in the case) for the per-step columns, the Hovmoeller and the time mean against the
restatement, for the box's zonal average of the Hovmoeller against the run's own scalars, and for a stationary track against
``compute(maps=True)`` on that fixed box: the project's parity bar (tests/test_gpu_maps.py).  NaN patterns are the restatement's exactly;
chunk independence and ``composites=False`` are bit for bit.
Measured on MI355X: composite_steps 1.3e-13, composite_lon 1.5e-13, composite_mean 1.7e-13 against the restatement (also with the NaN
inputs), closure on the scalars 9.1e-15, the stationary track against the fixed box's maps 3.3e-15 (each test prints its own figure)."""
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib
from lorenzcycletoolkit_amd.constants import MAP_TERMS, SCALAR_TERMS
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import composite_restatement as cr
from tests.helpers import as_f64, synthetic_domain

DEV = "cuda:0"
NT = 5
TOL = 1e-9
# (box columns, box rows, levels, layout, storage); layouts: "packed" (pack_series: fp64 a dTdt cube, fp32 tm / tp), "cube-dtdt" (the
# unpacked cube with a dT/dt array), "cube-own" (the unpacked cube with its own time neighbours)
CASES = [(5, 5, 5, "packed", np.float64), (63, 5, 5, "packed", np.float64), (64, 5, 5, "packed", np.float64),
         (65, 5, 5, "packed", np.float64), (130, 5, 5, "packed", np.float64), (5, 65, 5, "packed", np.float64),
         (5, 5, 70, "packed", np.float64), (5, 5, 5, "packed", np.float32), (65, 5, 5, "packed", np.float32),
         (130, 5, 5, "packed", np.float32), (65, 5, 5, "cube-dtdt", np.float64), (65, 5, 5, "cube-own", np.float64)]
IDS = [f"{nxb}cols-{nyb}rows-{nl}lev-{lay}-{np.dtype(d).name}" for nxb, nyb, nl, lay, d in CASES]
MARGIN_X, MARGIN_Y = 6, 4

_cache = {}


def _boxes(nxb, nyb):
    """Five boxes of one shape at five places of the (nyb + MARGIN_Y) x (nxb + MARGIN_X) grid: the south-west corner, the north-east
    corner, and three places inside."""
    at = [(0, 0), (MARGIN_X, MARGIN_Y), (3, 1), (1, 3), (4, 2)]
    return [(i, i + nxb - 1, j, j + nyb - 1) for i, j in at]


def _dom(nxb, nyb, nl, dtype=np.float64):
    key = ("dom", nxb, nyb, nl, np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = synthetic_domain(NT, nl, nyb + MARGIN_Y, nxb + MARGIN_X, seed=nxb + nyb + nl, dtype=dtype)
    return _cache[key]


def _reference(nxb, nyb, nl, dtype):
    """(boxes of the oracle, C, H, M), computed once per geometry and shared."""
    key = ("ref", nxb, nyb, nl, np.dtype(dtype).name)
    if key not in _cache:
        d = as_f64(_dom(nxb, nyb, nl, dtype))
        with np.errstate(invalid="ignore"):
            _cache[key] = (cr.step_boxes(d, _boxes(nxb, nyb)),) + cr.composites(d, _boxes(nxb, nyb))
    return _cache[key]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _run(dom, boxes, layout, **kw):
    """``compute`` of the series in the layout; returns the result."""
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    if layout == "packed":
        tc = eng.time_coefs_device(dom.time_s)
        ps = eng.pack_series(*f, boxes, tc)
        assert ("dTdt" in ps) == (dom.tair.dtype == np.float64)
        extra = {k: ps[k] for k in ("dTdt", "tm", "tp") if k in ps}
        if "tm" in ps:
            extra["tcoef"] = tc
        return eng.compute(ps["tair"], ps["u"], ps["v"], ps["omega"], ps["geopt"], eng.prepare_boxes(boxes, packed=True),
                           per_step_boxes=True, **extra, **kw)
    if layout == "cube-dtdt":
        return eng.compute(*f, boxes, per_step_boxes=True, dTdt=_dev(o.moving_dTdt(as_f64(dom))), **kw)
    return eng.compute(*f, boxes, per_step_boxes=True, time_s=dom.time_s, **kw)


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


@pytest.mark.parametrize("nxb, nyb, nl, layout, dtype", CASES, ids=IDS)
def test_composites_match_restatement_and_close(nxb, nyb, nl, layout, dtype):
    dom = _dom(nxb, nyb, nl, dtype)
    boxes = _boxes(nxb, nyb)
    assert boxes[0][0] == 0 and boxes[0][2] == 0 and boxes[1][1] == dom.lon.size - 1 and boxes[1][3] == dom.lat.size - 1
    bs, C, H, M = _reference(nxb, nyb, nl, dtype)
    res = _run(dom, boxes, layout, composites=True, composite_steps=True)
    steps, lon, mean = res.composite_steps.cpu().numpy(), res.composite_lon.cpu().numpy(), res.composite_mean.cpu().numpy()
    tag = f"{nxb}x{nyb}x{nl} {layout} {np.dtype(dtype).name}"
    assert steps.shape == (NT, 6, nyb, nxb) and lon.shape == (NT, 6, nxb) and mean.shape == (6, nyb, nxb)
    assert np.isfinite(C).all()
    _close(steps, C, (0, 2, 3), tag + " composite_steps")
    _close(lon, H, (0, 2), tag + " composite_lon")
    _close(mean, M, (1, 2), tag + " composite_mean")
    # closure on the same run's scalars, with every step's own box
    own_sc = res.scalars.cpu().numpy()[:, [SCALAR_TERMS.index(t) for t in MAP_TERMS]]
    _close(cr.box_zonal_average(lon, bs), own_sc, (0,), tag + " zonal average of composite_lon against the scalars")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_stationary_track_is_the_fixed_box_map(dtype):
    nxb, nyb, nl = 65, 5, 5
    dom = _dom(nxb, nyb, nl, dtype)
    box = (3, 3 + nxb - 1, 1, 1 + nyb - 1)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    fixed = eng.compute(*f, [box], time_s=dom.time_s, maps=True, map_steps=True)
    for layout in ("cube-own", "packed"):
        res = _run(dom, [box] * NT, layout, composites=True, composite_steps=True)
        for name, axes in (("steps", (0, 2, 3)), ("lon", (0, 2)), ("mean", (1, 2))):
            _close(getattr(res, "composite_" + name).cpu().numpy(), getattr(fixed, "map_" + name).cpu().numpy(), axes,
                   f"stationary {layout} {np.dtype(dtype).name}: composite_{name} against map_{name}")


NAN_CASES = {"interior level": dict(t=2, k=[2], row=2, cols=[7, 8]), "one point at every level": dict(t=2, k=[0, 1, 2, 3, 4], row=2, cols=[40])}


@pytest.mark.parametrize("layout", ["packed", "cube-own"])
def test_nan_patterns_are_the_restatements(layout):
    """Both NaN inputs at once, in step 2's box (box-relative row 2): T NaN at one interior level at two points -- the level of that row
    is NaN through the zonal mean and is BRIDGED --, and T NaN at every level of one point of another row -- that row's columns are NaN."""
    nxb, nyb, nl = 65, 5, 5
    base = _dom(nxb, nyb, nl)
    boxes = _boxes(nxb, nyb)
    iw, _, js, _ = boxes[2]
    T = base.tair.copy()
    T[2, 2, js + 1, [iw + 7, iw + 8]] = np.nan
    T[2, :, js + 3, iw + 40] = np.nan
    dom = o.Domain(T, base.u, base.v, base.omega, base.geopt, base.lat, base.lon, base.level, base.time_s)
    with np.errstate(invalid="ignore"):
        C, H, M, Y = cr.composites(dom, boxes, with_integrands=True)
    ae = MAP_TERMS.index("Ae")
    # the inputs do what they are meant to, in the restatement: a bridged column and a NaN column
    assert np.isnan(Y[2, ae, 2, 1]).all() and np.isfinite(C[2, ae, 1]).all(), "an interior NaN level that is bridged"
    assert np.isnan(C[2, ae, 3]).all() and np.isfinite(C[2, ae, 0]).all(), "a row of NaN columns"
    assert np.isfinite(C[[0, 4]]).all()
    res = _run(dom, boxes, layout, composites=True, composite_steps=True)
    steps = res.composite_steps.cpu().numpy()
    _close(steps, C, (0, 2, 3), f"NaN {layout}: composite_steps")
    _close(res.composite_lon.cpu().numpy(), H, (0, 2), f"NaN {layout}: composite_lon")
    _close(res.composite_mean.cpu().numpy(), M, (1, 2), f"NaN {layout}: composite_mean")
    assert np.isnan(steps[2, ae, 3]).all() and np.isfinite(steps[2, ae, 1]).all()


def test_sub_calls_and_chunks_bit_for_bit(monkeypatch):
    nxb, nyb, nl = 130, 5, 5
    dom = _dom(nxb, nyb, nl)
    boxes = _boxes(nxb, nyb)
    whole = _run(dom, boxes, "packed", composites=True)
    kept = _run(dom, boxes, "packed", composites=True, composite_steps=True)
    assert whole.composite_steps is None and not torch.isnan(whole.composite_mean).any()
    # a byte cap that holds two steps of the column values and row factors: the series is cut in 2 + 2 + 1 sub-calls
    monkeypatch.setattr(LECEngine, "MAP_CHUNK_BYTES", 2 * 8 * (6 * nyb * nxb + nl * nyb * _lib.LEC_MAPS_NCOEF))
    cut = _run(dom, boxes, "packed", composites=True)
    monkeypatch.undo()
    for name in ("composite_mean", "composite_lon"):
        assert torch.equal(getattr(cut, name), getattr(whole, name)), name
        assert torch.equal(getattr(kept, name), getattr(whole, name)), name
    # ... and composite_stage fed the series in chunks of 2 + 3 steps of the unpacked cube
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    pb = eng.prepare_boxes(boxes)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s, per_step_boxes=True)
    levraw = torch.empty((NT, nl, _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
    eng.level_stage(rows, pb, levraw)
    out = []
    for cuts in ([(0, 5)], [(0, 2), (2, 5)]):
        st = eng.composite_begin(NT, pb, DEV)
        for a, b in cuts:
            eng.composite_stage(*f[:4], rows[a:b], pb.part(a, b), levraw[a:b], st, a, time_s=dom.time_s, t_begin=a)
        out.append((st["mapsum"].clone(), st["hov"].clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert not torch.isnan(out[0][0]).any()


def test_without_composites_nothing_changes():
    dom = _dom(65, 5, 5)
    boxes = _boxes(65, 5)
    for layout in ("packed", "cube-own"):
        plain, again, with_c = _run(dom, boxes, layout), _run(dom, boxes, layout, composites=False), _run(dom, boxes, layout, composites=True)
        for f in dataclasses.fields(plain):
            a, b, c = getattr(plain, f.name), getattr(again, f.name), getattr(with_c, f.name)
            if f.name.startswith("composite_"):
                assert a is None and b is None, f.name
                continue
            assert (a is None) == (b is None) == (c is None), f.name
            if a is not None:
                assert torch.equal(a, b) and torch.equal(a, c), f.name
        assert with_c.composite_mean is not None and with_c.composite_lon is not None and with_c.composite_steps is None


def test_refused_in_words():
    nxb, nyb, nl = 5, 5, 5
    dom = _dom(nxb, nyb, nl)
    boxes = _boxes(nxb, nyb)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    kw = dict(time_s=dom.time_s, composites=True)
    two = list(boxes)
    two[3] = (1, 1 + nxb, 3, 3 + nyb - 1)                       # one column more at step 3
    with pytest.raises(ValueError, match=r"step 3 has 5 x 6 points .* step 0 has 5 x 5"):
        eng.compute(*f, two, per_step_boxes=True, **kw)
    with pytest.raises(ValueError, match="per_step_boxes=True"):
        eng.compute(*f, boxes[:1], **kw)
    with pytest.raises(ValueError, match="per_step_boxes=True"):
        eng.compute(*f, boxes, per_step_boxes=False, **kw)
    with pytest.raises(ValueError, match="at least 3 box columns"):
        eng.compute(*f, [(i, i + 1, j, jn) for i, _, j, jn in boxes], per_step_boxes=True, **kw)
    with pytest.raises(ValueError, match="composites need with_q"):
        eng.compute(*f, boxes, per_step_boxes=True, with_q=False, **kw)
    with pytest.raises(ValueError, match="one process on one GPU"):
        eng.compute(*f, boxes, per_step_boxes=True, merge_dropmask=lambda m: None, **kw)
    with pytest.raises(ValueError, match="part of composites=True"):
        eng.compute(*f, boxes, per_step_boxes=True, time_s=dom.time_s, composite_steps=True)
    with pytest.raises(ValueError, match="ONE fixed box"):          # maps keep refusing per-step boxes, as before
        eng.compute(*f, boxes, per_step_boxes=True, time_s=dom.time_s, maps=True)
    uneven = synthetic_domain(NT, nl, nyb + MARGIN_Y, nxb + MARGIN_X, seed=1, nonuniform_lon=True)
    eng2 = LECEngine(uneven.lat, uneven.lon, uneven.level, device=DEV)
    with pytest.raises(ValueError, match="evenly spaced longitudes"):
        eng2.compute(*[_dev(a) for a in (uneven.tair, uneven.u, uneven.v, uneven.omega, uneven.geopt)], boxes, per_step_boxes=True, **kw)
