"""-t / -c --composite-lon-sections on the GPU: ``lec_composite_lonsections`` through ``LECEngine.compute(..., per_step_boxes=True,
composite_lon_sections=True)`` / ``composite_lonsection_stage`` against the CPU restatement (tests/lonsections_restatement.py), against
the same run's composites and against the fixed box's ``lon_sections``.

Shapes.  tests/test_gpu_composite.py's geometry, rebuilt here: T = 5, every step's box at another place of a grid ``MARGIN`` larger than
the box, step 0 touching the domain's south-west corner, step 1 its north-east corner.  Boxes of 5, 64, 65 and 130 columns at 5 rows x 5
levels (one wave per 64 box columns), 2 rows once (both phi-neighbours missing), 65 rows once (the factors kernel's second trip, a long
march), 70 levels once.  Layouts: the box-packed series in fp64 (dT/dt as a cube: DMODE 0) and in fp32 (tm / tp: DMODE 1; the restatement
is fed the float32-rounded fields as fp64), the unpacked cube with a dT/dt cube and with its own time neighbours (DMODE 2).

Bars.  1e-9 of the term's scale for the per-step sections and the time mean against the restatement, for s_f times the vertical
trapezoid against the run's own ``composite_lon``, and for a stationary track against ``compute(lon_sections=True)`` on that fixed open
box: the project's parity bar.  Chunk independence and the flag off are bit for bit.
Measured on MI355X: composite_lonsection_steps 1.5e-13, composite_lonsection_mean 1.5e-13 against the restatement, the vertical
trapezoid against composite_lon 5.1e-16, the stationary track against the fixed box's sections 2.9e-15 (each test prints its own
figure)."""
import ctypes
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import lonsections_restatement as lr
from tests import test_lonsections_cpu as cpu
from tests.helpers import as_f64, synthetic_domain

DEV = "cuda:0"
NT = 5
TOL = 1e-9
# (box columns, box rows, levels, layout, storage)
CASES = [(5, 5, 5, "packed", np.float64), (64, 5, 5, "packed", np.float64), (65, 5, 5, "packed", np.float64),
         (130, 5, 5, "packed", np.float64), (5, 2, 5, "packed", np.float64), (5, 65, 5, "packed", np.float64),
         (5, 5, 70, "packed", np.float64), (65, 5, 5, "packed", np.float32), (65, 5, 5, "cube-dtdt", np.float64),
         (65, 5, 5, "cube-own", np.float64)]
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
    """(X [T, 6, nl, nxb], M [6, nl, nxb]), computed once per geometry and shared."""
    key = ("ref", nxb, nyb, nl, np.dtype(dtype).name)
    if key not in _cache:
        with np.errstate(invalid="ignore"):
            X = lr.composite_lon_sections(as_f64(_dom(nxb, nyb, nl, dtype)), _boxes(nxb, nyb))
        _cache[key] = (X, lr.time_mean(X))
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
def test_sections_match_restatement_and_close(nxb, nyb, nl, layout, dtype):
    dom = _dom(nxb, nyb, nl, dtype)
    boxes = _boxes(nxb, nyb)
    assert boxes[0][0] == 0 and boxes[0][2] == 0 and boxes[1][1] == dom.lon.size - 1 and boxes[1][3] == dom.lat.size - 1
    X, M = _reference(nxb, nyb, nl, dtype)
    res = _run(dom, boxes, layout, composite_lon_sections=True, composite_lon_section_steps=True, composites=True)
    steps, mean = res.composite_lonsection_steps.cpu().numpy(), res.composite_lonsection_mean.cpu().numpy()
    tag = f"{nxb}x{nyb}x{nl} {layout} {np.dtype(dtype).name}"
    assert steps.shape == (NT, 6, nl, nxb) and mean.shape == (6, nl, nxb)
    assert np.isfinite(X).all()
    _close(steps, X, (0, 2, 3), tag + " composite_lonsection_steps")
    _close(mean, M, (1, 2), tag + " composite_lonsection_mean")
    # closure on the same run's composites: s_f times the vertical trapezoid is the Hovmoeller row
    _close(lr.columns(steps, dom.level), res.composite_lon.cpu().numpy(), (0, 2), tag + " vertical trapezoid against composite_lon")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_stationary_track_is_the_fixed_box_section(dtype):
    nxb, nyb, nl = 65, 5, 5
    dom = _dom(nxb, nyb, nl, dtype)
    box = (3, 3 + nxb - 1, 1, 1 + nyb - 1)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    fixed = eng.compute(*f, [box], time_s=dom.time_s, lon_sections=True, lon_section_steps=True)
    for layout in ("cube-own", "packed"):
        res = _run(dom, [box] * NT, layout, composite_lon_sections=True, composite_lon_section_steps=True)
        for name, axes in (("steps", (0, 2, 3)), ("mean", (1, 2))):
            _close(getattr(res, "composite_lonsection_" + name).cpu().numpy(), getattr(fixed, "lonsection_" + name).cpu().numpy(), axes,
                   f"stationary {layout} {np.dtype(dtype).name}: composite_lonsection_{name} against lonsection_{name}")


def test_sub_calls_and_chunks_bit_for_bit(monkeypatch):
    nxb, nyb, nl = 130, 5, 5
    dom = _dom(nxb, nyb, nl)
    boxes = _boxes(nxb, nyb)
    kw = dict(composite_lon_sections=True)
    whole = _run(dom, boxes, "packed", **kw)
    kept = _run(dom, boxes, "packed", composite_lon_section_steps=True, **kw)
    assert whole.composite_lonsection_steps is None and not torch.isnan(whole.composite_lonsection_mean).any()
    # a byte cap that holds two steps of the sections and row factors: the series is cut in 2 + 2 + 1 sub-calls
    monkeypatch.setattr(LECEngine, "MAP_CHUNK_BYTES", 2 * 8 * (6 * nl * nxb + nl * nyb * _lib.LEC_MAPS_NCOEF))
    cut = _run(dom, boxes, "packed", **kw)
    monkeypatch.undo()
    assert torch.equal(cut.composite_lonsection_mean, whole.composite_lonsection_mean)
    assert torch.equal(kept.composite_lonsection_mean, whole.composite_lonsection_mean)
    # ... and composite_lonsection_stage fed the series in chunks of 1, 2 and 2 + 3 steps of the unpacked cube
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    pb = eng.prepare_boxes(boxes)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s, per_step_boxes=True)
    levraw = torch.empty((NT, nl, _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
    eng.level_stage(rows, pb, levraw)
    out = []
    for cuts in ([(0, 5)], [(0, 2), (2, 5)], [(0, 2), (2, 4), (4, 5)], [(t, t + 1) for t in range(NT)]):
        st = eng.composite_lonsection_begin(NT, pb, DEV)
        for a, b in cuts:
            eng.composite_lonsection_stage(*f[:4], rows[a:b], pb.part(a, b), levraw[a:b], st, a, time_s=dom.time_s, t_begin=a)
        out.append(st["lonsecsum"].clone())
    assert all(torch.equal(x, out[0]) for x in out[1:]) and not torch.isnan(out[0]).any()


def test_flag_off_keeps_every_bit():
    dom = _dom(65, 5, 5)
    boxes = _boxes(65, 5)
    for layout in ("packed", "cube-own"):
        base = dict(composites=True, composite_sections=True)
        plain, again = _run(dom, boxes, layout, **base), _run(dom, boxes, layout, composite_lon_sections=False, **base)
        with_c = _run(dom, boxes, layout, composite_lon_sections=True, **base)
        for f in dataclasses.fields(plain):
            a, b, c = getattr(plain, f.name), getattr(again, f.name), getattr(with_c, f.name)
            if f.name.startswith("composite_lonsection_"):
                assert a is None and b is None, f.name
                continue
            assert (a is None) == (b is None) == (c is None), f.name
            if a is not None:
                assert torch.equal(a, b) and torch.equal(a, c), f.name
        assert with_c.composite_lonsection_mean is not None and with_c.composite_lonsection_steps is None


def test_engine_refusals_in_words():
    nxb, nyb, nl = 5, 5, 5
    dom = _dom(nxb, nyb, nl)
    boxes = _boxes(nxb, nyb)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    kw = dict(time_s=dom.time_s, composite_lon_sections=True)
    two = list(boxes)
    two[3] = (1, 1 + nxb, 3, 3 + nyb - 1)                       # one column more at step 3
    with pytest.raises(ValueError, match=r"composite longitude-pressure sections need boxes of ONE shape.*step 3 has 5 x 6 points .* step 0 has 5 x 5"):
        eng.compute(*f, two, per_step_boxes=True, **kw)
    with pytest.raises(ValueError, match="per_step_boxes=True"):
        eng.compute(*f, boxes[:1], **kw)
    with pytest.raises(ValueError, match="a step table"):
        eng.compute(*f, boxes, per_step_boxes=True, steps=torch.zeros((NT, 3), dtype=torch.int32, device=DEV), **kw)
    uneven = synthetic_domain(NT, nl, nyb + MARGIN_Y, nxb + MARGIN_X, seed=1, nonuniform_lon=True)
    eng2 = LECEngine(uneven.lat, uneven.lon, uneven.level, device=DEV)
    with pytest.raises(ValueError, match="composite longitude-pressure sections need evenly spaced longitudes"):
        eng2.compute(*[_dev(a) for a in (uneven.tair, uneven.u, uneven.v, uneven.omega, uneven.geopt)], boxes, per_step_boxes=True, **kw)


# -- the C call's refusals on real arguments: nothing is launched ---------------------------------------------------------------------
SENTINEL = -12345.0


def _real_args():
    """A valid ``lec_composite_lonsections`` call with the scalars and boxes of ``test_lonsections_cpu.moving_args`` on real device
    arrays (the unpacked cube, dT/dt from its own neighbours); returns (args, the two outputs prefilled with SENTINEL, what must live)."""
    proto, box = cpu.moving_args()
    dom = synthetic_domain(proto.nt, proto.nl, proto.ny, proto.nx, seed=3)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    a, b = proto.t_begin, proto.t_begin + proto.t_count
    series = [tuple(int(x) for x in box[0])] * a + [tuple(int(x) for x in q) for q in box] + [tuple(int(x) for x in box[-1])] * (proto.nt - b)
    pb = eng.prepare_boxes(series)
    f = [_dev(x) for x in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    rows = eng.rowstats(*f, pb, time_s=dom.time_s, per_step_boxes=True)
    levraw = torch.empty((proto.nt, proto.nl, _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
    eng.level_stage(rows, pb, levraw)
    part = pb.part(a, b)
    f64 = dict(dtype=torch.float64, device=DEV)
    keep = dict(f=f, rows=rows[a:b].contiguous(), levraw=levraw[a:b].contiguous(), tcoef=eng.time_coefs_device(dom.time_s), eng=eng, pb=pb,
                part=part, box=box, coef=torch.empty((proto.t_count, proto.nl, proto.nyb, _lib.LEC_MAPS_NCOEF), **f64))
    sec = torch.full((proto.t_count, 6, proto.nl, proto.nxb), SENTINEL, **f64)
    tot = torch.full((6, proto.nl, proto.nxb), SENTINEL, **f64)
    for name, t in (("tair_d", f[0]), ("u_d", f[1]), ("v_d", f[2]), ("omega_d", f[3]), ("rows_d", keep["rows"]), ("levraw_d", keep["levraw"]),
                    ("box_d", part.dev["box"]), ("boxtab_d", part.dev["boxtab"]), ("lattab_d", part.dev["lattab"]),
                    ("lattab2_d", part.dev["lattab2"]), ("levtab_d", eng._levtab), ("levtab2_d", eng._levtab2), ("tcoef_d", keep["tcoef"]),
                    ("coef_d", keep["coef"]), ("lonsec_d", sec), ("lonsecsum_d", tot)):
        setattr(proto, name, t.data_ptr())
    proto.stream = torch.cuda.current_stream(DEV).cuda_stream
    return proto, sec, tot, keep


def test_c_call_refusals_launch_nothing():
    lib = _lib.load()
    a, sec, tot, keep = _real_args()
    assert int(keep["part"].bt.nyb_max) == a.nyb
    cases = [(f, c, None) for f, c in cpu.MOVING_ARG] + [(w, None, bx) for w, bx in cpu.MOVING_BOXES]
    for field, change, boxes in cases:
        b = _lib.CompositeLonSectionsArgs.from_buffer_copy(a)
        if change is not None:
            change(b)
        else:
            bad = np.ascontiguousarray(boxes, dtype=np.int32)
            b.box_h = bad.ctypes.data
        with torch.cuda.device(DEV):
            assert lib.lec_composite_lonsections(ctypes.byref(b)) == 1, field
        msg = lib.lec_last_error()
        assert msg.startswith(b"lec_composite_lonsections:") and field.encode() in msg, (field, msg)
        torch.cuda.synchronize()
        assert bool((sec == SENTINEL).all()) and bool((tot == SENTINEL).all()), field
    # ... and the arguments are otherwise valid: unchanged, the call runs
    tot.zero_()
    with torch.cuda.device(DEV):
        assert lib.lec_composite_lonsections(ctypes.byref(a)) == 0, lib.lec_last_error()
    torch.cuda.synchronize()
    assert not bool((sec == SENTINEL).any()) and bool(torch.isfinite(sec).all())
    s = sec[0].clone()
    for t in range(1, sec.shape[0]):
        s = s + sec[t]
    assert torch.equal(tot, s)
