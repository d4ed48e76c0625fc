"""-t / -c --composite-sections on the GPU: ``lec_composite_sections`` through ``LECEngine.compute(..., per_step_boxes=True,
composite_sections=True)`` / ``composite_section_stage`` against the CPU restatement (tests/composite_sections_restatement.py) and
against the same run's per-level tables and scalars.

Shapes.  T = 5, the boxes of tests/test_gpu_composite.py: one shape at five places of a grid a few points larger, step 0 in the
south-west corner, step 1 in the north-east corner.  The seams of the kernels lie along the rows (the rows kernel walks them in trips of
64; the fold has 64-thread blocks over (term, row)) and along the levels (the fold loads them in batches of 8): boxes of 5, 63, 64, 65 and
130 rows with 5 columns on 5 levels, 8, 9 and 70 levels once each with 5 rows, and 65 columns once (the width does not matter: only row
records are read); the time sums load eight steps ahead: series of 8, 9 and 17 steps once each.  Layouts: the box-packed series in fp64 (dT/dt as a cube) and in fp32 (tm / tp; the restatement is fed the
float32-rounded fields as fp64), the unpacked cube with a dT/dt cube once and with its own time neighbours once.

Bars.  1e-9 of the term's scale (its largest |value| in the case) for the per-step sections, the columns and the time mean against the
restatement, for sum_j cw_j(t) X_f against the run's own ``levels`` and sum_j cw_j(t) C_f against its ``scalars`` with every step's own
box, and for a stationary track against ``compute(sections=True)`` on that fixed box: the project's parity bar
(tests/test_gpu_sections.py, tests/test_gpu_composite.py).  NaN patterns are the restatement's exactly; chunk independence and
``composite_sections=False`` are bit for bit.
Measured on MI355X (each test prints its own figure): against the restatement composite_section_steps 1.4e-13, composite_section_lat
1.3e-13, composite_section_mean 1.5e-13 over the thirteen cases (the 70-level case the largest), 1.3e-13 with boxes of three widths,
6.4e-14 with the NaN inputs, 9.2e-14 for the series of 8, 9 and 17 steps, 7.4e-14 through a step table; closure on the run's own levels 4.0e-16 and scalars 5.0e-16;
the stationary track against the fixed box's sections 3.2e-14 (fp64) and 1.8e-14 (fp32 storage), packed and unpacked alike."""
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib
from lorenzcycletoolkit_amd.constants import LEVEL_TERMS, SCALAR_TERMS, SECTION_TERMS
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import composite_sections_restatement as csr
from tests.helpers import as_f64, synthetic_domain

DEV = "cuda:0"
NT = 5
TOL = 1e-9
# (box columns, box rows, levels, layout, storage); layouts: "packed" (pack_series: fp64 a dTdt cube, fp32 tm / tp), "cube-dtdt" (the
# unpacked cube with a dT/dt array), "cube-own" (the unpacked cube with its own time neighbours)
CASES = [(5, 5, 5, "packed", np.float64), (5, 63, 5, "packed", np.float64), (5, 64, 5, "packed", np.float64),
         (5, 65, 5, "packed", np.float64), (5, 130, 5, "packed", np.float64), (5, 5, 8, "packed", np.float64),
         (5, 5, 9, "packed", np.float64), (5, 5, 70, "packed", np.float64), (65, 5, 5, "packed", np.float64),
         (5, 5, 5, "packed", np.float32), (5, 65, 5, "packed", np.float32), (5, 65, 5, "cube-dtdt", np.float64),
         (5, 65, 5, "cube-own", np.float64)]
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
    """(X, C, M, cw) of the restatement, computed once per geometry and shared."""
    key = ("ref", nxb, nyb, nl, np.dtype(dtype).name)
    if key not in _cache:
        with np.errstate(invalid="ignore"):
            _cache[key] = csr.composite_sections(as_f64(_dom(nxb, nyb, nl, dtype)), _boxes(nxb, nyb))
    return _cache[key]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _run(dom, boxes, layout, **kw):
    """``compute`` of the series in the layout; returns (the result, the engine's tables of the boxes)."""
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    if layout == "packed":
        tc = eng.time_coefs_device(dom.time_s)
        ps = eng.pack_series(*f, boxes, tc)
        assert ("dTdt" in ps) == (dom.tair.dtype == np.float64)
        extra = {k: ps[k] for k in ("dTdt", "tm", "tp") if k in ps}
        if "tm" in ps:
            extra["tcoef"] = tc
        pb = eng.prepare_boxes(boxes, packed=True)
        return eng.compute(ps["tair"], ps["u"], ps["v"], ps["omega"], ps["geopt"], pb, per_step_boxes=True, **extra, **kw), pb.bt
    pb = eng.prepare_boxes(boxes)
    if layout == "cube-dtdt":
        return eng.compute(*f, pb, per_step_boxes=True, dTdt=_dev(o.moving_dTdt(as_f64(dom))), **kw), pb.bt
    return eng.compute(*f, pb, per_step_boxes=True, time_s=dom.time_s, **kw), pb.bt


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


def _fields_of(res):
    return res.composite_section_steps.cpu().numpy(), res.composite_section_lat.cpu().numpy(), res.composite_section_mean.cpu().numpy()


@pytest.mark.parametrize("nxb, nyb, nl, layout, dtype", CASES, ids=IDS)
def test_sections_match_restatement_and_close(nxb, nyb, nl, layout, dtype):
    dom = _dom(nxb, nyb, nl, dtype)
    boxes = _boxes(nxb, nyb)
    assert boxes[0][0] == 0 and boxes[0][2] == 0 and boxes[1][1] == dom.lon.size - 1 and boxes[1][3] == dom.lat.size - 1
    X, C, M, _ = _reference(nxb, nyb, nl, dtype)
    res, bt = _run(dom, boxes, layout, composite_sections=True, composite_section_steps=True)
    steps, lat, mean = _fields_of(res)
    tag = f"{nxb}x{nyb}x{nl} {layout} {np.dtype(dtype).name}"
    assert steps.shape == (NT, 10, nl, nyb) and lat.shape == (NT, 10, nyb) and mean.shape == (10, nl, nyb)
    assert np.isfinite(X).all()
    _close(steps, X, (0, 2, 3), tag + " composite_section_steps")
    _close(lat, C, (0, 2), tag + " composite_section_lat")
    _close(mean, M, (1, 2), tag + " composite_section_mean")
    # closure on the same run's per-level tables and scalars, with the row weights of every step's own box (the level stage's)
    cw = np.asarray(bt.lattab2)[:, :nyb, 0]                                                     # [T, nyb]
    levels, scalars = res.levels.cpu().numpy(), res.scalars.cpu().numpy()
    own_lv = np.stack([levels[:, LEVEL_TERMS.index(t)] for t in SECTION_TERMS], axis=1)        # [T, 10, nl]
    own_sc = np.stack([scalars[:, SCALAR_TERMS.index(t)] for t in SECTION_TERMS], axis=1)       # [T, 10]
    _close((steps * cw[:, None, None, :]).sum(axis=-1), own_lv, (0, 2), tag + " closure on levels")
    _close((lat * cw[:, None, :]).sum(axis=-1), own_sc, (0,), tag + " closure on scalars")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_stationary_track_is_the_fixed_box_section(dtype):
    nxb, nyb, nl = 5, 65, 5
    dom = _dom(nxb, nyb, nl, dtype)
    box = (3, 3 + nxb - 1, 1, 1 + nyb - 1)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    fixed = eng.compute(*f, [box], time_s=dom.time_s, sections=True, section_steps=True)
    for layout in ("cube-own", "packed"):
        res, _ = _run(dom, [box] * NT, layout, composite_sections=True, composite_section_steps=True)
        for name, axes in (("steps", (0, 2, 3)), ("lat", (0, 2)), ("mean", (1, 2))):
            _close(getattr(res, "composite_section_" + name).cpu().numpy(), getattr(fixed, "section_" + name).cpu().numpy(), axes,
                   f"stationary {layout} {np.dtype(dtype).name}: composite_section_{name} against section_{name}")


@pytest.mark.parametrize("layout", ["packed", "cube-own"])
def test_boxes_of_two_widths_are_accepted(layout):
    """One row count, two widths: only the row count must be common (a row record holds the zonal means over its own box's width)."""
    nxb, nyb, nl = 9, 5, 5
    dom = _dom(nxb, nyb, nl)
    boxes = _boxes(nxb, nyb)
    boxes[1] = (boxes[1][0] + 4, boxes[1][1], boxes[1][2], boxes[1][3])        # 5 columns at step 1 ...
    boxes[3] = (boxes[3][0], boxes[3][1] - 2, boxes[3][2], boxes[3][3])        # ... and 7 at step 3
    assert sorted({b[1] - b[0] + 1 for b in boxes}) == [5, 7, 9] and {b[3] - b[2] + 1 for b in boxes} == {nyb}
    X, C, M, _ = csr.composite_sections(dom, boxes)
    res, _ = _run(dom, boxes, layout, composite_sections=True, composite_section_steps=True)
    steps, lat, mean = _fields_of(res)
    _close(steps, X, (0, 2, 3), f"widths {layout}: composite_section_steps")
    _close(lat, C, (0, 2), f"widths {layout}: composite_section_lat")
    _close(mean, M, (1, 2), f"widths {layout}: composite_section_mean")


@pytest.mark.parametrize("layout", ["packed", "cube-own"])
def test_nan_patterns_are_the_restatements(layout):
    """Both NaN inputs at once, in step 2's box: T NaN at one interior level at two points of box-relative row 1 -- that level of that row
    is NaN through the zonal mean and is BRIDGED in the column --, and T NaN at every level of one point of row 3 -- that row's column is
    NaN, and the time mean is NaN there and nowhere else."""
    nxb, nyb, nl = 65, 5, 5
    base = _dom(nxb, nyb, nl)
    boxes = _boxes(nxb, nyb)
    iw, _, js, _ = boxes[2]
    T = base.tair.copy()
    T[2, 2, js + 1, [iw + 7, iw + 8]] = np.nan
    T[2, :, js + 3, iw + 40] = np.nan
    dom = o.Domain(T, base.u, base.v, base.omega, base.geopt, base.lat, base.lon, base.level, base.time_s)
    with np.errstate(invalid="ignore"):
        X, C, M, _ = csr.composite_sections(dom, boxes)
    ae = SECTION_TERMS.index("Ae")
    # the inputs do what they are meant to, in the restatement: a bridged level and a NaN column
    assert np.isnan(X[2, ae, 2, 1]) and np.isfinite(X[2, ae, [0, 1, 3, 4], 1]).all() and np.isfinite(C[2, ae, 1]), "an interior NaN level, bridged"
    assert np.isnan(X[2, ae, :, 3]).all() and np.isnan(C[2, ae, 3]) and np.isfinite(C[2, ae, [0, 4]]).all(), "a NaN column"
    assert np.isfinite(X[[0, 4]]).all() and np.isfinite(C[[0, 4]]).all()
    res, _ = _run(dom, boxes, layout, composite_sections=True, composite_section_steps=True)
    steps, lat, mean = _fields_of(res)
    _close(steps, X, (0, 2, 3), f"NaN {layout}: composite_section_steps")
    _close(lat, C, (0, 2), f"NaN {layout}: composite_section_lat")
    _close(mean, M, (1, 2), f"NaN {layout}: composite_section_mean")
    assert np.isnan(lat[2, ae, 3]) and np.isfinite(lat[2, ae, 1]) and np.isnan(steps[2, ae, 2, 1])
    assert np.isnan(mean[ae, :, 3]).all() and np.isnan(mean[ae, 2, 1]) and np.isfinite(mean[ae, [0, 1, 3, 4], 1]).all()
    assert np.isfinite(mean[ae][:, [0, 2, 4]]).all()


def test_chunks_bit_for_bit():
    """``composite_section_stage`` over the steps [0:5] against [0:2] + [2:5] and five calls of one step each, packed and not."""
    nxb, nyb, nl = 5, 65, 9
    dom = _dom(nxb, nyb, nl)
    boxes = _boxes(nxb, nyb)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    rows = eng.rowstats(*f, eng.prepare_boxes(boxes), time_s=dom.time_s, per_step_boxes=True)
    for packed in (False, True):
        pb = eng.prepare_boxes(boxes, packed=packed)
        levraw = torch.empty((NT, nl, _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
        eng.level_stage(rows, pb, levraw)
        out, kept = [], []
        for cuts in ([(0, 5)], [(0, 2), (2, 5)], [(t, t + 1) for t in range(NT)]):
            for keep in (False, True):
                st = eng.composite_section_begin(NT, pb, DEV, keep_steps=keep)
                for a, b in cuts:
                    eng.composite_section_stage(rows[a:b], pb.part(a, b), levraw[a:b], st, a)
                out.append((st["secsum"].clone(), st["col"].clone()))
                if keep:
                    kept.append(st["steps"].clone())
        for s, c in out[1:]:
            assert torch.equal(s, out[0][0]) and torch.equal(c, out[0][1])
        for k in kept[1:]:
            assert torch.equal(k, kept[0])
        assert not torch.isnan(out[0][0]).any() and not torch.isnan(out[0][1]).any() and not torch.isnan(kept[0]).any()
    res, _ = _run(dom, boxes, "cube-own", composite_sections=True)
    assert res.composite_section_steps is None
    assert torch.equal(res.composite_section_lat, out[0][1])
    assert torch.equal(res.composite_section_mean, (out[0][0] / float(NT)).permute(1, 0, 2).contiguous())


def test_a_step_table_is_served():
    """``steps=`` (the batch's table: one box per processed step) costs the call nothing -- it reads the row records and the boxes' tables
    only --, so it is allowed: the identity table of one track against the restatement."""
    from lorenzcycletoolkit_amd import tables
    nxb, nyb, nl = 5, 65, 5
    dom = _dom(nxb, nyb, nl)
    boxes = _boxes(nxb, nyb)
    X, C, M, _ = _reference(nxb, nyb, nl, np.float64)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    u = np.arange(NT)
    st = _dev(np.stack([u, np.maximum(u - 1, 0), np.minimum(u + 1, NT - 1)], 1).astype(np.int32))
    res = eng.compute(*f, eng.prepare_boxes(boxes), steps=st, tcoef=_dev(tables.time_coefs(dom.time_s)), per_step_boxes=True,
                      drop_any_time=False, composite_sections=True, composite_section_steps=True)
    steps, lat, mean = _fields_of(res)
    _close(steps, X, (0, 2, 3), "step table: composite_section_steps")
    _close(lat, C, (0, 2), "step table: composite_section_lat")
    _close(mean, M, (1, 2), "step table: composite_section_mean")


@pytest.mark.parametrize("nt", [8, 9, 17])
def test_time_sums_across_their_batches_of_eight_steps(nt):
    """The time sums load eight steps ahead: series of 8, 9 and 17 steps against the restatement, and cut at and beside the batch's end
    bit for bit."""
    nxb, nyb, nl = 5, 5, 5
    dom = synthetic_domain(nt, nl, nyb + MARGIN_Y, nxb + MARGIN_X, seed=nt)
    boxes = [_boxes(nxb, nyb)[t % NT] for t in range(nt)]
    X, C, M, _ = csr.composite_sections(dom, boxes)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    pb = eng.prepare_boxes(boxes)
    res = eng.compute(*f, pb, per_step_boxes=True, time_s=dom.time_s, composite_sections=True, composite_section_steps=True)
    steps, lat, mean = _fields_of(res)
    _close(steps, X, (0, 2, 3), f"{nt} steps: composite_section_steps")
    _close(lat, C, (0, 2), f"{nt} steps: composite_section_lat")
    _close(mean, M, (1, 2), f"{nt} steps: composite_section_mean")
    rows = eng.rowstats(*f, pb, time_s=dom.time_s, per_step_boxes=True)
    levraw = torch.empty((nt, nl, _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
    eng.level_stage(rows, pb, levraw)
    for cut in sorted(c for c in {1, 7, 8, nt - 1} if 0 < c < nt):
        st = eng.composite_section_begin(nt, pb, DEV)
        for a, b in ((0, cut), (cut, nt)):
            eng.composite_section_stage(rows[a:b], pb.part(a, b), levraw[a:b], st, a)
        assert torch.equal((st["secsum"] / float(nt)).permute(1, 0, 2).contiguous(), res.composite_section_mean), cut
        assert torch.equal(st["col"], res.composite_section_lat), cut


def test_without_the_keyword_nothing_changes():
    dom = _dom(5, 65, 5)
    boxes = _boxes(5, 65)
    for layout in ("packed", "cube-own"):
        plain, again, with_c = (_run(dom, boxes, layout)[0], _run(dom, boxes, layout, composite_sections=False)[0],
                                _run(dom, boxes, layout, composite_sections=True)[0])
        for f in dataclasses.fields(plain):
            a, b, c = getattr(plain, f.name), getattr(again, f.name), getattr(with_c, f.name)
            if f.name.startswith("composite_section_"):
                assert a is None and b is None, f.name
                continue
            assert (a is None) == (b is None) == (c is None), f.name
            if a is not None:
                assert torch.equal(a, b) and torch.equal(a, c), f.name
        assert with_c.composite_section_mean is not None and with_c.composite_section_lat is not None
        assert with_c.composite_section_steps is None


def test_refused_in_words():
    nxb, nyb, nl = 5, 5, 5
    dom = _dom(nxb, nyb, nl)
    boxes = _boxes(nxb, nyb)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    kw = dict(time_s=dom.time_s, composite_sections=True)
    two = list(boxes)
    two[3] = (1, 1 + nxb - 1, 3, 3 + nyb)                       # one row more at step 3
    with pytest.raises(ValueError, match="ONE row count: the box of step 3 has 6 rows, that of step 0 has 5"):
        eng.compute(*f, two, per_step_boxes=True, **kw)
    with pytest.raises(ValueError, match="per_step_boxes=True"):
        eng.compute(*f, boxes[:1], **kw)
    with pytest.raises(ValueError, match="per_step_boxes=True"):
        eng.compute(*f, boxes, per_step_boxes=False, **kw)
    with pytest.raises(ValueError, match="one process on one GPU"):
        eng.compute(*f, boxes, per_step_boxes=True, merge_dropmask=lambda m: None, **kw)
    with pytest.raises(ValueError, match="one process on one GPU"):
        eng.compute(*f, boxes, per_step_boxes=True, out=torch.empty((NT, LECEngine.packed_width(nl)), dtype=torch.float64, device=DEV), **kw)
    with pytest.raises(ValueError, match="part of composite_sections=True"):
        eng.compute(*f, boxes, per_step_boxes=True, time_s=dom.time_s, composite_section_steps=True)
    with pytest.raises(ValueError, match="sections exist for ONE fixed box"):          # sections keep refusing per-step boxes, as before
        eng.compute(*f, boxes, per_step_boxes=True, time_s=dom.time_s, sections=True)
    # the stage's own refusals: plain boxes, a chunk that does not fit, another row count than the series'
    pb = eng.prepare_boxes(boxes)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s, per_step_boxes=True)
    levraw = torch.empty((NT, nl, _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
    eng.level_stage(rows, pb, levraw)
    st = eng.composite_section_begin(NT, pb, DEV)
    with pytest.raises(ValueError, match="boxes from prepare_boxes"):
        eng.composite_section_stage(rows, boxes, levraw, st, 0)
    with pytest.raises(ValueError, match="does not fit the series"):
        eng.composite_section_stage(rows, pb, levraw, st, 1)
    with pytest.raises(ValueError, match="one box per step"):
        eng.composite_section_stage(rows, pb.part(0, 1), levraw, st, 0)
    # the library's own refusal, should a caller pass it boxes the engine has not seen: nothing was launched
    import ctypes
    host = np.ascontiguousarray([(0, 4, 0, 4)] * 4 + [(0, 4, 0, 5)], dtype=np.int32)
    work = torch.empty((NT, nl, 10, nyb), dtype=torch.float64, device=DEV)
    a = _lib.CompositeSectionsArgs(rows_d=rows.data_ptr(), levraw_d=levraw.data_ptr(), t_count=NT, nl=nl, nyb=nyb, reserved0=0,
                                   box_h=host.ctypes.data, box_d=pb.dev["box"].data_ptr(), lattab2_d=pb.dev["lattab2"].data_ptr(),
                                   levtab2_d=eng._levtab2.data_ptr(), sec_d=work.data_ptr(), col_d=st["col"].data_ptr(),
                                   secsum_d=st["secsum"].data_ptr(), stream=None)
    with pytest.raises(ValueError, match="lec_composite_sections: box_h: the box of step 4 has 6 rows, the call's nyb is 5"):
        _lib.check(eng.lib.lec_composite_sections(ctypes.byref(a)), "lec_composite_sections")
