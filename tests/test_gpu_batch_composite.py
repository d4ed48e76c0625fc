"""Composites of a batch of tracks on the GPU: ``lec_composite_steps`` / ``lec_composite_ensemble`` through
``LECEngine.compute(..., steps=, per_step_boxes=True, batch_composites=sizes)`` against every track's OWN run
(``compute(per_step_boxes=True, composites=True)`` on the cube of the track's steps: bit for bit) and against the CPU restatement
(tests/batch_composite_restatement.py).

Shapes.  A union of 9 steps; three tracks of one box shape: A on every union step, B on every second one (its time neighbours are not
adjacent in the cube), C on two steps that A has too.  The boxes drift by a point or two per step.  5 x 65 boxes (rows x columns) on a
24 x 80 grid cross the column kernel's 64-lane segment; there the tracks lie in three bands of rows, so a NaN laid into B's band is seen
by B alone.  64 x 3 and 65 x 5 boxes cross the factor kernel's trips of 64 rows and take the columns to their minimum.  8, 9 and once 70
levels; fp64 and fp32 cubes.  Tracks of 16 and 17 steps on an 18-step union stand on both sides of the time sum's load batch of 16.

Bars.  Bit for bit against the own runs, between batches of different company, between cuts into sub-calls and for the ensemble against
the in-order NumPy sum of the API's own means.  1e-9 of the term's scale against the restatement, tests/test_gpu_composite.py's bar; NaN
patterns are the restatement's exactly.  Each test prints its figures.
Measured on MI355X, the largest over all cases: batch_composite_steps 3.9e-13, batch_composite_lon 5.1e-13, batch_composite_mean 2.9e-13,
batch_composite_ensemble 2.2e-13 against the restatement; everything else is equality."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib, tables
from lorenzcycletoolkit_amd.constants import MAP_TERMS
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import batch_composite_restatement as br
from tests.helpers import as_f64, synthetic_domain

DEV = "cuda:0"
TOL = 1e-9
NT = 9
# (box rows, box columns, levels, storage, grid rows, grid columns)
CASES = [(5, 65, 8, np.float64, 24, 80), (5, 65, 9, np.float32, 24, 80), (64, 3, 8, np.float64, 70, 12), (65, 5, 9, np.float64, 71, 14),
         (5, 65, 70, np.float64, 24, 80), (65, 5, 8, np.float32, 71, 14)]
IDS = [f"{nyb}x{nxb}-{nl}lev-{np.dtype(d).name}" for nyb, nxb, nl, d, _, _ in CASES]

_cache = {}


def _tracks(nyb, nxb, ny, nx, nt=NT):
    """[(union steps, boxes)]: A on every step, B on every second, C on steps 3 and 4.  Track k drifts inside its band of rows (a third
    of the grid's rows where three bands of nyb + 2 rows fit, else the whole grid) and over the grid's columns."""
    banded = 3 * (nyb + 2) <= ny
    out = []
    for k, u in enumerate((np.arange(nt), np.arange(0, nt, 2), np.array([3, 4]))):
        j0 = k * (ny // 3) if banded else 0
        jroom = (ny // 3 if banded else ny) - nyb
        iroom = nx - nxb
        boxes = []
        for n, t in enumerate(u):
            j, i = j0 + (n + 2 * k) % (jroom + 1), (3 * n + 5 * k) % (iroom + 1)
            boxes.append((i, i + nxb - 1, j, j + nyb - 1))
        out.append((u, boxes))
    return out


def _dom(nl, ny, nx, dtype, nt=NT):
    key = ("dom", nt, nl, ny, nx, np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = synthetic_domain(nt, nl, ny, nx, seed=nl + ny + nx, dtype=dtype, dt_s=10800.0)
    return _cache[key]


def _reference(key, dom, tracks):
    """The restatement of the case, computed once and shared."""
    if key not in _cache:
        _cache[key] = br.composites(as_f64(dom), tracks)
    return _cache[key]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _table(dom, tracks):
    """(steps int32 [S, 3], tcoef [S, 3], boxes, sizes) of the tracks, as frameworks.lec_moving_batch forms them."""
    steps, tcoef, boxes = [], [], []
    for u, bx in tracks:
        n = len(u)
        steps.append(np.stack([u, u[np.maximum(np.arange(n) - 1, 0)], u[np.minimum(np.arange(n) + 1, n - 1)]], 1))
        tcoef.append(tables.time_coefs(dom.time_s[u] - dom.time_s[u[0]]))
        boxes += bx
    return np.concatenate(steps).astype(np.int32), np.concatenate(tcoef), boxes, [len(u) for u, _ in tracks]


def _batch(eng, cubes, dom, tracks, **kw):
    st, tc, boxes, sizes = _table(dom, tracks)
    kw.setdefault("batch_composites", sizes)
    if kw["batch_composites"] is None:
        del kw["batch_composites"]
    return eng.compute(*cubes, eng.prepare_boxes(boxes), steps=_dev(st), tcoef=_dev(tc), per_step_boxes=True, drop_any_time=False, **kw)


def _own(eng, cubes, dom, u, boxes):
    """The track alone: the cube of its own steps, its own time axis, one box per step."""
    sub = [c[torch.as_tensor(u, device=DEV)].contiguous() for c in cubes]
    return eng.compute(*sub, boxes, per_step_boxes=True, drop_any_time=False, time_s=dom.time_s[u] - dom.time_s[u[0]], composites=True,
                       composite_steps=True)


def _bits(a, b):
    """Equal bit for bit, NaN at the same places (payloads aside)."""
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)) and torch.equal(a.isnan(), b.isnan())


def _scale(ref, axes):
    a = np.where(np.isnan(ref), -np.inf, np.abs(ref)).max(axis=axes, keepdims=True)
    return np.where(np.isfinite(a), a, 1.0)


def _close(got, ref, axes, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern"
    err = np.nanmax(np.abs(got - ref) / _scale(ref, axes)) if np.isfinite(ref).any() else 0.0
    print(f"{what}: max error / scale = {err:.3e}")
    assert err <= TOL, (what, err)
    return err


def _ensemble_in_order(mean: np.ndarray) -> np.ndarray:
    s = mean[0].copy()
    for k in range(1, mean.shape[0]):
        s = s + mean[k]
    return s / float(mean.shape[0])


def _check_against_own_and_restatement(eng, cubes, dom, tracks, res, ref, tag):
    per, ens = ref
    mean, lon, steps = res.batch_composite_mean, res.batch_composite_lon, res.batch_composite_steps
    nyb, nxb = tracks[0][1][0][3] - tracks[0][1][0][2] + 1, tracks[0][1][0][1] - tracks[0][1][0][0] + 1
    S = sum(len(u) for u, _ in tracks)
    assert mean.shape == (len(tracks), 6, nyb, nxb) and lon.shape == (S, 6, nxb) and steps.shape == (S, 6, nyb, nxb)
    a = 0
    for k, (u, boxes) in enumerate(tracks):
        b = a + len(u)
        own = _own(eng, cubes, dom, u, boxes)
        assert _bits(steps[a:b], own.composite_steps), f"{tag} track {k}: batch_composite_steps is not the own run's"
        assert _bits(lon[a:b], own.composite_lon), f"{tag} track {k}: batch_composite_lon is not the own run's"
        assert _bits(mean[k], own.composite_mean), f"{tag} track {k}: batch_composite_mean is not the own run's"
        Ck, Hk, Mk = per[k]
        _close(steps[a:b].cpu().numpy(), Ck, (0, 2, 3), f"{tag} track {k} batch_composite_steps")
        _close(lon[a:b].cpu().numpy(), Hk, (0, 2), f"{tag} track {k} batch_composite_lon")
        _close(mean[k].cpu().numpy(), Mk, (1, 2), f"{tag} track {k} batch_composite_mean")
        a = b
    got = res.batch_composite_ensemble.cpu().numpy()
    assert got.shape == (6, nyb, nxb)
    _close(got, ens, (1, 2), f"{tag} batch_composite_ensemble")
    assert np.array_equal(got, _ensemble_in_order(mean.cpu().numpy()), equal_nan=True), f"{tag}: the ensemble is the in-order sum / K"


@pytest.mark.parametrize("nyb, nxb, nl, dtype, ny, nx", CASES, ids=IDS)
def test_every_track_is_its_own_run_and_the_restatement(nyb, nxb, nl, dtype, ny, nx):
    dom = _dom(nl, ny, nx, dtype)
    tracks = _tracks(nyb, nxb, ny, nx)
    assert [len(u) for u, _ in tracks] == [9, 5, 2] and all(b[1] < nx and b[3] < ny for _, bx in tracks for b in bx)
    ref = _reference(("ref", nyb, nxb, nl, np.dtype(dtype).name), dom, tracks)
    assert all(np.isfinite(c).all() for c, _, _ in ref[0])
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    cubes = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    res = _batch(eng, cubes, dom, tracks, batch_composite_steps=True)
    _check_against_own_and_restatement(eng, cubes, dom, tracks, res, ref, f"{nyb}x{nxb}x{nl} {np.dtype(dtype).name}")


def test_nan_in_one_track_is_the_restatements_and_leaves_the_others():
    """In B's band, at union step 4 (B's step 2): T NaN at one interior level at two points of one box row -- that level of the row is NaN
    through the zonal mean and is BRIDGED --, and T NaN at every level of one point of another row -- that row's columns are NaN."""
    nyb, nxb, nl, ny, nx = 5, 65, 8, 24, 80
    base = _dom(nl, ny, nx, np.float64)
    tracks = _tracks(nyb, nxb, ny, nx)
    iw, _, js, _ = tracks[1][1][2]
    assert tracks[1][0][2] == 4
    T = base.tair.copy()
    T[4, 3, js + 1, [iw + 7, iw + 8]] = np.nan
    T[4, :, js + 3, iw + 40] = np.nan
    for k in (0, 2):            # the other tracks' boxes never hold those rows
        assert all(b[3] < js or b[2] > js + nyb - 1 for b in tracks[k][1])
    dom = o.Domain(T, base.u, base.v, base.omega, base.geopt, base.lat, base.lon, base.level, base.time_s)
    ref = br.composites(dom, tracks)
    ae = MAP_TERMS.index("Ae")
    Cb = ref[0][1][0]
    # (B's steps 1 and 3 take T of union step 4 on their own boxes for dT/dt: their Ge may see the NaN too, as in B's own run)
    assert np.isfinite(Cb[2, ae, 1]).all() and np.isnan(Cb[2, ae, 3]).all() and np.isfinite(Cb[[0, 4]]).all()
    assert np.isnan(ref[1][ae, 3]).all() and np.isfinite(ref[1][ae, 1]).all()
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    clean = [_dev(a) for a in (base.tair, base.u, base.v, base.omega, base.geopt)]
    cubes = [_dev(T)] + clean[1:]
    res = _batch(eng, cubes, dom, tracks, batch_composite_steps=True)
    _check_against_own_and_restatement(eng, cubes, dom, tracks, res, ref, "NaN in track 1")
    plain = _batch(eng, clean, base, tracks, batch_composite_steps=True)
    for k, (a, b) in ((0, (0, 9)), (2, (14, 16))):
        assert torch.equal(res.batch_composite_mean[k], plain.batch_composite_mean[k]), k
        assert torch.equal(res.batch_composite_lon[a:b], plain.batch_composite_lon[a:b]), k
        assert torch.equal(res.batch_composite_steps[a:b], plain.batch_composite_steps[a:b]), k
    assert not torch.equal(res.batch_composite_mean[1].isnan(), plain.batch_composite_mean[1].isnan())


def test_a_tracks_bits_do_not_depend_on_its_company():
    nyb, nxb, nl, ny, nx = 5, 65, 8, 24, 80
    dom = _dom(nl, ny, nx, np.float64)
    A, B, Ct = _tracks(nyb, nxb, ny, nx)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    cubes = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    alone = _batch(eng, cubes, dom, [B], batch_composite_steps=True)
    two = _batch(eng, cubes, dom, [A, B], batch_composite_steps=True)
    three = _batch(eng, cubes, dom, [Ct, A, B], batch_composite_steps=True)
    for res, k, a in ((two, 1, 9), (three, 2, 11)):
        assert torch.equal(res.batch_composite_mean[k], alone.batch_composite_mean[0])
        assert torch.equal(res.batch_composite_lon[a:a + 5], alone.batch_composite_lon)
        assert torch.equal(res.batch_composite_steps[a:a + 5], alone.batch_composite_steps)
    assert torch.equal(alone.batch_composite_ensemble, alone.batch_composite_mean[0])       # K = 1: the mean itself
    assert not torch.isnan(three.batch_composite_ensemble).any()


@pytest.mark.parametrize("per_call", [3, 7, 1])
def test_sub_calls_inside_a_track_and_at_a_boundary_keep_the_bits(per_call):
    """MAP_CHUNK_BYTES set on the engine instance: 16 boxes (9 + 5 + 2) in sub-calls of 3 (cuts inside A and B, and exactly between
    them at 9), of 7 (a cut exactly between B and C at 14) and of 1."""
    nyb, nxb, nl, ny, nx = 5, 65, 8, 24, 80
    dom = _dom(nl, ny, nx, np.float64)
    tracks = _tracks(nyb, nxb, ny, nx)
    cubes = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    whole = _batch(eng, cubes, dom, tracks)
    assert whole.batch_composite_steps is None
    kept_whole = _batch(eng, cubes, dom, tracks, batch_composite_steps=True)
    cut_eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    cut_eng.MAP_CHUNK_BYTES = per_call * 8 * (6 * nyb * nxb + nl * nyb * _lib.LEC_MAPS_NCOEF)
    assert LECEngine.MAP_CHUNK_BYTES == 256 << 20
    for kept in (False, True):
        cut = _batch(cut_eng, cubes, dom, tracks, batch_composite_steps=kept)
        for name in ("batch_composite_mean", "batch_composite_lon", "batch_composite_ensemble"):
            assert torch.equal(getattr(cut, name), getattr(whole, name)), (name, kept)
            assert torch.equal(getattr(kept_whole, name), getattr(whole, name)), name
        if kept:        # every sub-call's columns at their own place of the kept array
            assert torch.equal(cut.batch_composite_steps, kept_whole.batch_composite_steps)
        else:
            assert cut.batch_composite_steps is None
    assert not torch.isnan(whole.batch_composite_mean).any()


def test_ensemble_call_forms_the_means_and_their_mean_in_order():
    """``lec_composite_ensemble`` on sums of its own (``batch_composite_finish``): mean[k] is the sum TIMES the rounded reciprocal of the
    count (fp64 products and reciprocals are IEEE on both sides), the ensemble the in-order sum of the means over K; NaN propagates."""
    nyb, nxb, sizes = 5, 65, [9, 5, 2, 7]
    dom = _dom(8, 24, 80, np.float64)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    boxes = [(n % 10, n % 10 + nxb - 1, n % 7, n % 7 + nyb - 1) for n in range(sum(sizes))]
    state = eng.batch_composite_begin(sizes, eng.prepare_boxes(boxes), DEV)
    sums = torch.randn(state["mapsum"].shape, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) * 1e3
    sums[2, 1, 3, 40] = float("nan")
    state["mapsum"].copy_(sums)
    res = types.SimpleNamespace()
    eng.batch_composite_finish(res, state)
    torch.cuda.synchronize()
    want = sums.cpu().numpy() * (1.0 / np.asarray(sizes, dtype=np.float64))[:, None, None, None]
    got = res.batch_composite_mean.cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True) and np.isnan(got).sum() == 1
    ens = res.batch_composite_ensemble.cpu().numpy()
    assert np.array_equal(ens, _ensemble_in_order(want), equal_nan=True) and np.isnan(ens).sum() == 1 and np.isnan(ens[1, 3, 40])


def test_sixteen_and_seventeen_steps_side_by_side():
    """The time sum issues its loads 16 at a time: a track of exactly 16 steps and one of 17, in one call."""
    nyb, nxb, nl, ny, nx, nt = 4, 5, 8, 8, 14, 18
    dom = _dom(nl, ny, nx, np.float64, nt=nt)
    place = lambda n, k: ((2 * n + 3 * k) % (nx - nxb + 1), (n + k) % (ny - nyb + 1))
    tracks = []
    for k, u in enumerate((np.arange(1, 17), np.arange(0, 17))):
        tracks.append((u, [(i, i + nxb - 1, j, j + nyb - 1) for i, j in (place(n, k) for n in range(len(u)))]))
    assert [len(u) for u, _ in tracks] == [16, 17]
    ref = _reference(("ref-16-17",), dom, tracks)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    cubes = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    res = _batch(eng, cubes, dom, tracks, batch_composite_steps=True)
    _check_against_own_and_restatement(eng, cubes, dom, tracks, res, ref, "16 + 17 steps")


def test_without_the_keyword_nothing_changes():
    nyb, nxb, nl, ny, nx = 5, 65, 8, 24, 80
    dom = _dom(nl, ny, nx, np.float64)
    tracks = _tracks(nyb, nxb, ny, nx)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    cubes = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    plain, again, with_b = (_batch(eng, cubes, dom, tracks, batch_composites=None), _batch(eng, cubes, dom, tracks, batch_composites=None),
                            _batch(eng, cubes, dom, tracks))
    for f in dataclasses.fields(plain):
        a, b, c = getattr(plain, f.name), getattr(again, f.name), getattr(with_b, f.name)
        if f.name.startswith("batch_composite_"):
            assert a is None and b is None, f.name
            continue
        assert (a is None) == (b is None) == (c is None), f.name
        if a is not None:
            assert torch.equal(a, b) and torch.equal(a, c), f.name
    assert with_b.batch_composite_mean is not None and with_b.batch_composite_ensemble is not None and with_b.batch_composite_steps is None
    assert with_b.composite_mean is None


def test_device_table_entry_outside_the_cube_reads_nothing_and_gives_nan():
    """The host copy of the table is what the call validates; the kernel checks the device copy once more.  A device row that names a step
    outside the cube (the host copy is valid) leaves that box's columns NaN and every other box's bits alone."""
    nyb, nxb, nl, ny, nx = 5, 65, 8, 24, 80
    dom = _dom(nl, ny, nx, np.float64)
    tracks = _tracks(nyb, nxb, ny, nx)[:1]
    st, tc, boxes, sizes = _table(dom, tracks)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    cubes = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    pb = eng.prepare_boxes(boxes)
    rows = eng.rowstats(*cubes, pb, steps=_dev(st), tcoef=_dev(tc), per_step_boxes=True)
    levraw = torch.empty((len(boxes), nl, _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
    eng.level_stage(rows, pb, levraw)
    out = {}
    for name, table in (("good", st), ("bad", np.where(np.arange(9)[:, None] == 4, np.array([[4, 3, NT]]), st).astype(np.int32))):
        f64 = dict(dtype=torch.float64, device=DEV)
        col, hov = torch.zeros((9, 6, nyb, nxb), **f64), torch.zeros((9, 6, nxb), **f64)
        ms, coef = torch.zeros((1, 6, nyb, nxb), **f64), torch.empty((9, nl, nyb, _lib.LEC_MAPS_NCOEF), **f64)
        box_h, seg_h, st_d = np.ascontiguousarray(boxes, dtype=np.int32), np.array([0, 9], dtype=np.int32), _dev(table)
        seg_d, tc_d = _dev(seg_h), _dev(tc)
        p = lambda t: C.c_void_p(t.data_ptr())
        a = _lib.CompositeStepsArgs(
            tair_d=p(cubes[0]), u_d=p(cubes[1]), v_d=p(cubes[2]), omega_d=p(cubes[3]), dtype=_lib.LEC_F64, nt=NT, nl=nl, ny=ny, nx=nx,
            s_count=9, nyb=nyb, nxb=nxb, n_seg=1, reserved0=0, step_h=st.ctypes.data, step_d=p(st_d), seg_h=seg_h.ctypes.data, seg_d=p(seg_d),
            box_h=box_h.ctypes.data, box_d=p(pb.dev["box"]), boxtab_d=p(pb.dev["boxtab"]), lattab_d=p(pb.dev["lattab"]),
            lattab2_d=p(pb.dev["lattab2"]), rows_d=p(rows), levraw_d=p(levraw), levtab_d=p(eng._levtab), levtab2_d=p(eng._levtab2),
            tcoef_d=p(tc_d), coef_d=p(coef), col_d=p(col), mapsum_d=p(ms), hov_d=p(hov),
            stream=C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        _lib.check(eng.lib.lec_composite_steps(C.byref(a)), "lec_composite_steps")
        torch.cuda.synchronize()
        out[name] = (col, hov, ms)
    good, bad = out["good"], out["bad"]
    assert not torch.isnan(good[0]).any()
    assert torch.isnan(bad[0][4]).all() and torch.isnan(bad[1][4]).all() and torch.isnan(bad[2]).all()
    keep = [0, 1, 2, 3, 5, 6, 7, 8]
    assert torch.equal(bad[0][keep], good[0][keep]) and torch.equal(bad[1][keep], good[1][keep])
