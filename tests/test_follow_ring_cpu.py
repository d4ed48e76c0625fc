"""-c --choose-periodic and the track across the +-180 meridian, the parts that need no GPU: the longitude origin of the axes and of a
track, births / resolve on the ring, the command line's refusals, the periodic vorticity tables, the ring calls' argument validation
(before any HIP call), and the NumPy restatement of the ring rule (tests/follow_ring_restatement.py): its roll invariance and the
margins of the cases tests/test_gpu_follow_ring.py holds the kernels to."""
import ctypes
import os
import shutil

import numpy as np
import pandas as pd
import pytest

from lorenzcycletoolkit_amd import _lib, dataset as ds, follow as fw
from lorenzcycletoolkit_amd.diagnostics import vorticity_tables
from tests import follow_ring_cases as rc
from tests import follow_ring_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TESTDATA = os.path.join(GOLDEN, "testdata_NCEP-R2.nc")
NAMES = {"Vertical Level": "level"}
LEV = np.array([1000.0, 850.0, 500.0])
TIME = np.arange(4).astype("datetime64[h]").astype("datetime64[ns]")
NEAR_TIE = 1e-9


# ---- the axes ------------------------------------------------------------------------------------------------------------------
def test_sorted_axes_with_origin_180_is_one_axis_for_both_file_conventions():
    a = ds._sorted_axes(None, rc.LAT, rc.LON % 360.0, LEV, TIME, "hPa", NAMES, lon_origin=180.0)        # a 0 .. 360 file (unsorted there)
    b = ds._sorted_axes(None, rc.LAT, rc.LON, LEV, TIME, "hPa", NAMES, lon_origin=180.0)                # a -180 .. 180 file
    assert np.array_equal(a.lon, b.lon) and np.array_equal(a.lon, 5.0 * np.arange(72))
    for px, file_lon in ((a, rc.LON % 360.0), (b, rc.LON)):
        assert sorted(px.io.tolist()) == list(range(72))                                               # a permutation
        assert np.array_equal(file_lon[px.io] % 360.0, px.lon)
    today = ds._sorted_axes(None, rc.LAT, rc.LON % 360.0, LEV, TIME, "hPa", NAMES)
    assert np.array_equal(today.lon, rc.LON) and np.array_equal(today.lon, ds._sorted_axes(None, rc.LAT, rc.LON, LEV, TIME, "hPa", NAMES, lon_origin=0.0).lon)
    with pytest.raises(ValueError, match="origin"):
        ds._sorted_axes(None, rc.LAT, rc.LON, LEV, TIME, "hPa", NAMES, lon_origin=90.0)


def _track(lons, width=None):
    t = pd.DataFrame({"Lat": -40.0, "Lon": np.asarray(lons, dtype=np.float64)}, index=pd.DatetimeIndex(TIME[:len(lons)], name="time"))
    if width is not None:
        t["length"], t["width"] = 10.0, width
    return t


def test_track_lon_origin():
    regional = -180.0 + 2.5 * np.arange(33)                                    # -180 .. -100
    assert ds.track_lon_origin(rc.LON, _track([-60.0, -55.0, -50.0])) == 0.0   # interior
    assert ds.track_lon_origin(rc.LON, _track([177.5, -177.5])) == 180.0       # steps across the meridian
    assert ds.track_lon_origin(rc.LON, _track([-178.0, -178.0])) == 180.0      # a box edge beyond -180 on a ring
    assert ds.track_lon_origin(rc.LON % 360.0, _track([-178.0, -178.0])) == 180.0
    assert ds.track_lon_origin(regional, _track([-178.0, -178.0])) == 0.0      # ... on a regional file: nothing west of it to read
    assert ds.track_lon_origin(rc.LON, _track([-174.0, -174.0], width=10.0)) == 0.0          # the track's own width decides: -179 is inside
    assert ds.track_lon_origin(rc.LON, _track([-174.0, -174.0], width=15.0)) == 180.0
    gappy = np.r_[np.arange(0.0, 181.0, 5.0), np.arange(200.0, 360.0, 5.0)] - 180.0 + 180.0  # no column between 180 and 200 on 0 .. 360
    assert ds.track_lon_origin(gappy, _track([177.5, -177.5])) == 0.0
    why = []
    assert ds.track_lon_origin(rc.LON, _track([177.5, -177.5]), why) == 180.0 and "180 degrees" in why[0]
    # what everything downstream reads
    on = ds.track_on_axis(_track([177.5, -177.5]), 5.0 * np.arange(72))
    assert on["Lon"].tolist() == [177.5, 182.5] and ds.track_on_axis(_track([177.5, -177.5]), rc.LON)["Lon"].tolist() == [177.5, -177.5]
    assert ds.wrap180(np.array([177.5, 182.5, 180.0, 359.0])).tolist() == [177.5, -177.5, -180.0, -1.0]


def test_process_index_derives_the_origin_from_the_track(tmp_path):
    path = tmp_path / "track"
    fw.write_track(path, TIME[:2], [-40.0, -40.0], [177.5, -177.5], 10.0, 10.0)
    args = lambda **kw: type("A", (), dict(track=True, trackfile=str(path), **kw))()
    px = ds.process_index(rc.LAT, rc.LON, LEV, TIME, "hPa", NAMES, args())
    assert px.lon[0] == 0.0 and px.lon[-1] == 355.0 and px.tpos.tolist() == [0, 1]
    js, is_ = ds.domain_slices(px.lat, px.lon, args())
    assert px.lon[is_][0] == 170.0 and px.lon[is_][-1] == 190.0                # 167.5 .. 192.5 (the extent -+ half a box -+ dx): across the meridian, contiguous
    assert ds.process_index(rc.LAT, rc.LON, LEV, TIME, "hPa", NAMES, args(lon_origin=0.0)).lon[0] == -180.0


# ---- births / resolve on the ring ------------------------------------------------------------------------------------------------
def test_births_and_resolve_measure_columns_on_the_ring():
    seed_pos = np.array([[[10, 71]], [[10, 1]]])
    n_found = np.array([1, 1])
    assert fw.births(seed_pos, n_found, rc.SJ, rc.SI).tolist() == [[0, 10, 71, 0], [1, 10, 1, 0]]          # 70 columns apart: a second birth
    assert fw.births(seed_pos, n_found, rc.SJ, rc.SI, nx=72).tolist() == [[0, 10, 71, 0]]                  # 2 columns apart on the ring
    assert fw.births(seed_pos, n_found, rc.SJ, 1, nx=72).tolist() == [[0, 10, 71, 0], [1, 10, 1, 0]]
    starts = np.array([[0, 10, 71], [1, 10, 1]])
    pos = np.array([[[10, 71], [10, 71]], [[-1, -1], [10, 1]]])
    span = np.array([[0, 1], [1, 1]])
    kept, cont = fw.resolve(starts, pos, span, 2, 2)
    assert kept.tolist() == [True, True] and cont.tolist() == [-1, -1]
    kept, cont = fw.resolve(starts, pos, span, 2, 2, nx=72)
    assert kept.tolist() == [True, False] and cont.tolist() == [-1, 0]
    assert fw.ring_distance(np.array([0, 71, 36]), 1, 72).tolist() == [1, 2, 35]


def test_ring_error_and_the_ring_s_admissible_centres():
    assert fw.ring_error(rc.LON) is None and fw.ring_error(5.0 * np.arange(72)) is None
    assert "71 columns of 5.0 degrees = 355.0 degrees, not the 360" in fw.ring_error(rc.LON[:-1])
    assert "unevenly" in fw.ring_error(np.r_[rc.LON[:40], rc.LON[41:]])
    assert fw.admissible(rc.LAT, rc.LON, 10, 10) == (2, 30, 1, 70)
    assert fw.admissible(rc.LAT, rc.LON, 10, 10, periodic=True) == (2, 30, 0, 71)
    assert fw.start_index(rc.LAT, rc.LON, (-40.0, 179.0), (2, 30, 0, 71), periodic=True) == (16, 0)
    assert fw.start_index(rc.LAT, rc.LON, (-40.0, 179.0), (2, 30, 1, 70)) == (16, 70)


def test_without_the_flag_a_chain_that_ends_at_the_seam_is_named(caplog):
    import logging
    import types
    log = logging.getLogger("seam-notes")
    note = lambda periodic, lon, cols: fw._seam_notes(log, types.SimpleNamespace(periodic=periodic, lon=lon), [f"choose_s{n + 1:02d}" for n in range(len(cols))], cols, rc.SI)
    with caplog.at_level(logging.INFO, logger="seam-notes"):
        note(False, rc.LON, [40, 69, None, 3, 67, 4])                   # within si = 3 columns of either edge: 69 and 3
    said = [r.getMessage() for r in caplog.records]
    assert len(said) == 2 and "choose_s02" in said[0] and "choose_s04" in said[1] and all("ended at the seam: --choose-periodic" in m for m in said)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="seam-notes"):
        note(True, rc.LON, [69])                                        # with the flag there is no seam to end at
        note(False, rc.LON[:41], [40])                                  # a regional domain's edge is an edge
    assert not caplog.records
    assert fw._last_good_columns(np.array([[[5, 70], [5, 71], [5, 71]]]), np.array([[0, 0, 1]])) == [71]
    assert fw._last_good_columns(np.array([[[5, 70]]]), np.array([[1]])) == [None]


# ---- the command line --------------------------------------------------------------------------------------------------------------
@pytest.fixture
def workdir(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    shutil.copy(os.path.join(GOLDEN, "inputs", "namelist_NCEP-R2"), tmp_path / "inputs" / "namelist")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return tmp_path


def test_choose_periodic_on_a_regional_file_is_refused_with_the_extent(workdir):
    import lorenzcycletoolkit
    with pytest.raises(ValueError, match=r"--choose-periodic.*from -100\.0 to 0\.0 in 41 columns.*not the 360"):
        lorenzcycletoolkit.main([TESTDATA, "-r", "-c", "--choose-periodic"])
    assert os.listdir(workdir / "LEC_Results" / "testdata_NCEP-R2_choose") == ["log.testdata_NCEP-R2"]
    with pytest.raises(ValueError, match="--choose-periodic.*41 columns"):
        lorenzcycletoolkit.main([TESTDATA, "-r", "-c", "--choose-periodic", "--choose-systems", "2"])


def test_choose_periodic_goes_with_choose(workdir):
    import lorenzcycletoolkit
    with pytest.raises(SystemExit, match="--choose-periodic goes with -c/--choose"):
        lorenzcycletoolkit.main([TESTDATA, "-r", "-t", "--choose-periodic"])
    assert "choose_periodic" in lorenzcycletoolkit.CHOOSE_OPTIONS


# ---- tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["metpy_no_crs", "spherical"])
def test_periodic_tables_are_the_plain_ones_away_from_the_seam(form):
    plain, ring = vorticity_tables(rc.LAT, rc.LON, form), vorticity_tables(rc.LAT, rc.LON, form, periodic=True)
    assert ring[0].shape == plain[0].shape == (33, 72, 3)
    assert np.array_equal(ring[0][:, 1:-1].view(np.int64), plain[0][:, 1:-1].view(np.int64))            # bit for bit
    assert np.array_equal(ring[1].view(np.int64), plain[1].view(np.int64)) and np.array_equal(ring[2].view(np.int64), plain[2].view(np.int64))
    # at the seam: the centred stencil over the arc across it -- on an even ring what every other column has (to rounding)
    for i in (0, 71):
        assert np.allclose(ring[0][:, i], ring[0][:, 5], rtol=1e-12, atol=0) and not np.allclose(ring[0][:, i], plain[0][:, i], rtol=1e-3)
    # the restatement's field (independent: the oracle's stencil on a wrapped slice) is what these tables give
    u, v, h, _, _ = rc.planted(3, nt=1, **rc.EAST)
    F = rr.field_of(u, v, h, rc.LAT, rc.LON, "zeta", form)[0]
    xc, yc, cv = ring
    vw, ve = np.roll(v[0], 1, axis=1), np.roll(v[0], -1, axis=1)
    dv = xc[..., 0] * vw + xc[..., 1] * v[0] + xc[..., 2] * ve
    j0 = np.clip(np.arange(33) - 1, 0, 30)
    du = yc[:, 0, None] * u[0][j0] + yc[:, 1, None] * u[0][j0 + 1] + yc[:, 2, None] * u[0][j0 + 2]
    assert np.max(np.abs(dv - du + cv[:, None] * u[0] - F)) <= 1e-11 * np.max(np.abs(F))


# ---- the ring calls' validation: before any HIP call --------------------------------------------------------------------------------
def _chunk_args(**change):
    a = _lib.FollowChunkArgs()
    for f in ("u_d", "v_d", "hgt_d", "xcoef_d", "ycoef_d", "curv_d", "start_d", "pos_d", "val_d", "status_d", "span_d", "state_d"):
        setattr(a, f, 4096)                        # an address nothing dereferences: validation comes first
    a.nt, a.ny, a.nx = 4, 33, 72
    a.field, a.sense, a.smooth_r, a.sj, a.si = _lib.FOLLOW_ZETA, _lib.FOLLOW_MIN, 2, 6, 3
    a.jlo, a.jhi, a.ilo, a.ihi, a.n_chains, a.patience, a.t_base = 2, 30, 0, 71, 1, 2, 0
    a.end_threshold = float("nan")
    for k, v in change.items():
        setattr(a, k, v)
    return a


def _seeds_args(**change):
    a = _lib.FollowSeedsSeriesArgs()
    for f in ("u_d", "v_d", "hgt_d", "xcoef_d", "ycoef_d", "curv_d", "work_d", "seed_pos_d", "seed_val_d", "n_found_d"):
        setattr(a, f, 4096)
    a.nt, a.ny, a.nx = 4, 33, 72
    a.field, a.sense, a.smooth_r, a.ej, a.ei, a.k_max = _lib.FOLLOW_ZETA, _lib.FOLLOW_MIN, 0, 2, 1, 4
    a.jlo, a.jhi, a.ilo, a.ihi, a.threshold = 2, 30, 0, 71, float("nan")
    for k, v in change.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("change, word", [
    ({"nx": 10, "ihi": 9}, b"2 si + 1 + 2 smooth_r"),              # 11 columns on a ring of 10: the window would meet itself
    ({"ilo": 1}, b"ilo = 0"), ({"ihi": 70}, b"ihi = nx - 1"),
    ({"si": 34, "smooth_r": 2}, b"2 si + 1 + 2 smooth_r"),
    ({"u_d": None}, b"u_d"), ({"state_d": None}, b"state_d"), ({"patience": -1}, b"patience"), ({"t_base": -1}, b"t_base"),
    ({"si": 0}, b"si"), ({"jhi": 33}, b"jhi"), ({"field": 7}, b"field"),
])
def test_spans_chunk_ring_refuses_without_a_gpu(change, word):
    lib = _lib.load()
    assert lib.lec_follow_spans_chunk_ring(ctypes.byref(_chunk_args(**change))) == 1
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_follow_spans_chunk_ring") and word in msg, msg


@pytest.mark.parametrize("change, word", [
    ({"ei": 36}, b"2 ei + 1"), ({"ilo": 1}, b"ilo = 0"), ({"ihi": 70}, b"ihi = nx - 1"), ({"smooth_r": 36}, b"2 smooth_r + 1"),
    ({"work_d": None}, b"work_d"), ({"k_max": 0}, b"k_max"), ({"ej": 0}, b"ej"), ({"nt": 0}, b"nt"),
])
def test_seeds_series_ring_refuses_without_a_gpu(change, word):
    lib = _lib.load()
    assert lib.lec_follow_seeds_series_ring(ctypes.byref(_seeds_args(**change))) == 1
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_follow_seeds_series_ring") and word in msg, msg


def test_the_ring_calls_are_additive():
    lib = _lib.load()
    assert lib.lec_version() == _lib.LEC_ABI_VERSION == 11
    assert lib.lec_follow_spans_chunk_ring(None) == 1 and lib.lec_follow_seeds_series_ring(None) == 1
    # the same structs as the non-ring calls, unchanged (every call in this file is one the library refuses: nothing is ever launched)
    assert ctypes.sizeof(_lib.FollowChunkArgs) == ctypes.sizeof(_lib.FollowSpansArgs) + 16
    assert ctypes.sizeof(_lib.FollowSeedsSeriesArgs) == 3 * 8 + 4 * 4 + 3 * 8 + 10 * 4 + 6 * 8


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _walk(u, v, h, field, r, start, sizes=(rc.NT,), form="metpy_no_crs", **kw):
    j, i = rc.start_of(start)
    return rr.walk_chunked(u, v, h, rc.LAT, rc.LON, [(0, j, i)], list(sizes), smooth=r, field=field, formulation=form, patience=0, **rc.BOX, **kw)


@pytest.mark.parametrize("field", ["hgt", "zeta"])
@pytest.mark.parametrize("r", [0, 2])
def test_the_restatement_is_roll_invariant(field, r):
    """A ring has no preferred meridian: the data rolled by k columns give the positions shifted by k and the same values -- hgt bit
    for bit (no arithmetic depends on the column), zeta to rounding (the oracle's stencil runs on the running sum of the spacings)."""
    u, v, h, start, _ = rc.planted(11, **rc.EAST)
    ref = _walk(u, v, h, field, r, start)
    assert ref["margin"].min() > NEAR_TIE
    for k in (1, 36, 69):
        roll = lambda a: np.roll(a, k, axis=-1)
        got = _walk(roll(u), roll(v), roll(h), field, r, (start[0], start[1] + 5.0 * k))
        assert np.array_equal(got["pos"][..., 0], ref["pos"][..., 0]) and np.array_equal(got["pos"][..., 1], (ref["pos"][..., 1] + k) % 72)
        assert np.array_equal(got["status"], ref["status"])
        if field == "hgt":
            assert np.array_equal(got["val"].view(np.int64), ref["val"].view(np.int64))
        else:
            assert np.max(np.abs(got["val"] - ref["val"])) <= 1e-12 * ref["scale"]
        s0 = rr.seeds(u[0], v[0], h[0], rc.LAT, rc.LON, k=3, smooth=r, field=field, length=10.0, width=10.0)
        s1 = rr.seeds(roll(u[0]), roll(v[0]), roll(h[0]), rc.LAT, rc.LON, k=3, smooth=r, field=field, length=10.0, width=10.0)
        assert s0["margin"] > NEAR_TIE and np.array_equal(s1["pos"][:, 0], s0["pos"][:, 0]) and np.array_equal(s1["pos"][:, 1], (s0["pos"][:, 1] + k) % 72)


@pytest.mark.parametrize("case", ["EAST", "WEST"])
def test_the_planted_systems_cross_the_seam_with_margins_far_above_the_bar(case):
    """What tests/test_gpu_follow_ring.py relies on: the chain walks columns 69, 70, 71, 0, 1, 2 (or the other way), every window's
    margin is far above NEAR_TIE, for both fields, both formulations and r = 0 and 2 -- so no step there may be left out as a near tie."""
    u, v, h, start, path = rc.planted(11, **getattr(rc, case))
    want = [69, 70, 71, 0, 1, 2] if case == "EAST" else [2, 1, 0, 71, 70, 69]
    for field, form in (("hgt", "metpy_no_crs"), ("zeta", "metpy_no_crs"), ("zeta", "spherical")):
        for r in (0, 2):
            ref = _walk(u, v, h, field, r, start, form=form)
            cols = ref["pos"][0, :, 1].tolist()
            assert [c for n, c in enumerate(cols) if n == 0 or c != cols[n - 1]] == want, (field, form, r, cols)
            assert ref["margin"].min() > 1000 * NEAR_TIE, (field, form, r, ref["margin"].min())
            assert not ref["status"].any()
            track_lon = rc.LON[ref["pos"][0, :, 1]]
            assert np.all(np.abs(rc.ring_dx(track_lon, path)) <= 5.0)                                   # on the planted path, across the meridian
            cut = _walk(u, v, h, field, r, start, sizes=(5, 1, 6), form=form)                            # the state carries the crossing
            assert np.array_equal(cut["pos"], ref["pos"]) and np.array_equal(cut["val"].view(np.int64), ref["val"].view(np.int64))


def test_restated_seeds_on_the_seam():
    """One low at column 0 with a weaker twin at column 71: one seed on the ring -- the twin lies within ei of the low."""
    h = np.full((33, 72), 1500.0)
    h[16, 0], h[16, 71] = 1400.0, 1450.0
    z = np.zeros((33, 72))
    s = rr.seeds(z, z, h, rc.LAT, rc.LON, k=4, threshold=1480.0, field="hgt", length=10.0, width=10.0)
    assert s["pos"].tolist() == [[16, 0]] and s["val"].tolist() == [1400.0] and (s["ej"], s["ei"]) == (2, 1)
    # a tie across the seam: the slice's absolute row-major order decides -- column 0 comes before column 71
    h[16, 71] = 1400.0
    assert rr.seeds(z, z, h, rc.LAT, rc.LON, k=4, threshold=1480.0, field="hgt", length=10.0, width=10.0)["pos"].tolist() == [[16, 0]]
