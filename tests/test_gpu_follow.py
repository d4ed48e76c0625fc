"""-c/--choose without a display, on the GPU: ``lec_follow`` against the NumPy restatement of the rule (tests/follow_restatement.py),
against ``lec_track_diag`` on its own windows, and the defining property of the command line -- a ``-c`` run IS the ``-t`` run on the
track it wrote, byte for byte."""
import os
import shutil
import types

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import diagnostics as dg
from lorenzcycletoolkit_amd import follow as fw
from lorenzcycletoolkit_amd.constants import LEVEL_TERMS
from oracle import lec_oracle as o
from tests import follow_restatement as fr
from tests.test_follow_cpu import GOLDEN_CENTRES

NEAR_TIE = 1e-9          # of the field's scale: below it the restatement's own runner-up could win on another rounding
VALUE_BAR = 1e-11        # x max |F| of the tile: the bar test_gpu_diagnostics.py holds zeta to, which a mean of such values inherits
BOX = dict(length=10.0, width=10.0, search=3.0)


def planted(seed, nt=8, stretched=False, north=False, nan_patch=False, blind_step=None):
    """A vortex (and a height low) moving along a known path over noise, plus a rival twice as strong that stays more than the search
    radius away from the path.  1-degree axes (or stretched ones); southern hemisphere: cyclonic = negative vorticity."""
    rng = np.random.default_rng(seed)
    lat = -60.0 + np.arange(51.0)
    lon = -90.0 + np.arange(71.0)
    if stretched:
        lat = np.sort(lat + 0.25 * np.sin(np.arange(lat.size)))
        lon = np.sort(lon + 0.3 * np.cos(np.arange(lon.size)))
    if north:
        lat = lat + 70.0
    y, x = lat[None, :, None], lon[None, None, :]
    t = np.arange(nt)[:, None, None]
    y0, x0 = lat[0] + 35.0 - 0.7 * t, lon[0] + 22.0 + 1.3 * t        # the path: 1.3 degrees east, 0.7 south per step
    yr, xr = lat[0] + 14.0, lon[0] + 55.0                            # the rival: never nearer than 12 degrees to the path
    sign = 1.0 if north else -1.0

    def vortex(yc, xc, amp, sigma=2.5):
        dy, dx = y - yc, x - xc
        g = np.exp(-(dx * dx + dy * dy) / (2 * sigma * sigma))
        return -sign * amp * dy * g, sign * amp * dx * g, g          # u, v: dv/dx - du/dy = sign * 2 amp at the centre

    u1, v1, g1 = vortex(y0, x0, 6.0)
    u2, v2, g2 = vortex(yr, xr, 12.0)
    shape = (nt, lat.size, lon.size)
    u = u1 + u2 + 0.3 * rng.standard_normal(shape)
    v = v1 + v2 + 0.3 * rng.standard_normal(shape)
    h = 1500.0 - 80.0 * g1 - 160.0 * g2 + 2.0 * rng.standard_normal(shape)
    if nan_patch:                                                    # below-ground points across the path at step 4
        j, i = int(np.argmin(np.abs(lat - y0[4, 0, 0]))), int(np.argmin(np.abs(lon - x0[4, 0, 0])))
        for a in (u, h):
            a[3:6, j - 1: j + 2, i - 1: i + 2] = np.nan
    if blind_step is not None:                                       # a step with nothing finite anywhere
        for a in (u, v, h):
            a[blind_step] = np.nan
    start = (float(y0[0, 0, 0]), float(x0[0, 0, 0]))
    return lat, lon, u, v, h, start, (yr, xr)


def compare(got, ref, what):
    """Positions and status EQUAL; values within the bar; no step may be left out as a near tie."""
    pos, val, status = got
    ok = ref["status"] == 0
    err = np.abs(val[ok] - ref["val"][ok]) / ref["tile_scale"][ok]
    print(what, "margin min %.3e" % ref["margin"].min(), "worst value error / tile scale %.3e" % (err.max() if err.size else 0.0))
    assert int((ref["margin"] < NEAR_TIE).sum()) == 0, (what, ref["margin"])
    assert np.array_equal(status, ref["status"]), (what, status, ref["status"])
    assert np.array_equal(pos, ref["pos"]), (what, pos.tolist(), ref["pos"].tolist())
    assert np.all(np.isnan(val[~ok]))
    assert np.all(err <= VALUE_BAR), (what, val, ref["val"])


@pytest.mark.parametrize("r", [0, 1, 3])
@pytest.mark.parametrize("field", ["zeta", "hgt"])
@pytest.mark.parametrize("form", ["metpy_no_crs", "spherical"])
@pytest.mark.parametrize("stretched", [False, True])
def test_kernel_matches_the_restatement(stretched, form, field, r):
    lat, lon, u, v, h, start, rival = planted(seed=21 + r, stretched=stretched, nan_patch=True)
    for st in (start, None):
        kw = dict(BOX, smooth=r, field=field, start=st, formulation=form)
        ref = fr.follow(u, v, h, lat, lon, **kw)
        got = fw.follow_system(u, v, h, lat, lon, **kw)
        compare(got, ref, (stretched, form, field, r, st))
        track = np.c_[lat[got[0][:, 0]], lon[got[0][:, 1]]]
        if st is None:                                               # without a start the stronger system is picked at step 0 ...
            assert np.all(np.hypot(track[:, 0] - rival[0], track[:, 1] - rival[1]) < 3.0)
        else:                                                        # ... with one the box never jumps to it, and stays on the path
            want = np.c_[start[0] - 0.7 * np.arange(8), start[1] + 1.3 * np.arange(8)]
            assert np.all(np.hypot(track[:, 0] - want[:, 0], track[:, 1] - want[:, 1]) < 4.0)


def test_northern_hemisphere_follows_the_maximum():
    lat, lon, u, v, h, start, _ = planted(seed=5, north=True)
    kw = dict(BOX, start=start)
    ref = fr.follow(u, v, h, lat, lon, **kw)
    got = fw.follow_system(u, v, h, lat, lon, **kw)
    compare(got, ref, "north")
    assert np.all(got[1] > 0)
    south = fw.follow_system(u, v, h, lat, lon, hemisphere="south", **kw)          # asked for: the minimum, another chain
    compare(south, fr.follow(u, v, h, lat, lon, hemisphere="south", **kw), "north data, south rule")
    assert np.all(south[1] < 0)


def test_a_window_without_a_finite_value_keeps_the_centre():
    lat, lon, u, v, h, start, _ = planted(seed=7, blind_step=3)
    for field in ("zeta", "hgt"):
        kw = dict(BOX, start=start, field=field, smooth=1)
        ref = fr.follow(u, v, h, lat, lon, **kw)
        pos, val, status = fw.follow_system(u, v, h, lat, lon, **kw)
        compare((pos, val, status), ref, ("blind", field))
        assert status.tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and tuple(pos[3]) == tuple(pos[2]) and np.isnan(val[3])
    lat, lon, u, v, h, start, _ = planted(seed=7, blind_step=0)
    with pytest.raises(ValueError, match="first time step"):
        fw.follow_system(u, v, h, lat, lon, start=start, **BOX)
    with pytest.raises(ValueError, match="first time step"):
        fw.follow_system(u, v, h, lat, lon, **BOX)


def test_equal_values_take_the_first_in_row_major_order():
    lat, lon, u, v, h, start, _ = planted(seed=9, nt=3)
    bounds = fw.admissible(lat, lon, 10, 10)
    j, i = fw.start_index(lat, lon, start, bounds)
    h[:] = 1500.0
    h[0, j + 2, i - 1] = h[0, j - 1, i + 2] = h[0, j - 1, i + 3] = 1400.0           # three equal minima inside the first window (sj = si = 3)
    pos, val, status = fw.follow_system(u, v, h, lat, lon, field="hgt", start=start, **BOX)
    assert tuple(pos[0]) == (j - 1, i + 2) and val[0] == 1400.0
    assert tuple(pos[1]) == (j - 4, i - 1) and val[1] == 1500.0                     # all equal: the window's first point
    assert not status.any()
    ref = fr.follow(u, v, h, lat, lon, field="hgt", start=start, **BOX)
    assert np.array_equal(pos, ref["pos"]) and np.array_equal(val, ref["val"])


@pytest.mark.parametrize("form", ["metpy_no_crs", "spherical"])
def test_windows_agree_with_lec_track_diag_bit_for_bit(form):
    """Kernel against kernel, r = 0: lec_track_diag on boxes equal to the tracker's own windows finds the same extremum -- the same
    double and the same grid point -- at every step (one zeta_at for both)."""
    lat, lon, u, v, h, start, _ = planted(seed=31, nt=12, stretched=True, nan_patch=True)
    pos, val, status = fw.follow_system(u, v, h, lat, lon, start=start, formulation=form, **BOX)
    jlo, jhi, ilo, ihi = fw.admissible(lat, lon, 10, 10)
    sj, si = fw.window_steps(lat, lon, 3.0)
    centre = fw.start_index(lat, lon, start, (jlo, jhi, ilo, ihi))
    limits = []
    for t in range(len(pos)):
        j0, j1, i0, i1 = max(jlo, centre[0] - sj), min(jhi, centre[0] + sj), max(ilo, centre[1] - si), min(ihi, centre[1] + si)
        limits.append({"min_lat": lat[j0], "max_lat": lat[j1], "min_lon": lon[i0], "max_lon": lon[i1], "central_lat": lat[centre[0]], "central_lon": lon[centre[1]]})
        centre = tuple(pos[t])
    dval, dpos = dg.device_extrema(u, v, h, lat, lon, limits, formulation=form)
    assert not status.any()
    assert np.array_equal(dval[:, 0].copy().view(np.int64), val.view(np.int64))   # bit for bit
    assert np.array_equal(dpos[:, 0:2], pos)


def test_a_tile_beyond_64_kib_of_lds():
    """A wide search window: 127 x 127 doubles = 129 KB of the 160 KiB a workgroup may declare."""
    rng = np.random.default_rng(3)
    lat, lon = -70.0 + 0.5 * np.arange(140), -100.0 + 0.5 * np.arange(150)
    u, v = rng.standard_normal((2, 3, 140, 150))
    kw = dict(length=4.0, width=4.0, search=31.0, smooth=1, start=(-35.0, -62.0))
    assert fw.window_steps(lat, lon, 31.0) == (62, 62)
    ref = fr.follow(u, v, None, lat, lon, **kw)
    compare(fw.follow_system(u, v, None, lat, lon, **kw), ref, "large tile")
    with pytest.raises(fw._lib.LecLibraryError, match="limit"):
        fw.follow_system(u, v, None, lat, lon, **dict(kw, search=36.0))         # 145 + 2 rows: the slice itself (140 x 147) is over the limit


# ---------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def workdir(tmp_path, golden_dir, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_NCEP-R2"), tmp_path / "inputs" / "namelist")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return tmp_path


def _main(argv):
    import lorenzcycletoolkit
    lorenzcycletoolkit.main(argv)


def _tree(directory, method):
    """name (with the method's word taken out) -> bytes, for the results CSV, the 21 level tables and the trackfile."""
    stem = "testdata_NCEP-R2"
    files = {"results": directory / f"{stem}_{method}_results.csv", "trackfile": directory / f"{stem}_{method}_trackfile"}
    lv = directory / "results_vertical_levels"
    assert sorted(os.listdir(lv)) == sorted(f"{t}_lv_ISBL3.csv" for t in LEVEL_TERMS) and len(LEVEL_TERMS) == 21
    files.update({name: lv / name for name in os.listdir(lv)})
    return {k: p.read_bytes() for k, p in files.items()}


@pytest.mark.parametrize("ingest", ["auto", "device"])
def test_choose_is_track_on_the_track_it_wrote(workdir, golden_dir, ingest):
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    extra = [] if ingest == "auto" else ["--ingest", "device"]
    _main([infile, "-r", "-c", "--choose-start", "-22.5", "-45"] + extra)
    chosen = workdir / "LEC_Results" / "testdata_NCEP-R2_choose"
    written = chosen / "testdata_NCEP-R2_choose_track"
    assert (chosen / "log.testdata_NCEP-R2").exists() and "lec_follow" in (chosen / "log.testdata_NCEP-R2").read_text()
    tr = pd.read_csv(written, sep=";")
    assert list(tr.columns) == ["time", "Lat", "Lon", "length", "width"] and tr["time"][1] == "2005-08-08-0600"
    assert list(zip(tr.Lat, tr.Lon)) == GOLDEN_CENTRES[(-22.5, -45)] and (tr.length == 15).all() and (tr.width == 15).all()
    _main([infile, "-r", "-t", "--trackfile", str(written)] + extra)
    a, b = _tree(chosen, "choose"), _tree(workdir / "LEC_Results" / "testdata_NCEP-R2_track", "track")
    assert a.keys() == b.keys() and len(a) == 23
    for name in a:
        assert a[name] == b[name], name
    # the numbers: the oracle's moving framework on those boxes
    got = pd.read_csv(chosen / "testdata_NCEP-R2_choose_results.csv", index_col=0)
    dom = o.load_ncep_sample(infile, dtype=np.float64)
    domt = o.crop_domain_track(dom, tr.Lat.values, tr.Lon.values)
    ref, _ = o.lec_moving(domt, [(lo - 7.5, lo + 7.5, la - 7.5, la + 7.5) for la, lo in zip(tr.Lat, tr.Lon)])
    for c in ("Az", "Ae", "Kz", "Ke", "Cz", "Ca", "Ck", "Ce", "BAz", "BAe", "BKz", "BKe", "BΦZ", "BΦE", "Gz", "Ge"):
        r = np.asarray(ref[c], dtype=np.float64)
        assert np.max(np.abs(got[c].values - r)) <= 1e-9 * np.max(np.abs(r)), c


def test_choose_options_reach_the_tracker(workdir, golden_dir):
    """No start, a search domain file, smoothing: the written track is the restatement's on that domain."""
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    _main([infile, "-r", "-c"])
    tr = pd.read_csv(workdir / "LEC_Results" / "testdata_NCEP-R2_choose" / "testdata_NCEP-R2_choose_track", sep=";")
    assert list(zip(tr.Lat, tr.Lon)) == GOLDEN_CENTRES[None]
    (workdir / "inputs" / "domain").write_text("min_lon;-80\nmax_lon;-20\nmin_lat;-60\nmax_lat;-5\n")
    _main([infile, "-r", "-c", "--choose-domain", "inputs/domain", "--choose-box", "10", "12.5", "--choose-search", "2.5", "--choose-smooth", "1",
           "--choose-field", "hgt", "--vorticity-form", "spherical"])
    tr = pd.read_csv(workdir / "LEC_Results" / "testdata_NCEP-R2_choose" / "testdata_NCEP-R2_choose_track", sep=";")
    a = types.SimpleNamespace(infile=infile, mpas=False, choose_domain="inputs/domain")
    u, v, h, lat, lon, _ = fw.search_domain_slices(a, "inputs/namelist")
    ref = fr.follow(u, v, h, lat, lon, length=10, width=12.5, search=2.5, smooth=1, field="hgt")
    assert ref["margin"].min() > NEAR_TIE
    assert list(zip(tr.Lat, tr.Lon)) == [(lat[j], lon[i]) for j, i in ref["pos"]]
    assert (tr.length == 10).all() and (tr.width == 12.5).all()
    trk = pd.read_csv(workdir / "LEC_Results" / "testdata_NCEP-R2_choose" / "testdata_NCEP-R2_choose_trackfile", sep=";")
    assert np.allclose(trk["max_lat"] - trk["min_lat"], 10) and np.allclose(trk["max_lon"] - trk["min_lon"], 12.5)


def test_a_box_that_does_not_fit_leaves_only_the_log(workdir, golden_dir):
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    with pytest.raises(ValueError, match="does not fit"):
        _main([infile, "-r", "-c", "--choose-box", "90", "15"])
    assert os.listdir(workdir / "LEC_Results" / "testdata_NCEP-R2_choose") == ["log.testdata_NCEP-R2"]
