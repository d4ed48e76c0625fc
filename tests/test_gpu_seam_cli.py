"""The +-180 meridian on the command line: ``-t`` with a track that crosses it (the longitude axis of such a run is cut at Greenwich
instead, dataset.track_lon_origin), ``-c --choose-periodic`` writing such a track, and ``--choose-systems`` with one system on the seam
and one mid-domain (two partitions of the batch).  The file is a small classic NetCDF ring the test writes itself: 5 levels x 33 x 72,
6 steps, a vortex that crosses the seam and a weaker one at Greenwich.  Numbers: the oracle's moving framework on the same data on a
continuous 0 .. 360 axis, held to the bar tests/test_gpu_parity.py holds fp64 moving-box parity to."""
import os
import shutil

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd.constants import LEVEL_TERMS
from oracle import lec_oracle as o
from tests.helpers import compare
from tests.test_gpu_parity import TOL

STEM = "ring"
NT = 6
LAT = -80.0 + 2.5 * np.arange(33)
LON = -180.0 + 5.0 * np.arange(72)
LEV_HPA = np.array([1000, 925, 850, 700, 500], dtype=np.int32)
BOX = 20.0
TIME_0 = np.datetime64("2005-04-05T00", "ns")
HOURS_0 = float((TIME_0 - np.datetime64("1800-01-01T00", "ns")) / np.timedelta64(1, "h"))
# the hand-written track: 5 degrees east per step through the meridian, every longitude inside [-180, 180)
TRACK_LON = [170.0, 175.0, -180.0, -175.0, -170.0, -165.0]
TRACK_LAT = [-40.0, -40.0, -42.5, -42.5, -45.0, -45.0]


def fields():
    """[nt][nl][ny][nx] T, U, V, W (omega), Z (height, gpm): a smooth background, noise, and two cyclonic vortices with their lows -- one
    moving east along the track above, twice as strong as the other, which moves east from Greenwich."""
    rng = np.random.default_rng(4)
    nl, ny, nx = LEV_HPA.size, LAT.size, LON.size
    p = (LEV_HPA[None, :, None, None] * 100.0) / 1e5
    tt = np.arange(NT)[:, None, None, None]
    y, x = LAT[None, None, :, None], LON[None, None, None, :]
    lam, phi = np.deg2rad(x), np.deg2rad(y)
    shape = (NT, nl, ny, nx)
    u = 12.0 * np.cos(phi) * (1.3 - p) + 0.3 * rng.standard_normal(shape)
    v = 2.0 * np.sin(2 * lam) * np.cos(phi) + 0.3 * rng.standard_normal(shape)
    z = 7000.0 * np.log(1.0 / p) + 30.0 * np.cos(2 * phi) + 2.0 * rng.standard_normal(shape)
    for x0, y0, amp in ((170.0 + 5.0 * tt, -40.0 - 1.0 * tt, 2.0), (0.0 + 5.0 * tt, -45.0 + 0.0 * tt, 1.0)):
        dy, dx = y - y0, (x - x0 + 180.0) % 360.0 - 180.0
        g = np.exp(-(dx * dx + dy * dy) / (2 * 7.0 * 7.0)) * p
        u, v, z = u + 3.0 * amp * dy * g, v - 3.0 * amp * dx * g, z - 60.0 * amp * g
    t = 288.0 * p ** 0.19 + 8.0 * np.cos(2 * phi) * p + 2.0 * np.sin(3 * lam + 0.1 * tt) + 0.3 * rng.standard_normal(shape)
    w = 0.1 * rng.standard_normal(shape)
    return t, u, v, w, z


def write_ring(path):
    from scipy.io import netcdf_file
    t, u, v, w, z = fields()
    f = netcdf_file(path, "w", version=2)
    for n, s in (("initial_time0_hours", NT), ("lv_ISBL3", LEV_HPA.size), ("lat_2", LAT.size), ("lon_2", LON.size)):
        f.createDimension(n, s)
    tv = f.createVariable("initial_time0_hours", "d", ("initial_time0_hours",)); tv[:] = HOURS_0 + 6.0 * np.arange(NT)
    tv.units = "hours since 1800-01-01 00:00"
    lv = f.createVariable("lv_ISBL3", "i", ("lv_ISBL3",)); lv[:] = LEV_HPA; lv.units = "hPa"
    la = f.createVariable("lat_2", "d", ("lat_2",)); la[:] = LAT
    lo = f.createVariable("lon_2", "d", ("lon_2",)); lo[:] = LON
    for name, a in (("TMP_2_ISBL", t), ("U_GRD_2_ISBL", u), ("V_GRD_2_ISBL", v), ("V_VEL_2_ISBL", w), ("HGT_2_ISBL", z)):
        var = f.createVariable(name, "d", ("initial_time0_hours", "lv_ISBL3", "lat_2", "lon_2"))
        var[:] = a
    f.close()


def oracle_domain():
    """The same data as the oracle takes a data set -- levels ascending in Pa, latitudes S -> N -- on a continuous 0 .. 360 axis."""
    t, u, v, w, z = fields()
    io, ik = np.argsort(LON % 360.0, kind="stable"), np.argsort(LEV_HPA, kind="stable")
    cut = lambda a: np.ascontiguousarray(a[:, ik][..., io])
    return o.Domain(cut(t), cut(u), cut(v), cut(w), cut(z) * o.G, LAT, (LON % 360.0)[io], LEV_HPA[ik] * 100.0, 6.0 * 3600.0 * np.arange(NT))


@pytest.fixture
def workdir(tmp_path, golden_dir, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_NCEP-R2"), tmp_path / "inputs" / "namelist")
    write_ring(str(tmp_path / f"{STEM}.nc"))
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return tmp_path


def _main(argv):
    import lorenzcycletoolkit
    lorenzcycletoolkit.main(argv)


def _tree(directory, method):
    """name (with the method's word taken out) -> bytes, for the results CSV, the 21 level tables and the trackfile."""
    files = {"results": directory / f"{STEM}_{method}_results.csv", "trackfile": directory / f"{STEM}_{method}_trackfile"}
    lv = directory / "results_vertical_levels"
    assert sorted(os.listdir(lv)) == sorted(f"{t}_lv_ISBL3.csv" for t in LEVEL_TERMS)
    files.update({name: lv / name for name in os.listdir(lv)})
    return {k: p.read_bytes() for k, p in files.items()}


def _same(a, b):
    assert a.keys() == b.keys() and len(a) == 23
    for name in a:
        assert a[name] == b[name], name


def _inside(trackfile):
    """Every longitude of a written trackfile lies inside [-180, 180)."""
    trk = pd.read_csv(trackfile, sep=";")
    cols = [c for c in trk.columns if c in ("Lon", "min_lon", "max_lon") or c.endswith("_lon")]
    assert len(cols) == 6
    for c in cols:
        assert ((trk[c] >= -180.0) & (trk[c] < 180.0)).all(), (c, trk[c].tolist())
    return trk


def _against_the_oracle(directory, method, track_lat, track_lon, width, length):
    dom = oracle_domain()
    lon360 = np.asarray(track_lon) % 360.0
    domt = o.crop_domain_track(dom, np.asarray(track_lat), lon360, max_width=width, max_length=length)
    boxes = [(lo - width / 2, lo + width / 2, la - length / 2, la + length / 2) for la, lo in zip(track_lat, lon360)]
    ref_s, ref_l = o.lec_moving(domt, boxes)
    got = pd.read_csv(directory / f"{STEM}_{method}_results.csv", index_col=0)
    assert len(got) == len(track_lat)
    levels = {}
    for name in LEVEL_TERMS:
        tab = pd.read_csv(directory / "results_vertical_levels" / f"{name}_lv_ISBL3.csv", index_col=0)
        tab = tab.rename(columns=float)[list(dom.level)]
        levels[name] = tab.values if len(tab) == len(track_lat) else tab.loc[name].values[None].repeat(len(track_lat), axis=0)
    worst = compare({c: got[c].values for c in got.columns}, levels, ref_s, ref_l, TOL, f"{method} across the seam", time_s=dom.time_s[:len(track_lat)])
    print(max(worst.values()))


def test_a_track_across_the_seam(workdir):
    """-r -t with the hand-written crossing track: all 16 terms, the budgets and the level tables against the oracle; the trackfile's
    longitudes inside [-180, 180); --device-ingest byte-identical."""
    from lorenzcycletoolkit_amd.follow import write_track
    time = TIME_0 + np.arange(NT) * np.timedelta64(6, "h")
    write_track(workdir / "inputs" / "track", time, TRACK_LAT, TRACK_LON, BOX, BOX)
    _main([f"{STEM}.nc", "-r", "-t"])
    out = workdir / "LEC_Results" / f"{STEM}_track"
    log = (out / f"log.{STEM}").read_text()
    assert "0..360" in log and "differ by more than 180 degrees" in log
    trk = _inside(out / f"{STEM}_track_trackfile")
    assert trk["Lon"].tolist() == TRACK_LON and trk["min_lon"].tolist() == [160.0, 165.0, 170.0, 175.0, -180.0, -175.0]
    assert trk["max_lon"].tolist() == [-180.0, -175.0, -170.0, -165.0, -160.0, -155.0]
    assert np.all(np.abs((trk["min_max_zeta_850_lon"].values - np.array(TRACK_LON) + 180.0) % 360.0 - 180.0) <= 5.0)    # the vortex, in its box
    assert (trk["min_max_zeta_850"] < 0).all()
    _against_the_oracle(out, "track", TRACK_LAT, TRACK_LON, BOX, BOX)
    host = _tree(out, "track")
    shutil.rmtree(workdir / "LEC_Results")
    _main([f"{STEM}.nc", "-r", "-t", "--device-ingest"])
    assert "0..360" in (out / f"log.{STEM}").read_text()
    _same(_tree(out, "track"), host)


def test_choose_periodic_follows_the_system_across_the_seam(workdir):
    """-c --choose-periodic --choose-start: the written track crosses the seam, and its analysis IS -t on that track, file for file."""
    common = ["--choose-box", str(BOX), str(BOX), "--choose-search", "10"]
    _main([f"{STEM}.nc", "-r", "-c", "--choose-periodic", "--choose-start", "-40", "170"] + common)
    chosen = workdir / "LEC_Results" / f"{STEM}_choose"
    assert "lec_follow_spans_chunk_ring" in (chosen / f"log.{STEM}").read_text()
    tr = pd.read_csv(chosen / f"{STEM}_choose_track", sep=";")
    assert ((tr.Lon >= -180.0) & (tr.Lon < 180.0)).all() and tr.Lon.iloc[0] >= 165.0 and tr.Lon.iloc[-1] <= -160.0      # across the meridian
    assert np.all(np.abs((tr.Lon.values - (170.0 + 5.0 * np.arange(NT)) + 180.0) % 360.0 - 180.0) <= 5.0)               # on the planted path
    _inside(chosen / f"{STEM}_choose_trackfile")
    _main([f"{STEM}.nc", "-r", "-t", "--trackfile", str(chosen / f"{STEM}_choose_track")])
    _same(_tree(chosen, "choose"), _tree(workdir / "LEC_Results" / f"{STEM}_track", "track"))
    _against_the_oracle(chosen, "choose", tr.Lat.values, tr.Lon.values, BOX, BOX)
    # without --choose-start the ring run starts from seed 0 of step 0: the stronger vortex, the same track
    first = (chosen / f"{STEM}_choose_track").read_bytes()
    _main([f"{STEM}.nc", "-r", "-c", "--choose-periodic"] + common)
    assert (chosen / f"{STEM}_choose_track").read_bytes() == first and "seed 0" in (chosen / f"log.{STEM}").read_text()
    # without the flag the run is what it was: the search stops at the seam (no admissible centre east of 165 E for this box)
    _main([f"{STEM}.nc", "-r", "-c", "--choose-start", "-40", "170"] + common)
    stuck = pd.read_csv(chosen / f"{STEM}_choose_track", sep=";")
    assert (stuck.Lon > 0).all() and stuck.Lon.max() <= 165.0 and "lec_follow_spans_chunk_ring" not in (chosen / f"log.{STEM}").read_text()


def test_two_systems_two_partitions(workdir):
    """-c --choose-periodic --choose-systems 2: the system on the seam and the one at Greenwich take different longitude axes, so the batch
    runs as two partitions -- each tree byte for byte its own -t --trackfile run, batch.csv in the given order."""
    _main([f"{STEM}.nc", "-r", "-c", "--choose-periodic", "--choose-systems", "2", "--choose-box", str(BOX), str(BOX), "--choose-search", "10"])
    batch_dir = workdir / "LEC_Results" / f"{STEM}_choose_batch"
    log = (batch_dir / f"log.{STEM}").read_text()
    assert "2 pass(es) over the data" in log and "lec_follow_seeds_series_ring" in log
    table = pd.read_csv(batch_dir / "batch.csv")
    assert [os.path.basename(p) for p in table.trackfile] == ["choose_s01", "choose_s02"] and table.steps.tolist() == [NT, NT]
    s1, s2 = (pd.read_csv(batch_dir / n, sep=";") for n in ("choose_s01", "choose_s02"))
    assert s1.Lon.iloc[0] >= 165.0 and s1.Lon.iloc[-1] <= -160.0 and (np.abs(s2.Lon - 12.5) <= 17.5).all()           # the stronger one is on the seam
    trees = {n: _tree(workdir / "LEC_Results" / f"{STEM}_{n}_track", "track") for n in ("choose_s01", "choose_s02")}
    _inside(workdir / "LEC_Results" / f"{STEM}_choose_s01_track" / f"{STEM}_track_trackfile")
    for n in ("choose_s01", "choose_s02"):
        _main([f"{STEM}.nc", "-r", "-t", "--trackfile", str(batch_dir / n)])
        _same(_tree(workdir / "LEC_Results" / f"{STEM}_track", "track"), trees[n])
