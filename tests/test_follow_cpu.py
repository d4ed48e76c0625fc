"""-c/--choose without a display, the parts that need no GPU: lec_follow's argument validation (before any HIP call), the host's
admissible centres / window sizes, the track file round trip, the command line's refusals, and the NumPy restatement of the
rule (tests/follow_restatement.py) on the golden sample."""
import ctypes
import os
import types

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib, dataset as ds, follow as fw
from tests import follow_restatement as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TESTDATA = os.path.join(GOLDEN, "testdata_NCEP-R2.nc")
NAMELIST = os.path.join(GOLDEN, "inputs", "namelist_NCEP-R2")


def _valid_args():
    """Every pointer set (to an address nothing dereferences: validation comes before any HIP call), every scalar in range."""
    a = _lib.FollowArgs()
    for f in ("u_d", "v_d", "hgt_d", "xcoef_d", "ycoef_d", "curv_d", "pos_d", "val_d", "status_d"):
        setattr(a, f, 4096)
    a.nt, a.ny, a.nx = 4, 33, 41
    a.field, a.sense, a.smooth_r, a.sj, a.si = _lib.FOLLOW_ZETA, _lib.FOLLOW_MIN, 0, 2, 2
    a.jlo, a.jhi, a.ilo, a.ihi, a.j_start, a.i_start = 3, 29, 3, 37, -1, -1
    return a


@pytest.mark.parametrize("change, code, word", [
    ({"u_d": None}, 1, b"u_d"), ({"v_d": None}, 1, b"v_d"), ({"xcoef_d": None}, 1, b"xcoef_d"), ({"curv_d": None}, 1, b"curv_d"),
    ({"pos_d": None}, 1, b"pos_d"), ({"val_d": None}, 1, b"val_d"), ({"status_d": None}, 1, b"status_d"),
    ({"nt": 0}, 1, b"nt"), ({"ny": 2}, 1, b"3 x 3"), ({"nx": 2}, 1, b"3 x 3"),
    ({"field": 2}, 1, b"field"), ({"sense": -1}, 1, b"sense"),
    ({"jlo": 30}, 1, b"jlo"), ({"jhi": 33}, 1, b"jhi"), ({"jlo": -1}, 1, b"jlo"), ({"ilo": 38}, 1, b"ilo"), ({"ihi": 41}, 1, b"ihi"),
    ({"j_start": 2, "i_start": 10}, 1, b"j_start"), ({"j_start": 10, "i_start": 38}, 1, b"i_start"), ({"j_start": 10}, 1, b"i_start"),
    ({"smooth_r": -1}, 1, b"smooth_r"), ({"sj": 0}, 1, b"sj"), ({"si": -3}, 1, b"si"),
    ({"field": _lib.FOLLOW_HGT, "hgt_d": None}, 1, b"hgt_d"),
    # 2 * 70 + 1 + 2 * 2 = 145 rows and columns: 145 * 145 * 8 = 168200 bytes, over the 160 KiB a workgroup may declare
    ({"ny": 400, "nx": 400, "jhi": 300, "ihi": 300, "sj": 70, "si": 70, "smooth_r": 2}, 2, b"145 x 145"),
])
def test_lec_follow_refuses_bad_arguments_without_a_gpu(change, code, word):
    lib = _lib.load()
    a = _valid_args()
    for k, v in change.items():
        setattr(a, k, v)
    assert lib.lec_follow(ctypes.byref(a)) == code
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_follow") and word in msg, msg
    if code == 2:
        assert b"168200" in msg and b"163776" in msg          # the tile's size and the limit (160 KiB less the 64 bytes of partials)


def test_lec_follow_null_and_struct_layout():
    lib = _lib.load()
    assert lib.lec_follow(None) == 1 and b"null" in lib.lec_last_error()
    assert lib.lec_follow(ctypes.byref(_lib.FollowArgs())) == 1 and b"null pointer" in lib.lec_last_error()
    # 3 pointers + 4 int32 + 3 pointers + 10 int32 + 4 pointers; an additive call: the ABI version and every other struct stay
    assert ctypes.sizeof(_lib.FollowArgs) == 3 * 8 + 4 * 4 + 3 * 8 + 10 * 4 + 4 * 8
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11
    with pytest.raises(ValueError, match="smooth_r"):
        a = _valid_args()
        a.smooth_r = -2
        _lib.check(lib.lec_follow(ctypes.byref(a)), "lec_follow")


def test_a_search_radius_beyond_the_slice_needs_only_the_slice():
    """The tile never outgrows the slice, so a huge radius on a small grid passes validation up to the launch -- checked through the
    limit's message on a grid just too large."""
    lib = _lib.load()
    a = _valid_args()
    a.ny, a.nx, a.jhi, a.ihi, a.sj, a.si = 150, 140, 100, 100, 1 << 30, 1 << 30
    assert lib.lec_follow(ctypes.byref(a)) == 2 and b"150 x 140" in lib.lec_last_error()


def test_admissible_centres_and_window_sizes():
    lat, lon = np.arange(-80.0, 0.1, 2.5), np.arange(-100.0, 0.1, 2.5)
    assert fw.admissible(lat, lon, 15, 15) == (3, 29, 3, 37) == fr.admissible(lat, lon, 15, 15)
    assert fw.admissible(lat, lon, 10, 20) == (2, 30, 4, 36)
    assert fw.admissible(lat, lon, 80, 100) == (16, 16, 20, 20)            # the one centre of a box as large as the domain
    assert fw.window_steps(lat, lon, 5) == (2, 2) == fr.window_steps(lat, lon, 5)
    assert fw.window_steps(lat, lon, 1) == (1, 1) and fw.window_steps(lat, lon, 7.4) == (2, 2) and fw.window_steps(lat, lon, 7.5) == (3, 3)
    # stretched axes: the bounds are inclusive index ranges of the points whose box fits, whatever the spacing
    slat = np.array([-60.0, -58.0, -55.0, -51.0, -46.0, -40.0, -33.0, -25.0, -16.0, -6.0])
    slon = np.sort(np.linspace(-80, -20, 31) + 0.4 * np.sin(np.arange(31)))
    jlo, jhi, ilo, ihi = fw.admissible(slat, slon, 10, 12)
    assert (jlo, jhi) == (2, 8)                                           # -55 - 5 >= -60 (not -58 - 5) ... -16 + 5 <= -6 (not -6 + 5)
    assert fw.admissible(slat, slon, 10, 12) == fr.admissible(slat, slon, 10, 12)
    for i in range(31):
        fits = slon[i] - 6 >= slon[0] and slon[i] + 6 <= slon[-1]
        assert fits == (ilo <= i <= ihi)
    assert fw.window_steps(slat, slon, 10)[0] == max(1, int(10 // np.median(np.diff(slat))))
    for length, width in ((81, 15), (15, 100.5)):
        with pytest.raises(ValueError, match=r"81|100\.5") as e:
            fw.admissible(lat, lon, length, width)
        assert "80.0 x 100.0" in str(e.value)                             # both sizes are named
    assert fw.start_index(lat, lon, (-22.5, -45), (3, 29, 3, 37)) == (23, 22)
    assert fw.start_index(lat, lon, (-79, 10), (3, 29, 3, 37)) == (3, 37)  # clamped into the admissible centres
    assert fw.sense_of("zeta", None, lat) == ("south", _lib.FOLLOW_MIN) and fw.sense_of("zeta", None, -lat[::-1] + 5) == ("north", _lib.FOLLOW_MAX)
    assert fw.sense_of("hgt", "north", lat) == ("north", _lib.FOLLOW_MIN) and fw.sense_of("zeta", "north", lat)[1] == _lib.FOLLOW_MAX
    with pytest.raises(ValueError):
        fw.sense_of("wind", None, lat)


def test_follow_system_refuses_a_box_larger_than_the_domain_before_any_gpu_work():
    lat, lon = np.arange(-40.0, -19.9, 2.5), np.arange(-60.0, -39.9, 2.5)
    z = np.zeros((2, lat.size, lon.size))
    with pytest.raises(ValueError, match="does not fit"):
        fw.follow_system(z, z, z, lat, lon, length=25, width=15)


def test_written_track_reads_back_identical_doubles(tmp_path):
    """Every coordinate of a grid in binary fractions of a degree -- all the shipped samples, NCEP, ERA5 -- and the box sizes come
    back from dataset.read_track as the identical doubles."""
    grid = np.concatenate([-90 + s * np.arange(int(180 / s) + 1) for s in (2.5, 1.25, 1.0, 0.5, 0.25, 0.125, 0.28125)])
    grid = np.concatenate([grid, 2 * grid, np.linspace(-90, 90, 721).astype(np.float32).astype(np.float64)])
    time = np.datetime64("2005-08-08T00:00") + np.arange(grid.size) * np.timedelta64(6, "h")
    path = fw.write_track(tmp_path / "t", time, grid, grid[::-1], 15.0, np.resize([12.5, 15.0, 7.25], grid.size))
    lines = open(path).read().splitlines()
    assert lines[0] == "time;Lat;Lon;length;width" and lines[1] == "2005-08-08-0000;-90.0;90.0;15.0;12.5" and lines[2].startswith("2005-08-08-0600;-87.5;")
    track = ds.read_track(path)
    assert np.array_equal(track["Lat"].values, grid) and np.array_equal(track["Lon"].values, grid[::-1])
    assert (track["length"].values == 15.0).all() and np.array_equal(track["width"].values, np.resize([12.5, 15.0, 7.25], grid.size))
    assert np.array_equal(track.index.values, time.astype("datetime64[ns]"))
    with pytest.raises(ValueError):
        fw.write_track(tmp_path / "bad", time[:2], [np.nan, 1.0], [0.0, 0.0], 15, 15)


def test_written_track_of_a_stretched_axis_comes_back_within_the_reader_s_precision(tmp_path):
    """Doubles of full length (a stretched axis).  The reader's parser is the reference's (pandas' default): it keeps 17 decimal
    digits counted from the first one written and scales by repeated multiplication, so of 120,000 random coordinates it read 13 %
    beside their shortest round-trip form and could not produce 8 % from ANY decimal form tried (17-19 digits of the double and of
    its four neighbours either side): identity is not the writer's to give there.  What holds: the numbers are written in the
    form a correct parser reads back exactly (checked with Python's float), and the reference's parser stays within 1e-12 degrees
    (17 digits of a number below 1000 keep 14 decimals; each of its <= 5 scaling steps rounds by <= 4e-14 at 360)."""
    rng = np.random.default_rng(11)
    lat_c = np.r_[0.1, 1 / 3, -1e-7, rng.uniform(-90, 90, 500)]
    lon_c = np.r_[179.99999999999997, -2 / 3, 123.456, rng.uniform(-180, 180, 500)]
    time = np.datetime64("2005-08-08T00:00") + np.arange(lat_c.size) * np.timedelta64(6, "h")
    path = fw.write_track(tmp_path / "t", time, lat_c, lon_c, 15.0, 15.0)
    rows = [ln.split(";") for ln in open(path).read().splitlines()[1:]]
    assert np.array_equal([float(r[1]) for r in rows], lat_c) and np.array_equal([float(r[2]) for r in rows], lon_c)
    track = ds.read_track(path)
    worst = max(np.max(np.abs(track["Lat"].values - lat_c)), np.max(np.abs(track["Lon"].values - lon_c)))
    print("worst read-back difference: %.2e degrees" % worst)
    assert worst <= 1e-12


def test_written_track_is_accepted_by_the_track_path(tmp_path):
    """The written file is a track like any other: the time selection and the crop of -t take it."""
    a = types.SimpleNamespace(infile=TESTDATA, mpas=False, choose_domain=None)
    u, v, h, lat, lon, time = fw.search_domain_slices(a, NAMELIST)
    assert u.shape == (5, 33, 41) and lat[0] == -80 and lon[-1] == 0 and u.dtype == np.float64 and 1000 < np.nanmean(h) < 2000     # gpm
    path = fw.write_track(tmp_path / "t", time, [-17.5, -22.5, -27.5, -27.5, -27.5], [-47.5, -52.5, -55, -55, -55], 15, 15)
    track = ds.read_track(path)
    assert list(ds.select_track_times(time, track)) == [0, 1, 2, 3, 4]
    js, is_ = ds.domain_slices(lat, lon, types.SimpleNamespace(fixed=False, track=True, trackfile=path))
    chosen = ds.domain_slices(lat, lon, types.SimpleNamespace(fixed=False, track=False, choose=True, choose_track=path, trackfile="nowhere"))
    assert (js, is_) == chosen                                       # the choose branch IS the track branch on the written track
    assert lat[js][0] == -37.5 and lat[js][-1] == -7.5 and lon[is_][0] == -65 and lon[is_][-1] == -37.5
    with pytest.raises(ValueError, match="choose_track"):
        ds.domain_slices(lat, lon, types.SimpleNamespace(fixed=False, track=False, choose=True))


def test_search_domain_file_and_missing_level(tmp_path):
    (tmp_path / "dom").write_text("min_lon;-70\nmax_lon;-30\nmin_lat;-50\nmax_lat;-10\n")
    a = types.SimpleNamespace(infile=TESTDATA, mpas=False, choose_domain=str(tmp_path / "dom"))
    u, v, h, lat, lon, time = fw.search_domain_slices(a, NAMELIST)
    full = fw.search_domain_slices(types.SimpleNamespace(infile=TESTDATA, mpas=False, choose_domain=None), NAMELIST)
    assert (lat[0], lat[-1], lon[0], lon[-1]) == (-50, -10, -70, -30)
    j0, i0 = int(np.searchsorted(full[3], -50)), int(np.searchsorted(full[4], -70))
    assert np.array_equal(u, full[0][:, j0: j0 + lat.size, i0: i0 + lon.size]) and np.array_equal(h, full[2][:, j0: j0 + lat.size, i0: i0 + lon.size])
    (tmp_path / "tiny").write_text("min_lon;-70\nmax_lon;-66\nmin_lat;-50\nmax_lat;-10\n")
    a.choose_domain = str(tmp_path / "tiny")
    with pytest.raises(ValueError, match="3 x 3"):
        fw.search_domain_slices(a, NAMELIST)


@pytest.mark.parametrize("argv, word", [
    (["-r", "-t", "--choose-start", "-22.5", "-45"], "--choose-start goes with -c"),
    (["-r", "-f", "--choose-box", "10", "10", "--choose-field", "hgt"], "--choose-box, --choose-field go with -c"),
    (["-r", "-f", "--choose-search", "3"], "--choose-search"), (["-r", "-t", "--choose-smooth", "1"], "--choose-smooth"),
    (["-r", "-t", "--choose-hemisphere", "north"], "--choose-hemisphere"), (["-r", "-f", "--choose-domain", "inputs/box_limits"], "--choose-domain"),
    (["-r", "-c", "--gpus", "2"], "-t --trackfile LEC_Results/testdata_NCEP-R2_choose/testdata_NCEP-R2_choose_track --gpus N"),
    (["-r", "-c", "--choose-search", "0"], "--choose-search"), (["-r", "-c", "--choose-smooth", "-1"], "--choose-smooth"),
    (["-r", "-c", "--trackfiles", "a", "b"], "--trackfiles goes with -t"),
])
def test_command_line_refusals_leave_nothing_behind(tmp_path, monkeypatch, argv, word):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main([TESTDATA] + argv)
    assert word in str(e.value)
    assert os.listdir(tmp_path) == []                                 # no LEC_Results


def test_choose_under_a_launcher_with_several_ranks_is_refused(tmp_path, monkeypatch):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="run -c once"):
        lorenzcycletoolkit.main([TESTDATA, "-r", "-c"])
    assert os.listdir(tmp_path) == []


# the centres (Lat, Lon) the rule gives on the golden sample: search domain = the whole file, box 15 x 15, search 5 degrees, metpy_no_crs
GOLDEN_CENTRES = {
    None: [(-50, -7.5), (-47.5, -7.5), (-45, -7.5), (-42.5, -7.5), (-40, -7.5)],           # -7.5: the eastern bound of the admissible centres
    (-22.5, -45): [(-17.5, -47.5), (-22.5, -52.5), (-27.5, -55), (-27.5, -55), (-27.5, -55)],
    (-30, -60): [(-25, -57.5), (-25, -55), (-27.5, -55), (-27.5, -55), (-27.5, -55)],
}


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("start", list(GOLDEN_CENTRES))
def test_restatement_on_the_golden_sample(start, r):
    a = types.SimpleNamespace(infile=TESTDATA, mpas=False, choose_domain=None)
    u, v, h, lat, lon, time = fw.search_domain_slices(a, NAMELIST)
    out = fr.follow(u, v, h, lat, lon, length=15, width=15, search=5, smooth=r, start=start, formulation="metpy_no_crs")
    assert [(lat[j], lon[i]) for j, i in out["pos"]] == GOLDEN_CENTRES[start]
    assert not out["status"].any() and out["margin"].min() > 1e-3        # far from a tie: the positions are meaningful
    if start is None:
        assert out["windows"][0] == (3, 29, 3, 37) and all(p[1] == 37 for p in out["pos"])      # the clamp at the bound is exercised
