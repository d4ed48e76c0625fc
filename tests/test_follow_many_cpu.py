"""-c --choose-systems, the parts that need no GPU: the two new calls' argument validation (before any HIP call), the struct
layouts, the host's separation steps and starts file, the command line's refusals, and the NumPy restatement of the rule
(tests/follow_many_restatement.py) on a slice small enough to work out by hand."""
import ctypes
import os

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib, follow as fw
from tests import follow_many_restatement as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTDATA = os.path.join(ROOT, "tests", "golden", "testdata_NCEP-R2.nc")

SEEDS_POINTERS = ("u_d", "v_d", "hgt_d", "xcoef_d", "ycoef_d", "curv_d", "work_d", "seed_pos_d", "seed_val_d", "n_found_d")
MANY_POINTERS = ("u_d", "v_d", "hgt_d", "xcoef_d", "ycoef_d", "curv_d", "start_d", "pos_d", "val_d", "status_d")


def _seeds_args():
    """Every pointer set (to an address nothing dereferences: validation comes before any HIP call), every scalar in range."""
    a = _lib.FollowSeedsArgs()
    for f in SEEDS_POINTERS:
        setattr(a, f, 4096)
    a.ny, a.nx, a.field, a.sense, a.smooth_r = 33, 41, _lib.FOLLOW_ZETA, _lib.FOLLOW_MIN, 0
    a.ej, a.ei, a.k_max, a.threshold = 3, 3, 8, float("nan")
    a.jlo, a.jhi, a.ilo, a.ihi = 3, 29, 3, 37
    return a


def _many_args():
    a = _lib.FollowManyArgs()
    for f in MANY_POINTERS:
        setattr(a, f, 4096)
    a.nt, a.ny, a.nx = 4, 33, 41
    a.field, a.sense, a.smooth_r, a.sj, a.si = _lib.FOLLOW_ZETA, _lib.FOLLOW_MIN, 0, 2, 2
    a.jlo, a.jhi, a.ilo, a.ihi, a.n_chains = 3, 29, 3, 37, 5
    return a


BAD_SLICE = [({"ny": 2}, b"3 x 3"), ({"nx": 2}, b"3 x 3"), ({"field": 2}, b"field"), ({"sense": -1}, b"sense"), ({"smooth_r": -1}, b"smooth_r"),
             ({"jlo": 30}, b"jlo"), ({"jhi": 33}, b"jhi"), ({"jlo": -1}, b"jlo"), ({"ilo": 38}, b"ilo"), ({"ihi": 41}, b"ihi"),
             ({"field": _lib.FOLLOW_HGT, "hgt_d": None}, b"hgt_d")]


def _refused(call, a, change, code, word, who):
    lib = _lib.load()
    for k, v in change.items():
        setattr(a, k, v)
    assert getattr(lib, call)(ctypes.byref(a)) == code
    msg = lib.lec_last_error()
    assert msg.startswith(who + b":") and word in msg, msg
    return msg


@pytest.mark.parametrize("change, word", [({p: None}, p.encode()) for p in SEEDS_POINTERS if p != "hgt_d"] + BAD_SLICE + [
    ({"k_max": 0}, b"k_max"), ({"k_max": 257}, b"k_max"), ({"ej": 0}, b"ej"), ({"ei": 0}, b"ei"), ({"ei": -2}, b"ei")])
def test_lec_follow_seeds_refuses_bad_arguments_without_a_gpu(change, word):
    _refused("lec_follow_seeds", _seeds_args(), change, 1, word, b"lec_follow_seeds")


@pytest.mark.parametrize("change, word", [({p: None}, p.encode()) for p in MANY_POINTERS if p != "hgt_d"] + BAD_SLICE + [
    ({"nt": 0}, b"nt"), ({"n_chains": 0}, b"n_chains"), ({"n_chains": -4}, b"n_chains"), ({"sj": 0}, b"sj"), ({"si": -3}, b"si")])
def test_lec_follow_many_refuses_bad_arguments_without_a_gpu(change, word):
    _refused("lec_follow_many", _many_args(), change, 1, word, b"lec_follow_many")


def test_lec_follow_many_refuses_the_over_limit_tile_with_both_figures():
    # 2 * 70 + 1 + 2 * 2 = 145 rows and columns: 145 * 145 * 8 = 168200 bytes, over the 160 KiB (less 64 bytes of partials) of one workgroup
    change = {"ny": 400, "nx": 400, "jhi": 300, "ihi": 300, "sj": 70, "si": 70, "smooth_r": 2}
    msg = _refused("lec_follow_many", _many_args(), change, 2, b"145 x 145", b"lec_follow_many")
    assert b"168200" in msg and b"163776" in msg


def test_exports_null_structs_and_layouts():
    lib = _lib.load()
    assert "lec_follow_seeds" in _lib.EXPORTS and "lec_follow_many" in _lib.EXPORTS
    assert lib.lec_follow_seeds and lib.lec_follow_many
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11                  # additive calls
    assert _lib.FOLLOW_BAD_START == 2
    for call, empty in (("lec_follow_seeds", _lib.FollowSeedsArgs()), ("lec_follow_many", _lib.FollowManyArgs())):
        assert getattr(lib, call)(None) == 1 and b"null args" in lib.lec_last_error() and lib.lec_last_error().startswith(call.encode())
        assert getattr(lib, call)(ctypes.byref(empty)) == 1 and b"null pointer argument u_d" in lib.lec_last_error()
    # the header: 3 pointers + 4 int32 + 3 pointers + 8 int32 + 1 double + 5 pointers
    assert ctypes.sizeof(_lib.FollowSeedsArgs) == 3 * 8 + 4 * 4 + 3 * 8 + 8 * 4 + 8 + 5 * 8 == 144
    assert _lib.FollowSeedsArgs.threshold.offset == 96 and _lib.FollowSeedsArgs.work_d.offset == 104
    # 3 pointers + 4 int32 + 3 pointers + 10 int32 + 5 pointers: lec_follow_args with the start pair replaced and start_d put in
    assert ctypes.sizeof(_lib.FollowManyArgs) == 3 * 8 + 4 * 4 + 3 * 8 + 10 * 4 + 5 * 8 == 144
    assert _lib.FollowManyArgs.n_chains.offset == _lib.FollowArgs.j_start.offset and _lib.FollowManyArgs.start_d.offset == 104
    with pytest.raises(ValueError, match="k_max"):
        a = _seeds_args()
        a.k_max = 1000
        _lib.check(lib.lec_follow_seeds(ctypes.byref(a)), "lec_follow_seeds")


def test_separation_steps_on_even_and_stretched_axes():
    lat, lon = np.arange(-80.0, 0.1, 2.5), np.arange(-100.0, 0.1, 1.25)
    assert fw.separation_steps(lat, lon, 7.5, 7.5) == (3, 6) == fm.separation_steps(lat, lon, 7.5, 7.5)
    assert fw.separation_steps(lat, lon, 7.4, 1.0) == (2, 1)                       # floor, and never less than one grid step
    assert fw.separation_steps(lat, lon, 5, 10) == (fw.window_steps(lat, lon, 5)[0], fw.window_steps(lat, lon, 10)[1])
    slat = np.array([-60.0, -58.0, -55.0, -51.0, -46.0, -40.0, -33.0, -25.0, -16.0, -6.0])       # spacings 2 .. 10, median 6
    slon = np.sort(np.linspace(-80, -20, 31) + 0.4 * np.sin(np.arange(31)))
    ej, ei = fw.separation_steps(slat, slon, 13, 5)
    assert ej == 2 and ei == max(1, int(5 // np.median(np.diff(slon)))) and (ej, ei) == fm.separation_steps(slat, slon, 13, 5)


def test_read_starts_round_trips_write_track_s_numbers(tmp_path):
    grid = np.concatenate([-90 + s * np.arange(int(180 / s) + 1) for s in (2.5, 1.0, 0.25, 0.28125)])
    time = np.datetime64("2005-08-08T00:00") + np.arange(grid.size) * np.timedelta64(6, "h")
    path = fw.write_track(tmp_path / "t", time, grid, 2 * grid[::-1], 15.0, 15.0)
    got = fw.read_starts(path)                                                     # a track is a starts file: the other columns are ignored
    assert got.shape == (grid.size, 2) and np.array_equal(got[:, 0], grid) and np.array_equal(got[:, 1], 2 * grid[::-1])
    (tmp_path / "s").write_text("Lat;Lon\n-50.0;-7.5\n-70;-60\n")
    assert fw.read_starts(tmp_path / "s").tolist() == [[-50.0, -7.5], [-70.0, -60.0]]
    (tmp_path / "bad").write_text("lat;lon\n1;2\n")
    with pytest.raises(ValueError, match="Lat"):
        fw.read_starts(tmp_path / "bad")
    (tmp_path / "empty").write_text("Lat;Lon\n")
    with pytest.raises(ValueError, match="at least one"):
        fw.read_starts(tmp_path / "empty")
    with pytest.raises(FileNotFoundError):
        fw.read_starts(tmp_path / "nowhere")


def test_first_shared_centre():
    pos = np.array([[[1, 1], [2, 2], [3, 3]], [[5, 5], [2, 2], [3, 3]], [[7, 7], [8, 8], [3, 3]], [[9, 9], [9, 9], [9, 9]]])
    assert fw.first_shared_centre(pos) == [None, (0, 1), (0, 2), None]


@pytest.mark.parametrize("argv, word", [
    (["-r", "-t", "--choose-systems", "2"], "--choose-systems goes with -c"),
    (["-r", "-f", "--choose-starts", "x"], "--choose-starts goes with -c"),
    (["-r", "-f", "--choose-threshold", "-5e-5", "--choose-separation", "5", "5"], "--choose-threshold, --choose-separation go with -c"),
    (["-r", "-c", "--choose-systems", "2", "--choose-starts", "x"], "give one of the two"),
    (["-r", "-c", "--choose-systems", "2", "--choose-start", "-22.5", "-45"], "--choose-start is the one system"),
    (["-r", "-c", "--choose-starts", "x", "--choose-start", "-22.5", "-45"], "--choose-start is the one system"),
    (["-r", "-c", "--choose-threshold", "-5e-5"], "--choose-threshold goes with --choose-systems"),
    (["-r", "-c", "--choose-separation", "5", "5"], "--choose-separation goes with --choose-systems"),
    (["-r", "-c", "--choose-starts", TESTDATA, "--choose-threshold", "-5e-5"], "--choose-threshold goes with --choose-systems"),
    (["-r", "-c", "--choose-systems", "2", "--ingest", "device"], "--ingest device / --device-ingest is not supported for a batch of tracks"),
    (["-r", "-c", "--choose-starts", TESTDATA, "--device-ingest"], "--ingest device / --device-ingest is not supported for a batch of tracks"),
    (["-r", "-c", "--choose-systems", "2", "--gpus", "2"], "on one GPU"),
    (["-r", "-c", "--choose-starts", TESTDATA, "--gpus", "4"], "on one GPU"),
    (["-r", "-c", "--choose-systems", "0"], "--choose-systems must be 1..256"), (["-r", "-c", "--choose-systems", "257"], "--choose-systems must be 1..256"),
    (["-r", "-c", "--choose-systems", "2", "--choose-separation", "5", "0"], "--choose-separation"),
    (["-r", "-c", "--choose-starts", "no_such_file"], "--choose-starts: no_such_file not found"),
])
def test_command_line_refusals_leave_nothing_behind(tmp_path, monkeypatch, argv, word):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main([TESTDATA] + argv)
    assert word in str(e.value)
    assert os.listdir(tmp_path) == []                                 # no LEC_Results


def test_the_help_says_which_sign_the_threshold_takes():
    import lorenzcycletoolkit
    text = " ".join(lorenzcycletoolkit.create_arg_parser().format_help().split())
    assert "--choose-threshold" in text and "negative number" in text and "--choose-separation LAT_DEG LON_DEG" in text


def _hand_made():
    """7 x 9, height, the minimum, a 2 x 2 degree box on 1-degree axes (admissible centres 1..5 x 1..7), neighbourhood +-1:
        two lows (90 at (1, 1), 95 at (1, 5)), an equal pair (97 at (3, 3) and (3, 4)), a 2 x 2 plateau of 98 at rows 4-5, columns 6-7,
        and the deepest low of all, 80 at (0, 3), OUTSIDE the admissible centres, with its flank 96 at (1, 3) inside them.  Everything
        else is 100: a plateau of its own, none of whose admissible points is its row-major first."""
    h = np.full((7, 9), 100.0)
    h[1, 1], h[1, 5] = 90.0, 95.0
    h[3, 3] = h[3, 4] = 97.0
    h[4:6, 6:8] = 98.0
    h[0, 3], h[1, 3] = 80.0, 96.0
    return h, -30.0 + np.arange(7.0), -50.0 + np.arange(9.0)


def test_restatement_on_a_slice_worked_out_by_hand():
    h, lat, lon = _hand_made()
    kw = dict(length=2.0, width=2.0, separation=(1.0, 1.0), field="hgt")
    out = fm.find_systems(None, None, h, lat, lon, k=8, **kw)
    assert (out["ej"], out["ei"], out["bounds"]) == (1, 1, (1, 5, 1, 7))
    # the lows in order; the pair and the plateau give their first point each; the flank of the low outside gives nothing, nor does the 100s' plateau
    assert out["pos"].tolist() == [[1, 1], [1, 5], [3, 3], [4, 6]] and out["val"].tolist() == [90.0, 95.0, 97.0, 98.0] and out["n_found"] == 4
    assert np.allclose(out["neighbourhood"], [0.1, 0.05, 0.03, 0.02]) and np.allclose(out["rank"], [0.05, 0.02, 0.01])      # of max |F| = 100
    two = fm.find_systems(None, None, h, lat, lon, k=2, **kw)
    assert two["pos"].tolist() == [[1, 1], [1, 5]] and np.allclose(two["rank"], [0.05, 0.02])       # ... and the gap to the first one left out
    thr = fm.find_systems(None, None, h, lat, lon, k=8, threshold=96.5, **kw)
    assert thr["pos"].tolist() == [[1, 1], [1, 5]] and np.allclose(sorted(thr["threshold"]), [0.005, 0.015, 0.015, 0.065]) and np.isclose(thr["margin"], 0.005)
    assert fm.find_systems(None, None, h, lat, lon, k=8, threshold=97.0, **kw)["pos"].tolist() == [[1, 1], [1, 5], [3, 3]]     # "at least as good"
    # a wider neighbourhood: both lows now see the low outside the admissible centres, (0, 3), and the plateau sees the pair
    wide = fm.find_systems(None, None, h, lat, lon, k=8, **dict(kw, separation=(1.0, 2.0)))
    assert wide["pos"].tolist() == [[3, 3]]
    # the maximum of the same slice through zeta's northern rule is another matter: here only the sign rule of the restatement
    top = fm.candidates_of(np.where(np.isfinite(h), -h, np.nan), (1, 5, 1, 7), 1, 1, True)
    assert [(c[2], c[3]) for c in top] == [(1, 1), (1, 5), (3, 3), (4, 6)]
