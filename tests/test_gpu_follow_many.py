"""-c --choose-systems on the GPU: ``lec_follow_seeds`` against the NumPy restatement of its rule (tests/follow_many_restatement.py),
``lec_follow_many`` against ``lec_follow`` chain by chain and bit for bit, and the defining property of the command line -- a
``-c --choose-systems`` run IS the ``-t --trackfiles`` run on the tracks it wrote, each of which is the track ``-c --choose-start``
writes from that system's seed."""
import filecmp
import os
import shutil

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib, follow as fw
from tests import follow_many_restatement as fm
from tests import follow_restatement as fr
from tests.test_gpu_follow import BOX, NEAR_TIE, VALUE_BAR, compare, planted

# (degrees north of lat[0], degrees east of lon[0], amplitude); the last one's centre lies outside the admissible centres of a 10 x 10 box
VORTICES = [(14.0, 55.0, 12.0), (16.0, 20.0, 9.0), (35.0, 22.0, 6.0), (38.0, 50.0, 4.5), (3.0, 36.0, 15.0)]
THRESHOLD = {"zeta": -4.5e-5, "hgt": 1470.0}
SEEDS_KW = dict(length=10.0, width=10.0, separation=(5.0, 5.0))


def planted_systems(seed, stretched=False, nan_patch=False):
    """ONE slice of planted()'s grid with four vortices / height lows of different strength over noise, and a fifth, the strongest, whose
    centre no 10 x 10 box can have.  Southern hemisphere: cyclonic = negative vorticity."""
    rng = np.random.default_rng(seed)
    lat, lon = -60.0 + np.arange(51.0), -90.0 + np.arange(71.0)
    if stretched:
        lat = np.sort(lat + 0.25 * np.sin(np.arange(lat.size)))
        lon = np.sort(lon + 0.3 * np.cos(np.arange(lon.size)))
    y, x = lat[:, None], lon[None, :]
    shape = (lat.size, lon.size)
    u, v, h = 0.3 * rng.standard_normal(shape), 0.3 * rng.standard_normal(shape), 1500.0 + 2.0 * rng.standard_normal(shape)
    for dy0, dx0, amp in VORTICES:
        dy, dx = y - (lat[0] + dy0), x - (lon[0] + dx0)
        g = np.exp(-(dx * dx + dy * dy) / 12.5)
        u += amp * dy * g
        v += -amp * dx * g
        h -= amp * 80.0 / 6.0 * g
    if nan_patch:                                                    # below-ground points on the flank of the second vortex
        j, i = int(np.argmin(np.abs(lat - (lat[0] + 18.0)))), int(np.argmin(np.abs(lon - (lon[0] + 22.0))))
        for a in (u, h):
            a[j - 1: j + 2, i - 1: i + 2] = np.nan
    return lat, lon, u, v, h


def _check_seeds(got, ref, what):
    """Positions, order and n_found EQUAL; values within the bar; no case may be left out as a near tie."""
    pos, val = got
    print(what, "n_found", ref["n_found"], "margins: neighbourhood %.3e rank %.3e threshold %.3e" % tuple(
        float(np.min(ref[k])) if len(ref[k]) else np.inf for k in ("neighbourhood", "rank", "threshold")))
    assert ref["margin"] > NEAR_TIE, (what, ref["margin"])
    assert len(pos) == ref["n_found"] and np.array_equal(pos, ref["pos"]), (what, pos.tolist(), ref["pos"].tolist())
    assert np.all(np.abs(val - ref["val"]) <= VALUE_BAR * ref["scale"]), (what, val, ref["val"])


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("field", ["zeta", "hgt"])
@pytest.mark.parametrize("stretched, nan_patch", [(False, False), (True, False), (False, True)])
def test_seeds_match_the_restatement(stretched, nan_patch, field, r):
    lat, lon, u, v, h = planted_systems(40 + r, stretched, nan_patch)
    kw = dict(SEEDS_KW, smooth=r, field=field)
    centres = [(lat[0] + dy, lon[0] + dx) for dy, dx, _ in VORTICES]
    near = lambda p, c: np.hypot(lat[p[0]] - c[0], lon[p[1]] - c[1]) < 2.0
    # the three strongest, in order
    ref = fm.find_systems(u, v, h, lat, lon, k=3, **kw)
    got = fw.find_systems(u, v, h, lat, lon, k=3, **kw)
    _check_seeds(got, ref, (stretched, nan_patch, field, r, "k 3"))
    assert len(got[0]) == 3 and all(near(p, c) for p, c in zip(got[0], centres[:3]))
    # more room than systems, with a threshold: the four, and not the fifth or its flank, whose centre lies outside the admissible centres
    ref = fm.find_systems(u, v, h, lat, lon, k=8, threshold=THRESHOLD[field], **kw)
    got = fw.find_systems(u, v, h, lat, lon, k=8, threshold=THRESHOLD[field], **kw)          # (checks that the rest is (-2, -2) and NaN)
    _check_seeds(got, ref, (stretched, nan_patch, field, r, "k 8, threshold"))
    assert len(got[0]) == 4 and all(near(p, c) for p, c in zip(got[0], centres[:4]))


def test_ties_and_plateaus_yield_their_first_point():
    lat, lon = -60.0 + np.arange(51.0), -90.0 + np.arange(71.0)
    h = np.full((51, 71), 1500.0)
    z = np.zeros_like(h)
    h[22, 19] = h[20, 21] = h[20, 23] = 1400.0                        # three equal minima inside one neighbourhood (+-5 points)
    h[33:35, 40:43] = 1450.0                                          # a 2 x 3 plateau elsewhere
    kw = dict(SEEDS_KW, field="hgt")
    pos, val = fw.find_systems(z, z, h, lat, lon, k=8, **kw)
    assert pos.tolist() == [[20, 21], [33, 40]] and val.tolist() == [1400.0, 1450.0]       # (the constant around them seeds nothing)
    ref = fm.find_systems(z, z, h, lat, lon, k=8, **kw)
    assert np.array_equal(pos, ref["pos"]) and np.array_equal(val, ref["val"])
    pos, val = fw.find_systems(z, z, h, lat, lon, k=1, **kw)
    assert pos.tolist() == [[20, 21]] and val.tolist() == [1400.0]
    pos, val = fw.find_systems(z, z, h, lat, lon, k=8, threshold=1300.0, **kw)
    assert len(pos) == 0 and len(val) == 0


def _single(u, v, h, lat, lon, start_ji, **kw):
    """follow_system from a grid point (None: no start): the coordinates of an admissible centre come back as that centre."""
    start = None if start_ji is None else (lat[start_ji[0]], lon[start_ji[1]])
    return fw.follow_system(u, v, h, lat, lon, start=start, **kw)


def _same_chain(many, c, single, what):
    pos, val, status = (a[c] for a in many)
    assert np.array_equal(status, single[2]), (what, c, status, single[2])
    assert np.array_equal(pos, single[0]), (what, c, pos.tolist(), single[0].tolist())
    assert np.array_equal(val.view(np.int64), single[1].view(np.int64)), (what, c, val, single[1])      # bit for bit


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("field", ["zeta", "hgt"])
@pytest.mark.parametrize("case", ["nan_patch", "blind_step"])
def test_every_chain_is_lec_follow_from_its_start(case, field, r):
    lat, lon, u, v, h, start, _ = planted(seed=21 + r, nan_patch=True) if case == "nan_patch" else planted(seed=7, blind_step=3)
    kw = dict(BOX, smooth=r, field=field)
    bounds = fw.admissible(lat, lon, BOX["length"], BOX["width"])
    seeds, _ = fw.find_systems(u[0], v[0], h[0], lat, lon, k=4, length=BOX["length"], width=BOX["width"], smooth=r, field=field)
    assert len(seeds) >= 2
    bad = [(bounds[0] - 1, bounds[2]), (-2, -2), (-1, bounds[2]), (bounds[1], bounds[3] + 1)]
    table = [tuple(s) for s in seeds] + [fw.start_index(lat, lon, start, bounds), (-1, -1)] + bad
    many = fw.follow_systems(u, v, h, lat, lon, seeds=np.array(table, dtype=np.int32), **kw)
    assert many[0].shape == (len(table), 8, 2) and many[1].shape == many[2].shape == (len(table), 8)
    for c, ji in enumerate(table[:-len(bad)]):
        _same_chain(many, c, _single(u, v, h, lat, lon, None if ji == (-1, -1) else ji, **kw), (case, field, r))
    for c in range(len(table) - len(bad), len(table)):                  # no admissible centre: nothing is read
        assert np.all(many[2][c] == _lib.FOLLOW_BAD_START) and np.all(many[0][c] == -1) and np.all(np.isnan(many[1][c]))
    if case == "blind_step":
        assert many[2][0].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    # (lat, lon) starts and None go the same way as follow_system's
    again = fw.follow_systems(u, v, h, lat, lon, starts=[start, None], **kw)
    k = len(seeds)
    assert np.array_equal(again[0], many[0][k: k + 2]) and np.array_equal(again[2], many[2][k: k + 2])
    assert np.array_equal(again[1].view(np.int64), many[1][k: k + 2].view(np.int64))
    if (case, field, r) == ("nan_patch", "zeta", 1):                    # ... and one case against the rule's restatement itself
        compare(tuple(a[k] for a in many), fr.follow(u, v, h, lat, lon, start=start, **kw), "chain of lec_follow_many")


def test_more_chains_than_compute_units():
    lat, lon, u, v, h, _, _ = planted(seed=13, nt=3)
    jlo, jhi, ilo, ihi = fw.admissible(lat, lon, BOX["length"], BOX["width"])
    distinct = [(jlo + (7 * n) % (jhi - jlo + 1), ilo + (11 * n) % (ihi - ilo + 1)) for n in range(12)]
    table = np.array([distinct[c % len(distinct)] for c in range(300)], dtype=np.int32)
    many = fw.follow_systems(u, v, h, lat, lon, seeds=table, smooth=1, **BOX)
    singles = [_single(u, v, h, lat, lon, ji, smooth=1, **BOX) for ji in distinct]                 # once per distinct start
    for c in range(300):
        _same_chain(many, c, singles[c % len(distinct)], "300 chains")


def test_a_tile_beyond_64_kib_of_lds_in_several_workgroups():
    """test_gpu_follow.py's wide search window (127 x 127 doubles = 129 KB of LDS), three workgroups of it."""
    rng = np.random.default_rng(3)
    lat, lon = -70.0 + 0.5 * np.arange(140), -100.0 + 0.5 * np.arange(150)
    u, v = rng.standard_normal((2, 3, 140, 150))
    kw = dict(length=4.0, width=4.0, search=31.0, smooth=1)
    starts = [(-35.0, -62.0), (-50.0, -80.0), None]
    many = fw.follow_systems(u, v, None, lat, lon, starts=starts, **kw)
    for c, st in enumerate(starts):
        _same_chain(many, c, fw.follow_system(u, v, None, lat, lon, start=st, **kw), "large tile")
    with pytest.raises(_lib.LecLibraryError, match="limit"):
        fw.follow_systems(u, v, None, lat, lon, starts=starts, **dict(kw, search=36.0))


# ---------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------
STEM = "testdata_NCEP-R2"
SEEDS = [(-50.0, -7.5), (-70.0, -60.0)]          # what the rule gives on the sample's first step at the default 15 x 15 box (restated below)


def _main(argv):
    import lorenzcycletoolkit
    lorenzcycletoolkit.main(argv)


def _tree_files(d):
    out = []
    for root, dirs, files in os.walk(d):
        rel = os.path.relpath(root, d)
        out += [os.path.join(rel, x) + "/" for x in dirs]
        out += [os.path.join(rel, x) for x in files if not x.startswith("log.")]
    return sorted(out)


def _workdir(path, golden_dir):
    os.makedirs(path / "inputs")
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_NCEP-R2"), path / "inputs" / "namelist")
    return path


@pytest.fixture
def workdir(tmp_path, golden_dir, monkeypatch):
    monkeypatch.chdir(_workdir(tmp_path, golden_dir))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return tmp_path


@pytest.fixture(scope="module")
def systems_run(tmp_path_factory, golden_dir):
    """ONE ``-c --choose-systems 2`` run, shared: its directory and the text of the two tracks."""
    path = _workdir(tmp_path_factory.mktemp("systems"), golden_dir)
    before = os.getcwd()
    world = os.environ.pop("WORLD_SIZE", None)
    os.chdir(path)
    try:
        _main([os.path.join(golden_dir, STEM + ".nc"), "-r", "-c", "--choose-systems", "2"])
    finally:
        os.chdir(before)
        if world is not None:
            os.environ["WORLD_SIZE"] = world
    batch = path / "LEC_Results" / f"{STEM}_choose_batch"
    return path, {n: (batch / f"choose_s{n:02d}").read_text() for n in (1, 2)}


def test_cli_writes_the_systems_and_their_tracks(systems_run, golden_dir):
    import types
    path, tracks = systems_run
    batch = path / "LEC_Results" / f"{STEM}_choose_batch"
    assert sorted(os.listdir(batch)) == ["batch.csv", "choose_s01", "choose_s02", f"log.{STEM}", "systems.csv"]
    log = (batch / f"log.{STEM}").read_text()
    assert "lec_follow_seeds" in log and "lec_follow_many" in log and "2 of at most 2 systems found" in log
    # the seeds are the rule's: restated on the sample's first step, far from a tie
    a = types.SimpleNamespace(infile=os.path.join(golden_dir, STEM + ".nc"), mpas=False, choose_domain=None)
    u, v, h, lat, lon, _ = fw.search_domain_slices(a, os.path.join(golden_dir, "inputs", "namelist_NCEP-R2"))
    ref = fm.find_systems(u[0], v[0], h[0], lat, lon, k=2)
    print("sample: rank margins", ref["rank"], "neighbourhood margins", ref["neighbourhood"])
    assert ref["margin"] > NEAR_TIE and [(lat[j], lon[i]) for j, i in ref["pos"]] == SEEDS
    table = pd.read_csv(batch / "systems.csv")
    assert list(table["system"]) == ["choose_s01", "choose_s02"] and list(zip(table["lat"], table["lon"])) == SEEDS
    assert np.all(np.abs(table["value"].values - ref["val"]) <= VALUE_BAR * ref["scale"])
    assert {"trackfile", "same_centre_as", "same_centre_from"} <= set(table.columns) and table["same_centre_as"].isna().all()
    listing = pd.read_csv(batch / "batch.csv")
    assert [os.path.basename(p) for p in listing["trackfile"]] == ["choose_s01", "choose_s02"] and list(listing["steps"]) == [5, 5]
    for n in (1, 2):
        tr = pd.read_csv(batch / f"choose_s{n:02d}", sep=";")
        assert list(tr.columns) == ["time", "Lat", "Lon", "length", "width"] and (tr.length == 15).all() and (tr.width == 15).all()
        assert (tr.Lat[0], tr.Lon[0]) == SEEDS[n - 1]          # (the search window of 5 degrees lies inside the seed's neighbourhood of 7.5)


@pytest.mark.parametrize("n", [1, 2])
def test_cli_each_system_is_the_choose_start_run_and_the_track_run(systems_run, golden_dir, monkeypatch, n):
    path, tracks = systems_run
    monkeypatch.chdir(path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    infile = os.path.join(golden_dir, STEM + ".nc")
    res = path / "LEC_Results"
    # the track: line for line what -c --choose-start <the seed> writes
    _main([infile, "-r", "-c", "--choose-start", repr(SEEDS[n - 1][0]), repr(SEEDS[n - 1][1])])
    assert (res / f"{STEM}_choose" / f"{STEM}_choose_track").read_text().splitlines() == tracks[n].splitlines()
    # the tree: byte for byte what -t --trackfile <that track> writes
    shutil.rmtree(res / f"{STEM}_track", ignore_errors=True)
    _main([infile, "-r", "-t", "--trackfile", str(res / f"{STEM}_choose_batch" / f"choose_s{n:02d}")])
    single, tree = res / f"{STEM}_track", res / f"{STEM}_choose_s{n:02d}_track"
    files = _tree_files(single)
    assert files == _tree_files(tree) and f"./{STEM}_track_results.csv" in files and f"./{STEM}_track_trackfile" in files
    for f in files:
        if not f.endswith("/"):
            assert filecmp.cmp(single / f, tree / f, shallow=False), f


def test_cli_starts_file_and_threshold(systems_run, workdir, golden_dir):
    _, tracks = systems_run
    infile = os.path.join(golden_dir, STEM + ".nc")
    batch = workdir / "LEC_Results" / f"{STEM}_choose_batch"
    (workdir / "starts").write_text("Lat;Lon\n" + "".join(f"{la!r};{lo!r}\n" for la, lo in SEEDS))
    _main([infile, "-r", "-c", "--choose-starts", "starts"])
    assert {n: (batch / f"choose_s{n:02d}").read_text() for n in (1, 2)} == tracks
    _main([infile, "-r", "-c", "--choose-systems", "3", "--choose-threshold", "-5e-5"])
    assert "2 of at most 3 systems found" in (batch / f"log.{STEM}").read_text()
    assert {n: (batch / f"choose_s{n:02d}").read_text() for n in (1, 2)} == tracks and not (batch / "choose_s03").exists()
    assert len(pd.read_csv(batch / "systems.csv")) == 2


def test_cli_a_box_that_does_not_fit_leaves_only_the_log(workdir, golden_dir):
    infile = os.path.join(golden_dir, STEM + ".nc")
    with pytest.raises(ValueError, match="does not fit"):
        _main([infile, "-r", "-c", "--choose-systems", "2", "--choose-box", "90", "15"])
    assert os.listdir(workdir / "LEC_Results") == [f"{STEM}_choose_batch"]
    assert os.listdir(workdir / "LEC_Results" / f"{STEM}_choose_batch") == [f"log.{STEM}"]
