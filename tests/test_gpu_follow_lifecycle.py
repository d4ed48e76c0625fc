"""-c --choose-lifecycle on the GPU: ``lec_follow_seeds_series`` against ``lec_follow_seeds`` slice by slice and bit for bit,
``lec_follow_spans`` against ``lec_follow`` / ``lec_follow_many`` on the sub-series a chain walks, bit for bit, the ending rule on a
vortex whose strength is set step by step and against the NumPy restatement (tests/follow_lifecycle_restatement.py), and the command
line on the NCEP-R2 sample: the systems test_follow_lifecycle_cpu.py pins, each one's tree the ``-t --trackfile`` run of its track."""
import ctypes as C
import filecmp
import os
import shutil

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib, follow as fw
from tests import follow_lifecycle_restatement as fl
from tests.test_follow_lifecycle_cpu import SAMPLE
from tests.test_gpu_follow import BOX, NEAR_TIE, VALUE_BAR, planted
from tests.test_gpu_follow_many import SEEDS_KW, STEM, THRESHOLD, _main, _tree_files, _workdir, planted_systems

NOT_LIVE, BAD_START = _lib.FOLLOW_NOT_LIVE, _lib.FOLLOW_BAD_START
bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# the seeds of a series
# ---------------------------------------------------------------------------------------------------------------------------
def series_of_slices(stretched):
    """Five slices on one grid: three of planted_systems with different noise, one with the NaN patch, one without a finite value."""
    parts = [planted_systems(40, stretched), planted_systems(41, stretched), planted_systems(42, stretched, nan_patch=True), planted_systems(43, stretched)]
    lat, lon = parts[0][0], parts[0][1]
    u, v, h = (np.stack([p[n] for p in parts[:3]] + [np.full_like(parts[0][n], np.nan)] + [parts[3][n]]) for n in (2, 3, 4))
    return lat, lon, u, v, h


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("field", ["zeta", "hgt"])
@pytest.mark.parametrize("stretched", [False, True])
def test_the_seeds_of_a_series_are_the_seeds_of_its_slices(stretched, field, r):
    lat, lon, u, v, h = series_of_slices(stretched)
    kw = dict(SEEDS_KW, smooth=r, field=field)
    for k in (1, 8):
        for threshold in (None, THRESHOLD[field]):
            single = [fw.find_systems(u[t], v[t], h[t], lat, lon, k=k, threshold=threshold, **kw) for t in range(5)]          # once, for both chunkings
            for chunk in (2, 5):                                        # 2: chunks of 2, 2, 1 steps -- boundaries inside the series
                pos, val, n = fw.find_systems_series(u, v, h, lat, lon, k=k, threshold=threshold, chunk_steps=chunk, **kw)
                what = (stretched, field, r, k, threshold, chunk)
                assert pos.shape == (5, k, 2) and val.shape == (5, k) and n.shape == (5,)
                assert n.tolist() == [len(s[0]) for s in single], (what, n)
                assert n[3] == 0 and n[0] >= 1                          # (the step without a finite value gives none)
                for t in range(5):
                    assert np.array_equal(pos[t, :n[t]], single[t][0]), (what, t)
                    assert np.array_equal(bits(val[t, :n[t]]), bits(single[t][1])), (what, t)                                  # bit for bit
                    assert np.all(pos[t, n[t]:] == -2) and np.all(np.isnan(val[t, n[t]:])), (what, t)
    default = fw.find_systems_series(u, v, h, lat, lon, k=8, threshold=THRESHOLD[field], **kw)                                # the default chunk
    assert np.array_equal(default[0], pos) and np.array_equal(bits(default[1]), bits(val)) and np.array_equal(default[2], n)
    if (stretched, field, r) == (False, "zeta", 1):                     # ... and one case against the rule's restatement itself
        ref = fl.seeds_series(u, v, h, lat, lon, k=8, threshold=THRESHOLD[field], **kw)
        for t in range(5):
            print("series step", t, "n_found", ref[t]["n_found"], "margin %.3e" % ref[t]["margin"])
            assert ref[t]["margin"] > NEAR_TIE
            assert n[t] == ref[t]["n_found"] and np.array_equal(pos[t, :n[t]], ref[t]["pos"])
            assert np.all(np.abs(val[t, :n[t]] - ref[t]["val"]) <= VALUE_BAR * ref[t]["scale"])


# ---------------------------------------------------------------------------------------------------------------------------
# chains with a life of their own
# ---------------------------------------------------------------------------------------------------------------------------
def _walked_is(spans, c, t0, single, what):
    """Chain c of a follow_spans result: the steps from t0 on are ``single`` (pos, val, status of the sub-series), bit for bit;
    everything before t0 is not live."""
    pos, val, status, _ = (a[c] for a in spans)
    assert np.all(status[:t0] == NOT_LIVE) and np.all(pos[:t0] == -1) and np.all(np.isnan(val[:t0])), (what, c, status)
    assert np.array_equal(status[t0:], single[2]), (what, c, status, single[2])
    assert np.array_equal(pos[t0:], single[0]), (what, c, pos.tolist(), single[0].tolist())
    assert np.array_equal(bits(val[t0:]), bits(single[1])), (what, c, val, single[1])


def _sub_series_chain(u, v, h, lat, lon, t0, ji, **kw):
    """follow_system on the sub-series from t0, started at grid point ji; where it refuses a blind first step, lec_follow_many's chain
    (which is lec_follow's, bit for bit, and refuses nothing)."""
    sub = lambda a: None if a is None else a[t0:]
    try:
        return fw.follow_system(sub(u), sub(v), sub(h), lat, lon, start=(lat[ji[0]], lon[ji[1]]), **kw)
    except ValueError:
        return tuple(a[0] for a in fw.follow_systems(sub(u), sub(v), sub(h), lat, lon, seeds=np.array([ji], dtype=np.int32), **kw))


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("field", ["zeta", "hgt"])
@pytest.mark.parametrize("case", ["nan_patch", "blind_step"])
def test_every_chain_is_lec_follow_on_its_sub_series(case, field, r):
    lat, lon, u, v, h, start, _ = planted(seed=21 + r, nan_patch=True) if case == "nan_patch" else planted(seed=7, blind_step=3)
    nt = 8
    kw = dict(BOX, smooth=r, field=field)
    bounds = fw.admissible(lat, lon, BOX["length"], BOX["width"])
    seeds, _ = fw.find_systems(u[0], v[0], h[0], lat, lon, k=4, length=BOX["length"], width=BOX["width"], smooth=r, field=field)
    assert len(seeds) >= 2
    table = [tuple(int(x) for x in s) for s in seeds] + [fw.start_index(lat, lon, start, bounds)]
    # born at step 0, no threshold: lec_follow_many's chains (one blind step does not end a chain of patience 2)
    many = fw.follow_systems(u, v, h, lat, lon, seeds=np.array(table, dtype=np.int32), **kw)
    spans = fw.follow_spans(u, v, h, lat, lon, starts=np.array([(0, *ji) for ji in table], dtype=np.int32), **kw)
    assert spans[0].shape == (len(table), nt, 2) and spans[1].shape == spans[2].shape == (len(table), nt) and spans[3].shape == (len(table), 2)
    for c in range(len(table)):
        _walked_is(spans, c, 0, tuple(a[c] for a in many), (case, field, r, "t0 0"))
        good = np.flatnonzero(many[2][c] == 0)
        assert spans[3][c].tolist() == [good[0], good[-1]]
    # born later: the walked steps are follow_system on u[t0:] from that start
    starts = [(t0, *ji) for t0 in (1, 3, nt - 1) for ji in table[-2:]]
    spans = fw.follow_spans(u, v, h, lat, lon, starts=np.array(starts, dtype=np.int32), **kw)
    for c, (t0, j, i) in enumerate(starts):
        _walked_is(spans, c, t0, _sub_series_chain(u, v, h, lat, lon, t0, (j, i), **kw), (case, field, r, "t0", t0))
        good = t0 + np.flatnonzero(spans[2][c, t0:] == 0)
        assert spans[3][c].tolist() == ([good[0], good[-1]] if good.size else [-1, -1])
    if case == "blind_step":
        # a blind window counts as not good: patience 1 ends the chain there, and a chain born there alone never becomes good before it ends
        c = len(table) - 1
        pos, val, status, span = fw.follow_spans(u, v, h, lat, lon, starts=np.array([(0, *table[c]), (3, *table[c])], dtype=np.int32), patience=1, **kw)
        assert status[0].tolist() == [0, 0, 0, 1] + [NOT_LIVE] * 4 and span[0].tolist() == [0, 2]
        assert np.array_equal(pos[0, :4], many[0][c, :4]) and np.array_equal(bits(val[0, :3]), bits(many[1][c, :3])) and np.all(pos[0, 4:] == -1)
        assert status[1].tolist() == [NOT_LIVE] * 3 + [1] + [NOT_LIVE] * 4 and span[1].tolist() == [-1, -1] and pos[1, 3].tolist() == list(table[c])


STRONG, WEAK = 1.0, 0.3
LYSIS_THRESHOLD = -6e-5         # the planted vortex has about -1.1e-4 1/s at full strength, -3.2e-5 at 0.3 of it; the noise about 5e-6


def _scaled(pattern, seed=11):
    """planted()'s moving vortex with the wind of step t scaled by pattern[t]: the vorticity scales with it."""
    lat, lon, u, v, h, start, _ = planted(seed=seed, nt=len(pattern))
    f = np.asarray(pattern, dtype=np.float64)[:, None, None]
    return lat, lon, u * f, v * f, h, start


def _check_against_restatement(got, c, ref, what):
    pos, val, status, span = (a[c] for a in got)
    print(what, "span", ref["span"], "stop", ref["stop"], "window margin %.3e threshold margin %.3e" % (ref["margin"], ref["threshold_margin"]))
    assert min(ref["margin"], ref["threshold_margin"]) > NEAR_TIE, (what, ref["margin"], ref["threshold_margin"])
    assert tuple(span) == ref["span"], (what, span, ref["span"])
    assert np.array_equal(status, ref["status"]) and np.array_equal(pos, ref["pos"]), (what, status, ref["status"], pos.tolist(), ref["pos"].tolist())
    assert np.array_equal(np.isnan(val), ref["status"] != 0)           # (the values themselves: lec_follow's bits, held to the bar in test_gpu_follow.py)


def test_lysis_by_construction():
    S, W = STRONG, WEAK
    lat, lon, u, v, h, start = _scaled([S, S, W, S, W, W, W, S])
    kw = dict(BOX, smooth=1)
    ji = fw.start_index(lat, lon, start, fw.admissible(lat, lon, BOX["length"], BOX["width"]))
    whole = fw.follow_system(u, v, h, lat, lon, start=start, **kw)
    assert np.array_equal(whole[1] <= LYSIS_THRESHOLD, np.array([1, 1, 0, 1, 0, 0, 0, 1], dtype=bool))         # the construction holds
    #          patience: (span, the last walked step)
    expected = {1: ((0, 1), 2), 2: ((0, 3), 5), 3: ((0, 3), 6), 4: ((0, 7), 7)}
    for patience, (span, stop) in expected.items():
        got = fw.follow_spans(u, v, h, lat, lon, starts=np.array([(0, *ji)], dtype=np.int32), end_threshold=LYSIS_THRESHOLD, patience=patience, **kw)
        assert tuple(got[3][0]) == span, (patience, got[3][0])
        assert got[2][0].tolist() == [0] * (stop + 1) + [NOT_LIVE] * (7 - stop), (patience, got[2][0])
        assert np.all(got[0][0, stop + 1:] == -1) and np.all(np.isnan(got[1][0, stop + 1:]))
        assert np.array_equal(got[0][0, :stop + 1], whole[0][:stop + 1]) and np.array_equal(bits(got[1][0, :stop + 1]), bits(whole[1][:stop + 1]))
        ref = fl.chain(u, v, h, lat, lon, 0, ji, end_threshold=LYSIS_THRESHOLD, patience=patience, **kw)
        assert (ref["span"], ref["stop"]) == (span, stop)
        _check_against_restatement(got, 0, ref, ("lysis, patience", patience))


@pytest.mark.parametrize("pattern, patience, t0, span, stop", [
    ([STRONG] * 6 + [WEAK] * 2, 3, 0, (0, 5), 7),           # weak up to the series' end, the patience not used up: last = the last good step
    ([STRONG] * 6 + [WEAK] * 2, 2, 2, (2, 5), 7),           # ... used up exactly at the last step, born at step 2
    ([WEAK] * 8, 2, 0, (-1, -1), 1),                        # never good
    ([WEAK] * 8, 9, 3, (-1, -1), 7),                        # never good, walked to the end
    ([WEAK, WEAK, STRONG, STRONG, WEAK, WEAK, WEAK, STRONG], 3, 0, (2, 3), 6),      # good only after two weak steps: first = the first good step
])
def test_spans_at_the_ends_of_the_series(pattern, patience, t0, span, stop):
    lat, lon, u, v, h, start = _scaled(pattern)
    kw = dict(BOX, smooth=0)
    whole = fw.follow_system(u, v, h, lat, lon, start=start, **kw)
    ji = tuple(int(x) for x in whole[0][t0])                # on the vortex at the step of birth
    got = fw.follow_spans(u, v, h, lat, lon, starts=np.array([(t0, *ji)], dtype=np.int32), end_threshold=LYSIS_THRESHOLD, patience=patience, **kw)
    assert tuple(got[3][0]) == span
    assert got[2][0].tolist() == [NOT_LIVE] * t0 + [0] * (stop + 1 - t0) + [NOT_LIVE] * (7 - stop)
    ref = fl.chain(u, v, h, lat, lon, t0, ji, end_threshold=LYSIS_THRESHOLD, patience=patience, **kw)
    assert (ref["span"], ref["stop"]) == (span, stop)
    _check_against_restatement(got, 0, ref, ("ends", pattern, patience, t0))


def test_bad_table_entries_read_nothing():
    lat, lon, u, v, h, start, _ = planted(seed=13, nt=4)
    jlo, jhi, ilo, ihi = fw.admissible(lat, lon, BOX["length"], BOX["width"])
    good = (1, jlo + 5, ilo + 7)
    bad = [(-1, jlo, ilo), (4, jlo, ilo), (0, jlo - 1, ilo), (0, jhi + 1, ilo), (0, jlo, ilo - 1), (0, jlo, ihi + 1), (0, -1, -1), (2, -2, -2)]
    pos, val, status, span = fw.follow_spans(u, v, h, lat, lon, starts=np.array([good] + bad + [good], dtype=np.int32), **BOX)
    for c in range(1, len(bad) + 1):
        assert np.all(status[c] == BAD_START) and np.all(pos[c] == -1) and np.all(np.isnan(val[c])) and span[c].tolist() == [-1, -1], (c, bad[c - 1])
    for c in (0, len(bad) + 1):                              # their neighbours in the table are chains as ever
        assert status[c].tolist() == [NOT_LIVE, 0, 0, 0] and span[c].tolist() == [1, 3]
    assert np.array_equal(pos[0], pos[-1]) and np.array_equal(bits(val[0]), bits(val[-1]))


def test_more_chains_than_compute_units():
    lat, lon, u, v, h, start, rival = planted(seed=13, nt=3)
    bounds = fw.admissible(lat, lon, BOX["length"], BOX["width"])
    jlo, jhi, ilo, ihi = bounds
    # on the path's vortex, on the rival, and twice over noise that never reaches the threshold: 12 distinct (t0, start), chains of every length
    places = [fw.start_index(lat, lon, start, bounds), fw.start_index(lat, lon, rival, bounds), (jlo + 2, ilo + 3), (jhi - 1, ihi - 20)]
    distinct = [(t0, *ji) for t0 in range(3) for ji in places]
    table = np.array([distinct[c % len(distinct)] for c in range(300)], dtype=np.int32)
    kw = dict(BOX, smooth=1, end_threshold=LYSIS_THRESHOLD, patience=1)
    many = fw.follow_spans(u, v, h, lat, lon, starts=table, **kw)
    alone = [fw.follow_spans(u, v, h, lat, lon, starts=np.array([row], dtype=np.int32), **kw) for row in distinct]          # once per distinct start
    for c in range(300):
        one = alone[c % len(distinct)]
        assert np.array_equal(many[0][c], one[0][0]) and np.array_equal(many[2][c], one[2][0]) and np.array_equal(many[3][c], one[3][0]), c
        assert np.array_equal(bits(many[1][c]), bits(one[1][0])), c
    print("300 chains: the spans of the 12", many[3][:12].tolist())
    assert many[3][:12].tolist() == [[t0, 2] if n < 2 else [-1, -1] for t0 in range(3) for n in range(4)]
    assert many[2][2].tolist() == [0, NOT_LIVE, NOT_LIVE] and many[2][8].tolist() == [NOT_LIVE, NOT_LIVE, 0]


def test_a_tile_beyond_64_kib_of_lds_born_at_two_steps():
    """test_gpu_follow_many.py's wide search window (127 x 127 doubles = 129 KB of LDS), chains born at steps 0 and 1."""
    rng = np.random.default_rng(3)
    lat, lon = -70.0 + 0.5 * np.arange(140), -100.0 + 0.5 * np.arange(150)
    u, v = rng.standard_normal((2, 3, 140, 150))
    kw = dict(length=4.0, width=4.0, search=31.0, smooth=1)
    bounds = fw.admissible(lat, lon, 4.0, 4.0)
    starts = [(t0, *fw.start_index(lat, lon, st, bounds)) for t0 in (0, 1) for st in ((-35.0, -62.0), (-50.0, -80.0))]
    got = fw.follow_spans(u, v, None, lat, lon, starts=np.array(starts, dtype=np.int32), **kw)
    for c, (t0, j, i) in enumerate(starts):
        _walked_is(got, c, t0, fw.follow_system(u[t0:], v[t0:], None, lat, lon, start=(lat[j], lon[i]), **kw), "large tile")
        assert got[3][c].tolist() == [t0, 2]
    with pytest.raises(_lib.LecLibraryError, match="limit"):
        fw.follow_spans(u, v, None, lat, lon, starts=np.array(starts, dtype=np.int32), **dict(kw, search=36.0))


def test_bad_scalars_are_refused_with_the_field_named_and_nothing_is_launched():
    lat, lon, u, v, h, _, _ = planted(seed=13, nt=3)
    s = fw._Slices(u, v, h, lat, lon, 3, length=10.0, width=10.0, smooth=0, field="zeta", hemisphere=None, formulation="metpy_no_crs", device="cuda:0")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    i32 = lambda *shape: torch.full(shape, 77, dtype=torch.int32, device=s.dev)
    f64 = lambda *shape: torch.full(shape, 77.0, dtype=torch.float64, device=s.dev)
    start = torch.as_tensor(np.array([(0, s.bounds[0], s.bounds[2])], dtype=np.int32)).to(s.dev)
    out = dict(pos=i32(1, 3, 2), val=f64(1, 3), status=i32(1, 3), span=i32(1, 2), work=f64(3, 51, 71), seed_pos=i32(3, 8, 2), seed_val=f64(3, 8), n_found=i32(3))

    def spans(**change):
        a = _lib.FollowSpansArgs(**dict(dict(nt=3, sj=3, si=3, n_chains=1, patience=2, start_d=ptr(start), end_threshold=float("nan"), pos_d=ptr(out["pos"]),
                                             val_d=ptr(out["val"]), status_d=ptr(out["status"]), span_d=ptr(out["span"]), **s.common()), **change))
        return s.lib.lec_follow_spans(C.byref(a))

    def series(**change):
        a = _lib.FollowSeedsSeriesArgs(**dict(dict(nt=3, ej=5, ei=5, k_max=8, threshold=float("nan"), work_d=ptr(out["work"]), seed_pos_d=ptr(out["seed_pos"]),
                                                   seed_val_d=ptr(out["seed_val"]), n_found_d=ptr(out["n_found"]), **s.common()), **change))
        return s.lib.lec_follow_seeds_series(C.byref(a))

    for call, change, word in ((spans, {"patience": 0}, b"patience"), (spans, {"nt": 0}, b"nt"), (series, {"k_max": 0}, b"k_max"), (series, {"nt": 0}, b"nt")):
        assert call(**change) == 1 and word in s.lib.lec_last_error(), (change, s.lib.lec_last_error())
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in out.values())            # nothing ran
    assert spans() == 0 and series() == 0                              # the same arguments without the change: accepted
    torch.cuda.synchronize()
    assert out["span"].cpu().numpy().tolist() == [[0, 2]] and int(out["n_found"].cpu().numpy().min()) >= 1
    with pytest.raises(ValueError, match="patience"):
        fw.follow_spans(u, v, h, lat, lon, starts=np.array([(0, s.bounds[0], s.bounds[2])], dtype=np.int32), patience=0, **BOX)


# ---------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------
LIFECYCLE = ["-r", "-c", "--choose-systems", "8", "--choose-lifecycle", "--choose-threshold", "-5e-5"]
TIMES = ["2005-08-08-0000", "2005-08-08-0600", "2005-08-08-1200", "2005-08-08-1800", "2005-08-09-0000"]


@pytest.fixture(scope="module")
def lifecycle_run(tmp_path_factory, golden_dir):
    """ONE ``-c --choose-systems 8 --choose-lifecycle --choose-threshold -5e-5`` run on the sample, shared: its directory."""
    path = _workdir(tmp_path_factory.mktemp("lifecycle"), golden_dir)
    before = os.getcwd()
    world = os.environ.pop("WORLD_SIZE", None)
    os.chdir(path)
    try:
        _main([os.path.join(golden_dir, STEM + ".nc")] + LIFECYCLE)
    finally:
        os.chdir(before)
        if world is not None:
            os.environ["WORLD_SIZE"] = world
    return path


def test_cli_writes_the_systems_of_the_sample_and_their_tracks(lifecycle_run):
    batch = lifecycle_run / "LEC_Results" / f"{STEM}_choose_batch"
    kept = [n + 1 for n, row in enumerate(SAMPLE) if row[3] == "kept"]
    assert kept == [1, 2, 3, 5]
    assert sorted(os.listdir(batch)) == ["batch.csv"] + [f"choose_s{n:02d}" for n in kept] + [f"log.{STEM}", "systems.csv"]
    log = (batch / f"log.{STEM}").read_text()
    assert "lec_follow_seeds_series" in log and "lec_follow_spans" in log and "6 of them are births" in log
    table = pd.read_csv(batch / "systems.csv", keep_default_na=False)
    assert list(table.columns) == ["system", "lat", "lon", "value", "trackfile", "same_centre_as", "same_centre_from", "first_time", "last_time",
                                   "steps", "ended", "continuation_of", "left_out"]
    assert list(table["system"]) == [f"choose_s{n:02d}" for n in range(1, 7)]
    for n, (row, (t0, (la, lo), span, outcome, of)) in enumerate(zip(table.to_dict("records"), SAMPLE), start=1):
        assert (row["lat"], row["lon"]) == (la, lo) and float(row["value"]) <= -5e-5, row
        assert row["left_out"] == ("" if outcome == "kept" else outcome) and row["continuation_of"] == ("" if of is None else f"choose_s{of + 1:02d}"), row
        assert (os.path.basename(row["trackfile"]) == f"choose_s{n:02d}") if outcome == "kept" else row["trackfile"] == "", row
        if span is not None:
            assert (row["first_time"], row["last_time"], int(row["steps"])) == (TIMES[span[0]], TIMES[span[1]], span[1] - span[0] + 1), row
            assert row["ended"] == ("end of series" if span[1] == 4 else "weak"), row
        assert outcome != "kept" or row["same_centre_as"] == "", row
    listing = pd.read_csv(batch / "batch.csv")
    assert [os.path.basename(p) for p in listing["trackfile"]] == [f"choose_s{n:02d}" for n in kept] and list(listing["steps"]) == [3, 3, 3, 2]
    for n in kept:
        t0, (la, lo), span, _, _ = SAMPLE[n - 1]
        tr = pd.read_csv(batch / f"choose_s{n:02d}", sep=";")
        assert list(tr.columns) == ["time", "Lat", "Lon", "length", "width"] and (tr.length == 15).all() and (tr.width == 15).all()
        assert list(tr.time) == TIMES[span[0]: span[1] + 1] and span[0] == t0
        assert (tr.Lat[0], tr.Lon[0]) == (la, lo)           # the first line: the birth's time and position


@pytest.mark.parametrize("n", [1, 5])                      # one that dies early, one that is born late
def test_cli_each_system_is_the_track_run_of_its_own_time_steps(lifecycle_run, golden_dir, monkeypatch, n):
    path = lifecycle_run
    monkeypatch.chdir(path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    res = path / "LEC_Results"
    shutil.rmtree(res / f"{STEM}_track", ignore_errors=True)
    _main([os.path.join(golden_dir, STEM + ".nc"), "-r", "-t", "--trackfile", str(res / f"{STEM}_choose_batch" / f"choose_s{n:02d}")])
    single, tree = res / f"{STEM}_track", res / f"{STEM}_choose_s{n:02d}_track"
    files = _tree_files(single)
    assert files == _tree_files(tree) and f"./{STEM}_track_results.csv" in files and f"./{STEM}_track_trackfile" in files
    for f in files:
        if not f.endswith("/"):
            assert filecmp.cmp(single / f, tree / f, shallow=False), f


def test_cli_without_the_flag_follows_the_first_step_s_systems_through_the_series(tmp_path, golden_dir, monkeypatch):
    monkeypatch.chdir(_workdir(tmp_path, golden_dir))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    _main([os.path.join(golden_dir, STEM + ".nc")] + [a for a in LIFECYCLE if a != "--choose-lifecycle"])
    batch = tmp_path / "LEC_Results" / f"{STEM}_choose_batch"
    assert sorted(os.listdir(batch)) == ["batch.csv", "choose_s01", "choose_s02", f"log.{STEM}", "systems.csv"]
    assert list(pd.read_csv(batch / "systems.csv").columns) == ["system", "lat", "lon", "value", "trackfile", "same_centre_as", "same_centre_from"]
    assert list(pd.read_csv(batch / "batch.csv")["steps"]) == [5, 5]
    for n in (1, 2):
        tr = pd.read_csv(batch / f"choose_s{n:02d}", sep=";")
        assert list(tr.time) == TIMES and (tr.Lat[0], tr.Lon[0]) == SAMPLE[n - 1][1]
