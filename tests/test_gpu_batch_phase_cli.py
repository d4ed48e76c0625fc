"""--batch-composites --batch-composites-phase on the command line (GPU).  Every file of the run without the phase flag is there byte for
byte and the only additions are under the ensemble directory's phases/; the phase files parse back (repr(float) round-trips) to the API's
numbers exactly; phases.csv, phase_members.csv and phase_terms.csv agree with each other and with the tracks' own written files; with
``peak:L`` every track's peak is the first argmax of |min_max_zeta_850| of its own written ``*_trackfile`` and the lag-0 map the in-order
mean of the tracks' columns at those steps."""
import io
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import batch
from lorenzcycletoolkit_amd.constants import MAP_TERMS
from lorenzcycletoolkit_amd.synthetic import write_classic_nc
from tests.test_gpu_batch_composite_cli import _main, _table, _track_file, _tree, _under, workdir  # noqa: F401

T = lambda k: (pd.Timestamp("2020-01-01") + pd.Timedelta(hours=3 * k)).strftime("%Y-%m-%d-%H%M")


def _phase_names(n_bin):
    return sorted([f"{t}{sd}_dlat_dlon_phase{b:02d}.csv" for t in MAP_TERMS for sd in ("", "_sd") for b in range(n_bin)]
                  + ["phases.csv", "phase_members.csv", "phase_terms.csv"])


def _added(infile, flags, clock):
    """(the files the phase flag adds under the ensemble directory's phases/, the whole tree, the log): everything else is byte for byte
    the run without the flag."""
    plain, _ = _main([infile, "-r", *flags, "--batch-composites"])
    got, log = _main([infile, "-r", *flags, "--batch-composites", "--batch-composites-phase", clock])
    added = {k: v for k, v in got.items() if k not in plain}
    assert sorted(k for k in got if k not in added) == sorted(plain)
    for k, v in plain.items():
        assert got[k] == v, f"{k} differs from the run without --batch-composites-phase"
    return added, got, log


def _api(infile, tracks, ranges_of, **kw):
    """``LECEngine.compute(batch_composites=..., batch_composite_phases=...)`` on the same host-prepared union; ``ranges_of(plan)``."""
    from lorenzcycletoolkit_amd import dataset as ds
    from lorenzcycletoolkit_amd.engine import LECEngine
    from lorenzcycletoolkit_amd.frameworks import host_fields
    data, plan = batch.prepare_union(SimpleNamespace(infile=infile, mpas=False), tracks, "inputs/namelist")
    arrays, common, phi_scale = host_fields(data, ds.read_namelist("inputs/namelist"))
    eng = LECEngine(data.lat, data.lon, data.level, device="cuda:0")
    cubes = [torch.as_tensor(np.ascontiguousarray(a, dtype=common)).to("cuda:0") for a in arrays]
    assert list(plan.groups) == [(16, 16, True)]
    boxes = [b for tr in plan.tracks for b in tr.boxes]
    ranges = ranges_of(plan)
    res = eng.compute(*cubes, eng.prepare_boxes(boxes, nyb_min=16, lon_uniform=True), phi_scale=phi_scale, per_step_boxes=True,
                      drop_any_time=False, steps=torch.as_tensor(np.concatenate([tr.steps for tr in plan.tracks])).to("cuda:0"),
                      tcoef=torch.as_tensor(np.concatenate([tr.tcoef for tr in plan.tracks])).to("cuda:0"),
                      batch_composites=[tr.n for tr in plan.tracks], batch_composite_phases=ranges, **kw)
    return res, ranges, plan


def _setup(workdir, golden_dir, dtype):
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_ERA5"), workdir / "inputs" / "namelist")
    infile = str(workdir / "synth.nc")
    write_classic_nc(infile, dtype)
    return infile


def test_lifetime_3_adds_only_the_phase_files_and_they_are_the_api_s(workdir, golden_dir):
    infile = _setup(workdir, golden_dir, np.float64)
    tracks = [_track_file(workdir / "six_hourly.csv", [(T(k), -30.0 - k // 2, -55.0 + k) for k in range(0, 12, 2)]),
              _track_file(workdir / "three_hourly.csv", [(T(k), -25.0, -45.0 - k) for k in range(1, 9)]),
              _track_file(workdir / "late.csv", [(T(k), -40.0 + k, -35.0) for k in range(6, 8)])]
    stems = ["six_hourly", "three_hourly", "late"]
    added, got, log = _added(infile, ["-t", "--trackfiles", *tracks], "lifetime:3")
    phases_dir = os.path.join("synth_track_batch", "results_composites", "phases")
    files = _under(added, phases_dir)
    assert len(files) == len(added) and sorted(files) == _phase_names(3)          # nothing anywhere else, no track's tree gains a file
    assert "--batch-composites-phase lifetime:3: 3 bin(s) over 3 track(s) of 16 x 16 box points" in log
    res, ranges, plan = _api(infile, tracks, lambda plan: batch.phase_ranges(plan, "lifetime:3"))
    count = ranges[:, :, 1] - ranges[:, :, 0]
    assert count.tolist() == [[2, 2, 2], [3, 3, 2], [1, 1, 0]] and res.batch_phase_members.tolist() == [3, 3, 2]
    ens, spread = res.batch_phase_ensemble.cpu().numpy(), res.batch_phase_spread.cpu().numpy()
    mean_file = _table(got[os.path.join("synth_track_batch", "results_composites", "Ae_dlat_dlon.csv")])
    for b in range(3):
        for i, term in enumerate(MAP_TERMS):
            e, s = _table(files[f"{term}_dlat_dlon_phase{b:02d}.csv"]), _table(files[f"{term}_sd_dlat_dlon_phase{b:02d}.csv"])
            assert np.array_equal(e.values, ens[b, i]) and np.array_equal(s.values, spread[b, i]), (b, term)
            assert e.index.name == "dlat" and list(e.index) == list(mean_file.index) and list(e.columns) == list(mean_file.columns)
    assert not np.isnan(ens).any() and not np.isnan(spread).any()
    listing = pd.read_csv(io.BytesIO(files["phases.csv"]))
    members = pd.read_csv(io.BytesIO(files["phase_members.csv"]))
    assert list(listing["bin"]) == [0, 1, 2] and list(listing["label"]) == [f"lifetime [{b}/3, {b + 1}/3)" for b in range(3)]
    assert [os.path.splitext(os.path.basename(p))[0] for p in members["trackfile"]] == stems and list(members["steps"]) == [6, 8, 2]
    cells = members[[f"phase{b:02d}" for b in range(3)]].to_numpy()
    assert np.array_equal(cells, count)
    assert list(listing["members"]) == (cells >= 1).sum(axis=0).tolist() == [3, 3, 2] and list(listing["steps"]) == cells.sum(axis=0).tolist()
    # phase_terms.csv: the NumPy means of the tracks' own written results
    terms = pd.read_csv(io.BytesIO(files["phase_terms.csv"]), index_col=0, float_precision="round_trip")
    assert list(terms["label"]) == list(listing["label"])
    frames = [_table(got[os.path.join(f"synth_{s}_track", "synth_track_results.csv")]) for s in stems]
    assert list(terms.columns[1:]) == list(frames[0].columns)
    for b in range(3):
        per = [np.mean(f.to_numpy(dtype=float)[lo:hi], axis=0) for f, (lo, hi) in zip(frames, ranges[:, b]) if hi > lo]
        assert np.array_equal(terms.iloc[b, 1:].to_numpy(dtype=float), np.mean(np.stack(per), axis=0), equal_nan=True), b


def test_peak_1_aligns_on_the_written_track_files_peak(workdir, golden_dir):
    infile = _setup(workdir, golden_dir, np.float32)
    tracks = [_track_file(workdir / "long.csv", [(T(k), -25.0, -45.0 - k) for k in range(1, 9)]),
              _track_file(workdir / "mid.csv", [(T(k), -30.0 - k // 2, -55.0 + k) for k in range(2, 7)]),
              _track_file(workdir / "late.csv", [(T(k), -40.0 + k, -35.0) for k in range(6, 9)])]
    stems = ["long", "mid", "late"]
    added, got, log = _added(infile, ["-t", "--trackfiles", *tracks], "peak:1")
    files = _under(added, os.path.join("synth_track_batch", "results_composites", "phases"))
    assert len(files) == len(added) and sorted(files) == _phase_names(3)
    members = pd.read_csv(io.BytesIO(files["phase_members.csv"]))
    peaks = []
    for stem, n in zip(stems, (8, 5, 3)):
        z = pd.read_csv(io.BytesIO(got[os.path.join(f"synth_{stem}_track", "synth_track_trackfile")]), sep=";")["min_max_zeta_850"].to_numpy(dtype=float)
        assert len(z) == n and np.isfinite(z).all()
        peaks.append(int(np.argmax(np.abs(z))))
        row = members.iloc[len(peaks) - 1]
        assert int(row["s_peak"]) == peaks[-1] and float(row["peak_min_max_zeta_850"]) == z[peaks[-1]]
        assert pd.Timestamp(row["peak_time"]) == pd.Timestamp("2020-01-01") + pd.Timedelta(hours=3 * ((1, 2, 6)[len(peaks) - 1] + peaks[-1]))
    listing = pd.read_csv(io.BytesIO(files["phases.csv"]))
    assert list(listing["label"]) == ["lag -1 steps (-3 h)", "lag +0 steps (+0 h)", "lag +1 steps (+3 h)"]
    want = np.array([[int(0 <= p + l < n) for l in (-1, 0, 1)] for p, n in zip(peaks, (8, 5, 3))])
    assert np.array_equal(members[["phase00", "phase01", "phase02"]].to_numpy(), want)
    assert list(listing["members"]) == want.sum(axis=0).tolist() and listing["members"][1] == 3
    # lag 0: the in-order mean of the tracks' columns at their peaks
    res, ranges, plan = _api(infile, tracks, lambda plan: np.array([[(p + l, p + l + 1) if 0 <= p + l < tr.n else (0, 0) for l in (-1, 0, 1)]
                                                                    for p, tr in zip(peaks, plan.tracks)]), batch_composite_steps=True)
    steps = res.batch_composite_steps.cpu().numpy()
    seg = np.concatenate([[0], np.cumsum([tr.n for tr in plan.tracks])])
    lag0 = (steps[seg[0] + peaks[0]] + steps[seg[1] + peaks[1]] + steps[seg[2] + peaks[2]]) / 3.0
    ens = res.batch_phase_ensemble.cpu().numpy()
    for i, term in enumerate(MAP_TERMS):
        assert np.array_equal(_table(files[f"{term}_dlat_dlon_phase01.csv"]).values, lag0[i]), term
        for b in (0, 2):
            assert np.array_equal(_table(files[f"{term}_dlat_dlon_phase{b:02d}.csv"]).values, ens[b, i], equal_nan=True), (term, b)


@pytest.mark.parametrize("flags, text", [
    (["--batch-composites", "--batch-composites-phase", "peak:1", "--batch-chunk", "4"], "--batch-chunk streams the batch"),
    (["--batch-composites", "--batch-composites-phase", "peak:1", "--gpus", "2"], "--batch-composites runs on one GPU"),
    (["--batch-composites", "--batch-composites-phase", "peak:1", "--ingest", "device"], "--batch-composites prepares the data on the host"),
    (["--batch-composites-phase", "peak:1"], "it goes with --batch-composites"),
])
def test_refusals_leave_nothing(workdir, golden_dir, flags, text):
    import lorenzcycletoolkit
    infile = _setup(workdir, golden_dir, np.float32)
    tracks = [_track_file(workdir / "long.csv", [(T(k), -25.0, -45.0 - k) for k in range(1, 9)]),
              _track_file(workdir / "late.csv", [(T(k), -40.0 + k, -35.0) for k in range(6, 9)])]
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main([infile, "-r", "-t", "--trackfiles", *tracks, *flags])
    assert text in str(e.value)
    assert not os.path.exists("LEC_Results") or not os.listdir("LEC_Results")


def test_tracks_of_two_spacings_are_refused_by_name_with_peak(workdir, golden_dir):
    import lorenzcycletoolkit
    infile = _setup(workdir, golden_dir, np.float32)
    tracks = [_track_file(workdir / "three_hourly.csv", [(T(k), -25.0, -45.0 - k) for k in range(1, 9)]),
              _track_file(workdir / "six_hourly.csv", [(T(k), -30.0 - k // 2, -55.0 + k) for k in range(0, 12, 2)])]
    with pytest.raises(ValueError, match=r"six_hourly.csv: its steps are 6 h apart, those of .*three_hourly.csv 3 h"):
        lorenzcycletoolkit.main([infile, "-r", "-t", "--trackfiles", *tracks, "--batch-composites", "--batch-composites-phase", "peak:1"])
    shutil.rmtree("LEC_Results")


def test_choose_systems_with_lifetime_2(workdir, golden_dir):
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_NCEP-R2"), workdir / "inputs" / "namelist")
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    added, got, log = _added(infile, ["-c", "--choose-systems", "2"], "lifetime:2")
    files = _under(added, os.path.join("testdata_NCEP-R2_choose_batch", "results_composites", "phases"))
    assert len(files) == len(added) and sorted(files) == _phase_names(2)
    listing = pd.read_csv(io.BytesIO(files["phases.csv"]))
    members = pd.read_csv(io.BytesIO(files["phase_members.csv"]))
    assert len(members) == 2 and list(listing["members"]) == [2, 2]
    cells = members[["phase00", "phase01"]].to_numpy()
    assert list(cells.sum(axis=1)) == list(members["steps"]) and list(listing["steps"]) == cells.sum(axis=0).tolist()
    for n, steps in enumerate(members["steps"]):
        assert cells[n].tolist() == [(steps + 1) // 2, steps // 2]
    e = _table(files["Ce_dlat_dlon_phase00.csv"])
    assert e.shape == (7, 7) and np.isfinite(e.values).all() and np.isfinite(_table(files["Ce_sd_dlat_dlon_phase01.csv"]).values).all()
    assert "2 bin(s) over 2 track(s) of 7 x 7 box points" in log
