"""-t --trackfiles / -c --choose-systems --batch-composites on the command line (GPU).  Every track's results_composites/ is byte for
byte that of the track's own ``-t --trackfile --composites`` run; every other file of the run is byte for byte that of the run without
the flag; the ensemble files in the batch directory parse back (repr(float) round-trips) to the in-order mean of the tracks' own files,
and to the API's numbers; composites.csv lists the tracks; tracks of two box shapes give two ensemble directories."""
import io
import os
import shutil

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd.constants import MAP_TERMS
from lorenzcycletoolkit_amd.synthetic import write_classic_nc

NAMES = sorted([f"{t}_dlat_dlon.csv" for t in MAP_TERMS] + [f"{t}_dlon.csv" for t in MAP_TERMS])
ENSEMBLE = sorted([f"{t}_dlat_dlon.csv" for t in MAP_TERMS] + ["composites.csv"])


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return tmp_path


def _tree():
    """{relative path: bytes} of everything under LEC_Results but the logs, and the logs' text; the tree is removed."""
    out, logs = {}, ""
    for base, _, files in os.walk("LEC_Results"):
        for f in files:
            p = os.path.join(base, f)
            if f.startswith("log."):
                logs += open(p).read()
            else:
                out[os.path.relpath(p, "LEC_Results")] = open(p, "rb").read()
    shutil.rmtree("LEC_Results")
    return out, logs


def _main(argv):
    import lorenzcycletoolkit
    lorenzcycletoolkit.main(argv)
    return _tree()


def _table(blob):
    return pd.read_csv(io.BytesIO(blob), index_col=0, float_precision="round_trip")


def _track_file(path, rows, size=None):
    lines = ["time;Lat;Lon" + (";width;length" if size else "")]
    lines += [f"{t};{la};{lo}" + (f";{size[0]};{size[1]}" if size else "") for t, la, lo in rows]
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def _under(tree, prefix):
    prefix = prefix.rstrip(os.sep) + os.sep
    return {k[len(prefix):]: v for k, v in tree.items() if k.startswith(prefix)}


def _check_batch(infile, stem, trackfiles, batch_flags, batch_name, groups):
    """The batch with --batch-composites against the batch without it and against every track's own --composites run.  ``groups``:
    [[track stems]], the ensembles expected, each of the box shape its members' own files have.  Returns the run's log."""
    own = {}
    for tf in trackfiles:
        tree, _ = _main([infile, "-r", "-t", "--trackfile", tf, "--composites"])
        own[os.path.splitext(os.path.basename(tf))[0]] = _under(tree, os.path.join(f"{stem}_track", "results_composites"))
        assert sorted(own[os.path.splitext(os.path.basename(tf))[0]]) == NAMES
    plain, _ = _main([infile, "-r", *batch_flags])
    got, log = _main([infile, "-r", *batch_flags, "--batch-composites"])
    added = {k: v for k, v in got.items() if k not in plain}
    assert sorted(k for k in got if k not in added) == sorted(plain)
    for k, v in plain.items():
        assert got[k] == v, f"{k} differs from the run without --batch-composites"
    # every track's tree: the files of its own --composites run, byte for byte
    for tstem, files in own.items():
        mine = _under(added, os.path.join(f"{stem}_{tstem}_track", "results_composites"))
        assert sorted(mine) == NAMES, tstem
        for name in NAMES:
            assert mine[name] == files[name], (tstem, name)
    # the ensembles
    shapes = {_table(own[members[0]]["Ae_dlat_dlon.csv"]).shape: members for members in groups}
    assert len(shapes) == len(groups)
    dirs = {("results_composites" if len(shapes) == 1 else f"results_composites_{h}x{w}"): (h, w, members) for (h, w), members in shapes.items()}
    left = {k for k in added if k.startswith(batch_name + os.sep)}
    assert sorted({k.split(os.sep)[1] for k in left}) == sorted(dirs)
    assert len(added) == len(left) + 12 * len(own)
    for d, (h, w, members) in dirs.items():
        ens = _under(added, os.path.join(batch_name, d))
        assert sorted(ens) == ENSEMBLE, d
        listing = pd.read_csv(io.BytesIO(ens["composites.csv"]))
        assert [os.path.splitext(os.path.basename(p))[0] for p in listing["trackfile"]] == members
        assert list(listing["rows"]) == [h] * len(members) and list(listing["columns"]) == [w] * len(members)
        assert list(listing["steps"]) == [len(_table(own[m]["Ae_dlon.csv"])) for m in members]
        assert list(listing["nan_points"]) == [sum(int(np.isnan(_table(own[m][f"{t}_dlat_dlon.csv"]).values).sum()) for t in MAP_TERMS)
                                               for m in members]
        assert list(listing["results_directory"]) == [os.path.join("./LEC_Results/", f"{stem}_{m}_track") for m in members]
        for term in MAP_TERMS:
            e = _table(ens[f"{term}_dlat_dlon.csv"])
            first = _table(own[members[0]][f"{term}_dlat_dlon.csv"])
            assert e.shape == (h, w) and e.index.name == "dlat" and list(e.index) == list(first.index) and list(e.columns) == list(first.columns)
            s = first.values.copy()
            for m in members[1:]:
                s = s + _table(own[m][f"{term}_dlat_dlon.csv"]).values
            assert np.array_equal(e.values, s / float(len(members))), (d, term)      # the in-order mean of the tracks' own files
        assert f"{len(members)} track(s) of {h} x {w} box points" in log
    return log


def test_synthetic_file_three_tracks_and_two_shapes(workdir, golden_dir):
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_ERA5"), workdir / "inputs" / "namelist")
    infile = str(workdir / "synth.nc")
    write_classic_nc(infile, np.float32)
    t = lambda k: (pd.Timestamp("2020-01-01") + pd.Timedelta(hours=3 * k)).strftime("%Y-%m-%d-%H%M")
    tracks = [
        _track_file(workdir / "six_hourly.csv", [(t(k), -30.0 - k // 2, -55.0 + k) for k in range(0, 12, 2)]),
        _track_file(workdir / "three_hourly.csv", [(t(k), -25.0, -45.0 - k) for k in range(1, 9)]),
        _track_file(workdir / "late.csv", [(t(k), -40.0 + k, -35.0) for k in range(6, 9)]),
    ]
    flags = ["-t", "--trackfiles", *tracks]
    log = _check_batch(infile, "synth", tracks, flags, "synth_track_batch", [["six_hourly", "three_hourly", "late"]])
    assert "--ingest auto resolves to host" in log
    # a fourth track of another box shape: one ensemble directory per shape
    small = _track_file(workdir / "small.csv", [(t(k), -35.0, -60.0 + k) for k in range(2, 7)], size=(9, 7))
    _check_batch(infile, "synth", [tracks[0], small], ["-t", "--trackfiles", tracks[0], small], "synth_track_batch",
                 [["six_hourly"], ["small"]])


def test_ensemble_is_the_api_s(workdir, golden_dir):
    """The ensemble file holds ``LECEngine.compute(batch_composites=...)``'s numbers on the same host-prepared union."""
    from types import SimpleNamespace
    from lorenzcycletoolkit_amd import batch
    from lorenzcycletoolkit_amd import dataset as ds
    from lorenzcycletoolkit_amd.engine import LECEngine
    from lorenzcycletoolkit_amd.frameworks import host_fields
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_ERA5"), workdir / "inputs" / "namelist")
    infile = str(workdir / "synth.nc")
    write_classic_nc(infile, np.float64)
    t = lambda k: (pd.Timestamp("2020-01-01") + pd.Timedelta(hours=3 * k)).strftime("%Y-%m-%d-%H%M")
    tracks = [_track_file(workdir / "a.csv", [(t(k), -30.0, -55.0 + k) for k in range(0, 8, 2)]),
              _track_file(workdir / "b.csv", [(t(k), -28.0 - k, -40.0) for k in range(3, 6)])]
    got, _ = _main([infile, "-r", "-t", "--trackfiles", *tracks, "--batch-composites"])
    data, plan = batch.prepare_union(SimpleNamespace(infile=infile, mpas=False), tracks, "inputs/namelist")
    df = ds.read_namelist("inputs/namelist")
    arrays, common, phi_scale = host_fields(data, df)
    eng = LECEngine(data.lat, data.lon, data.level, device="cuda:0")
    cubes = [torch.as_tensor(np.ascontiguousarray(a, dtype=common)).to("cuda:0") for a in arrays]
    assert list(plan.groups) == [(16, 16, True)]
    boxes = [b for tr in plan.tracks for b in tr.boxes]
    res = eng.compute(*cubes, eng.prepare_boxes(boxes, nyb_min=16, lon_uniform=True), phi_scale=phi_scale, per_step_boxes=True,
                      drop_any_time=False, steps=torch.as_tensor(np.concatenate([tr.steps for tr in plan.tracks])).to("cuda:0"),
                      tcoef=torch.as_tensor(np.concatenate([tr.tcoef for tr in plan.tracks])).to("cuda:0"), batch_composites=[4, 3])
    ens, mean = res.batch_composite_ensemble.cpu().numpy(), res.batch_composite_mean.cpu().numpy()
    for i, term in enumerate(MAP_TERMS):
        assert np.array_equal(_table(got[os.path.join("synth_track_batch", "results_composites", f"{term}_dlat_dlon.csv")]).values, ens[i]), term
        for k, name in enumerate("ab"):
            assert np.array_equal(_table(got[os.path.join(f"synth_{name}_track", "results_composites", f"{term}_dlat_dlon.csv")]).values, mean[k, i])


def test_ncep_sample_and_a_shifted_copy(workdir, golden_dir):
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_NCEP-R2"), workdir / "inputs" / "namelist")
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    base = pd.read_csv(os.path.join(golden_dir, "inputs", "track_testdata_NCEP-R2"), sep=";")
    tracks = [str(shutil.copy(os.path.join(golden_dir, "inputs", "track_testdata_NCEP-R2"), workdir / "track_testdata"))]
    shifted = base.copy()
    shifted["Lon"] += 2.5                   # one grid step of the sample
    shifted.to_csv(workdir / "track_shifted", sep=";", index=False)
    tracks.append(str(workdir / "track_shifted"))
    _check_batch(infile, "testdata_NCEP-R2", tracks, ["-t", "--trackfiles", *tracks], "testdata_NCEP-R2_track_batch",
                 [["track_testdata", "track_shifted"]])


def test_choose_systems_writes_what_the_written_tracks_own_runs_write(workdir, golden_dir):
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_NCEP-R2"), workdir / "inputs" / "namelist")
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    stem = "testdata_NCEP-R2"
    import lorenzcycletoolkit
    lorenzcycletoolkit.main([infile, "-r", "-c", "--choose-systems", "2", "--batch-composites"])
    batch_dir = os.path.join("LEC_Results", f"{stem}_choose_batch")
    written = {}
    for n in (1, 2):
        written[n] = str(shutil.copy(os.path.join(batch_dir, f"choose_s{n:02d}"), workdir / f"choose_s{n:02d}"))
    got, log = _tree()
    assert sorted(_under(got, os.path.join(f"{stem}_choose_batch", "results_composites"))) == ENSEMBLE
    assert "2 track(s) of 7 x 7 box points" in log
    for n, tf in written.items():
        own, _ = _main([infile, "-r", "-t", "--trackfile", tf, "--composites"])
        own = _under(own, os.path.join(f"{stem}_track", "results_composites"))
        mine = _under(got, os.path.join(f"{stem}_choose_s{n:02d}_track", "results_composites"))
        assert sorted(mine) == NAMES == sorted(own)
        for name in NAMES:
            assert mine[name] == own[name], (n, name)
