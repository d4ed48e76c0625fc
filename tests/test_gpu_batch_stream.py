"""The streamed batch on the GPU (``-t --trackfiles --batch-chunk N``, ``ingest.lec_streamed_batch``): every file a track's tree holds
is byte for byte the file the host batch (the same command without the flag) writes -- which test_gpu_batch.py ties to the single
runs --, on a plain classic file, an int16-packed file with fill values and two longitude origins, and deflated NetCDF-4 files
inflated on the device; once against the streamed single runs; and at function level that results do not depend on how a chunk's
records are cut into launches and that the device buffers do not grow with the file."""
import filecmp
import os
import shutil

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import batch, ingest                # noqa: E402
from lorenzcycletoolkit_amd import dataset as ds                # noqa: E402
from lorenzcycletoolkit_amd.synthetic import write_classic_nc   # noqa: E402
from tests.helpers import write_packed_era5_style               # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERA5_NAMELIST = (";Variable;Units\nAir Temperature;t;K\nGeopotential;z;m**2/s**2\nOmega Velocity;w;Pa/s\n"
                 "Eastward Wind Component;u;m/s\nNorthward Wind Component;v;m/s\nLongitude;longitude\nLatitude;latitude\n"
                 "Time;time\nVertical Level;level\n")
NAN_WARNING = "NaN level values were interpolated/dropped"


def _track_file(path, rows, sizes=None):
    head = "time;Lat;Lon" + (";width;length" if sizes else "")
    lines = [head]
    for k, (t, la, lo) in enumerate(rows):
        lines.append(f"{t};{la};{lo}" + (f";{sizes[k][0]};{sizes[k][1]}" if sizes else ""))
    path.write_text("\n".join(lines) + "\n")
    return str(path)


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


def _same_trees(a, b, what):
    files = _tree_files(a)
    assert files == _tree_files(b), what
    assert any(f.endswith("_track_results.csv") for f in files) and any(f.endswith("_track_trackfile") for f in files), what
    for f in files:
        if not f.endswith("/"):
            assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), (what, f)


def _run_batch(workdir, infile, trackfiles, extra, keep):
    """One ``--trackfiles`` run in ``workdir``; its LEC_Results moved to ``workdir/keep``.  Returns (that directory, the log's text)."""
    stem = os.path.basename(infile).split(".nc")[0]
    res = workdir / "LEC_Results"
    assert not res.exists()
    _main([infile, "-r", "-t", "--trackfiles", *trackfiles, *extra])
    log = (res / f"{stem}_track_batch" / f"log.{stem}").read_text()
    dst = workdir / keep
    shutil.move(str(res), str(dst))
    return dst, log


def _same_batches(a, b, infile, trackfiles, what):
    """Every track's tree and batch.csv of two ``--trackfiles`` runs: the same files, the same bytes."""
    stem = os.path.basename(infile).split(".nc")[0]
    listing = pd.read_csv(a / f"{stem}_track_batch" / "batch.csv")
    assert list(listing["trackfile"]) == list(trackfiles)
    assert filecmp.cmp(a / f"{stem}_track_batch" / "batch.csv", b / f"{stem}_track_batch" / "batch.csv", shallow=False), what
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)), what
    for tf in trackfiles:
        tstem = os.path.splitext(os.path.basename(tf))[0]
        _same_trees(a / f"{stem}_{tstem}_track", b / f"{stem}_{tstem}_track", f"{what}: {tstem}")


def _synthetic_tracks(d):
    t = lambda k: (pd.Timestamp("2020-01-01") + pd.Timedelta(hours=3 * k)).strftime("%Y-%m-%d-%H%M")
    return [
        _track_file(d / "six_hourly.csv", [(t(k), -30.0 + 0.4 * k, -55.0 + 0.7 * k) for k in range(0, 12, 2)]),
        _track_file(d / "sized.csv", [(t(k), -25.0, -45.0 - 0.5 * k) for k in range(2, 9)],
                    sizes=[(8 + (k % 3), 10 + (k % 2)) for k in range(7)]),
        _track_file(d / "edge.csv", [(t(k), -52.4, -72.3 + 0.5 * k) for k in range(4, 11)]),     # its box meets the data's edge
    ]


_CASES = {}


@pytest.fixture
def synthetic_case(request, tmp_path_factory, golden_dir, monkeypatch):
    """(workdir, infile, track files, the host batch's results) of the synthetic file in one storage dtype: written and run once."""
    dtype, extra = request.param
    key = np.dtype(dtype).name
    if key not in _CASES:
        work = tmp_path_factory.mktemp(f"stream_{key}")
        os.makedirs(work / "inputs")
        shutil.copy(os.path.join(golden_dir, "inputs", "namelist_ERA5"), work / "inputs" / "namelist")
        infile = str(work / f"synth_{key}.nc")
        write_classic_nc(infile, dtype)
        tracks = _synthetic_tracks(work)
        monkeypatch.chdir(work)
        host, _ = _run_batch(work, infile, tracks, extra, "host_batch")
        _CASES[key] = (work, infile, tracks, host)
    work = _CASES[key][0]
    monkeypatch.chdir(work)
    yield _CASES[key] + (extra,)
    shutil.rmtree(work / "streamed", ignore_errors=True)
    shutil.rmtree(work / "LEC_Results", ignore_errors=True)


SYNTHETIC = [(np.float32, []), (np.float64, ["-z"])]


@pytest.mark.parametrize("n_chunk", [1, 2, 5, 100])
@pytest.mark.parametrize("synthetic_case", SYNTHETIC, indirect=True, ids=["float32", "float64-z"])
def test_cli_streamed_batch_equals_the_host_batch_synthetic(synthetic_case, n_chunk):
    """N = 1 and 2: a track's time neighbour lies in another chunk, tracks start and end inside a chunk, and there are chunks in which a
    track or a whole group has no record."""
    work, infile, tracks, host, extra = synthetic_case
    got, log = _run_batch(work, infile, tracks, [*extra, "--batch-chunk", str(n_chunk)], "streamed")
    _same_batches(host, got, infile, tracks, f"--batch-chunk {n_chunk}")
    n_union = 10
    assert f"{-(-n_union // n_chunk)} chunk(s) of {min(n_chunk, n_union)} step(s)" in log and "bytes) over the link" in log
    assert log.count("chunk(s) of") == 1


@pytest.mark.parametrize("synthetic_case", SYNTHETIC[:1], indirect=True, ids=["float32"])
def test_cli_streamed_batch_equals_the_streamed_single_runs(synthetic_case):
    work, infile, tracks, host, extra = synthetic_case
    stem = os.path.basename(infile).split(".nc")[0]
    got, _ = _run_batch(work, infile, tracks, [*extra, "--batch-chunk", "2"], "streamed")
    for tf in tracks:
        _main([infile, "-r", "-t", "--trackfile", tf, "--device-ingest", *extra])
        tstem = os.path.splitext(os.path.basename(tf))[0]
        _same_trees(work / "LEC_Results" / f"{stem}_track", got / f"{stem}_{tstem}_track", f"-t --trackfile {tstem} --device-ingest")
        shutil.rmtree(work / "LEC_Results")


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    monkeypatch.chdir(tmp_path)
    return tmp_path


def test_cli_streamed_batch_decodes_packed_data_and_keeps_nan_on_two_longitude_origins(workdir):
    """int16 with scale / offset / fill values, lon 0..357.5, lat N -> S, a 5-hPa level that is dropped; one track in the Atlantic, one
    across the +-180 meridian (its own pass on the 0..360 axis).  v is all fill at 50 hPa at one step and at one interior point."""
    (workdir / "inputs" / "namelist").write_text(ERA5_NAMELIST)
    infile = str(workdir / "packed.nc")
    write_packed_era5_style(infile, fill=True)
    t = lambda k: (pd.Timestamp("2020-01-01") + pd.Timedelta(hours=6 * k)).strftime("%Y-%m-%d-%H%M")
    tracks = [
        _track_file(workdir / "atlantic.csv", [(t(k), 30.0 + 1.0 * k, 45.0 + 2.0 * k) for k in range(0, 7)]),      # holds the interior fill point (35 N, 50 E)
        _track_file(workdir / "dateline.csv", [(t(k), -20.0 - 1.5 * k, ((170.0 + 5.0 * k + 180.0) % 360.0) - 180.0) for k in range(1, 6)]),
    ]
    host, host_log = _run_batch(workdir, infile, tracks, [], "host_batch")
    assert "2 pass(es) over the data" in host_log
    got, log = _run_batch(workdir, infile, tracks, ["--batch-chunk", "3"], "streamed")
    _same_batches(host, got, infile, tracks, "--batch-chunk 3")
    assert "2 pass(es) over the data" in log and log.count("chunk(s) of 3 step(s)") == 2
    for tf in tracks:
        said = lambda text: any(tf in line and NAN_WARNING in line for line in text.splitlines())
        assert said(log) == said(host_log), tf
    assert NAN_WARNING in host_log               # (the case has what it is there for)


def _sized_tracks(d, hours, n):
    stamp = lambda t: (pd.Timestamp("2020-01-01") + pd.Timedelta(hours=hours * t)).strftime("%Y-%m-%d-%H%M")
    return [
        _track_file(d / "whole.csv", [(stamp(t), -10 + 5 * t, -30 + 10 * t) for t in range(n)], sizes=[(60, 50)] * n),
        _track_file(d / "short.csv", [(stamp(t), 5 - 5 * t, -20 + 5 * t) for t in range(1, n - 1)], sizes=[(50, 40)] * (n - 2)),      # shorter than the file
    ]


def test_cli_streamed_batch_inflates_on_the_device_cds_layout(workdir):
    """float32 + shuffle + deflate, NaN _FillValue, hourly `valid_time`, `pressure_level` descending: the chunks cross the link
    compressed and lec_inflate rebuilds them; --inflate host gives the same bytes."""
    shutil.copy(os.path.join(ROOT, "inputs", "namelist_ERA5-copernicus-new"), workdir / "inputs" / "namelist")
    infile = os.path.join(ROOT, "tests", "golden", "hdf5", "cds_new_layout.nc")
    tracks = _sized_tracks(workdir, 1, 5)
    host, host_log = _run_batch(workdir, infile, tracks, [], "host_batch")
    got, log = _run_batch(workdir, infile, tracks, ["--batch-chunk", "2"], "streamed")
    _same_batches(host, got, infile, tracks, "--batch-chunk 2")
    assert "inflate device" in log
    for tf in tracks:
        said = lambda text: any(tf in line and NAN_WARNING in line for line in text.splitlines())
        assert said(log) == said(host_log), tf
    again, log = _run_batch(workdir, infile, tracks, ["--batch-chunk", "2", "--inflate", "host"], "streamed_host_inflate")
    _same_batches(host, again, infile, tracks, "--batch-chunk 2 --inflate host")
    assert "inflate host" in log


def test_cli_streamed_batch_inflates_chunks_of_two_time_steps(workdir):
    """packed_timechunk2_latest.nc: int16, deflated chunks of 2 time steps x 2 levels x 5 latitudes; --batch-chunk 3 cuts the union
    where the file's time chunks do not end."""
    (workdir / "inputs" / "namelist").write_text(ERA5_NAMELIST)
    infile = os.path.join(ROOT, "tests", "golden", "hdf5", "packed_timechunk2_latest.nc")
    tracks = _sized_tracks(workdir, 6, 5)
    host, _ = _run_batch(workdir, infile, tracks, [], "host_batch")
    got, log = _run_batch(workdir, infile, tracks, ["--batch-chunk", "3"], "streamed")
    _same_batches(host, got, infile, tracks, "--batch-chunk 3")
    assert "inflate device" in log and "2 chunk(s) of 3 step(s)" in log


# ---------------------------------------------------------------------------------------------------------------------- function level
def _open_and_plan(infile, tracks):
    df = ds.read_namelist("inputs/namelist")
    raw = ds.open_raw(infile, df)
    return raw, df, batch.plan_batch(raw.lat, raw.lon, raw.level, raw.time, raw.level_units, raw.names, tracks)


def _equal(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_results_do_not_depend_on_how_records_are_cut_into_launches(workdir, golden_dir):
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_ERA5"), workdir / "inputs" / "namelist")
    infile = str(workdir / "synth.nc")
    write_classic_nc(infile, np.float32)
    raw, df, plan = _open_and_plan(infile, _synthetic_tracks(workdir))
    try:
        runs = {}
        for cap in (1, 3, None):
            st = {}
            res = ingest.lec_streamed_batch(raw, plan, df, chunk_steps=4, device="cuda:0", max_records=cap, stats=st)
            torch.cuda.synchronize()
            assert [int(r.packed.shape[0]) for r in res] == [tr.n for tr in plan.tracks] and st["chunks"] == 3
            assert max(st["records_per_launch"].values()) <= (cap or 10 ** 9)
            runs[cap] = res
        for cap in (1, 3):
            for k, (a, b) in enumerate(zip(runs[cap], runs[None])):
                assert _equal(a.packed, b.packed) and torch.equal(a.nanflag, b.nanflag), (cap, k)
        assert all(torch.isfinite(r.scalars[:, :4]).all() for r in runs[None])
    finally:
        raw.close()


def test_device_buffers_do_not_grow_with_the_file(workdir, golden_dir):
    """The same tracks at the same times in a 12-step and in a 48-step file: the same device buffers, and every field but T is staged
    once per union step (T also for the neighbours a chunk's records name in other chunks)."""
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_ERA5"), workdir / "inputs" / "namelist")
    tracks = _synthetic_tracks(workdir)
    seen = {}
    for nt in (12, 48):
        infile = str(workdir / f"synth_{nt}.nc")
        write_classic_nc(infile, np.float32, nt=nt)
        raw, df, plan = _open_and_plan(infile, tracks)
        try:
            st = {}
            ingest.lec_streamed_batch(raw, plan, df, chunk_steps=4, device="cuda:0", stats=st)
            torch.cuda.synchronize()
        finally:
            raw.close()
        n_union = len(plan.tpos)
        assert n_union == 10 and st["chunks"] == 3 and st["chunk_steps"] == 4
        assert {k: v for k, v in st["staged_steps"].items() if k != "tair"} == {"u": n_union, "v": n_union, "omega": n_union, "geopt": n_union}
        named = sum(len(ch.t_steps) for ch in batch.plan_chunks(plan, 4))
        assert st["staged_steps"]["tair"] == named and n_union < named <= 3 * n_union
        seen[nt] = st
    assert seen[12]["device_buffer_bytes"] == seen[48]["device_buffer_bytes"] > 0
    assert seen[12]["bytes_moved"] == seen[48]["bytes_moved"] > 0
    for k in ("chunks", "chunk_steps", "bytes_moved", "device_buffer_bytes", "inflate", "staging", "staged_steps"):
        assert k in seen[12], k
