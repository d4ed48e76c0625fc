"""``--series`` through the command line: a run over the parts of a series (3 + 1 + 3 time steps, each part int16-packed with its own
scale_factor / add_offset, tests/series_cases.py) writes the bytes of the run over ONE merged file of the same name that holds the
per-part decoded values -- every CSV, every per-level table and every track file; the log is left out (it carries the command line).
In-process ``main(argv)`` as tests/test_gpu_cli.py runs it; the sharded case starts the rank processes as tests/test_gpu_cli_sharded.py does."""
import io
import os
import shutil
import subprocess
import sys

import pandas as pd
import pytest

torch = pytest.importorskip("torch")

from tests import series_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BASELINES = {}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    root = tmp_path_factory.mktemp("cli_series")
    parts, merged, _, _ = sc.standard_case(root)
    os.makedirs(root / "inputs")
    (root / "inputs" / "namelist").write_text(sc.NAMELIST)
    (root / "inputs" / "box_limits").write_text("min_lon;-60\nmax_lon;20\nmin_lat;-45\nmax_lat;30\n")
    t = lambda k: (pd.Timestamp("2020-01-01") + pd.Timedelta(hours=6 * k)).strftime("%Y-%m-%d-%H%M")
    track = lambda name, rows: (root / name).write_text("time;Lat;Lon\n" + "".join(f"{a};{b};{c}\n" for a, b, c in rows)) and str(root / name)
    # all seven steps, over the interior fill point (35 N, 50 E) of step 4; a shorter one elsewhere
    tracks = [track("atlantic.csv", [(t(k), 30.0 + 1.0 * k, 45.0 + 2.0 * k) for k in range(7)]),
              track("south.csv", [(t(k), -20.0 - 1.5 * k, -40.0 + 5.0 * k) for k in range(1, 6)])]
    shutil.copy(tracks[0], root / "inputs" / "track")
    return dict(root=root, parts=parts, merged=merged, tracks=tracks)


@pytest.fixture
def work(case, monkeypatch):
    monkeypatch.chdir(case["root"])
    yield case
    shutil.rmtree(case["root"] / "LEC_Results", ignore_errors=True)


def _tree():
    """{relative path: bytes} of everything under LEC_Results but the logs, then the tree is removed."""
    out = {}
    for base, _, files in os.walk("LEC_Results"):
        for f in files:
            if not f.startswith("log."):
                out[os.path.relpath(os.path.join(base, f), "LEC_Results")] = open(os.path.join(base, f), "rb").read()
    logs = "".join(open(os.path.join(base, f)).read() for base, _, files in os.walk("LEC_Results") for f in files if f.startswith("log."))
    shutil.rmtree("LEC_Results")
    return out, logs


def _main(argv):
    import lorenzcycletoolkit
    lorenzcycletoolkit.main(argv)
    return _tree()


def _merged(case, flags, key=None):
    """The merged run's files for these flags (run once per module)."""
    key = key or (case["merged"],) + tuple(flags)
    if key not in _BASELINES:
        _BASELINES[key] = _main([key[0]] + list(flags))[0]
        assert _BASELINES[key], flags
    return _BASELINES[key]


def _same(one, two, what):
    assert sorted(one) == sorted(two), what
    for k in one:
        assert one[k] == two[k], f"{what}: {k} differs from the merged run's"


def _series_argv(case, flags):
    p = case["parts"]
    return [p[0]] + list(flags) + ["--series", p[2], p[1], p[0]]        # any order, infile named again


@pytest.fixture
def chunks_of_two(monkeypatch):
    """The streamed path with two time steps per chunk (``prepare_streamed``'s ``chunk_steps``): over parts of 3 + 1 + 3 steps the chunks
    are [0, 1) [1, 3) [3, 5) [5, 7) -- the first seam lies on a chunk boundary (T's halo step comes from the other file), the second
    inside a chunk.  Also counts the gathers by the call they took."""
    from lorenzcycletoolkit_amd import ingest
    real_prepare, real_call = ingest.prepare_streamed, ingest._ingest_call
    calls = {"series": 0, "plain": 0}

    def counted(lib, v, *a, **k):
        calls["plain" if v.uniform_packing else "series"] += 1
        return real_call(lib, v, *a, **k)
    monkeypatch.setattr(ingest, "prepare_streamed", lambda *a, **k: real_prepare(*a, **{**k, "chunk_steps": 2}))
    monkeypatch.setattr(ingest, "_ingest_call", counted)
    return calls


def test_fixed_framework_host(work):
    got, _ = _main(_series_argv(work, ["-r", "-f", "--ingest", "host"]))
    _same(_merged(work, ["-r", "-f", "--ingest", "host"]), got, "-f --ingest host")
    assert "era5_1_fixed/era5_1_fixed_results.csv" in got and len(got) == 22


def test_fixed_framework_device_with_a_seam_inside_a_chunk_and_one_on_a_boundary(work, chunks_of_two):
    want = _merged(work, ["-r", "-f", "--ingest", "host"])
    got, log = _main(_series_argv(work, ["-r", "-f", "--ingest", "device"]))
    _same(want, got, "-f --ingest device")
    assert "4 chunk(s) of 2 step(s), staging staged" in log and chunks_of_two["series"] == 4 * 5 and chunks_of_two["plain"] == 0
    assert "NaN level values" in log


def test_moving_framework_host(work):
    got, _ = _main(_series_argv(work, ["-r", "-t", "--ingest", "host"]))
    _same(_merged(work, ["-r", "-t", "--ingest", "host"]), got, "-t --ingest host")
    assert "era5_1_track/era5_1_track_trackfile" in got


def test_moving_framework_device_gathers_t_of_the_neighbouring_steps_across_both_seams(work, chunks_of_two):
    """The box-packed layout: T(t - 1) and T(t + 1) of the one-step part come from the other two files."""
    want = _merged(work, ["-r", "-t", "--ingest", "host"])
    got, log = _main(_series_argv(work, ["-r", "-t", "--ingest", "device"]))
    _same(want, got, "-t --ingest device")
    assert chunks_of_two["series"] > 0 and chunks_of_two["plain"] == 0 and "staging staged" in log


def test_choose_writes_the_track_and_the_analysis_of_the_merged_run(work):
    flags = ["-r", "-c", "--choose-start", "0", "45", "--choose-search", "2.5"]
    got, _ = _main(_series_argv(work, flags))
    _same(_merged(work, flags), got, "-c")
    assert "era5_1_choose/era5_1_choose_track" in got


def test_choose_in_chunks_of_two_steps(work):
    flags = ["-r", "-c", "--choose-start", "0", "45", "--choose-search", "2.5"]
    got, _ = _main(_series_argv(work, flags + ["--choose-chunk", "2"]))
    _same(_merged(work, flags), got, "-c --choose-chunk 2")


def test_batch_of_tracks_streamed_in_chunks(work, chunks_of_two):
    flags = ["-r", "-t", "--trackfiles", *work["tracks"], "--batch-chunk", "2"]
    want = _merged(work, flags)
    assert chunks_of_two["series"] == 0 and chunks_of_two["plain"] > 0            # (the merged file: one packing, the plain call)
    got, _ = _main(_series_argv(work, flags))
    _same(want, got, "-t --trackfiles --batch-chunk 2")
    assert chunks_of_two["series"] > 0 and "era5_1_atlantic_track/era5_1_track_results.csv" in got
    host, _ = _main(_series_argv(work, flags[:-2]))                                # ... and the host-prepared batch of the series
    _same(want, host, "-t --trackfiles")


def test_parts_with_one_packing_take_the_plain_call(work, chunks_of_two, tmp_path):
    parts, packed = sc.write_series(tmp_path / "parts", same_packing=True)
    merged = str(tmp_path / "merged" / os.path.basename(parts[0]))
    sc.write_merged(merged, packed)
    want, _ = _main([merged, "-r", "-f", "--ingest", "host"])
    got, _ = _main([parts[0], "-r", "-f", "--ingest", "device", "--series", *parts[1:]])
    _same(want, got, "one packing")
    assert chunks_of_two["series"] == 0 and chunks_of_two["plain"] == 4 * 5


def test_fixed_framework_device_on_two_ranks(work, tmp_path):
    """Parts of 2 + 3 + 2 steps over two ranks: whichever way seven steps are shared (3 + 4 or 4 + 3), the shards are cut inside the
    middle part, so each rank has a seam of its own inside its block or at its halo.  The ranks share the GPU and meet over gloo."""
    cuts = (2, 3, 2)
    parts, packed = sc.write_series(tmp_path / "parts", cuts=cuts)
    merged = str(tmp_path / "merged" / os.path.basename(parts[0]))
    sc.write_merged(merged, packed, cuts=cuts)
    want, _ = _main([merged, "-r", "-f", "--ingest", "host"])
    env = dict(os.environ, LEC_DIST_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "LEC_FORCE_SHARD"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "lorenzcycletoolkit.py"), parts[0], "-r", "-f", "--ingest", "device", "--gpus", "2",
                        "--series", parts[2], parts[1]], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    got, log = _tree()
    assert "Time-sharded run: 2 ranks" in log
    _same(want, got, "--gpus 2")


def test_deflated_netcdf4_parts_are_inflated_on_the_host_and_say_so(work, chunks_of_two, tmp_path):
    """Two shuffled + deflated NetCDF-4 parts, the second packing T with another scale_factor: the streamed run stages what the reader
    inflates on the host (no device inflate for a series), decodes T through the table call, and writes the host preparation's bytes."""
    src = os.path.join(ROOT, "tests", "golden", "hdf5", "packed_chunked_tracked.nc")
    later = sc.later_copy_of_hdf5(src, tmp_path / "parts" / "later.nc", 30, rescale_t=1.5)
    (work["root"] / "inputs" / "box_limits").write_text("min_lon;-60\nmax_lon;30\nmin_lat;-40\nmax_lat;30\n")
    try:
        want, host_log = _main([src, "-r", "-f", "--ingest", "host", "--series", later])
        got, log = _main([src, "-r", "-f", "--ingest", "device", "--series", later])
    finally:
        (work["root"] / "inputs" / "box_limits").write_text("min_lon;-60\nmax_lon;20\nmin_lat;-45\nmax_lat;30\n")
    _same(want, got, "deflated parts, --ingest device")
    assert len(pd.read_csv(io.BytesIO(got["packed_chunked_tracked_fixed/packed_chunked_tracked_fixed_results.csv"]))) == 10
    assert "inflated by the reader on the host" in log and "staging staged, inflate host" in log and "being inflated on the host" in host_log
    assert chunks_of_two["series"] > 0 and chunks_of_two["plain"] > 0          # T through the table call, the other fields through the plain one
