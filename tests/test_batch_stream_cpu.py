"""The streamed batch (``-t --trackfiles --batch-chunk N``) without a GPU: what the command line refuses before anything is created, that
the flag reaches the batch run, and ``batch.plan_chunks`` against a plain restatement (loops over tracks and steps, written here) on
the three tracks of test_gpu_batch.py::test_cli_batch_matches_single_runs_synthetic."""
import os

import numpy as np
import pandas as pd
import pytest

from lorenzcycletoolkit_amd import batch

# the grid of synthetic.write_classic_nc: 12 three-hourly steps, 7 levels in hPa, lat N -> S, 1 degree
LAT = np.arange(-10.0, -60.5, -1.0)
LON = np.arange(-80.0, -19.5, 1.0)
LEV = np.array([1000, 925, 850, 700, 500, 300, 200])
TIME = np.datetime64("2020-01-01T00:00", "ns") + np.arange(12) * np.timedelta64(3, "h")
NAMES = {"Vertical Level": "level"}
# file steps of the three tracks: six-hourly over the 3-hourly data, per-step sizes, a box at the data's edge
KS = [list(range(0, 12, 2)), list(range(2, 9)), list(range(4, 11))]


def _stamp(k):
    return (pd.Timestamp("2020-01-01") + pd.Timedelta(hours=3 * k)).strftime("%Y-%m-%d-%H%M")


def _track_file(path, rows, sizes=None):
    head = "time;Lat;Lon" + (";width;length" if sizes else "")
    lines = [head]
    for k, (t, la, lo) in enumerate(rows):
        lines.append(f"{t};{la};{lo}" + (f";{sizes[k][0]};{sizes[k][1]}" if sizes else ""))
    path.write_text("\n".join(lines) + "\n")
    return str(path)


@pytest.fixture
def tracks(tmp_path):
    return [
        _track_file(tmp_path / "six_hourly.csv", [(_stamp(k), -30.0 + 0.4 * k, -55.0 + 0.7 * k) for k in KS[0]]),
        _track_file(tmp_path / "sized.csv", [(_stamp(k), -25.0, -45.0 - 0.5 * k) for k in KS[1]],
                    sizes=[(8 + (k % 3), 10 + (k % 2)) for k in range(7)]),
        _track_file(tmp_path / "edge.csv", [(_stamp(k), -52.4, -72.3 + 0.5 * k) for k in KS[2]]),
    ]


# ------------------------------------------------------------------------------------------------------------------ the command line
BATCH = ["-t", "--trackfiles"]
SYSTEMS = ["-c", "--choose-systems", "2"]


@pytest.mark.parametrize("argv,words", [
    (["-f", "--batch-chunk", "4"], "--batch-chunk goes with --trackfiles"),
    (["-t", "--trackfile", "TRACK0", "--batch-chunk", "4"], "--batch-chunk goes with --trackfiles"),
    (["-c", "--batch-chunk", "4"], "--batch-chunk goes with --trackfiles"),
    (BATCH + ["TRACKS", "--batch-chunk", "0"], "--batch-chunk must be >= 1"),
    (SYSTEMS + ["--batch-chunk", "-3"], "--batch-chunk must be >= 1"),
    (BATCH + ["TRACKS", "--batch-chunk", "4", "--ingest", "host"], "--ingest host"),
    (SYSTEMS + ["--batch-chunk", "4", "--ingest", "host"], "--ingest host"),
    (BATCH + ["TRACKS", "--batch-chunk", "4", "--gpus", "2"], "--trackfiles runs on one GPU: --gpus > 1 is not supported for a batch of tracks"),
    (SYSTEMS + ["--batch-chunk", "4", "--gpus", "2"], "-c/--choose follows the systems on one GPU"),
    # without the flag the device ingest of a batch stays refused, in the words it was refused with
    (BATCH + ["TRACKS", "--ingest", "device"], "--trackfiles prepares the data on the host: --ingest device / --device-ingest is not supported for a batch of tracks"),
    (BATCH + ["TRACKS", "--device-ingest"], "--trackfiles prepares the data on the host: --ingest device / --device-ingest is not supported for a batch of tracks"),
    (SYSTEMS + ["--ingest", "device"], "-c --choose-systems / --choose-starts prepares the data on the host: --ingest device / --device-ingest is not supported"),
    (SYSTEMS + ["--device-ingest"], "-c --choose-systems / --choose-starts prepares the data on the host: --ingest device / --device-ingest is not supported"),
])
def test_cli_refusals(tmp_path, monkeypatch, tracks, argv, words):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    before = sorted(os.listdir(tmp_path))
    full = []
    for a in argv:
        full += tracks if a == "TRACKS" else [tracks[0] if a == "TRACK0" else a]
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", *full])
    assert words in str(e.value), str(e.value)
    assert sorted(os.listdir(tmp_path)) == before          # refused before anything was created


@pytest.mark.parametrize("argv", [BATCH + ["TRACKS", "--batch-chunk", "4"], BATCH + ["TRACKS", "--batch-chunk", "4", "--ingest", "device"],
                                  BATCH + ["TRACKS", "--batch-chunk", "4", "--device-ingest"], SYSTEMS + ["--batch-chunk", "4"],
                                  SYSTEMS + ["--choose-threshold", "-5e-5", "--choose-lifecycle", "--choose-chunk", "3", "--choose-periodic",
                                             "--batch-chunk", "4", "--ingest", "device"],
                                  ["-c", "--choose-starts", "TRACK0", "--batch-chunk", "1"]])
def test_cli_hands_the_flag_to_the_batch_run(tmp_path, monkeypatch, tracks, argv):
    """Accepted with a batch of either kind (--ingest device means the same): the flag arrives where the batch is analysed."""
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    seen = []
    monkeypatch.setattr(lorenzcycletoolkit, "run_batch", lambda args, *rest: seen.append(args))
    full = []
    for a in argv:
        full += tracks if a == "TRACKS" else [tracks[0] if a == "TRACK0" else a]
    lorenzcycletoolkit.main(["nofile.nc", "-r", *full])
    assert len(seen) == 1 and seen[0].batch_chunk == int(argv[argv.index("--batch-chunk") + 1]) and seen[0].track
    assert not os.path.exists(tmp_path / "LEC_Results")


def test_without_the_flag_the_batch_run_has_no_chunk(tmp_path, monkeypatch, tracks):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    seen = []
    monkeypatch.setattr(lorenzcycletoolkit, "run_batch", lambda args, *rest: seen.append(args))
    lorenzcycletoolkit.main(["nofile.nc", "-r", "-t", "--trackfiles", *tracks])
    assert seen[0].batch_chunk is None


# ------------------------------------------------------------------------------------------------------------------------ plan_chunks
def _restated(plan, n_chunk):
    """Chunk by chunk what a streamed batch must hold, from the tracks' own file steps (KS) alone: the union's file steps, per group
    the records (track, position) in (track, step) order, per record the file steps of its own / previous / next track time, and per
    chunk the file steps staged for T and for the other fields."""
    union = sorted({k for ks in KS for k in ks})
    chunks = []
    for c0 in range(0, len(union), n_chunk):
        own_steps = union[c0: c0 + n_chunk]
        groups, t_named = {}, set(own_steps)
        for key, members in plan.groups.items():
            recs = []
            for m in members:
                for p, k in enumerate(KS[m]):
                    if k in own_steps:
                        prev, nxt = KS[m][max(p - 1, 0)], KS[m][min(p + 1, len(KS[m]) - 1)]
                        recs.append((m, p, k, prev, nxt))
                        t_named |= {k, prev, nxt}
            if recs:
                groups[key] = recs
        chunks.append((own_steps, sorted(t_named), groups))
    return union, chunks


@pytest.mark.parametrize("n_chunk", [1, 2, 5, 11, 100])
def test_plan_chunks_against_the_restatement(tracks, n_chunk):
    plan = batch.plan_batch(LAT, LON, LEV, TIME, "hPa", NAMES, tracks)
    assert len(plan.groups) == 2                              # 15 x 15 degree boxes, and the sized ones
    union, want = _restated(plan, n_chunk)
    assert plan.tpos.tolist() == union and 1 not in union     # (union steps are not file steps: step 1 is nobody's)
    got = batch.plan_chunks(plan, n_chunk)
    assert len(got) == len(want) == -(-len(union) // n_chunk)
    if n_chunk >= len(union):
        assert len(got) == 1
    seen = {}
    for ch, (own_steps, t_steps, groups) in zip(got, want):
        assert ch.steps.tolist() == own_steps                 # u, v, omega, Phi: the chunk's own steps
        assert ch.t_steps.tolist() == t_steps                 # T: exactly what the chunk's records name
        assert [plan.tpos[u] for u in range(ch.u0, ch.u1)] == own_steps
        assert set(ch.groups) == set(groups)                  # a group without a record in the chunk is absent: nothing to launch
        for key, recs in groups.items():
            g = ch.groups[key]
            assert list(zip(g.track.tolist(), g.pos.tolist())) == [(m, p) for m, p, *_ in recs]         # (track, step) order
            assert g.t_rows.dtype == np.int32 and g.t_rows.shape == (3, len(recs), 3) and g.f_rows.dtype == np.int32 and g.f_rows.shape == (len(recs), 3)
            for i, (m, p, k, prev, nxt) in enumerate(recs):
                seen[(m, p)] = seen.get((m, p), 0) + 1
                tr = plan.tracks[m]
                corner = [tr.boxes[p][2], tr.boxes[p][0]]     # box south row, box west column, in the union crop
                assert ch.steps[g.f_rows[i, 0]] == k and g.f_rows[i, 1:].tolist() == corner
                for q, file_step in enumerate((k, prev, nxt)):
                    assert ch.t_steps[g.t_rows[q, i, 0]] == file_step and g.t_rows[q, i, 1:].tolist() == corner
                if p == 0:                                    # the first and the last record of a track name themselves
                    assert ch.t_steps[g.t_rows[1, i, 0]] == k
                if p == len(KS[m]) - 1:
                    assert ch.t_steps[g.t_rows[2, i, 0]] == k
    assert seen == {(m, p): 1 for m in range(3) for p in range(len(KS[m]))}          # every record in exactly one chunk
    assert [k for ch in got for k in ch.steps.tolist()] == union                     # the non-T lists: the union, each step once
    if n_chunk == 1:
        # a six-hourly track's neighbours lie in other chunks; some chunks hold no record of a group
        assert any(len(ch.t_steps) == 3 for ch in got) and any(len(ch.groups) < 2 for ch in got)
        assert max(len(ch.t_steps) for ch in got) <= 5


def test_plan_chunks_refuses_an_empty_chunk(tracks):
    plan = batch.plan_batch(LAT, LON, LEV, TIME, "hPa", NAMES, tracks)
    with pytest.raises(ValueError):
        batch.plan_chunks(plan, 0)
