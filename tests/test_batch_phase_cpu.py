"""Phase-aligned ensembles of batch composites without a GPU: the clocks (``batch.phase_ranges``: ``lifetime:B`` by hand and exhaustively,
``peak:L`` with its ties, NaN values and refusals), ``batch.phase_terms``, the restatement (tests/batch_phase_restatement.py) on hand-made
columns, the additive C calls ``lec_composite_phase_sum`` / ``lec_composite_phase_ensemble`` (exports, the fifth extension header, ABI 11,
struct layouts, every refusal on the scalars and on the host copies of the tables before any HIP call), the engine's and the command
line's refusals and the documentation."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from lorenzcycletoolkit_amd import _lib, batch
from tests import batch_phase_restatement as pr
from tests.test_batch_composite_cpu import _fields_of, _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the clocks -----------------------------------------------------------------------------------------------------------------------
def _plan(sizes, dt_hours=6, paths=None):
    """What ``phase_ranges`` reads of a plan: per track its path and its times."""
    t0 = np.datetime64("2005-08-08T00", "ns")
    dts = dt_hours if isinstance(dt_hours, (list, tuple)) else [dt_hours] * len(sizes)
    tracks = []
    for k, (n, dt) in enumerate(zip(sizes, dts)):
        time = t0 + (np.asarray(dt) if np.ndim(dt) else np.arange(n) * dt) * np.timedelta64(3600, "s")
        tracks.append(SimpleNamespace(path=paths[k] if paths else f"tracks/t{k}", time=time.astype("datetime64[ns]"), n=n))
    return SimpleNamespace(tracks=tracks)


def test_lifetime_tables_by_hand():
    r = batch.phase_ranges(_plan([9, 5, 2]), "lifetime:4")
    assert r.dtype == np.int32 and r.shape == (3, 4, 2)
    assert (r[:, :, 1] - r[:, :, 0]).tolist() == [[3, 2, 2, 2], [2, 1, 1, 1], [1, 0, 1, 0]]
    assert r[0].tolist() == [[0, 3], [3, 5], [5, 7], [7, 9]] and r[1].tolist() == [[0, 2], [2, 3], [3, 4], [4, 5]]
    assert r[2, 0].tolist() == [0, 1] and r[2, 2].tolist() == [1, 2] and r[2, 1, 0] == r[2, 1, 1] and r[2, 3, 0] == r[2, 3, 1]
    assert batch.phase_ranges(_plan([9, 5, 2]), ("lifetime", 4)).tolist() == r.tolist()
    for n in (2, 7, 40):
        assert batch.phase_ranges(_plan([n]), "lifetime:1").tolist() == [[[0, n]]]


def test_lifetime_every_step_lies_in_exactly_one_bin():
    for n in range(1, 41):
        for B in range(1, 13):
            r = batch.lifetime_ranges(n, B)
            assert r.shape == (B, 2) and (0 <= r).all() and (r[:, 0] <= r[:, 1]).all() and (r <= n).all()
            owner = np.full(n, -1)
            for b, (lo, hi) in enumerate(r):
                assert (owner[lo:hi] == -1).all()
                owner[lo:hi] = b
            assert owner.tolist() == [(s * B) // n for s in range(n)], (n, B)


def test_peak_clock_first_last_ties_and_nan():
    nan = float("nan")
    plan = _plan([4, 5, 3, 4])
    z = [[-9.0, 1.0, 2.0, 3.0],            # the peak at the first step (|.| counts)
         [1.0, 2.0, 3.0, 4.0, -5.0],       # at the last
         [2.0, -7.0, 7.0],                 # a tie: the first wins
         [nan, 1.0, nan, float("inf")]]    # values that are not finite are skipped
    assert [batch.peak_step(v) for v in z] == [0, 4, 1, 1]
    r = batch.phase_ranges(plan, "peak:2", z)
    assert r.shape == (4, 5, 2) and r.dtype == np.int32
    cells = lambda k: [tuple(x) if x[1] > x[0] else None for x in r[k].tolist()]
    assert cells(0) == [None, None, (0, 1), (1, 2), (2, 3)]
    assert cells(1) == [(2, 3), (3, 4), (4, 5), None, None]
    assert cells(2) == [None, (0, 1), (1, 2), (2, 3), None]
    assert cells(3) == [None, (0, 1), (1, 2), (2, 3), (3, 4)]
    assert (r[:, :, 0] <= r[:, :, 1]).all() and (r >= 0).all()
    assert batch.phase_ranges(plan, "peak:0", z)[:, 0].tolist() == [[0, 1], [4, 5], [1, 2], [1, 2]]


def test_peak_clock_refusals_name_the_track_file():
    z = lambda sizes: [np.arange(1.0, n + 1) for n in sizes]
    with pytest.raises(batch.BatchRefusal, match=r"track file tracks/t1: no finite min_max_zeta_850"):
        batch.phase_ranges(_plan([3, 3]), "peak:1", [[1.0, 2.0, 3.0], [np.nan] * 3])
    uneven = _plan([3, 4], dt_hours=[6, [0, 6, 18, 24]])
    with pytest.raises(batch.BatchRefusal, match=r"track file tracks/t1: .*evenly spaced time axis"):
        batch.phase_ranges(uneven, "peak:1", z([3, 4]))
    with pytest.raises(batch.BatchRefusal, match=r"track file tracks/t1: its steps are 3 h apart, those of tracks/t0 6 h"):
        batch.phase_ranges(_plan([3, 4], dt_hours=[6, 3]), "peak:1", z([3, 4]))
    assert batch.phase_ranges(uneven, "lifetime:2").shape == (2, 2, 2)          # the lifetime clock asks nothing of the time axis
    with pytest.raises(ValueError, match="needs every track's intensities"):
        batch.phase_ranges(_plan([3, 3]), "peak:1")


@pytest.mark.parametrize("text, words", [("lifetime", "is not a clock"), ("lifetime:", "is not a clock"), ("lifetime:x", "is not a clock"),
                                         ("lifetime:2.5", "is not a clock"), ("days:3", "names the clock 'days'"),
                                         ("lifetime:0", "B >= 1"), ("lifetime:-2", "B >= 1"), ("peak:-1", "L >= 0")])
def test_clock_words(text, words):
    with pytest.raises(ValueError, match=re.escape(words)):
        batch.parse_phase_clock(text)
    assert batch.parse_phase_clock("lifetime:3") == ("lifetime", 3) and batch.parse_phase_clock("peak:0") == ("peak", 0)


def test_labels():
    assert batch.phase_labels("lifetime:2") == ["lifetime [0/2, 1/2)", "lifetime [1/2, 2/2)"]
    assert batch.phase_labels("peak:1", 6.0) == ["lag -1 steps (-6 h)", "lag +0 steps (+0 h)", "lag +1 steps (+6 h)"]


def test_phase_terms_on_hand_made_frames():
    a = pd.DataFrame({"Az": [1.0, 2.0, 3.0, 4.0], "Ck": [10.0, 20.0, 30.0, 40.0]})
    b = pd.DataFrame({"Az": [100.0, 200.0], "Ck": [-1.0, -2.0]})
    ranges = np.array([[[0, 2], [2, 4], [0, 0]], [[0, 1], [1, 1], [2, 2]]])
    got = batch.phase_terms([a, b], ranges)
    assert list(got.columns) == ["Az", "Ck"] and got.index.name == "bin" and len(got) == 3
    assert got.loc[0].tolist() == [(1.5 + 100.0) / 2, (15.0 - 1.0) / 2]
    assert got.loc[1].tolist() == [3.5, 35.0]                       # track b has no step in bin 1: a's mean alone
    assert got.loc[2].isna().all()                                  # nobody has


def test_restatement_on_hand_made_columns():
    C0 = np.arange(4.0).reshape(4, 1, 1, 1) * np.ones((4, 6, 2, 3))
    C1 = 10.0 + np.arange(2.0).reshape(2, 1, 1, 1) * np.ones((2, 6, 2, 3))
    mean, ens, spread, count, members = pr.phases([(C0, None, None), (C1, None, None)], [[[0, 2], [2, 4], [1, 1]], [[0, 2], [2, 2], [0, 0]]])
    assert count.tolist() == [[2, 2, 0], [2, 0, 0]] and members.tolist() == [2, 1, 0]
    assert (mean[0, 0] == 0.5).all() and (mean[0, 1] == 2.5).all() and np.isnan(mean[0, 2]).all() and (mean[1, 0] == 10.5).all()
    assert np.isnan(mean[1, 1:]).all()
    assert (ens[0] == 5.5).all() and (ens[1] == 2.5).all() and np.isnan(ens[2]).all()
    assert np.allclose(spread[0], np.sqrt(2 * 25.0)) and np.isnan(spread[1:]).all()


# -- the C calls ----------------------------------------------------------------------------------------------------------------------
def test_calls_are_the_fifth_extension():
    lib = _lib.load()
    assert _lib.EXT5_EXPORTS == ["lec_composite_phase_sum", "lec_composite_phase_ensemble"]
    assert not set(_lib.EXT5_EXPORTS) & set(_lib.EXPORTS + _lib.EXT_EXPORTS + _lib.EXT2_EXPORTS + _lib.EXT3_EXPORTS + _lib.EXT4_EXPORTS)
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    ext5 = read("include", "lec_hip_ext5.h")
    assert set(re.findall(r"^int (lec_\w+)\(", ext5, flags=re.M)) == set(_lib.EXT5_EXPORTS) and '#include "lec_hip.h"' in ext5
    for name in _lib.EXT5_EXPORTS:
        assert getattr(lib, name) is not None
        for old in ("lec_hip.h", "lec_hip_ext.h", "lec_hip_ext2.h", "lec_hip_ext3.h", "lec_hip_ext4.h"):
            assert name not in read("include", old), (name, old)
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11 and "#define LEC_ABI_VERSION 11" in read("include", "lec_hip.h")
    mk = read("lorenzcycletoolkit_amd", "csrc", "Makefile")
    assert "lec_composite_phase.hip" in mk and "lec_hip_ext5.h" in mk
    assert "lec_hip_ext5.h" in inspect.getsource(_lib.source_digest)
    assert "EXT5_EXPORTS" in read("__graft_entry__.py")
    src = read("lorenzcycletoolkit_amd", "csrc", "lec_composite_phase.hip")
    assert "__shared__" not in src and "atomic" not in src.lower()                 # one writer per element, nothing through LDS
    assert '#include "lec_mapcol.h"' not in src and "fp contract(off)" in src      # a code object of its own


@pytest.mark.parametrize("struct, cls, size", [("lec_composite_phase_sum_args", "CompositePhaseSumArgs", 4 * 8 + 5 * 4 + 4 + 8),
                                               ("lec_composite_phase_ensemble_args", "CompositePhaseEnsembleArgs", 3 * 8 + 5 * 4 + 4 + 4 * 8)])
def test_ctypes_structs_match_the_header(struct, cls, size):
    header = open(os.path.join(ROOT, "include", "lec_hip_ext5.h")).read()
    A = getattr(_lib, cls)
    declared = _fields_of(header, struct)
    assert [n for _, n in declared] == [n for n, _ in A._fields_]
    off = 0
    for (typ, name), (_, ctype) in zip(declared, A._fields_):
        want = 4 if typ == "int32_t" else 8
        assert ctypes.sizeof(ctype) == want, name
        off = (off + want - 1) // want * want
        assert getattr(A, name).offset == off, name
        off += want
    assert ctypes.sizeof(A) == size == (off + 7) // 8 * 8


def test_null_args():
    lib = _lib.load()
    for call, name in ((lib.lec_composite_phase_sum, b"lec_composite_phase_sum:"), (lib.lec_composite_phase_ensemble, b"lec_composite_phase_ensemble:")):
        assert call(None) == 1
        assert lib.lec_last_error().startswith(name) and b"null args" in lib.lec_last_error()


def _valid_sum(ranges=((0, 3), (3, 3), (1, 4), (0, 0))):
    """Scalars of a valid call over fake (never dereferenced) device pointers and a real host copy of the ranges: every refusal is made
    before any HIP call.  Returns (args, the host array, which must outlive the call)."""
    a = _lib.CompositePhaseSumArgs()
    for n in ("col_d", "range_d", "phasesum_d"):
        setattr(a, n, 0x10000)
    host = np.ascontiguousarray(ranges, dtype=np.int32)
    a.range_h = host.ctypes.data
    a.s_count, a.nyb, a.nxb, a.n_cell = 4, 4, 7, len(ranges)
    return a, host


@pytest.mark.parametrize("field, change", [(n, _set(**{n: None})) for n in ("col_d", "range_h", "range_d", "phasesum_d")] + [
    ("reserved0", _set(reserved0=1)), ("s_count", _set(s_count=0)), ("nyb", _set(nyb=0)), ("nxb", _set(nxb=0)), ("n_cell", _set(n_cell=0)),
    ("col_d", _set(col_d=0x10004)), ("phasesum_d", _set(phasesum_d=0x10004)), ("range_d", _set(range_d=0x10002)),
])
def test_sum_call_refusals_name_the_field(field, change):
    lib = _lib.load()
    a, host = _valid_sum()
    change(a)
    assert lib.lec_composite_phase_sum(ctypes.byref(a)) == 1          # LEC_ERR_ARG
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_phase_sum:") and field.encode() in msg, msg


def test_sum_call_refuses_a_misaligned_host_table():
    lib = _lib.load()
    a, host = _valid_sum()
    raw = np.zeros(64, dtype=np.uint8)
    a.range_h = (raw.ctypes.data + 3) // 4 * 4 + 2
    assert lib.lec_composite_phase_sum(ctypes.byref(a)) == 1 and b"range_h must be 4-byte aligned" in lib.lec_last_error()


@pytest.mark.parametrize("ranges, words", [
    (((0, 3), (-1, 2), (1, 4)), b"range_h: cell 1 has the range [-1, 2)"),
    (((0, 3), (3, 3), (3, 2)), b"range_h: cell 2 has the range [3, 2)"),
    (((0, 5), (3, 3), (1, 4)), b"range_h: cell 0 has the range [0, 5), which must satisfy 0 <= begin <= end <= s_count = 4"),
    (((0, 3), (3, 3), (1, 4), (5, 5)), b"range_h: cell 3 has the range [5, 5)"),
])
def test_sum_call_checks_the_host_copy_of_its_ranges(ranges, words):
    lib = _lib.load()
    a, host = _valid_sum(ranges)
    assert lib.lec_composite_phase_sum(ctypes.byref(a)) == 1
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_phase_sum: ") and words in msg, msg


def _valid_ensemble(counts=((3, 0, 2), (1, 0, 0))):
    a = _lib.CompositePhaseEnsembleArgs()
    for n in ("phasesum_d", "count_d", "mean_d", "ens_d", "spread_d"):
        setattr(a, n, 0x10000)
    host = np.ascontiguousarray(counts, dtype=np.int32)
    a.count_h = host.ctypes.data
    a.n_track, a.n_bin, a.nyb, a.nxb = host.shape[0], host.shape[1], 4, 7
    return a, host


@pytest.mark.parametrize("field, change", [(n, _set(**{n: None})) for n in ("phasesum_d", "count_h", "count_d", "mean_d", "ens_d", "spread_d")] + [
    ("reserved0", _set(reserved0=1)), ("n_track", _set(n_track=0)), ("n_bin", _set(n_bin=0)), ("nyb", _set(nyb=0)), ("nxb", _set(nxb=0)),
    ("count_d", _set(count_d=0x10002)), ("phasesum_d", _set(phasesum_d=0x10004)), ("mean_d", _set(mean_d=0x10004)),
    ("ens_d", _set(ens_d=0x10004)), ("spread_d", _set(spread_d=0x10004)),
])
def test_ensemble_call_refusals_name_the_field(field, change):
    lib = _lib.load()
    a, host = _valid_ensemble()
    change(a)
    assert lib.lec_composite_phase_ensemble(ctypes.byref(a)) == 1
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_phase_ensemble:") and field.encode() in msg, msg


def test_ensemble_call_checks_the_counts():
    lib = _lib.load()
    a, host = _valid_ensemble(((3, 0, 2), (1, -1, 0)))
    assert lib.lec_composite_phase_ensemble(ctypes.byref(a)) == 1
    assert b"lec_composite_phase_ensemble: count_h: track 1, bin 1 has -1 steps" in lib.lec_last_error()


def test_both_calls_beyond_two_to_the_32_threads():
    lib = _lib.load()
    # n_cell * 6 * nyb * nxb >= 2^32 - 256: 2^20 cells of 32 x 32 points; one point fewer than the limit passes this check (and is
    # refused by the next one, a range of the host table)
    n = 1 << 20
    a, host = _valid_sum(np.zeros((n, 2), dtype=np.int32))
    a.nyb, a.nxb = 32, 32
    assert lib.lec_composite_phase_sum(ctypes.byref(a)) == 2          # LEC_ERR_UNSUPPORTED
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_phase_sum:") and b"n_cell * 6 * nyb * nxb" in msg, msg
    small = np.zeros((4, 2), dtype=np.int32)
    small[3] = (0, 9)
    a, host = _valid_sum(small)
    a.nyb, a.nxb = 1 << 14, 1 << 13                                   # 4 * 6 * 2^27 = 3 * 2^30 < 2^32 - 256
    assert lib.lec_composite_phase_sum(ctypes.byref(a)) == 1 and b"cell 3" in lib.lec_last_error()
    a.nyb = 1 << 15                                                   # 3 * 2^31
    assert lib.lec_composite_phase_sum(ctypes.byref(a)) == 2
    a, host = _valid_ensemble(((1, 1, 1, 1), (1, 1, 1, -1)))
    a.nyb, a.nxb = 1 << 14, 1 << 13
    assert lib.lec_composite_phase_ensemble(ctypes.byref(a)) == 1 and b"track 1, bin 3" in lib.lec_last_error()
    a.nyb = 1 << 15
    assert lib.lec_composite_phase_ensemble(ctypes.byref(a)) == 2
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_phase_ensemble:") and b"n_bin * 6 * nyb * nxb" in msg, msg


# -- the engine -----------------------------------------------------------------------------------------------------------------------
def test_engine_refusals_in_words():
    import torch
    from lorenzcycletoolkit_amd.engine import LECEngine
    ok = LECEngine._check_batch_phases([3, 2], [[[0, 2], [2, 3]], [[0, 0], [0, 2]]])
    assert ok.dtype == np.int32 and ok.shape == (2, 2, 2) and ok.flags.c_contiguous
    for ranges, words in [([[0, 2], [2, 3]], r"an integer array \[K, B, 2\]"),
                          ([[[0, 2], [2, 3]]], r"K = 2 tracks"),
                          (np.zeros((2, 0, 2), dtype=int), r"B >= 1 ranges"),
                          (np.zeros((2, 2, 3), dtype=int), r"\[K, B, 2\]"),
                          (np.zeros((2, 2, 2)), r"an integer array"),
                          ([[[0, 2], [3, 2]], [[0, 0], [0, 2]]], r"track 0, bin 1: the range \[3, 2\) has begin > end"),
                          ([[[0, 2], [2, 4]], [[0, 0], [0, 2]]], r"track 0, bin 1: the range \[2, 4\) ends after the track's 3 steps"),
                          ([[[0, 2], [2, 3]], [[0, 0], [1, 3]]], r"track 1, bin 1: the range \[1, 3\) ends after the track's 2 steps"),
                          ([[[0, 2], [2, 3]], [[-1, 0], [0, 2]]], r"track 1, bin 0: the range \[-1, 0\) begins before")]:
        with pytest.raises(ValueError, match=words):
            LECEngine._check_batch_phases([3, 2], ranges)
    # compute refuses before it touches the engine's tables, the library or a device: an engine that was never initialised will do
    eng = object.__new__(LECEngine)
    t = torch.zeros((3, 2, 8, 8), dtype=torch.float64)
    st = torch.zeros((3, 3), dtype=torch.int32)
    boxes = [(0, 4, 0, 3), (1, 5, 2, 5), (2, 6, 1, 4)]
    for kw, words in [(dict(batch_composite_phases=[[[0, 3]]]), "give the sizes"),
                      (dict(batch_composites=[3], steps=st, batch_composite_phases=[[0, 3]]), r"an integer array \[K, B, 2\]"),
                      (dict(batch_composites=[3], steps=st, batch_composite_phases=[[[2, 1]]]), "begin > end"),
                      (dict(batch_composites=[2, 1], steps=st, batch_composite_phases=[[[0, 2]], [[0, 2]]]), "ends after the track's 1 steps")]:
        with pytest.raises(ValueError, match=words):
            eng.compute(t, t, t, t, None, boxes, per_step_boxes=True, **kw)


def test_device_bytes_count_the_accumulator():
    tracks = [SimpleNamespace(n=5), SimpleNamespace(n=3), SimpleNamespace(n=4)]
    plan = SimpleNamespace(tracks=tracks, groups={(4, 7, True): [0, 2], (3, 5, True): [1]}, tpos=np.arange(6), lat=np.arange(9), lon=np.arange(11),
                           px=SimpleNamespace(level=np.arange(4)))
    plain, with_b = batch.device_bytes(plan, 5, 8), batch.device_bytes(plan, 5, 8, phase_bins=3)
    extra = 8 * 3 * 6 * ((2 + 2) * 4 * 7 + (1 + 2) * 3 * 5)          # per group: K cells' sums, the ensemble and the spread, per bin
    assert with_b["results"] - plain["results"] == extra == with_b["total"] - plain["total"]
    assert with_b["cubes"] == plain["cubes"] and with_b["records"] == plain["records"]
    assert batch.device_bytes(plan, 5, 8, phase_bins=0) == plain


# -- the command line -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags, text", [
    (["-t", "--trackfiles", "a", "b", "--batch-composites-phase", "lifetime:3"], "it goes with --batch-composites"),
    (["-c", "--choose-systems", "2", "--batch-composites-phase", "peak:1"], "it goes with --batch-composites"),
    (["-t", "--trackfiles", "a", "b", "--batch-composites", "--batch-composites-phase", "lifetime"], "is not a clock: lifetime:B"),
    (["-t", "--trackfiles", "a", "b", "--batch-composites", "--batch-composites-phase", "phase:3"], "names the clock 'phase'"),
    (["-t", "--trackfiles", "a", "b", "--batch-composites", "--batch-composites-phase", "lifetime:0"], "a lifetime needs B >= 1 bins"),
    (["-t", "--trackfiles", "a", "b", "--batch-composites", "--batch-composites-phase=peak:-1"], "L >= 0 steps on either side"),
    (["-t", "--trackfiles", "a", "b", "--batch-composites", "--batch-composites-phase", "peak:1", "--gpus", "2"], "--batch-composites runs on one GPU"),
    (["-t", "--trackfiles", "a", "b", "--batch-composites", "--batch-composites-phase", "peak:1", "--ingest", "device"],
     "--batch-composites prepares the data on the host"),
    (["-t", "--trackfiles", "a", "b", "--batch-composites", "--batch-composites-phase", "lifetime:2", "--batch-chunk", "4"],
     "--batch-chunk streams the batch and never holds them"),
])
def test_cli_refusals(tmp_path, monkeypatch, flags, text):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", *flags])
    assert text in str(e.value)
    assert not os.path.exists(tmp_path / "LEC_Results")          # refused before anything was created


def test_help_docstring_readme_and_design_name_the_flag(capsys):
    import lorenzcycletoolkit
    with pytest.raises(SystemExit):
        lorenzcycletoolkit.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--batch-composites-phase" in text and "lec_composite_phase_sum" in text and "phase_terms.csv" in text
    assert "--batch-composites-phase" in lorenzcycletoolkit.__doc__
    assert "--batch-composites-phase" in open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.2i" in design and "lec_composite_phase_sum" in design and "lec_composite_phase_ensemble" in design
