"""-c --choose-lifecycle, the parts that need no GPU: the two new calls' argument validation (before any HIP call) and struct layouts,
the host's births / resolve on hand-made arrays, the command line's refusals, and the NumPy restatement of the rules
(tests/follow_lifecycle_restatement.py) on the NCEP-R2 sample, which pins what the GPU test's command line must write."""
import ctypes
import os
import types

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib, follow as fw
from tests import follow_lifecycle_restatement as fl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTDATA = os.path.join(ROOT, "tests", "golden", "testdata_NCEP-R2.nc")
NAMELIST = os.path.join(ROOT, "tests", "golden", "inputs", "namelist_NCEP-R2")
NEAR_TIE = 1e-9          # (tests/test_gpu_follow.py's, which a test without a GPU cannot import)

SERIES_POINTERS = ("u_d", "v_d", "hgt_d", "xcoef_d", "ycoef_d", "curv_d", "work_d", "seed_pos_d", "seed_val_d", "n_found_d")
SPANS_POINTERS = ("u_d", "v_d", "hgt_d", "xcoef_d", "ycoef_d", "curv_d", "start_d", "pos_d", "val_d", "status_d", "span_d")

# the sample at k = 8, threshold -5e-5, the default 15 x 15 box, search 5 degrees, patience 2, min-steps 2:
# (birth step, (lat, lon) of the birth, span, outcome, continuation of)
SAMPLE = [(0, (-50.0, -7.5), (0, 2), "kept", None), (0, (-70.0, -60.0), (0, 2), "kept", None), (2, (-62.5, -82.5), (2, 4), "kept", None),
          (3, (-60.0, -92.5), None, "continuation", 2), (3, (-70.0, -10.0), (3, 4), "kept", None), (4, (-67.5, -75.0), (4, 4), "too short", None)]


def _series_args():
    """Every pointer set (to an address nothing dereferences: validation comes before any HIP call), every scalar in range."""
    a = _lib.FollowSeedsSeriesArgs()
    for f in SERIES_POINTERS:
        setattr(a, f, 4096)
    a.nt, a.ny, a.nx, a.field, a.sense, a.smooth_r = 5, 33, 41, _lib.FOLLOW_ZETA, _lib.FOLLOW_MIN, 0
    a.ej, a.ei, a.k_max, a.threshold = 3, 3, 8, float("nan")
    a.jlo, a.jhi, a.ilo, a.ihi = 3, 29, 3, 37
    return a


def _spans_args():
    a = _lib.FollowSpansArgs()
    for f in SPANS_POINTERS:
        setattr(a, f, 4096)
    a.nt, a.ny, a.nx = 4, 33, 41
    a.field, a.sense, a.smooth_r, a.sj, a.si = _lib.FOLLOW_ZETA, _lib.FOLLOW_MIN, 0, 2, 2
    a.jlo, a.jhi, a.ilo, a.ihi, a.n_chains, a.patience, a.end_threshold = 3, 29, 3, 37, 5, 2, float("nan")
    return a


BAD_SLICE = [({"nt": 0}, b"nt"), ({"nt": -3}, b"nt"), ({"ny": 2}, b"3 x 3"), ({"nx": 2}, b"3 x 3"), ({"field": 2}, b"field"), ({"sense": -1}, b"sense"),
             ({"smooth_r": -1}, b"smooth_r"), ({"jlo": 30}, b"jlo"), ({"jhi": 33}, b"jhi"), ({"jlo": -1}, b"jlo"), ({"ilo": 38}, b"ilo"),
             ({"ihi": 41}, b"ihi"), ({"field": _lib.FOLLOW_HGT, "hgt_d": None}, b"hgt_d")]


def _refused(call, a, change, code, word):
    lib = _lib.load()
    for k, v in change.items():
        setattr(a, k, v)
    assert getattr(lib, call)(ctypes.byref(a)) == code
    msg = lib.lec_last_error()
    assert msg.startswith(call.encode() + b":") and word in msg, msg
    return msg


@pytest.mark.parametrize("change, word", [({p: None}, p.encode()) for p in SERIES_POINTERS if p != "hgt_d"] + BAD_SLICE + [
    ({"k_max": 0}, b"k_max"), ({"k_max": 257}, b"k_max"), ({"ej": 0}, b"ej"), ({"ei": -2}, b"ei")])
def test_lec_follow_seeds_series_refuses_bad_arguments_without_a_gpu(change, word):
    _refused("lec_follow_seeds_series", _series_args(), change, 1, word)


def test_lec_follow_seeds_series_refuses_a_series_whose_size_overflows():
    change = {"nt": 2 ** 31 - 1, "ny": 46340, "nx": 46340, "jhi": 100, "ihi": 100}          # 2^31 x 2^31 doubles: offsets beyond 64 bits
    _refused("lec_follow_seeds_series", _series_args(), change, 2, b"nt * ny * nx")


@pytest.mark.parametrize("change, word", [({p: None}, p.encode()) for p in SPANS_POINTERS if p != "hgt_d"] + BAD_SLICE + [
    ({"n_chains": 0}, b"n_chains"), ({"patience": 0}, b"patience"), ({"patience": -1}, b"patience"), ({"sj": 0}, b"sj"), ({"si": -3}, b"si")])
def test_lec_follow_spans_refuses_bad_arguments_without_a_gpu(change, word):
    _refused("lec_follow_spans", _spans_args(), change, 1, word)


def test_lec_follow_spans_refuses_the_over_limit_tile_with_both_figures():
    change = {"ny": 400, "nx": 400, "jhi": 300, "ihi": 300, "sj": 70, "si": 70, "smooth_r": 2}          # as lec_follow_many: 145 x 145 doubles
    msg = _refused("lec_follow_spans", _spans_args(), change, 2, b"145 x 145")
    assert b"168200" in msg and b"163776" in msg


def test_exports_null_structs_and_layouts():
    lib = _lib.load()
    assert "lec_follow_seeds_series" in _lib.EXPORTS and "lec_follow_spans" in _lib.EXPORTS
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11                  # additive calls
    assert _lib.FOLLOW_NOT_LIVE == 3 and _lib.FOLLOW_BAD_START == 2
    for call, empty in (("lec_follow_seeds_series", _lib.FollowSeedsSeriesArgs()), ("lec_follow_spans", _lib.FollowSpansArgs())):
        assert getattr(lib, call)(None) == 1 and b"null args" in lib.lec_last_error() and lib.lec_last_error().startswith(call.encode())
        assert getattr(lib, call)(ctypes.byref(empty)) == 1 and b"null pointer argument u_d" in lib.lec_last_error()
    # the header: 3 pointers + 4 int32 + 3 pointers + 10 int32 + 1 double + 5 pointers
    assert ctypes.sizeof(_lib.FollowSeedsSeriesArgs) == 3 * 8 + 4 * 4 + 3 * 8 + 10 * 4 + 8 + 5 * 8 == 152
    assert _lib.FollowSeedsSeriesArgs.threshold.offset == 104 and _lib.FollowSeedsSeriesArgs.work_d.offset == 112
    # lec_follow_many_args with patience in reserved0's place, end_threshold after start_d and span_d before the stream
    assert ctypes.sizeof(_lib.FollowSpansArgs) == ctypes.sizeof(_lib.FollowManyArgs) + 16 == 160
    assert _lib.FollowSpansArgs.patience.offset == _lib.FollowManyArgs.reserved0.offset and _lib.FollowSpansArgs.start_d.offset == 104
    assert _lib.FollowSpansArgs.end_threshold.offset == 112 and _lib.FollowSpansArgs.span_d.offset == 144
    # the two existing structs have not moved
    assert ctypes.sizeof(_lib.FollowSeedsArgs) == 144 and ctypes.sizeof(_lib.FollowManyArgs) == 144 and ctypes.sizeof(_lib.FollowArgs) == 136


def _seed_table(steps, k=4):
    pos, n = np.full((len(steps), k, 2), -2, dtype=np.int32), np.zeros(len(steps), dtype=np.int32)
    for t, seeds in enumerate(steps):
        n[t] = len(seeds)
        pos[t, :len(seeds)] = np.array(seeds, dtype=np.int32).reshape(-1, 2)
    return pos, n


def test_births_on_hand_made_seeds():
    sj, si = 2, 3
    steps = [[(10, 10), (20, 30)],                       # step 0: both are births
             [(12, 13), (20, 34), (13, 10)],             # exactly (sj, si) away: no birth; si + 1 away: a birth; sj + 1 away: a birth
             [],                                         # a step without a seed
             [(12, 13)],                                 # ... so that this one is a birth again
             [(30, 5), (12, 13)]]                        # a new one in front of a known one: rank 0 is the birth
    pos, n = _seed_table(steps)
    got = fw.births(pos, n, sj, si)
    assert got.dtype == np.int32 and got.tolist() == [[0, 10, 10, 0], [0, 20, 30, 1], [1, 20, 34, 1], [1, 13, 10, 2], [3, 12, 13, 0], [4, 30, 5, 0]]
    assert [list(b) for b in fl.births(steps, sj, si)] == got.tolist()                      # the restatement says the same
    assert fw.births(*_seed_table([[], []]), sj, si).shape == (0, 4)


def _chains(nt, tracks):
    """pos [K][nt][2] (-1 outside the walked steps) from {chain: (t0, [(j, i), ...])}."""
    pos = np.full((len(tracks), nt, 2), -1, dtype=np.int32)
    for c, (t0, centres) in enumerate(tracks):
        pos[c, t0: t0 + len(centres)] = centres
    return pos


def test_resolve_a_dip_seeded_again_and_the_same_dip_after_the_span_ended():
    ej = ei = 3
    # chain 0 lives 0..5 and sits at (20, 24) at step 3; chain 1 is born there and then, 3 away: its continuation.  Chain 2 is born at the
    # same place at step 6, after chain 0's span has ended: a system of its own.  Chain 3 is born inside chain 0's span but 4 away: kept.
    # Chain 4 has no good step: dropped, and no one's continuation.  Chain 5 would continue chain 1 -- but chain 1 is not kept -- and does
    # continue chain 0.
    tracks = [(0, [(20, 20), (20, 21), (20, 22), (20, 24), (20, 25), (20, 26), (20, 27), (20, 27)]), (3, [(23, 27)] * 5), (6, [(20, 27)] * 2),
              (3, [(24, 24)] * 5), (1, [(5, 5)] * 7), (4, [(22, 26)] * 4)]
    starts = np.array([(t0, *c[0], 0) for t0, c in tracks], dtype=np.int32)
    span = np.array([(0, 5), (3, 7), (6, 7), (3, 7), (-1, -1), (4, 7)], dtype=np.int32)
    kept, cont = fw.resolve(starts, _chains(8, tracks), span, ej, ei)
    assert kept.tolist() == [True, False, True, True, False, False] and cont.tolist() == [-1, 0, -1, -1, -1, 0]
    ref = fl.resolve([tuple(s) for s in starts.tolist()], [{"span": tuple(s), "pos": p} for s, p in zip(span.tolist(), _chains(8, tracks))], ej, ei)
    assert ref[0] == kept.tolist() and [-1 if c is None else c for c in ref[1]] == cont.tolist()
    # the end of the span counts as inside it
    kept, cont = fw.resolve(starts[:3], _chains(8, tracks)[:3], np.array([(0, 6), (3, 7), (6, 7)]), ej, ei)
    assert kept.tolist() == [True, False, False] and cont.tolist() == [-1, 0, 0]


def test_first_shared_centre_live_compares_the_common_steps_only():
    pos = _chains(4, [(0, [(1, 1), (2, 2), (3, 3), (4, 4)]), (1, [(2, 2), (3, 3), (9, 9)]), (0, [(-1, -1)] * 4), (2, [(3, 3), (4, 4)])])
    span = np.array([(0, 1), (1, 3), (-1, -1), (2, 3)])
    # chain 1 meets chain 0 at step 1 (inside both spans); chain 3 equals chain 0 at steps 2-3, where chain 0 no longer lives, and chain 1 at step 2
    assert fw.first_shared_centre_live(pos, span) == [None, (0, 1), None, (1, 2)]


@pytest.mark.parametrize("argv, word", [
    (["-r", "-t", "--choose-lifecycle"], "--choose-lifecycle goes with -c"),
    (["-r", "-c", "--choose-lifecycle"], "--choose-lifecycle needs --choose-systems K and --choose-threshold X"),
    (["-r", "-c", "--choose-lifecycle", "--choose-systems", "4"], "--choose-lifecycle needs --choose-systems K and --choose-threshold X"),
    (["-r", "-c", "--choose-lifecycle", "--choose-starts", TESTDATA], "--choose-starts names those of the first"),
    (["-r", "-c", "--choose-lifecycle", "--choose-start", "-50", "-7.5"], "--choose-lifecycle needs --choose-systems"),
    (["-r", "-c", "--choose-systems", "4", "--choose-threshold", "-5e-5", "--choose-end-threshold", "-4e-5"], "--choose-end-threshold goes with --choose-lifecycle"),
    (["-r", "-c", "--choose-systems", "4", "--choose-patience", "2"], "--choose-patience goes with --choose-lifecycle"),
    (["-r", "-c", "--choose-min-steps", "2"], "--choose-min-steps goes with --choose-lifecycle"),
    (["-r", "-c", "--choose-systems", "4", "--choose-lifecycle", "--choose-threshold", "-5e-5", "--choose-patience", "0"], "--choose-patience must be >= 1"),
    (["-r", "-c", "--choose-systems", "4", "--choose-lifecycle", "--choose-threshold", "-5e-5", "--choose-min-steps", "1"], "--choose-min-steps must be >= 2"),
    (["-r", "-c", "--choose-systems", "4", "--choose-lifecycle", "--choose-threshold", "-5e-5", "--choose-hemisphere", "south",
      "--choose-end-threshold", "-6e-5"], "is stricter than --choose-threshold"),
    (["-r", "-c", "--choose-systems", "4", "--choose-lifecycle", "--choose-threshold", "5e-5", "--choose-hemisphere", "north",
      "--choose-end-threshold", "6e-5"], "is stricter than --choose-threshold"),
    (["-r", "-c", "--choose-systems", "4", "--choose-lifecycle", "--choose-threshold", "1400", "--choose-field", "hgt",
      "--choose-end-threshold", "1390"], "is stricter than --choose-threshold"),
    (["-r", "-c", "--choose-systems", "4", "--choose-lifecycle", "--choose-threshold", "-5e-5", "--gpus", "2"], "on one GPU"),
    (["-r", "-c", "--choose-systems", "4", "--choose-lifecycle", "--choose-threshold", "-5e-5", "--device-ingest"], "is not supported for a batch of tracks"),
])
def test_command_line_refusals_leave_nothing_behind(tmp_path, monkeypatch, argv, word):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main([TESTDATA] + argv)
    assert word in str(e.value)
    assert os.listdir(tmp_path) == []                                 # no LEC_Results


def test_the_end_threshold_takes_a_negative_number_in_exponent_form():
    import lorenzcycletoolkit
    argv = ["f.nc", "-r", "-c", "--choose-systems", "4", "--choose-lifecycle", "--choose-threshold", "-5e-5", "--choose-end-threshold", "-4e-5",
            "--choose-patience", "3", "--choose-min-steps", "4"]
    args = lorenzcycletoolkit.create_arg_parser().parse_args(lorenzcycletoolkit._join_threshold(argv))
    assert (args.choose_lifecycle, args.choose_threshold, args.choose_end_threshold, args.choose_patience, args.choose_min_steps) == (True, -5e-5, -4e-5, 3, 4)
    lorenzcycletoolkit.refuse_choose_options(args)                    # weaker than the threshold: accepted
    plain = lorenzcycletoolkit.create_arg_parser().parse_args(["f.nc", "-r", "-c", "--choose-systems", "2"])
    assert plain.choose_lifecycle is None and plain.choose_end_threshold is None and plain.choose_patience is None and plain.choose_min_steps is None
    text = " ".join(lorenzcycletoolkit.create_arg_parser().format_help().split())
    assert all(o in text for o in ("--choose-lifecycle", "--choose-end-threshold", "--choose-patience", "--choose-min-steps"))


@pytest.fixture(scope="module")
def sample():
    a = types.SimpleNamespace(infile=TESTDATA, mpas=False, choose_domain=None)
    return fw.search_domain_slices(a, NAMELIST)


def _table(out, lat, lon):
    return [(t0, (float(lat[j]), float(lon[i])), None if oc == "continuation" else tuple(int(x) for x in sp), oc, of)
            for (t0, j, i, _), sp, oc, of in zip(out["births"], out["spans"], out["outcome"], out["continuation_of"])]


def test_the_restatement_on_the_sample_pins_the_fixture(sample):
    u, v, h, lat, lon, time = sample
    assert u.shape == (5, 33, 41)
    out = fl.lifecycle(u, v, h, lat, lon, k=8, threshold=-5e-5)
    print("sample: margins", out["margins"], "births", out["births"], "spans", out["spans"])
    assert _table(out, lat, lon) == SAMPLE
    assert (out["sj"], out["si"], out["ej"], out["ei"]) == (2, 2, 3, 3)
    # the fourth birth: the third's chain sits at (-60, -87.5) then, within ej = ei = 3 grid steps
    third = out["chains"][2]
    assert (lat[third["pos"][3][0]], lon[third["pos"][3][1]]) == (-60.0, -87.5)
    m = out["margins"]
    assert min(m.values()) > NEAR_TIE
    assert 2e-3 < m["seeds"] < 3e-3 and 7e-3 < m["windows"] < 8.5e-3 and 1e-2 < m["threshold"] < 2.5e-2        # 2.5e-3, 7.7e-3, 1.5e-2
    # the vorticity of the two systems of step 0 weakens as the issue of this mode says it does
    assert np.allclose(out["chains"][0]["val"][[0, 3]], [-9.8e-5, -2.7e-5], atol=1e-6) and np.allclose(out["chains"][1]["val"][[0, 3]], [-5.9e-5, -4.5e-5], atol=1e-6)


def test_the_restatement_on_the_sample_with_other_settings(sample):
    u, v, h, lat, lon, _ = sample
    one = fl.lifecycle(u, v, h, lat, lon, k=8, threshold=-5e-5, patience=1)
    assert _table(one, lat, lon) == SAMPLE and min(one["margins"].values()) > NEAR_TIE
    weaker = fl.lifecycle(u, v, h, lat, lon, k=8, threshold=-5e-5, end_threshold=-4e-5)
    assert min(weaker["margins"].values()) > NEAR_TIE
    assert weaker["births"] == one["births"] and weaker["spans"][1] == (0, 3) and weaker["spans"][0] == (0, 2)
