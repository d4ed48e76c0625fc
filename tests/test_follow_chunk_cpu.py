"""-c --choose-chunk, the parts that need no GPU: ``lec_follow_spans_chunk``'s export, struct layout and argument validation (before any
HIP call), the planner of the chunks, reading a range of time steps, the command line's refusals, and the NumPy restatement of the
resumed chain (tests/follow_chunk_restatement.py) on the NCEP-R2 sample against the whole-series restatement."""
import ctypes
import os
import types

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib, follow as fw
from tests import follow_chunk_restatement as fc
from tests import follow_lifecycle_restatement as fl
from tests.test_follow_lifecycle_cpu import NAMELIST, SAMPLE, TESTDATA, _refused, _spans_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "lec_follow_spans_chunk"
CHUNK_POINTERS = ("u_d", "v_d", "hgt_d", "xcoef_d", "ycoef_d", "curv_d", "start_d", "pos_d", "val_d", "status_d", "span_d", "state_d")


def _chunk_args():
    """_spans_args' values (every pointer an address nothing dereferences: validation comes before any HIP call) plus the two new fields."""
    a, b = _lib.FollowChunkArgs(), _spans_args()
    for name, _ in _lib.FollowSpansArgs._fields_:
        setattr(a, name, getattr(b, name))
    a.state_d, a.t_base = 4096, 8
    return a


def test_the_export_the_header_and_the_version():
    lib = _lib.load()
    assert CALL in _lib.EXPORTS and hasattr(lib, CALL)
    header = open(os.path.join(ROOT, "include", "lec_hip.h")).read()
    assert "int lec_follow_spans_chunk(const lec_follow_chunk_args* args);" in header
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11          # an additive call


def test_the_struct_is_the_spans_struct_and_two_more_fields():
    S, A = _lib.FollowSpansArgs, _lib.FollowChunkArgs
    assert [f[0] for f in A._fields_] == [f[0] for f in S._fields_] + ["t_base", "state_d"]
    for name, _ in S._fields_:
        assert getattr(A, name).offset == getattr(S, name).offset, name
    assert ctypes.sizeof(S) == 160
    assert A.t_base.offset == 160 and A.t_base.size == 4 and A.state_d.offset == 168 and ctypes.sizeof(A) == 160 + 4 + 4 + 8 == 176
    # the existing follow structs have not moved
    assert ctypes.sizeof(_lib.FollowSeedsArgs) == 144 and ctypes.sizeof(_lib.FollowManyArgs) == 144 and ctypes.sizeof(_lib.FollowArgs) == 136
    assert ctypes.sizeof(_lib.FollowSeedsSeriesArgs) == 152 and S.span_d.offset == 144 and S.end_threshold.offset == 112


def test_null_args():
    lib = _lib.load()
    assert lib.lec_follow_spans_chunk(None) == 1
    assert lib.lec_last_error().startswith(CALL.encode() + b":") and b"null args" in lib.lec_last_error()


@pytest.mark.parametrize("change, word", [({p: None}, p.encode()) for p in CHUNK_POINTERS if p != "hgt_d"] + [
    ({"t_base": -1}, b"t_base"), ({"nt": 0}, b"nt"), ({"patience": -1}, b"patience"), ({"n_chains": 0}, b"n_chains"), ({"sj": 0}, b"sj"),
    ({"si": -3}, b"si"), ({"ny": 2}, b"3 x 3"), ({"field": 2}, b"field"), ({"sense": -1}, b"sense"), ({"smooth_r": -1}, b"smooth_r"),
    ({"jlo": 30}, b"jlo"), ({"ihi": 41}, b"ihi"), ({"field": _lib.FOLLOW_HGT, "hgt_d": None}, b"hgt_d"),
    ({"t_base": 2 ** 31 - 4, "nt": 4}, b"t_base + nt")])
def test_bad_arguments_are_refused_without_a_gpu(change, word):
    _refused(CALL, _chunk_args(), change, 1, word)


def test_the_largest_series_step_and_patience_0_pass_the_validation_of_the_scalars():
    """t_base + nt = 2^31 - 1 is the last sum that fits; what is refused next is the tile, which comes after every scalar."""
    big = {"ny": 400, "nx": 400, "jhi": 300, "ihi": 300, "sj": 70, "si": 70, "smooth_r": 2}
    _refused(CALL, _chunk_args(), dict(big, t_base=2 ** 31 - 5, nt=4, patience=0), 2, b"145 x 145")


def test_the_over_limit_tile_is_refused_with_both_figures():
    change = {"ny": 400, "nx": 400, "jhi": 300, "ihi": 300, "sj": 70, "si": 70, "smooth_r": 2}          # as lec_follow_many: 145 x 145 doubles
    msg = _refused(CALL, _chunk_args(), change, 2, b"145 x 145")
    assert b"168200" in msg and b"163776" in msg


def test_patience_0_is_still_refused_by_lec_follow_spans():
    _refused("lec_follow_spans", _spans_args(), {"patience": 0}, 1, b"patience")


# ---------------------------------------------------------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------------------------------------------------------
def _tiles(chunks, nt):
    assert chunks[0][0] == 0 and chunks[-1][1] == nt
    assert all(a < b for a, b in chunks) and all(chunks[n][1] == chunks[n + 1][0] for n in range(len(chunks) - 1))


def test_slice_chunks():
    assert fw.SLICE_BYTES == 2 << 30
    assert fw.slice_chunks(8760, 33, 41) == [(0, 8760)]                                         # 285 MB: it fits
    assert fw.slice_chunks(5, 33, 41, asked=1) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert fw.slice_chunks(5, 33, 41, asked=9) == [(0, 5)] and fw.slice_chunks(5, 33, 41, asked=5) == [(0, 5)]
    assert fw.slice_chunks(5, 33, 41, asked=2) == [(0, 2), (2, 4), (4, 5)]                      # the last one shorter
    # exactly the budget is one chunk, a byte less is not
    step = 24 * 361 * 1440
    assert fw.slice_chunks(100, 361, 1440, budget=100 * step) == [(0, 100)]
    assert len(fw.slice_chunks(100, 361, 1440, budget=100 * step - 1)) == 2
    for nt, budget_steps in ((8760, 172), (100, 99), (100, 51), (100, 50), (100, 49), (7, 3), (7, 1), (1, 1)):
        chunks = fw.slice_chunks(nt, 361, 1440, budget=budget_steps * step + 5)
        _tiles(chunks, nt)
        sizes = [b - a for a, b in chunks]
        assert max(sizes) * step <= budget_steps * step + 5, (nt, budget_steps, sizes)
        assert len(chunks) == -(-nt // budget_steps), (nt, budget_steps, sizes)                  # no more chunks than the budget asks for
        assert max(sizes) - min(sizes[:-1] or sizes) == 0 and sizes[-1] <= sizes[0]              # equal chunks, the last one may be shorter
    # a year of hourly steps of the southern hemisphere at 0.25 degrees under the default budget
    chunks = fw.slice_chunks(8760, 361, 1440)
    _tiles(chunks, 8760)
    assert len(chunks) == -(-8760 // (fw.SLICE_BYTES // step)) == 51 and max(b - a for a, b in chunks) * step <= fw.SLICE_BYTES
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError):
            fw.slice_chunks(5, 33, 41, asked=bad)


# ---------------------------------------------------------------------------------------------------------------------------
# reading a range of time steps
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample():
    a = types.SimpleNamespace(infile=TESTDATA, mpas=False, choose_domain=None)
    return fw.search_domain_slices(a, NAMELIST)


def test_search_domain_slices_reads_a_range_of_time_steps(sample):
    a = types.SimpleNamespace(infile=TESTDATA, mpas=False, choose_domain=None)
    part = fw.search_domain_slices(a, NAMELIST, None, t_range=(1, 4))
    assert part[0].shape == (3, 33, 41)
    for n in range(3):
        assert part[n].dtype == np.float64 and np.array_equal(part[n], sample[n][1:4], equal_nan=True)
    for n in (3, 4, 5):                                                # lat, lon and time are the whole series'
        assert np.array_equal(part[n], sample[n])
    assert len(part[5]) == 5


# ---------------------------------------------------------------------------------------------------------------------------
# the resumed chain, restated
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_chunked_restatement_gives_the_whole_series_restatement_on_the_sample(sample):
    u, v, h, lat, lon, _ = sample
    whole = fl.lifecycle(u, v, h, lat, lon, k=8, threshold=-5e-5)
    born = whole["births"]
    assert len(born) == 6 == len(SAMPLE)
    starts = [b[:3] for b in born]
    for size in (1, 2, 3, 5):
        sizes = [size] * (5 // size) + ([5 % size] if 5 % size else [])
        pos, val, status, span, state = fc.walk_chunked(u, v, h, lat, lon, starts, sizes, end_threshold=-5e-5, patience=2)
        for c, ref in enumerate(whole["chains"]):
            assert np.array_equal(pos[c], ref["pos"]) and np.array_equal(status[c], ref["status"]), (size, c, pos[c].tolist(), status[c])
            assert np.array_equal(val[c], ref["val"], equal_nan=True), (size, c)
            assert tuple(span[c]) == ref["span"], (size, c, span[c], ref["span"])
            assert state[c][0] in (fc.WALKING, fc.STOPPED) and tuple(state[c][4:6]) == ref["span"] and state[c][6:] == [0, 0]
            assert (state[c][0] == fc.STOPPED) == _stops(ref), (size, c, state[c])
        # ... and so the pinned outcome: six births, four tracks
        chains = [{"pos": pos[c], "span": tuple(int(x) for x in span[c])} for c in range(6)]
        kept, cont = fl.resolve(born, chains, whole["ej"], whole["ei"])
        outcome = ["never good" if ch["span"][0] < 0 else "continuation" if cont[c] is not None else
                   "too short" if ch["span"][1] - ch["span"][0] + 1 < 2 else "kept" for c, ch in enumerate(chains)]
        assert outcome == [row[3] for row in SAMPLE] and outcome.count("kept") == 4
        assert [None if o == "continuation" else ch["span"] for o, ch in zip(outcome, chains)] == [row[2] for row in SAMPLE]
        assert [(t0, (float(lat[j]), float(lon[i]))) for t0, j, i, _ in born] == [row[:2] for row in SAMPLE]


def _stops(ref):
    """Whether the whole-series chain used its patience (2) up -- at the last step of the series included."""
    weak = 0
    for s, x in zip(ref["status"], ref["val"]):
        if s == fc.NOT_LIVE:
            continue
        weak = 0 if (s == 0 and x <= -5e-5) else weak + 1
        if weak == 2:
            return True
    return False


def test_the_restated_phases_on_a_hand_made_series():
    """hgt with smooth 0: S is the planted doubles.  One low that is deep at steps 2..4 of 8; patience 2 ends it after step 6."""
    lat, lon = -40.0 + 2.5 * np.arange(17), -60.0 + 2.5 * np.arange(21)
    h = np.full((8, 17, 21), 1500.0)
    for t, depth in enumerate([1499, 1499, 1400, 1400, 1400, 1499, 1499, 1400]):
        h[t, 8, 6 + t] = depth
    kw = dict(field="hgt", end_threshold=1450.0, patience=2, length=10.0, width=10.0, search=2.5)
    starts = [(1, 8, 7), (-1, 8, 7), (1, 0, 0), (9, 8, 7)]
    for sizes in ([8], [1] * 8, [3, 1, 4], [6, 2]):
        pos, val, status, span, state = fc.walk_chunked(np.zeros_like(h), np.zeros_like(h), h, lat, lon, starts, sizes, **kw)
        assert status[0].tolist() == [3, 0, 0, 0, 0, 0, 0, 3] and span[0].tolist() == [2, 4] and state[0][0] == fc.STOPPED, (sizes, status[0])
        assert pos[0, 1:7, 1].tolist() == [7, 8, 9, 10, 11, 12]
        for c in (1, 2):
            assert np.all(status[c] == fc.BAD_START) and span[c].tolist() == [-1, -1] and state[c][0] == fc.BAD
        assert np.all(status[3] == fc.NOT_LIVE) and span[3].tolist() == [-1, -1] and state[3] == [0] * 8      # never born: t0 beyond the series


# ---------------------------------------------------------------------------------------------------------------------------
# the host's drivers, with the restatement in the device's place
# ---------------------------------------------------------------------------------------------------------------------------
SETTINGS = dict(length=15.0, width=15.0, smooth=0, field="zeta", hemisphere="south", formulation="metpy_no_crs")


@pytest.fixture
def restated_device(monkeypatch):
    """follow.find_systems_series and follow.follow_spans_chunk answered by the NumPy restatements (CPU tensors for the state): what is
    left under test is the drivers' own bookkeeping -- the births across a border, the growing table, the assembly of the chunks."""
    import torch
    from tests import follow_restatement as fr

    def series(u, v, h, lat, lon, *, k, threshold=None, separation=None, device=None, chunk_steps=None, hemisphere=None, **kw):
        u, v, h = (x.cpu().numpy() for x in (u, v, h))
        found = fl.seeds_series(u, v, h, lat, lon, k=k, threshold=threshold, separation=separation, **kw)
        pos, val, n = np.full((len(u), k, 2), -2, dtype=np.int32), np.full((len(u), k), np.nan), np.zeros(len(u), dtype=np.int32)
        for t, s in enumerate(found):
            n[t] = s["n_found"]
            pos[t, :n[t]], val[t, :n[t]] = s["pos"], s["val"]
        return pos, val, n

    def chunk(u, v, h, lat, lon, *, starts, state, t_base, end_threshold=None, patience=2, device=None, **kw):
        u, v, h = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (u, v, h))
        rows = [[int(x) for x in r] for r in state.cpu().numpy()]
        table = [tuple(int(x) for x in r) for r in (starts.cpu().numpy() if isinstance(starts, torch.Tensor) else starts)]
        pos, val, status, span = fc.chunk_call(u, v, h, lat, lon, t_base, table, rows, end_threshold=end_threshold, patience=patience, **kw)
        state.copy_(torch.as_tensor(np.array(rows, dtype=np.int32)))
        return pos.astype(np.int32), val, status.astype(np.int32), span.astype(np.int32)

    monkeypatch.setattr(fw, "find_systems_series", series)
    monkeypatch.setattr(fw, "follow_spans_chunk", chunk)
    return fr


@pytest.mark.parametrize("size", [1, 2, 3, 4])
def test_the_lifecycle_driver_in_chunks_gives_the_whole_series_arrays(sample, restated_device, size):
    u, v, h, lat, lon, _ = sample
    ref = fl.lifecycle(u, v, h, lat, lon, k=8, threshold=-5e-5)
    src = fw._SliceSource(types.SimpleNamespace(infile=TESTDATA, mpas=False, choose_domain=None), NAMELIST)
    try:
        chunks = fw.slice_chunks(5, 33, 41, asked=size)
        born, born_val, pos, val, status, span, n_seeds, n_births = fw._lifecycle_chunks(
            src, chunks, src.read(chunks[0]), None, k=8, threshold=-5e-5, sep=(7.5, 7.5), sj=ref["sj"], si=ref["si"], end_threshold=-5e-5, patience=2,
            search=5.0, device="cpu", **SETTINGS)
    finally:
        src.close()
    assert [tuple(b) for b in born.tolist()] == ref["births"] and n_births == 6 and n_seeds == sum(s["n_found"] for s in ref["series"])
    assert pos.shape == (6, 5, 2) and val.shape == status.shape == (6, 5)
    for c, chain in enumerate(ref["chains"]):
        assert np.array_equal(pos[c], chain["pos"]) and np.array_equal(status[c], chain["status"]) and tuple(span[c]) == chain["span"], (size, c)
        assert np.array_equal(val[c], chain["val"], equal_nan=True)
        t0, _, _, rank = ref["births"][c]
        assert born_val[c] == ref["series"][t0]["val"][rank]


@pytest.mark.parametrize("size", [1, 2, 3])
def test_the_plain_driver_resumes_the_chain_of_the_first_chunk(sample, restated_device, size):
    u, v, h, lat, lon, _ = sample
    one = restated_device.follow(u, v, h, lat, lon, start=(-22.5, -45.0))
    src = fw._SliceSource(types.SimpleNamespace(infile=TESTDATA, mpas=False, choose_domain=None), NAMELIST)
    try:
        chunks = fw.slice_chunks(5, 33, 41, asked=size)
        n0 = chunks[0][1]
        first = one["pos"][None, :n0].astype(np.int32), one["val"][None, :n0], one["status"][None, :n0].astype(np.int32)
        pos, val, status = fw._resume_chunks(src, chunks, *first, first[0][:, 0], search=5.0, device="cpu", **SETTINGS)
    finally:
        src.close()
    assert np.array_equal(pos[0], one["pos"]) and np.array_equal(status[0], one["status"]) and np.array_equal(val[0], one["val"])


# ---------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv, word", [
    (["-r", "-t", "--choose-chunk", "2"], "--choose-chunk goes with -c"),
    (["-r", "-c", "--choose-chunk", "0"], "--choose-chunk must be >= 1"),
    (["-r", "-c", "--choose-systems", "2", "--choose-chunk", "-3"], "--choose-chunk must be >= 1"),
])
def test_command_line_refusals_leave_nothing_behind(tmp_path, monkeypatch, argv, word):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main([TESTDATA] + argv)
    assert word in str(e.value)
    assert os.listdir(tmp_path) == []                                 # no LEC_Results


def test_the_option_is_parsed_and_listed():
    import lorenzcycletoolkit
    args = lorenzcycletoolkit.create_arg_parser().parse_args(["f.nc", "-r", "-c", "--choose-chunk", "24"])
    assert args.choose_chunk == 24 and "choose_chunk" in lorenzcycletoolkit.CHOOSE_OPTIONS
    lorenzcycletoolkit.refuse_choose_options(args)
    assert lorenzcycletoolkit.create_arg_parser().parse_args(["f.nc", "-r", "-c"]).choose_chunk is None
    assert "--choose-chunk" in " ".join(lorenzcycletoolkit.create_arg_parser().format_help().split())
