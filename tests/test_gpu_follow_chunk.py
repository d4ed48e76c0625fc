"""-c --choose-chunk on the GPU: ``lec_follow_spans_chunk`` over every cut of a series against ONE ``lec_follow_spans`` call on the whole
series, bit for bit -- the phase transitions and the hand-over of centre and counters at the borders, each its own case --, with
patience 0 against ``lec_follow_many``, the bad table entries, the chain table grown between calls, and the command line on the NCEP-R2
sample: every file of a chunked run is the file of the run without the option."""
import filecmp
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib, follow as fw
from tests.test_gpu_follow_lifecycle import BOX, LIFECYCLE, LYSIS_THRESHOLD, STEM, STRONG, WEAK, _main, _tree_files, _workdir, planted

NOT_LIVE, BAD_START = _lib.FOLLOW_NOT_LIVE, _lib.FOLLOW_BAD_START
bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
NT = 12
LAT, LON = -40.0 + np.arange(33.0), -60.0 + np.arange(41.0)
HGT = dict(field="hgt", smooth=0, length=10.0, width=10.0, search=3.0)       # S is the planted doubles themselves; sj = si = 3
JLO, JHI, ILO, IHI = 5, 27, 5, 35                                            # the admissible centres of a 10 x 10 box
END = 1450.0                                                                 # good: at most this deep
G, W = 1400.0, 1480.0                                                        # a good step, a weak one (still the window's minimum: the noise is 1500 +- 2)


def heights(systems, blind=()):
    """[NT][33][41] heights: 1500 and noise, and per system (t0, j, i, dj, di, depths) the value depths[n] at (j + n dj, i + n di) of step
    t0 + n.  blind: (t, j, i) -- the 7 x 7 window around (j, i) of step t holds no finite value."""
    h = 1500.0 + 2.0 * np.random.default_rng(5).uniform(-1.0, 1.0, (NT, LAT.size, LON.size))
    for t0, j, i, dj, di, depths in systems:
        for n, d in enumerate(depths):
            h[t0 + n, j + n * dj, i + n * di] = d
    for t, j, i in blind:
        h[t, j - 3: j + 4, i - 3: i + 4] = np.nan
    return h


def sizes_of(size):
    return [size] * (NT // size) + ([NT % size] if NT % size else [])


def chunked(u, v, h, lat, lon, starts, sizes, known=None, **kw):
    """The series cut into consecutive chunks of ``sizes`` steps, ONE zeroed state carried through the calls; every call gets freshly
    allocated outputs (follow_spans_chunk makes them).  known: per chunk the number of chains of the table the call is given (the table
    grows between calls, the new state rows zeroed).  -> (pos, val, status concatenated over the chunks, the last call's span, the state)."""
    assert sum(sizes) == len(u)
    starts = np.asarray(starts, dtype=np.int32).reshape(-1, 3)
    K = len(starts)
    state = torch.zeros((K, 8), dtype=torch.int32, device="cuda:0")
    pos, val = np.full((K, len(u), 2), -1, dtype=np.int32), np.full((K, len(u)), np.nan)
    status = np.full((K, len(u)), NOT_LIVE, dtype=np.int32)
    a = 0
    for n, size in enumerate(sizes):
        k = K if known is None else known[n]
        cut = lambda x: None if x is None else x[a: a + size]
        p, x, s, span = fw.follow_spans_chunk(cut(u), cut(v), cut(h), lat, lon, starts=starts[:k], state=state[:k], t_base=a, **kw)
        assert p.shape == (k, size, 2) and x.shape == s.shape == (k, size) and span.shape == (k, 2)
        pos[:k, a: a + size], val[:k, a: a + size], status[:k, a: a + size] = p, x, s
        a += size
    return pos, val, status, span, state.cpu().numpy()


def same(got, ref, what):
    assert np.array_equal(got[2], ref[2]), (what, got[2].tolist(), ref[2].tolist())
    assert np.array_equal(got[0], ref[0]), (what, got[0].tolist(), ref[0].tolist())
    assert np.array_equal(bits(got[1]), bits(ref[1])), (what, got[1], ref[1])                   # the raw 64 bits of every val, NaNs included
    assert np.array_equal(got[3], ref[3]), (what, got[3].tolist(), ref[3].tolist())


def hgt_case(systems, starts, cuts, patience=2, blind=()):
    h = heights(systems, blind)
    z = np.zeros_like(h)
    kw = dict(HGT, end_threshold=END, patience=patience)
    ref = fw.follow_spans(z, z, h, LAT, LON, starts=np.asarray(starts, dtype=np.int32), **kw)
    out = []
    for sizes in cuts:
        got = chunked(z, z, h, LAT, LON, starts, sizes, **kw)
        same(got, ref, sizes)
        out.append(got)
    return ref, out


# three lows: one from step 0 that weakens from step 5 on, one from step 3 that weakens from step 9 on, one from step 7 to the end
THREE = [(0, 10, 8, 0, 1, [G] * 5 + [W] * 7), (3, 22, 20, -1, 0, [G] * 6 + [W] * 3), (7, 15, 30, 0, -1, [G] * 5)]
THREE_STARTS = [(0, 10, 8), (3, 22, 20), (7, 15, 30)]


def test_every_cut_is_the_one_shot_call():
    cuts = [sizes_of(n) for n in (1, 2, 5, 11, 12)] + [[3, 1, 6, 2]]
    ref, out = hgt_case(THREE, THREE_STARTS, cuts)
    # the construction holds: the chains are on their lows while these are good, and end two steps after
    assert ref[3].tolist() == [[0, 4], [3, 8], [7, 11]]
    assert ref[2][0].tolist() == [0] * 7 + [NOT_LIVE] * 5 and ref[2][1].tolist() == [NOT_LIVE] * 3 + [0] * 8 + [NOT_LIVE] and ref[2][2].tolist() == [NOT_LIVE] * 7 + [0] * 5
    assert ref[0][0, :7].tolist() == [[10, 8 + t] for t in range(7)] and ref[1][0, :7].tolist() == [G] * 5 + [W] * 2
    for got in out:
        assert got[4][:, 0].tolist() == [2, 2, 1] and got[4][:, 3].tolist()[:2] == [2, 2] and np.all(got[4][:, 6:] == 0)       # stopped, stopped, walking
        assert got[4][2, 1:3].tolist() == [15, 26]                                                                           # the centre after the last step


@pytest.mark.parametrize("what, cut", [
    ("the two weak steps on either side of a border", [6, 6]),
    ("the stopping step is the last step of a chunk", [7, 5]),
    ("a birth at the first local step", [3, 9]),
    ("a birth at the last local step", [4, 8]),
    ("a birth two chunks after the first", [3, 3, 6]),
])
def test_borders_of_the_three_lows(what, cut):
    hgt_case(THREE, THREE_STARTS, [cut])


def test_a_blind_window_at_the_last_step_of_a_chunk():
    """Step 5's window holds no finite value: the centre of step 4 is kept, and step 6 -- the next chunk's first -- searches around it."""
    systems = [(0, 12, 10, 0, 1, [G] * 12)]
    ref, _ = hgt_case(systems, [(0, 12, 10)], [[6, 6], [5, 7], [6, 1, 5]], blind=[(5, 12, 14)])
    assert ref[2][0].tolist() == [0] * 5 + [1] + [0] * 6 and ref[0][0, 4:7].tolist() == [[12, 14], [12, 14], [12, 16]] and ref[3][0].tolist() == [0, 11]
    # ... and with patience 1 the blind step is the stopping step: phase 2 on entry
    ref, _ = hgt_case(systems, [(0, 12, 10)], [[6, 6], [5, 7]], patience=1, blind=[(5, 12, 14)])
    assert ref[2][0].tolist() == [0] * 5 + [1] + [NOT_LIVE] * 6 and ref[3][0].tolist() == [0, 4]


def test_a_chain_that_is_never_good():
    systems = [(0, 12, 10, 0, 1, [W] * 12)]
    ref, out = hgt_case(systems, [(0, 12, 10)], [[1, 11], [2, 10], [4, 4, 4]], patience=2)
    assert ref[3][0].tolist() == [-1, -1] and ref[2][0].tolist() == [0, 0] + [NOT_LIVE] * 10
    assert all(got[3][0].tolist() == [-1, -1] and got[4][0, 0] == 2 for got in out)
    ref, out = hgt_case(systems, [(0, 12, 10)], [[4, 4, 4], [11, 1]], patience=20)                # ... and one that walks to the end without a good step
    assert ref[3][0].tolist() == [-1, -1] and ref[2][0].tolist() == [0] * 12
    assert all(got[3][0].tolist() == [-1, -1] and got[4][0].tolist() == [1, 12, 21, 12, -1, -1, 0, 0] for got in out)


def test_first_good_step_in_chunk_1_and_last_good_step_in_chunk_3():
    systems = [(0, 12, 10, 0, 1, [W, W, W, G, G, W, W, G, W, G, W, W])]
    ref, out = hgt_case(systems, [(0, 12, 10)], [[3, 3, 3, 3]], patience=4)
    assert ref[3][0].tolist() == [3, 9] and ref[2][0].tolist() == [0] * 12
    assert out[0][4][0].tolist() == [1, 12, 21, 2, 3, 9, 0, 0]


def scaled(pattern, stretched, seed=11):
    """planted()'s moving vortex over noise with the wind of step t scaled by pattern[t] (test_gpu_follow_lifecycle.py's _scaled, on either axis)."""
    lat, lon, u, v, h, start, rival = planted(seed=seed, nt=len(pattern), stretched=stretched)
    f = np.asarray(pattern, dtype=np.float64)[:, None, None]
    return lat, lon, u * f, v * f, h, start, rival


PATTERN = [STRONG, STRONG, WEAK, STRONG, STRONG, WEAK, WEAK, STRONG, STRONG, STRONG, WEAK, STRONG]


@pytest.fixture(scope="module")
def vortex():
    """(stretched) -> the series and its table of starts, built once per axis."""
    made = {}

    def get(stretched):
        if stretched not in made:
            lat, lon, u, v, h, start, rival = scaled(PATTERN, stretched)
            bounds = fw.admissible(lat, lon, BOX["length"], BOX["width"])
            on, off = fw.start_index(lat, lon, start, bounds), fw.start_index(lat, lon, rival, bounds)
            whole = fw.follow_system(u, v, h, lat, lon, start=start, **BOX)
            table = [(0, *on), (0, *off), (3, *(int(x) for x in whole[0][3])), (9, *(int(x) for x in whole[0][9])), (4, bounds[0] + 2, bounds[2] + 3)]
            made[stretched] = (lat, lon, u, v, h, table)
        return made[stretched]
    return get


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("stretched", [False, True])
def test_zeta_in_chunks_of_4_is_the_one_shot_call(vortex, stretched, r):
    lat, lon, u, v, h, table = vortex(stretched)
    kw = dict(BOX, smooth=r, end_threshold=LYSIS_THRESHOLD, patience=2)
    ref = fw.follow_spans(u, v, h, lat, lon, starts=np.array(table, dtype=np.int32), **kw)
    print("zeta", stretched, r, "spans", ref[3].tolist(), "status", ref[2].tolist())
    same(chunked(u, v, h, lat, lon, table, [4, 4, 4], **kw), ref, (stretched, r))
    # the vortex is good where PATTERN has it at full strength: steps 0-1 and 3-4, then two weak steps end both chains in the second chunk;
    # the chain born on it at step 3 -- the last step of the first chunk -- has steps 3-4 alone
    assert ref[3][0].tolist() == [0, 4] and ref[3][2].tolist() == [3, 4] and np.all(ref[2][2, :3] == NOT_LIVE) and np.all(ref[2][2, 7:] == NOT_LIVE)


def test_patience_0_is_lec_follow_many_on_300_chains(vortex):
    lat, lon, u, v, h, table = vortex(False)
    places = [t[1:] for t in table] + [(t[1] + 1, t[2] - 2) for t in table[:3]]
    seeds = np.array([places[c % len(places)] for c in range(300)], dtype=np.int32)
    kw = dict(BOX, smooth=1)
    many = fw.follow_systems(u, v, h, lat, lon, seeds=seeds, **kw)
    starts = np.c_[np.zeros(300, dtype=np.int32), seeds]
    got = chunked(u, v, h, lat, lon, starts, [5, 5, 2], patience=0, end_threshold=LYSIS_THRESHOLD, **kw)
    assert np.array_equal(got[0], many[0]) and np.array_equal(got[2], many[2]) and np.array_equal(bits(got[1]), bits(many[1]))
    assert np.all(got[4][:, 0] == 1)                                     # none has stopped, weak steps or not
    assert np.any(got[4][:, 3] >= 2)
    none = chunked(u, v, h, lat, lon, starts[:8], [5, 5, 2], patience=0, **kw)                   # ... and without a threshold
    assert np.array_equal(none[0], many[0][:8]) and np.array_equal(bits(none[1]), bits(many[1][:8]))


def test_bad_table_entries_read_nothing_in_any_chunk():
    good = (0, 10, 8)
    bad = [(7, JLO - 1, ILO), (7, JHI + 1, ILO), (2, JLO, ILO - 1), (0, JLO, IHI + 1), (0, -1, -1), (5, -2, -2), (-1, 10, 8), (-1, -1, -1)]
    table = [good] + bad + [good, (3, 22, 20)]
    h = heights(THREE)
    z = np.zeros_like(h)
    kw = dict(HGT, end_threshold=END, patience=2)
    alone = fw.follow_spans(z, z, h, LAT, LON, starts=np.array([good, (3, 22, 20)], dtype=np.int32), **kw)
    for sizes in ([3, 4, 5], [12], sizes_of(1)):
        pos, val, status, span, state = chunked(z, z, h, LAT, LON, table, sizes, **kw)
        for c in range(1, len(bad) + 1):                                 # at every step of every chunk, those before t0 included
            assert np.all(status[c] == BAD_START) and np.all(pos[c] == -1) and np.all(np.isnan(val[c])) and span[c].tolist() == [-1, -1], (sizes, c)
            assert state[c].tolist() == [3, -1, -1, 0, -1, -1, 0, 0]
        for c, one in ((0, 0), (len(bad) + 1, 0), (len(bad) + 2, 1)):    # their neighbours in the launch are the chains they are alone
            same(tuple(a[c] for a in (pos, val, status, span)), tuple(a[one] for a in alone), (sizes, c))


def test_the_state_is_the_whole_hand_over():
    """The chain table grown between the calls -- only the chains born so far, new rows with zeroed state -- and outputs allocated anew
    by every call give the bits of the calls on the whole table."""
    h = heights(THREE)
    z = np.zeros_like(h)
    kw = dict(HGT, end_threshold=END, patience=2)
    ref = fw.follow_spans(z, z, h, LAT, LON, starts=np.array(THREE_STARTS, dtype=np.int32), **kw)
    for sizes, known in (([3, 1, 6, 2], [1, 2, 3, 3]), ([2, 2, 2, 2, 2, 2], [1, 2, 2, 3, 3, 3]), ([4, 8], [2, 3])):
        same(chunked(z, z, h, LAT, LON, THREE_STARTS, sizes, known=known, **kw), ref, (sizes, known))


def test_bad_scalars_are_refused_and_nothing_is_launched():
    h = heights(THREE)
    z = np.zeros_like(h)
    state = torch.full((1, 8), 77, dtype=torch.int32, device="cuda:0")
    for change, word in (({"t_base": -1}, "t_base"), ({"patience": -1}, "patience"), ({"t_base": 2 ** 31 - 5}, "t_base")):
        with pytest.raises(ValueError, match=word):
            fw.follow_spans_chunk(z, z, h, LAT, LON, starts=[(0, 10, 8)], state=state, **dict(dict(HGT, t_base=0, patience=2), **change))
    torch.cuda.synchronize()
    assert bool((state == 77).all())
    with pytest.raises(ValueError, match="state: needs"):
        fw.follow_spans_chunk(z, z, h, LAT, LON, starts=[(0, 10, 8)], state=np.zeros((1, 8), dtype=np.int32), t_base=0, **HGT)


# ---------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------
PLAIN = ["-r", "-c", "--choose-start", "-22.5", "-45"]
MANY = ["-r", "-c", "--choose-systems", "2"]


def _run(path, golden_dir, argv, keep):
    """One run in ``path``; its LEC_Results is moved to ``keep`` (the relative paths the run writes into its files stay the same)."""
    before = os.getcwd()
    world = os.environ.pop("WORLD_SIZE", None)
    os.chdir(path)
    try:
        _main([os.path.join(golden_dir, STEM + ".nc")] + argv)
    finally:
        os.chdir(before)
        if world is not None:
            os.environ["WORLD_SIZE"] = world
    os.rename(path / "LEC_Results", path / keep)
    return path / keep


@pytest.fixture(scope="module")
def resident(tmp_path_factory, golden_dir):
    """mode -> (the working directory, the results of the run without --choose-chunk): one run per mode, shared."""
    made = {}

    def get(mode, argv):
        if mode not in made:
            path = _workdir(tmp_path_factory.mktemp(mode), golden_dir)
            made[mode] = (path, _run(path, golden_dir, argv, "resident"))
        return made[mode]
    return get


@pytest.mark.parametrize("mode, argv, chunk", [("lifecycle", LIFECYCLE, 2), ("lifecycle", LIFECYCLE, 1), ("plain", PLAIN, 2), ("many", MANY, 3)])
def test_cli_a_chunked_run_writes_the_files_of_the_resident_run(resident, golden_dir, mode, argv, chunk):
    path, whole = resident(mode, argv)
    got = _run(path, golden_dir, argv + ["--choose-chunk", str(chunk)], f"chunk{chunk}")
    files = _tree_files(whole)
    assert files == _tree_files(got) and len([f for f in files if not f.endswith("/")]) >= 23
    batch = f"{STEM}_choose_batch/"
    if mode != "plain":
        assert batch + "systems.csv" in files and batch + "batch.csv" in files and batch + "choose_s01" in files
    else:
        assert f"{STEM}_choose/{STEM}_choose_track" in files
    for f in files:
        if not f.endswith("/"):
            assert filecmp.cmp(whole / f, got / f, shallow=False), f
    log = (got / (f"{STEM}_choose" if mode == "plain" else f"{STEM}_choose_batch") / f"log.{STEM}").read_text()
    n = -(-5 // chunk)
    assert "lec_follow_spans_chunk" in log and f"{n} chunks of {chunk} time steps" in log, log
    assert "lec_follow_spans_chunk" not in (whole / (f"{STEM}_choose" if mode == "plain" else f"{STEM}_choose_batch") / f"log.{STEM}").read_text()
