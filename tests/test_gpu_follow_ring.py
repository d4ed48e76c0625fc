"""-c --choose-periodic on the GPU: ``lec_follow_spans_chunk_ring`` and ``lec_follow_seeds_series_ring`` against the existing kernels where
the ring cannot matter (mid-domain: equal, bit for bit), against the existing kernels on rolled data where it must not matter (``hgt``
across the seam: bit for bit), and against the NumPy restatement of the rule (tests/follow_ring_restatement.py) with the bars of
tests/test_gpu_follow.py.  The cases' margins are checked without a GPU in tests/test_follow_ring_cpu.py."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib
from lorenzcycletoolkit_amd import follow as fw
from tests import follow_ring_cases as rc
from tests import follow_ring_restatement as rr
from tests.test_follow_ring_cpu import _chunk_args, _seeds_args
from tests.test_gpu_follow import NEAR_TIE, VALUE_BAR

LAT, LON, NT = rc.LAT, rc.LON, rc.NT
NX = LON.size
DEV = "cuda:0"
bits = lambda a: np.ascontiguousarray(a).view(np.int64)


def chunked(u, v, h, starts, sizes, periodic=True, lon=LON, box=rc.BOX, **kw):
    """The series cut into consecutive chunks of ``sizes`` steps, ONE zeroed state carried through the calls -> (pos [K][nt][2], val,
    status [K][nt], the last span, [the state after every chunk])."""
    assert sum(sizes) == len(u)
    starts = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1, 3)
    state = torch.zeros((len(starts), 8), dtype=torch.int32, device=DEV)
    parts, states, a = [], [], 0
    for size in sizes:
        cut = lambda x: None if x is None else x[a: a + size]
        parts.append(fw.follow_spans_chunk(cut(u), cut(v), cut(h), LAT, lon, starts=starts, state=state, t_base=a, periodic=periodic, **box, **kw))
        states.append(state.cpu().numpy().copy())
        a += size
    return (np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1),
            np.concatenate([p[2] for p in parts], axis=1), parts[-1][3], states)


def start_row(start):
    return [(0,) + rc.start_of(start)]


def compare(got, ref, what):
    """tests/test_gpu_follow.compare on chunk_call's dict: positions and status EQUAL; values within the bar; no step may be left out
    as a near tie."""
    pos, val, status = got[:3]
    ok = ref["status"] == 0
    err = np.abs(val[ok] - ref["val"][ok]) / ref["tile_scale"][ok]
    print(what, "margin min %.3e" % ref["margin"].min(), "worst value error / tile scale %.3e" % (err.max() if err.size else 0.0))
    assert int((ref["margin"] < NEAR_TIE).sum()) == 0, (what, ref["margin"])
    assert np.array_equal(status, ref["status"]), (what, status, ref["status"])
    assert np.array_equal(pos, ref["pos"]), (what, pos.tolist(), ref["pos"].tolist())
    assert np.all(np.isnan(val[~ok]))
    assert np.all(err <= VALUE_BAR), (what, val, ref["val"])


# ---- where the ring cannot matter -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 2])
@pytest.mark.parametrize("form", ["metpy_no_crs", "spherical"])
def test_interior_equals_the_existing_kernel(form, r):
    """Mid-domain the two calls read the same points through the same expressions with the same coefficients: pos, status, span and
    state equal, val bit for bit -- the chain and the seeds of every step."""
    u, v, h, start, _ = rc.planted(5, **rc.INTERIOR)
    kw = dict(smooth=r, field="zeta", formulation=form, patience=2, end_threshold=-1e-5)
    ring = chunked(u, v, h, start_row(start), [NT], periodic=True, **kw)
    plain = chunked(u, v, h, start_row(start), [NT], periodic=False, **kw)
    cols = ring[0][0, :, 1]
    assert ring[2].tolist() == [[0] * NT]
    assert cols.min() - rc.SI - r >= 1 and cols.max() + rc.SI + r <= NX - 2          # the precondition: no tile touches column 0 or nx - 1
    assert fw.admissible(LAT, LON, 10, 10)[2] <= cols.min() - rc.SI and cols.max() + rc.SI <= fw.admissible(LAT, LON, 10, 10)[3]
    for a, b in zip(ring[:4], plain[:4]):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(bits(ring[1]), bits(plain[1])) and np.array_equal(ring[4][-1], plain[4][-1])
    # the seeds: the planted system and its rival, both far from the seam (the threshold keeps the noise out)
    skw = dict(k=4, threshold=-2e-5, length=10.0, width=10.0, smooth=r, field="zeta", formulation=form)
    sr = fw.find_systems_series(u, v, h, LAT, LON, periodic=True, **skw)
    sp = fw.find_systems_series(u, v, h, LAT, LON, **skw)
    assert sr[2].tolist() == [2] * NT and np.all((sr[0][:, :2, 1] > 8) & (sr[0][:, :2, 1] < NX - 9))
    assert np.array_equal(sr[0], sp[0]) and np.array_equal(sr[2], sp[2]) and np.array_equal(bits(sr[1]), bits(sp[1]))


# ---- across the seam ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 2])
@pytest.mark.parametrize("case", ["EAST", "WEST"])
def test_hgt_across_the_seam_is_the_existing_kernel_on_rolled_data(case, r):
    """A ring has no preferred meridian: the lows that move through columns 69, 70, 71, 0, 1, 2 (and the other way) are followed exactly
    as the existing kernel follows them mid-domain on the data rolled by half a ring -- the columns shifted back, val bit for bit."""
    u, v, h, start, _ = rc.planted(11, **getattr(rc, case))
    kw = dict(smooth=r, field="hgt", patience=2, end_threshold=1480.0)
    t0, j, i = start_row(start)[0]
    ring = chunked(u, v, h, [(t0, j, i)], [NT], periodic=True, **kw)
    roll = lambda a: np.ascontiguousarray(np.roll(a, 36, axis=-1))
    plain = chunked(roll(u), roll(v), roll(h), [(t0, j, (i + 36) % NX)], [NT], periodic=False, **kw)
    cols = ring[0][0, :, 1].tolist()
    assert [c for n, c in enumerate(cols) if n == 0 or c != cols[n - 1]] == ([69, 70, 71, 0, 1, 2] if case == "EAST" else [2, 1, 0, 71, 70, 69])
    assert not ring[2].any() and np.array_equal(ring[2], plain[2]) and np.array_equal(ring[3], plain[3])
    assert np.array_equal(ring[0][..., 0], plain[0][..., 0]) and np.array_equal(ring[0][..., 1], (plain[0][..., 1] - 36) % NX)
    assert np.array_equal(bits(ring[1]), bits(plain[1]))
    # and the seeds of every step: the low is a seed at its ring column
    sr = fw.find_systems_series(u, v, h, LAT, LON, k=4, threshold=1480.0, length=10.0, width=10.0, smooth=r, field="hgt", periodic=True)
    sp = fw.find_systems_series(roll(u), roll(v), roll(h), LAT, LON, k=4, threshold=1480.0, length=10.0, width=10.0, smooth=r, field="hgt")
    assert sr[2].tolist() == [2] * NT and np.array_equal(sr[2], sp[2]) and np.array_equal(bits(sr[1]), bits(sp[1]))
    assert np.array_equal(sr[0][:, :2, 0], sp[0][:, :2, 0]) and np.array_equal(sr[0][:, :2, 1], (sp[0][:, :2, 1] - 36) % NX)
    assert np.all(sr[0][:, 2:] == -2) and np.all(sp[0][:, 2:] == -2)


@pytest.mark.parametrize("r", [0, 2])
@pytest.mark.parametrize("form", ["metpy_no_crs", "spherical"])
@pytest.mark.parametrize("case", ["EAST", "WEST"])
def test_zeta_across_the_seam_matches_the_restatement(case, form, r):
    u, v, h, start, _ = rc.planted(11, **getattr(rc, case))
    kw = dict(smooth=r, field="zeta", formulation=form, patience=2, end_threshold=-1e-5)
    got = chunked(u, v, h, start_row(start), [NT], **kw)
    ref = rr.walk_chunked(u, v, h, LAT, LON, start_row(start), [NT], **rc.BOX, **kw)
    compare(got, ref, (case, form, r))
    assert np.array_equal(got[3], ref["span"]) and got[3].tolist() == [[0, NT - 1]]
    assert {69, 70, 71, 0, 1, 2} <= set(got[0][0, :, 1].tolist())
    # the seeds of every step against the restatement's
    pos, val, n = fw.find_systems_series(u, v, h, LAT, LON, k=3, threshold=-2e-5, length=10.0, width=10.0, smooth=r, field="zeta", formulation=form,
                                         periodic=True)
    for t in range(NT):
        s = rr.seeds(u[t], v[t], h[t], LAT, LON, k=3, threshold=-2e-5, length=10.0, width=10.0, smooth=r, field="zeta", formulation=form)
        assert s["margin"] > NEAR_TIE, (t, s["margin"])
        assert n[t] == s["n_found"] == 2 and np.array_equal(pos[t, :n[t]], s["pos"]), (t, pos[t], s["pos"])
        assert np.all(np.abs(val[t, :n[t]] - s["val"]) <= VALUE_BAR * s["scale"])


def test_the_state_carries_the_crossing():
    """Every cut of the 12 steps, one of them exactly where the centre goes from column 71 to column 0: the state hands ic = 71 to the
    next chunk, and the concatenated result is the one-chunk call's, bit for bit."""
    u, v, h, start, _ = rc.planted(11, **rc.EAST)
    kw = dict(smooth=2, field="zeta", patience=2, end_threshold=-1e-5)
    one = chunked(u, v, h, start_row(start), [NT], **kw)
    cols = one[0][0, :, 1]
    cross = int(np.flatnonzero((cols[:-1] == 71) & (cols[1:] == 0))[0]) + 1                  # the first step at column 0
    cuts = [[c, NT - c] for c in range(1, NT)] + [[1] * NT, [5, 5, 2], [3, 1, 6, 2]]
    assert [cross, NT - cross] in cuts
    for sizes in cuts:
        got = chunked(u, v, h, start_row(start), sizes, **kw)
        for a, b in zip(got[:4], one[:4]):
            assert np.array_equal(a, b, equal_nan=True), sizes
        assert np.array_equal(bits(got[1]), bits(one[1])) and np.array_equal(got[4][-1], one[4][-1]), sizes
        if sizes == [cross, NT - cross]:
            assert got[4][0][0, :3].tolist() == [1, int(one[0][0, cross - 1, 0]), 71]
    # a carried ic outside [0, nx) is no state of the rule's: the chain counts as stopped, nothing is read
    starts = np.array(start_row(start), dtype=np.int32)
    state = torch.as_tensor(np.array([[1, 16, NX, 0, 0, 3, 0, 0]], dtype=np.int32)).to(DEV)
    pos, val, status, span = fw.follow_spans_chunk(u[4:], v[4:], h[4:], LAT, LON, starts=starts, state=state, t_base=4, periodic=True, **rc.BOX, **kw)
    assert np.all(status == _lib.FOLLOW_NOT_LIVE) and np.all(pos == -1) and np.all(np.isnan(val)) and span.tolist() == [[0, 3]]


@pytest.mark.parametrize("field", ["zeta", "hgt"])
def test_a_blind_window_on_the_seam_keeps_the_centre(field):
    u, v, h, start, _ = rc.planted(11, blind_step=6, **rc.EAST)
    kw = dict(smooth=1, field=field, patience=0)
    got = chunked(u, v, h, start_row(start), [NT], **kw)
    ref = rr.walk_chunked(u, v, h, LAT, LON, start_row(start), [NT], **rc.BOX, **kw)
    compare(got, ref, ("blind", field))
    pos, val, status = got[:3]
    assert status[0].tolist() == [0] * 6 + [1] + [0] * 5 and tuple(pos[0, 6]) == tuple(pos[0, 5]) and np.isnan(val[0, 6])
    assert pos[0, 5, 1] in (71, 0) and pos[0, -1, 1] in (1, 2, 3)                        # kept ON the seam, and the chain goes on across it


def _seeds_raw(call, h, bounds, periodic, ej=2, ei=1, k=4, threshold=1480.0):
    """One slice through ``call`` with the admissible centres given as they are (the product's admissible() would hide the edge columns
    from the non-ring call) -> the seeds' positions."""
    z = np.zeros_like(h)
    s = fw._Slices(z[None], z[None], h[None], LAT, LON, 3, length=10.0, width=10.0, smooth=0, field="hgt", hemisphere=None,
                   formulation="metpy_no_crs", device=DEV, periodic=periodic)
    s.bounds = bounds
    work = torch.empty((1,) + h.shape, dtype=torch.float64, device=DEV)
    pos = torch.empty((1, k, 2), dtype=torch.int32, device=DEV)
    val = torch.empty((1, k), dtype=torch.float64, device=DEV)
    n = torch.empty((1,), dtype=torch.int32, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = _lib.FollowSeedsSeriesArgs(nt=1, ej=ej, ei=ei, k_max=k, reserved0=0, threshold=threshold, work_d=ptr(work), seed_pos_d=ptr(pos),
                                      seed_val_d=ptr(val), n_found_d=ptr(n), **s.common())
    _lib.check(getattr(s.lib, call)(C.byref(args)), call)
    torch.cuda.synchronize()
    return pos.cpu().numpy()[0, :int(n.cpu().numpy()[0])].tolist()


def test_seeds_on_the_seam():
    """One low at column 0 with a weaker twin at column 71: ONE system.  The existing call, for which the slice ends at the seam, seeds
    it twice on the same slice -- the bug; the ring call sees the twin within ei of the low."""
    h = np.full((33, NX), 1500.0)
    h[16, 0], h[16, 71] = 1400.0, 1450.0
    every = (2, 30, 0, NX - 1)
    assert _seeds_raw("lec_follow_seeds_series", h, every, False) == [[16, 0], [16, 71]]
    assert _seeds_raw("lec_follow_seeds_series_ring", h, every, True) == [[16, 0]]
    pos, val, n = fw.find_systems_series(np.zeros((1, 33, NX)), np.zeros((1, 33, NX)), h[None], LAT, LON, k=4, threshold=1480.0, length=10.0, width=10.0,
                                         field="hgt", periodic=True)
    assert n.tolist() == [1] and pos[0, 0].tolist() == [16, 0] and val[0, 0] == 1400.0
    # a tie across the seam keeps the slice's absolute row-major order: column 0 comes before column 71
    h[16, 71] = 1400.0
    assert _seeds_raw("lec_follow_seeds_series_ring", h, every, True) == [[16, 0]]
    z = np.zeros((33, NX))
    assert rr.seeds(z, z, h, LAT, LON, k=4, threshold=1480.0, field="hgt", length=10.0, width=10.0)["pos"].tolist() == [[16, 0]]


@pytest.mark.parametrize("field", ["zeta", "hgt"])
def test_a_tile_that_is_the_whole_ring(field):
    """nx = 11, si = 3, r = 2: the tile's 2 si + 1 + 2 r = 11 columns are the whole ring exactly once, wherever the centre is."""
    rng = np.random.default_rng(8)
    lon = -180.0 + (360.0 / 11) * np.arange(11)
    u, v, h = rng.standard_normal((3, 6, 33, 11))
    box = dict(length=10.0, width=10.0, search=100.0)
    assert fw.window_steps(LAT, lon, 100.0) == (40, 3)
    kw = dict(smooth=2, field=field, patience=0)
    starts = [(0, 16, 0), (0, 10, 5), (1, 20, 10)]
    got = chunked(u, v, h, starts, [2, 4], lon=lon, box=box, **kw)
    ref = rr.walk_chunked(u, v, h, LAT, lon, starts, [2, 4], **box, **kw)
    compare(got, ref, ("whole ring", field))


def test_refusals_return_before_any_launch():
    """Addresses nothing dereferences: a refused call has not launched."""
    lib = _lib.load()
    for call, args, word in (("lec_follow_spans_chunk_ring", _chunk_args(nx=10, ihi=9), b"2 si + 1 + 2 smooth_r"),
                             ("lec_follow_spans_chunk_ring", _chunk_args(ilo=1), b"ilo = 0"),
                             ("lec_follow_seeds_series_ring", _seeds_args(ilo=1), b"ilo = 0"),
                             ("lec_follow_seeds_series_ring", _seeds_args(ei=36), b"2 ei + 1")):
        assert getattr(lib, call)(C.byref(args)) == 1
        assert lib.lec_last_error().startswith(call.encode()) and word in lib.lec_last_error()
    torch.cuda.synchronize()
    u, v, h, start, _ = rc.planted(11, nt=2, **rc.EAST)
    with pytest.raises(ValueError, match="2 si \\+ 1 \\+ 2 smooth_r = 73 columns exceed nx = 72"):
        chunked(u, v, h, start_row(start), [2], smooth=33, field="hgt")
