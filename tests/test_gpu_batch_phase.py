"""Phase-aligned ensembles of batch composites on the GPU: ``lec_composite_phase_sum`` / ``lec_composite_phase_ensemble`` through
``LECEngine.compute(..., batch_composites=sizes, batch_composite_phases=ranges)`` against the in-order NumPy sums of the same run's
``batch_composite_steps`` (bit for bit), against ``batch_composite_mean`` / ``batch_composite_ensemble`` (``lifetime:1``: bit for bit) and
against the CPU restatement (tests/batch_phase_restatement.py on tests/batch_composite_restatement.py's columns).

Shapes.  tests/test_gpu_batch_composite.py's own domain and tracks: a union of 9 steps, A on every step (9), B on every second (5), C on
two (2); 5 x 65 boxes on a 24 x 80 grid (across the 64-lane column segment), 8 levels, fp64; once 65 x 5 boxes on 71 x 14 in fp32.
``lifetime:4`` gives the cells 3,2,2,2 / 2,1,1,1 / 1,0,1,0 steps: C is no member of bins 1 and 3.  Sub-calls of 3, 7 and 1 boxes cut inside
bins, on A's bin border at box 3 and on the A/B border at box 9.  Tracks of 16 and 17 steps on an 18-step union give ranges of 16, 17, 8
and 9 boxes, both sides of the time sum's load batch of 16.

Bars.  Bit for bit for the cells' means and the ensembles against the in-order sums, between cuts into sub-calls, and for every other field
of the result with and without the keyword.  1e-9 of the term's scale against the restatement (tests/test_gpu_composite.py's and
tests/test_gpu_batch_composite.py's bar) for means, ensembles and spread; NaN patterns are the restatement's exactly.  The spread is held
to that bar only: the last bit of the device's sqrt is not pinned.  Each test prints its figures.
Measured on MI355X, the largest over all cases: batch_phase_mean 1.9e-13, batch_phase_ensemble 1.0e-13, batch_phase_spread 1.3e-13 against
the restatement (the call alone on random sums: spread 0.0 against NumPy's in-order form); everything else is equality."""
import dataclasses
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib, batch
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import batch_phase_restatement as pr
from tests import test_gpu_batch_composite as tb

DEV = tb.DEV
TOL = 1e-9
PHASE_FIELDS = ("batch_phase_mean", "batch_phase_ensemble", "batch_phase_spread", "batch_phase_count", "batch_phase_members")


def _lifetime(tracks, n_bin):
    return np.stack([batch.lifetime_ranges(len(u), n_bin) for u, _ in tracks])


def _setup(nyb=5, nxb=65, nl=8, dtype=np.float64, ny=24, nx=80):
    dom = tb._dom(nl, ny, nx, dtype)
    tracks = tb._tracks(nyb, nxb, ny, nx)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    cubes = [tb._dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    return dom, tracks, eng, cubes


def _sum_in_order(cols: np.ndarray) -> np.ndarray:
    """0.0 + cols[0] + cols[1] + ...: the running sum the kernel forms on its zeroed accumulator."""
    s = np.zeros(cols.shape[1:])
    for c in cols:
        s = s + c
    return s


def _cells_in_order(steps: np.ndarray, sizes, ranges) -> np.ndarray:
    """mean [K, B, ...] from the run's own per-box columns: the in-order sum times the rounded reciprocal of the count; NaN without steps."""
    seg = np.concatenate([[0], np.cumsum(sizes)])
    K, B = ranges.shape[:2]
    out = np.full((K, B) + steps.shape[1:], np.nan)
    for k in range(K):
        for b in range(B):
            lo, hi = (int(x) for x in ranges[k, b])
            if hi > lo:
                out[k, b] = _sum_in_order(steps[seg[k] + lo: seg[k] + hi]) * (1.0 / float(hi - lo))
    return out


def _ensemble_in_order(mean: np.ndarray, count: np.ndarray) -> np.ndarray:
    """[B, ...]: the members' means added in track order from the first member's, over the members; NaN without one."""
    K, B = count.shape
    out = np.full((B,) + mean.shape[2:], np.nan)
    for b in range(B):
        who = [k for k in range(K) if count[k, b] >= 1]
        if who:
            s = mean[who[0], b].copy()
            for k in who[1:]:
                s = s + mean[k, b]
            out[b] = s / float(len(who))
    return out


def _same(got, want) -> bool:
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def _close(got, ref, scale, what):
    """Within TOL of the term's scale (``scale`` broadcasts over ``ref``), the NaN pattern exactly; prints and returns the figure."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern"
    err = float(np.nanmax(np.abs(got - ref) / scale)) if np.isfinite(ref).any() else 0.0
    print(f"{what}: max error / scale = {err:.3e}")
    assert err <= TOL, (what, err)
    return err


def _check_in_order(res, tracks, ranges, tag):
    """The phase fields of ``res`` (a run that kept its steps) against the in-order sums of its own columns."""
    sizes = [len(u) for u, _ in tracks]
    count = ranges[:, :, 1] - ranges[:, :, 0]
    steps = res.batch_composite_steps.cpu().numpy()
    mean = res.batch_phase_mean.cpu().numpy()
    assert mean.shape == ranges.shape[:2] + steps.shape[1:]
    assert _same(mean, _cells_in_order(steps, sizes, ranges)), f"{tag}: a cell's mean is not the in-order sum of its boxes' columns / count"
    assert np.isnan(mean[count == 0]).all()
    ens = res.batch_phase_ensemble.cpu().numpy()
    assert _same(ens, _ensemble_in_order(mean, count)), f"{tag}: a bin's ensemble is not the in-order sum of its members' means / members"
    assert np.array_equal(res.batch_phase_count, count) and res.batch_phase_count.dtype == np.int32
    assert np.array_equal(res.batch_phase_members, (count >= 1).sum(axis=0))
    spread = res.batch_phase_spread.cpu().numpy()
    assert spread.shape == ens.shape
    for b, m in enumerate(res.batch_phase_members):
        assert np.isnan(spread[b]).all() if m < 2 else np.array_equal(np.isnan(spread[b]), np.isnan(ens[b])), (tag, b)


def _check_restatement(res, ref_per, ranges, tag):
    mean_r, ens_r, spread_r, count_r, members_r = pr.phases(ref_per, ranges)
    scale = tb._scale(mean_r, (0, 1, 3, 4))                          # [1, 1, 6, 1, 1]: the term's scale over every cell
    errs = (_close(res.batch_phase_mean.cpu().numpy(), mean_r, scale, f"{tag} batch_phase_mean"),
            _close(res.batch_phase_ensemble.cpu().numpy(), ens_r, scale[0], f"{tag} batch_phase_ensemble"),
            _close(res.batch_phase_spread.cpu().numpy(), spread_r, scale[0], f"{tag} batch_phase_spread"))
    assert np.array_equal(res.batch_phase_count, count_r) and np.array_equal(res.batch_phase_members, members_r)
    return errs


@pytest.mark.parametrize("nyb, nxb, nl, dtype, ny, nx", [tb.CASES[0], tb.CASES[5]], ids=[tb.IDS[0], tb.IDS[5]])
def test_lifetime_4_is_the_in_order_sum_and_the_restatement(nyb, nxb, nl, dtype, ny, nx):
    dom, tracks, eng, cubes = _setup(nyb, nxb, nl, dtype, ny, nx)
    ranges = _lifetime(tracks, 4)
    assert (ranges[:, :, 1] - ranges[:, :, 0]).tolist() == [[3, 2, 2, 2], [2, 1, 1, 1], [1, 0, 1, 0]]
    res = tb._batch(eng, cubes, dom, tracks, batch_composite_steps=True, batch_composite_phases=ranges)
    tag = f"lifetime:4 {nyb}x{nxb} {np.dtype(dtype).name}"
    _check_in_order(res, tracks, ranges, tag)
    assert res.batch_phase_members.tolist() == [3, 2, 3, 2]
    mean = res.batch_phase_mean
    assert torch.isnan(mean[2, 1]).all() and torch.isnan(mean[2, 3]).all() and not torch.isnan(mean[:2]).any() and not torch.isnan(mean[2, [0, 2]]).any()
    assert not torch.isnan(res.batch_phase_ensemble).any() and not torch.isnan(res.batch_phase_spread).any()
    ref = tb._reference(("ref", nyb, nxb, nl, np.dtype(dtype).name), dom, tracks)
    _check_restatement(res, ref[0], ranges, tag)


def test_lifetime_1_is_the_batch_composites_own_mean_and_ensemble():
    dom, tracks, eng, cubes = _setup()
    res = tb._batch(eng, cubes, dom, tracks, batch_composite_phases=_lifetime(tracks, 1))
    assert res.batch_phase_mean.shape == (3, 1, 6, 5, 65) and res.batch_phase_members.tolist() == [3]
    assert torch.equal(res.batch_phase_mean[:, 0], res.batch_composite_mean)
    assert torch.equal(res.batch_phase_ensemble[0], res.batch_composite_ensemble)
    assert res.batch_phase_count.tolist() == [[9], [5], [2]] and not torch.isnan(res.batch_phase_spread).any()


@pytest.mark.parametrize("per_call", [3, 7, 1])
def test_sub_calls_inside_a_bin_and_on_its_borders_keep_the_bits(per_call):
    """MAP_CHUNK_BYTES set on the engine instance: 16 boxes (9 + 5 + 2) in sub-calls of 3 (cuts inside bins, on A's bin border at box 3 and
    between A and B at 9), of 7 (inside bins, between B and C at 14) and of 1 (every cell of more than one step is cut)."""
    nyb, nxb, nl = 5, 65, 8
    dom, tracks, eng, cubes = _setup()
    ranges = _lifetime(tracks, 4)
    whole = tb._batch(eng, cubes, dom, tracks, batch_composite_phases=ranges)
    kept_whole = tb._batch(eng, cubes, dom, tracks, batch_composite_steps=True, batch_composite_phases=ranges)
    cut_eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    cut_eng.MAP_CHUNK_BYTES = per_call * 8 * (6 * nyb * nxb + nl * nyb * _lib.LEC_MAPS_NCOEF)
    assert LECEngine.MAP_CHUNK_BYTES == 256 << 20
    for kept in (False, True):
        cut = tb._batch(cut_eng, cubes, dom, tracks, batch_composite_steps=kept, batch_composite_phases=ranges)
        for name in PHASE_FIELDS[:3] + ("batch_composite_mean", "batch_composite_ensemble", "batch_composite_lon"):
            assert tb._bits(getattr(cut, name), getattr(whole, name)), (name, kept)
            assert tb._bits(getattr(kept_whole, name), getattr(whole, name)), name
        assert np.array_equal(cut.batch_phase_count, whole.batch_phase_count) and np.array_equal(cut.batch_phase_members, whole.batch_phase_members)
    assert torch.isnan(whole.batch_phase_mean).sum() == 2 * 6 * nyb * nxb          # C's two empty cells and nothing else


def test_ranges_on_both_sides_of_the_load_batch_of_sixteen():
    nyb, nxb, nl, ny, nx, nt = 4, 5, 8, 8, 14, 18
    dom = tb._dom(nl, ny, nx, np.float64, nt=nt)
    place = lambda n, k: ((2 * n + 3 * k) % (nx - nxb + 1), (n + k) % (ny - nyb + 1))
    tracks = []
    for k, u in enumerate((np.arange(1, 17), np.arange(0, 17))):
        tracks.append((u, [(i, i + nxb - 1, j, j + nyb - 1) for i, j in (place(n, k) for n in range(len(u)))]))
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    cubes = [tb._dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    for n_bin, sizes in ((1, [[16], [17]]), (2, [[8, 8], [9, 8]])):
        ranges = _lifetime(tracks, n_bin)
        assert (ranges[:, :, 1] - ranges[:, :, 0]).tolist() == sizes
        res = tb._batch(eng, cubes, dom, tracks, batch_composite_steps=True, batch_composite_phases=ranges)
        _check_in_order(res, tracks, ranges, f"16 + 17 steps, lifetime:{n_bin}")
        assert not torch.isnan(res.batch_phase_mean).any()
        if n_bin == 1:
            assert torch.equal(res.batch_phase_mean[:, 0], res.batch_composite_mean)


def test_hand_made_ranges_single_steps_lone_members_empty_bins_and_overlaps():
    """A ``peak:1``-like table of single steps (bins 0-2; A's peak at its first step, so its lag -1 is empty), a bin that A alone enters
    (3), a bin nobody enters (4) and two bins of overlapping ranges (5, 6)."""
    dom, tracks, eng, cubes = _setup()
    E = (0, 0)
    ranges = np.array([[E, (0, 1), (1, 2), (4, 5), E, (2, 7), (4, 9)],
                       [(1, 2), (2, 3), (3, 4), E, (5, 5), (0, 3), (1, 5)],
                       [(0, 1), (1, 2), (2, 2), E, E, (0, 2), (1, 2)]], dtype=np.int64)
    res = tb._batch(eng, cubes, dom, tracks, batch_composite_steps=True, batch_composite_phases=ranges)
    _check_in_order(res, tracks, ranges, "hand-made ranges")
    assert res.batch_phase_members.tolist() == [2, 3, 2, 1, 0, 3, 3]
    steps, mean, ens, spread = res.batch_composite_steps, res.batch_phase_mean, res.batch_phase_ensemble, res.batch_phase_spread
    # a single step's mean is that step's columns: x * (1.0 / 1.0)
    assert torch.equal(mean[0, 1], steps[0]) and torch.equal(mean[1, 1], steps[9 + 2]) and torch.equal(mean[2, 1], steps[14 + 1])
    # one member: the ensemble is its mean, there is no spread
    assert torch.equal(ens[3], mean[0, 3]) and torch.equal(mean[0, 3], steps[4]) and torch.isnan(spread[3]).all()
    # no member: nothing but NaN
    assert torch.isnan(ens[4]).all() and torch.isnan(spread[4]).all() and torch.isnan(mean[:, 4]).all()
    assert not torch.isnan(ens[[0, 1, 2, 3, 5, 6]]).any() and not torch.isnan(spread[[0, 1, 2, 5, 6]]).any()
    ref = tb._reference(("ref", 5, 65, 8, "float64"), dom, tracks)
    _check_restatement(res, ref[0], ranges, "hand-made ranges")


def test_nan_reaches_the_cells_that_hold_a_box_that_sees_it_and_no_other():
    """tests/test_gpu_batch_composite.py's patch: T NaN in B's band at union step 4 (B's step 2; B's steps 1 and 3 read it for dT/dt)."""
    nyb, nxb, nl, ny, nx = 5, 65, 8, 24, 80
    base = tb._dom(nl, ny, nx, np.float64)
    tracks = tb._tracks(nyb, nxb, ny, nx)
    iw, _, js, _ = tracks[1][1][2]
    assert tracks[1][0][2] == 4
    T = base.tair.copy()
    T[4, 3, js + 1, [iw + 7, iw + 8]] = np.nan
    T[4, :, js + 3, iw + 40] = np.nan
    dom = o.Domain(T, base.u, base.v, base.omega, base.geopt, base.lat, base.lon, base.level, base.time_s)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    clean = [tb._dev(a) for a in (base.tair, base.u, base.v, base.omega, base.geopt)]
    ranges = _lifetime(tracks, 4)
    res = tb._batch(eng, [tb._dev(T)] + clean[1:], dom, tracks, batch_composite_steps=True, batch_composite_phases=ranges)
    plain = tb._batch(eng, clean, base, tracks, batch_composite_steps=True, batch_composite_phases=ranges)
    assert not torch.isnan(plain.batch_composite_steps).any()
    _check_in_order(res, tracks, ranges, "NaN in track 1")
    sees = torch.isnan(res.batch_composite_steps).flatten(1).any(dim=1).cpu().numpy()          # per box
    assert sees[9 + 2] and not sees[:9].any() and not sees[14:].any() and not sees[[9, 13]].any()
    seg = [0, 9, 14]
    hit = np.zeros((3, 4), dtype=bool)
    for k in range(3):
        for b in range(4):
            lo, hi = ranges[k, b]
            hit[k, b] = sees[seg[k] + lo: seg[k] + hi].any()
            got, was = res.batch_phase_mean[k, b], plain.batch_phase_mean[k, b]
            if hit[k, b]:
                assert not torch.equal(got.isnan(), was.isnan()), (k, b)
            else:
                assert tb._bits(got, was), (k, b)
    assert hit[1, 1] and not hit[1, 3] and not hit[[0, 2]].any()
    for b in range(4):
        if hit[:, b].any():         # at the member's NaN points and nowhere else
            assert torch.equal(res.batch_phase_ensemble[b].isnan(), res.batch_phase_mean[1, b].isnan()), b
            assert torch.equal(res.batch_phase_spread[b].isnan(), res.batch_phase_mean[1, b].isnan()), b
        else:
            assert torch.equal(res.batch_phase_ensemble[b], plain.batch_phase_ensemble[b]), b
            assert torch.equal(res.batch_phase_spread[b], plain.batch_phase_spread[b]), b
    ref_per = tb.br.composites(dom, tracks)[0]
    _check_restatement(res, ref_per, ranges, "NaN in track 1")


def test_ensemble_call_alone_on_random_sums():
    """``lec_composite_phase_ensemble`` on sums of its own (``batch_composite_finish``): a NaN planted in one sum, a bin without members,
    one with a single member, one with two."""
    nyb, nxb, sizes = 5, 65, [9, 5, 2, 7]
    dom = tb._dom(8, 24, 80, np.float64)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    boxes = [(n % 10, n % 10 + nxb - 1, n % 7, n % 7 + nyb - 1) for n in range(sum(sizes))]
    count = np.array([[9, 0, 2, 0], [5, 0, 0, 3], [2, 0, 1, 0], [7, 0, 0, 0]])
    ranges = np.stack([np.zeros_like(count), count], axis=2)
    state = eng.batch_composite_begin(sizes, eng.prepare_boxes(boxes), DEV, phases=ranges)
    assert state["phasesum"].shape == (4, 4, 6, nyb, nxb) and not state["phasesum"].any()
    sums = torch.randn(state["phasesum"].shape, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7)) * 1e3
    sums[2, 0, 1, 3, 40] = float("nan")
    state["phasesum"].copy_(sums)
    res = types.SimpleNamespace()
    eng.batch_composite_finish(res, state)
    torch.cuda.synchronize()
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(count[:, :, None, None, None] >= 1, sums.cpu().numpy() * (1.0 / count.astype(np.float64))[:, :, None, None, None], np.nan)
    mean = res.batch_phase_mean.cpu().numpy()
    assert _same(mean, want) and np.isnan(mean).sum() == 1 + (count == 0).sum() * 6 * nyb * nxb
    ens = res.batch_phase_ensemble.cpu().numpy()
    assert _same(ens, _ensemble_in_order(want, count))
    assert np.isnan(ens[0]).sum() == 1 and np.isnan(ens[0, 1, 3, 40]) and np.isnan(ens[1]).all() and not np.isnan(ens[2:]).any()
    assert np.array_equal(ens[3], want[1, 3])
    assert res.batch_phase_members.tolist() == [4, 0, 2, 1]
    spread = res.batch_phase_spread.cpu().numpy()
    ref = np.full(ens.shape, np.nan)
    for b, who in ((0, [0, 1, 2, 3]), (2, [0, 2])):
        s = np.zeros(ens.shape[1:])
        for k in who:
            s = s + (want[k, b] - ens[b]) * (want[k, b] - ens[b])
        ref[b] = np.sqrt(s / float(len(who) - 1))
    _close(spread, ref, 1e3, "lec_composite_phase_ensemble alone: spread")


def test_without_the_keyword_nothing_changes_and_with_it_nothing_else_does():
    dom, tracks, eng, cubes = _setup()
    plain, again = tb._batch(eng, cubes, dom, tracks), tb._batch(eng, cubes, dom, tracks)
    with_p = tb._batch(eng, cubes, dom, tracks, batch_composite_phases=_lifetime(tracks, 4))
    seen = 0
    for f in dataclasses.fields(plain):
        a, b, c = getattr(plain, f.name), getattr(again, f.name), getattr(with_p, f.name)
        if f.name in PHASE_FIELDS:
            assert a is None and b is None and c is not None, f.name
            seen += 1
            continue
        assert (a is None) == (b is None) == (c is None), f.name
        if a is not None:
            assert torch.equal(a, b) and torch.equal(a, c), f.name
    assert seen == 5 and plain.batch_composite_mean is not None
    none = tb._batch(eng, cubes, dom, tracks, batch_composites=None)
    assert all(getattr(none, n) is None for n in PHASE_FIELDS)
