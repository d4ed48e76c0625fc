"""Stage 2 (csrc/lec_reduce.hip) across the seams of its launch constants, against the oracle evaluated in extended precision.

The cases come from tests/stage2_cases.py (tests/test_stage2_cases_cpu.py shows, without a GPU, that they are what they claim to be
and that the float64 oracle lies within 1e-11 of the extended one):

* boxes of 63 ... 131 rows: the switch between the one-row-per-lane kernel (<= 64 rows) and the general one, the halo row at a trip
  seam of the general kernel (rows 63 / 64 / 65, 127 / 128), a last partial trip -- clean, and with NaNs placed at those rows
  (``baz3_repaired`` in a later trip, levels dropped for the whole series, the north-edge row in the last trip);
* per-step boxes of 130, 64, 65, 2 and 100 rows in one 130-row buffer (the ``jb >= nyb`` skip inside a trip), whose low boxes alone in a
  shard take the small kernel and must give the same bits;
* 64 ... 160 levels: the second and third pass of the lane-strided level loops, the repair scan, the any-time drop mask and the
  k0 / k1 trimming at levels >= 64, and the box-tile kernel's level chunks past three chunks;
* the ``axes_*`` cases: the same seams on uneven latitudes and pressures, where the middle gradient coefficients (``lattab2[.., 5]``,
  ``levtab2[.., 2]``) are non-zero in every interior row and level, every row has a coefficient triple of its own, the trapezoid
  weights differ from row to row and level to level, and gaps two to five levels deep are repaired with weights that depend on p.

Tolerance: TOL = 1e-9 of each term's scale, as everywhere in test_gpu_parity.py -- both sides evaluate in fp64 or better, and the
reference's own rounding stays below 1e-11."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import stage2_cases as sc
from tests.helpers import SCALARS, compare
from tests.test_gpu_parity import TOL, _dev, _engine, _rows_close, run_fixed

pytestmark = pytest.mark.gpu


def _fields(dom):
    return [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]


def _same_bits(a, b, what):
    """scalars, levels (NaN = a dropped level: at the same places) and nanflag carry the same bits."""
    for name in ("scalars", "levels"):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)), (what, name)
    assert torch.equal(a.nanflag, b.nanflag), (what, "nanflag")


def _cat(parts):
    from lorenzcycletoolkit_amd.engine import LECResult
    return LECResult(scalars=torch.cat([p.scalars for p in parts]), levels=torch.cat([p.levels for p in parts]),
                     nanflag=torch.cat([p.nanflag for p in parts]))


@pytest.mark.parametrize("case", sc.FIXED_IDS)
def test_fixed_box_against_the_extended_oracle(case):
    """All 16 terms, budgets, residuals and the 21 level tables.  The case's name says which seam it crosses."""
    dom, limits, exp = sc.build(case)
    res = run_fixed(dom, limits)
    assert res.rows is None and int(res.levels.shape[2]) == dom.level.size
    ref_s, ref_l = sc.reference(case)
    worst = compare(res.scalars_dict(), res.levels_dict(), ref_s, ref_l, TOL, case, time_s=dom.time_s)
    print(case, max(worst.values()) / TOL)
    got = res.scalars_dict()
    if case in sc.NAN_FIXED_IDS:
        assert int(res.nanflag.max()) > 0
        assert all(np.isfinite(got[k]).all() for k in SCALARS), "every integrated term survives: levels were repaired or dropped"
    else:
        assert int(res.nanflag.sum()) == 0


def test_moving_boxes_of_mixed_heights_and_their_small_kernel_shards(case=sc.MOVING_ID):
    """Boxes of 130, 64, 65, 2 and 100 rows in one 130-row record buffer (the general level kernel, NaNs in it) against the oracle's moving
    framework; then the 64-row and the 2-row box each alone in a shard, where the buffer is at most 64 rows high and the small kernel
    runs: the project's stated bit-identity of the two level kernels.  ``axes_moving``: on uneven axes, every box from a grid row of
    its own."""
    dom, limits, exp = sc.build(case)
    eng = _engine(dom)
    boxes = [eng.box_from_limits(*lim) for lim in limits]
    assert boxes == exp["boxes"]
    f = _fields(dom)
    whole = eng.compute(*f, boxes, time_s=dom.time_s, keep_rows=True)
    torch.cuda.synchronize()
    assert whole.rows.shape[2] == 130
    ref_s, ref_l = sc.reference(case)
    worst = compare(whole.scalars_dict(), whole.levels_dict(), ref_s, ref_l, TOL, case, time_s=dom.time_s)
    print(case, max(worst.values()) / TOL)
    got = whole.scalars_dict()
    assert all(np.isfinite(got[k]).all() for k in SCALARS)
    flags = whole.nanflag.cpu().numpy()
    assert flags[2] > 0 and flags[4] > 0 and flags[1] == 0 and flags[3] == 0
    for a, b in ((1, 2), (3, 4)):
        part = eng.compute(*f, boxes[a:b], time_s=dom.time_s, t_begin=a, t_count=b - a, keep_rows=True, per_step_boxes=True)
        assert part.rows.shape[2] == exp["height"][a] <= 64
        assert torch.equal(part.scalars, whole.scalars[a:b]), (a, b)
        assert torch.equal(part.levels, whole.levels[a:b]), (a, b)
        assert torch.equal(part.nanflag, whole.nanflag[a:b]), (a, b)


def test_moving_boxes_on_uneven_axes_and_their_small_kernel_shards():
    """``axes_moving``: the same heights, every box from a grid row of its own -- per-box latitude tables that differ in every row."""
    test_moving_boxes_of_mixed_heights_and_their_small_kernel_shards(sc.AXES_MOVING_ID)


@pytest.mark.parametrize("case", [sc.MANY_NAN_ID, "tall131_seam_omega", "axes_levels130_nan", "axes_tall131_nan"])
def test_level_stage_then_vertical_stage_gives_the_bits_of_reduce(case):
    """The two halves of stage 2 (what a streamed series runs) on the same row records: 130 levels with NaNs in every pass of the level
    loops, and the tall box with NaNs at its first trip seam -- on even and on uneven axes."""
    from lorenzcycletoolkit_amd import _lib
    dom, limits, _ = sc.build(case)
    eng = _engine(dom)
    box = eng.box_from_limits(*limits)
    rows = eng.rowstats(*_fields(dom), [box], time_s=dom.time_s)
    whole = eng.reduce(rows, [box])
    levraw = torch.empty((rows.shape[0], rows.shape[1], _lib.LEC_NLEVRAW), dtype=torch.float64, device=rows.device)
    eng.level_stage(rows, [box], levraw)
    halves = eng.vertical_stage(levraw, [box])
    torch.cuda.synchronize()
    assert int(whole.nanflag.max()) > 0
    _same_bits(halves, whole, case)


@pytest.mark.parametrize("case", ["tall131_bottom_rows_64_65", sc.MANY_NAN_ID, "axes_tall131_nan"])
def test_any_time_mask_merged_from_two_time_shards(case):
    """A level that stays NaN at one step leaves the integrals of EVERY step.  The series in two time shards -- the first one (step 0)
    holds none of the steps at which the level is lost -- whose masks are merged by element-wise max through ``merge_dropmask`` (one
    device, one process): the concatenation equals the whole series, bit for bit."""
    dom, limits, _ = sc.build(case)
    nt = dom.time_s.size
    whole = run_fixed(dom, limits)
    shards = ((0, 1), (1, nt - 1))
    masks = []
    for a, n in shards:                              # first pass: every shard's own mask
        run_fixed(dom, limits, t_begin=a, t_count=n, merge_dropmask=lambda m: masks.append(m.clone()))
    assert len(masks) == 2 and int(masks[0].sum()) != int(masks[1].sum())
    merged = torch.maximum(masks[0], masks[1])
    assert int(merged[:, 64:].sum()) > 0 or dom.level.size < 64, "the mask must reach the levels of a later pass"
    parts = [run_fixed(dom, limits, t_begin=a, t_count=n, merge_dropmask=lambda m: m.copy_(merged)) for a, n in shards]
    _same_bits(_cat(parts), whole, case)
    # without the merge the first shard keeps the level: the test would not notice a mask that is never applied otherwise
    alone = run_fixed(dom, limits, t_begin=0, t_count=1)
    assert not torch.equal(torch.nan_to_num(alone.scalars, nan=-7.0), torch.nan_to_num(whole.scalars[0:1], nan=-7.0))


def test_small_and_general_kernel_agree_on_uneven_axes():
    """``axes_small64``: a 64-row box on uneven axes takes the small level kernel.  The same row records in a buffer padded to 70 rows
    take the general kernels (area means, then 64 staged rows with a halo row per trip), which read the same ``lattab2`` / ``levtab2``
    rows by other indices: the same bits."""
    dom, limits, exp = sc.build("axes_small64")
    eng = _engine(dom)
    box = eng.box_from_limits(*limits)
    f = _fields(dom)
    small = eng.compute(*f, [box], time_s=dom.time_s, keep_rows=True)
    nt, nl, nyb, ns = small.rows.shape
    assert nyb == exp["height"] == 64
    padded = torch.zeros((nt, nl, 70, ns), dtype=torch.float64, device="cuda:0")
    eng.rowstats(*f, [box], rows_out=padded, time_s=dom.time_s)
    assert torch.equal(padded[:, :, :nyb], small.rows)
    general = eng.reduce(padded, [box])
    torch.cuda.synchronize()
    _same_bits(general, small, "axes_small64: general vs small kernel")
    assert int(small.nanflag.sum()) == 0


@pytest.mark.parametrize("nl", [129, 160])
def test_kernel_families_agree_at_many_levels(nl):
    """Stage 1's three formulations at 129 and 160 levels (the box-tile kernel walks seven and more level chunks of at most 21), and the
    box-tile kernel's level chunks of 5 and 21 against its automatic choice: the same bits, stage 2's outputs included."""
    dom, limits, _ = sc.build(f"levels{nl}")
    a = run_fixed(dom, limits, keep_rows=True)
    b = run_fixed(dom, limits, keep_rows=True, tuning={"kernel": "two_sweep"})
    c = run_fixed(dom, limits, keep_rows=True, tuning={"kernel": "box_tile"})
    _rows_close(a, b, f"default vs two-sweep, {nl} levels")
    _rows_close(c, b, f"box tiles vs two-sweep, {nl} levels")
    for tj in (5, 21):
        r = run_fixed(dom, limits, keep_rows=True, tuning={"kernel": "box_tile", "tile_j": tj})
        assert torch.equal(r.rows, c.rows), (nl, tj)
        assert torch.equal(r.scalars, c.scalars) and torch.equal(r.levels, c.levels), (nl, tj)


def test_161_levels_are_refused_before_any_launch():
    """LEC_MAX_LEVELS = 160 computes (test_fixed_box_against_the_extended_oracle[levels160]); one more is refused by stage 2's argument
    validation.  Zero-filled row records: no stage-1 work, and nothing is launched."""
    from lorenzcycletoolkit_amd import _lib
    from lorenzcycletoolkit_amd.engine import LECEngine
    lat, lon = np.linspace(-60.0, -10.0, 7), np.linspace(-80.0, -20.0, 10)
    eng = LECEngine(lat, lon, np.linspace(10000.0, 100000.0, 161), device="cuda:0")
    rows = torch.zeros((2, 161, 5, _lib.LEC_NSTAT), dtype=torch.float64, device="cuda:0")
    with pytest.raises(_lib.LecLibraryError, match="more than 160 levels"):
        eng.reduce(rows, [(1, 8, 1, 5)])
