"""The row-block kernel's schedule on the device: which workgroup computes a row, and when, must not show in the records.
``tuning kernel=row_block`` against ``kernel=row_sweep`` (one wave per row, its own workgroup order; fp32 rows in float2 vectors as the
row-block kernel walks them) on the same synthetic cubes,
all 32 slots of every record with ``torch.equal``; the record buffer is pre-filled with NaN, so a row that no workgroup wrote shows.

Box heights 1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 31, 33, 47, 65: every remainder of the latitude cells over the 8 XCDs, odd and even
heights (a cell with a wave beyond the box), chunks of 0 and 1 cells per XCD and chunks cut into tiles of unequal height.  1, 2, 3, 5
and 9 time steps, each as the whole series and as a shard with a halo step on either side.  Rows of 66 columns (one trip) and 194
(two); 3 levels; fp64 and fp32 storage; the default block (2 x 1 x 2 waves) and 212, 122, 222 through ``tuning``.

A box one row high is no box to the library (dT/dy needs two rows): both requests are refused alike before anything is launched, and
that is what the height-1 case asserts; so is a one-step series (dT/dt needs a second step).  A one-step shard of a row-block request
runs one wave per row (``lec_rowstats``) with the request's ``f32_vec``, so the row-block requests carry ``f32_vec = 2`` as well."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.helpers import synthetic_domain

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HEIGHTS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 31, 33, 47, 65]
T_COUNTS = [1, 2, 3, 5, 9]
NL, NY, NT = 3, max(HEIGHTS) + 2, max(T_COUNTS) + 2
_cubes, _sweep = {}, {}
# the row-block kernel walks fp32 rows in float2 vectors: f32_vec = 2 gives the one-wave-per-row kernel the same lane-to-element map
# (float4 trips sum a row's elements in another order); fp64 storage ignores it
SWEEP = {"kernel": "row_sweep", "f32_vec": 2}


def _cube(nx, dtype):
    """Engine and device fields of the (nx, dtype) cube, built once."""
    if (nx, dtype) not in _cubes:
        from lorenzcycletoolkit_amd.engine import LECEngine
        dom = synthetic_domain(NT, NL, NY, nx, seed=7 + nx, dtype=dtype)
        f = [torch.as_tensor(a).to(DEV) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
        _cubes[nx, dtype] = (dom, LECEngine(dom.lat, dom.lon, dom.level, device=DEV), f)
    return _cubes[nx, dtype]


def _records(nx, dtype, h, tc, shard, tuning):
    """Records of ``tc`` steps of the box of height ``h``: the whole series of a tc-step cube, or steps 1 .. tc of a cube of tc + 2."""
    dom, eng, f = _cube(nx, dtype)
    n, tb = (tc + 2, 1) if shard else (tc, 0)
    out = torch.full((tc, NL, h, 32), float("nan"), dtype=torch.float64, device=DEV)
    got = eng.rowstats(*[t[:n] for t in f], [(3, nx - 4, 1, h)], time_s=dom.time_s[:n], t_begin=tb, t_count=tc, rows_out=out, tuning=tuning)
    assert got is out
    return out


def _reference(nx, dtype, h, tc, shard):
    """One wave per row: computed once per case, shared by the block shapes, never written again."""
    key = (nx, dtype, h, tc, shard)
    if key not in _sweep:
        _sweep[key] = _records(nx, dtype, h, tc, shard, SWEEP)
    return _sweep[key]


CASES = [(72, np.float64, 0), (200, np.float64, 0), (72, np.float32, 0), (200, np.float32, 0),
         (72, np.float64, 212), (72, np.float64, 122), (200, np.float32, 122), (72, np.float64, 222), (200, np.float32, 222)]


@pytest.mark.parametrize("nx,dtype,shape", CASES, ids=[f"nx{n}-{np.dtype(d).name}-block{s}" for n, d, s in CASES])
def test_row_block_records_equal_one_wave_per_row(nx, dtype, shape):
    tuning = {"kernel": "row_block", "f32_vec": 2, **({"block_shape": shape} if shape else {})}
    bad = []
    for h in HEIGHTS:
        if h < 2:       # refused alike, before any launch
            for tu in (tuning, SWEEP):
                with pytest.raises(ValueError):
                    _records(nx, dtype, h, 2, False, tu)
            continue
        for tc in T_COUNTS:
            for shard in (False, True):
                if tc == 1 and not shard:       # a one-step cube has no time neighbour: dT/dt needs two steps (refused alike)
                    for tu in (tuning, SWEEP):
                        with pytest.raises(ValueError):
                            _records(nx, dtype, h, tc, shard, tu)
                    continue
                ref, got = _reference(nx, dtype, h, tc, shard), _records(nx, dtype, h, tc, shard, tuning)
                if not torch.equal(got, ref):       # (NaN != NaN: an unwritten row fails here too)
                    rows = (got != ref).any(dim=-1).nonzero().tolist()
                    bad.append(f"height {h}, {tc} steps{' (shard)' if shard else ''}: {len(rows)} rows differ, first (t, k, j) = {rows[0]}")
    assert not torch.isnan(torch.stack([r.sum() for r in _sweep.values()])).any(), "the reference itself has unwritten rows"
    assert not bad, "; ".join(bad[:10]) + (f" ... ({len(bad)} in all)" if len(bad) > 10 else "")
