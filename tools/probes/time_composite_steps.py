"""Times the composites of a batch of tracks -- ONE ``lec_composite_steps`` call and ``lec_composite_ensemble`` -- against the route that
existed before them: one ``lec_composite`` call per track on the same resident cubes and records.  Geometry of ``tools/bench_batch.py``:
16 tracks of 40 six-hourly steps, 37 levels, 61 x 61 boxes on the 162 x 243 union crop of a 64-step data set, fp32 and fp64 storage.
Stage 1 + stage 2 of the same batch (``compute(steps=...)``) is timed beside them for scale.

Method.  HIP events on the launch stream around each route, which ends in ``event.synchronize()``; two warm-up passes of every route,
then ``--repeat`` timed passes of the three ALTERNATING in one process; the figure is the median, the spread is min .. max.  Both
composite routes read the same row records and level records (made once, by the batch's stage 1 + stage 2), allocate and zero their
accumulators inside the window (the batch is handed its host copy of the step table, as ``compute`` hands it) and end with the tracks' means (the per-track route: ``composite_finish``'s division; the batch:
``lec_composite_ensemble``, which forms the ensemble too).  The boxes move by index, a column or so per step, so every box has one shape
and tables of its own.  The tracks' steps are consecutive cube steps, so the per-track route takes dT/dt from the cube's own neighbours.

    python tools/probes/time_composite_steps.py [--tracks 16] [--steps 40] [--repeat 7] [--out FILE]

Prints one JSON line per storage dtype (and appends them to ``--out``)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from lorenzcycletoolkit_amd import _lib, tables  # noqa: E402
from lorenzcycletoolkit_amd.engine import LECEngine, LECResult  # noqa: E402
from lorenzcycletoolkit_amd.synthetic import era5_like_levels, synthetic_cube  # noqa: E402
from tools.probes.time_composite import timed  # noqa: E402

NYB = NXB = 61


def _tracks(k, n, nt, ny, nx, rng):
    """K tracks of n consecutive steps: the start step, and a 61 x 61 box that drifts three columns east in two steps and a row south in
    five."""
    out = []
    for _ in range(k):
        t0 = int(rng.integers(0, nt - n + 1))
        i0 = int(rng.integers(0, nx - NXB - (3 * n) // 2))
        j0 = int(rng.integers(n // 5 + 1, ny - NYB + 1))
        out.append((np.arange(t0, t0 + n), [(i0 + (3 * s) // 2, i0 + (3 * s) // 2 + NXB - 1, j0 - s // 5, j0 - s // 5 + NYB - 1) for s in range(n)]))
    return out


def _stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "range": max(ms) - min(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--nt", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_composite_steps.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    level = era5_like_levels()
    lat, lon = np.arange(-57.75, -17.5 + 1e-9, 0.25), np.arange(-80.25, -19.75 + 1e-9, 0.25)
    time_s = np.arange(a.nt) * 21600.0
    tracks = _tracks(a.tracks, a.steps, a.nt, lat.size, lon.size, np.random.default_rng(a.seed))
    sizes = [len(u) for u, _ in tracks]
    boxes = [b for _, bx in tracks for b in bx]
    st = np.concatenate([np.stack([u, np.r_[u[0], u[:-1]], np.r_[u[1:], u[-1]]], 1) for u, _ in tracks]).astype(np.int32)
    tc = np.concatenate([tables.time_coefs(time_s[u] - time_s[u[0]]) for u, _ in tracks])
    eng = LECEngine(lat, lon, level, device=dev)
    stream = torch.cuda.current_stream(dev)
    for dtype in (torch.float32, torch.float64):
        f = synthetic_cube(a.nt, level, lat, lon, device=dev, dtype=dtype, seed=a.seed)
        cubes = [f[k] for k in ("tair", "u", "v", "omega", "geopt")]
        pb = eng.prepare_boxes(boxes)
        steps, tcoef = torch.as_tensor(st).to(dev), torch.as_tensor(tc).to(dev)
        cube_tcoef = eng.time_coefs_device(time_s)
        own = []
        o = 0
        for u, bx in tracks:
            own.append((int(u[0]), o, o + len(u), eng.prepare_boxes(bx)))
            o += len(u)

        def totals():
            return eng.compute(*cubes, pb, steps=steps, tcoef=tcoef, per_step_boxes=True, drop_any_time=False, keep_rows=True)

        rows = totals().rows
        levraw = eng._workspace(len(boxes), level.size, dev)[1].clone()

        def per_track():
            out = []
            for t0, lo, hi, pbk in own:
                state = eng.composite_begin(hi - lo, pbk, dev)
                eng.composite_stage(*cubes[:4], rows[lo:hi], pbk, levraw[lo:hi], state, 0, tcoef=cube_tcoef, t_begin=t0)
                res = LECResult.__new__(LECResult)
                eng.composite_finish(res, state)
                out.append(res)
            return out

        def batch():
            state = eng.batch_composite_begin(sizes, pb, dev)
            eng.batch_composite_stage(*cubes[:4], rows, pb, levraw, state, 0, steps=steps, tcoef=tcoef, steps_host=st)
            res = LECResult.__new__(LECResult)
            eng.batch_composite_finish(res, state)
            return res

        for _ in range(2):
            totals(), per_track(), batch()
        torch.cuda.synchronize(dev)
        t12, tl, tb = [], [], []
        for _ in range(a.repeat):
            t12.append(timed(totals, stream)[0])
            tl.append(timed(per_track, stream)[0])
            ms, res = timed(batch, stream)
            tb.append(ms)
        # interior steps of a track read the same neighbours on both routes: the same bits there (the ends differ: the cube has a
        # neighbour where the track has none)
        ref = per_track()
        same = all(torch.equal(res.batch_composite_lon[lo + 1: hi - 1], r.composite_lon[1:-1]) for (_, lo, hi, _), r in zip(own, ref))
        y, b = _stats(tl), _stats(tb)
        line = {"probe": "time_composite_steps", "storage": str(dtype).replace("torch.", ""), "tracks": a.tracks, "steps_per_track": a.steps,
                "boxes": len(boxes), "box": [int(level.size), NYB, NXB], "union": [a.nt, int(level.size), int(lat.size), int(lon.size)],
                "repeat": a.repeat, "source_digest": _lib.source_digest(),
                "stage1_plus_stage2_ms": _stats(t12), "per_track_lec_composite_ms": y, "batch_lec_composite_steps_and_ensemble_ms": b,
                "batch_over_per_track": b["median"] / y["median"],
                "condition_batch_median_within_yardstick_median_plus_its_range": b["median"] <= y["median"] + y["range"],
                "interior_steps_bit_for_bit": bool(same)}
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")
        del f, cubes, rows, levraw


if __name__ == "__main__":
    main()
