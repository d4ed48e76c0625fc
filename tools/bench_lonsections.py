#!/usr/bin/env python3
"""What the longitude x pressure sections cost.

Fixed box (default): ``lec_lonsections`` alone on a near-global ring -- a 37 x 721 x 1440 fp64 grid, box +-89.75 degrees over all
longitudes, 4 steps per call --, next to ``lec_maps`` of the same cubes and records (the yardstick: unchanged code, timed in the same run).
By bytes the two calls read the same cubes; the sections write 37 x 1440 values per term and step where the maps write 719 x 1440.

    python tools/bench_lonsections.py [--steps 4] [--rounds 3] [--repeat 5] [--out profiles/lonsections_bench.json]

Moving boxes (``--moving``): ``lec_composite_lonsections`` on the geometry of tools/probes/time_composite_sections.py -- a box-packed
series of 512 steps of 37 x 61 x 61, fp64 (dT/dt as a cube) and fp32 (tm / tp) --, as a fraction of stage 1 + stage 2 on the same series.

Every call is timed with HIP events around it (median of ``--repeat`` after a warm-up) and the forms ALTERNATE within a round;
``--rounds`` rounds; reported: the median over the rounds, per call and per time step.  One JSON line; ``--out`` appends it to a file.
Run each form in a process of its own, under a time limit of its own."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(torch, fn, repeat):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def fixed(a, torch, _lib, LECEngine, dev):
    nl, ny, nx = a.grid
    nt = a.steps
    lat = np.linspace(-90.0, 90.0, ny)
    lon = -180.0 + 360.0 / nx * np.arange(nx)
    level = np.linspace(100.0, 100000.0, nl)
    eng = LECEngine(lat, lon, level, device=dev)
    ring = eng.prepare_boxes([(0, nx - 1, 1, ny - 2)], ring=True)        # the polar rows stay out
    g = torch.Generator(device=dev).manual_seed(1)
    shape = (nt, nl, ny, nx)
    T = 250.0 + 10.0 * torch.randn(shape, dtype=torch.float64, device=dev, generator=g)
    U, V, W, P = (torch.randn(shape, dtype=torch.float64, device=dev, generator=g) for _ in range(4))
    time_s = 21600.0 * np.arange(nt)
    nyb = ny - 2
    f64 = dict(dtype=torch.float64, device=dev)
    rows = torch.empty((nt, nl, nyb, _lib.LEC_NSTAT), **f64)
    eng.rowstats(T, U, V, W, P, ring, time_s=time_s, rows_out=rows)
    levraw = torch.empty((nt, nl, _lib.LEC_NLEVRAW), **f64)
    eng.level_stage(rows, ring, levraw)
    mp = eng.map_begin(nt, ring, dev)
    ls = eng.lonsection_begin(nt, ring, dev)
    torch.cuda.synchronize()
    calls = [("maps", lambda: eng.map_stage(T, U, V, W, rows, ring, levraw, mp, 0, time_s=time_s)),
             ("lonsections", lambda: eng.lonsection_stage(T, U, V, W, rows, ring, levraw, ls, 0, time_s=time_s))]
    out = {"bench": "lonsections_fixed", "grid": [nl, ny, nx], "steps": nt, "dtype": "float64", "box_rows": nyb, "box_columns": nx,
           "rounds": a.rounds, "repeat": a.repeat, "map_chunk_bytes": int(LECEngine.MAP_CHUNK_BYTES), "csrc_sha": _lib.source_digest(),
           "waves": nt * nl * ((nx + 63) // 64)}
    for _ in range(a.rounds):
        for name, fn in calls:
            out.setdefault(f"{name}_ms", []).append(round(_timed(torch, fn, a.repeat), 4))
    med = lambda k: float(np.median(out[f"{k}_ms"]))
    for name, _ in calls:
        out[f"{name}_ms_per_step"] = round(med(name) / nt, 4)
    out["lonsections_over_maps"] = round(med("lonsections") / med("maps"), 3)
    pts = nyb * nx
    # the four cubes read once (T's neighbours are re-reads the caches may hold: not counted), the sections written and read twice by
    # the time sums, the factors written and read
    out["bytes_per_step"] = 8 * (4 * nl * pts + 3 * _lib.LEC_NMAP * nl * nx + 2 * nl * nyb * _lib.LEC_MAPS_NCOEF)
    out["lonsections_GBps"] = round(out["bytes_per_step"] * nt / (med("lonsections") * 1e-3) / 1e9, 1)
    return [out]


def moving(a, torch, _lib, LECEngine, dev):
    from tools.probes.time_composite import NL, NXB, NYB, series, timed
    import statistics
    steps = a.moving_steps
    lat, lon = np.arange(-60.0, 0.25, 0.25), np.arange(-100.0, 20.25, 0.25)
    level = np.linspace(1000.0, 100000.0, NL)
    time_s = np.arange(steps) * 21600.0
    eng = LECEngine(lat, lon, level, device=dev)
    boxes = [((t // 2) % 300, (t // 2) % 300 + NXB - 1, (t // 3) % 150, (t // 3) % 150 + NYB - 1) for t in range(steps)]
    pb = eng.prepare_boxes(boxes, packed=True)
    tcoef = eng.time_coefs_device(time_s)
    stream = torch.cuda.current_stream(dev)
    lines = []
    for dtype in (torch.float64, torch.float32):
        f = series(steps, dtype, dev)
        kw = eng.packed_dtdt(f["tm"], f["tair"], f["tp"], tcoef)
        fields = (f["tair"], f["u"], f["v"], f["omega"])

        def totals():
            rows = eng.rowstats(*fields, f["geopt"], pb, per_step_boxes=True, **kw)
            return rows, eng.reduce(rows, pb, drop_any_time=False)

        rows, _ = totals()
        levraw = eng._workspace(steps, NL, dev)[1].clone()

        def sections():
            st = eng.composite_lonsection_begin(steps, pb, dev)
            eng.composite_lonsection_stage(*fields, rows, pb, levraw, st, 0, **kw)
            return st

        for _ in range(2):
            totals()
            sections()
        torch.cuda.synchronize(dev)
        t12, ts = [], []
        for _ in range(a.repeat):
            t12.append(timed(totals, stream)[0])
            ts.append(timed(sections, stream)[0])
        med12, meds = statistics.median(t12), statistics.median(ts)
        lines.append({"bench": "lonsections_moving", "storage": str(dtype).replace("torch.", ""), "dTdt": "cube" if "dTdt" in kw else "tm/tp",
                      "box": [NL, NYB, NXB], "steps": steps, "repeat": a.repeat, "csrc_sha": _lib.source_digest(),
                      "stage1_plus_stage2_ms": {"median": med12, "min": min(t12), "max": max(t12)},
                      "composite_lonsections_ms": {"median": meds, "min": min(ts), "max": max(ts)},
                      "composite_lonsections_over_stage1_plus_stage2": meds / med12})
        del f, kw, rows, levraw
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--grid", type=int, nargs=3, default=[37, 721, 1440], metavar=("NL", "NY", "NX"))
    ap.add_argument("--moving", action="store_true", help="the moving boxes' call against stage 1 + stage 2 instead of the fixed box's")
    ap.add_argument("--moving-steps", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from lorenzcycletoolkit_amd import _lib
    from lorenzcycletoolkit_amd.engine import LECEngine
    if not torch.cuda.is_available():
        raise SystemExit("bench_lonsections.py needs a GPU: a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    lines = (moving if a.moving else fixed)(a, torch, _lib, LECEngine, dev)
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
