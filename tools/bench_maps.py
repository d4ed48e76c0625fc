#!/usr/bin/env python3
"""What the longitude-resolved maps cost (-f [--periodic] --maps): ``lec_maps`` alone on a near-global ring -- a 37 x 721 x 1440 fp64
grid, box +-89.75 degrees over all longitudes --, next to the ring pass ``lec_rowstats_ring`` of the same cubes (the yardstick: unchanged
code, timed in the same run), and a whole ``LECEngine.compute`` with and without ``maps``.

    python tools/bench_maps.py [--steps 4] [--rounds 3] [--repeat 5] [--out profiles/maps_bench.json]

Every call is timed with HIP events around it (median of ``--repeat`` after a warm-up) and the forms ALTERNATE within a round;
``--rounds`` rounds; reported: the median over the rounds, per call and per time step.  The bytes of the call are counted from the
shapes: the four cubes read once (T's neighbours in t, p, lat and lon are re-reads that the caches may or may not hold: not counted),
the column values written and read twice by the sums, the factors written and read.  One JSON line; ``--out`` writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--grid", type=int, nargs=3, default=[37, 721, 1440], metavar=("NL", "NY", "NX"))
    ap.add_argument("--no-compute", action="store_true", help="time the calls only, not the whole compute calls")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from lorenzcycletoolkit_amd import _lib
    from lorenzcycletoolkit_amd.engine import LECEngine
    if not torch.cuda.is_available():
        raise SystemExit("bench_maps.py needs a GPU: a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
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

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    rows = torch.empty((nt, nl, nyb, _lib.LEC_NSTAT), **f64)
    eng.rowstats(T, U, V, W, P, ring, time_s=time_s, rows_out=rows)
    levraw = torch.empty((nt, nl, _lib.LEC_NLEVRAW), **f64)
    eng.level_stage(rows, ring, levraw)
    st = eng.map_begin(nt, ring, dev)
    torch.cuda.synchronize()

    calls = [("ring_pass", lambda: eng.rowstats(T, U, V, W, P, ring, time_s=time_s, rows_out=rows)),
             ("maps", lambda: eng.map_stage(T, U, V, W, rows, ring, levraw, st, 0, time_s=time_s))]
    if not a.no_compute:
        calls += [("compute", lambda: eng.compute(T, U, V, W, P, ring, time_s=time_s)),
                  ("compute_maps", lambda: eng.compute(T, U, V, W, P, ring, time_s=time_s, maps=True))]
    out = {"grid": [nl, ny, nx], "steps": nt, "dtype": "float64", "box_rows": nyb, "box_columns": nx, "rounds": a.rounds,
           "repeat": a.repeat, "map_chunk_bytes": int(LECEngine.MAP_CHUNK_BYTES), "csrc_sha": _lib.source_digest()}
    for _ in range(a.rounds):
        for name, fn in calls:
            out.setdefault(f"{name}_ms", []).append(round(timed(fn), 4))
    med = lambda k: float(np.median(out[f"{k}_ms"]))
    for name, _ in calls:
        out[f"{name}_ms_per_step"] = round(med(name) / nt, 4)
    out["maps_over_ring_pass"] = round(med("maps") / med("ring_pass"), 3)
    if not a.no_compute:
        out["compute_maps_over_compute"] = round(med("compute_maps") / med("compute"), 3)
    pts = nyb * nx
    out["bytes_per_step"] = 8 * (4 * nl * pts + 3 * _lib.LEC_NMAP * pts + 2 * nl * nyb * _lib.LEC_MAPS_NCOEF)
    out["maps_GBps"] = round(out["bytes_per_step"] * nt / (med("maps") * 1e-3) / 1e9, 1)
    out["ring_pass_cube_bytes_per_step"] = 8 * 5 * nl * pts
    out["ring_pass_GBps"] = round(out["ring_pass_cube_bytes_per_step"] * nt / (med("ring_pass") * 1e-3) / 1e9, 1)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
