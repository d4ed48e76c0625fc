#!/usr/bin/env python3
"""What the latitude-pressure sections cost (-f [--periodic] --sections): ``lec_sections`` alone on the records of a global ring -- a
37 x 721 x 1440 fp64 grid, box +-89.75 degrees over all longitudes --, at N = 0 (the ten terms) and at N wavenumbers (the spectral terms
too), next to the ring pass ``lec_rowstats_ring`` and the fused level stage ``lec_level_spec_ring`` of the same N, and a whole
``LECEngine.compute`` with and without ``sections``.

    python tools/bench_sections.py [--steps 4] [--rounds 3] [--repeat 5] [--n 20] [--out profiles/sections_bench.json]

Every call is timed with HIP events around it (median of ``--repeat`` after a warm-up) and the forms ALTERNATE within a round;
``--rounds`` rounds; reported: the median over the rounds, per call and per time step.  The bytes of the call are counted from the
shapes: the records read, the sections written and read once more by the fold.  One JSON line; ``--out`` writes it to a file."""
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
    ap.add_argument("--n", type=int, default=20, help="wavenumbers of the spectral form")
    ap.add_argument("--no-compute", action="store_true", help="time the calls only, not the whole compute calls")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from lorenzcycletoolkit_amd import _lib
    from lorenzcycletoolkit_amd.engine import LECEngine
    if not torch.cuda.is_available():
        raise SystemExit("bench_sections.py needs a GPU: a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    nl, ny, nx = a.grid
    nt, n = a.steps, a.n
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
    spec = eng.rowspec(T, U, V, W, ring, n)
    qspec = eng.rowspec_q(T, U, V, W, ring, n, time_s=time_s)
    levraw_n = torch.empty((n, nt, nl, _lib.LEC_NLEVRAW), **f64)
    st0 = eng.section_begin(nt, nyb, dev)
    stn = eng.section_begin(nt, nyb, dev, n_wave=n, generation=True)
    torch.cuda.synchronize()

    calls = [("ring_pass", lambda: eng.rowstats(T, U, V, W, P, ring, time_s=time_s, rows_out=rows)),
             ("level_stage", lambda: eng.level_stage(rows, ring, levraw)),
             ("sections_N0", lambda: eng.section_stage(rows, ring, levraw, st0, 0)),
             (f"level_spec_N{n}", lambda: eng.spectrum_level_stage(rows, spec, qspec, ring, levraw_n)),
             (f"sections_N{n}", lambda: eng.section_stage(rows, ring, levraw, stn, 0, spec=spec, qspec=qspec))]
    if not a.no_compute:
        kw = dict(time_s=time_s)
        kwn = dict(time_s=time_s, wavenumbers=n, spectrum_generation=True, spectrum_fused=True)
        calls += [("compute", lambda: eng.compute(T, U, V, W, P, ring, **kw)),
                  ("compute_sections", lambda: eng.compute(T, U, V, W, P, ring, sections=True, **kw)),
                  (f"compute_N{n}", lambda: eng.compute(T, U, V, W, P, ring, **kwn)),
                  (f"compute_N{n}_sections", lambda: eng.compute(T, U, V, W, P, ring, sections=True, **kwn))]
    out = {"grid": [nl, ny, nx], "steps": nt, "dtype": "float64", "box_rows": nyb, "rounds": a.rounds, "repeat": a.repeat, "n": n,
           "csrc_sha": _lib.source_digest()}
    for _ in range(a.rounds):
        for name, fn in calls:
            out.setdefault(f"{name}_ms", []).append(round(timed(fn), 4))
    med = lambda k: float(np.median(out[f"{k}_ms"]))
    for name, _ in calls:
        out[f"{name}_ms_per_step"] = round(med(name) / nt, 4)
    out["sections_N0_over_ring_pass"] = round(med("sections_N0") / med("ring_pass"), 3)
    out[f"sections_N{n}_over_level_spec_N{n}"] = round(med(f"sections_N{n}") / med(f"level_spec_N{n}"), 3)
    if not a.no_compute:
        out["compute_sections_over_compute"] = round(med("compute_sections") / med("compute"), 3)
        out[f"compute_N{n}_sections_over_compute_N{n}"] = round(med(f"compute_N{n}_sections") / med(f"compute_N{n}"), 3)
    rec = nl * nyb
    out["bytes_per_step_N0"] = rec * (_lib.LEC_NSTAT * 8 + 3 * 10 * 8)
    out[f"bytes_per_step_N{n}"] = out["bytes_per_step_N0"] + rec * n * (_lib.LEC_NSTAT * 8 + 64 + 8 + 3 * 6 * 8)
    out["sections_N0_GBps"] = round(out["bytes_per_step_N0"] * nt / (med("sections_N0") * 1e-3) / 1e9, 1)
    out[f"sections_N{n}_GBps"] = round(out[f"bytes_per_step_N{n}"] * nt / (med(f"sections_N{n}") * 1e-3) / 1e9, 1)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
