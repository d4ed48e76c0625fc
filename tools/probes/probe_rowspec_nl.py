#!/usr/bin/env python3
"""What one call of ``lec_rowspec_nl_ring`` costs next to its two siblings on the same cubes and with the same N: a global
37 x 721 x 1440 fp64 grid, band +-89.75 degrees over all longitudes, N = 20, as many time steps as asked for (default 4).

    python tools/probes/probe_rowspec_nl.py [--steps 4] [--n 20] [--rounds 3] [--repeat 5] [--lib NAME=PATH ...] [--out FILE]

The three calls -- ``lec_rowspec_nl_ring``, ``lec_rowspec_q_ring``, ``lec_rowspec_ring`` -- are timed with HIP events around the call
(median of ``--repeat`` after a warm-up) and ALTERNATE within a round; the median over the rounds is reported as ms per call and steps
per second.  For the new call also the part of the vector fp64 FMA rate of the part (78.6 TFLOP/s = 39.3 T FMA/s) that the 12 FMAs
per (row, column, n) of its projection amount to -- a count from the shapes, not a counter.  ``--lib NAME=PATH``: another build of the
library (another trip length or rows per workgroup of the new kernel; or the parent commit's build for the two siblings), whose calls
are timed in the same rounds under ``NAME:``.  One JSON line; ``--out`` writes it to a file."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

FP64_VECTOR_PEAK_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--grid", type=int, nargs=3, default=[37, 721, 1440], metavar=("NL", "NY", "NX"))
    ap.add_argument("--lib", nargs="*", default=[], metavar="NAME=PATH")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from lorenzcycletoolkit_amd import _lib, tables
    from lorenzcycletoolkit_amd.engine import LECEngine
    if not torch.cuda.is_available():
        raise SystemExit("probe_rowspec_nl.py needs a GPU: a time is measured on the device or not at all")
    lib = _lib.load()
    dev = torch.device("cuda:0")
    nl, ny, nx = a.grid
    nt, n = a.steps, a.n
    lat = np.linspace(-90.0, 90.0, ny)
    lon = -180.0 + 360.0 / nx * np.arange(nx)
    level = np.linspace(100.0, 100000.0, nl)
    eng = LECEngine(lat, lon, level, device=dev)
    js, jn = 1, ny - 2                                   # the polar rows stay out
    ring = eng.prepare_boxes([(0, nx - 1, js, jn)], ring=True)
    g = torch.Generator(device=dev).manual_seed(1)
    shape = (nt, nl, ny, nx)
    T = 250.0 + 10.0 * torch.randn(shape, dtype=torch.float64, device=dev, generator=g)
    U, V, W, P = (torch.randn(shape, dtype=torch.float64, device=dev, generator=g) for _ in range(4))
    time_s = 21600.0 * np.arange(max(nt, 2))[:nt]
    nyb = jn - js + 1
    rows = eng.rowstats(T, U, V, W, P, ring, time_s=time_s if nt > 1 else None, with_q=nt > 1)
    twid = eng._up(tables.twiddle_table(nx))
    lat5 = eng._up(tables.nl_lat_table(ring.bt.lattab[0], lat[js:jn + 1]))
    ptab = eng._up(tables.pressure_coefs(level))
    tcoef = eng.time_coefs_device(time_s) if nt > 1 else None
    f64 = dict(dtype=torch.float64, device=dev)
    nlspec, nltot = torch.empty((nt, nl, nyb, n, 8), **f64), torch.empty((nt, nl, nyb, 8), **f64)
    spec, qspec = torch.empty((nt, nl, nyb, n, 8), **f64), torch.empty((nt, nl, nyb, n), **f64)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    common = dict(tair_d=ptr(T), u_d=ptr(U), v_d=ptr(V), omega_d=ptr(W), dtype=_lib.LEC_F64, nt=nt, nl=nl, ny=ny, nx=nx, t_begin=0, t_count=nt,
                  js=js, jn=jn, n_wave=n, twid_d=ptr(twid), stream=stream)
    args = {
        "lec_rowspec_nl_ring": _lib.RowspecNlArgs(rows_d=ptr(rows), lattab_d=ptr(lat5), ptab_d=ptr(ptab), inv_hdeg=float(ring.bt.boxtab[0, 2]),
                                                  nlspec_d=ptr(nlspec), nltot_d=ptr(nltot), **common),
        "lec_rowspec_ring": _lib.RowspecArgs(spec_d=ptr(spec), **common),
    }
    if nt > 1:       # (Q holds dT/dt over the cube's time axis)
        args["lec_rowspec_q_ring"] = _lib.RowspecQArgs(lattab_d=ptr(ring.dev["lattab"]), levtab_d=ptr(eng._levtab), tcoef_d=ptr(tcoef),
                                                       inv_hdeg=float(ring.bt.boxtab[0, 2]), qspec_d=ptr(qspec), **common)
    libs = [("", lib)]
    for item in a.lib:
        name, path = item.split("=", 1)
        other = C.CDLL(path)
        libs.append((name + ":", other))

    def call(which, name):
        fn = getattr(which, name)
        fn.restype = C.c_int
        if fn(C.byref(args[name])):
            raise RuntimeError(f"{name} failed: {lib.lec_last_error()}")

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

    runs = {}
    for _ in range(a.rounds):
        for tag, which in libs:
            for name in args:
                if tag and not hasattr(which, name):
                    continue
                runs.setdefault(tag + name, []).append(timed(lambda: call(which, name)))
    out = {"grid": [nl, ny, nx], "steps": nt, "n": n, "dtype": "float64", "band_rows": nyb, "rounds": a.rounds, "repeat": a.repeat,
           "csrc_sha": _lib.source_digest(), "fp64_vector_peak_TFLOPs": FP64_VECTOR_PEAK_TFLOPS, "calls": {}}
    fma = 12.0 * nt * nl * nyb * nx * n
    for key, ms in runs.items():
        med = float(np.median(ms))
        rec = {"ms_per_call": round(med, 4), "ms_per_call_rounds": [round(x, 4) for x in ms], "steps_per_s": round(nt / (med * 1e-3), 1)}
        if key.endswith("lec_rowspec_nl_ring"):
            rec["fraction_of_fp64_fma_rate"] = round(fma / (med * 1e-3) / (FP64_VECTOR_PEAK_TFLOPS * 1e12 / 2), 4)
        out["calls"][key] = rec
    own = out["calls"]
    if "lec_rowspec_q_ring" in own:
        out["nl_over_q"] = round(own["lec_rowspec_nl_ring"]["ms_per_call"] / own["lec_rowspec_q_ring"]["ms_per_call"], 3)
    out["nl_over_spec"] = round(own["lec_rowspec_nl_ring"]["ms_per_call"] / own["lec_rowspec_ring"]["ms_per_call"], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
