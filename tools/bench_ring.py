#!/usr/bin/env python3
"""What a ring pass of stage 1 costs: ``lec_rowstats_ring`` (-f --periodic) next to ``lec_rowstats`` with ``tuning.kernel =
LEC_KERNEL_ROW_SWEEP`` on the same cubes -- a global 37 x 721 x 1440 fp64 grid, all terms (dT/dt from the cube's time axis), box
+-89.75 degrees over all longitudes.  Only the first and last trip of a 1440-column row differ between the two, so the expectation is
the same time.

    python tools/bench_ring.py [--steps 8] [--rounds 5] [--repeat 5] [--parent PATH] [--out FILE]

The calls are timed with HIP events around the call (median of ``--repeat`` after a warm-up) and ALTERNATE within a round; ``--rounds``
rounds.  ``--parent PATH``: a liblec_hip.so built from the parent commit, loaded beside this one -- its non-ring row sweep is the
baseline, and the spread of its rounds' medians is the margin the ring gets.  Without it the baseline is this library's own non-ring
row sweep.  Also timed: this library's AUTO choice for the limited-area call (the row-block kernel, which has no ring form): what AUTO on
a ring gives up -- and, with ``--parent``, the parent's AUTO call beside it (the shipped kernels must cost what they cost).  One JSON line; ``--out`` writes it to a file."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--grid", type=int, nargs=3, default=[37, 721, 1440], metavar=("NL", "NY", "NX"))
    ap.add_argument("--parent", default=None, metavar="PATH")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from lorenzcycletoolkit_amd import _lib
    from lorenzcycletoolkit_amd.engine import LECEngine, make_tuning
    if not torch.cuda.is_available():
        raise SystemExit("bench_ring.py needs a GPU: a time is measured on the device or not at all")
    lib = _lib.load()
    dev = torch.device("cuda:0")
    nl, ny, nx = a.grid
    nt = a.steps
    lat = np.linspace(-90.0, 90.0, ny)
    lon = -180.0 + 360.0 / nx * np.arange(nx)
    level = np.linspace(100.0, 100000.0, nl)
    eng = LECEngine(lat, lon, level, device=dev)
    box = (0, nx - 1, 1, ny - 2)                         # +-89.75 degrees on the 0.25-degree grid: the polar rows stay out
    g = torch.Generator(device=dev).manual_seed(1)
    shape = (nt, nl, ny, nx)
    T = 250.0 + 10.0 * torch.randn(shape, dtype=torch.float64, device=dev, generator=g)
    U, V, W, P = (torch.randn(shape, dtype=torch.float64, device=dev, generator=g) for _ in range(4))
    tcoef = eng.time_coefs_device(21600.0 * np.arange(nt))
    rows = torch.empty((nt, nl, ny - 2, _lib.LEC_NSTAT), dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def args_of(pb, kernel):
        return _lib.RowstatsArgs(
            tair_d=ptr(T), u_d=ptr(U), v_d=ptr(V), omega_d=ptr(W), geopt_d=ptr(P), dTdt_d=None, dtype=_lib.LEC_F64, with_q=1,
            nt=nt, nl=nl, ny=ny, nx=nx, t_begin=0, t_count=nt, n_box=1, nxb_max=pb.bt.nxb_max, nyb_max=pb.bt.nyb_max, lon_uniform=1,
            box_per_step=0, reserved0=0, box_d=ptr(pb.dev["box"]), boxtab_d=ptr(pb.dev["boxtab"]), wlon_d=ptr(pb.dev["wlon"]),
            glon_d=ptr(pb.dev["glon"]), lattab_d=ptr(pb.dev["lattab"]), levtab_d=ptr(eng._levtab), tcoef_d=ptr(tcoef), rows_d=ptr(rows),
            stream=stream, tuning=make_tuning({"kernel": kernel}), tm_d=None, tp_d=None)

    plain, ring = eng.prepare_boxes([box]), eng.prepare_boxes([box], ring=True)
    old = lib
    if a.parent:
        old = C.CDLL(a.parent)
        old.lec_rowstats.restype, old.lec_rowstats.argtypes = C.c_int, [C.POINTER(_lib.RowstatsArgs)]
    calls = [("parent_row_sweep" if a.parent else "baseline_row_sweep", old, "lec_rowstats", args_of(plain, "row_sweep")),
             ("ring", lib, "lec_rowstats_ring", args_of(ring, "auto")),
             ("row_sweep", lib, "lec_rowstats", args_of(plain, "row_sweep")),
             ("auto_row_block", lib, "lec_rowstats", args_of(plain, "auto"))]
    if a.parent:        # what the ring's instantiations cost the shipped headline kernel: the parent's AUTO call beside this library's
        calls.append(("parent_auto_row_block", old, "lec_rowstats", args_of(plain, "auto")))

    def run(which, call, ra):
        if getattr(which, call)(C.byref(ra)):
            raise RuntimeError(f"{call} failed: {lib.lec_last_error()}")

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
        return float(np.median(ms)), [round(x, 4) for x in ms]

    out = {"grid": [nl, ny, nx], "steps": nt, "dtype": "float64", "box_rows": ny - 2, "parent_library": bool(a.parent), "rounds": a.rounds,
           "repeat": a.repeat, "csrc_sha": _lib.source_digest()}
    for _ in range(a.rounds):
        for name, which, call, ra in calls:
            med, all_ms = timed(lambda: run(which, call, ra))
            out.setdefault(f"{name}_ms", []).append(round(med, 4))
            out.setdefault(f"{name}_all_ms", []).append(all_ms)
    base = out[calls[0][0] + "_ms"]
    out["baseline_median_ms"] = round(float(np.median(base)), 4)
    out["baseline_spread_ms"] = round(max(base) - min(base), 4)
    for name in ["ring", "row_sweep", "auto_row_block"] + (["parent_auto_row_block"] if a.parent else []):
        out[f"{name}_median_ms"] = round(float(np.median(out[f"{name}_ms"])), 4)
    out["ring_minus_baseline_ms"] = round(out["ring_median_ms"] - out["baseline_median_ms"], 4)
    out["ring_within_spread"] = bool(out["ring_minus_baseline_ms"] <= out["baseline_spread_ms"])
    out["ring_over_auto_row_block"] = round(out["ring_median_ms"] / out["auto_row_block_median_ms"], 4)
    # bytes the algorithm needs per pass (5 fields read once, the records written) over the ring's time: a rate, not a share of peak
    algo_bytes = 5 * T.numel() * 8 + rows.numel() * 8
    out["ring_algorithmic_GBps"] = round(algo_bytes / (out["ring_median_ms"] * 1e-3) / 1e9, 1)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
