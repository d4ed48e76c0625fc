#!/usr/bin/env python3
"""What the row-block kernel's workgroup schedule is worth: ``lec_rowstats`` (AUTO: ``lec_rowblock_kernel`` + ``lec_qtime_kernel``) of
this library beside the same call of another build -- the parent commit's -- in ONE process, on the cubes ``bench.py`` times: a global
37 x 721 x 1440 fp64 grid, all terms (dT/dt from the cube's time axis), the box = the whole grid, 64 steps.

    python tools/bench_schedule.py --parent PATH [--steps 64] [--rounds 5] [--repeat 10] [--tuning k=v,...] [--out FILE]

HIP events around the call, median of ``--repeat`` calls after a warm-up; the libraries ALTERNATE within a round, ``--rounds`` rounds;
the parent's library is timed twice per round (first and last), so the spread of one build against itself stands beside the difference.
``separated``: every round's median of this library lies below every round's median of the parent's -- the only outcome that counts as a
gain.  The records of the two libraries are compared bit for bit before anything is timed.  One JSON line; ``--out`` writes it to a file."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, metavar="PATH", help="a liblec_hip.so of the same ABI built from the parent commit")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--grid", type=int, nargs=3, default=[37, 721, 1440], metavar=("NL", "NY", "NX"))
    ap.add_argument("--tuning", default="", help="lec_tuning fields for both libraries, e.g. tile_j=8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from lorenzcycletoolkit_amd import _lib
    from lorenzcycletoolkit_amd.engine import LECEngine, make_tuning
    if not torch.cuda.is_available():
        raise SystemExit("bench_schedule.py needs a GPU: a time is measured on the device or not at all")
    lib = _lib.load()
    old = C.CDLL(a.parent)
    old.lec_rowstats.restype, old.lec_rowstats.argtypes = C.c_int, [C.POINTER(_lib.RowstatsArgs)]
    dev = torch.device("cuda:0")
    nl, ny, nx = a.grid
    nt = a.steps
    eng = LECEngine(np.linspace(-90.0, 90.0, ny), -180.0 + 360.0 / nx * np.arange(nx), np.linspace(100.0, 100000.0, nl), device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    shape = (nt, nl, ny, nx)
    T = 250.0 + 10.0 * torch.randn(shape, dtype=torch.float64, device=dev, generator=g)
    U, V, W, P = (torch.randn(shape, dtype=torch.float64, device=dev, generator=g) for _ in range(4))
    tcoef = eng.time_coefs_device(21600.0 * np.arange(nt))
    pb = eng.prepare_boxes([(0, nx - 1, 0, ny - 1)])
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    tuning = dict(kv.split("=") for kv in a.tuning.split(",") if kv)
    tuning = {k: (v if k in ("kernel", "order") else int(v)) for k, v in tuning.items()}

    def args_of(rows):
        return _lib.RowstatsArgs(
            tair_d=ptr(T), u_d=ptr(U), v_d=ptr(V), omega_d=ptr(W), geopt_d=ptr(P), dTdt_d=None, dtype=_lib.LEC_F64, with_q=1,
            nt=nt, nl=nl, ny=ny, nx=nx, t_begin=0, t_count=nt, n_box=1, nxb_max=pb.bt.nxb_max, nyb_max=pb.bt.nyb_max, lon_uniform=1,
            box_per_step=0, reserved0=0, box_d=ptr(pb.dev["box"]), boxtab_d=ptr(pb.dev["boxtab"]), wlon_d=ptr(pb.dev["wlon"]),
            glon_d=ptr(pb.dev["glon"]), lattab_d=ptr(pb.dev["lattab"]), levtab_d=ptr(eng._levtab), tcoef_d=ptr(tcoef), rows_d=ptr(rows),
            stream=stream, tuning=make_tuning(tuning), tm_d=None, tp_d=None)

    rows_new, rows_old = (torch.full((nt, nl, ny, _lib.LEC_NSTAT), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
    calls = [("parent", old, args_of(rows_old)), ("this", lib, args_of(rows_new)), ("parent_again", old, args_of(rows_old))]

    def run(which, ra):
        if which.lec_rowstats(C.byref(ra)):
            raise RuntimeError(f"lec_rowstats failed: {lib.lec_last_error()}")

    for _, which, ra in calls[:2]:
        run(which, ra)
    torch.cuda.synchronize()
    # by bits: the polar rows of the whole-grid box divide by cos(90 deg), so their records hold non-finite values in either library;
    # a row one library left unwritten keeps the buffer's NaN and differs from the other's record
    same = bool(torch.equal(rows_new.view(torch.int64), rows_old.view(torch.int64)))

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

    out = {"grid": [nl, ny, nx], "steps": nt, "dtype": "float64", "box_rows": ny, "tuning": a.tuning, "rounds": a.rounds, "repeat": a.repeat,
           "csrc_sha": _lib.source_digest(), "records_bit_equal": same}
    for _ in range(a.rounds):
        for name, which, ra in calls:
            med, all_ms = timed(lambda: run(which, ra))
            out.setdefault(f"{name}_ms", []).append(round(med, 4))
            out.setdefault(f"{name}_all_ms", []).append(all_ms)
    par = out["parent_ms"] + out["parent_again_ms"]
    out["parent_median_ms"] = round(float(np.median(par)), 4)
    out["parent_spread_ms"] = round(max(par) - min(par), 4)
    out["this_median_ms"] = round(float(np.median(out["this_ms"])), 4)
    out["this_spread_ms"] = round(max(out["this_ms"]) - min(out["this_ms"]), 4)
    out["this_over_parent"] = round(out["this_median_ms"] / out["parent_median_ms"], 5)
    out["separated"] = bool(max(out["this_ms"]) < min(par))
    out["not_slower"] = bool(out["this_median_ms"] <= out["parent_median_ms"] + out["parent_spread_ms"])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("the records of the two libraries differ")


if __name__ == "__main__":
    main()
