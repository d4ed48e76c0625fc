#!/usr/bin/env python3
"""Many tracks over one data set: one batch pass (``LECEngine.compute(steps=...)``, ``lec_rowstats_steps``) against the loop of
single-track computations the moving framework runs today, on a seeded synthetic data set at ERA5 spacing (37 levels, 0.25 degrees,
a regional union crop, K tracks of ~40 six-hourly steps with 15 x 15 degree boxes).  Prints ONE JSON line:

  batch        one upload of the union cubes, then stage 1 + stage 2 per group of tracks (device events, after a synchronize)
  loop         K single-track resident computations in-process, as frameworks.BoxData does them (host slice of every box, upload of
               the box-packed series, lec_dtdt / stage 1 / stage 2); its terms must equal the batch's bit for bit (checked)
  one_track    lec_rowstats on the cube with t +- 1 addressing against lec_rowstats_steps with the identity table: same records
               (checked), kernel times of both

``--cli``: the command line instead -- K single ``-r -t --trackfile`` processes one after another against ONE ``-r -t --trackfiles``
process over the same seeded file (synthetic.write_classic_nc: float32, 7 levels, 1 degree, 40 three-hourly steps; K tracks of 16
steps, default 15 x 15 degree boxes), both wall clocks and whether every track's results CSV and trackfile are the same bytes.  Works
in a temporary directory.  ``--cli --batch-chunk N``: on the same file and tracks, the ``--trackfiles`` run prepared on the host against
the streamed one (``--batch-chunk N``), ``--reps`` runs of each in turn after one untimed run of each: every wall clock, the medians, the
streamed run's own phase seconds from its log, and whether every file of every track's tree is the same bytes.  ``--host-cli PATH``: the
host-prepared leg runs another checkout's lorenzcycletoolkit.py (the parent commit's, for a comparison that does not rest on this tree).

``--batch-composites``: the batch's ``compute`` calls also composite their tracks (``batch_composites=sizes``; the loop leg and the bits
check are as without it).  ``--batch-composites-phase lifetime:B`` (with it): also the phase-aligned ensembles
(``batch_composite_phases=``), and the JSON line carries the two phase kernels' own times, HIP events around ``lec_composite_phase_sum``
over all of the batch's boxes in one call and around ``lec_composite_phase_ensemble``, on buffers of the batch's shapes.

Reads nothing outside the tree.  Usage: python tools/bench_batch.py [--tracks K] [--steps 40] [--reps 5] [--batch-composites
       [--batch-composites-phase lifetime:B]] | --cli [--tracks K] [--batch-chunk N [--reps 5] [--host-cli PATH]]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lorenzcycletoolkit_amd import tables                                     # noqa: E402
from lorenzcycletoolkit_amd.engine import LECEngine, pack_host               # noqa: E402
from lorenzcycletoolkit_amd.synthetic import era5_like_levels, synthetic_cube  # noqa: E402

HBM_PEAK_GBS = 8000.0          # as bench.py


def _tracks(k, n, nt, lat, lon, rng):
    """K tracks of n six-hourly steps (the data are 6-hourly): start step, centre drifting east / south-east, 15 x 15 degree boxes."""
    out = []
    for _ in range(k):
        t0 = int(rng.integers(0, nt - n + 1))
        la0, lo0 = rng.uniform(lat[0] + 10, lat[-1] - 15), rng.uniform(lon[0] + 10, lon[-1] - 25)
        steps = np.arange(t0, t0 + n)
        cen = [(la0 - 0.05 * i, lo0 + 0.3 * i) for i in range(n)]
        out.append((steps, [tables.box_indices(lat, lon, c[1] - 7.5, c[1] + 7.5, c[0] - 7.5, c[0] + 7.5) for c in cen]))
    return out


def _events():
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    return a, b


def _phase_kernel_times(eng, group, dev, reps):
    """The two phase kernels alone on buffers of the group's shapes: lec_composite_phase_sum over all the group's boxes in ONE call (the
    engine issues it per sub-call) and lec_composite_phase_ensemble; HIP events around each call, medians and quartiles over ``reps``."""
    import ctypes as C

    from lorenzcycletoolkit_amd import _lib
    members, pb, st, tc, extra = group
    sizes, ranges = extra["batch_composites"], extra["batch_composite_phases"]
    state = eng.batch_composite_begin(sizes, pb, dev, phases=ranges)
    nyb, nxb, S = state["nyb"], state["nxb"], int(sum(sizes))
    col = torch.randn((S, _lib.LEC_NMAP, nyb, nxb), dtype=torch.float64, device=dev)
    rng_h = np.ascontiguousarray(state["phase_abs"], dtype=np.int32)
    rng_d = torch.as_tensor(rng_h).to(dev)
    ps, cnt = state["phasesum"], state["phase_count"]
    ens, spread = torch.empty_like(ps[0]), torch.empty_like(ps[0])
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    sa = _lib.CompositePhaseSumArgs(col_d=p(col), range_h=C.c_void_p(rng_h.ctypes.data), range_d=p(rng_d), phasesum_d=p(ps), s_count=S, nyb=nyb,
                                    nxb=nxb, n_cell=int(rng_h.shape[0]), reserved0=0, stream=stream)
    mean = torch.empty_like(ps)
    ea = _lib.CompositePhaseEnsembleArgs(phasesum_d=p(ps), count_h=C.c_void_p(cnt.ctypes.data), count_d=p(state["phase_count_dev"]),
                                         n_track=int(ps.shape[0]), n_bin=int(ps.shape[1]), nyb=nyb, nxb=nxb, reserved0=0, mean_d=p(mean),
                                         ens_d=p(ens), spread_d=p(spread), stream=stream)
    ts, te = [], []
    for r in range(reps + 2):                   # (two warm-up rounds)
        e = [_events(), _events()]
        e[0][0].record(); _lib.check(eng.lib.lec_composite_phase_sum(C.byref(sa)), "lec_composite_phase_sum"); e[0][1].record()
        e[1][0].record(); _lib.check(eng.lib.lec_composite_phase_ensemble(C.byref(ea)), "lec_composite_phase_ensemble"); e[1][1].record()
        torch.cuda.synchronize()
        if r >= 2:
            ts.append(e[0][0].elapsed_time(e[0][1]))
            te.append(e[1][0].elapsed_time(e[1][1]))
    q = lambda v: {"median": float(np.median(v)), "iqr": [float(np.percentile(v, 25)), float(np.percentile(v, 75))]}
    return {"boxes": S, "cells": int(rng_h.shape[0]), "box_points": [nyb, nxb], "lec_composite_phase_sum": q(ts), "lec_composite_phase_ensemble": q(te),
            "bytes_read_by_phase_sum": int(8 * S * _lib.LEC_NMAP * nyb * nxb)}


CLI_FILE = "synthetic.write_classic_nc: float32 classic NetCDF, 7 levels, 1 degree, 40 three-hourly steps"


def _cli_case(work: str, k: int, seed: int):
    """The seeded file and K track files of the command-line legs, in ``work``: (data file, track files)."""
    import shutil

    import pandas as pd
    from lorenzcycletoolkit_amd.synthetic import write_classic_nc
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(work, "inputs"))
    shutil.copy(os.path.join(ROOT, "tests", "golden", "inputs", "namelist_ERA5"), os.path.join(work, "inputs", "namelist"))
    infile = os.path.join(work, "synth.nc")
    write_classic_nc(infile, np.float32, nt=40, seed=seed)
    tracks = []
    for i in range(k):
        t0, n = int(rng.integers(0, 20)), 16
        rows = [f"{(pd.Timestamp('2020-01-01') + pd.Timedelta(hours=3 * (t0 + s))).strftime('%Y-%m-%d-%H%M')};"
                f"{-35 + rng.uniform(-5, 5) - 0.2 * s:.2f};{-55 + rng.uniform(-8, 8) + 0.4 * s:.2f}" for s in range(n)]
        p = os.path.join(work, f"trk{i:02d}")
        with open(p, "w") as f:
            f.write("time;Lat;Lon\n" + "\n".join(rows) + "\n")
        tracks.append(p)
    return infile, tracks


def cli_streamed_batch(k: int, seed: int, chunk: int, reps: int, host_cli: str = None) -> dict:
    """One --trackfiles process prepared on the host against one with --batch-chunk ``chunk`` (see the module docstring)."""
    import filecmp
    import shutil
    import subprocess
    import tempfile
    cli = os.path.join(ROOT, "lorenzcycletoolkit.py")
    host_cli = os.path.abspath(host_cli) if host_cli else cli           # (the legs run in the temporary directory)
    with tempfile.TemporaryDirectory() as work:
        infile, tracks = _cli_case(work, k, seed)
        results, kept = os.path.join(work, "LEC_Results"), os.path.join(work, "host_results")

        def run(program, extra):
            shutil.rmtree(results, ignore_errors=True)
            t0 = time.perf_counter()
            subprocess.run([sys.executable, program, infile, "-r", "-t", "--trackfiles", *tracks, *extra], cwd=work, check=True, capture_output=True, timeout=600)
            return time.perf_counter() - t0

        legs = {"host": (host_cli, []), "streamed": (cli, ["--batch-chunk", str(chunk)])}
        wall = {name: [] for name in legs}
        same, seconds = None, []
        for r in range(reps + 1):                    # (the first run of each: untimed -- page cache, code objects)
            for name, (program, extra) in legs.items():
                s = run(program, extra)
                if r:
                    wall[name].append(s)
                if name == "host" and same is None:
                    shutil.copytree(results, kept)
                if name == "streamed":
                    log = open(os.path.join(results, "synth_track_batch", "log.synth")).read()
                    line = [x for x in log.splitlines() if "Streamed batch seconds: " in x][-1].split("Streamed batch seconds: ")[1]
                    if r:
                        seconds.append({p.rsplit(" ", 1)[0]: float(p.rsplit(" ", 1)[1]) for p in line.split(", ")})
                    if same is None:
                        same = True
                        for p in tracks:
                            tree = f"synth_{os.path.basename(p)}_track"
                            for root, _dirs, files in os.walk(os.path.join(kept, tree)):
                                for f in files:
                                    if not f.startswith("log."):
                                        other = os.path.join(results, os.path.relpath(os.path.join(root, f), kept))
                                        same = same and os.path.exists(other) and filecmp.cmp(os.path.join(root, f), other, shallow=False)
    med = {name: float(np.median(v)) for name, v in wall.items()}
    return {"tracks": k, "steps_per_track": 16, "file": CLI_FILE, "batch_chunk": chunk, "reps": reps,
            "what": "one `-r -t --trackfiles` process prepared on the host vs one with --batch-chunk, in turn, same file and tracks; one untimed run of each first",
            "host_cli": os.path.relpath(host_cli, ROOT), "host_batch_s": [round(x, 3) for x in wall["host"]],
            "streamed_batch_s": [round(x, 3) for x in wall["streamed"]], "host_batch_s_median": med["host"], "streamed_batch_s_median": med["streamed"],
            "host_batch_s_range": [float(np.min(wall["host"])), float(np.max(wall["host"]))],
            "streamed_batch_s_range": [float(np.min(wall["streamed"])), float(np.max(wall["streamed"]))],
            "streamed_over_host": med["streamed"] / med["host"], "streamed_phase_seconds": seconds, "every_file_identical": bool(same)}


def cli_wall_clock(k: int, seed: int) -> dict:
    """K single-track CLI processes against one --trackfiles process on the same file (see the module docstring)."""
    import filecmp
    import shutil
    import subprocess
    import tempfile
    cli = os.path.join(ROOT, "lorenzcycletoolkit.py")
    with tempfile.TemporaryDirectory() as work:
        infile, tracks = _cli_case(work, k, seed)
        t0 = time.perf_counter()
        for p in tracks:
            subprocess.run([sys.executable, cli, infile, "-r", "-t", "--trackfile", p], cwd=work, check=True, capture_output=True, timeout=300)
            shutil.move(os.path.join(work, "LEC_Results", "synth_track"), os.path.join(work, "single_" + os.path.basename(p)))
        single_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        subprocess.run([sys.executable, cli, infile, "-r", "-t", "--trackfiles", *tracks], cwd=work, check=True, capture_output=True, timeout=600)
        batch_s = time.perf_counter() - t0
        same = all(filecmp.cmp(os.path.join(work, "single_" + os.path.basename(p), f),
                               os.path.join(work, "LEC_Results", f"synth_{os.path.basename(p)}_track", f), shallow=False)
                   for p in tracks for f in ("synth_track_results.csv", "synth_track_trackfile"))
    return {"tracks": k, "steps_per_track": 16, "file": CLI_FILE,
            "what": f"{k} single `-r -t --trackfile` processes one after another vs one `-r -t --trackfiles` process, same file",
            "single_runs_s": single_s, "batch_run_s": batch_s, "speedup": single_s / batch_s, "results_and_trackfiles_identical": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--nt", type=int, default=64, help="6-hourly steps of the data set")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", choices=["float32", "float64"], default="float32")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--only-steps-kernel", action="store_true", help="run the batch's stage-1 launches alone (profiler runs)")
    ap.add_argument("--batch-composites", action="store_true", help="the batch leg also composites its tracks (compute(batch_composites=sizes))")
    ap.add_argument("--batch-composites-phase", metavar="lifetime:B", help="with --batch-composites: also the phase-aligned ensembles")
    ap.add_argument("--cli", action="store_true", help="the command line: K single-track processes against one --trackfiles process")
    ap.add_argument("--batch-chunk", type=int, metavar="N", help="with --cli: the --trackfiles run prepared on the host against the streamed one "
                    "(--batch-chunk N), --reps runs of each")
    ap.add_argument("--host-cli", metavar="PATH", help="with --cli --batch-chunk: the lorenzcycletoolkit.py the host-prepared leg runs (default: this tree's)")
    a = ap.parse_args()
    if a.batch_chunk is not None and not a.cli:
        ap.error("--batch-chunk goes with --cli")
    if a.batch_composites_phase and not a.batch_composites:
        ap.error("--batch-composites-phase goes with --batch-composites")
    if a.cli:
        print(json.dumps(cli_wall_clock(a.tracks, a.seed) if a.batch_chunk is None else
                         cli_streamed_batch(a.tracks, a.seed, a.batch_chunk, a.reps, a.host_cli)))
        return
    dev = "cuda:0"
    dt = torch.float32 if a.dtype == "float32" else torch.float64
    level = era5_like_levels()
    lat = np.arange(-57.75, -17.5 + 1e-9, 0.25)
    lon = np.arange(-80.25, -19.75 + 1e-9, 0.25)
    rng = np.random.default_rng(a.seed)
    f = synthetic_cube(a.nt, level, lat, lon, device=dev, dtype=dt, seed=a.seed)
    host = [f[k].cpu().numpy() for k in ("tair", "u", "v", "omega", "geopt")]
    del f
    torch.cuda.empty_cache()
    time_s = np.arange(a.nt) * 21600.0
    tracks = _tracks(a.tracks, a.steps, a.nt, lat, lon, rng)
    eng = LECEngine(lat, lon, level, device=dev)
    esz = np.dtype(a.dtype).itemsize
    nl = level.size

    # ---- (a) batch: one upload, one stage-1 + stage-2 call per group
    groups = {}
    for k, (u, bx) in enumerate(tracks):
        groups.setdefault((max(b[3] - b[2] + 1 for b in bx), max(b[1] - b[0] + 1 for b in bx)), []).append(k)
    prepared = []
    for (nyb, _), members in groups.items():
        boxes = [b for k in members for b in tracks[k][1]]
        st = np.concatenate([np.stack([tracks[k][0], np.r_[tracks[k][0][0], tracks[k][0][:-1]], np.r_[tracks[k][0][1:], tracks[k][0][-1]]], 1)
                             for k in members]).astype(np.int32)
        tc = np.concatenate([tables.time_coefs(time_s[tracks[k][0]] - time_s[tracks[k][0][0]]) for k in members])
        extra = {}
        if a.batch_composites:
            extra["batch_composites"] = [len(tracks[k][0]) for k in members]
        if a.batch_composites_phase:
            from lorenzcycletoolkit_amd import batch
            kind, n_bin = batch.parse_phase_clock(a.batch_composites_phase)
            if kind != "lifetime":
                ap.error("--batch-composites-phase: lifetime:B here (a peak needs the tracks' 850-hPa diagnostics)")
            extra["batch_composite_phases"] = np.stack([batch.lifetime_ranges(len(tracks[k][0]), n_bin) for k in members])
        prepared.append((members, eng.prepare_boxes(boxes, nyb_min=nyb), torch.as_tensor(st).to(dev), torch.as_tensor(tc).to(dev), extra))

    def batch_pass(timing=None):
        cubes = [torch.as_tensor(h).to(dev) for h in host]
        outs = {}
        for members, pb, st, tc, extra in prepared:
            if a.only_steps_kernel:
                eng.rowstats(*cubes, pb, steps=st, tcoef=tc, timing=timing)
                continue
            res = eng.compute(*cubes, pb, steps=st, tcoef=tc, per_step_boxes=True, drop_any_time=False, timing=timing, **extra)
            o = 0
            for k in members:
                outs[k] = res.packed[o: o + len(tracks[k][0])]
                o += len(tracks[k][0])
        return outs

    # ---- (b) loop: one single-track resident computation per track (frameworks.BoxData._compute_resident_packed)
    def loop_pass():
        outs = {}
        for k, (u, bx) in enumerate(tracks):
            nyb, nxb = max(b[3] - b[2] + 1 for b in bx), max(b[1] - b[0] + 1 for b in bx)
            src = lambda shift: u[np.clip(np.arange(len(u)) + shift, 0, len(u) - 1)]       # (the step itself at the track's ends)
            pack = lambda arr, shift=0: torch.as_tensor(pack_host(arr, bx, src(shift), nyb, nxb)).to(dev)
            fl = [pack(h) for h in host]
            tm, tp = pack(host[0], -1), pack(host[0], +1)
            tcoef = eng.time_coefs_device(time_s[u] - time_s[u[0]])
            pb = eng.prepare_boxes(bx, nyb_min=nyb, packed=True)
            kw = eng.packed_dtdt(tm, fl[0], tp, tcoef)
            outs[k] = eng.compute(*fl, pb, per_step_boxes=True, drop_any_time=False, **kw).packed
        return outs

    def wall(fn, *args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    out = {"workload": f"synthetic {a.dtype} {nl} levels x {lat.size} x {lon.size} 0.25-degree union crop, {a.nt} six-hourly steps, "
                       f"{a.tracks} tracks of {a.steps} steps, 15 x 15 degree boxes", "groups": len(groups),
           "boxes": int(sum(len(t[0]) for t in tracks))}
    if a.only_steps_kernel:
        for _ in range(a.reps):
            batch_pass()
        torch.cuda.synchronize()
        out["only_steps_kernel"] = True
        print(json.dumps(out))
        return
    batch_pass(); loop_pass()            # warm-up (library load, allocator, box tables)
    bw, lw, kms = [], [], []
    for _ in range(a.reps):
        tm_ = []
        ms, ob = wall(batch_pass, tm_)
        bw.append(ms)
        kms.append(sum(x.elapsed_time(y) for x, y in tm_))
        ms, ol = wall(loop_pass)
        lw.append(ms)
    same_ab = all(torch.equal(torch.nan_to_num(ob[k], nan=7.0), torch.nan_to_num(ol[k], nan=7.0)) for k in range(a.tracks))
    out["batch_ms"] = {"median": float(np.median(bw)), "min": float(np.min(bw)), "all": [round(x, 2) for x in bw],
                       "what": "wall clock: upload of the union cubes + stage 1 + stage 2 per group, synchronized"}
    out["loop_ms"] = {"median": float(np.median(lw)), "min": float(np.min(lw)), "all": [round(x, 2) for x in lw],
                      "what": "wall clock: per track host slice of every box + upload of the box-packed series + dT/dt + stage 1 + stage 2"}
    out["speedup_median"] = out["loop_ms"]["median"] / out["batch_ms"]["median"]
    out["batch_composites"], out["batch_composites_phase"] = bool(a.batch_composites), a.batch_composites_phase
    if a.batch_composites_phase:
        out["phase_kernels_ms"] = _phase_kernel_times(eng, prepared[0], dev, max(a.reps, 5) * 4)
    out["bits_equal_batch_vs_loop"] = bool(same_ab)
    # share of the roofline of the step-table stage-1 launches, counted as bench.py counts the cube layout (the box is read: 5 fields)
    kbytes = 5 * nl * 61 * 61 * esz * out["boxes"]
    out["steps_kernel_ms_median"] = float(np.median(kms))
    out["steps_kernel_roofline_frac"] = kbytes / (np.median(kms) * 1e-3) / 1e9 / HBM_PEAK_GBS

    # ---- (c) one track: t +- 1 addressing against the identity table, same records
    u, bx = tracks[0]
    n = len(u)
    cubes = [torch.as_tensor(np.ascontiguousarray(h[u[0]: u[0] + n])).to(dev) for h in host]
    ts = time_s[u] - time_s[u[0]]
    ident = torch.as_tensor(np.stack([np.arange(n), np.r_[0, np.arange(n - 1)], np.r_[np.arange(1, n), n - 1]], 1).astype(np.int32)).to(dev)
    tc = eng.time_coefs_device(ts)
    r_pm = eng.rowstats(*cubes, bx, time_s=ts, per_step_boxes=True, tuning={"kernel": "box_tile"})
    r_st = eng.rowstats(*cubes, bx, steps=ident, tcoef=tc)
    torch.cuda.synchronize()
    same_c = bool(((r_pm[..., :28] == r_st[..., :28]) | (torch.isnan(r_pm[..., :28]) & torch.isnan(r_st[..., :28]))).all())
    t_pm, t_st = [], []
    for _ in range(max(a.reps, 5) * 4):            # interleaved, so that drift hits both alike
        e = []
        eng.rowstats(*cubes, bx, time_s=ts, per_step_boxes=True, tuning={"kernel": "box_tile"}, timing=e)
        eng.rowstats(*cubes, bx, steps=ident, tcoef=tc, timing=e)
        torch.cuda.synchronize()
        t_pm.append(e[0][0].elapsed_time(e[0][1]))
        t_st.append(e[1][0].elapsed_time(e[1][1]))
    out["one_track"] = {"steps": n, "bits_equal": same_c, "tpm1_kernel_ms_median": float(np.median(t_pm)), "steps_kernel_ms_median": float(np.median(t_st)),
                        "tpm1_kernel_ms_iqr": [float(np.percentile(t_pm, 25)), float(np.percentile(t_pm, 75))],
                        "steps_kernel_ms_iqr": [float(np.percentile(t_st, 25)), float(np.percentile(t_st, 75))]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
