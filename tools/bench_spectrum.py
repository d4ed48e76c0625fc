#!/usr/bin/env python3
"""What the zonal-wavenumber spectra of a ring cost (-f --periodic --wavenumbers N): ``lec_rowspec_ring`` next to the ring pass
``lec_rowstats_ring`` on the same cubes -- a global 37 x 721 x 1440 fp64 grid, box +-89.75 degrees over all longitudes -- and
``LECEngine.compute(..., wavenumbers=N)`` next to the same ``compute`` without it, for N = 8, 20 and 64.

    python tools/bench_spectrum.py [--steps 2] [--rounds 3] [--repeat 5] [--n 8 20 64] [--generation] [--fused] [--budget] [--other NAME=PATH ...] [--out FILE]

The calls are timed with HIP events around the call (median of ``--repeat`` after a warm-up) and ALTERNATE within a round; ``--rounds``
rounds.  Reported per N: the spectral pass's time, its ratio to the ring pass, and the fp64 rate it achieves on the operations the
projection needs -- 8 FMAs per (row, column, wavenumber): the four fields on cos and sin -- counted from the shapes; a rate, with the
vector fp64 peak of the part (78.6 TFLOP/s) beside it.  ``--other NAME=PATH``: a liblec_hip.so built with another form of the kernel,
loaded beside this one; its ``lec_rowspec_ring`` is timed in the same rounds and its records are compared with this library's (largest
difference relative to the slot's scale).  ``--generation``: ``lec_rowspec_q_ring`` (the shares of [Q'T'], for Ge(n)) is timed in the same
rounds, of this library and of every ``--other`` one, as ``specq_N<n>``: its ratio to ``lec_rowspec_ring`` at the same N is the yardstick
(half the FMAs per twiddle -- 4 per (row, column, wavenumber) -- and 2.5 times the rows loaded), and ``compute`` with
``spectrum_generation=True`` next to ``compute`` with the wavenumbers alone.  ``--fused``: ``compute(..., spectrum_fused=True)`` (stage 2 of
the spectra by ``lec_level_spec_ring``, no assembled records) in the same rounds next to the assembled form: both medians, what the fused
form saves per step, the spread of each between the rounds (largest minus smallest), and the bytes of the chunk's spectral records next
to the bytes of the assembled records the other form would hold at the same chunk size.  ``--budget``: ``lec_rowspec_b_ring`` (the shares
of the four triple products behind BAe(n) and BKe(n)) as ``specb_N<n>``, with ``lec_rowspec_nl_ring`` (``specnl_N<n>``) and
``lec_rowspec_q_ring`` (``specq_N<n>``) timed in the same rounds beside it: ms per step, its ratio to either, and the part of the vector
fp64 FMA rate (half the peak: 39.3 T FMA/s) that its 18 FMAs per (wall row, column, n) and 12 per (interior row, column, n) amount to --
a count from the shapes; of every ``--other`` library that exports the call too (another trip length), with the largest difference of
its records; and ``compute`` with ``spectrum_budget=True`` next to ``compute`` with the wavenumbers alone.  One JSON line; ``--out`` writes it to a file."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_VECTOR_PEAK_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--grid", type=int, nargs=3, default=[37, 721, 1440], metavar=("NL", "NY", "NX"))
    ap.add_argument("--n", type=int, nargs="+", default=[8, 20, 64])
    ap.add_argument("--other", nargs="*", default=[], metavar="NAME=PATH")
    ap.add_argument("--generation", action="store_true", help="also time lec_rowspec_q_ring (the shares of [Q'T'])")
    ap.add_argument("--fused", action="store_true", help="also time compute(..., spectrum_fused=True) next to the assembled form")
    ap.add_argument("--budget", action="store_true", help="also time lec_rowspec_b_ring beside lec_rowspec_nl_ring and lec_rowspec_q_ring")
    ap.add_argument("--no-compute", action="store_true", help="time the passes only, not the whole compute calls")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from lorenzcycletoolkit_amd import _lib, tables
    from lorenzcycletoolkit_amd.engine import LECEngine
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectrum.py needs a GPU: a time is measured on the device or not at all")
    lib = _lib.load()
    dev = torch.device("cuda:0")
    nl, ny, nx = a.grid
    nt = a.steps
    lat = np.linspace(-90.0, 90.0, ny)
    lon = -180.0 + 360.0 / nx * np.arange(nx)
    level = np.linspace(100.0, 100000.0, nl)
    eng = LECEngine(lat, lon, level, device=dev)
    box = (0, nx - 1, 1, ny - 2)                         # +-89.75 degrees on the 0.25-degree grid: the polar rows stay out
    ring = eng.prepare_boxes([box], ring=True)
    g = torch.Generator(device=dev).manual_seed(1)
    shape = (nt, nl, ny, nx)
    T = 250.0 + 10.0 * torch.randn(shape, dtype=torch.float64, device=dev, generator=g)
    U, V, W, P = (torch.randn(shape, dtype=torch.float64, device=dev, generator=g) for _ in range(4))
    time_s = 21600.0 * np.arange(nt)
    nyb = ny - 2
    rows_per_step = nl * nyb

    others = []
    for item in a.other:
        name, path = item.split("=", 1)
        o = C.CDLL(path)
        o.lec_rowspec_ring.restype, o.lec_rowspec_ring.argtypes = C.c_int, [C.POINTER(_lib.RowspecArgs)]
        if a.budget and hasattr(o, "lec_rowspec_b_ring"):
            o.lec_rowspec_b_ring.restype, o.lec_rowspec_b_ring.argtypes = C.c_int, [C.POINTER(_lib.RowspecBArgs)]
        if a.generation:
            o.lec_rowspec_q_ring.restype, o.lec_rowspec_q_ring.argtypes = C.c_int, [C.POINTER(_lib.RowspecQArgs)]
        others.append((name, o))
    twid = eng._up(tables.twiddle_table(nx))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def spec_call(which, n, out):
        sa = _lib.RowspecArgs(tair_d=ptr(T), u_d=ptr(U), v_d=ptr(V), omega_d=ptr(W), dtype=_lib.LEC_F64, nt=nt, nl=nl, ny=ny, nx=nx, t_begin=0,
                              t_count=nt, js=1, jn=ny - 2, n_wave=n, twid_d=ptr(twid), spec_d=ptr(out), stream=stream)
        if which.lec_rowspec_ring(C.byref(sa)):
            raise RuntimeError(f"lec_rowspec_ring failed: {lib.lec_last_error()}")

    tcoef = eng.time_coefs_device(time_s) if nt > 1 else None

    def specq_call(which, n, out):
        qa = _lib.RowspecQArgs(tair_d=ptr(T), u_d=ptr(U), v_d=ptr(V), omega_d=ptr(W), dtype=_lib.LEC_F64, nt=nt, nl=nl, ny=ny, nx=nx, t_begin=0,
                               t_count=nt, js=1, jn=ny - 2, n_wave=n, twid_d=ptr(twid), lattab_d=ptr(ring.dev["lattab"]), levtab_d=ptr(eng._levtab),
                               tcoef_d=ptr(tcoef), inv_hdeg=float(ring.bt.boxtab[0, 2]), qspec_d=ptr(out), stream=stream)
        if which.lec_rowspec_q_ring(C.byref(qa)):
            raise RuntimeError(f"lec_rowspec_q_ring failed: {lib.lec_last_error()}")

    def specb_call(which, n, out):
        ba = _lib.RowspecBArgs(tair_d=ptr(T), u_d=ptr(U), v_d=ptr(V), omega_d=ptr(W), dtype=_lib.LEC_F64, nt=nt, nl=nl, ny=ny, nx=nx, t_begin=0,
                               t_count=nt, js=1, jn=ny - 2, n_wave=n, rows_d=ptr(rows), twid_d=ptr(twid), bspec_d=ptr(out), stream=stream)
        if which.lec_rowspec_b_ring(C.byref(ba)):
            raise RuntimeError(f"lec_rowspec_b_ring failed: {lib.lec_last_error()}")

    def specnl_call(n, out, tot):
        na = _lib.RowspecNlArgs(tair_d=ptr(T), u_d=ptr(U), v_d=ptr(V), omega_d=ptr(W), dtype=_lib.LEC_F64, nt=nt, nl=nl, ny=ny, nx=nx, t_begin=0,
                                t_count=nt, js=1, jn=ny - 2, n_wave=n, rows_d=ptr(rows), twid_d=ptr(twid), lattab_d=ptr(lat5), ptab_d=ptr(ptab),
                                inv_hdeg=float(ring.bt.boxtab[0, 2]), nlspec_d=ptr(out), nltot_d=ptr(tot), stream=stream)
        if lib.lec_rowspec_nl_ring(C.byref(na)):
            raise RuntimeError(f"lec_rowspec_nl_ring failed: {lib.lec_last_error()}")

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

    out = {"grid": [nl, ny, nx], "steps": nt, "dtype": "float64", "box_rows": nyb, "rounds": a.rounds, "repeat": a.repeat,
           "csrc_sha": _lib.source_digest(), "fp64_vector_peak_TFLOPs": FP64_VECTOR_PEAK_TFLOPS, "n": a.n}
    rows = torch.empty((nt, nl, nyb, _lib.LEC_NSTAT), dtype=torch.float64, device=dev)
    calls = [("ring_pass", lambda: eng.rowstats(T, U, V, W, P, ring, time_s=time_s, rows_out=rows))]
    bufs, qbufs, bbufs = {}, {}, {}
    with_q = a.generation or (a.budget and nt > 1)
    if a.budget:
        lat5 = eng._up(tables.nl_lat_table(ring.bt.lattab[0], lat[1:ny - 1]))
        ptab = eng._up(tables.pressure_coefs(level))
        nltot = torch.empty((nt, nl, nyb, 8), dtype=torch.float64, device=dev)
    for n in a.n:
        bufs[n] = torch.empty((nt, nl, nyb, n, 8), dtype=torch.float64, device=dev)
        calls.append((f"spec_N{n}", lambda n=n: spec_call(lib, n, bufs[n])))
        for name, o in others:
            calls.append((f"spec_N{n}_{name}", lambda n=n, o=o: spec_call(o, n, bufs[n])))
        if a.budget:
            bbufs[n] = torch.empty((nt, nl, nyb, n, 4), dtype=torch.float64, device=dev)
            calls.append((f"specb_N{n}", lambda n=n: specb_call(lib, n, bbufs[n])))
            for name, o in others:
                if hasattr(o, "lec_rowspec_b_ring"):
                    calls.append((f"specb_N{n}_{name}", lambda n=n, o=o: specb_call(o, n, bbufs[n])))
            calls.append((f"specnl_N{n}", lambda n=n: specnl_call(n, bufs[n], nltot)))
        if with_q:
            qbufs[n] = torch.empty((nt, nl, nyb, n), dtype=torch.float64, device=dev)
            calls.append((f"specq_N{n}", lambda n=n: specq_call(lib, n, qbufs[n])))
            for name, o in others if a.generation else []:
                calls.append((f"specq_N{n}_{name}", lambda n=n, o=o: specq_call(o, n, qbufs[n])))
    if not a.no_compute:
        calls.append(("compute", lambda: eng.compute(T, U, V, W, P, ring, time_s=time_s)))
        for n in a.n:
            calls.append((f"compute_N{n}", lambda n=n: eng.compute(T, U, V, W, P, ring, time_s=time_s, wavenumbers=n)))
            if a.budget:
                calls.append((f"compute_N{n}_budget", lambda n=n: eng.compute(T, U, V, W, P, ring, time_s=time_s, wavenumbers=n, spectrum_budget=True)))
            if a.fused:
                calls.append((f"compute_N{n}_fused", lambda n=n: eng.compute(T, U, V, W, P, ring, time_s=time_s, wavenumbers=n, spectrum_fused=True)))
            if a.generation:
                calls.append((f"compute_N{n}_ge", lambda n=n: eng.compute(T, U, V, W, P, ring, time_s=time_s, wavenumbers=n, spectrum_generation=True)))
                if a.fused:
                    calls.append((f"compute_N{n}_ge_fused", lambda n=n: eng.compute(T, U, V, W, P, ring, time_s=time_s, wavenumbers=n,
                                                                                    spectrum_generation=True, spectrum_fused=True)))
    for _ in range(a.rounds):
        for name, fn in calls:
            out.setdefault(f"{name}_ms", []).append(round(timed(fn), 4))
    med = lambda k: float(np.median(out[f"{k}_ms"]))
    out["ring_pass_ms_per_step"] = round(med("ring_pass") / nt, 4)
    for n in a.n:
        flop = 2.0 * 8.0 * nt * rows_per_step * nx * n
        for name in [""] + ["_" + x for x, _ in others]:
            k = f"spec_N{n}{name}"
            out[f"{k}_ms_per_step"] = round(med(k) / nt, 4)
            out[f"{k}_over_ring_pass"] = round(med(k) / med("ring_pass"), 3)
            out[f"{k}_fp64_TFLOPs"] = round(flop / (med(k) * 1e-3) / 1e12, 3)
            if a.generation or (with_q and not name):
                k = f"specq_N{n}{name}"
                out[f"{k}_ms_per_step"] = round(med(k) / nt, 4)
                out[f"{k}_over_ring_pass"] = round(med(k) / med("ring_pass"), 3)
                out[f"{k}_over_spec_N{n}"] = round(med(k) / med(f"spec_N{n}"), 3)
                out[f"{k}_fp64_TFLOPs"] = round(0.5 * flop / (med(k) * 1e-3) / 1e12, 3)
        if a.budget:
            fma = float(nt) * nl * nx * n * (18.0 * 2 + 12.0 * (nyb - 2))
            bnames = [""] + ["_" + x for x, o in others if hasattr(o, "lec_rowspec_b_ring")]
            for name in bnames:
                k = f"specb_N{n}{name}"
                out[f"{k}_ms_per_step"] = round(med(k) / nt, 4)
                out[f"{k}_fraction_of_fp64_fma_rate"] = round(fma / (med(k) * 1e-3) / (FP64_VECTOR_PEAK_TFLOPS * 1e12 / 2), 4)
            out[f"specnl_N{n}_ms_per_step"] = round(med(f"specnl_N{n}") / nt, 4)
            out[f"specb_N{n}_over_specnl_N{n}"] = round(med(f"specb_N{n}") / med(f"specnl_N{n}"), 3)
            if with_q:
                out[f"specq_N{n}_ms_per_step"] = round(med(f"specq_N{n}") / nt, 4)
                out[f"specb_N{n}_over_specq_N{n}"] = round(med(f"specb_N{n}") / med(f"specq_N{n}"), 3)
            if not a.no_compute:
                out[f"compute_N{n}_budget_ms_per_step"] = round(med(f"compute_N{n}_budget") / nt, 4)
                out[f"compute_N{n}_budget_over_compute_N{n}"] = round(med(f"compute_N{n}_budget") / med(f"compute_N{n}"), 3)
        if a.generation and not a.no_compute:
            out[f"compute_N{n}_ge_over_compute_N{n}"] = round(med(f"compute_N{n}_ge") / med(f"compute_N{n}"), 3)
            out[f"compute_N{n}_ge_ms_per_step"] = round(med(f"compute_N{n}_ge") / nt, 4)
        if a.fused and not a.no_compute:
            spread = lambda k: round(max(out[f"{k}_ms"]) - min(out[f"{k}_ms"]), 4)
            for k in [f"compute_N{n}"] + ([f"compute_N{n}_ge"] if a.generation else []):
                out[f"{k}_fused_ms_per_step"] = round(med(k + "_fused") / nt, 4)
                out[f"{k}_fused_saves_ms_per_step"] = round((med(k) - med(k + "_fused")) / nt, 4)
                out[f"{k}_spread_ms"], out[f"{k}_fused_spread_ms"] = spread(k), spread(k + "_fused")
            tc = eng.spectrum_chunk_steps(nt, nl, nyb, n)
            out[f"N{n}_fused_chunk_steps"] = tc
            out[f"N{n}_spectrum_buffer_bytes"] = tc * rows_per_step * n * (64 + (8 if a.generation else 0))
            out[f"N{n}_assembled_bytes_at_that_chunk"] = tc * rows_per_step * n * _lib.LEC_NSTAT * 8
        if not a.no_compute:
            out[f"compute_N{n}_over_compute"] = round(med(f"compute_N{n}") / med("compute"), 3)
            out[f"compute_N{n}_ms_per_step"] = round(med(f"compute_N{n}") / nt, 4)
    if not a.no_compute:
        out["compute_ms_per_step"] = round(med("compute") / nt, 4)
    # other forms give the same records (reordered fp64 sums: the last bits)
    for n in a.n:
        if not others:
            break
        mine = torch.empty_like(bufs[n])
        spec_call(lib, n, mine)
        scale = mine.abs().amax(dim=(0, 1, 2, 3))
        for name, o in others:
            spec_call(o, n, bufs[n])
            torch.cuda.synchronize()
            out[f"spec_N{n}_{name}_max_diff_of_scale"] = float(((bufs[n] - mine).abs().amax(dim=(0, 1, 2, 3)) / scale).max())
        if a.budget:
            mine = torch.empty_like(bbufs[n])
            specb_call(lib, n, mine)
            for name, o in others:
                if hasattr(o, "lec_rowspec_b_ring"):
                    specb_call(o, n, bbufs[n])
                    torch.cuda.synchronize()
                    out[f"specb_N{n}_{name}_max_diff_of_scale"] = float((bbufs[n] - mine).abs().max() / mine.abs().max())
        if a.generation:
            mine = torch.empty_like(qbufs[n])
            specq_call(lib, n, mine)
            for name, o in others:
                specq_call(o, n, qbufs[n])
                torch.cuda.synchronize()
                out[f"specq_N{n}_{name}_max_diff_of_scale"] = float((qbufs[n] - mine).abs().max() / mine.abs().max())
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
