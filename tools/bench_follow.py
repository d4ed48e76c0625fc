#!/usr/bin/env python3
"""What following a system costs: ``lec_follow`` (one workgroup, the steps in sequence) for a long series on a 0.25-degree slice, next
to ``lec_track_diag`` over the very windows it visited (one workgroup per step: the parallel kernel the chain cannot be).  HIP events
around the calls, median of ``--repeat`` after a warm-up; one JSON line.

    python tools/bench_follow.py [--steps 4096] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from lorenzcycletoolkit_amd import _lib, diagnostics as dg, follow as fw
    lib = _lib.load()
    dev = torch.device("cuda:0")
    # a regional 0.25-degree slice (40 x 60 degrees): the search domain of a case study; the chain's cost does not depend on its size
    lat, lon = -60.0 + 0.25 * np.arange(161), -90.0 + 0.25 * np.arange(241)
    nt, ny, nx = a.steps, lat.size, lon.size
    g = torch.Generator(device=dev).manual_seed(1)
    u, v, h = (torch.randn((nt, ny, nx), dtype=torch.float64, device=dev, generator=g) for _ in range(3))
    xc, yc, cv = (torch.as_tensor(t).to(dev) for t in dg.vorticity_tables(lat, lon, "metpy_no_crs"))
    bounds = fw.admissible(lat, lon, *fw.DEFAULT_BOX)
    sj, si = fw.window_steps(lat, lon, fw.DEFAULT_SEARCH)
    js, is_ = fw.start_index(lat, lon, (-40.0, -60.0), bounds)
    pos = torch.empty((nt, 2), dtype=torch.int32, device=dev)
    val = torch.empty((nt,), dtype=torch.float64, device=dev)
    status = torch.empty((nt,), dtype=torch.int32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def timed(call):
        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), [round(x, 4) for x in ms]

    out = {"steps": nt, "slice": [ny, nx], "window": [2 * sj + 1, 2 * si + 1], "csrc_sha": _lib.source_digest()}
    for r in (0, 2):
        fa = _lib.FollowArgs(u_d=ptr(u), v_d=ptr(v), hgt_d=ptr(h), nt=nt, ny=ny, nx=nx, field=_lib.FOLLOW_ZETA, xcoef_d=ptr(xc), ycoef_d=ptr(yc),
                             curv_d=ptr(cv), sense=_lib.FOLLOW_MIN, smooth_r=r, sj=sj, si=si, jlo=bounds[0], jhi=bounds[1], ilo=bounds[2],
                             ihi=bounds[3], j_start=js, i_start=is_, pos_d=ptr(pos), val_d=ptr(val), status_d=ptr(status), stream=stream)
        med, all_ms = timed(lambda: _lib.check(lib.lec_follow(C.byref(fa)), "lec_follow"))
        out[f"lec_follow_r{r}_ms"], out[f"lec_follow_r{r}_all_ms"] = round(med, 4), all_ms
        out[f"lec_follow_r{r}_us_per_step"] = round(1e3 * med / nt, 3)
        if r == 0:
            p = pos.cpu().numpy()
    # lec_track_diag over the windows the r = 0 chain visited
    centre = np.vstack([[js, is_], p[:-1]])
    box = np.stack([np.maximum(bounds[2], centre[:, 1] - si), np.minimum(bounds[3], centre[:, 1] + si),
                    np.maximum(bounds[0], centre[:, 0] - sj), np.minimum(bounds[1], centre[:, 0] + sj), centre[:, 0], centre[:, 1]], axis=1).astype(np.int32)
    box_d = torch.as_tensor(np.ascontiguousarray(box)).to(dev)
    dval = torch.empty((nt, 5), dtype=torch.float64, device=dev)
    dpos = torch.empty((nt, 8), dtype=torch.int32, device=dev)
    da = _lib.DiagArgs(u_d=ptr(u), v_d=ptr(v), hgt_d=ptr(h), nt=nt, ny=ny, nx=nx, reserved0=0, box_d=ptr(box_d), xcoef_d=ptr(xc), ycoef_d=ptr(yc),
                       curv_d=ptr(cv), val_d=ptr(dval), pos_d=ptr(dpos), stream=stream)
    med, all_ms = timed(lambda: _lib.check(lib.lec_track_diag(C.byref(da)), "lec_track_diag"))
    out["lec_track_diag_same_windows_ms"], out["lec_track_diag_all_ms"] = round(med, 4), all_ms
    # the r = 2 run was last: repeat r = 0 once more for the comparison of the two kernels' extrema
    fa.smooth_r = 0
    _lib.check(lib.lec_follow(C.byref(fa)), "lec_follow")
    torch.cuda.synchronize()
    out["same_extrema_as_lec_track_diag"] = bool(torch.equal(dval[:, 0], val) and torch.equal(dpos[:, 0:2], pos))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
