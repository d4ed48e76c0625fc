#!/usr/bin/env python3
"""What following a system costs: ``lec_follow`` (one workgroup, the steps in sequence) for a long series on a 0.25-degree slice, next
to ``lec_track_diag`` over the very windows it visited (one workgroup per step: the parallel kernel the chain cannot be).  HIP events
around the calls, median of ``--repeat`` after a warm-up; one JSON line.

    python tools/bench_follow.py [--steps 4096] [--out FILE]

``--systems K [K ...]``: several systems in one run instead.  Same series, same window; per K one ``lec_follow_many`` launch of K chains
(starts spread over the admissible centres) against K back-to-back ``lec_follow`` launches -- of the library ``--parent PATH`` names (a
liblec_hip.so built from the parent commit, loaded beside this one; without it: this library's own ``lec_follow``) --, the chains
compared bit for bit; ``lec_follow`` itself (one chain through the old entry) in both libraries, alternating; and ``lec_follow_seeds`` on
one slice.  The values go under the key ``systems`` of ``--out`` (whatever else the file holds is kept).

``--lifecycle``: the two calls of ``-c --choose-lifecycle`` instead.  Same series; ONE ``lec_follow_seeds_series`` call over all steps
against ``steps`` back-to-back ``lec_follow_seeds`` calls of the library ``--parent PATH`` names (without it: this library's own), the
seeds compared bit for bit; and ONE ``lec_follow_spans`` launch of ``--chains`` chains with mixed lifetimes (births spread over the
series, the end threshold at the 0.9 quantile of the values the chains meet, patience 2) against ``lec_follow_many`` walking the same starts
through the whole series.  The values go under the key ``lifecycle`` of ``--out``.

``--chunked``: the resumed chains of ``-c --choose-chunk`` instead.  Same series, ``--lifecycle``'s table of ``--chains`` chains and its
end threshold.  (a) ONE ``lec_follow_spans`` launch against the ``lec_follow_spans_chunk`` calls over chunks of 64 and of 512 steps with
the state carried (the timed call zeroes the state and makes every chunk's call; the outputs are compared bit for bit with the one
launch's in a pass of their own).  (b) with ``--parent PATH``: ``lec_follow_spans`` and ``lec_follow_many`` of the parent's library and
of this one, alternating, two rounds -- what the chains' shared device function cost the existing calls when it gained the resumed
variant.  The values go under the key ``chunked`` of ``--out``.

``--ring``: the two ring calls of ``-c --choose-periodic`` instead.  Same series with its 241 columns relabelled as a full ring of
longitudes (window 41 x 41), ``--chains`` chains from ``--lifecycle``'s table, k_max 8.  ``lec_follow_spans_chunk_ring`` (one chunk: the
whole series) and ``lec_follow_seeds_series_ring`` of this library against ``lec_follow_spans_chunk`` and ``lec_follow_seeds_series`` of
the library ``--parent PATH`` names (without it: this library's own) on the same arrays with the same bounds (every column a centre)
and the open axis' tables, alternating, two rounds.  The non-ring chain cuts its window at columns 0 and nx - 1 where the ring's wraps,
so the two do not walk the same chains: the figures compare the cost per call, not bits.  The values go under the key ``ring`` of ``--out``.
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
    ap.add_argument("--systems", type=int, nargs="+", metavar="K", default=None)
    ap.add_argument("--parent", default=None, metavar="PATH")
    ap.add_argument("--lifecycle", action="store_true")
    ap.add_argument("--chunked", action="store_true")
    ap.add_argument("--ring", action="store_true")
    ap.add_argument("--chains", type=int, default=64, help="with --lifecycle / --chunked: chains of the lec_follow_spans launch")
    a = ap.parse_args()
    import torch
    from lorenzcycletoolkit_amd import _lib, diagnostics as dg, follow as fw
    lib = _lib.load()
    dev = torch.device("cuda:0")
    # a regional 0.25-degree slice (40 x 60 degrees): the search domain of a case study; the chain's cost does not depend on its size
    lat, lon = -60.0 + 0.25 * np.arange(161), -90.0 + 0.25 * np.arange(241)
    if a.ring:
        lon = -180.0 + (360.0 / 241) * np.arange(241)
    nt, ny, nx = a.steps, lat.size, lon.size
    g = torch.Generator(device=dev).manual_seed(1)
    u, v, h = (torch.randn((nt, ny, nx), dtype=torch.float64, device=dev, generator=g) for _ in range(3))
    xc, yc, cv = (torch.as_tensor(t).to(dev) for t in dg.vorticity_tables(lat, lon, "metpy_no_crs"))
    bounds = fw.admissible(lat, lon, *fw.DEFAULT_BOX)
    sj, si = fw.window_steps(lat, lon, fw.DEFAULT_SEARCH)
    if a.ring:
        sj, si = 20, 20                                  # the window of the other modes, 41 x 41 points, on the relabelled axis
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
    if a.ring:
        rt = [torch.as_tensor(t).to(dev) for t in dg.vorticity_tables(lat, lon, "metpy_no_crs", periodic=True)]
        return ring(a, lib, out, dict(u=u, v=v, h=h, xc=xc, yc=yc, cv=cv, ring_tables=rt, bounds=(bounds[0], bounds[1], 0, nx - 1), sj=sj, si=si,
                                     nt=nt, ny=ny, nx=nx, dev=dev, stream=stream), timed)
    if a.chunked:
        return chunked(a, lib, out, dict(u=u, v=v, h=h, xc=xc, yc=yc, cv=cv, bounds=bounds, sj=sj, si=si, nt=nt, ny=ny, nx=nx, dev=dev, stream=stream), timed)
    if a.lifecycle:
        return lifecycle(a, lib, out, dict(u=u, v=v, h=h, xc=xc, yc=yc, cv=cv, bounds=bounds, sj=sj, si=si,
                                          sep=fw.separation_steps(lat, lon, fw.DEFAULT_BOX[0] / 2, fw.DEFAULT_BOX[1] / 2), nt=nt, ny=ny, nx=nx, dev=dev, stream=stream), timed)
    if a.systems:
        return systems(a, lib, out, dict(u=u, v=v, h=h, xc=xc, yc=yc, cv=cv, bounds=bounds, sj=sj, si=si, start=(js, is_),
                                        sep=fw.separation_steps(lat, lon, fw.DEFAULT_BOX[0] / 2, fw.DEFAULT_BOX[1] / 2), nt=nt, ny=ny, nx=nx, dev=dev, stream=stream), timed)
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


def systems(a, lib, out, w, timed):
    import torch
    from lorenzcycletoolkit_amd import _lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    nt, dev, bounds = w["nt"], w["dev"], w["bounds"]
    old = lib
    if a.parent:
        old = C.CDLL(a.parent)
        old.lec_follow.restype, old.lec_follow.argtypes = C.c_int, [C.POINTER(_lib.FollowArgs)]
    common = dict(u_d=ptr(w["u"]), v_d=ptr(w["v"]), hgt_d=ptr(w["h"]), ny=w["ny"], nx=w["nx"], field=_lib.FOLLOW_ZETA, xcoef_d=ptr(w["xc"]),
                  ycoef_d=ptr(w["yc"]), curv_d=ptr(w["cv"]), sense=_lib.FOLLOW_MIN, smooth_r=0, jlo=bounds[0], jhi=bounds[1], ilo=bounds[2],
                  ihi=bounds[3], stream=w["stream"])
    kmax = max(a.systems)
    rng = np.random.default_rng(2)
    starts = np.c_[rng.integers(bounds[0], bounds[1] + 1, kmax), rng.integers(bounds[2], bounds[3] + 1, kmax)].astype(np.int32)
    starts[0] = w["start"]                               # chain 0: the start of the tool's one-chain figures
    start_d = torch.as_tensor(starts).to(dev)
    pos = torch.empty((kmax, nt, 2), dtype=torch.int32, device=dev)
    val = torch.empty((kmax, nt), dtype=torch.float64, device=dev)
    status = torch.empty((kmax, nt), dtype=torch.int32, device=dev)
    pos1, val1, status1 = torch.empty_like(pos), torch.empty_like(val), torch.empty_like(status)

    def single(which, c):
        fa = _lib.FollowArgs(nt=nt, sj=w["sj"], si=w["si"], j_start=int(starts[c, 0]), i_start=int(starts[c, 1]), pos_d=ptr(pos1[c]),
                             val_d=ptr(val1[c]), status_d=ptr(status1[c]), **common)
        rc = which.lec_follow(C.byref(fa))
        if rc:
            raise RuntimeError(f"lec_follow failed (code {rc})")

    def singles(which, k):
        for c in range(k):
            single(which, c)

    res = {"parent_library": bool(a.parent), "chains": {}}
    # lec_follow itself, one chain through the old entry: the parent's kernel and this one's (the shared device function), alternating
    for rep in range(2):
        for name, which in (("parent", old), ("this", lib)):
            med, all_ms = timed(lambda: single(which, 0))
            res.setdefault(f"lec_follow_{name}_ms", []).append(round(med, 4))
    for k in a.systems:
        ma = _lib.FollowManyArgs(nt=nt, sj=w["sj"], si=w["si"], n_chains=k, reserved0=0, start_d=ptr(start_d), pos_d=ptr(pos), val_d=ptr(val),
                                 status_d=ptr(status), **common)
        med, all_ms = timed(lambda: _lib.check(lib.lec_follow_many(C.byref(ma)), "lec_follow_many"))
        med1, all1 = timed(lambda: singles(old, k))
        same = bool(torch.equal(pos[:k], pos1[:k]) and torch.equal(val[:k].view(torch.int64), val1[:k].view(torch.int64))
                    and torch.equal(status[:k], status1[:k]))
        res["chains"][str(k)] = {"lec_follow_many_ms": round(med, 4), "lec_follow_many_all_ms": all_ms, "lec_follow_back_to_back_ms": round(med1, 4),
                                 "lec_follow_back_to_back_all_ms": all1, "same_bits": same}
    # lec_follow_seeds on the first slice: no better value within half the default box
    ej, ei = w["sep"]
    work = torch.empty((w["ny"], w["nx"]), dtype=torch.float64, device=dev)
    for k in (8, 256):
        spos, sval, sn = torch.empty((k, 2), dtype=torch.int32, device=dev), torch.empty((k,), dtype=torch.float64, device=dev), torch.empty((1,), dtype=torch.int32, device=dev)
        sa = _lib.FollowSeedsArgs(ej=ej, ei=ei, k_max=k, threshold=float("nan"), work_d=ptr(work), seed_pos_d=ptr(spos), seed_val_d=ptr(sval),
                                  n_found_d=ptr(sn), **common)
        med, all_ms = timed(lambda: _lib.check(lib.lec_follow_seeds(C.byref(sa)), "lec_follow_seeds"))
        res[f"lec_follow_seeds_k{k}_ms"], res[f"lec_follow_seeds_k{k}_all_ms"] = round(med, 4), all_ms
        res[f"lec_follow_seeds_k{k}_found"], res["lec_follow_seeds_neighbourhood"] = int(sn.cpu()[0]), [2 * ej + 1, 2 * ei + 1]
    out["systems"] = res
    print(json.dumps(out))
    if a.out:
        kept = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                kept = json.loads(f.read())
        kept["systems"] = dict(res, csrc_sha=out["csrc_sha"])
        with open(a.out, "w") as f:
            f.write(json.dumps(kept) + "\n")


def lifecycle(a, lib, out, w, timed):
    import torch
    from lorenzcycletoolkit_amd import _lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    nt, ny, nx, dev, bounds = w["nt"], w["ny"], w["nx"], w["dev"], w["bounds"]
    old = lib
    if a.parent:
        old = C.CDLL(a.parent)
        old.lec_follow_seeds.restype, old.lec_follow_seeds.argtypes = C.c_int, [C.POINTER(_lib.FollowSeedsArgs)]
    common = dict(ny=ny, nx=nx, field=_lib.FOLLOW_ZETA, xcoef_d=ptr(w["xc"]), ycoef_d=ptr(w["yc"]), curv_d=ptr(w["cv"]), sense=_lib.FOLLOW_MIN,
                  smooth_r=0, jlo=bounds[0], jhi=bounds[1], ilo=bounds[2], ihi=bounds[3], stream=w["stream"])
    series = dict(common, u_d=ptr(w["u"]), v_d=ptr(w["v"]), hgt_d=ptr(w["h"]))
    res = {"parent_library": bool(a.parent)}
    # the seeds of every step: one call, and the parent's one-slice call step by step
    ej, ei = w["sep"]
    k = 8
    work = torch.empty((nt, ny, nx), dtype=torch.float64, device=dev)
    spos, sval, sn = (torch.empty(shape, dtype=dt, device=dev) for shape, dt in (((nt, k, 2), torch.int32), ((nt, k), torch.float64), ((nt,), torch.int32)))
    spos1, sval1, sn1 = torch.empty_like(spos), torch.empty_like(sval), torch.empty_like(sn)
    sa = _lib.FollowSeedsSeriesArgs(nt=nt, ej=ej, ei=ei, k_max=k, reserved0=0, threshold=float("nan"), work_d=ptr(work), seed_pos_d=ptr(spos),
                                    seed_val_d=ptr(sval), n_found_d=ptr(sn), **series)
    one = [_lib.FollowSeedsArgs(u_d=ptr(w["u"][t]), v_d=ptr(w["v"][t]), hgt_d=ptr(w["h"][t]), ej=ej, ei=ei, k_max=k, threshold=float("nan"),
                                work_d=ptr(work), seed_pos_d=ptr(spos1[t]), seed_val_d=ptr(sval1[t]), n_found_d=ptr(sn1[t]), **common) for t in range(nt)]

    def step_by_step():
        for t in range(nt):
            if old.lec_follow_seeds(C.byref(one[t])):
                raise RuntimeError("lec_follow_seeds failed")

    med1, all1 = timed(step_by_step)
    med, all_ms = timed(lambda: _lib.check(lib.lec_follow_seeds_series(C.byref(sa)), "lec_follow_seeds_series"))
    res["seeds"] = {"k": k, "neighbourhood": [2 * ej + 1, 2 * ei + 1], "lec_follow_seeds_series_ms": round(med, 4), "lec_follow_seeds_series_all_ms": all_ms,
                    "lec_follow_seeds_back_to_back_ms": round(med1, 4), "lec_follow_seeds_back_to_back_all_ms": all1,
                    "same_bits": bool(torch.equal(spos, spos1) and torch.equal(sval.view(torch.int64), sval1.view(torch.int64)) and torch.equal(sn, sn1))}
    del work
    # chains with mixed lifetimes: lec_follow_many walks every start through the whole series, lec_follow_spans from its birth to its end
    K = a.chains
    rng = np.random.default_rng(2)
    t0 = np.sort(rng.integers(0, max(1, nt - 1), K))
    t0[0] = 0
    table = np.c_[t0, rng.integers(bounds[0], bounds[1] + 1, K), rng.integers(bounds[2], bounds[3] + 1, K)].astype(np.int32)
    start3, start2 = torch.as_tensor(table).to(dev), torch.as_tensor(np.ascontiguousarray(table[:, 1:])).to(dev)
    pos, val, status = (torch.empty(shape, dtype=dt, device=dev) for shape, dt in (((K, nt, 2), torch.int32), ((K, nt), torch.float64), ((K, nt), torch.int32)))
    span = torch.empty((K, 2), dtype=torch.int32, device=dev)
    chain = dict(series, nt=nt, sj=w["sj"], si=w["si"], n_chains=K, pos_d=ptr(pos), val_d=ptr(val), status_d=ptr(status))
    ma = _lib.FollowManyArgs(reserved0=0, start_d=ptr(start2), **chain)
    med_many, all_many = timed(lambda: _lib.check(lib.lec_follow_many(C.byref(ma)), "lec_follow_many"))
    threshold = float(torch.quantile(val.flatten(), 0.9).cpu())       # nine steps in ten are good: lifetimes from a few steps to hundreds
    pa = _lib.FollowSpansArgs(patience=2, end_threshold=threshold, start_d=ptr(start3), span_d=ptr(span), **chain)
    med, all_ms = timed(lambda: _lib.check(lib.lec_follow_spans(C.byref(pa)), "lec_follow_spans"))
    walked = (status != _lib.FOLLOW_NOT_LIVE).sum(dim=1).cpu().numpy()
    res["chains"] = {"n_chains": K, "end_threshold": threshold, "patience": 2, "lec_follow_spans_ms": round(med, 4), "lec_follow_spans_all_ms": all_ms,
                     "lec_follow_many_whole_series_ms": round(med_many, 4), "lec_follow_many_whole_series_all_ms": all_many,
                     "walked_steps_min_median_max": [int(walked.min()), float(np.median(walked)), int(walked.max())], "walked_steps_total": int(walked.sum())}
    out["lifecycle"] = res
    print(json.dumps(out))
    if a.out:
        kept = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                kept = json.loads(f.read())
        kept["lifecycle"] = dict(res, steps=nt, csrc_sha=out["csrc_sha"])
        with open(a.out, "w") as f:
            f.write(json.dumps(kept) + "\n")


def chunked(a, lib, out, w, timed):
    import torch
    from lorenzcycletoolkit_amd import _lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    nt, ny, nx, dev, bounds = w["nt"], w["ny"], w["nx"], w["dev"], w["bounds"]
    common = dict(ny=ny, nx=nx, field=_lib.FOLLOW_ZETA, xcoef_d=ptr(w["xc"]), ycoef_d=ptr(w["yc"]), curv_d=ptr(w["cv"]), sense=_lib.FOLLOW_MIN,
                  smooth_r=0, jlo=bounds[0], jhi=bounds[1], ilo=bounds[2], ihi=bounds[3], stream=w["stream"], sj=w["sj"], si=w["si"])
    series = dict(common, u_d=ptr(w["u"]), v_d=ptr(w["v"]), hgt_d=ptr(w["h"]), nt=nt)
    # --lifecycle's table: births spread over the series, the end threshold at the 0.9 quantile of the values the chains meet
    K = a.chains
    rng = np.random.default_rng(2)
    t0 = np.sort(rng.integers(0, max(1, nt - 1), K))
    t0[0] = 0
    table = np.c_[t0, rng.integers(bounds[0], bounds[1] + 1, K), rng.integers(bounds[2], bounds[3] + 1, K)].astype(np.int32)
    start3, start2 = torch.as_tensor(table).to(dev), torch.as_tensor(np.ascontiguousarray(table[:, 1:])).to(dev)
    pos, val, status = (torch.empty(shape, dtype=dt, device=dev) for shape, dt in (((K, nt, 2), torch.int32), ((K, nt), torch.float64), ((K, nt), torch.int32)))
    span = torch.empty((K, 2), dtype=torch.int32, device=dev)
    outs = dict(n_chains=K, pos_d=ptr(pos), val_d=ptr(val), status_d=ptr(status))
    ma = _lib.FollowManyArgs(reserved0=0, start_d=ptr(start2), **series, **outs)
    _lib.check(lib.lec_follow_many(C.byref(ma)), "lec_follow_many")
    threshold = float(torch.quantile(val.flatten(), 0.9).cpu())
    pa = _lib.FollowSpansArgs(patience=2, end_threshold=threshold, start_d=ptr(start3), span_d=ptr(span), **series, **outs)
    res = {"parent_library": bool(a.parent), "n_chains": K, "end_threshold": threshold, "patience": 2}
    # (b) first, while pos / val / status still serve both calls: the parent's kernels and this library's, alternating
    if a.parent:
        old = C.CDLL(a.parent)
        old.lec_follow_spans.restype, old.lec_follow_spans.argtypes = C.c_int, [C.POINTER(_lib.FollowSpansArgs)]
        old.lec_follow_many.restype, old.lec_follow_many.argtypes = C.c_int, [C.POINTER(_lib.FollowManyArgs)]

        def run(which, call, args):
            if getattr(which, call)(C.byref(args)):
                raise RuntimeError(f"{call} failed")

        for rep in range(2):
            for name, which in (("parent", old), ("this", lib)):
                for call, args in (("lec_follow_spans", pa), ("lec_follow_many", ma)):
                    med, all_ms = timed(lambda: run(which, call, args))
                    res.setdefault(f"{call}_{name}_ms", []).append(round(med, 4))
                    res.setdefault(f"{call}_{name}_all_ms", []).append(all_ms)
    # (a) one launch ...
    med, all_ms = timed(lambda: _lib.check(lib.lec_follow_spans(C.byref(pa)), "lec_follow_spans"))
    res["lec_follow_spans_ms"], res["lec_follow_spans_all_ms"] = round(med, 4), all_ms
    torch.cuda.synchronize()
    # ... and the chunk calls, the state carried
    state = torch.zeros((K, 8), dtype=torch.int32, device=dev)
    span_c = torch.empty((K, 2), dtype=torch.int32, device=dev)
    res["chunks"] = {}
    for size in (64, 512):
        size = min(size, nt)
        pos_c, val_c, status_c = (torch.empty(shape, dtype=dt, device=dev) for shape, dt in (((K, size, 2), torch.int32), ((K, size), torch.float64), ((K, size), torch.int32)))
        calls = []
        for t in range(0, nt, size):
            n = min(size, nt - t)
            calls.append((t, n, _lib.FollowChunkArgs(
                **dict(common, u_d=ptr(w["u"][t: t + n]), v_d=ptr(w["v"][t: t + n]), hgt_d=ptr(w["h"][t: t + n]), nt=n), n_chains=K, patience=2,
                end_threshold=threshold, start_d=ptr(start3), pos_d=ptr(pos_c), val_d=ptr(val_c), status_d=ptr(status_c), span_d=ptr(span_c),
                t_base=t, state_d=ptr(state))))

        def all_chunks(check=None):
            state.zero_()
            for t, n, ca in calls:
                _lib.check(lib.lec_follow_spans_chunk(C.byref(ca)), "lec_follow_spans_chunk")
                if check is not None:
                    check(t, n)

        same = []

        def compare(t, n):
            same.append(bool(torch.equal(pos_c[:, :n], pos[:, t: t + n]) and torch.equal(status_c[:, :n], status[:, t: t + n])
                             and torch.equal(val_c[:, :n].contiguous().view(torch.int64), val[:, t: t + n].contiguous().view(torch.int64))))

        # (a short last chunk writes [K][n] into the front of the [K][size] buffers: compared on a view of that shape)
        if nt % size == 0:
            all_chunks(compare)
        med, all_ms = timed(all_chunks)
        res["chunks"][str(size)] = {"calls": len(calls), "lec_follow_spans_chunk_ms": round(med, 4), "lec_follow_spans_chunk_all_ms": all_ms,
                                    "same_bits": (all(same) and bool(torch.equal(span_c, span))) if same else None}
    out["chunked"] = res
    print(json.dumps(out))
    if a.out:
        kept = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                kept = json.loads(f.read())
        kept["chunked"] = dict(res, steps=nt, csrc_sha=out["csrc_sha"])
        with open(a.out, "w") as f:
            f.write(json.dumps(kept) + "\n")


def ring(a, lib, out, w, timed):
    import torch
    from lorenzcycletoolkit_amd import _lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    nt, ny, nx, dev, bounds = w["nt"], w["ny"], w["nx"], w["dev"], w["bounds"]
    old = lib
    if a.parent:
        old = C.CDLL(a.parent)
        old.lec_follow_spans_chunk.restype, old.lec_follow_spans_chunk.argtypes = C.c_int, [C.POINTER(_lib.FollowChunkArgs)]
        old.lec_follow_seeds_series.restype, old.lec_follow_seeds_series.argtypes = C.c_int, [C.POINTER(_lib.FollowSeedsSeriesArgs)]
    tables = lambda t: dict(xcoef_d=ptr(t[0]), ycoef_d=ptr(t[1]), curv_d=ptr(t[2]))
    common = dict(u_d=ptr(w["u"]), v_d=ptr(w["v"]), hgt_d=ptr(w["h"]), nt=nt, ny=ny, nx=nx, field=_lib.FOLLOW_ZETA, sense=_lib.FOLLOW_MIN, smooth_r=0,
                  jlo=bounds[0], jhi=bounds[1], ilo=bounds[2], ihi=bounds[3], stream=w["stream"])
    open_t, ring_t = tables((w["xc"], w["yc"], w["cv"])), tables(w["ring_tables"])
    K, k = a.chains, 8
    rng = np.random.default_rng(2)
    t0 = np.sort(rng.integers(0, max(1, nt - 1), K))
    t0[0] = 0
    table = np.c_[t0, rng.integers(bounds[0], bounds[1] + 1, K), rng.integers(bounds[2], bounds[3] + 1, K)].astype(np.int32)
    start3 = torch.as_tensor(table).to(dev)
    pos, val, status = (torch.empty(shape, dtype=dt, device=dev) for shape, dt in (((K, nt, 2), torch.int32), ((K, nt), torch.float64), ((K, nt), torch.int32)))
    span, state = torch.empty((K, 2), dtype=torch.int32, device=dev), torch.zeros((K, 8), dtype=torch.int32, device=dev)
    chain = dict(common, sj=w["sj"], si=w["si"], n_chains=K, patience=0, end_threshold=float("nan"), start_d=ptr(start3), pos_d=ptr(pos), val_d=ptr(val),
                 status_d=ptr(status), span_d=ptr(span), t_base=0, state_d=ptr(state))
    ca_open, ca_ring = _lib.FollowChunkArgs(**chain, **open_t), _lib.FollowChunkArgs(**chain, **ring_t)
    ej, ei = 30, 30                                      # half the default box on the 0.25-degree slice, as --lifecycle
    work = torch.empty((nt, ny, nx), dtype=torch.float64, device=dev)
    spos, sval, sn = (torch.empty(shape, dtype=dt, device=dev) for shape, dt in (((nt, k, 2), torch.int32), ((nt, k), torch.float64), ((nt,), torch.int32)))
    seeds = dict(common, ej=ej, ei=ei, k_max=k, reserved0=0, threshold=float("nan"), work_d=ptr(work), seed_pos_d=ptr(spos), seed_val_d=ptr(sval), n_found_d=ptr(sn))
    sa_open, sa_ring = _lib.FollowSeedsSeriesArgs(**seeds, **open_t), _lib.FollowSeedsSeriesArgs(**seeds, **ring_t)

    def run(which, call, args, zero):
        if zero:
            state.zero_()
        if getattr(which, call)(C.byref(args)):
            raise RuntimeError(f"{call} failed: {lib.lec_last_error()}")

    res = {"parent_library": bool(a.parent), "n_chains": K, "k_max": k, "window": [2 * w["sj"] + 1, 2 * w["si"] + 1], "neighbourhood": [2 * ej + 1, 2 * ei + 1]}
    for rnd in range(2):
        for name, which, call, args, zero in (("parent_chunk", old, "lec_follow_spans_chunk", ca_open, True),
                                              ("ring_chunk", lib, "lec_follow_spans_chunk_ring", ca_ring, True),
                                              ("parent_seeds", old, "lec_follow_seeds_series", sa_open, False),
                                              ("ring_seeds", lib, "lec_follow_seeds_series_ring", sa_ring, False)):
            med, all_ms = timed(lambda: run(which, call, args, zero))
            res.setdefault(f"{name}_ms", []).append(round(med, 4))
            res.setdefault(f"{name}_all_ms", []).append(all_ms)
    res["chunk_ratio_ring_over_parent"] = [round(r / p, 4) for r, p in zip(res["ring_chunk_ms"], res["parent_chunk_ms"])]
    res["seeds_ratio_ring_over_parent"] = [round(r / p, 4) for r, p in zip(res["ring_seeds_ms"], res["parent_seeds_ms"])]
    out["ring"] = res
    print(json.dumps(out))
    if a.out:
        kept = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                kept = json.loads(f.read())
        kept["ring"] = dict(res, steps=nt, csrc_sha=out["csrc_sha"])
        with open(a.out, "w") as f:
            f.write(json.dumps(kept) + "\n")


if __name__ == "__main__":
    main()
