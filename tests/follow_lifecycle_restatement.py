"""NumPy restatement of the rules of ``-c --choose-lifecycle`` (``lec_follow_seeds_series``, ``lec_follow_spans`` -- the rules' text:
include/lec_hip.h -- and the host's births / resolve, lorenzcycletoolkit_amd/follow.py) -- TEST INFRASTRUCTURE ONLY, written from that
text on top of follow_restatement / follow_many_restatement, independent of the product's host and device code.

Seeds of a series: follow_many_restatement's seeds of every slice.  Births: every seed of step 0; a seed of step t >= 1 unless a seed
of step t - 1 lies within (sj, si) grid steps of it; ordered by (step, rank).  A chain from (t0, start): follow_restatement's chain
on the sub-series that begins at t0.  A walked step is good when its status is 0 and its value at least as good as the end threshold
(None: status 0 alone); the chain stops after the first step that completes ``patience`` not-good steps in a row, or at the end;
span = (first good, last good) or (-1, -1); steps not walked: pos -1, NaN, status 3.  Resolve, in birth order: no span -> dropped; a
chain born inside the span of an earlier KEPT chain whose centre then lies within (ej, ei) of the birth is that chain's continuation
(the first such chain) and dropped.  Tracks: the span; fewer than ``min_steps`` steps: too short.
"""
import numpy as np

from tests import follow_many_restatement as fm
from tests import follow_restatement as fr

NOT_LIVE = 3


def seeds_series(u, v, h, lat, lon, *, k, **kw):
    """[nt] of follow_many_restatement.find_systems' dicts (a slice without a finite value: nothing found, margin inf)."""
    out = []
    for t in range(len(u)):
        F = fr.field_of(u[t][None], v[t][None], None if h is None else h[t][None], lat, lon, kw.get("field", "zeta"), kw.get("formulation", "metpy_no_crs"))
        if not np.isfinite(F).any():
            out.append({"pos": np.zeros((0, 2), dtype=np.int64), "val": np.zeros(0), "n_found": 0, "margin": np.inf, "scale": 0.0})
            continue
        out.append(fm.find_systems(u[t], v[t], None if h is None else h[t], lat, lon, k=k, **kw))
    return out


def births(seeds, sj, si):
    """[(step, j, i, rank)] from [nt] arrays of seed positions."""
    out = []
    for t, now in enumerate(seeds):
        for rank, (j, i) in enumerate(now):
            explained = t > 0 and any(abs(int(a) - int(j)) <= sj and abs(int(b) - int(i)) <= si for a, b in seeds[t - 1])
            if not explained:
                out.append((t, int(j), int(i), rank))
    return out


def _walk(u, v, h, lat, lon, t0, ji, kw):
    """follow_restatement's chain on the sub-series from t0 (lists of pos, val, status, margin, scale per step).  A first step whose
    window is blind -- which follow_restatement refuses -- keeps the start, and the chain goes on from it at the next step."""
    nt = len(u)
    pos, val, status, margin, scale = [], [], [], [], []
    t = t0
    while t < nt:
        try:
            ref = fr.follow(u[t:], v[t:], None if h is None else h[t:], lat, lon, start=(lat[ji[0]], lon[ji[1]]), **kw)
        except ValueError:
            pos.append(tuple(ji)); val.append(np.nan); status.append(1); margin.append(np.inf); scale.append(np.nan)
            t += 1
            continue
        pos += [tuple(p) for p in ref["pos"]]; val += list(ref["val"]); status += list(ref["status"]); margin += list(ref["margin"])
        scale += [ref["scale"]] * (nt - t)
        break
    return pos, val, status, margin, scale


def chain(u, v, h, lat, lon, t0, ji, *, end_threshold=None, patience=2, **kw):
    """-> dict(pos [nt][2], val [nt], status [nt], span (first, last), stop: the last walked step, margin: the smallest window margin
    over the walked steps as follow_restatement gives it on the sub-series, threshold_margin: the smallest |val - end_threshold| over the
    walked steps with a value, as a fraction of max |finite F| of the WHOLE series, whichever step the chain is born at)."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    nt = len(u)
    F = fr.field_of(u, v, h, lat, lon, kw.get("field", "zeta"), kw.get("formulation", "metpy_no_crs"))
    scale = float(np.max(np.abs(F[np.isfinite(F)])))
    hemisphere = kw.get("hemisphere") or ("south" if lat[0] < 0 else "north")
    want_max = kw.get("field", "zeta") == "zeta" and hemisphere == "north"
    wpos, wval, wstatus, wmargin, wscale = _walk(u, v, h, lat, lon, t0, ji, kw)
    pos, val, status = np.full((nt, 2), -1, dtype=np.int64), np.full(nt, np.nan), np.full(nt, NOT_LIVE, dtype=np.int64)
    first = last = -1
    weak, stop, margin, thr = 0, nt - 1, np.inf, np.inf
    for n, t in enumerate(range(t0, nt)):
        pos[t], val[t], status[t] = wpos[n], wval[n], wstatus[n]
        margin = min(margin, wmargin[n])                                      # (follow_restatement's: a fraction of the sub-series' scale)
        good = wstatus[n] == 0
        if good and end_threshold is not None:
            thr = min(thr, abs(wval[n] - end_threshold) / scale)
            good = wval[n] >= end_threshold if want_max else wval[n] <= end_threshold
        if good:
            first, last, weak = (t if first < 0 else first), t, 0
        else:
            weak += 1
            if weak == patience:
                stop = t
                break
    return {"pos": pos, "val": val, "status": status, "span": (first, last), "stop": stop, "margin": float(margin), "threshold_margin": float(thr)}


def resolve(born, chains, ej, ei):
    """-> (kept [K] of bool, continuation_of [K]: a chain's index or None)."""
    kept, cont = [], []
    for c, (t0, j, i, _) in enumerate(born):
        of = None
        if chains[c]["span"][0] >= 0:
            for b in range(c):
                first, last = chains[b]["span"]
                if kept[b] and first <= t0 <= last and abs(int(chains[b]["pos"][t0][0]) - j) <= ej and abs(int(chains[b]["pos"][t0][1]) - i) <= ei:
                    of = b
                    break
        cont.append(of)
        kept.append(chains[c]["span"][0] >= 0 and of is None)
    return kept, cont


def lifecycle(u, v, h, lat, lon, *, k, threshold, end_threshold=None, patience=2, min_steps=2, separation=None, length=15.0, width=15.0,
              search=5.0, smooth=0, field="zeta", hemisphere=None, formulation="metpy_no_crs"):
    """The whole rule -> dict(births [(step, j, i, rank)], chains, spans, outcome [K]: 'kept' / 'continuation' / 'too short' / 'never good',
    continuation_of [K], and the margins: seeds, windows, threshold -- each the smallest of its kind, a fraction of the field's scale)."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    common = dict(length=length, width=width, smooth=smooth, field=field, hemisphere=hemisphere, formulation=formulation)
    series = seeds_series(u, v, h, lat, lon, k=k, threshold=threshold, separation=separation, **common)
    sj, si = fr.window_steps(lat, lon, search)
    sep = (length / 2, width / 2) if separation is None else separation
    ej, ei = fm.separation_steps(lat, lon, *sep)
    born = births([s["pos"] for s in series], sj, si)
    end = threshold if end_threshold is None else end_threshold
    chains = [chain(u, v, h, lat, lon, t0, (j, i), end_threshold=end, patience=patience, search=search, **common) for t0, j, i, _ in born]
    kept, cont = resolve(born, chains, ej, ei)
    outcome = []
    for c, ch in enumerate(chains):
        first, last = ch["span"]
        outcome.append("never good" if first < 0 else "continuation" if cont[c] is not None else "too short" if last - first + 1 < min_steps else "kept")
    return {"births": born, "chains": chains, "spans": [c["span"] for c in chains], "outcome": outcome, "continuation_of": cont, "series": series,
            "ej": ej, "ei": ei, "sj": sj, "si": si,
            "margins": {"seeds": float(min([np.inf] + [s["margin"] for s in series])),
                        "windows": float(min([np.inf] + [c["margin"] for c in chains])),
                        "threshold": float(min([np.inf] + [c["threshold_margin"] for c in chains]))}}
