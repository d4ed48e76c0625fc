"""NumPy restatement of the rule by which ``-c --choose-systems`` finds the systems of the first time step (``lec_follow_seeds``;
the rule's text: include/lec_hip.h) -- TEST INFRASTRUCTURE ONLY, written from that text on top of follow_restatement's field and
smoothing, independent of the product's host and device code.

S: the smoothed field on the WHOLE slice.  Better: smaller for the minimum, larger for the maximum.  A grid point is a candidate when
it is an admissible centre, its S is finite and at least as good as the threshold (None: no threshold), and among the finite S within
(ej, ei) grid points inside the slice none is better and none that comes before it in row-major order is equal.  Seeds: the
candidates by value, best first, equal values by row-major index; the first k of them.
"""
import numpy as np

from tests import follow_restatement as fr


def separation_steps(lat, lon, sep_lat, sep_lon):
    ej = max(1, int(np.floor(sep_lat / np.median(np.abs(np.diff(lat))))))
    ei = max(1, int(np.floor(sep_lon / np.median(np.abs(np.diff(lon))))))
    return ej, ei


def candidates_of(S, bounds, ej, ei, want_max, threshold=None):
    """[(key, row-major index, j, i, S, neighbourhood gap)] of every candidate, best first; key = S for the minimum, -S for the
    maximum.  Plain loops.  The gap: the distance to the best OTHER value of the neighbourhood (equal values are decided by the
    order, not by arithmetic, and do not count); inf when there is none."""
    ny, nx = S.shape
    jlo, jhi, ilo, ihi = bounds
    sgn = -1.0 if want_max else 1.0
    out = []
    for j in range(jlo, jhi + 1):
        for i in range(ilo, ihi + 1):
            s = S[j, i]
            if not np.isfinite(s):
                continue
            if threshold is not None and sgn * s > sgn * threshold:
                continue
            ok, gap = True, np.inf
            for jj in range(max(j - ej, 0), min(j + ej, ny - 1) + 1):
                for ii in range(max(i - ei, 0), min(i + ei, nx - 1) + 1):
                    if (jj, ii) == (j, i) or not np.isfinite(S[jj, ii]):
                        continue
                    d = sgn * (S[jj, ii] - s)                      # > 0: the neighbour is worse
                    if d < 0 or (d == 0 and (jj, ii) < (j, i)):
                        ok = False
                        break
                    if d > 0:
                        gap = min(gap, d)
                if not ok:
                    break
            if ok:
                out.append((sgn * s, j * nx + i, j, i, float(s), float(gap)))
    out.sort()
    return out


def find_systems(u0, v0, h0, lat, lon, *, k, threshold=None, separation=None, length=15.0, width=15.0, smooth=0, field="zeta",
                 hemisphere=None, formulation="metpy_no_crs"):
    """-> dict(pos [n][2], val [n], n_found, scale = max |finite F|, and the margins, each as a fraction of scale:
    neighbourhood [n] (every seed against the best other value of its neighbourhood), rank (the gaps between consecutive seeds and
    between the last one taken and the first one left out), threshold (the distance of every candidate-before-threshold from the
    threshold; empty without one), margin = the smallest of them all).  Exact ties count as inf."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    one = lambda a: None if a is None else np.asarray(a, dtype=np.float64)[None]
    F = fr.field_of(one(u0), one(v0), one(h0), lat, lon, field, formulation)[0]
    if hemisphere is None:
        hemisphere = "south" if lat[0] < 0 else "north"
    want_max = field == "zeta" and hemisphere == "north"
    bounds = fr.admissible(lat, lon, length, width)
    sep = (length / 2, width / 2) if separation is None else separation
    ej, ei = separation_steps(lat, lon, *sep)
    S = fr.smoothed(F, smooth)
    scale = float(np.max(np.abs(F[np.isfinite(F)])))
    cands = candidates_of(S, bounds, ej, ei, want_max, threshold)
    seeds = cands[:k]
    keys = [c[0] for c in cands[:k + 1]]
    gaps = np.diff(keys) if len(keys) > 1 else np.array([])
    rank = np.where(gaps == 0, np.inf, gaps) / scale
    nb = np.array([c[5] for c in seeds]) / scale
    thr = np.array([])
    if threshold is not None:
        thr = np.array([abs(c[4] - threshold) for c in candidates_of(S, bounds, ej, ei, want_max, None)]) / scale
        thr = np.where(thr == 0, np.inf, thr)
    margin = float(min([np.inf] + list(rank) + list(nb) + list(thr)))
    return {"pos": np.array([(c[2], c[3]) for c in seeds], dtype=np.int64).reshape(-1, 2), "val": np.array([c[4] for c in seeds]),
            "n_found": len(seeds), "scale": scale, "neighbourhood": nb, "rank": rank, "threshold": thr, "margin": margin,
            "ej": ej, "ei": ei, "bounds": bounds, "S": S}
