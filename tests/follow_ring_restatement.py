"""NumPy restatement of the rule of the two ring calls, ``lec_follow_seeds_series_ring`` and ``lec_follow_spans_chunk_ring`` (the rule's
text: include/lec_hip.h) -- TEST INFRASTRUCTURE ONLY, written from that text, independent of the product's host and device code.

Longitude is periodic: column nx - 1 is the western neighbour of column 0.
  field        ``hgt`` as it is; ``zeta`` through oracle/track_diagnostics.py on the slice with one wrapped column added on either side
               (at lon[nx - 1] - 360 and lon[0] + 360), of which the middle nx columns are kept: every column then has the centred
               three-point stencil, the two at the seam over the arc across it.  The latitude stencil is the oracle's.
  centres      every column; the rows whose box lies inside the latitude range.
  S            the mean of the finite field values with |dj| <= r inside the slice and the 2 r + 1 columns i - r .. i + r on the ring,
               summed in row-major order of that neighbourhood, west to east from i - r.
  window       rows [jc - sj, jc + sj] cut to [jlo, jhi]; columns ic - si .. ic + si, never cut, west to east, mod nx.
  centre       the first extreme finite S in row-major order of the WINDOW; its column is written mod nx; none: the centre stays.
  chain        good / stop / span / state and the status codes: follow_chunk_restatement's, statement for statement.
  seeds        follow_many_restatement's candidates with the neighbourhood |dj| <= ej inside the slice and ring distance <= ei; the tie
               clause keeps the slice's absolute row-major index (a tie is the one thing that depends on where the seam lies).
  refused      2 si + 1 + 2 r > nx, 2 ei + 1 > nx, 2 r + 1 > nx: the window would meet itself.
"""
import numpy as np

from oracle import track_diagnostics as td
from tests import follow_restatement as fr

BAD_START, NOT_LIVE = 2, 3
UNBORN, WALKING, STOPPED, BAD = 0, 1, 2, 3


def field_of(u, v, h, lat, lon, field="zeta", formulation="metpy_no_crs"):
    """[nt][ny][nx] float64 on the ring."""
    if field == "hgt":
        return np.asarray(h, dtype=np.float64)
    lon = np.asarray(lon, dtype=np.float64)
    wrap = lambda a: np.concatenate([a[..., -1:], a, a[..., :1]], axis=-1)
    lon3 = np.concatenate([[lon[-1] - 360.0], lon, [lon[0] + 360.0]])
    fn = td.vorticity_no_crs if formulation == "metpy_no_crs" else td.vorticity_sphere
    return fn(wrap(np.asarray(u, dtype=np.float64)), wrap(np.asarray(v, dtype=np.float64)), lat, lon3)[..., 1:-1]


def rows_admissible(lat, length):
    lat = np.asarray(lat, dtype=np.float64)
    jj = [j for j in range(lat.size) if lat[j] - length / 2 >= lat[0] and lat[j] + length / 2 <= lat[-1]]
    if not jj:
        raise ValueError("the box does not fit into the domain")
    return jj[0], jj[-1]


def smoothed_at(F, r, j, i):
    """S of one [ny][nx] slice at (j, i), i any integer (taken mod nx): python loops, the rule's order.  NaN where nothing is finite."""
    ny, nx = F.shape
    total, count = 0.0, 0
    for jj in range(max(j - r, 0), min(j + r, ny - 1) + 1):
        for k in range(2 * r + 1):
            f = F[jj, (i - r + k) % nx]
            if np.isfinite(f):
                total += float(f)
                count += 1
    return total / count if count else np.nan


def smoothed(F, r):
    """S of the whole slice."""
    F = np.asarray(F, dtype=np.float64)
    assert 2 * r + 1 <= F.shape[1], "refused: 2 r + 1 > nx"
    return np.array([[smoothed_at(F, r, j, i) for i in range(F.shape[1])] for j in range(F.shape[0])])


def chunk_call(u, v, h, lat, lon, t_base, starts, state, *, end_threshold=None, patience=2, length=15.0, width=15.0, search=5.0, smooth=0,
               field="zeta", hemisphere=None, formulation="metpy_no_crs"):
    """One call on the chunk's slices u, v, h [nt][ny][nx].  starts: [(t0, j, i)], state: [K] lists of eight ints, updated in place.
    -> dict(pos [K][nt][2], val [K][nt], status [K][nt], span [K][2]; for the bars: margin [K][nt] -- the distance between the best and
    the second-best DIFFERENT value of the window as a fraction of ``scale`` = max |finite F| of the chunk, inf for a tie or a lone
    value -- and tile_scale [K][nt]: max |finite F| of the window grown by the smoothing radius)."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    F = field_of(u, v, h, lat, lon, field, formulation)
    nt, ny, nx = F.shape
    if hemisphere is None:
        hemisphere = "south" if lat[0] < 0 else "north"
    want_max = field == "zeta" and hemisphere == "north"
    jlo, jhi = rows_admissible(lat, length)
    sj, si = fr.window_steps(lat, lon, search)
    r = smooth
    assert 2 * si + 1 + 2 * r <= nx, "refused: 2 si + 1 + 2 r > nx"
    scale = float(np.max(np.abs(F[np.isfinite(F)]))) if np.isfinite(F).any() else 0.0
    K = len(starts)
    pos, val = np.full((K, nt, 2), -1, dtype=np.int64), np.full((K, nt), np.nan)
    status, span = np.full((K, nt), NOT_LIVE, dtype=np.int64), np.full((K, 2), -1, dtype=np.int64)
    margin, tile_scale = np.full((K, nt), np.inf), np.zeros((K, nt))
    for c, (t0, j, i) in enumerate(starts):
        st = state[c]
        if t0 < 0 or not (jlo <= j <= jhi and 0 <= i < nx):
            status[c] = BAD_START
            st[:] = [BAD, -1, -1, 0, -1, -1, 0, 0]
            continue
        if st[0] == UNBORN:
            if not t_base <= t0 < t_base + nt:
                continue
            begin = t0 - t_base
            st[:] = [WALKING, int(j), int(i), 0, -1, -1, 0, 0]
        elif st[0] == WALKING and jlo <= st[1] <= jhi and 0 <= st[2] < nx:
            begin = 0
        else:
            if st[0] in (WALKING, STOPPED):
                span[c] = (st[4], st[5])                        # stopped (or a walking state that is none of the rule's): what it had
            continue
        for t in range(begin, nt):
            j0, j1 = max(jlo, st[1] - sj), min(jhi, st[1] + sj)
            cols = [(st[2] - si + k) % nx for k in range(2 * si + 1)]              # west to east, never cut
            W = np.array([[smoothed_at(F[t], r, jj, ii) for ii in cols] for jj in range(j0, j1 + 1)])
            tile = F[t][max(j0 - r, 0): min(j1 + r, ny - 1) + 1][:, [(st[2] - si - r + k) % nx for k in range(2 * si + 1 + 2 * r)]]
            tile_scale[c, t] = float(np.max(np.abs(tile[np.isfinite(tile)]))) if np.isfinite(tile).any() else 0.0
            ok = np.isfinite(W)
            good = False
            if ok.any():
                key = np.where(ok, W, -np.inf if want_max else np.inf)
                n = int(np.argmax(key) if want_max else np.argmin(key))            # the first in row-major order of the window
                st[1], st[2] = j0 + n // W.shape[1], cols[n % W.shape[1]]
                best = float(W.ravel()[n])
                val[c, t], status[c, t] = best, 0
                others = W[ok & (W != best)]
                if others.size:
                    margin[c, t] = float(np.min(np.abs(others - best))) / scale
                good = end_threshold is None or (best >= end_threshold if want_max else best <= end_threshold)
            else:
                status[c, t] = 1
            pos[c, t] = (st[1], st[2])
            if good:
                st[4] = t_base + t if st[4] < 0 else st[4]
                st[5], st[3] = t_base + t, 0
            else:
                st[3] += 1
                if st[3] == patience:
                    st[0] = STOPPED
                    break
        span[c] = (st[4], st[5])
    return {"pos": pos, "val": val, "status": status, "span": span, "margin": margin, "tile_scale": tile_scale, "scale": scale}


def walk_chunked(u, v, h, lat, lon, starts, sizes, **kw):
    """The series cut into consecutive chunks of ``sizes`` steps, the state carried: chunk_call's dict with the per-step arrays
    concatenated, the last call's span, and ``state``: the final one."""
    assert sum(sizes) == len(u)
    state = [[0] * 8 for _ in starts]
    parts, a = [], 0
    for n in sizes:
        cut = lambda x: None if x is None else x[a: a + n]
        parts.append(chunk_call(cut(u), cut(v), cut(h), lat, lon, a, starts, state, **kw))
        a += n
    out = {k: np.concatenate([p[k] for p in parts], axis=1) for k in ("pos", "val", "status", "margin", "tile_scale")}
    out.update(span=parts[-1]["span"], state=state, scale=max(p["scale"] for p in parts))
    return out


def seeds(u0, v0, h0, lat, lon, *, k, threshold=None, separation=None, length=15.0, width=15.0, smooth=0, field="zeta", hemisphere=None,
          formulation="metpy_no_crs"):
    """The seeds of ONE slice on the ring -> dict(pos [n][2], val [n], n_found, S, scale, margin: the smallest gap, as a fraction of
    scale, between a seed and the best other value of its neighbourhood, between consecutive candidates up to the first one left out,
    and between any candidate-before-threshold and the threshold; exact ties are decided by the order and count as inf)."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    one = lambda a: None if a is None else np.asarray(a, dtype=np.float64)[None]
    F = field_of(one(u0), one(v0), one(h0), lat, lon, field, formulation)[0]
    ny, nx = F.shape
    if hemisphere is None:
        hemisphere = "south" if lat[0] < 0 else "north"
    want_max = field == "zeta" and hemisphere == "north"
    sgn = -1.0 if want_max else 1.0
    jlo, jhi = rows_admissible(lat, length)
    sep = (length / 2, width / 2) if separation is None else separation
    ej = max(1, int(np.floor(sep[0] / np.median(np.abs(np.diff(lat))))))
    ei = max(1, int(np.floor(sep[1] / np.median(np.abs(np.diff(lon))))))
    assert 2 * ei + 1 <= nx, "refused: 2 ei + 1 > nx"
    S = smoothed(F, smooth)
    scale = float(np.max(np.abs(F[np.isfinite(F)]))) if np.isfinite(F).any() else 0.0

    def candidates(thr):
        out = []
        for j in range(jlo, jhi + 1):
            for i in range(nx):
                s = S[j, i]
                if not np.isfinite(s) or (thr is not None and sgn * s > sgn * thr):
                    continue
                ok, gap = True, np.inf
                for jj in range(max(j - ej, 0), min(j + ej, ny - 1) + 1):
                    for d in range(-ei, ei + 1):
                        ii = (i + d) % nx
                        if (jj, ii) == (j, i) or not np.isfinite(S[jj, ii]):
                            continue
                        diff = sgn * (S[jj, ii] - s)                              # > 0: the neighbour is worse
                        if diff < 0 or (diff == 0 and (jj, ii) < (j, i)):         # the slice's absolute row-major order
                            ok = False
                        elif diff > 0:
                            gap = min(gap, diff)
                if ok:
                    out.append((sgn * s, j * nx + i, j, i, float(s), float(gap)))
        out.sort()
        return out

    cands = candidates(threshold)
    taken = cands[:k]
    keys = [c[0] for c in cands[:k + 1]]
    gaps = np.diff(keys) if len(keys) > 1 else np.array([])
    parts = list(np.where(gaps == 0, np.inf, gaps)) + [c[5] for c in taken]
    if threshold is not None:
        thr = np.array([abs(c[4] - threshold) for c in candidates(None)])
        parts += list(np.where(thr == 0, np.inf, thr))
    margin = float(min([np.inf] + parts)) / scale if scale else np.inf
    return {"pos": np.array([(c[2], c[3]) for c in taken], dtype=np.int64).reshape(-1, 2), "val": np.array([c[4] for c in taken]),
            "n_found": len(taken), "S": S, "scale": scale, "margin": margin, "ej": ej, "ei": ei}
