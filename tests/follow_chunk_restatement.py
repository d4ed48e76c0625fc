"""NumPy restatement of the rule of ``lec_follow_spans_chunk`` (the rule's text: include/lec_hip.h) -- TEST INFRASTRUCTURE ONLY, written
from that text on top of follow_restatement's field, window and smoothing functions, independent of the product's host and device code.

A chain's state is eight ints {phase, jc, ic, weak, first, last, 0, 0}, zeroed before the first chunk and carried by the caller.
Per chain and call on the chunk's steps [t_base, t_base + nt):
  bad start    (j, i) outside the admissible centres or t0 < 0: phase 3; every step BAD_START, pos -1, NaN; span (-1, -1).
  phase 0      t_base <= t0 < t_base + nt: born here -- the local steps before t0 NOT_LIVE, then it walks from t0 with start (j, i);
               t0 beyond the chunk: every step NOT_LIVE, the phase stays 0.
  phase 1      it walks from local step 0 with the centre and the counters of the state.
  phase 2      every step NOT_LIVE.
  walked step  the window of admissible centres within (sj, si) of the previous centre, the first extreme finite S in row-major order;
               none: the centre stays, status 1.  Good: status 0 and the value at least as good as the end threshold (None: status 0
               alone).  Good: first / last (series steps), weak = 0; else weak + 1, and weak == patience stops the chain: the rest of
               the chunk NOT_LIVE, phase 2.  Patience 0 never stops.
  span         (first, last) of the state after the chunk, (-1, -1) for a chain without a good step, not yet born or with a bad start.
"""
import numpy as np

from tests import follow_restatement as fr

BAD_START, NOT_LIVE = 2, 3
UNBORN, WALKING, STOPPED, BAD = 0, 1, 2, 3


def chunk_call(u, v, h, lat, lon, t_base, starts, state, *, end_threshold=None, patience=2, length=15.0, width=15.0, search=5.0, smooth=0,
               field="zeta", hemisphere=None, formulation="metpy_no_crs"):
    """One call on the chunk's slices u, v, h [nt][ny][nx].  starts: [(t0, j, i)], state: [K] lists of eight ints, updated in place.
    -> (pos [K][nt][2], val [K][nt], status [K][nt], span [K][2])."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    F = fr.field_of(u, v, h, lat, lon, field, formulation)
    nt = F.shape[0]
    if hemisphere is None:
        hemisphere = "south" if lat[0] < 0 else "north"
    want_max = field == "zeta" and hemisphere == "north"
    jlo, jhi, ilo, ihi = fr.admissible(lat, lon, length, width)
    sj, si = fr.window_steps(lat, lon, search)
    K = len(starts)
    pos, val = np.full((K, nt, 2), -1, dtype=np.int64), np.full((K, nt), np.nan)
    status, span = np.full((K, nt), NOT_LIVE, dtype=np.int64), np.full((K, 2), -1, dtype=np.int64)
    for c, (t0, j, i) in enumerate(starts):
        st = state[c]
        if t0 < 0 or not (jlo <= j <= jhi and ilo <= i <= ihi):
            status[c] = BAD_START
            st[:] = [BAD, -1, -1, 0, -1, -1, 0, 0]
            continue
        if st[0] == UNBORN:
            if not t_base <= t0 < t_base + nt:
                continue                                        # not yet: nothing changes
            begin = t0 - t_base
            st[:] = [WALKING, int(j), int(i), 0, -1, -1, 0, 0]
        elif st[0] == WALKING:
            begin = 0
        else:
            span[c] = (st[4], st[5])                            # stopped: what it had
            continue
        for t in range(begin, nt):
            j0, j1 = max(jlo, st[1] - sj), min(jhi, st[1] + sj)
            i0, i1 = max(ilo, st[2] - si), min(ihi, st[2] + si)
            W = fr.smoothed(F[t], smooth, (j0, j1, i0, i1))[j0: j1 + 1, i0: i1 + 1]
            ok = np.isfinite(W)
            good = False
            if ok.any():
                key = np.where(ok, W, -np.inf if want_max else np.inf)
                n = int(np.argmax(key) if want_max else np.argmin(key))
                st[1], st[2] = j0 + n // W.shape[1], i0 + n % W.shape[1]
                val[c, t], status[c, t] = float(W.ravel()[n]), 0
                good = end_threshold is None or (val[c, t] >= end_threshold if want_max else val[c, t] <= end_threshold)
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
    return pos, val, status, span


def walk_chunked(u, v, h, lat, lon, starts, sizes, **kw):
    """The series cut into consecutive chunks of ``sizes`` steps, the state carried: (pos [K][nt][2], val, status [K][nt] concatenated,
    the last call's span, the final state)."""
    assert sum(sizes) == len(u)
    state = [[0] * 8 for _ in starts]
    parts, a = [], 0
    for n in sizes:
        cut = lambda x: None if x is None else x[a: a + n]
        parts.append(chunk_call(cut(u), cut(v), cut(h), lat, lon, a, starts, state, **kw))
        a += n
    return (np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1),
            np.concatenate([p[2] for p in parts], axis=1), parts[-1][3], state)
