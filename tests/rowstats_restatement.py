"""The 28 interface statistics of a stage-1 row record (``enum lec_stat``, include/lec_hip.h), restated on the CPU from the oracle's own
functions  --  TEST INFRASTRUCTURE ONLY; no GPU, no torch.

Nothing is re-derived here.  ``oracle.lec_oracle.make_box`` (``tests/ring_restatement.ring_box`` for a ring) already yields X, [X]
(``X_ZA``) and X' (``X_ZE``) of T, u, v, omega, Phi and of Q -- ``adiabatic_heating`` on the box-cropped arrays --, and every
statistic of a record is ``zonal_average`` of a pointwise product of those:

  0..5    [T] [u] [v] [w] [Phi] [Q]
  6..15   [T'T'] [u'u'] [v'v'] [v'T'] [w'T'] [u'v'] [w'u'] [w'v'] [w'Phi'] [Q'T']
  16..21  [vT'T'] [wT'T'] [Kv] [Kw] [Ev] [Ew]   with K = u^2 + v^2 - u'^2 - v'^2 and E = u'^2 + v'^2, the full v / w as a factor, as
          ``boundary_terms`` forms them (BAe's second and third piece, BKz / BKe)
  22..27  the stored T, T, u, u, v, v at the west / east box column

Slots 28..31 of a record are scratch of the kernels and are no interface.  Evaluated in np.longdouble (``extended``) the restatement's
rounding lies far below float64's; ``extended=False`` is the same code in float64 (tests/test_rowstats_cases_cpu.py measures the
distance between the two).  The result is float64 either way.
"""
from __future__ import annotations

import numpy as np

from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests.helpers import as_f64, as_longdouble

NSLOT = 28
MEANS = slice(0, 5)             # judged by the summation bound
MOMENTS = slice(5, 22)          # [Q], second and third moments: judged against the statistic's largest value
EDGES = slice(22, 28)           # stored values: bit-equal
SLOT = {n: i for i, n in enumerate(("MT", "MU", "MV", "MW", "MP", "MQ", "TT", "UU", "VV", "VT", "WT", "UV", "WU", "WV", "WP", "QT",
                                    "VTT", "WTT", "KV", "KW", "EV", "EW", "TW", "TE", "UW", "UE", "VW", "VE"))}
Q_SLOTS = (SLOT["MQ"], SLOT["QT"])
PHI_SLOTS = (SLOT["MP"], SLOT["WP"])


def _wide(dom, extended):
    return as_longdouble(dom) if extended else as_f64(dom)


def _cube(a, extended):
    return None if a is None else np.ascontiguousarray(np.asarray(a).astype(np.longdouble if extended else np.float64))


def records_of_box(b: o.Box, with_q=True, with_phi=True) -> np.ndarray:
    """[nt, nl, nyb, 28] of a ``Box``, in the box's own precision."""
    f = b.f
    za = lambda X: o.zonal_average(X, b.rlons, b.xlength)
    T, u, v, w = f["tair"], f["u"], f["v"], f["omega"]
    Te, ue, ve, we, Pe, Qe = (f[n + "_ZE"] for n in ("tair", "u", "v", "omega", "geopt", "Q"))
    K = u ** 2 + v ** 2 - ue ** 2 - ve ** 2            # boundary_terms: BKz
    E = ue ** 2 + ve ** 2                              # boundary_terms: BKe
    cols = [f[n + "_ZA"] for n in ("tair", "u", "v", "omega", "geopt", "Q")]
    cols += [za(Te * Te), za(ue * ue), za(ve * ve), za(ve * Te), za(we * Te), za(ue * ve), za(we * ue), za(we * ve), za(we * Pe), za(Qe * Te)]
    cols += [za(v * Te ** 2), za(w * Te ** 2), za(K * v), za(K * w), za(E * v), za(E * w)]
    cols += [T[..., 0], T[..., -1], u[..., 0], u[..., -1], v[..., 0], v[..., -1]]
    rec = np.stack(cols, axis=-1)
    if not with_q:
        rec[..., list(Q_SLOTS)] = 0.0
    if not with_phi:
        rec[..., list(PHI_SLOTS)] = 0.0
    return rec


def row_records(dom: o.Domain, limits, *, dTdt=None, with_q=True, with_phi=True, extended=True) -> np.ndarray:
    """float64 [nt, nl, nyb, 28]: the records of ONE fixed box (west, east, south, north) over every step of ``dom``.  ``dTdt``: a dT/dt
    cube on ``dom``'s grid instead of np.gradient over ``dom.time_s``.  ``with_q`` False: [Q] = [Q'T'] = 0; ``with_phi`` False (a call
    without a geopotential cube): [Phi] = [w'Phi'] = 0, exactly."""
    with np.errstate(invalid="ignore"):
        b = o.make_box(_wide(dom, extended), *limits, dTdt=_cube(dTdt, extended))
        return np.asarray(records_of_box(b, with_q, with_phi), dtype=np.float64)


def row_records_moving(dom: o.Domain, limits_per_step, dTdt=None, *, with_phi=True, extended=True) -> np.ndarray:
    """float64 [nt, nl, nyb_max, 28]: step t's rows come from ``make_box`` of box t on that step alone, with slice t of the dT/dt cube
    (default: ``moving_dTdt``, np.gradient over the cube's time axis) -- what ``lec_moving`` hands its analysis classes.  Only the rows
    inside a step's box are defined; the others are NaN here."""
    d = _wide(dom, extended)
    dT = o.moving_dTdt(d) if dTdt is None else _cube(dTdt, extended)
    nt, nl = d.tair.shape[:2]
    recs = []
    with np.errstate(invalid="ignore"):
        for t in range(nt):
            sub = o.Domain(d.tair[t:t + 1], d.u[t:t + 1], d.v[t:t + 1], d.omega[t:t + 1], d.geopt[t:t + 1], d.lat, d.lon, d.level, d.time_s[t:t + 1])
            b = o.make_box(sub, *limits_per_step[t], dTdt=dT[t:t + 1], fixed=False)
            recs.append(np.asarray(records_of_box(b, True, with_phi), dtype=np.float64)[0])
    out = np.full((nt, nl, max(r.shape[1] for r in recs), NSLOT), np.nan)
    for t, r in enumerate(recs):
        out[t, :, :r.shape[1]] = r
    return out


def row_records_ring(dom: o.Domain, south, north, *, dTdt=None, with_q=True, with_phi=True, extended=True) -> np.ndarray:
    """float64 [nt, nl, nyb, 28] of the latitude band [south, north] over all of ``dom``'s longitudes as a closed ring
    (``ring_restatement.ring_box``: the closed axis' zonal mean, Q on the axis extended by one wrap column either side).  The closed
    axis ends on column 0 again, so the east values equal the west values."""
    with np.errstate(invalid="ignore"):
        b = rr.ring_box(_wide(dom, extended), south, north, dTdt=_cube(dTdt, extended), with_geopt=with_phi)
        return np.asarray(records_of_box(b, with_q, with_phi), dtype=np.float64)
