"""The longitude-resolved maps of the six eddy terms (-f [--periodic] --maps), restated on the CPU from the
oracle's 4-D fields.  Nothing of the kernel is restated here: a map is the integrand of ``tests/sections_restatement.sections`` with the
zonal average ``za(...)`` left off -- the pointwise product of the oracle's ``*_ZE`` fields times the very factors the oracle's
``energy_contents`` / ``conversion_terms`` / ``generation_terms`` multiply them by, with the oracle's ``sigma_AA``.  ``zonal_average`` is
linear, so the box's zonal average of a map (``zonal_average`` below) is the section, and that of the Hovmoeller the oracle's scalar.

Order of the terms: Ae Ke Ca Ce Ck Ge (``TERMS``).  A ring's ``Box`` carries the closed axis (column 0 once more at the end): ``maps``
drops that closing column, ``zonal_average`` puts it back."""
from __future__ import annotations

import numpy as np

from oracle import lec_oracle as o
from tests import sections_restatement as sr

TERMS = ["Ae", "Ke", "Ca", "Ce", "Ck", "Ge"]


def maps(b: o.Box, ring: bool) -> np.ndarray:
    """Y [time, 6, level, lat, lon] of the box as it stands; ``ring``: ``b`` is ``ring_restatement.ring_box``'s (closed axis)."""
    f = b.f
    s4 = b.sigma_AA[:, :, None, None]
    c4 = lambda c: c[None, None, :, None]
    c1 = (o.RD / (b.level * o.G))[None, :, None, None]
    out = {}
    # energy_contents
    out["Ae"] = f["tair_ZE"] ** 2 / (2 * s4)
    out["Ke"] = f["u_ZE"] ** 2 + f["v_ZE"] ** 2
    # conversion_terms
    dphi_tae = o.differentiate(f["tair_AE"] * b.coslats[None, None, :], b.rlats, axis=2)
    t1 = (f["v_ZE"] * f["tair_ZE"] * dphi_tae[..., None]) / (2 * o.RE * s4)
    dp_tae = o.differentiate(f["tair_AE"], b.level, axis=1)
    t2 = (f["omega_ZE"] * f["tair_ZE"]) * dp_tae[..., None]
    out["Ca"] = -(t1 + t2 / s4)
    out["Ce"] = -(c1 * (f["omega_ZE"] * f["tair_ZE"]))
    tan_lats = np.tan(b.rlats)
    d1 = o.differentiate(f["u_ZA"] / b.coslats[None, None, :], b.rlats, axis=2)
    d2 = o.differentiate(f["v_ZA"], b.rlats, axis=2)
    d4 = o.differentiate(f["u_ZA"], b.level, axis=1)
    out["Ck"] = ((c4(b.coslats) * f["u_ZE"] * f["v_ZE"] / o.RE) * d1[..., None] + ((f["v_ZE"] ** 2) / o.RE) * d2[..., None]
                 + (c4(tan_lats) * (f["u_ZE"] ** 2) * f["v_ZA"][..., None]) / o.RE + f["omega_ZE"] * f["u_ZE"] * d4[..., None]
                 + f["omega_ZE"] * f["v_ZE"] * d4[..., None])          # term 5 with d[u]/dp, as the oracle has it
    # generation_terms
    out["Ge"] = (f["Q_ZE"] * f["tair_ZE"]) / (o.CP_D * s4)
    Y = np.stack([np.asarray(out[k], dtype=np.float64) for k in TERMS], axis=1)
    return Y[..., :-1] if ring else Y


def zonal_average(Y: np.ndarray, b: o.Box, ring: bool) -> np.ndarray:
    """The box's own zonal average over the last axis of ``Y`` (the columns ``maps`` returns): ``oracle.zonal_average`` on the box's
    ``rlons`` / ``xlength`` -- closed on a ring (column 0 once more), the half-weight trapezoid on an open box."""
    if ring:
        Y = np.concatenate([Y, Y[..., :1]], axis=-1)
    return o.zonal_average(Y, b.rlons, b.xlength)


def columns(Y: np.ndarray, level: np.ndarray) -> np.ndarray:
    """C [time, 6, lat, lon] of Y [time, 6, level, lat, lon]: ``sections_restatement.columns`` applied per point."""
    nt, nf, nl, ny, nx = Y.shape
    return sr.columns(Y.reshape(nt, nf, nl, ny * nx), level, TERMS).reshape(nt, nf, ny, nx)


def time_mean(C: np.ndarray) -> np.ndarray:
    """(1 / T) sum_t C[t], summed in time order; NaN at any step gives NaN."""
    return sr.time_mean(C)


def hovmoller(C: np.ndarray, cw: np.ndarray) -> np.ndarray:
    """H [time, 6, lon] = sum_j cw_j C[time, 6, j, lon], rows ascending (``cw``: ``sections_restatement.area_weights``); NaN propagates."""
    H = np.zeros(C.shape[:2] + C.shape[3:])
    for j in range(C.shape[2]):
        H = H + cw[j] * C[:, :, j]
    return H
