"""The per-wavenumber boundary terms BAe(n), BKe(n), tendencies and residuals on a ring (-f --periodic --wavenumbers N
--wavenumbers-budget), restated on the CPU from the oracle's own functions, in the way of tests/spectrum_restatement.py.

The fields are those of ``ring_restatement.ring_box``.  A triple product [a b'b'] is the covariance of the pointwise product P = a b'
with b, so the four zonal means the oracle's ``boundary_terms`` forms for BAe and BKe on a ring -- [v T'T'],
[w T'T'], [E v], [E w], E = u'^2 + v'^2 -- split into the shares
    VTT(n) = C_n(v T', T)    WTT(n) = C_n(w T', T)    EV(n) = C_n(v u', u) + C_n(v v', v)    EW(n) = C_n(w u', u) + C_n(w v', v)
with C_n(a, b) = w_n Re(a^_n conj(b^_n)), a^ = rfft / nx, w_n = 2, or 1 at n = nx / 2: the products are formed with numpy, the shares
taken from ``np.fft.rfft`` (``row_shares``).  BAe(n) and BKe(n) are then built from the shares with the oracle's ``area_average``,
``interpolate_and_drop_nan_levels`` and ``_int_p`` in the order ``boundary_terms`` combines them (``b_terms``; the east-minus-west term
is 0 on the closed axis), and the tendencies and residuals by ``budgets_and_residuals`` column by column (``budget_terms``).
"""
from __future__ import annotations

import numpy as np

from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests import spectrum_restatement as sr

TERMS = ["BAe", "BKe"]
SLOTS = ["VTT", "WTT", "EV", "EW"]


def row_shares(T, u, v, w, n_wave, means=None):
    """[..., N, 4]: VTT(n), WTT(n), EV(n), EW(n) of rows along the last axis (the ring's nx columns), from ``np.fft.rfft`` of the fp64
    fields and products.  ``means``: the zonal means [T], [u], [v] the eddies are taken against (default: ``mean(axis=-1)``)."""
    T, u, v, w = (np.asarray(a, dtype=np.float64) for a in (T, u, v, w))
    nx = T.shape[-1]
    mT, mU, mV = means if means is not None else (a.mean(axis=-1) for a in (T, u, v))
    with np.errstate(invalid="ignore"):
        Tp, up, vp = T - mT[..., None], u - mU[..., None], v - mV[..., None]
        F = lambda a: np.fft.rfft(a, axis=-1)[..., 1:n_wave + 1] / nx
        wn = np.where(2 * np.arange(1, n_wave + 1) == nx, 1.0, 2.0)
        C = lambda a, b: wn * np.real(F(a) * np.conj(F(b)))
        return np.stack([C(v * Tp, T), C(w * Tp, T), C(v * up, u) + C(v * vp, v), C(w * up, u) + C(w * vp, v)], axis=-1)


def row_totals(T, u, v, w):
    """[..., 4]: [v T'T'], [w T'T'], [E v], [E w] of rows along the last axis: slots 16, 17, 20, 21 of a row record."""
    T, u, v, w = (np.asarray(a, dtype=np.float64) for a in (T, u, v, w))
    zm = lambda a: a.mean(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        Tp, up, vp = T - zm(T), u - zm(u), v - zm(v)
        E = up * up + vp * vp
        return np.stack([(v * Tp * Tp).mean(axis=-1), (w * Tp * Tp).mean(axis=-1), (E * v).mean(axis=-1), (E * w).mean(axis=-1)], axis=-1)


def _bae_bke(b: o.Box, VTT, WTT, EV, EW):
    """BAe and BKe [time] of the ring box from the four zonal means [time, level, latitude] -- of one wavenumber or the whole --, in the
    order ``boundary_terms`` combines them (oracle/lec_oracle.py:395-417); its first term, east minus west, is 0 on the closed axis."""
    s3 = b.sigma_AA[:, :, None]
    c2 = -1 / (o.RE * b.ylength)
    ns = lambda X: X[:, :, -1] - X[:, :, 0]
    bt = lambda X: X[:, -1] - X[:, 0]
    cos3 = b.coslats[None, None, :]
    t2 = ns((VTT * cos3) / (2 * s3))
    t2 = o._int_p(t2, b.level) * c2
    t3 = o.area_average(WTT / (2 * s3), b.rlats, b.coslats)
    t3, _ = o.interpolate_and_drop_nan_levels(t3, b.level)
    bae = t2 - bt(t3)
    t2 = ns(EV * cos3)
    t2 = o._int_p(t2 / (2 * o.G), b.level) * c2
    t3 = o.area_average(EW, b.rlats, b.coslats) / (2 * o.G)
    t3, _ = o.interpolate_and_drop_nan_levels(t3, b.level)
    return bae, t2 - bt(t3)


def b_terms(dom: o.Domain, south, north, n_wave, box=None):
    """(b [time, 2, N], rest [time, 2], total [time, 2]) of the band [south, north] of the ring ``dom``: order BAe, BKe; the total is the
    oracle's own ``boundary_terms``."""
    with np.errstate(invalid="ignore"):
        b = rr.ring_box(dom, south, north) if box is None else box
        T, u, v, w = (np.asarray(b.f[k][..., :-1], dtype=np.float64) for k in ("tair", "u", "v", "omega"))
        means = [np.asarray(b.f[k + "_ZA"], dtype=np.float64) for k in ("tair", "u", "v")]
        sh = row_shares(T, u, v, w, n_wave, means)
        parts = [_bae_bke(b, *(sh[..., n, i] for i in range(4))) for n in range(n_wave)]
        tot = o.boundary_terms(b)
    out = np.stack([np.stack(p, axis=1) for p in parts], axis=-1)
    total = np.stack([tot["BAe"], tot["BKe"]], axis=1)
    return out, total - out.sum(axis=2), total


def budget_columns(spectrum, spectrum_rest, b, b_rest, time_s):
    """(tendency [time, 2, N], tendency_rest [time, 2], residual [time, 2, N], residual_rest [time, 2]) by the oracle's
    ``budgets_and_residuals`` on every column (a wavenumber or the rest) with the zonal reservoirs' terms 0."""
    nt, _, n = spectrum.shape
    cols = np.concatenate([spectrum, spectrum_rest[:, :, None]], axis=2)
    bcols = np.concatenate([b, b_rest[:, :, None]], axis=2)
    tend, resid = np.empty((nt, 2, n + 1)), np.empty((nt, 2, n + 1))
    zero = np.zeros(nt)
    for i in range(n + 1):
        col = {t: cols[:, k, i] for k, t in enumerate(sr.TERMS)}
        col.update({t: bcols[:, k, i] for k, t in enumerate(TERMS)})
        col.update({t: zero for t in ("Az", "Kz", "Cz", "BAz", "BKz")})
        out = o.budgets_and_residuals(col, time_s)
        tend[:, 0, i], tend[:, 1, i] = out["∂Ae/∂t (finite diff.)"], out["∂Ke/∂t (finite diff.)"]
        resid[:, 0, i], resid[:, 1, i] = out["RGe"], out["RKe"]
    return tend[:, :, :n], tend[:, :, n], resid[:, :, :n], resid[:, :, n]


def budget_terms(dom: o.Domain, south, north, n_wave):
    """Everything --wavenumbers-budget writes, as a dict: ``spectrum`` [time, 5, N] / ``spectrum_rest`` (tests/spectrum_restatement.py),
    ``b`` / ``b_rest`` / ``b_total``, ``tendency`` / ``tendency_rest``, ``residual`` / ``residual_rest``."""
    spec, spec_rest, _, _ = sr.spectrum_terms(dom, south, north, n_wave)
    b, b_rest, b_total = b_terms(dom, south, north, n_wave)
    tend, tend_rest, resid, resid_rest = budget_columns(spec, spec_rest, b, b_rest, dom.time_s)
    return dict(spectrum=spec, spectrum_rest=spec_rest, b=b, b_rest=b_rest, b_total=b_total, tendency=tend, tendency_rest=tend_rest,
                residual=resid, residual_rest=resid_rest)
