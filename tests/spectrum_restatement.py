"""The zonal-wavenumber spectra of the eddy terms on a ring (-f --periodic --wavenumbers), restated on the CPU from the oracle's own
functions.  Nothing is restated here: the wavenumber-n part of a field is ``np.fft.rfft`` over the ring's nx columns, bin n kept,
``np.fft.irfft``, column 0 appended once more for the closed axis; with the four eddy fields ``tair_ZE``, ``u_ZE``, ``v_ZE`` and
``omega_ZE`` of ``ring_restatement.ring_box`` replaced by their wavenumber-n parts -- and every other field of the box left as it is
-- the oracle's ``energy_contents`` and ``conversion_terms`` give Ae(n), Ke(n), Ca(n), Ce(n), Ck(n) and their per-level tables.  The
zonal mean of a product of two single-wavenumber fields is exactly the share C_n of DESIGN.md section 4.2b, so the N shares and the
totals close to rounding.
"""
from __future__ import annotations

import numpy as np

from oracle import lec_oracle as o
from tests import ring_restatement as rr

TERMS = ["Ae", "Ke", "Ca", "Ce", "Ck"]
LEVEL_TERMS = ["Ae", "Ke", "Ca", "Ca_1", "Ca_2", "Ce", "Ce_1", "Ce_2", "Ck", "Ck_1", "Ck_2", "Ck_3", "Ck_4", "Ck_5"]
EDDY = ("tair", "u", "v", "omega")


def wave_part(X, n):
    """The zonal-wavenumber-n part of X along its last axis (the ring's nx columns)."""
    nx = X.shape[-1]
    F = np.fft.rfft(X, axis=-1)
    G = np.zeros_like(F)
    G[..., n] = F[..., n]
    return np.fft.irfft(G, n=nx, axis=-1)


def _terms(b):
    """(5 scalars [time], 14 level tables [time, level]) of the box as it stands."""
    e, el = o.energy_contents(b)
    c, cl = o.conversion_terms(b)
    s = {**e, **c}
    lv = {**el, **cl}
    nt, nl = b.f["tair_ZE"].shape[:2]
    tab = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64), (nt, nl)) if np.ndim(a) == 1 else np.asarray(a, dtype=np.float64)
    return np.stack([np.asarray(s[k], dtype=np.float64) for k in TERMS]), np.stack([tab(lv[k]) for k in LEVEL_TERMS])


def spectrum_terms(dom: o.Domain, south, north, n_wave, dTdt=None):
    """(spectrum [time, 5, N], rest [time, 5], spectrum_levels [time, 14, N, level], totals [time, 5]) of the band [south, north] of the
    ring ``dom``: term order Ae, Ke, Ca, Ce, Ck; table order ``LEVEL_TERMS``."""
    with np.errstate(invalid="ignore"):
        b = rr.ring_box(dom, south, north, dTdt=dTdt)
        full = {k: b.f[k + "_ZE"] for k in EDDY}
        tot, _ = _terms(b)
        S, L = [], []
        for n in range(1, n_wave + 1):
            for k in EDDY:
                b.f[k + "_ZE"] = rr._close(wave_part(full[k][..., :-1], n))
            s, lv = _terms(b)
            S.append(s)
            L.append(lv)
        for k in EDDY:
            b.f[k + "_ZE"] = full[k]
    spec = np.stack(S, axis=-1).transpose(1, 0, 2)                    # [5, time, N] -> [time, 5, N]
    levels = np.stack(L, axis=0).transpose(2, 1, 0, 3)               # [N, 14, time, level] -> [time, 14, N, level]
    tot = tot.T
    return spec, tot - spec.sum(axis=2), levels, tot


def row_shares(T, u, v, w, n_wave):
    """[..., N, 8]: C_n of the eight covariances (slot order [T'T'] [u'u'] [v'v'] [v'T'] [w'T'] [u'v'] [w'u'] [w'v']) of rows along the
    last axis, from ``np.fft.rfft`` of the fp64 fields: C_n(a, b) = w_n Re(a^_n conj(b^_n)), a^ = rfft / nx, w_n = 2, or 1 at n = nx / 2."""
    nx = T.shape[-1]
    F = [np.fft.rfft(np.asarray(a, dtype=np.float64), axis=-1)[..., 1:n_wave + 1] / nx for a in (T, u, v, w)]
    wn = np.where(2 * np.arange(1, n_wave + 1) == nx, 1.0, 2.0)
    pairs = [(0, 0), (1, 1), (2, 2), (2, 0), (3, 0), (1, 2), (3, 1), (3, 2)]
    return np.stack([wn * np.real(F[a] * np.conj(F[b])) for a, b in pairs], axis=-1)
