"""The latitude x pressure sections of the ten terms of the cycle (-f [--periodic] --sections), restated on the CPU
from the oracle's 4-D fields.  Nothing of the kernel is restated here: a section is the zonal average, on the box's own axis rule
(``oracle.zonal_average`` with the box's ``rlons`` / ``xlength``: the open trapezoid of ``oracle.make_box``, the closed axis of
``ring_restatement.ring_box``), of the very integrand that ``oracle.energy_contents`` / ``conversion_terms`` / ``generation_terms`` hand to
``area_average``, with the oracle's ``sigma_AA``.  ``area_average`` is linear in its argument, so the sections close on the oracle's own
per-level tables, and their columns -- ``oracle.trapz`` over the finite levels -- on its scalars.

Order of the terms: Az Ae Kz Ke Cz Ca Ck Ce Gz Ge (``TERMS``).  Spectral sections (a ring): the eddy fields replaced by their wavenumber-n
parts, as tests/spectrum_restatement.py and tests/spectrum_ge_restatement.py do for the totals; order Ae Ke Ca Ce Ck (Ge).
"""
from __future__ import annotations

import numpy as np

from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests.spectrum_restatement import wave_part

TERMS = ["Az", "Ae", "Kz", "Ke", "Cz", "Ca", "Ck", "Ce", "Gz", "Ge"]
SPEC_TERMS = ["Ae", "Ke", "Ca", "Ce", "Ck", "Ge"]
# C_f = COLUMN_SCALE[f] * integral of X_f dp: the factor the oracle applies to the term's pressure integral
COLUMN_SCALE = {"Kz": 1.0 / (2 * o.G), "Ke": 1.0 / (2 * o.G), "Ck": 1.0 / o.G}


def sections(b: o.Box) -> np.ndarray:
    """X [time, 10, level, lat] of the box as it stands."""
    f = b.f
    s3 = b.sigma_AA[:, :, None]
    s4 = b.sigma_AA[:, :, None, None]
    za = lambda X: o.zonal_average(X, b.rlons, b.xlength)
    c3 = lambda c: c[None, None, :]
    c4 = lambda c: c[None, None, :, None]
    c1 = (o.RD / (b.level * o.G))[None, :, None]
    out = {}
    # energy_contents
    out["Az"] = f["tair_AE"] ** 2 / (2 * s3)
    out["Ae"] = za(f["tair_ZE"] ** 2) / (2 * s3)
    out["Kz"] = f["u_ZA"] ** 2 + f["v_ZA"] ** 2
    out["Ke"] = za(f["u_ZE"] ** 2 + f["v_ZE"] ** 2)
    # conversion_terms
    dphi_tae = o.differentiate(f["tair_AE"] * c3(b.coslats), b.rlats, axis=2)
    t1 = (f["v_ZE"] * f["tair_ZE"] * dphi_tae[..., None]) / (2 * o.RE * s4)
    dp_tae = o.differentiate(f["tair_AE"], b.level, axis=1)
    t2 = (f["omega_ZE"] * f["tair_ZE"]) * dp_tae[..., None]
    out["Ca"] = -(za(t1) + za(t2) / s3)
    out["Ce"] = -(c1 * za(f["omega_ZE"] * f["tair_ZE"]))
    out["Cz"] = -(c1 * (f["omega_AE"] * f["tair_AE"]))
    tan_lats = np.tan(b.rlats)
    d1 = o.differentiate(f["u_ZA"] / c3(b.coslats), b.rlats, axis=2)
    d2 = o.differentiate(f["v_ZA"], b.rlats, axis=2)
    d4 = o.differentiate(f["u_ZA"], b.level, axis=1)
    out["Ck"] = (za((c4(b.coslats) * f["u_ZE"] * f["v_ZE"] / o.RE) * d1[..., None]) + za(((f["v_ZE"] ** 2) / o.RE) * d2[..., None])
                 + za((c4(tan_lats) * (f["u_ZE"] ** 2) * f["v_ZA"][..., None]) / o.RE) + za(f["omega_ZE"] * f["u_ZE"] * d4[..., None])
                 + za(f["omega_ZE"] * f["v_ZE"] * d4[..., None]))          # term 5 with d[u]/dp, as the oracle has it
    # generation_terms
    out["Gz"] = f["Q_AE"] * f["tair_AE"] / (o.CP_D * s3)
    out["Ge"] = za(f["Q_ZE"] * f["tair_ZE"]) / (o.CP_D * s3)
    return np.stack([np.asarray(out[k], dtype=np.float64) for k in TERMS], axis=1)


def columns(X: np.ndarray, level: np.ndarray, terms=TERMS) -> np.ndarray:
    """C [time, F, lat] of X [time, F, level, lat]: per (t, f, j) the trapezoid over the FINITE levels -- interior gaps are bridged
    linearly in p (a trapezoid between the two finite neighbours is that), NaN levels at either end are left out, no finite level
    gives NaN -- times the term's scale."""
    nt, nf, nl, ny = X.shape
    C = np.full((nt, nf, ny), np.nan)
    p = np.asarray(level, dtype=np.float64)
    for t in range(nt):
        for f in range(nf):
            for j in range(ny):
                y = X[t, f, :, j]
                ok = ~np.isnan(y)
                if ok.any():
                    C[t, f, j] = o.trapz(y[ok], p[ok], axis=0) * COLUMN_SCALE.get(terms[f], 1.0)
    return C


def time_mean(X: np.ndarray) -> np.ndarray:
    """(1 / T) sum_t X[t], summed in time order; NaN at any step gives NaN."""
    s = np.array(X[0], dtype=np.float64, copy=True)
    for t in range(1, X.shape[0]):
        s = s + X[t]
    return s / X.shape[0]


def area_weights(b: o.Box) -> np.ndarray:
    """cw [lat] with sum_j cw_j X_j = ``oracle.area_average`` of X: the trapezoid weights of cos(phi) X over ``rlats``, over ylength."""
    eye = np.eye(b.rlats.size)[:, None, :]                              # [which, 1, lat]: area_average runs over axis 2
    return o.area_average(eye, b.rlats, b.coslats)[:, 0]


def spectral_sections(b: o.Box, n_wave: int, generation: bool = False) -> np.ndarray:
    """X^n [time, F, N, level, lat] of a ring's box, F = 5 (Ae Ke Ca Ce Ck) or 6 (Ge too): the sections of the box whose eddy fields
    (and Q's, with ``generation``) are replaced by their wavenumber-n parts.  The box is left as it was."""
    names = ["tair", "u", "v", "omega"] + (["Q"] if generation else [])
    nf = 6 if generation else 5
    idx = [TERMS.index(k) for k in SPEC_TERMS[:nf]]
    full = {k: b.f[k + "_ZE"] for k in names}
    out = []
    try:
        for n in range(1, n_wave + 1):
            for k in names:
                b.f[k + "_ZE"] = rr._close(wave_part(full[k][..., :-1], n))
            out.append(sections(b)[:, idx])
    finally:
        for k in names:
            b.f[k + "_ZE"] = full[k]
    return np.stack(out, axis=2)


def spectral_columns_mean(b: o.Box, n_wave: int, generation: bool = False, total_columns=None) -> np.ndarray:
    """[F, N + 1, lat]: the time mean of the column value of X_f^n for n = 1 .. N, then the rest (the total's minus the N shares')."""
    nf = 6 if generation else 5
    Xn = spectral_sections(b, n_wave, generation)
    shares = np.stack([time_mean(columns(Xn[:, :, n], b.level, SPEC_TERMS[:nf])) for n in range(n_wave)], axis=1)      # [F, N, lat]
    if total_columns is None:
        total_columns = columns(sections(b), b.level)
    tot = time_mean(total_columns[:, [TERMS.index(k) for k in SPEC_TERMS[:nf]]])
    return np.concatenate([shares, (tot - shares.sum(axis=1))[:, None]], axis=1)
