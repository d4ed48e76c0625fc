"""The zonal-wavenumber spectrum of the generation term Ge on a ring (-f --periodic --wavenumbers N --wavenumbers-generation), restated
on the CPU from the oracle's own functions, in the way of tests/spectrum_restatement.py.  Nothing is restated here: Q is the ``Q`` of
``ring_restatement.ring_box`` (the oracle's ``adiabatic_heating`` on the wrapped axis), the wavenumber-n part of a field is
``spectrum_restatement.wave_part``, and with ``Q_ZE`` and ``tair_ZE`` of the box replaced by their wavenumber-n parts -- everything else,
sigma included, left as it is -- the oracle's ``generation_terms`` gives Ge(n) and its per-level table.  The zonal mean of the product
of the two single-wavenumber fields is the share C_n(Q, T) of DESIGN.md section 4.2b, so the N shares and the total close to rounding.
"""
from __future__ import annotations

import numpy as np

from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests.spectrum_restatement import wave_part


def row_shares_q(dom: o.Domain, south, north, n_wave):
    """[time, level, latitude, N]: C_n(Q, T) = w_n Re(Q^_n conj(T^_n)), a^ = rfft / nx, w_n = 2, or 1 at n = nx / 2, of every row of the
    band [south, north] of the ring ``dom``, from ``np.fft.rfft`` of the box's ``Q`` and ``tair`` (the ring's own nx columns)."""
    with np.errstate(invalid="ignore"):
        b = rr.ring_box(dom, south, north)
    Q, T = b.f["Q"][..., :-1], b.f["tair"][..., :-1]
    nx = T.shape[-1]
    FQ = np.fft.rfft(np.asarray(Q, dtype=np.float64), axis=-1)[..., 1:n_wave + 1] / nx
    FT = np.fft.rfft(np.asarray(T, dtype=np.float64), axis=-1)[..., 1:n_wave + 1] / nx
    wn = np.where(2 * np.arange(1, n_wave + 1) == nx, 1.0, 2.0)
    return wn * np.real(FQ * np.conj(FT))


def ge_terms(dom: o.Domain, south, north, n_wave):
    """(ge [time, N], rest [time], ge_levels [time, N, level], total [time]) of the band [south, north] of the ring ``dom``."""
    with np.errstate(invalid="ignore"):
        b = rr.ring_box(dom, south, north)
        full = {k: b.f[k + "_ZE"] for k in ("Q", "tair")}
        tot, _ = o.generation_terms(b)
        nt, nl = full["tair"].shape[:2]
        S, L = [], []
        for n in range(1, n_wave + 1):
            for k in full:
                b.f[k + "_ZE"] = rr._close(wave_part(full[k][..., :-1], n))
            s, lv = o.generation_terms(b)
            S.append(np.asarray(s["Ge"], dtype=np.float64))
            L.append(np.broadcast_to(np.asarray(lv["Ge"], dtype=np.float64), (nt, nl)))
        for k in full:
            b.f[k + "_ZE"] = full[k]
    ge = np.stack(S, axis=-1)                                   # [time, N]
    levels = np.stack(L, axis=1)                                # [time, N, level]
    total = np.asarray(tot["Ge"], dtype=np.float64)
    return ge, total - ge.sum(axis=1), levels, total
