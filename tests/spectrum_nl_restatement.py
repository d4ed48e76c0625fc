"""The non-linear eddy-eddy (triad) transfers S(n) and L(n) on a ring (-f --periodic --wavenumbers N --wavenumbers-interactions), restated
on the CPU from the oracle's own functions, in the way of tests/spectrum_restatement.py and tests/spectrum_ge_restatement.py.

The fields are those of ``ring_restatement.ring_box``.  The eddy-eddy advective tendencies
    A_T = u' D_lambda T + v' D_phi T' + w' D_p T'
    A_u = u' D_lambda u + v' D_phi u' + w' D_p u' - (tan phi / a) u' v'
    A_v = u' D_lambda v + v' D_phi v' + w' D_p v' + (tan phi / a) u' u'
are formed with ``np.roll`` over the ring's nx columns for the zonal derivative and ``np.gradient(edge_order=1)`` over the band's
latitudes and the levels for the other two (the derivative of an eddy is the derivative of the field minus that of its zonal mean); the
eddies are taken against ``mean(axis=-1)`` of the nx columns.  Ae is linear in [T'T'] and Ke in [u'u'] + [v'v'], and the change of
[x'x'] / 2 by the advection is -[A_x' x'], so S(n) is the oracle's Ae operator -- ``area_average`` over the closed axis, / (2 sigma),
``_handle_nans`` and the pressure integral, as ``energy_contents`` combines them -- on -2 wave_part(A_T, n) wave_part(T, n) in the place
of tair_ZE ** 2, and L(n) its Ke operator on -2 (wave_part(A_u, n) wave_part(u, n) + wave_part(A_v, n) wave_part(v, n)): route 1,
``nl_terms``.  Route 2, ``nl_terms_polarised``, goes through the unchanged ``energy_contents`` itself by polarisation,
E[a b] = (E[((c a + b) / 2) ** 2] - E[((c a - b) / 2) ** 2]) / c; tests/test_spectrum_nl_cpu.py checks one against the other.
"""
from __future__ import annotations

import numpy as np

from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests.spectrum_restatement import wave_part

TERMS = ["S", "L"]


def tendencies(dom: o.Domain, south, north):
    """(box, eddies [T', u', v'], tendencies [A_T, A_u, A_v]) of the band [south, north] of the ring ``dom``; every field
    [time, level, latitude, nx] on the ring's own nx columns.  With one level the pressure derivative vanishes (and the box is None)."""
    if np.size(dom.level) > 1:
        with np.errstate(invalid="ignore"):
            b = rr.ring_box(dom, south, north)
        T, u, v, w = (np.asarray(b.f[k][..., :-1], dtype=np.float64) for k in ("tair", "u", "v", "omega"))
        lat = b.lat
    else:       # one level: the oracle's box needs two for its static stability; the band's fields themselves, and no box
        b = None
        js, jn = o.select_nearest(dom.lat, south), o.select_nearest(dom.lat, north)
        T, u, v, w = (np.asarray(a[:, :, js:jn + 1], dtype=np.float64) for a in (dom.tair, dom.u, dom.v, dom.omega))
        lat = dom.lat[js:jn + 1]
    lat = np.asarray(lat, dtype=np.float64)
    level = np.asarray(dom.level, dtype=np.float64)
    h = rr.closed_axis(dom.lon)[0]
    dx = (np.deg2rad(1.0) * np.cos(np.deg2rad(lat)) * o.RE)[None, None, :, None]
    dy = np.deg2rad(1.0) * o.RE
    m = (np.tan(np.deg2rad(lat)) / o.RE)[None, None, :, None]
    zm = lambda X: X.mean(axis=-1, keepdims=True)
    d_lam = lambda X: (np.roll(X, -1, axis=-1) - np.roll(X, 1, axis=-1)) / (2.0 * h) / dx
    g_phi = lambda X: np.gradient(X, lat, axis=2, edge_order=1) / dy
    g_p = lambda X: np.gradient(X, level, axis=1, edge_order=1) if level.size > 1 else np.zeros_like(X)
    with np.errstate(invalid="ignore"):
        e_phi = lambda X: g_phi(X) - g_phi(zm(X))
        e_p = lambda X: g_p(X) - g_p(zm(X))
        Tp, up, vp, wp = T - zm(T), u - zm(u), v - zm(v), w - zm(w)
        adv = lambda X: up * d_lam(X) + vp * e_phi(X) + wp * e_p(X)
        A_T = adv(T)
        A_u = adv(u) - m * up * vp
        A_v = adv(v) + m * up * up
    return b, [Tp, up, vp], [A_T, A_u, A_v]


def planted_domain(nx, waves, nt=3, nl=4, ny=5):
    """Zonal means of ``ring_domain`` without noise plus eddies of the wavenumbers ``waves`` alone (the construction of
    tests/test_gpu_spectrum_ge.test_planted_wave, one wave per entry)."""
    base = rr.ring_domain(nt, nl, ny, nx, seed=5, lat0=-60.0, lat1=60.0, noise=0.0)
    lam = np.deg2rad(base.lon)[None, None, None, :]
    phi = np.deg2rad(base.lat)[None, None, :, None]
    p = base.level[None, :, None, None] / 1e5
    tt = (np.arange(nt) / nt)[:, None, None, None]
    zm = lambda a: a.mean(axis=-1, keepdims=True)
    wave = lambda amp, ph: sum(amp / (1 + q) * np.cos(m * lam + ph + 0.9 * q + 0.3 * p + tt) * np.cos(phi) for q, m in enumerate(waves))
    f = [np.ascontiguousarray(zm(a) + w) for a, w in ((base.tair, wave(4.0, 0.0)), (base.u, wave(6.0, 0.7)), (base.v, wave(5.0, 1.9)),
                                                     (base.omega, wave(0.2, 2.6)))]
    return o.Domain(f[0], f[1], f[2], f[3], base.geopt, base.lat, base.lon, base.level, base.time_s)


def row_shares(dom: o.Domain, south, north, n_wave):
    """(shares [time, level, latitude, N, 3], totals [time, level, latitude, 3]): -2 C_n(A_x, x) and the same for the whole eddy
    covariance, -2 (mean(A_x x') - mean(A_x) mean(x')), x = T, u, v; C_n(a, b) = w_n Re(a^_n conj(b^_n)), a^ = rfft / nx, w_n = 2, or 1
    at n = nx / 2."""
    _, X, A = tendencies(dom, south, north)
    nx = X[0].shape[-1]
    wn = np.where(2 * np.arange(1, n_wave + 1) == nx, 1.0, 2.0)
    S, Tt = [], []
    with np.errstate(invalid="ignore"):
        for x, a in zip(X, A):
            Fx = np.fft.rfft(x, axis=-1)[..., 1:n_wave + 1] / nx
            Fa = np.fft.rfft(a, axis=-1)[..., 1:n_wave + 1] / nx
            S.append(-2.0 * wn * np.real(Fa * np.conj(Fx)))
            Tt.append(-2.0 * ((a * x).mean(axis=-1) - a.mean(axis=-1) * x.mean(axis=-1)))
    return np.stack(S, axis=-1), np.stack(Tt, axis=-1)


def _operators(b, pT, pK):
    """The oracle's Ae operator on ``pT`` in the place of tair_ZE ** 2 and its Ke operator on ``pK`` in the place of
    u_ZE ** 2 + v_ZE ** 2 (both on the closed axis): (S, L [time], their tables [time, level]) -- oracle/lec_oracle.py:286-296."""
    s = b.sigma_AA
    lvS = o.area_average(pT, b.rlats, b.coslats, b.xlength, b.rlons) / (2 * s)
    lvL = o.area_average(pK, b.rlats, b.coslats, b.xlength, b.rlons)
    S = o._int_p(lvS, b.level)
    L = o._int_p(lvL, b.level) / (2 * o.G)
    return S, L, o.handle_nans_table(lvS, b.level), o.handle_nans_table(lvL, b.level)


def _stack(parts, tot):
    nl_ = np.stack([np.stack([p[0], p[1]], axis=1) for p in parts], axis=-1)               # [time, 2, N]
    levels = np.stack([np.stack([p[2], p[3]], axis=1) for p in parts], axis=2)             # [time, 2, N, level]
    total = np.stack([tot[0], tot[1]], axis=1)                                             # [time, 2]
    return nl_, total - nl_.sum(axis=2), levels, total


def nl_terms(dom: o.Domain, south, north, n_wave):
    """Route 1.  (nl [time, 2, N], rest [time, 2], levels [time, 2, N, level], total [time, 2]) of the band [south, north] of the ring
    ``dom``; order S, L; the total is formed in physical space."""
    b, X, A = tendencies(dom, south, north)
    with np.errstate(invalid="ignore"):
        ed = [x - x.mean(axis=-1, keepdims=True) for x in X]
        an = [a - a.mean(axis=-1, keepdims=True) for a in A]
        tot = _operators(b, rr._close(-2.0 * an[0] * ed[0]), rr._close(-2.0 * (an[1] * ed[1] + an[2] * ed[2])))
        parts = []
        for n in range(1, n_wave + 1):
            wx = [wave_part(x, n) for x in X]
            wa = [wave_part(a, n) for a in A]
            parts.append(_operators(b, rr._close(-2.0 * wa[0] * wx[0]), rr._close(-2.0 * (wa[1] * wx[1] + wa[2] * wx[2]))))
    return _stack(parts, tot)


def _pow2(a, b):
    """The power of two that brings c a to b's size."""
    ma, mb = np.nanmax(np.abs(a)), np.nanmax(np.abs(b))
    return 1.0 if not (ma > 0 and mb > 0) else float(2.0 ** np.round(np.log2(mb / ma)))


def nl_terms_polarised(dom: o.Domain, south, north, n_wave):
    """Route 2.  (nl [time, 2, N], levels [time, 2, N, level]) through the unchanged ``energy_contents``:
    E[a b] = (E[((c a + b) / 2) ** 2] - E[((c a - b) / 2) ** 2]) / c with tair_ZE (for S) and u_ZE, v_ZE (for L) of the box replaced."""
    b, X, A = tendencies(dom, south, north)
    full = {k: b.f[k + "_ZE"] for k in ("tair", "u", "v")}
    nt, nlev = full["tair"].shape[:2]
    tab = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64), (nt, nlev))
    S, L = [], []
    with np.errstate(invalid="ignore"):
        for n in range(1, n_wave + 1):
            wx = [wave_part(x, n) for x in X]
            wa = [wave_part(a, n) for a in A]
            cT = _pow2(wa[0], wx[0])
            cK = _pow2(np.stack(wa[1:]), np.stack(wx[1:]))
            got = []
            for sign in (1.0, -1.0):
                b.f["tair_ZE"] = rr._close((cT * wa[0] + sign * wx[0]) / 2)
                b.f["u_ZE"] = rr._close((cK * wa[1] + sign * wx[1]) / 2)
                b.f["v_ZE"] = rr._close((cK * wa[2] + sign * wx[2]) / 2)
                got.append(o.energy_contents(b))
            (sp, lp), (sm, lm) = got
            S.append(np.stack([-2.0 * (sp["Ae"] - sm["Ae"]) / cT, -2.0 * (sp["Ke"] - sm["Ke"]) / cK], axis=1))
            L.append(np.stack([-2.0 * (tab(lp["Ae"]) - tab(lm["Ae"])) / cT, -2.0 * (tab(lp["Ke"]) - tab(lm["Ke"])) / cK], axis=1))
    for k in full:
        b.f[k + "_ZE"] = full[k]
    return np.stack(S, axis=-1), np.stack(L, axis=2)
