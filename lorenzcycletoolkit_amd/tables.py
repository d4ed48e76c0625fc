"""Host-side coefficient tables consumed by the HIP kernels (layouts: include/lec_hip.h).

Everything here is O(nx + ny + nl + nt) NumPy fp64 work done once per call: trapezoid weights,
np.gradient coefficients for the box-local axes, the static-stability coefficients of the
diabatic-heating residual and the (level, lat) tables of stage 2.  The 4-D arithmetic itself
happens only in the kernels.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from .constants import KAPPA, P0_PA, RE, SPECTRUM_BUDGET_TERMS, SPECTRUM_RESIDUAL_TERMS, SPECTRUM_TENDENCY_TERMS, SPECTRUM_TERMS


def gradient_coefs(x: np.ndarray) -> np.ndarray:
    """(n, 3) coefficients a, b, c with d f/dx [i] = a f[i-1] + b f[i] + c f[i+1], equal to
    ``np.gradient(f, x, edge_order=1)`` (which DataArray.differentiate calls): second-order
    non-uniform interior, first-order one-sided ends.  Coefficients of missing neighbours are 0."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    if n < 2:
        raise ValueError("np.gradient needs at least 2 points along the axis")
    co = np.zeros((n, 3), dtype=np.float64)
    d = np.diff(x)
    if n > 2:
        dx1, dx2 = d[:-1], d[1:]
        co[1:-1, 0] = -dx2 / (dx1 * (dx1 + dx2))
        co[1:-1, 1] = (dx2 - dx1) / (dx1 * dx2)
        co[1:-1, 2] = dx1 / (dx2 * (dx1 + dx2))
    co[0, 1], co[0, 2] = -1.0 / d[0], 1.0 / d[0]
    co[-1, 0], co[-1, 1] = -1.0 / d[-1], 1.0 / d[-1]
    return co


def trapz_weights(x: np.ndarray) -> np.ndarray:
    """w with sum(w * f) == trapezoid integral of f over x (xarray ``integrate``)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.zeros_like(x)
    d = np.diff(x)
    w[:-1] += 0.5 * d
    w[1:] += 0.5 * d
    return w


def is_uniform(x: np.ndarray, rtol: float = 1e-12) -> bool:
    d = np.diff(np.asarray(x, dtype=np.float64))
    return bool(np.all(np.abs(d - d[0]) <= rtol * np.abs(d[0])))


def nearest_index(coord: np.ndarray, value: float) -> int:
    """``data[indexer].sel({indexer: value}, method="nearest")`` (box_data.py:133-135 of the
    reference): ties go to the larger label on an increasing index."""
    d = np.abs(np.asarray(coord, dtype=np.float64) - float(value))
    return int(np.flatnonzero(d == d.min())[-1])


def box_indices(lat_deg, lon_deg, west, east, south, north):
    """Inclusive grid-index box (iw, ie, js, jn) from geographic limits (box_data.py:115-131)."""
    iw, ie = nearest_index(lon_deg, west), nearest_index(lon_deg, east)
    js, jn = nearest_index(lat_deg, south), nearest_index(lat_deg, north)
    if ie - iw < 1 or jn - js < 1:
        raise ValueError(f"box [{west}, {east}] x [{south}, {north}] selects fewer than 2 grid points along an axis")
    return iw, ie, js, jn


@dataclass
class BoxTables:
    box: np.ndarray       # int32 [n_box, 4]
    boxtab: np.ndarray    # [n_box, 4]
    wlon: np.ndarray      # [n_box, nxb_max]
    glon: np.ndarray      # [n_box, nxb_max, 3]
    lattab: np.ndarray    # [n_box, nyb_max, 4]
    boxtab2: np.ndarray   # [n_box, 4]
    lattab2: np.ndarray   # [n_box, nyb_max, 8]
    nxb_max: int
    nyb_max: int
    lon_uniform: bool
    ring: bool = False    # one box whose columns are a full ring of longitudes: stage 1 is lec_rowstats_ring


def ring_axis(lon_deg: np.ndarray):
    """(h, xlength) of the CLOSED axis of a ring of longitudes: column 0 once more at lon[nx - 1] + h, h the axis' own step;
    xlength = deg2rad(lon[nx - 1] + h) - deg2rad(lon[0]) (box_data.py:128 on the closed axis)."""
    lon = np.asarray(lon_deg, dtype=np.float64)
    h = (lon[-1] - lon[0]) / (lon.size - 1)
    return h, float(np.deg2rad(lon[-1] + h) - np.deg2rad(lon[0]))


def twiddle_table(nx: int) -> np.ndarray:
    """[nx, 2] fp64: cos and sin of 2 pi m / nx for m = 0 .. nx - 1 -- the one source of the twiddles of ``lec_rowspec_ring``, which
    indexes it with (n i) mod nx as an integer (no recurrence and no device sincos: every lane reads the same correctly rounded pair
    for the same angle)."""
    nx = int(nx)
    if nx < 3:
        raise ValueError("a ring has at least 3 columns")
    ang = 2.0 * np.pi * np.arange(nx, dtype=np.float64) / nx
    return np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=1))


def build_box_tables(lat_deg: np.ndarray, lon_deg: np.ndarray, boxes: Sequence[Sequence[int]], nyb_min: int = 0,
                     lon_uniform: Optional[bool] = None, ring: bool = False) -> BoxTables:
    """Per-box tables for both stages.  ``boxes`` = inclusive index quadruples (iw, ie, js, jn).
    ``nyb_min``: pad the latitude extent of the tables (and of the row records) to at least this many rows -- chunks of one
    series of moving boxes share one record buffer, whose row count is the tallest box of the whole series.
    ``lon_uniform``: the formulation's flag as decided on ANOTHER longitude axis than ``lon_deg`` -- a track of a batch (batch.py) keeps
    the flag of its own crop while its boxes are addressed in the union crop; None = decided on ``lon_deg`` (the default everywhere
    else).  True needs every box's longitudes evenly spaced.
    ``ring``: ONE box over the whole longitude axis, which is a full ring (``follow.ring_error``): ``boxtab`` / ``boxtab2`` carry the
    closed axis' xlength (``ring_axis``), h_rad = xlength / nx and 1 / h_deg for ``lec_rowstats_ring``; ``wlon`` / ``glon`` stay 0 (unused)."""
    lat = np.asarray(lat_deg, dtype=np.float64)
    lon = np.asarray(lon_deg, dtype=np.float64)
    box = np.asarray(boxes, dtype=np.int32).reshape(-1, 4)
    nb = box.shape[0]
    if np.any(box[:, 0] < 0) or np.any(box[:, 1] >= lon.size) or np.any(box[:, 2] < 0) or np.any(box[:, 3] >= lat.size):
        raise ValueError("box indices outside the grid")
    if ring:
        from .follow import ring_error
        why = ring_error(lon)
        if why:
            raise ValueError("a periodic box needs a full ring of longitudes: " + why)
        if nb != 1 or int(box[0, 0]) != 0 or int(box[0, 1]) != lon.size - 1:
            raise ValueError(f"a periodic box is ONE box over the whole longitude axis (columns 0..{lon.size - 1}), not columns "
                             + ", ".join(f"{int(b[0])}..{int(b[1])}" for b in box) + ": a periodic box of part of a circle does not exist")
        if lon_uniform is False:
            raise ValueError("a ring of longitudes is evenly spaced: lon_uniform cannot be False")
    nxb = box[:, 1] - box[:, 0] + 1
    nyb = box[:, 3] - box[:, 2] + 1
    if np.any(nxb < 2) or np.any(nyb < 2):
        raise ValueError("every box needs at least 2 grid points along lat and lon")
    nxm, nym = int(nxb.max()), max(int(nyb.max()), int(nyb_min))
    if nym > lat.size:
        raise ValueError("nyb_min exceeds the grid")
    t = BoxTables(box=box, boxtab=np.zeros((nb, 4)), wlon=np.zeros((nb, nxm)), glon=np.zeros((nb, nxm, 3)),
                  lattab=np.zeros((nb, nym, 4)), boxtab2=np.zeros((nb, 4)), lattab2=np.zeros((nb, nym, 8)),
                  nxb_max=nxm, nyb_max=nym, lon_uniform=True if ring else (is_uniform(lon) if lon_uniform is None else bool(lon_uniform)),
                  ring=bool(ring))
    if lon_uniform and not all(is_uniform(lon[int(b[0]): int(b[1]) + 1]) for b in box):
        raise ValueError("lon_uniform: a box's longitudes are not evenly spaced")
    # (lon_uniform selects the kernels' fast path and is decided on the grid's whole longitude axis, not on the boxes at hand: a
    # chunk or shard of a moving series may hold only boxes that happen to lie in an evenly spaced part of a stretched grid -- any
    # two-point-wide box does -- and must still use the formulation the whole series uses, or it differs from it by an ulp;
    # tests/soak_gpu.py found exactly that.)
    inv_dy = 1.0 / (np.deg2rad(1.0) * RE)      # dy = deg2rad(d lat/d lat) Re, thermodynamics.py:102
    cache = {}
    for b in range(nb):
        iw, ie, js, jn = (int(v) for v in box[b])
        key = (iw, ie, js, jn)
        if key in cache:                         # a stationary track repeats its box
            src = cache[key]
            for arr in (t.boxtab, t.wlon, t.glon, t.lattab, t.boxtab2, t.lattab2):
                arr[b] = arr[src]
            continue
        cache[key] = b
        lo, la = lon[iw:ie + 1], lat[js:jn + 1]
        rlon, rlat = np.deg2rad(lo), np.deg2rad(la)
        xlen = rlon[-1] - rlon[0]                                  # box_data.py:128
        ylen = np.sin(rlat[-1]) - np.sin(rlat[0])                  # box_data.py:129-131
        n = lo.size
        if ring:                                                   # the closed axis: n intervals of h, every column weight 1
            h, xlen = ring_axis(lo)
            t.boxtab[b] = (1.0 / xlen, xlen / n, n / ((lo[-1] + h) - lo[0]), 0.0)
        else:
            t.boxtab[b] = (1.0 / xlen, xlen / (n - 1), (n - 1) / (lo[-1] - lo[0]), 0.0)
            t.wlon[b, :n] = trapz_weights(rlon)
            t.glon[b, :n] = gradient_coefs(lo)
        m = la.size
        cosl = np.cos(rlat)
        t.lattab[b, :m, :3] = gradient_coefs(la) * inv_dy
        t.lattab[b, :m, 3] = 1.0 / (np.deg2rad(1.0) * cosl * RE)  # 1/dx, thermodynamics.py:101
        wphi = trapz_weights(rlat)
        t.boxtab2[b] = (-1.0 / (RE * xlen * ylen), -1.0 / (RE * ylen), xlen, ylen)   # boundary_terms.py:122-123
        t.lattab2[b, :m, 0] = cosl * wphi / ylen
        t.lattab2[b, :m, 1] = wphi
        t.lattab2[b, :m, 2] = cosl
        t.lattab2[b, :m, 3] = np.tan(rlat)
        t.lattab2[b, :m, 4:7] = gradient_coefs(rlat)
        t.lattab2[b, m:, 2] = 1.0                                   # keeps padded rows finite
    return t


def level_tables(level_pa: np.ndarray):
    """levtab [nl, 3]: S = -(T/theta) d theta/dp = al T[k-1] + be T[k] + ga T[k+1] with
    theta = T (P0/p)^kappa (thermodynamics.py:107-117); levtab2 [nl, 4]: p and d/dp coefficients."""
    p = np.asarray(level_pa, dtype=np.float64)
    if p.size < 2 or np.any(np.diff(p) <= 0):
        raise ValueError("levels must be ascending pressures in Pa (at least 2)")
    gc = gradient_coefs(p)
    ex = (p / P0_PA) ** KAPPA
    levtab = np.zeros((p.size, 3))
    levtab[1:, 0] = -ex[1:] * gc[1:, 0] / ex[:-1]
    levtab[:, 1] = -gc[:, 1]
    levtab[:-1, 2] = -ex[:-1] * gc[:-1, 2] / ex[1:]
    levtab2 = np.concatenate([p[:, None], gc], axis=1)
    return levtab, levtab2


def time_coefs(time_s: np.ndarray) -> np.ndarray:
    """[nt, 3] np.gradient coefficients over the time axis in seconds (thermodynamics.py:109-110)."""
    return gradient_coefs(np.asarray(time_s, dtype=np.float64))


def pressure_coefs(level_pa: np.ndarray) -> np.ndarray:
    """ptab [nl, 3] of ``lec_rowspec_nl_ring``: np.gradient(edge_order=1) coefficients over the level axis in Pa, one-sided at the top
    and bottom level; one level has no pressure derivative: all 0."""
    p = np.asarray(level_pa, dtype=np.float64)
    if p.size < 2:
        return np.zeros((p.size, 3), dtype=np.float64)
    return gradient_coefs(p)


def nl_lat_table(lattab: np.ndarray, lat_deg: np.ndarray) -> np.ndarray:
    """The [nyb, 5] latitude table of ``lec_rowspec_nl_ring``: the four columns of the ring box's ``lattab`` (d/dlat a, b, c; 1 / dx_j:
    what ``lec_rowspec_q_ring`` takes) and m_j = tan(lat_j) / Re, the metric factor of the advection of u and v -- 0 on a pole row,
    where the curvature terms have no meaning (and 1 / dx_j is whatever the box's table carries)."""
    lat = np.asarray(lat_deg, dtype=np.float64)
    lattab = np.asarray(lattab, dtype=np.float64)
    if lattab.shape != (lat.size, 4):
        raise ValueError("nl_lat_table: lattab must be the band's [nyb, 4] table")
    out = np.empty((lat.size, 5), dtype=np.float64)
    out[:, :4] = lattab
    out[:, 4] = np.where(np.abs(lat) >= 90.0, 0.0, np.tan(np.deg2rad(lat)) / RE)
    return out


def budgets_and_residuals(scalars: dict, time_s: np.ndarray, residuals: bool = True) -> dict:
    """Budget (dX/dt by np.gradient with dt = t[1]-t[0]) and residual columns of the results CSV
    (calc_budget_and_residual.py:32-56,131-154 of the reference).  O(nt) host work on the gathered
    per-time scalars."""
    dt = float(time_s[1] - time_s[0])
    out = dict(scalars)
    for term in ("Az", "Ae", "Kz", "Ke"):
        out[f"∂{term}/∂t (finite diff.)"] = np.gradient(np.asarray(scalars[term], dtype=np.float64), dt)
    if residuals:
        out["RGz"] = out["∂Az/∂t (finite diff.)"] + out["Cz"] + out["Ca"] - out["BAz"]
        out["RKz"] = out["∂Kz/∂t (finite diff.)"] - out["Cz"] - out["Ck"] - out["BKz"]
        out["RGe"] = out["∂Ae/∂t (finite diff.)"] - out["Ca"] + out["Ce"] - out["BAe"]
        out["RKe"] = out["∂Ke/∂t (finite diff.)"] - out["Ce"] + out["Ck"] - out["BKe"]
    return out


def spectrum_budgets(spectrum: np.ndarray, spectrum_rest: np.ndarray, spectrum_b: np.ndarray, spectrum_b_rest: np.ndarray,
                     time_s: np.ndarray) -> dict:
    """The per-wavenumber budget of the eddy reservoirs: ``spectrum`` [time, 5, N] (Ae, Ke, Ca, Ce, Ck of SPECTRUM_TERMS) and
    ``spectrum_b`` [time, 2, N] (BAe, BKe) with their ``rest`` columns -> ``tendency`` [time, 2, N] (dAe(n)/dt, dKe(n)/dt),
    ``residual`` [time, 2, N] (RGe(n), RKe(n)) and ``tendency_rest`` / ``residual_rest`` [time, 2].  Every column -- a wavenumber or
    the rest -- goes through ``budgets_and_residuals``, the function that forms the totals' budget, with the zonal reservoir's terms 0:
    np.gradient with dt = time_s[1] - time_s[0], RGe = dAe/dt - Ca + Ce - BAe, RKe = dKe/dt - Ce + Ck - BKe.  Linear, so the columns and
    the rest sum to the totals' figures to rounding."""
    spectrum, spectrum_b = np.asarray(spectrum, dtype=np.float64), np.asarray(spectrum_b, dtype=np.float64)
    nt, _, n = spectrum.shape
    if nt < 2 or np.asarray(time_s).size < 2:
        raise ValueError("the tendencies are finite differences in time: at least 2 time steps")
    cols = np.concatenate([spectrum, np.asarray(spectrum_rest, dtype=np.float64)[:, :, None]], axis=2)
    bcols = np.concatenate([spectrum_b, np.asarray(spectrum_b_rest, dtype=np.float64)[:, :, None]], axis=2)
    tend, resid = np.empty((nt, 2, n + 1)), np.empty((nt, 2, n + 1))
    zero = np.zeros(nt)
    for i in range(n + 1):
        col = {term: cols[:, k, i] for k, term in enumerate(SPECTRUM_TERMS)}
        col.update({term: bcols[:, k, i] for k, term in enumerate(SPECTRUM_BUDGET_TERMS)})
        col.update({term: zero for term in ("Az", "Kz", "Cz", "BAz", "BKz")})
        out = budgets_and_residuals(col, time_s, residuals=True)
        for k, term in enumerate(SPECTRUM_TENDENCY_TERMS):
            tend[:, k, i] = out[f"∂{term}/∂t (finite diff.)"]
        for k, term in enumerate(SPECTRUM_RESIDUAL_TERMS):
            resid[:, k, i] = out[term]
    return {"tendency": tend[:, :, :n], "tendency_rest": tend[:, :, n], "residual": resid[:, :, :n], "residual_rest": resid[:, :, n]}
