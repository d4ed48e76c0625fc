"""The fixed framework on a full ring of longitudes (-f --periodic), restated on the CPU from the oracle's own functions.

The periodic evaluation is the reference's formulas on the CLOSED axis: column 0 appended once more at lon[nx - 1] + h, which gives
nx + 1 points and xlength = deg2rad(lon[nx - 1] + h) - deg2rad(lon[0]).  Nothing is restated here: Q is ``adiabatic_heating`` on the
fields extended by one wrap column on each side (its centred d/dlon is then the wrapped three-point difference at every column of the
ring, its one-sided ends fall on the two extension columns, which are cut away), every zonal mean, eddy field and product is
``zonal_average`` / ``area_average`` / ``static_stability`` on the closed axis -- whose trapezoid is h * sum over the nx columns --, and
``all_terms`` evaluates the four analysis classes on that ``Box``.  The east column of the closed axis is the west column, so every
east-minus-west difference of the boundary terms is exactly 0 without a special case.
"""
from __future__ import annotations

import numpy as np

from oracle import lec_oracle as o


def closed_axis(lon):
    """(h, the nx + 1 longitudes of the closed axis in degrees, xlength in radians)."""
    lon = np.asarray(lon, dtype=np.float64)
    h = (lon[-1] - lon[0]) / (lon.size - 1)
    closed = np.append(lon, lon[-1] + h)
    return h, closed, float(np.deg2rad(closed[-1]) - np.deg2rad(closed[0]))


def _wrap(X):
    """One wrap column on each side: [X[nx - 1], X[0], ..., X[nx - 1], X[0]]."""
    return np.concatenate([X[..., -1:], X, X[..., :1]], axis=-1)


def _close(X):
    """nx columns -> the closed axis' nx + 1 (column 0 once more)."""
    return np.concatenate([X, X[..., :1]], axis=-1)


def ring_box(dom: o.Domain, south, north, dTdt=None, with_geopt=True) -> o.Box:
    """The ``Box`` of the latitude band [south, north] over all of ``dom``'s longitudes, taken as a closed ring.  ``dTdt``: a dT/dt
    cube on ``dom``'s grid instead of np.gradient over ``dom.time_s``; ``with_geopt`` False: the geopotential is 0 everywhere (a call
    without a geopotential cube)."""
    js, jn = o.select_nearest(dom.lat, south), o.select_nearest(dom.lat, north)
    lat = dom.lat[js:jn + 1]
    rlats = np.deg2rad(lat)
    coslats = np.cos(np.deg2rad(lat))
    h, lon_c, xlength = closed_axis(dom.lon)
    rlons = np.deg2rad(lon_c)
    ylength = np.sin(rlats[-1]) - np.sin(rlats[0])
    band = lambda X: X[:, :, js:jn + 1, :]
    b = o.Box(rlats=rlats, rlons=rlons, coslats=coslats, lat=lat, lon=lon_c, level=dom.level, xlength=xlength, ylength=ylength,
              idx=(0, dom.lon.size - 1, js, jn))

    def add(name, X):
        ZA = o.zonal_average(X, rlons, xlength)
        AA = o.area_average(ZA, rlats, coslats)
        b.f[name] = X
        b.f[name + "_ZA"] = ZA
        b.f[name + "_AA"] = AA
        b.f[name + "_ZE"] = X - ZA[..., None]
        b.f[name + "_AE"] = ZA - AA[..., None]

    T, u, v, w = band(dom.tair), band(dom.u), band(dom.v), band(dom.omega)
    ph = band(dom.geopt) if with_geopt else np.zeros_like(T)
    for name, X in (("tair", T), ("u", u), ("v", v), ("omega", w), ("geopt", ph)):
        add(name, _close(X))
    # Q on the axis extended by one wrap column on each side, then cut to the ring's own nx columns
    lon_x = np.concatenate([[dom.lon[0] - h], np.asarray(dom.lon, dtype=np.float64), [dom.lon[-1] + h]])
    Qx = o.adiabatic_heating(_wrap(T), dom.level, _wrap(w), _wrap(u), _wrap(v), lat, lon_x, coslats, dom.time_s,
                             dTdt=None if dTdt is None else _wrap(band(dTdt)))
    add("Q", _close(Qx[..., 1:-1]))
    b.sigma_AA = o.static_stability(b.f["tair"], dom.level, rlats, rlons, coslats, xlength, ylength)
    return b


def ring_terms(dom: o.Domain, south, north, dTdt=None, with_geopt=True):
    """(scalars, level tables) of the periodic evaluation: ``all_terms`` on ``ring_box``."""
    return o.all_terms(ring_box(dom, south, north, dTdt=dTdt, with_geopt=with_geopt))


def ring_domain(nt, nl, ny, nx, seed=0, dtype=np.float64, lat0=-60.0, lat1=60.0, noise=0.1, level=None):
    """Smooth waves plus noise on a full ring: nx longitudes from -180 with nx * h = 360, ny latitudes lat0..lat1 (off the poles)."""
    rng = np.random.default_rng(seed)
    lat = np.linspace(lat0, lat1, ny)
    lon = -180.0 + 360.0 / nx * np.arange(nx)
    level = np.linspace(20000.0, 100000.0, nl) if level is None else np.asarray(level, dtype=np.float64)
    time_s = np.arange(nt) * 21600.0
    phi, lam = np.deg2rad(lat)[None, None, :, None], np.deg2rad(lon)[None, None, None, :]
    p = level[None, :, None, None] / 1e5
    tt = (np.arange(nt) / max(nt, 1))[:, None, None, None]
    shp = (nt, nl, ny, nx)
    n = lambda amp: noise * amp * rng.standard_normal(shp)
    T = 288.0 * p ** 0.19 + 10.0 * np.cos(2 * phi) * p + 4.0 * np.sin(2 * lam + tt) * np.cos(phi) + n(10.0)
    u = 25.0 * np.cos(phi) * (1.2 - p) + 6.0 * np.cos(lam - tt) + n(20.0)
    v = 5.0 * np.sin(2 * lam + 0.5) * np.cos(phi) + n(5.0)
    w = 0.2 * np.sin(lam + 2 * tt) * np.cos(phi) * p + n(0.2)
    ph = o.G * 7000.0 * np.log(1.0 / p) + 300.0 * np.cos(lam) * np.cos(phi) + n(300.0)
    f = [np.ascontiguousarray(a.astype(dtype)) for a in (T, u, v, w, ph)]
    return o.Domain(f[0], f[1], f[2], f[3], f[4], lat, lon, level, time_s)


def rolled(dom: o.Domain, k: int) -> o.Domain:
    """The same fields with the ring rotated by k columns (the longitude axis keeps its labels: a ring has no preferred meridian)."""
    r = lambda a: np.ascontiguousarray(np.roll(a, k, axis=-1))
    return o.Domain(r(dom.tair), r(dom.u), r(dom.v), r(dom.omega), r(dom.geopt), dom.lat, dom.lon, dom.level, dom.time_s)


RING_NAMELIST = (";Variable;Units\nAir Temperature;t;K\nGeopotential;z;m**2/s**2\nOmega Velocity;w;Pa/s\n"
                 "Eastward Wind Component;u;m/s\nNorthward Wind Component;v;m/s\nLongitude;longitude\nLatitude;latitude\n"
                 "Time;time\nVertical Level;level\n")


def write_ring_file(path, dom: o.Domain):
    """``dom`` (axes ascending, levels in Pa) as a classic NetCDF file the command line reads with ``RING_NAMELIST``: the fields in
    their own dtype (float64 or float32), the axes as doubles, levels in hPa, time in hours."""
    from scipy.io import netcdf_file
    nt, nl, ny, nx = dom.tair.shape
    code = "d" if dom.tair.dtype == np.float64 else "f"
    f = netcdf_file(path, "w", version=2)
    for n, s in (("time", nt), ("level", nl), ("latitude", ny), ("longitude", nx)):
        f.createDimension(n, s)
    tv = f.createVariable("time", "i", ("time",)); tv[:] = np.round(dom.time_s / 3600.0).astype(np.int32); tv.units = "hours since 2020-01-01 00:00:00"
    lv = f.createVariable("level", "d", ("level",)); lv[:] = dom.level / 100.0; lv.units = "millibars"
    la = f.createVariable("latitude", "d", ("latitude",)); la[:] = dom.lat
    lo = f.createVariable("longitude", "d", ("longitude",)); lo[:] = dom.lon
    for name, a in (("t", dom.tair), ("u", dom.u), ("v", dom.v), ("w", dom.omega), ("z", dom.geopt)):
        v = f.createVariable(name, code, ("time", "level", "latitude", "longitude"))
        v[:] = a
    f.close()


def cli_domain(nx=24, step=None, nt=4, seed=3) -> o.Domain:
    """The command-line tests' data: ``nx`` longitudes from -180 in steps of ``step`` degrees (default 360 / nx: a full ring), 7
    latitudes -45..45, the levels 300, 500, 700, 850, 1000 hPa, ``nt`` 6-hourly steps."""
    dom = ring_domain(nt, 5, 7, nx, seed=seed, lat0=-45.0, lat1=45.0, level=np.array([30000.0, 50000.0, 70000.0, 85000.0, 100000.0]))
    if step is not None:
        dom.lon = -180.0 + step * np.arange(nx)
    return dom
