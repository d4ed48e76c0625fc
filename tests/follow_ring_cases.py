"""The grid and the planted systems that tests/test_follow_ring_cpu.py and tests/test_gpu_follow_ring.py share -- TEST INFRASTRUCTURE ONLY.

33 latitudes (-80 .. 0 by 2.5 degrees), a ring of 72 longitudes (-180 .. 175 by 5 degrees), 12 time steps; a box of 10 x 10 degrees and
a search radius of 15 degrees: sj = 6, si = 3."""
import numpy as np

LAT = -80.0 + 2.5 * np.arange(33)
LON = -180.0 + 5.0 * np.arange(72)
NT = 12
BOX = dict(length=10.0, width=10.0, search=15.0)
SJ, SI = 6, 3


def ring_dx(x, xc):
    """x - xc in degrees on the ring, in [-180, 180)."""
    return (x - xc + 180.0) % 360.0 - 180.0


def planted(seed, x_start, speed, rival_lon, nt=NT, lon=LON, lat=LAT, blind_step=None):
    """As test_gpu_follow.planted, on the ring: a vortex (and a height low) moving along a known path -- from longitude ``x_start``,
    ``speed`` degrees east per step (negative: west), 0.5 degrees south per step from 40 S -- over noise, plus a rival twice as strong
    that stays at (55 S, ``rival_lon``), far beyond the search radius and far from the seam.  Southern hemisphere: cyclonic = negative vorticity.
    -> (u, v, h [nt][ny][nx], start (lat, lon), the path's longitudes [nt] in [-180, 180))."""
    rng = np.random.default_rng(seed)
    y, x = lat[None, :, None], lon[None, None, :]
    t = np.arange(nt)[:, None, None]
    y0, x0 = -40.0 - 0.5 * t, x_start + speed * t
    yr, xr = -55.0, rival_lon

    def vortex(yc, xc, amp, sigma=7.0):
        dy, dx = y - yc, ring_dx(x, xc)
        g = np.exp(-(dx * dx + dy * dy) / (2 * sigma * sigma))
        return amp * dy * g, -amp * dx * g, g                        # u, v: dv/dx - du/dy = -2 amp at the centre

    u1, v1, g1 = vortex(y0, x0, 6.0)
    u2, v2, g2 = vortex(yr, xr, 12.0)
    shape = (nt, lat.size, lon.size)
    u = u1 + u2 + 0.3 * rng.standard_normal(shape)
    v = v1 + v2 + 0.3 * rng.standard_normal(shape)
    h = 1500.0 - 80.0 * g1 - 160.0 * g2 + 2.0 * rng.standard_normal(shape)
    if blind_step is not None:
        for a in (u, v, h):
            a[blind_step] = np.nan
    path = ring_dx(x0[:, 0, 0], 0.0)
    return u, v, h, (float(y0[0, 0, 0]), float(path[0])), path


def start_of(start, lat=LAT, lon=LON):
    """(j, i) of the grid point nearest (lat, lon), nearest measured on the ring."""
    d = np.abs(ring_dx(lon, start[1]))
    return int(np.argmin(np.abs(lat - start[0]))), int(np.argmin(d))


EAST = dict(x_start=166.0, speed=2.3, rival_lon=-90.0)          # columns 69 .. 71, 0 .. 2
WEST = dict(x_start=-168.5, speed=-2.3, rival_lon=-90.0)        # and the other way
INTERIOR = dict(x_start=-30.0, speed=2.3, rival_lon=60.0)      # mid-domain: no tile touches column 0 or nx - 1
