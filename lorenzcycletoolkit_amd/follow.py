"""-c/--choose without a display: the box of every time step follows the 850-hPa system, on the GPU.

The reference's ``-c`` is a matplotlib click loop (src/utils/select_area.py:158-251 there): per time step it draws the 850-hPa
vorticity, height and wind, circles the vorticity minimum of the current box (``plot_min_zeta``, select_area.py:106-155) and waits
for the user to drag the next box; ``get_limits`` turns the clicks into that step's limits (lec_moving_framework.py:227-245).  The
engine runs on nodes without a display, so the loop closes itself: the extremum of step t inside a search window around the
centre of step t - 1 becomes the centre of step t (``lec_follow``, csrc/lec_follow.hip: one workgroup walks the steps).  The
result is written as a track file in the reference's format, and ``-c`` is then, by definition, ``-t`` on that track.

The rule (include/lec_hip.h has the device's half):

* field: ``zeta`` -- the 850-hPa relative vorticity ``lec_track_diag`` evaluates, on the search domain's coordinates, in the
  formulation of ``--vorticity-form`` -- or ``hgt`` (geopotential height, gpm); optionally the mean over (2 r + 1)^2 grid points;
* sense: the minimum for ``hgt``; for ``zeta`` the minimum in the southern hemisphere, the maximum in the northern (hemisphere:
  ``south`` when the search domain's southern edge is below the equator -- lec_moving_framework.py:340's rule -- unless given);
* admissible centres: grid points whose box lies inside the search domain's coordinate range (``admissible``);
* window: the admissible centres within ``search`` degrees (in grid steps, ``window_steps``) of the previous centre; step 0: of the
  grid point nearest ``start``, or every admissible centre.

Nothing in the reference pins this (its chooser's boxes are a person's clicks): restatement only (tests/follow_restatement.py).
There is no CPU path, like ``diagnostics.device_extrema``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pandas as pd

from . import _lib
from . import dataset as ds
from .constants import G
from .diagnostics import vorticity_tables

FIELDS = ("zeta", "hgt")
HEMISPHERES = ("south", "north")
DEFAULT_BOX = (15.0, 15.0)              # length, width in degrees: the reference's default box (lec_moving_framework.py:224-225)
DEFAULT_SEARCH = 5.0                    # degrees per time step


def admissible(lat, lon, length, width, periodic=False) -> tuple:
    """(jlo, jhi, ilo, ihi): inclusive index bounds of the grid points whose box (lat +- length / 2, lon +- width / 2) lies inside the
    coordinate range of the (sorted, possibly stretched) axes.  A box larger than the domain is refused.  ``periodic``: the longitudes
    are a ring -- every column is a centre (0, nx - 1); the latitude half is the same."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    jj = np.flatnonzero((lat - length / 2 >= lat[0]) & (lat + length / 2 <= lat[-1]))
    ii = np.arange(lon.size) if periodic else np.flatnonzero((lon - width / 2 >= lon[0]) & (lon + width / 2 <= lon[-1]))
    if jj.size == 0 or ii.size == 0:
        raise ValueError(f"a box of {length} x {width} degrees (length x width) does not fit into the search domain of "
                         f"{float(lat[-1] - lat[0])} x {float(lon[-1] - lon[0])} degrees (lat {float(lat[0])}..{float(lat[-1])}, "
                         f"lon {float(lon[0])}..{float(lon[-1])}): no grid point can be its centre")
    return int(jj[0]), int(jj[-1]), int(ii[0]), int(ii[-1])


def ring_error(lon):
    """None when the sorted longitudes are a full ring -- evenly spaced with nx * dx = 360 degrees, both to within 1e-6 dx -- else the
    sentence that says what they are instead (--choose-periodic refuses with it)."""
    lon = np.asarray(lon, dtype=np.float64)
    d = np.diff(lon)
    dx = float(np.median(d))
    extent = f"the search domain's longitudes run from {float(lon[0])} to {float(lon[-1])} in {lon.size} columns"
    if not (dx > 0 and np.all(np.abs(d - dx) <= 1e-6 * dx)):
        return f"{extent}, unevenly spaced: no ring"
    if abs(lon.size * dx - 360.0) > 1e-6 * dx:
        return f"{extent} of {dx} degrees = {lon.size * dx} degrees, not the 360 of a full ring"
    return None


def ring_distance(a, b, nx):
    """|a - b| on a ring of nx columns (arrays or ints); nx None: the plain distance."""
    d = np.abs(np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64))
    return d if nx is None else np.minimum(d % nx, nx - d % nx)


def window_steps(lat, lon, search) -> tuple:
    """(sj, si): the largest move per time step in grid points, max(1, floor(search / median |spacing|)) per axis."""
    step = lambda x: max(1, int(np.floor(search / np.median(np.abs(np.diff(np.asarray(x, dtype=np.float64)))))))
    return step(lat), step(lon)


def start_index(lat, lon, start, bounds, periodic=False) -> tuple:
    """The grid point nearest (LAT, LON) (the first of two equally near ones), clamped into the admissible centres.  ``periodic``: the
    longitudes are a ring, nearest is measured on it."""
    jlo, jhi, ilo, ihi = bounds
    j = int(np.argmin(np.abs(np.asarray(lat, dtype=np.float64) - float(start[0]))))
    di = np.abs(np.asarray(lon, dtype=np.float64) - float(start[1]))
    i = int(np.argmin(np.minimum(di % 360.0, 360.0 - di % 360.0) if periodic else di))
    return min(max(j, jlo), jhi), min(max(i, ilo), ihi)


def sense_of(field, hemisphere, lat) -> tuple:
    """(hemisphere, LEC_FOLLOW_MIN / LEC_FOLLOW_MAX) after the default rule."""
    if field not in FIELDS:
        raise ValueError(f"field must be one of {FIELDS}, not {field!r}")
    if hemisphere is None:
        hemisphere = "south" if float(np.asarray(lat)[0]) < 0 else "north"
    if hemisphere not in HEMISPHERES:
        raise ValueError(f"hemisphere must be one of {HEMISPHERES}, not {hemisphere!r}")
    return hemisphere, (_lib.FOLLOW_MIN if field == "hgt" or hemisphere == "south" else _lib.FOLLOW_MAX)


def follow_system(u850, v850, hgt850, lat, lon, *, length=DEFAULT_BOX[0], width=DEFAULT_BOX[1], search=DEFAULT_SEARCH, smooth=0,
                  field="zeta", hemisphere=None, start=None, formulation="metpy_no_crs", device="cuda:0"):
    """``lec_follow`` on [time, lat, lon] slices of the search domain (host arrays or device tensors; ``hgt850`` may be None unless the
    field is ``hgt``): (pos [nt][2] grid indices of every step's centre, val [nt] the (smoothed) field there, status [nt]: 1 where
    the window held no finite value and the centre was kept) as NumPy arrays.  Raises ValueError when the box does not fit into
    the domain (before any GPU work) and when the first step finds nothing."""
    import torch
    if not search > 0:
        raise ValueError(f"search must be > 0 degrees, not {search!r}")
    s = _Slices(u850, v850, hgt850, lat, lon, 3, length=length, width=width, smooth=smooth, field=field, hemisphere=hemisphere,
                formulation=formulation, device=device)
    sj, si = window_steps(s.lat, s.lon, search)
    js, is_ = (-1, -1) if start is None else start_index(s.lat, s.lon, start, s.bounds)
    nt = int(s.u.shape[0])
    pos = torch.empty((nt, 2), dtype=torch.int32, device=s.dev)
    val = torch.empty((nt,), dtype=torch.float64, device=s.dev)
    status = torch.empty((nt,), dtype=torch.int32, device=s.dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = _lib.FollowArgs(nt=nt, sj=sj, si=si, j_start=js, i_start=is_, pos_d=ptr(pos), val_d=ptr(val), status_d=ptr(status), **s.common())
    with torch.cuda.device(s.dev):
        _lib.check(s.lib.lec_follow(C.byref(args)), "lec_follow")
    pos, val, status = pos.cpu().numpy(), val.cpu().numpy(), status.cpu().numpy()
    if status[0]:
        raise ValueError("the first time step's search window holds no finite value of the field: nothing to follow "
                         "(another --choose-start or --choose-domain?)")
    return pos, val, status


def write_track(path, time, lat_c, lon_c, length, width) -> str:
    """A track file in the reference's format (``time;Lat;Lon;length;width``, time as YYYY-MM-DD-HHMM).  ``length`` / ``width``:
    scalars or one value per step.  Every number is written as its shortest decimal form that identifies the double (``repr``).
    ``dataset.read_track`` reads with the reference's parser (pandas' default), which gives back the identical double for every
    coordinate of a grid in binary fractions of a degree (2.5, 1, 0.5, 0.25, 0.125 ...: every sample, NCEP, ERA5) but cannot
    produce about one double in twelve of full length at all (a stretched axis): such a coordinate comes back within 1e-12 degrees,
    and the analysis -- of this run and of any later ``-t`` run on the file alike -- uses what the reader reads."""
    stamps = pd.DatetimeIndex(np.asarray(time)).strftime("%Y-%m-%d-%H%M")
    n = len(stamps)
    cols = [np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)) for a in (lat_c, lon_c, length, width)]
    if not all(np.all(np.isfinite(c)) for c in cols):
        raise ValueError("a track holds finite numbers only")
    cols = [[repr(float(x)) for x in c] for c in cols]
    with open(path, "w") as f:
        f.write("time;Lat;Lon;length;width\n")
        for row in zip(stamps, *cols):
            f.write(";".join(row) + "\n")
    return str(path)


class _SliceSource:
    """The 85000-Pa slices of u, v and geopotential height (gpm) of ``args.infile`` on the search domain, opened once and read by ranges
    of time steps: ``lat``, ``lon``, ``time`` are the whole series', ``read((a, b))`` gives (u, v, hgt [b - a][ny][nx] float64)."""

    def __init__(self, args, varlist="inputs/namelist", app_logger=None):
        variable_list_df = ds.read_namelist(varlist, app_logger)
        mpas = bool(getattr(args, "mpas", False))
        self.geo_role = "Geopotential" if "Geopotential" in variable_list_df.index else "Geopotential Height"
        self.roles = ("Eastward Wind Component", "Northward Wind Component", self.geo_role)
        self.app_logger, self.raw, self.data, self.told = app_logger, None, None, False

        def crop(px):
            k = np.flatnonzero(px.level == 85000.0)
            if k.size == 0:
                raise KeyError(85000)                           # as -t: lec_moving_framework.py:653-657 selects 85000 Pa exactly
            jj, ii = np.arange(px.lat.size), np.arange(px.lon.size)
            if getattr(args, "choose_domain", None):
                w, e, s, n = ds.read_box_limits(args.choose_domain)
                jj = np.flatnonzero((px.lat >= s) & (px.lat <= n))
                ii = np.flatnonzero((px.lon >= w) & (px.lon <= e))
            if jj.size < 3 or ii.size < 3:
                raise ValueError("the search domain selects fewer than 3 x 3 grid points of the data")
            return int(k[0]), jj, ii

        try:
            raw = ds.open_raw(ds.series_paths(args, varlist), variable_list_df, mpas=mpas, app_logger=app_logger)
        except ValueError as e:
            if "order" not in str(e) and "device ingest reads" not in str(e):
                raise
            self.data = data = ds.open_dataset(ds.series_paths(args, varlist), variable_list_df, mpas=mpas)  # another dimension order: the whole file
            px = ds._sorted_axes(None, data.lat, data.lon, data.level, data.time, data.level_units, data.names, app_logger)
            k, jj, ii = crop(px)
            self.sel = (px.ik[k], px.ij[jj], px.io[ii])
            lat, lon, time = px.lat[jj], px.lon[ii], px.time
        else:
            self.raw = raw
            try:
                px = ds._sorted_axes(None, raw.lat, raw.lon, raw.level, raw.time, raw.level_units, raw.names, app_logger)
                k, jj, ii = crop(px)
                i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
                self.plan = ds.IngestPlan(np.arange(raw.time.size), i32(px.ik[k: k + 1]), i32(px.ij[jj]), i32(px.io[ii]), px.lat[jj], px.lon[ii],
                                          px.level[k: k + 1], px.time)
            except BaseException:
                raw.close()
                raise
            lat, lon, time = self.plan.lat, self.plan.lon, self.plan.time
        self.lat, self.lon, self.time = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64), time
        self.periodic = bool(getattr(args, "choose_periodic", False))
        if self.periodic and ring_error(self.lon):
            self.close()
            raise ValueError("--choose-periodic needs a search domain that is a full ring of longitudes: " + ring_error(self.lon)
                             + " (--choose-domain may cut latitudes only)")

    def read(self, t_range=None):
        """(u, v, hgt) of the time steps [a, b) (None: all)."""
        if self.raw is None:
            if t_range is not None and not self.told and self.app_logger is not None:
                self.app_logger.info("-c/--choose: this file's dimension order takes the whole-file reader: reading the 850-hPa slices in "
                                     "chunks bounds the GPU's memory, it does not save host memory for this file")
                self.told = True
            steps = slice(None) if t_range is None else slice(int(t_range[0]), int(t_range[1]))
            ik, ij, io = self.sel
            get = lambda role: self.data.variables[self.data.names[role]][steps][:, ik][:, ij][:, :, io].astype(np.float64)
            u, v, g = (get(r) for r in self.roles)
        else:
            u, v, g = (ds.gather_on_host(self.raw.variables[self.raw.names[r]], self.plan, t_range)[:, 0].astype(np.float64) for r in self.roles)
        return u, v, (g if self.geo_role == "Geopotential Height" else g / G)      # -> gpm, as diagnostics.track_diagnostics

    def close(self):
        if self.raw is not None:
            self.raw.close()
            self.raw = None


def search_domain_slices(args, varlist="inputs/namelist", app_logger=None, t_range=None):
    """The 85000-Pa slices of u, v and geopotential height (gpm) of ALL time steps of ``args.infile`` on the search domain
    (``args.choose_domain``: a box-limits file, label slices; default: the file's whole domain), with sorted axes:
    (u, v, hgt [nt][ny][nx] float64, lat, lon, time).  Only that level and that domain are read from the file.
    ``t_range`` (a, b): u, v and hgt hold the time steps [a, b) only, and only those are read; lat, lon and time are the whole
    series' either way.  (A file in another dimension order is opened whole: there the range bounds nothing on the host.)"""
    src = _SliceSource(args, varlist, app_logger)
    try:
        u, v, hgt = src.read(t_range)
    finally:
        src.close()
    return u, v, hgt, src.lat, src.lon, src.time


SLICE_BYTES = 2 << 30                   # the 850-hPa slices held at a time (host, and again on the device): a memory bound, not a tuned figure


def slice_chunks(nt, ny, nx, asked=None, budget=SLICE_BYTES) -> list:
    """[(a, b)]: the consecutive ranges of time steps whose slices (u, v, hgt: 24 bytes per grid point and step) a -c run holds at a
    time.  ``asked`` (--choose-chunk N): chunks of N steps, the last one shorter.  Without it: ONE chunk when the whole series fits
    ``budget`` bytes, else the largest equal chunks that fit (a single step that does not fit is still a chunk)."""
    nt = int(nt)
    if nt < 1:
        raise ValueError("no time steps")
    if asked is not None:
        if asked != int(asked) or int(asked) < 1:
            raise ValueError(f"a chunk is a whole number of time steps >= 1, not {asked!r}")
        size = min(int(asked), nt)
    else:
        per_step = 24 * int(ny) * int(nx)
        most = max(1, int(budget) // per_step)                           # steps that fit
        n_chunks = -(-nt // most)
        size = -(-nt // n_chunks)                                         # equal chunks: no short tail beyond rounding
    return [(a, min(a + size, nt)) for a in range(0, nt, size)]


def write_choose_track(args, results_subdirectory, app_logger, varlist="inputs/namelist", device="cuda:0") -> str:
    """Phase A of a ``-c`` run: slices -> ``follow_system`` -> ``<results>/<stem>_choose_track``.  Returns the track's path."""
    length, width = (float(x) for x in (getattr(args, "choose_box", None) or DEFAULT_BOX))
    search = float(getattr(args, "choose_search", None) or DEFAULT_SEARCH)
    smooth = int(getattr(args, "choose_smooth", None) or 0)
    field = getattr(args, "choose_field", None) or "zeta"
    form = getattr(args, "vorticity_form", None) or "metpy_no_crs"
    start = getattr(args, "choose_start", None)
    src = _SliceSource(args, varlist, app_logger)
    try:
        lat, lon, time = src.lat, src.lon, src.time
        pos, val, status = _choose_track_chains(args, app_logger, src, length, width, search, smooth, field, form, start, device)
    finally:
        src.close()
    for t in np.flatnonzero(status):
        app_logger.warning(f"-c/--choose: no finite value of {field} in the search window of {pd.Timestamp(time[t])}: the box stays where it was")
    stem = os.path.basename(args.infile).split(".nc")[0]
    lat_c, lon_c = lat[pos[:, 0]], lon[pos[:, 1]]
    path = write_track(os.path.join(results_subdirectory, f"{stem}_choose_track"), time, lat_c, lon_c, length, width)
    back = ds.read_track(path)
    off = max(float(np.max(np.abs(back["Lat"].values - lat_c))), float(np.max(np.abs(back["Lon"].values - lon_c))))
    if off > 0:
        app_logger.warning(f"-c/--choose: the track reader's parser (pandas' default, as in the reference) reads some centres up to {off:.1e} "
                           "degrees beside the grid's coordinates; the analysis uses them as read, as a -t run on this file does")
    app_logger.info(f"-c/--choose: track written to {path} (a track file: -t --trackfile {path} repeats this run, --gpus N included)")
    return path


def _log_chunks(app_logger, chunks, ny, nx, how):
    n = chunks[0][1] - chunks[0][0]
    app_logger.info(f"-c/--choose: the 850-hPa slices are read and uploaded in {len(chunks)} chunks of {n} time steps ({24 * n * ny * nx} bytes a chunk, "
                    f"on the host and again on the GPU); {how}")


def _resume_chunks(src, chunks, pos, val, status, starts, *, search, device, **kw):
    """The chunks after the first of a plain or --choose-systems run.  pos [K][n0][2], val, status [K][n0]: what lec_follow / lec_follow_many
    gave on the first chunk; starts [K][2]: the chains' starts.  Every chain goes on from the centre of the first chunk's last step
    through ``lec_follow_spans_chunk`` with patience 0 (it never stops) -> the arrays over the whole series."""
    import torch
    K = len(pos)
    start = np.zeros((K, 3), dtype=np.int32)
    start[:, 1:] = starts
    state = np.zeros((K, 8), dtype=np.int32)
    for c in range(K):
        if status[c, 0] != _lib.FOLLOW_BAD_START:             # (a bad start is found again by the kernel, from its entry of the table)
            state[c] = (1, pos[c, -1, 0], pos[c, -1, 1], 0, -1, -1, 0, 0)
    start_d, state_d = torch.as_tensor(start).to(device), torch.as_tensor(state).to(device)
    pos, val, status = [pos], [val], [status]
    for a, b in chunks[1:]:
        u, v, hgt = src.read((a, b))
        p, x, st, _ = follow_spans_chunk(u, v, hgt, src.lat, src.lon, starts=start_d, state=state_d, t_base=a, patience=0, search=search, device=device, **kw)
        del u, v, hgt
        pos.append(p); val.append(x); status.append(st)
    return np.concatenate(pos, axis=1), np.concatenate(val, axis=1), np.concatenate(status, axis=1)


def _seam_notes(app_logger, src, names, last_i, si):
    """Without --choose-periodic, on a domain that IS a ring: one line per chain whose last good step lies within si columns of either
    edge -- it may have ended at the seam, not with its system.  last_i: per chain the column of that step, None: no good step."""
    if src.periodic or ring_error(src.lon):
        return
    nx = src.lon.size
    for name, i in zip(names, last_i):
        if i is not None and (i <= si or i >= nx - 1 - si):
            app_logger.info(f"-c/--choose: {name}: its last good time step lies within {si} grid steps of the domain's edge at the +-180 meridian, and "
                            "the domain is a full ring of longitudes -- the chain may have ended at the seam: --choose-periodic (it follows a system across it)")


def _last_good_columns(pos, status):
    """Per chain of pos [K][nt][2], status [K][nt]: the column of the last step with status 0, or None."""
    out = []
    for c in range(len(pos)):
        good = np.flatnonzero(np.asarray(status[c]) == 0)
        out.append(int(pos[c][good[-1]][1]) if good.size else None)
    return out


def _ring_chains(src, chunks, first, seeds, *, search, device, **kw):
    """The chains of a plain, --choose-systems or --choose-starts run on a ring (--choose-periodic): every chunk, the first included, goes
    through ``lec_follow_spans_chunk_ring`` with every t0 = 0 and patience 0 -- the resumed form of lec_follow_many (include/lec_hip.h).
    first: the first chunk's slices, already read; seeds [K][2].  -> (pos [K][nt][2], val [K][nt], status [K][nt])."""
    import torch
    K = len(seeds)
    start = np.zeros((K, 3), dtype=np.int32)
    start[:, 1:] = seeds
    start_d = torch.as_tensor(start).to(device)
    state_d = torch.zeros((K, 8), dtype=torch.int32, device=device)
    pos, val, status = [], [], []
    for n, (a, b) in enumerate(chunks):
        u, v, hgt = first if n == 0 else src.read((a, b))
        first = None
        p, x, st, _ = follow_spans_chunk(u, v, hgt, src.lat, src.lon, starts=start_d, state=state_d, t_base=a, patience=0, search=search, device=device,
                                         periodic=True, **kw)
        del u, v, hgt
        pos.append(p); val.append(x); status.append(st)
    return np.concatenate(pos, axis=1), np.concatenate(val, axis=1), np.concatenate(status, axis=1)


def _ring_start(app_logger, u, v, hgt, lat, lon, time, start, *, length, width, device, **kw):
    """The start of a plain -c run on a ring: the grid point nearest --choose-start, or -- the ring call has no "whole domain" step --
    seed 0 of step 0 (k_max 1, no threshold), logged."""
    if start is not None:
        return start_index(lat, lon, start, admissible(lat, lon, length, width, True), periodic=True)
    seed_pos, seed_val, n_found = find_systems_series(u[:1], v[:1], None if hgt is None else hgt[:1], lat, lon, k=1, length=length, width=width,
                                                      device=device, periodic=True, **kw)
    if n_found[0] == 0:
        raise ValueError("--choose-periodic: the first time step holds no system to start from: give --choose-start LAT LON")
    j, i = (int(x) for x in seed_pos[0, 0])
    app_logger.info(f"-c/--choose: --choose-periodic without --choose-start: the start is the strongest system of {pd.Timestamp(time[0])} "
                    f"(lec_follow_seeds_series_ring, seed 0: {seed_val[0, 0]} at lat {lat[j]}, lon {lon[i]})")
    return j, i


def _choose_track_chains(args, app_logger, src, length, width, search, smooth, field, form, start, device):
    """write_choose_track's chain: (pos [nt][2], val [nt], status [nt]) over the whole series."""
    chunks, u, v, hgt = _first_chunk(args, src)
    lat, lon, time = src.lat, src.lon, src.time
    hemisphere, sense = sense_of(field, getattr(args, "choose_hemisphere", None), lat)
    sj, si = window_steps(lat, lon, search)
    if src.periodic:
        kw = dict(smooth=smooth, field=field, hemisphere=hemisphere, formulation=form)
        seed = _ring_start(app_logger, u, v, hgt, lat, lon, time, start, length=length, width=width, device=device, **kw)
        app_logger.info(f"-c/--choose: following the 850 hPa {'minimum' if sense == _lib.FOLLOW_MIN else 'maximum'} of {field} "
                        f"({hemisphere}ern hemisphere" + (f", vorticity formulation '{form}'" if field == "zeta" else "") + f") on the GPU across the +-180 "
                        f"meridian (--choose-periodic: lec_follow_spans_chunk_ring in {len(chunks)} chunk(s)): {len(time)} time steps, search domain lat "
                        f"{lat[0]}..{lat[-1]}, a ring of {lon.size} longitudes, box {length} x {width} degrees (length x width), at most {search} degrees "
                        f"= {sj} x {si} grid steps per time step, smoothing radius {smooth}, start lat {lat[seed[0]]}, lon {lon[seed[1]]}")
        pos, val, status = (a[0] for a in _ring_chains(src, chunks, (u, v, hgt), np.array([seed], dtype=np.int32), search=search, device=device,
                                                       length=length, width=width, **kw))
        if status[0]:
            raise ValueError("the first time step's search window holds no finite value of the field: nothing to follow "
                             "(another --choose-start or --choose-domain?)")
        return pos, val, status
    app_logger.info(f"-c/--choose: following the 850 hPa {'minimum' if sense == _lib.FOLLOW_MIN else 'maximum'} of {field} "
                    f"({hemisphere}ern hemisphere" + (f", vorticity formulation '{form}'" if field == "zeta" else "") + f") on the GPU (lec_follow): "
                    f"{len(time)} time steps, search domain lat {lat[0]}..{lat[-1]}, lon {lon[0]}..{lon[-1]} ({lat.size} x {lon.size} points), "
                    f"box {length} x {width} degrees (length x width), at most {search} degrees = {sj} x {si} grid steps per time step, "
                    f"smoothing radius {smooth}, start {'the extremum of the whole domain' if start is None else tuple(start)}")
    if len(chunks) > 1:
        _log_chunks(app_logger, chunks, lat.size, lon.size, "the first chunk goes through lec_follow, every later one resumes the chain "
                    "(lec_follow_spans_chunk)")
    kw = dict(length=length, width=width, smooth=smooth, field=field, hemisphere=hemisphere, formulation=form)
    pos, val, status = follow_system(u, v, hgt, lat, lon, search=search, start=start, device=device, **kw)
    if len(chunks) > 1:
        del u, v, hgt
        pos, val, status = (a[0] for a in _resume_chunks(src, chunks, pos[None], val[None], status[None], pos[None, 0], search=search, device=device, **kw))
    _seam_notes(app_logger, src, ["the chain"], _last_good_columns(pos[None], status[None]), si)
    return pos, val, status


# ---------------------------------------------------------------------------------------------------------------------------
# several systems in one run: lec_follow_seeds finds them at the first time step, lec_follow_many follows them in one launch
# ---------------------------------------------------------------------------------------------------------------------------
def separation_steps(lat, lon, sep_lat, sep_lon) -> tuple:
    """(ej, ei): the half-extent of a seed's neighbourhood in grid points, max(1, floor(sep / median |spacing|)) per axis (as
    ``window_steps``, with a separation of its own per axis)."""
    return window_steps(lat, lon, sep_lat)[0], window_steps(lat, lon, sep_lon)[1]


def read_starts(path) -> np.ndarray:
    """[n][2] (lat, lon) from a ``Lat;Lon`` file (other columns are ignored), read with the track reader's parser (pandas' default,
    ``dataset.read_track``): what ``write_track`` wrote comes back as a track's centres do."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"Starts file not found: {path}")
    with open(path) as f:
        first = f.readline().strip()
    delim = ";" if ";" in first else ","
    cols = [c.strip() for c in first.split(delim)]
    missing = [c for c in ("Lat", "Lon") if c not in cols]
    if missing:
        raise ValueError(f"Starts file missing required columns: {missing}\nExpected: ['Lat', 'Lon']\nFound: {cols}")
    table = pd.read_csv(path, delimiter=delim)
    out = np.c_[table["Lat"].values.astype(np.float64), table["Lon"].values.astype(np.float64)]
    if out.shape[0] < 1 or not np.all(np.isfinite(out)):
        raise ValueError(f"Starts file {path}: needs at least one row, finite numbers only")
    return out


class _Slices:
    """What lec_follow, lec_follow_seeds and lec_follow_many share: the checked options, the slices and the vorticity tables on the device."""

    def __init__(self, u, v, h, lat, lon, ndim, *, length, width, smooth, field, hemisphere, formulation, device, periodic=False):
        import torch
        self.lat, self.lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
        if smooth != int(smooth) or int(smooth) < 0:
            raise ValueError(f"smooth must be a whole number of grid points >= 0, not {smooth!r}")
        self.smooth, self.field = int(smooth), field
        self.hemisphere, self.sense = sense_of(field, hemisphere, self.lat)
        if periodic and ring_error(self.lon):
            raise ValueError("the ring calls need a full ring of longitudes: " + ring_error(self.lon))
        self.bounds = admissible(self.lat, self.lon, length, width, periodic)
        if field == "hgt" and h is None:
            raise ValueError("field 'hgt' needs the geopotential height slices")
        tables = vorticity_tables(self.lat, self.lon, formulation, periodic=periodic)
        self.lib = _lib.load()
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise _lib.LecLibraryError("the system is followed on the GPU: there is no CPU path")
        up = lambda a: (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a))).to(device=self.dev, dtype=torch.float64).contiguous()
        self.u, self.v = up(u), up(v)
        self.h = None if h is None else up(h)
        if self.u.dim() != ndim or self.v.shape != self.u.shape or (self.h is not None and self.h.shape != self.u.shape):
            raise ValueError("u, v and height must be " + ("[time, lat, lon] slices" if ndim == 3 else "[lat, lon] slices") + " of one shape")
        if tuple(self.u.shape[-2:]) != (self.lat.size, self.lon.size):
            raise ValueError("slices and coordinates do not match")
        self.tables = [torch.as_tensor(t).to(self.dev) for t in tables]

    def common(self):
        ptr = lambda t: C.c_void_p(t.data_ptr())
        import torch
        return dict(u_d=ptr(self.u), v_d=ptr(self.v), hgt_d=None if self.h is None else ptr(self.h), ny=self.lat.size, nx=self.lon.size,
                    field=_lib.FOLLOW_HGT if self.field == "hgt" else _lib.FOLLOW_ZETA, xcoef_d=ptr(self.tables[0]), ycoef_d=ptr(self.tables[1]),
                    curv_d=ptr(self.tables[2]), sense=self.sense, smooth_r=self.smooth, jlo=self.bounds[0], jhi=self.bounds[1],
                    ilo=self.bounds[2], ihi=self.bounds[3], stream=C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))


def find_systems(u0, v0, h0, lat, lon, *, k, threshold=None, separation=None, length=DEFAULT_BOX[0], width=DEFAULT_BOX[1], smooth=0,
                 field="zeta", hemisphere=None, formulation="metpy_no_crs", device="cuda:0"):
    """``lec_follow_seeds`` on ONE [lat, lon] slice (the first time step): (pos [n][2] grid indices, val [n]) of the at most ``k``
    systems the rule of include/lec_hip.h finds, best first (n may be 0).  ``threshold``: in the field's own unit and sign, None: none.
    ``separation``: (degrees of latitude, degrees of longitude) within which a system tolerates no better one; default: half the box."""
    import torch
    if k != int(k) or not 1 <= int(k) <= 256:
        raise ValueError(f"k must be a whole number of systems, 1..256, not {k!r}")
    sep = (length / 2, width / 2) if separation is None else tuple(float(x) for x in separation)
    if len(sep) != 2 or not min(sep) > 0:
        raise ValueError(f"separation must be two positive numbers of degrees (latitude, longitude), not {separation!r}")
    s = _Slices(u0, v0, h0, lat, lon, 2, length=length, width=width, smooth=smooth, field=field, hemisphere=hemisphere,
                formulation=formulation, device=device)
    ej, ei = separation_steps(s.lat, s.lon, *sep)
    work = torch.empty((s.lat.size, s.lon.size), dtype=torch.float64, device=s.dev)
    pos = torch.empty((int(k), 2), dtype=torch.int32, device=s.dev)
    val = torch.empty((int(k),), dtype=torch.float64, device=s.dev)
    n = torch.empty((1,), dtype=torch.int32, device=s.dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = _lib.FollowSeedsArgs(ej=ej, ei=ei, k_max=int(k), threshold=float("nan") if threshold is None else float(threshold),
                                work_d=ptr(work), seed_pos_d=ptr(pos), seed_val_d=ptr(val), n_found_d=ptr(n), **s.common())
    with torch.cuda.device(s.dev):
        _lib.check(s.lib.lec_follow_seeds(C.byref(args)), "lec_follow_seeds")
    n = int(n.cpu().numpy()[0])
    pos, val = pos.cpu().numpy(), val.cpu().numpy()
    if not (np.all(pos[n:] == -2) and np.all(np.isnan(val[n:]))):
        raise _lib.LecLibraryError("lec_follow_seeds: the unused entries are not marked")
    return pos[:n], val[:n]


def follow_systems(u850, v850, hgt850, lat, lon, *, starts=None, seeds=None, length=DEFAULT_BOX[0], width=DEFAULT_BOX[1],
                   search=DEFAULT_SEARCH, smooth=0, field="zeta", hemisphere=None, formulation="metpy_no_crs", device="cuda:0"):
    """``lec_follow_many``: K chains over [time, lat, lon] slices in one launch -> (pos [K][nt][2], val [K][nt], status [K][nt]).
    Exactly one of ``starts`` -- K entries, each (lat, lon) (through ``start_index``) or None (the extremum of the whole domain) --
    and ``seeds`` -- [K][2] grid indices as ``find_systems`` returns them (a host array or a device tensor), handed to the kernel as
    they are: an entry that is no admissible centre gives status ``FOLLOW_BAD_START`` at every step.  Chain c is ``follow_system``
    from that start, bit for bit; unlike it, nothing is raised for a chain whose first step finds nothing (status[c, 0] = 1)."""
    import torch
    if (starts is None) == (seeds is None):
        raise ValueError("follow_systems needs either starts or seeds")
    if not search > 0:
        raise ValueError(f"search must be > 0 degrees, not {search!r}")
    s = _Slices(u850, v850, hgt850, lat, lon, 3, length=length, width=width, smooth=smooth, field=field, hemisphere=hemisphere,
                formulation=formulation, device=device)
    sj, si = window_steps(s.lat, s.lon, search)
    if starts is not None:
        seeds = np.array([(-1, -1) if st is None else start_index(s.lat, s.lon, st, s.bounds) for st in starts], dtype=np.int32).reshape(-1, 2)
    start_d = (seeds if isinstance(seeds, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(seeds, dtype=np.int32))).to(device=s.dev, dtype=torch.int32).contiguous()
    if start_d.dim() != 2 or start_d.shape[1] != 2 or start_d.shape[0] < 1:
        raise ValueError("starts / seeds: needs at least one (j, i) pair")
    K, nt = int(start_d.shape[0]), int(s.u.shape[0])
    pos = torch.empty((K, nt, 2), dtype=torch.int32, device=s.dev)
    val = torch.empty((K, nt), dtype=torch.float64, device=s.dev)
    status = torch.empty((K, nt), dtype=torch.int32, device=s.dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = _lib.FollowManyArgs(nt=nt, sj=sj, si=si, n_chains=K, reserved0=0, start_d=ptr(start_d), pos_d=ptr(pos), val_d=ptr(val),
                               status_d=ptr(status), **s.common())
    with torch.cuda.device(s.dev):
        _lib.check(s.lib.lec_follow_many(C.byref(args)), "lec_follow_many")
    return pos.cpu().numpy(), val.cpu().numpy(), status.cpu().numpy()


def first_shared_centre(pos) -> list:
    """For every chain of pos [K][nt][2]: None, or (the lowest-numbered earlier chain it ever shares a centre with, the first time step at
    which it does).  Chains may converge on one system; that is reported, never resolved."""
    out = []
    for c in range(len(pos)):
        hit = None
        for b in range(c):
            same = np.flatnonzero(np.all(pos[c] == pos[b], axis=1))
            if same.size and (hit is None or same[0] < hit[1]):
                hit = (b, int(same[0]))
        out.append(hit)
    return out


def write_choose_tracks(args, batch_dir, app_logger, varlist="inputs/namelist", device="cuda:0") -> list:
    """Phase A of a ``-c --choose-systems K`` / ``--choose-starts FILE`` run: the slices once, one upload, the seeds (``lec_follow_seeds``)
    or the file's starts, ONE ``lec_follow_many`` launch -> ``<batch_dir>/choose_s01``, ``choose_s02``, ... (``write_track``) and
    ``systems.csv``.  Returns the tracks' paths.  A chain whose first step finds nothing (or whose start is bad) is logged and left
    out; none left: the error ``follow_system`` raises.  With ``--choose-lifecycle``: ``write_lifecycle_tracks``."""
    if getattr(args, "choose_lifecycle", False):
        return write_lifecycle_tracks(args, batch_dir, app_logger, varlist, device)
    src = _SliceSource(args, varlist, app_logger)
    try:
        return _choose_tracks_written(args, batch_dir, app_logger, src, device)
    finally:
        src.close()


def _first_chunk(args, src):
    """(chunks, u, v, hgt of the first chunk): the whole series, and the file closed, when the planner gives one chunk."""
    chunks = slice_chunks(len(src.time), src.lat.size, src.lon.size, getattr(args, "choose_chunk", None))
    u, v, hgt = src.read(None if len(chunks) == 1 else chunks[0])
    if len(chunks) == 1:
        src.close()
    return chunks, u, v, hgt


def _choose_tracks_written(args, batch_dir, app_logger, src, device) -> list:
    """write_choose_tracks on an open source of slices."""
    import torch
    chunks, u, v, hgt = _first_chunk(args, src)
    length, width = (float(x) for x in (getattr(args, "choose_box", None) or DEFAULT_BOX))
    search = float(getattr(args, "choose_search", None) or DEFAULT_SEARCH)
    smooth = int(getattr(args, "choose_smooth", None) or 0)
    field = getattr(args, "choose_field", None) or "zeta"
    form = getattr(args, "vorticity_form", None) or "metpy_no_crs"
    k, starts_file = getattr(args, "choose_systems", None), getattr(args, "choose_starts", None)
    threshold, separation = getattr(args, "choose_threshold", None), getattr(args, "choose_separation", None)
    lat, lon, time = src.lat, src.lon, src.time
    hemisphere, sense = sense_of(field, getattr(args, "choose_hemisphere", None), lat)
    periodic = src.periodic
    bounds = admissible(lat, lon, length, width, periodic)            # (refused here, before the upload, if the box does not fit)
    kw = dict(length=length, width=width, smooth=smooth, field=field, hemisphere=hemisphere, formulation=form, device=device)
    what = f"the 850 hPa {'minima' if sense == _lib.FOLLOW_MIN else 'maxima'} of {field}"
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.LecLibraryError("the systems are found and followed on the GPU: there is no CPU path")
    u, v = (torch.as_tensor(a).to(dev) for a in (u, v))
    hgt = torch.as_tensor(hgt).to(dev)
    if starts_file is not None:
        seed_ll = read_starts(starts_file)
        seeds = np.array([start_index(lat, lon, st, bounds, periodic) for st in seed_ll], dtype=np.int32)
        seed_val = np.full(len(seeds), np.nan)
        app_logger.info(f"-c/--choose: {len(seeds)} starts from {starts_file}")
    else:
        sep = (length / 2, width / 2) if separation is None else tuple(float(x) for x in separation)
        if periodic:
            sp, sv, sn = find_systems_series(u[:1], v[:1], hgt[:1], lat, lon, k=k, threshold=threshold, separation=sep, periodic=True, **kw)
            seeds, seed_val = sp[0, :sn[0]], sv[0, :sn[0]]
        else:
            seeds, seed_val = find_systems(u[0], v[0], hgt[0], lat, lon, k=k, threshold=threshold, separation=sep, **kw)
        ej, ei = separation_steps(lat, lon, *sep)
        app_logger.info(f"-c/--choose: {len(seeds)} of at most {k} systems found at {pd.Timestamp(time[0])} ({'lec_follow_seeds_series_ring' if periodic else 'lec_follow_seeds'}: {what}, "
                        f"no better value within {sep[0]} x {sep[1]} degrees = {ej} x {ei} grid steps"
                        + ("" if threshold is None else f", threshold {threshold}") + ")")
        if len(seeds) == 0:
            raise ValueError("the first time step holds no system: nothing to follow (another --choose-threshold, --choose-separation or --choose-domain?)")
    sj, si = window_steps(lat, lon, search)
    app_logger.info(f"-c/--choose: following {what} ({hemisphere}ern hemisphere" + (f", vorticity formulation '{form}'" if field == "zeta" else "")
                    + f") on the GPU (lec_follow_many, {len(seeds)} chains in one launch): {len(time)} time steps, search domain lat {lat[0]}..{lat[-1]}, "
                    f"lon {lon[0]}..{lon[-1]} ({lat.size} x {lon.size} points), box {length} x {width} degrees (length x width), at most {search} degrees = "
                    f"{sj} x {si} grid steps per time step, smoothing radius {smooth}")
    if len(chunks) > 1:
        _log_chunks(app_logger, chunks, lat.size, lon.size, "the first chunk goes through lec_follow_many, every later one resumes the chains "
                    "(lec_follow_spans_chunk)")
    if periodic:
        app_logger.info(f"-c/--choose: --choose-periodic: the longitudes are a ring of {lon.size} columns, the chains cross the +-180 meridian "
                        f"(lec_follow_spans_chunk_ring in {len(chunks)} chunk(s) instead of lec_follow_many)")
        first = (u, v, hgt)
        del u, v, hgt
        pos, val, status = _ring_chains(src, chunks, first, seeds, search=search, **kw)
        del first
    else:
        pos, val, status = follow_systems(u, v, hgt, lat, lon, seeds=seeds, search=search, **kw)
        if len(chunks) > 1:
            del u, v, hgt
            pos, val, status = _resume_chunks(src, chunks, pos, val, status, seeds, search=search, **kw)
    _seam_notes(app_logger, src, [f"choose_s{c + 1:02d}" for c in range(len(seeds))], _last_good_columns(pos, status), si)
    shared = first_shared_centre(pos)
    for name in os.listdir(batch_dir):                                # an earlier run's tracks (it may have found more systems)
        if name.startswith("choose_s") and name[8:].isdigit():
            os.remove(os.path.join(batch_dir, name))
    rows, written = [], []
    for c in range(len(seeds)):
        name = f"choose_s{c + 1:02d}"
        row = {"system": name, "lat": lat[seeds[c, 0]], "lon": lon[seeds[c, 1]], "value": seed_val[c], "trackfile": "",
               "same_centre_as": "" if shared[c] is None else f"choose_s{shared[c][0] + 1:02d}",
               "same_centre_from": "" if shared[c] is None else pd.Timestamp(time[shared[c][1]]).strftime("%Y-%m-%d-%H%M")}
        rows.append(row)
        if status[c, 0]:
            app_logger.warning(f"-c/--choose: {name} (start {row['lat']}, {row['lon']}) is left out: " + ("its start is no admissible centre"
                               if status[c, 0] == _lib.FOLLOW_BAD_START else "its first search window holds no finite value of the field"))
            continue
        for t in np.flatnonzero(status[c]):
            app_logger.warning(f"-c/--choose: {name}: no finite value of {field} in the search window of {pd.Timestamp(time[t])}: the box stays where it was")
        if shared[c] is not None:
            app_logger.warning(f"-c/--choose: {name} sits on the same centre as {row['same_centre_as']} from {row['same_centre_from']} on: "
                               "the chains have converged on one system (both are analysed)")
        row["trackfile"] = write_track(os.path.join(batch_dir, name), time, lat[pos[c, :, 0]], lon[pos[c, :, 1]], length, width)
        written.append(row["trackfile"])
    if not written:
        raise ValueError("the first time step's search window holds no finite value of the field: nothing to follow "
                         "(another --choose-start or --choose-domain?)")
    pd.DataFrame(rows).to_csv(os.path.join(batch_dir, "systems.csv"), index=False)
    app_logger.info(f"-c/--choose: {len(written)} tracks written to {batch_dir} (track files: -t --trackfiles {' '.join(written)} repeats this run)")
    return written


# ---------------------------------------------------------------------------------------------------------------------------
# --choose-lifecycle: systems that form late or end early.  lec_follow_seeds_series seeds every time step, the seeds that no seed of
# the step before explains are births, ONE lec_follow_spans launch walks every birth from its own step until the rule ends it
# (include/lec_hip.h), and the bookkeeping in between -- nt x K ints -- is host NumPy.
# ---------------------------------------------------------------------------------------------------------------------------
MAX_BIRTHS = 256
WORK_BYTES = 256 << 20                  # find_systems_series' default chunk keeps work_d within this
DEFAULT_PATIENCE = 2
DEFAULT_MIN_STEPS = 2                   # what batch.plan_batch accepts as a track


def find_systems_series(u850, v850, hgt850, lat, lon, *, k, threshold=None, separation=None, length=DEFAULT_BOX[0], width=DEFAULT_BOX[1],
                        smooth=0, field="zeta", hemisphere=None, formulation="metpy_no_crs", device="cuda:0", chunk_steps=None, periodic=False):
    """``lec_follow_seeds_series`` on [time, lat, lon] slices: (pos [nt][k][2], val [nt][k], n_found [nt]) -- step t's are ``find_systems``
    on slice t, bit for bit, the unused entries (-2, -2) / NaN.  The library is called on chunks of ``chunk_steps`` steps, so that its
    scratch stays bounded (default: as many steps as keep it within 256 MiB); the chunks are independent.
    ``periodic``: ``lec_follow_seeds_series_ring`` -- the longitudes are a full ring (include/lec_hip.h has the rule)."""
    import torch
    if k != int(k) or not 1 <= int(k) <= 256:
        raise ValueError(f"k must be a whole number of systems, 1..256, not {k!r}")
    sep = (length / 2, width / 2) if separation is None else tuple(float(x) for x in separation)
    if len(sep) != 2 or not min(sep) > 0:
        raise ValueError(f"separation must be two positive numbers of degrees (latitude, longitude), not {separation!r}")
    s = _Slices(u850, v850, hgt850, lat, lon, 3, length=length, width=width, smooth=smooth, field=field, hemisphere=hemisphere,
                formulation=formulation, device=device, periodic=periodic)
    ej, ei = separation_steps(s.lat, s.lon, *sep)
    nt, k = int(s.u.shape[0]), int(k)
    call = "lec_follow_seeds_series_ring" if periodic else "lec_follow_seeds_series"
    if chunk_steps is None:
        chunk_steps = max(1, WORK_BYTES // (8 * s.lat.size * s.lon.size))
    if chunk_steps != int(chunk_steps) or int(chunk_steps) < 1:
        raise ValueError(f"chunk_steps must be a whole number of time steps >= 1, not {chunk_steps!r}")
    chunk = min(int(chunk_steps), nt)
    work = torch.empty((chunk, s.lat.size, s.lon.size), dtype=torch.float64, device=s.dev)
    pos = torch.empty((nt, k, 2), dtype=torch.int32, device=s.dev)
    val = torch.empty((nt, k), dtype=torch.float64, device=s.dev)
    n = torch.empty((nt,), dtype=torch.int32, device=s.dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    common = s.common()
    with torch.cuda.device(s.dev):
        for t0 in range(0, nt, chunk):
            t1 = min(t0 + chunk, nt)
            part = dict(common, u_d=ptr(s.u[t0:t1]), v_d=ptr(s.v[t0:t1]), hgt_d=None if s.h is None else ptr(s.h[t0:t1]))
            args = _lib.FollowSeedsSeriesArgs(nt=t1 - t0, ej=ej, ei=ei, k_max=k, reserved0=0,
                                              threshold=float("nan") if threshold is None else float(threshold), work_d=ptr(work),
                                              seed_pos_d=ptr(pos[t0:t1]), seed_val_d=ptr(val[t0:t1]), n_found_d=ptr(n[t0:t1]), **part)
            _lib.check(getattr(s.lib, call)(C.byref(args)), call)
    pos, val, n = pos.cpu().numpy(), val.cpu().numpy(), n.cpu().numpy()
    used = np.arange(k)[None, :] < n[:, None]
    if not (np.all((n >= 0) & (n <= k)) and np.all(pos[~used] == -2) and np.all(np.isnan(val[~used])) and np.all(pos[used] >= 0)):
        raise _lib.LecLibraryError(f"{call}: the unused entries are not marked")
    return pos, val, n


def births(seed_pos, n_found, sj, si, nx=None) -> np.ndarray:
    """[n][4] (step, j, i, seed rank) of the seeds that are births, ordered by (step, seed rank): every seed of step 0, and a seed of
    step t >= 1 unless some seed of step t - 1 lies within |dj| <= sj and |di| <= si of it (the largest move per step the chain has).
    ``nx``: the longitudes are a ring of nx columns, |di| is measured on it."""
    seed_pos, n_found = np.asarray(seed_pos), np.asarray(n_found)
    out = []
    for t in range(len(n_found)):
        now = seed_pos[t, :n_found[t]].astype(np.int64)
        before = seed_pos[t - 1, :n_found[t - 1]].astype(np.int64) if t else now[:0]
        for rank, (j, i) in enumerate(now):
            if not np.any((np.abs(before[:, 0] - j) <= sj) & (ring_distance(before[:, 1], i, nx) <= si)):
                out.append((t, int(j), int(i), rank))
    return np.array(out, dtype=np.int32).reshape(-1, 4)


def follow_spans(u850, v850, hgt850, lat, lon, *, starts, end_threshold=None, patience=DEFAULT_PATIENCE, length=DEFAULT_BOX[0],
                 width=DEFAULT_BOX[1], search=DEFAULT_SEARCH, smooth=0, field="zeta", hemisphere=None, formulation="metpy_no_crs", device="cuda:0"):
    """``lec_follow_spans``: one chain per row (t0, j, i) of ``starts`` (grid indices; a host array or a device tensor, handed to the
    kernel as it is), all in one launch -> (pos [K][nt][2], val [K][nt], status [K][nt], span [K][2]).  The rule: include/lec_hip.h.
    ``end_threshold``: in the field's own unit and sign, None: none."""
    import torch
    if not search > 0:
        raise ValueError(f"search must be > 0 degrees, not {search!r}")
    s = _Slices(u850, v850, hgt850, lat, lon, 3, length=length, width=width, smooth=smooth, field=field, hemisphere=hemisphere,
                formulation=formulation, device=device)
    sj, si = window_steps(s.lat, s.lon, search)
    start_d = (starts if isinstance(starts, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(starts, dtype=np.int32))).to(device=s.dev, dtype=torch.int32).contiguous()
    if start_d.dim() != 2 or start_d.shape[1] != 3 or start_d.shape[0] < 1:
        raise ValueError("starts: needs at least one (t0, j, i) triple")
    K, nt = int(start_d.shape[0]), int(s.u.shape[0])
    pos = torch.empty((K, nt, 2), dtype=torch.int32, device=s.dev)
    val = torch.empty((K, nt), dtype=torch.float64, device=s.dev)
    status = torch.empty((K, nt), dtype=torch.int32, device=s.dev)
    span = torch.empty((K, 2), dtype=torch.int32, device=s.dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = _lib.FollowSpansArgs(nt=nt, sj=sj, si=si, n_chains=K, patience=int(patience), start_d=ptr(start_d),
                                end_threshold=float("nan") if end_threshold is None else float(end_threshold),
                                pos_d=ptr(pos), val_d=ptr(val), status_d=ptr(status), span_d=ptr(span), **s.common())
    with torch.cuda.device(s.dev):
        _lib.check(s.lib.lec_follow_spans(C.byref(args)), "lec_follow_spans")
    return pos.cpu().numpy(), val.cpu().numpy(), status.cpu().numpy(), span.cpu().numpy()


def follow_spans_chunk(u850, v850, hgt850, lat, lon, *, starts, state, t_base, end_threshold=None, patience=DEFAULT_PATIENCE,
                       length=DEFAULT_BOX[0], width=DEFAULT_BOX[1], search=DEFAULT_SEARCH, smooth=0, field="zeta", hemisphere=None,
                       formulation="metpy_no_crs", device="cuda:0", periodic=False):
    """``lec_follow_spans_chunk``: ``follow_spans`` on ONE CHUNK of a series -- the slices hold the steps [t_base, t_base + nt) only --
    with chains that are resumed from ``state`` and leave it for the next chunk.  ``starts`` [K][3] (t0, j, i), t0 a series step;
    ``state`` [K][8] an int32 DEVICE tensor, zeroed before the first chunk, passed on unchanged from then on and updated in place
    (rows may be appended, zeroed, between calls).  -> (pos [K][nt][2], val [K][nt], status [K][nt] of the chunk's steps, span [K][2]
    in series steps as the state stands after the chunk).  ``patience`` 0: the chains never stop.  The rule: include/lec_hip.h.
    ``periodic``: ``lec_follow_spans_chunk_ring`` -- the longitudes are a full ring, the window crosses the seam."""
    import torch
    if not search > 0:
        raise ValueError(f"search must be > 0 degrees, not {search!r}")
    s = _Slices(u850, v850, hgt850, lat, lon, 3, length=length, width=width, smooth=smooth, field=field, hemisphere=hemisphere,
                formulation=formulation, device=device, periodic=periodic)
    call = "lec_follow_spans_chunk_ring" if periodic else "lec_follow_spans_chunk"
    sj, si = window_steps(s.lat, s.lon, search)
    start_d = (starts if isinstance(starts, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(starts, dtype=np.int32))).to(device=s.dev, dtype=torch.int32).contiguous()
    if start_d.dim() != 2 or start_d.shape[1] != 3 or start_d.shape[0] < 1:
        raise ValueError("starts: needs at least one (t0, j, i) triple")
    K, nt = int(start_d.shape[0]), int(s.u.shape[0])
    if not (isinstance(state, torch.Tensor) and state.dtype == torch.int32 and state.device == s.u.device and state.is_contiguous()
            and tuple(state.shape) == (K, 8)):
        raise ValueError(f"state: needs a contiguous int32 tensor [{K}][8] on {s.u.device} (the call updates it in place)")
    pos = torch.empty((K, nt, 2), dtype=torch.int32, device=s.dev)
    val = torch.empty((K, nt), dtype=torch.float64, device=s.dev)
    status = torch.empty((K, nt), dtype=torch.int32, device=s.dev)
    span = torch.empty((K, 2), dtype=torch.int32, device=s.dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = _lib.FollowChunkArgs(nt=nt, sj=sj, si=si, n_chains=K, patience=int(patience), start_d=ptr(start_d),
                                end_threshold=float("nan") if end_threshold is None else float(end_threshold),
                                pos_d=ptr(pos), val_d=ptr(val), status_d=ptr(status), span_d=ptr(span), t_base=int(t_base), state_d=ptr(state),
                                **s.common())
    with torch.cuda.device(s.dev):
        _lib.check(getattr(s.lib, call)(C.byref(args)), call)
    return pos.cpu().numpy(), val.cpu().numpy(), status.cpu().numpy(), span.cpu().numpy()


def resolve(starts, pos, span, ej, ei, nx=None) -> tuple:
    """(kept [K] bool, continuation_of [K]: a chain's number or -1), going through the chains in birth order.  A chain with span (-1, -1)
    is dropped.  A chain c is a continuation of the FIRST kept chain b with span_b[0] <= t0_c <= span_b[1] whose centre at step t0_c lies
    within (ej, ei) of c's start; a continuation is dropped.  (A system that dips under the threshold for a step is seeded again while its
    chain still lives: this is where the second chain goes.)  ``nx``: the longitudes are a ring of nx columns, |di| is measured on it."""
    starts, pos, span = np.asarray(starts), np.asarray(pos), np.asarray(span)
    K = len(starts)
    kept, cont = np.zeros(K, dtype=bool), np.full(K, -1, dtype=np.int64)
    for c in range(K):
        if span[c, 0] < 0:
            continue
        t0, j, i = (int(x) for x in starts[c, :3])
        for b in np.flatnonzero(kept[:c]):
            if span[b, 0] <= t0 <= span[b, 1] and abs(int(pos[b, t0, 0]) - j) <= ej and int(ring_distance(pos[b, t0, 1], i, nx)) <= ei:
                cont[c] = b
                break
        kept[c] = cont[c] < 0
    return kept, cont


def first_shared_centre_live(pos, span) -> list:
    """``first_shared_centre`` for chains with a life of their own: only the steps inside BOTH chains' spans are compared."""
    out = []
    for c in range(len(pos)):
        hit = None
        for b in range(c):
            lo, hi = max(span[c][0], span[b][0]), min(span[c][1], span[b][1])
            if min(span[c][0], span[b][0]) < 0 or lo > hi:
                continue
            same = np.flatnonzero(np.all(pos[c][lo: hi + 1] == pos[b][lo: hi + 1], axis=1))
            if same.size and (hit is None or lo + same[0] < hit[1]):
                hit = (b, int(lo + same[0]))
        out.append(hit)
    return out


def write_lifecycle_tracks(args, batch_dir, app_logger, varlist="inputs/namelist", device="cuda:0") -> list:
    """Phase A of a ``-c --choose-systems K --choose-lifecycle --choose-threshold X`` run: the slices once, one upload, the seeds of every
    step (``find_systems_series``), the births, ONE ``lec_follow_spans`` launch, ``resolve`` -> a track per kept chain over its span
    (``choose_sNN``, NN the birth's number) and ``systems.csv`` with a row per birth.  Returns the tracks' paths."""
    import torch
    length, width = (float(x) for x in (getattr(args, "choose_box", None) or DEFAULT_BOX))
    search = float(getattr(args, "choose_search", None) or DEFAULT_SEARCH)
    smooth = int(getattr(args, "choose_smooth", None) or 0)
    field = getattr(args, "choose_field", None) or "zeta"
    form = getattr(args, "vorticity_form", None) or "metpy_no_crs"
    k, threshold, separation = args.choose_systems, float(args.choose_threshold), getattr(args, "choose_separation", None)
    end_threshold = getattr(args, "choose_end_threshold", None)
    end_threshold = threshold if end_threshold is None else float(end_threshold)
    patience = getattr(args, "choose_patience", None) or DEFAULT_PATIENCE
    min_steps = getattr(args, "choose_min_steps", None) or DEFAULT_MIN_STEPS
    src = _SliceSource(args, varlist, app_logger)
    try:
        return _lifecycle_tracks_written(args, batch_dir, app_logger, src, device, length, width, search, smooth, field, form, k, threshold,
                                         separation, end_threshold, patience, min_steps)
    finally:
        src.close()


def _lifecycle_chunks(src, chunks, first, app_logger, *, k, threshold, sep, sj, si, end_threshold, patience, search, device, **kw):
    """The chunked form of write_lifecycle_tracks' middle: per chunk the slices (``first``: the first chunk's, already read), their
    seeds, the births of the chunk's steps (its first step's against the seeds of the step before, kept from the chunk before), the new
    births appended to the chain table with zeroed state rows, ONE ``lec_follow_spans_chunk`` launch for every chain known so far.
    -> (born [K][4], value [K] of each birth's seed, pos [K][nt][2], val, status [K][nt], span [K][2], seeds in all, births in all):
    the arrays one ``lec_follow_spans`` launch on the whole series gives."""
    import torch
    dev = torch.device(device)
    nt = len(src.time)
    nx = src.lon.size if kw.get("periodic") else None                # (a ring: |di| of the births is measured on it)
    start_d = torch.zeros((MAX_BIRTHS, 3), dtype=torch.int32, device=dev)
    state_d = torch.zeros((MAX_BIRTHS, 8), dtype=torch.int32, device=dev)
    born, born_val = np.zeros((0, 4), dtype=np.int32), np.zeros(0)
    n_seeds = n_births = 0
    last_pos, last_n = None, None                                    # the seeds of the step before the chunk
    parts, span = [], None                                            # (a, b, chains then, pos, val, status)
    for n, (a, b) in enumerate(chunks):
        u, v, hgt = first if n == 0 else src.read((a, b))
        first = None
        u, v, hgt = (torch.as_tensor(x).to(dev) for x in (u, v, hgt))
        seed_pos, seed_val, n_found = find_systems_series(u, v, hgt, src.lat, src.lon, k=k, threshold=threshold, separation=sep, device=device, **kw)
        n_seeds += int(n_found.sum())
        if last_pos is None:
            new = births(seed_pos, n_found, sj, si, nx)
            new_val = seed_val[new[:, 0], new[:, 3]]
        else:
            new = births(np.concatenate([last_pos, seed_pos]), np.concatenate([last_n, n_found]), sj, si, nx)
            new = new[new[:, 0] >= 1]                                 # (step 0 here is the step before the chunk)
            new[:, 0] -= 1
            new_val = seed_val[new[:, 0], new[:, 3]]
        new[:, 0] += a
        last_pos, last_n = seed_pos[-1:], n_found[-1:]
        n_births += len(new)
        new, new_val = new[:MAX_BIRTHS - len(born)], new_val[:MAX_BIRTHS - len(born)]      # births come ordered by step: the first MAX_BIRTHS
        if len(new):
            start_d[len(born): len(born) + len(new)] = torch.as_tensor(np.ascontiguousarray(new[:, :3])).to(dev)
            born, born_val = np.concatenate([born, new]), np.concatenate([born_val, new_val])
        K = len(born)
        if K:
            p, x, st, span = follow_spans_chunk(u, v, hgt, src.lat, src.lon, starts=start_d[:K], state=state_d[:K], t_base=a, end_threshold=end_threshold,
                                                patience=patience, search=search, device=device, **kw)
            parts.append((a, b, K, p, x, st))
        del u, v, hgt
    K = len(born)
    pos, val = np.full((K, nt, 2), -1, dtype=np.int32), np.full((K, nt), np.nan)
    status = np.full((K, nt), _lib.FOLLOW_NOT_LIVE, dtype=np.int32)   # a chunk before a chain was known: before its birth
    for a, b, Kc, p, x, st in parts:
        pos[:Kc, a:b], val[:Kc, a:b], status[:Kc, a:b] = p, x, st
    return born, born_val, pos, val, status, span, n_seeds, n_births


def _lifecycle_tracks_written(args, batch_dir, app_logger, src, device, length, width, search, smooth, field, form, k, threshold, separation,
                              end_threshold, patience, min_steps) -> list:
    """write_lifecycle_tracks on an open source of slices."""
    import torch
    lat, lon, time = src.lat, src.lon, src.time
    chunks, u, v, hgt = _first_chunk(args, src)
    hemisphere, sense = sense_of(field, getattr(args, "choose_hemisphere", None), lat)
    if (end_threshold < threshold) if sense == _lib.FOLLOW_MIN else (end_threshold > threshold):
        raise ValueError(f"--choose-end-threshold {end_threshold} is stricter than --choose-threshold {threshold}: it may be weaker, never stricter")
    periodic = src.periodic
    admissible(lat, lon, length, width, periodic)                     # (refused here, before the upload, if the box does not fit)
    kw = dict(length=length, width=width, smooth=smooth, field=field, hemisphere=hemisphere, formulation=form, device=device)
    if periodic:
        kw["periodic"] = True
    nx = lon.size if periodic else None
    what = f"the 850 hPa {'minima' if sense == _lib.FOLLOW_MIN else 'maxima'} of {field}"
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.LecLibraryError("the systems are found and followed on the GPU: there is no CPU path")
    u, v = (torch.as_tensor(a).to(dev) for a in (u, v))
    hgt = torch.as_tensor(hgt).to(dev)
    sep = (length / 2, width / 2) if separation is None else tuple(float(x) for x in separation)
    ej, ei = separation_steps(lat, lon, *sep)
    sj, si = window_steps(lat, lon, search)
    if periodic:
        app_logger.info(f"-c/--choose: --choose-periodic: the longitudes are a ring of {lon.size} columns, seeds, births and chains cross the +-180 "
                        f"meridian (lec_follow_seeds_series_ring and lec_follow_spans_chunk_ring in {len(chunks)} chunk(s))")
    if len(chunks) > 1 or periodic:                                   # (the ring calls are the chunked ones: one chunk is a chunk too)
        if len(chunks) > 1:
            _log_chunks(app_logger, chunks, lat.size, lon.size, "per chunk the seeds (lec_follow_seeds_series), the births, and one launch that "
                        "resumes every chain known so far (lec_follow_spans_chunk)")
        first = (u, v, hgt)
        del u, v, hgt
        born, born_val, pos, val, status, span, n_seeds, n_births = _lifecycle_chunks(
            src, chunks, first, app_logger, k=k, threshold=threshold, sep=sep, sj=sj, si=si, end_threshold=end_threshold, patience=patience,
            search=search, **kw)
        app_logger.info(f"-c/--choose: {n_seeds} seeds in {len(time)} time steps, at most {k} per step ({what}, no better value within {sep[0]} x {sep[1]} "
                        f"degrees = {ej} x {ei} grid steps, threshold {threshold}); {n_births} of them are births (no seed of the step before within "
                        f"{sj} x {si} grid steps); a chain ends after {patience} time steps in a row weaker than {end_threshold}")
        if n_births == 0:
            raise ValueError("no time step holds a system: nothing to follow (another --choose-threshold, --choose-separation or --choose-domain?)")
        if n_births > MAX_BIRTHS:
            app_logger.warning(f"-c/--choose: {n_births} births found, the first {MAX_BIRTHS} of them (by time step, then strength) are followed")
        return _lifecycle_outputs(batch_dir, app_logger, lat, lon, time, born, born_val, pos, status, span, ej, ei, field, length, width, end_threshold,
                                  min_steps, nx=nx, seam=(src, si))
    seed_pos, seed_val, n_found = find_systems_series(u, v, hgt, lat, lon, k=k, threshold=threshold, separation=sep, **kw)
    born = births(seed_pos, n_found, sj, si)
    app_logger.info(f"-c/--choose: {int(n_found.sum())} seeds in {len(time)} time steps, at most {k} per step (lec_follow_seeds_series: {what}, "
                    f"no better value within {sep[0]} x {sep[1]} degrees = {ej} x {ei} grid steps, threshold {threshold}); {len(born)} of them are births "
                    f"(no seed of the step before within {sj} x {si} grid steps)")
    if len(born) == 0:
        raise ValueError("no time step holds a system: nothing to follow (another --choose-threshold, --choose-separation or --choose-domain?)")
    if len(born) > MAX_BIRTHS:
        app_logger.warning(f"-c/--choose: {len(born)} births found, the first {MAX_BIRTHS} of them (by time step, then strength) are followed")
        born = born[:MAX_BIRTHS]
    app_logger.info(f"-c/--choose: following {what} ({hemisphere}ern hemisphere" + (f", vorticity formulation '{form}'" if field == "zeta" else "")
                    + f") on the GPU (lec_follow_spans, {len(born)} chains in one launch, each from its own time step): {len(time)} time steps, "
                    f"search domain lat {lat[0]}..{lat[-1]}, lon {lon[0]}..{lon[-1]} ({lat.size} x {lon.size} points), box {length} x {width} degrees "
                    f"(length x width), at most {search} degrees = {sj} x {si} grid steps per time step, smoothing radius {smooth}; a chain ends after "
                    f"{patience} time steps in a row weaker than {end_threshold}")
    pos, val, status, span = follow_spans(u, v, hgt, lat, lon, starts=born[:, :3], end_threshold=end_threshold, patience=patience, search=search, **kw)
    return _lifecycle_outputs(batch_dir, app_logger, lat, lon, time, born, seed_val[born[:, 0], born[:, 3]], pos, status, span, ej, ei, field, length,
                              width, end_threshold, min_steps, seam=(src, si))


def _lifecycle_outputs(batch_dir, app_logger, lat, lon, time, born, born_val, pos, status, span, ej, ei, field, length, width, end_threshold,
                       min_steps, nx=None, seam=None) -> list:
    """From the chains of every birth (born [K][4], born_val [K] the births' seed values) to the tracks and ``systems.csv``.
    nx: the longitudes are a ring of nx columns (``resolve``); seam (the slice source, si): for ``_seam_notes``."""
    kept, cont = resolve(born, pos, span, ej, ei, nx)
    if seam is not None:
        _seam_notes(app_logger, seam[0], [f"choose_s{c + 1:02d}" for c in range(len(born))],
                    [int(pos[c, span[c][1], 1]) if span[c][1] >= 0 and span[c][1] < len(time) - 1 else None for c in range(len(born))], seam[1])
    shared = first_shared_centre_live(pos, span)
    for name in os.listdir(batch_dir):                                # an earlier run's tracks (it may have found more systems)
        if name.startswith("choose_s") and name[8:].isdigit():
            os.remove(os.path.join(batch_dir, name))
    stamp = lambda t: pd.Timestamp(time[t]).strftime("%Y-%m-%d-%H%M")
    rows, written = [], []
    for c, (t0, j, i, rank) in enumerate(born):
        name = f"choose_s{c + 1:02d}"
        first, last = (int(x) for x in span[c])
        row = {"system": name, "lat": lat[j], "lon": lon[i], "value": born_val[c], "trackfile": "",
               "same_centre_as": "" if shared[c] is None else f"choose_s{shared[c][0] + 1:02d}",
               "same_centre_from": "" if shared[c] is None else stamp(shared[c][1]),
               "first_time": "" if first < 0 else stamp(first), "last_time": "" if first < 0 else stamp(last),
               "steps": 0 if first < 0 else last - first + 1, "ended": "" if first < 0 else ("end of series" if last == len(time) - 1 else "weak"),
               "continuation_of": "" if cont[c] < 0 else f"choose_s{cont[c] + 1:02d}", "left_out": ""}
        rows.append(row)
        born_at = f"{name} (born {stamp(t0)} at {row['lat']}, {row['lon']})"
        if first < 0:
            row["left_out"] = "never good"
            app_logger.warning(f"-c/--choose: {born_at} is left out: " + ("its start is no admissible centre" if status[c, t0] == _lib.FOLLOW_BAD_START
                               else f"no time step of it is as strong as {end_threshold}"))
            continue
        if cont[c] >= 0:
            row["left_out"] = "continuation"
            app_logger.info(f"-c/--choose: {born_at} is left out: it continues {row['continuation_of']}, whose box is within {ej} x {ei} grid steps of it then")
            continue
        if row["steps"] < min_steps:
            row["left_out"] = "too short"
            app_logger.info(f"-c/--choose: {born_at} is left out: too short ({row['steps']} time step{'s' if row['steps'] != 1 else ''}, --choose-min-steps {min_steps})")
            continue
        for t in first + np.flatnonzero(status[c, first: last + 1] == 1):
            app_logger.warning(f"-c/--choose: {name}: no finite value of {field} in the search window of {pd.Timestamp(time[t])}: the box stays where it was")
        if shared[c] is not None:
            app_logger.warning(f"-c/--choose: {name} sits on the same centre as {row['same_centre_as']} from {row['same_centre_from']} on: "
                               "the chains have converged on one system (both are analysed)")
        live = slice(first, last + 1)
        row["trackfile"] = write_track(os.path.join(batch_dir, name), time[live], lat[pos[c, live, 0]], lon[pos[c, live, 1]], length, width)
        written.append(row["trackfile"])
        app_logger.info(f"-c/--choose: {name}: {row['first_time']} .. {row['last_time']} ({row['steps']} time steps), ended: {row['ended']}")
    pd.DataFrame(rows).to_csv(os.path.join(batch_dir, "systems.csv"), index=False)
    if not written:
        raise ValueError(f"no system lives for {min_steps} time steps: nothing to analyse (another --choose-threshold, --choose-end-threshold, "
                         "--choose-patience or --choose-min-steps?)")
    app_logger.info(f"-c/--choose: {len(written)} tracks written to {batch_dir} (track files: -t --trackfiles {' '.join(written)} repeats this run)")
    return written
