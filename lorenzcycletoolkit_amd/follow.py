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


def admissible(lat, lon, length, width) -> tuple:
    """(jlo, jhi, ilo, ihi): inclusive index bounds of the grid points whose box (lat +- length / 2, lon +- width / 2) lies inside the
    coordinate range of the (sorted, possibly stretched) axes.  A box larger than the domain is refused."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    jj = np.flatnonzero((lat - length / 2 >= lat[0]) & (lat + length / 2 <= lat[-1]))
    ii = np.flatnonzero((lon - width / 2 >= lon[0]) & (lon + width / 2 <= lon[-1]))
    if jj.size == 0 or ii.size == 0:
        raise ValueError(f"a box of {length} x {width} degrees (length x width) does not fit into the search domain of "
                         f"{float(lat[-1] - lat[0])} x {float(lon[-1] - lon[0])} degrees (lat {float(lat[0])}..{float(lat[-1])}, "
                         f"lon {float(lon[0])}..{float(lon[-1])}): no grid point can be its centre")
    return int(jj[0]), int(jj[-1]), int(ii[0]), int(ii[-1])


def window_steps(lat, lon, search) -> tuple:
    """(sj, si): the largest move per time step in grid points, max(1, floor(search / median |spacing|)) per axis."""
    step = lambda x: max(1, int(np.floor(search / np.median(np.abs(np.diff(np.asarray(x, dtype=np.float64)))))))
    return step(lat), step(lon)


def start_index(lat, lon, start, bounds) -> tuple:
    """The grid point nearest (LAT, LON) (the first of two equally near ones), clamped into the admissible centres."""
    jlo, jhi, ilo, ihi = bounds
    j = int(np.argmin(np.abs(np.asarray(lat, dtype=np.float64) - float(start[0]))))
    i = int(np.argmin(np.abs(np.asarray(lon, dtype=np.float64) - float(start[1]))))
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
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    if smooth != int(smooth) or int(smooth) < 0:
        raise ValueError(f"smooth must be a whole number of grid points >= 0, not {smooth!r}")
    if not search > 0:
        raise ValueError(f"search must be > 0 degrees, not {search!r}")
    hemisphere, sense = sense_of(field, hemisphere, lat)
    bounds = admissible(lat, lon, length, width)
    sj, si = window_steps(lat, lon, search)
    js, is_ = (-1, -1) if start is None else start_index(lat, lon, start, bounds)
    if field == "hgt" and hgt850 is None:
        raise ValueError("field 'hgt' needs the geopotential height slices")
    xcoef, ycoef, curv = vorticity_tables(lat, lon, formulation)
    lib = _lib.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.LecLibraryError("the system is followed on the GPU: there is no CPU path")
    up = lambda a: (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a))).to(device=dev, dtype=torch.float64).contiguous()
    u, v = up(u850), up(v850)
    h = None if hgt850 is None else up(hgt850)
    if u.dim() != 3 or v.shape != u.shape or (h is not None and h.shape != u.shape):
        raise ValueError("u, v and height must be [time, lat, lon] slices of one shape")
    nt, ny, nx = (int(x) for x in u.shape)
    if (ny, nx) != (lat.size, lon.size):
        raise ValueError("slices and coordinates do not match")
    xc_d, yc_d, cv_d = torch.as_tensor(xcoef).to(dev), torch.as_tensor(ycoef).to(dev), torch.as_tensor(curv).to(dev)
    pos = torch.empty((nt, 2), dtype=torch.int32, device=dev)
    val = torch.empty((nt,), dtype=torch.float64, device=dev)
    status = torch.empty((nt,), dtype=torch.int32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = _lib.FollowArgs(u_d=ptr(u), v_d=ptr(v), hgt_d=None if h is None else ptr(h), nt=nt, ny=ny, nx=nx,
                           field=_lib.FOLLOW_HGT if field == "hgt" else _lib.FOLLOW_ZETA, xcoef_d=ptr(xc_d), ycoef_d=ptr(yc_d), curv_d=ptr(cv_d),
                           sense=sense, smooth_r=int(smooth), sj=sj, si=si, jlo=bounds[0], jhi=bounds[1], ilo=bounds[2], ihi=bounds[3],
                           j_start=js, i_start=is_, pos_d=ptr(pos), val_d=ptr(val), status_d=ptr(status),
                           stream=C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    with torch.cuda.device(dev):
        _lib.check(lib.lec_follow(C.byref(args)), "lec_follow")
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


def search_domain_slices(args, varlist="inputs/namelist", app_logger=None):
    """The 85000-Pa slices of u, v and geopotential height (gpm) of ALL time steps of ``args.infile`` on the search domain
    (``args.choose_domain``: a box-limits file, label slices; default: the file's whole domain), with sorted axes:
    (u, v, hgt [nt][ny][nx] float64, lat, lon, time).  Only that level and that domain are read from the file."""
    variable_list_df = ds.read_namelist(varlist, app_logger)
    mpas = bool(getattr(args, "mpas", False))
    geo_role = "Geopotential" if "Geopotential" in variable_list_df.index else "Geopotential Height"
    roles = ("Eastward Wind Component", "Northward Wind Component", geo_role)

    def crop(px):
        k = np.flatnonzero(px.level == 85000.0)
        if k.size == 0:
            raise KeyError(85000)                               # as -t: lec_moving_framework.py:653-657 selects 85000 Pa exactly
        jj, ii = np.arange(px.lat.size), np.arange(px.lon.size)
        if getattr(args, "choose_domain", None):
            w, e, s, n = ds.read_box_limits(args.choose_domain)
            jj = np.flatnonzero((px.lat >= s) & (px.lat <= n))
            ii = np.flatnonzero((px.lon >= w) & (px.lon <= e))
        if jj.size < 3 or ii.size < 3:
            raise ValueError("the search domain selects fewer than 3 x 3 grid points of the data")
        return int(k[0]), jj, ii

    try:
        raw = ds.open_raw(args.infile, variable_list_df, mpas=mpas, app_logger=app_logger)
    except ValueError as e:
        if "order" not in str(e) and "device ingest reads" not in str(e):
            raise
        data = ds.open_dataset(args.infile, variable_list_df, mpas=mpas)              # another dimension order: the whole file
        px = ds._sorted_axes(None, data.lat, data.lon, data.level, data.time, data.level_units, data.names, app_logger)
        k, jj, ii = crop(px)
        get = lambda role: data.variables[data.names[role]][:, px.ik[k]][:, px.ij[jj]][:, :, px.io[ii]].astype(np.float64)
        u, v, g = (get(r) for r in roles)
        lat, lon, time = px.lat[jj], px.lon[ii], px.time
    else:
        try:
            px = ds._sorted_axes(None, raw.lat, raw.lon, raw.level, raw.time, raw.level_units, raw.names, app_logger)
            k, jj, ii = crop(px)
            i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
            plan = ds.IngestPlan(np.arange(raw.time.size), i32(px.ik[k: k + 1]), i32(px.ij[jj]), i32(px.io[ii]), px.lat[jj], px.lon[ii],
                                 px.level[k: k + 1], px.time)
            u, v, g = (ds.gather_on_host(raw.variables[raw.names[r]], plan)[:, 0].astype(np.float64) for r in roles)
            lat, lon, time = plan.lat, plan.lon, plan.time
        finally:
            raw.close()
    hgt = g if geo_role == "Geopotential Height" else g / G                        # -> gpm, as diagnostics.track_diagnostics
    return u, v, hgt, np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64), time


def write_choose_track(args, results_subdirectory, app_logger, varlist="inputs/namelist", device="cuda:0") -> str:
    """Phase A of a ``-c`` run: slices -> ``follow_system`` -> ``<results>/<stem>_choose_track``.  Returns the track's path."""
    length, width = (float(x) for x in (getattr(args, "choose_box", None) or DEFAULT_BOX))
    search = float(getattr(args, "choose_search", None) or DEFAULT_SEARCH)
    smooth = int(getattr(args, "choose_smooth", None) or 0)
    field = getattr(args, "choose_field", None) or "zeta"
    form = getattr(args, "vorticity_form", None) or "metpy_no_crs"
    start = getattr(args, "choose_start", None)
    u, v, hgt, lat, lon, time = search_domain_slices(args, varlist, app_logger)
    hemisphere, sense = sense_of(field, getattr(args, "choose_hemisphere", None), lat)
    sj, si = window_steps(lat, lon, search)
    app_logger.info(f"-c/--choose: following the 850 hPa {'minimum' if sense == _lib.FOLLOW_MIN else 'maximum'} of {field} "
                    f"({hemisphere}ern hemisphere" + (f", vorticity formulation '{form}'" if field == "zeta" else "") + f") on the GPU (lec_follow): "
                    f"{len(time)} time steps, search domain lat {lat[0]}..{lat[-1]}, lon {lon[0]}..{lon[-1]} ({lat.size} x {lon.size} points), "
                    f"box {length} x {width} degrees (length x width), at most {search} degrees = {sj} x {si} grid steps per time step, "
                    f"smoothing radius {smooth}, start {'the extremum of the whole domain' if start is None else tuple(start)}")
    pos, val, status = follow_system(u, v, hgt, lat, lon, length=length, width=width, search=search, smooth=smooth, field=field,
                                     hemisphere=hemisphere, start=start, formulation=form, device=device)
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
