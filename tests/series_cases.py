"""A time series that continues across files (``--series``): the writer of the parts and of the one merged file their runs are
compared with.

The fields are those of ``tests/helpers.py:write_packed_era5_style`` (same generator, same two fill points of ``v``), nt = 7 on
9 levels x 49 x 144, cut into parts of 3, 1 and 3 time steps.  Every part is quantised to int16 with its OWN scale_factor and
add_offset, taken from that part's minimum and maximum, and the second and third parts count their time from another reference date;
the fill points (steps 2 and 4) fall into the first and the third part.  The merged file is one classic file of float32 values without
packing attributes: each part's values as ``oracle/cf_decode.py`` decodes them, fill points NaN.
"""
from __future__ import annotations

import os

import numpy as np

from oracle import cf_decode as cf

NAMELIST = (";Variable;Units\nAir Temperature;t;K\nGeopotential;z;m**2/s**2\nOmega Velocity;w;Pa/s\n"
            "Eastward Wind Component;u;m/s\nNorthward Wind Component;v;m/s\nLongitude;longitude\nLatitude;latitude\n"
            "Time;time\nVertical Level;level\n")
CUTS = (3, 1, 3)
NAMES = ("t", "u", "v", "w", "z")
LON = np.arange(0.0, 360.0, 2.5)
LAT = np.arange(60.0, -62.5, -2.5)
LEV = np.array([1000, 850, 700, 500, 300, 200, 100, 50, 5], dtype=np.int32)
FILL = np.int16(-32767)
# (reference date, hours from it to the series' first step): parts two and three count from another date than the first
ORIGINS = (("2020-01-01 00:00:00", 0), ("2019-12-31 00:00:00", 24), ("2019-12-31 00:00:00", 24))


def fields(nt=7):
    """``write_packed_era5_style``'s fields, in its order of random draws."""
    rng = np.random.default_rng(4)
    nl, ny, nx = LEV.size, LAT.size, LON.size
    p = (LEV[None, :, None, None] * 100.0) / 1e5
    return {
        "t": 288.0 * p ** 0.19 + 8.0 * np.cos(np.deg2rad(2 * LAT))[None, None, :, None] * p + rng.standard_normal((nt, nl, ny, nx)),
        "u": 20.0 * np.cos(np.deg2rad(LAT))[None, None, :, None] * (1 - p / 1.2) + 5 * rng.standard_normal((nt, nl, ny, nx)),
        "v": 3.0 * rng.standard_normal((nt, nl, ny, nx)),
        "w": 0.1 * rng.standard_normal((nt, nl, ny, nx)),
        "z": 9.80665 * 7000.0 * np.log(1.0 / p) + 100.0 * rng.standard_normal((nt, nl, ny, nx)),
    }


def _create(path, nt, hours, units):
    from scipy.io import netcdf_file
    f = netcdf_file(path, "w", version=2)
    for n, s in (("time", nt), ("level", LEV.size), ("latitude", LAT.size), ("longitude", LON.size)):
        f.createDimension(n, s)
    tv = f.createVariable("time", "i", ("time",)); tv[:] = hours; tv.units = units
    lv = f.createVariable("level", "i", ("level",)); lv[:] = LEV; lv.units = "millibars"
    la = f.createVariable("latitude", "f", ("latitude",)); la[:] = LAT
    lo = f.createVariable("longitude", "f", ("longitude",)); lo[:] = LON
    return f


def quantise(a, offset=True):
    """(int16 values, scale_factor, add_offset) of one part's values, as ``write_packed_era5_style`` packs a whole file."""
    lo_, hi_ = a.min(), a.max()
    off = 0.5 * (hi_ + lo_) if offset else 0.0
    scale = (hi_ - lo_) / 65000.0 if offset else max(abs(hi_), abs(lo_)) / 32000.0
    return np.clip(np.round((a - off) / scale), -32000, 32000).astype(np.int16), float(scale), float(off)


def write_series(directory, stem="era5", cuts=CUTS, same_packing=False, fill=True, offset=True, origins=ORIGINS):
    """Writes the parts ``<stem>_1.nc`` ... into ``directory``.  Returns (paths in time order, per part {name: (int16 values, attrs)}).
    ``same_packing``: every part is quantised with the constants of the whole series."""
    os.makedirs(directory, exist_ok=True)
    nt = sum(cuts)
    f_all = fields(nt)
    whole = {n: quantise(a, offset) for n, a in f_all.items()}
    paths, packed, a0 = [], [], 0
    for k, n_steps in enumerate(cuts):
        units, shift = origins[k]
        path = os.path.join(str(directory), f"{stem}_{k + 1}.nc")
        f = _create(path, n_steps, 6 * np.arange(a0, a0 + n_steps) + shift, f"hours since {units}")
        part = {}
        for name in NAMES:
            a = f_all[name][a0: a0 + n_steps]
            if same_packing:
                _, scale, off = whole[name]
                q = np.clip(np.round((a - off) / scale), -32000, 32000).astype(np.int16)
            else:
                q, scale, off = quantise(a, offset)
            if name == "v" and fill:
                for t, sel in ((2, (7, slice(None), slice(None))), (4 % nt, (3, 10, 20))):
                    if a0 <= t < a0 + n_steps:
                        q[(t - a0,) + sel] = FILL
            v = f.createVariable(name, "h", ("time", "level", "latitude", "longitude"))
            v[:] = q
            # (NumPy doubles: the classic writer stores a Python float as a 32-bit attribute; ERA5's are doubles)
            attrs = {"scale_factor": np.float64(scale)}
            v.scale_factor = np.float64(scale)
            if offset:
                v.add_offset = np.float64(off)
                attrs["add_offset"] = np.float64(off)
            if fill:
                v._FillValue = FILL
                attrs["_FillValue"] = FILL
            part[name] = (q, attrs)
        f.close()
        paths.append(path)
        packed.append(part)
        a0 += n_steps
    return paths, packed


def write_merged(path, packed, cuts=CUTS):
    """The comparison file: float32, no packing attributes, every part's values as the oracle's CF decode gives them."""
    nt = sum(cuts)
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    f = _create(str(path), nt, 6 * np.arange(nt), "hours since 2020-01-01 00:00:00")
    decoded = {}
    for name in NAMES:
        a = np.concatenate([cf.decode_cf_variable(q, attrs) for q, attrs in (part[name] for part in packed)])
        assert a.dtype == np.float32, (name, a.dtype)       # int16 + scale_factor + add_offset + _FillValue: float32 in the reference
        v = f.createVariable(name, "f", ("time", "level", "latitude", "longitude"))
        v[:] = a
        decoded[name] = a
    f.close()
    return decoded


def standard_case(root):
    """(parts, merged path, per-part packed values, decoded values): the parts in ``root/parts``, the merged file of the first
    part's basename in ``root/merged``."""
    parts, packed = write_series(os.path.join(str(root), "parts"))
    merged = os.path.join(str(root), "merged", os.path.basename(parts[0]))
    decoded = write_merged(merged, packed)
    return parts, merged, packed, decoded


def later_copy_of_hdf5(src, dst, hours, rescale_t=None):
    """A copy of one of the NetCDF-4 fixtures (tests/golden/hdf5) that continues it in time: the five int32 values of its contiguous
    ``time`` variable are moved on by ``hours`` in place (no HDF5 writer is needed for that).  ``rescale_t``: the float64
    ``scale_factor`` attribute of ``t`` is multiplied by it, so that the copy packs T with other constants than the original."""
    from lorenzcycletoolkit_amd.hdf5_lite import H5File
    h = H5File(src)
    time, t = h.variables["time"], h.variables["t"]
    assert time._layout["class"] == "contiguous" and time.dtype == np.dtype("<i4") and time.shape == (5,)
    at, scale = int(time._layout["addr"]), np.float64(t.attrs["scale_factor"])
    h.close()
    raw = bytearray(open(src, "rb").read())
    raw[at: at + 20] = (np.frombuffer(bytes(raw[at: at + 20]), dtype="<i4") + np.int32(hours)).tobytes()
    if rescale_t is not None:
        old = scale.astype("<f8").tobytes()
        assert raw.count(old) == 1
        raw[raw.index(old): raw.index(old) + 8] = np.float64(scale * rescale_t).astype("<f8").tobytes()
    os.makedirs(os.path.dirname(str(dst)), exist_ok=True)
    with open(dst, "wb") as f:
        f.write(bytes(raw))
    return str(dst)
