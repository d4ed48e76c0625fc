"""Many tracks over one data set in ONE moving-framework pass (``lorenzcycletoolkit.py -t --trackfiles``).

The reference runs one process per track (its documented batch is a shell loop, docs/source/examples_and_tutorials.rst); every run
opens, decodes and crops the same file again.  Here the tracks are planned together on the host:

* every track is validated exactly as a single ``-t --trackfile`` run validates it, before any GPU work; a failure refuses the whole
  batch and names the track file;
* the data are prepared ONCE on the union of the tracks' time steps and the bounding rectangle of their crops (each track's own
  ``domain_slices`` window);
* every track's boxes are found on its OWN window's coordinates (so they are the grid points of its single run) and shifted into the
  union crop; a slice table {step, previous step, next step} in union steps and the track's own d/dt coefficients go with them
  (``LECEngine.rowstats(steps=...)``, ``lec_rowstats_steps``);
* tracks are grouped by what a single run of the track decides from its own data -- the record extents (tallest / widest box) and
  the longitude formulation of its own crop (``TrackPlan.group_key``): one engine call per group, so no track's bits depend on which
  other tracks share the batch.

With ``--batch-chunk N`` the union is never decoded or uploaded whole: ``plan_chunks`` cuts its time steps into runs of N, each with the
file steps to stage (T also for the time neighbours its records name in other chunks) and, per group, the records and their
``lec_ingest`` step rows; ``ingest.lec_streamed_batch`` streams the file chunk by chunk.

``--batch-composites-phase``: ``phase_ranges`` is the clock that gives every track B ranges of its own steps (``lifetime:B``, ``peak:L``),
``phase_terms`` the per-bin ensemble mean of the tracks' results.

This module is host-only (NumPy / pandas); ``frameworks.lec_moving_batch`` / ``lec_moving_batch_streamed`` run the plan on the GPU.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Dict, List, Sequence, Tuple

import numpy as np
import pandas as pd

from . import dataset as ds
from . import tables


class BatchRefusal(ValueError):
    """A batch that cannot run as given (a track that a single run would refuse, duplicate track names)."""


@dataclass
class TrackPlan:
    path: str                    # the track file
    stem: str                    # its name without the extension: the results directory's suffix
    track: pd.DataFrame
    time: np.ndarray             # datetime64[ns]: the track's times (= the time axis of its single run)
    ustep: np.ndarray            # int [n]: the union step of each of the track's times
    js: slice                    # the track's own crop (single run) in the sorted grid
    is_: slice
    joff: int                    # offset of that crop inside the union crop
    ioff: int
    limits: List[dict]           # get_limits per time step (the single run's)
    boxes: List[Tuple[int, int, int, int]]       # inclusive (iw, ie, js, jn) in UNION crop indices
    steps: np.ndarray            # int32 [n, 3]: {union step, previous, next} of the track's own time axis
    tcoef: np.ndarray            # [n, 3]: tables.time_coefs of the track's own time axis
    lon_uniform: bool = True     # the kernels' longitude formulation, decided on the track's OWN crop as its single run decides it

    @property
    def n(self) -> int:
        return len(self.time)

    @property
    def time_s(self) -> np.ndarray:
        return (self.time - self.time.min()) / np.timedelta64(1, "s")

    @property
    def extents(self) -> Tuple[int, int]:
        """(nyb_max, nxb_max) of the track's single run: its record buffer's rows and the widest box."""
        return (int(max(b[3] - b[2] + 1 for b in self.boxes)), int(max(b[1] - b[0] + 1 for b in self.boxes)))

    @property
    def group_key(self) -> Tuple[int, int, bool]:
        """What a single run of the track decides from its own data and a batch must keep: the record extents and the longitude
        formulation (tables.build_box_tables: on a partly stretched grid a track's crop can be evenly spaced while the union's is not,
        and the two formulations differ in the last bits)."""
        return self.extents + (self.lon_uniform,)

    def window(self, lat: np.ndarray, lon: np.ndarray):
        """(lat, lon) of the track's own crop, from the union crop's coordinates."""
        ny, nx = self.js.stop - self.js.start, self.is_.stop - self.is_.start
        return lat[self.joff: self.joff + ny], lon[self.ioff: self.ioff + nx]


@dataclass
class BatchPlan:
    tracks: List[TrackPlan]
    px: ds.ProcessIndex          # the file's sorted axes over ALL its time steps
    tpos: np.ndarray             # sorted file time steps of the union
    js: slice                    # union crop in the sorted grid
    is_: slice
    groups: Dict[Tuple[int, int, bool], List[int]] = field(default_factory=dict)   # TrackPlan.group_key -> track indices, in batch order

    @property
    def lat(self) -> np.ndarray:
        return self.px.lat[self.js]

    @property
    def lon(self) -> np.ndarray:
        return self.px.lon[self.is_]

    @property
    def time(self) -> np.ndarray:
        return self.px.time[self.tpos]


def expand_trackfiles(paths: Sequence[str]) -> List[str]:
    """The ``--trackfiles`` arguments as a list of files: a directory stands for every regular file in it, sorted by name.  Two
    files with the same stem would write one results directory: refused."""
    out = []
    for p in paths:
        if os.path.isdir(p):
            out += [os.path.join(p, f) for f in sorted(os.listdir(p)) if os.path.isfile(os.path.join(p, f))]
        else:
            out.append(p)
    if not out:
        raise BatchRefusal("--trackfiles: no track files given")
    seen = {}
    for p in out:
        stem = track_stem(p)
        if stem in seen:
            raise BatchRefusal(f"track files {seen[stem]} and {p} have the same name '{stem}': their results directories would collide")
        seen[stem] = p
    return out


def track_stem(path: str) -> str:
    return os.path.splitext(os.path.basename(path))[0]


def _refuse(path: str, e: BaseException):
    msg = e.args[0] if (isinstance(e, KeyError) and e.args) else str(e)
    raise BatchRefusal(f"track file {path}: {msg}") from e


def plan_batch(lat, lon, lev, time, level_units, names, trackfiles: Sequence[str], app_logger=None, lon_origin: float = 0.0) -> BatchPlan:
    """The batch on the FILE's coordinates (as ``process_index`` takes them): per track the checks of a single run, its time steps,
    its crop, its boxes, slice table and d/dt coefficients; then the union and the groups.  No data are read.
    ``lon_origin``: the origin of the longitude axis every track of this batch takes (``partition_by_origin``)."""
    from .frameworks import get_limits
    px = ds.process_index(lat, lon, lev, time, level_units, names, SimpleNamespace(track=False, lon_origin=lon_origin), app_logger)
    raw = []
    for path in trackfiles:
        try:
            track = ds.track_on_axis(ds.read_track(path, app_logger), px.lon) if lon_origin else ds.read_track(path, app_logger)
            if len(track) < 2:
                raise ValueError(f"a track needs at least 2 time steps, this one has {len(track)}")
            tpos = ds.select_track_times(px.time, track)
            js, is_ = ds.domain_slices(px.lat, px.lon, None, track=track)
            wlat, wlon = px.lat[js], px.lon[is_]
            # the checks lec_moving makes on its (cropped) data set (lec_moving_framework.py:112-154)
            t = px.time[tpos]
            if track.index[0] < t.min() or track.index[-1] > t.max():
                raise ValueError("Track time limits do not match with data time limits.")
            for name, coord in (("Lon", wlon), ("Lat", wlat)):
                word = "longitude" if name == "Lon" else "latitude"
                if track[name].max() > coord.max():
                    raise ValueError(f"Track file {word} max limit ({track[name].max():.2f}) exceeds data max {word} limit ({float(coord.max()):.2f}).")
                if track[name].min() < coord.min():
                    raise ValueError(f"Track file {word} min limit ({track[name].min():.2f}) is below data min {word} limit ({float(coord.min()):.2f}).")
            if 85000.0 not in px.level:
                raise KeyError("no 85000 Pa level in the data (the 850-hPa track diagnostics select it)")
            limits = [get_limits(track, tt) for tt in pd.DatetimeIndex(t)]
            wboxes = [tables.box_indices(wlat, wlon, l["min_lon"], l["max_lon"], l["min_lat"], l["max_lat"]) for l in limits]
        except BatchRefusal:
            raise
        except (ValueError, KeyError, IndexError, FileNotFoundError) as e:
            _refuse(path, e)
        raw.append((path, track, np.asarray(tpos), t, js, is_, limits, wboxes))

    tpos_u = np.unique(np.concatenate([r[2] for r in raw]))
    j0, j1 = min(r[4].start for r in raw), max(r[4].stop for r in raw)
    i0, i1 = min(r[5].start for r in raw), max(r[5].stop for r in raw)
    plans = []
    for path, track, tpos, t, js, is_, limits, wboxes in raw:
        joff, ioff = js.start - j0, is_.start - i0
        boxes = [(int(iw + ioff), int(ie + ioff), int(jsb + joff), int(jn + joff)) for iw, ie, jsb, jn in wboxes]
        u = np.searchsorted(tpos_u, tpos)
        n = u.size
        steps = np.stack([u, u[np.maximum(np.arange(n) - 1, 0)], u[np.minimum(np.arange(n) + 1, n - 1)]], axis=1).astype(np.int32)
        tr = TrackPlan(path=path, stem=track_stem(path), track=track, time=t, ustep=u, js=js, is_=is_, joff=joff, ioff=ioff,
                       limits=limits, boxes=boxes, steps=steps, tcoef=None, lon_uniform=tables.is_uniform(px.lon[is_]))
        tr.tcoef = tables.time_coefs(tr.time_s)
        plans.append(tr)
    plan = BatchPlan(plans, px, tpos_u, slice(j0, j1), slice(i0, i1))
    for k, tr in enumerate(plans):
        plan.groups.setdefault(tr.group_key, []).append(k)
    return plan


def composites_check(plan: BatchPlan) -> Dict[Tuple[int, int], List[int]]:
    """``--batch-composites``: ``frameworks.composites_check`` -- boxes of one shape along the track's life, at least 3 columns, evenly
    spaced longitudes and latitudes -- applied to every track on its OWN crop, as its ``-t --trackfile --composites`` run applies it; a
    violation refuses the batch naming the track file (the rule's message names the step).  Returns {(rows, columns): track indices in
    batch order}: the tracks that enter one ensemble.  Host work only."""
    from .frameworks import composites_check as check
    shapes = {}
    for k, tr in enumerate(plan.tracks):
        wlat, wlon = tr.window(plan.lat, plan.lon)
        try:
            shapes.setdefault(check(wlat, wlon, tr.boxes, flag="--batch-composites"), []).append(k)
        except ValueError as e:
            _refuse(tr.path, e)
    return shapes


def parse_phase_clock(text) -> Tuple[str, int]:
    """``--batch-composites-phase``'s value ``lifetime:B`` (B >= 1) or ``peak:L`` (L >= 0) as (kind, number); a ValueError in words
    otherwise."""
    if isinstance(text, tuple) and len(text) == 2:
        kind, num = text
    else:
        kind, sep, num = str(text).partition(":")
        if not sep or not (num[1:] if num[:1] in "+-" else num).isdigit():
            raise ValueError(f"--batch-composites-phase: '{text}' is not a clock: lifetime:B (B >= 1 bins of the normalised lifetime) or "
                             f"peak:L (L >= 0 steps on either side of the step of peak intensity)")
        num = int(num)
    if kind not in ("lifetime", "peak"):
        raise ValueError(f"--batch-composites-phase: '{text}' names the clock '{kind}': the clocks are lifetime:B and peak:L")
    if kind == "lifetime" and num < 1:
        raise ValueError(f"--batch-composites-phase: lifetime:{num}: a lifetime needs B >= 1 bins")
    if kind == "peak" and num < 0:
        raise ValueError(f"--batch-composites-phase: peak:{num}: L >= 0 steps on either side of the peak")
    return kind, int(num)


def lifetime_ranges(n: int, n_bin: int) -> np.ndarray:
    """int32 [B, 2]: step s of a track of ``n`` steps lies in bin (s * B) // n, so bin b is [ceil(b n / B), ceil((b + 1) n / B)) -- integer
    arithmetic only.  Every step lies in exactly one bin; a track with n < B has empty bins."""
    edges = [(b * int(n) + n_bin - 1) // n_bin for b in range(n_bin + 1)]
    return np.array([[edges[b], edges[b + 1]] for b in range(n_bin)], dtype=np.int32)


def peak_step(values) -> int:
    """The first step at which |value| is largest among the finite values; -1 when there is none."""
    v = np.abs(np.asarray(values, dtype=np.float64))
    v = np.where(np.isfinite(v), v, -1.0)
    return int(np.argmax(v)) if v.size and v.max() >= 0.0 else -1


def _spacing(tr) -> np.timedelta64:
    """The one spacing of the track's time axis; a BatchRefusal naming the track file when it has none."""
    d = np.diff(np.asarray(tr.time, dtype="datetime64[ns]"))
    if d.size == 0 or not np.all(d == d[0]):
        raise BatchRefusal(f"track file {tr.path}: --batch-composites-phase peak:L needs an evenly spaced time axis (a lag in steps must be a "
                           f"lag in hours), this track's steps are " + ", ".join(sorted({f"{x / np.timedelta64(1, 'h'):g} h" for x in d})) + " apart")
    return d[0]


def phase_ranges(plan, clock, intensities=None) -> np.ndarray:
    """int32 [K, B, 2]: the clock's B ranges [begin, end) of every track's own step indices (``LECEngine.compute``'s
    ``batch_composite_phases``).  ``clock``: ``lifetime:B`` / ``peak:L`` or ``parse_phase_clock``'s pair.  ``peak:L``: B = 2 L + 1, bin b
    holds the single step s_peak + (b - L) where the track has it, s_peak = ``peak_step(intensities[k])`` -- ``intensities``: per track
    its ``min_max_zeta_850`` series, the column of its ``*_trackfile``.  A track without a finite value, with an uneven time axis or with
    another spacing than the first track's refuses the batch by name."""
    kind, num = parse_phase_clock(clock)
    if kind == "lifetime":
        return np.stack([lifetime_ranges(tr.n, num) for tr in plan.tracks])
    if intensities is None or len(intensities) != len(plan.tracks):
        raise ValueError("phase_ranges: peak:L needs every track's intensities (min_max_zeta_850 per step)")
    spacing = [_spacing(tr) for tr in plan.tracks]
    for tr, d in zip(plan.tracks, spacing):
        if d != spacing[0]:
            raise BatchRefusal(f"track file {tr.path}: its steps are {d / np.timedelta64(1, 'h'):g} h apart, those of {plan.tracks[0].path} "
                               f"{spacing[0] / np.timedelta64(1, 'h'):g} h: with --batch-composites-phase peak:L a lag in steps would not be a lag in hours")
    out = np.zeros((len(plan.tracks), 2 * num + 1, 2), dtype=np.int32)
    for k, (tr, val) in enumerate(zip(plan.tracks, intensities)):
        if len(val) != tr.n:
            raise ValueError(f"phase_ranges: track {k} has {tr.n} steps and {len(val)} intensities")
        sp = peak_step(val)
        if sp < 0:
            raise BatchRefusal(f"track file {tr.path}: no finite min_max_zeta_850 at any step: --batch-composites-phase peak:L has no peak to align it on")
        for b in range(2 * num + 1):
            s = sp + b - num
            out[k, b] = (s, s + 1) if 0 <= s < tr.n else (0, 0)
    return out


def phase_labels(clock, spacing_hours=None) -> List[str]:
    """The bins' labels in ``phases.csv``: ``lifetime [b/B, (b+1)/B)`` or ``lag -2 steps (-12 h)``."""
    kind, num = parse_phase_clock(clock)
    if kind == "lifetime":
        return [f"lifetime [{b}/{num}, {b + 1}/{num})" for b in range(num)]
    return [f"lag {l:+d} steps" + ("" if spacing_hours is None else f" ({l * spacing_hours:+g} h)") for l in range(-num, num + 1)]


def phase_terms(frames: Sequence[pd.DataFrame], ranges) -> pd.DataFrame:
    """Per bin the ensemble mean of every column of the tracks' results: each track's mean over its steps in the bin, then the mean over
    the tracks that have a step there (NaN where none has).  ``frames``: the tracks' results DataFrames, ``ranges`` [K, B, 2].  The
    per-period cycle the reference's plot scripts form from ``periods.csv``, on host NumPy."""
    ranges = np.asarray(ranges)
    columns = list(frames[0].columns)
    out = np.full((ranges.shape[1], len(columns)), np.nan)
    for b in range(ranges.shape[1]):
        per = [np.mean(f[columns].to_numpy(dtype=float)[lo:hi], axis=0) for f, (lo, hi) in zip(frames, ranges[:, b]) if hi > lo]
        if per:
            out[b] = np.mean(np.stack(per), axis=0)
    return pd.DataFrame(out, columns=columns, index=pd.RangeIndex(ranges.shape[1], name="bin"))


@dataclass
class ChunkGroup:
    """One group's records of a chunk (``plan_chunks``), in (track, step) order."""
    track: np.ndarray            # int [n]: the record's track, an index into BatchPlan.tracks
    pos: np.ndarray              # int [n]: the record's position in its track
    t_rows: np.ndarray           # int32 [3, n, 3]: lec_ingest step rows of T for shift 0 / -1 / +1: {entry of ChunkPlan.t_steps, box south row, box west column}
    f_rows: np.ndarray           # int32 [n, 3]: the same for the other four fields: {entry of ChunkPlan.steps, box south row, box west column}

    @property
    def n(self) -> int:
        return len(self.track)


@dataclass
class ChunkPlan:
    """A run of consecutive union steps [u0, u1) of a BatchPlan, as one pipeline slot of the streamed batch holds it."""
    u0: int
    u1: int
    steps: np.ndarray            # file steps staged for u, v, omega, geopotential: the chunk's own union steps
    t_steps: np.ndarray          # file steps staged for T, ascending: the own steps and every previous / next step a record of the chunk names
    groups: Dict[Tuple[int, int, bool], ChunkGroup] = field(default_factory=dict)     # TrackPlan.group_key -> records; a group without a record is absent


def plan_chunks(plan: BatchPlan, chunk_steps: int) -> List[ChunkPlan]:
    """The batch cut into runs of ``chunk_steps`` consecutive union steps.  A record (one time of one track) belongs to the chunk that
    holds its union step; its T neighbours (``TrackPlan.steps``: the step itself at the track's ends) may lie in other chunks and are
    staged with this one.  Box offsets are entries into the union crop's index maps; staged steps count from the slot's first one."""
    chunk_steps = int(chunk_steps)
    if chunk_steps < 1:
        raise ValueError("chunk_steps must be >= 1")
    chunks = []
    for u0 in range(0, len(plan.tpos), chunk_steps):
        u1 = min(u0 + chunk_steps, len(plan.tpos))
        own = [np.flatnonzero((tr.ustep >= u0) & (tr.ustep < u1)) for tr in plan.tracks]
        named = np.unique(np.concatenate([np.arange(u0, u1)] + [tr.steps[p].ravel() for tr, p in zip(plan.tracks, own)]))
        ch = ChunkPlan(u0, u1, np.asarray(plan.tpos[u0:u1]), np.asarray(plan.tpos[named]))
        for key, members in plan.groups.items():
            track = np.concatenate([np.full(own[k].size, k, dtype=np.int64) for k in members])
            if track.size == 0:
                continue
            pos = np.concatenate([own[k] for k in members])
            org = np.array([(plan.tracks[k].boxes[p][2], plan.tracks[k].boxes[p][0]) for k, p in zip(track, pos)], dtype=np.int64)
            st = np.stack([plan.tracks[k].steps[p] for k, p in zip(track, pos)])           # [n, 3] union steps: own, previous, next
            t_rows = np.stack([np.column_stack([np.searchsorted(named, st[:, q]), org]) for q in range(3)]).astype(np.int32)
            f_rows = np.column_stack([st[:, 0] - u0, org]).astype(np.int32)
            ch.groups[key] = ChunkGroup(track, pos, t_rows, f_rows)
        chunks.append(ch)
    return chunks


def union_bytes(plan: BatchPlan, n_fields: int, itemsize: int) -> int:
    """Device bytes of the union cubes (``n_fields`` cubes of ``itemsize``-byte elements)."""
    return n_fields * itemsize * len(plan.tpos) * len(plan.px.level) * len(plan.lat) * len(plan.lon)


def device_bytes(plan: BatchPlan, n_fields: int, itemsize: int, phase_bins: int = 0) -> dict:
    """Device memory of a batch run (``frameworks.lec_moving_batch``): the union cubes (held throughout), the row records of the
    largest group (one group's stage-1 output at a time: fp64 [boxes, nl, nyb_max, 32]) with stage 2's workspaces, and the packed
    per-step results of all tracks (kept until the files are written).  ``phase_bins`` = B (``--batch-composites-phase``): the results
    also hold every group's accumulator of the (track, bin) cells [K, B, 6, nyb, nxb] and the bins' ensemble and spread."""
    from . import _lib
    nl = len(plan.px.level)
    cubes = union_bytes(plan, n_fields, itemsize)
    rows = 0
    for key, members in plan.groups.items():
        n = sum(plan.tracks[k].n for k in members)
        rows = max(rows, 8 * n * nl * (key[0] * _lib.LEC_NSTAT + 8 + _lib.LEC_NLEVRAW))
    results = 8 * sum(tr.n for tr in plan.tracks) * (_lib.LEC_NSCALAR + _lib.LEC_NLEVTAB * nl + 1)
    if phase_bins:
        results += 8 * sum((len(members) + 2) * int(phase_bins) * _lib.LEC_NMAP * key[0] * key[1] for key, members in plan.groups.items())
    return {"cubes": cubes, "records": rows, "results": results, "total": cubes + rows + results}


def partition_by_origin(args, trackfiles: Sequence[str], varlist: str = "inputs/namelist", app_logger=None) -> list:
    """[(origin, [positions in ``trackfiles``])], at most two entries, origin 0.0 first: the tracks by the origin of the longitude axis
    each one's own ``-t`` run takes (``dataset.track_lon_origin``).  A track that cannot be read counts as origin 0: ``plan_batch``
    refuses it there with its name."""
    lon = ds.file_longitudes(ds.series_paths(args, varlist), ds.read_namelist(varlist, app_logger), bool(getattr(args, "mpas", False)))
    parts = {}
    for n, path in enumerate(trackfiles):
        try:
            origin = ds.track_lon_origin(lon, ds.read_track(path))
        except (ValueError, KeyError, IndexError, FileNotFoundError):
            origin = 0.0
        parts.setdefault(origin, []).append(n)
    return sorted(parts.items())


def prepare_union(args, trackfiles: Sequence[str], varlist: str = "inputs/namelist", app_logger=None, lon_origin: float = 0.0):
    """``prepare_data`` for a batch: the plan, and the data set of the union (its time steps, its crop), decoded once.
    Returns (LECDataset, BatchPlan).  ``lon_origin``: as ``plan_batch``."""
    variable_list_df = ds.read_namelist(varlist, app_logger)
    mpas = bool(getattr(args, "mpas", False))
    try:
        raw = ds.open_raw(ds.series_paths(args, varlist), variable_list_df, mpas=mpas, app_logger=app_logger)
    except ValueError as e:
        if "order" not in str(e) and "device ingest reads" not in str(e):
            raise
        data = ds.open_dataset(ds.series_paths(args, varlist), variable_list_df, mpas=mpas)
        plan = plan_batch(data.lat, data.lon, data.level, data.time, data.level_units, data.names, trackfiles, app_logger, lon_origin)
        data = ds.process_data(data, SimpleNamespace(track=False, lon_origin=lon_origin), variable_list_df, app_logger)
        return data.isel(t=plan.tpos, j=plan.js, i=plan.is_), plan
    try:
        plan = plan_batch(raw.lat, raw.lon, raw.level, raw.time, raw.level_units, raw.names, trackfiles, app_logger, lon_origin)
        px = plan.px
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        ip = ds.IngestPlan(plan.tpos, i32(px.ik), i32(px.ij[plan.js]), i32(px.io[plan.is_]), plan.lat, plan.lon, px.level, plan.time)
        variables = {name: ds.gather_on_host(var, ip) for name, var in raw.variables.items()}
        return ds.LECDataset(variables, ip.lat, ip.lon, ip.level, ip.time, dict(raw.names), "Pa"), plan
    finally:
        raw.close()


def track_view(data: ds.LECDataset, tr: TrackPlan) -> ds.LECDataset:
    """The union data set restricted to one track's times and its own crop: the data set of the track's single run."""
    ny, nx = tr.js.stop - tr.js.start, tr.is_.stop - tr.is_.start
    return data.isel(t=tr.ustep, j=slice(tr.joff, tr.joff + ny), i=slice(tr.ioff, tr.ioff + nx))
