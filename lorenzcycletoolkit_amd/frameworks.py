"""Drop-in counterparts of the reference's L4/L3 call surface, backed by the HIP engine.

* ``lec_fixed`` / ``lec_moving``: same arguments, results tree and CSV schema as
  src/frameworks/lec_fixed_framework.py:30-303 and lec_moving_framework.py:546-745.
* ``BoxData`` + ``EnergyContents`` / ``ConversionTerms`` / ``BoundaryTerms`` /
  ``GenerationDissipationTerms`` with the reference's ``calc_*`` methods (box_data.py:78-90,
  lec_fixed_framework.py:216-271): BoxData runs the two HIP stages once for the whole cube; the
  ``calc_*`` methods hand out the finished series and append the per-level CSV rows.

Where the reference loops over time steps in Python (lec_moving_framework.py:639) this module
issues ONE engine call with one box per time step.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Optional

import numpy as np
import pandas as pd
import torch

from . import dataset as ds
from . import phases
from .constants import LEVEL_TERMS
from .engine import LECEngine, LECResult, pack_host
from .tables import budgets_and_residuals

FIXED_COLUMNS = ["Az", "Ae", "Kz", "Ke", "Cz", "Ca", "Ck", "Ce", "BAz", "BAe", "BKz", "BKe", "Gz", "Ge"]
MOVING_COLUMNS = ["Az", "Ae", "Kz", "Ke", "Cz", "Ca", "Ck", "Ce", "BAz", "BAe", "BKz", "BKe", "BΦZ", "BΦE", "Gz", "Ge"]


def _device(args=None):
    shard = getattr(args, "shard", None)
    dev = shard.device if shard is not None else (getattr(args, "device", None) or os.environ.get("LEC_DEVICE", "cuda:0"))
    if not torch.cuda.is_available():
        raise RuntimeError("lorenzcycletoolkit_amd needs an AMD GPU (PyTorch-ROCm): there is no CPU path")
    return torch.device(dev)


class BoxData:
    """Counterpart of box_data.py:58-105.  ``data`` is an LECDataset (time, level, lat, lon).

    Fixed framework: one box for all time steps, dT/dt by finite differences over the cube's time axis.
    Moving framework: pass ``boxes_limits`` = one (west, east, south, north) per time step (the four
    scalar limits are then ignored); ``dTdt`` may be None (differentiated on the device, as
    lorenzcycletoolkit.py:184-186 does over the same time axis) or a host cube.

    Time-sharded runs (``args.shard``, a parallel.ShardContext: one process per GPU): every rank computes its contiguous block of
    time steps from the steps it holds (own + one-step T halo; ``data.t_held``), the any-time NaN-level mask is merged across the
    ranks, and ONE gather brings the packed per-step records to rank 0, whose BoxData then looks exactly like the one-process one;
    on the other ranks ``result`` / ``scalars`` / ``levels`` are None.

    ``periodic`` (fixed framework only): the box is the latitude band [south, north] over ALL of ``data``'s longitudes, which must be
    a full ring (evenly spaced, nx * dx = 360 degrees), and the western / eastern limits must select its first / last column: zonal
    means over the closed circle, Q's d/dlon centred across the seam, no east-west boundary flux (``lec_rowstats_ring``).

    ``wavenumbers`` = N (``periodic`` only, one process; a ``StreamedDataset`` computes them chunk by chunk): ``spectrum`` [time, 5, N], ``spectrum_rest`` [time, 5] and
    ``spectrum_levels`` [time, 14, N, level] -- the shares of the zonal wavenumbers 1 .. N in Ae, Ke, Ca, Ce, Ck (``lec_rowspec_ring``).
    ``spectrum_generation`` (with ``wavenumbers``; no ``dTdt`` cube): also ``spectrum_ge`` [time, N], ``spectrum_ge_rest`` [time] and
    ``spectrum_ge_levels`` [time, N, level], the same shares of Ge (``lec_rowspec_q_ring``).
    ``spectrum_interactions`` (with ``wavenumbers``): also ``spectrum_nl`` [time, 2, N], ``spectrum_nl_total`` [time, 2],
    ``spectrum_nl_rest`` [time, 2] and ``spectrum_nl_levels`` [time, 2, N, level], the non-linear eddy-eddy transfers S(n) into Ae and
    L(n) into Ke (``lec_rowspec_nl_ring``).
    ``spectrum_budget`` (with ``wavenumbers``; at least two time steps): also ``spectrum_b`` [time, 2, N] (BAe(n), BKe(n):
    ``lec_rowspec_b_ring``), ``spectrum_tendency`` [time, 2, N] (dAe(n)/dt, dKe(n)/dt) and ``spectrum_residual`` [time, 2, N] (RGe(n),
    RKe(n)), each with its ``_rest`` [time, 2].
    """

    def __init__(self, data: ds.LECDataset, variable_list_df: pd.DataFrame, western_limit=None, eastern_limit=None,
                 southern_limit=None, northern_limit=None, args=None, results_subdirectory: str = ".",
                 results_subdirectory_vertical_levels: str = ".", dTdt: Optional[np.ndarray] = None,
                 boxes_limits=None, periodic: bool = False, wavenumbers: Optional[int] = None,
                 spectrum_generation: bool = False, spectrum_interactions: bool = False, spectrum_budget: bool = False,
                 sections: bool = False, maps: bool = False, composites: bool = False, composite_sections: bool = False,
                 lon_sections: bool = False, composite_lon_sections: bool = False):
        if args is not None and not getattr(args, "residuals", True):
            # the reference looks up "Friction Velocity" here and fails (box_data.py:190-195; SURVEY B-8)
            raise KeyError("Friction Velocity")
        self.periodic = bool(periodic)
        if self.periodic:               # (host work only: refused before the GPU is touched)
            if boxes_limits is not None:
                raise ValueError("periodic: one fixed box (the moving framework's ring is the 0..360 axis of --choose-periodic)")
            from .tables import box_indices
            self.xlength = ring_box_check(data.lon, box_indices(data.lat, data.lon, western_limit, eastern_limit, southern_limit, northern_limit))
        self.sections = bool(sections)
        self.section_mean = self.section_lat = self.section_spec_lat = None
        if self.sections:               # (host work only, as above)
            if boxes_limits is not None:
                raise ValueError("sections exist for ONE fixed box: a series of per-step boxes (a track, chosen boxes) has no common rows "
                                 "to lay a section on")
            if getattr(args, "shard", None) is not None:
                raise ValueError("sections run on one GPU (no time shards)")
        self.maps = bool(maps)
        self.map_mean = self.map_lon = None
        if self.maps:                   # (host work only, as above)
            from .ingest import StreamedDataset as _StreamedData
            if boxes_limits is not None:
                raise ValueError("maps exist for ONE fixed box: a series of per-step boxes (a track, chosen boxes) has no common points "
                                 "to lay a map on")
            if getattr(args, "shard", None) is not None:
                raise ValueError("maps run on one GPU (no time shards)")
            if dTdt is not None:
                raise ValueError("maps: a dTdt cube is not supported (lec_maps forms dT/dt from the time axis)")
            if isinstance(data, _StreamedData):
                raise ValueError("maps prepare the data on the host: the streamed path (--ingest device / --device-ingest) is not supported")
        self.lon_sections = bool(lon_sections)
        self.lonsection_mean = None
        if self.lon_sections:           # (host work only, as above)
            from .ingest import StreamedDataset as _StreamedData
            if boxes_limits is not None:
                raise ValueError("longitude-pressure sections exist for ONE fixed box: a series of per-step boxes (a track, chosen boxes) "
                                 "has no common columns to lay a section on; it has composite_lon_sections")
            if getattr(args, "shard", None) is not None:
                raise ValueError("longitude-pressure sections run on one GPU (no time shards)")
            if dTdt is not None:
                raise ValueError("longitude-pressure sections: a dTdt cube is not supported (lec_lonsections forms dT/dt from the time axis)")
            if isinstance(data, _StreamedData):
                raise ValueError("longitude-pressure sections prepare the data on the host: the streamed path (--ingest device / "
                                 "--device-ingest) is not supported")
        self.composite_lon_sections = bool(composite_lon_sections)
        self.composite_lonsection_mean = None
        if self.composite_lon_sections:     # (host work only, as above)
            from .ingest import StreamedDataset as _StreamedData
            if boxes_limits is None:
                raise ValueError("composite longitude-pressure sections exist for the per-step boxes of a track (boxes_limits): ONE fixed "
                                 "box has lon_sections")
            if getattr(args, "shard", None) is not None:
                raise ValueError("composite longitude-pressure sections run on one GPU (no time shards)")
            if isinstance(data, _StreamedData):
                raise ValueError("composite longitude-pressure sections prepare the data on the host: the streamed path (--ingest device / "
                                 "--device-ingest) is not supported")
            from .tables import box_indices
            composites_check(data.lat, data.lon, [box_indices(data.lat, data.lon, *lim) for lim in boxes_limits],
                             flag="composite longitude-pressure sections", lat_too=False)
        self.composites = bool(composites)
        self.composite_mean = self.composite_lon = None
        if self.composites:             # (host work only, as above)
            from .ingest import StreamedDataset as _StreamedData
            if boxes_limits is None:
                raise ValueError("composites exist for the per-step boxes of a track (boxes_limits): ONE fixed box has maps")
            if getattr(args, "shard", None) is not None:
                raise ValueError("composites run on one GPU (no time shards)")
            if isinstance(data, _StreamedData):
                raise ValueError("composites prepare the data on the host: the streamed path (--ingest device / --device-ingest) is not supported")
            from .tables import box_indices
            composites_check(data.lat, data.lon, [box_indices(data.lat, data.lon, *lim) for lim in boxes_limits], flag="composites", lat_too=False)
        self.composite_sections = bool(composite_sections)
        self.composite_section_mean = self.composite_section_lat = None
        if self.composite_sections:     # (host work only, as above; the streamed path is served: only row records are read)
            if boxes_limits is None:
                raise ValueError("composite sections exist for the per-step boxes of a track (boxes_limits): ONE fixed box has sections")
            if getattr(args, "shard", None) is not None:
                raise ValueError("composite sections run on one GPU (no time shards)")
            from .tables import box_indices
            composite_sections_check(data.lat, [box_indices(data.lat, data.lon, *lim) for lim in boxes_limits], flag="composite sections",
                                     lat_too=False)
        self.wavenumbers = None if wavenumbers is None else int(wavenumbers)
        self.spectrum = self.spectrum_rest = self.spectrum_levels = None
        if wavenumbers is not None:     # (host work only, as above)
            from .ingest import StreamedDataset as _Streamed
            if not self.periodic:
                raise ValueError("wavenumbers: a zonal-wavenumber spectrum exists on a ring only (periodic=True)")
            wavenumbers_check(self.wavenumbers, len(data.lon))
            if getattr(args, "shard", None) is not None:
                raise ValueError("wavenumbers: one process (no time shards)")
        self.spectrum_generation = bool(spectrum_generation)
        self.spectrum_ge = self.spectrum_ge_rest = self.spectrum_ge_levels = None
        if self.spectrum_generation:
            if wavenumbers is None:
                raise ValueError("spectrum_generation: Ge(n) is part of the zonal-wavenumber spectra: give wavenumbers=N")
            if dTdt is not None:
                raise ValueError("spectrum_generation: a dTdt cube is not supported (lec_rowspec_q_ring forms dT/dt from the time axis)")
        self.spectrum_interactions = bool(spectrum_interactions)
        self.spectrum_nl = self.spectrum_nl_total = self.spectrum_nl_rest = self.spectrum_nl_levels = None
        if self.spectrum_interactions and wavenumbers is None:
            raise ValueError("spectrum_interactions: S(n) and L(n) are part of the zonal-wavenumber spectra: give wavenumbers=N")
        self.spectrum_budget = bool(spectrum_budget)
        self.spectrum_b = self.spectrum_b_rest = self.spectrum_tendency = self.spectrum_tendency_rest = None
        self.spectrum_residual = self.spectrum_residual_rest = None
        if self.spectrum_budget:
            if wavenumbers is None:
                raise ValueError("spectrum_budget: BAe(n), BKe(n) and the residuals are part of the zonal-wavenumber spectra: give wavenumbers=N")
            if len(data.time) < 2:
                raise ValueError("spectrum_budget: the tendencies are finite differences in time: at least 2 time steps")
        self.args = args
        self.results_subdirectory = results_subdirectory
        self.results_subdirectory_vertical_levels = results_subdirectory_vertical_levels
        self.LonIndexer = variable_list_df.loc["Longitude"]["Variable"]
        self.LatIndexer = variable_list_df.loc["Latitude"]["Variable"]
        self.TimeName = variable_list_df.loc["Time"]["Variable"]
        self.VerticalCoordIndexer = variable_list_df.loc["Vertical Level"]["Variable"]
        self.PressureData = data.level
        self.time = data.time
        self._row_labels = {}
        dev = _device(args)
        self.engine = LECEngine(data.lat, data.lon, data.level, device=dev)
        limits = boxes_limits if boxes_limits is not None else [(western_limit, eastern_limit, southern_limit, northern_limit)]
        self.per_step_boxes = boxes_limits is not None
        self.boxes = [self.engine.box_from_limits(*lim) for lim in limits]
        iw, ie, js, jn = self.boxes[0]
        self.western_limit, self.eastern_limit = float(data.lon[iw]), float(data.lon[ie])
        self.southern_limit, self.northern_limit = float(data.lat[js]), float(data.lat[jn])

        n_steps, nl = len(data.time), len(data.level)
        shard = self.shard = getattr(args, "shard", None)
        t0, t1, h0, h1 = (0, n_steps, 0, n_steps) if shard is None else shard.ranges(n_steps)
        self.t_own, self.t_held = (t0, t1), (h0, h1)
        width = LECEngine.packed_width(nl)
        out, merge, gat = None, None, None
        if shard is not None:
            # one extra column carries the NaN counter of the step, so that ONE gather moves everything rank 0 needs
            from .parallel import SeriesGatherer
            gat = SeriesGatherer(n_steps, width + 1, dev, group=shard.group, dst=0, slots=1, force=True)
            out = gat.send(0)[:, :width]
            merge = shard.merge_dropmask if not self.per_step_boxes else None

        from . import ingest
        from .ingest import StreamedDataset
        if isinstance(data, StreamedDataset):
            # device ingest: the file bytes are streamed, decoded, sorted and cropped on the GPU (ingest.py); in the moving
            # framework dT/dt is differentiated on the device over the (track-selected) time axis
            if dTdt is not None:
                raise NotImplementedError("the device ingest differentiates T in time itself; do not pass a dTdt cube")
            self.ingest_stats = {}
            # the moving framework's 850-hPa diagnostics take their three slices from the cubes this pass decodes (no second read of the
            # file); only where the namelist's units leave the values as they are in the file, so that both paths see the same numbers
            plain_units = all(ds.field_scale(variable_list_df, r) == 1.0 for r in ("Eastward Wind Component", "Northward Wind Component"))
            keep = 85000.0 if (boxes_limits is not None and plain_units and 85000.0 in data.level) else None
            with ingest.refusals():       # (what --ingest auto may fall back from: an input the streamed path declines, nothing later)
                self.result: LECResult = ingest.lec_streamed(data.raw, data.plan, variable_list_df, limits, per_step_boxes=boxes_limits is not None,
                                                             device=dev, chunk_steps=data.chunk_steps, stats=self.ingest_stats, inflate=data.inflate,
                                                             t_range=None if shard is None else (t0, t1), merge_dropmask=merge, out=out, keep_level=keep,
                                                             ring=self.periodic,
                                                             **({} if self.wavenumbers is None else {"wavenumbers": self.wavenumbers}),
                                                             **({"spectrum_generation": True} if self.spectrum_generation else {}),
                                                             **({"spectrum_interactions": True} if self.spectrum_interactions else {}),
                                                             **({"spectrum_budget": True} if self.spectrum_budget else {}),
                                                             **({"sections": True} if self.sections else {}),
                                                             **({"composite_sections": True} if self.composite_sections else {}))
            self.level_slices = self.ingest_stats.pop("level_slices", None)
        else:
            self.result = self._compute_resident(data, variable_list_df, dev, dTdt, merge, out)
        if shard is not None:
            gat.send(0)[:, width] = self.result.nanflag.to(torch.float64)
            gat.start(0)
            series = gat.finish(0)
            torch.cuda.synchronize(dev)
            if series is None:                   # not the rank that writes the results
                self.result = self.scalars = self.levels = self.nanflag = None
                return
            self.result = LECResult(scalars=series[:, :16], levels=series[:, 16:width].unflatten(1, (21, nl)),
                                    nanflag=series[:, width].to(torch.int32), packed=series[:, :width])
        torch.cuda.synchronize(dev)
        self.scalars = self.result.scalars_dict()
        self.levels = self.result.levels_dict()
        self.nanflag = self.result.nanflag.cpu().numpy()
        if self.result.spectrum is not None:
            self.spectrum = self.result.spectrum.cpu().numpy()
            self.spectrum_rest = self.result.spectrum_rest.cpu().numpy()
            self.spectrum_levels = self.result.spectrum_levels.cpu().numpy()
        if self.result.spectrum_ge is not None:
            self.spectrum_ge = self.result.spectrum_ge.cpu().numpy()
            self.spectrum_ge_rest = self.result.spectrum_ge_rest.cpu().numpy()
            self.spectrum_ge_levels = self.result.spectrum_ge_levels.cpu().numpy()
        if self.result.spectrum_nl is not None:
            self.spectrum_nl = self.result.spectrum_nl.cpu().numpy()
            self.spectrum_nl_total = self.result.spectrum_nl_total.cpu().numpy()
            self.spectrum_nl_rest = self.result.spectrum_nl_rest.cpu().numpy()
            self.spectrum_nl_levels = self.result.spectrum_nl_levels.cpu().numpy()
        if self.result.spectrum_b is not None:
            for name in ("spectrum_b", "spectrum_tendency", "spectrum_residual"):
                setattr(self, name, getattr(self.result, name).cpu().numpy())
                setattr(self, name + "_rest", getattr(self.result, name + "_rest").cpu().numpy())
        if self.result.section_mean is not None:
            self.section_mean = self.result.section_mean.cpu().numpy()
            self.section_lat = self.result.section_lat.cpu().numpy()
            if self.result.section_spec_lat is not None:
                self.section_spec_lat = self.result.section_spec_lat.cpu().numpy()
            js, jn = self.boxes[0][2], self.boxes[0][3]
            self.section_latitudes = np.asarray(data.lat[js: jn + 1], dtype=np.float64)
        if self.result.map_mean is not None:
            self.map_mean = self.result.map_mean.cpu().numpy()
            self.map_lon = self.result.map_lon.cpu().numpy()
            iw, ie, js, jn = self.boxes[0]
            self.map_latitudes = np.asarray(data.lat[js: jn + 1], dtype=np.float64)
            self.map_longitudes = np.asarray(data.lon[iw: ie + 1], dtype=np.float64)
        if self.result.composite_mean is not None:
            self.composite_mean = self.result.composite_mean.cpu().numpy()
            self.composite_lon = self.result.composite_lon.cpu().numpy()
            self.composite_dlat, self.composite_dlon = composite_offsets(data.lat, data.lon, self.boxes[0])
        if self.result.composite_section_mean is not None:
            self.composite_section_mean = self.result.composite_section_mean.cpu().numpy()
            self.composite_section_lat = self.result.composite_section_lat.cpu().numpy()
            self.composite_section_dlat = composite_offsets(data.lat, data.lon, self.boxes[0])[0]
        if self.result.lonsection_mean is not None:
            self.lonsection_mean = self.result.lonsection_mean.cpu().numpy()
            iw, ie = self.boxes[0][0], self.boxes[0][1]
            self.lonsection_longitudes = np.asarray(data.lon[iw: ie + 1], dtype=np.float64)
        if self.result.composite_lonsection_mean is not None:
            self.composite_lonsection_mean = self.result.composite_lonsection_mean.cpu().numpy()
            self.composite_lonsection_dlon = composite_offsets(data.lat, data.lon, self.boxes[0])[1]

    def row_labels(self, method: str):
        """The time-stamp column of the per-level tables (formatted once per series, not once per table)."""
        got = self._row_labels.get(method)
        if got is None:
            got = self._row_labels[method] = time_labels(self.time, method)
        return got

    def _compute_resident(self, data: ds.LECDataset, variable_list_df: pd.DataFrame, dev, dTdt, merge=None, out=None) -> LECResult:
        """Host-prepared cubes, uploaded whole (a time-sharded rank: the steps it holds)."""
        (t0, t1), (h0, h1) = self.t_own, self.t_held
        n_steps = len(data.time)
        held = getattr(data, "t_held", None) or (0, n_steps)
        if self.shard is not None and tuple(held) == (0, n_steps) and (h0, h1) != (0, n_steps):
            data = data.held_steps((h0, h1))         # a whole data set handed to a sharded BoxData: keep this rank's steps only
            held = (h0, h1)
        if tuple(held) != (h0, h1):
            raise ValueError(f"data set holds time steps {held}, this rank needs {(h0, h1)}")
        arrays, common, phi_scale = host_fields(data, variable_list_df)
        if self.per_step_boxes and dTdt is None:
            return self._compute_resident_packed(arrays, common, data, dev, phi_scale, merge, out)
        cubes = [torch.as_tensor(np.ascontiguousarray(a, dtype=common)).to(dev) for a in arrays]
        dTdt_dev = None
        if dTdt is not None:
            dTdt = np.asarray(dTdt)
            if dTdt.shape[0] == n_steps and (h0, h1) != (0, n_steps):
                dTdt = dTdt[h0:h1]
            dTdt_dev = torch.as_tensor(np.ascontiguousarray(dTdt, dtype=common)).to(dev)
        boxes = self.boxes[t0:t1] if self.per_step_boxes else self.boxes
        if self.periodic:
            boxes = self.engine.prepare_boxes(boxes, ring=True)
        if self.per_step_boxes and self.shard is not None:
            # the records of every rank have the row count of the tallest box of the WHOLE series (as the one-process run's)
            nyb = max(b[3] - b[2] + 1 for b in self.boxes)
            boxes = self.engine.prepare_boxes(boxes, nyb_min=nyb)
        return self.engine.compute(cubes[0], cubes[1], cubes[2], cubes[3], cubes[4], boxes,
                                   time_s=data.time_s[h0:h1] if dTdt is None or self.spectrum_budget else None, dTdt=dTdt_dev,
                                   phi_scale=phi_scale, t_begin=t0 - h0, t_count=t1 - t0, per_step_boxes=self.per_step_boxes,
                                   drop_any_time=not self.per_step_boxes, merge_dropmask=merge, out=out,
                                   **({} if self.wavenumbers is None else {"wavenumbers": self.wavenumbers}),
                                   **({"spectrum_generation": True} if self.spectrum_generation else {}),
                                   **({"spectrum_interactions": True} if self.spectrum_interactions else {}),
                                   **({"spectrum_budget": True} if self.spectrum_budget else {}),
                                   **({"sections": True} if self.sections else {}), **({"maps": True} if self.maps else {}),
                                   **({"composites": True} if self.composites else {}),
                                   **({"composite_sections": True} if self.composite_sections else {}),
                                   **({"lon_sections": True} if self.lon_sections else {}),
                                   **({"composite_lon_sections": True} if self.composite_lon_sections else {}))

    def _compute_resident_packed(self, arrays, common, data, dev, phi_scale, merge, out) -> LECResult:
        """The moving framework on host-prepared data: the reference slices every step's box out of the crop (box_data.py:297-310);
        here the host does that slice BEFORE the upload -- each step's box to the origin of its slab, T also from the two neighbouring
        steps -- so a tenth of the crop crosses the link and stage 1 gets the box-packed series the streamed path hands it too
        (include/lec_hip.h; fp64 storage: dT/dt as a cube, `lec_dtdt`; fp32: the two neighbours).  Same records as the crop, bit for bit."""
        (t0, t1), (h0, h1) = self.t_own, self.t_held
        boxes = self.boxes[t0:t1]
        nyb = max(b[3] - b[2] + 1 for b in self.boxes)       # (the records of every rank have the row count of the tallest box of the WHOLE series)
        nxb = max(b[1] - b[0] + 1 for b in self.boxes)

        def pack(a, shift=0):
            src = np.clip(np.arange(t0, t1) + shift, h0, h1 - 1) - h0       # the step itself where the series has no neighbour (coefficient 0)
            return torch.as_tensor(pack_host(a, boxes, src, nyb, nxb, dtype=common)).to(dev)

        f = [pack(a) for a in arrays]
        tm, tp = pack(arrays[0], -1), pack(arrays[0], +1)
        tcoef = self.engine.time_coefs_device(data.time_s[h0:h1])[t0 - h0: t1 - h0].contiguous()
        pb = self.engine.prepare_boxes(boxes, nyb_min=nyb, packed=True)
        kw = self.engine.packed_dtdt(tm, f[0], tp, tcoef)
        return self.engine.compute(f[0], f[1], f[2], f[3], f[4], pb, phi_scale=phi_scale, t_begin=0, t_count=t1 - t0, per_step_boxes=True,
                                   drop_any_time=False, merge_dropmask=merge, out=out, **kw,
                                   **({"composites": True} if self.composites else {}),
                                   **({"composite_sections": True} if self.composite_sections else {}),
                                   **({"composite_lon_sections": True} if self.composite_lon_sections else {}))


def ring_box_check(lon, box) -> float:
    """A periodic box on the longitude axis ``lon``: the axis must be a full ring and the box (iw, ie, js, jn) must span it from its first
    to its last column -- a periodic box of part of a circle does not exist, and nothing is clamped.  Returns the closed axis' xlength
    in radians; raises ValueError."""
    from .follow import ring_error
    from .tables import ring_axis
    lon = np.asarray(lon, dtype=np.float64)
    why = ring_error(lon)
    if why:
        raise ValueError("--periodic needs a full ring of longitudes: " + why)
    if box[0] != 0 or box[1] != lon.size - 1:
        raise ValueError(f"--periodic: the box limits select the longitudes {float(lon[box[0]])} and {float(lon[box[1]])}, not the axis' first "
                         f"and last ({float(lon[0])} and {float(lon[-1])}): a periodic box of part of a circle does not exist "
                         "(min_lon -180 and max_lon 180 always select the whole ring)")
    return ring_axis(lon)[1]


def wavenumbers_check(n: int, nx: int) -> None:
    """--wavenumbers N on a ring of ``nx`` longitudes: 1 <= N <= nx / 2 (the ring holds no other wavenumbers) and N <= the library's
    limit; raises ValueError, nothing is clamped."""
    from ._lib import LEC_MAX_WAVENUMBERS
    if n < 1 or n > nx // 2:
        raise ValueError(f"--wavenumbers {n}: a ring of {nx} longitudes holds the zonal wavenumbers 1 .. {nx // 2}")
    if n > LEC_MAX_WAVENUMBERS:
        raise ValueError(f"--wavenumbers {n}: at most {LEC_MAX_WAVENUMBERS} (LEC_MAX_WAVENUMBERS)")


def _write_labelled_rows(path: str, first: str, columns, names, table) -> None:
    """``path``: the header line ``first`` and ``columns`` (strings), then one row of ``table`` per entry of ``names``, its label: in one
    ``format_level_table`` call where the labels have one width, else in one call per row (the same bytes)."""
    width = len(names[0])
    with open(path, "wb") as f:
        f.write((",".join([str(first)] + list(columns)) + "\n").encode("utf-8"))
        if all(len(x) == width for x in names):
            f.write(format_level_table(table, ("".join(names).encode("ascii"), width)))
        else:
            for name, row in zip(names, np.asarray(table, dtype=np.float64)):
                f.write(format_level_table(row[None, :], (name.encode("ascii"), len(name))))


def _write_time_table(path: str, first: str, columns, labels, times, table) -> None:
    """``path``: the header line ``first`` and ``columns`` (strings), then one row of ``table`` per time step under the fixed-width
    ``labels`` of ``time_labels`` -- or, for time stamps pandas prints at mixed widths, written by pandas itself, as for the per-level
    tables."""
    with open(path, "wb") as f:
        f.write((",".join([str(first)] + list(columns)) + "\n").encode("utf-8"))
        if labels[0] is not None:
            f.write(format_level_table(table, labels))
    if labels[0] is None:
        pd.DataFrame(table, index=pd.DatetimeIndex(times)).to_csv(path, mode="a", header=None)


def write_spectrum_csvs(box_obj: "BoxData", directory: str, time_name: str) -> None:
    """results_wavenumbers/<term>_n.csv for Ae, Ke, Ca, Ce, Ck -- and Ge, and the non-linear transfers S and L (W m-2, positive: wavenumber
    n gains), and the budget's BAe, BKe, dAedt, dKedt, RGe, RKe, when their spectra were asked for --: one row per time step -- the time labels and number formatting of the per-level
    tables --, columns 1 .. N and ``rest`` (the total minus the N shares), in the units of the results CSV."""
    from .constants import (SPECTRUM_BUDGET_TERMS, SPECTRUM_GENERATION_TERM, SPECTRUM_INTERACTION_TERMS, SPECTRUM_RESIDUAL_TERMS,
                            SPECTRUM_TENDENCY_FILES, SPECTRUM_TERMS)
    os.makedirs(directory, exist_ok=True)
    n = box_obj.spectrum.shape[2]
    columns = [str(k) for k in range(1, n + 1)] + ["rest"]
    labels = box_obj.row_labels("fixed")
    files = [(term, box_obj.spectrum[:, i, :], box_obj.spectrum_rest[:, i: i + 1]) for i, term in enumerate(SPECTRUM_TERMS)]
    if box_obj.spectrum_ge is not None:
        files.append((SPECTRUM_GENERATION_TERM, box_obj.spectrum_ge, box_obj.spectrum_ge_rest[:, None]))
    if getattr(box_obj, "spectrum_nl", None) is not None:
        files += [(term, box_obj.spectrum_nl[:, i, :], box_obj.spectrum_nl_rest[:, i: i + 1]) for i, term in enumerate(SPECTRUM_INTERACTION_TERMS)]
    if getattr(box_obj, "spectrum_b", None) is not None:
        for names, field in ((SPECTRUM_BUDGET_TERMS, "spectrum_b"), (SPECTRUM_TENDENCY_FILES, "spectrum_tendency"),
                             (SPECTRUM_RESIDUAL_TERMS, "spectrum_residual")):
            shares_, rest_ = getattr(box_obj, field), getattr(box_obj, field + "_rest")
            files += [(term, shares_[:, i, :], rest_[:, i: i + 1]) for i, term in enumerate(names)]
    for term, shares, rest in files:
        _write_time_table(os.path.join(directory, f"{term}_n.csv"), time_name, columns, labels, box_obj.time, np.concatenate([shares, rest], axis=1))


def write_section_csvs(box_obj: "BoxData", directory: str, time_name: str, vert_name: str) -> None:
    """results_sections/: for each of the ten terms ``<term>_lat_lv.csv`` -- the time mean of the term's latitude-pressure section, one row
    per level (labelled as the columns of the per-level tables are: the level in Pa as a float), one column per latitude of the box in
    degrees, in the units of the per-level table -- and ``<term>_lat.csv`` -- the section's vertical integral, one row per time step
    (the time labels and number formatting of the per-level tables), in the units of the results CSV.  With spectra also
    ``<term>_n_lat.csv`` for Ae, Ke, Ca, Ce, Ck (and Ge): the time mean of the vertical integral of every wavenumber's share, rows
    1 .. N and ``rest``."""
    from .constants import SECTION_TERMS
    os.makedirs(directory, exist_ok=True)
    lats = [repr(float(x)) for x in box_obj.section_latitudes]
    labels = box_obj.row_labels("fixed")
    level_names = [repr(float(p)) for p in box_obj.PressureData]
    for i, term in enumerate(SECTION_TERMS):
        _write_labelled_rows(os.path.join(directory, f"{term}_lat_lv.csv"), vert_name, lats, level_names, box_obj.section_mean[i])
        _write_time_table(os.path.join(directory, f"{term}_lat.csv"), time_name, lats, labels, box_obj.time, box_obj.section_lat[:, i, :])
    if box_obj.section_spec_lat is not None:
        nf, n1 = box_obj.section_spec_lat.shape[:2]
        names = [str(k) for k in range(1, n1)] + ["rest"]
        for i, term in enumerate(LECEngine.SECTION_SPEC_TERMS[:nf]):
            _write_labelled_rows(os.path.join(directory, f"{term}_n_lat.csv"), "n", lats, names, box_obj.section_spec_lat[i])


def write_map_csvs(box_obj: "BoxData", directory: str, time_name: str, lat_name: str) -> None:
    """results_maps/: for each of the six eddy terms ``<term>_lat_lon.csv`` -- the time mean of the term's map, one row per latitude of the
    box (labelled in degrees, as a float), one column per longitude of the box in degrees, in the units of the results CSV -- and
    ``<term>_lon.csv`` -- the map's area-weighted sum over latitude, one row per time step (the time labels and number formatting of the
    per-level tables), one column per longitude: a Hovmoeller diagram whose zonal average is the results CSV."""
    from .constants import MAP_TERMS
    os.makedirs(directory, exist_ok=True)
    lons = [repr(float(x)) for x in box_obj.map_longitudes]
    lat_names = [repr(float(x)) for x in box_obj.map_latitudes]
    labels = box_obj.row_labels("fixed")
    for i, term in enumerate(MAP_TERMS):
        _write_labelled_rows(os.path.join(directory, f"{term}_lat_lon.csv"), lat_name, lons, lat_names, box_obj.map_mean[i])
        _write_time_table(os.path.join(directory, f"{term}_lon.csv"), time_name, lons, labels, box_obj.time, box_obj.map_lon[:, i, :])


def composites_check(lat, lon, boxes, flag: str = "--composites", lat_too: bool = True) -> tuple:
    """The boxes of a track that is to be composited (index quadruples, one per time step) on the axes ``lat`` / ``lon``: all of ONE shape
    (ValueError naming the first step that differs and both shapes), at least 3 columns wide, on evenly spaced longitudes -- and, for the
    command line, latitudes (the offsets that label the files are those of the first step's box).  Host work only.  Returns (rows,
    columns) of every box."""
    from .tables import is_uniform
    boxes = [tuple(int(x) for x in b) for b in boxes]
    nyb, nxb = boxes[0][3] - boxes[0][2] + 1, boxes[0][1] - boxes[0][0] + 1
    for t, b in enumerate(boxes):
        h, w = b[3] - b[2] + 1, b[1] - b[0] + 1
        if (h, w) != (nyb, nxb):
            raise ValueError(f"{flag} needs boxes of ONE shape: the box of step {t} has {h} x {w} points (rows x columns), that of step 0 "
                             f"has {nyb} x {nxb} (a track near the data's edge, or one with width / length columns that change)")
    if nxb < 3:
        raise ValueError(f"{flag} needs boxes of at least 3 longitudes")
    if not is_uniform(np.asarray(lon, dtype=np.float64)):
        raise ValueError(f"{flag} needs evenly spaced longitudes")
    if lat_too and not is_uniform(np.asarray(lat, dtype=np.float64)):
        raise ValueError(f"{flag} needs evenly spaced latitudes: a box-relative row means the same offset at every step only there")
    return nyb, nxb


def composite_offsets(lat, lon, box):
    """(dlat [nyb], dlon [nxb]): the offsets in degrees of the box's rows and columns from its midpoint, lat[js + j] - (lat[js] + lat[jn]) / 2
    and likewise in longitude -- the labels of the composites' files, taken from the first step's box."""
    iw, ie, js, jn = (int(x) for x in box)
    la, lo = np.asarray(lat[js: jn + 1], dtype=np.float64), np.asarray(lon[iw: ie + 1], dtype=np.float64)
    return la - (la[0] + la[-1]) / 2, lo - (lo[0] + lo[-1]) / 2


def write_composite_csvs(box_obj: "BoxData", directory: str, time_name: str) -> None:
    """results_composites/: for each of the six eddy terms ``<term>_dlat_dlon.csv`` -- the time-mean system-relative composite, one row per
    box row, one column per box column, both labelled by the offset in degrees from the box's midpoint (``composite_offsets``), in the
    units of the results CSV -- and ``<term>_dlon.csv`` -- the composite's area-weighted sum over the box's rows, one row per time step
    (the time labels and number formatting of the per-level tables), one column per box column.  ``write_map_csvs``' format."""
    from .constants import MAP_TERMS
    write_composite_mean_csvs(box_obj.composite_mean, box_obj.composite_dlat, box_obj.composite_dlon, directory)
    lons = [repr(float(x)) for x in box_obj.composite_dlon]
    labels = box_obj.row_labels("fixed")
    for i, term in enumerate(MAP_TERMS):
        _write_time_table(os.path.join(directory, f"{term}_dlon.csv"), time_name, lons, labels, box_obj.time, box_obj.composite_lon[:, i, :])


def write_composite_mean_csvs(mean, dlat, dlon, directory: str, name: str = "{term}_dlat_dlon.csv") -> None:
    """``<term>_dlat_dlon.csv`` for each of the six eddy terms in ``directory``: ``mean`` [6, rows, columns], one row per box row, one
    column per box column, labelled by the offsets ``dlat`` / ``dlon``.  The time-mean files of ``write_composite_csvs``, and the ensemble
    mean of a batch of tracks (``lec_moving_batch``); ``name``: the files' name where it is another (the phases of a batch)."""
    from .constants import MAP_TERMS
    os.makedirs(directory, exist_ok=True)
    columns, lat_names = [repr(float(x)) for x in dlon], [repr(float(x)) for x in dlat]
    for i, term in enumerate(MAP_TERMS):
        _write_labelled_rows(os.path.join(directory, name.format(term=term)), "dlat", columns, lat_names, mean[i])


def composite_sections_check(lat, boxes, flag: str = "--composite-sections", lat_too: bool = True) -> int:
    """The boxes of a track whose system-relative sections are wanted (index quadruples, one per time step) on the latitude axis ``lat``:
    all of ONE row count (ValueError naming the first step that differs and both counts; widths may differ: a row record holds the zonal
    means over its own box's width), at least 2 rows -- and, for the command line, evenly spaced latitudes (the offsets that label the
    files are those of the first step's box).  Longitudes are not looked at.  Host work only.  Returns the row count of every box."""
    from .tables import is_uniform
    boxes = [tuple(int(x) for x in b) for b in boxes]
    nyb = boxes[0][3] - boxes[0][2] + 1
    for t, b in enumerate(boxes):
        if b[3] - b[2] + 1 != nyb:
            raise ValueError(f"{flag} needs boxes of ONE row count: the box of step {t} has {b[3] - b[2] + 1} rows, that of step 0 has {nyb} "
                             "(a track near the data's edge, or one whose length column changes)")
    if nyb < 2:
        raise ValueError(f"{flag} needs boxes of at least 2 latitudes")
    if lat_too and not is_uniform(np.asarray(lat, dtype=np.float64)):
        raise ValueError(f"{flag} needs evenly spaced latitudes: a box-relative row means the same offset at every step only there")
    return nyb


def write_composite_section_csvs(box_obj: "BoxData", directory: str, time_name: str, vert_name: str) -> None:
    """results_composite_sections/: for each of the ten terms ``<term>_dlat_lv.csv`` -- the time mean over the system's life of the term's
    system-relative latitude-pressure section, one row per level (labelled as ``write_section_csvs`` labels them), one column per box row
    labelled by its offset in degrees from the box's midpoint (``composite_offsets``, first step's box), in the units of the per-level
    table -- and ``<term>_dlat.csv`` -- the section's vertical integral, one row per time step, in the units of the results CSV.
    ``write_section_csvs``' number and time formatting."""
    from .constants import SECTION_TERMS
    os.makedirs(directory, exist_ok=True)
    head = [repr(float(x)) for x in box_obj.composite_section_dlat]
    labels = box_obj.row_labels("fixed")
    level_names = [repr(float(p)) for p in box_obj.PressureData]
    for i, term in enumerate(SECTION_TERMS):
        _write_labelled_rows(os.path.join(directory, f"{term}_dlat_lv.csv"), vert_name, head, level_names, box_obj.composite_section_mean[i])
        _write_time_table(os.path.join(directory, f"{term}_dlat.csv"), time_name, head, labels, box_obj.time,
                          box_obj.composite_section_lat[:, i, :])


def _write_lon_lv_csvs(mean, columns, level_names, directory: str, suffix: str, vert_name: str) -> None:
    """``<term><suffix>`` for each of the six eddy terms in ``directory``: ``mean`` [6, levels, columns], one row per level labelled as
    ``write_section_csvs`` labels them, one column per entry of ``columns`` (degrees).  The number format of the ``--sections`` files."""
    from .constants import MAP_TERMS
    os.makedirs(directory, exist_ok=True)
    columns = [repr(float(x)) for x in columns]
    for i, term in enumerate(MAP_TERMS):
        _write_labelled_rows(os.path.join(directory, f"{term}{suffix}"), vert_name, columns, level_names, mean[i])


def write_lon_section_csvs(box_obj: "BoxData", directory: str, vert_name: str) -> None:
    """results_lon_sections/: for each of the six eddy terms ``<term>_lon_lv.csv`` -- the time mean of the term's longitude-pressure
    section, one row per level (labelled as ``write_section_csvs`` labels them), one column per longitude of the box in degrees, in the
    units of ``<term>_lat_lv.csv``.  ``write_section_csvs``' number formatting."""
    _write_lon_lv_csvs(box_obj.lonsection_mean, box_obj.lonsection_longitudes, [repr(float(p)) for p in box_obj.PressureData], directory,
                       "_lon_lv.csv", vert_name)


def write_composite_lon_section_csvs(box_obj: "BoxData", directory: str, vert_name: str) -> None:
    """results_composite_lon_sections/: for each of the six eddy terms ``<term>_dlon_lv.csv`` -- the time mean over the system's life of
    the term's system-relative longitude-pressure section, one row per level, one column per box column labelled by its offset in degrees
    from the box's midpoint (``composite_offsets``, first step's box)."""
    _write_lon_lv_csvs(box_obj.composite_lonsection_mean, box_obj.composite_lonsection_dlon, [repr(float(p)) for p in box_obj.PressureData],
                       directory, "_dlon_lv.csv", vert_name)


def ring_hint(lon, box):
    """The line a plain -f run logs when its box spans the whole longitude axis of a ring (None otherwise): the run treats the circle
    as a limited area, --periodic closes it."""
    from .follow import ring_error
    if box[0] != 0 or box[1] != len(lon) - 1 or ring_error(lon):
        return None
    return (f"the box spans all {len(lon)} longitudes of a full ring, but is evaluated as a limited area (half weight on the two seam columns, "
            "one-sided d/dlon there, an east-west boundary flux): --periodic closes the circle")


def host_fields(data: ds.LECDataset, variable_list_df: pd.DataFrame):
    """The five field arrays of a host-prepared data set in SI units (geopotential as stored), their common storage dtype and
    the geopotential's factor to m^2/s^2."""
    geo_role = "Geopotential" if "Geopotential" in variable_list_df.index else "Geopotential Height"
    roles = ["Air Temperature", "Eastward Wind Component", "Northward Wind Component", "Omega Velocity", geo_role]
    arrays = []
    for role in roles:
        a = data.variables[str(variable_list_df.loc[role]["Variable"])]
        if a.dtype.kind != "f":                     # an unpacked integer variable: xarray would compute with it as it is
            a = a.astype(np.float32 if a.dtype.itemsize <= 2 else np.float64)
        scale = ds.field_scale(variable_list_df, role)
        if role != geo_role and scale != 1.0:
            a = a * a.dtype.type(scale)
        arrays.append(a)
    # a file may mix dtypes (float32 T, u, v with an int16-packed z that decodes to float64): the engine wants one storage
    # dtype, the widest of them -- widening is exact, and all arithmetic is fp64 anyway (xarray would promote pairwise)
    common = np.result_type(*[a.dtype for a in arrays])
    return arrays, common, ds.field_scale(variable_list_df, geo_role)


def time_labels(times, method: str):
    """The first field of every row of a per-level table, as the reference's pandas call prints it, as one byte string of
    fixed-width labels: the moving framework formats its index itself ("%Y-%m-%d %H:%M:%S", conversion_terms.py:299-300); the fixed
    framework leaves a DatetimeIndex to pandas, which prints dates alone when every stamp is a midnight -- taken from pandas itself
    (an index without columns through to_csv) so that the rule is pandas' own."""
    idx = pd.DatetimeIndex(times)
    if method == "fixed":
        labels = pd.DataFrame(index=idx).to_csv(header=None).splitlines()
    else:
        labels = list(idx.strftime("%Y-%m-%d %H:%M:%S"))
    width = len(labels[0]) if labels else 0
    if any(len(x) != width for x in labels) or any(("," in x or '"' in x) for x in labels):
        return None, 0                           # (stamps pandas prints at mixed widths: the caller falls back to pandas itself)
    return "".join(labels).encode("ascii"), width


def format_level_table(table, labels) -> bytes:
    """`table` [time, level] (float64) as the lines DataFrame.to_csv(header=None) writes for it (lec_format_csv_rows)."""
    import ctypes as C
    from . import _lib
    blob, width = labels
    a = np.ascontiguousarray(table, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("a per-level table is [time, level]")
    rows, cols = a.shape
    if blob is None or rows * width != len(blob):
        raise ValueError("one fixed-width label per row")
    lib = _lib.load()
    cap = rows * (width + 27 * cols + 1)
    out = C.create_string_buffer(max(cap, 1))
    n = lib.lec_format_csv_rows(a.ctypes.data, rows, cols, cols, blob, width, C.addressof(out), cap)
    if n < 0:
        _lib.check(1, "lec_format_csv_rows")
    return out.raw[:n]


class _Terms:
    """Shared plumbing of the four analysis classes: hand out a finished series and append its
    per-level CSV rows exactly where the reference's calc_* would (``_save_vertical_levels``,
    e.g. conversion_terms.py:287-308)."""

    def __init__(self, box_obj: BoxData, method: str, app_logger=None):
        if method not in ("fixed", "moving"):
            raise ValueError("method must be 'fixed' or 'moving'")
        self.box_obj, self.method, self.app_logger = box_obj, method, app_logger

    def _save_vertical_levels(self, name: str):
        """One table appended to its CSV file: byte for byte what the reference's pandas call writes (conversion_terms.py:287-308:
        DataFrame.to_csv(mode="a", header=None) -- float cells as repr(float), NaN as an empty field), formatted for the whole
        series in one call of the library (lec_format_csv_rows) instead of one Python object per cell."""
        b = self.box_obj
        path = f"{b.results_subdirectory_vertical_levels}/{name}_{b.VerticalCoordIndexer}.csv"
        table = b.levels[name]
        if self.method == "fixed" and name in ("Cz_1", "Ce_1"):        # level-only term: written transposed (conversion_terms.py:293-294)
            df = pd.DataFrame({b.VerticalCoordIndexer: b.PressureData, name: table[0]}).T
            df.to_csv(path, mode="a", header=None)
            return
        labels = b.row_labels(self.method)
        if labels[0] is None:                    # time stamps pandas prints at mixed widths (sub-second steps): pandas writes the table
            idx = pd.DatetimeIndex(b.time) if self.method == "fixed" else pd.DatetimeIndex(b.time).strftime("%Y-%m-%d %H:%M:%S")
            pd.DataFrame(table, index=idx, columns=b.PressureData).to_csv(path, mode="a", header=None)
            return
        with open(path, "ab") as f:
            f.write(format_level_table(table, labels))

    def _series(self, name: str, tables):
        for t in tables:
            self._save_vertical_levels(t)
        s = self.box_obj.scalars[name]
        return s


class EnergyContents(_Terms):
    """energy_contents.py:99-165"""
    def calc_az(self): return self._series("Az", ["Az"])
    def calc_ae(self): return self._series("Ae", ["Ae"])
    def calc_kz(self): return self._series("Kz", ["Kz"])
    def calc_ke(self): return self._series("Ke", ["Ke"])


class ConversionTerms(_Terms):
    """conversion_terms.py:103-245"""
    def calc_ca(self): return self._series("Ca", ["Ca_1", "Ca_2", "Ca"])
    def calc_ce(self): return self._series("Ce", ["Ce_1", "Ce_2", "Ce"])
    def calc_cz(self): return self._series("Cz", ["Cz_1", "Cz_2", "Cz"])
    def calc_ck(self): return self._series("Ck", ["Ck_1", "Ck_2", "Ck_3", "Ck_4", "Ck_5", "Ck"])


class BoundaryTerms(_Terms):
    """boundary_terms.py:125-418"""
    def calc_baz(self): return self._series("BAz", [])
    def calc_bae(self): return self._series("BAe", [])
    def calc_bkz(self): return self._series("BKz", [])
    def calc_bke(self): return self._series("BKe", [])
    def calc_boz(self): return self._series("BΦZ", [])
    def calc_boe(self): return self._series("BΦE", [])


class GenerationDissipationTerms(_Terms):
    """generation_and_dissipation_terms.py:122-188"""
    def calc_gz(self): return self._series("Gz", ["Gz"])
    def calc_ge(self): return self._series("Ge", ["Ge"])

    def calc_dz(self):
        raise NotImplementedError("Dz needs friction velocities; the reference marks it unfinished "
                                  "(generation_and_dissipation_terms.py:158) -- run with -r")

    calc_de = calc_dz


def _create_level_csvs(directory, time_name, vert_name, level_pa):
    """lec_fixed_framework.py:172-197 / lec_moving_framework.py:583-611"""
    for term in LEVEL_TERMS:
        columns = [time_name] + [float(i) for i in level_pa]
        pd.DataFrame(columns=columns).to_csv(Path(directory, f"{term}_{vert_name}.csv"), index=None)


def _log_ingest(box_obj, app_logger):
    st = getattr(box_obj, "ingest_stats", None)
    if st:
        app_logger.info("Device ingest: %.1f MB over the link in %d chunk(s) of %d step(s), staging %s, inflate %s, storage %s, device buffers %.2f GB" % (
            st["bytes_moved"] / 1e6, st["chunks"], st["chunk_steps"], st["staging"], st.get("inflate", "none"), st["storage"],
            st.get("device_buffer_bytes", 0) / 1e9))
        if "seconds" in st:
            app_logger.info("Device ingest seconds: " + ", ".join(f"{k} {v:.3f}" for k, v in st["seconds"].items()) +
                            (f"; {st['register_calls']} registrations, {st['registered_bytes'] / 1e9:.2f} GB" if "register_calls" in st else ""))


def _compute_all(box_obj, method, app_logger):
    _log_ingest(box_obj, app_logger)
    ec = EnergyContents(box_obj, method, app_logger)
    out = {"Az": ec.calc_az(), "Ae": ec.calc_ae(), "Kz": ec.calc_kz(), "Ke": ec.calc_ke()}
    ct = ConversionTerms(box_obj, method, app_logger)
    out.update({"Cz": ct.calc_cz(), "Ca": ct.calc_ca(), "Ck": ct.calc_ck(), "Ce": ct.calc_ce()})
    bt = BoundaryTerms(box_obj, method, app_logger)
    out.update({"BAz": bt.calc_baz(), "BAe": bt.calc_bae(), "BKz": bt.calc_bkz(), "BKe": bt.calc_bke(),
                "BΦZ": bt.calc_boz(), "BΦE": bt.calc_boe()})
    gd = GenerationDissipationTerms(box_obj, method, app_logger)
    out.update({"Gz": gd.calc_gz(), "Ge": gd.calc_ge()})
    return out


def lec_fixed(data: ds.LECDataset, variable_list_df: pd.DataFrame, results_subdirectory: str,
              results_subdirectory_vertical_levels: str, app_logger, args):
    """Eulerian framework, lec_fixed_framework.py:30-303 (plots are out of scope)."""
    app_logger.info("Computing energetics using fixed framework (MI355X HIP engine)...")
    min_lon, max_lon, min_lat, max_lat = ds.read_box_limits(args.box_limits)
    time_name = variable_list_df.loc["Time"]["Variable"]
    vert_name = variable_list_df.loc["Vertical Level"]["Variable"]
    app_logger.info(f"Bounding box: lon=[{min_lon}, {max_lon}], lat=[{min_lat}, {max_lat}]")
    shard = getattr(args, "shard", None)
    root = shard is None or shard.root
    periodic = bool(getattr(args, "periodic", False))
    if periodic:        # refused here, before a file is written: no ring, or limits that do not span it
        from .tables import box_indices
        ring_box_check(data.lon, box_indices(data.lat, data.lon, min_lon, max_lon, min_lat, max_lat))
    wavenumbers = getattr(args, "wavenumbers", None)
    if wavenumbers is not None:     # likewise: N must fit the ring the file holds
        if not periodic:
            raise ValueError("--wavenumbers goes with -f --periodic")
        wavenumbers_check(int(wavenumbers), len(data.lon))
    generation = bool(getattr(args, "wavenumbers_generation", False))
    if generation and wavenumbers is None:
        raise ValueError("--wavenumbers-generation goes with --wavenumbers N")
    interactions = bool(getattr(args, "wavenumbers_interactions", False))
    if interactions and wavenumbers is None:
        raise ValueError("--wavenumbers-interactions goes with --wavenumbers N")
    budget = bool(getattr(args, "wavenumbers_budget", False))
    if budget and wavenumbers is None:
        raise ValueError("--wavenumbers-budget goes with --wavenumbers N")
    if budget and len(data.time) < 2:
        raise ValueError("--wavenumbers-budget: the tendencies are finite differences in time: the series needs at least 2 time steps")
    sections = bool(getattr(args, "sections", False))
    if sections and shard is not None:
        raise ValueError("--sections runs on one GPU")
    maps = bool(getattr(args, "maps", False))
    if maps:            # likewise refused before a file is written
        from .ingest import StreamedDataset
        from .tables import box_indices, is_uniform
        if shard is not None:
            raise ValueError("--maps runs on one GPU")
        if isinstance(data, StreamedDataset):
            raise ValueError("--maps prepares the data on the host: --ingest device / --device-ingest is not supported for the maps")
        iw, ie, _, _ = box_indices(data.lat, data.lon, min_lon, max_lon, min_lat, max_lat)
        if ie - iw + 1 < 3:
            raise ValueError("--maps needs a box of at least 3 longitudes")
        if not periodic and not is_uniform(np.asarray(data.lon, dtype=np.float64)):
            raise ValueError("--maps needs evenly spaced longitudes")
    lon_sections = bool(getattr(args, "lon_sections", False))
    if lon_sections:    # likewise refused before a file is written
        from .ingest import StreamedDataset
        from .tables import box_indices, is_uniform
        if shard is not None:
            raise ValueError("--lon-sections runs on one GPU")
        if isinstance(data, StreamedDataset):
            raise ValueError("--lon-sections prepares the data on the host: --ingest device / --device-ingest is not supported for the "
                             "longitude-pressure sections")
        iw, ie, _, _ = box_indices(data.lat, data.lon, min_lon, max_lon, min_lat, max_lat)
        if ie - iw + 1 < 3:
            raise ValueError("--lon-sections needs a box of at least 3 longitudes")
        if not periodic and not is_uniform(np.asarray(data.lon, dtype=np.float64)):
            raise ValueError("--lon-sections needs evenly spaced longitudes")
    if root:
        _create_level_csvs(results_subdirectory_vertical_levels, time_name, vert_name, data.level)
    try:
        box_obj = BoxData(data, variable_list_df, min_lon, max_lon, min_lat, max_lat, args, results_subdirectory,
                          results_subdirectory_vertical_levels, periodic=periodic, wavenumbers=wavenumbers,
                          spectrum_generation=generation, **({"spectrum_interactions": True} if interactions else {}),
                          **({"spectrum_budget": True} if budget else {}), **({"sections": True} if sections else {}),
                          **({"maps": True} if maps else {}), **({"lon_sections": True} if lon_sections else {}))
    except Exception:
        app_logger.exception("An exception occurred while creating BoxData object")
        raise
    phases.mark("ingest_compute_gather")
    if box_obj.result is None:              # time-sharded run: rank 0 holds the gathered series and writes every file
        return None
    if periodic:
        app_logger.info(f"--periodic: the box is a ring of {len(data.lon)} longitudes, lat=[{box_obj.southern_limit}, {box_obj.northern_limit}], "
                        f"closed xlength {box_obj.xlength!r} rad (lec_rowstats_ring)")
    else:
        hint = ring_hint(data.lon, box_obj.boxes[0])
        if hint:
            app_logger.info("Bounding box: " + hint)
    if int(box_obj.nanflag.sum()):
        app_logger.warning("NaN level values were interpolated/dropped per time step (_handle_nans semantics)")
    terms = _compute_all(box_obj, "fixed", app_logger)
    app_logger.info("Computed energy, conversion, boundary and generation terms")
    if wavenumbers is not None:
        spectrum_directory = os.path.join(results_subdirectory, "results_wavenumbers")
        write_spectrum_csvs(box_obj, spectrum_directory, time_name)
        app_logger.info(f"--wavenumbers: Ae, Ke, Ca, Ce, Ck split into the zonal wavenumbers 1 .. {int(wavenumbers)} of the ring's "
                        f"{len(data.lon)} longitudes (lec_rowspec_kernel: N = {int(wavenumbers)}, nx = {len(data.lon)}); written to {spectrum_directory}")
        if generation:
            app_logger.info(f"--wavenumbers-generation: Ge split likewise, Q evaluated at every point of the ring's rows "
                            f"(lec_rowspec_q_kernel: N = {int(wavenumbers)}, nx = {len(data.lon)}); written to {spectrum_directory}")
        if interactions:
            app_logger.info(f"--wavenumbers-interactions: the non-linear eddy-eddy transfers S(n) into Ae and L(n) into Ke, the advective "
                            f"tendencies evaluated at every point of the ring's rows (lec_rowspec_nl_kernel: N = {int(wavenumbers)}, "
                            f"nx = {len(data.lon)}); written to {spectrum_directory}")
        if budget:
            app_logger.info(f"--wavenumbers-budget: BAe(n) and BKe(n) from the shares of the four triple products of the ring's rows, "
                            f"the tendencies dAe(n)/dt, dKe(n)/dt and the residuals RGe(n), RKe(n) (lec_rowspec_b_kernel: N = {int(wavenumbers)}, "
                            f"nx = {len(data.lon)}); written to {spectrum_directory}")
    if sections:
        section_directory = os.path.join(results_subdirectory, "results_sections")
        write_section_csvs(box_obj, section_directory, time_name, vert_name)
        app_logger.info(f"--sections: the latitude-pressure sections of Az, Ae, Kz, Ke, Cz, Ca, Ck, Ce, Gz, Ge on the box's "
                        f"{len(box_obj.section_latitudes)} rows (lec_sections); written to {section_directory}")
    if maps:
        map_directory = os.path.join(results_subdirectory, "results_maps")
        write_map_csvs(box_obj, map_directory, time_name, variable_list_df.loc["Latitude"]["Variable"])
        app_logger.info(f"--maps: the longitude-resolved maps of Ae, Ke, Ca, Ce, Ck, Ge on the box's {len(box_obj.map_latitudes)} x "
                        f"{len(box_obj.map_longitudes)} points (lec_maps); written to {map_directory}")
    if lon_sections:
        lonsec_directory = os.path.join(results_subdirectory, "results_lon_sections")
        write_lon_section_csvs(box_obj, lonsec_directory, vert_name)
        app_logger.info(f"--lon-sections: the longitude-pressure sections of Ae, Ke, Ca, Ce, Ck, Ge on the box's {len(data.level)} levels x "
                        f"{len(box_obj.lonsection_longitudes)} longitudes (lec_lonsections); written to {lonsec_directory}")
    df = pd.DataFrame(index=pd.DatetimeIndex(data.time))
    for col in FIXED_COLUMNS:                       # BΦZ / BΦE are computed, then dropped (:252-253,:287-290)
        df[col] = terms[col]
    full = budgets_and_residuals({c: df[c].values for c in df.columns}, data.time_s, residuals=True)
    for col in full:
        if col not in df.columns:
            df[col] = full[col]
    if getattr(args, "outname", None):
        results_filename = args.outname
    else:
        results_filename = os.path.basename(args.infile).split(".nc")[0] + "_fixed_results"
    results_file = Path(results_subdirectory, f"{results_filename}.csv")
    df.to_csv(results_file)
    phases.mark("csv_writes")
    app_logger.info(f"Results saved to {results_file}")
    if getattr(args, "plots", False):
        app_logger.warning("-p/--plots: plotting is out of scope of the MI355X engine; the CSVs feed the reference's plot scripts unchanged")
    return df


def get_limits(track: pd.DataFrame, t):
    """get_limits (lec_moving_framework.py:199-266), track branch: nearest track row in time,
    default 15 x 15 degree box unless the track has width/length columns."""
    row = track.iloc[int(np.argmin(np.abs(track.index - t)))]
    clat, clon = float(row["Lat"]), float(row["Lon"])
    width, length = row.get("width", 15), row.get("length", 15)
    return {"datestr": pd.to_datetime(t).strftime("%Y-%m-%d-%H%M"), "central_lat": clat, "central_lon": clon,
            "length": length, "width": width, "min_lon": clon - width / 2, "max_lon": clon + width / 2,
            "min_lat": clat - length / 2, "max_lat": clat + length / 2}


def lec_moving(data: ds.LECDataset, variable_list_df: pd.DataFrame, dTdt, results_subdirectory: str,
               figures_directory: str, results_subdirectory_vertical_levels: str, app_logger, args):
    """Semi-Lagrangian framework, lec_moving_framework.py:546-745.  ``dTdt`` may be None: the engine then
    differentiates T over the dataset's (track-selected) time axis on the device, which is what
    run_lec_analysis computes (lorenzcycletoolkit.py:184-186)."""
    app_logger.info("Computing energetics using moving framework (MI355X HIP engine)...")
    # -c/--choose is -t on the track the GPU wrote (follow.write_choose_track: args.choose_track names it)
    trackfile = getattr(args, "choose_track", None) or (args.trackfile if getattr(args, "track", False) else None)
    if not trackfile:
        raise ValueError("the moving framework needs a track: -t --trackfile FILE, or -c, whose track follow.write_choose_track writes first")
    time_name = variable_list_df.loc["Time"]["Variable"]
    vert_name = variable_list_df.loc["Vertical Level"]["Variable"]
    shard = getattr(args, "shard", None)
    root = shard is None or shard.root
    composites = bool(getattr(args, "composites", False))
    if composites:      # refused before a file is written
        from .ingest import StreamedDataset
        from .tables import box_indices
        if shard is not None:
            raise ValueError("--composites runs on one GPU")
        if isinstance(data, StreamedDataset):
            raise ValueError("--composites prepares the data on the host: --ingest device / --device-ingest is not supported for the composites")
        track0 = ds.track_on_axis(ds.read_track(trackfile, app_logger), data.lon)
        lims = [get_limits(track0, t) for t in pd.DatetimeIndex(data.time)]
        composites_check(data.lat, data.lon, [box_indices(data.lat, data.lon, l["min_lon"], l["max_lon"], l["min_lat"], l["max_lat"]) for l in lims])
    composite_sections = bool(getattr(args, "composite_sections", False))
    if composite_sections:      # refused before a file is written
        from .tables import box_indices
        if shard is not None:
            raise ValueError("--composite-sections runs on one GPU")
        track0 = ds.track_on_axis(ds.read_track(trackfile, app_logger), data.lon)
        lims = [get_limits(track0, t) for t in pd.DatetimeIndex(data.time)]
        composite_sections_check(data.lat, [box_indices(data.lat, data.lon, l["min_lon"], l["max_lon"], l["min_lat"], l["max_lat"]) for l in lims])
    composite_lon_sections = bool(getattr(args, "composite_lon_sections", False))
    if composite_lon_sections:      # refused before a file is written
        from .ingest import StreamedDataset
        from .tables import box_indices
        if shard is not None:
            raise ValueError("--composite-lon-sections runs on one GPU")
        if isinstance(data, StreamedDataset):
            raise ValueError("--composite-lon-sections prepares the data on the host: --ingest device / --device-ingest is not supported "
                             "for the composite longitude-pressure sections")
        track0 = ds.track_on_axis(ds.read_track(trackfile, app_logger), data.lon)
        lims = [get_limits(track0, t) for t in pd.DatetimeIndex(data.time)]
        composites_check(data.lat, data.lon, [box_indices(data.lat, data.lon, l["min_lon"], l["max_lon"], l["min_lat"], l["max_lat"]) for l in lims],
                         flag="--composite-lon-sections")
    if root:
        _create_level_csvs(results_subdirectory_vertical_levels, time_name, vert_name, data.level)
    times = pd.DatetimeIndex(data.time)
    track = ds.track_on_axis(ds.read_track(trackfile, app_logger), data.lon)      # (across the +-180 meridian: Lon mod 360, as the axis)
    # handle_track_file (lec_moving_framework.py:58-160)
    if track.index[0] < times.min() or track.index[-1] > times.max():
        raise ValueError("Track time limits do not match with data time limits.")
    for name, coord in (("Lon", data.lon), ("Lat", data.lat)):
        word = "longitude" if name == "Lon" else "latitude"
        if track[name].max() > coord.max():
            raise ValueError(f"Track file {word} max limit ({track[name].max():.2f}) exceeds data max {word} limit ({float(coord.max()):.2f}).")
        if track[name].min() < coord.min():
            raise ValueError(f"Track file {word} min limit ({track[name].min():.2f}) is below data min {word} limit ({float(coord.min()):.2f}).")
    if 85000.0 not in data.level:
        raise KeyError(85000)                                   # lec_moving_framework.py:653-657 selects 85000 Pa exactly
    limits = [get_limits(track, t) for t in times]
    boxes = [(l["min_lon"], l["max_lon"], l["min_lat"], l["max_lat"]) for l in limits]
    box_obj = BoxData(data, variable_list_df, args=args, results_subdirectory=results_subdirectory,
                      results_subdirectory_vertical_levels=results_subdirectory_vertical_levels, dTdt=dTdt,
                      boxes_limits=boxes, **({"composites": True} if composites else {}),
                      **({"composite_sections": True} if composite_sections else {}),
                      **({"composite_lon_sections": True} if composite_lon_sections else {}))
    phases.mark("ingest_compute_gather")
    if composite_lon_sections:
        clon_directory = os.path.join(results_subdirectory, "results_composite_lon_sections")
        write_composite_lon_section_csvs(box_obj, clon_directory, vert_name)
        app_logger.info(f"--composite-lon-sections: the system-relative longitude-pressure sections of Ae, Ke, Ca, Ce, Ck, Ge on the boxes' "
                        f"{len(data.level)} levels x {len(box_obj.composite_lonsection_dlon)} box-relative columns "
                        f"(lec_composite_lonsections); written to {clon_directory}")
    if composite_sections:
        csec_directory = os.path.join(results_subdirectory, "results_composite_sections")
        write_composite_section_csvs(box_obj, csec_directory, time_name, vert_name)
        app_logger.info(f"--composite-sections: the system-relative latitude-pressure sections of Az, Ae, Kz, Ke, Cz, Ca, Ck, Ce, Gz, Ge on "
                        f"the boxes' {len(box_obj.composite_section_dlat)} box-relative rows (lec_composite_sections); written to {csec_directory}")
    if composites:
        composite_directory = os.path.join(results_subdirectory, "results_composites")
        write_composite_csvs(box_obj, composite_directory, time_name)
        app_logger.info(f"--composites: the system-relative composites of Ae, Ke, Ca, Ce, Ck, Ge on the boxes' {len(box_obj.composite_dlat)} x "
                        f"{len(box_obj.composite_dlon)} box-relative points (lec_composite); written to {composite_directory}")
    # 850-hPa diagnostics of every box (lec_moving_framework.py:650-709); a time-sharded rank does its own steps, rank 0 gets them all
    from .diagnostics import track_diagnostics
    form = getattr(args, "vorticity_form", None) or "metpy_no_crs"
    positions = track_diagnostics(data, variable_list_df, limits, track, use_track_zeta=bool(getattr(args, "zeta", False)),
                                  device=_device(args), shard=shard, formulation=form, slices=getattr(box_obj, "level_slices", None))
    phases.mark("track_diagnostics")
    if box_obj.result is None:              # time-sharded run: rank 0 holds the gathered series and writes every file
        return None
    return _write_moving_results(box_obj, times, data.time_s, limits, positions, results_subdirectory, form, app_logger, args,
                                 lon_origin=ds.lon_origin_of_axis(data.lon))


def _write_moving_results(box_obj, times, time_s, limits, positions, results_subdirectory, form, app_logger, args, lon_origin=0.0):
    """The files of one track (after its numbers exist): terms -> DataFrame -> budgets -> results CSV -> trackfile.  ``box_obj``:
    a BoxData or anything with its series and per-level plumbing (``_TrackResult``).  ``lon_origin`` 180: the run's longitudes are on
    0..360 (dataset.track_lon_origin); every longitude written is wrapped back into [-180, 180)."""
    terms = _compute_all(box_obj, "moving", app_logger)
    df = pd.DataFrame({c: terms[c] for c in MOVING_COLUMNS}, index=times, dtype=float)
    full = budgets_and_residuals({c: df[c].values for c in df.columns}, time_s,
                                 residuals=bool(getattr(args, "residuals", False)))
    for col in full:
        if col not in df.columns:
            df[col] = full[col]
    method = "choose" if getattr(args, "choose_track", None) else "track"       # (-c: the same files under the chooser's names)
    infile_name = os.path.basename(args.infile).split(".nc")[0]
    results_file = os.path.join(results_subdirectory, f"{infile_name}_{method}_results.csv")
    df.to_csv(results_file)
    app_logger.info(f"Results saved to {results_file}")
    # 850-hPa diagnostics of every box (lec_moving_framework.py:650-709); parity unpinned, see diagnostics.py
    app_logger.info(f"850 hPa track diagnostics (min_max_zeta_850, min_hgt_850, max_wind_850) on the GPU (lec_track_diag), vorticity formulation "
                    f"'{form}' (" + ("plain dv/dx - du/dy on great-circle grid distances, a = 6370997 m: MetPy 1.6.2 for DataArrays without a CRS, as the "
                                     "reference passes them" if form == "metpy_no_crs" else "spherical: dv/dx - du/dy + u tan(phi) / Re") +
                    "); NOT pinned against MetPy itself (--vorticity-form selects the other formulation)")
    out_track = pd.DataFrame([{**l, **p} for l, p in zip(limits, positions)])
    out_track = out_track.rename(columns={"datestr": "time", "central_lat": "Lat", "central_lon": "Lon"})
    if lon_origin:
        for col in [c for c in out_track.columns if c in ("Lon", "min_lon", "max_lon") or c.endswith("_lon")]:
            out_track[col] = ds.wrap180(out_track[col].values)
    out_track.to_csv(os.path.join(results_subdirectory, f"{infile_name}_{method}_trackfile"), index=False, sep=";")
    phases.mark("csv_writes")
    return results_file, df


class _TrackResult:
    """One track's share of a batch (``lec_moving_batch``), shaped like the BoxData the per-level writers read."""

    def __init__(self, data: ds.LECDataset, variable_list_df: pd.DataFrame, result: LECResult, results_subdirectory: str,
                 results_subdirectory_vertical_levels: str):
        self.results_subdirectory = results_subdirectory
        self.results_subdirectory_vertical_levels = results_subdirectory_vertical_levels
        self.VerticalCoordIndexer = variable_list_df.loc["Vertical Level"]["Variable"]
        self.PressureData = data.level
        self.time = data.time
        self._row_labels = {}
        self.result = result
        self.scalars = result.scalars_dict()
        self.levels = result.levels_dict()
        self.nanflag = result.nanflag.cpu().numpy()

    row_labels = BoxData.row_labels


def lec_moving_batch(data: ds.LECDataset, variable_list_df: pd.DataFrame, plan, directories, app_logger, args, batch_dir=None,
                     composite_shapes=None):
    """Many tracks over one data set (``batch.prepare_union``): ONE upload of the union cubes, one stage-1 + stage-2 call per group of
    tracks with equal record extents (``LECEngine.compute(steps=...)``), then every track's files written by the code ``lec_moving``
    writes them with.  ``directories``: per track (results, figures, vertical levels).  The files of every track are byte for byte
    those of its own ``-t --trackfile`` run.  Returns [(results file, DataFrame)] in batch order.
    ``composite_shapes`` (``--batch-composites``): what ``batch.composites_check(plan)`` returned, {(rows, columns): tracks}.  Every
    group's call then also composites its tracks (``compute(batch_composites=...)``); every track's tree gets the ``results_composites/``
    of its own ``--composites`` run, and ``batch_dir`` the ensemble mean of every box shape (``_write_batch_composites``).  The check
    has left every track with one box shape on evenly spaced longitudes, so the plan's groups ARE those shapes.
    ``args.batch_composites_phase`` (``--batch-composites-phase``, with ``composite_shapes``): a clock ``lifetime:B`` / ``peak:L``; the
    groups' calls also fold the composites over the clock's ranges (``batch.phase_ranges``, ``compute(batch_composite_phases=...)``) and
    every ensemble directory gets ``phases/`` (``_write_batch_phases``).  The peak clock needs every track's ``min_max_zeta_850``: the
    tracks' 850-hPa diagnostics are then evaluated before the groups' calls, and the write loop reuses them."""
    from . import batch as bt
    from .diagnostics import track_diagnostics
    dev = _device(args)
    time_name = variable_list_df.loc["Time"]["Variable"]
    vert_name = variable_list_df.loc["Vertical Level"]["Variable"]
    arrays, common, phi_scale = host_fields(data, variable_list_df)
    with_composites = composite_shapes is not None
    clock = bt.parse_phase_clock(args.batch_composites_phase) if with_composites and getattr(args, "batch_composites_phase", None) else None
    mem = bt.device_bytes(plan, len(arrays), np.dtype(common).itemsize,
                          **({"phase_bins": clock[1] if clock[0] == "lifetime" else 2 * clock[1] + 1} if clock else {}))
    need = mem["total"]
    free = torch.cuda.mem_get_info(dev)[0]
    if need > free // 2:
        raise MemoryError(f"the batch needs {need / 1e9:.2f} GB of device memory (union cubes {mem['cubes'] / 1e9:.2f} GB, row records of the "
                          f"largest group {mem['records'] / 1e9:.2f} GB, results {mem['results'] / 1e9:.2f} GB), more than half of the "
                          f"{free / 1e9:.2f} GB free: run the tracks in smaller batches")
    engine = LECEngine(data.lat, data.lon, data.level, device=dev)
    cubes = [torch.as_tensor(np.ascontiguousarray(a, dtype=common)).to(dev) for a in arrays]
    app_logger.info(f"Batch of {len(plan.tracks)} tracks: union of {len(plan.tpos)} time steps on a {len(plan.lat)} x {len(plan.lon)} crop "
                    f"({need / 1e9:.2f} GB on the device), {len(plan.groups)} group(s) of equal box extents and longitude formulation")
    results = [None] * len(plan.tracks)
    form = getattr(args, "vorticity_form", None) or "metpy_no_crs"

    def diagnostics_of(tr):
        # the 850-hPa diagnostics on the track's own crop: the stencil's end coefficients depend on the crop's edges
        return track_diagnostics(bt.track_view(data, tr), variable_list_df, tr.limits, tr.track, use_track_zeta=bool(getattr(args, "zeta", False)),
                                 device=dev, formulation=form)
    found, ranges, phase_out = None, None, []
    if clock is not None:
        if clock[0] == "peak":
            found = [diagnostics_of(tr) for tr in plan.tracks]
        ranges = bt.phase_ranges(plan, clock, None if found is None else [[p["min_max_zeta_850"] for p in f] for f in found])
    if with_composites and {k[:2]: v for k, v in plan.groups.items()} != composite_shapes:
        raise ValueError("composite_shapes: not batch.composites_check's result for this plan")
    composites, ensembles = [None] * len(plan.tracks), []
    for (nyb, nxb, uniform), members in plan.groups.items():
        trs = [plan.tracks[k] for k in members]
        boxes = [b for tr in trs for b in tr.boxes]
        steps = torch.as_tensor(np.concatenate([tr.steps for tr in trs])).to(dev)
        tcoef = torch.as_tensor(np.concatenate([tr.tcoef for tr in trs])).to(dev)
        pb = engine.prepare_boxes(boxes, nyb_min=nyb, lon_uniform=uniform)      # (the formulation of the tracks' own crops)
        res = engine.compute(cubes[0], cubes[1], cubes[2], cubes[3], cubes[4], pb, phi_scale=phi_scale, per_step_boxes=True,
                             drop_any_time=False, steps=steps, tcoef=tcoef,
                             **({"batch_composites": [tr.n for tr in trs]} if with_composites else {}),
                             **({"batch_composite_phases": ranges[members]} if ranges is not None else {}))
        a = 0
        for n, (k, tr) in enumerate(zip(members, trs)):
            b = a + tr.n
            results[k] = LECResult(scalars=res.scalars[a:b], levels=res.levels[a:b], nanflag=res.nanflag[a:b], packed=res.packed[a:b])
            if with_composites:
                composites[k] = (res.batch_composite_mean[n].cpu().numpy(), res.batch_composite_lon[a:b].cpu().numpy())
            a = b
        if with_composites:
            ensembles.append(((nyb, nxb), members, res.batch_composite_ensemble.cpu().numpy()))
        if ranges is not None:
            phase_out.append((res.batch_phase_ensemble.cpu().numpy(), res.batch_phase_spread.cpu().numpy(), res.batch_phase_count,
                              res.batch_phase_members))
    torch.cuda.synchronize(dev)
    phases.mark("ingest_compute_gather")
    written = []
    for k, (tr, res, (results_subdirectory, figures_directory, vl_directory)) in enumerate(zip(plan.tracks, results, directories)):
        view = bt.track_view(data, tr)
        _create_level_csvs(vl_directory, time_name, vert_name, view.level)
        holder = _TrackResult(view, variable_list_df, res, results_subdirectory, vl_directory)
        if int(holder.nanflag.sum()):
            app_logger.warning(f"{tr.path}: NaN level values were interpolated/dropped per time step (_handle_nans semantics)")
        positions = diagnostics_of(tr) if found is None else found[k]
        app_logger.info(f"Track {tr.path}: {tr.n} time steps -> {results_subdirectory}")
        written.append(_write_moving_results(holder, pd.DatetimeIndex(view.time), view.time_s, tr.limits, positions, results_subdirectory,
                                             form, app_logger, args, lon_origin=ds.lon_origin_of_axis(view.lon)))
        if with_composites:     # the files of the track's own --composites run (lec_moving), from the batch's numbers
            holder.composite_mean, holder.composite_lon = composites[k]
            holder.composite_dlat, holder.composite_dlon = composite_offsets(data.lat, data.lon, tr.boxes[0])
            write_composite_csvs(holder, os.path.join(results_subdirectory, "results_composites"), time_name)
    if with_composites:
        _write_batch_composites(plan, data, ensembles, composites, directories, batch_dir, app_logger)
    if ranges is not None:
        _write_batch_phases(plan, data, ensembles, phase_out, clock, ranges, found, [df for _, df in written], batch_dir, app_logger)
    return written


def _write_batch_phases(plan, data, ensembles, phase_out, clock, ranges, found, frames, batch_dir, app_logger):
    """``phases/`` in every ensemble directory of a batch (``_write_batch_composites``' directories): per bin ``<term>_dlat_dlon_phase<bb>.csv``
    (the ensemble over the bin's members) and ``<term>_sd_dlat_dlon_phase<bb>.csv`` (their n - 1 standard deviation) in
    ``write_composite_mean_csvs``' layout and labels; ``phases.csv`` (per bin: label, members, total steps), ``phase_members.csv`` (per
    track its steps in every bin; with the peak clock also its peak's step, time and value) and ``phase_terms.csv``
    (``batch.phase_terms`` of the tracks' results)."""
    from . import batch as bt
    n_bin = int(ranges.shape[1])
    width = max(2, len(str(n_bin - 1)))
    hours = None
    if clock[0] == "peak":
        t = plan.tracks[0].time
        hours = float((t[1] - t[0]) / np.timedelta64(1, "h"))
    labels = bt.phase_labels(clock, hours)
    for ((nyb, nxb), members, _), (ens, spread, count, n_members) in zip(ensembles, phase_out):
        name = "results_composites" if len(ensembles) == 1 else f"results_composites_{nyb}x{nxb}"
        directory = os.path.join(batch_dir, name, "phases")
        dlat, dlon = composite_offsets(data.lat, data.lon, plan.tracks[members[0]].boxes[0])
        for b in range(n_bin):
            bb = f"{b:0{width}d}"
            write_composite_mean_csvs(ens[b], dlat, dlon, directory, name="{term}_dlat_dlon_phase" + bb + ".csv")
            write_composite_mean_csvs(spread[b], dlat, dlon, directory, name="{term}_sd_dlat_dlon_phase" + bb + ".csv")
        pd.DataFrame({"bin": np.arange(n_bin), "label": labels, "members": np.asarray(n_members, dtype=int),
                      "steps": np.asarray(count, dtype=int).sum(axis=0)}).to_csv(os.path.join(directory, "phases.csv"), index=False)
        table = {"trackfile": [plan.tracks[k].path for k in members], "steps": [plan.tracks[k].n for k in members]}
        if found is not None:
            peaks = [bt.peak_step([p["min_max_zeta_850"] for p in found[k]]) for k in members]
            table["s_peak"] = peaks
            table["peak_time"] = [str(pd.Timestamp(plan.tracks[k].time[s])) for k, s in zip(members, peaks)]
            table["peak_min_max_zeta_850"] = [repr(float(found[k][s]["min_max_zeta_850"])) for k, s in zip(members, peaks)]
        for b in range(n_bin):
            table[f"phase{b:0{width}d}"] = np.asarray(count, dtype=int)[:, b]
        pd.DataFrame(table).to_csv(os.path.join(directory, "phase_members.csv"), index=False)
        terms = bt.phase_terms([frames[k] for k in members], ranges[members])
        terms.insert(0, "label", labels)
        terms.to_csv(os.path.join(directory, "phase_terms.csv"))
        app_logger.info(f"--batch-composites-phase {clock[0]}:{clock[1]}: {n_bin} bin(s) over {len(members)} track(s) of {nyb} x {nxb} box points "
                        f"(lec_composite_phase_sum, lec_composite_phase_ensemble), members per bin {np.asarray(n_members).tolist()}, written to {directory}")
    return None


def _write_batch_composites(plan, data, ensembles, composites, directories, batch_dir, app_logger):
    """The ensemble means of a batch (``lec_moving_batch``): per box shape ``<term>_dlat_dlon.csv`` in ``write_composite_csvs``' layout
    -- labelled by the offsets of the first track's first box -- and ``composites.csv``, one line per track that entered the mean.  One
    shape: ``batch_dir/results_composites/``; several: ``batch_dir/results_composites_<rows>x<columns>/`` each."""
    for (nyb, nxb), members, ens in ensembles:
        name = "results_composites" if len(ensembles) == 1 else f"results_composites_{nyb}x{nxb}"
        directory = os.path.join(batch_dir, name)
        first = plan.tracks[members[0]]
        dlat, dlon = composite_offsets(data.lat, data.lon, first.boxes[0])
        write_composite_mean_csvs(ens, dlat, dlon, directory)
        pd.DataFrame({"trackfile": [plan.tracks[k].path for k in members], "results_directory": [directories[k][0] for k in members],
                      "steps": [plan.tracks[k].n for k in members], "rows": nyb, "columns": nxb,
                      "nan_points": [int(np.isnan(composites[k][0]).sum()) for k in members]}).to_csv(os.path.join(directory, "composites.csv"), index=False)
        app_logger.info(f"--batch-composites: {len(members)} track(s) of {nyb} x {nxb} box points (rows x columns) entered the ensemble mean of Ae, "
                        f"Ke, Ca, Ce, Ck, Ge (lec_composite_steps, lec_composite_ensemble), written to {directory}: "
                        + ", ".join(plan.tracks[k].path for k in members))


def lec_moving_batch_streamed(raw: ds.RawDataset, variable_list_df: pd.DataFrame, plan, directories, app_logger, args):
    """``lec_moving_batch`` without the union cubes (``-t --trackfiles --batch-chunk N``): the file is streamed ``args.batch_chunk`` union
    time steps at a time (``ingest.lec_streamed_batch``), so the device holds a chunk's buffers and 12 KB per record however long the
    series is, and the host decodes nothing.  ``raw``: the opened file (``dataset.open_raw``); coordinates and times come from the plan.
    Every track's files are written by the code ``lec_moving_batch`` writes them with, byte for byte the same."""
    from types import SimpleNamespace
    from . import ingest
    from .diagnostics import positions, track_diagnostics
    dev = _device(args)
    time_name = variable_list_df.loc["Time"]["Variable"]
    vert_name = variable_list_df.loc["Vertical Level"]["Variable"]
    form = getattr(args, "vorticity_form", None) or "metpy_no_crs"
    # the 850-hPa diagnostics from the bytes this pass stages, where the namelist's wind units leave the file's values as they are
    # (BoxData's rule for the single streamed run); otherwise from three level slices per track, decoded on the host
    plain_units = all(ds.field_scale(variable_list_df, r) == 1.0 for r in ("Eastward Wind Component", "Northward Wind Component"))
    diag = {"formulation": form} if plain_units else None
    st = {}
    with ingest.refusals():
        results = ingest.lec_streamed_batch(raw, plan, variable_list_df, chunk_steps=args.batch_chunk, device=dev,
                                            inflate=getattr(args, "inflate", None) or "auto", stats=st, diag=diag)
    phases.mark("ingest_compute_gather")
    app_logger.info(f"Batch of {len(plan.tracks)} tracks, streamed: union of {len(plan.tpos)} time steps on a {len(plan.lat)} x {len(plan.lon)} crop, "
                    f"{len(plan.groups)} group(s) of equal box extents and longitude formulation; {st['chunks']} chunk(s) of {st['chunk_steps']} "
                    f"step(s), {st['bytes_moved'] / 1e6:.1f} MB ({st['bytes_moved']} bytes) over the link, staging {st['staging']}, inflate {st['inflate']}, "
                    f"storage {st['storage']}, device buffers {st['device_buffer_bytes'] / 1e9:.2f} GB")
    app_logger.info("Streamed batch seconds: " + ", ".join(f"{k} {v:.3f}" for k, v in st["seconds"].items()))
    written = []
    for n, (tr, res, (results_subdirectory, figures_directory, vl_directory)) in enumerate(zip(plan.tracks, results, directories)):
        wlat, wlon = tr.window(plan.lat, plan.lon)
        view = SimpleNamespace(lat=wlat, lon=wlon, level=plan.px.level, time=tr.time, time_s=tr.time_s)
        _create_level_csvs(vl_directory, time_name, vert_name, view.level)
        holder = _TrackResult(view, variable_list_df, res, results_subdirectory, vl_directory)
        if int(holder.nanflag.sum()):
            app_logger.warning(f"{tr.path}: NaN level values were interpolated/dropped per time step (_handle_nans semantics)")
        use_zeta = bool(getattr(args, "zeta", False))
        if diag is not None:
            val, pos = diag["extrema"][n]
            rows = [tr.track.iloc[int(np.argmin(np.abs(tr.track.index - t)))] for t in tr.time]
            found = [positions(val[t], pos[t], wlat, wlon, tr.limits[t], rows[t], use_zeta) for t in range(tr.n)]
        else:
            i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
            px = plan.px
            own = ds.IngestPlan(np.asarray(plan.tpos[tr.ustep]), i32(px.ik), i32(px.ij[tr.js]), i32(px.io[tr.is_]), wlat, wlon, px.level, tr.time)
            found = track_diagnostics(ingest.StreamedDataset(raw, own), variable_list_df, tr.limits, tr.track, use_track_zeta=use_zeta,
                                      device=dev, formulation=form)
        app_logger.info(f"Track {tr.path}: {tr.n} time steps -> {results_subdirectory}")
        written.append(_write_moving_results(holder, pd.DatetimeIndex(view.time), view.time_s, tr.limits, found, results_subdirectory,
                                             form, app_logger, args, lon_origin=ds.lon_origin_of_axis(view.lon)))
    return written
