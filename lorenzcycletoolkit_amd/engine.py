"""LECEngine: device-resident Lorenz-Energy-Cycle computation through the C-ABI HIP library.

Holds the (time, level, lat, lon) fields as PyTorch-ROCm tensors, builds the small coefficient
tables on the host, and issues ``lec_rowstats`` + ``lec_reduce`` on the current HIP stream.
It is the replacement for ``BoxData`` + the four analysis classes of the reference
(box_data.py:58-105, energy_contents.py, conversion_terms.py, boundary_terms.py,
generation_and_dissipation_terms.py).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib, tables
from .constants import (LEVEL_TERMS, SCALAR_TERMS, SECTION_TERMS, SPECTRUM_BUDGET_TERMS, SPECTRUM_GENERATION_TERM, SPECTRUM_INTERACTION_PLACES,
                        SPECTRUM_LEVEL_TERMS, SPECTRUM_TERMS)


@dataclass
class LECResult:
    """Per-time-step outputs (device tensors) of one engine call.  ``scalars`` and ``levels`` are views of ``packed``: one record of
    16 + 21 nl doubles per time step, written by ``lec_reduce`` in place -- the unit the time-sharded gather moves (parallel.py)."""
    scalars: torch.Tensor      # [t_count, 16] fp64, columns = constants.SCALAR_TERMS
    levels: torch.Tensor       # [t_count, 21, nl] fp64, tables = constants.LEVEL_TERMS
    nanflag: torch.Tensor      # [t_count] int32: NaN level values repaired/dropped by _handle_nans
    rows: Optional[torch.Tensor] = None   # [t_count, nl, nyb_max, 32] row records (kept on request)
    packed: Optional[torch.Tensor] = None  # [t_count, 16 + 21 nl] fp64
    # compute(..., wavenumbers=N) on a ring: the zonal-wavenumber shares of the eddy terms (constants.SPECTRUM_TERMS / SPECTRUM_LEVEL_TERMS)
    spectrum: Optional[torch.Tensor] = None         # [t_count, 5, N] fp64: Ae, Ke, Ca, Ce, Ck of the wavenumbers 1 .. N
    spectrum_rest: Optional[torch.Tensor] = None    # [t_count, 5] fp64: the total minus the N shares
    spectrum_levels: Optional[torch.Tensor] = None  # [t_count, 14, N, nl] fp64
    # compute(..., wavenumbers=N, spectrum_generation=True): the same for the generation term Ge (``rowspec_q``)
    spectrum_ge: Optional[torch.Tensor] = None         # [t_count, N] fp64
    spectrum_ge_rest: Optional[torch.Tensor] = None    # [t_count] fp64: Ge minus the N shares
    spectrum_ge_levels: Optional[torch.Tensor] = None  # [t_count, N, nl] fp64
    # compute(..., wavenumbers=N, spectrum_interactions=True): the non-linear (eddy-eddy) transfers S(n), L(n) (``rowspec_nl``), W m-2,
    # positive: wavenumber n gains
    spectrum_nl: Optional[torch.Tensor] = None         # [t_count, 2, N] fp64: S, L
    spectrum_nl_total: Optional[torch.Tensor] = None   # [t_count, 2] fp64: the same for the whole eddy covariance (summed in physical space)
    spectrum_nl_rest: Optional[torch.Tensor] = None    # [t_count, 2] fp64: the total minus the N shares
    spectrum_nl_levels: Optional[torch.Tensor] = None  # [t_count, 2, N, nl] fp64
    # compute(..., wavenumbers=N, spectrum_budget=True): the boundary terms BAe(n), BKe(n) (``rowspec_b``), the finite-difference
    # tendencies dAe(n)/dt, dKe(n)/dt and the residuals RGe(n), RKe(n) of the wavenumbers 1 .. N (constants.SPECTRUM_BUDGET_*); the
    # ``rest`` of each is formed from the ``rest`` columns in the same way
    spectrum_b: Optional[torch.Tensor] = None                # [t_count, 2, N] fp64: BAe, BKe
    spectrum_b_rest: Optional[torch.Tensor] = None           # [t_count, 2] fp64: the total minus the N shares
    spectrum_tendency: Optional[torch.Tensor] = None         # [t_count, 2, N] fp64: dAe/dt, dKe/dt
    spectrum_tendency_rest: Optional[torch.Tensor] = None    # [t_count, 2] fp64
    spectrum_residual: Optional[torch.Tensor] = None         # [t_count, 2, N] fp64: RGe, RKe
    spectrum_residual_rest: Optional[torch.Tensor] = None    # [t_count, 2] fp64
    # compute(..., sections=True) on ONE fixed box: the latitude x pressure sections of the ten terms (constants.SECTION_TERMS;
    # ``lec_sections``).  Rows are the box's rows; sum_j cw_j X_f closes on ``levels``, sum_j cw_j C_f on ``scalars``
    section_mean: Optional[torch.Tensor] = None      # [10, nl, nyb] fp64: the time mean of X_f(t, k, j) (NaN at any step: NaN)
    section_lat: Optional[torch.Tensor] = None       # [t_count, 10, nyb] fp64: the column values C_f(t, j), in the units of ``scalars``
    section_steps: Optional[torch.Tensor] = None     # [t_count, 10, nl, nyb] fp64: X_f itself (on request; a series that was one chunk)
    section_spec_lat: Optional[torch.Tensor] = None  # [F, N + 1, nyb] fp64 (with wavenumbers=N): the time mean of the column value of
                                                     # X_f^n, f = Ae Ke Ca Ce Ck (Ge), n = 1 .. N, then the rest (the total minus the N)
    # compute(..., maps=True) on ONE fixed box: the longitude-resolved maps of the six eddy terms (constants.MAP_TERMS; ``lec_maps``,
    # DESIGN.md section 4.2d).  The box's zonal average of a map row closes on ``section_lat``, that of ``map_lon`` on ``scalars``
    map_mean: Optional[torch.Tensor] = None          # [6, nyb, nxb] fp64: the time mean of the column values C_f(t, j, i) (NaN at any step: NaN)
    map_lon: Optional[torch.Tensor] = None           # [t_count, 6, nxb] fp64: the Hovmoeller H_f(t, i) = sum_j cw_j C_f(t, j, i)
    map_steps: Optional[torch.Tensor] = None         # [t_count, 6, nyb, nxb] fp64: C_f itself (on request; a series that was one chunk)
    # compute(..., per_step_boxes=True, composites=True) on per-step boxes of ONE shape: the system-relative composites of the same six
    # terms on box-relative indices (``lec_composite``).  The zonal average over step t's box of
    # ``composite_lon[t]`` closes on ``scalars[t]``
    composite_mean: Optional[torch.Tensor] = None    # [6, nyb, nxb] fp64: the time mean of C_f(t, j, i), (j, i) relative to each step's box
    composite_lon: Optional[torch.Tensor] = None     # [t_count, 6, nxb] fp64: H_f(t, i) = sum_j cw_j(t) C_f(t, j, i), cw of step t's box
    composite_steps: Optional[torch.Tensor] = None   # [t_count, 6, nyb, nxb] fp64: C_f itself (on request)
    # compute(..., steps=tab, per_step_boxes=True, batch_composites=sizes): the composites of a BATCH of K tracks over one cube, track k
    # owning sizes[k] consecutive boxes of the step table (``lec_composite_steps`` / ``lec_composite_ensemble``).
    # Every track's share is, bit for bit, ``composite_*`` of the track's own run
    batch_composite_mean: Optional[torch.Tensor] = None      # [K, 6, nyb, nxb] fp64: every track's time-mean composite
    batch_composite_lon: Optional[torch.Tensor] = None       # [S, 6, nxb] fp64: H_f of every box, in table order
    batch_composite_ensemble: Optional[torch.Tensor] = None  # [6, nyb, nxb] fp64: (mean[0] + mean[1] + ...) / K, tracks ascending
    batch_composite_steps: Optional[torch.Tensor] = None     # [S, 6, nyb, nxb] fp64: C_f of every box (on request)
    # ... batch_composite_phases=ranges [K, B, 2]: B ranges [begin, end) of every track's own steps, a CELL per (track, bin); a range may be
    # empty (``lec_composite_phase_sum`` / ``lec_composite_phase_ensemble``).  A track is a MEMBER of the bins in
    # which it has a step; the ensemble and its spread run over a bin's members
    batch_phase_mean: Optional[torch.Tensor] = None          # [K, B, 6, nyb, nxb] fp64: the mean over the cell's steps; NaN for an empty cell
    batch_phase_ensemble: Optional[torch.Tensor] = None      # [B, 6, nyb, nxb] fp64: the members' means, added in track order, / members
    batch_phase_spread: Optional[torch.Tensor] = None        # [B, 6, nyb, nxb] fp64: the members' n - 1 standard deviation; NaN below 2 members
    batch_phase_count: Optional[np.ndarray] = None           # host int32 [K, B]: the steps of every cell
    batch_phase_members: Optional[np.ndarray] = None         # host int32 [B]: the tracks with at least one step in the bin
    # compute(..., per_step_boxes=True, composite_sections=True) on per-step boxes of ONE row count: the system-relative latitude x
    # pressure sections of the ten terms on box-relative rows (``lec_composite_sections``).  With cw of step t's
    # box, sum_j cw_j(t) X_f closes on ``levels[t]`` and sum_j cw_j(t) C_f on ``scalars[t]``
    composite_section_mean: Optional[torch.Tensor] = None    # [10, nl, nyb] fp64: the time mean of X_f(t, k, j) (NaN at any step: NaN)
    composite_section_lat: Optional[torch.Tensor] = None     # [t_count, 10, nyb] fp64: C_f(t, j), in the units of ``scalars``
    composite_section_steps: Optional[torch.Tensor] = None   # [t_count, 10, nl, nyb] fp64: X_f itself (on request)
    # compute(..., lon_sections=True) on ONE fixed box: the longitude x pressure sections of the six eddy terms (constants.MAP_TERMS;
    # ``lec_lonsections``), X_f(t, k, i) = sum_j cw_j Y_f(t, k, j, i) in the units of ``section_steps``.  The box's
    # zonal average closes on sum_j cw_j ``section_steps``, s_f times the vertical trapezoid on ``map_lon``
    lonsection_mean: Optional[torch.Tensor] = None   # [6, nl, nxb] fp64: the time mean of X_f(t, k, i) (NaN at any step: NaN)
    lonsection_steps: Optional[torch.Tensor] = None  # [t_count, 6, nl, nxb] fp64: X_f itself (on request; a series that was one chunk)
    # compute(..., per_step_boxes=True, composite_lon_sections=True) on per-step boxes of ONE shape: the same on the boxes' box-relative
    # columns, cw of step t's box (``lec_composite_lonsections``).  The vertical trapezoid closes on ``composite_lon``
    composite_lonsection_mean: Optional[torch.Tensor] = None    # [6, nl, nxb] fp64
    composite_lonsection_steps: Optional[torch.Tensor] = None   # [t_count, 6, nl, nxb] fp64 (on request)

    def scalars_dict(self) -> Dict[str, np.ndarray]:
        s = self.scalars.cpu().numpy()
        return {name: s[:, i].copy() for i, name in enumerate(SCALAR_TERMS)}

    def levels_dict(self) -> Dict[str, np.ndarray]:
        lv = self.levels.cpu().numpy()
        return {name: lv[:, i, :].copy() for i, name in enumerate(LEVEL_TERMS)}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


_LEC_S_TT = 6      # enum lec_stat: the eight eddy covariances [T'T'] .. [w'v'] are slots 6 .. 13 of a row record
_LEC_S_QT = 15     # ... and [Q'T'] is slot 15
_LEC_S_BUDGET = (16, 17, 20, 21)   # ... and [vT'T'] [wT'T'] [Ev] [Ew], the slots lec_rowspec_b_ring splits

_KERNELS = {"auto": _lib.KERNEL_AUTO, "two_sweep": _lib.KERNEL_TWO_SWEEP, "row_sweep": _lib.KERNEL_ROW_SWEEP,
            "row_block": _lib.KERNEL_ROW_BLOCK, "box_tile": _lib.KERNEL_BOX_TILE, "box_plane": _lib.KERNEL_BOX_PLANE}
_ORDERS = {"auto": _lib.ORDER_AUTO, "memory": _lib.ORDER_MEMORY, "xcd_lat": _lib.ORDER_XCD_LAT, "xcd_tiled": _lib.ORDER_XCD_TILED}


def make_tuning(tuning: Optional[dict]) -> "_lib.Tuning":
    """``lec_tuning`` from a dict with any of: kernel ("auto" | "two_sweep" | "row_sweep" | "row_block" | "box_tile" | "box_plane"),
    block_shape (e.g. 212), order ("auto" | "memory" | "xcd_lat" | "xcd_tiled"), tile_t, tile_j, f32_vec.
    None / {} = the library's defaults (what is measured and shipped); the rest is for cross-checks and A/B runs."""
    t = _lib.Tuning()
    if not tuning:
        return t
    unknown = set(tuning) - {"kernel", "block_shape", "order", "tile_t", "tile_j", "f32_vec"}
    if unknown:
        raise ValueError(f"unknown tuning keys {sorted(unknown)}")
    k, o = tuning.get("kernel", "auto"), tuning.get("order", "auto")
    if k not in _KERNELS or o not in _ORDERS:
        raise ValueError(f"tuning: kernel must be one of {sorted(_KERNELS)}, order one of {sorted(_ORDERS)}")
    t.kernel, t.order = _KERNELS[k], _ORDERS[o]
    t.block_shape = int(tuning.get("block_shape", 0))
    t.tile_t, t.tile_j = int(tuning.get("tile_t", 0)), int(tuning.get("tile_j", 0))
    t.f32_vec = int(tuning.get("f32_vec", 0))
    return t


def pack_host(a: np.ndarray, boxes, src, nyb: int, nxb: int, dtype=None) -> np.ndarray:
    """The box-packed form of the host array ``a`` [steps, level, lat, lon]: step i of the result holds box i (iw, ie, js, jn) of
    ``a[src[i]]`` at the origin of an ``nyb`` x ``nxb`` slab, zeros beside it (``dtype``: default ``a``'s) -- the reference's per-step
    slice (box_data.py:297-310) done on the host before the upload (``LECEngine.pack_boxes`` gathers on the device)."""
    p = np.zeros((len(boxes), a.shape[1], nyb, nxb), dtype=a.dtype if dtype is None else dtype)
    for i, ((iw, ie, js, jn), ts) in enumerate(zip(boxes, src)):
        p[i, :, : jn - js + 1, : ie - iw + 1] = a[ts, :, js: jn + 1, iw: ie + 1]
    return p


class PreparedBoxes:
    """Boxes whose host tables are built and uploaded (``LECEngine.prepare_boxes``): a series of thousands of per-time-step boxes
    is normalised, keyed and looked up once instead of at every call."""

    def __init__(self, boxes, bt, dev):
        self.boxes, self.bt, self.dev = boxes, bt, dev

    def __len__(self):
        return len(self.boxes)

    def part(self, a: int, b: int) -> "PreparedBoxes":
        """Boxes [a, b) of a series of per-time-step boxes (a chunk of the series): views of the uploaded tables, no host work and no
        copy -- every table is indexed by box along its first axis."""
        import dataclasses
        if not (0 <= a < b <= len(self.boxes)):
            raise ValueError("part: need 0 <= a < b <= number of boxes")
        bt = dataclasses.replace(self.bt, box=self.bt.box[a:b], boxtab=self.bt.boxtab[a:b], wlon=self.bt.wlon[a:b], glon=self.bt.glon[a:b],
                                 lattab=self.bt.lattab[a:b], boxtab2=self.bt.boxtab2[a:b], lattab2=self.bt.lattab2[a:b])
        return PreparedBoxes(self.boxes[a:b], bt, {k: v[a:b] for k, v in self.dev.items()})


class LECEngine:
    """One engine per (grid, device).

    Parameters
    ----------
    lat_deg, lon_deg : 1-D arrays, degrees, ascending (lat S->N, lon W->E in (-180, 180])
    level_pa         : 1-D array, Pa, ascending
    device           : torch device of the field tensors (``cuda:N`` on ROCm)
    """

    MAX_STEPS_PER_LAUNCH = 32768       # time steps per lec_rowstats launch (longer calls are cut into parts by `rowstats`)

    def __init__(self, lat_deg, lon_deg, level_pa, device="cuda"):
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.LecLibraryError("LECEngine needs a GPU device: the HIP path is the only path")
        self.lat = np.asarray(lat_deg, dtype=np.float64)
        self.lon = np.asarray(lon_deg, dtype=np.float64)
        self.level = np.asarray(level_pa, dtype=np.float64)
        if np.any(np.diff(self.lat) <= 0) or np.any(np.diff(self.lon) <= 0):
            raise ValueError("lat and lon must be strictly ascending (preprocessing.py:358-362 sorts them)")
        levtab, levtab2 = tables.level_tables(self.level)
        self._levtab = self._up(levtab)
        self._levtab2 = self._up(levtab2)
        self._box_cache = {}
        self._pack_maps = {}   # pack_boxes' index maps of the last grid / slab shape
        self._work = {}        # stage-2 workspaces by shape: am, levraw, dropmask (true scratch: never handed out)
        self._tcoef = None     # (time axis, its d/dt coefficients on the device) of the last call
        self._ptab = None      # the d/dp coefficients of lec_rowspec_nl_ring for the engine's levels
        self._twid = None      # the twiddle table of lec_rowspec_ring for the engine's nx longitudes

    # -- helpers ---------------------------------------------------------------------------
    def _up(self, a: np.ndarray, dtype=torch.float64) -> torch.Tensor:
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(self.device)

    def box_from_limits(self, west, east, south, north):
        """Nearest-grid-point inclusive box, as BoxData._set_domain_limits (box_data.py:115-131)."""
        return tables.box_indices(self.lat, self.lon, west, east, south, north)

    def prepare_boxes(self, boxes, nyb_min: int = 0, packed: bool = False, lon_uniform: Optional[bool] = None, ring: bool = False) -> PreparedBoxes:
        """Index quadruples (iw, ie, js, jn) -> PreparedBoxes for ``rowstats`` / ``reduce`` / ``compute``.  ``nyb_min``: the row
        count of the record buffer the boxes will be used with (chunks of a series share the tallest box's).  ``packed``: the boxes
        of a BOX-PACKED series (``pack_boxes``; include/lec_hip.h): stage 1 then addresses every step's box at the origin of its
        slab, while every table is built from the true grid boxes as always.  ``lon_uniform``: see ``tables.build_box_tables`` (a track
        of a batch keeps its own crop's formulation).  ``ring``: ONE fixed box over the engine's whole longitude axis, which is a full
        ring (``tables.build_box_tables(ring=True)`` refuses anything else): stage 1 of these boxes is ``lec_rowstats_ring`` -- zonal
        means over the closed circle, Q's d/dlon centred across the seam, no east-west boundary flux."""
        boxes = [tuple(int(x) for x in b) for b in boxes]
        if ring and packed:
            raise ValueError("a ring is one fixed box: a box-packed series has no ring form")
        bt, dev = self._box_tables(boxes, nyb_min, lon_uniform, ring)
        if packed:
            dev = dict(dev, box_data=self._up(np.array([(0, b[1] - b[0], 0, b[3] - b[2]) for b in boxes], dtype=np.int32), torch.int32))
        return PreparedBoxes(boxes, bt, dev)

    @staticmethod
    def _pack_geometry(cube: torch.Tensor, boxes, ny: Optional[int], nx: Optional[int]):
        """(boxes as int64 [nt, 4], box rows, box columns, slab rows, slab columns) of a ``pack_boxes`` call: one box per step of the
        cube, each inside its grid; the slab defaults to the tallest / widest box."""
        b = np.array([tuple(int(x) for x in q) for q in (boxes.boxes if isinstance(boxes, PreparedBoxes) else boxes)], dtype=np.int64)
        nt, _, ny_in, nx_in = (int(x) for x in cube.shape)
        if len(b) != nt:
            raise ValueError("pack_boxes: one box per time step of the cube")
        bad = np.flatnonzero((b[:, 0] < 0) | (b[:, 2] < 0) | (b[:, 1] >= nx_in) | (b[:, 3] >= ny_in))
        if bad.size:
            raise ValueError(f"pack_boxes: box {int(bad[0])} (iw, ie, js, jn) = {tuple(b[bad[0]].tolist())} lies outside the {ny_in} x {nx_in} grid")
        nxb, nyb = b[:, 1] - b[:, 0] + 1, b[:, 3] - b[:, 2] + 1
        return b, nyb, nxb, int(ny or nyb.max()), int(nx or nxb.max())

    def pack_boxes(self, cube: torch.Tensor, boxes, shift: int = 0, ny: Optional[int] = None, nx: Optional[int] = None) -> torch.Tensor:
        """[nt, nl, ny_grid, nx_grid] -> the box-packed layout [len(boxes), nl, ny, nx] (default: the tallest / widest box): step t
        holds box t of ``cube[t + shift]`` (clamped to the cube: the step itself where a time neighbour does not exist) at its
        origin.  ONE launch of ``lec_ingest`` per 8192 steps -- the gather the streamed moving framework packs its series with
        (``ingest.lec_streamed``: there the source is the file's raw bytes, here a cube in HBM; ``lec_ingest_args.step_d`` = per step
        {source step, where the box starts}) -- for tests, ``bench.py --moving`` and cubes a caller already holds.  Every box must lie
        inside the grid (ValueError naming the first that does not).  What a slab holds beside a box lower / narrower than the slab is
        whatever the lengthened index maps point at (the grid's last row / column): stage 1 never reads it."""
        b, nyb, nxb, ny, nx = self._pack_geometry(cube, boxes, ny, nx)
        nt, nl, ny_in, nx_in = (int(x) for x in cube.shape)
        if cube.dtype not in (torch.float64, torch.float32) or not cube.is_contiguous() or cube.device.type != "cuda":
            raise ValueError("pack_boxes: a contiguous float64 / float32 cube on the GPU")
        if ny < nyb.max() or nx < nxb.max() or ny > ny_in or nx > nx_in:
            raise ValueError("pack_boxes: slabs must hold the tallest / widest box and fit the grid")
        dev = cube.device
        key = (nl, ny_in, nx_in, ny, nx, str(dev))
        maps = self._pack_maps.get(key)
        if maps is None:            # identity maps, lengthened by a slab (their last entry repeated): a box at the grid's edge is gathered with the slab's extents
            up = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32).to(dev)
            maps = (up(np.arange(nl)), up(np.minimum(np.arange(ny_in + ny), ny_in - 1)), up(np.minimum(np.arange(nx_in + nx), nx_in - 1)))
            self._pack_maps = {key: maps}
        step = torch.as_tensor(np.column_stack([np.clip(np.arange(nt) + shift, 0, nt - 1), b[:, 2], b[:, 0]]).astype(np.int32)).to(dev)
        out = torch.empty((nt, nl, ny, nx), dtype=cube.dtype, device=dev)
        code = _lib.LEC_F64 if cube.dtype == torch.float64 else _lib.LEC_F32
        for a0 in range(0, nt, 8192):            # (a call addresses its output rows with a 31-bit grid index)
            a1 = min(nt, a0 + 8192)
            ga = _lib.IngestArgs(
                src_d=_ptr(cube), src_dtype=code, swap_bytes=0, nt=a1 - a0, nl_in=nl, ny_in=ny_in, nx_in=nx_in, nl=nl, ny=ny, nx=nx,
                kmap_d=_ptr(maps[0]), jmap_d=_ptr(maps[1]), imap_d=_ptr(maps[2]), has_packing=0, has_fill=0, scale_factor=1.0, add_offset=0.0,
                fill_value=0.0, unit_scale=1.0, out_dtype=code, decode_dtype=code, out_d=_ptr(out[a0:a1]),
                stream=C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), step_d=_ptr(step[a0:a1]), step_base=0, nt_src=nt,
                jmap_len=int(maps[1].numel()), imap_len=int(maps[2].numel()))
            with torch.cuda.device(dev):
                _lib.check(self.lib.lec_ingest(C.byref(ga)), "lec_ingest")
        return out

    def pack_boxes_by_indexing(self, cube: torch.Tensor, boxes, shift: int = 0, ny: Optional[int] = None, nx: Optional[int] = None) -> torch.Tensor:
        """``pack_boxes`` as one torch advanced-indexing gather, zeros beside the boxes: the independent form the tests hold the
        ``lec_ingest`` gather to (inside the boxes: the same values)."""
        b, nyb, nxb, ny, nx = self._pack_geometry(cube, boxes, ny, nx)
        nt = cube.shape[0]
        dev = cube.device
        tt = torch.as_tensor(np.clip(np.arange(nt) + shift, 0, nt - 1), device=dev)[:, None, None, None]
        kk = torch.arange(cube.shape[1], device=dev)[None, :, None, None]
        jj = torch.arange(ny, device=dev)[None, None, :, None]
        ii = torch.arange(nx, device=dev)[None, None, None, :]
        up = lambda a: torch.as_tensor(a, device=dev)[:, None, None, None]
        inside = (jj < up(nyb)) & (ii < up(nxb))
        rows = torch.minimum(up(b[:, 2]) + jj, up(b[:, 3]))
        cols = torch.minimum(up(b[:, 0]) + ii, up(b[:, 1]))
        return torch.where(inside, cube[tt, kk, rows, cols], torch.zeros((), dtype=cube.dtype, device=dev)).contiguous()

    def time_stencil(self, tm: torch.Tensor, t: torch.Tensor, tp: torch.Tensor, tcoef: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dT/dt of a box-packed series as an fp64 cube (``lec_dtdt``): tcoef[s] . (tm[s], t[s], tp[s]) with the bits of stage 1's own
        per-point evaluation.  ``tcoef``: fp64 [steps, 3] on the device, the rows of the steps the cubes hold."""
        if tm.shape != t.shape or tp.shape != t.shape or tm.dtype != t.dtype or tp.dtype != t.dtype or not (tm.is_contiguous() and t.is_contiguous() and tp.is_contiguous()):
            raise ValueError("time_stencil: three contiguous cubes of one shape and dtype")
        n = int(t.shape[0])
        if tcoef.shape != (n, 3) or tcoef.dtype != torch.float64 or not tcoef.is_contiguous() or tcoef.device != t.device:
            raise ValueError("time_stencil: tcoef must be a contiguous fp64 [steps, 3] tensor on the cubes' device")
        if out is None:
            out = torch.empty(t.shape, dtype=torch.float64, device=t.device)
        elif out.shape != t.shape or out.dtype != torch.float64 or not out.is_contiguous() or out.device != t.device:
            raise ValueError("time_stencil: out must be a contiguous fp64 tensor of the cubes' shape")
        for a in range(0, n, 65535):
            b = min(n, a + 65535)
            args = _lib.DtdtArgs(tm_d=_ptr(tm[a:b]), t_d=_ptr(t[a:b]), tp_d=_ptr(tp[a:b]), dtype=_lib.LEC_F64 if t.dtype == torch.float64 else _lib.LEC_F32,
                                 n_steps=b - a, step_elems=int(t[0].numel()), tcoef_d=_ptr(tcoef[a:b]), out_d=_ptr(out[a:b]),
                                 stream=C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream))
            with torch.cuda.device(t.device):
                _lib.check(self.lib.lec_dtdt(C.byref(args)), "lec_dtdt")
        return out

    def packed_dtdt(self, tm: torch.Tensor, t: torch.Tensor, tp: torch.Tensor, tcoef: torch.Tensor, out: Optional[torch.Tensor] = None) -> dict:
        """The dT/dt arguments of ``rowstats`` for a box-packed series whose T is ``t`` and whose time neighbours on every step's box are
        ``tm`` / ``tp`` (``tcoef``: the rows of the cubes' steps): for fp64 storage {"dTdt"}, an fp64 cube made by ``time_stencil``
        (one operand fewer per point; written into ``out`` when given); for fp32 storage {"tm", "tp", "tcoef"} (the same bytes as a
        cube would be, and no rounding of dT/dt to the storage dtype).  The one place that picks the form."""
        if t.dtype == torch.float64:
            return {"dTdt": self.time_stencil(tm, t, tp, tcoef, out=out)}
        return {"tm": tm, "tp": tp, "tcoef": tcoef}

    def pack_series(self, tair, u, v, omega, geopt, boxes, tcoef: torch.Tensor, ny: Optional[int] = None, nx: Optional[int] = None,
                    timing: Optional[dict] = None) -> dict:
        """The box-packed form of a moving series held as whole cubes (tests, ``bench.py --moving``): the five fields packed per step
        (``pack_boxes``) and dT/dt in the form of ``packed_dtdt`` -- "dTdt", or "tm" / "tp" (the caller adds ``tcoef``).  ``tcoef``:
        rows of the cubes' steps.  ``timing``: a dict that receives HIP events recorded on the current stream -- "pack" = (start, end)
        around the gathers (the per-step slice, box_data.py:297-310), "dtdt" = (start, end) around ``lec_dtdt`` (fp64 storage only):
        what the PRODUCER of a packed series spends, which ``bench.py --moving`` reports beside the consumer's rate."""
        def ev():
            if timing is None:
                return None
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e

        with torch.cuda.device(tair.device):
            e0 = ev()
            pk = {k: self.pack_boxes(c, boxes, ny=ny, nx=nx) for k, c in (("tair", tair), ("u", u), ("v", v), ("omega", omega), ("geopt", geopt)) if c is not None}
            tm, tp = self.pack_boxes(tair, boxes, shift=-1, ny=ny, nx=nx), self.pack_boxes(tair, boxes, shift=+1, ny=ny, nx=nx)
            e1 = ev()
            dt = self.packed_dtdt(tm, pk["tair"], tp, tcoef)
            e2 = ev()
        dt.pop("tcoef", None)
        pk.update(dt)
        if timing is not None:
            timing["pack"] = (e0, e1)
            if "dTdt" in pk:
                timing["dtdt"] = (e1, e2)
        pk.setdefault("geopt", None)
        return pk

    def _resolve_boxes(self, boxes, nyb_min: int = 0):
        if isinstance(boxes, PreparedBoxes):
            if boxes.bt.nyb_max < nyb_min:
                raise ValueError("PreparedBoxes were built for a lower record buffer: pass nyb_min to prepare_boxes")
            return boxes.boxes, boxes.bt, boxes.dev
        boxes = [tuple(int(x) for x in b) for b in (boxes if isinstance(boxes[0], (tuple, list, np.ndarray)) else [boxes])]
        bt, dev = self._box_tables(boxes, nyb_min)
        return boxes, bt, dev

    def _box_tables(self, boxes, nyb_min: int = 0, lon_uniform: Optional[bool] = None, ring: bool = False):
        key = (int(nyb_min), lon_uniform, bool(ring)) + tuple(int(v) for b in boxes for v in b)
        hit = self._box_cache.get(key)
        if hit is not None:
            return hit
        bt = tables.build_box_tables(self.lat, self.lon, boxes, nyb_min=nyb_min, lon_uniform=lon_uniform, ring=ring)
        dev = {
            "box": self._up(bt.box, torch.int32), "boxtab": self._up(bt.boxtab), "wlon": self._up(bt.wlon),
            "glon": self._up(bt.glon), "lattab": self._up(bt.lattab), "boxtab2": self._up(bt.boxtab2),
            "lattab2": self._up(bt.lattab2),
        }
        if len(self._box_cache) > 8:
            self._box_cache.clear()
        self._box_cache[key] = (bt, dev)
        return bt, dev

    def time_coefs_device(self, time_s) -> torch.Tensor:
        """np.gradient's coefficients over a whole series' time axis, on the device ([n, 3]).  Rows [h0, h1) serve any cube that holds
        the steps [h0, h1) of the series and processes only steps whose neighbours it holds (own steps + one-step halo): there the
        coefficients of the sub-axis equal the series' (they differ only at the halo steps, which are not processed)."""
        return self._up(tables.time_coefs(np.asarray(time_s, dtype=np.float64)))

    # -- the hot path ----------------------------------------------------------------------
    def compute(self, tair: torch.Tensor, u: torch.Tensor, v: torch.Tensor, omega: torch.Tensor,
                geopt: Optional[torch.Tensor], boxes: Sequence[Sequence[int]], *,
                time_s=None, dTdt: Optional[torch.Tensor] = None, t_begin: int = 0,
                t_count: Optional[int] = None, with_q: bool = True, phi_scale: float = 1.0,
                keep_rows: bool = False, timing: Optional[list] = None,
                drop_any_time: Optional[bool] = None,
                merge_dropmask: Optional[Callable[[torch.Tensor], None]] = None,
                tuning: Optional[dict] = None, per_step_boxes: Optional[bool] = None,
                out: Optional[torch.Tensor] = None, tm: Optional[torch.Tensor] = None, tp: Optional[torch.Tensor] = None,
                tcoef: Optional[torch.Tensor] = None, steps: Optional[torch.Tensor] = None,
                wavenumbers: Optional[int] = None, spectrum_generation: bool = False, spectrum_fused: bool = False,
                spectrum_interactions: bool = False, spectrum_budget: bool = False,
                sections: bool = False, section_steps: bool = False, maps: bool = False, map_steps: bool = False,
                composites: bool = False, composite_steps: bool = False,
                composite_sections: bool = False, composite_section_steps: bool = False,
                batch_composites: Optional[Sequence[int]] = None, batch_composite_steps: bool = False,
                batch_composite_phases=None,
                lon_sections: bool = False, lon_section_steps: bool = False,
                composite_lon_sections: bool = False, composite_lon_section_steps: bool = False) -> LECResult:
        """All LEC terms for time steps [t_begin, t_begin + t_count) of the cubes: ``rowstats`` then ``reduce``.
        (``tm`` / ``tp`` / ``tcoef``: a box-packed series; ``steps`` / ``tcoef``: the boxes of several tracks over one cube -- see
        ``rowstats``.)

        ``boxes``: one (iw, ie, js, jn) quadruple (fixed framework) or one per processed time step
        (moving framework).  ``per_step_boxes``: True = the moving framework's semantics (default when more than one
        box is given); say so explicitly for a ONE-step shard or chunk of a moving series, which would otherwise read
        as a fixed box (same numbers to rounding, but another kernel family: not the same bits).  ``time_s`` (seconds, length nt) gives dT/dt by np.gradient over the
        cube's time axis unless a ``dTdt`` cube is supplied (moving framework).
        ``drop_any_time``: _handle_nans' dropna semantics -- True drops a level that stays NaN at any processed
        time step from every time step's integrals (what the fixed framework's [time, level] arrays do); default:
        True for one fixed box, False for per-time-step boxes (the moving framework builds one BoxData per step).
        ``merge_dropmask``: see ``reduce`` (time-sharded runs).
        ``timing``: a list that receives one (start, end) pair of HIP events recorded on the launch
        stream around every stage-1 launch (bench.py's roofline figure).
        ``wavenumbers`` = N (boxes from ``prepare_boxes(..., ring=True)`` only): the result also carries ``spectrum``,
        ``spectrum_rest`` and ``spectrum_levels``, the shares of the zonal wavenumbers 1 .. N in Ae, Ke, Ca, Ce and Ck (``rowspec``
        and stage 2 on row records that carry one wavenumber's covariances).  Everything else of the result is, bit for bit, what
        the call without it returns.
        ``spectrum_generation`` (with ``wavenumbers``, ``with_q`` and dT/dt from ``time_s`` / ``tcoef``, not a ``dTdt`` cube): also
        ``spectrum_ge``, ``spectrum_ge_rest`` and ``spectrum_ge_levels``, the same shares of Ge (``rowspec_q``: Q is evaluated at every
        point of a row once more and projected beside T).  It changes no bit of anything else.
        ``spectrum_fused`` (with ``wavenumbers``): stage 2 of the spectra by ``spectrum_level_stage`` (``lec_level_spec_ring``), which
        takes a wavenumber's shares straight from the spectral records instead of from N assembled copies of the row records.  The
        same bits; the default stays the assembled form, the yardstick the fused kernels are tested against.
        ``spectrum_interactions`` (with ``wavenumbers``): also ``spectrum_nl``, ``spectrum_nl_total``, ``spectrum_nl_rest`` and
        ``spectrum_nl_levels``, the non-linear eddy-eddy transfers S(n) (into Ae) and L(n) (into Ke) of the wavenumbers 1 .. N
        (``rowspec_nl`` and ``spectrum_level_stage`` on its records).  It changes no bit of anything else.
        ``spectrum_budget`` (with ``wavenumbers`` and ``time_s``, at least two processed steps): also ``spectrum_b`` (BAe(n), BKe(n):
        ``rowspec_b``, whose four shares enter the same stage-2 batch in slots 16, 17, 20, 21), ``spectrum_tendency`` (dAe(n)/dt,
        dKe(n)/dt by ``tables.budgets_and_residuals``: np.gradient with dt = time_s[1] - time_s[0]) and ``spectrum_residual`` (RGe(n),
        RKe(n)), each with its ``_rest``.  It changes no bit of anything else; both ``spectrum_fused`` forms give the same bits.
        ``sections`` (ONE fixed box, one process): also ``section_mean`` and ``section_lat`` -- and ``section_steps`` when asked for, and
        ``section_spec_lat`` with ``wavenumbers`` --, the latitude x pressure sections of the ten terms (``section_stage``).  It
        changes no bit of anything else; without it nothing new runs or allocates.
        ``maps`` (ONE fixed box with evenly spaced longitudes, one process, ``with_q`` and dT/dt from ``time_s`` / ``tcoef``): also
        ``map_mean`` and ``map_lon`` -- and ``map_steps`` when asked for --, the longitude-resolved maps of the six eddy terms
        (``map_stage``: the cubes are read once more).  It changes no bit of anything else; without it nothing new runs or allocates.
        ``composites`` (per-step boxes that all have ONE shape, evenly spaced longitudes, one process, ``with_q``; cubes, or a box-packed
        series with its ``dTdt`` cube or ``tm`` / ``tp``): also ``composite_mean`` and ``composite_lon`` -- and ``composite_steps`` when
        asked for --, the system-relative composites of the six eddy terms on box-relative indices (``composite_stage``: the cubes are
        read once more).  It changes no bit of anything else; without it nothing new runs or allocates.
        ``composite_sections`` (per-step boxes that all have ONE row count -- widths may differ --, one process; any layout stage 1
        takes, a ``steps`` table of one box per processed step included): also ``composite_section_mean`` and ``composite_section_lat``
        -- and ``composite_section_steps`` when asked for --, the system-relative latitude x pressure sections of the ten terms on
        box-relative rows (``composite_section_stage``: only the row records are read).  It changes no bit of anything else; without it
        nothing new runs or allocates.
        ``batch_composites`` = sizes (with ``steps``: the boxes of K tracks over one cube, track k owning ``sizes[k]`` consecutive rows
        of the table; every box of ONE shape, evenly spaced longitudes, one process, ``with_q``): also ``batch_composite_mean``,
        ``batch_composite_lon`` and ``batch_composite_ensemble`` -- and ``batch_composite_steps`` when asked for --, every track's
        composites and their ensemble mean (``batch_composite_stage``: the cubes are read once more).  A track's share has the bits of
        ``composites=True`` on the track's own cube.  It changes no bit of anything else; without it nothing new runs or allocates.
        ``batch_composite_phases`` = ranges (with ``batch_composites``: an int array [K, B, 2], B ranges [begin, end) of every track's
        own step indices, 0 <= begin <= end <= sizes[k]; a range may be empty and ranges may overlap): also ``batch_phase_mean``,
        ``batch_phase_ensemble``, ``batch_phase_spread``, ``batch_phase_count`` and ``batch_phase_members``, every (track, bin) cell's
        mean composite and per bin the ensemble and spread of the tracks that have a step in it (``lec_composite_phase_sum`` after
        every ``lec_composite_steps``, then ``lec_composite_phase_ensemble``).  It changes no bit of anything else.
        ``lon_sections`` (what ``maps`` needs: ONE fixed box with evenly spaced longitudes, one process, ``with_q`` and dT/dt from
        ``time_s`` / ``tcoef``): also ``lonsection_mean`` -- and ``lonsection_steps`` when asked for --, the longitude x pressure sections
        of the six eddy terms (``lonsection_stage``: the cubes are read once more; beside ``maps`` each call forms its own row factors).
        ``composite_lon_sections`` (what ``composites`` needs): also ``composite_lonsection_mean`` -- and ``composite_lonsection_steps``
        when asked for --, the same on the box-relative columns of per-step boxes of ONE shape (``composite_lonsection_stage``).  Neither
        changes a bit of anything else; without them nothing new runs or allocates.
        """
        if batch_composite_phases is not None:      # in words, before the library or a device is touched
            if batch_composites is None:
                raise ValueError("batch_composite_phases: the phases are ranges of the steps of batch_composites=sizes: give the sizes")
            batch_composite_phases = self._check_batch_phases(batch_composites, batch_composite_phases)
        if lon_section_steps and not lon_sections:
            raise ValueError("lon_section_steps: the per-step sections are part of lon_sections=True")
        if lon_sections:
            self._check_lonsections(boxes, per_step_boxes, steps, tm, tp)
            if merge_dropmask is not None or out is not None:
                raise ValueError("longitude-pressure sections run in one process on one GPU: a sharded run (merge_dropmask, out) has none")
            if dTdt is not None:
                raise ValueError("longitude-pressure sections: a dTdt cube is not supported (lec_lonsections forms dT/dt from the cube's "
                                 "time axis: give time_s or tcoef)")
            if not with_q:
                raise ValueError("longitude-pressure sections need with_q: the section of Ge is Q'T' at every point, and its zonal mean "
                                 "[Q] comes from the row records")
        if composite_lon_section_steps and not composite_lon_sections:
            raise ValueError("composite_lon_section_steps: the per-step sections are part of composite_lon_sections=True")
        if composite_lon_sections:
            lon = getattr(self, "lon", None)
            self._check_composites(boxes, per_step_boxes, steps, boxes.bt.lon_uniform if isinstance(boxes, PreparedBoxes)
                                   else (None if lon is None else tables.is_uniform(lon)), what=self._COMPOSITE_LONSECTION_WORDS)
            if merge_dropmask is not None or out is not None:
                raise ValueError("composite longitude-pressure sections run in one process on one GPU: a sharded run (merge_dropmask, out) has none")
            if not with_q:
                raise ValueError("composite longitude-pressure sections need with_q: the section of Ge is Q'T' at every point, and its "
                                 "zonal mean [Q] comes from the row records")
        if batch_composite_steps and batch_composites is None:
            raise ValueError("batch_composite_steps: the per-box columns are part of batch_composites=sizes")
        if batch_composites is not None:
            if steps is None:
                raise ValueError("batch composites need a step table (steps=, the batch of lec_rowstats_steps): ONE track has composites=True")
            lon = getattr(self, "lon", None)
            nyb, _ = self._check_batch_composites(boxes, int(steps.shape[0]), batch_composites, boxes.bt.lon_uniform
                                                  if isinstance(boxes, PreparedBoxes) else (None if lon is None else tables.is_uniform(lon)))
            if isinstance(boxes, PreparedBoxes) and boxes.bt.nyb_max != nyb:
                raise ValueError("batch composites: the boxes' records must have the boxes' own row count (prepare_boxes without nyb_min above it)")
            # the table's host copy, taken before anything of this call is launched (later it would wait for stage 1 + stage 2)
            steps_host = steps.cpu().numpy() if steps.device.type != "cpu" else steps.numpy()
            if merge_dropmask is not None or out is not None:
                raise ValueError("batch composites run in one process on one GPU: a sharded run (merge_dropmask, out) has none")
            if not with_q:
                raise ValueError("batch composites need with_q: the composite of Ge is Q'T' at every point, and its zonal mean [Q] comes from the row records")
        if composite_section_steps and not composite_sections:
            raise ValueError("composite_section_steps: the per-step sections are part of composite_sections=True")
        if composite_sections:
            self._check_composite_sections(boxes, True if steps is not None else per_step_boxes)
            if merge_dropmask is not None or out is not None:
                raise ValueError("composite sections run in one process on one GPU: a sharded run (merge_dropmask, out) has none")
        if composite_steps and not composites:
            raise ValueError("composite_steps: the per-step columns are part of composites=True")
        if composites:
            lon = getattr(self, "lon", None)
            self._check_composites(boxes, per_step_boxes, steps, boxes.bt.lon_uniform if isinstance(boxes, PreparedBoxes)
                                   else (None if lon is None else tables.is_uniform(lon)))
            if merge_dropmask is not None or out is not None:
                raise ValueError("composites run in one process on one GPU: a sharded run (merge_dropmask, out) has none")
            if not with_q:
                raise ValueError("composites need with_q: the composite of Ge is Q'T' at every point, and its zonal mean [Q] comes from the row records")
        if map_steps and not maps:
            raise ValueError("map_steps: the per-step maps are part of maps=True")
        if maps:
            self._check_maps(boxes, per_step_boxes, steps, tm, tp)
            if merge_dropmask is not None or out is not None:
                raise ValueError("maps run in one process on one GPU: a sharded run (merge_dropmask, out) has none")
            if dTdt is not None:
                raise ValueError("maps: a dTdt cube is not supported (lec_maps forms dT/dt from the cube's time axis: give time_s or tcoef)")
            if not with_q:
                raise ValueError("maps need with_q: the map of Ge is Q'T' at every point, and its zonal mean [Q] comes from the row records")
        if section_steps and not sections:
            raise ValueError("section_steps: the per-step sections are part of sections=True")
        if sections:
            self._check_sections(boxes, per_step_boxes, steps, tm, tp)
            if merge_dropmask is not None or out is not None:
                raise ValueError("sections run in one process on one GPU: a sharded run (merge_dropmask, out) has none")
        if spectrum_budget:
            if wavenumbers is None:
                raise ValueError("spectrum_budget: BAe(n), BKe(n) and the residuals are part of the zonal-wavenumber spectra: give wavenumbers=N")
            if time_s is None:
                raise ValueError("spectrum_budget needs time_s (seconds): the tendencies are np.gradient with dt = time_s[1] - time_s[0]")
            n_steps = (int(tair.shape[0]) - t_begin) if t_count is None else int(t_count)
            if n_steps < 2 or np.asarray(time_s).size < 2:
                raise ValueError("spectrum_budget: the tendencies are finite differences in time: at least 2 time steps")
        if spectrum_interactions and wavenumbers is None:
            raise ValueError("spectrum_interactions: S(n) and L(n) are part of the zonal-wavenumber spectra: give wavenumbers=N")
        if spectrum_fused and wavenumbers is None:
            raise ValueError("spectrum_fused: a form of the zonal-wavenumber spectra: give wavenumbers=N")
        if spectrum_generation:
            if wavenumbers is None:
                raise ValueError("spectrum_generation: Ge(n) is part of the zonal-wavenumber spectra: give wavenumbers=N")
            if not with_q:
                raise ValueError("spectrum_generation needs with_q: Ge(n) is the spectrum of [Q'T']")
            if dTdt is not None:
                raise ValueError("spectrum_generation: a dTdt cube is not supported (lec_rowspec_q_ring forms dT/dt from the cube's time axis)")
        if wavenumbers is not None:
            self._check_wavenumbers(wavenumbers, boxes, int(tair.shape[-1]) if tair.dim() == 4 else 0)
            if merge_dropmask is not None or out is not None or steps is not None or tm is not None or tp is not None:
                raise ValueError("wavenumbers: one ring on whole cubes in one process (no merge_dropmask, out, steps, tm / tp)")
        rows = self.rowstats(tair, u, v, omega, geopt, boxes, time_s=time_s, dTdt=dTdt, t_begin=t_begin, t_count=t_count,
                             with_q=with_q, timing=timing, tuning=tuning, per_step_boxes=per_step_boxes, tm=tm, tp=tp, tcoef=tcoef,
                             steps=steps)
        if steps is not None:
            per_step_boxes = True
        if drop_any_time is None and per_step_boxes:
            drop_any_time = False
        res = self.reduce(rows, boxes, phi_scale=phi_scale, drop_any_time=drop_any_time, merge_dropmask=merge_dropmask,
                          keep_rows=keep_rows, out=out)
        sec = None
        if sections:
            # the level half of `reduce` left sigma in its levraw workspace; the next stage-2 call of this shape reuses it, so the
            # sections keep a copy of their own
            sec = self.section_begin(int(rows.shape[0]), int(rows.shape[2]), rows.device, n_wave=int(wavenumbers or 0),
                                     generation=spectrum_generation, keep_steps=section_steps)
            sec["levraw"] = self._workspace(int(rows.shape[0]), int(rows.shape[1]), rows.device)[1].clone()
            if wavenumbers is None:
                self.section_stage(rows, boxes, sec["levraw"], sec, 0)
        if maps:
            mp = self.map_begin(int(rows.shape[0]), boxes, rows.device, keep_steps=map_steps)
            # (sigma is read from the level stage's levraw: the sections' copy, or one of the maps' own)
            lr = sec["levraw"] if sec is not None else self._workspace(int(rows.shape[0]), int(rows.shape[1]), rows.device)[1].clone()
            self.map_stage(tair, u, v, omega, rows, boxes, lr, mp, 0, time_s=time_s, tcoef=tcoef, t_begin=t_begin)
            self.map_finish(res, mp)
        if composites:
            pb = boxes if isinstance(boxes, PreparedBoxes) else PreparedBoxes(*self._resolve_boxes(boxes))
            cp = self.composite_begin(int(rows.shape[0]), pb, rows.device, keep_steps=composite_steps)
            lr = self._workspace(int(rows.shape[0]), int(rows.shape[1]), rows.device)[1].clone()
            self.composite_stage(tair, u, v, omega, rows, pb, lr, cp, 0, time_s=time_s, dTdt=dTdt, tm=tm, tp=tp, tcoef=tcoef, t_begin=t_begin)
            self.composite_finish(res, cp)
        if composite_sections:
            pb = boxes if isinstance(boxes, PreparedBoxes) else PreparedBoxes(*self._resolve_boxes(boxes))
            cs = self.composite_section_begin(int(rows.shape[0]), pb, rows.device, keep_steps=composite_section_steps)
            lr = self._workspace(int(rows.shape[0]), int(rows.shape[1]), rows.device)[1].clone()
            self.composite_section_stage(rows, pb, lr, cs, 0)
            self.composite_section_finish(res, cs)
        if batch_composites is not None:
            pb = boxes if isinstance(boxes, PreparedBoxes) else PreparedBoxes(*self._resolve_boxes(boxes))
            bc = self.batch_composite_begin(batch_composites, pb, rows.device, keep_steps=batch_composite_steps,
                                            phases=batch_composite_phases)
            lr = self._workspace(int(rows.shape[0]), int(rows.shape[1]), rows.device)[1].clone()
            self.batch_composite_stage(tair, u, v, omega, rows, pb, lr, bc, 0, steps=steps, tcoef=tcoef, steps_host=steps_host)
            self.batch_composite_finish(res, bc)
        if lon_sections:
            ls = self.lonsection_begin(int(rows.shape[0]), boxes, rows.device, keep_steps=lon_section_steps)
            lr = sec["levraw"] if sec is not None else self._workspace(int(rows.shape[0]), int(rows.shape[1]), rows.device)[1].clone()
            self.lonsection_stage(tair, u, v, omega, rows, boxes, lr, ls, 0, time_s=time_s, tcoef=tcoef, t_begin=t_begin)
            self.lonsection_finish(res, ls)
        if composite_lon_sections:
            pb = boxes if isinstance(boxes, PreparedBoxes) else PreparedBoxes(*self._resolve_boxes(boxes))
            cl = self.composite_lonsection_begin(int(rows.shape[0]), pb, rows.device, keep_steps=composite_lon_section_steps)
            lr = self._workspace(int(rows.shape[0]), int(rows.shape[1]), rows.device)[1].clone()
            self.composite_lonsection_stage(tair, u, v, omega, rows, pb, lr, cl, 0, time_s=time_s, dTdt=dTdt, tm=tm, tp=tp, tcoef=tcoef,
                                            t_begin=t_begin)
            self.composite_lonsection_finish(res, cl)
        if wavenumbers is not None:
            self._spectrum(res, rows, tair, u, v, omega, boxes, int(wavenumbers), t_begin, phi_scale, drop_any_time,
                           generation=dict(time_s=time_s, tcoef=tcoef) if spectrum_generation else None, fused=spectrum_fused,
                           interactions=spectrum_interactions, budget=spectrum_budget, sections=sec)
            if spectrum_budget:
                self.spectrum_budget_terms(res, time_s)
        if sec is not None:
            self.section_finish(res, sec)
        return res

    # -- latitude x pressure sections of one fixed box (lec_sections) -----------------------------------------------------------------
    SECTION_SPEC_TERMS = ("Ae", "Ke", "Ca", "Ce", "Ck", "Ge")      # the order of lec_sections' spectral functions (Ge with qspec only)

    @staticmethod
    def _check_sections(boxes, per_step_boxes, steps=None, tm=None, tp=None) -> None:
        n = len(boxes.boxes) if isinstance(boxes, PreparedBoxes) else len(boxes)
        if per_step_boxes or n != 1 or steps is not None or tm is not None or tp is not None:
            raise ValueError("sections exist for ONE fixed box: a series of per-step boxes (a track, chosen boxes, a packed layout) has "
                             "no common rows to lay a section on")

    def _section_accumulators(self, t_total: int, nyb: int, device, keep_steps: bool) -> dict:
        """The accumulators that ``section_*`` and ``composite_section_*`` have alike, zeroed: the time sums, the column values and --
        on request -- the per-step sections of ``t_total`` steps on ``nyb`` rows."""
        nl = int(self.level.size)
        f64 = dict(dtype=torch.float64, device=device)
        return dict(t_total=int(t_total), nyb=int(nyb), secsum=torch.zeros((nl, _lib.LEC_NSECTION, nyb), **f64),
                    col=torch.empty((t_total, _lib.LEC_NSECTION, nyb), **f64),
                    steps=torch.empty((t_total, nl, _lib.LEC_NSECTION, nyb), **f64) if keep_steps else None, work=None)

    @staticmethod
    def _section_chunk(who: str, rows: torch.Tensor, levraw: torch.Tensor, state: dict, t_offset: int, nyb: int) -> torch.Tensor:
        """What ``section_stage`` and ``composite_section_stage`` do alike once their boxes are checked: the chunk's fit into the series,
        ``levraw``'s check, and where the chunk's sections go -- its steps of ``state["steps"]``, or the workspace grown to the chunk."""
        t_count, nl = int(rows.shape[0]), int(rows.shape[1])
        if nyb != state["nyb"] or not (0 <= t_offset and t_offset + t_count <= state["t_total"]):
            raise ValueError(f"{who}_stage: the chunk does not fit the series {who}_begin was given")
        if (levraw.shape != (t_count, nl, _lib.LEC_NLEVRAW) or levraw.dtype != torch.float64 or levraw.device != rows.device
                or not levraw.is_contiguous()):
            raise ValueError("levraw must be a contiguous fp64 [t_count, nl, 40] tensor on the rows' device")
        if state["steps"] is not None:
            return state["steps"][t_offset: t_offset + t_count]
        if state["work"] is None or state["work"].shape[0] < t_count:
            state["work"] = torch.empty((t_count, nl, _lib.LEC_NSECTION, nyb), dtype=torch.float64, device=rows.device)
        return state["work"][:t_count]

    def section_begin(self, t_total: int, nyb: int, device, *, n_wave: int = 0, generation: bool = False, keep_steps: bool = False) -> dict:
        """The accumulators of the sections of a series of ``t_total`` steps (zeroed once, here): ``section_stage`` adds every chunk to
        them, ``section_finish`` turns them into the result's fields."""
        nf = 6 if generation else 5
        return dict(self._section_accumulators(t_total, nyb, device, keep_steps), n_wave=int(n_wave), nf=nf, generation=bool(generation),
                    specwork=None,
                    speccolsum=torch.zeros((n_wave, nf, nyb), dtype=torch.float64, device=device) if n_wave else None)

    def section_stage(self, rows: torch.Tensor, boxes, levraw: torch.Tensor, state: dict, t_offset: int, *,
                      spec: Optional[torch.Tensor] = None, qspec: Optional[torch.Tensor] = None) -> None:
        """``lec_sections`` on a chunk: rows [t_count, nl, nyb, 32] and ``levraw`` [t_count, nl, 40] as ``level_stage`` left it for the
        same steps (sigma is read from it) -> the chunk's sections, their column values into ``state["col"][t_offset: t_offset + t_count]``
        and their time sums added to ``state["secsum"]`` (``section_begin``).  ``spec`` [t_count, nl, nyb, N, 8] / ``qspec`` [t_count,
        nl, nyb, N] (a ring's ``rowspec`` / ``rowspec_q``): also the sections of the wavenumbers' shares, their column values summed
        over time into ``state["speccolsum"]``.  Chunks must come in time order; every number is independent of how the series is cut."""
        t_count, nl = int(rows.shape[0]), int(rows.shape[1])
        boxes, bt, dev = self._stage2_input(rows, boxes)
        self._check_sections(boxes, False)
        nyb = bt.nyb_max
        sec = self._section_chunk("section", rows, levraw, state, t_offset, nyb)
        n = state["n_wave"]
        if (spec is None) != (n == 0):
            raise ValueError("section_stage: spec goes with section_begin(n_wave=N)")
        if spec is not None and (spec.shape != (t_count, nl, nyb, n, 8) or spec.dtype != torch.float64 or spec.device != rows.device
                                 or not spec.is_contiguous()):
            raise ValueError("spec must be a contiguous fp64 [t_count, nl, nyb, N, 8] tensor on the rows' device")
        if (qspec is not None) != (n > 0 and state["generation"]):
            raise ValueError("section_stage: qspec goes with section_begin(generation=True)")
        if qspec is not None and (qspec.shape != (t_count, nl, nyb, n) or qspec.dtype != torch.float64 or qspec.device != rows.device
                                  or not qspec.is_contiguous()):
            raise ValueError("qspec must be a contiguous fp64 [t_count, nl, nyb, N] tensor on the rows' device")
        f64 = dict(dtype=torch.float64, device=rows.device)
        specsec = None
        if n:
            if state["specwork"] is None or state["specwork"].shape[0] < t_count:
                state["specwork"] = torch.empty((t_count, nl, n, state["nf"], nyb), **f64)
            specsec = state["specwork"][:t_count]
        sa = _lib.SectionsArgs(
            rows_d=_ptr(rows), t_count=t_count, nl=nl, n_box=1, nyb=nyb, box_d=_ptr(dev["box"]), lattab2_d=_ptr(dev["lattab2"]),
            levtab2_d=_ptr(self._levtab2), levraw_d=_ptr(levraw), sec_d=_ptr(sec), col_d=_ptr(state["col"][t_offset: t_offset + t_count]),
            secsum_d=_ptr(state["secsum"]), spec_d=_ptr(spec), qspec_d=_ptr(qspec), n_wave=n, reserved0=0, specsec_d=_ptr(specsec),
            speccolsum_d=_ptr(state["speccolsum"]), stream=C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream))
        with torch.cuda.device(rows.device):
            _lib.check(self.lib.lec_sections(C.byref(sa)), "lec_sections")

    def section_finish(self, res: LECResult, state: dict) -> None:
        """``res.section_*`` from the accumulators of a finished series."""
        t_total = state["t_total"]
        res.section_mean = (state["secsum"] / float(t_total)).permute(1, 0, 2).contiguous()
        res.section_lat = state["col"]
        if state["steps"] is not None:
            res.section_steps = state["steps"].permute(0, 2, 1, 3).contiguous()
        if state["n_wave"]:
            # the totals' column values summed over time in time order too, so that the rest does not depend on the chunks either
            idx = torch.as_tensor([SECTION_TERMS.index(x) for x in self.SECTION_SPEC_TERMS[:state["nf"]]], device=state["col"].device)
            tot = torch.zeros((state["nf"], state["nyb"]), dtype=torch.float64, device=state["col"].device)
            for t in range(t_total):
                tot += state["col"][t].index_select(0, idx)
            shares = state["speccolsum"].permute(1, 0, 2)            # [F, N, nyb]
            ssum = shares[:, 0].clone()
            for k in range(1, state["n_wave"]):
                ssum += shares[:, k]
            res.section_spec_lat = (torch.cat([shares, (tot - ssum).unsqueeze(1)], dim=1) / float(t_total)).contiguous()

    # -- system-relative sections over per-step boxes of one row count (lec_composite_sections) ------------------------------------------
    @staticmethod
    def _check_composite_sections(boxes, per_step_boxes) -> int:
        """The refusals of the system-relative sections that need nothing but the boxes: returns nyb, the one row count of every box."""
        # (a series has thousands of boxes: no Python loop over them; PreparedBoxes hold them as an int32 [n, 4] table already)
        bx = boxes.bt.box if isinstance(boxes, PreparedBoxes) else np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
        if per_step_boxes is False or (per_step_boxes is None and len(bx) == 1):
            raise ValueError("composite sections exist for per-step boxes (per_step_boxes=True): a system-relative section is laid on the "
                             "box-relative rows of a series of moving boxes; ONE fixed box has sections=True")
        h = bx[:, 3].astype(np.int64) - bx[:, 2] + 1
        nyb = int(h[0])
        other = np.flatnonzero(h != nyb)
        if other.size:
            t = int(other[0])
            raise ValueError(f"composite sections need boxes of ONE row count: the box of step {t} has {int(h[t])} rows, that of "
                             f"step 0 has {nyb}")
        if nyb < 2:
            raise ValueError("composite sections need at least 2 box rows")
        return nyb

    def composite_section_begin(self, t_total: int, boxes: PreparedBoxes, device, *, keep_steps: bool = False) -> dict:
        """The accumulators of the system-relative sections of a series of ``t_total`` steps whose boxes all have the row count of
        ``boxes``' (zeroed once, here): ``composite_section_stage`` adds every chunk to them, ``composite_section_finish`` turns them
        into the result's fields."""
        nyb = self._check_composite_sections(boxes, True)
        if boxes.bt.nyb_max != nyb:
            raise ValueError("composite sections: the boxes' records must have the boxes' own row count (prepare_boxes without nyb_min)")
        return self._section_accumulators(t_total, nyb, device, keep_steps)

    def composite_section_stage(self, rows: torch.Tensor, boxes: PreparedBoxes, levraw: torch.Tensor, state: dict, t_offset: int) -> None:
        """``lec_composite_sections`` on a chunk: rows [t_count, nl, nyb, 32] of one box of ``boxes`` per step (packed or not: only the
        records are read) and ``levraw`` [t_count, nl, 40] as ``level_stage`` left it for the same steps (sigma is read from it) -> the
        chunk's sections on box-relative rows, their column values into ``state["col"][t_offset: t_offset + t_count]`` and their time sums
        added to ``state["secsum"]`` (``composite_section_begin``).  Chunks must come in time order; every number is independent of how
        the series is cut, bit for bit."""
        if not isinstance(boxes, PreparedBoxes):
            raise ValueError("composite_section_stage: boxes from prepare_boxes")
        t_count, nl = int(rows.shape[0]), int(rows.shape[1])
        bx, bt, dev = self._stage2_input(rows, boxes)
        if len(bx) != t_count:
            raise ValueError("composite_section_stage: one box per step of the chunk")
        nyb = self._check_composite_sections(boxes, True)
        if bt.nyb_max != nyb:
            raise ValueError("composite sections: the boxes' records must have the boxes' own row count (prepare_boxes without nyb_min)")
        sec = self._section_chunk("composite_section", rows, levraw, state, t_offset, nyb)
        packed = "box_data" in dev
        box_host = np.ascontiguousarray(bt.box, dtype=np.int32)
        if packed:          # as the cubes hold them: every box at the origin of its slab
            zero = np.zeros(len(box_host), dtype=np.int32)
            box_host = np.ascontiguousarray(np.stack([zero, box_host[:, 1] - box_host[:, 0], zero, box_host[:, 3] - box_host[:, 2]], axis=1))
        ca = _lib.CompositeSectionsArgs(
            rows_d=_ptr(rows), levraw_d=_ptr(levraw), t_count=t_count, nl=nl, nyb=nyb, reserved0=0,
            box_h=C.c_void_p(box_host.ctypes.data), box_d=_ptr(dev["box_data" if packed else "box"]), lattab2_d=_ptr(dev["lattab2"]),
            levtab2_d=_ptr(self._levtab2), sec_d=_ptr(sec), col_d=_ptr(state["col"][t_offset: t_offset + t_count]),
            secsum_d=_ptr(state["secsum"]), stream=C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream))
        with torch.cuda.device(rows.device):
            _lib.check(self.lib.lec_composite_sections(C.byref(ca)), "lec_composite_sections")

    def composite_section_finish(self, res: LECResult, state: dict) -> None:
        """``res.composite_section_*`` from the accumulators of a finished series."""
        res.composite_section_mean = (state["secsum"] / float(state["t_total"])).permute(1, 0, 2).contiguous()
        res.composite_section_lat = state["col"]
        if state["steps"] is not None:
            res.composite_section_steps = state["steps"].permute(0, 2, 1, 3).contiguous()

    # -- the family of csrc/lec_mapcol.h: maps and longitude x pressure sections of the eddy terms on one fixed box (lec_maps,
    # lec_lonsections), composites and composite sections over per-step boxes of one shape (lec_composite, lec_composite_lonsections) ------
    # the per-step output and the row factors of the steps of ONE call: a chunk that needs more is cut into sub-calls
    MAP_CHUNK_BYTES = 256 << 20
    # the two outputs of the family: (``state``'s key of the time sums, the args structs' field of the per-step output, that of its time
    # sums, whether the output is laid on the box's rows).  A step's output is [LEC_NMAP, ext, nxb]: ext is nyb where it is, and Hovmoeller
    # rows ``state["hov"]`` go with it; for the sections ext is nl
    _MAPS_OUT = ("mapsum", "col_d", "mapsum_d", True)
    _LONSEC_OUT = ("lonsecsum", "lonsec_d", "lonsecsum_d", False)

    def _mapcol_begin(self, out: tuple, t_total: int, nyb: int, nxb: int, device, keep_steps: bool) -> dict:
        """The accumulators of the output ``out`` over ``t_total`` steps on boxes of ``nyb`` x ``nxb`` points, zeroed."""
        f64 = dict(dtype=torch.float64, device=device)
        total, _, _, on_rows = out
        ext = nyb if on_rows else int(self.level.size)
        state = dict(t_total=int(t_total), nyb=nyb, nxb=nxb, ext=ext, out=out, work=None, coef=None)
        state[total] = torch.zeros((_lib.LEC_NMAP, ext, nxb), **f64)
        if on_rows:
            state["hov"] = torch.empty((t_total, _lib.LEC_NMAP, nxb), **f64)
        state["steps"] = torch.empty((t_total, _lib.LEC_NMAP, ext, nxb), **f64) if keep_steps else None
        return state

    def _mapcol_sub(self, nl: int, state: dict, t_count: int) -> int:
        """Steps per sub-call of a chunk of ``t_count`` steps: as many as keep the per-step output and the row factors within
        ``MAP_CHUNK_BYTES``."""
        per_step = 8 * (_lib.LEC_NMAP * state["ext"] * state["nxb"] + nl * state["nyb"] * _lib.LEC_MAPS_NCOEF)
        return max(1, min(t_count, int(self.MAP_CHUNK_BYTES) // per_step))

    def _mapcol_stage(self, cubes, rows: torch.Tensor, levraw: torch.Tensor, state: dict, t_offset: int, t_begin: int, issue) -> None:
        """What the stages of the family do alike once their own arguments are checked: ``levraw``'s check, the cut of the chunk into
        sub-calls whose per-step output and row factors stay within ``MAP_CHUNK_BYTES``, the workspaces grown to a sub-call, and the
        sub-calls in time order: ``issue(a, b, shared)`` calls on the chunk's steps [a, b), ``shared`` the fields the args structs of
        ``state``'s output have in common."""
        tair, u, v, omega = cubes
        nt, nl, ny, nx = (int(x) for x in tair.shape)
        t_count, nyb, nxb, ext = int(rows.shape[0]), state["nyb"], state["nxb"], state["ext"]
        total, step_field, sum_field, on_rows = state["out"]
        if (levraw.shape != (t_count, nl, _lib.LEC_NLEVRAW) or levraw.dtype != torch.float64 or levraw.device != rows.device
                or not levraw.is_contiguous()):
            raise ValueError("levraw must be a contiguous fp64 [t_count, nl, 40] tensor on the rows' device")
        if not on_rows and ext != nl:
            raise ValueError("the cubes' levels are not the engine's")
        f64 = dict(dtype=torch.float64, device=rows.device)
        sub = self._mapcol_sub(nl, state, t_count)
        if state["coef"] is None or state["coef"].shape[0] < sub:
            state["coef"] = torch.empty((sub, nl, nyb, _lib.LEC_MAPS_NCOEF), **f64)
        if state["steps"] is None and (state["work"] is None or state["work"].shape[0] < sub):
            state["work"] = torch.empty((sub, _lib.LEC_NMAP, ext, nxb), **f64)
        for a in range(0, t_count, sub):
            b = min(t_count, a + sub)
            step = state["steps"][t_offset + a: t_offset + b] if state["steps"] is not None else state["work"][: b - a]
            shared = dict(
                tair_d=_ptr(tair), u_d=_ptr(u), v_d=_ptr(v), omega_d=_ptr(omega),
                dtype=_lib.LEC_F64 if tair.dtype == torch.float64 else _lib.LEC_F32, nt=nt, nl=nl, ny=ny, nx=nx,
                t_begin=t_begin + a, t_count=b - a, reserved0=0, rows_d=_ptr(rows[a:b]), levraw_d=_ptr(levraw[a:b]),
                levtab_d=_ptr(self._levtab), levtab2_d=_ptr(self._levtab2), coef_d=_ptr(state["coef"]),
                stream=C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream))
            shared[step_field], shared[sum_field] = _ptr(step), _ptr(state[total])
            if on_rows:
                shared["hov_d"] = _ptr(state["hov"][t_offset + a: t_offset + b])
            with torch.cuda.device(rows.device):
                issue(a, b, shared)

    @staticmethod
    def _check_maps(boxes, per_step_boxes, steps=None, tm=None, tp=None) -> None:
        n = len(boxes.boxes) if isinstance(boxes, PreparedBoxes) else len(boxes)
        if per_step_boxes or n != 1 or steps is not None or tm is not None or tp is not None:
            raise ValueError("maps exist for ONE fixed box: a series of per-step boxes (a track, chosen boxes, a packed layout) has "
                             "no common points to lay a map on")

    @staticmethod
    def _check_lonsections(boxes, per_step_boxes, steps=None, tm=None, tp=None) -> None:
        n = len(boxes.boxes) if isinstance(boxes, PreparedBoxes) else len(boxes)
        if per_step_boxes or n != 1 or steps is not None or tm is not None or tp is not None:
            raise ValueError("longitude-pressure sections exist for ONE fixed box: a series of per-step boxes (a track, chosen boxes, a "
                             "packed layout) has no common columns to lay a section on; it has composite_lon_sections=True")

    def _fixed_begin(self, out: tuple, noun: str, check, t_total: int, boxes, device, keep_steps: bool) -> dict:
        """``map_begin`` and ``lonsection_begin``: the fixed box's refusals in the words of the output ``noun``, then its accumulators."""
        check(boxes, False)
        bx, bt, _ = self._resolve_boxes(boxes)
        iw, ie, js, jn = bx[0]
        nyb, nxb = jn - js + 1, ie - iw + 1
        if bt.nyb_max != nyb:
            raise ValueError(f"{noun}: the box's records must have the box's own row count (prepare_boxes without nyb_min)")
        if not bt.lon_uniform:
            raise ValueError(f"{noun} need evenly spaced longitudes: the d/dlon of Q at a point is the uniform axis' difference")
        if nxb < 3:
            raise ValueError(f"{noun} need at least 3 box columns")
        return self._mapcol_begin(out, t_total, nyb, nxb, device, keep_steps)

    def _fixed_chunk(self, who: str, begin: str, check, struct, call: str, *, cubes, rows, boxes, levraw, state: dict, t_offset: int,
                     t_begin: int, time_s, tcoef) -> None:
        """``map_stage`` and ``lonsection_stage``: the chunk against the cubes and against ``state``, then the C call ``call`` on the args
        struct ``struct`` per sub-call.  The stage's own arguments come by keyword, ``cubes`` = (tair, u, v, omega)."""
        tair, u, v, omega = cubes
        self._check_fields([tair, u, v, omega], None)
        nt, t_count = int(tair.shape[0]), int(rows.shape[0])
        bx, bt, dev = self._stage2_input(rows, boxes)
        check(bx, False)
        iw, ie, js, jn = bx[0]
        nyb, nxb = jn - js + 1, ie - iw + 1
        if (nyb != state["nyb"] or nxb != state["nxb"] or bt.nyb_max != nyb
                or not (0 <= t_offset and t_offset + t_count <= state["t_total"])):
            raise ValueError(f"{who}: the chunk does not fit the series and box {begin} was given")
        if not (0 <= t_begin and t_begin + t_count <= nt):
            raise ValueError(f"{who}: [t_begin, t_begin + t_count) lies outside the cubes")
        if rows.device != tair.device:
            raise ValueError(f"{who}: rows and fields on one device")
        tcoef = self._cube_tcoef(who, time_s, tcoef, nt, tair.device)

        def issue(a, b, shared):
            fa = struct(iw=iw, ie=ie, js=js, jn=jn, ring=1 if bt.ring else 0, lattab2_d=_ptr(dev["lattab2"]), lattab_d=_ptr(dev["lattab"]),
                        tcoef_d=_ptr(tcoef), inv_hdeg=float(bt.boxtab[0, 2]), **shared)
            _lib.check(getattr(self.lib, call)(C.byref(fa)), call)
        self._mapcol_stage((tair, u, v, omega), rows, levraw, state, t_offset, t_begin, issue)

    def map_begin(self, t_total: int, boxes, device, *, keep_steps: bool = False) -> dict:
        """The accumulators of the maps of a series of ``t_total`` steps on the fixed box ``boxes`` (zeroed once, here): ``map_stage``
        adds every chunk to them, ``map_finish`` turns them into the result's fields."""
        return self._fixed_begin(self._MAPS_OUT, "maps", self._check_maps, t_total, boxes, device, keep_steps)

    def map_stage(self, tair: torch.Tensor, u: torch.Tensor, v: torch.Tensor, omega: torch.Tensor, rows: torch.Tensor, boxes,
                  levraw: torch.Tensor, state: dict, t_offset: int, *, time_s=None, tcoef: Optional[torch.Tensor] = None,
                  t_begin: int = 0) -> None:
        """``lec_maps`` on a chunk: the cubes' steps [t_begin, t_begin + t_count), their row records ``rows`` [t_count, nl, nyb, 32] and
        ``levraw`` [t_count, nl, 40] as ``level_stage`` left it for the same steps (sigma is read from it) -> the Hovmoeller rows
        ``state["hov"][t_offset: t_offset + t_count]`` and the time sums added to ``state["mapsum"]`` (``map_begin``).  dT/dt over the
        cube's time axis ``time_s`` (seconds, one entry per step of the cube) or ``tcoef``, as ``rowspec_q`` takes them.  A chunk whose
        column values and row factors exceed ``MAP_CHUNK_BYTES`` is cut into sub-calls.  Chunks must come in time order; every number is
        independent of how the series is cut, bit for bit."""
        self._fixed_chunk("map_stage", "map_begin", self._check_maps, _lib.MapsArgs, "lec_maps", cubes=(tair, u, v, omega), rows=rows,
                          boxes=boxes, levraw=levraw, state=state, t_offset=t_offset, t_begin=t_begin, time_s=time_s, tcoef=tcoef)

    def map_finish(self, res: LECResult, state: dict) -> None:
        """``res.map_*`` from the accumulators of a finished series."""
        res.map_mean = state["mapsum"] / float(state["t_total"])
        res.map_lon = state["hov"]
        if state["steps"] is not None:
            res.map_steps = state["steps"]

    def lonsection_begin(self, t_total: int, boxes, device, *, keep_steps: bool = False) -> dict:
        """The accumulators of the longitude x pressure sections of a series of ``t_total`` steps on the fixed box ``boxes`` (zeroed once,
        here): ``lonsection_stage`` adds every chunk to them, ``lonsection_finish`` turns them into the result's fields."""
        return self._fixed_begin(self._LONSEC_OUT, "longitude-pressure sections", self._check_lonsections, t_total, boxes, device, keep_steps)

    def lonsection_stage(self, tair: torch.Tensor, u: torch.Tensor, v: torch.Tensor, omega: torch.Tensor, rows: torch.Tensor, boxes,
                         levraw: torch.Tensor, state: dict, t_offset: int, *, time_s=None, tcoef: Optional[torch.Tensor] = None,
                         t_begin: int = 0) -> None:
        """``lec_lonsections`` on a chunk, with ``map_stage``'s arguments: the time sums are added to ``state["lonsecsum"]`` and, when
        kept, the steps written to ``state["steps"][t_offset: t_offset + t_count]``.  A chunk whose sections and row factors exceed
        ``MAP_CHUNK_BYTES`` is cut into sub-calls.  Chunks must come in time order; every number is independent of how the series is cut,
        bit for bit."""
        self._fixed_chunk("lonsection_stage", "lonsection_begin", self._check_lonsections, _lib.LonSectionsArgs, "lec_lonsections",
                          cubes=(tair, u, v, omega), rows=rows, boxes=boxes, levraw=levraw, state=state, t_offset=t_offset, t_begin=t_begin,
                          time_s=time_s, tcoef=tcoef)

    def lonsection_finish(self, res: LECResult, state: dict) -> None:
        """``res.lonsection_*`` from the accumulators of a finished series."""
        res.lonsection_mean = state["lonsecsum"] / float(state["t_total"])
        if state["steps"] is not None:
            res.lonsection_steps = state["steps"]

    # (the output that asks, one of it, the fixed box's flag): the words of _check_composites' refusals
    _COMPOSITE_WORDS = ("composites", "a composite", "maps=True")
    _COMPOSITE_LONSECTION_WORDS = ("composite longitude-pressure sections", "a section", "lon_sections=True")

    @staticmethod
    def _one_shape(bx, lon_uniform: Optional[bool], noun: str, box: str, first: str) -> tuple:
        """(nyb, nxb) of boxes of ONE shape with three columns or more on evenly spaced longitudes, or the refusal in the words of the
        output ``noun``; ``box``, ``first``: how it names box t and box 0."""
        bx = [tuple(int(x) for x in b) for b in bx]
        nyb, nxb = bx[0][3] - bx[0][2] + 1, bx[0][1] - bx[0][0] + 1
        for t, b in enumerate(bx):
            h, w = b[3] - b[2] + 1, b[1] - b[0] + 1
            if (h, w) != (nyb, nxb):
                raise ValueError(f"{noun} need boxes of ONE shape: {box} {t} has {h} x {w} points (rows x columns), {first} has {nyb} x {nxb}")
        if nxb < 3:
            raise ValueError(f"{noun} need at least 3 box columns")
        if lon_uniform is False:
            raise ValueError(f"{noun} need evenly spaced longitudes: the d/dlon of Q at a point is the uniform axis' difference")
        return nyb, nxb

    @staticmethod
    def _check_composites(boxes, per_step_boxes, steps=None, lon_uniform: Optional[bool] = None,
                          what: tuple = _COMPOSITE_WORDS) -> tuple:
        """The refusals of the composites that need nothing but the boxes: returns (nyb, nxb), the one shape of every box.  ``what``: the
        words of the output that asks (the composites', or those of the composite longitude-pressure sections, which need the same)."""
        noun, one, fixed = what
        bx = boxes.boxes if isinstance(boxes, PreparedBoxes) else boxes
        if steps is not None:
            raise ValueError(f"{noun}: a step table (steps=, the batch of lec_rowstats_steps) has none: {noun} exist for ONE track")
        if per_step_boxes is False or (per_step_boxes is None and len(bx) == 1):
            raise ValueError(f"{noun} exist for per-step boxes (per_step_boxes=True): {one} is laid on the box-relative points "
                             f"of a series of moving boxes; ONE fixed box has {fixed}")
        return LECEngine._one_shape(bx, lon_uniform, noun, "the box of step", "that of step 0")

    def _composite_begin(self, out: tuple, what: tuple, t_total: int, boxes: PreparedBoxes, device, keep_steps: bool) -> dict:
        """``composite_begin`` and ``composite_lonsection_begin``: the boxes' refusals in the words ``what``, then the accumulators."""
        nyb, nxb = self._check_composites(boxes, True, None, boxes.bt.lon_uniform, what=what)
        if boxes.bt.nyb_max != nyb:
            raise ValueError(f"{what[0]}: the boxes' records must have the boxes' own row count (prepare_boxes without nyb_min)")
        return self._mapcol_begin(out, t_total, nyb, nxb, device, keep_steps)

    def _composite_chunk(self, who: str, begin: str, what: tuple, struct, call: str, *, cubes, rows, boxes, levraw, state: dict,
                         t_offset: int, t_begin: int, time_s, dTdt, tm, tp, tcoef) -> None:
        """``composite_stage`` and ``composite_lonsection_stage``: the layout and its source of dT/dt, the boxes' one shape against
        ``state``, the chunk against the cubes, then the C call ``call`` on the args struct ``struct`` per sub-call, with the boxes as
        the cubes hold them.  The stage's own arguments come by keyword, ``cubes`` = (tair, u, v, omega)."""
        tair, u, v, omega = cubes
        if not isinstance(boxes, PreparedBoxes):
            raise ValueError(f"{who}: boxes from prepare_boxes")
        packed = "box_data" in boxes.dev
        if (tm is None) != (tp is None):
            raise ValueError(f"{who}: tm and tp come together")
        if dTdt is not None and tm is not None:
            raise ValueError(f"{who}: a dTdt cube or tm / tp, not both")
        if packed and dTdt is None and tm is None:
            raise ValueError(f"{who}: a box-packed series needs its dTdt cube or tm / tp (its time neighbours are other boxes)")
        self._check_fields([tair, u, v, omega] + [c for c in (tm, tp) if c is not None], boxes if packed else None)
        nt, t_count = int(tair.shape[0]), int(rows.shape[0])
        bx, bt, dev = self._stage2_input(rows, boxes)
        if len(bx) != t_count:
            raise ValueError(f"{who}: one box per step of the chunk")
        nyb, nxb = self._check_composites(bx, True, None, bt.lon_uniform, what=what)
        if (nyb != state["nyb"] or nxb != state["nxb"] or bt.nyb_max != nyb
                or not (0 <= t_offset and t_offset + t_count <= state["t_total"])):
            raise ValueError(f"{who}: the chunk does not fit the series and box shape {begin} was given")
        if not (0 <= t_begin and t_begin + t_count <= nt):
            raise ValueError(f"{who}: [t_begin, t_begin + t_count) lies outside the cubes")
        if rows.device != tair.device:
            raise ValueError(f"{who}: rows and fields on one device")
        if dTdt is not None:
            if dTdt.shape != tair.shape or dTdt.device != tair.device or dTdt.dtype not in (torch.float64, torch.float32):
                raise ValueError("dTdt must be a cube of the fields' shape on their device")
            dTdt = dTdt.to(torch.float64).contiguous()
            tcoef = None
        elif tm is not None:
            if tcoef is None or tcoef.shape != (nt, 3) or tcoef.dtype != torch.float64 or tcoef.device != tair.device or not tcoef.is_contiguous():
                raise ValueError("tm / tp need tcoef: a contiguous fp64 [nt, 3] tensor on the fields' device (the rows of the cubes' steps)")
        else:
            tcoef = self._cube_tcoef(who, time_s, tcoef, nt, tair.device)
        box_host = np.ascontiguousarray([(0, b[1] - b[0], 0, b[3] - b[2]) for b in bx] if packed else bx, dtype=np.int32)
        box_dev = dev["box_data" if packed else "box"]

        def issue(a, b, shared):
            ca = struct(dTdt_d=_ptr(dTdt), tm_d=_ptr(tm), tp_d=_ptr(tp), nyb=nyb, nxb=nxb, tcoef_d=_ptr(tcoef),
                        box_h=C.c_void_p(box_host[a:b].ctypes.data), box_d=_ptr(box_dev[a:b]), boxtab_d=_ptr(dev["boxtab"][a:b]),
                        lattab_d=_ptr(dev["lattab"][a:b]), lattab2_d=_ptr(dev["lattab2"][a:b]), **shared)
            _lib.check(getattr(self.lib, call)(C.byref(ca)), call)
        self._mapcol_stage((tair, u, v, omega), rows, levraw, state, t_offset, t_begin, issue)

    def composite_begin(self, t_total: int, boxes: PreparedBoxes, device, *, keep_steps: bool = False) -> dict:
        """The accumulators of the composites of a series of ``t_total`` steps whose boxes all have the shape of ``boxes``' (zeroed once,
        here): ``composite_stage`` adds every chunk to them, ``composite_finish`` turns them into the result's fields."""
        return self._composite_begin(self._MAPS_OUT, self._COMPOSITE_WORDS, t_total, boxes, device, keep_steps)

    def composite_stage(self, tair: torch.Tensor, u: torch.Tensor, v: torch.Tensor, omega: torch.Tensor, rows: torch.Tensor,
                        boxes: PreparedBoxes, levraw: torch.Tensor, state: dict, t_offset: int, *, time_s=None,
                        dTdt: Optional[torch.Tensor] = None, tm: Optional[torch.Tensor] = None, tp: Optional[torch.Tensor] = None,
                        tcoef: Optional[torch.Tensor] = None, t_begin: int = 0) -> None:
        """``lec_composite`` on a chunk: the cubes' steps [t_begin, t_begin + t_count), one box of ``boxes`` per step (prepared with
        ``packed=True`` for a box-packed series, whose cubes are slabs), their row records ``rows`` [t_count, nl, nyb, 32] and ``levraw``
        [t_count, nl, 40] as ``level_stage`` left it for the same steps -> the Hovmoeller rows ``state["hov"][t_offset: t_offset + t_count]``
        and the time sums added to ``state["mapsum"]`` (``composite_begin``).  dT/dt as ``rowstats`` takes it: a ``dTdt`` cube (one in the
        fields' fp32 is widened to fp64, the value stage 1 reads), or ``tm`` / ``tp`` with ``tcoef``, or -- an unpacked cube only -- the
        cube's own time axis ``time_s`` / ``tcoef``.  A chunk whose column values and row factors exceed ``MAP_CHUNK_BYTES`` is cut into
        sub-calls.  Chunks must come in time order; every number is independent of how the series is cut, bit for bit."""
        self._composite_chunk("composite_stage", "composite_begin", self._COMPOSITE_WORDS, _lib.CompositeArgs, "lec_composite",
                              cubes=(tair, u, v, omega), rows=rows, boxes=boxes, levraw=levraw, state=state, t_offset=t_offset,
                              t_begin=t_begin, time_s=time_s, dTdt=dTdt, tm=tm, tp=tp, tcoef=tcoef)

    def composite_finish(self, res: LECResult, state: dict) -> None:
        """``res.composite_*`` from the accumulators of a finished series."""
        res.composite_mean = state["mapsum"] / float(state["t_total"])
        res.composite_lon = state["hov"]
        if state["steps"] is not None:
            res.composite_steps = state["steps"]

    def composite_lonsection_begin(self, t_total: int, boxes: PreparedBoxes, device, *, keep_steps: bool = False) -> dict:
        """The accumulators of the composite longitude x pressure sections of a series of ``t_total`` steps whose boxes all have the shape
        of ``boxes``' (zeroed once, here)."""
        return self._composite_begin(self._LONSEC_OUT, self._COMPOSITE_LONSECTION_WORDS, t_total, boxes, device, keep_steps)

    def composite_lonsection_stage(self, tair: torch.Tensor, u: torch.Tensor, v: torch.Tensor, omega: torch.Tensor, rows: torch.Tensor,
                                   boxes: PreparedBoxes, levraw: torch.Tensor, state: dict, t_offset: int, *, time_s=None,
                                   dTdt: Optional[torch.Tensor] = None, tm: Optional[torch.Tensor] = None,
                                   tp: Optional[torch.Tensor] = None, tcoef: Optional[torch.Tensor] = None, t_begin: int = 0) -> None:
        """``lec_composite_lonsections`` on a chunk, with ``composite_stage``'s arguments (layouts and the three sources of dT/dt): the
        time sums are added to ``state["lonsecsum"]`` and, when kept, the steps written to ``state["steps"]``.  Chunks must come in time
        order; every number is independent of how the series is cut, bit for bit."""
        self._composite_chunk("composite_lonsection_stage", "composite_lonsection_begin", self._COMPOSITE_LONSECTION_WORDS,
                              _lib.CompositeLonSectionsArgs, "lec_composite_lonsections", cubes=(tair, u, v, omega), rows=rows, boxes=boxes,
                              levraw=levraw, state=state, t_offset=t_offset, t_begin=t_begin, time_s=time_s, dTdt=dTdt, tm=tm, tp=tp,
                              tcoef=tcoef)

    def composite_lonsection_finish(self, res: LECResult, state: dict) -> None:
        """``res.composite_lonsection_*`` from the accumulators of a finished series."""
        res.composite_lonsection_mean = state["lonsecsum"] / float(state["t_total"])
        if state["steps"] is not None:
            res.composite_lonsection_steps = state["steps"]

    # -- composites of a batch of tracks over one cube and their ensemble (lec_composite_steps, lec_composite_ensemble) ------------------
    @staticmethod
    def _check_batch_composites(boxes, n_rows: int, sizes, lon_uniform: Optional[bool] = None) -> tuple:
        """The refusals of the batch composites that need nothing but the boxes, the step table's row count and the tracks' sizes: returns
        (nyb, nxb), the one shape of every box."""
        bx = boxes.boxes if isinstance(boxes, PreparedBoxes) else boxes
        sizes = [int(n) for n in sizes]
        if not sizes or min(sizes) < 1:
            raise ValueError(f"batch_composites: every track needs at least one box, the sizes are {sizes}")
        if sum(sizes) != len(bx) or sum(sizes) != n_rows:
            raise ValueError(f"batch_composites: the sizes sum to {sum(sizes)}, the step table has {n_rows} rows and there are "
                             f"{len(bx)} boxes: one box and one row per step of every track")
        return LECEngine._one_shape(bx, lon_uniform, "batch composites", "box", "box 0")

    @staticmethod
    def _check_batch_phases(sizes, ranges) -> np.ndarray:
        """The refusals of ``batch_composite_phases`` that need nothing but the tracks' sizes: returns the ranges as int32 [K, B, 2]."""
        sizes = [int(n) for n in sizes]
        try:
            r = np.asarray(ranges)
        except (ValueError, TypeError):
            r = np.empty(0, dtype=object)
        if r.ndim != 3 or r.shape[0] != len(sizes) or r.shape[1] < 1 or r.shape[2] != 2 or r.dtype.kind not in "iu":
            raise ValueError(f"batch_composite_phases: an integer array [K, B, 2] of B >= 1 ranges [begin, end) for each of the K = {len(sizes)} "
                             f"tracks, not {getattr(r, 'dtype', None)} {tuple(r.shape)}")
        r = r.astype(np.int64)
        for k, n in enumerate(sizes):
            for b in range(r.shape[1]):
                lo, hi = int(r[k, b, 0]), int(r[k, b, 1])
                if lo < 0:
                    raise ValueError(f"batch_composite_phases: track {k}, bin {b}: the range [{lo}, {hi}) begins before the track's first step")
                if lo > hi:
                    raise ValueError(f"batch_composite_phases: track {k}, bin {b}: the range [{lo}, {hi}) has begin > end (an empty range has begin = end)")
                if hi > n:
                    raise ValueError(f"batch_composite_phases: track {k}, bin {b}: the range [{lo}, {hi}) ends after the track's {n} steps")
        return np.ascontiguousarray(r, dtype=np.int32)

    def batch_composite_begin(self, sizes: Sequence[int], boxes: PreparedBoxes, device, *, keep_steps: bool = False, phases=None) -> dict:
        """The accumulators of the composites of K tracks whose boxes are ``boxes``, track k owning ``sizes[k]`` consecutive ones (zeroed
        once, here): ``batch_composite_stage`` adds every chunk to them, ``batch_composite_finish`` turns them into the result's fields.
        ``phases``: ranges [K, B, 2] of the tracks' own steps (``compute``'s ``batch_composite_phases``): also the zeroed accumulator
        [K, B, 6, nyb, nxb] of the cells' sums."""
        sizes = [int(n) for n in sizes]
        if phases is not None:
            phases = self._check_batch_phases(sizes, phases)
        nyb, nxb = self._check_batch_composites(boxes, len(boxes.boxes), sizes, boxes.bt.lon_uniform)
        if boxes.bt.nyb_max != nyb:
            raise ValueError("batch composites: the boxes' records must have the boxes' own row count (prepare_boxes without nyb_min above it)")
        state = self._mapcol_begin(self._MAPS_OUT, sum(sizes), nyb, nxb, device, keep_steps)
        state["mapsum"] = torch.zeros((len(sizes), _lib.LEC_NMAP, nyb, nxb), dtype=torch.float64, device=device)
        state["sizes"] = np.ascontiguousarray(sizes, dtype=np.int32)
        state["sizes_dev"] = torch.as_tensor(state["sizes"]).to(device)      # (uploaded here: an upload after the launches would wait for them)
        state["seg"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        if phases is not None:
            n_bin = int(phases.shape[1])
            state["phasesum"] = torch.zeros((len(sizes), n_bin, _lib.LEC_NMAP, nyb, nxb), dtype=torch.float64, device=device)
            # the cells' ranges in the batch's boxes, cell = k * B + b
            state["phase_abs"] = (phases.astype(np.int64) + state["seg"][:-1, None, None]).reshape(-1, 2)
            state["phase_count"] = np.ascontiguousarray(phases[:, :, 1] - phases[:, :, 0], dtype=np.int32)
            state["phase_count_dev"] = torch.as_tensor(state["phase_count"]).to(device)
        return state

    def batch_composite_stage(self, tair: torch.Tensor, u: torch.Tensor, v: torch.Tensor, omega: torch.Tensor, rows: torch.Tensor,
                              boxes: PreparedBoxes, levraw: torch.Tensor, state: dict, t_offset: int, *, steps: torch.Tensor,
                              tcoef: torch.Tensor, steps_host: Optional[np.ndarray] = None) -> None:
        """``lec_composite_steps`` on a chunk of the batch's boxes [t_offset, t_offset + s_count): one box of ``boxes``, one row of
        ``steps`` / ``tcoef`` and one record of ``rows`` [s_count, nl, nyb, 32] / ``levraw`` [s_count, nl, 40] each -> the Hovmoeller rows
        ``state["hov"][t_offset: t_offset + s_count]`` and every track's time sum added to its ``state["mapsum"][k]``.  A chunk whose
        column values and row factors exceed ``MAP_CHUNK_BYTES`` is cut into sub-calls; a sub-call passes the tracks it intersects as
        segments and the first of their accumulators.  Chunks must come in table order; a track cut by a sub-call or a chunk has the
        bits of one that is not.  ``steps_host``: the caller's host copy of ``steps`` (int32 [s_count, 3]; the caller keeps the two
        equal), which the call validates; without it the table is copied back from the device, which waits for the stream."""
        if not isinstance(boxes, PreparedBoxes) or "box_data" in boxes.dev:
            raise ValueError("batch_composite_stage: boxes from prepare_boxes, on the cubes' grid (a box-packed series has no step table)")
        self._check_fields([tair, u, v, omega], None)
        nt, s_count = int(tair.shape[0]), int(rows.shape[0])
        bx, bt, dev = self._stage2_input(rows, boxes)
        if len(bx) != s_count:
            raise ValueError("batch_composite_stage: one box per record of the chunk")
        if steps_host is None:
            if self.check_steps(steps, tcoef, nt, tair.device) != s_count:
                raise ValueError("batch_composite_stage: one table row per record of the chunk")
            steps_host = steps.cpu().numpy()
        step_host = np.ascontiguousarray(steps_host, dtype=np.int32)
        if (step_host.shape != (s_count, 3) or not isinstance(steps, torch.Tensor) or steps.dtype != torch.int32 or tuple(steps.shape) != (s_count, 3)
                or steps.device != tair.device or not steps.is_contiguous()):
            raise ValueError("batch_composite_stage: steps must be a contiguous int32 [s_count, 3] tensor on the fields' device, steps_host its host copy")
        if (not isinstance(tcoef, torch.Tensor) or tuple(tcoef.shape) != (s_count, 3) or tcoef.dtype != torch.float64 or tcoef.device != tair.device
                or not tcoef.is_contiguous()):
            raise ValueError(f"batch_composite_stage: tcoef must be a contiguous fp64 [{s_count}, 3] tensor (by box) on the fields' device")
        bad = np.flatnonzero(np.any((step_host < 0) | (step_host >= nt), axis=1))
        if bad.size:
            raise ValueError(f"steps: box {int(bad[0])} names cube steps {step_host[bad[0]].tolist()} outside [0, {nt})")
        seg = state["seg"]
        if (bt.nyb_max != state["nyb"] or not (0 <= t_offset and t_offset + s_count <= state["t_total"])
                or any((b[3] - b[2] + 1, b[1] - b[0] + 1) != (state["nyb"], state["nxb"]) for b in bx)):
            raise ValueError("batch_composite_stage: the chunk does not fit the boxes and shape batch_composite_begin was given")
        if rows.device != tair.device:
            raise ValueError("batch_composite_stage: rows and fields on one device")
        box_host = np.ascontiguousarray(bx, dtype=np.int32)
        # every sub-call [a, b): the tracks it intersects, their offsets relative to a, and the first of their accumulators.  The tables
        # of all sub-calls go to the device in ONE upload before the first launch (an upload between the sub-calls would wait for them)
        sub, cuts, n_off = self._mapcol_sub(int(rows.shape[1]), state, s_count), {}, 0
        for a in range(0, s_count, sub):
            lo, hi = t_offset + a, t_offset + min(s_count, a + sub)
            g0, g1 = int(np.searchsorted(seg, lo, side="right")) - 1, int(np.searchsorted(seg, hi, side="left"))
            cuts[a] = (g0, g1, n_off, np.ascontiguousarray(np.clip(seg[g0: g1 + 1], lo, hi) - lo, dtype=np.int32))
            n_off += g1 - g0 + 1
        # the phases' cells likewise: the contiguous run from the first to the last cell whose range holds a box of the sub-call, the
        # ranges clipped to it and relative to it (a cell of the run that holds none is empty there and is not written)
        pabs, pcuts, n_cell = state.get("phase_abs"), {}, 0
        if pabs is not None:
            for a in range(0, s_count, sub):
                lo, hi = t_offset + a, t_offset + min(s_count, a + sub)
                hit = np.flatnonzero((np.minimum(pabs[:, 1], hi) > np.maximum(pabs[:, 0], lo)))
                if hit.size:
                    c0, c1 = int(hit[0]), int(hit[-1]) + 1
                    pcuts[a] = (c0, c1, n_cell, np.ascontiguousarray(np.clip(pabs[c0:c1], lo, hi) - lo, dtype=np.int32))
                    n_cell += c1 - c0
        tabs = torch.as_tensor(np.concatenate([c[3] for c in cuts.values()] + [c[3].ravel() for c in pcuts.values()])).to(rows.device)
        seg_dev, range_dev = tabs[:n_off], tabs[n_off:].view(-1, 2)

        def issue(a, b, shared):
            g0, g1, off, seg_host = cuts[a]
            shared = {k: x for k, x in shared.items() if k not in ("t_begin", "t_count", "mapsum_d")}
            ca = _lib.CompositeStepsArgs(
                s_count=b - a, nyb=state["nyb"], nxb=state["nxb"], n_seg=g1 - g0, step_h=C.c_void_p(step_host[a:b].ctypes.data),
                step_d=_ptr(steps[a:b]), seg_h=C.c_void_p(seg_host.ctypes.data), seg_d=_ptr(seg_dev[off: off + g1 - g0 + 1]),
                box_h=C.c_void_p(box_host[a:b].ctypes.data), box_d=_ptr(dev["box"][a:b]), boxtab_d=_ptr(dev["boxtab"][a:b]),
                lattab_d=_ptr(dev["lattab"][a:b]), lattab2_d=_ptr(dev["lattab2"][a:b]), tcoef_d=_ptr(tcoef[a:b]),
                mapsum_d=_ptr(state["mapsum"][g0:]), **shared)
            _lib.check(self.lib.lec_composite_steps(C.byref(ca)), "lec_composite_steps")
            if a in pcuts:      # the cells' sums from the columns this sub-call wrote, on its stream
                c0, c1, off, range_host = pcuts[a]
                pa = _lib.CompositePhaseSumArgs(
                    col_d=shared["col_d"], range_h=C.c_void_p(range_host.ctypes.data), range_d=_ptr(range_dev[off: off + c1 - c0]),
                    phasesum_d=_ptr(state["phasesum"].view(-1, _lib.LEC_NMAP, state["nyb"], state["nxb"])[c0:]), s_count=b - a,
                    nyb=state["nyb"], nxb=state["nxb"], n_cell=c1 - c0, reserved0=0, stream=shared["stream"])
                _lib.check(self.lib.lec_composite_phase_sum(C.byref(pa)), "lec_composite_phase_sum")
        self._mapcol_stage((tair, u, v, omega), rows, levraw, state, t_offset, 0, issue)

    def batch_composite_finish(self, res: LECResult, state: dict) -> None:
        """``res.batch_composite_*`` from the accumulators of a finished batch: ``lec_composite_ensemble`` turns the time sums into the
        tracks' means (in place) and forms their ensemble mean."""
        ms = state["mapsum"]
        counts, counts_dev = state["sizes"], state["sizes_dev"]
        ens = torch.empty(tuple(ms.shape[1:]), dtype=torch.float64, device=ms.device)
        ea = _lib.CompositeEnsembleArgs(mapsum_d=_ptr(ms), count_h=C.c_void_p(counts.ctypes.data), count_d=_ptr(counts_dev),
                                        n_track=int(ms.shape[0]), nyb=state["nyb"], nxb=state["nxb"], reserved0=0, mean_d=_ptr(ms),
                                        ens_d=_ptr(ens), stream=C.c_void_p(torch.cuda.current_stream(ms.device).cuda_stream))
        with torch.cuda.device(ms.device):
            _lib.check(self.lib.lec_composite_ensemble(C.byref(ea)), "lec_composite_ensemble")
        res.batch_composite_mean = ms
        res.batch_composite_ensemble = ens
        res.batch_composite_lon = state["hov"]
        if state["steps"] is not None:
            res.batch_composite_steps = state["steps"]
        if "phasesum" in state:
            ps, cnt = state["phasesum"], state["phase_count"]
            f64 = dict(dtype=torch.float64, device=ps.device)
            pens, spread = torch.empty(tuple(ps.shape[1:]), **f64), torch.empty(tuple(ps.shape[1:]), **f64)
            pe = _lib.CompositePhaseEnsembleArgs(
                phasesum_d=_ptr(ps), count_h=C.c_void_p(cnt.ctypes.data), count_d=_ptr(state["phase_count_dev"]), n_track=int(ps.shape[0]),
                n_bin=int(ps.shape[1]), nyb=state["nyb"], nxb=state["nxb"], reserved0=0, mean_d=_ptr(ps), ens_d=_ptr(pens),
                spread_d=_ptr(spread), stream=C.c_void_p(torch.cuda.current_stream(ps.device).cuda_stream))
            with torch.cuda.device(ps.device):
                _lib.check(self.lib.lec_composite_phase_ensemble(C.byref(pe)), "lec_composite_phase_ensemble")
            res.batch_phase_mean, res.batch_phase_ensemble, res.batch_phase_spread = ps, pens, spread
            res.batch_phase_count = cnt.copy()
            res.batch_phase_members = (cnt >= 1).sum(axis=0).astype(np.int32)

    # -- zonal-wavenumber spectra on a ring ----------------------------------------------------------------------------------------
    # assembled row records (N wavenumbers x a chunk of time steps) resident at once; the fused form: the chunk's spectral records
    SPECTRUM_CHUNK_BYTES = 256 << 20

    @staticmethod
    def _check_wavenumbers(wavenumbers, boxes, nx: int) -> None:
        if not isinstance(boxes, PreparedBoxes) or not boxes.bt.ring:
            raise ValueError("wavenumbers: a zonal-wavenumber spectrum exists on a ring only: boxes from prepare_boxes(..., ring=True)")
        if boxes.bt.nyb_max != boxes.boxes[0][3] - boxes.boxes[0][2] + 1:
            raise ValueError("wavenumbers: the ring's records must have the band's own row count (prepare_boxes without nyb_min)")
        if isinstance(wavenumbers, bool) or not isinstance(wavenumbers, (int, np.integer)):
            raise ValueError("wavenumbers must be an integer")
        if wavenumbers < 1 or wavenumbers > nx // 2:
            raise ValueError(f"wavenumbers must be 1 .. nx / 2 = {nx // 2} (a ring of {nx} columns holds no others), got {wavenumbers}")
        if wavenumbers > _lib.LEC_MAX_WAVENUMBERS:
            raise ValueError(f"wavenumbers must be at most {_lib.LEC_MAX_WAVENUMBERS} (LEC_MAX_WAVENUMBERS), got {wavenumbers}")

    def rowspec(self, tair: torch.Tensor, u: torch.Tensor, v: torch.Tensor, omega: torch.Tensor, boxes: PreparedBoxes, wavenumbers: int, *,
                t_begin: int = 0, t_count: Optional[int] = None, spec_out: Optional[torch.Tensor] = None,
                timing: Optional[list] = None) -> torch.Tensor:
        """``lec_rowspec_ring``: [t_count, nl, nyb, N, 8] fp64, the shares of the zonal wavenumbers 1 .. N in the eight eddy covariances
        (slots 6 .. 13 of a row record, in that order) of every row of the ring's latitude band, for time steps
        [t_begin, t_begin + t_count) of the cubes.  ``boxes`` from ``prepare_boxes(..., ring=True)``; ``spec_out``: a caller-owned
        buffer; ``timing``: a list that receives one (start, end) pair of HIP events around the launch."""
        return self._rowspec_call("lec_rowspec_ring", _lib.RowspecArgs, (tair, u, v, omega), boxes, wavenumbers, t_begin, t_count, (),
                                  [("spec_d", "spec_out", spec_out, ("N", 8))], None, timing)[0]

    def _rowspec_call(self, call: str, args_type, cubes, boxes: PreparedBoxes, wavenumbers, t_begin: int, t_count: Optional[int], rows: tuple,
                      outs: list, own, timing: Optional[list]) -> list:
        """What ``rowspec``, ``rowspec_q``, ``rowspec_nl`` and ``rowspec_b`` share, in the order their checks have always come: the
        field and wavenumber checks, the ``t_count`` default, the band, ``own(nt, js, jn)`` -- the call's own checks and tables, returned
        as its own fields of ``args_type`` --, the ``rows`` check (``rows``: ``()`` for a call that takes none, or ``(rows,)``), the
        outputs ``outs`` -- (field, argument name, the caller's buffer or None, the shape after [t_count, nl, nyb] with "N" for the
        wavenumbers) each --, the twiddle table and the call itself between a pair of events for ``timing``.  Returns the outputs."""
        tair = cubes[0]
        self._check_fields(list(cubes), None)
        nt, nl, ny, nx = (int(x) for x in tair.shape)
        self._check_wavenumbers(wavenumbers, boxes, nx)
        n = int(wavenumbers)
        if t_count is None:
            t_count = nt - t_begin
        _, _, js, jn = boxes.boxes[0]
        nyb = jn - js + 1
        fields = own(nt, js, jn) if own is not None else {}
        for r in rows:
            if (r.shape != (t_count, nl, nyb, _lib.LEC_NSTAT) or r.dtype != torch.float64 or r.device != tair.device
                    or not r.is_contiguous()):
                raise ValueError("rows must be a contiguous fp64 [t_count, nl, nyb, 32] tensor on the fields' device: the ring pass's records of the same steps")
            fields["rows_d"] = _ptr(r)
        tensors = []
        for field, name, given, tail in outs:
            shape = (t_count, nl, nyb) + tuple(n if d == "N" else d for d in tail)
            out = torch.empty(shape, dtype=torch.float64, device=tair.device) if given is None else given
            if out.shape != shape or out.dtype != torch.float64 or out.device != tair.device or not out.is_contiguous():
                raise ValueError(f"{name} must be a contiguous fp64 [t_count, nl, nyb, {', '.join(str(d) for d in tail)}] tensor on the fields' device")
            fields[field] = _ptr(out)
            tensors.append(out)
        if self._twid is None:
            self._twid = self._up(tables.twiddle_table(nx))
        args = args_type(
            tair_d=_ptr(cubes[0]), u_d=_ptr(cubes[1]), v_d=_ptr(cubes[2]), omega_d=_ptr(cubes[3]),
            dtype=_lib.LEC_F64 if tair.dtype == torch.float64 else _lib.LEC_F32,
            nt=nt, nl=nl, ny=ny, nx=nx, t_begin=t_begin, t_count=t_count, js=js, jn=jn, n_wave=n, twid_d=_ptr(self._twid),
            stream=C.c_void_p(torch.cuda.current_stream(tair.device).cuda_stream), **fields)
        with torch.cuda.device(tair.device):
            if timing is not None:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
            _lib.check(getattr(self.lib, call)(C.byref(args)), call)
            if timing is not None:
                ev1.record()
                timing.append((ev0, ev1))
        return tensors

    def _cube_tcoef(self, who: str, time_s, tcoef: Optional[torch.Tensor], nt: int, device) -> torch.Tensor:
        """The d/dt coefficients [nt, 3] of a cube's time axis on the device: ``tcoef`` checked, or built from ``time_s`` (seconds, one
        entry per step of the cube) and kept for the next call on the same axis -- for the calls that form Q at every point."""
        if tcoef is None:
            if time_s is None:
                raise ValueError(f"{who} needs time_s (seconds) or tcoef: Q holds dT/dt over the cube's time axis")
            time_s = np.asarray(time_s, dtype=np.float64)
            if time_s.size != nt:
                raise ValueError("time_s must have one entry per time step of the cube")
            if nt < 2:
                raise ValueError("dT/dt by finite differences needs at least 2 time steps")
            if self._tcoef is None or self._tcoef[0].shape != time_s.shape or not np.array_equal(self._tcoef[0], time_s):
                self._tcoef = (time_s.copy(), self._up(tables.time_coefs(time_s)))
            return self._tcoef[1]
        if tcoef.shape != (nt, 3) or tcoef.dtype != torch.float64 or tcoef.device != device or not tcoef.is_contiguous():
            raise ValueError("tcoef must be a contiguous fp64 [nt, 3] tensor on the fields' device")
        return tcoef

    def rowspec_q(self, tair: torch.Tensor, u: torch.Tensor, v: torch.Tensor, omega: torch.Tensor, boxes: PreparedBoxes, wavenumbers: int, *,
                  time_s=None, tcoef: Optional[torch.Tensor] = None, t_begin: int = 0, t_count: Optional[int] = None,
                  out: Optional[torch.Tensor] = None, timing: Optional[list] = None) -> torch.Tensor:
        """``lec_rowspec_q_ring``: [t_count, nl, nyb, N] fp64, the shares C_n(Q, T) of the zonal wavenumbers 1 .. N in [Q'T'] (slot 15 of
        a row record) of every row of the ring's latitude band, for time steps [t_begin, t_begin + t_count) of the cubes.  Q is the ring
        pass's, with dT/dt over the cube's time axis ``time_s`` (seconds, one entry per step of the cube; or ``tcoef``, its d/dt
        coefficients already on the device); the tables are the prepared ring box's and the engine's own.  ``out``: a caller-owned
        buffer; ``timing``: a list that receives one (start, end) pair of HIP events around the launch."""
        def own(nt, js, jn):
            return dict(lattab_d=_ptr(boxes.dev["lattab"]), levtab_d=_ptr(self._levtab), inv_hdeg=float(boxes.bt.boxtab[0, 2]),
                        tcoef_d=_ptr(self._cube_tcoef("rowspec_q", time_s, tcoef, nt, tair.device)))
        return self._rowspec_call("lec_rowspec_q_ring", _lib.RowspecQArgs, (tair, u, v, omega), boxes, wavenumbers, t_begin, t_count, (),
                                  [("qspec_d", "out", out, ("N",))], own, timing)[0]

    def rowspec_nl(self, tair: torch.Tensor, u: torch.Tensor, v: torch.Tensor, omega: torch.Tensor, rows: torch.Tensor, boxes: PreparedBoxes,
                   n: int, *, t_begin: int = 0, t_count: Optional[int] = None, out: Optional[torch.Tensor] = None,
                   out_total: Optional[torch.Tensor] = None, timing: Optional[list] = None):
        """``lec_rowspec_nl_ring``: (nlspec [t_count, nl, nyb, N, 8], nltot [t_count, nl, nyb, 8]) fp64 -- slots 0, 1, 2 hold
        -2 C_n(A_T, T), -2 C_n(A_u, u), -2 C_n(A_v, v) of the eddy-eddy advective tendencies A_x of every row of the ring's latitude band,
        for the wavenumbers 1 .. N and for the whole eddy covariance, slots 3 .. 7 are 0: ``spectrum_level_stage`` takes either as
        ``spec``.  ``rows`` [t_count, nl, nyb, 32]: the ring pass's records of the same steps [t_begin, t_begin + t_count) (their zonal
        means are the eddies' reference).  ``out`` / ``out_total``: caller-owned buffers; ``timing``: as ``rowspec``."""
        def own(nt, js, jn):
            if self._ptab is None:
                self._ptab = self._up(tables.pressure_coefs(self.level))
            if "nl_lattab" not in boxes.dev:
                boxes.dev["nl_lattab"] = self._up(tables.nl_lat_table(boxes.bt.lattab[0], self.lat[js:jn + 1]))
            return dict(lattab_d=_ptr(boxes.dev["nl_lattab"]), ptab_d=_ptr(self._ptab), inv_hdeg=float(boxes.bt.boxtab[0, 2]))
        nlspec, nltot = self._rowspec_call("lec_rowspec_nl_ring", _lib.RowspecNlArgs, (tair, u, v, omega), boxes, n, t_begin, t_count, (rows,),
                                           [("nlspec_d", "out", out, ("N", 8)), ("nltot_d", "out_total", out_total, (8,))], own, timing)
        return nlspec, nltot

    def rowspec_b(self, tair: torch.Tensor, u: torch.Tensor, v: torch.Tensor, omega: torch.Tensor, rows: torch.Tensor, boxes: PreparedBoxes,
                  n: int, *, t_begin: int = 0, t_count: Optional[int] = None, out: Optional[torch.Tensor] = None,
                  timing: Optional[list] = None) -> torch.Tensor:
        """``lec_rowspec_b_ring``: bspec [t_count, nl, nyb, N, 4] fp64 -- the shares VTT(n), WTT(n), EV(n), EW(n) of the wavenumbers
        1 .. N in slots 16, 17, 20, 21 of every row record of the ring's latitude band (the triple products behind BAe and BKe); VTT and
        EV at the band's first and last row only, 0 elsewhere.  ``rows`` [t_count, nl, nyb, 32]: the ring pass's records of the same
        steps [t_begin, t_begin + t_count).  ``out``: a caller-owned buffer; ``timing``: as ``rowspec``.  One call per time chunk: the
        callers keep ``out`` within ``SPECTRUM_CHUNK_BYTES`` (``spectrum_chunk_steps``)."""
        return self._rowspec_call("lec_rowspec_b_ring", _lib.RowspecBArgs, (tair, u, v, omega), boxes, n, t_begin, t_count, (rows,),
                                  [("bspec_d", "out", out, ("N", 4))], None, timing)[0]

    def spectrum_budget_terms(self, res: LECResult, time_s) -> None:
        """``res.spectrum_tendency*`` and ``res.spectrum_residual*`` from ``res.spectrum*`` and ``res.spectrum_b*`` of a whole series
        (host arithmetic on [time, N] arrays by ``tables.spectrum_budgets``); ``time_s``: the run's time axis in seconds."""
        if res.spectrum is None or res.spectrum_b is None:
            raise ValueError("spectrum_budget_terms: a result of compute(..., wavenumbers=N, spectrum_budget=True)")
        dev = res.spectrum.device
        host = lambda x: x.cpu().numpy()
        b = tables.spectrum_budgets(host(res.spectrum), host(res.spectrum_rest), host(res.spectrum_b), host(res.spectrum_b_rest), time_s)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        res.spectrum_tendency, res.spectrum_tendency_rest = up(b["tendency"]), up(b["tendency_rest"])
        res.spectrum_residual, res.spectrum_residual_rest = up(b["residual"]), up(b["residual_rest"])

    def spectrum_nl_chunk_steps(self, t_count: int, nl: int, nyb: int, n: int) -> int:
        """Time steps per ``rowspec_nl`` call: the chunk's records ([tc, nl, nyb, N + 1, 8] fp64, shares and total) stay within
        ``SPECTRUM_CHUNK_BYTES``."""
        return max(1, min(int(t_count), self.SPECTRUM_CHUNK_BYTES // (nl * nyb * (n + 1) * 64)))

    def spectrum_nl_stage(self, tair, u, v, omega, rows: torch.Tensor, boxes: PreparedBoxes, n: int, levraw_nl: torch.Tensor, *,
                          t_begin: int = 0, phi_scale: float = 1.0, buffers=None) -> None:
        """``rowspec_nl`` and the level x latitude half of stage 2 for the steps [t_begin, t_begin + rows.shape[0]) of the cubes, in chunks
        of ``spectrum_nl_chunk_steps``: ``levraw_nl`` [N + 1, t_count, nl, 40] (a time slice of the series' buffer) receives the records
        of the N shares and, at index N, of the total.  ``buffers``: (nlspec, nltot) of at least one chunk, to be reused between calls."""
        t_count, nl, nyb = (int(x) for x in rows.shape[:3])
        tc = self.spectrum_nl_chunk_steps(t_count, nl, nyb, n)
        if buffers is None:
            f64 = dict(dtype=torch.float64, device=rows.device)
            buffers = (torch.empty((tc, nl, nyb, n, 8), **f64), torch.empty((tc, nl, nyb, 8), **f64))
        tc = min(tc, int(buffers[0].shape[0]))
        for a in range(0, t_count, tc):
            b = min(a + tc, t_count)
            ns, ntot = self.rowspec_nl(tair, u, v, omega, rows[a:b], boxes, n, t_begin=t_begin + a, t_count=b - a,
                                       out=buffers[0][:b - a], out_total=buffers[1][:b - a])
            self.spectrum_level_stage(rows[a:b], ns, None, boxes, levraw_nl[:n, a:b], phi_scale=phi_scale)
            self.spectrum_level_stage(rows[a:b], ntot.unsqueeze(3), None, boxes, levraw_nl[n:, a:b], phi_scale=phi_scale)

    def _spectrum_nl_shares(self, res: LECResult, levraw_nl: torch.Tensor, boxes, drop_any_time: Optional[bool]) -> None:
        """The tail of the interactions: ``levraw_nl`` [N + 1, t_count, nl, 40] -> ONE vertical half over the (n, step) batch (_handle_nans
        sees the shares and the total together: they are NaN at the same levels) and ``res.spectrum_nl*``: S from the Ae place, L from the
        Ke place of stage 2; the other places of these records mean nothing and are ignored."""
        n1, t_count, nl = (int(x) for x in levraw_nl.shape[:3])
        n = n1 - 1
        shares = self.vertical_stage(levraw_nl.view(n1 * t_count, nl, _lib.LEC_NLEVRAW), boxes, drop_any_time=drop_any_time)
        si = torch.as_tensor([SCALAR_TERMS.index(x) for x in SPECTRUM_INTERACTION_PLACES], device=levraw_nl.device)
        li = torch.as_tensor([LEVEL_TERMS.index(x) for x in SPECTRUM_INTERACTION_PLACES], device=levraw_nl.device)
        sc = shares.scalars.reshape(n1, t_count, _lib.LEC_NSCALAR)[:, :, si]
        res.spectrum_nl = sc[:n].permute(1, 2, 0).contiguous()
        res.spectrum_nl_total = sc[n].contiguous()
        res.spectrum_nl_rest = res.spectrum_nl_total - res.spectrum_nl.sum(dim=2)
        res.spectrum_nl_levels = shares.levels.reshape(n1, t_count, _lib.LEC_NLEVTAB, nl)[:n][:, :, li].permute(1, 2, 0, 3).contiguous()

    def spectrum_chunk_steps(self, t_count: int, nl: int, nyb: int, n: int, budget: bool = False) -> int:
        """Time steps per spectral call of the fused form: the chunk's ``spec`` records ([tc, nl, nyb, N, 8] fp64) -- with ``budget``
        together with ``rowspec_b``'s ([tc, nl, nyb, N, 4]) -- stay within ``SPECTRUM_CHUNK_BYTES``."""
        return max(1, min(int(t_count), self.SPECTRUM_CHUNK_BYTES // (nl * nyb * n * (96 if budget else 64))))

    def spectrum_level_stage(self, rows: torch.Tensor, spec: torch.Tensor, qspec: Optional[torch.Tensor], boxes, levraw_out: torch.Tensor, *,
                             phi_scale: float = 1.0, bspec: Optional[torch.Tensor] = None) -> None:
        """``lec_level_spec_ring``: rows [t_count, nl, nyb, 32], ``spec`` [t_count, nl, nyb, N, 8] (``rowspec``) and ``qspec``
        [t_count, nl, nyb, N] (``rowspec_q``) or None -> ``levraw_out`` [N, t_count, nl, 40]: what ``level_stage`` gives on the row
        records that carry wavenumber n's shares in slots 6 .. 13 (and 15), for every n, without those records being assembled.
        ``levraw_out`` may be a time slice of a larger [N, T, nl, 40] tensor (contiguous in its last two dimensions).  ``bspec``
        [t_count, nl, nyb, N, 4] (``rowspec_b``): ``lec_level_spec_b_ring``, slots 16, 17, 20, 21 replaced too."""
        t_count, nl = int(rows.shape[0]), int(rows.shape[1])
        boxes, bt, dev = self._stage2_input(rows, boxes)
        if len(boxes) != 1 or not bt.ring:
            raise ValueError("spectrum_level_stage: one ring box (prepare_boxes(..., ring=True))")
        nyb = bt.nyb_max
        if (spec.dim() != 5 or spec.shape[:3] != (t_count, nl, nyb) or spec.shape[4] != 8 or spec.dtype != torch.float64
                or spec.device != rows.device or not spec.is_contiguous()):
            raise ValueError("spec must be a contiguous fp64 [t_count, nl, nyb, N, 8] tensor on the rows' device")
        n = int(spec.shape[3])
        if qspec is not None and (qspec.shape != (t_count, nl, nyb, n) or qspec.dtype != torch.float64 or qspec.device != rows.device
                                  or not qspec.is_contiguous()):
            raise ValueError("qspec must be a contiguous fp64 [t_count, nl, nyb, N] tensor on the rows' device")
        if bspec is not None and (bspec.shape != (t_count, nl, nyb, n, 4) or bspec.dtype != torch.float64 or bspec.device != rows.device
                                  or not bspec.is_contiguous()):
            raise ValueError("bspec must be a contiguous fp64 [t_count, nl, nyb, N, 4] tensor on the rows' device")
        step = nl * _lib.LEC_NLEVRAW
        if (levraw_out.shape != (n, t_count, nl, _lib.LEC_NLEVRAW) or levraw_out.dtype != torch.float64 or levraw_out.device != rows.device
                or tuple(levraw_out.stride()[2:]) != (_lib.LEC_NLEVRAW, 1) or (t_count > 1 and levraw_out.stride(1) != step)
                or (n > 1 and levraw_out.stride(0) < t_count * step)):
            raise ValueError("levraw_out must be an fp64 [N, t_count, nl, 40] tensor on the rows' device, contiguous in its last two "
                             "dimensions (a time slice of an [N, T, nl, 40] tensor)")
        am = self._workspace(t_count, nl, rows.device, am_only=True)
        la = _lib.LevelSpecArgs(
            rows_d=_ptr(rows), spec_d=_ptr(spec), qspec_d=_ptr(qspec), t_count=t_count, nl=nl, nyb=nyb, n_wave=n,
            box_d=_ptr(dev["box"]), lattab2_d=_ptr(dev["lattab2"]), levtab2_d=_ptr(self._levtab2), phi_scale=float(phi_scale),
            am_d=_ptr(am), levraw_d=_ptr(levraw_out), wave_stride=int(levraw_out.stride(0)) if n > 1 else 0,
            stream=C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream))
        with torch.cuda.device(rows.device):
            if bspec is not None:
                lb = _lib.LevelSpecBArgs(spec=la, bspec_d=_ptr(bspec))
                _lib.check(self.lib.lec_level_spec_b_ring(C.byref(lb)), "lec_level_spec_b_ring")
            else:
                _lib.check(self.lib.lec_level_spec_ring(C.byref(la)), "lec_level_spec_ring")

    def _spectrum(self, res: LECResult, rows: torch.Tensor, tair, u, v, omega, boxes: PreparedBoxes, n: int, t_begin: int, phi_scale: float,
                  drop_any_time: Optional[bool], generation: Optional[dict] = None, fused: bool = False, interactions: bool = False,
                  budget: bool = False, sections: Optional[dict] = None) -> None:
        """Fills ``res.spectrum*``.  X(n) is what stage 2 gives for X on row records whose slots 6 .. 13 hold the wavenumber-n shares and
        whose other entries are the ring pass's: the records are assembled for a chunk of time steps and all N wavenumbers at a time
        (at most ``SPECTRUM_CHUNK_BYTES``), the level x latitude half of ``lec_reduce`` turns each chunk into 40 numbers per (n, step,
        level), and ONE vertical half over all (n, step) applies _handle_nans: a share is NaN exactly where its total is, so the
        any-time mask over the batch is the totals' own.  ``generation`` ({"time_s", "tcoef"} of the call): slot 15 of the assembled
        records holds the wavenumber's share of [Q'T'] too (``rowspec_q``), which only Ge reads: Ge(n) and its table come out of the
        same batch, and nothing else of it moves.  ``fused``: no assembled records -- ``spectrum_level_stage`` reads the ring
        pass's records and the chunk's ``spec`` / ``qspec`` (the chunk is bounded by ``spec``), the same bits.  ``interactions``: S(n)
        and L(n) by ``spectrum_nl_stage`` in time chunks of its own records, a batch of its own.  ``budget``: slots 16, 17, 20, 21 of
        the same records hold ``rowspec_b``'s shares, which only the BAe and BKe columns read: BAe(n) and BKe(n) come out of the same
        batch, and nothing else of it moves.  ``sections`` (the state of ``section_begin``, with the totals' levraw under "levraw"):
        every chunk's ``spec`` / ``qspec`` also go through ``section_stage``."""
        t_count, nl, nyb = (int(x) for x in rows.shape[:3])
        dev = rows.device
        f64 = dict(dtype=torch.float64, device=dev)
        if interactions:
            levraw_nl = torch.empty((n + 1, t_count, nl, _lib.LEC_NLEVRAW), **f64)
            self.spectrum_nl_stage(tair, u, v, omega, rows, boxes, n, levraw_nl, t_begin=t_begin, phi_scale=phi_scale)
            self._spectrum_nl_shares(res, levraw_nl, boxes, drop_any_time)
        levraw = torch.empty((n, t_count, nl, _lib.LEC_NLEVRAW), **f64)
        if fused:
            tc = self.spectrum_chunk_steps(t_count, nl, nyb, n, budget)
            spec = torch.empty((tc, nl, nyb, n, 8), **f64)
            qspec = torch.empty((tc, nl, nyb, n), **f64) if generation is not None else None
            bspec = torch.empty((tc, nl, nyb, n, 4), **f64) if budget else None
            for a in range(0, t_count, tc):
                b = min(a + tc, t_count)
                sp = self.rowspec(tair, u, v, omega, boxes, n, t_begin=t_begin + a, t_count=b - a, spec_out=spec[:b - a])
                qs = None
                if generation is not None:
                    qs = self.rowspec_q(tair, u, v, omega, boxes, n, t_begin=t_begin + a, t_count=b - a, out=qspec[:b - a], **generation)
                bs = None
                if budget:
                    bs = self.rowspec_b(tair, u, v, omega, rows[a:b], boxes, n, t_begin=t_begin + a, t_count=b - a, out=bspec[:b - a])
                self.spectrum_level_stage(rows[a:b], sp, qs, boxes, levraw[:, a:b], phi_scale=phi_scale, bspec=bs)
                if sections is not None:
                    self.section_stage(rows[a:b], boxes, sections["levraw"][a:b], sections, a, spec=sp, qspec=qs)
            self._spectrum_shares(res, levraw, boxes, drop_any_time, generation is not None, budget)
            return
        tc = max(1, min(t_count, self.SPECTRUM_CHUNK_BYTES // (n * nl * nyb * _lib.LEC_NSTAT * 8)))
        asm = torch.empty((n, tc, nl, nyb, _lib.LEC_NSTAT), **f64)
        spec = torch.empty((tc, nl, nyb, n, 8), **f64)
        qspec = torch.empty((tc, nl, nyb, n), **f64) if generation is not None else None
        bspec = torch.empty((tc, nl, nyb, n, 4), **f64) if budget else None
        part = torch.empty((n, tc, nl, _lib.LEC_NLEVRAW), **f64)
        for a in range(0, t_count, tc):
            b = min(a + tc, t_count)
            c = b - a
            sp = self.rowspec(tair, u, v, omega, boxes, n, t_begin=t_begin + a, t_count=c, spec_out=spec[:c])
            rec = asm[:, :c]
            rec.copy_(rows[a:b].unsqueeze(0))
            rec[..., _LEC_S_TT:_LEC_S_TT + 8] = sp.permute(3, 0, 1, 2, 4)
            if generation is not None:
                qs = self.rowspec_q(tair, u, v, omega, boxes, n, t_begin=t_begin + a, t_count=c, out=qspec[:c], **generation)
                rec[..., _LEC_S_QT] = qs.permute(3, 0, 1, 2)
            if sections is not None:
                self.section_stage(rows[a:b], boxes, sections["levraw"][a:b], sections, a, spec=sp, qspec=qs if generation is not None else None)
            if budget:
                bs = self.rowspec_b(tair, u, v, omega, rows[a:b], boxes, n, t_begin=t_begin + a, t_count=c, out=bspec[:c]).permute(3, 0, 1, 2, 4)
                rec.index_copy_(4, torch.as_tensor(_LEC_S_BUDGET, device=dev), bs)
            if c == tc:
                self.level_stage(rec.reshape(n * c, nl, nyb, _lib.LEC_NSTAT), boxes, part.view(n * c, nl, _lib.LEC_NLEVRAW), phi_scale=phi_scale)
                levraw[:, a:b] = part
            else:                       # the last, shorter chunk: a contiguous batch of its own
                last = torch.empty((n * c, nl, _lib.LEC_NLEVRAW), **f64)
                self.level_stage(rec.contiguous().view(n * c, nl, nyb, _lib.LEC_NSTAT), boxes, last, phi_scale=phi_scale)
                levraw[:, a:b] = last.view(n, c, nl, _lib.LEC_NLEVRAW)
        self._spectrum_shares(res, levraw, boxes, drop_any_time, generation is not None, budget)

    def _spectrum_shares(self, res: LECResult, levraw: torch.Tensor, boxes, drop_any_time: Optional[bool], generation: bool,
                         budget: bool = False) -> None:
        """The tail of the spectra: ``levraw`` [N, t_count, nl, 40] of all wavenumbers and steps -> ONE vertical half over the (n, step)
        batch and ``res.spectrum*`` (``res`` holds the totals)."""
        n, t_count, nl = (int(x) for x in levraw.shape[:3])
        dev = levraw.device
        shares = self.vertical_stage(levraw.view(n * t_count, nl, _lib.LEC_NLEVRAW), boxes, drop_any_time=drop_any_time)
        si = torch.as_tensor([SCALAR_TERMS.index(x) for x in SPECTRUM_TERMS], device=dev)
        li = torch.as_tensor([LEVEL_TERMS.index(x) for x in SPECTRUM_LEVEL_TERMS], device=dev)
        res.spectrum = shares.scalars.reshape(n, t_count, _lib.LEC_NSCALAR)[:, :, si].permute(1, 2, 0).contiguous()
        res.spectrum_levels = shares.levels.reshape(n, t_count, _lib.LEC_NLEVTAB, nl)[:, :, li].permute(1, 2, 0, 3).contiguous()
        res.spectrum_rest = res.scalars[:, si] - res.spectrum.sum(dim=2)
        if generation:
            ge, gl = SCALAR_TERMS.index(SPECTRUM_GENERATION_TERM), LEVEL_TERMS.index(SPECTRUM_GENERATION_TERM)
            res.spectrum_ge = shares.scalars.reshape(n, t_count, _lib.LEC_NSCALAR)[:, :, ge].permute(1, 0).contiguous()
            res.spectrum_ge_levels = shares.levels.reshape(n, t_count, _lib.LEC_NLEVTAB, nl)[:, :, gl].permute(1, 0, 2).contiguous()
            res.spectrum_ge_rest = res.scalars[:, ge] - res.spectrum_ge.sum(dim=1)
        if budget:
            bi = torch.as_tensor([SCALAR_TERMS.index(x) for x in SPECTRUM_BUDGET_TERMS], device=dev)
            res.spectrum_b = shares.scalars.reshape(n, t_count, _lib.LEC_NSCALAR)[:, :, bi].permute(1, 2, 0).contiguous()
            res.spectrum_b_rest = res.scalars[:, bi] - res.spectrum_b.sum(dim=2)

    def rowstats(self, tair: torch.Tensor, u: torch.Tensor, v: torch.Tensor, omega: torch.Tensor,
                 geopt: Optional[torch.Tensor], boxes: Sequence[Sequence[int]], *,
                 time_s=None, dTdt: Optional[torch.Tensor] = None, t_begin: int = 0,
                 t_count: Optional[int] = None, with_q: bool = True, timing: Optional[list] = None,
                 rows_out: Optional[torch.Tensor] = None, tuning: Optional[dict] = None,
                 per_step_boxes: Optional[bool] = None, tcoef: Optional[torch.Tensor] = None,
                 tm: Optional[torch.Tensor] = None, tp: Optional[torch.Tensor] = None,
                 steps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Stage 1: row records [t_count, nl, nyb_max, 32] of time steps [t_begin, t_begin + t_count) of the cubes.  Three kinds of call
        share one path (a fourth is the first with ``boxes`` from ``prepare_boxes(..., ring=True)``: ``lec_rowstats_ring``):

        * whole cubes on the engine's grid (``lec_rowstats``), dT/dt from ``time_s`` / ``tcoef`` or a ``dTdt`` cube;
        * a BOX-PACKED series (``pack_boxes``; ``boxes`` prepared with ``packed=True``): the cubes hold every step's box at the origin
          of its slab, with dT/dt as ``packed_dtdt`` hands it over -- a ``dTdt`` cube, or ``tm`` / ``tp`` (T of the previous / next
          step on that box) with ``tcoef``.  The records of the whole cubes, bit for bit;
        * ``steps``: the boxes of SEVERAL tracks over one cube on the engine's grid (``lec_rowstats_steps``): int32 [S, 3] on the
          device, one row per box = {cube step, previous step, next step} of the box's own track (the step itself at the track's
          ends), with ``tcoef`` fp64 [S, 3] by box and S boxes; ``t_begin`` 0, no ``dTdt`` / ``tm`` / ``tp``.  The records of every box
          are those of its track's own cube, bit for bit.  The table is checked on the host (``check_steps``) before anything is
          launched.

        ``tuning``: see ``make_tuning`` (kernel family / order / tile shape; default = the library's choice).
        ``tcoef`` (cubes, packed series): the d/dt coefficients of the cube's time steps already on the device (fp64 [nt, 3], e.g. rows
        [h0, h1) of ``time_coefs_device`` of the whole series) instead of ``time_s`` -- a chunk loop then uploads nothing per call (an
        upload from pageable memory makes the host wait for the stream, which serialises a copy / compute pipeline).
        ``rows_out``: a caller-owned record buffer (e.g. a slice of a longer series' one; its row count may exceed this call's boxes).
        A call is cut into launches of at most ``MAX_STEPS_PER_LAUNCH`` steps (boxes of a step table): some kernel families address
        their time steps with 16-bit grid coordinates.  Same kernels, same bits: results do not depend on how a series is cut.
        ``timing``: a list that receives one (start, end) pair of HIP events per launch, recorded on the launch stream."""
        if steps is not None and (dTdt is not None or tm is not None or tp is not None or not with_q or t_begin != 0 or per_step_boxes is False):
            raise ValueError("steps: dT/dt from the cube's own steps (no dTdt / tm / tp), with_q, t_begin = 0, per-step boxes")
        packed = steps is None and (tm is not None or tp is not None or (isinstance(boxes, PreparedBoxes) and "box_data" in boxes.dev))
        if packed and (not isinstance(boxes, PreparedBoxes) or "box_data" not in boxes.dev or (with_q and (dTdt is None) == (tm is None or tp is None))):
            raise ValueError("a box-packed series: boxes from prepare_boxes(..., packed=True) and, with_q, either tm and tp or a dTdt cube")
        self._check_fields([tair, u, v, omega] + [c for c in (geopt, dTdt, tm, tp) if c is not None], boxes if packed else None)
        nt, nl, ny, nx = (int(x) for x in tair.shape)

        if steps is not None:
            n = self.check_steps(steps, tcoef, nt, tair.device)
            if t_count is not None and t_count != n:
                raise ValueError("steps: t_count must equal the number of table rows")
            t_count, per_step_boxes = n, True
        else:
            if t_count is None:
                t_count = nt - t_begin
            if tcoef is not None:
                if tcoef.shape != (nt, 3) or tcoef.dtype != torch.float64 or tcoef.device != tair.device or not tcoef.is_contiguous():
                    raise ValueError("tcoef must be a contiguous fp64 [nt, 3] tensor on the fields' device")
                if nt < 2 and tm is None:           # (a box-packed series brings its time neighbours along: one step is a series)
                    raise ValueError("dT/dt by finite differences needs at least 2 time steps")
            elif with_q and dTdt is None:
                if time_s is None:
                    raise ValueError("with_q needs time_s (seconds) or a dTdt cube")
                time_s = np.asarray(time_s, dtype=np.float64)
                if time_s.size != nt:
                    raise ValueError("time_s must have one entry per time step of the cube")
                if nt < 2:
                    raise ValueError("dT/dt by finite differences needs at least 2 time steps")
                # cached: an upload from pageable memory makes the host wait for the stream at every call
                if self._tcoef is None or self._tcoef[0].shape != time_s.shape or not np.array_equal(self._tcoef[0], time_s):
                    self._tcoef = (time_s.copy(), self._up(tables.time_coefs(time_s)))
                tcoef = self._tcoef[1]
        boxes, bt, dev = self._resolve_boxes(boxes, nyb_min=0 if rows_out is None else int(rows_out.shape[2]))
        if per_step_boxes is None:
            per_step_boxes = len(boxes) != 1
        if len(boxes) != (t_count if per_step_boxes else 1):
            raise ValueError("boxes: give one box, or one per processed time step" if steps is None else "steps: one box per table row")
        if bt.ring and (per_step_boxes or packed or steps is not None):
            raise ValueError("a ring is one fixed box on whole cubes: no per-step boxes, packed series or step table")
        shape = (t_count, nl, bt.nyb_max, _lib.LEC_NSTAT)
        rows = torch.empty(shape, dtype=torch.float64, device=tair.device) if rows_out is None else rows_out
        if rows.shape != shape or rows.dtype != torch.float64 or not rows.is_contiguous():
            raise ValueError("rows_out must be a contiguous fp64 [t_count, nl, nyb_max, 32] tensor")

        whole = PreparedBoxes(boxes, bt, dev)
        stream = C.c_void_p(torch.cuda.current_stream(tair.device).cuda_stream)
        for a in range(0, max(t_count, 1), self.MAX_STEPS_PER_LAUNCH):      # (t_count 0: one launch, which the library refuses)
            b = min(a + self.MAX_STEPS_PER_LAUNCH, t_count)
            part = whole.part(a, b) if per_step_boxes and (a, b) != (0, t_count) else whole
            ra = _lib.RowstatsArgs(
                tair_d=_ptr(tair), u_d=_ptr(u), v_d=_ptr(v), omega_d=_ptr(omega), geopt_d=_ptr(geopt), dTdt_d=_ptr(dTdt),
                dtype=_lib.LEC_F64 if tair.dtype == torch.float64 else _lib.LEC_F32, with_q=int(bool(with_q)),
                nt=nt, nl=nl, ny=ny, nx=nx, t_begin=t_begin + a if steps is None else 0, t_count=b - a,
                n_box=len(part), nxb_max=bt.nxb_max, nyb_max=bt.nyb_max, lon_uniform=int(bt.lon_uniform),
                box_per_step=int(bool(per_step_boxes)), reserved0=0, box_d=_ptr(part.dev["box_data" if packed else "box"]),
                boxtab_d=_ptr(part.dev["boxtab"]), wlon_d=_ptr(part.dev["wlon"]), glon_d=_ptr(part.dev["glon"]), lattab_d=_ptr(part.dev["lattab"]),
                levtab_d=_ptr(self._levtab), tcoef_d=_ptr(tcoef if steps is None else tcoef[a:b]),
                rows_d=_ptr(rows[a:b]), stream=stream, tuning=make_tuning(tuning), tm_d=_ptr(tm), tp_d=_ptr(tp))
            with torch.cuda.device(tair.device):
                if timing is not None:
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()
                if bt.ring:
                    _lib.check(self.lib.lec_rowstats_ring(C.byref(ra)), "lec_rowstats_ring")
                elif steps is None:
                    _lib.check(self.lib.lec_rowstats(C.byref(ra)), "lec_rowstats")
                else:
                    _lib.check(self.lib.lec_rowstats_steps(C.byref(ra), _ptr(steps[a:b])), "lec_rowstats_steps")
                if timing is not None:
                    ev1.record()
                    timing.append((ev0, ev1))
        return rows

    def _check_fields(self, cubes: Sequence[torch.Tensor], packed: Optional[PreparedBoxes]) -> None:
        """The field cubes of a stage-1 call (T first): [time, level, lat, lon], fp64 or fp32, one shape, dtype and GPU device,
        contiguous; on the engine's grid -- or, for a box-packed series (``packed``: its boxes), on slabs that hold the tallest /
        widest box."""
        tair = cubes[0]
        if tair.dim() != 4:
            raise ValueError("fields must be [time, level, lat, lon]")
        nl, ny, nx = tair.shape[1:]
        if packed is not None:
            if nl != self.level.size or ny < packed.bt.nyb_max or nx < packed.bt.nxb_max or ny > self.lat.size or nx > self.lon.size:
                raise ValueError(f"packed cubes {tuple(tair.shape)}: need {self.level.size} levels and slabs that hold the tallest / widest box")
        elif (nl, ny, nx) != (self.level.size, self.lat.size, self.lon.size):
            raise ValueError(f"field shape {tuple(tair.shape)} does not match the engine grid "
                             f"({self.level.size} levels, {self.lat.size} lats, {self.lon.size} lons)")
        if tair.dtype not in (torch.float64, torch.float32):
            raise ValueError("fields must be float64 or float32")
        for c in cubes:
            if c.shape != tair.shape or c.dtype != tair.dtype or c.device != tair.device or not c.is_contiguous():
                raise ValueError("all field cubes must share shape, dtype, device and be contiguous")
        if tair.device.type != "cuda":
            raise _lib.LecLibraryError("fields must live on the GPU: there is no CPU path")

    def check_steps(self, steps: torch.Tensor, tcoef: Optional[torch.Tensor], nt: int, device) -> int:
        """Host validation of a step table (``rowstats(steps=...)``) before any launch: int32 [S, 3] contiguous on ``device``, entries in
        [0, nt); ``tcoef`` fp64 [S, 3] contiguous on ``device``.  Returns S; raises ValueError."""
        if not isinstance(steps, torch.Tensor) or steps.dtype != torch.int32 or steps.dim() != 2 or steps.shape[1] != 3 or steps.shape[0] < 1:
            raise ValueError("steps must be an int32 [S, 3] tensor (S >= 1): {cube step, previous step, next step} per box")
        if steps.device != torch.device(device) or not steps.is_contiguous():
            raise ValueError("steps must be contiguous and on the fields' device")
        s = int(steps.shape[0])
        if (tcoef is None or not isinstance(tcoef, torch.Tensor) or tuple(tcoef.shape) != (s, 3) or tcoef.dtype != torch.float64
                or tcoef.device != torch.device(device) or not tcoef.is_contiguous()):
            raise ValueError(f"steps needs tcoef: a contiguous fp64 [{s}, 3] tensor (by box) on the fields' device")
        host = steps.cpu().numpy()
        bad = np.flatnonzero(np.any((host < 0) | (host >= nt), axis=1))
        if bad.size:
            raise ValueError(f"steps: box {int(bad[0])} names cube steps {host[bad[0]].tolist()} outside [0, {nt})")
        return s

    @staticmethod
    def packed_width(nl: int) -> int:
        """Doubles per time step of a packed result record: 16 scalars + 21 level tables."""
        return _lib.LEC_NSCALAR + _lib.LEC_NLEVTAB * int(nl)

    def reduce(self, rows: torch.Tensor, boxes: Sequence[Sequence[int]], *, phi_scale: float = 1.0,
               drop_any_time: Optional[bool] = None, merge_dropmask: Optional[Callable[[torch.Tensor], None]] = None,
               keep_rows: bool = False, out: Optional[torch.Tensor] = None,
               nanflag_out: Optional[torch.Tensor] = None) -> LECResult:
        """Stage 2 on row records [t_count, nl, nyb_max, 32] (``lec_reduce``).

        ``out``: a caller-owned fp64 [t_count, 16 + 21 nl] tensor (rows may be strided, columns contiguous) that receives the packed
        records -- e.g. the send buffer of the time-sharded gather (``parallel.SeriesGatherer``), so a pass allocates nothing and
        repacks nothing; ``nanflag_out``: int32 [t_count].  Default: fresh tensors.

        ``merge_dropmask``: for a series processed in shards -- called with this shard's any-time NaN-level mask
        (int32 [28, nl], non-zero = drop) and must merge it in place with the other shards' masks (element-wise
        max, e.g. an all_reduce); the merged mask then applies to every shard, as xarray's dropna(dim=level) on the
        whole [time, level] array does in the reference (energy_contents.py:203-207)."""
        t_count, nl = int(rows.shape[0]), int(rows.shape[1])
        boxes, bt, dev = self._stage2_input(rows, boxes)
        am, levraw, dropmask_ws = self._workspace(t_count, nl, rows.device)
        res = self._stage2(_lib.STAGE_BOTH, rows, levraw, am, dropmask_ws, boxes, bt, dev, phi_scale, drop_any_time, merge_dropmask, out, nanflag_out)
        res.rows = rows if keep_rows else None
        return res

    # -- the two halves of stage 2, for series whose row records are not held whole (ingest.lec_streamed) ---------------------------
    def level_stage(self, rows: torch.Tensor, boxes, levraw_out: torch.Tensor, *, phi_scale: float = 1.0) -> None:
        """rows [t_count, nl, nyb_max, 32] -> ``levraw_out`` [t_count, nl, 40] (``lec_reduce`` with stage LEC_STAGE_LEVELS): the level x
        latitude half of stage 2 for a chunk of a series.  6.8 MB of row records per 37 x 721 time step become 12 KB, so a streamed
        series keeps ONE levraw buffer for all its steps and recycles the chunk's row records."""
        t_count, nl = int(rows.shape[0]), int(rows.shape[1])
        boxes, bt, dev = self._stage2_input(rows, boxes)
        if (levraw_out.shape != (t_count, nl, _lib.LEC_NLEVRAW) or levraw_out.dtype != torch.float64 or levraw_out.device != rows.device
                or not levraw_out.is_contiguous()):
            raise ValueError("levraw_out must be a contiguous fp64 [t_count, nl, 40] tensor on the rows' device")
        am = self._workspace(t_count, nl, rows.device, am_only=True)
        self._stage2(_lib.STAGE_LEVELS, rows, levraw_out, am, None, boxes, bt, dev, phi_scale, False, None, None, None)

    def vertical_stage(self, levraw: torch.Tensor, boxes, *, drop_any_time: Optional[bool] = None,
                       merge_dropmask: Optional[Callable[[torch.Tensor], None]] = None, out: Optional[torch.Tensor] = None,
                       nanflag_out: Optional[torch.Tensor] = None) -> LECResult:
        """levraw [t_count, nl, 40] of a whole series (or shard) -> the packed records (``lec_reduce`` with stage LEC_STAGE_VERTICAL):
        _handle_nans with the any-time mask over ALL the steps (``drop_any_time`` / ``merge_dropmask`` as in ``reduce``), the pressure
        integrals and the boundary assembly.  ``boxes``: the series' box(es), for the per-box constants."""
        t_count, nl = int(levraw.shape[0]), int(levraw.shape[1])
        boxes, bt, dev = self._stage2_input(levraw, boxes, levraw=True)
        dropmask_ws = torch.empty((_lib.LEC_NLEVFUN, nl), dtype=torch.int32, device=levraw.device)
        return self._stage2(_lib.STAGE_VERTICAL, None, levraw, None, dropmask_ws, boxes, bt, dev, 1.0, drop_any_time, merge_dropmask, out, nanflag_out)

    def _stage2_input(self, rec: torch.Tensor, boxes, levraw: bool = False):
        """(boxes, tables, device tables) of a stage-2 call on its input records: row records [t_count, nl, nyb_max, 32], or
        ``levraw`` [t_count, nl, 40] -- contiguous fp64 on the engine's levels, with one box or one per step."""
        t_count = int(rec.shape[0])
        boxes, bt, dev = self._resolve_boxes(boxes, nyb_min=0 if levraw else int(rec.shape[2]))
        if len(boxes) not in (1, t_count):
            raise ValueError("boxes: give one box, or one per processed time step")
        tail = (_lib.LEC_NLEVRAW,) if levraw else (bt.nyb_max, _lib.LEC_NSTAT)
        if rec.shape != (t_count, self.level.size) + tail or rec.dtype != torch.float64 or not rec.is_contiguous():
            raise ValueError("levraw must be a contiguous fp64 [t_count, nl, 40] tensor" if levraw else
                             "rows must be a contiguous fp64 [t_count, nl, nyb_max, 32] tensor")
        return boxes, bt, dev

    def _workspace(self, t_count: int, nl: int, device, am_only: bool = False):
        # the workspaces are scratch of one call only (stream-ordered: the next call on the stream may reuse them); keyed by the
        # stream too: two calls of one shape on different streams must not share scratch (or the dropmask)
        f64 = dict(dtype=torch.float64, device=device)
        wkey = (t_count, nl, str(device), int(torch.cuda.current_stream(device).cuda_stream))
        if wkey not in self._work:
            if len(self._work) > 4:
                self._work.clear()
            self._work[wkey] = (torch.empty((t_count, nl, 8), **f64), torch.empty((t_count, nl, _lib.LEC_NLEVRAW), **f64),
                                torch.empty((_lib.LEC_NLEVFUN, nl), dtype=torch.int32, device=device))
        return self._work[wkey][0] if am_only else self._work[wkey]

    def _stage2(self, stage, rows, levraw, am, dropmask_ws, boxes, bt, dev, phi_scale, drop_any_time, merge_dropmask, out, nanflag_out) -> Optional[LECResult]:
        t_count, nl = int(levraw.shape[0]), int(levraw.shape[1])
        device = levraw.device
        f64 = dict(dtype=torch.float64, device=device)
        width = self.packed_width(nl)
        scalars = levels = nanflag = None
        if stage != _lib.STAGE_LEVELS:
            if out is None:
                out = torch.empty((t_count, width), **f64)
            elif (out.shape != (t_count, width) or out.dtype != torch.float64 or out.device != device or out.stride(1) != 1
                  or out.stride(0) < width or out.data_ptr() % 8):
                raise ValueError(f"out must be an fp64 [t_count, {width}] tensor on the rows' device with contiguous columns")
            scalars = out[:, :_lib.LEC_NSCALAR]
            levels = out[:, _lib.LEC_NSCALAR:].unflatten(1, (_lib.LEC_NLEVTAB, nl))
            if nanflag_out is None:
                nanflag = torch.empty((t_count,), dtype=torch.int32, device=device)
            else:
                nanflag = nanflag_out
                if nanflag.shape != (t_count,) or nanflag.dtype != torch.int32 or nanflag.device != device or not nanflag.is_contiguous():
                    raise ValueError("nanflag_out must be a contiguous int32 [t_count] tensor on the rows' device")
        if drop_any_time is None:
            drop_any_time = len(boxes) == 1
        dropmask = dropmask_ws if (drop_any_time and stage != _lib.STAGE_LEVELS) else None
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        mode = 0 if dropmask is None else (2 if merge_dropmask is not None else 1)
        rd = _lib.ReduceArgs(
            rows_d=_ptr(rows), t_count=t_count, nl=nl, n_box=len(boxes), nyb_max=bt.nyb_max,
            box_d=_ptr(dev["box"]), boxtab2_d=_ptr(dev["boxtab2"]), lattab2_d=_ptr(dev["lattab2"]),
            levtab2_d=_ptr(self._levtab2), phi_scale=float(phi_scale),
            drop_any_time=mode, stage=stage, dropmask_d=_ptr(dropmask),
            am_d=_ptr(am), levraw_d=_ptr(levraw), scalars_d=_ptr(scalars), levels_d=_ptr(levels),
            nanflag_d=_ptr(nanflag), stream=stream, scalars_stride=0 if out is None else int(out.stride(0)),
            levels_stride=0 if out is None else int(out.stride(0)))
        with torch.cuda.device(device):
            if mode == 2:
                _lib.check(self.lib.lec_dropmask(C.byref(rd)), "lec_dropmask")
                merge_dropmask(dropmask)
                if stage == _lib.STAGE_BOTH:
                    rd.stage = _lib.STAGE_VERTICAL          # lec_dropmask has filled levraw: the level half need not run again
            _lib.check(self.lib.lec_reduce(C.byref(rd)), "lec_reduce")
        if stage == _lib.STAGE_LEVELS:
            return None
        return LECResult(scalars=scalars, levels=levels, nanflag=nanflag, rows=None, packed=out)
