/*
 * lec_hip.h -- C ABI of the MI355X (gfx950) Lorenz-Energy-Cycle engine.
 *
 * The reference (daniloceano/LorenzCycleToolkit, pure Python) has no FFI; its hot path is the Python
 * call surface between the frameworks and the numerics.  Each entry point below names the reference
 * interface it replaces (paths relative to the reference repository root):
 *
 *   lec_rowstats  replaces the 4-D passes of  BoxData.__init__            src/utils/box_data.py:78-295
 *                 (CalcZonalAverage            src/utils/calc_averages.py:25-43,
 *                  AdiabaticHEating            src/utils/thermodynamics.py:76-124)
 *                 and every 4-D eddy product / edge selection inside
 *                 EnergyContents.calc_*        src/analysis/energy_contents.py:99-165
 *                 ConversionTerms.calc_*       src/analysis/conversion_terms.py:103-245
 *                 BoundaryTerms.calc_*         src/analysis/boundary_terms.py:125-418
 *                 GenerationDissipationTerms   src/analysis/generation_and_dissipation_terms.py:122-152
 *   lec_ingest    replaces, for data that is already in device memory as raw file bytes, the decode of
 *                 xr.open_dataset (CF scale_factor / add_offset / _FillValue; get_data,
 *                 src/utils/preprocessing.py:35-146), the longitude wrap + sorts + >= 10 hPa filter of
 *                 process_data (preprocessing.py:275-365), the crop of slice_domain
 *                 (src/utils/select_area.py:254-338) and the unit conversion of BoxData._extract_data
 *                 (box_data.py:297-310): one gather pass instead of four host copies.
 *   lec_reduce    replaces the (level x lat) math of the same calc_* methods: CalcAreaAverage
 *                 (calc_averages.py:46-78), StaticStability (thermodynamics.py:26-73), the
 *                 differentiate("rlats"/level) calls, _handle_nans (energy_contents.py:190-208),
 *                 and the integrate(level) epilogues.
 *   lec_track_diag  replaces MetPy's wind_speed / vorticity on the 850-hPa slice and get_position /
 *                 find_extremum_coordinates of the moving framework
 *                 (src/frameworks/lec_moving_framework.py:269-417,650-663; src/utils/tools.py:95-128).
 *   lec_follow    replaces the click loop of the interactive chooser (-c/--choose: src/utils/select_area.py:201-251, with the
 *                 circle on the box's vorticity minimum, select_area.py:106-155) and get_limits' choose branch
 *                 (lec_moving_framework.py:227-245): the box of every time step is centred on the system by the device.
 *
 * Conventions
 *   - All pointers named *_d are DEVICE pointers owned by the caller; the library allocates nothing.
 *   - Field cubes are C-contiguous [nt][nl][ny][nx] (time, level, lat S->N, lon W->E), fp64 or fp32.
 *   - Calls are asynchronous on `stream` (a hipStream_t passed as void*); they do not synchronise.
 *   - Return value 0 = success; non-zero = error, text via lec_last_error() (thread-local).
 *   - No exceptions cross the ABI.  Thread-safe across distinct streams.
 */
#ifndef LEC_HIP_H
#define LEC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 8 (round 4): lec_reduce_args.stage (the two halves of stage 2 run apart; no 65535-step limit), lec_inflate_args.dst_bytes and
 * lec_chunk_scatter_args.src_bytes (the destination / payload ranges of every descriptor are bounds-checked on the device). */
#define LEC_ABI_VERSION 11
/* ABI 11: lec_rowstats_steps -- stage 1 over the boxes of several tracks on ONE cube, each box naming its cube step and that step's time
 * neighbours in a device table (lec_rowstats_args unchanged).
 * ABI 10 (round 6): lec_ingest_args.nt_src (was reserved0) / jmap_len / imap_len: a per-step gather table (step_d) is bounds-checked --
 * lec_ingest refuses one without them, its kernel writes NaN rows for an entry that points outside the source or the maps instead of
 * reading there, and lec_check_maps scans the table and names the first bad entry.
 * ABI 9 (round 5): lec_format_csv_rows (host): a per-level table as the text pandas writes for it, one call per table;
 * lec_rowstats_args.tm_d / tp_d: box-packed series of the moving framework (the struct grew by two pointers at its end); lec_dtdt;
 * lec_ingest_args.step_d / step_base: per-step gathers (the struct grew at its end). */

/* number of fp64 values per (time, level, lat) row record written by lec_rowstats */
#define LEC_NSTAT 32
/* number of per-(time, level) intermediate values written by lec_reduce into `levraw_d` */
#define LEC_NLEVRAW 40
/* per-time outputs of lec_reduce */
#define LEC_NSCALAR 16 /* Az Ae Kz Ke Cz Ca Ck Ce BAz BAe BKz BKe BPhiZ BPhiE Gz Ge */
#define LEC_NLEVFUN 28 /* functions of level that _handle_nans repairs (10 terms + 3 x 6 boundary pieces) */
#define LEC_NLEVTAB 21 /* Az Ae Kz Ke Ge Gz Cz Cz_1 Cz_2 Ca Ca_1 Ca_2 Ce Ce_1 Ce_2 Ck Ck_1..Ck_5 */

enum lec_dtype { LEC_F64 = 0, LEC_F32 = 1, LEC_I16 = 2, LEC_I32 = 3, LEC_I8 = 4 /* the integers: lec_ingest source only */ };

/* Stage-1 kernel families (lec_tuning.kernel).  Every family writes the same row records; AUTO is what is
 * measured and shipped, the others exist for cross-checks and A/B measurements.  The library reads NO
 * environment variables: everything that steers it is in the argument structs.
 * The workgroup orders assume the MI355X's 8 XCDs (workgroups are dealt to them round-robin, so blockIdx % 8 labels the XCD); on a
 * part with another count the results are the same and only the locality differs. */
enum lec_kernel {
    LEC_KERNEL_AUTO = 0,       /* box tiles for per-time-step boxes, row blocks for all terms on one fixed fp64 box, else one wave per row */
    LEC_KERNEL_TWO_SWEEP = 1,  /* lec_rowstats.hip: the reference's own order (deviation from the zonal mean, then products); rows <= lec_max_row() */
    LEC_KERNEL_ROW_SWEEP = 2,  /* lec_rowsweep.hip: one wave per row, one sweep */
    LEC_KERNEL_ROW_BLOCK = 3,  /* lec_rowblock.hip: blocks of neighbouring rows exchange T through LDS (all terms, one fixed box, dT/dt from the cube) */
    LEC_KERNEL_BOX_TILE = 4,   /* lec_boxtile.hip: one wave per four box rows walks the levels; six values per point transposed through LDS */
    LEC_KERNEL_BOX_PLANE = 5   /* lec_boxplane.hip (ABI 10): the same rows and sums with the planes' rows loaded straight into the compute layout -- a
                                  box-packed series on even longitudes, slabs of at most 64 columns: fp64 or fp32 storage with a dT/dt cube, or fp32
                                  storage with T of the time neighbours as tm_d / tp_d (what LEC_KERNEL_AUTO picks there; bit-identical records) */
};

/* workgroup -> row order of the row kernels (speed only) */
enum lec_order {
    LEC_ORDER_AUTO = 0,
    LEC_ORDER_MEMORY = 1,      /* rows in memory order */
    LEC_ORDER_XCD_LAT = 2,     /* every XCD owns a latitude chunk, walked latitude-fastest per (time, level) */
    LEC_ORDER_XCD_TILED = 7    /* one wave per row: every XCD owns a chunk of ceil(rows / 8) latitudes (the last one what is left), walked in
                                  tiles of tile_t time steps x tile_j latitudes at one level, levels next (all terms on one fixed box).
                                  The row-block kernel has one order of its own, which this field does not select: the XCDs own equal
                                  chunks of whole blocks, walked in such tiles of near-equal extent (at most tile_t blocks in time, about
                                  tile_j and at most tile_j + 1 in latitude); the blocks left over at the north end are dealt to the XCDs
                                  by time group (csrc/lec_schedule.h) */
};

/* Kernel selection of lec_rowstats; all zero = library defaults. */
typedef struct lec_tuning {
    int32_t kernel;        /* enum lec_kernel */
    int32_t block_shape;   /* LEC_KERNEL_ROW_BLOCK: 100 bt + 10 bk + bj waves (time x level x latitude, each 1 or 2); 0 = 212.
                              Box-tile / box-plane calls: 0 or 1 (one time step per workgroup) */
    int32_t order;         /* enum lec_order */
    int32_t tile_t, tile_j; /* tile extents of LEC_ORDER_XCD_TILED / of the row-block kernel (in blocks); box tiles: tile_t = time steps per
                               workgroup group, tile_j = levels per wave (default: from the launch size; at most 21 for the box-tile kernel
                               and 42 for the box-plane kernel, more is LEC_ERR_ARG);
                               0 = default; must be >= 0 */
    int32_t f32_vec;       /* fp32 storage, one wave per row: 0 = float4 trips when the cubes are 16-byte aligned, 2 = float2 trips */
    int32_t reserved[2];   /* must be 0 */
} lec_tuning;

enum lec_status {
    LEC_OK = 0,
    LEC_ERR_ARG = 1,      /* bad argument (null pointer, shape, alignment) */
    LEC_ERR_UNSUPPORTED = 2, /* row longer than the kernels support */
    LEC_ERR_LAUNCH = 3    /* HIP reported a launch error */
};

/* row-record layout (index into the LEC_NSTAT values of one row) */
enum lec_stat {
    LEC_S_MT = 0, LEC_S_MU, LEC_S_MV, LEC_S_MW, LEC_S_MP, LEC_S_MQ,      /* zonal means [T] [u] [v] [w] [Phi] [Q] */
    LEC_S_TT = 6, LEC_S_UU, LEC_S_VV, LEC_S_VT, LEC_S_WT, LEC_S_UV,      /* [T'T'] [u'u'] [v'v'] [v'T'] [w'T'] [u'v'] */
    LEC_S_WU = 12, LEC_S_WV, LEC_S_WP, LEC_S_QT,                         /* [w'u'] [w'v'] [w'Phi'] [Q'T'] */
    LEC_S_VTT = 16, LEC_S_WTT, LEC_S_KV, LEC_S_KW, LEC_S_EV, LEC_S_EW,   /* [vT'T'] [wT'T'] [Kv] [Kw] [Ev] [Ew] */
    LEC_S_TW = 22, LEC_S_TE, LEC_S_UW, LEC_S_UE, LEC_S_VW, LEC_S_VE,     /* T,u,v at the west / east box column */
    LEC_S_SPARE = 28    /* 28..31: scratch of lec_rowstats (cross-time covariance pieces), not an interface */
};

/*
 * Stage 1: one pass over the field cubes -> LEC_NSTAT row statistics per (time, level, box-lat) row.
 *
 * Boxes: `box_d` holds n_box quadruples {iw, ie, js, jn} (inclusive grid indices).  box_per_step == 0: one
 * fixed (Eulerian) box for every time step, n_box == 1; box_per_step == 1: one box per processed time step
 * (semi-Lagrangian), n_box == t_count -- also when t_count == 1, so that a one-step shard or chunk of a
 * moving series runs the same kernels (and gives the same bits) as the whole series.  Every table indexed
 * by box has room for nxb_max / nyb_max entries per box.
 *
 * dT/dt for the diabatic-heating residual: if dTdt_d != NULL it is a cube like the fields (moving
 * framework, lorenzcycletoolkit.py:184-186); otherwise dT/dt = tc[t][0] T[t-1] + tc[t][1] T[t] +
 * tc[t][2] T[t+1] with tc = tcoef_d (np.gradient coefficients over the cube's time axis;
 * thermodynamics.py:109-110), neighbours taken from the same cube (so the cube must include the
 * halo time steps a shard needs; coefficients of non-existent neighbours must be 0).
 *
 * Box-packed series (ABI 9; box_per_step == 1, served by the box-tile kernel).  The reference's moving framework slices the box of
 * every time step out of the data (src/utils/box_data.py:297-310) before anything is computed; a producer that gathers anyway -- the
 * device ingest from file bytes, a host that uploads a track -- may hand over just those slices: cubes [nt][nl][ny][nx] whose step t
 * holds box t alone, its south-west corner at [t][k][0][0] (ny, nx >= the tallest / widest box; what lies outside a step's box is
 * never read).  `box_d` then describes the boxes AS THE CUBES HOLD THEM, {0, nxb - 1, 0, nyb - 1}, while every table indexed by box
 * (boxtab_d, wlon_d, glon_d, lattab_d) is built from the box's true grid coordinates as always.  The cube's time neighbours of step t
 * are other boxes, so T(t - 1) and T(t + 1) ON THE BOX OF STEP t come in two more cubes of the same layout, `tm_d` / `tp_d` (the step
 * itself where a neighbour does not exist: its coefficient is 0 -- but 0 x NaN is NaN), and dT/dt = tc[t][0] tm[t] + tc[t][1] T[t] +
 * tc[t][2] tp[t].  Same arithmetic on the same values: the row records are bit-identical to those of the unpacked cubes.  Rows of
 * 488 bytes scattered through a 243-column crop replay at 4.8 TB/s on MI355X, a step's box stored as one dense block at 5.7
 * (tools/probes/probe_boxread.hip) -- and a producer writes a tenth of the bytes.
 */
typedef struct lec_rowstats_args {
    /* fields */
    const void* tair_d;
    const void* u_d;
    const void* v_d;
    const void* omega_d;
    const void* geopt_d; /* may be NULL: Phi statistics are written as 0 */
    const void* dTdt_d;  /* may be NULL, see above */
    int32_t dtype;       /* enum lec_dtype, common to all cubes */
    int32_t with_q;      /* 0: skip the diabatic-heating statistics (MQ, QT written as 0) */
    int32_t nt, nl, ny, nx;     /* cube dimensions */
    int32_t t_begin, t_count;   /* process time steps [t_begin, t_begin + t_count) */
    /* boxes */
    int32_t n_box, nxb_max, nyb_max;
    int32_t lon_uniform;        /* 1: longitudes of every box are uniformly spaced (fast path) */
    int32_t box_per_step;       /* 0: one fixed box (n_box == 1); 1: one box per processed time step (n_box == t_count) */
    int32_t reserved0;          /* must be 0 */
    const int32_t* box_d;       /* [n_box][4] iw ie js jn */
    const double* boxtab_d;     /* [n_box][4]  1/xlength [rad^-1], h_rad, 1/h_deg, spare (h_* used if lon_uniform) */
    const double* wlon_d;       /* [n_box][nxb_max]     trapezoid weights in radians   (used if !lon_uniform) */
    const double* glon_d;       /* [n_box][nxb_max][3]  d/dlon[deg] coefficients a,b,c (used if !lon_uniform) */
    const double* lattab_d;     /* [n_box][nyb_max][4]  d/dlat[deg]/dy coefficients a,b,c ; 1/dx_j   (with_q) */
    const double* levtab_d;     /* [nl][3]  S = al T[k-1] + be T[k] + ga T[k+1] static-stability coefficients (with_q) */
    const double* tcoef_d;      /* [nt][3]  (with_q && dTdt_d == NULL) */
    /* output */
    double* rows_d;             /* [t_count][nl][nyb_max][LEC_NSTAT] */
    void* stream;
    lec_tuning tuning;          /* all zero = defaults */
    /* ABI 9: a BOX-PACKED series (see above); both NULL otherwise */
    const void* tm_d;           /* T of the previous time step on the box of step t, laid out like tair_d */
    const void* tp_d;           /* T of the next time step on the box of step t */
} lec_rowstats_args;

/*
 * Stage 2: (level x lat) math on the row records -> per-time scalars and per-level tables.
 * Limits: nl <= 160 levels (LEC_ERR_UNSUPPORTED beyond); nl * t_count < 2^26 per call (the launch is nl * t_count workgroups of 64
 * threads and HIP takes fewer than 2^32 threads per launch; LEC_ERR_UNSUPPORTED beyond: 1.8 million steps of 37 levels).
 *
 * The call has two halves that may also be run apart (`stage`, ABI 8), for series whose row records are not held whole:
 *   LEC_STAGE_LEVELS    rows_d -> levraw_d : the level x latitude work of the call's time steps; needs rows_d, box / lat / lev tables,
 *                       am_d, levraw_d -- 6.8 MB of row records per 37 x 721 time step become 12 KB, so a streamed series runs
 *                       this half chunk by chunk into ONE levraw buffer of the whole series and recycles the row records;
 *   LEC_STAGE_VERTICAL  levraw_d -> dropmask / scalars / levels / nanflag over t_count steps of levraw records (rows_d, box_d, am_d and
 *                       lattab2_d are not read and may be NULL; boxtab2_d is: the per-box constants c1, c2).
 * LEC_STAGE_BOTH (0) is the whole call.  Either way every number is the same: the halves are the same kernels.
 */
#define LEC_MAX_LEVELS 160
#define LEC_STAGE_BOTH 0
#define LEC_STAGE_LEVELS 1
#define LEC_STAGE_VERTICAL 2
typedef struct lec_reduce_args {
    const double* rows_d;       /* [t_count][nl][nyb_max][LEC_NSTAT] from lec_rowstats; 16-byte aligned */
    int32_t t_count, nl;
    int32_t n_box, nyb_max;
    const int32_t* box_d;       /* [n_box][4] */
    const double* boxtab2_d;    /* [n_box][4]  c1 = -1/(Re xlen ylen), c2 = -1/(Re ylen), spare, spare */
    const double* lattab2_d;    /* [n_box][nyb_max][8]  cos*wphi/ylen, wphi, cos, tan, d/dphi[rad] a,b,c, spare; 16-byte aligned */
    const double* levtab2_d;    /* [nl][4]  p [Pa], d/dp a,b,c */
    double phi_scale;           /* multiplies the geopotential statistics (g when the file holds height) */
    int32_t drop_any_time;      /* _handle_nans' dropna(dim=level) on a [time, level] array (energy_contents.py:203-207), fixed framework:
                                   a level that is still NaN after the interpolation at ANY time step is dropped from the pressure
                                   integrals of EVERY time step.
                                   0: per time step (moving framework: one BoxData per step);
                                   1: any-time over the time steps of this call (mask computed by the call);
                                   2: any-time with the mask in dropmask_d taken as given: the caller ran lec_dropmask on every
                                      shard / chunk of the series and merged the masks (element-wise max) */
    int32_t stage;              /* LEC_STAGE_BOTH (0), LEC_STAGE_LEVELS, LEC_STAGE_VERTICAL (see above) */
    int32_t* dropmask_d;        /* [LEC_NLEVFUN][nl] (needed when drop_any_time): workspace zeroed by the call (mode 1), input (mode 2) */
    double* am_d;               /* workspace [t_count][nl][8]  area means (always required; left untouched when nyb_max <= 64) */
    double* levraw_d;           /* workspace [t_count][nl][LEC_NLEVRAW] */
    double* scalars_d;          /* out [t_count][LEC_NSCALAR] */
    double* levels_d;           /* out [t_count][LEC_NLEVTAB][nl] */
    int32_t* nanflag_d;         /* out [t_count] number of NaN level values repaired/dropped (0 = clean) */
    void* stream;
    int64_t scalars_stride;     /* doubles between the scalars of consecutive time steps; 0 = dense (LEC_NSCALAR) */
    int64_t levels_stride;      /* doubles between the level tables of consecutive time steps; 0 = dense (LEC_NLEVTAB * nl).  With
                                   scalars_d = buf, levels_d = buf + LEC_NSCALAR and both strides = LEC_NSCALAR + LEC_NLEVTAB * nl the call
                                   writes one packed record per time step: the send buffer of the time-sharded gather, no repacking */
} lec_reduce_args;

/*
 * Ingest: raw source cube [nt][nl_in][ny_in][nx_in] (file order, file byte order, possibly CF-packed) ->
 * field cube [nt][nl][ny][nx] in the order lec_rowstats wants (level ascending in Pa, lat S->N, lon W->E),
 * cropped to the analysis domain, in SI units.
 *
 *   value = decode(src[t][kmap[k]][jmap[j]][imap[i]])            source element, byte-swapped if asked
 *   fill:                  value == fill_value (compared before scaling) -> NaN
 *   decode_dtype LEC_F64:  v = (double)value; packed: v = v * scale_factor; v = v + add_offset      (two roundings, fp64)
 *   decode_dtype LEC_F32:  v = (float)value;  packed: v = (float)((double)v * scale_factor); v = (float)((double)v + add_offset)
 *                          -- the reference's pinned xarray 2024.2.0 decodes int16 data to float32 when the variable has a
 *                          fill value or no add_offset, and keeps float32 data float32 (float64 attributes: each operation
 *                          is computed in fp64 and rounded to float32); the caller picks the dtype by those rules
 *   out = v * unit_scale   in decode_dtype, stored as out_dtype
 */
typedef struct lec_ingest_args {
    const void* src_d;          /* device copy of the raw variable bytes for nt time steps */
    int32_t src_dtype;          /* LEC_I8, LEC_I16, LEC_I32, LEC_F32 or LEC_F64 (int32 values are exact in fp64 only: decode_dtype LEC_F64) */
    int32_t swap_bytes;         /* 1: source is in the opposite byte order (classic NetCDF is big-endian) */
    int32_t nt, nl_in, ny_in, nx_in;
    int32_t nl, ny, nx;         /* output extents */
    const int32_t* kmap_d;      /* [nl] output level -> source level */
    const int32_t* jmap_d;      /* [ny] output latitude -> source latitude */
    const int32_t* imap_d;      /* [nx] output longitude -> source longitude */
    int32_t has_packing, has_fill;
    double scale_factor, add_offset, fill_value, unit_scale;
    int32_t out_dtype;          /* LEC_F64 or LEC_F32: storage of the output cube (>= decode_dtype; widening is exact) */
    int32_t decode_dtype;       /* LEC_F64 or LEC_F32: the precision the reference's decode gives this variable (see below) */
    void* out_d;                /* [nt][nl][ny][nx] */
    void* stream;
    /* ABI 9: per-step gathers (a box-packed series of the moving framework: every output step holds another box, possibly of another
     * source step).  NULL: output step t reads source step t with the maps as they are.  Else step_d[t] = {source step, latitude
     * offset, longitude offset}: output step t reads source step step_d[t][0] - step_base of src_d through jmap_d[j + step_d[t][1]] and
     * imap_d[i + step_d[t][2]] -- the maps must be long enough for the largest offset + ny / nx (lengthen them by repeating their last
     * entry); nt counts OUTPUT steps, the source holds nt_src steps.
     * ABI 10: the table lives in device memory, where argument validation cannot see it (the reference bounds-checks its track against
     * the data on the host, lec_moving_framework.py:112-154), so the call carries what bounds it: nt_src, jmap_len, imap_len.  An entry
     * with a source step outside [step_base, step_base + nt_src) or an offset outside [0, jmap_len - ny] / [0, imap_len - nx] never
     * reads: lec_ingest writes NaN into that output step's rows, and lec_check_maps names the first such entry. */
    const int32_t* step_d;      /* [nt][3] or NULL */
    int32_t step_base;          /* the source step that src_d starts with */
    int32_t nt_src;             /* time steps src_d holds (step_d given: >= 1; else ignored -- the source then holds nt steps) */
    int32_t jmap_len, imap_len; /* entries of jmap_d / imap_d (step_d given: >= ny / nx; else 0 = ny / nx) */
} lec_ingest_args;

/*
 * 850-hPa track diagnostics of the moving framework, one box per time step:
 *   lec_moving_framework.py:650-663  wind_speed(u, v), vorticity(u, v) on the whole 850-hPa slice
 *   lec_moving_framework.py:269-417  get_position: the extrema inside the box (inclusive label slices)
 *   tools.py:95-128                  find_extremum_coordinates
 * zeta(j, i) = sum_k xcoef[j][i][k] v[j][i0 + k] - sum_k ycoef[j][k] u[j0 + k][i] + curv[j] u[j][i],  i0 = clamp(i - 1, 0, nx - 3),
 * j0 = clamp(j - 1, 0, ny - 3): three-point derivatives, second order also at the ends of the slice (the stencil of
 * metpy.calc.first_derivative).  The FORMULATION is the caller's: the coefficient tables carry the metric (1/m).  The Python host
 * builds two (diagnostics.vorticity_tables): "metpy_no_crs" -- what MetPy 1.6.2 evaluates for DataArrays without a CRS, as the
 * reference passes them: plain dv/dx - du/dy, distances = great-circle arcs between neighbouring grid points on pyproj's default
 * sphere (a = 6,370,997 m), curv = 0 -- and "spherical": dx = Re cos(phi) dlambda, dy = Re dphi, curv = tan(phi) / Re.
 * NaN (below-ground points) is skipped, values and positions alike; among equal values the first in row-major order of the box
 * wins (numpy's argmin / argmax).  Parity of the vorticity against MetPy itself is unpinned.
 */
typedef struct lec_diag_args {
    const double* u_d;          /* [nt][ny][nx] eastward wind at 850 hPa (m/s) */
    const double* v_d;          /* [nt][ny][nx] northward wind */
    const double* hgt_d;        /* [nt][ny][nx] geopotential height (gpm) */
    int32_t nt, ny, nx, reserved0;
    const int32_t* box_d;       /* [nt][6]  iw, ie, js, jn: inclusive index ranges of the box; jc, ic: the grid point nearest its centre */
    const double* xcoef_d;      /* [ny][nx][3]  d/dx coefficients of point (j, i) along its row (1/m) */
    const double* ycoef_d;      /* [ny][3]      d/dy coefficients of row j along a column (1/m) */
    const double* curv_d;       /* [ny]         coefficient of u (1/m): tan(phi) / Re on the sphere, 0 for the plain Cartesian form */
    double* val_d;              /* [nt][5]  zeta minimum, zeta maximum, height minimum, wind-speed maximum, zeta at (jc, ic);
                                            NaN when the box holds no finite value */
    int32_t* pos_d;             /* [nt][8]  (j, i) grid indices of the four extrema, in that order; -1 when there is none */
    void* stream;
} lec_diag_args;

/*
 * -c/--choose without a display: one box per time step that FOLLOWS the 850-hPa system.  Replaces the click loop of
 *   select_area.py:201-251      draw_box_map: the user drags a box over the step's vorticity / height / wind map
 *   select_area.py:106-155      plot_min_zeta: the circle on the minimum vorticity of the box that guides the next click
 *   lec_moving_framework.py:227-245  get_limits, choose branch: the clicked box becomes the step's limits
 * by a chain the device closes itself (additive call: no struct of ABI 11 changes).  Per time step t:
 *   F_t(j, i)  field = LEC_FOLLOW_ZETA: the zeta of lec_track_diag (same tables, same expression);  LEC_FOLLOW_HGT: hgt_d
 *   S_t(j, i)  the arithmetic mean of the finite F_t(j', i') with |j' - j| <= smooth_r, |i' - i| <= smooth_r inside the slice, summed in
 *              row-major order; NaN when none is finite.  smooth_r = 0: F_t itself.
 *   window     admissible centres [jlo, jhi] x [ilo, ihi] (grid points whose box lies inside the slice: the host's business) cut to
 *              [jc - sj, jc + sj] x [ic - si, ic + si] around the centre (jc, ic) of step t - 1; step 0: around (j_start, i_start), or
 *              all admissible centres when both are -1
 *   centre     the position of the minimum (LEC_FOLLOW_MIN) / maximum (LEC_FOLLOW_MAX) finite S_t of the window; among equal values the
 *              first in row-major order of the window (numpy's argmin / argmax); a window without a finite value keeps the previous
 *              centre (step 0 without a start: jlo, ilo) and sets status 1
 * The chain is sequential in time: ONE workgroup of 256 threads walks the steps and keeps the window's field in an LDS tile of
 * min(2 sj + 1 + 2 smooth_r, ny) x min(2 si + 1 + 2 smooth_r, nx) doubles; a tile beyond the 160 KiB one workgroup may declare is
 * LEC_ERR_UNSUPPORTED (the message gives both figures).  Scalars are validated before any HIP call, refused and never clamped
 * (LEC_ERR_ARG names the field).
 */
enum lec_follow_field { LEC_FOLLOW_ZETA = 0, LEC_FOLLOW_HGT = 1 };
enum lec_follow_sense { LEC_FOLLOW_MIN = 0, LEC_FOLLOW_MAX = 1 };

typedef struct lec_follow_args {
    const double* u_d;          /* [nt][ny][nx] eastward wind at 850 hPa (m/s) on the search domain (lat S->N, lon W->E) */
    const double* v_d;          /* [nt][ny][nx] northward wind */
    const double* hgt_d;        /* [nt][ny][nx] geopotential height (gpm); may be NULL unless field = LEC_FOLLOW_HGT */
    int32_t nt, ny, nx;
    int32_t field;              /* enum lec_follow_field */
    const double* xcoef_d;      /* [ny][nx][3], [ny][3], [ny]: the vorticity tables of lec_diag_args */
    const double* ycoef_d;
    const double* curv_d;
    int32_t sense;              /* enum lec_follow_sense */
    int32_t smooth_r;           /* >= 0 grid points */
    int32_t sj, si;             /* >= 1: the largest move per step, in grid points */
    int32_t jlo, jhi, ilo, ihi; /* inclusive bounds of the admissible centres: 0 <= jlo <= jhi < ny, 0 <= ilo <= ihi < nx */
    int32_t j_start, i_start;   /* an admissible centre, or both -1 */
    int32_t* pos_d;             /* [nt][2]  (j, i) of every step's centre */
    double* val_d;              /* [nt]     S_t at the centre it found; NaN where status is 1 */
    int32_t* status_d;          /* [nt]     0, or 1: the window held no finite value and the centre was kept */
    void* stream;
} lec_follow_args;

/*
 * -c/--choose for SEVERAL systems in one run (additive calls: no struct of ABI 11 changes).
 *
 * lec_follow_seeds: the systems of the FIRST time step.  The rule:
 *   S         lec_follow's S on that slice: the mean of the finite field values within smooth_r, summed in row-major order, NaN where
 *             none is finite.  S is defined on the WHOLE slice, not only on the admissible centres.
 *   better    smaller for LEC_FOLLOW_MIN, larger for LEC_FOLLOW_MAX.
 *   candidate a grid point (j, i) for which all four hold:
 *               - it is an admissible centre (jlo..jhi x ilo..ihi);
 *               - S(j, i) is finite;
 *               - S(j, i) is at least as good as `threshold` (a NaN threshold: no threshold);
 *               - among the finite S(j', i') with |j' - j| <= ej, |i' - i| <= ei inside the slice none is better than S(j, i), and none
 *                 that comes before (j, i) in the slice's row-major order is equal to it.
 *             The last condition makes a plateau or a tie yield exactly one candidate, its first point.  The neighbourhood reaches
 *             over inadmissible points on purpose: a system whose centre lies outside the admissible centres is not seeded by its flank.
 *   seeds     the candidates ordered by value, best first, equal values by row-major index; the first k_max of them are taken, and
 *             n_found may be smaller than k_max.  Seed 0 is usually what lec_follow picks at step 0 without a start; the rule does not
 *             promise it (lec_follow's extremum need not be a candidate: a better value may lie outside the admissible centres).
 * Three phases on the caller's stream: (a) S of the whole slice into work_d, one thread per point, lanes along longitude, through the
 * function lec_follow's first step uses; (b) the candidate test, one thread per admissible centre, the neighbourhood read from work_d;
 * (c) ONE workgroup takes the best remaining candidate k_max times (the wave64 shuffles and LDS partials of lec_follow's extremum; key:
 * the value, then the row-major index).  The library owns no device memory: work_d is the caller's, and its contents after the call
 * are unspecified.  Every scalar is validated before any HIP call, refused and never clamped (LEC_ERR_ARG names the field).
 *
 * lec_follow_many: n_chains chains of lec_follow in ONE launch, workgroup c walking chain c from start_d[c] through the very device
 * function lec_follow's kernel runs: chain c IS lec_follow with that start -- the same positions, the same status, the same val bit
 * for bit -- and no workgroup communicates with another, so a chain's bits do not depend on its company.  start_d lives in DEVICE
 * memory (the output of lec_follow_seeds plugs straight in), where argument validation cannot see it, so the kernel checks its entry
 * first: (-1, -1) keeps lec_follow's meaning (step 0 scans every admissible centre); any other entry outside the admissible centres,
 * (-2, -2) included, makes the chain read nothing: status LEC_FOLLOW_BAD_START, pos -1 and val NaN at every step.  The LDS tile, its
 * 160 KiB refusal and the validation of the scalars are lec_follow's.
 */
#define LEC_FOLLOW_BAD_START 2  /* status of a chain of lec_follow_many whose start_d entry is no admissible centre */

typedef struct lec_follow_seeds_args {
    const double* u_d;          /* [ny][nx] ONE slice: eastward wind at 850 hPa on the search domain */
    const double* v_d;          /* [ny][nx] northward wind */
    const double* hgt_d;        /* [ny][nx] geopotential height (gpm); may be NULL unless field = LEC_FOLLOW_HGT */
    int32_t ny, nx;
    int32_t field, sense;       /* enum lec_follow_field, enum lec_follow_sense */
    const double* xcoef_d;      /* the vorticity tables of lec_diag_args */
    const double* ycoef_d;
    const double* curv_d;
    int32_t smooth_r;           /* >= 0 */
    int32_t ej, ei;             /* >= 1: half-extent of the neighbourhood (the least separation of two seeds), in grid points */
    int32_t k_max;              /* 1..256 */
    int32_t jlo, jhi, ilo, ihi; /* inclusive bounds of the admissible centres */
    double threshold;           /* the field's own value and sign; NaN: none */
    double* work_d;             /* [ny][nx] caller-owned scratch */
    int32_t* seed_pos_d;        /* [k_max][2] (j, i), best first; unused entries (-2, -2) */
    double* seed_val_d;         /* [k_max]    S at the seed; NaN where unused */
    int32_t* n_found_d;         /* [1]        seeds found, 0..k_max */
    void* stream;
} lec_follow_seeds_args;

typedef struct lec_follow_many_args {
    const double* u_d;          /* [nt][ny][nx], as lec_follow_args */
    const double* v_d;
    const double* hgt_d;
    int32_t nt, ny, nx;
    int32_t field;
    const double* xcoef_d;
    const double* ycoef_d;
    const double* curv_d;
    int32_t sense, smooth_r, sj, si;
    int32_t jlo, jhi, ilo, ihi;
    int32_t n_chains;           /* >= 1 */
    int32_t reserved0;
    const int32_t* start_d;     /* [n_chains][2] DEVICE memory: (j, i) an admissible centre, or (-1, -1) */
    int32_t* pos_d;             /* [n_chains][nt][2] */
    double* val_d;              /* [n_chains][nt] */
    int32_t* status_d;          /* [n_chains][nt]  0, 1 as lec_follow, or LEC_FOLLOW_BAD_START */
    void* stream;
} lec_follow_many_args;

/*
 * -c --choose-lifecycle: systems that form after the first time step or end before the last (additive calls: no struct of ABI 11 changes).
 *
 * lec_follow_seeds_series: the seeds of EVERY time step of [nt][ny][nx] slices in one call.  Step t's outputs -- seed_pos_d[t],
 * seed_val_d[t], n_found_d[t] -- are exactly what lec_follow_seeds gives on slice t: positions, order, n_found, the (-2, -2) / NaN marks
 * and the value bits.  The three phases of lec_follow_seeds are batched over t through the same device functions: the smooth and the
 * candidate kernel run over (point, step), the select kernel one workgroup per step; every index over the series has 64 bits and the grids
 * are strided over, so no grid dimension bounds nt.  work_d is [nt][ny][nx], the caller's; the library owns no device memory.  Every
 * scalar is validated before any HIP call, refused and never clamped (LEC_ERR_ARG names the field); a series whose nt * ny * nx does not
 * leave the byte offsets room in 64 bits is LEC_ERR_UNSUPPORTED.
 *
 * lec_follow_spans: n_chains chains, each BORN at its own step and ENDED by a rule.  start_d [n_chains][3] = (t0, j, i).  The rule:
 *   - The chain walks steps t0, t0+1, ... as lec_follow does on the sub-series starting at t0 with start (j, i).  The window, tie rule and
 *     kept centre on a blind window are unchanged.
 *   - A walked step is *good* when its status is 0 and its val is at least as good as end_threshold.  With a NaN threshold, status 0
 *     alone makes it good.
 *   - The chain *stops* after the first walked step that completes `patience` consecutive not-good steps, or at the end of the series.
 *   - span = (first good step, last good step), or (-1, -1) when no walked step is good.
 *   - Walked steps carry lec_follow's pos / val / status.
 *   - Steps never walked (before t0, after the stop) carry pos -1, val NaN and the status LEC_FOLLOW_NOT_LIVE (3).
 *   - The table lives where validation cannot see it.  An entry with t0 outside [0, nt) or (j, i) outside the admissible centres gives
 *     LEC_FOLLOW_BAD_START at every step and span (-1, -1), and reads nothing else.  (-1, -1) as (j, i) is NOT accepted here, because a
 *     born chain always has a start.
 * One workgroup per chain through the device function lec_follow's kernel runs, no communication between workgroups; a stopped chain's
 * workgroup returns at once: a short-lived system costs its own steps, not the series'.  The LDS tile, its 160 KiB refusal and the
 * validation of the scalars are lec_follow_many's.
 */
#define LEC_FOLLOW_NOT_LIVE 3   /* status of a step a chain of lec_follow_spans never walked */

typedef struct lec_follow_seeds_series_args {
    const double* u_d;          /* [nt][ny][nx], as lec_follow_args */
    const double* v_d;
    const double* hgt_d;        /* may be NULL unless field = LEC_FOLLOW_HGT */
    int32_t nt, ny, nx;
    int32_t field;
    const double* xcoef_d;
    const double* ycoef_d;
    const double* curv_d;
    int32_t sense, smooth_r;
    int32_t ej, ei;             /* >= 1, as lec_follow_seeds_args */
    int32_t k_max;              /* 1..256 */
    int32_t reserved0;
    int32_t jlo, jhi, ilo, ihi;
    double threshold;           /* NaN: none */
    double* work_d;             /* [nt][ny][nx] caller-owned scratch */
    int32_t* seed_pos_d;        /* [nt][k_max][2] */
    double* seed_val_d;         /* [nt][k_max] */
    int32_t* n_found_d;         /* [nt] */
    void* stream;
} lec_follow_seeds_series_args;

typedef struct lec_follow_spans_args {
    const double* u_d;          /* [nt][ny][nx], as lec_follow_many_args */
    const double* v_d;
    const double* hgt_d;
    int32_t nt, ny, nx;
    int32_t field;
    const double* xcoef_d;
    const double* ycoef_d;
    const double* curv_d;
    int32_t sense, smooth_r, sj, si;
    int32_t jlo, jhi, ilo, ihi;
    int32_t n_chains;           /* >= 1 */
    int32_t patience;           /* >= 1 */
    const int32_t* start_d;     /* [n_chains][3] DEVICE memory: (t0, j, i), 0 <= t0 < nt, (j, i) an admissible centre */
    double end_threshold;       /* the field's own value and sign; NaN: none */
    int32_t* pos_d;             /* [n_chains][nt][2] */
    double* val_d;              /* [n_chains][nt] */
    int32_t* status_d;          /* [n_chains][nt]  0, 1 as lec_follow, LEC_FOLLOW_BAD_START or LEC_FOLLOW_NOT_LIVE */
    int32_t* span_d;            /* [n_chains][2]   (first good step, last good step) or (-1, -1) */
    void* stream;
} lec_follow_spans_args;

/*
 * -c --choose-chunk: a series longer than memory (additive call: no struct of ABI 11 changes).
 *
 * lec_follow_spans_chunk: lec_follow_spans on ONE CHUNK of consecutive steps of a series, with chains that can be resumed.  What the
 * fields mean in this call: nt counts the steps of THIS chunk and u_d / v_d / hgt_d hold only those steps; t_base is the series step that
 * slice 0 of this call holds; start_d [n_chains][3] = (t0, j, i) with t0 a series step; pos_d / val_d / status_d are [n_chains][nt], for
 * the chunk's steps; span_d [n_chains][2] is written on every call, in series steps, from the state as it stands after the chunk.
 * state_d [n_chains][8] int32, device memory, read and written: the state of chain c is {phase, jc, ic, weak, first, last, 0, 0}.
 *   - phase 0 = not yet born, 1 = walking, 2 = stopped, 3 = bad start.
 *   - jc, ic = the centre after the last walked step.
 *   - weak = the not-good steps in a row so far.
 *   - first, last = the good steps so far, in series steps, -1 when none.
 *   - The caller zeroes the state before the first chunk and passes it on unchanged from then on.  A chain table may grow between calls:
 *     new rows are appended with zeroed state rows.
 * The rule, per chain and call:
 *   - Bad start.  If (j, i) is outside the admissible centres or t0 < 0, the chain is phase 3 in every call.  Every step gets
 *     LEC_FOLLOW_BAD_START, pos -1, val NaN; span is (-1, -1).  Nothing else is read.  The kernel checks start_d first, as
 *     lec_follow_many does.  The table is device memory the validation cannot see.
 *   - Not yet born (phase 0).  If t_base <= t0 < t_base + nt, the chain is born in this chunk.  Local steps before t0 are
 *     LEC_FOLLOW_NOT_LIVE, and it walks from t0 with start (j, i).  If t0 lies beyond the chunk, every step is LEC_FOLLOW_NOT_LIVE and
 *     the phase stays 0.
 *   - Walking (phase 1).  It walks from local step 0 with the centre and counters of the state.
 *   - Stopped (phase 2).  Every step is LEC_FOLLOW_NOT_LIVE.
 *   - A walked step is lec_follow_spans' walked step, statement for statement.  The same window around the previous centre, the same
 *     tile, the same row-major mean, the same extremum and tie rule, the same kept centre on a blind window.  The same good / stop
 *     decision with end_threshold and patience.  A chain that stops marks the rest of the chunk LEC_FOLLOW_NOT_LIVE, goes to phase 2,
 *     and its workgroup returns.
 *   - patience = 0 is accepted here and means "never stops".  It stays refused by lec_follow_spans.  This is how the resumed form of
 *     lec_follow / lec_follow_many is obtained.
 * The defining property: for ANY cut of a series into consecutive chunks, the chunk calls with the state carried through give the
 * following, bit for bit.  With patience >= 1: concatenated pos / val / status and a final span_d equal to one lec_follow_spans call on
 * the whole series.  With patience 0 and every t0 = 0: every pos / val / status of lec_follow_many from the same starts.
 * What the property does not cover: a t0 at or beyond the end of the series is never born here (every step LEC_FOLLOW_NOT_LIVE), where
 * lec_follow_spans, which sees the whole series, calls it a bad start; a chain appended after the chunk of its t0 has passed is never
 * born either; a walking state whose centre is no admissible centre (one the caller did not pass on unchanged) reads nothing and counts
 * as stopped.
 * One workgroup of 256 per chain, no workgroup waits for another; the state is read and written by one thread with plain vector loads
 * and stores.  The LDS tile and its 160 KiB refusal (the message gives both figures) are lec_follow_many's.  Scalars are validated
 * before any HIP call, refused with LEC_ERR_ARG and never clamped: everything lec_follow_spans checks, t_base >= 0, nt >= 1,
 * patience >= 0, state_d not null, and a t_base + nt that overflows int32.
 */
typedef struct lec_follow_chunk_args {
    const double* u_d;          /* [nt][ny][nx]: the chunk's steps only */
    const double* v_d;
    const double* hgt_d;
    int32_t nt, ny, nx;         /* nt: the steps of this chunk */
    int32_t field;
    const double* xcoef_d;
    const double* ycoef_d;
    const double* curv_d;
    int32_t sense, smooth_r, sj, si;
    int32_t jlo, jhi, ilo, ihi;
    int32_t n_chains;           /* >= 1 */
    int32_t patience;           /* >= 0; 0: never stops */
    const int32_t* start_d;     /* [n_chains][3] DEVICE memory: (t0, j, i), t0 a series step >= 0, (j, i) an admissible centre */
    double end_threshold;       /* the field's own value and sign; NaN: none */
    int32_t* pos_d;             /* [n_chains][nt][2] */
    double* val_d;              /* [n_chains][nt] */
    int32_t* status_d;          /* [n_chains][nt]  0, 1 as lec_follow, LEC_FOLLOW_BAD_START or LEC_FOLLOW_NOT_LIVE */
    int32_t* span_d;            /* [n_chains][2]   series steps, from the state after this chunk */
    void* stream;
    int32_t t_base;             /* >= 0: the series step that slice 0 of this call holds */
    int32_t* state_d;           /* [n_chains][8] DEVICE memory, read and written; zeroed by the caller before the first chunk */
} lec_follow_chunk_args;

/*
 * -c --choose-periodic: a search domain that is a full RING of longitudes (additive calls: no struct, export or kernel result of ABI 11
 * changes).  A ring has no preferred meridian.
 *
 *   int lec_follow_seeds_series_ring(const lec_follow_seeds_series_args*);
 *   int lec_follow_spans_chunk_ring (const lec_follow_chunk_args*);
 *
 * They take the existing structs with the same field meanings.  The one difference: longitude is periodic, so column nx - 1 is the
 * western neighbour of column 0.  Only the two most general calls get a ring form: one chunk with patience >= 1 is lec_follow_spans;
 * patience 0 with t0 = 0 is lec_follow / lec_follow_many; one step of the seeds series is lec_follow_seeds.  The rule:
 *
 * Stencil and tables.
 *   - The zeta stencil at column i reads columns i - 1, i, i + 1 mod nx, for every i.
 *   - xcoef[j][i] holds the centred coefficients at all columns (the host's vorticity_tables(..., periodic=True) builds them).  The
 *     spacing from column nx - 1 to column 0 is the arc across the seam.
 *   - Interior columns get the same doubles as today.
 *   - The latitude stencil and curv are unchanged.
 * Admissible centres.
 *   - Every column is an admissible centre.  ilo = 0 and ihi = nx - 1 are required.
 *   - jlo / jhi keep their meaning.
 * Window.
 *   - Rows [jc - sj, jc + sj] are cut to [jlo, jhi], as today.
 *   - Columns ic - si ... ic + si are never cut.  They run west to east and are taken mod nx.
 * S (the smoothed field).
 *   - S is the mean of the finite field values with |dj| <= r inside the slice and |di| <= r on the ring.
 *   - It is summed in row-major order of that neighbourhood, west to east from i - r.
 *   - A point always has 2 r + 1 columns.
 * Extremum and ties.
 *   - The extremum rule, the tie rule (first in row-major order of the *window*), the centre kept on a blind window, good / stop / span /
 *     state and every status code are lec_follow_spans_chunk's, statement for statement.
 *   - Positions are written as i mod nx.
 *   - A walking state whose ic is outside [0, nx) counts as stopped, as an inadmissible centre does today.
 * Seeds.
 *   - The neighbourhood is |dj| <= ej inside the slice and ring distance <= ei.
 *   - The tie clause keeps the slice's absolute row-major index.
 *   - A tie is therefore the one thing that depends on where the seam lies.
 * Validation.  Every refusal is LEC_ERR_ARG naming the field, made before any HIP call, never clamped:
 *   - 2 si + 1 + 2 r > nx or 2 ei + 1 > nx is refused, because the window would meet itself (for the seeds, 2 r + 1 > nx likewise).
 *   - ilo != 0 or ihi != nx - 1 is refused.
 *   - Everything the non-ring calls check is checked here too.
 * The kernels are the existing ones' device functions with one more compile-time parameter.  The chain's LDS tile is
 * min(2 sj + 1 + 2 r, ny) x (2 si + 1 + 2 r) doubles, its column c ring column (ic - si - r + c) mod nx; each tile row is loaded as at
 * most two contiguous runs, the wrap is a compare-and-subtract.  The 160 KiB refusal is as before.
 */
int lec_follow_seeds_series_ring(const lec_follow_seeds_series_args* args);
int lec_follow_spans_chunk_ring(const lec_follow_chunk_args* args);

int lec_version(void);
const char* lec_last_error(void);

/* longest box row (in grid points) lec_rowstats accepts for the given dtype / alignment / kernel family
 * (enum lec_kernel; only LEC_KERNEL_TWO_SWEEP, which holds a row in registers, has a practical limit) */
int lec_max_row(int dtype, int aligned, int kernel);

int lec_rowstats(const lec_rowstats_args* args);

/*
 * Stage 1 over the boxes of MANY tracks on one cube (ABI 11).  The reference runs one process per track (its documented batch is a
 * shell loop, docs/source/examples_and_tutorials.rst); here K tracks over one file share one cube -- the union of their time steps on
 * the union of their crops -- and one launch.  Box b reads cube step step_d[b][0] and forms dT/dt per point as
 *   tc[b][0] T[step_d[b][1]] + tc[b][1] T[step_d[b][0]] + tc[b][2] T[step_d[b][2]],   tc = tcoef_d indexed BY BOX ([t_count][3])
 * -- the track's own previous / next time, which need not be the cube's neighbouring step (a 6-hourly track over 3-hourly data) and may
 * be shared with other tracks' boxes.  At a track's first / last time the neighbour is the step itself and its coefficient 0, as in
 * lec_rowstats.  The records (and so lec_reduce) are those of lec_rowstats on the track's own cube, bit for bit.
 *   step_d   device memory, int32 [t_count][3] = {t, t_prev, t_next}, absolute cube steps.  An entry outside [0, nt) never reads: that
 *            box's records are written as NaN (the table lives where argument validation cannot see it; the Python host checks it first).
 *   args     as for lec_rowstats, with box_per_step = 1, n_box = t_count, t_begin = 0 (t_count may exceed nt), with_q = 1 and tcoef_d;
 *            dTdt_d, tm_d and tp_d NULL (the cube layout only).  tuning.kernel other than LEC_KERNEL_AUTO / LEC_KERNEL_BOX_TILE:
 *            LEC_ERR_UNSUPPORTED (the box-tile kernel serves every call).
 */
int lec_rowstats_steps(const lec_rowstats_args* args, const int32_t* step_d);

/*
 * -f --periodic: ONE fixed box whose columns are a full RING of longitudes -- a zonal band, a hemisphere, the globe (an additive call: no
 * struct, export or kernel result of ABI 11 changes).  A ring has no preferred meridian.
 *
 *   int lec_rowstats_ring(const lec_rowstats_args*);
 *
 * It takes the existing struct with the same field meanings.  The one difference: the box's columns iw .. ie are a closed circle, so
 * column ie is the western neighbour of column iw.  The rule is the reference's own formulas on the CLOSED axis:
 *
 * The closed axis.
 *   - The nxb = ie - iw + 1 evenly spaced columns (step h) get column iw once more at lon[ie] + h: nxb + 1 points,
 *     xlength = deg2rad(lon[ie] + h) - deg2rad(lon[iw]).
 *   - The library knows no longitudes: boxtab_d carries {1 / xlength, h_rad = xlength / nxb, 1 / h_deg} (tables.build_box_tables(ring=True)).
 *   - A box narrower than the cube is computed as if closed and reads nothing outside it; that it is a full circle is the caller's statement.
 * Zonal means and products.
 *   - The trapezoid over the closed axis is h * sum over the nxb columns: every column has weight 1 (a limited-area row gives its two end
 *     columns 1/2 and leaves out the interval that closes the circle).
 * Q.
 *   - dT/dlon is the centred three-point difference at EVERY column: column iw reads column ie, column ie reads column iw.
 *   - d/dphi, d/dp and d/dt are unchanged.
 * Records.
 *   - The same LEC_NSTAT numbers per row.  LEC_S_TE / UE / VE are written with the WEST column's values: the east column of the closed
 *     axis is the west column, so every east-minus-west difference of the boundary terms is exactly 0 in lec_reduce, which is untouched.
 *   - boxtab2_d of lec_reduce carries c1 = -1 / (Re xlength ylength) and xlen with the closed xlength.  The quirks the reference has in
 *     latitude and pressure are kept (ylength from sines, Ck term 5, the second terms of BPhiE / BPhiZ, _handle_nans).
 * Kernels.
 *   - tuning.kernel LEC_KERNEL_AUTO or LEC_KERNEL_ROW_SWEEP: both run one wave per row (the kernel of lec_rowsweep.hip with one more
 *     compile-time parameter, instantiated in lec_rowsweep_ring.hip; only the first and last trip of a row differ).  Any other family: LEC_ERR_UNSUPPORTED.  tuning.order keeps its meaning.
 *   - dT/dt from the cube's time axis goes through the cross-time covariances and lec_qtime_kernel as for any fixed box.
 * Validation.  Every refusal is LEC_ERR_ARG naming the field, made before any HIP call, never clamped:
 *   - box_per_step != 0, n_box != 1, lon_uniform != 1, tm_d / tp_d given, nxb_max < 3 (a ring has at least 3 columns).
 *   - Everything lec_rowstats checks is checked here too.  lec_check_boxes serves ring calls unchanged.
 */
int lec_rowstats_ring(const lec_rowstats_args* args);

/*
 * -f --periodic --wavenumbers N: the ZONAL-WAVENUMBER SHARES of the eight eddy covariances of every ring row (an additive call: no
 * struct, export or kernel result of ABI 11 changes; lec_rowspec.hip is a code object of its own, loaded by spectral calls only).
 *
 * On the closed, evenly spaced axis the zonal mean is the plain mean over the nx columns, so the discrete Parseval identity splits every
 * covariance of a row a_0 .. a_{nx-1}, b_0 .. b_{nx-1} exactly:
 *   a^_n = (1 / nx) sum_i a_i exp(-2 pi i n i / nx),    C_n(a, b) = w_n Re(a^_n conj(b^_n)),    [a'b'] = sum_{n = 1}^{nx / 2} C_n(a, b),
 *   w_n = 2 for 1 <= n < nx / 2, w_n = 1 for n = nx / 2 (nx even: the Nyquist wavenumber).
 * The call writes, for the rows of the latitude band js .. jn of time steps [t_begin, t_begin + t_count),
 *   spec_d [t_count][nl][jn - js + 1][n_wave][8]:  C_n of LEC_S_TT, UU, VV, VT, WT, UV, WU, WV (slots 6 .. 13 of a row record, in that
 *   order) for n = 1 .. n_wave.
 * Every eddy term lec_reduce forms (Ae, Ke, Ca, Ce, Ck) is linear in those eight slots given the zonal means, so row records that carry
 * the shares of one n in slots 6 .. 13 and everything else as lec_rowstats_ring wrote it give that term's wavenumber-n part: no
 * second formulation of stage 2 (the Python host assembles the records).
 *   - Cubes [nt][nl][ny][nx] as lec_rowstats_ring takes them (fp64 or fp32 storage; all nx columns are the ring).  Accumulation is fp64.
 *   - twid_d [nx][2]: cos and sin of 2 pi m / nx, m = 0 .. nx - 1, fp64, built on the host (tables.twiddle_table), 16-byte aligned.  The
 *     kernel indexes it with (n i) mod nx kept as an integer: no recurrence and no device sincos, so a result does not depend on how the
 *     row is walked beyond the order of its fp64 sums.
 *   - A row's column 0 is subtracted from the row before it is projected (T is about 288 K with eddies of about 1 K; a constant has no
 *     share in n >= 1).
 *   - NaN: a NaN anywhere in a row of a field makes every share that field enters NaN, for every n -- the pattern of the covariances
 *     lec_rowstats_ring writes for that row.
 * Validation.  Every refusal is LEC_ERR_ARG naming the field, made before any HIP call, never clamped: null tair_d / u_d / v_d /
 * omega_d / twid_d / spec_d, dtype, nx < 3, t_begin / t_count outside the cube, js / jn outside 0 <= js <= jn < ny, n_wave < 1 or
 * n_wave > nx / 2, twid_d / spec_d not 16-byte aligned.  n_wave > LEC_MAX_WAVENUMBERS, or more than 2^31 - 1 rows: LEC_ERR_UNSUPPORTED.
 */
#define LEC_MAX_WAVENUMBERS 64 /* the largest n_wave of one lec_rowspec_ring call */
typedef struct lec_rowspec_args {
    const void* tair_d;
    const void* u_d;
    const void* v_d;
    const void* omega_d;
    int32_t dtype;              /* enum lec_dtype (LEC_F64 or LEC_F32), common to the four cubes */
    int32_t nt, nl, ny, nx;     /* cube dimensions; the nx columns are the ring */
    int32_t t_begin, t_count;   /* process time steps [t_begin, t_begin + t_count) */
    int32_t js, jn;             /* the latitude band (inclusive grid rows) */
    int32_t n_wave;             /* wavenumbers 1 .. n_wave; 1 <= n_wave <= min(nx / 2, LEC_MAX_WAVENUMBERS) */
    const double* twid_d;       /* [nx][2] cos, sin of 2 pi m / nx; 16-byte aligned */
    double* spec_d;             /* out [t_count][nl][jn - js + 1][n_wave][8]; 16-byte aligned */
    void* stream;
} lec_rowspec_args;
int lec_rowspec_ring(const lec_rowspec_args* args);

/*
 * -f --periodic --wavenumbers N --wavenumbers-generation: the ZONAL-WAVENUMBER SHARES of the generation covariance [Q'T'] of every ring
 * row (an additive call: no struct, export or kernel result of ABI 11 changes; lec_rowspecq.hip is a code object of its own).
 *
 * Q itself never reaches a row record -- lec_rowstats_ring keeps its row statistics [Q] and [Q'T'] only -- so this call evaluates the
 * diabatic-heating residual at every point of a row and projects it, beside T, onto the wavenumbers:
 *   qspec_d [t_count][nl][jn - js + 1][n_wave]:  C_n(Q, T) = w_n Re(Q^_n conj(T^_n)), n = 1 .. n_wave  (a^_n, w_n as above), so that
 *   [Q'T'] = sum_{n = 1}^{nx / 2} C_n(Q, T) = slot LEC_S_QT of the row's record.
 * Ge is linear in that slot, so row records that carry C_n(Q, T) there give Ge(n) in the stage-2 batch of lec_rowspec_ring's shares.
 *   - Q = cp (dT/dt + u dT/dx + v dT/dy - S w), the Q of lec_rowstats_ring: d/dlon the centred three-point difference at every column
 *     (column 0 reads column nx - 1 and the reverse; inv_hdeg = boxtab[2] of the ring box, lattab_d[j][3] = 1 / dx_j); d/dlat from
 *     lattab_d[j][0..2], the ring box's own table: one-sided at the band's first and last row, and no row outside js .. jn is read;
 *     S from levtab_d, one-sided at the top and bottom level; dT/dt = tcoef_d[t][0] T[t-1] + tcoef_d[t][1] T[t] + tcoef_d[t][2] T[t+1]
 *     over the CUBE's time axis (tcoef_d has nt rows; steps outside [t_begin, t_begin + t_count) are read as neighbours).  A neighbour
 *     that does not exist is the row itself with coefficient 0.  A dT/dt cube is not supported.
 *   - Cubes, twid_d, the integer twiddle index, fp64 accumulation and the removal of T's column 0: as lec_rowspec_ring.  The column
 *     classes of a wavenumber are summed in a fixed order: a row's result depends on (nx, n_wave) and on nothing else.
 *   - NaN: qspec_d of a row is NaN for every n exactly where LEC_S_QT of lec_rowstats_ring's record of that row is NaN.
 * Validation.  Every refusal is LEC_ERR_ARG naming the field, made before any HIP call, never clamped: null tair_d / u_d / v_d /
 * omega_d / twid_d / lattab_d / levtab_d / tcoef_d / qspec_d, dtype, nt < 2, nx < 3, t_begin / t_count outside the cube, js / jn outside
 * 0 <= js < jn < ny (a band needs two rows for d/dlat; lec_rowstats_ring refuses a one-row box likewise), n_wave < 1 or n_wave > nx / 2,
 * twid_d / qspec_d not 16-byte aligned, the tables not 8-byte aligned, a cube not aligned to its element.  n_wave > LEC_MAX_WAVENUMBERS,
 * or more than 2^31 - 1 rows: LEC_ERR_UNSUPPORTED.
 */
typedef struct lec_rowspec_q_args {
    const void* tair_d;
    const void* u_d;
    const void* v_d;
    const void* omega_d;
    int32_t dtype;              /* enum lec_dtype (LEC_F64 or LEC_F32), common to the four cubes */
    int32_t nt, nl, ny, nx;     /* cube dimensions; the nx columns are the ring */
    int32_t t_begin, t_count;   /* process time steps [t_begin, t_begin + t_count) */
    int32_t js, jn;             /* the latitude band (inclusive grid rows), js < jn */
    int32_t n_wave;             /* wavenumbers 1 .. n_wave; 1 <= n_wave <= min(nx / 2, LEC_MAX_WAVENUMBERS) */
    const double* twid_d;       /* [nx][2] cos, sin of 2 pi m / nx; 16-byte aligned */
    const double* lattab_d;     /* [jn - js + 1][4]: d/dlat a, b, c; 1 / dx_j (the ring box's lattab) */
    const double* levtab_d;     /* [nl][3]: the static-stability coefficients of lec_rowstats */
    const double* tcoef_d;      /* [nt][3]: np.gradient coefficients over the cube's time axis */
    double inv_hdeg;            /* boxtab[2] of the ring box: 1 / (longitude step in degrees) */
    double* qspec_d;            /* out [t_count][nl][jn - js + 1][n_wave]; 16-byte aligned */
    void* stream;
} lec_rowspec_q_args;
int lec_rowspec_q_ring(const lec_rowspec_q_args* args);

/*
 * -f --periodic --wavenumbers N --wavenumbers-interactions: the ZONAL-WAVENUMBER SHARES of the NON-LINEAR (eddy-eddy, triad) transfers of
 * every ring row (an additive call: no struct, export or kernel result of ABI 11 changes; lec_rowspec_nl.hip is a code object of its own).
 *
 * Ae is linear in the row covariance [T'T'] and Ke in [u'u'] + [v'v'].  With A_x the eddy-eddy advective tendency of x, the change of
 * [x'x'] / 2 by that advection is -[A_x' x'], so row records that carry -2 C_n(A_T, T) in slot LEC_S_TT give S(n) -- the available
 * potential energy wavenumber n receives from all the other eddies -- in the Ae place of stage 2, and records that carry
 * -2 C_n(A_u, u) / -2 C_n(A_v, v) in LEC_S_UU / LEC_S_VV give L(n), the same for kinetic energy, in the Ke place (Saltzman's S(n) and
 * L(n); positive: wavenumber n gains).  The call evaluates the tendencies at every point of a row and projects them beside T, u and v.
 *   For a row (t, k, j) of the band js .. jn, [x] = the row's zonal mean as lec_rowstats_ring wrote it into rows_d, x' = x - [x]:
 *     D_lambda x (i) = cx_j (x[i+1] - x[i-1]), wrapped indices, cx_j = 0.5 inv_hdeg lattab_d[j][3] (the stencil of lec_rowspec_q_ring);
 *     D_phi x = lattab_d[j][0] x[j-1] + lattab_d[j][1] x[j] + lattab_d[j][2] x[j+1], one-sided at the band's first and last row;
 *     D_p x = ptab_d[k][0] x[k-1] + ptab_d[k][1] x[k] + ptab_d[k][2] x[k+1], the coefficients of np.gradient(edge_order=1) over the
 *       levels in Pa, one-sided at the top and bottom level (tables.pressure_coefs; all 0 when nl = 1);
 *     A_T = u' D_lambda T + v' (D_phi T - D_phi [T]) + w' (D_p T - D_p [T])
 *     A_u = u' D_lambda u + v' (D_phi u - D_phi [u]) + w' (D_p u - D_p [u]) - m_j u' v'
 *     A_v = u' D_lambda v + v' (D_phi v - D_phi [v]) + w' (D_p v - D_p [v]) + m_j u' u',     m_j = tan(lat_j) / Re = lattab_d[j][4].
 *   A neighbour that does not exist is the row itself with coefficient 0: nothing outside the band, the levels or the requested steps
 *   is read.  The zonal means of the neighbour rows are taken from the neighbours' records in rows_d, not summed again.  There is no
 *   time stencil: a chunk of a streamed series needs no halo.
 *   nlspec_d [t_count][nl][jn - js + 1][n_wave][8]:  slot 0 = -2 C_n(A_T, T), slot 1 = -2 C_n(A_u, u), slot 2 = -2 C_n(A_v, v), slots
 *     3 .. 7 = 0 (C_n, w_n and the Nyquist weight as above): the layout of lec_rowspec_ring's spec_d, so lec_level_spec_ring takes it.
 *   nltot_d [t_count][nl][jn - js + 1][8]:  the same three slots for the whole eddy covariance, summed in physical space:
 *     -2 ((1 / nx) sum_i A_x(i) x'(i) - [A_x] [x']); slots 3 .. 7 = 0.  By Parseval the n_wave = nx / 2 shares sum to it.
 *   - Cubes, twid_d, the integer twiddle index and fp64 accumulation: as lec_rowspec_ring.  The column classes of a wavenumber are
 *     summed in a fixed order: a row's result depends on (nx, n_wave) and on nothing else.
 *   - NaN: slots 0 .. 2 of a row are NaN for every n -- and in nltot_d -- exactly where any value the row's stencil reads is NaN: the
 *     row itself, its existing j +- 1 / k +- 1 neighbours of T, u, v, or a record mean.  Slots 3 .. 7 are 0 even then.
 * Validation.  Every refusal names the field, is made before any HIP call, never clamped.  LEC_ERR_ARG: null tair_d / u_d / v_d /
 * omega_d / rows_d / twid_d / lattab_d / ptab_d / nlspec_d / nltot_d, dtype, nx < 3, nl < 1, ny < 2, t_begin / t_count outside the cube,
 * js / jn outside 0 <= js < jn < ny, n_wave < 1 or n_wave > nx / 2, twid_d / rows_d / nlspec_d / nltot_d not 16-byte aligned, the tables
 * not 8-byte aligned, a cube not aligned to its element.  LEC_ERR_UNSUPPORTED: n_wave > LEC_MAX_WAVENUMBERS, more than 2^31 - 1 rows.
 */
typedef struct lec_rowspec_nl_args {
    const void* tair_d;
    const void* u_d;
    const void* v_d;
    const void* omega_d;
    int32_t dtype;              /* enum lec_dtype (LEC_F64 or LEC_F32), common to the four cubes */
    int32_t nt, nl, ny, nx;     /* cube dimensions; the nx columns are the ring */
    int32_t t_begin, t_count;   /* process time steps [t_begin, t_begin + t_count) */
    int32_t js, jn;             /* the latitude band (inclusive grid rows), js < jn */
    int32_t n_wave;             /* wavenumbers 1 .. n_wave; 1 <= n_wave <= min(nx / 2, LEC_MAX_WAVENUMBERS) */
    const double* rows_d;       /* [t_count][nl][jn - js + 1][LEC_NSTAT], lec_rowstats_ring's records of the same steps and band; 16-byte aligned */
    const double* twid_d;       /* [nx][2] cos, sin of 2 pi m / nx; 16-byte aligned */
    const double* lattab_d;     /* [jn - js + 1][5]: d/dlat a, b, c; 1 / dx_j; tan(lat_j) / Re (tables.nl_lat_table) */
    const double* ptab_d;       /* [nl][3]: np.gradient coefficients over the levels in Pa (tables.pressure_coefs) */
    double inv_hdeg;            /* boxtab[2] of the ring box: 1 / (longitude step in degrees) */
    double* nlspec_d;           /* out [t_count][nl][jn - js + 1][n_wave][8]; 16-byte aligned */
    double* nltot_d;            /* out [t_count][nl][jn - js + 1][8]; 16-byte aligned */
    void* stream;
} lec_rowspec_nl_args;
int lec_rowspec_nl_ring(const lec_rowspec_nl_args* args);

/*
 * -f --periodic --wavenumbers N --wavenumbers-budget: the ZONAL-WAVENUMBER SHARES of the TRIPLE PRODUCTS behind the boundary terms of the
 * eddy budgets, BAe(n) and BKe(n), of every ring row (an additive call: no struct, export or kernel result of ABI 11 changes;
 * lec_rowspec_b.hip is a code object of its own).
 *
 * On a ring the east-west pieces of the boundary terms vanish (the ring pass writes the west column into the east slots), so stage 2
 * forms BAe from slots LEC_S_VTT (the band's first and last row) and LEC_S_WTT (bottom minus top level) of a row record and BKe from
 * LEC_S_EV and LEC_S_EW.  A triple product [a b'b'] is the covariance of the pointwise product P = a b' with b, because [b'] = 0:
 * [a b'b'] = [P'b'] = sum_n C_n(P, b), exactly, by the discrete Parseval identity of lec_rowspec_ring.
 *   For a row (t, k, j) of the band js .. jn, [x] = the row's zonal mean as lec_rowstats_ring wrote it into rows_d, x' = x - [x], v and w
 *   the FULL fields (their zonal means included: the transport by the mean flow and the triad part are both in a share):
 *   bspec_d [t_count][nl][jn - js + 1][n_wave][4]:
 *     slot 0  VTT(n) = C_n(v T', T)                      sum over n = 1 .. nx / 2:  [v T'T']  = slot LEC_S_VTT (16) of the row's record
 *     slot 1  WTT(n) = C_n(w T', T)                                                 [w T'T']  = slot LEC_S_WTT (17)
 *     slot 2  EV(n)  = C_n(v u', u) + C_n(v v', v)                                  [E v]     = slot LEC_S_EV  (20),  E = u'^2 + v'^2
 *     slot 3  EW(n)  = C_n(w u', u) + C_n(w v', v)                                  [E w]     = slot LEC_S_EW  (21)
 *   (C_n, w_n and the Nyquist weight as above.)  Slots 0 and 2 are computed for the rows j = js and j = jn only -- stage 2 reads them
 *   nowhere else -- and are 0.0 for every other row; slots 1 and 3 for every row and level (_handle_nans can move "bottom" and "top" to
 *   any level).  Row records that carry the four slots in places 16, 17, 20, 21 beside lec_rowspec_ring's shares in 6 .. 13 give BAe(n) and
 *   BKe(n) in the BAe and BKe places of stage 2 (lec_level_spec_b_ring).
 *   - Cubes, twid_d, the integer twiddle index and fp64 accumulation: as lec_rowspec_ring.  The products are formed with contraction
 *     off; the column classes of a wavenumber are summed in a fixed order: a row's result depends on (nx, n_wave) and on nothing else.
 *   - No derivative and no neighbour row is read, and there is no time stencil: a chunk of a streamed series needs no halo.
 *   - NaN: a computed slot of a row is NaN for every n exactly where the corresponding slot of the row's record is NaN (a NaN in any
 *     field the product reads, or in a record mean).  The skipped slots of interior rows stay 0.
 * Validation.  Every refusal names the field, is made before any HIP call, never clamped.  LEC_ERR_ARG: null tair_d / u_d / v_d /
 * omega_d / rows_d / twid_d / bspec_d, dtype, nx < 3, nl < 1, ny < 2, t_begin / t_count outside the cube, js / jn outside
 * 0 <= js < jn < ny, n_wave < 1 or n_wave > nx / 2, twid_d / rows_d / bspec_d not 16-byte aligned, a cube not aligned to its element.
 * LEC_ERR_UNSUPPORTED: n_wave > LEC_MAX_WAVENUMBERS, more than 2^31 - 1 rows.
 */
typedef struct lec_rowspec_b_args {
    const void* tair_d;
    const void* u_d;
    const void* v_d;
    const void* omega_d;
    int32_t dtype;              /* enum lec_dtype (LEC_F64 or LEC_F32), common to the four cubes */
    int32_t nt, nl, ny, nx;     /* cube dimensions; the nx columns are the ring */
    int32_t t_begin, t_count;   /* process time steps [t_begin, t_begin + t_count) */
    int32_t js, jn;             /* the latitude band (inclusive grid rows), js < jn */
    int32_t n_wave;             /* wavenumbers 1 .. n_wave; 1 <= n_wave <= min(nx / 2, LEC_MAX_WAVENUMBERS) */
    const double* rows_d;       /* [t_count][nl][jn - js + 1][LEC_NSTAT], lec_rowstats_ring's records of the same steps and band; 16-byte aligned */
    const double* twid_d;       /* [nx][2] cos, sin of 2 pi m / nx; 16-byte aligned */
    double* bspec_d;            /* out [t_count][nl][jn - js + 1][n_wave][4]; 16-byte aligned */
    void* stream;
} lec_rowspec_b_args;
int lec_rowspec_b_ring(const lec_rowspec_b_args* args);

/*
 * Stage 2 of the spectra without assembled records: the level x latitude half of lec_reduce for all n_wave wavenumbers of a chunk of
 * time steps (an additive call: no struct, export or kernel result of ABI 11 changes; lec_level_spec.hip is a code object of its own).
 *
 * For every wavenumber n, time step t and level k the call writes the LEC_NLEVRAW numbers that lec_reduce with LEC_STAGE_LEVELS writes for
 * the row records  rows_d[t][k][j]  with slots LEC_S_TT .. LEC_S_WV (6 .. 13) replaced by  spec_d[t][k][j][n][0..7]  and, when qspec_d is
 * given, slot LEC_S_QT (15) by  qspec_d[t][k][j][n]  -- bit for bit: the kernels are lec_reduce's two level kernels (one for bands of at
 * most 64 rows, one for taller bands) on the same source lines, and the only difference is where those nine slots of a record come from.
 * That is the definition of X(n); N copies of the row records are never formed.
 *   - Nothing else of a record is replaced: zonal means, edge values, the triple products 16 .. 21 and [w'Phi'] stay the ring pass's.
 *   - BAz's bottom-top term is repaired per latitude from the records of OTHER levels; their LEC_S_WT is read from spec_d at that level.
 *   - The area means read no replaced slot: they are formed once per (t, k) into am_d, not once per n.
 *   - box_d / lattab2_d / levtab2_d / phi_scale: of the ONE ring box, as lec_reduce takes them; nyb is the row count of the records.
 *   - levraw_d: record (n, t, k) at  levraw_d + n * wave_stride + (t * nl + k) * LEC_NLEVRAW,  so a chunk of a streamed series writes into
 *     the series' [n_wave][T][nl][LEC_NLEVRAW] buffer directly (wave_stride = T * nl * LEC_NLEVRAW, levraw_d at the chunk's first step).
 *     lec_reduce with LEC_STAGE_VERTICAL over the n_wave * T records then gives the shares.
 * Validation.  Every refusal names the field and is made before any HIP call.  LEC_ERR_ARG: null args, rows_d, spec_d, box_d, lattab2_d,
 * levtab2_d, am_d or levraw_d (qspec_d may be NULL: slot 15 stays the ring pass's); rows_d / spec_d / lattab2_d not 16-byte aligned;
 * n_wave < 1, t_count < 1, nl < 1, nyb < 2; wave_stride non-zero and smaller than dense.  LEC_ERR_UNSUPPORTED: n_wave >
 * LEC_MAX_WAVENUMBERS, nl > LEC_MAX_LEVELS, n_wave * t_count * nl >= 2^26 (one 64-lane workgroup per (n, t, k); the caller chunks).
 */
typedef struct lec_level_spec_args {
    const double* rows_d;       /* [t_count][nl][nyb][LEC_NSTAT], lec_rowstats_ring's records; 16-byte aligned */
    const double* spec_d;       /* [t_count][nl][nyb][n_wave][8], lec_rowspec_ring's; 16-byte aligned */
    const double* qspec_d;      /* [t_count][nl][nyb][n_wave], lec_rowspec_q_ring's, or NULL: slot 15 stays the ring pass's */
    int32_t t_count, nl, nyb, n_wave;
    const int32_t* box_d;       /* [1][4] */
    const double* lattab2_d;    /* [nyb][8]; 16-byte aligned */
    const double* levtab2_d;    /* [nl][4] */
    double phi_scale;
    double* am_d;               /* workspace [t_count][nl][8]: the area means */
    double* levraw_d;           /* out: record (n, t, k) at levraw_d + n * wave_stride + (t * nl + k) * LEC_NLEVRAW */
    int64_t wave_stride;        /* doubles between consecutive wavenumbers; 0 = dense (t_count * nl * LEC_NLEVRAW) */
    void* stream;
} lec_level_spec_args;
int lec_level_spec_ring(const lec_level_spec_args* args);
/*
 * lec_level_spec_ring with the boundary terms' triple products replaced too (--wavenumbers-budget; an additive call, ABI 11 unchanged):
 * besides what lec_level_spec_ring replaces, slots LEC_S_VTT, LEC_S_WTT, LEC_S_EV, LEC_S_EW (16, 17, 20, 21) of the record of row
 * (t, k, j) are  bspec_d[t][k][j][n][0..3]  of lec_rowspec_b_ring.  With lec_reduce's LEC_STAGE_VERTICAL over the (n, step) records the BAe
 * and BKe columns of the scalars are then BAe(n) and BKe(n); _handle_nans and the bottom-minus-top difference stay the totals'.  The
 * kernels are instantiations of their own of the same source: lec_level_spec_ring's results keep their bits, and every number of this
 * call that reads none of the four slots has lec_level_spec_ring's bits.  With bspec_d holding the records' own four slots for every
 * n the call reproduces lec_level_spec_ring bit for bit.
 * Validation: lec_level_spec_ring's, under this call's name; LEC_ERR_ARG also for a null bspec_d or one not 16-byte aligned.
 */
typedef struct lec_level_spec_b_args {
    lec_level_spec_args spec;   /* as lec_level_spec_ring takes it */
    const double* bspec_d;      /* [t_count][nl][nyb][n_wave][4], lec_rowspec_b_ring's; 16-byte aligned */
} lec_level_spec_b_args;
int lec_level_spec_b_ring(const lec_level_spec_b_args* args);

/*
 * -f [--periodic] --sections: the LATITUDE x PRESSURE SECTIONS of the ten terms of the cycle on one fixed box (an additive call: no
 * struct, export or kernel result of ABI 11 changes; lec_sections.hip is a code object of its own).
 *
 * The level stage of lec_reduce forms, for every row j of a (time step t, level k), the row's contribution to the per-level sums and
 * keeps only their cw-weighted sum over rows.  The section X_f(t, k, j) is that contribution itself -- the same source lines
 * (csrc/lec_level_row.inc) with cw = 1, then the level's divisor and sign -- with sigma READ from slot LEC_LEVRAW_SIGMA of levraw_d, so
 * it is the clamped sigma the totals used.  Names as in lec_level_row.inc, c1k = Rd / (p_k g):
 *   f = 0 Az  Ts Ts / (2 sigma)              1 Ae  sTT / (2 sigma)         2 Kz  mU^2 + mV^2           3 Ke  sUU + sVV
 *   4 Cz  -c1k Ws Ts                         5 Ca  -(sVT dphiTc / (2 Re sigma) + sWT dpT / sigma)
 *   6 Ck  c sUV / Re dphiUc + sVV / Re dphiV + tn sUU mV / Re + sWU dpU + sWV dpU              7 Ce  -c1k sWT
 *   8 Gz  Qs Ts / (cp sigma)                 9 Ge  sQT / (cp sigma)
 * so that sum_j cw_j X_f(t, k, j), cw_j = lattab2_d[j][0], is term f of the per-level table of (t, k).  The boundary terms have none.
 *   sec_d    [t_count][nl][LEC_NSECTION][nyb]  X_f(t, k, j): term-major, lanes over rows store consecutive doubles
 *   col_d    [t_count][LEC_NSECTION][nyb]      C_f(t, j) = s_f * trapezoid of X_f over the levels' pressures, s_f = 1 / (2 g) for Kz and
 *            Ke, 1 / g for Ck, else 1: on data without NaN sum_j cw_j C_f(t, j) is the step's scalar.  NaN rule, per (t, j, f), the
 *            vertical kernel's with drop_any_time = 0: interior NaN levels are bridged linearly in p, NaN levels at either end are left
 *            out, a column without a finite level is NaN (not the 0.0 of the totals' empty integral).  The totals' any-time mask is
 *            NOT applied (it is known only after the whole series), so with NaN levels the closure on the scalars is not claimed.
 *   secsum_d [nl][LEC_NSECTION][nyb]           += sum over the call's steps of X_f, added step by step in time order; the caller zeroes it
 *            once and divides by the number of steps: a NaN at any step makes the mean NaN.
 * With spec_d (a ring's records; qspec_d optional): the same for X_f^n, f in {Ae, Ke, Ca, Ce, Ck} (and Ge with qspec_d), n = 1 .. n_wave:
 * the same expression with slots 6 .. 13 of the record taken from spec_d[t][k][j][n - 1] (and slot 15 from qspec_d), lec_level_spec_ring's
 * definition of X(n).
 *   specsec_d    workspace [t_count][nl][n_wave][F][nyb], F = 5 (6 with qspec_d)
 *   speccolsum_d [n_wave][F][nyb]              += sum over the call's steps of the column value of X_f^n, in time order
 * Rows of the record buffer beyond the box's own (nyb > jn - js + 1) are written as NaN.  Every output element has ONE writer and the
 * time sums are added in time order: the numbers do not depend on the launch or on how a series is cut into calls, bit for bit.
 * Validation.  Every refusal names the field and is made before any HIP call, never clamped.  LEC_ERR_ARG: null args, rows_d, box_d,
 * lattab2_d, levtab2_d, levraw_d, sec_d, col_d, secsum_d; n_box != 1; t_count < 1, nl < 2, nyb < 2; n_wave < 0; reserved0 != 0; qspec_d
 * without spec_d; n_wave > 0 without spec_d, spec_d with n_wave < 1 or without specsec_d / speccolsum_d; rows_d, lattab2_d, spec_d not
 * 16-byte aligned.  LEC_ERR_UNSUPPORTED: nl > LEC_MAX_LEVELS, n_wave > LEC_MAX_WAVENUMBERS, (1 + n_wave) * t_count * nl >= 2^26 or
 * functions * nyb >= 2^32 - 64 (HIP takes fewer than 2^32 threads per launch; the caller chunks).
 */
#define LEC_NSECTION 10      /* Az Ae Kz Ke Cz Ca Ck Ce Gz Ge */
#define LEC_LEVRAW_SIGMA 33  /* the slot of a levraw record that holds the clamped static stability of (t, k) */
typedef struct lec_sections_args {
    const double* rows_d;       /* [t_count][nl][nyb][LEC_NSTAT], the chunk's row records; 16-byte aligned */
    int32_t t_count, nl;
    int32_t n_box, nyb;         /* n_box must be 1 */
    const int32_t* box_d;       /* [1][4] */
    const double* lattab2_d;    /* [nyb][8], as lec_reduce takes it; 16-byte aligned */
    const double* levtab2_d;    /* [nl][4] */
    const double* levraw_d;     /* [t_count][nl][LEC_NLEVRAW] as lec_reduce's level stage left it for these steps */
    double* sec_d;              /* out [t_count][nl][LEC_NSECTION][nyb] */
    double* col_d;              /* out [t_count][LEC_NSECTION][nyb] */
    double* secsum_d;           /* in/out [nl][LEC_NSECTION][nyb], accumulated */
    const double* spec_d;       /* [t_count][nl][nyb][n_wave][8] or NULL; 16-byte aligned */
    const double* qspec_d;      /* [t_count][nl][nyb][n_wave] or NULL */
    int32_t n_wave;             /* 0 without spec_d, else 1 .. LEC_MAX_WAVENUMBERS */
    int32_t reserved0;          /* must be 0 */
    double* specsec_d;          /* workspace [t_count][nl][n_wave][F][nyb] (with spec_d) */
    double* speccolsum_d;       /* in/out [n_wave][F][nyb], accumulated (with spec_d) */
    void* stream;
} lec_sections_args;
int lec_sections(const lec_sections_args* args);

/*
 * -f [--periodic] --maps: the LONGITUDE-RESOLVED MAPS of the six eddy terms Ae Ke Ca Ce Ck Ge on one fixed box (an additive call: no
 * struct, export or kernel result of ABI 11 changes; lec_maps.hip is a code object of its own).
 *
 * Every eddy term of stage 2 is the zonal average of a pointwise product times a factor of (time step t, level k, box row j) only; the
 * map is the same expression with the zonal average left off, at box column i.  Primes are deviations from the row's zonal means, which
 * are READ from the row record (slots LEC_S_MT / MU / MV / MW / MQ), never formed again; sigma is READ from slot LEC_LEVRAW_SIGMA of
 * levraw_d; dphiTc, dphiUc, dphiV, dpT, dpU are the row factors of csrc/lec_level_row.inc (from the records of rows j +- 1 and levels
 * k +- 1 and the area means), c1k = Rd / (p_k g), c / tn / mV the row's cos, tan and [v]:
 *   f = 0 Ae  T'T' / (2 sigma)        1 Ke  u'u' + v'v'        2 Ca  -(v'T' dphiTc / (2 Re sigma) + w'T' dpT / sigma)        3 Ce  -c1k w'T'
 *   4 Ck  c u'v' / Re dphiUc + v'v' / Re dphiV + tn u'u' mV / Re + w'u' dpU + w'v' dpU                      5 Ge  Q'T' / (cp sigma)
 * (the factor of a product is formed ONCE per (t, k, j) and multiplied in: the zonal average of a map row equals the section's value to
 * rounding, not bit for bit).  Q = cp (dT/dt + u dT/dx + v dT/dy - S w) at the point, the expression of lec_rowspec_q_ring and of
 * lec_rowstats: tables and time axis as there; d/dlon centred with wrapped neighbours when ring = 1, and one-sided, 2 (T[i+1] - T[i]) /
 * 2 (T[i] - T[i-1]), at the first / last column of an open box (ring = 0).  Nothing outside the box, the levels or the cube's steps is read.
 *   col_d    [t_count][LEC_NMAP][nyb][nxb]  C_f(t, j, i) = s_f * trapezoid of the integrand over the levels' pressures, s_f = 1 / (2 g) for
 *            Ke, 1 / g for Ck, else 1, with lec_sections' NaN rule per (t, j, i): interior NaN levels are bridged linearly in p, NaN levels
 *            at either end are left out, a column without a finite level is NaN.  The caller's to keep, and the workspace of the sums.
 *   mapsum_d [LEC_NMAP][nyb][nxb]           += sum over the call's steps of C_f, added step by step in time order; the caller zeroes it
 *            once and divides by the number of steps: a NaN at any step makes the mean NaN.
 *   hov_d    [t_count][LEC_NMAP][nxb]       H_f(t, i) = sum_j cw_j C_f(t, j, i), rows ascending, cw_j = lattab2_d[j][0]; NaN propagates.
 *   coef_d   workspace [t_count][nl][nyb][LEC_MAPS_NCOEF]: the zonal means and factors of (t, k, j), written by the call's first kernel.
 * nyb = jn - js + 1, nxb = ie - iw + 1; rows_d has exactly nyb rows per level.  On data without NaN the box's zonal average of
 * C_f(t, j, .) (closed on a ring, the half-weight trapezoid on an open box) is lec_sections' col_d of that term, and that of H_f(t, .)
 * the step's scalar.  Every output element has ONE writer and the sums run in a fixed order: no atomics, and the numbers depend neither
 * on the launch nor on how a series is cut into calls, bit for bit.
 * Validation.  Every refusal names the field and is made before any HIP call, never clamped.  LEC_ERR_ARG: null args or any null
 * pointer; dtype; ring not 0 / 1, or ring = 1 with iw .. ie not 0 .. nx - 1; reserved0 != 0; nt < 2, nl < 2, ny < 2, nx < 3; t_begin /
 * t_count outside the cube; iw / ie / js / jn outside 0 <= iw, iw + 2 <= ie < nx, 0 <= js < jn < ny; rows_d, lattab2_d, coef_d not
 * 16-byte aligned, another table or output not 8-byte aligned, a cube not aligned to its element.  LEC_ERR_UNSUPPORTED: nl >
 * LEC_MAX_LEVELS, t_count * nl >= 2^26, t_count * nyb * ceil(nxb / 64) >= 2^26, 6 * nyb * nxb or t_count * 6 * nxb >= 2^32 - 256 (HIP
 * takes fewer than 2^32 threads per launch; the caller chunks).
 */
#define LEC_NMAP 6           /* Ae Ke Ca Ce Ck Ge */
#define LEC_MAPS_NCOEF 16    /* doubles per (t, k, j) of coef_d */
typedef struct lec_maps_args {
    const void* tair_d;
    const void* u_d;
    const void* v_d;
    const void* omega_d;
    int32_t dtype;              /* enum lec_dtype (LEC_F64 or LEC_F32), common to the four cubes */
    int32_t nt, nl, ny, nx;     /* cube dimensions */
    int32_t t_begin, t_count;   /* process time steps [t_begin, t_begin + t_count) */
    int32_t iw, ie, js, jn;     /* the box (inclusive grid columns and rows) */
    int32_t ring;               /* 1: the box is the closed circle 0 .. nx - 1; 0: an open box */
    int32_t reserved0;          /* must be 0 */
    const double* rows_d;       /* [t_count][nl][nyb][LEC_NSTAT], the records of the same steps and box; 16-byte aligned */
    const double* levraw_d;     /* [t_count][nl][LEC_NLEVRAW] as lec_reduce's level stage left it for these steps */
    const double* lattab2_d;    /* [nyb][8], as lec_reduce takes it; 16-byte aligned */
    const double* levtab2_d;    /* [nl][4] */
    const double* lattab_d;     /* [nyb][4]: d/dlat a, b, c; 1 / dx_j (the box's lattab) */
    const double* levtab_d;     /* [nl][3]: the static-stability coefficients of lec_rowstats */
    const double* tcoef_d;      /* [nt][3]: np.gradient coefficients over the cube's time axis */
    double inv_hdeg;            /* boxtab[2] of the box: 1 / (longitude step in degrees) */
    double* coef_d;             /* workspace [t_count][nl][nyb][LEC_MAPS_NCOEF]; 16-byte aligned */
    double* col_d;              /* out [t_count][LEC_NMAP][nyb][nxb] */
    double* mapsum_d;           /* in/out [LEC_NMAP][nyb][nxb], accumulated */
    double* hov_d;              /* out [t_count][LEC_NMAP][nxb] */
    void* stream;
} lec_maps_args;
int lec_maps(const lec_maps_args* args);

int lec_ingest(const lec_ingest_args* args);
/*
 * lec_ingest for a series that continues across files (ABI 11, additive; lec_ingest_args unchanged): every file packs its values with
 * its own scale_factor / add_offset / fill value, so the steps src_d holds may differ in all three.
 *   - pack_d[s] = {scale_factor, add_offset, fill_value} of SOURCE step s of src_d, fp64, in device memory.  s = 0 is the first step
 *     src_d holds: with step_d that is the step step_base, and output step t takes row step_d[t][0] - step_base; without step_d output
 *     step t takes row t.
 *   - pack_len: rows of pack_d.  It must be nt_src when step_d is given, else nt; anything else, or pack_d == NULL, is LEC_ERR_ARG,
 *     said before any launch.
 *   - args->scale_factor / add_offset / fill_value are ignored.  has_packing, has_fill, decode_dtype, unit_scale, the maps and the
 *     bounds rule of step_d apply as in lec_ingest: one series has one decode dtype, because the PRESENCE of the attributes decides it.
 *     An out-of-range step_d entry writes NaN rows and reads neither the source nor the table.
 *   - The arithmetic is lec_ingest's, operation by operation (contraction off; the fill comparison is against that step's fill value,
 *     before scaling): a table whose rows are all equal gives lec_ingest's bits.  The three constants are uniform per workgroup (the
 *     source step follows from blockIdx and step_d) and are fetched once per workgroup: 24 bytes more traffic per output row.
 */
int lec_ingest_series(const lec_ingest_args* args, const double* pack_d, int32_t pack_len);
int lec_reduce(const lec_reduce_args* args);

/* The any-time NaN-level mask of the time steps in `args` alone -> dropmask_d (zeroed first; non-zero = drop).
 * Uses am_d / levraw_d as workspace (stage LEC_STAGE_VERTICAL: reads levraw_d as given); scalars_d, levels_d, nanflag_d are not
 * touched and may be NULL.
 * For series processed in shards or chunks: merge the masks, then call lec_reduce with drop_any_time = 2. */
int lec_dropmask(const lec_reduce_args* args);

int lec_track_diag(const lec_diag_args* args);
int lec_follow(const lec_follow_args* args);
int lec_follow_seeds(const lec_follow_seeds_args* args);
int lec_follow_many(const lec_follow_many_args* args);
int lec_follow_seeds_series(const lec_follow_seeds_series_args* args);
int lec_follow_spans(const lec_follow_spans_args* args);
int lec_follow_spans_chunk(const lec_follow_chunk_args* args);

/*
 * What the library cannot see at launch: indices that live in DEVICE memory.  lec_rowstats validates every scalar argument, but a
 * quadruple of box_d outside [0, nx) x [0, ny), with ie < iw + 1 / jn < js + 1, or wider / higher than nxb_max / nyb_max would be
 * an out-of-bounds read; likewise an entry of the three ingest maps outside the source extents.  The Python host checks its boxes
 * before it uploads them (tables.box_indices; the reference validates its box the same way, lec_fixed_framework.py:98-154); a
 * plain-C caller calls these first.  One small kernel on args->stream scans the table(s), the call WAITS for it (the only
 * synchronous entry points) and returns LEC_OK, or LEC_ERR_ARG with the first offending entry in lec_last_error().
 * status_d: caller-owned device scratch of 4 int32.
 */
int lec_check_boxes(const lec_rowstats_args* args, int32_t* status_d);
int lec_check_maps(const lec_ingest_args* args, int32_t* status_d);

/*
 * Host-memory plumbing of the device ingest: move file bytes to the GPU WITHOUT a staging copy.  The reference reads its file
 * through xarray into NumPy memory (src/utils/preprocessing.py:35-146); here a span of the memory-mapped file (or of any host
 * array) is registered with the HIP runtime -- its pages are pinned and mapped for the copy engines --, the rows a chunk needs are
 * copied from it asynchronously, and the span is unregistered once the copies have completed (the caller synchronises on them
 * first and keeps the bookkeeping: registered spans must not overlap).
 *   lec_host_register    ptr / bytes: page-aligned span of host memory (read-only file mappings are fine)
 *   lec_host_unregister  the pointer a span was registered with
 *   lec_copy_rows_async  `rows` rows of `width_bytes`, source rows `src_pitch` bytes apart (host), destination rows `dst_pitch` apart
 *                        (device), on `stream`; rows == 1 or both pitches == width: one linear copy.  Truly asynchronous only from
 *                        registered (or pinned) memory.
 * Return LEC_OK, LEC_ERR_ARG, or LEC_ERR_LAUNCH with the runtime's message when HIP refuses (the Python host then falls back to its
 * pinned staging buffers).
 */
int lec_host_register(const void* ptr, size_t bytes);
int lec_host_unregister(const void* ptr);
int lec_copy_rows_async(void* dst_d, size_t dst_pitch, const void* src_h, size_t src_pitch, size_t width_bytes, size_t rows, void* stream);

/*
 * Deflated NetCDF-4 input on the device.  The reference reads such files through netCDF4 / HDF5, which inflate every chunk on one
 * host thread (src/utils/preprocessing.py:35-146 -> xr.open_dataset); here the compressed chunks cross the link as they lie in
 * the file and the GPU inflates them, one wave per chunk:
 *   lec_inflate        n_streams independent zlib streams (RFC 1950 / 1951: stored, fixed and dynamic blocks) -> their
 *                      inflated bytes.  desc_d[s] = {byte offset of the stream in src_d (any), its size, byte offset of
 *                      its output in dst_d (a multiple of 16), the output's exact size}; a NEGATIVE size marks |size| bytes that are
 *                      not compressed (HDF5 stores a chunk as it is when deflate does not pay) and are copied.  src_bytes is the size of the src_d
 *                      allocation (the kernel reads whole dwords: it may touch up to 512 bytes after a stream's end, never beyond
 *                      src_bytes).  status_d[s] = {code, deflate block, output position, input bit position}; code 0 = ok, anything
 *                      else names what was wrong with the stream (lec_inflate_status_text); zlib's Adler-32 trailer is verified against the
 *                      inflated data, HDF5's Fletcher-32 of the compressed bytes when flags says the chunks carry one.
 *                      Asynchronous like every other entry point: the caller reads status_d after synchronising.
 *   lec_chunk_scatter  the payloads of n_chunks HDF5 chunks (each ct x ck x cj x ci elements of elem_size bytes, all of one
 *                      variable; shuffled = 1: the HDF5 shuffle filter's byte planes, undone here) -> a contiguous array
 *                      [nt][nl][ny][nx] of raw elements, which lec_ingest then decodes.  chunk_d[c] = {byte offset of the payload
 *                      in src_d, the chunk's origin in FILE coordinates t, k, j, i}; file step t lands in output step
 *                      tmap_d[t - t_base], file level k in output level kmap_d[k] (either < 0: not wanted), file row j in output
 *                      row j - j0, column i in column i; whatever falls outside the output (edge chunks are padded) is skipped.
 */
typedef struct lec_inflate_args {
    const void* src_d;
    int64_t src_bytes;
    const int64_t* desc_d;      /* [n_streams][4] */
    int32_t n_streams;
    int32_t flags;              /* bit 0: every stream is followed by 4 bytes of HDF5 Fletcher-32 over its bytes (filter 3): verified first;
                                   bit 1: a hint -- matches rarely reach more than 3 KB back (byte-shuffled rows of < 3000 elements): a 4 KiB
                                   instead of an 8 KiB history ring in LDS, 18 instead of 12 streams per CU; any stream still inflates */
    void* dst_d;
    int32_t* status_d;          /* [n_streams][4] */
    void* stream;
    int64_t dst_bytes;          /* size of the dst_d allocation (ABI 8): a descriptor whose output offset is negative, not a multiple of 16, or
                                   whose output does not end inside dst_d gets the status "size" and nothing of it is written */
} lec_inflate_args;

typedef struct lec_chunk_scatter_args {
    const void* src_d;
    const int64_t* chunk_d;     /* [n_chunks][5] */
    int32_t n_chunks, elem_size, shuffled, reserved0;
    int32_t ct, ck, cj, ci;
    int32_t t_base, n_tmap, n_kmap, j0;
    const int32_t* tmap_d;      /* [n_tmap] */
    const int32_t* kmap_d;      /* [n_kmap] */
    int32_t nt, nl, ny, nx;
    void* out_d;
    void* stream;
    int64_t src_bytes;          /* size of the src_d allocation (ABI 8): a chunk whose payload does not lie inside it is skipped */
} lec_chunk_scatter_args;

int lec_inflate(const lec_inflate_args* args);
const char* lec_inflate_status_text(int code);
int lec_chunk_scatter(const lec_chunk_scatter_args* args);

/*
 * dT/dt of a box-packed series as a cube of its own: out[s][e] = tc[s][0] tm[s][e] + tc[s][1] t[s][e] + tc[s][2] tp[s][e] in fp64, evaluated
 * exactly as lec_rowstats evaluates it per point from tm_d / tp_d (the two outer products rounded, then one fused multiply-add), so a
 * series handed over as T, u, v, omega, Phi + this cube (dTdt_d) gives the records of the same series handed over with tm_d / tp_d,
 * bit for bit -- with one streamed operand fewer per point (fp64 storage: 48 instead of 56 bytes; the producer reads its three T
 * slices once).  Replaces, for a moving box, the np.gradient over time of run_lec_analysis (lorenzcycletoolkit.py:184-186) restricted
 * to each step's box.  `dtype` is the cubes' (LEC_F64 / LEC_F32); the output is fp64 (as a dTdt_d of lec_rowstats it serves fp64 storage).
 */
typedef struct lec_dtdt_args {
    const void* tm_d;          /* [n_steps][step_elems] T of the previous time step on the step's box */
    const void* t_d;           /* T */
    const void* tp_d;          /* T of the next time step */
    int32_t dtype, n_steps;
    int64_t step_elems;        /* elements per time step (nl * ny * nx of the packed slabs) */
    const double* tcoef_d;     /* [n_steps][3] np.gradient coefficients of the steps these cubes hold */
    double* out_d;             /* [n_steps][step_elems] fp64 */
    void* stream;
} lec_dtdt_args;
int lec_dtdt(const lec_dtdt_args* args);

/*
 * The text of a per-level table (HOST memory in, host memory out; no device work).  Replaces the per-cell formatting inside
 * `_save_vertical_levels` (src/analysis/conversion_terms.py:287-308 and its copies in energy_contents.py,
 * generation_and_dissipation_terms.py: DataFrame.to_csv(mode="a", header=None)) for the 21 tables of a series: `rows` lines, each
 * `labels + r * label_len` (label_len bytes: the time stamp as the reference prints it), then for each of the `cols` values of the row
 * (`row_stride` doubles from one row to the next) a ',' and the value as Python's repr(float) -- shortest round-trip digits,
 * positional for 1e-4 <= |x| < 1e16 with at least ".0", else d[.ddd]e[+-]XX --, NaN as an empty field (pandas' na_rep), and '\n'.
 * Byte for byte what pandas writes for float64 columns.  `out` must hold rows * (label_len + 27 * cols + 1) bytes.
 * Returns the number of bytes written, or -1 (text via lec_last_error()).
 */
long long lec_format_csv_rows(const double* values, long long rows, long long cols, long long row_stride,
                              const char* labels, int label_len, char* out, long long cap);

#ifdef __cplusplus
}
#endif
#endif /* LEC_HIP_H */
