/*
 * lec_hip_ext3.h -- calls of liblec_hip.so that came after include/lec_hip_ext2.h was closed.
 *
 * include/lec_hip.h is the library's ABI 11, include/lec_hip_ext.h and include/lec_hip_ext2.h its first two additions; the tests pin the
 * three surfaces.  A call declared HERE is exported from the same liblec_hip.so, is an addition to those surfaces (no struct, export or
 * kernel result of theirs changes with it) and is bound in lorenzcycletoolkit_amd/_lib.py under EXT3_EXPORTS.  Error codes, the dtype
 * enum and lec_last_error() are lec_hip.h's.
 */
#ifndef LEC_HIP_EXT3_H
#define LEC_HIP_EXT3_H

#include "lec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * -t --trackfiles / -c --choose-systems --batch-composites: the SYSTEM-RELATIVE COMPOSITES of the six eddy terms Ae Ke Ca Ce Ck Ge of a
 * BATCH of tracks over one union cube (csrc/lec_composite_steps.hip, a code object of its own).
 *
 * The call is lec_composite (lec_hip_ext.h) with each box's cube step taken from a step table, as lec_rowstats_steps takes it, and the
 * time sums kept per SEGMENT of the call's boxes (a segment = the boxes of one track that the call holds).  Definitions, factors, Q, the
 * open box's one-sided d/dlon and the NaN rule are lec_composite's; what differs:
 *   Cubes      [nt][nl][ny][nx], unpacked only: there is no dTdt_d, tm_d or tp_d.
 *   step_d     device int32 [s_count][3] {t, t_prev, t_next}, ABSOLUTE cube steps (lec_rowstats_steps' table).  Box s reads cube step
 *              step[s][0]; dT/dt = stencil3(tc[0], T[t_prev], tc[2], T[t_next], tc[1], T[t]) with tc = tcoef_d[s] -- [s_count][3], indexed
 *              by the BOX --, the expression and fma form of lec_composite's "cube's own neighbours" source, so a track's numbers are
 *              those of lec_composite on a cube that holds the track's own steps, bit for bit.  step_h is the HOST copy: every entry
 *              must lie in [0, nt), which is checked on step_h before any HIP call (LEC_ERR_ARG names the box and the entry).  The
 *              kernel reads step_d only and still reads NOTHING of the cubes for a box with an entry outside [0, nt): that box's columns
 *              are written as NaN.
 *   box_h / box_d [s_count][4], boxtab_d [s_count][4], lattab_d [s_count][nyb][4], lattab2_d [s_count][nyb][8], rows_d
 *              [s_count][nl][nyb][LEC_NSTAT], levraw_d [s_count][nl][LEC_NLEVRAW]: per box, exactly as lec_composite takes them per step.
 *              Every box is nyb x nxb and lies inside the cube (checked on box_h).
 *   seg_h / seg_d int32 [n_seg + 1]: ascending offsets into the call's boxes, seg[0] = 0, seg[n_seg] = s_count, no empty segment.
 * Outputs:
 *   col_d      [s_count][LEC_NMAP][nyb][nxb], hov_d [s_count][LEC_NMAP][nxb], coef_d (workspace [s_count][nl][nyb][LEC_MAPS_NCOEF]): per
 *              box, as lec_composite's per step.
 *   mapsum_d   [n_seg][LEC_NMAP][nyb][nxb], in/out: the columns of segment g's boxes are added to mapsum_d[g] one by one in table order,
 *              starting from the value found there -- a plain running sum, so a track cut over several calls has the bits of one call.
 * One thread per (g, f, j, i) and per output element: ONE writer each, no atomics.
 *
 * Validation, before any HIP call, never clamped; every message starts with "lec_composite_steps:".  LEC_ERR_ARG: lec_composite's
 * refusals of the fields the two calls share (s_count in the place of t_count; nt >= 1); a null step_h, step_d, seg_h, seg_d or tcoef_d;
 * step_h / step_d / seg_h / seg_d not 4-byte aligned; an entry of step_h outside [0, nt); n_seg < 1; seg_h[0] != 0; offsets that do not
 * ascend strictly (an empty segment); seg_h[n_seg] != s_count.  LEC_ERR_UNSUPPORTED: lec_composite's limits, and
 * n_seg * 6 * nyb * nxb >= 2^32 - 256.
 */
typedef struct lec_composite_steps_args {
    const void* tair_d;
    const void* u_d;
    const void* v_d;
    const void* omega_d;
    int32_t dtype;              /* enum lec_dtype (LEC_F64 or LEC_F32), common to the four cubes */
    int32_t nt, nl, ny, nx;     /* cube dimensions */
    int32_t s_count;            /* boxes of the call */
    int32_t nyb, nxb;           /* the shape of EVERY box: rows, columns */
    int32_t n_seg;              /* segments of the call's boxes */
    int32_t reserved0;          /* must be 0 */
    const int32_t* step_h;      /* HOST [s_count][3] {t, t_prev, t_next}: checked before any HIP call */
    const int32_t* step_d;      /* device copy of step_h */
    const int32_t* seg_h;       /* HOST [n_seg + 1] offsets into the boxes: checked before any HIP call */
    const int32_t* seg_d;       /* device copy of seg_h */
    const int32_t* box_h;       /* HOST [s_count][4] iw ie js jn in the cube: checked before any HIP call */
    const int32_t* box_d;       /* device copy of box_h */
    const double* boxtab_d;     /* [s_count][4]: [2] = 1 / h_deg of the box */
    const double* lattab_d;     /* [s_count][nyb][4] */
    const double* lattab2_d;    /* [s_count][nyb][8]; 16-byte aligned */
    const double* rows_d;       /* [s_count][nl][nyb][LEC_NSTAT]; 16-byte aligned */
    const double* levraw_d;     /* [s_count][nl][LEC_NLEVRAW] as lec_reduce's level stage left it for these boxes */
    const double* levtab_d;     /* [nl][3] */
    const double* levtab2_d;    /* [nl][4] */
    const double* tcoef_d;      /* [s_count][3], by box */
    double* coef_d;             /* workspace [s_count][nl][nyb][LEC_MAPS_NCOEF]; 16-byte aligned */
    double* col_d;              /* out [s_count][LEC_NMAP][nyb][nxb] */
    double* mapsum_d;           /* in/out [n_seg][LEC_NMAP][nyb][nxb], accumulated per segment */
    double* hov_d;              /* out [s_count][LEC_NMAP][nxb] */
    void* stream;
} lec_composite_steps_args;
int lec_composite_steps(const lec_composite_steps_args* args);

/*
 * The per-track means and the ENSEMBLE mean of K tracks' composites (same file): with mapsum_d [K][LEC_NMAP][nyb][nxb] as
 * lec_composite_steps left it and count[k] >= 1 the number of steps of track k,
 *   mean_d[k] = mapsum_d[k] * (1.0 / (double)count[k])            (mean_d may alias mapsum_d).  The rounded reciprocal, then one product:
 *               what the engine's division of a single track's sum by its step count, a host scalar, evaluates to -- so a track's
 *               mean has the bits of its own lec_composite run.  It can differ from the quotient in the last bit.
 *   ens_d     = (mean_d[0] + mean_d[1] + ... + mean_d[K - 1]) / K  [LEC_NMAP][nyb][nxb], tracks ascending, starting from mean_d[0];
 *               the IEEE quotient
 * One thread per point (f, j, i); NaN propagates.  count_h is the HOST copy of count_d, checked before any HIP call.
 * LEC_ERR_ARG ("lec_composite_ensemble: ..."): null args, mapsum_d, mean_d, ens_d, count_h or count_d; n_track < 1, nyb < 1, nxb < 1;
 * reserved0 != 0; a count below 1 (the message names the track); a table not 8-byte, a count table not 4-byte aligned.
 * LEC_ERR_UNSUPPORTED: 6 * nyb * nxb >= 2^32 - 256.
 */
typedef struct lec_composite_ensemble_args {
    const double* mapsum_d;     /* [n_track][LEC_NMAP][nyb][nxb] */
    const int32_t* count_h;     /* HOST [n_track]: steps per track, each >= 1 */
    const int32_t* count_d;     /* device copy of count_h */
    int32_t n_track, nyb, nxb;
    int32_t reserved0;          /* must be 0 */
    double* mean_d;             /* out [n_track][LEC_NMAP][nyb][nxb]; may be mapsum_d */
    double* ens_d;              /* out [LEC_NMAP][nyb][nxb] */
    void* stream;
} lec_composite_ensemble_args;
int lec_composite_ensemble(const lec_composite_ensemble_args* args);

#ifdef __cplusplus
}
#endif

#endif
