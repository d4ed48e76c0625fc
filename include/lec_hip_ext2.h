/*
 * lec_hip_ext2.h -- calls of liblec_hip.so that came after include/lec_hip_ext.h was closed.
 *
 * include/lec_hip.h is the library's ABI 11 and include/lec_hip_ext.h its first addition; the tests pin both surfaces.  A call declared
 * HERE is exported from the same liblec_hip.so, is an addition to those surfaces (no struct, export or kernel result of theirs changes
 * with it) and is bound in lorenzcycletoolkit_amd/_lib.py under EXT2_EXPORTS.  Error codes and lec_last_error() are lec_hip.h's.
 */
#ifndef LEC_HIP_EXT2_H
#define LEC_HIP_EXT2_H

#include "lec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * -t / -c --composite-sections: the SYSTEM-RELATIVE latitude x pressure sections of the ten terms Az Ae Kz Ke Cz Ca Ck Ce Gz Ge over a
 * series of per-step boxes that all have nyb ROWS (csrc/lec_composite_sections.hip, a code object of its own).
 *
 * The moving framework has one box per time step, which follows a system; the boxes share no grid rows, but they share their
 * BOX-RELATIVE row index j = 0 .. nyb - 1 from the box's southern edge.  The call is lec_sections (lec_hip.h) on that index with three
 * things taken PER STEP: the box (box_d + 4 t), the latitude table (lattab2_d + t * nyb * 8) and with it the area means, formed with step
 * t's cw.  Definitions, integrands, divisors and signs are lec_sections': X_f(t, k, j) is the factor of cw_j in the per-level sum of
 * lec_reduce's level stage (csrc/lec_level_row.inc, part A, with cw = 1 on zeroed sums), sigma is READ from slot LEC_LEVRAW_SIGMA of
 * step t's levraw record.  Only row records are read, never a field cube: the call needs the boxes' ROW COUNT to be common, their widths
 * may differ from step to step (a row record holds the zonal means over its own box's width).  There is no spectral input: spectra do
 * not exist for open, moving boxes.
 *
 * Layouts (step s of the call uses box s, table s, records s):
 *   rows_d    [t_count][nl][nyb][LEC_NSTAT], levraw_d [t_count][nl][LEC_NLEVRAW]: stage 1's records and the level stage's records of the
 *             same steps (exactly nyb rows per level).
 *   box_d     [t_count][4] {iw, ie, js, jn} as the cubes hold them (lec_rowstats' contract; only jn - js + 1 is used).  box_h is the HOST
 *             copy of the same table: every box must have exactly nyb rows, which is checked on box_h before any HIP call (LEC_ERR_ARG
 *             names the first step that differs and both row counts).  The kernels read box_d only; the caller keeps the two equal.
 *   lattab2_d [t_count][nyb][8], as lec_reduce takes it for per-step boxes.
 *   levtab2_d [nl][4], as lec_sections takes it.
 * Outputs:
 *   sec_d     [t_count][nl][LEC_NSECTION][nyb]  X_f(t, k, j), term-major.  The caller's to keep, and the workspace of the sums.
 *   col_d     [t_count][LEC_NSECTION][nyb]      C_f(t, j) = s_f * trapezoid of X_f over the levels' pressures, s_f = 1 / (2 g) for Kz and
 *             Ke, 1 / g for Ck, else 1, with lec_sections' NaN rule per (t, j): interior NaN levels are bridged linearly in p, NaN levels
 *             at either end are left out, a column without a finite level is NaN.
 *   secsum_d  [nl][LEC_NSECTION][nyb]           += sum over the call's steps of X_f, added step by step in time order; the caller zeroes it
 *             once and divides by the number of steps: a NaN at any step makes the mean NaN.
 * On data without NaN sum_j cw_j(t) X_f(t, k, j), cw_j(t) = lattab2_d[t][j][0], is step t's per-level value of the moving framework and
 * sum_j cw_j(t) C_f(t, j) its scalar, to rounding.  Every output element has ONE writer and the sums run in a fixed order: no atomics,
 * and the numbers depend neither on the launch nor on how a series is cut into calls, bit for bit.
 *
 * Validation.  Every refusal names the field, starts with "lec_composite_sections:" and is made before any HIP call, never clamped.
 * LEC_ERR_ARG: null args; a null rows_d, levraw_d, box_h, box_d, lattab2_d, levtab2_d, sec_d, col_d or secsum_d; t_count < 1, nl < 2,
 * nyb < 2; reserved0 != 0; rows_d or lattab2_d not 16-byte aligned; a box of box_h that does not have nyb rows.  LEC_ERR_UNSUPPORTED:
 * nl > LEC_MAX_LEVELS, t_count * nl >= 2^26, LEC_NSECTION * nyb >= 2^32 - 64 (HIP takes fewer than 2^32 threads per launch; the caller
 * chunks).
 */
typedef struct lec_composite_sections_args {
    const double* rows_d;       /* [t_count][nl][nyb][LEC_NSTAT]; 16-byte aligned */
    const double* levraw_d;     /* [t_count][nl][LEC_NLEVRAW] as lec_reduce's level stage left it for these steps */
    int32_t t_count, nl;
    int32_t nyb;                /* the row count of EVERY box, and of the record buffer */
    int32_t reserved0;          /* must be 0 */
    const int32_t* box_h;       /* HOST [t_count][4] iw ie js jn: the row counts are checked before any HIP call */
    const int32_t* box_d;       /* device copy of box_h */
    const double* lattab2_d;    /* [t_count][nyb][8]; 16-byte aligned */
    const double* levtab2_d;    /* [nl][4] */
    double* sec_d;              /* out [t_count][nl][LEC_NSECTION][nyb] */
    double* col_d;              /* out [t_count][LEC_NSECTION][nyb] */
    double* secsum_d;           /* in/out [nl][LEC_NSECTION][nyb], accumulated */
    void* stream;
} lec_composite_sections_args;
int lec_composite_sections(const lec_composite_sections_args* args);

#ifdef __cplusplus
}
#endif

#endif
