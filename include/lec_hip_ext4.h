/*
 * lec_hip_ext4.h -- calls of liblec_hip.so that came after include/lec_hip_ext3.h was closed.
 *
 * include/lec_hip.h is the library's ABI 11, include/lec_hip_ext.h, lec_hip_ext2.h and lec_hip_ext3.h its additions; the tests pin those
 * surfaces.  A call declared HERE is exported from the same liblec_hip.so, is an addition to them (no struct, export or kernel result of
 * theirs changes with it) and is bound in lorenzcycletoolkit_amd/_lib.py under EXT4_EXPORTS.  Error codes, lec_last_error() and the dtype
 * enum are lec_hip.h's.
 */
#ifndef LEC_HIP_EXT4_H
#define LEC_HIP_EXT4_H

#include "lec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * -f [--periodic] --lon-sections and -t / -c --composite-lon-sections: the LONGITUDE x PRESSURE sections of the six eddy terms Ae Ke Ca Ce
 * Ck Ge (csrc/lec_lonsections.hip, a code object of its own).
 *
 * Let Y_f(t, k, j, i) be the point integrand of lec_maps (lec_hip.h) / lec_composite (lec_hip_ext.h): the same primes (deviations from the
 * row's zonal means READ from the row records), the same factors of (t, k, j) (the coefficient record [t][nl][nyb][LEC_MAPS_NCOEF], written
 * by the same first kernel), sigma READ from slot LEC_LEVRAW_SIGMA of the levraw record, Q the expression and fma form of lec_rowstats with
 * the same d/dlon rule (wrapped on a ring, one-sided at the first and last column of an open box: nothing outside the box is read).  Where
 * those calls integrate Y_f over pressure and keep the rows, these sum it over the rows and keep the levels:
 *   lonsec_d    [t_count][LEC_NMAP][nl][nxb]  X_f(t, k, i) = sum_j cw_j(t) Y_f(t, k, j, i): the rows ascending in a plain running sum that
 *               starts from 0.0, contraction off; cw_j(t) = lattab2_d[j][0] (lec_lonsections) or lattab2_d[t][j][0], the step's own
 *               (lec_composite_lonsections).  The units of lec_sections' X_f: no 1 / g or 1 / (2 g) is applied.  NaN propagates as the sum
 *               evaluates; a NaN point makes its level NaN at every column, through the row's zonal mean.  The caller's to keep, and the
 *               workspace of the time sums.
 *   lonsecsum_d [LEC_NMAP][nl][nxb]           += sum over the call's steps of X_f, added step by step in time order; the caller zeroes it
 *               once and divides by the number of steps: a NaN at any step makes the mean NaN.
 *   coef_d      workspace [t_count][nl][nyb][LEC_MAPS_NCOEF], as lec_maps takes it.
 * On data without NaN the box's own zonal average of X_f(t, k, .) is sum_j cw_j times lec_sections' X_f(t, k, j), and s_f times the
 * trapezoid of X_f(t, ., i) over the levels' pressures (s_f = 1 / (2 g) for Ke, 1 / g for Ck, else 1) is the Hovmoeller row hov_d[t][f][i]
 * of lec_maps / lec_composite, each to rounding.  Every output element has ONE writer and the sums run in a fixed order: no atomics, and
 * the numbers depend neither on the launch nor on how a series is cut into calls, bit for bit.
 *
 * lec_lonsections serves ONE fixed box: every other field is lec_maps_args' and means what it means there (ring: lambda wraps and the box
 * is the whole circle; dT/dt over the cube's own time axis by tcoef_d).
 *
 * Validation.  Every refusal names the field, starts with "lec_lonsections:" and is made before any HIP call, never clamped.  LEC_ERR_ARG:
 * null args; a null tair_d, u_d, v_d, omega_d, rows_d, levraw_d, lattab2_d, levtab2_d, lattab_d, levtab_d, tcoef_d, coef_d, lonsec_d or
 * lonsecsum_d; dtype; ring not 0 / 1; reserved0 != 0; nt < 2, nl < 2, ny < 2, nx < 3; t_begin / t_count outside the cube; iw, ie, js, jn
 * outside the cube, fewer than 3 columns (ie - iw + 1) or 2 rows (jn - js + 1), a ring that is not 0 .. nx - 1; rows_d, lattab2_d, coef_d
 * not 16-byte aligned, another table or output not 8-byte aligned, a cube not aligned to its element.  LEC_ERR_UNSUPPORTED:
 * nl > LEC_MAX_LEVELS, t_count * nl * ceil(nxb / 64) >= 2^26, 6 * nl * nxb >= 2^32 - 256 (HIP takes fewer than 2^32 threads per launch; the
 * caller chunks).
 */
typedef struct lec_lonsections_args {
    const void* tair_d;
    const void* u_d;
    const void* v_d;
    const void* omega_d;
    int32_t dtype;              /* enum lec_dtype (LEC_F64 or LEC_F32), common to the four cubes */
    int32_t nt, nl, ny, nx;     /* cube dimensions */
    int32_t t_begin, t_count;   /* process cube steps [t_begin, t_begin + t_count) */
    int32_t iw, ie, js, jn;     /* the box, inclusive grid indices */
    int32_t ring;               /* 1: the box is the whole circle 0 .. nx - 1 and lambda wraps */
    int32_t reserved0;          /* must be 0 */
    const double* rows_d;       /* [t_count][nl][nyb][LEC_NSTAT]; 16-byte aligned */
    const double* levraw_d;     /* [t_count][nl][LEC_NLEVRAW] as lec_reduce's level stage left it for these steps */
    const double* lattab2_d;    /* [nyb][8], as lec_reduce takes it; 16-byte aligned */
    const double* levtab2_d;    /* [nl][4] */
    const double* lattab_d;     /* [nyb][4]: d/dlat a, b, c; 1 / dx_j */
    const double* levtab_d;     /* [nl][3] */
    const double* tcoef_d;      /* [nt][3] */
    double inv_hdeg;            /* 1 / h_deg of the box */
    double* coef_d;             /* workspace [t_count][nl][nyb][LEC_MAPS_NCOEF]; 16-byte aligned */
    double* lonsec_d;           /* out [t_count][LEC_NMAP][nl][nxb] */
    double* lonsecsum_d;        /* in/out [LEC_NMAP][nl][nxb], accumulated */
    void* stream;
} lec_lonsections_args;
int lec_lonsections(const lec_lonsections_args* args);

/*
 * lec_composite_lonsections: the same sections over a series of per-step boxes of ONE shape, nyb rows x nxb columns, on the boxes'
 * BOX-RELATIVE columns i = 0 .. nxb - 1.  Geometry (box_h / box_d, boxtab_d, per-step lattab_d and lattab2_d), layouts and the three
 * sources of dT/dt (dTdt_d | tm_d + tp_d | the cube's own neighbours) are lec_composite_args' (lec_hip_ext.h) and mean what they mean
 * there.  A moving box is always an open box.
 *
 * Validation.  As above under the name "lec_composite_lonsections:", with lec_composite's own in place of the fixed box's: a null box_h,
 * box_d or boxtab_d; tm_d without tp_d or the reverse; dTdt_d together with tm_d / tp_d; tcoef_d null without dTdt_d; nt < 1, or nt < 2
 * when dT/dt comes from the cube's own neighbours; nyb < 2, nxb < 3, ny < nyb, nx < nxb; a box of box_h that is not nyb x nxb or lies
 * outside the cube (LEC_ERR_ARG names the step and both shapes); box_d / box_h not 4-byte aligned.
 */
typedef struct lec_composite_lonsections_args {
    const void* tair_d;
    const void* u_d;
    const void* v_d;
    const void* omega_d;
    const double* dTdt_d;       /* may be NULL; fp64 whatever dtype is */
    const void* tm_d;           /* may be NULL (then tp_d too): T of the previous step on the box of step t, laid out like tair_d */
    const void* tp_d;           /* T of the next step */
    int32_t dtype;              /* enum lec_dtype (LEC_F64 or LEC_F32), common to tair_d, u_d, v_d, omega_d, tm_d, tp_d */
    int32_t nt, nl, ny, nx;     /* cube dimensions (a box-packed series: the slabs') */
    int32_t t_begin, t_count;   /* process cube steps [t_begin, t_begin + t_count) */
    int32_t nyb, nxb;           /* the shape of EVERY box: rows, columns */
    int32_t reserved0;          /* must be 0 */
    const int32_t* box_h;       /* HOST [t_count][4] iw ie js jn as the cubes hold them: checked before any HIP call */
    const int32_t* box_d;       /* device copy of box_h */
    const double* boxtab_d;     /* [t_count][4]: [2] = 1 / h_deg of the step's box */
    const double* lattab_d;     /* [t_count][nyb][4] */
    const double* lattab2_d;    /* [t_count][nyb][8]; 16-byte aligned */
    const double* rows_d;       /* [t_count][nl][nyb][LEC_NSTAT]; 16-byte aligned */
    const double* levraw_d;     /* [t_count][nl][LEC_NLEVRAW] */
    const double* levtab_d;     /* [nl][3] */
    const double* levtab2_d;    /* [nl][4] */
    const double* tcoef_d;      /* [nt][3], the rows of the cubes' steps; may be NULL with dTdt_d */
    double* coef_d;             /* workspace [t_count][nl][nyb][LEC_MAPS_NCOEF]; 16-byte aligned */
    double* lonsec_d;           /* out [t_count][LEC_NMAP][nl][nxb] */
    double* lonsecsum_d;        /* in/out [LEC_NMAP][nl][nxb], accumulated */
    void* stream;
} lec_composite_lonsections_args;
int lec_composite_lonsections(const lec_composite_lonsections_args* args);

#ifdef __cplusplus
}
#endif

#endif
