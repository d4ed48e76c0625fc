/*
 * lec_hip_ext.h -- calls of liblec_hip.so that came after ABI 11 was closed.
 *
 * include/lec_hip.h is the library's ABI 11: its structs, its exports and LEC_ABI_VERSION stay as they are, and the tests pin that
 * surface.  A call declared HERE is exported from the same liblec_hip.so, is an addition to that surface (no struct, export or kernel
 * result of ABI 11 changes with it) and is bound in lorenzcycletoolkit_amd/_lib.py under EXT_EXPORTS, not under EXPORTS.  Error codes,
 * lec_last_error() and the dtype enum are lec_hip.h's.
 */
#ifndef LEC_HIP_EXT_H
#define LEC_HIP_EXT_H

#include "lec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * -t / -c --composites: the SYSTEM-RELATIVE COMPOSITES of the six eddy terms Ae Ke Ca Ce Ck Ge over a series of per-step boxes that all
 * have ONE shape, nyb rows x nxb columns (csrc/lec_composite.hip, a code object of its own).
 *
 * The moving framework has one box per time step, which follows a system; the boxes share no grid points, but they share their
 * BOX-RELATIVE indices: row j = 0 .. nyb - 1 from the box's southern edge, column i = 0 .. nxb - 1 from its western edge.  The call is
 * lec_maps (lec_hip.h) on those indices, with the box, its tables and the Hovmoeller weights taken PER STEP and dT/dt by lec_rowstats'
 * rule.  Definitions, factors and the NaN rule are lec_maps':
 *   f = 0 Ae  T'T' / (2 sigma)        1 Ke  u'u' + v'v'        2 Ca  -(v'T' dphiTc / (2 Re sigma) + w'T' dpT / sigma)        3 Ce  -c1k w'T'
 *   4 Ck  c u'v' / Re dphiUc + v'v' / Re dphiV + tn u'u' mV / Re + w'u' dpU + w'v' dpU                      5 Ge  Q'T' / (cp sigma)
 * Primes are deviations from the row's zonal means over step t's box, READ from step t's row records (slots LEC_S_MT / MU / MV / MW / MQ);
 * sigma is READ from slot LEC_LEVRAW_SIGMA of step t's levraw record; dphiTc, dphiUc, dphiV, dpT, dpU are the row factors of
 * csrc/lec_level_row.inc formed from step t's records with step t's lattab2; c1k = Rd / (p_k g).  The factor of a product is formed once
 * per (t, k, j) and multiplied in.
 *
 * Q = cp (dT/dt + u dT/dx + v dT/dy - S w) at the point, the expression and fma form of lec_rowstats (stencil3 of csrc/lec_sweep.h):
 *   - d/dlon: a moving box is an OPEN box.  Centred inside, one-sided 2 (T[i+1] - T[i]) / 2 (T[i] - T[i-1]) at the box's first / last
 *     column, times 0.5 * boxtab_d[t][2] * lattab_d[t][j][3]; d/dlat by lattab_d[t][j][0..2], whose coefficient of a row that does not
 *     exist is 0 (the row itself is read in its place); S by levtab_d.  There is no ring form.  Nothing outside step t's box is read: in
 *     the box-packed layout the slab beside a box is zeros, in the cube layout it is other data, and reading either would be a wrong
 *     number, not a fault.
 *   - dT/dt, in this order (lec_rowstats' rule):
 *       dTdt_d != NULL            an fp64 cube [nt][nl][ny][nx] laid out like the fields, as lec_dtdt writes it (or any dT/dt the caller
 *                                 has; an fp32 one widened to fp64 is the value lec_rowstats reads): used as it is;
 *       else tm_d, tp_d != NULL   tc[t] . (tm[t], T[t], tp[t]): T of the previous / next step ON THE BOX OF STEP t, laid out like tair_d
 *                                 (the box-packed series of lec_rowstats_args.tm_d / tp_d);
 *       else                      tc[t] . (T[t - 1], T[t], T[t + 1]) of the cube itself (the step itself where a neighbour does not exist:
 *                                 its coefficient is 0), lec_maps' form -- meaningful for an UNPACKED cube only, whose time neighbours hold
 *                                 the same grid points; the library cannot tell the layouts apart, the caller must.
 *     tc = tcoef_d[t], t the CUBE's step t_begin + (step of the call): [nt][3], the rows of the cubes' steps, as lec_rowstats takes it.
 *
 * Layouts.  The cubes are [nt][nl][ny][nx]; step s of the call is cube step t_begin + s and uses box s, tables s, records s:
 *   box_d     [t_count][4]  {iw, ie, js, jn} AS THE CUBES HOLD THEM (lec_rowstats' contract): {0, nxb - 1, 0, nyb - 1} for a box-packed
 *             series, the grid indices for an unpacked cube.  box_h is the HOST copy of the same table: every box must be nyb x nxb and
 *             lie inside the cube, which is checked on box_h before any HIP call (LEC_ERR_ARG names the first step that differs and both
 *             shapes).  The kernels read box_d only; the caller keeps the two equal.
 *   lattab_d  [t_count][nyb][4], lattab2_d [t_count][nyb][8], boxtab_d [t_count][4]: the per-box tables of lec_rowstats / lec_reduce, built
 *             from the boxes' TRUE grid coordinates (tables.build_box_tables); boxtab_d[t][2] = 1 / h_deg of step t's box.
 *   rows_d    [t_count][nl][nyb][LEC_NSTAT], levraw_d [t_count][nl][LEC_NLEVRAW]: stage 1's records and the level stage's records of the
 *             same steps (exactly nyb rows per level).
 *   levtab_d  [nl][3], levtab2_d [nl][4]: as lec_rowstats / lec_reduce take them.
 * Outputs:
 *   col_d     [t_count][LEC_NMAP][nyb][nxb]  C_f(t, j, i) = s_f * trapezoid of the integrand over the levels' pressures, s_f = 1 / (2 g) for
 *             Ke, 1 / g for Ck, else 1, with lec_sections' NaN rule per (t, j, i): interior NaN levels are bridged linearly in p, NaN levels
 *             at either end are left out, a column without a finite level is NaN.  The caller's to keep, and the workspace of the sums.
 *   mapsum_d  [LEC_NMAP][nyb][nxb]           += sum over the call's steps of C_f, added step by step in time order; the caller zeroes it
 *             once and divides by the number of steps (the time-mean composite M_f): a NaN at any step makes the mean NaN.
 *   hov_d     [t_count][LEC_NMAP][nxb]       H_f(t, i) = sum_j cw_j(t) C_f(t, j, i), rows ascending, cw_j(t) = lattab2_d[t][j][0]; NaN
 *             propagates.
 *   coef_d    workspace [t_count][nl][nyb][LEC_MAPS_NCOEF]: the zonal means and factors of (t, k, j), written by the call's first kernel.
 * On data without NaN the zonal average over step t's box (the half-weight trapezoid of an open box) of H_f(t, .) is the step's scalar of
 * the moving framework, to rounding.  Every output element has ONE writer and the sums run in a fixed order: no atomics, and the numbers
 * depend neither on the launch nor on how a series is cut into calls, bit for bit.
 *
 * Validation.  Every refusal names the field and is made before any HIP call, never clamped.  LEC_ERR_ARG: null args; a null tair_d, u_d,
 * v_d, omega_d, box_h, box_d, boxtab_d, lattab_d, lattab2_d, rows_d, levraw_d, levtab_d, levtab2_d, coef_d, col_d, hov_d or mapsum_d;
 * dtype; reserved0 != 0; tm_d without tp_d or the reverse; dTdt_d together with tm_d / tp_d; tcoef_d null without dTdt_d; nt < 1, or
 * nt < 2 when dT/dt comes from the cube's own neighbours; nl < 2, nyb < 2, nxb < 3, ny < nyb, nx < nxb; t_begin / t_count outside the
 * cube; a box of box_h that is not nyb x nxb or lies outside the cube; rows_d, lattab2_d, coef_d not 16-byte aligned, another table or
 * output not 8-byte aligned, box_d / box_h not 4-byte aligned, a cube not aligned to its element.  LEC_ERR_UNSUPPORTED (lec_maps' limits):
 * nl > LEC_MAX_LEVELS, t_count * nl >= 2^26, t_count * nyb * ceil(nxb / 64) >= 2^26, 6 * nyb * nxb or t_count * 6 * nxb >= 2^32 - 256 (HIP
 * takes fewer than 2^32 threads per launch; the caller chunks).
 */
typedef struct lec_composite_args {
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
    const double* lattab_d;     /* [t_count][nyb][4]: d/dlat a, b, c; 1 / dx_j */
    const double* lattab2_d;    /* [t_count][nyb][8], as lec_reduce takes it; 16-byte aligned */
    const double* rows_d;       /* [t_count][nl][nyb][LEC_NSTAT]; 16-byte aligned */
    const double* levraw_d;     /* [t_count][nl][LEC_NLEVRAW] as lec_reduce's level stage left it for these steps */
    const double* levtab_d;     /* [nl][3] */
    const double* levtab2_d;    /* [nl][4] */
    const double* tcoef_d;      /* [nt][3], the rows of the cubes' steps; may be NULL with dTdt_d */
    double* coef_d;             /* workspace [t_count][nl][nyb][LEC_MAPS_NCOEF]; 16-byte aligned */
    double* col_d;              /* out [t_count][LEC_NMAP][nyb][nxb] */
    double* mapsum_d;           /* in/out [LEC_NMAP][nyb][nxb], accumulated */
    double* hov_d;              /* out [t_count][LEC_NMAP][nxb] */
    void* stream;
} lec_composite_args;
int lec_composite(const lec_composite_args* args);

#ifdef __cplusplus
}
#endif

#endif
