/*
 * lec_hip_ext5.h -- calls of liblec_hip.so that came after include/lec_hip_ext4.h was closed.
 *
 * include/lec_hip.h is the library's ABI 11, include/lec_hip_ext.h, lec_hip_ext2.h, lec_hip_ext3.h and lec_hip_ext4.h its additions; the
 * tests pin those surfaces.  A call declared HERE is exported from the same liblec_hip.so, is an addition to them (no struct, export or
 * kernel result of theirs changes with it) and is bound in lorenzcycletoolkit_amd/_lib.py under EXT5_EXPORTS.  Error codes and
 * lec_last_error() are lec_hip.h's.
 */
#ifndef LEC_HIP_EXT5_H
#define LEC_HIP_EXT5_H

#include "lec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * --batch-composites-phase: PHASE-ALIGNED ensembles of the composites of a batch of tracks (csrc/lec_composite_phase.hip, a code object of
 * its own).  A clock gives every track B ranges of its own steps (a range may be empty, ranges may overlap); a
 * CELL is one (track, bin) pair.  lec_composite_phase_sum folds the columns lec_composite_steps (lec_hip_ext3.h) left for a call's boxes
 * over the cells' ranges; lec_composite_phase_ensemble turns the sums into per-cell means and per-bin ensembles whose membership differs
 * from bin to bin.
 *
 * lec_composite_phase_sum:
 *   col_d       [s_count][LEC_NMAP][nyb][nxb], the columns of a call's boxes as lec_composite_steps left them; read only.
 *   range_h / range_d  int32 [n_cell][2] {begin, end}: box offsets into THIS call's boxes, 0 <= begin <= end <= s_count.  range_h is the
 *               HOST copy, checked before any HIP call; the kernel reads range_d only, checks it once more and touches NOTHING for a cell
 *               whose device range lies outside [0, s_count] or has end < begin.
 *   phasesum_d  [n_cell][LEC_NMAP][nyb][nxb], in/out: the columns of boxes begin .. end - 1 are added to phasesum_d[cell] one by one in
 *               table order, starting from the value found there -- a plain running sum, so a range cut over several calls has the bits
 *               of one call.  A cell with begin == end is not written.  NaN propagates.  Ranges of different cells may overlap.
 * One thread per (cell, f, j, i) and per output element: ONE writer each, no atomics, no LDS.
 * Validation, before any HIP call, never clamped; every message starts with "lec_composite_phase_sum:".  LEC_ERR_ARG: null args, col_d,
 * range_h, range_d or phasesum_d; reserved0 != 0; s_count, nyb, nxb or n_cell < 1; a range with begin < 0, end < begin or end > s_count
 * (the message names the cell); col_d / phasesum_d not 8-byte, range_h / range_d not 4-byte aligned.  LEC_ERR_UNSUPPORTED:
 * n_cell * 6 * nyb * nxb >= 2^32 - 256.
 */
typedef struct lec_composite_phase_sum_args {
    const double* col_d;        /* [s_count][LEC_NMAP][nyb][nxb] */
    const int32_t* range_h;     /* HOST [n_cell][2] {begin, end}: checked before any HIP call */
    const int32_t* range_d;     /* device copy of range_h */
    double* phasesum_d;         /* in/out [n_cell][LEC_NMAP][nyb][nxb] */
    int32_t s_count;            /* boxes of the call */
    int32_t nyb, nxb;           /* the shape of every box */
    int32_t n_cell;             /* (track, bin) cells of the call */
    int32_t reserved0;          /* must be 0 */
    void* stream;
} lec_composite_phase_sum_args;
int lec_composite_phase_sum(const lec_composite_phase_sum_args* args);

/*
 * lec_composite_phase_ensemble: with phasesum_d [K][B][n], n = LEC_NMAP * nyb * nxb, as lec_composite_phase_sum left it and count[k][b] >= 0
 * the number of steps of track k in bin b,
 *   mean_d[k][b]  = phasesum_d[k][b] * (1.0 / (double)count[k][b]) where the count is >= 1 -- the rounded reciprocal and one product, the
 *                   rule of lec_composite_ensemble --, NaN where it is 0.  mean_d may alias phasesum_d.
 *   m_b           = the number of tracks with count[k][b] >= 1, the MEMBERS of bin b.
 *   ens_d[b]      = (the means of the members, added in track order starting from the first member's) / (double)m_b, the IEEE quotient;
 *                   NaN for m_b = 0.
 *   spread_d[b]   = sqrt(S / (double)(m_b - 1)), S the sum in track order, from 0.0, of (mean - ens) * (mean - ens) over the members
 *                   (products and sums rounded separately); NaN for m_b < 2.
 * One thread per (b, point), tracks ascending, contraction off.  A NaN in a member's mean propagates into that bin's ens_d and spread_d at
 * that point only.  count_h is the HOST copy of count_d, checked before any HIP call.
 * LEC_ERR_ARG ("lec_composite_phase_ensemble: ..."): null args, phasesum_d, count_h, count_d, mean_d, ens_d or spread_d; n_track, n_bin,
 * nyb or nxb < 1; reserved0 != 0; a negative count (the message names the track and the bin); a table not 8-byte, a count table not
 * 4-byte aligned.  LEC_ERR_UNSUPPORTED: n_bin * 6 * nyb * nxb >= 2^32 - 256.
 */
typedef struct lec_composite_phase_ensemble_args {
    const double* phasesum_d;   /* [n_track][n_bin][LEC_NMAP][nyb][nxb] */
    const int32_t* count_h;     /* HOST [n_track][n_bin]: steps per cell, each >= 0 */
    const int32_t* count_d;     /* device copy of count_h */
    int32_t n_track, n_bin, nyb, nxb;
    int32_t reserved0;          /* must be 0 */
    double* mean_d;             /* out [n_track][n_bin][LEC_NMAP][nyb][nxb]; may be phasesum_d */
    double* ens_d;              /* out [n_bin][LEC_NMAP][nyb][nxb] */
    double* spread_d;           /* out [n_bin][LEC_NMAP][nyb][nxb] */
    void* stream;
} lec_composite_phase_ensemble_args;
int lec_composite_phase_ensemble(const lec_composite_phase_ensemble_args* args);

#ifdef __cplusplus
}
#endif

#endif
