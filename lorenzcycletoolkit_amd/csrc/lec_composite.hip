// lec_composite.hip -- lec_composite: the SYSTEM-RELATIVE composites of the six eddy terms Ae Ke Ca Ce Ck Ge over a series of per-step
// boxes of ONE shape (-t / -c --composites; include/lec_hip_ext.h).  A translation unit of its own: its code object
// is loaded by calls that ask for composites only.
//
// The call is lec_maps (lec_maps.hip) with three things lifted to "per step": the box and its tables (box_d, lattab_d, lattab2_d, boxtab_d
// are indexed by the step), dT/dt by lec_rowstats' rule (a dT/dt cube, or T of the two time neighbours ON THE STEP'S BOX, or the cube's own
// neighbours), and the Hovmoeller weights.  Box-relative indices (j, i) take the place of the grid's.  The kernels -- factors, column
// values, time sums, Hovmoeller -- and the refusals shared with lec_maps are lec_mapcol.h's, instantiated here.  This file holds what a
// series of MOVING boxes has of its own: the step's box, 1 / h_deg and lattab row come from box_d / boxtab_d / lattab_d (ColParams;
// wave-uniform: scalar loads), lattab2 is nyb * 8 doubles on per step, and the source of dT/dt picks DMODE.  A moving box is an open box:
// one-sided d/dlon at its first and last column, and nothing outside the box is read.
#include "../../include/lec_hip_ext.h"
#include "lec_mapcol.h"

namespace {
using namespace lec;

struct ColParams : MapColGrid {
    const double* DT;        // the dT/dt cube (DMODE 0)
    const void *TM, *TP;     // T of the time neighbours on the step's box (DMODE 1)
    const int32_t* box;      // [t_count][4] as the cubes hold them
    const double* boxtab;    // [t_count][4]: [2] = 1 / h_deg
    const double* lattab;    // [t_count][nyb][4]
    // the step's own box (its shape was checked on the host) and tables
    __device__ int iw(int tl) const { return box[4 * tl + 0]; }
    __device__ int js(int tl) const { return box[4 * tl + 2]; }
    __device__ const double* lattab_row(int tl, int jb) const { return lattab + ((size_t)tl * nyb + jb) * 4; }
    __device__ double inv_hdeg(int tl) const { return boxtab[4 * tl + 2]; }
};

}  // namespace

extern "C" int lec_composite(const lec_composite_args* a) {
    const MapcolRefusals chk{"lec_composite"};
    if (!a) return chk.refuse(LEC_ERR_ARG, "null args");
    if (!a->tair_d) return chk.refuse(LEC_ERR_ARG, "null tair_d");
    if (!a->u_d) return chk.refuse(LEC_ERR_ARG, "null u_d");
    if (!a->v_d) return chk.refuse(LEC_ERR_ARG, "null v_d");
    if (!a->omega_d) return chk.refuse(LEC_ERR_ARG, "null omega_d");
    if (!a->box_h) return chk.refuse(LEC_ERR_ARG, "null box_h (the host copy of the boxes: their shapes are checked before anything is launched)");
    if (!a->box_d) return chk.refuse(LEC_ERR_ARG, "null box_d");
    if (!a->boxtab_d) return chk.refuse(LEC_ERR_ARG, "null boxtab_d");
    if (!a->lattab_d) return chk.refuse(LEC_ERR_ARG, "null lattab_d");
    if (!a->lattab2_d) return chk.refuse(LEC_ERR_ARG, "null lattab2_d");
    if (!a->rows_d) return chk.refuse(LEC_ERR_ARG, "null rows_d");
    if (!a->levraw_d) return chk.refuse(LEC_ERR_ARG, "null levraw_d");
    if (!a->levtab_d) return chk.refuse(LEC_ERR_ARG, "null levtab_d");
    if (!a->levtab2_d) return chk.refuse(LEC_ERR_ARG, "null levtab2_d");
    if (!a->coef_d) return chk.refuse(LEC_ERR_ARG, "null coef_d (the workspace of the row factors)");
    if (!a->col_d) return chk.refuse(LEC_ERR_ARG, "null col_d (the column values, which are the workspace of the sums too)");
    if (!a->hov_d) return chk.refuse(LEC_ERR_ARG, "null hov_d");
    if (!a->mapsum_d) return chk.refuse(LEC_ERR_ARG, "null mapsum_d");
    if (int r = chk.dtype(a->dtype)) return r;
    if (a->reserved0 != 0) return chk.refuse(LEC_ERR_ARG, "reserved0 must be 0");
    // dT/dt by lec_rowstats' rule
    if ((a->tm_d != nullptr) != (a->tp_d != nullptr))
        return chk.refuse(LEC_ERR_ARG, a->tm_d ? "tm_d without tp_d (a box-packed series needs both time neighbours)"
                                               : "tp_d without tm_d (a box-packed series needs both time neighbours)");
    if (a->dTdt_d && a->tm_d) return chk.refuse(LEC_ERR_ARG, "dTdt_d together with tm_d / tp_d: give one source of dT/dt");
    if (!a->dTdt_d && !a->tcoef_d) return chk.refuse(LEC_ERR_ARG, "null tcoef_d without dTdt_d: no source of dT/dt");
    const int dmode = a->dTdt_d ? 0 : (a->tm_d ? 1 : 2);
    if (a->nt < 1) return chk.refuse(LEC_ERR_ARG, "nt must be >= 1");
    if (dmode == 2 && a->nt < 2) return chk.refuse(LEC_ERR_ARG, "nt must be >= 2 when dT/dt comes from the cube's own time neighbours (no dTdt_d, tm_d / tp_d)");
    if (int r = chk.levels(a->nl)) return r;
    if (a->nyb < 2) return chk.refuse(LEC_ERR_ARG, "nyb must be >= 2 (a box needs two rows for d/dlat)");
    if (a->nxb < 3) return chk.refuse(LEC_ERR_ARG, "nxb must be >= 3 (a composite needs three box columns)");
    if (a->ny < a->nyb) return chk.refuse(LEC_ERR_ARG, "ny must be >= nyb");
    if (a->nx < a->nxb) return chk.refuse(LEC_ERR_ARG, "nx must be >= nxb");
    if (int r = chk.steps(a->nt, a->t_begin, a->t_count)) return r;
    // every box nyb x nxb and inside the cube: on the HOST copy, before any HIP call
    for (int t = 0; t < a->t_count; ++t) {
        const int32_t* b = a->box_h + 4 * (size_t)t;
        const long long w = (long long)b[1] - b[0] + 1, h = (long long)b[3] - b[2] + 1;
        char m[256];
        if (w != a->nxb || h != a->nyb) {
            snprintf(m, sizeof(m), "box_h: the box of step %d is %lld x %lld (rows x columns), the call's nyb x nxb is %d x %d: every box of a "
                     "composite has one shape", t, h, w, a->nyb, a->nxb);
            return chk.refuse(LEC_ERR_ARG, m);
        }
        if (b[0] < 0 || b[1] >= a->nx || b[2] < 0 || b[3] >= a->ny) {
            snprintf(m, sizeof(m), "box_h: the box of step %d {iw, ie, js, jn} = {%d, %d, %d, %d} lies outside the %d x %d cube", t, b[0], b[1],
                     b[2], b[3], a->ny, a->nx);
            return chk.refuse(LEC_ERR_ARG, m);
        }
    }
    if (int r = chk.align16(a->rows_d, a->lattab2_d, a->coef_d)) return r;
    if ((uintptr_t)a->box_d % 4) return chk.refuse(LEC_ERR_ARG, "box_d must be 4-byte aligned");
    if ((uintptr_t)a->box_h % 4) return chk.refuse(LEC_ERR_ARG, "box_h must be 4-byte aligned");
    const void* tabs[] = {a->levraw_d, a->levtab2_d, a->lattab_d, a->levtab_d, a->tcoef_d, a->boxtab_d, a->dTdt_d, a->col_d, a->hov_d, a->mapsum_d};
    const char* tabn[] = {"levraw_d", "levtab2_d", "lattab_d", "levtab_d", "tcoef_d", "boxtab_d", "dTdt_d", "col_d", "hov_d", "mapsum_d"};
    const void* cubes[] = {a->tair_d, a->u_d, a->v_d, a->omega_d, a->tm_d, a->tp_d};
    const int nyb = a->nyb, nxb = a->nxb;
    if (int r = chk.tables_cubes_limits(tabs, tabn, 10, cubes, 6, "tair_d, u_d, v_d, omega_d, tm_d, tp_d", a->dtype, a->t_count, a->nl, nyb,
                                        nxb, "nyb, nxb"))
        return r;

    ColParams p;
    p.DT = a->dTdt_d; p.TM = a->tm_d; p.TP = a->tp_d; p.box = a->box_d; p.boxtab = a->boxtab_d; p.lattab = a->lattab_d;
    // a moving box is an open box: no ring form
    return mapcol_launch(a, p, nyb, nxb, nyb * 8, [a, dmode](const ColParams& q, dim3 grid, hipStream_t st) {
        if (dmode == 0) mapcol_col<false, 0>(q, a->dtype, grid, st);
        else if (dmode == 1) mapcol_col<false, 1>(q, a->dtype, grid, st);
        else mapcol_col<false, 2>(q, a->dtype, grid, st);
    });
}
