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
    const void* outs[] = {a->col_d, a->hov_d, a->mapsum_d};
    const char* out_null[] = {"null col_d (the column values, which are the workspace of the sums too)", "null hov_d", "null mapsum_d"};
    int dmode;
    if (int r = chk.moving_boxes(a, outs, out_null, 3, "nxb must be >= 3 (a composite needs three box columns)", &dmode)) return r;
    const void* tabs[] = {a->levraw_d, a->levtab2_d, a->lattab_d, a->levtab_d, a->tcoef_d, a->boxtab_d, a->dTdt_d, a->col_d, a->hov_d, a->mapsum_d};
    const char* tabn[] = {"levraw_d", "levtab2_d", "lattab_d", "levtab_d", "tcoef_d", "boxtab_d", "dTdt_d", "col_d", "hov_d", "mapsum_d"};
    const void* cubes[] = {a->tair_d, a->u_d, a->v_d, a->omega_d, a->tm_d, a->tp_d};
    const int nyb = a->nyb, nxb = a->nxb;
    if (int r = chk.tables_cubes_limits({tabs, tabn, 10, cubes, 6, "tair_d, u_d, v_d, omega_d, tm_d, tp_d", a->dtype}, a->t_count, a->nl, nyb,
                                        nxb, "nyb, nxb"))
        return r;

    ColParams p;
    p.DT = a->dTdt_d; p.TM = a->tm_d; p.TP = a->tp_d; p.box = a->box_d; p.boxtab = a->boxtab_d; p.lattab = a->lattab_d;
    // a moving box is an open box: no ring form
    const MapcolRun run{a->col_d, a->mapsum_d, a->hov_d, nyb, a->t_begin, a->t_count};
    return mapcol_launch(a, p, run, nyb, nxb, nyb * 8, [a, dmode](const ColParams& q, dim3 grid, hipStream_t st) {
        if (dmode == 0) mapcol_col<false, 0>(q, a->dtype, grid, st);
        else if (dmode == 1) mapcol_col<false, 1>(q, a->dtype, grid, st);
        else mapcol_col<false, 2>(q, a->dtype, grid, st);
    });
}
