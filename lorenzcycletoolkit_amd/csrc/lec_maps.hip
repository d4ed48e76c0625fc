// lec_maps.hip -- lec_maps: the LONGITUDE-resolved maps of the six eddy terms Ae Ke Ca Ce Ck Ge on ONE fixed box (-f [--periodic] --maps;
// include/lec_hip.h).  A translation unit of its own: its code object is loaded by calls that ask for maps only.
//
// Every eddy term of stage 2 is the zonal average of a pointwise product times a factor of (time step, level, row) only (lec_level_row.inc;
// the table in DESIGN.md section 4.2c).  The map is that expression with the zonal average left off.  Stage 1 sums over longitude before
// anything leaves the chip, so this call reads the field cubes again.  The kernels -- factors, column values, time sums, Hovmoeller -- and
// the refusals shared with lec_composite are lec_mapcol.h's, instantiated here.  This file holds what a FIXED box has of its own: the box,
// its 1 / h_deg and its tables come from the arguments and are the same at every step (ColParams; lattab2's stride per step is 0), lambda
// wraps on a ring (RING), and dT/dt is taken over the cube's own time axis (DMODE 2).
#include "lec_mapcol.h"

namespace {
using namespace lec;

struct ColParams : MapColGrid {
    const double* lattab;    // [nyb][4]
    double inv_hdeg_;
    int iw_, js_;
    // one box for every step
    __device__ int iw(int) const { return iw_; }
    __device__ int js(int) const { return js_; }
    __device__ const double* lattab_row(int, int jb) const { return lattab + (size_t)jb * 4; }
    __device__ double inv_hdeg(int) const { return inv_hdeg_; }
};

}  // namespace

extern "C" int lec_maps(const lec_maps_args* a) {
    const MapcolRefusals chk{"lec_maps"};
    if (!a) return chk.refuse(LEC_ERR_ARG, "null args");
    const void* outs[] = {a->col_d, a->hov_d, a->mapsum_d};
    const char* out_null[] = {"null col_d (the column values, which are the workspace of the sums too)", "null hov_d", "null mapsum_d"};
    if (int r = chk.fixed_box(a, outs, out_null, 3, "ie - iw + 1 must be >= 3 (a map needs three box columns)",
                              "jn must be js + 1 .. ny - 1 (a box needs two rows for d/dlat)"))
        return r;
    const void* tabs[] = {a->levraw_d, a->levtab2_d, a->lattab_d, a->levtab_d, a->tcoef_d, a->col_d, a->hov_d, a->mapsum_d};
    const char* tabn[] = {"levraw_d", "levtab2_d", "lattab_d", "levtab_d", "tcoef_d", "col_d", "hov_d", "mapsum_d"};
    const void* cubes[] = {a->tair_d, a->u_d, a->v_d, a->omega_d};
    const int nyb = a->jn - a->js + 1, nxb = a->ie - a->iw + 1;
    if (int r = chk.tables_cubes_limits({tabs, tabn, 8, cubes, 4, "tair_d, u_d, v_d, omega_d", a->dtype}, a->t_count, a->nl, nyb, nxb,
                                        "js, jn, iw, ie"))
        return r;

    ColParams p;
    p.lattab = a->lattab_d; p.inv_hdeg_ = a->inv_hdeg; p.iw_ = a->iw; p.js_ = a->js;
    // dT/dt over the cube's own time axis: DMODE 2
    const MapcolRun run{a->col_d, a->mapsum_d, a->hov_d, nyb, a->t_begin, a->t_count};
    return mapcol_launch(a, p, run, nyb, nxb, 0, [a](const ColParams& q, dim3 grid, hipStream_t st) {
        if (a->ring) mapcol_col<true, 2>(q, a->dtype, grid, st);
        else mapcol_col<false, 2>(q, a->dtype, grid, st);
    });
}
