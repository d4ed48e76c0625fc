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
    if (!a->tair_d) return chk.refuse(LEC_ERR_ARG, "null tair_d");
    if (!a->u_d) return chk.refuse(LEC_ERR_ARG, "null u_d");
    if (!a->v_d) return chk.refuse(LEC_ERR_ARG, "null v_d");
    if (!a->omega_d) return chk.refuse(LEC_ERR_ARG, "null omega_d");
    if (!a->rows_d) return chk.refuse(LEC_ERR_ARG, "null rows_d");
    if (!a->levraw_d) return chk.refuse(LEC_ERR_ARG, "null levraw_d");
    if (!a->lattab2_d) return chk.refuse(LEC_ERR_ARG, "null lattab2_d");
    if (!a->levtab2_d) return chk.refuse(LEC_ERR_ARG, "null levtab2_d");
    if (!a->lattab_d) return chk.refuse(LEC_ERR_ARG, "null lattab_d");
    if (!a->levtab_d) return chk.refuse(LEC_ERR_ARG, "null levtab_d");
    if (!a->tcoef_d) return chk.refuse(LEC_ERR_ARG, "null tcoef_d (a dT/dt cube is not supported: dT/dt comes from the cube's time axis)");
    if (!a->coef_d) return chk.refuse(LEC_ERR_ARG, "null coef_d (the workspace of the row factors)");
    if (!a->col_d) return chk.refuse(LEC_ERR_ARG, "null col_d (the column values, which are the workspace of the sums too)");
    if (!a->hov_d) return chk.refuse(LEC_ERR_ARG, "null hov_d");
    if (!a->mapsum_d) return chk.refuse(LEC_ERR_ARG, "null mapsum_d");
    if (int r = chk.dtype(a->dtype)) return r;
    if (a->ring != 0 && a->ring != 1) return chk.refuse(LEC_ERR_ARG, "ring must be 0 or 1");
    if (a->reserved0 != 0) return chk.refuse(LEC_ERR_ARG, "reserved0 must be 0");
    if (a->nt < 2) return chk.refuse(LEC_ERR_ARG, "nt must be >= 2 (dT/dt by finite differences over the cube's time axis)");
    if (int r = chk.levels(a->nl)) return r;
    if (a->ny < 2) return chk.refuse(LEC_ERR_ARG, "ny must be >= 2");
    if (a->nx < 3) return chk.refuse(LEC_ERR_ARG, "nx must be >= 3");
    if (int r = chk.steps(a->nt, a->t_begin, a->t_count)) return r;
    if (a->iw < 0 || a->iw >= a->nx) return chk.refuse(LEC_ERR_ARG, "iw outside the cube's longitudes");
    if (a->ie < a->iw || a->ie >= a->nx) return chk.refuse(LEC_ERR_ARG, "ie must be iw .. nx - 1");
    if (a->ie - a->iw + 1 < 3) return chk.refuse(LEC_ERR_ARG, "ie - iw + 1 must be >= 3 (a map needs three box columns)");
    if (a->ring && (a->iw != 0 || a->ie != a->nx - 1)) return chk.refuse(LEC_ERR_ARG, "ring: iw .. ie must be 0 .. nx - 1 (a ring is the whole circle)");
    if (a->js < 0 || a->js >= a->ny) return chk.refuse(LEC_ERR_ARG, "js outside the cube's latitudes");
    if (a->jn <= a->js || a->jn >= a->ny) return chk.refuse(LEC_ERR_ARG, "jn must be js + 1 .. ny - 1 (a box needs two rows for d/dlat)");
    if (int r = chk.align16(a->rows_d, a->lattab2_d, a->coef_d)) return r;
    const void* tabs[] = {a->levraw_d, a->levtab2_d, a->lattab_d, a->levtab_d, a->tcoef_d, a->col_d, a->hov_d, a->mapsum_d};
    const char* tabn[] = {"levraw_d", "levtab2_d", "lattab_d", "levtab_d", "tcoef_d", "col_d", "hov_d", "mapsum_d"};
    const void* cubes[] = {a->tair_d, a->u_d, a->v_d, a->omega_d};
    const int nyb = a->jn - a->js + 1, nxb = a->ie - a->iw + 1;
    if (int r = chk.tables_cubes_limits(tabs, tabn, 8, cubes, 4, "tair_d, u_d, v_d, omega_d", a->dtype, a->t_count, a->nl, nyb, nxb,
                                        "js, jn, iw, ie"))
        return r;

    ColParams p;
    p.lattab = a->lattab_d; p.inv_hdeg_ = a->inv_hdeg; p.iw_ = a->iw; p.js_ = a->js;
    // dT/dt over the cube's own time axis: DMODE 2
    return mapcol_launch(a, p, nyb, nxb, 0, [a](const ColParams& q, dim3 grid, hipStream_t st) {
        if (a->ring) mapcol_col<true, 2>(q, a->dtype, grid, st);
        else mapcol_col<false, 2>(q, a->dtype, grid, st);
    });
}
