// lec_lonsections.hip -- lec_lonsections and lec_composite_lonsections: the LONGITUDE x PRESSURE sections of the six eddy terms Ae Ke Ca
// Ce Ck Ge on one fixed box (-f [--periodic] --lon-sections) and on the box-relative columns of a series of moving boxes of one shape (-t /
// -c --composite-lon-sections; include/lec_hip_ext4.h).  A translation unit of its own: its code object is loaded
// by calls that ask for these sections only.
//
// lec_maps and lec_composite integrate the point integrand Y_f(t, k, j, i) over pressure in registers and never write it (lec_mapcol.h);
// this file sums it over the ROWS instead, X_f(t, k, i) = sum_j cw_j(t) Y_f(t, k, j, i), and keeps the levels.  The factors of (t, k, j) --
// lec_mapcol_coef_kernel -- and the time sums -- lec_mapcol_sum_kernel, which is generic over its element count: nl stands where it has
// nyb -- are lec_mapcol.h's, instantiated here.  The new kernel marches UP THE ROWS of one level, where lec_mapcol_col_kernel marches down
// the levels of one row.
#include "../../include/lec_hip_ext.h"
#include "../../include/lec_hip_ext4.h"
#include "lec_mapcol.h"

namespace {
using namespace lec;

// the two launch structs: MapColGrid (col = lonsec_d) with the members lec_mapcol.h documents, and lattab2 for the rows' weights
struct FixedParams : MapColGrid {
    const double* lattab;    // [nyb][4]
    const double* lattab2;   // [nyb][8]
    double inv_hdeg_;
    int iw_, js_;
    // one box for every step
    __device__ int iw(int) const { return iw_; }
    __device__ int js(int) const { return js_; }
    __device__ const double* lattab_row(int, int jb) const { return lattab + (size_t)jb * 4; }
    __device__ double inv_hdeg(int) const { return inv_hdeg_; }
    __device__ double cw(int, int jb) const { return lattab2[8 * (size_t)jb]; }
};

struct MovingParams : MapColGrid {
    const double* DT;        // the dT/dt cube (DMODE 0)
    const void *TM, *TP;     // T of the time neighbours on the step's box (DMODE 1)
    const int32_t* box;      // [t_count][4] as the cubes hold them
    const double* boxtab;    // [t_count][4]: [2] = 1 / h_deg
    const double* lattab;    // [t_count][nyb][4]
    const double* lattab2;   // [t_count][nyb][8]
    // the step's own box (its shape was checked on the host) and tables
    __device__ int iw(int tl) const { return box[4 * tl + 0]; }
    __device__ int js(int tl) const { return box[4 * tl + 2]; }
    __device__ const double* lattab_row(int tl, int jb) const { return lattab + ((size_t)tl * nyb + jb) * 4; }
    __device__ double inv_hdeg(int tl) const { return boxtab[4 * tl + 2]; }
    __device__ double cw(int tl, int jb) const { return lattab2[8 * ((size_t)tl * nyb + jb)]; }
};

// the sections X_f(t, k, i): grid (t_count * nl * nseg), column segment fastest, then level, then time step; block 64: one wave per (time
// step, level, 64 columns), lanes ALONG LONGITUDE (every cube load is a row segment), marching up the rows jb = 0 .. nyb - 1 of level k with
// T(j - 1) T(j) T(j + 1) in registers; the box, its tables, cw_jb and the record of (t, k, jb) -- contiguous along the march -- are
// wave-uniform (scalar loads).  RING and DMODE 0 / 1 / 2 as lec_mapcol_col_kernel has them.
//
// The point's Q and six integrands are lec_mapcol_point.inc, the text lec_mapcol_col_kernel includes too: one text, so a correction to Ck
// or Ge is made once.  A text include and not a __device__ function: the function form changed the schedule of the three older code
// objects, while an include hands the compiler the tokens each kernel held before -- the device assembly of all four files is the former,
// instruction for instruction.
template <typename E, bool RING, int DMODE, typename P>
__global__ void __launch_bounds__(64) lec_lonsec_kernel(const P p) {
#pragma clang fp contract(off)
    constexpr double kCp = LEC_CP_D;
    static_assert(DMODE >= 0 && DMODE <= 2, "a dT/dt cube, the box's time neighbours, or the cube's own");
    const int nx = p.nx, nl = p.nl, nyb = p.nyb, nxb = p.nxb;
    const int seg = blockIdx.x % p.nseg, tk = blockIdx.x / p.nseg;
    const int k = tk % nl, tl = tk / nl;
    const int e = seg * 64 + (int)threadIdx.x;          // box column
    if (e >= nxb) return;                               // (no barrier below)
    const int t = p.t_begin + tl;
    const size_t plane = (size_t)p.ny * nx, cube = plane * nl;
    const int i = p.iw(tl) + e;
    const bool first = e == 0, last = e == nxb - 1;
    // the lambda neighbours: wrapped on a ring; an open box reads nothing outside its columns (the one-sided difference needs none)
    const int il = RING ? (i == 0 ? nx - 1 : i - 1) : (first ? i : i - 1);
    const int ir = RING ? (i == nx - 1 ? 0 : i + 1) : (last ? i : i + 1);
    const size_t row0 = (size_t)t * cube + (size_t)k * plane + (size_t)p.js(tl) * nx;      // box row 0 of the level
    const E* __restrict__ pT = (const E*)p.T + row0;
    const E* __restrict__ pU = (const E*)p.U + row0;
    const E* __restrict__ pV = (const E*)p.V + row0;
    const E* __restrict__ pW = (const E*)p.W + row0;
    const double* __restrict__ pD = nullptr;
    const E* __restrict__ pM = nullptr;
    const E* __restrict__ pP = nullptr;
    if constexpr (DMODE == 0) pD = p.DT + row0;
    if constexpr (DMODE == 1) { pM = (const E*)p.TM + row0; pP = (const E*)p.TP + row0; }
    // a level that does not exist: the level itself, whose coefficient in the table is 0
    const ptrdiff_t okm = k > 0 ? -(ptrdiff_t)plane : 0, okp = k < nl - 1 ? (ptrdiff_t)plane : 0;
    // from T[t] to its time neighbours (DMODE 2)
    const ptrdiff_t otm = t > 0 ? -(ptrdiff_t)cube : 0, otp = t < p.nt - 1 ? (ptrdiff_t)cube : 0;
    const double* lv = p.levtab + (size_t)k * 3;
    const double al = lv[0], be = lv[1], gm = lv[2];
    double ta = 0.0, tb = 0.0, tc = 0.0;
    if (DMODE != 0) { const double* tcf = p.tcoef + (size_t)t * 3; ta = tcf[0]; tb = tcf[1]; tc = tcf[2]; }
    const double* cf = p.coef + ((size_t)tl * nl + k) * nyb * kNC;

    double acc[kNMap];
#pragma unroll
    for (int f = 0; f < kNMap; ++f) acc[f] = 0.0;

    // a row that does not exist: the row itself, whose coefficient in the tables is 0
    double Tc = (double)pT[i], Tjm = Tc;
    for (int jb = 0; jb < nyb; ++jb) {
        const size_t po = (size_t)jb * nx + i;
        const E* __restrict__ rT = pT + (size_t)jb * nx;
        const double Tjp = jb < nyb - 1 ? (double)rT[nx + i] : Tc;
        const double Tl = (double)rT[il], Tr = (double)rT[ir];
        const double Tm = (double)rT[okm + i], Tp = (double)rT[okp + i];
        const double Uv = (double)pU[po], Vv = (double)pV[po], Wv = (double)pW[po];
        const double* lt = p.lattab_row(tl, jb);
        const double ga = lt[0], gb = lt[1], gc = lt[2];
        const double cx = 0.5 * p.inv_hdeg(tl) * lt[3];            // centred d/dlon -> d/dx
        const double cw = p.cw(tl, jb);
        const double* c = cf + (size_t)jb * kNC;                    // wave-uniform: scalar loads

#include "lec_mapcol_point.inc"
        acc[M_AE] += cw * yAe;
        acc[M_KE] += cw * yKe;
        acc[M_CA] += cw * yCa;
        acc[M_CE] += cw * yCe;
        acc[M_CK] += cw * yCk;
        acc[M_GE] += cw * yGe;
        Tjm = Tc; Tc = Tjp;
    }
    double* o = p.col + ((size_t)tl * kNMap * nl + k) * nxb + e;
    const size_t fs = (size_t)nl * nxb;
#pragma unroll
    for (int f = 0; f < kNMap; ++f) o[(size_t)f * fs] = acc[f];
}

template <bool RING, int DMODE, typename P>
void lonsec_col(const P& p, const int dtype, const dim3 grid, hipStream_t st) {
    if (dtype == LEC_F64) hipLaunchKernelGGL((lec_lonsec_kernel<double, RING, DMODE, P>), grid, dim3(64), 0, st, p);
    else hipLaunchKernelGGL((lec_lonsec_kernel<float, RING, DMODE, P>), grid, dim3(64), 0, st, p);
}

}  // namespace

extern "C" int lec_lonsections(const lec_lonsections_args* a) {
    const MapcolRefusals chk{"lec_lonsections"};
    if (!a) return chk.refuse(LEC_ERR_ARG, "null args");
    const void* outs[] = {a->lonsec_d, a->lonsecsum_d};
    const char* out_null[] = {"null lonsec_d (the sections, which are the workspace of the time sums too)", "null lonsecsum_d"};
    if (int r = chk.fixed_box(a, outs, out_null, 2, "ie - iw + 1 (nxb) must be >= 3 (a section needs three box columns)",
                              "jn must be js + 1 .. ny - 1 (nyb >= 2: a box needs two rows for d/dlat)"))
        return r;
    const void* tabs[] = {a->levraw_d, a->levtab2_d, a->lattab_d, a->levtab_d, a->tcoef_d, a->lonsec_d, a->lonsecsum_d};
    const char* tabn[] = {"levraw_d", "levtab2_d", "lattab_d", "levtab_d", "tcoef_d", "lonsec_d", "lonsecsum_d"};
    const void* cubes[] = {a->tair_d, a->u_d, a->v_d, a->omega_d};
    const int nyb = a->jn - a->js + 1, nxb = a->ie - a->iw + 1;
    if (int r = chk.tables_cubes_lonsec_limits({tabs, tabn, 7, cubes, 4, "tair_d, u_d, v_d, omega_d", a->dtype}, a->t_count, a->nl, nxb, "iw, ie"))
        return r;

    FixedParams p;
    p.lattab = a->lattab_d; p.lattab2 = a->lattab2_d; p.inv_hdeg_ = a->inv_hdeg; p.iw_ = a->iw; p.js_ = a->js;
    // dT/dt over the cube's own time axis: DMODE 2
    const MapcolRun run{a->lonsec_d, a->lonsecsum_d, nullptr, a->nl, a->t_begin, a->t_count};
    return mapcol_launch(a, p, run, nyb, nxb, 0, [a](const FixedParams& q, dim3 grid, hipStream_t st) {
        if (a->ring) lonsec_col<true, 2>(q, a->dtype, grid, st);
        else lonsec_col<false, 2>(q, a->dtype, grid, st);
    });
}

extern "C" int lec_composite_lonsections(const lec_composite_lonsections_args* a) {
    const MapcolRefusals chk{"lec_composite_lonsections"};
    if (!a) return chk.refuse(LEC_ERR_ARG, "null args");
    const void* outs[] = {a->lonsec_d, a->lonsecsum_d};
    const char* out_null[] = {"null lonsec_d (the sections, which are the workspace of the time sums too)", "null lonsecsum_d"};
    int dmode;
    if (int r = chk.moving_boxes(a, outs, out_null, 2, "nxb must be >= 3 (a section needs three box columns)", &dmode)) return r;
    const void* tabs[] = {a->levraw_d, a->levtab2_d, a->lattab_d, a->levtab_d, a->tcoef_d, a->boxtab_d, a->dTdt_d, a->lonsec_d, a->lonsecsum_d};
    const char* tabn[] = {"levraw_d", "levtab2_d", "lattab_d", "levtab_d", "tcoef_d", "boxtab_d", "dTdt_d", "lonsec_d", "lonsecsum_d"};
    const void* cubes[] = {a->tair_d, a->u_d, a->v_d, a->omega_d, a->tm_d, a->tp_d};
    const int nyb = a->nyb, nxb = a->nxb;
    if (int r = chk.tables_cubes_lonsec_limits({tabs, tabn, 9, cubes, 6, "tair_d, u_d, v_d, omega_d, tm_d, tp_d", a->dtype}, a->t_count, a->nl,
                                               nxb, "nxb"))
        return r;

    MovingParams p;
    p.DT = a->dTdt_d; p.TM = a->tm_d; p.TP = a->tp_d; p.box = a->box_d; p.boxtab = a->boxtab_d; p.lattab = a->lattab_d; p.lattab2 = a->lattab2_d;
    // a moving box is an open box: no ring form
    const MapcolRun run{a->lonsec_d, a->lonsecsum_d, nullptr, a->nl, a->t_begin, a->t_count};
    return mapcol_launch(a, p, run, nyb, nxb, nyb * 8, [a, dmode](const MovingParams& q, dim3 grid, hipStream_t st) {
        if (dmode == 0) lonsec_col<false, 0>(q, a->dtype, grid, st);
        else if (dmode == 1) lonsec_col<false, 1>(q, a->dtype, grid, st);
        else lonsec_col<false, 2>(q, a->dtype, grid, st);
    });
}
