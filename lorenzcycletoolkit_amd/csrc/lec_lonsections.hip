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
// The point's Q and six integrands are a COPY of lec_mapcol_col_kernel's (lec_mapcol.h, "Q / cp = ..." to yGe): that kernel and the three
// files that instantiate it are left as they are, so their device code is the parent's by construction.
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
        const size_t jo = (size_t)jb * nx + i;
        const E* __restrict__ rT = pT + (size_t)jb * nx;
        const double Tjp = jb < nyb - 1 ? (double)rT[nx + i] : Tc;
        const double Tl = (double)rT[il], Tr = (double)rT[ir];
        const double Tm = (double)rT[okm + i], Tp = (double)rT[okp + i];
        const double Uv = (double)pU[jo], Vv = (double)pV[jo], Wv = (double)pW[jo];
        const double* lt = p.lattab_row(tl, jb);
        const double ga = lt[0], gb = lt[1], gc = lt[2];
        const double cx = 0.5 * p.inv_hdeg(tl) * lt[3];            // centred d/dlon -> d/dx
        const double cw = p.cw(tl, jb);
        const double* c = cf + (size_t)jb * kNC;                    // wave-uniform: scalar loads

        // Q / cp = dT/dt + u dT/dx + v dT/dy - S w: stage_row's expression (lec_rowspecq.hip), fma form kept
        // centred on a ring; one-sided at an open box's first and last column
        const double d = RING ? Tr - Tl : (first ? 2.0 * (Tr - Tc) : (last ? 2.0 * (Tc - Tl) : Tr - Tl));
        const double adv = (Uv * cx) * d;
        const double sP = stencil3(ga, Tjm, gc, Tjp, gb, Tc);
        const double sS = stencil3(al, Tm, gm, Tp, be, Tc);
        double dTdt;
        if (DMODE == 0) dTdt = pD[jo];
        else if (DMODE == 1) dTdt = stencil3(ta, (double)pM[jo], tc, (double)pP[jo], tb, Tc);
        else dTdt = stencil3(ta, (double)rT[otm + i], tc, (double)rT[otp + i], tb, Tc);
        const double rest = dTdt + adv;
        const double fq = fma(-Wv, sS, fma(Vv, sP, rest));

        const double a = Tc - c[C_MT], b = Uv - c[C_MU], v = Vv - c[C_MV], w = Wv - c[C_MW];
        const double q = kCp * fq - c[C_MQ];
        const double wT = w * a, vv = v * v, uu = b * b;
        const double yAe = (a * a) * c[C_AE];
        const double yKe = uu + vv;
        const double yCa = -((v * a) * c[C_CA1] + wT * c[C_CA2]);
        const double yCe = -(c[C_CE] * wT);
        const double yCk = (b * v) * c[C_CK1] + vv * c[C_CK2] + uu * c[C_CK3] + (w * b) * c[C_DPU] + (w * v) * c[C_DPU];
        const double yGe = (q * a) * c[C_GE];
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

// the three launches of a call on its stream: the factors, the sections, their time sums.  A: either args struct, whose common fields are
// read by name; launch_col(p, grid, stream) picks RING and DMODE
template <typename A, typename P, typename L>
int lonsec_launch(const A* a, P p, const int nyb, const int nxb, const int lt_stride, L launch_col) {
    hipStream_t st = (hipStream_t)a->stream;
    const MapCoefParams c{a->rows_d, a->lattab2_d, a->levtab2_d, a->levraw_d, a->coef_d, a->t_count, a->nl, nyb, lt_stride};
    hipLaunchKernelGGL(lec_mapcol_coef_kernel, dim3((unsigned)(a->t_count * a->nl)), dim3(64), 0, st, c);
    p.T = a->tair_d; p.U = a->u_d; p.V = a->v_d; p.W = a->omega_d;
    p.coef = a->coef_d; p.levtab = a->levtab_d; p.levtab2 = a->levtab2_d; p.tcoef = a->tcoef_d; p.col = a->lonsec_d;
    p.nt = a->nt; p.nl = a->nl; p.ny = a->ny; p.nx = a->nx; p.t_begin = a->t_begin; p.t_count = a->t_count;
    p.nyb = nyb; p.nxb = nxb; p.nseg = (nxb + 63) / 64;
    launch_col(p, dim3((unsigned)((long long)a->t_count * a->nl * p.nseg)), st);
    // the time sums: lec_mapcol_sum_kernel over [kNMap][nl][nxb] elements, nl where the maps have nyb (lattab2 and hov are not read)
    const MapFoldParams f{a->lonsec_d, a->lattab2_d, a->lonsecsum_d, nullptr, a->t_count, a->nl, nxb, lt_stride};
    hipLaunchKernelGGL(lec_mapcol_sum_kernel, dim3((unsigned)(((long long)kNMap * a->nl * nxb + 255) / 256)), dim3(256), 0, st, f);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}

// the alignments of the 8-byte tables and of the cubes, and the two launch limits of these calls
int lonsec_tables_cubes_limits(const MapcolRefusals& chk, const void* const* tabs, const char* const* tabn, int ntab, const void* const* cubes,
                               int ncube, const char* cube_names, int dtype, int t_count, int nl, int nxb, const char* cols) {
    char m[160];
    for (int i = 0; i < ntab; ++i)
        if ((uintptr_t)tabs[i] % 8) {
            snprintf(m, sizeof(m), "%s must be 8-byte aligned", tabn[i]);
            return chk.refuse(LEC_ERR_ARG, m);
        }
    const size_t esz = dtype == LEC_F32 ? 4 : 8;
    for (int i = 0; i < ncube; ++i)
        if ((uintptr_t)cubes[i] % esz) {
            snprintf(m, sizeof(m), "cube pointer (%s) not aligned to its element size", cube_names);
            return chk.refuse(LEC_ERR_ARG, m);
        }
    // one 64-lane workgroup per (time step, level, 64 columns) -- which bounds the factors' (time step, level) too -- and one thread per
    // element of lonsecsum_d
    if ((long long)t_count * nl * ((nxb + 63) / 64) >= (1LL << 26)) {
        snprintf(m, sizeof(m), "t_count * nl * ceil(columns / 64) (%s) must stay below 2^26 in one call (cut the series into several calls)", cols);
        return chk.refuse(LEC_ERR_UNSUPPORTED, m);
    }
    if ((long long)kNMap * nl * nxb >= (1LL << 32) - 256) {
        snprintf(m, sizeof(m), "6 * nl * columns (%s) must stay below 2^32 threads", cols);
        return chk.refuse(LEC_ERR_UNSUPPORTED, m);
    }
    return LEC_OK;
}

}  // namespace

extern "C" int lec_lonsections(const lec_lonsections_args* a) {
    const MapcolRefusals chk{"lec_lonsections"};
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
    if (!a->lonsec_d) return chk.refuse(LEC_ERR_ARG, "null lonsec_d (the sections, which are the workspace of the time sums too)");
    if (!a->lonsecsum_d) return chk.refuse(LEC_ERR_ARG, "null lonsecsum_d");
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
    if (a->ie - a->iw + 1 < 3) return chk.refuse(LEC_ERR_ARG, "ie - iw + 1 (nxb) must be >= 3 (a section needs three box columns)");
    if (a->ring && (a->iw != 0 || a->ie != a->nx - 1)) return chk.refuse(LEC_ERR_ARG, "ring: iw .. ie must be 0 .. nx - 1 (a ring is the whole circle)");
    if (a->js < 0 || a->js >= a->ny) return chk.refuse(LEC_ERR_ARG, "js outside the cube's latitudes");
    if (a->jn <= a->js || a->jn >= a->ny) return chk.refuse(LEC_ERR_ARG, "jn must be js + 1 .. ny - 1 (nyb >= 2: a box needs two rows for d/dlat)");
    if (int r = chk.align16(a->rows_d, a->lattab2_d, a->coef_d)) return r;
    const void* tabs[] = {a->levraw_d, a->levtab2_d, a->lattab_d, a->levtab_d, a->tcoef_d, a->lonsec_d, a->lonsecsum_d};
    const char* tabn[] = {"levraw_d", "levtab2_d", "lattab_d", "levtab_d", "tcoef_d", "lonsec_d", "lonsecsum_d"};
    const void* cubes[] = {a->tair_d, a->u_d, a->v_d, a->omega_d};
    const int nyb = a->jn - a->js + 1, nxb = a->ie - a->iw + 1;
    if (int r = lonsec_tables_cubes_limits(chk, tabs, tabn, 7, cubes, 4, "tair_d, u_d, v_d, omega_d", a->dtype, a->t_count, a->nl, nxb, "iw, ie"))
        return r;

    FixedParams p;
    p.lattab = a->lattab_d; p.lattab2 = a->lattab2_d; p.inv_hdeg_ = a->inv_hdeg; p.iw_ = a->iw; p.js_ = a->js;
    // dT/dt over the cube's own time axis: DMODE 2
    return lonsec_launch(a, p, nyb, nxb, 0, [a](const FixedParams& q, dim3 grid, hipStream_t st) {
        if (a->ring) lonsec_col<true, 2>(q, a->dtype, grid, st);
        else lonsec_col<false, 2>(q, a->dtype, grid, st);
    });
}

extern "C" int lec_composite_lonsections(const lec_composite_lonsections_args* a) {
    const MapcolRefusals chk{"lec_composite_lonsections"};
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
    if (!a->lonsec_d) return chk.refuse(LEC_ERR_ARG, "null lonsec_d (the sections, which are the workspace of the time sums too)");
    if (!a->lonsecsum_d) return chk.refuse(LEC_ERR_ARG, "null lonsecsum_d");
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
    if (a->nxb < 3) return chk.refuse(LEC_ERR_ARG, "nxb must be >= 3 (a section needs three box columns)");
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
    const void* tabs[] = {a->levraw_d, a->levtab2_d, a->lattab_d, a->levtab_d, a->tcoef_d, a->boxtab_d, a->dTdt_d, a->lonsec_d, a->lonsecsum_d};
    const char* tabn[] = {"levraw_d", "levtab2_d", "lattab_d", "levtab_d", "tcoef_d", "boxtab_d", "dTdt_d", "lonsec_d", "lonsecsum_d"};
    const void* cubes[] = {a->tair_d, a->u_d, a->v_d, a->omega_d, a->tm_d, a->tp_d};
    const int nyb = a->nyb, nxb = a->nxb;
    if (int r = lonsec_tables_cubes_limits(chk, tabs, tabn, 9, cubes, 6, "tair_d, u_d, v_d, omega_d, tm_d, tp_d", a->dtype, a->t_count, a->nl, nxb,
                                           "nxb"))
        return r;

    MovingParams p;
    p.DT = a->dTdt_d; p.TM = a->tm_d; p.TP = a->tp_d; p.box = a->box_d; p.boxtab = a->boxtab_d; p.lattab = a->lattab_d; p.lattab2 = a->lattab2_d;
    // a moving box is an open box: no ring form
    return lonsec_launch(a, p, nyb, nxb, nyb * 8, [a, dmode](const MovingParams& q, dim3 grid, hipStream_t st) {
        if (dmode == 0) lonsec_col<false, 0>(q, a->dtype, grid, st);
        else if (dmode == 1) lonsec_col<false, 1>(q, a->dtype, grid, st);
        else lonsec_col<false, 2>(q, a->dtype, grid, st);
    });
}
