// lec_composite.hip -- lec_composite: the SYSTEM-RELATIVE composites of the six eddy terms Ae Ke Ca Ce Ck Ge over a series of per-step
// boxes of ONE shape (-t / -c --composites; include/lec_hip_ext.h).  A translation unit of its own: its code object
// is loaded by calls that ask for composites only, and lec_maps.hip is not touched by it (nothing is shared but lec_sweep.h's stencil3).
//
// The call is lec_maps (lec_maps.hip) with three things lifted to "per step": the box and its tables (box_d, lattab_d, lattab2_d, boxtab_d
// are indexed by the step), dT/dt by lec_rowstats' rule (a dT/dt cube, or T of the two time neighbours ON THE STEP'S BOX, or the cube's own
// neighbours), and the Hovmoeller weights.  Box-relative indices (j, i) take the place of the grid's.  Three kernels, as there:
//   lec_composite_coef_kernel  one wave per (time step, level), lanes over rows in trips of 64: the record of LEC_MAPS_NCOEF doubles per
//                              (t, k, j) -- zonal means, row factors of lec_level_row.inc, sigma READ from levraw -- with step t's lattab2.
//   lec_composite_col_kernel   one wave per (time step, row, 64 columns), lanes ALONG LONGITUDE, marching down the levels with T(k - 1) T(k)
//                              T(k + 1) in registers; the step's box, tables and record are wave-uniform (scalar loads).  A moving box is an
//                              open box: one-sided d/dlon at its first and last column, and nothing outside the box is read.
//   lec_composite_sum_kernel / lec_composite_hov_kernel  one thread per output element: the time sums step by step in time order, the
//                              Hovmoeller sum_j cw_j(t) C_f rows ascending.  No atomics: every element has one writer, so the numbers depend
//                              neither on the launch nor on how a series is cut into calls.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/lec_hip_ext.h"
#include "lec_internal.h"
#include "lec_sweep.h"

namespace {
using lec::dbl2_t;

constexpr double kG = LEC_G, kRe = LEC_RE, kRd = LEC_RD, kCp = LEC_CP_D;
constexpr int kNMap = LEC_NMAP;
constexpr int kNC = LEC_MAPS_NCOEF;
// the record of one (t, k, j): what a point of that row subtracts and multiplies by (lec_maps.hip's)
enum { C_MT = 0, C_MU, C_MV, C_MW, C_MQ, C_AE, C_CA1, C_CA2, C_CE, C_CK1, C_CK2, C_CK3, C_DPU, C_GE, C_USED };
static_assert(C_USED <= kNC, "the record holds the factors");
enum { M_AE = 0, M_KE, M_CA, M_CE, M_CK, M_GE };
static_assert(M_GE + 1 == kNMap, "six composites");

struct CoefParams {
    const double* rows;      // [t_count][nl][nyb][LEC_NSTAT]
    const double* lattab2;   // [t_count][nyb][8]
    const double* levtab2;   // [nl][4]
    const double* levraw;    // [t_count][nl][LEC_NLEVRAW]
    double* coef;            // [t_count][nl][nyb][kNC]
    int t_count, nl, nyb;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (t_count * nl), level fastest; block 64
__global__ void __launch_bounds__(64) lec_composite_coef_kernel(const CoefParams p) {
#pragma clang fp contract(off)
    const int nl = p.nl, nyb = p.nyb, lane = threadIdx.x;
    const int tl = blockIdx.x / nl, k = blockIdx.x - tl * nl;
    const int km = k > 0 ? k - 1 : k, kp = k < nl - 1 ? k + 1 : k;
    const size_t lstride = (size_t)nyb * LEC_NSTAT;
    const double* rec = p.rows + (size_t)(tl * nl + k) * lstride;
    const double* recm = p.rows + (size_t)(tl * nl + km) * lstride;
    const double* recp = p.rows + (size_t)(tl * nl + kp) * lstride;
    const double* lt = p.lattab2 + (size_t)tl * nyb * 8;      // the step's own box

    // the area means {[T]} of the level, of the one above and of the one below, in the order of the level stage
    double aT = 0.0, aTm = 0.0, aTp = 0.0;
    for (int j0 = 0; j0 < nyb; j0 += 64) {
        const int jb = j0 + lane, jc = min(jb, nyb - 1);
        const double t0 = rec[(size_t)jc * LEC_NSTAT], tm = recm[(size_t)jc * LEC_NSTAT], tp = recp[(size_t)jc * LEC_NSTAT];
        const double cw = lt[8 * jc + 0];
        if (jb < nyb) { aT += cw * t0; aTm += cw * tm; aTp += cw * tp; }
    }
    aT = wave_sum(aT);
    aTm = (km == k) ? aT : wave_sum(aTm);
    aTp = (kp == k) ? aT : wave_sum(aTp);

    const double pk = p.levtab2[4 * k + 0], pa = p.levtab2[4 * k + 1], pb = p.levtab2[4 * k + 2], pc = p.levtab2[4 * k + 3];
    const double sig = p.levraw[(size_t)(tl * nl + k) * LEC_NLEVRAW + LEC_LEVRAW_SIGMA];      // the clamped sigma the totals used
    const double c1k = kRd / (pk * kG);

    for (int j0 = 0; j0 < nyb; j0 += 64) {
        const int jb = j0 + lane;
        if (jb >= nyb) break;
        const int jm = jb > 0 ? jb - 1 : jb, jp = jb < nyb - 1 ? jb + 1 : jb;
        const dbl2_t* rr = reinterpret_cast<const dbl2_t*>(rec + (size_t)jb * LEC_NSTAT);
        const dbl2_t r0 = rr[0], r1 = rr[1], r2 = rr[2];
        const double mT = r0.x, mU = r0.y, mV = r1.x, mW = r1.y, mQ = r2.y;
        const dbl2_t* rm2 = reinterpret_cast<const dbl2_t*>(rec + (size_t)jm * LEC_NSTAT);
        const dbl2_t* rp2 = reinterpret_cast<const dbl2_t*>(rec + (size_t)jp * LEC_NSTAT);
        const dbl2_t m0 = rm2[0], m1 = rm2[1], q0 = rp2[0], q1 = rp2[1];
        const dbl2_t km2 = *reinterpret_cast<const dbl2_t*>(recm + (size_t)jb * LEC_NSTAT);
        const dbl2_t kp2 = *reinterpret_cast<const dbl2_t*>(recp + (size_t)jb * LEC_NSTAT);
        const dbl2_t* ll = reinterpret_cast<const dbl2_t*>(lt + (size_t)jb * 8);
        const dbl2_t L1 = ll[1], L2 = ll[2], L3 = ll[3];
        const double c = L1.x, tn = L1.y, gra = L2.x, grb = L2.y, grc = L3.x;
        const double cm = lt[8 * jm + 2], cp = lt[8 * jp + 2];
        // lec_level_row.inc, part A
        const double Ts = mT - aT;
        const double dphiTc = gra * (m0.x - aT) * cm + grb * Ts * c + grc * (q0.x - aT) * cp;
        const double dphiUc = gra * (m0.y / cm) + grb * (mU / c) + grc * (q0.y / cp);
        const double dphiV = gra * m1.x + grb * mV + grc * q1.x;
        const double dpT = pa * (km2.x - aTm) + pb * Ts + pc * (kp2.x - aTp);
        const double dpU = pa * km2.y + pb * mU + pc * kp2.y;
        double o[kNC];
#pragma unroll
        for (int i = 0; i < kNC; ++i) o[i] = 0.0;
        o[C_MT] = mT; o[C_MU] = mU; o[C_MV] = mV; o[C_MW] = mW; o[C_MQ] = mQ;
        o[C_AE] = 1.0 / (2 * sig);
        o[C_CA1] = dphiTc / (2 * kRe * sig);
        o[C_CA2] = dpT / sig;
        o[C_CE] = c1k;
        o[C_CK1] = c / kRe * dphiUc;
        o[C_CK2] = dphiV / kRe;
        o[C_CK3] = tn * mV / kRe;
        o[C_DPU] = dpU;
        o[C_GE] = 1.0 / (kCp * sig);
        dbl2_t* dst = reinterpret_cast<dbl2_t*>(p.coef + ((size_t)(tl * nl + k) * nyb + jb) * kNC);
#pragma unroll
        for (int i = 0; i < kNC / 2; ++i) { dbl2_t v; v.x = o[2 * i]; v.y = o[2 * i + 1]; dst[i] = v; }
    }
}

struct ColParams {
    const void *T, *U, *V, *W;
    const double* DT;        // the dT/dt cube (DMODE 0)
    const void *TM, *TP;     // T of the time neighbours on the step's box (DMODE 1)
    const int32_t* box;      // [t_count][4] as the cubes hold them
    const double* boxtab;    // [t_count][4]: [2] = 1 / h_deg
    const double* coef;      // [t_count][nl][nyb][kNC]
    const double* lattab;    // [t_count][nyb][4]
    const double* levtab;    // [nl][3]
    const double* levtab2;   // [nl][4]
    const double* tcoef;     // [nt][3] (DMODE 1, 2)
    double* col;             // [t_count][kNMap][nyb][nxb]
    int nt, nl, ny, nx, t_begin, t_count, nyb, nxb, nseg;
};

// one level of one term's column integral: the trapezoid over the finite levels, as lec_section_fold_kernel runs it
struct Trap { double r, xl, yl; int last; };
__device__ __forceinline__ void trap_step(Trap& s, const double x, const double y, const int k) {
#pragma clang fp contract(off)
    if (!isnan(y)) {
        if (s.last >= 0) s.r += (x - s.xl) * 0.5 * (y + s.yl);
        s.last = k; s.xl = x; s.yl = y;
    }
}

// grid (t_count * nyb * nseg), column segment fastest, then row, then time step; block 64: lane = column of the segment.
// DMODE: where dT/dt comes from -- 0 the fp64 cube DT, 1 tc[t] . (TM[t], T[t], TP[t]), 2 tc[t] . (T[t - 1], T[t], T[t + 1]) of the cube itself
template <typename E, int DMODE>
__global__ void __launch_bounds__(64) lec_composite_col_kernel(const ColParams p) {
#pragma clang fp contract(off)
    const int nx = p.nx, nl = p.nl, nyb = p.nyb, nxb = p.nxb;
    const int seg = blockIdx.x % p.nseg, tj = blockIdx.x / p.nseg;
    const int jb = tj % nyb, tl = tj / nyb;
    const int e = seg * 64 + (int)threadIdx.x;          // box column
    if (e >= nxb) return;                               // (no barrier below)
    const int t = p.t_begin + tl;
    const int iw = p.box[4 * tl + 0], js = p.box[4 * tl + 2];      // wave-uniform: the step's box (its shape was checked on the host)
    const size_t plane = (size_t)p.ny * nx, cube = plane * nl;
    const int i = iw + e;
    const bool first = e == 0, last = e == nxb - 1;
    // the lambda neighbours: an open box reads nothing outside its columns (the one-sided difference needs none)
    const int il = first ? i : i - 1, ir = last ? i : i + 1;
    const size_t row0 = (size_t)t * cube + (size_t)(js + jb) * nx;      // level 0 of the row
    const E* __restrict__ pT = (const E*)p.T + row0;
    const E* __restrict__ pU = (const E*)p.U + row0;
    const E* __restrict__ pV = (const E*)p.V + row0;
    const E* __restrict__ pW = (const E*)p.W + row0;
    const double* __restrict__ pD = DMODE == 0 ? p.DT + row0 : nullptr;
    const E* __restrict__ pM = DMODE == 1 ? (const E*)p.TM + row0 : nullptr;
    const E* __restrict__ pP = DMODE == 1 ? (const E*)p.TP + row0 : nullptr;
    // a neighbour that does not exist: the row itself, whose coefficient in the tables is 0
    const ptrdiff_t ojm = jb > 0 ? -(ptrdiff_t)nx : 0, ojp = jb < nyb - 1 ? (ptrdiff_t)nx : 0;
    const ptrdiff_t otm = t > 0 ? -(ptrdiff_t)cube : 0, otp = t < p.nt - 1 ? (ptrdiff_t)cube : 0;      // (DMODE 2)
    const double* lt = p.lattab + ((size_t)tl * nyb + jb) * 4;
    const double ga = lt[0], gb = lt[1], gc = lt[2];
    const double cx = 0.5 * p.boxtab[4 * tl + 2] * lt[3];            // centred d/dlon -> d/dx, with the step's 1 / h_deg
    double ta = 0.0, tb = 0.0, tc = 0.0;
    if (DMODE != 0) { const double* tcf = p.tcoef + (size_t)t * 3; ta = tcf[0]; tb = tcf[1]; tc = tcf[2]; }
    const double* cf = p.coef + ((size_t)tl * nl * nyb + jb) * kNC;

    Trap s[kNMap];
#pragma unroll
    for (int f = 0; f < kNMap; ++f) { s[f].r = 0.0; s[f].xl = 0.0; s[f].yl = 0.0; s[f].last = -1; }

    double Tc = (double)pT[i], Tm = Tc;
    for (int k = 0; k < nl; ++k) {
        const E* __restrict__ rT = pT + (size_t)k * plane;
        const size_t ko = (size_t)k * plane + i;
        const double Tp = k < nl - 1 ? (double)rT[plane + i] : Tc;
        const double Tl = (double)rT[il], Tr = (double)rT[ir];
        const double Tjm = (double)rT[ojm + i], Tjp = (double)rT[ojp + i];
        const double Uv = (double)pU[ko], Vv = (double)pV[ko], Wv = (double)pW[ko];
        const double* lv = p.levtab + (size_t)k * 3;
        const double al = lv[0], be = lv[1], gm = lv[2];
        const double x = p.levtab2[4 * k];
        const double* c = cf + (size_t)k * nyb * kNC;      // wave-uniform: scalar loads

        // Q / cp = dT/dt + u dT/dx + v dT/dy - S w: stage 1's expression (lec_boxtile.hip), fma form kept
        const double d = first ? 2.0 * (Tr - Tc) : (last ? 2.0 * (Tc - Tl) : Tr - Tl);      // one-sided at the box's first and last column
        const double adv = (Uv * cx) * d;
        const double sP = lec::stencil3(ga, Tjm, gc, Tjp, gb, Tc);
        const double sS = lec::stencil3(al, Tm, gm, Tp, be, Tc);
        double dTdt;
        if (DMODE == 0) dTdt = pD[ko];
        else if (DMODE == 1) dTdt = lec::stencil3(ta, (double)pM[ko], tc, (double)pP[ko], tb, Tc);
        else dTdt = lec::stencil3(ta, (double)rT[otm + i], tc, (double)rT[otp + i], tb, Tc);
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
        trap_step(s[M_AE], x, yAe, k);
        trap_step(s[M_KE], x, yKe, k);
        trap_step(s[M_CA], x, yCa, k);
        trap_step(s[M_CE], x, yCe, k);
        trap_step(s[M_CK], x, yCk, k);
        trap_step(s[M_GE], x, yGe, k);
        Tm = Tc; Tc = Tp;
    }
    double* o = p.col + ((size_t)tl * kNMap * nyb + jb) * nxb + e;
    const size_t fs = (size_t)nyb * nxb;
#pragma unroll
    for (int f = 0; f < kNMap; ++f) {
        const double div = f == M_KE ? 2 * kG : (f == M_CK ? kG : 1.0);
        o[(size_t)f * fs] = s[f].last < 0 ? nan("") : s[f].r / div;      // x / 1.0 is x
    }
}

struct FoldParams {
    const double* col;       // [t_count][kNMap][nyb][nxb]
    const double* lattab2;   // [t_count][nyb][8]
    double* mapsum;          // [kNMap][nyb][nxb], +=
    double* hov;             // [t_count][kNMap][nxb]
    int t_count, nyb, nxb;
};

// grid ceil(kNMap * nyb * nxb / 256), block 256: thread (f, j, i), columns fastest; the steps in time order.  A track's box is small and
// its series long (6 x 61 x 61 threads walking 512 steps): a thread's life is a chain of memory round trips, so the loads are issued
// kSumBatch at a time before any of them is used -- the ORDER of the sum is that of the plain loop, only the loads run ahead
constexpr int kSumBatch = 16;
__global__ void __launch_bounds__(256) lec_composite_sum_kernel(const FoldParams p) {
    const size_t n = (size_t)kNMap * p.nyb * p.nxb;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
    const double* __restrict__ c = p.col + id;
    double s = p.mapsum[id];
    for (int t0 = 0; t0 < p.t_count; t0 += kSumBatch) {
        double v[kSumBatch];
#pragma unroll
        for (int q = 0; q < kSumBatch; ++q) v[q] = c[(size_t)min(t0 + q, p.t_count - 1) * n];
#pragma unroll
        for (int q = 0; q < kSumBatch; ++q)
            if (t0 + q < p.t_count) s += v[q];
    }
    p.mapsum[id] = s;
}

// grid ceil(t_count * kNMap * nxb / 256), block 256: thread (t, f, i), columns fastest; the rows ascending, the weights step t's
constexpr int kHovBatch = 8;
__global__ void __launch_bounds__(256) lec_composite_hov_kernel(const FoldParams p) {
#pragma clang fp contract(off)
    const size_t n = (size_t)p.t_count * kNMap * p.nxb;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
    const size_t tf = id / p.nxb, i = id - tf * p.nxb;
    const double* __restrict__ c = p.col + tf * p.nyb * p.nxb + i;
    const double* __restrict__ lt = p.lattab2 + (tf / kNMap) * (size_t)p.nyb * 8;
    // the loads are issued kHovBatch at a time before any of them is used (lec_maps_hov_kernel's remedy): the ORDER of the sum is that of
    // the plain loop, only the loads run ahead
    double s = 0.0;
    for (int j0 = 0; j0 < p.nyb; j0 += kHovBatch) {
        double v[kHovBatch], w[kHovBatch];
#pragma unroll
        for (int q = 0; q < kHovBatch; ++q) {
            const int j = min(j0 + q, p.nyb - 1);
            v[q] = c[(size_t)j * p.nxb];
            w[q] = lt[8 * j];
        }
#pragma unroll
        for (int q = 0; q < kHovBatch; ++q)
            if (j0 + q < p.nyb) s += w[q] * v[q];
    }
    p.hov[id] = s;
}

int refuse(int code, const char* what) {
    char msg[320];
    snprintf(msg, sizeof(msg), "lec_composite: %s", what);
    return lec_set_error(code, msg);
}

template <typename E>
void launch_col(const ColParams& p, int dmode, unsigned nblk, hipStream_t st) {
    if (dmode == 0) hipLaunchKernelGGL((lec_composite_col_kernel<E, 0>), dim3(nblk), dim3(64), 0, st, p);
    else if (dmode == 1) hipLaunchKernelGGL((lec_composite_col_kernel<E, 1>), dim3(nblk), dim3(64), 0, st, p);
    else hipLaunchKernelGGL((lec_composite_col_kernel<E, 2>), dim3(nblk), dim3(64), 0, st, p);
}

}  // namespace

extern "C" int lec_composite(const lec_composite_args* a) {
    if (!a) return refuse(LEC_ERR_ARG, "null args");
    if (!a->tair_d) return refuse(LEC_ERR_ARG, "null tair_d");
    if (!a->u_d) return refuse(LEC_ERR_ARG, "null u_d");
    if (!a->v_d) return refuse(LEC_ERR_ARG, "null v_d");
    if (!a->omega_d) return refuse(LEC_ERR_ARG, "null omega_d");
    if (!a->box_h) return refuse(LEC_ERR_ARG, "null box_h (the host copy of the boxes: their shapes are checked before anything is launched)");
    if (!a->box_d) return refuse(LEC_ERR_ARG, "null box_d");
    if (!a->boxtab_d) return refuse(LEC_ERR_ARG, "null boxtab_d");
    if (!a->lattab_d) return refuse(LEC_ERR_ARG, "null lattab_d");
    if (!a->lattab2_d) return refuse(LEC_ERR_ARG, "null lattab2_d");
    if (!a->rows_d) return refuse(LEC_ERR_ARG, "null rows_d");
    if (!a->levraw_d) return refuse(LEC_ERR_ARG, "null levraw_d");
    if (!a->levtab_d) return refuse(LEC_ERR_ARG, "null levtab_d");
    if (!a->levtab2_d) return refuse(LEC_ERR_ARG, "null levtab2_d");
    if (!a->coef_d) return refuse(LEC_ERR_ARG, "null coef_d (the workspace of the row factors)");
    if (!a->col_d) return refuse(LEC_ERR_ARG, "null col_d (the column values, which are the workspace of the sums too)");
    if (!a->hov_d) return refuse(LEC_ERR_ARG, "null hov_d");
    if (!a->mapsum_d) return refuse(LEC_ERR_ARG, "null mapsum_d");
    if (a->dtype != LEC_F64 && a->dtype != LEC_F32) return refuse(LEC_ERR_ARG, "dtype must be LEC_F64 or LEC_F32");
    if (a->reserved0 != 0) return refuse(LEC_ERR_ARG, "reserved0 must be 0");
    // dT/dt by lec_rowstats' rule
    if ((a->tm_d != nullptr) != (a->tp_d != nullptr))
        return refuse(LEC_ERR_ARG, a->tm_d ? "tm_d without tp_d (a box-packed series needs both time neighbours)"
                                           : "tp_d without tm_d (a box-packed series needs both time neighbours)");
    if (a->dTdt_d && a->tm_d) return refuse(LEC_ERR_ARG, "dTdt_d together with tm_d / tp_d: give one source of dT/dt");
    if (!a->dTdt_d && !a->tcoef_d) return refuse(LEC_ERR_ARG, "null tcoef_d without dTdt_d: no source of dT/dt");
    const int dmode = a->dTdt_d ? 0 : (a->tm_d ? 1 : 2);
    if (a->nt < 1) return refuse(LEC_ERR_ARG, "nt must be >= 1");
    if (dmode == 2 && a->nt < 2) return refuse(LEC_ERR_ARG, "nt must be >= 2 when dT/dt comes from the cube's own time neighbours (no dTdt_d, tm_d / tp_d)");
    if (a->nl < 2) return refuse(LEC_ERR_ARG, "nl must be >= 2 (a column integral needs two levels)");
    if (a->nl > LEC_MAX_LEVELS) return refuse(LEC_ERR_UNSUPPORTED, "nl above LEC_MAX_LEVELS (160)");
    if (a->nyb < 2) return refuse(LEC_ERR_ARG, "nyb must be >= 2 (a box needs two rows for d/dlat)");
    if (a->nxb < 3) return refuse(LEC_ERR_ARG, "nxb must be >= 3 (a composite needs three box columns)");
    if (a->ny < a->nyb) return refuse(LEC_ERR_ARG, "ny must be >= nyb");
    if (a->nx < a->nxb) return refuse(LEC_ERR_ARG, "nx must be >= nxb");
    if (a->t_begin < 0 || a->t_begin >= a->nt) return refuse(LEC_ERR_ARG, "t_begin outside the cube");
    if (a->t_count < 1 || a->t_count > a->nt - a->t_begin) return refuse(LEC_ERR_ARG, "t_count: [t_begin, t_begin + t_count) outside the cube");
    // every box nyb x nxb and inside the cube: on the HOST copy, before any HIP call
    for (int t = 0; t < a->t_count; ++t) {
        const int32_t* b = a->box_h + 4 * (size_t)t;
        const long long w = (long long)b[1] - b[0] + 1, h = (long long)b[3] - b[2] + 1;
        char m[256];
        if (w != a->nxb || h != a->nyb) {
            snprintf(m, sizeof(m), "box_h: the box of step %d is %lld x %lld (rows x columns), the call's nyb x nxb is %d x %d: every box of a "
                     "composite has one shape", t, h, w, a->nyb, a->nxb);
            return refuse(LEC_ERR_ARG, m);
        }
        if (b[0] < 0 || b[1] >= a->nx || b[2] < 0 || b[3] >= a->ny) {
            snprintf(m, sizeof(m), "box_h: the box of step %d {iw, ie, js, jn} = {%d, %d, %d, %d} lies outside the %d x %d cube", t, b[0], b[1],
                     b[2], b[3], a->ny, a->nx);
            return refuse(LEC_ERR_ARG, m);
        }
    }
    if ((uintptr_t)a->rows_d % 16) return refuse(LEC_ERR_ARG, "rows_d must be 16-byte aligned");
    if ((uintptr_t)a->lattab2_d % 16) return refuse(LEC_ERR_ARG, "lattab2_d must be 16-byte aligned");
    if ((uintptr_t)a->coef_d % 16) return refuse(LEC_ERR_ARG, "coef_d must be 16-byte aligned");
    if ((uintptr_t)a->box_d % 4) return refuse(LEC_ERR_ARG, "box_d must be 4-byte aligned");
    if ((uintptr_t)a->box_h % 4) return refuse(LEC_ERR_ARG, "box_h must be 4-byte aligned");
    const void* tabs[] = {a->levraw_d, a->levtab2_d, a->lattab_d, a->levtab_d, a->tcoef_d, a->boxtab_d, a->dTdt_d, a->col_d, a->hov_d, a->mapsum_d};
    const char* tabn[] = {"levraw_d", "levtab2_d", "lattab_d", "levtab_d", "tcoef_d", "boxtab_d", "dTdt_d", "col_d", "hov_d", "mapsum_d"};
    for (int i = 0; i < 10; ++i)
        if ((uintptr_t)tabs[i] % 8) {
            char m[64];
            snprintf(m, sizeof(m), "%s must be 8-byte aligned", tabn[i]);
            return refuse(LEC_ERR_ARG, m);
        }
    const size_t esz = a->dtype == LEC_F32 ? 4 : 8;
    const void* cubes[6] = {a->tair_d, a->u_d, a->v_d, a->omega_d, a->tm_d, a->tp_d};
    for (const void* c : cubes)
        if ((uintptr_t)c % esz) return refuse(LEC_ERR_ARG, "cube pointer (tair_d, u_d, v_d, omega_d, tm_d, tp_d) not aligned to its element size");
    const int nyb = a->nyb, nxb = a->nxb, nseg = (nxb + 63) / 64;
    // HIP takes fewer than 2^32 threads per launch (lec_maps' limits)
    if ((long long)a->t_count * a->nl >= (1LL << 26))
        return refuse(LEC_ERR_UNSUPPORTED, "t_count * nl must stay below 2^26 in one call (cut the series into several calls)");
    if ((long long)a->t_count * nyb * nseg >= (1LL << 26))
        return refuse(LEC_ERR_UNSUPPORTED, "t_count * rows * ceil(columns / 64) must stay below 2^26 in one call (cut the series into several calls)");
    if ((long long)kNMap * nyb * nxb >= (1LL << 32) - 256)
        return refuse(LEC_ERR_UNSUPPORTED, "6 * rows * columns (nyb, nxb) must stay below 2^32 threads");
    if ((long long)a->t_count * kNMap * nxb >= (1LL << 32) - 256)
        return refuse(LEC_ERR_UNSUPPORTED, "t_count * 6 * columns must stay below 2^32 threads in one call");

    hipStream_t st = (hipStream_t)a->stream;
    CoefParams c;
    c.rows = a->rows_d; c.lattab2 = a->lattab2_d; c.levtab2 = a->levtab2_d; c.levraw = a->levraw_d; c.coef = a->coef_d;
    c.t_count = a->t_count; c.nl = a->nl; c.nyb = nyb;
    hipLaunchKernelGGL(lec_composite_coef_kernel, dim3((unsigned)(a->t_count * a->nl)), dim3(64), 0, st, c);

    ColParams p;
    p.T = a->tair_d; p.U = a->u_d; p.V = a->v_d; p.W = a->omega_d; p.DT = a->dTdt_d; p.TM = a->tm_d; p.TP = a->tp_d;
    p.box = a->box_d; p.boxtab = a->boxtab_d;
    p.coef = a->coef_d; p.lattab = a->lattab_d; p.levtab = a->levtab_d; p.levtab2 = a->levtab2_d; p.tcoef = a->tcoef_d;
    p.col = a->col_d;
    p.nt = a->nt; p.nl = a->nl; p.ny = a->ny; p.nx = a->nx; p.t_begin = a->t_begin; p.t_count = a->t_count;
    p.nyb = nyb; p.nxb = nxb; p.nseg = nseg;
    const unsigned nblk = (unsigned)((long long)a->t_count * nyb * nseg);
    if (a->dtype == LEC_F64) launch_col<double>(p, dmode, nblk, st);
    else launch_col<float>(p, dmode, nblk, st);

    FoldParams f;
    f.col = a->col_d; f.lattab2 = a->lattab2_d; f.mapsum = a->mapsum_d; f.hov = a->hov_d;
    f.t_count = a->t_count; f.nyb = nyb; f.nxb = nxb;
    hipLaunchKernelGGL(lec_composite_sum_kernel, dim3((unsigned)(((long long)kNMap * nyb * nxb + 255) / 256)), dim3(256), 0, st, f);
    hipLaunchKernelGGL(lec_composite_hov_kernel, dim3((unsigned)(((long long)a->t_count * kNMap * nxb + 255) / 256)), dim3(256), 0, st, f);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}
