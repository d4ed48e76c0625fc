// lec_mapcol.h -- what lec_maps (lec_maps.hip), lec_composite (lec_composite.hip), lec_composite_steps (lec_composite_steps.hip) and the two
// calls of lec_lonsections.hip share: the column integrals C_f(t, j, i) of the six eddy terms Ae Ke Ca Ce Ck Ge at the points of a box, their
// time sums and their Hovmoeller rows (DESIGN.md sections 4.2d, 4.2e, 4.2g, 4.2h).  The record layout, the trapezoid rule, the launches of a
// call (mapcol_launch) and the refusals the calls have in common (MapcolRefusals) are written once, here; the Q expression and the
// integrands of a point once in lec_mapcol_point.inc, which the column kernel here and lec_lonsections.hip's row-march kernel include.  The
// kernels have internal linkage and the column kernel is a template over the including file's launch struct, so each of the files
// instantiates kernels of its own and remains a code object of its own.
//   lec_mapcol_coef_kernel  one wave per (time step, level), lanes over rows in trips of 64: the area means in the order of the level stage
//                  (lec_section_rows_kernel's), the row factors dphiTc dphiUc dphiV dpT dpU of lec_level_row.inc, and with sigma READ from
//                  the levraw record everything a point multiplies by, as one record of LEC_MAPS_NCOEF doubles per (t, k, j).
//   lec_mapcol_col_kernel<E, RING, DMODE, P>  one wave per (time step, row, 64 columns), lanes ALONG LONGITUDE, marching down the levels with
//                  T(k - 1) T(k) T(k + 1) in registers: Q is stage_row's expression (lec_rowspecq.hip; one-sided at the ends of an open box as
//                  sweep_one, lec_sweep.h), and the vertical trapezoid with the NaN rule runs in registers with a running "last finite
//                  level" per term (lec_section_fold_kernel's rule).  The level march IS the kernel's body; the file's P resolves the box
//                  of a step through four small members.  (A __device__ march called from a kernel of each file was tried first: the
//                  compiler optimises a callee on its own before it inlines it, and the trapezoid steps came out if-converted, the
//                  fp64 composites 4 % slower.  With the march in the kernel the instructions are the former kernels'.)
//   lec_mapcol_sum_kernel / lec_mapcol_hov_kernel  one thread per output element: the time sums step by step in time order, the Hovmoeller
//                  sum_j cw_j(t) C_f rows ascending.  No atomics: every element has one writer, so the numbers depend neither on the launch
//                  nor on how a series is cut into calls.
// Contraction is off in every kernel, and Q keeps its explicit fma / stencil3 form: the numbers are those of the two files' former own
// copies, bit for bit.  No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/lec_hip.h"
#include "lec_internal.h"
#include "lec_sweep.h"

namespace lec {

constexpr int kNMap = LEC_NMAP;
constexpr int kNC = LEC_MAPS_NCOEF;
// the record of one (t, k, j): what a point of that row subtracts and multiplies by
enum { C_MT = 0, C_MU, C_MV, C_MW, C_MQ, C_AE, C_CA1, C_CA2, C_CE, C_CK1, C_CK2, C_CK3, C_DPU, C_GE, C_USED };
static_assert(C_USED <= kNC, "the record holds the factors");
enum { M_AE = 0, M_KE, M_CA, M_CE, M_CK, M_GE };
static_assert(M_GE + 1 == kNMap, "six maps");

struct MapCoefParams {
    const double* rows;      // [t_count][nl][nyb][LEC_NSTAT]
    const double* lattab2;   // step t's [nyb][8] at lattab2 + t * lt_stride
    const double* levtab2;   // [nl][4]
    const double* levraw;    // [t_count][nl][LEC_NLEVRAW]
    double* coef;            // [t_count][nl][nyb][kNC]
    int t_count, nl, nyb;
    int lt_stride;           // 0: one box for every step (lec_maps); nyb * 8: the step's own (lec_composite)
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the kernels: internal to the file that includes this header, so each file's code object has its own
namespace {

// the factors: grid (t_count * nl), level fastest; block 64: one wave per (time step, level), lanes over rows in trips of 64
__global__ void __launch_bounds__(64) lec_mapcol_coef_kernel(const MapCoefParams p) {
#pragma clang fp contract(off)
    constexpr double kG = LEC_G, kRe = LEC_RE, kRd = LEC_RD, kCp = LEC_CP_D;
    const int nl = p.nl, nyb = p.nyb, lane = threadIdx.x;
    const int tl = blockIdx.x / nl, k = blockIdx.x - tl * nl;
    const int km = k > 0 ? k - 1 : k, kp = k < nl - 1 ? k + 1 : k;
    const size_t lstride = (size_t)nyb * LEC_NSTAT;
    const double* rec = p.rows + (size_t)(tl * nl + k) * lstride;
    const double* recm = p.rows + (size_t)(tl * nl + km) * lstride;
    const double* recp = p.rows + (size_t)(tl * nl + kp) * lstride;
    const double* lt = p.lattab2 + (size_t)tl * p.lt_stride;

    // the area means {[T]} of the level, of the one above and of the one below: the products and the order of the level stage (running
    // sums of a lane over its 64-row trips, then the xor butterfly), as lec_section_rows_kernel forms them
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

// one level of one term's column integral: the trapezoid over the finite levels, as lec_section_fold_kernel runs it
struct Trap { double r, xl, yl; int last; };
__device__ __forceinline__ void trap_step(Trap& s, const double x, const double y, const int k) {
#pragma clang fp contract(off)
    if (!isnan(y)) {
        if (s.last >= 0) s.r += (x - s.xl) * 0.5 * (y + s.yl);
        s.last = k; s.xl = x; s.yl = y;
    }
}

// what the launch of a column kernel carries, whichever call it serves.  A file's own launch struct P derives from it and adds what
// resolves the geometry of its boxes, wave-uniform, for the call's step tl:
//   int iw(tl), js(tl)                        the grid column and row of the box's first point
//   const double* lattab_row(tl, jb)          the [4] entry of box row jb: the d/dlat triple and the d/dlon -> d/dx factor
//   double inv_hdeg(tl)                       1 / h_deg of the box
// and the members a DMODE reads: DT (0), TM and TP (1), step (3)
struct MapColGrid {
    const void *T, *U, *V, *W;
    const double* coef;      // [t_count][nl][nyb][kNC]
    const double* levtab;    // [nl][3]
    const double* levtab2;   // [nl][4]
    const double* tcoef;     // [nt][3] (DMODE 1, 2); [t_count][3], by box (DMODE 3)
    double* col;             // [t_count][kNMap][nyb][nxb]
    int nt, nl, ny, nx, t_begin, t_count, nyb, nxb, nseg;
};

// the column values C_f(t, j, i): grid (t_count * nyb * nseg), column segment fastest, then row, then time step; block 64: one wave per
// (time step, row, 64 columns), lanes ALONG LONGITUDE (every cube load is a row segment), marching down the levels with T(k - 1) T(k)
// T(k + 1) in registers; the box, its tables and the record of (t, k, j) are wave-uniform (scalar loads).
// RING: lambda wraps; otherwise the box is open: one-sided d/dlon at its first and last column, nothing outside its columns is read.
// DMODE: where dT/dt comes from -- 0 the fp64 cube DT, 1 tc[t] . (TM[t], T[t], TP[t]), 2 tc[t] . (T[t - 1], T[t], T[t + 1]) of the cube itself,
// 3 a step table (lec_composite_steps): box tl reads cube step p.step[tl][0] and tc[tl] . (T[step[tl][1]], T[t], T[step[tl][2]]), DMODE 2's
// expression; an entry outside [0, nt) reads nothing and the box's columns are NaN
template <typename E, bool RING, int DMODE, typename P>
__global__ void __launch_bounds__(64) lec_mapcol_col_kernel(const P p) {
#pragma clang fp contract(off)
    constexpr double kG = LEC_G, kCp = LEC_CP_D;
    const int nx = p.nx, nl = p.nl, nyb = p.nyb, nxb = p.nxb;
    const int seg = blockIdx.x % p.nseg, tj = blockIdx.x / p.nseg;
    const int jb = tj % nyb, tl = tj / nyb;
    const int e = seg * 64 + (int)threadIdx.x;          // box column
    if (e >= nxb) return;                               // (no barrier below)
    // (DMODE 3) the table's row of box tl: wave-uniform, scalar loads.  A row with an entry outside the cube marches over no level at all:
    // nothing of the cubes is read, and a column without a finite level is NaN
    int st = 0, stm = 0, stp = 0;
    bool off_cube = false;
    if constexpr (DMODE == 3) {
        const int32_t* sr = p.step + 3 * (size_t)tl;
        st = sr[0]; stm = sr[1]; stp = sr[2];
        off_cube = (unsigned)st >= (unsigned)p.nt || (unsigned)stm >= (unsigned)p.nt || (unsigned)stp >= (unsigned)p.nt;
        if (off_cube) st = stm = stp = 0;
    }
    const int t = DMODE == 3 ? st : p.t_begin + tl;
    const size_t plane = (size_t)p.ny * nx, cube = plane * nl;
    const int i = p.iw(tl) + e;
    const bool first = e == 0, last = e == nxb - 1;
    // the lambda neighbours: wrapped on a ring; an open box reads nothing outside its columns (the one-sided difference needs none)
    const int il = RING ? (i == 0 ? nx - 1 : i - 1) : (first ? i : i - 1);
    const int ir = RING ? (i == nx - 1 ? 0 : i + 1) : (last ? i : i + 1);
    const size_t row0 = (size_t)t * cube + (size_t)(p.js(tl) + jb) * nx;      // level 0 of the row
    const E* __restrict__ pT = (const E*)p.T + row0;
    const E* __restrict__ pU = (const E*)p.U + row0;
    const E* __restrict__ pV = (const E*)p.V + row0;
    const E* __restrict__ pW = (const E*)p.W + row0;
    const double* __restrict__ pD = nullptr;
    const E* __restrict__ pM = nullptr;
    const E* __restrict__ pP = nullptr;
    if constexpr (DMODE == 0) pD = p.DT + row0;
    if constexpr (DMODE == 1) { pM = (const E*)p.TM + row0; pP = (const E*)p.TP + row0; }
    // a neighbour that does not exist: the row itself, whose coefficient in the tables is 0
    const ptrdiff_t ojm = jb > 0 ? -(ptrdiff_t)nx : 0, ojp = jb < nyb - 1 ? (ptrdiff_t)nx : 0;
    // from T[t] to its time neighbours (DMODE 2; 3: those the table names)
    const ptrdiff_t otm = DMODE == 3 ? (ptrdiff_t)(stm - st) * (ptrdiff_t)cube : (t > 0 ? -(ptrdiff_t)cube : 0);
    const ptrdiff_t otp = DMODE == 3 ? (ptrdiff_t)(stp - st) * (ptrdiff_t)cube : (t < p.nt - 1 ? (ptrdiff_t)cube : 0);
    const double* lt = p.lattab_row(tl, jb);
    const double ga = lt[0], gb = lt[1], gc = lt[2];
    const double cx = 0.5 * p.inv_hdeg(tl) * lt[3];            // centred d/dlon -> d/dx
    double ta = 0.0, tb = 0.0, tc = 0.0;
    if (DMODE != 0) { const double* tcf = p.tcoef + (size_t)(DMODE == 3 ? tl : t) * 3; ta = tcf[0]; tb = tcf[1]; tc = tcf[2]; }
    const double* cf = p.coef + ((size_t)tl * nl * nyb + jb) * kNC;

    Trap s[kNMap];
#pragma unroll
    for (int f = 0; f < kNMap; ++f) { s[f].r = 0.0; s[f].xl = 0.0; s[f].yl = 0.0; s[f].last = -1; }

    const bool skip = DMODE == 3 && off_cube;
    double Tc = skip ? 0.0 : (double)pT[i], Tm = Tc;
    for (int k = 0; k < (skip ? 0 : nl); ++k) {
        const E* __restrict__ rT = pT + (size_t)k * plane;
        const size_t po = (size_t)k * plane + i;
        const double Tp = k < nl - 1 ? (double)rT[plane + i] : Tc;
        const double Tl = (double)rT[il], Tr = (double)rT[ir];
        const double Tjm = (double)rT[ojm + i], Tjp = (double)rT[ojp + i];
        const double Uv = (double)pU[po], Vv = (double)pV[po], Wv = (double)pW[po];
        const double* lv = p.levtab + (size_t)k * 3;
        const double al = lv[0], be = lv[1], gm = lv[2];
        const double x = p.levtab2[4 * k];
        const double* c = cf + (size_t)k * nyb * kNC;      // wave-uniform: scalar loads

#include "lec_mapcol_point.inc"
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

struct MapFoldParams {
    const double* col;       // [t_count][kNMap][nyb][nxb]
    const double* lattab2;   // step t's [nyb][8] at lattab2 + t * lt_stride
    double* mapsum;          // [kNMap][nyb][nxb], +=
    double* hov;             // [t_count][kNMap][nxb]
    int t_count, nyb, nxb;
    int lt_stride;           // 0: one box for every step (lec_maps); nyb * 8: the step's own (lec_composite)
};

// grid ceil(kNMap * nyb * nxb / 256), block 256: thread (f, j, i), columns fastest; the steps in time order.  A track's box is small and
// its series long (6 x 61 x 61 threads walking 512 steps): a thread's life is a chain of memory round trips, so the loads are issued
// kSumBatch at a time before any of them is used -- the ORDER of the sum is that of the plain loop, only the loads run ahead
constexpr int kSumBatch = 16;
__global__ void __launch_bounds__(256) lec_mapcol_sum_kernel(const MapFoldParams p) {
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

// grid ceil(t_count * kNMap * nxb / 256), block 256: thread (t, f, i), columns fastest; the rows ascending, the weights step t's.  The
// loads are issued kHovBatch at a time before any of them is used (lec_section_fold_kernel's remedy), the order of the sum kept
constexpr int kHovBatch = 8;
__global__ void __launch_bounds__(256) lec_mapcol_hov_kernel(const MapFoldParams p) {
#pragma clang fp contract(off)
    const size_t n = (size_t)p.t_count * kNMap * p.nxb;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
    const size_t tf = id / p.nxb, i = id - tf * p.nxb;
    const double* __restrict__ c = p.col + tf * p.nyb * p.nxb + i;
    const double* __restrict__ lt = p.lattab2 + (tf / kNMap) * (size_t)p.lt_stride;
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

// the column kernel of a file's launch struct P for the cubes' storage dtype
template <bool RING, int DMODE, typename P>
void mapcol_col(const P& p, const int dtype, const dim3 grid, hipStream_t st) {
    if (dtype == LEC_F64) hipLaunchKernelGGL((lec_mapcol_col_kernel<double, RING, DMODE, P>), grid, dim3(64), 0, st, p);
    else hipLaunchKernelGGL((lec_mapcol_col_kernel<float, RING, DMODE, P>), grid, dim3(64), 0, st, p);
}

// what differs between the calls of the family at launch: the per-step output [t_count][kNMap][ext][nxb] and the target of its time sums,
// the extent the column grid and the sum kernel run over (the box's rows nyb for maps and composites, the levels nl for the longitude x
// pressure sections), the Hovmoeller rows (null: no such launch), and the call's steps
struct MapcolRun {
    double *step, *sum, *hov;
    int ext, t_begin, t_count;
};

// the launches of a call on its stream: the factors, the file's column kernel, the time sums and (r.hov) the Hovmoeller rows.  A: the
// call's args struct, whose common fields are read by name; p: the file's column launch struct with its own members set; lt_stride:
// doubles from one step's lattab2 to the next; launch_col(p, grid, stream) picks the file's kernel, RING and DMODE; launch_sum(f, stream)
// the file's time sums of the per-step output
template <typename A, typename P, typename L, typename S>
int mapcol_launch(const A* a, P p, const MapcolRun r, const int nyb, const int nxb, const int lt_stride, L launch_col, S launch_sum) {
    hipStream_t st = (hipStream_t)a->stream;
    const MapCoefParams c{a->rows_d, a->lattab2_d, a->levtab2_d, a->levraw_d, a->coef_d, r.t_count, a->nl, nyb, lt_stride};
    hipLaunchKernelGGL(lec_mapcol_coef_kernel, dim3((unsigned)(r.t_count * a->nl)), dim3(64), 0, st, c);
    p.T = a->tair_d; p.U = a->u_d; p.V = a->v_d; p.W = a->omega_d;
    p.coef = a->coef_d; p.levtab = a->levtab_d; p.levtab2 = a->levtab2_d; p.tcoef = a->tcoef_d; p.col = r.step;
    p.nt = a->nt; p.nl = a->nl; p.ny = a->ny; p.nx = a->nx; p.t_begin = r.t_begin; p.t_count = r.t_count;
    p.nyb = nyb; p.nxb = nxb; p.nseg = (nxb + 63) / 64;
    launch_col(p, dim3((unsigned)((long long)r.t_count * r.ext * p.nseg)), st);
    // lec_mapcol_sum_kernel is generic over its element count: for the sections nl stands where the maps have nyb (lattab2, hov not read)
    const MapFoldParams f{r.step, a->lattab2_d, r.sum, r.hov, r.t_count, r.ext, nxb, lt_stride};
    launch_sum(f, st);
    if (r.hov)
        hipLaunchKernelGGL(lec_mapcol_hov_kernel, dim3((unsigned)(((long long)r.t_count * kNMap * nxb + 255) / 256)), dim3(256), 0, st, f);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}

// every call but lec_composite_steps: ONE time sum over all the call's steps
template <typename A, typename P, typename L>
int mapcol_launch(const A* a, P p, const MapcolRun r, const int nyb, const int nxb, const int lt_stride, L launch_col) {
    return mapcol_launch(a, p, r, nyb, nxb, lt_stride, launch_col, [r, nxb](const MapFoldParams& f, hipStream_t st) {
        hipLaunchKernelGGL(lec_mapcol_sum_kernel, dim3((unsigned)(((long long)kNMap * r.ext * nxb + 255) / 256)), dim3(256), 0, st, f);
    });
}

}  // namespace

// the refusals the calls of the family have in common, under the call's name.  Each returns LEC_OK or the refusal's code; the calls run
// them between their own, in the order their messages have always come.  Members templated on A read the args struct's fields by name
struct MapcolRefusals {
    const char* call;      // "lec_maps", "lec_composite", ...

    int refuse(int code, const char* what) const {
        char msg[320];
        snprintf(msg, sizeof(msg), "%s: %s", call, what);
        return lec_set_error(code, msg);
    }
    int dtype(int dtype) const {
        if (dtype != LEC_F64 && dtype != LEC_F32) return refuse(LEC_ERR_ARG, "dtype must be LEC_F64 or LEC_F32");
        return LEC_OK;
    }
    int levels(int nl) const {
        if (nl < 2) return refuse(LEC_ERR_ARG, "nl must be >= 2 (a column integral needs two levels)");
        if (nl > LEC_MAX_LEVELS) return refuse(LEC_ERR_UNSUPPORTED, "nl above LEC_MAX_LEVELS (160)");
        return LEC_OK;
    }
    int steps(int nt, int t_begin, int t_count) const {
        if (t_begin < 0 || t_begin >= nt) return refuse(LEC_ERR_ARG, "t_begin outside the cube");
        if (t_count < 1 || t_count > nt - t_begin) return refuse(LEC_ERR_ARG, "t_count: [t_begin, t_begin + t_count) outside the cube");
        return LEC_OK;
    }
    int align16(const void* rows_d, const void* lattab2_d, const void* coef_d) const {
        if ((uintptr_t)rows_d % 16) return refuse(LEC_ERR_ARG, "rows_d must be 16-byte aligned");
        if ((uintptr_t)lattab2_d % 16) return refuse(LEC_ERR_ARG, "lattab2_d must be 16-byte aligned");
        if ((uintptr_t)coef_d % 16) return refuse(LEC_ERR_ARG, "coef_d must be 16-byte aligned");
        return LEC_OK;
    }
    // the first null of ptrs[n] under its message
    int nulls(const void* const* ptrs, const char* const* what, int n) const {
        for (int i = 0; i < n; ++i)
            if (!ptrs[i]) return refuse(LEC_ERR_ARG, what[i]);
        return LEC_OK;
    }
    // a FIXED box (lec_maps, lec_lonsections), a non-null: the inputs, the call's outputs outs[nout] under their messages, then the cube,
    // the steps and the box.  few_cols, few_rows: the call's words for a box of fewer than three columns and of fewer than two rows
    template <typename A>
    int fixed_box(const A* a, const void* const* outs, const char* const* out_null, int nout, const char* few_cols, const char* few_rows) const {
        const void* in[] = {a->tair_d, a->u_d, a->v_d, a->omega_d, a->rows_d, a->levraw_d, a->lattab2_d, a->levtab2_d, a->lattab_d, a->levtab_d,
                            a->tcoef_d, a->coef_d};
        const char* in_null[] = {"null tair_d", "null u_d", "null v_d", "null omega_d", "null rows_d", "null levraw_d", "null lattab2_d",
                                 "null levtab2_d", "null lattab_d", "null levtab_d",
                                 "null tcoef_d (a dT/dt cube is not supported: dT/dt comes from the cube's time axis)",
                                 "null coef_d (the workspace of the row factors)"};
        if (int r = nulls(in, in_null, 12)) return r;
        if (int r = nulls(outs, out_null, nout)) return r;
        if (int r = dtype(a->dtype)) return r;
        if (a->ring != 0 && a->ring != 1) return refuse(LEC_ERR_ARG, "ring must be 0 or 1");
        if (a->reserved0 != 0) return refuse(LEC_ERR_ARG, "reserved0 must be 0");
        if (a->nt < 2) return refuse(LEC_ERR_ARG, "nt must be >= 2 (dT/dt by finite differences over the cube's time axis)");
        if (int r = levels(a->nl)) return r;
        if (a->ny < 2) return refuse(LEC_ERR_ARG, "ny must be >= 2");
        if (a->nx < 3) return refuse(LEC_ERR_ARG, "nx must be >= 3");
        if (int r = steps(a->nt, a->t_begin, a->t_count)) return r;
        if (a->iw < 0 || a->iw >= a->nx) return refuse(LEC_ERR_ARG, "iw outside the cube's longitudes");
        if (a->ie < a->iw || a->ie >= a->nx) return refuse(LEC_ERR_ARG, "ie must be iw .. nx - 1");
        if (a->ie - a->iw + 1 < 3) return refuse(LEC_ERR_ARG, few_cols);
        if (a->ring && (a->iw != 0 || a->ie != a->nx - 1)) return refuse(LEC_ERR_ARG, "ring: iw .. ie must be 0 .. nx - 1 (a ring is the whole circle)");
        if (a->js < 0 || a->js >= a->ny) return refuse(LEC_ERR_ARG, "js outside the cube's latitudes");
        if (a->jn <= a->js || a->jn >= a->ny) return refuse(LEC_ERR_ARG, few_rows);
        return align16(a->rows_d, a->lattab2_d, a->coef_d);
    }
    // dT/dt by lec_rowstats' rule (lec_composite, lec_composite_lonsections): one source, and a cube long enough for it.  *dmode: the
    // column kernel's DMODE
    template <typename A>
    int dTdt_source(const A* a, int* dmode) const {
        if ((a->tm_d != nullptr) != (a->tp_d != nullptr))
            return refuse(LEC_ERR_ARG, a->tm_d ? "tm_d without tp_d (a box-packed series needs both time neighbours)"
                                               : "tp_d without tm_d (a box-packed series needs both time neighbours)");
        if (a->dTdt_d && a->tm_d) return refuse(LEC_ERR_ARG, "dTdt_d together with tm_d / tp_d: give one source of dT/dt");
        if (!a->dTdt_d && !a->tcoef_d) return refuse(LEC_ERR_ARG, "null tcoef_d without dTdt_d: no source of dT/dt");
        *dmode = a->dTdt_d ? 0 : (a->tm_d ? 1 : 2);
        if (a->nt < 1) return refuse(LEC_ERR_ARG, "nt must be >= 1");
        if (*dmode == 2 && a->nt < 2)
            return refuse(LEC_ERR_ARG, "nt must be >= 2 when dT/dt comes from the cube's own time neighbours (no dTdt_d, tm_d / tp_d)");
        return LEC_OK;
    }
    // a series of MOVING boxes (lec_composite, lec_composite_lonsections), a non-null: fixed_box's counterpart.  few_cols: the call's words
    // for boxes of fewer than three columns; *dmode: dTdt_source's
    template <typename A>
    int moving_boxes(const A* a, const void* const* outs, const char* const* out_null, int nout, const char* few_cols, int* dmode) const {
        const void* in[] = {a->tair_d, a->u_d, a->v_d, a->omega_d, a->box_h, a->box_d, a->boxtab_d, a->lattab_d, a->lattab2_d, a->rows_d,
                            a->levraw_d, a->levtab_d, a->levtab2_d, a->coef_d};
        const char* in_null[] = {"null tair_d", "null u_d", "null v_d", "null omega_d",
                                 "null box_h (the host copy of the boxes: their shapes are checked before anything is launched)", "null box_d",
                                 "null boxtab_d", "null lattab_d", "null lattab2_d", "null rows_d", "null levraw_d", "null levtab_d",
                                 "null levtab2_d", "null coef_d (the workspace of the row factors)"};
        if (int r = nulls(in, in_null, 14)) return r;
        if (int r = nulls(outs, out_null, nout)) return r;
        if (int r = dtype(a->dtype)) return r;
        if (a->reserved0 != 0) return refuse(LEC_ERR_ARG, "reserved0 must be 0");
        if (int r = dTdt_source(a, dmode)) return r;
        if (int r = levels(a->nl)) return r;
        if (a->nyb < 2) return refuse(LEC_ERR_ARG, "nyb must be >= 2 (a box needs two rows for d/dlat)");
        if (a->nxb < 3) return refuse(LEC_ERR_ARG, few_cols);
        if (a->ny < a->nyb) return refuse(LEC_ERR_ARG, "ny must be >= nyb");
        if (a->nx < a->nxb) return refuse(LEC_ERR_ARG, "nx must be >= nxb");
        if (int r = steps(a->nt, a->t_begin, a->t_count)) return r;
        if (int r = boxes(a, a->t_count, "the box of step")) return r;
        if (int r = align16(a->rows_d, a->lattab2_d, a->coef_d)) return r;
        if ((uintptr_t)a->box_d % 4) return refuse(LEC_ERR_ARG, "box_d must be 4-byte aligned");
        if ((uintptr_t)a->box_h % 4) return refuse(LEC_ERR_ARG, "box_h must be 4-byte aligned");
        return LEC_OK;
    }
    // every box of box_h[n] nyb x nxb and inside the cube: on the HOST copy, before any HIP call.  which: "the box of step" / "box"
    template <typename A>
    int boxes(const A* a, int n, const char* which) const {
        for (int t = 0; t < n; ++t) {
            const int32_t* b = a->box_h + 4 * (size_t)t;
            const long long w = (long long)b[1] - b[0] + 1, h = (long long)b[3] - b[2] + 1;
            char m[256];
            if (w != a->nxb || h != a->nyb) {
                snprintf(m, sizeof(m), "box_h: %s %d is %lld x %lld (rows x columns), the call's nyb x nxb is %d x %d: every box of a "
                         "composite has one shape", which, t, h, w, a->nyb, a->nxb);
                return refuse(LEC_ERR_ARG, m);
            }
            if (b[0] < 0 || b[1] >= a->nx || b[2] < 0 || b[3] >= a->ny) {
                snprintf(m, sizeof(m), "box_h: %s %d {iw, ie, js, jn} = {%d, %d, %d, %d} lies outside the %d x %d cube", which, t, b[0], b[1],
                         b[2], b[3], a->ny, a->nx);
                return refuse(LEC_ERR_ARG, m);
            }
        }
        return LEC_OK;
    }
    // the 8-byte tables tabs[ntab] by their names and the cubes (cube_names: as the message lists them)
    struct Aligned {
        const void* const* tabs; const char* const* tabn; int ntab;
        const void* const* cubes; int ncube; const char* cube_names; int dtype;
    };
    int tables_cubes(const Aligned& p) const {
        char m[128];
        for (int i = 0; i < p.ntab; ++i)
            if ((uintptr_t)p.tabs[i] % 8) {
                snprintf(m, sizeof(m), "%s must be 8-byte aligned", p.tabn[i]);
                return refuse(LEC_ERR_ARG, m);
            }
        const size_t esz = p.dtype == LEC_F32 ? 4 : 8;
        for (int i = 0; i < p.ncube; ++i)
            if ((uintptr_t)p.cubes[i] % esz) {
                snprintf(m, sizeof(m), "cube pointer (%s) not aligned to its element size", p.cube_names);
                return refuse(LEC_ERR_ARG, m);
            }
        return LEC_OK;
    }
    // those alignments, then the launch limits of maps and composites (dims: the fields that set rows and columns).  HIP takes fewer than
    // 2^32 threads per launch: one 64-lane workgroup per (time step, level) and per (time step, row, 64 columns), one thread per element of
    // mapsum_d and of hov_d
    int tables_cubes_limits(const Aligned& p, int t_count, int nl, int nyb, int nxb, const char* dims) const {
        if (int r = tables_cubes(p)) return r;
        char m[128];
        if ((long long)t_count * nl >= (1LL << 26))
            return refuse(LEC_ERR_UNSUPPORTED, "t_count * nl must stay below 2^26 in one call (cut the series into several calls)");
        if ((long long)t_count * nyb * ((nxb + 63) / 64) >= (1LL << 26))
            return refuse(LEC_ERR_UNSUPPORTED, "t_count * rows * ceil(columns / 64) must stay below 2^26 in one call (cut the series into several calls)");
        if ((long long)kNMap * nyb * nxb >= (1LL << 32) - 256) {
            snprintf(m, sizeof(m), "6 * rows * columns (%s) must stay below 2^32 threads", dims);
            return refuse(LEC_ERR_UNSUPPORTED, m);
        }
        if ((long long)t_count * kNMap * nxb >= (1LL << 32) - 256)
            return refuse(LEC_ERR_UNSUPPORTED, "t_count * 6 * columns must stay below 2^32 threads in one call");
        return LEC_OK;
    }
    // those alignments, then the launch limits of the longitude x pressure sections: one 64-lane workgroup per (time step, level, 64
    // columns) -- which bounds the factors' (time step, level) too -- and one thread per element of lonsecsum_d
    int tables_cubes_lonsec_limits(const Aligned& p, int t_count, int nl, int nxb, const char* cols) const {
        if (int r = tables_cubes(p)) return r;
        char m[160];
        if ((long long)t_count * nl * ((nxb + 63) / 64) >= (1LL << 26)) {
            snprintf(m, sizeof(m), "t_count * nl * ceil(columns / 64) (%s) must stay below 2^26 in one call (cut the series into several calls)", cols);
            return refuse(LEC_ERR_UNSUPPORTED, m);
        }
        if ((long long)kNMap * nl * nxb >= (1LL << 32) - 256) {
            snprintf(m, sizeof(m), "6 * nl * columns (%s) must stay below 2^32 threads", cols);
            return refuse(LEC_ERR_UNSUPPORTED, m);
        }
        return LEC_OK;
    }
};

}  // namespace lec
