// lec_section_core.h -- what lec_sections (lec_sections.hip) and lec_composite_sections (lec_composite_sections.hip) share: the latitude x
// pressure sections X_f(t, k, j) of the ten terms of the cycle from the row records of stage 1, their column values and their time sums
// (DESIGN.md sections 4.2c, 4.2f).  Written once, here, as lec_mapcol.h does for maps and composites.  The kernels have internal linkage
// and the rows kernel is a template over the including file's launch struct, so each of the two files instantiates kernels of its own and
// remains a code object of its own.
//   lec_section_rows_kernel<P>  one wave per (time step, level[, wavenumber]), rows in trips of 64: the integrands are lec_level_row.inc's
//                            own lines with cw = 1.0 on zeroed sums (0 + 1 x is x), then the level's divisor and sign as lec_reduce.hip
//                            applies them.  sigma is READ from the levraw record of the level stage, never formed again.  The march over
//                            the rows IS the kernel's body (lec_mapcol.h records why); the file's P resolves "the box of step t" and "the
//                            lattab2 of step t" through two small members, both wave-uniform: scalar loads and address arithmetic.
//   lec_section_fold_kernel  one thread per (function, row): per time step one scan of the levels with a running "last finite level"
//                            (trapezoid and NaN rule in one pass), then the time sums, step by step in time order.  No atomics: every
//                            output element has one writer, so the numbers do not depend on the launch or on how a series is cut.
// A launch struct P has:
//   rows, levtab2, levraw, sec, t_count, nl, nyb   by name (nyb: rows of the record buffer)
//   kSpectral                                      true: wavenumber nw >= 1 of the grid takes its shares from spec / qspec (n_wave, n_specfn)
//                                                  and writes specsec; false: the grid is (t_count * nl), the totals only
//   box_of(box, tl), lattab2_of(lattab2, tl, nyb)  the step's {iw, ie, js, jn} and its [nyb][8] table, given the call's tables: STATIC members
//                                                  that take the pointer by value (called on `p` itself they cost lec_sections' rows kernel two
//                                                  VGPRs and another schedule; this way its instructions are those of its former own copy)
// No LDS, no scratch.
#pragma once
#include <stdio.h>

// the levraw record (V_*), wave_sum and the physical constants of the level stage; contraction is off from here on: the row's source
// lines give the products stage 2 forms, none of them fused
#include "lec_level_core.h"

namespace lec {

constexpr int kNSec = LEC_NSECTION;
constexpr int kSpecSlots = 8;      // LEC_S_TT .. LEC_S_WV
constexpr int V_PART_A = V_GE + 1;      // the sums of lec_level_row.inc's part A: V_AZ .. V_GE
// the sections, in the order of F_AZ .. F_GE of lec_reduce.hip
enum { X_AZ = 0, X_AE, X_KZ, X_KE, X_CZ, X_CA, X_CK, X_CE, X_GZ, X_GE };
static_assert(X_GE + 1 == kNSec, "ten sections");

struct FoldParams {
    const double* sec;       // [t_count][nl][n_fn][nyb]
    const double* levtab2;
    int t_count, nl, n_fn, nyb;
    int fn_period;           // function g is term g % fn_period of its group
    int f_2g_a, f_2g_b, f_g; // the vertical kernel's divisor of a term's integral: 2 g for these two terms, g for that one, else 1
    double* col;             // [t_count][n_fn][nyb] or null
    double* colsum;          // [n_fn][nyb], += , or null
    double* secsum;          // [nl][n_fn][nyb], +=, or null
};

// the kernels: internal to the file that includes this header, so each file's code object has its own
namespace {

// grid ((1 + n_wave) * t_count * nl) -- level fastest, then time step, then wavenumber (0: the totals) --, block 64
template <class P>
__global__ void __launch_bounds__(64) lec_section_rows_kernel(const P p) {
    const int nl = p.nl, nyb_rec = p.nyb, lane = threadIdx.x;
    const int per_wave = p.t_count * nl;
    const int nw = P::kSpectral ? blockIdx.x / per_wave : 0, tk = blockIdx.x - nw * per_wave;      // nw = 0: the totals; nw >= 1: wavenumber nw
    const int tl = tk / nl, k = tk - tl * nl;
    const int km = k > 0 ? k - 1 : k, kp = k < nl - 1 ? k + 1 : k;
    const size_t lstride = (size_t)nyb_rec * LEC_NSTAT;
    const double* rec = p.rows + (size_t)(tl * nl + k) * lstride;
    const double* recm = p.rows + (size_t)(tl * nl + km) * lstride;
    const double* recp = p.rows + (size_t)(tl * nl + kp) * lstride;
    const double* lt = P::lattab2_of(p.lattab2, tl, nyb_rec);
    const int* box = P::box_of(p.box, tl);
    const int nyb = max(1, min(box[3] - box[2] + 1, nyb_rec));      // (box_d lives where validation cannot see it: never index below row 0)
    const double ps = 1.0;      // the geopotential enters the boundary terms only, which have no section

    // the area means {[T]} (own level, one up, one down), {[w]}, {[Q]}: the products and the order of the level stage -- running sums of
    // a lane over its 64-row trips, then the xor butterfly (lec_area_means_kernel; one trip: lec_level_small_kernel's own sums)
    static_assert(LEC_S_MT == 0 && LEC_S_MU == 1 && LEC_S_MW == 3 && LEC_S_MQ == 5, "the zonal means are the first three 16-byte pairs");
    double aT = 0.0, aW = 0.0, aQ = 0.0, aTm = 0.0, aTp = 0.0;
    for (int j0 = 0; j0 < nyb; j0 += 64) {
        const int jb = j0 + lane, jc = min(jb, nyb - 1);
        const dbl2_t* r2 = reinterpret_cast<const dbl2_t*>(rec + (size_t)jc * LEC_NSTAT);
        const dbl2_t v0 = r2[0], v1 = r2[1], v2 = r2[2];
        const double tm = recm[(size_t)jc * LEC_NSTAT], tp = recp[(size_t)jc * LEC_NSTAT];
        const double cw = lt[8 * jc + 0];
        if (jb < nyb) { aT += cw * v0.x; aW += cw * v1.y; aQ += cw * v2.y; aTm += cw * tm; aTp += cw * tp; }
    }
    aT = wave_sum(aT); aW = wave_sum(aW); aQ = wave_sum(aQ);
    aTm = (km == k) ? aT : wave_sum(aTm);
    aTp = (kp == k) ? aT : wave_sum(aTp);
    const double aP = 0.0;

    const double pk = p.levtab2[4 * k + 0], pa = p.levtab2[4 * k + 1], pb = p.levtab2[4 * k + 2], pc = p.levtab2[4 * k + 3];
    const double sig = p.levraw[(size_t)(tl * nl + k) * LEC_NLEVRAW + LEC_LEVRAW_SIGMA];      // the clamped sigma the totals used
    const double c1k = kRd / (pk * kG);                                                     // Rd / (p g), as lec_reduce.hip

    for (int j0 = 0; j0 < nyb_rec; j0 += 64) {
        const int jb = j0 + lane;
        if (jb >= nyb_rec) break;
        double X[kNSec];
        if (jb < nyb) {
            const int jm = jb > 0 ? jb - 1 : jb, jp = jb < nyb - 1 ? jb + 1 : jb;
            constexpr int kUsed = LEC_S_SPARE / 2;
            const dbl2_t* rr = reinterpret_cast<const dbl2_t*>(rec + (size_t)jb * LEC_NSTAT);
            double r[LEC_S_SPARE];
#pragma unroll
            for (int i = 0; i < kUsed; ++i) { const dbl2_t v = rr[i]; r[2 * i] = v.x; r[2 * i + 1] = v.y; }
            if constexpr (P::kSpectral) {
                if (nw > 0) {       // the wavenumber's shares of the lane's own row in slots 6 .. 13 (and 15)
                    const size_t srow = ((size_t)(tl * nl + k) * nyb_rec + jb) * p.n_wave + (nw - 1);
                    const dbl2_t* sp = reinterpret_cast<const dbl2_t*>(p.spec + srow * kSpecSlots);
                    const dbl2_t s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
                    r[LEC_S_TT + 0] = s0.x; r[LEC_S_TT + 1] = s0.y; r[LEC_S_TT + 2] = s1.x; r[LEC_S_TT + 3] = s1.y;
                    r[LEC_S_TT + 4] = s2.x; r[LEC_S_TT + 5] = s2.y; r[LEC_S_TT + 6] = s3.x; r[LEC_S_TT + 7] = s3.y;
                    if (p.qspec) r[LEC_S_QT] = p.qspec[srow];
                }
            }
            const dbl2_t* rm2 = reinterpret_cast<const dbl2_t*>(rec + (size_t)jm * LEC_NSTAT);
            const dbl2_t* rp2 = reinterpret_cast<const dbl2_t*>(rec + (size_t)jp * LEC_NSTAT);
            const dbl2_t m0 = rm2[0], m1 = rm2[1], q0 = rp2[0], q1 = rp2[1];
            const double rjm[3] = {m0.x, m0.y, m1.x}, rjp[3] = {q0.x, q0.y, q1.x};      // [T] [u] [v] of the rows j - 1 / j + 1
            const dbl2_t km2 = *reinterpret_cast<const dbl2_t*>(recm + (size_t)jb * LEC_NSTAT);
            const dbl2_t kp2 = *reinterpret_cast<const dbl2_t*>(recp + (size_t)jb * LEC_NSTAT);
            const dbl2_t* ll = reinterpret_cast<const dbl2_t*>(lt + (size_t)jb * 8);
            const dbl2_t L1 = ll[1], L2 = ll[2], L3 = ll[3];
            const double cw = 1.0, c = L1.x, tn = L1.y, gra = L2.x, grb = L2.y, grc = L3.x;
            const double cm = lt[8 * jm + 2], cp = lt[8 * jp + 2];
            double acc[V_PART_A];
#pragma unroll
            for (int i = 0; i < V_PART_A; ++i) acc[i] = 0.0;
#define LEC_ROW_COMMON
#define LEC_ROW_PART_A
#include "lec_level_row.inc"
#undef LEC_ROW_COMMON
#undef LEC_ROW_PART_A
            (void)Ps; (void)sWP; (void)aP;
            // the level's divisors (tot / div of the level kernels) and the signs and sums of build_level_functions
            X[X_AZ] = acc[V_AZ] / (2 * sig);
            X[X_AE] = acc[V_AE] / (2 * sig);
            X[X_KZ] = acc[V_KZ];
            X[X_KE] = acc[V_KE];
            X[X_CZ] = -(c1k * acc[V_CZ2]);
            X[X_CA] = -(acc[V_CA1] / (2 * kRe * sig) + acc[V_CA2] / sig);
            X[X_CK] = acc[V_CK1] + acc[V_CK2] + acc[V_CK3] + acc[V_CK4] + acc[V_CK5];
            X[X_CE] = -(c1k * acc[V_CE2]);
            X[X_GZ] = acc[V_GZ] / (kCp * sig);
            X[X_GE] = acc[V_GE] / (kCp * sig);
        } else {
#pragma unroll
            for (int f = 0; f < kNSec; ++f) X[f] = nan("");      // rows of the record buffer below a lower box: no section
        }
        if (nw == 0) {
            double* o = p.sec + ((size_t)(tl * nl + k) * kNSec) * nyb_rec + jb;
#pragma unroll
            for (int f = 0; f < kNSec; ++f) o[(size_t)f * nyb_rec] = X[f];
        } else if constexpr (P::kSpectral) {
            double* o = p.specsec + (((size_t)(tl * nl + k) * p.n_wave + (nw - 1)) * p.n_specfn) * nyb_rec + jb;
            o[0] = X[X_AE];
            o[(size_t)1 * nyb_rec] = X[X_KE];
            o[(size_t)2 * nyb_rec] = X[X_CA];
            o[(size_t)3 * nyb_rec] = X[X_CE];
            o[(size_t)4 * nyb_rec] = X[X_CK];
            if (p.n_specfn > 5) o[(size_t)5 * nyb_rec] = X[X_GE];
        }
    }
}

// grid.x ceil(n_fn * nyb / 64), block 64: thread (g, j), rows fastest.  A thread's life is a chain of memory round trips (one value per
// (step, level), a few flops each), so the loads are issued kFoldBatch at a time before any of them is used: the ORDER of every sum is
// that of the plain loops (levels ascending within a step, steps ascending), only the loads run ahead.
// SHAPE is how the work of one (g, j) is laid on the launch; rule, order and bits are the same in all three:
//   kFoldWhole  one thread does every step's scan and then the time sums (lec_sections: a few steps of many rows)
//   kFoldScan   grid.y walks the STEPS: a thread does the scan of steps blockIdx.y, blockIdx.y + gridDim.y, ... and nothing else
//   kFoldSum    grid.y is the LEVEL: a thread adds that level's values to the time sum, steps ascending, kFoldBatch loads ahead
// (lec_composite_sections: hundreds of steps of a few dozen rows -- one thread per (g, j) would be ten waves walking the whole series;
// a scan needs no other step, and a level's time sum no other level, so they go side by side.  colsum is kFoldWhole's.)
constexpr int kFoldBatch = 8;
enum { kFoldWhole = 0, kFoldScan = 1, kFoldSum = 2 };
template <int SHAPE>
__global__ void __launch_bounds__(64) lec_section_fold_kernel(const FoldParams p) {
    const long long id = (long long)blockIdx.x * 64 + threadIdx.x;
    const long long n_out = (long long)p.n_fn * p.nyb;
    if (id >= n_out) return;
    const int g = (int)(id / p.nyb), nl = p.nl, t_count = p.t_count;
    const size_t lev = (size_t)n_out, step = (size_t)nl * lev;          // doubles between levels / time steps of one (g, j)
    const double* __restrict__ s = p.sec + id;
    if constexpr (SHAPE != kFoldSum) {
        const int f = g % p.fn_period;
        const double div = (f == p.f_2g_a || f == p.f_2g_b) ? 2 * kG : (f == p.f_g ? kG : 1.0);
        double csum = p.colsum ? p.colsum[id] : 0.0;
        const int t_first = SHAPE == kFoldScan ? (int)blockIdx.y : 0, t_stride = SHAPE == kFoldScan ? (int)gridDim.y : 1;
        for (int t = t_first; t < t_count; t += t_stride) {
            // the trapezoid over the finite levels: interior gaps are bridged linearly in p (a trapezoid between the two finite
            // neighbours is that), NaN levels at either end are left out, no finite level at all is NaN
            const double* __restrict__ st = s + (size_t)t * step;
            int last = -1;
            double xl = 0.0, yl = 0.0, r = 0.0;
            for (int k0 = 0; k0 < nl; k0 += kFoldBatch) {
                double yb[kFoldBatch];
#pragma unroll
                for (int i = 0; i < kFoldBatch; ++i) yb[i] = st[(size_t)min(k0 + i, nl - 1) * lev];
#pragma unroll
                for (int i = 0; i < kFoldBatch; ++i) {
                    const int k = k0 + i;
                    const double y = yb[i];
                    if (k < nl && !isnan(y)) {
                        const double x = p.levtab2[4 * k];
                        if (last >= 0) r += (x - xl) * 0.5 * (y + yl);
                        last = k; xl = x; yl = y;
                    }
                }
            }
            const double cv = last < 0 ? nan("") : r / div;                 // x / 1.0 is x
            if (p.col) p.col[(size_t)t * lev + id] = cv;
            csum += cv;
        }
        if constexpr (SHAPE == kFoldWhole)
            if (p.colsum) p.colsum[id] = csum;
    }
    if constexpr (SHAPE == kFoldWhole) {
        if (p.secsum) {
            double* __restrict__ sum = p.secsum + id;
            for (int k0 = 0; k0 < nl; k0 += kFoldBatch) {
                double a[kFoldBatch];
#pragma unroll
                for (int i = 0; i < kFoldBatch; ++i) a[i] = sum[(size_t)min(k0 + i, nl - 1) * lev];
                for (int t = 0; t < t_count; ++t) {
                    double v[kFoldBatch];
#pragma unroll
                    for (int i = 0; i < kFoldBatch; ++i) v[i] = s[(size_t)t * step + (size_t)min(k0 + i, nl - 1) * lev];
#pragma unroll
                    for (int i = 0; i < kFoldBatch; ++i) a[i] += v[i];
                }
#pragma unroll
                for (int i = 0; i < kFoldBatch; ++i)
                    if (k0 + i < nl) sum[(size_t)(k0 + i) * lev] = a[i];
            }
        }
    }
    if constexpr (SHAPE == kFoldSum) {
        // the same sum of the same level: a += X(t), t ascending, on what the sum held
        const size_t at = (size_t)blockIdx.y * lev;
        double* __restrict__ sum = p.secsum + id + at;
        double a = *sum;
        for (int t0 = 0; t0 < t_count; t0 += kFoldBatch) {
            double v[kFoldBatch];
#pragma unroll
            for (int i = 0; i < kFoldBatch; ++i) v[i] = s[(size_t)min(t0 + i, t_count - 1) * step + at];
#pragma unroll
            for (int i = 0; i < kFoldBatch; ++i)
                if (t0 + i < t_count) a += v[i];
        }
        *sum = a;
    }
}

}  // namespace

// the fold of the ten totals: Kz and Ke over 2 g, Ck over g
inline FoldParams section_fold_totals(const double* sec, const double* levtab2, int t_count, int nl, int nyb, double* col, double* secsum) {
    FoldParams f;
    f.sec = sec; f.levtab2 = levtab2; f.t_count = t_count; f.nl = nl; f.n_fn = kNSec; f.nyb = nyb;
    f.fn_period = kNSec; f.f_2g_a = X_KZ; f.f_2g_b = X_KE; f.f_g = X_CK;
    f.col = col; f.colsum = nullptr; f.secsum = secsum;
    return f;
}

}  // namespace lec
