// lec_sections.hip -- lec_sections: the latitude x pressure sections of the ten terms of the cycle on ONE fixed box (-f --sections;
// include/lec_hip.h).  A translation unit of its own: lec_reduce.hip and the bits of its kernels are not
// touched, and the code object is loaded by calls that ask for sections only.
//
// Stage 2 forms every row's contribution to the per-level sums, acc[V_X] += cw * (...), and only the sum over rows leaves it.  The
// bracketed factor is the section.  Two kernels:
//   lec_section_rows_kernel  one wave per (time step, level[, wavenumber]), rows in trips of 64: the integrands are lec_level_row.inc's
//                            own lines with cw = 1.0 on zeroed sums (0 + 1 x is x), then the level's divisor and sign as lec_reduce.hip
//                            applies them.  sigma is READ from the levraw record of the level stage, never formed again.
//   lec_section_fold_kernel  one thread per (function, row): per time step one scan of the levels with a running "last finite level"
//                            (trapezoid and NaN rule in one pass), then the time sums, step by step in time order.  No atomics: every
//                            output element has one writer, so the numbers do not depend on the launch or on how a series is cut.
#include <stdio.h>

// the levraw record (V_*), wave_sum and the physical constants of the level stage; contraction is off from here on: the row's source
// lines give the products stage 2 forms, none of them fused
#include "lec_level_core.h"

namespace {
using namespace lec;

constexpr int kNSec = LEC_NSECTION;
constexpr int kSpecSlots = 8;      // LEC_S_TT .. LEC_S_WV
constexpr int V_PART_A = V_GE + 1;      // the sums of lec_level_row.inc's part A: V_AZ .. V_GE
// the sections, in the order of F_AZ .. F_GE of lec_reduce.hip
enum { X_AZ = 0, X_AE, X_KZ, X_KE, X_CZ, X_CA, X_CK, X_CE, X_GZ, X_GE };
static_assert(X_GE + 1 == kNSec, "ten sections");

struct SecParams {
    const double* rows;      // [t_count][nl][nyb][LEC_NSTAT]
    const double* spec;      // [t_count][nl][nyb][n_wave][8] or null
    const double* qspec;     // [t_count][nl][nyb][n_wave] or null
    int t_count, nl, nyb, n_wave, n_specfn;
    const int* box;
    const double* lattab2;
    const double* levtab2;
    const double* levraw;    // [t_count][nl][LEC_NLEVRAW]
    double* sec;             // [t_count][nl][10][nyb]
    double* specsec;         // [t_count][nl][n_wave][n_specfn][nyb]
};

// grid ((1 + n_wave) * t_count * nl) -- level fastest, then time step, then wavenumber (0: the totals) --, block 64
__global__ void __launch_bounds__(64) lec_section_rows_kernel(const SecParams p) {
    const int nl = p.nl, nyb_rec = p.nyb, lane = threadIdx.x;
    const int per_wave = p.t_count * nl;
    const int nw = blockIdx.x / per_wave, tk = blockIdx.x - nw * per_wave;      // nw = 0: the totals; nw >= 1: wavenumber nw
    const int tl = tk / nl, k = tk - tl * nl;
    const int km = k > 0 ? k - 1 : k, kp = k < nl - 1 ? k + 1 : k;
    const size_t lstride = (size_t)nyb_rec * LEC_NSTAT;
    const double* rec = p.rows + (size_t)(tl * nl + k) * lstride;
    const double* recm = p.rows + (size_t)(tl * nl + km) * lstride;
    const double* recp = p.rows + (size_t)(tl * nl + kp) * lstride;
    const double* lt = p.lattab2;
    const int nyb = max(1, min(p.box[3] - p.box[2] + 1, nyb_rec));      // (box_d lives where validation cannot see it: never index below row 0)
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
            if (nw > 0) {       // the wavenumber's shares of the lane's own row in slots 6 .. 13 (and 15)
                const size_t srow = ((size_t)(tl * nl + k) * nyb_rec + jb) * p.n_wave + (nw - 1);
                const dbl2_t* sp = reinterpret_cast<const dbl2_t*>(p.spec + srow * kSpecSlots);
                const dbl2_t s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
                r[LEC_S_TT + 0] = s0.x; r[LEC_S_TT + 1] = s0.y; r[LEC_S_TT + 2] = s1.x; r[LEC_S_TT + 3] = s1.y;
                r[LEC_S_TT + 4] = s2.x; r[LEC_S_TT + 5] = s2.y; r[LEC_S_TT + 6] = s3.x; r[LEC_S_TT + 7] = s3.y;
                if (p.qspec) r[LEC_S_QT] = p.qspec[srow];
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
        } else {
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

// grid ceil(n_fn * nyb / 64), block 64: thread (g, j), rows fastest.  A thread's life is a chain of memory round trips (one value per
// (step, level), a few flops each), so the loads are issued kFoldBatch at a time before any of them is used: the ORDER of every sum is
// that of the plain loops (levels ascending within a step, steps ascending), only the loads run ahead.
constexpr int kFoldBatch = 8;
__global__ void __launch_bounds__(64) lec_section_fold_kernel(const FoldParams p) {
    const long long id = (long long)blockIdx.x * 64 + threadIdx.x;
    const long long n_out = (long long)p.n_fn * p.nyb;
    if (id >= n_out) return;
    const int g = (int)(id / p.nyb), nl = p.nl, t_count = p.t_count;
    const size_t lev = (size_t)n_out, step = (size_t)nl * lev;          // doubles between levels / time steps of one (g, j)
    const double* __restrict__ s = p.sec + id;
    const int f = g % p.fn_period;
    const double div = (f == p.f_2g_a || f == p.f_2g_b) ? 2 * kG : (f == p.f_g ? kG : 1.0);
    double csum = p.colsum ? p.colsum[id] : 0.0;
    for (int t = 0; t < t_count; ++t) {
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
    if (p.colsum) p.colsum[id] = csum;
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

int refuse(int code, const char* what) {
    char msg[256];
    snprintf(msg, sizeof(msg), "lec_sections: %s", what);
    return lec_set_error(code, msg);
}

}  // namespace

extern "C" int lec_sections(const lec_sections_args* a) {
    if (!a) return refuse(LEC_ERR_ARG, "null args");
    if (!a->rows_d) return refuse(LEC_ERR_ARG, "null rows_d");
    if (!a->box_d) return refuse(LEC_ERR_ARG, "null box_d");
    if (!a->lattab2_d) return refuse(LEC_ERR_ARG, "null lattab2_d");
    if (!a->levtab2_d) return refuse(LEC_ERR_ARG, "null levtab2_d");
    if (!a->levraw_d) return refuse(LEC_ERR_ARG, "null levraw_d");
    if (!a->sec_d) return refuse(LEC_ERR_ARG, "null sec_d");
    if (!a->col_d) return refuse(LEC_ERR_ARG, "null col_d");
    if (!a->secsum_d) return refuse(LEC_ERR_ARG, "null secsum_d");
    if (a->n_box != 1) return refuse(LEC_ERR_ARG, "n_box must be 1 (sections exist for one fixed box)");
    if (a->t_count < 1) return refuse(LEC_ERR_ARG, "t_count must be >= 1");
    if (a->nl < 2) return refuse(LEC_ERR_ARG, "nl must be >= 2");
    if (a->nyb < 2) return refuse(LEC_ERR_ARG, "nyb must be >= 2");
    if (a->nl > LEC_MAX_LEVELS) return refuse(LEC_ERR_UNSUPPORTED, "nl above LEC_MAX_LEVELS (160)");
    if (a->n_wave < 0) return refuse(LEC_ERR_ARG, "n_wave must be >= 0");
    if (a->n_wave > LEC_MAX_WAVENUMBERS) return refuse(LEC_ERR_UNSUPPORTED, "n_wave above LEC_MAX_WAVENUMBERS");
    if (a->reserved0 != 0) return refuse(LEC_ERR_ARG, "reserved0 must be 0");
    if (a->qspec_d && !a->spec_d) return refuse(LEC_ERR_ARG, "qspec_d without spec_d");
    if (a->n_wave > 0 && !a->spec_d) return refuse(LEC_ERR_ARG, "n_wave > 0 needs spec_d");
    if (a->spec_d && a->n_wave < 1) return refuse(LEC_ERR_ARG, "spec_d needs n_wave >= 1");
    if (a->spec_d && !a->specsec_d) return refuse(LEC_ERR_ARG, "spec_d needs the workspace specsec_d");
    if (a->spec_d && !a->speccolsum_d) return refuse(LEC_ERR_ARG, "spec_d needs speccolsum_d");
    if ((uintptr_t)a->rows_d % 16) return refuse(LEC_ERR_ARG, "rows_d must be 16-byte aligned");
    if ((uintptr_t)a->lattab2_d % 16) return refuse(LEC_ERR_ARG, "lattab2_d must be 16-byte aligned");
    if (a->spec_d && (uintptr_t)a->spec_d % 16) return refuse(LEC_ERR_ARG, "spec_d must be 16-byte aligned");
    const int n_specfn = a->qspec_d ? 6 : 5;
    // HIP takes fewer than 2^32 threads per launch: one 64-lane workgroup per (wavenumber or total, time step, level), and one
    // thread per (function, row) of the fold
    if ((long long)(1 + a->n_wave) * a->t_count * a->nl >= (1LL << 26))
        return refuse(LEC_ERR_UNSUPPORTED, "(1 + n_wave) * t_count * nl must stay below 2^26 in one call (cut the series into several calls)");
    if ((long long)(a->n_wave * n_specfn > kNSec ? a->n_wave * n_specfn : kNSec) * a->nyb >= (1LL << 32) - 64)
        return refuse(LEC_ERR_UNSUPPORTED, "functions * nyb must stay below 2^32 threads in one call");

    hipStream_t st = (hipStream_t)a->stream;
    SecParams p;
    p.rows = a->rows_d; p.spec = a->spec_d; p.qspec = a->qspec_d;
    p.t_count = a->t_count; p.nl = a->nl; p.nyb = a->nyb; p.n_wave = a->spec_d ? a->n_wave : 0; p.n_specfn = n_specfn;
    p.box = a->box_d; p.lattab2 = a->lattab2_d; p.levtab2 = a->levtab2_d; p.levraw = a->levraw_d;
    p.sec = a->sec_d; p.specsec = a->specsec_d;
    const dim3 grid((unsigned)((1 + p.n_wave) * a->t_count * a->nl));
    hipLaunchKernelGGL(lec_section_rows_kernel, grid, dim3(64), 0, st, p);

    FoldParams f;
    f.sec = a->sec_d; f.levtab2 = a->levtab2_d; f.t_count = a->t_count; f.nl = a->nl; f.n_fn = kNSec; f.nyb = a->nyb;
    f.fn_period = kNSec; f.f_2g_a = X_KZ; f.f_2g_b = X_KE; f.f_g = X_CK;
    f.col = a->col_d; f.colsum = nullptr; f.secsum = a->secsum_d;
    hipLaunchKernelGGL(lec_section_fold_kernel, dim3((unsigned)(((long long)kNSec * a->nyb + 63) / 64)), dim3(64), 0, st, f);
    if (p.n_wave > 0) {
        FoldParams s = f;
        s.sec = a->specsec_d; s.n_fn = p.n_wave * n_specfn; s.fn_period = n_specfn;
        s.f_2g_a = s.f_2g_b = 1; s.f_g = 4;     // Ae Ke Ca Ce Ck (Ge)
        s.col = nullptr; s.colsum = a->speccolsum_d; s.secsum = nullptr;
        hipLaunchKernelGGL(lec_section_fold_kernel, dim3((unsigned)(((long long)s.n_fn * a->nyb + 63) / 64)), dim3(64), 0, st, s);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}
