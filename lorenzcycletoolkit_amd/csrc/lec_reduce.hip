// lec_reduce.hip -- stage 2 of the MI355X Lorenz-Energy-Cycle engine (gfx950, wave64).
//
// Consumes the per-(time, level, lat) row records of lec_rowstats and produces, per time step, the 16
// integrated terms and the 21 per-level tables.  Small kernels (O(level x lat) work, <1 % of the
// stage-1 bytes):
//   the level stage         lec_level_core.h's kernels on plain records (LevelRecords, below): the area means, sigma and every
//                           per-level integrand and boundary piece of one (time step, level), into the levraw record
//   lec_dropmask_kernel     the levels still NaN after the interpolation at any time step
//   lec_vertical_kernel     _handle_nans + integrate(level) + boundary assembly               (energy_contents.py:190-208)
// Formulas: SURVEY.md appendix A / F (factored through row statistics; exact in exact arithmetic).
#include "lec_level_core.h"      // contraction is off from here on: the vertical kernels' products are not fused either

namespace {
using namespace lec;

constexpr int kMaxNl = 160;

struct RedParams {
    const double* rows;
    int t_count, nl, n_box, nyb_max;
    const int* box;
    const double* boxtab2;
    const double* lattab2;
    const double* levtab2;
    double phi_scale;
    int drop_any_time;      // fixed framework: a level still NaN at ANY time step is dropped for every time step
    int* dropmask;          // [F_COUNT][nl], filled by lec_dropmask_kernel
    double* am;
    double* levraw;
    double* scalars;
    double* levels;
    int* nanflag;
    long long sstride, lstride;     // doubles between consecutive time steps of `scalars` / `levels`
};

// {[T]} of another level exactly as that level's own wave forms it: the products of lec_area_means_kernel summed in the order of
// wave_sum's xor butterfly -- lane 0 ends with ((((l0 + l32) + (l16 + l48)) + ...): pairs 32 apart first, then 16, 8, 4, 2, 1 -- written
// as five nested two-trip loops (rolled: this is the rare NaN-repair path and must not cost the kernel its registers)
__device__ double area_mean_T_small(const RedParams& p, const double* lt, int nyb, int tl, int level) {
    const double* rec = p.rows + (size_t)(tl * p.nl + level) * p.nyb_max * LEC_NSTAT;
    auto leaf = [&](int l) -> double { return l < nyb ? lt[8 * l] * rec[(size_t)l * LEC_NSTAT + LEC_S_MT] : 0.0; };
    double a1 = 0.0, a2 = 0.0, a4 = 0.0, a8 = 0.0, a16 = 0.0;
#pragma unroll 1
    for (int b1 = 0; b1 < 2; b1 += 1) {
#pragma unroll 1
        for (int b2 = 0; b2 < 4; b2 += 2) {
#pragma unroll 1
            for (int b4 = 0; b4 < 8; b4 += 4) {
#pragma unroll 1
                for (int b8 = 0; b8 < 16; b8 += 8) {
#pragma unroll 1
                    for (int b16 = 0; b16 < 32; b16 += 16) {
                        const int i = b1 | b2 | b4 | b8 | b16;
                        const double s32 = leaf(i) + leaf(i ^ 32);
                        a16 = b16 ? a16 + s32 : s32;
                    }
                    a8 = b8 ? a8 + a16 : a16;
                }
                a4 = b4 ? a4 + a8 : a8;
            }
            a2 = b2 ? a2 + a4 : a4;
        }
        a1 = b1 ? a1 + a2 : a2;
    }
    return a1;
}

// lec_level_core.h's record source for the row records as lec_rowstats wrote them: one workgroup per (time step, level), a box per
// step or one for all, nothing substituted.  The small kernel forms its own area means (am_d is not used for boxes of at most 64 rows),
// so its repair re-forms those of the other levels.
struct LevelRecords {
    using Params = RedParams;
    static constexpr bool kMeansInSmallKernel = true;
    int tl, k;
    __device__ __forceinline__ LevelRecords(const RedParams& p, unsigned block) : tl(block / p.nl), k(block - tl * p.nl) {}
    static __device__ __forceinline__ int box_index(const RedParams& p, int tl) { return (p.n_box == 1) ? 0 : tl; }
    static __device__ __forceinline__ int band_rows(const RedParams&, int h) { return h; }
    __device__ __forceinline__ double* out(const RedParams& p) const { return p.levraw + (size_t)(tl * p.nl + k) * LEC_NLEVRAW; }
    struct Shares {};
    __device__ __forceinline__ Shares load_shares(const RedParams&, int) const { return {}; }
    __device__ __forceinline__ void put(const RedParams&, const Shares&, double*) const {}
    __device__ __forceinline__ double wT(const RedParams&, const double* r, size_t) const { return r[LEC_S_WT]; }
    __device__ double small_mean_T(const RedParams& p, const double*, const double* lt, int nyb, int level) const {
        return area_mean_T_small(p, lt, nyb, tl, level);
    }
};

// functions of level handled by lec_vertical_kernel (one lane each)
enum {
    F_AZ = 0, F_AE, F_KZ, F_KE, F_CZ, F_CA, F_CK, F_CE, F_GZ, F_GE,
    F_B1 = 10, F_B2 = 16, F_B3 = 22, F_COUNT = 28
};

// Builds the F_COUNT functions of level of time step `tl` into fn[f][0..nl) and applies the interpolation half of
// _handle_nans (energy_contents.py:190-208): linear in p across interior gaps, no extrapolation.
// BAz's bottom-top term (F_B3) is the exception: the reference interpolates it per latitude before the area mean
// (lec_level_terms_kernel has done that) and only DROPS the levels that are still NaN (boundary_terms.py:169-176).
// Phase 1: one LEVEL per lane (its levraw record read once, every function evaluated without divergence);
// phase 2: one FUNCTION per lane scans its levels in LDS.  Returns, on lane f < F_COUNT, the number of NaN levels
// of function f found before the repair (0 on the other lanes).
__device__ int build_level_functions(const RedParams& p, int tl, double (*fn)[kMaxNl], int lane) {
    const int nl = p.nl;
    const double* raw = p.levraw + (size_t)tl * nl * LEC_NLEVRAW;
    const double* lv = p.levtab2;
    for (int k = lane; k < nl; k += 64) {
        const double* o = raw + (size_t)k * LEC_NLEVRAW;
        const double c1k = kRd / (lv[4 * k] * kG);   // Rd / (p g), conversion_terms.py:146,172
        fn[F_AZ][k] = o[V_AZ];
        fn[F_AE][k] = o[V_AE];
        fn[F_KZ][k] = o[V_KZ];
        fn[F_KE][k] = o[V_KE];
        fn[F_CZ][k] = -(c1k * o[V_CZ2]);
        fn[F_CA][k] = -(o[V_CA1] + o[V_CA2]);
        fn[F_CK][k] = o[V_CK1] + o[V_CK2] + o[V_CK3] + o[V_CK4] + o[V_CK5];
        fn[F_CE][k] = -(c1k * o[V_CE2]);
        fn[F_GZ][k] = o[V_GZ];
        fn[F_GE][k] = o[V_GE];
#pragma unroll
        for (int i = 0; i < 18; ++i) fn[F_B1 + i][k] = o[V_B1 + i];       // V_B1.. V_B3 are contiguous like F_B1..F_B3
    }
    __syncthreads();
    int nnan = 0;
    if (lane < F_COUNT) {
        double* row = fn[lane];
        for (int k = 0; k < nl; ++k) nnan += isnan(row[k]) ? 1 : 0;
        if (nnan && lane != F_B3) {
            int last_ok = -1;
            for (int k = 0; k < nl; ++k) {
                if (!isnan(row[k])) { last_ok = k; continue; }
                int nxt = k + 1;
                while (nxt < nl && isnan(row[nxt])) ++nxt;
                if (last_ok >= 0 && nxt < nl) {
                    const double xl = lv[4 * last_ok], xr = lv[4 * nxt], yl = row[last_ok], yr = row[nxt];
                    const double slope = (yr - yl) / (xr - xl);
                    for (int q = k; q < nxt; ++q) row[q] = slope * (lv[4 * q] - xl) + yl;
                }
                k = nxt - 1;
            }
        }
    }
    return nnan;
}

// grid (t_count), block 64: marks the levels that are still NaN after the interpolation at this time step.
// xarray's dropna(dim=level) on a [time, level] array drops such a level for EVERY time step.
__global__ void __launch_bounds__(64) lec_dropmask_kernel(const RedParams p) {
    __shared__ double fn[F_COUNT][kMaxNl];
    const int tl = blockIdx.x, lane = threadIdx.x;
    if (build_level_functions(p, tl, fn, lane)) {
        for (int k = 0; k < p.nl; ++k)
            if (isnan(fn[lane][k])) atomicOr(&p.dropmask[lane * p.nl + k], 1);
    }
}

// grid (t_count), block 64
__global__ void __launch_bounds__(64) lec_vertical_kernel(const RedParams p) {
    __shared__ double fn[F_COUNT][kMaxNl];
    __shared__ double res[F_COUNT];
    __shared__ int nans[64];
    const int tl = blockIdx.x, lane = threadIdx.x, nl = p.nl;
    const int bi = (p.n_box == 1) ? 0 : tl;
    const double* raw = p.levraw + (size_t)tl * nl * LEC_NLEVRAW;
    const double* lv = p.levtab2;

    int nnan = build_level_functions(p, tl, fn, lane);
    if (lane < F_COUNT) {
        const int f = lane;
        // the dropping half of _handle_nans: levels that are still NaN (here, or at any time step in the fixed framework)
        int k0 = 0, k1 = nl - 1;
        if (p.drop_any_time) {
            const int* dm = p.dropmask + f * nl;
            bool any = false;
            for (int k = 0; k < nl; ++k) if (dm[k]) { fn[f][k] = nan(""); any = true; }
            if (any && !nnan) nnan = 1;
        }
        if (nnan) {
            while (k0 < nl && isnan(fn[f][k0])) ++k0;
            while (k1 >= 0 && isnan(fn[f][k1])) --k1;
        }
        double r;
        if (k0 > k1) {
            // no level left: the reference integrates an EMPTY array after dropna -- xarray's integrate gives 0.0 --, while its
            // bottom-top terms would stop at .isel(level=-1) of nothing (IndexError); here those are NaN
            r = f >= F_B3 ? nan("") : 0.0;
        } else if (f >= F_B3) {
            r = fn[f][k1] - fn[f][k0];                       // .isel(level=-1) - .isel(level=0)
        } else {
            r = 0.0;
            for (int k = k0; k < k1; ++k) r += (lv[4 * (k + 1)] - lv[4 * k]) * 0.5 * (fn[f][k + 1] + fn[f][k]);
        }
        res[f] = r;
    }
    nans[lane] = nnan;
    __syncthreads();

    if (lane == 0) {
        const double c1 = p.boxtab2[4 * bi + 0], c2 = p.boxtab2[4 * bi + 1];
        double* s = p.scalars + (size_t)tl * (size_t)p.sstride;
        s[0] = res[F_AZ];
        s[1] = res[F_AE];
        s[2] = res[F_KZ] / (2 * kG);
        s[3] = res[F_KE] / (2 * kG);
        s[4] = res[F_CZ];
        s[5] = res[F_CA];
        s[6] = res[F_CK] / kG;
        s[7] = res[F_CE];
        for (int i = 0; i < 6; ++i) s[8 + i] = res[F_B1 + i] * c1 + res[F_B2 + i] * c2 - res[F_B3 + i];
        s[14] = res[F_GZ];
        s[15] = res[F_GE];
        int tot = 0;
        for (int i = 0; i < F_COUNT; ++i) tot += nans[i];
        p.nanflag[tl] = tot;
    }

    // per-level tables, order of lec_fixed_framework.py:172-194
    double* L = p.levels + (size_t)tl * (size_t)p.lstride;
    for (int k = lane; k < nl; k += 64) {
        const double* o = raw + (size_t)k * LEC_NLEVRAW;
        const double c1k = kRd / (lv[4 * k] * kG);
        L[0 * nl + k] = fn[F_AZ][k];
        L[1 * nl + k] = fn[F_AE][k];
        L[2 * nl + k] = fn[F_KZ][k];
        L[3 * nl + k] = fn[F_KE][k];
        L[4 * nl + k] = fn[F_GE][k];
        L[5 * nl + k] = fn[F_GZ][k];
        L[6 * nl + k] = fn[F_CZ][k];
        L[7 * nl + k] = c1k;
        L[8 * nl + k] = o[V_CZ2];
        L[9 * nl + k] = fn[F_CA][k];
        L[10 * nl + k] = o[V_CA1];
        L[11 * nl + k] = o[V_CA2];
        L[12 * nl + k] = fn[F_CE][k];
        L[13 * nl + k] = c1k;
        L[14 * nl + k] = o[V_CE2];
        L[15 * nl + k] = fn[F_CK][k];
        L[16 * nl + k] = o[V_CK1];
        L[17 * nl + k] = o[V_CK2];
        L[18 * nl + k] = o[V_CK3];
        L[19 * nl + k] = o[V_CK4];
        L[20 * nl + k] = o[V_CK5];
    }
}

}  // namespace

static int reduce_impl(const lec_reduce_args* a, bool mask_only, const char* who) {
    if (!a) return lec_set_error(LEC_ERR_ARG, "lec_reduce: null args");
    if (a->stage < LEC_STAGE_BOTH || a->stage > LEC_STAGE_VERTICAL) return lec_set_error(LEC_ERR_ARG, "lec_reduce / lec_dropmask: stage must be 0 (both), 1 (levels) or 2 (vertical)");
    const bool levels = a->stage != LEC_STAGE_VERTICAL, vertical = a->stage != LEC_STAGE_LEVELS;
    if (mask_only && a->stage == LEC_STAGE_LEVELS) return lec_set_error(LEC_ERR_ARG, "lec_dropmask: stage LEC_STAGE_LEVELS forms no mask (use lec_reduce)");
    if (!a->boxtab2_d || !a->levtab2_d || !a->levraw_d)
        return lec_set_error(LEC_ERR_ARG, "lec_reduce / lec_dropmask: null pointer argument");
    if (levels && (!a->rows_d || !a->box_d || !a->lattab2_d || !a->am_d)) return lec_set_error(LEC_ERR_ARG, "lec_reduce / lec_dropmask: null pointer argument");
    if (vertical && !mask_only && (!a->scalars_d || !a->levels_d || !a->nanflag_d)) return lec_set_error(LEC_ERR_ARG, "lec_reduce: null output pointer");
    if (a->t_count < 1 || a->nl < 2 || a->nyb_max < 2) return lec_set_error(LEC_ERR_ARG, "lec_reduce: needs t_count>=1, nl>=2, nyb_max>=2");
    if (a->nl > kMaxNl) return lec_set_error(LEC_ERR_UNSUPPORTED, "lec_reduce: more than 160 levels");
    // HIP refuses a launch whose grid x block reaches 2^32 threads: (nl * t_count) workgroups of 64 threads and, for the vertical
    // half, t_count workgroups of 64
    if ((long long)a->t_count * a->nl * 64 > 0xffffffffLL)
        return lec_set_error(LEC_ERR_UNSUPPORTED, "lec_reduce: nl * t_count must stay below 2^26 in one call (cut the series into several calls)");
    if (a->n_box != 1 && a->n_box != a->t_count) return lec_set_error(LEC_ERR_ARG, "lec_reduce: n_box must be 1 or t_count");
    if (a->drop_any_time < 0 || a->drop_any_time > 2) return lec_set_error(LEC_ERR_ARG, "lec_reduce: drop_any_time must be 0, 1 or 2");
    if (levels && ((reinterpret_cast<uintptr_t>(a->rows_d) | reinterpret_cast<uintptr_t>(a->lattab2_d)) & 15))
        return lec_set_error(LEC_ERR_ARG, "lec_reduce / lec_dropmask: rows_d and lattab2_d must be 16-byte aligned");
    if (a->scalars_stride < 0 || a->levels_stride < 0 || (a->scalars_stride && a->scalars_stride < LEC_NSCALAR) ||
        (a->levels_stride && a->levels_stride < (long long)LEC_NLEVTAB * a->nl))
        return lec_set_error(LEC_ERR_ARG, "lec_reduce: scalars_stride / levels_stride must be 0 (dense) or at least one record long");
    if (vertical && (a->drop_any_time || mask_only) && !a->dropmask_d) return lec_set_error(LEC_ERR_ARG, "lec_reduce / lec_dropmask: drop_any_time needs dropmask_d");
    (void)who;
    RedParams p;
    p.rows = a->rows_d; p.t_count = a->t_count; p.nl = a->nl; p.n_box = a->n_box; p.nyb_max = a->nyb_max;
    p.box = a->box_d; p.boxtab2 = a->boxtab2_d; p.lattab2 = a->lattab2_d; p.levtab2 = a->levtab2_d;
    p.phi_scale = a->phi_scale; p.am = a->am_d; p.levraw = a->levraw_d; p.scalars = a->scalars_d;
    p.levels = a->levels_d; p.nanflag = a->nanflag_d;
    p.sstride = a->scalars_stride ? a->scalars_stride : LEC_NSCALAR;
    p.lstride = a->levels_stride ? a->levels_stride : (long long)LEC_NLEVTAB * a->nl;
    p.drop_any_time = (a->drop_any_time || mask_only) ? 1 : 0; p.dropmask = a->dropmask_d;
    hipStream_t st = (hipStream_t)a->stream;
    if (levels) {
        const dim3 grid2((unsigned)a->nl * (unsigned)a->t_count);      // one workgroup per (time step, level), level fastest
        if (a->nyb_max <= kSmallRows) {
            hipLaunchKernelGGL(lec_level_small_kernel<LevelRecords>, grid2, dim3(64), 0, st, p);       // forms its own area means; am_d is not used
        } else {
            hipLaunchKernelGGL(lec_area_means_kernel<LevelRecords>, grid2, dim3(64), 0, st, p);
            hipLaunchKernelGGL(lec_level_terms_kernel<LevelRecords>, grid2, dim3(64), 0, st, p);
        }
    }
    if (vertical) {
        if (mask_only || a->drop_any_time == 1) {
            if (hipMemsetAsync(p.dropmask, 0, sizeof(int) * F_COUNT * a->nl, st) != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, "lec_reduce: hipMemsetAsync failed");
            hipLaunchKernelGGL(lec_dropmask_kernel, dim3(a->t_count), dim3(64), 0, st, p);
        }
        if (!mask_only) hipLaunchKernelGGL(lec_vertical_kernel, dim3(a->t_count), dim3(64), 0, st, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}

extern "C" int lec_reduce(const lec_reduce_args* a) { return reduce_impl(a, false, "lec_reduce"); }
extern "C" int lec_dropmask(const lec_reduce_args* a) { return reduce_impl(a, true, "lec_dropmask"); }
