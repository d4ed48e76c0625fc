// lec_level_spec.hip -- lec_level_spec_ring and lec_level_spec_b_ring: the level x latitude half of stage 2 for the zonal-wavenumber
// spectra of a ring (-f --periodic --wavenumbers; include/lec_hip.h).  A translation unit of its own: the code
// object is loaded by spectral calls only.
//
// X(n) is what stage 2 gives on the ring pass's row records with slots LEC_S_TT .. LEC_S_WV (6 .. 13) replaced by lec_rowspec_ring's
// shares of wavenumber n and slot LEC_S_QT (15) by lec_rowspec_q_ring's.  lec_reduce needs those records assembled in memory, N copies of
// every record.  Here the level kernels lec_reduce runs (lec_level_core.h) are instantiated on another record source, SpecRecords: one
// workgroup per (wavenumber, time step, level) loads the ring pass's record and takes the nine slots straight from spec_d / qspec_d, in
// the register array for bands of at most 64 rows, in the LDS tile for taller ones.  The area means are formed once per (time step,
// level): no replaced slot enters them.  BAz's bottom-top term is repaired per latitude from OTHER levels' LEC_S_WT: a replaced slot,
// read from spec_d at that level.
#include <stdio.h>

#include "lec_level_core.h"

namespace {
using namespace lec;

constexpr int kSpecSlots = 8;      // LEC_S_TT .. LEC_S_WV
constexpr int kBudgetSlots = 4;    // lec_rowspec_b_ring's: LEC_S_VTT, LEC_S_WTT, LEC_S_EV, LEC_S_EW
static_assert(LEC_S_WV - LEC_S_TT + 1 == kSpecSlots && LEC_S_QT == LEC_S_WV + 2, "slots 6 .. 13 and 15 are the replaced ones");

struct SpecLevParams {
    const double* rows;     // [t_count][nl][nyb_max][LEC_NSTAT]
    const double* spec;     // [t_count][nl][nyb_max][n_wave][8]
    const double* qspec;    // [t_count][nl][nyb_max][n_wave] or null
    int t_count, nl, nyb_max, n_wave;      // nyb_max: the rows of the record buffer (the call's nyb)
    const int* box;
    const double* lattab2;
    const double* levtab2;
    double phi_scale;
    double* am;             // [t_count][nl][8]
    double* levraw;
    long long wstride;      // doubles between consecutive wavenumbers of levraw
    const double* bspec;    // [t_count][nl][nyb_max][n_wave][4], the instantiations of lec_level_spec_b_ring only
};

// lec_level_core.h's record source for the ring pass's records with the shares of wavenumber n in slots 6 .. 13 (and 15 where qspec is
// given): one workgroup per (wavenumber, time step, level) -- level fastest, then time step, then wavenumber --, always box 0, no taller
// than the record buffer, wavenumber n's levraw records at n * wstride.  The area means come from `am`, which the area-means kernel
// writes for every band height.
// B (lec_level_spec_b_ring): slots LEC_S_VTT, LEC_S_WTT, LEC_S_EV, LEC_S_EW likewise, from bspec; instantiations of their own, those
// without it are the kernels lec_level_spec_ring has always launched.
template <bool B>
struct SpecRecords {
    using Params = SpecLevParams;
    static constexpr bool kMeansInSmallKernel = false;
    int n, tl, k;
    __device__ __forceinline__ SpecRecords(const SpecLevParams& p, unsigned block) {
        const int per_wave = p.t_count * p.nl;
        n = block / per_wave;
        const int tk = block - n * per_wave;
        tl = tk / p.nl; k = tk - tl * p.nl;
    }
    static __device__ __forceinline__ int box_index(const SpecLevParams&, int) { return 0; }
    static __device__ __forceinline__ int band_rows(const SpecLevParams& p, int h) { return min(h, p.nyb_max); }
    __device__ __forceinline__ double* out(const SpecLevParams& p) const {
        return p.levraw + (size_t)n * (size_t)p.wstride + (size_t)(tl * p.nl + k) * LEC_NLEVRAW;
    }
    struct Shares { dbl2_t s0, s1, s2, s3; double sq; dbl2_t b0, b1; };
    // the wavenumber's shares of the lane's own row
    __device__ __forceinline__ Shares load_shares(const SpecLevParams& p, int jbc) const {
        const size_t srow = ((size_t)(tl * p.nl + k) * p.nyb_max + jbc) * p.n_wave + n;
        const dbl2_t* sp = reinterpret_cast<const dbl2_t*>(p.spec + srow * kSpecSlots);
        Shares s{sp[0], sp[1], sp[2], sp[3], p.qspec ? p.qspec[srow] : 0.0, {0.0, 0.0}, {0.0, 0.0}};
        if (B) {
            const dbl2_t* bp = reinterpret_cast<const dbl2_t*>(p.bspec + srow * kBudgetSlots);
            s.b0 = bp[0]; s.b1 = bp[1];
        }
        return s;
    }
    __device__ __forceinline__ void put(const SpecLevParams& p, const Shares& s, double* r) const {
        r[LEC_S_TT + 0] = s.s0.x; r[LEC_S_TT + 1] = s.s0.y; r[LEC_S_TT + 2] = s.s1.x; r[LEC_S_TT + 3] = s.s1.y;
        r[LEC_S_TT + 4] = s.s2.x; r[LEC_S_TT + 5] = s.s2.y; r[LEC_S_TT + 6] = s.s3.x; r[LEC_S_TT + 7] = s.s3.y;
        if (p.qspec) r[LEC_S_QT] = s.sq;
        if (B) { r[LEC_S_VTT] = s.b0.x; r[LEC_S_WTT] = s.b0.y; r[LEC_S_EV] = s.b1.x; r[LEC_S_EW] = s.b1.y; }
    }
    // [w'T'] of another level: the wavenumber's share there
    __device__ __forceinline__ double wT(const SpecLevParams& p, const double*, size_t row) const {
        return p.spec[(row * p.n_wave + n) * kSpecSlots + (LEC_S_WT - LEC_S_TT)];
    }
    __device__ __forceinline__ double small_mean_T(const SpecLevParams&, const double* am, const double*, int, int level) const {
        return am[8 * level + 0];
    }
};

// a refusal of either call, under the call's own name
int refuse(int code, const char* who, const char* what) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return lec_set_error(code, msg);
}

// both calls: `who` names the call, `bspec` is lec_level_spec_b_ring's fourth input (checked by the caller) or null
int level_spec(const lec_level_spec_args* a, const double* bspec, const char* who) {
    if (!a) return refuse(LEC_ERR_ARG, who, "null args");
    if (!a->rows_d) return refuse(LEC_ERR_ARG, who, "null rows_d");
    if (!a->spec_d) return refuse(LEC_ERR_ARG, who, "null spec_d");
    if (!a->box_d) return refuse(LEC_ERR_ARG, who, "null box_d");
    if (!a->lattab2_d) return refuse(LEC_ERR_ARG, who, "null lattab2_d");
    if (!a->levtab2_d) return refuse(LEC_ERR_ARG, who, "null levtab2_d");
    if (!a->am_d) return refuse(LEC_ERR_ARG, who, "null am_d");
    if (!a->levraw_d) return refuse(LEC_ERR_ARG, who, "null levraw_d");
    if ((uintptr_t)a->rows_d % 16) return refuse(LEC_ERR_ARG, who, "rows_d must be 16-byte aligned");
    if ((uintptr_t)a->spec_d % 16) return refuse(LEC_ERR_ARG, who, "spec_d must be 16-byte aligned");
    if ((uintptr_t)a->lattab2_d % 16) return refuse(LEC_ERR_ARG, who, "lattab2_d must be 16-byte aligned");
    if (a->n_wave < 1) return refuse(LEC_ERR_ARG, who, "n_wave must be >= 1");
    if (a->t_count < 1) return refuse(LEC_ERR_ARG, who, "t_count must be >= 1");
    if (a->nl < 1) return refuse(LEC_ERR_ARG, who, "nl must be >= 1");
    if (a->nyb < 2) return refuse(LEC_ERR_ARG, who, "nyb must be >= 2 (a band needs two rows)");
    if (a->n_wave > LEC_MAX_WAVENUMBERS) return refuse(LEC_ERR_UNSUPPORTED, who, "n_wave above LEC_MAX_WAVENUMBERS");
    if (a->nl > LEC_MAX_LEVELS) return refuse(LEC_ERR_UNSUPPORTED, who, "nl above LEC_MAX_LEVELS");
    // one 64-lane workgroup per (n, t, k), and HIP takes fewer than 2^32 threads per launch
    if ((long long)a->n_wave * a->t_count * a->nl >= (1LL << 26))
        return refuse(LEC_ERR_UNSUPPORTED, who, "n_wave * t_count * nl must stay below 2^26 in one call (cut the series into several calls)");
    const long long dense = (long long)a->t_count * a->nl * LEC_NLEVRAW;
    if (a->wave_stride != 0 && a->wave_stride < dense)
        return refuse(LEC_ERR_ARG, who, "wave_stride must be 0 (dense) or at least t_count * nl * LEC_NLEVRAW");
    SpecLevParams p;
    p.rows = a->rows_d; p.spec = a->spec_d; p.qspec = a->qspec_d; p.bspec = bspec;
    p.t_count = a->t_count; p.nl = a->nl; p.nyb_max = a->nyb; p.n_wave = a->n_wave;
    p.box = a->box_d; p.lattab2 = a->lattab2_d; p.levtab2 = a->levtab2_d; p.phi_scale = a->phi_scale;
    p.am = a->am_d; p.levraw = a->levraw_d; p.wstride = a->wave_stride ? a->wave_stride : dense;
    hipStream_t st = (hipStream_t)a->stream;
    const dim3 grid_tk((unsigned)(a->t_count * a->nl)), grid((unsigned)(a->n_wave * a->t_count * a->nl));
    hipLaunchKernelGGL(lec_area_means_kernel<SpecRecords<false>>, grid_tk, dim3(64), 0, st, p);      // (no share enters the means)
    if (bspec) {
        if (a->nyb <= kSmallRows) hipLaunchKernelGGL(lec_level_small_kernel<SpecRecords<true>>, grid, dim3(64), 0, st, p);
        else hipLaunchKernelGGL(lec_level_terms_kernel<SpecRecords<true>>, grid, dim3(64), 0, st, p);
    } else {
        if (a->nyb <= kSmallRows) hipLaunchKernelGGL(lec_level_small_kernel<SpecRecords<false>>, grid, dim3(64), 0, st, p);
        else hipLaunchKernelGGL(lec_level_terms_kernel<SpecRecords<false>>, grid, dim3(64), 0, st, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}

}  // namespace

extern "C" int lec_level_spec_ring(const lec_level_spec_args* a) { return level_spec(a, nullptr, "lec_level_spec_ring"); }

extern "C" int lec_level_spec_b_ring(const lec_level_spec_b_args* a) {
    if (!a) return lec_set_error(LEC_ERR_ARG, "lec_level_spec_b_ring: null args");
    if (!a->bspec_d) return lec_set_error(LEC_ERR_ARG, "lec_level_spec_b_ring: null bspec_d");
    if ((uintptr_t)a->bspec_d % 16) return lec_set_error(LEC_ERR_ARG, "lec_level_spec_b_ring: bspec_d must be 16-byte aligned");
    return level_spec(&a->spec, a->bspec_d, "lec_level_spec_b_ring");
}
