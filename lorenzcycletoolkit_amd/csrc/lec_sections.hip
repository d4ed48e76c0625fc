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
// The two kernel bodies are lec_section_core.h's (shared with lec_composite_sections.hip), instantiated here on the FIXED form: one box and
// one lattab2 for every step.
#include "lec_section_core.h"

namespace {
using namespace lec;

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
    // one fixed box: every step's box and table are the call's
    static constexpr bool kSpectral = true;
    static __device__ const int* box_of(const int* b, int) { return b; }
    static __device__ const double* lattab2_of(const double* lt, int, int) { return lt; }
};

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
    hipLaunchKernelGGL(lec_section_rows_kernel<SecParams>, grid, dim3(64), 0, st, p);

    const FoldParams f = section_fold_totals(a->sec_d, a->levtab2_d, a->t_count, a->nl, a->nyb, a->col_d, a->secsum_d);
    hipLaunchKernelGGL(lec_section_fold_kernel<kFoldWhole>, dim3((unsigned)(((long long)kNSec * a->nyb + 63) / 64)), dim3(64), 0, st, f);
    if (p.n_wave > 0) {
        FoldParams s = f;
        s.sec = a->specsec_d; s.n_fn = p.n_wave * n_specfn; s.fn_period = n_specfn;
        s.f_2g_a = s.f_2g_b = 1; s.f_g = 4;     // Ae Ke Ca Ce Ck (Ge)
        s.col = nullptr; s.colsum = a->speccolsum_d; s.secsum = nullptr;
        hipLaunchKernelGGL(lec_section_fold_kernel<kFoldWhole>, dim3((unsigned)(((long long)s.n_fn * a->nyb + 63) / 64)), dim3(64), 0, st, s);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}
