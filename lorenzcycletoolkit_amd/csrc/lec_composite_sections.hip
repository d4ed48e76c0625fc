// lec_composite_sections.hip -- lec_composite_sections: the SYSTEM-RELATIVE latitude x pressure sections of the ten terms of the cycle over
// a series of per-step boxes that all have one ROW COUNT (-t / -c --composite-sections; include/lec_hip_ext2.h).
// A translation unit of its own: its code object is loaded by calls that ask for these sections only.
//
// The call is lec_sections (lec_sections.hip) with three things lifted to "per step": the box (box_d + 4 t), the latitude table
// (lattab2_d + t * nyb * 8) and with it the area means, formed with that step's cw.  The box-relative row j takes the place of the fixed
// box's.  The two kernels -- integrands, divisors, the trapezoid with its NaN rule, the time sums in time order -- are
// lec_section_core.h's, instantiated here on the per-step form; the step's table base is wave-uniform (scalar loads and address
// arithmetic).  Only row records are read: the boxes' widths may differ, and there is no spectral input (no spectra on open boxes).
#include "../../include/lec_hip_ext2.h"
#include "lec_section_core.h"

namespace {
using namespace lec;

struct StepSecParams {
    const double* rows;      // [t_count][nl][nyb][LEC_NSTAT]
    int t_count, nl, nyb;
    const int* box;          // [t_count][4]
    const double* lattab2;   // [t_count][nyb][8]
    const double* levtab2;
    const double* levraw;    // [t_count][nl][LEC_NLEVRAW]
    double* sec;             // [t_count][nl][10][nyb]
    // the step's own box (its row count was checked on the host) and table
    static constexpr bool kSpectral = false;
    static __device__ const int* box_of(const int* b, int tl) { return b + 4 * (size_t)tl; }
    static __device__ const double* lattab2_of(const double* lt, int tl, int nyb) { return lt + (size_t)tl * nyb * 8; }
};

int refuse(int code, const char* what) {
    char msg[320];
    snprintf(msg, sizeof(msg), "lec_composite_sections: %s", what);
    return lec_set_error(code, msg);
}

}  // namespace

extern "C" int lec_composite_sections(const lec_composite_sections_args* a) {
    if (!a) return refuse(LEC_ERR_ARG, "null args");
    if (!a->rows_d) return refuse(LEC_ERR_ARG, "null rows_d");
    if (!a->levraw_d) return refuse(LEC_ERR_ARG, "null levraw_d");
    if (!a->box_h) return refuse(LEC_ERR_ARG, "null box_h (the host copy of the boxes: their row counts are checked before anything is launched)");
    if (!a->box_d) return refuse(LEC_ERR_ARG, "null box_d");
    if (!a->lattab2_d) return refuse(LEC_ERR_ARG, "null lattab2_d");
    if (!a->levtab2_d) return refuse(LEC_ERR_ARG, "null levtab2_d");
    if (!a->sec_d) return refuse(LEC_ERR_ARG, "null sec_d");
    if (!a->col_d) return refuse(LEC_ERR_ARG, "null col_d");
    if (!a->secsum_d) return refuse(LEC_ERR_ARG, "null secsum_d");
    if (a->t_count < 1) return refuse(LEC_ERR_ARG, "t_count must be >= 1");
    if (a->nl < 2) return refuse(LEC_ERR_ARG, "nl must be >= 2");
    if (a->nyb < 2) return refuse(LEC_ERR_ARG, "nyb must be >= 2");
    if (a->nl > LEC_MAX_LEVELS) return refuse(LEC_ERR_UNSUPPORTED, "nl above LEC_MAX_LEVELS (160)");
    if (a->reserved0 != 0) return refuse(LEC_ERR_ARG, "reserved0 must be 0");
    if ((uintptr_t)a->rows_d % 16) return refuse(LEC_ERR_ARG, "rows_d must be 16-byte aligned");
    if ((uintptr_t)a->lattab2_d % 16) return refuse(LEC_ERR_ARG, "lattab2_d must be 16-byte aligned");
    // HIP takes fewer than 2^32 threads per launch: one 64-lane workgroup per (time step, level), one thread per (term, row) of the fold
    if ((long long)a->t_count * a->nl >= (1LL << 26))
        return refuse(LEC_ERR_UNSUPPORTED, "t_count * nl must stay below 2^26 in one call (cut the series into several calls)");
    if ((long long)kNSec * a->nyb >= (1LL << 32) - 64)
        return refuse(LEC_ERR_UNSUPPORTED, "10 * nyb must stay below 2^32 threads in one call");
    // every box nyb rows high: on the HOST copy, before any HIP call
    for (int t = 0; t < a->t_count; ++t) {
        const int32_t* b = a->box_h + 4 * (size_t)t;
        const long long h = (long long)b[3] - b[2] + 1;
        if (h != a->nyb) {
            char m[256];
            snprintf(m, sizeof(m), "box_h: the box of step %d has %lld rows, the call's nyb is %d: every box of a system-relative section "
                     "has one row count", t, h, a->nyb);
            return refuse(LEC_ERR_ARG, m);
        }
    }

    hipStream_t st = (hipStream_t)a->stream;
    StepSecParams p;
    p.rows = a->rows_d; p.t_count = a->t_count; p.nl = a->nl; p.nyb = a->nyb;
    p.box = a->box_d; p.lattab2 = a->lattab2_d; p.levtab2 = a->levtab2_d; p.levraw = a->levraw_d; p.sec = a->sec_d;
    hipLaunchKernelGGL(lec_section_rows_kernel<StepSecParams>, dim3((unsigned)(a->t_count * a->nl)), dim3(64), 0, st, p);
    const FoldParams f = section_fold_totals(a->sec_d, a->levtab2_d, a->t_count, a->nl, a->nyb, a->col_d, a->secsum_d);
    // a moving series is many steps of few rows: the steps' scans side by side, then the levels' time sums side by side (in time order each)
    const unsigned nblk = (unsigned)(((long long)kNSec * a->nyb + 63) / 64);
    hipLaunchKernelGGL(lec_section_fold_kernel<kFoldScan>, dim3(nblk, (unsigned)(a->t_count < 65535 ? a->t_count : 65535)), dim3(64), 0, st, f);
    hipLaunchKernelGGL(lec_section_fold_kernel<kFoldSum>, dim3(nblk, (unsigned)a->nl), dim3(64), 0, st, f);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}
