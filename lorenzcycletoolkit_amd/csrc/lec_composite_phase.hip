// lec_composite_phase.hip -- lec_composite_phase_sum and lec_composite_phase_ensemble: the phase-aligned ensembles of the composites of a
// BATCH of tracks (--batch-composites-phase; include/lec_hip_ext5.h).  A translation unit of its own: its code
// object is loaded by calls that ask for phases only, and no other kernel's text moves with it.
//
// A clock gives every track B ranges of its own steps; a CELL is one (track, bin).  lec_composite_phase_sum is lec_mapcol_segsum_kernel's
// running sum (lec_composite_steps.hip) over ranges that may be empty, may overlap and need not cover the call's boxes: a thread per
// (cell, term, row, column), the cell's boxes in table order, added to what the accumulator holds.  lec_composite_phase_ensemble is
// lec_composite_ensemble_kernel with a count per cell: a cell without steps has no mean and is no member of its bin's ensemble.
// One writer per output element, sums in a fixed order, nothing shared between threads.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/lec_hip_ext5.h"
#include "lec_internal.h"

namespace {

constexpr int kNMap = LEC_NMAP;
// loads issued before any of them is used, lec_mapcol.h's figure: the ORDER of the sum is that of the plain loop
constexpr int kSumBatch = 16;

struct PhaseSumParams {
    const double* col;       // [s_count][n]
    const int32_t* range;    // [n_cell][2]
    double* sum;             // [n_cell][n], +=
    size_t n;                // kNMap * nyb * nxb
    int n_cell, s_count;
};

// grid ceil(n_cell * n / 256), block 256: thread (cell, f, j, i), columns fastest
__global__ void __launch_bounds__(256) lec_composite_phase_sum_kernel(const PhaseSumParams p) {
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= p.n * p.n_cell) return;
    const size_t cell = id / p.n;
    const int a = p.range[2 * cell], b = p.range[2 * cell + 1];
    if (a < 0 || b < a || b > p.s_count) return;      // the host copy was refused for this; the device copy reads and writes nothing
    const int count = b - a;
    if (count == 0) return;
    const double* c = p.col + (size_t)a * p.n + (id - cell * p.n);
    double s = p.sum[id];
    for (int t0 = 0; t0 < count; t0 += kSumBatch) {
        double v[kSumBatch];
#pragma unroll
        for (int q = 0; q < kSumBatch; ++q) v[q] = c[(size_t)min(t0 + q, count - 1) * p.n];
#pragma unroll
        for (int q = 0; q < kSumBatch; ++q)
            if (t0 + q < count) s += v[q];
    }
    p.sum[id] = s;
}

struct PhaseEnsParams {
    const double* sum;       // [n_track][n_bin][n]
    const int32_t* count;    // [n_track][n_bin]
    double *mean, *ens, *spread;     // [n_track][n_bin][n] (may be `sum`), [n_bin][n], [n_bin][n]
    size_t n;
    int n_track, n_bin;
};

// grid ceil(n_bin * n / 256), block 256: thread (b, f, j, i); the tracks ascending, twice: the means and their sum, then the squares of
// the deviations.  A thread reads a sum before it writes the mean at the same place and reads back only what it wrote itself, so `mean`
// may be `sum`
__global__ void __launch_bounds__(256) lec_composite_phase_ensemble_kernel(const PhaseEnsParams p) {
#pragma clang fp contract(off)
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= p.n * p.n_bin) return;
    const size_t stride = p.n * p.n_bin;
    const int b = (int)(id / p.n);
    const double nan = __builtin_nan("");
    double s = 0.0;
    int members = 0;
    for (int k = 0; k < p.n_track; ++k) {
        const int c = p.count[(size_t)k * p.n_bin + b];
        double m = nan;
        if (c >= 1) {
            m = p.sum[k * stride + id] * (1.0 / (double)c);
            s = members == 0 ? m : s + m;
            ++members;
        }
        p.mean[k * stride + id] = m;
    }
    const double e = members ? s / (double)members : nan;
    p.ens[id] = e;
    double sq = 0.0;
    for (int k = 0; k < p.n_track; ++k)
        if (p.count[(size_t)k * p.n_bin + b] >= 1) {
            const double d = p.mean[k * stride + id] - e;
            sq += d * d;
        }
    p.spread[id] = members >= 2 ? sqrt(sq / (double)(members - 1)) : nan;
}

struct Refusals {
    const char* call;
    int refuse(int code, const char* what) const {
        char msg[320];
        snprintf(msg, sizeof(msg), "%s: %s", call, what);
        return lec_set_error(code, msg);
    }
};

}  // namespace

extern "C" int lec_composite_phase_sum(const lec_composite_phase_sum_args* a) {
    const Refusals chk{"lec_composite_phase_sum"};
    if (!a) return chk.refuse(LEC_ERR_ARG, "null args");
    if (!a->col_d) return chk.refuse(LEC_ERR_ARG, "null col_d (the columns lec_composite_steps left for the call's boxes)");
    if (!a->range_h) return chk.refuse(LEC_ERR_ARG, "null range_h (the host copy of the ranges: they are checked before anything is launched)");
    if (!a->range_d) return chk.refuse(LEC_ERR_ARG, "null range_d");
    if (!a->phasesum_d) return chk.refuse(LEC_ERR_ARG, "null phasesum_d");
    if (a->reserved0 != 0) return chk.refuse(LEC_ERR_ARG, "reserved0 must be 0");
    if (a->s_count < 1) return chk.refuse(LEC_ERR_ARG, "s_count must be >= 1");
    if (a->nyb < 1) return chk.refuse(LEC_ERR_ARG, "nyb must be >= 1");
    if (a->nxb < 1) return chk.refuse(LEC_ERR_ARG, "nxb must be >= 1");
    if (a->n_cell < 1) return chk.refuse(LEC_ERR_ARG, "n_cell must be >= 1");
    if ((uintptr_t)a->col_d % 8) return chk.refuse(LEC_ERR_ARG, "col_d must be 8-byte aligned");
    if ((uintptr_t)a->phasesum_d % 8) return chk.refuse(LEC_ERR_ARG, "phasesum_d must be 8-byte aligned");
    if ((uintptr_t)a->range_h % 4) return chk.refuse(LEC_ERR_ARG, "range_h must be 4-byte aligned");
    if ((uintptr_t)a->range_d % 4) return chk.refuse(LEC_ERR_ARG, "range_d must be 4-byte aligned");
    const long long n = (long long)kNMap * a->nyb * a->nxb;
    if (n >= (1LL << 32) - 256 || n * a->n_cell >= (1LL << 32) - 256)
        return chk.refuse(LEC_ERR_UNSUPPORTED, "n_cell * 6 * nyb * nxb must stay below 2^32 threads in one call");
    for (int c = 0; c < a->n_cell; ++c) {
        const int b = a->range_h[2 * (size_t)c], e = a->range_h[2 * (size_t)c + 1];
        if (b < 0 || e < b || e > a->s_count) {
            char m[200];
            snprintf(m, sizeof(m), "range_h: cell %d has the range [%d, %d), which must satisfy 0 <= begin <= end <= s_count = %d", c, b, e,
                     a->s_count);
            return chk.refuse(LEC_ERR_ARG, m);
        }
    }
    const PhaseSumParams p{a->col_d, a->range_d, a->phasesum_d, (size_t)n, a->n_cell, a->s_count};
    hipLaunchKernelGGL(lec_composite_phase_sum_kernel, dim3((unsigned)((n * a->n_cell + 255) / 256)), dim3(256), 0, (hipStream_t)a->stream, p);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(err));
    return LEC_OK;
}

extern "C" int lec_composite_phase_ensemble(const lec_composite_phase_ensemble_args* a) {
    const Refusals chk{"lec_composite_phase_ensemble"};
    if (!a) return chk.refuse(LEC_ERR_ARG, "null args");
    if (!a->phasesum_d) return chk.refuse(LEC_ERR_ARG, "null phasesum_d");
    if (!a->count_h) return chk.refuse(LEC_ERR_ARG, "null count_h (the host copy of the step counts: they are checked before anything is launched)");
    if (!a->count_d) return chk.refuse(LEC_ERR_ARG, "null count_d");
    if (!a->mean_d) return chk.refuse(LEC_ERR_ARG, "null mean_d");
    if (!a->ens_d) return chk.refuse(LEC_ERR_ARG, "null ens_d");
    if (!a->spread_d) return chk.refuse(LEC_ERR_ARG, "null spread_d");
    if (a->reserved0 != 0) return chk.refuse(LEC_ERR_ARG, "reserved0 must be 0");
    if (a->n_track < 1) return chk.refuse(LEC_ERR_ARG, "n_track must be >= 1");
    if (a->n_bin < 1) return chk.refuse(LEC_ERR_ARG, "n_bin must be >= 1");
    if (a->nyb < 1) return chk.refuse(LEC_ERR_ARG, "nyb must be >= 1");
    if (a->nxb < 1) return chk.refuse(LEC_ERR_ARG, "nxb must be >= 1");
    if ((uintptr_t)a->count_h % 4) return chk.refuse(LEC_ERR_ARG, "count_h must be 4-byte aligned");
    if ((uintptr_t)a->count_d % 4) return chk.refuse(LEC_ERR_ARG, "count_d must be 4-byte aligned");
    if ((uintptr_t)a->phasesum_d % 8) return chk.refuse(LEC_ERR_ARG, "phasesum_d must be 8-byte aligned");
    if ((uintptr_t)a->mean_d % 8) return chk.refuse(LEC_ERR_ARG, "mean_d must be 8-byte aligned");
    if ((uintptr_t)a->ens_d % 8) return chk.refuse(LEC_ERR_ARG, "ens_d must be 8-byte aligned");
    if ((uintptr_t)a->spread_d % 8) return chk.refuse(LEC_ERR_ARG, "spread_d must be 8-byte aligned");
    const long long n = (long long)kNMap * a->nyb * a->nxb;
    if (n >= (1LL << 32) - 256 || n * a->n_bin >= (1LL << 32) - 256)
        return chk.refuse(LEC_ERR_UNSUPPORTED, "n_bin * 6 * nyb * nxb must stay below 2^32 threads in one call");
    for (int k = 0; k < a->n_track; ++k)
        for (int b = 0; b < a->n_bin; ++b) {
            const int c = a->count_h[(size_t)k * a->n_bin + b];
            if (c < 0) {
                char m[160];
                snprintf(m, sizeof(m), "count_h: track %d, bin %d has %d steps, a count cannot be negative", k, b, c);
                return chk.refuse(LEC_ERR_ARG, m);
            }
        }
    const PhaseEnsParams p{a->phasesum_d, a->count_d, a->mean_d, a->ens_d, a->spread_d, (size_t)n, a->n_track, a->n_bin};
    hipLaunchKernelGGL(lec_composite_phase_ensemble_kernel, dim3((unsigned)((n * a->n_bin + 255) / 256)), dim3(256), 0, (hipStream_t)a->stream,
                       p);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(err));
    return LEC_OK;
}
