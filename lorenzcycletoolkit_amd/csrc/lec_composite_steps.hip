// lec_composite_steps.hip -- lec_composite_steps and lec_composite_ensemble: the system-relative composites of a BATCH of tracks over one
// union cube and their ensemble mean (-t --trackfiles / -c --choose-systems --batch-composites; include/lec_hip_ext3.h, DESIGN.md section
// 4.2g).  A translation unit of its own: its code object is loaded by calls that ask for batch composites only.
//
// lec_composite_steps is lec_composite (lec_composite.hip) with two things changed.  Each box names its cube step and the step's two time
// neighbours in a table, as lec_rowstats_steps takes it: lec_mapcol.h's column kernel in its DMODE 3, whose launch struct adds the table
// to lec_composite's per-step members (wave-uniform: scalar loads).  And the time sums are kept per SEGMENT of the call's boxes -- one
// segment per track --: lec_mapcol_segsum_kernel, lec_mapcol_sum_kernel's running sum with a thread per (segment, term, row, column).
// The factors and the Hovmoeller rows are per box, lec_mapcol.h's kernels as they are.
#include "../../include/lec_hip_ext3.h"
#include "lec_mapcol.h"

namespace {
using namespace lec;

struct ColParams : MapColGrid {
    const int32_t* step;     // [t_count][3] {t, t_prev, t_next}: absolute cube steps (DMODE 3)
    const int32_t* box;      // [t_count][4] in the cube
    const double* boxtab;    // [t_count][4]: [2] = 1 / h_deg
    const double* lattab;    // [t_count][nyb][4]
    __device__ int iw(int tl) const { return box[4 * tl + 0]; }
    __device__ int js(int tl) const { return box[4 * tl + 2]; }
    __device__ const double* lattab_row(int tl, int jb) const { return lattab + ((size_t)tl * nyb + jb) * 4; }
    __device__ double inv_hdeg(int tl) const { return boxtab[4 * tl + 2]; }
};

struct SegSumParams {
    MapFoldParams f;         // mapsum: [n_seg][kNMap][nyb][nxb]
    const int32_t* seg;      // [n_seg + 1]
    int n_seg;
};

// grid ceil(n_seg * kNMap * nyb * nxb / 256), block 256: thread (g, f, j, i), columns fastest; segment g's boxes in table order, added
// to what mapsum[g] holds.  lec_mapcol_sum_kernel's loop over a segment's boxes, loads kSumBatch ahead.  (The loop is written out here: as
// a __device__ function shared with lec_mapcol_sum_kernel it swapped the operands of that kernel's adds, and lec_maps / lec_composite
// keep their instructions.)
__global__ void __launch_bounds__(256) lec_mapcol_segsum_kernel(const SegSumParams p) {
    const size_t n = (size_t)kNMap * p.f.nyb * p.f.nxb;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n * p.n_seg) return;
    const size_t g = id / n;
    const int a = p.seg[g], count = p.seg[g + 1] - a;
    const double* __restrict__ c = p.f.col + (size_t)a * n + (id - g * n);
    double s = p.f.mapsum[id];
    for (int t0 = 0; t0 < count; t0 += kSumBatch) {
        double v[kSumBatch];
#pragma unroll
        for (int q = 0; q < kSumBatch; ++q) v[q] = c[(size_t)min(t0 + q, count - 1) * n];
#pragma unroll
        for (int q = 0; q < kSumBatch; ++q)
            if (t0 + q < count) s += v[q];
    }
    p.f.mapsum[id] = s;
}

struct EnsParams {
    const double* mapsum;    // [n_track][n]
    const int32_t* count;    // [n_track]
    double *mean, *ens;      // [n_track][n], [n]
    int n_track;
    size_t n;
};

// grid ceil(n / 256), block 256: thread (f, j, i); the tracks ascending.  A track's mean is its sum TIMES the rounded reciprocal of its
// step count: the product LECEngine.composite_finish's division by a host scalar forms, so the mean has the bits of the track's own run
__global__ void __launch_bounds__(256) lec_composite_ensemble_kernel(const EnsParams p) {
#pragma clang fp contract(off)
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= p.n) return;
    double s = 0.0;
    for (int k = 0; k < p.n_track; ++k) {
        const double m = p.mapsum[(size_t)k * p.n + id] * (1.0 / (double)p.count[k]);
        p.mean[(size_t)k * p.n + id] = m;
        s = k == 0 ? m : s + m;
    }
    p.ens[id] = s / (double)p.n_track;
}

}  // namespace

extern "C" int lec_composite_steps(const lec_composite_steps_args* a) {
    const MapcolRefusals chk{"lec_composite_steps"};
    if (!a) return chk.refuse(LEC_ERR_ARG, "null args");
    if (!a->tair_d) return chk.refuse(LEC_ERR_ARG, "null tair_d");
    if (!a->u_d) return chk.refuse(LEC_ERR_ARG, "null u_d");
    if (!a->v_d) return chk.refuse(LEC_ERR_ARG, "null v_d");
    if (!a->omega_d) return chk.refuse(LEC_ERR_ARG, "null omega_d");
    if (!a->step_h) return chk.refuse(LEC_ERR_ARG, "null step_h (the host copy of the step table: its entries are checked before anything is launched)");
    if (!a->step_d) return chk.refuse(LEC_ERR_ARG, "null step_d");
    if (!a->seg_h) return chk.refuse(LEC_ERR_ARG, "null seg_h (the host copy of the segments: they are checked before anything is launched)");
    if (!a->seg_d) return chk.refuse(LEC_ERR_ARG, "null seg_d");
    if (!a->box_h) return chk.refuse(LEC_ERR_ARG, "null box_h (the host copy of the boxes: their shapes are checked before anything is launched)");
    if (!a->box_d) return chk.refuse(LEC_ERR_ARG, "null box_d");
    if (!a->boxtab_d) return chk.refuse(LEC_ERR_ARG, "null boxtab_d");
    if (!a->lattab_d) return chk.refuse(LEC_ERR_ARG, "null lattab_d");
    if (!a->lattab2_d) return chk.refuse(LEC_ERR_ARG, "null lattab2_d");
    if (!a->rows_d) return chk.refuse(LEC_ERR_ARG, "null rows_d");
    if (!a->levraw_d) return chk.refuse(LEC_ERR_ARG, "null levraw_d");
    if (!a->levtab_d) return chk.refuse(LEC_ERR_ARG, "null levtab_d");
    if (!a->levtab2_d) return chk.refuse(LEC_ERR_ARG, "null levtab2_d");
    if (!a->tcoef_d) return chk.refuse(LEC_ERR_ARG, "null tcoef_d ([s_count][3], by box)");
    if (!a->coef_d) return chk.refuse(LEC_ERR_ARG, "null coef_d (the workspace of the row factors)");
    if (!a->col_d) return chk.refuse(LEC_ERR_ARG, "null col_d (the column values, which are the workspace of the sums too)");
    if (!a->hov_d) return chk.refuse(LEC_ERR_ARG, "null hov_d");
    if (!a->mapsum_d) return chk.refuse(LEC_ERR_ARG, "null mapsum_d");
    if (int r = chk.dtype(a->dtype)) return r;
    if (a->reserved0 != 0) return chk.refuse(LEC_ERR_ARG, "reserved0 must be 0");
    if (a->nt < 1) return chk.refuse(LEC_ERR_ARG, "nt must be >= 1");
    if (int r = chk.levels(a->nl)) return r;
    if (a->nyb < 2) return chk.refuse(LEC_ERR_ARG, "nyb must be >= 2 (a box needs two rows for d/dlat)");
    if (a->nxb < 3) return chk.refuse(LEC_ERR_ARG, "nxb must be >= 3 (a composite needs three box columns)");
    if (a->ny < a->nyb) return chk.refuse(LEC_ERR_ARG, "ny must be >= nyb");
    if (a->nx < a->nxb) return chk.refuse(LEC_ERR_ARG, "nx must be >= nxb");
    if (a->s_count < 1) return chk.refuse(LEC_ERR_ARG, "s_count must be >= 1");
    if ((uintptr_t)a->step_d % 4) return chk.refuse(LEC_ERR_ARG, "step_d must be 4-byte aligned");
    if ((uintptr_t)a->step_h % 4) return chk.refuse(LEC_ERR_ARG, "step_h must be 4-byte aligned");
    if ((uintptr_t)a->seg_d % 4) return chk.refuse(LEC_ERR_ARG, "seg_d must be 4-byte aligned");
    if ((uintptr_t)a->seg_h % 4) return chk.refuse(LEC_ERR_ARG, "seg_h must be 4-byte aligned");
    if ((uintptr_t)a->box_d % 4) return chk.refuse(LEC_ERR_ARG, "box_d must be 4-byte aligned");
    if ((uintptr_t)a->box_h % 4) return chk.refuse(LEC_ERR_ARG, "box_h must be 4-byte aligned");
    char m[256];
    // the tables on their HOST copies, before any HIP call
    static const char* const entry[3] = {"t", "t_prev", "t_next"};
    for (int s = 0; s < a->s_count; ++s)
        for (int q = 0; q < 3; ++q) {
            const int v = a->step_h[3 * (size_t)s + q];
            if (v < 0 || v >= a->nt) {
                snprintf(m, sizeof(m), "step_h: box %d names cube step %d as its %s (entry %d), outside [0, %d)", s, v, entry[q], q, a->nt);
                return chk.refuse(LEC_ERR_ARG, m);
            }
        }
    if (a->n_seg < 1) return chk.refuse(LEC_ERR_ARG, "n_seg must be >= 1");
    if (a->seg_h[0] != 0) return chk.refuse(LEC_ERR_ARG, "seg_h[0] must be 0");
    for (int g = 0; g < a->n_seg; ++g)
        if (a->seg_h[g + 1] <= a->seg_h[g]) {
            snprintf(m, sizeof(m), "seg_h: offsets must ascend and no segment may be empty: seg_h[%d] = %d, seg_h[%d] = %d", g, a->seg_h[g], g + 1,
                     a->seg_h[g + 1]);
            return chk.refuse(LEC_ERR_ARG, m);
        }
    if (a->seg_h[a->n_seg] != a->s_count) {
        snprintf(m, sizeof(m), "seg_h[n_seg] = %d must be s_count = %d", a->seg_h[a->n_seg], a->s_count);
        return chk.refuse(LEC_ERR_ARG, m);
    }
    if (int r = chk.boxes(a, a->s_count, "box")) return r;
    if (int r = chk.align16(a->rows_d, a->lattab2_d, a->coef_d)) return r;
    const void* tabs[] = {a->levraw_d, a->levtab2_d, a->lattab_d, a->levtab_d, a->tcoef_d, a->boxtab_d, a->col_d, a->hov_d, a->mapsum_d};
    const char* tabn[] = {"levraw_d", "levtab2_d", "lattab_d", "levtab_d", "tcoef_d", "boxtab_d", "col_d", "hov_d", "mapsum_d"};
    const void* cubes[] = {a->tair_d, a->u_d, a->v_d, a->omega_d};
    const int nyb = a->nyb, nxb = a->nxb, n_seg = a->n_seg;
    if (int r = chk.tables_cubes_limits({tabs, tabn, 9, cubes, 4, "tair_d, u_d, v_d, omega_d", a->dtype}, a->s_count, a->nl, nyb, nxb, "nyb, nxb"))
        return r;
    if ((long long)n_seg * kNMap * nyb * nxb >= (1LL << 32) - 256)
        return chk.refuse(LEC_ERR_UNSUPPORTED, "n_seg * 6 * nyb * nxb must stay below 2^32 threads in one call");

    ColParams p;
    p.step = a->step_d; p.box = a->box_d; p.boxtab = a->boxtab_d; p.lattab = a->lattab_d;
    const int32_t* seg_d = a->seg_d;
    const int dtype = a->dtype;
    const MapcolRun run{a->col_d, a->mapsum_d, a->hov_d, nyb, 0, a->s_count};      // the call's steps are its boxes
    return mapcol_launch(a, p, run, nyb, nxb, nyb * 8,
                         [dtype](const ColParams& q, dim3 grid, hipStream_t st) { mapcol_col<false, 3>(q, dtype, grid, st); },
                         [seg_d, n_seg, nyb, nxb](const MapFoldParams& f, hipStream_t st) {
                             const SegSumParams sp{f, seg_d, n_seg};
                             hipLaunchKernelGGL(lec_mapcol_segsum_kernel, dim3((unsigned)(((long long)n_seg * kNMap * nyb * nxb + 255) / 256)),
                                                dim3(256), 0, st, sp);
                         });
}

extern "C" int lec_composite_ensemble(const lec_composite_ensemble_args* a) {
    const MapcolRefusals chk{"lec_composite_ensemble"};
    if (!a) return chk.refuse(LEC_ERR_ARG, "null args");
    if (!a->mapsum_d) return chk.refuse(LEC_ERR_ARG, "null mapsum_d");
    if (!a->count_h) return chk.refuse(LEC_ERR_ARG, "null count_h (the host copy of the step counts: they are checked before anything is launched)");
    if (!a->count_d) return chk.refuse(LEC_ERR_ARG, "null count_d");
    if (!a->mean_d) return chk.refuse(LEC_ERR_ARG, "null mean_d");
    if (!a->ens_d) return chk.refuse(LEC_ERR_ARG, "null ens_d");
    if (a->reserved0 != 0) return chk.refuse(LEC_ERR_ARG, "reserved0 must be 0");
    if (a->n_track < 1) return chk.refuse(LEC_ERR_ARG, "n_track must be >= 1");
    if (a->nyb < 1 || a->nxb < 1) return chk.refuse(LEC_ERR_ARG, "nyb and nxb must be >= 1");
    if ((uintptr_t)a->count_h % 4) return chk.refuse(LEC_ERR_ARG, "count_h must be 4-byte aligned");
    if ((uintptr_t)a->count_d % 4) return chk.refuse(LEC_ERR_ARG, "count_d must be 4-byte aligned");
    if ((uintptr_t)a->mapsum_d % 8) return chk.refuse(LEC_ERR_ARG, "mapsum_d must be 8-byte aligned");
    if ((uintptr_t)a->mean_d % 8) return chk.refuse(LEC_ERR_ARG, "mean_d must be 8-byte aligned");
    if ((uintptr_t)a->ens_d % 8) return chk.refuse(LEC_ERR_ARG, "ens_d must be 8-byte aligned");
    for (int k = 0; k < a->n_track; ++k)
        if (a->count_h[k] < 1) {
            char m[128];
            snprintf(m, sizeof(m), "count_h: track %d has %d steps, a mean needs at least 1", k, a->count_h[k]);
            return chk.refuse(LEC_ERR_ARG, m);
        }
    const long long n = (long long)kNMap * a->nyb * a->nxb;
    if (n >= (1LL << 32) - 256) return chk.refuse(LEC_ERR_UNSUPPORTED, "6 * nyb * nxb must stay below 2^32 threads");
    const EnsParams p{a->mapsum_d, a->count_d, a->mean_d, a->ens_d, a->n_track, (size_t)n};
    hipLaunchKernelGGL(lec_composite_ensemble_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)a->stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}
