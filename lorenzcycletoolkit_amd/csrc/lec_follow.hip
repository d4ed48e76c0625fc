// lec_follow.hip -- -c/--choose without a display: the box follows the 850-hPa system on the device (gfx950, wave64).
//
// The reference's chooser is a click loop: it draws the 850-hPa vorticity, height and wind of a time step, circles the vorticity minimum
// of the current box and waits for the user to drag the next box (select_area.py:106-155,201-251; lec_moving_framework.py:227-245).
// Here the loop closes itself: the extremum of step t inside a search window around the centre of step t - 1 is the centre of step t.
// The chain is sequential in time, so it runs inside ONE workgroup: nothing waits for another workgroup, the centre passes from
// step to step through LDS.  Per step: the field on the window grown by the smoothing radius into an LDS tile, the box mean from the
// tile, the extremum with its row-major index (numpy's tie rule, as lec_diag.hip), the new centre.  O(window points) per step.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/lec_hip.h"
#include "lec_internal.h"
#include "lec_zeta.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr long long kLdsLimit = 160 * 1024;      // what one workgroup may declare on this part
constexpr int kLdsFixed = 64;                    // the waves' partial extrema, in front of the tile (keeps the tile 16-byte aligned)

struct FollowParams {
    const double* u; const double* v; const double* h;
    int nt, ny, nx;
    const double* xcoef;    // [ny][nx][3]
    const double* ycoef;    // [ny][3]
    const double* curv;     // [ny]
    int field, sense, r, sj, si;
    int jlo, jhi, ilo, ihi, j_start, i_start;
    int* pos; double* val; int* status;
};

__device__ __forceinline__ bool finite(double x) { return fabs(x) < __builtin_huge_val(); }

__device__ __forceinline__ double field_at(const FollowParams& p, const double* u, const double* v, const double* h, int j, int i) {
    return p.field == LEC_FOLLOW_HGT ? h[(size_t)j * p.nx + i] : zeta_at(p, u, v, j, i);
}

// the extremum of the whole workgroup, in every thread: wave64 shuffles, then the waves' partials through LDS.  The caller keeps a
// barrier between two calls (the tile's), so that no wave overwrites a partial another wave has yet to read.
__device__ __forceinline__ Best reduce_best(Best b, bool want_max, double* sv, int* sn) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(b.v, off);
        const int on = __shfl_down(b.n, off);
        if (want_max) b.take_max(ov, on); else b.take_min(ov, on);
    }
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) { sv[tid >> 6] = b.v; sn[tid >> 6] = b.n; }
    __syncthreads();
    Best r{sv[0], sn[0]};
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        if (want_max) r.take_max(sv[w], sn[w]); else r.take_min(sv[w], sn[w]);
    }
    return r;
}

// grid 1, block kThreads, dynamic LDS kLdsFixed + the tile
__global__ void __launch_bounds__(kThreads) lec_follow_kernel(const FollowParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* sv = (double*)smem;                     // [kWaves]
    int* sn = (int*)(smem + 8 * kWaves);            // [kWaves]
    double* tile = (double*)(smem + kLdsFixed);
    const int tid = threadIdx.x, r = p.r;
    const bool want_max = p.sense == LEC_FOLLOW_MAX;
    const size_t plane = (size_t)p.ny * p.nx;
    const double inf = __builtin_huge_val();
    const int none = 0x7fffffff;
    int jc = p.j_start, ic = p.i_start;             // the centre: the same in every thread, from the partials in LDS
    for (int t = 0; t < p.nt; ++t) {
        const double* u = p.u + t * plane;
        const double* v = p.v + t * plane;
        const double* h = p.h ? p.h + t * plane : nullptr;
        const bool whole = jc < 0;                  // step 0 without a start: every admissible centre
        const int j0 = whole ? p.jlo : max(p.jlo, jc - p.sj), j1 = whole ? p.jhi : min(p.jhi, jc + p.sj);
        const int i0 = whole ? p.ilo : max(p.ilo, ic - p.si), i1 = whole ? p.ihi : min(p.ihi, ic + p.si);
        const int nxw = i1 - i0 + 1, npt = nxw * (j1 - j0 + 1);
        Best b{want_max ? -inf : inf, none};
        if (whole) {
            // strided over all of A, the field straight from global memory (it happens once)
            for (int n = tid; n < npt; n += kThreads) {
                const int j = j0 + n / nxw, i = i0 + n % nxw;
                double sum = 0.0; int cnt = 0;
                for (int jj = max(j - r, 0); jj <= min(j + r, p.ny - 1); ++jj)
                    for (int ii = max(i - r, 0); ii <= min(i + r, p.nx - 1); ++ii) {
                        const double f = field_at(p, u, v, h, jj, ii);
                        if (finite(f)) { sum += f; ++cnt; }
                    }
                if (cnt) { const double s = sum / cnt; if (want_max) b.take_max(s, n); else b.take_min(s, n); }
            }
        } else {
            // (a) the field on the window grown by r (clipped to the slice), coalesced along longitude
            const int jt0 = max(j0 - r, 0), jt1 = min(j1 + r, p.ny - 1), it0 = max(i0 - r, 0), it1 = min(i1 + r, p.nx - 1);
            const int tw = it1 - it0 + 1, ntile = tw * (jt1 - jt0 + 1);
            for (int n = tid; n < ntile; n += kThreads) tile[n] = field_at(p, u, v, h, jt0 + n / tw, it0 + n % tw);
            __syncthreads();
            // (b) the mean of the finite neighbours, summed in row-major order; (c) this thread's extremum
            for (int n = tid; n < npt; n += kThreads) {
                const int j = j0 + n / nxw, i = i0 + n % nxw;
                double sum = 0.0; int cnt = 0;
                for (int jj = max(j - r, jt0); jj <= min(j + r, jt1); ++jj) {
                    const int base = (jj - jt0) * tw - it0;
                    for (int ii = max(i - r, it0); ii <= min(i + r, it1); ++ii) {
                        const double f = tile[base + ii];
                        if (finite(f)) { sum += f; ++cnt; }
                    }
                }
                if (cnt) { const double s = sum / cnt; if (want_max) b.take_max(s, n); else b.take_min(s, n); }
            }
        }
        b = reduce_best(b, want_max, sv, sn);
        const bool found = b.n != none;
        // (d) the next step's centre; a window without a finite value keeps the one it has
        if (found) { jc = j0 + b.n / nxw; ic = i0 + b.n % nxw; }
        else if (whole) { jc = p.jlo; ic = p.ilo; }
        if (tid == 0) {
            p.pos[2 * (size_t)t] = jc; p.pos[2 * (size_t)t + 1] = ic;
            p.val[t] = found ? b.v : nan("");
            p.status[t] = found ? 0 : 1;
        }
    }
}

}  // namespace

extern "C" int lec_follow(const lec_follow_args* a) {
    if (!a) return lec_set_error(LEC_ERR_ARG, "lec_follow: null args");
    const struct { const void* p; const char* name; } ptrs[] = {
        {a->u_d, "u_d"}, {a->v_d, "v_d"}, {a->xcoef_d, "xcoef_d"}, {a->ycoef_d, "ycoef_d"}, {a->curv_d, "curv_d"},
        {a->pos_d, "pos_d"}, {a->val_d, "val_d"}, {a->status_d, "status_d"}};
    for (const auto& q : ptrs)
        if (!q.p) {
            char msg[80];
            snprintf(msg, sizeof msg, "lec_follow: null pointer argument %s", q.name);
            return lec_set_error(LEC_ERR_ARG, msg);
        }
    if (a->nt < 1 || a->ny < 3 || a->nx < 3) return lec_set_error(LEC_ERR_ARG, "lec_follow: needs nt >= 1 and at least 3 x 3 grid points (nt, ny, nx)");
    if ((unsigned long long)a->ny * (unsigned long long)a->nx > 0x7fffffffULL) return lec_set_error(LEC_ERR_UNSUPPORTED, "lec_follow: slice too large (ny * nx)");
    if (a->field != LEC_FOLLOW_ZETA && a->field != LEC_FOLLOW_HGT) return lec_set_error(LEC_ERR_ARG, "lec_follow: field must be LEC_FOLLOW_ZETA or LEC_FOLLOW_HGT");
    if (a->sense != LEC_FOLLOW_MIN && a->sense != LEC_FOLLOW_MAX) return lec_set_error(LEC_ERR_ARG, "lec_follow: sense must be LEC_FOLLOW_MIN or LEC_FOLLOW_MAX");
    if (a->field == LEC_FOLLOW_HGT && !a->hgt_d) return lec_set_error(LEC_ERR_ARG, "lec_follow: field LEC_FOLLOW_HGT needs hgt_d");
    if (a->smooth_r < 0) return lec_set_error(LEC_ERR_ARG, "lec_follow: smooth_r must be >= 0");
    if (a->sj < 1 || a->si < 1) return lec_set_error(LEC_ERR_ARG, "lec_follow: sj and si must be >= 1");
    if (a->jlo < 0 || a->jlo > a->jhi || a->jhi >= a->ny) return lec_set_error(LEC_ERR_ARG, "lec_follow: needs 0 <= jlo <= jhi < ny");
    if (a->ilo < 0 || a->ilo > a->ihi || a->ihi >= a->nx) return lec_set_error(LEC_ERR_ARG, "lec_follow: needs 0 <= ilo <= ihi < nx");
    const bool no_start = a->j_start == -1 && a->i_start == -1;
    if (!no_start && (a->j_start < a->jlo || a->j_start > a->jhi || a->i_start < a->ilo || a->i_start > a->ihi))
        return lec_set_error(LEC_ERR_ARG, "lec_follow: j_start, i_start must be an admissible centre (jlo..jhi, ilo..ihi) or both -1");
    // the tile never outgrows the slice: a search radius beyond the domain is a window of the whole of A
    const long long th = (long long)a->ny < 2LL * a->sj + 1 + 2LL * a->smooth_r ? a->ny : 2LL * a->sj + 1 + 2LL * a->smooth_r;
    const long long tw = (long long)a->nx < 2LL * a->si + 1 + 2LL * a->smooth_r ? a->nx : 2LL * a->si + 1 + 2LL * a->smooth_r;
    const long long lds = kLdsFixed + 8 * th * tw;
    if (lds > kLdsLimit) {
        char msg[200];
        snprintf(msg, sizeof msg, "lec_follow: the LDS tile of sj, si, smooth_r is %lld x %lld doubles = %lld bytes, the limit is %lld bytes",
                 th, tw, 8 * th * tw, kLdsLimit - kLdsFixed);
        return lec_set_error(LEC_ERR_UNSUPPORTED, msg);
    }
    FollowParams p;
    p.u = a->u_d; p.v = a->v_d; p.h = a->hgt_d; p.nt = a->nt; p.ny = a->ny; p.nx = a->nx;
    p.xcoef = a->xcoef_d; p.ycoef = a->ycoef_d; p.curv = a->curv_d;
    p.field = a->field; p.sense = a->sense; p.r = a->smooth_r; p.sj = a->sj; p.si = a->si;
    p.jlo = a->jlo; p.jhi = a->jhi; p.ilo = a->ilo; p.ihi = a->ihi; p.j_start = a->j_start; p.i_start = a->i_start;
    p.pos = a->pos_d; p.val = a->val_d; p.status = a->status_d;
    hipStream_t st = (hipStream_t)a->stream;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)lec_follow_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(lec_follow_kernel, dim3(1), dim3(kThreads), (size_t)lds, st, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}
