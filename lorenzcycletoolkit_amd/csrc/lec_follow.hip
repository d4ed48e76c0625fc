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

// kRing, here and below: the ring calls' compile-time variant (include/lec_hip.h) -- column nx - 1 is the western neighbour of column 0.
// i is a ring column, 0 <= i < nx.  Done the way kMode is: the instantiations without it are the code they were.
template <bool kRing = false>
__device__ __forceinline__ double field_at(const FollowParams& p, const double* u, const double* v, const double* h, int j, int i) {
    if constexpr (kRing) return p.field == LEC_FOLLOW_HGT ? h[(size_t)j * p.nx + i] : zeta_ring_at(p, u, v, j, i);
    else return p.field == LEC_FOLLOW_HGT ? h[(size_t)j * p.nx + i] : zeta_at(p, u, v, j, i);
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

// S at one point straight from global memory: the mean of the finite field values within r, summed in row-major order.  False (and s
// untouched) where none is finite.  ONE function for lec_follow's first step without a start and for lec_follow_seeds: the same doubles.
// kRing: always 2 r + 1 columns, west to east from i - r on the ring (2 r + 1 <= nx: the host's check); the wrap is a compare.
template <bool kRing = false>
__device__ __forceinline__ bool smooth_global(const FollowParams& p, const double* u, const double* v, const double* h, int j, int i, double& s) {
    const int r = p.r;
    double sum = 0.0; int cnt = 0;
    if (kRing) {
        const int iw = i - r < 0 ? i - r + p.nx : i - r;
        for (int jj = max(j - r, 0); jj <= min(j + r, p.ny - 1); ++jj)
            for (int k = 0, ii = iw; k <= 2 * r; ++k) {
                const double f = field_at<true>(p, u, v, h, jj, ii);
                if (finite(f)) { sum += f; ++cnt; }
                if (++ii == p.nx) ii = 0;
            }
    } else {
        for (int jj = max(j - r, 0); jj <= min(j + r, p.ny - 1); ++jj)
            for (int ii = max(i - r, 0); ii <= min(i + r, p.nx - 1); ++ii) {
                const double f = field_at(p, u, v, h, jj, ii);
                if (finite(f)) { sum += f; ++cnt; }
            }
    }
    if (cnt) s = sum / cnt;
    return cnt != 0;
}

// lec_follow_spans' rule for one chain (include/lec_hip.h): born at step t0, ended by end_threshold and patience, span [2] its output.
// The resumed form (lec_follow_spans_chunk) adds what a chunk inherits: t0 is then the first LOCAL step the chain walks, t_base the
// series step of local step 0, weak / first / last the counters so far, state [8] where the chain leaves them for the next chunk.
struct SpanRule { int t0; double end_threshold; int patience; int* span; int t_base, weak, first, last; int* state; };

// follow_chain's compile-time variants
constexpr int kPlain = 0, kSpans = 1, kResume = 2;
// lec_follow_spans_chunk's phases (state[0])
constexpr int kUnborn = 0, kWalking = 1, kStopped = 2, kBadStart = 3;

// steps [t_begin, t_end) of a chain that does not walk them, by the whole workgroup
__device__ __forceinline__ void not_live(int* pos, double* val, int* status, int t_begin, int t_end) {
    for (int t = t_begin + (int)threadIdx.x; t < t_end; t += kThreads) {
        pos[2 * (size_t)t] = -1; pos[2 * (size_t)t + 1] = -1;
        val[t] = nan("");
        status[t] = LEC_FOLLOW_NOT_LIVE;
    }
}

// One chain, walked by one workgroup of kThreads: lec_follow_kernel's only one, lec_follow_many_kernel's chain blockIdx.x.  Nothing in
// here knows which: the same start gives the same positions, status and val bits in either kernel, whatever the other workgroups do.
// pos [nt][2], val [nt], status [nt]: this chain's; smem: kLdsFixed + the tile.
// kSpans (lec_follow_spans): the chain is born at step sp.t0 and ended by sp's rule (include/lec_hip.h); the steps it does not walk are
// LEC_FOLLOW_NOT_LIVE, span [2] gets (first good step, last good step).  The walked steps are the very statements of the other two.
// kResume (lec_follow_spans_chunk): kSpans on a chunk of the series -- the counters start from sp's, the good steps are counted in
// series steps (local step + sp.t_base), and the chain's state goes to sp.state at the end.
// kRing (kResume only): the window's columns ic - si .. ic + si are never cut, they run west to east on the ring; LDS tile column c is
// ring column (ic - si - r + c) mod nx, so a tile row is at most two contiguous runs of the slice's row and the lanes stay along
// longitude.  i0, i1, it0, it1 are UNWRAPPED columns (i0 may be negative, i1 beyond nx - 1): only the tile's load and the new centre
// wrap, each with a compare, and nothing in the mean's inner loop knows of the ring.  2 si + 1 + 2 r <= nx is the host's check.
template <int kMode, bool kRing = false>
__device__ __forceinline__ void follow_chain(const FollowParams& p, int jc, int ic, int* pos, double* val, int* status, char* smem,
                                             const SpanRule sp = SpanRule{}) {
    double* sv = (double*)smem;                     // [kWaves]
    int* sn = (int*)(smem + 8 * kWaves);            // [kWaves]
    double* tile = (double*)(smem + kLdsFixed);
    const int tid = threadIdx.x, r = p.r;
    const bool want_max = p.sense == LEC_FOLLOW_MAX;
    const size_t plane = (size_t)p.ny * p.nx;
    const double inf = __builtin_huge_val();
    const int none = 0x7fffffff;
    int first = -1, last = -1, weak = 0;            // (kSpans) the good steps so far, the not-good steps in a row
    if (kMode == kResume) { first = sp.first; last = sp.last; weak = sp.weak; }
    const int tb = kMode == kResume ? sp.t_base : 0;
    bool stopped = false;                           // (kResume)
    if (kMode != kPlain) not_live(pos, val, status, 0, sp.t0);
    // (jc, ic) the centre: the same in every thread, from the partials in LDS
    for (int t = kMode != kPlain ? sp.t0 : 0; t < p.nt; ++t) {
        const double* u = p.u + t * plane;
        const double* v = p.v + t * plane;
        const double* h = p.h ? p.h + t * plane : nullptr;
        const bool whole = kMode == kPlain && jc < 0;      // step 0 without a start: every admissible centre
        const int j0 = whole ? p.jlo : max(p.jlo, jc - p.sj), j1 = whole ? p.jhi : min(p.jhi, jc + p.sj);
        const int i0 = kRing ? ic - p.si : whole ? p.ilo : max(p.ilo, ic - p.si), i1 = kRing ? ic + p.si : whole ? p.ihi : min(p.ihi, ic + p.si);
        const int nxw = i1 - i0 + 1, npt = nxw * (j1 - j0 + 1);
        Best b{want_max ? -inf : inf, none};
        if (whole) {
            // strided over all of A, the field straight from global memory (it happens once)
            for (int n = tid; n < npt; n += kThreads) {
                double s;
                if (smooth_global(p, u, v, h, j0 + n / nxw, i0 + n % nxw, s)) { if (want_max) b.take_max(s, n); else b.take_min(s, n); }
            }
        } else {
            // (a) the field on the window grown by r (clipped to the slice), coalesced along longitude
            const int jt0 = max(j0 - r, 0), jt1 = min(j1 + r, p.ny - 1);
            const int it0 = kRing ? i0 - r : max(i0 - r, 0), it1 = kRing ? i1 + r : min(i1 + r, p.nx - 1);
            const int tw = it1 - it0 + 1, ntile = tw * (jt1 - jt0 + 1);
            for (int n = tid; n < ntile; n += kThreads) {
                if (kRing) {
                    int i = it0 + n % tw;                       // -nx < i < 2 nx
                    i = i < 0 ? i + p.nx : i >= p.nx ? i - p.nx : i;
                    tile[n] = field_at<true>(p, u, v, h, jt0 + n / tw, i);
                } else {
                    tile[n] = field_at(p, u, v, h, jt0 + n / tw, it0 + n % tw);
                }
            }
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
        if (found) {
            jc = j0 + b.n / nxw; ic = i0 + b.n % nxw;
            if (kRing) ic = ic < 0 ? ic + p.nx : ic >= p.nx ? ic - p.nx : ic;
        }
        else if (whole) { jc = p.jlo; ic = p.ilo; }
        if (tid == 0) {
            pos[2 * (size_t)t] = jc; pos[2 * (size_t)t + 1] = ic;
            val[t] = found ? b.v : nan("");
            status[t] = found ? 0 : 1;
        }
        if (kMode != kPlain) {
            // b is reduce_best's result, which every thread holds: the exit is uniform and lies after the step's barriers
            const bool good = found && (sp.end_threshold != sp.end_threshold || (want_max ? b.v >= sp.end_threshold : b.v <= sp.end_threshold));
            if (good) { if (first < 0) first = t + tb; last = t + tb; weak = 0; }
            else if (++weak == sp.patience) { not_live(pos, val, status, t + 1, p.nt); stopped = true; break; }
        }
    }
    if (kMode != kPlain && tid == 0) { sp.span[0] = first; sp.span[1] = last; }
    if (kMode == kResume && tid == 0) {
        sp.state[0] = stopped ? kStopped : kWalking; sp.state[1] = jc; sp.state[2] = ic; sp.state[3] = weak; sp.state[4] = first; sp.state[5] = last;
        sp.state[6] = 0; sp.state[7] = 0;
    }
}

// grid 1, block kThreads, dynamic LDS kLdsFixed + the tile
__global__ void __launch_bounds__(kThreads) lec_follow_kernel(const FollowParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    follow_chain<kPlain>(p, p.j_start, p.i_start, p.pos, p.val, p.status, smem);
}

// grid n_chains, block kThreads, dynamic LDS as lec_follow_kernel: workgroup c walks chain c from start[c].  The table lives in device
// memory, so the kernel checks its entry before it reads anything else: (-1, -1) is lec_follow's "no start", anything else outside
// the admissible centres makes the chain LEC_FOLLOW_BAD_START at every step.  (p.j_start, p.i_start are not used.)
__global__ void __launch_bounds__(kThreads) lec_follow_many_kernel(const FollowParams p, const int* __restrict__ start) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t c = blockIdx.x;
    const int js = start[2 * c], is = start[2 * c + 1];
    int* pos = p.pos + 2 * c * (size_t)p.nt;
    double* val = p.val + c * (size_t)p.nt;
    int* status = p.status + c * (size_t)p.nt;
    const bool no_start = js == -1 && is == -1;
    if (!no_start && (js < p.jlo || js > p.jhi || is < p.ilo || is > p.ihi)) {
        for (int t = threadIdx.x; t < p.nt; t += kThreads) {
            pos[2 * (size_t)t] = -1; pos[2 * (size_t)t + 1] = -1;
            val[t] = nan("");
            status[t] = LEC_FOLLOW_BAD_START;
        }
        return;
    }
    follow_chain<kPlain>(p, js, is, pos, val, status, smem);
}

// grid n_chains, block kThreads, dynamic LDS as lec_follow_kernel: workgroup c walks chain c from start[c] = (t0, j, i) until the rule
// ends it, and returns.  The entry is checked before anything else is read; (-1, -1) is no start here.
__global__ void __launch_bounds__(kThreads) lec_follow_spans_kernel(const FollowParams p, const int* __restrict__ start, double end_threshold,
                                                                    int patience, int* __restrict__ span) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t c = blockIdx.x;
    const int t0 = start[3 * c], js = start[3 * c + 1], is = start[3 * c + 2];
    int* pos = p.pos + 2 * c * (size_t)p.nt;
    double* val = p.val + c * (size_t)p.nt;
    int* status = p.status + c * (size_t)p.nt;
    if (t0 < 0 || t0 >= p.nt || js < p.jlo || js > p.jhi || is < p.ilo || is > p.ihi) {
        for (int t = threadIdx.x; t < p.nt; t += kThreads) {
            pos[2 * (size_t)t] = -1; pos[2 * (size_t)t + 1] = -1;
            val[t] = nan("");
            status[t] = LEC_FOLLOW_BAD_START;
        }
        if (threadIdx.x == 0) { span[2 * c] = -1; span[2 * c + 1] = -1; }
        return;
    }
    follow_chain<kSpans>(p, js, is, pos, val, status, smem, SpanRule{t0, end_threshold, patience, span + 2 * c, 0, 0, -1, -1, nullptr});
}

// grid n_chains, block kThreads, dynamic LDS as lec_follow_kernel: workgroup c walks the steps of THIS chunk that chain c lives in, from
// the state the chunk before left (include/lec_hip.h has the rule).  p.nt counts the chunk's steps, t_base is the series step of its
// slice 0.  The start entry is checked before anything else is read.  The state is read by thread 0 alone and reaches the others through
// LDS (the tile's first bytes, free until the first step fills it: the tile holds 3 x 3 doubles at the least), so the phase and with it
// every exit is uniform.  A walking chain whose carried centre is no admissible centre -- a state the caller has not passed on
// unchanged -- reads nothing: it is treated as stopped.
__global__ void __launch_bounds__(kThreads) lec_follow_spans_chunk_kernel(const FollowParams p, const int* __restrict__ start, double end_threshold,
                                                                          int patience, int* __restrict__ span, int t_base, int* state_all) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t c = blockIdx.x;
    const int tid = threadIdx.x;
    const int t0 = start[3 * c], js = start[3 * c + 1], is = start[3 * c + 2];
    int* pos = p.pos + 2 * c * (size_t)p.nt;
    double* val = p.val + c * (size_t)p.nt;
    int* status = p.status + c * (size_t)p.nt;
    int* state = state_all + 8 * c;
    if (t0 < 0 || js < p.jlo || js > p.jhi || is < p.ilo || is > p.ihi) {
        for (int t = tid; t < p.nt; t += kThreads) {
            pos[2 * (size_t)t] = -1; pos[2 * (size_t)t + 1] = -1;
            val[t] = nan("");
            status[t] = LEC_FOLLOW_BAD_START;
        }
        if (tid == 0) {
            span[2 * c] = -1; span[2 * c + 1] = -1;
            state[0] = kBadStart; state[1] = -1; state[2] = -1; state[3] = 0; state[4] = -1; state[5] = -1; state[6] = 0; state[7] = 0;
        }
        return;
    }
    int* sh = (int*)(smem + kLdsFixed);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) sh[k] = state[k];
    }
    __syncthreads();
    const int phase = sh[0], jc = sh[1], ic = sh[2], weak = sh[3], first = sh[4], last = sh[5];
    __syncthreads();                                // (the tile is free again)
    const long long born_at = (long long)t0 - t_base;                 // the local step of the birth
    const bool born = phase == kUnborn && born_at >= 0 && born_at < p.nt;
    const bool walks = phase == kWalking && jc >= p.jlo && jc <= p.jhi && ic >= p.ilo && ic <= p.ihi;
    if (!born && !walks) {
        // not yet born (the state stays as it is), stopped, or a state that is none of the rule's: no step of this chunk is walked
        not_live(pos, val, status, 0, p.nt);
        const bool has_span = phase == kStopped || phase == kWalking;
        if (tid == 0) { span[2 * c] = has_span ? first : -1; span[2 * c + 1] = has_span ? last : -1; }
        return;
    }
    // born here: from the table's start with fresh counters; walking: from the state's centre with its counters
    follow_chain<kResume>(p, born ? js : jc, born ? is : ic, pos, val, status, smem,
                          SpanRule{born ? (int)born_at : 0, end_threshold, patience, span + 2 * c, t_base, born ? 0 : weak, born ? -1 : first,
                                   born ? -1 : last, state});
}

// lec_follow_spans_chunk_ring: the kernel above, statement for statement, around the chain's ring variant.  (A copy, not a shared
// body: with the entry checks in a function of their own the existing kernel no longer compiled to the instructions it had.)  ilo = 0
// and ihi = nx - 1 here (the host's check): every column is a centre, and a carried ic outside [0, nx) counts as stopped.
__global__ void __launch_bounds__(kThreads) lec_follow_spans_chunk_ring_kernel(const FollowParams p, const int* __restrict__ start, double end_threshold,
                                                                               int patience, int* __restrict__ span, int t_base, int* state_all) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t c = blockIdx.x;
    const int tid = threadIdx.x;
    const int t0 = start[3 * c], js = start[3 * c + 1], is = start[3 * c + 2];
    int* pos = p.pos + 2 * c * (size_t)p.nt;
    double* val = p.val + c * (size_t)p.nt;
    int* status = p.status + c * (size_t)p.nt;
    int* state = state_all + 8 * c;
    if (t0 < 0 || js < p.jlo || js > p.jhi || is < p.ilo || is > p.ihi) {
        for (int t = tid; t < p.nt; t += kThreads) {
            pos[2 * (size_t)t] = -1; pos[2 * (size_t)t + 1] = -1;
            val[t] = nan("");
            status[t] = LEC_FOLLOW_BAD_START;
        }
        if (tid == 0) {
            span[2 * c] = -1; span[2 * c + 1] = -1;
            state[0] = kBadStart; state[1] = -1; state[2] = -1; state[3] = 0; state[4] = -1; state[5] = -1; state[6] = 0; state[7] = 0;
        }
        return;
    }
    int* sh = (int*)(smem + kLdsFixed);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) sh[k] = state[k];
    }
    __syncthreads();
    const int phase = sh[0], jc = sh[1], ic = sh[2], weak = sh[3], first = sh[4], last = sh[5];
    __syncthreads();                                // (the tile is free again)
    const long long born_at = (long long)t0 - t_base;                 // the local step of the birth
    const bool born = phase == kUnborn && born_at >= 0 && born_at < p.nt;
    const bool walks = phase == kWalking && jc >= p.jlo && jc <= p.jhi && ic >= p.ilo && ic <= p.ihi;
    if (!born && !walks) {
        // not yet born (the state stays as it is), stopped, or a state that is none of the rule's: no step of this chunk is walked
        not_live(pos, val, status, 0, p.nt);
        const bool has_span = phase == kStopped || phase == kWalking;
        if (tid == 0) { span[2 * c] = has_span ? first : -1; span[2 * c + 1] = has_span ? last : -1; }
        return;
    }
    // born here: from the table's start with fresh counters; walking: from the state's centre with its counters
    follow_chain<kResume, true>(p, born ? js : jc, born ? is : ic, pos, val, status, smem,
                                SpanRule{born ? (int)born_at : 0, end_threshold, patience, span + 2 * c, t_base, born ? 0 : weak, born ? -1 : first,
                                         born ? -1 : last, state});
}

// ---- lec_follow_seeds: the systems of ONE slice (the rule: include/lec_hip.h) ----------------------------------------------------
struct SeedParams {
    FollowParams f;             // one slice: nt = 1; the field, the tables, r, the admissible bounds
    int ej, ei, k_max;
    double threshold;           // NaN: none
    double* work;               // [ny][nx]
    int* seed_pos; double* seed_val; int* n_found;
};

// The three phases as device functions of ONE slice's SeedParams: lec_follow_seeds' kernels run them on the slice, lec_follow_seeds_series'
// on slice t of a series (at()), so that step t's seeds are lec_follow_seeds' on that slice by construction.

// (a) S of the whole slice -> work; NaN where S is not finite.  One thread per point, row-major: the lanes run along longitude.
template <bool kRing = false>
__device__ __forceinline__ void seeds_smooth(const SeedParams& q, unsigned n) {
    const FollowParams& p = q.f;
    double s;
    const bool any = smooth_global<kRing>(p, p.u, p.v, p.h, n / p.nx, n % p.nx, s);
    q.work[n] = any && finite(s) ? s : nan("");
}

__global__ void __launch_bounds__(kThreads) lec_seeds_smooth_kernel(const SeedParams q) {
    const unsigned n = blockIdx.x * kThreads + threadIdx.x;          // (ny * nx < 2^31: no wrap)
    if (n >= (unsigned)(q.f.ny * q.f.nx)) return;
    seeds_smooth(q, n);
}

// (b) the candidate test, one thread per admissible centre, the neighbourhood from work.  A CANDIDATE overwrites its own S with the
// sentinel "better than any finite value" (-inf for the minimum, +inf for the maximum); nothing else is written.  Other workgroups may
// read that point before or after: it does not change their answer.  A point R that has the candidate P in its neighbourhood lies in
// P's (the neighbourhood is symmetric), so S(R) is worse than S(P), or equal and later in row-major order: R fails its test on P's true
// value and on the sentinel alike.  (Marking NON-candidates in place would not be safe: a point could lose the very neighbour that
// disqualifies it.)  Every thread reads its own S before it may write it.  8-byte relaxed atomics: a reader sees the old or the new double.
// kRing: the neighbourhood's columns are the 2 ei + 1 within ring distance ei (2 ei + 1 <= nx: the host's check), and "before" keeps the
// slice's absolute row-major index -- a tie is the one thing that depends on where the seam lies.
template <bool kRing = false>
__device__ __forceinline__ void seeds_candidate(const SeedParams& q, unsigned n) {
    const FollowParams& p = q.f;
    const int nxa = p.ihi - p.ilo + 1;
    const int j = p.jlo + n / nxa, i = p.ilo + n % nxa;
    const bool want_max = p.sense == LEC_FOLLOW_MAX;
    const double inf = __builtin_huge_val();
    const double s = __hip_atomic_load(q.work + (size_t)j * p.nx + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!finite(s)) return;
    if (q.threshold == q.threshold && (want_max ? s < q.threshold : s > q.threshold)) return;
    if (kRing) {
        const int iw = i - q.ei < 0 ? i - q.ei + p.nx : i - q.ei;
        for (int jj = max(j - q.ej, 0); jj <= min(j + q.ej, p.ny - 1); ++jj) {
            const double* row = q.work + (size_t)jj * p.nx;
            for (int k = 0, ii = iw; k <= 2 * q.ei; ++k) {
                const double o = __hip_atomic_load(row + ii, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool before = jj < j || (jj == j && ii < i);
                const bool self = jj == j && ii == i;
                if (++ii == p.nx) ii = 0;
                if (o != o || self) continue;
                if (want_max ? (o > s || (o == s && before)) : (o < s || (o == s && before))) return;
            }
        }
    } else {
        for (int jj = max(j - q.ej, 0); jj <= min(j + q.ej, p.ny - 1); ++jj) {
            const double* row = q.work + (size_t)jj * p.nx;
            for (int ii = max(i - q.ei, 0); ii <= min(i + q.ei, p.nx - 1); ++ii) {
                const double o = __hip_atomic_load(row + ii, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (o != o || (jj == j && ii == i)) continue;
                const bool before = jj < j || (jj == j && ii < i);
                if (want_max ? (o > s || (o == s && before)) : (o < s || (o == s && before))) return;
            }
        }
    }
    __hip_atomic_store(q.work + (size_t)j * p.nx + i, want_max ? inf : -inf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kThreads) lec_seeds_candidate_kernel(const SeedParams q) {
    const int na = (q.f.ihi - q.f.ilo + 1) * (q.f.jhi - q.f.jlo + 1);
    const unsigned n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= (unsigned)na) return;
    seeds_candidate(q, n);
}

// (c) ONE workgroup.  First the admissible centres of work become what the selection reads: a candidate gets its S back (smooth_global
// again: the double of phase (a)), everything else NaN.  Then k_max times: the best remaining candidate -- key: the value, then the
// slice's row-major index, through reduce_best -- is written out and struck by the thread that scans it.
template <bool kRing = false>
__device__ __forceinline__ void seeds_select(const SeedParams& q, double* sv, int* sn) {
    const FollowParams& p = q.f;
    const int tid = threadIdx.x;
    const int nxa = p.ihi - p.ilo + 1, na = nxa * (p.jhi - p.jlo + 1);
    const bool want_max = p.sense == LEC_FOLLOW_MAX;
    const double inf = __builtin_huge_val();
    const int none = 0x7fffffff;
    for (int n = tid; n < na; n += kThreads) {
        const int j = p.jlo + n / nxa, i = p.ilo + n % nxa;
        double* w = q.work + (size_t)j * p.nx + i;
        double s = nan("");
        if (*w == (want_max ? inf : -inf)) smooth_global<kRing>(p, p.u, p.v, p.h, j, i, s);
        *w = s;
    }
    int found = 0;
    for (int k = 0; k < q.k_max; ++k) {
        Best b{want_max ? -inf : inf, none};
        for (int n = tid; n < na; n += kThreads) {          // (each thread re-reads the points it wrote itself: no fence needed)
            const int m = (p.jlo + n / nxa) * p.nx + p.ilo + n % nxa;
            const double s = q.work[m];
            if (s == s) { if (want_max) b.take_max(s, m); else b.take_min(s, m); }
        }
        b = reduce_best(b, want_max, sv, sn);
        __syncthreads();                                    // the partials are read: the next round may overwrite them
        if (b.n == none) break;                             // (the same in every thread)
        const int j = b.n / p.nx, i = b.n % p.nx;
        if (((j - p.jlo) * nxa + (i - p.ilo)) % kThreads == tid) q.work[b.n] = nan("");
        if (tid == 0) { q.seed_pos[2 * k] = j; q.seed_pos[2 * k + 1] = i; q.seed_val[k] = b.v; }
        ++found;
    }
    for (int k = found + tid; k < q.k_max; k += kThreads) { q.seed_pos[2 * k] = -2; q.seed_pos[2 * k + 1] = -2; q.seed_val[k] = nan(""); }
    if (tid == 0) *q.n_found = found;
}

__global__ void __launch_bounds__(kThreads) lec_seeds_select_kernel(const SeedParams q) {
    __shared__ double sv[kWaves];
    __shared__ int sn[kWaves];
    seeds_select(q, sv, sn);
}

// ---- lec_follow_seeds_series: the three phases over (point, step); every index that runs over the series has 64 bits, and the grids are
// capped and strided over, so that no grid dimension bounds nt --------------------------------------------------------------------------
constexpr unsigned kSeriesGrid = 1u << 16;      // workgroups per launch at the most: each strides over the rest

// q: slice 0 of the series; -> slice t
__device__ __forceinline__ SeedParams at(const SeedParams& q, size_t t) {
    SeedParams s = q;
    const size_t off = t * ((size_t)q.f.ny * q.f.nx);
    s.f.u += off; s.f.v += off;
    if (s.f.h) s.f.h += off;
    s.work += off;
    s.seed_pos += 2 * t * (size_t)q.k_max; s.seed_val += t * (size_t)q.k_max; s.n_found += t;
    return s;
}

__global__ void __launch_bounds__(kThreads) lec_seeds_series_smooth_kernel(const SeedParams q, int nt) {
    const unsigned long long plane = (unsigned long long)q.f.ny * q.f.nx, total = plane * nt;
    for (unsigned long long m = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; m < total; m += (unsigned long long)gridDim.x * kThreads)
        seeds_smooth(at(q, m / plane), (unsigned)(m % plane));
}

__global__ void __launch_bounds__(kThreads) lec_seeds_series_candidate_kernel(const SeedParams q, int nt) {
    const unsigned long long na = (unsigned long long)(q.f.ihi - q.f.ilo + 1) * (q.f.jhi - q.f.jlo + 1), total = na * nt;
    for (unsigned long long m = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; m < total; m += (unsigned long long)gridDim.x * kThreads)
        seeds_candidate(at(q, m / na), (unsigned)(m % na));
}

// one workgroup per step (strided).  t and its bound are the same in every thread of the workgroup: the barriers inside stay uniform.
__global__ void __launch_bounds__(kThreads) lec_seeds_series_select_kernel(const SeedParams q, int nt) {
    __shared__ double sv[kWaves];
    __shared__ int sn[kWaves];
    for (long long t = blockIdx.x; t < nt; t += gridDim.x) {
        seeds_select(at(q, (size_t)t), sv, sn);
        __syncthreads();                                    // (the partials are free again before the next step's first round)
    }
}

// lec_follow_seeds_series_ring: the three kernels above with the ring variants of the phases
__global__ void __launch_bounds__(kThreads) lec_seeds_series_smooth_ring_kernel(const SeedParams q, int nt) {
    const unsigned long long plane = (unsigned long long)q.f.ny * q.f.nx, total = plane * nt;
    for (unsigned long long m = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; m < total; m += (unsigned long long)gridDim.x * kThreads)
        seeds_smooth<true>(at(q, m / plane), (unsigned)(m % plane));
}

__global__ void __launch_bounds__(kThreads) lec_seeds_series_candidate_ring_kernel(const SeedParams q, int nt) {
    const unsigned long long na = (unsigned long long)(q.f.ihi - q.f.ilo + 1) * (q.f.jhi - q.f.jlo + 1), total = na * nt;
    for (unsigned long long m = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; m < total; m += (unsigned long long)gridDim.x * kThreads)
        seeds_candidate<true>(at(q, m / na), (unsigned)(m % na));
}

__global__ void __launch_bounds__(kThreads) lec_seeds_series_select_ring_kernel(const SeedParams q, int nt) {
    __shared__ double sv[kWaves];
    __shared__ int sn[kWaves];
    for (long long t = blockIdx.x; t < nt; t += gridDim.x) {
        seeds_select<true>(at(q, (size_t)t), sv, sn);
        __syncthreads();
    }
}

}  // namespace

namespace {

int refuse(int code, const char* who, const char* what) {
    char msg[240];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return lec_set_error(code, msg);
}

struct NamedPtr { const void* p; const char* name; };

template <size_t N>
int check_pointers(const char* who, const NamedPtr (&ptrs)[N]) {
    for (const auto& q : ptrs)
        if (!q.p) {
            char msg[80];
            snprintf(msg, sizeof msg, "null pointer argument %s", q.name);
            return refuse(LEC_ERR_ARG, who, msg);
        }
    return LEC_OK;
}

// what the three calls share: the slice, the field and its sense, the smoothing radius, the admissible centres (nt = 1 for one slice)
template <class A>
int check_slice(const char* who, const A* a, int nt) {
    if (nt < 1 || a->ny < 3 || a->nx < 3) return refuse(LEC_ERR_ARG, who, "needs nt >= 1 and at least 3 x 3 grid points (nt, ny, nx)");
    if ((unsigned long long)a->ny * (unsigned long long)a->nx > 0x7fffffffULL) return refuse(LEC_ERR_UNSUPPORTED, who, "slice too large (ny * nx)");
    if (a->field != LEC_FOLLOW_ZETA && a->field != LEC_FOLLOW_HGT) return refuse(LEC_ERR_ARG, who, "field must be LEC_FOLLOW_ZETA or LEC_FOLLOW_HGT");
    if (a->sense != LEC_FOLLOW_MIN && a->sense != LEC_FOLLOW_MAX) return refuse(LEC_ERR_ARG, who, "sense must be LEC_FOLLOW_MIN or LEC_FOLLOW_MAX");
    if (a->field == LEC_FOLLOW_HGT && !a->hgt_d) return refuse(LEC_ERR_ARG, who, "field LEC_FOLLOW_HGT needs hgt_d");
    if (a->smooth_r < 0) return refuse(LEC_ERR_ARG, who, "smooth_r must be >= 0");
    if (a->jlo < 0 || a->jlo > a->jhi || a->jhi >= a->ny) return refuse(LEC_ERR_ARG, who, "needs 0 <= jlo <= jhi < ny");
    if (a->ilo < 0 || a->ilo > a->ihi || a->ihi >= a->nx) return refuse(LEC_ERR_ARG, who, "needs 0 <= ilo <= ihi < nx");
    return LEC_OK;
}

// the chain's window: sj, si and the dynamic LDS of its tile (-> lds), refused beyond what one workgroup may declare
template <class A>
int check_window(const char* who, const A* a, long long* lds) {
    if (a->sj < 1 || a->si < 1) return refuse(LEC_ERR_ARG, who, "sj and si must be >= 1");
    // the tile never outgrows the slice: a search radius beyond the domain is a window of the whole of A
    const long long th = (long long)a->ny < 2LL * a->sj + 1 + 2LL * a->smooth_r ? a->ny : 2LL * a->sj + 1 + 2LL * a->smooth_r;
    const long long tw = (long long)a->nx < 2LL * a->si + 1 + 2LL * a->smooth_r ? a->nx : 2LL * a->si + 1 + 2LL * a->smooth_r;
    *lds = kLdsFixed + 8 * th * tw;
    if (*lds > kLdsLimit) {
        char msg[200];
        snprintf(msg, sizeof msg, "the LDS tile of sj, si, smooth_r is %lld x %lld doubles = %lld bytes, the limit is %lld bytes",
                 th, tw, 8 * th * tw, kLdsLimit - kLdsFixed);
        return refuse(LEC_ERR_UNSUPPORTED, who, msg);
    }
    return LEC_OK;
}

template <class A>
FollowParams slice_params(const A* a, int nt) {
    FollowParams p{};
    p.u = a->u_d; p.v = a->v_d; p.h = a->hgt_d; p.nt = nt; p.ny = a->ny; p.nx = a->nx;
    p.xcoef = a->xcoef_d; p.ycoef = a->ycoef_d; p.curv = a->curv_d;
    p.field = a->field; p.sense = a->sense; p.r = a->smooth_r;
    p.jlo = a->jlo; p.jhi = a->jhi; p.ilo = a->ilo; p.ihi = a->ihi; p.j_start = -1; p.i_start = -1;
    return p;
}

// what the ring calls ask on top: every column is an admissible centre, and the columns a point reads (`reach`: the tile's
// 2 si + 1 + 2 smooth_r, a seed's 2 ei + 1 or 2 smooth_r + 1) do not meet themselves on the ring.  Refused, never clamped.
template <class A>
int check_ring(const char* who, const A* a, long long reach, const char* what) {
    if (a->ilo != 0 || a->ihi != a->nx - 1) return refuse(LEC_ERR_ARG, who, "on a ring every column is an admissible centre: needs ilo = 0 and ihi = nx - 1");
    if (reach > a->nx) {
        char msg[200];
        snprintf(msg, sizeof msg, "%s = %lld columns exceed nx = %d: on a ring the window would meet itself", what, reach, a->nx);
        return refuse(LEC_ERR_ARG, who, msg);
    }
    return LEC_OK;
}

int launched(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return refuse(LEC_ERR_LAUNCH, who, hipGetErrorString(e));
    return LEC_OK;
}

}  // namespace

extern "C" int lec_follow(const lec_follow_args* a) {
    const char* who = "lec_follow";
    if (!a) return refuse(LEC_ERR_ARG, who, "null args");
    const NamedPtr ptrs[] = {{a->u_d, "u_d"}, {a->v_d, "v_d"}, {a->xcoef_d, "xcoef_d"}, {a->ycoef_d, "ycoef_d"}, {a->curv_d, "curv_d"},
                             {a->pos_d, "pos_d"}, {a->val_d, "val_d"}, {a->status_d, "status_d"}};
    if (int rc = check_pointers(who, ptrs)) return rc;
    if (int rc = check_slice(who, a, a->nt)) return rc;
    if (a->sj < 1 || a->si < 1) return refuse(LEC_ERR_ARG, who, "sj and si must be >= 1");
    const bool no_start = a->j_start == -1 && a->i_start == -1;
    if (!no_start && (a->j_start < a->jlo || a->j_start > a->jhi || a->i_start < a->ilo || a->i_start > a->ihi))
        return refuse(LEC_ERR_ARG, who, "j_start, i_start must be an admissible centre (jlo..jhi, ilo..ihi) or both -1");
    long long lds;
    if (int rc = check_window(who, a, &lds)) return rc;
    FollowParams p = slice_params(a, a->nt);
    p.sj = a->sj; p.si = a->si; p.j_start = a->j_start; p.i_start = a->i_start;
    p.pos = a->pos_d; p.val = a->val_d; p.status = a->status_d;
    hipStream_t st = (hipStream_t)a->stream;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)lec_follow_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return refuse(LEC_ERR_LAUNCH, who, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(lec_follow_kernel, dim3(1), dim3(kThreads), (size_t)lds, st, p);
    return launched(who);
}

extern "C" int lec_follow_many(const lec_follow_many_args* a) {
    const char* who = "lec_follow_many";
    if (!a) return refuse(LEC_ERR_ARG, who, "null args");
    const NamedPtr ptrs[] = {{a->u_d, "u_d"}, {a->v_d, "v_d"}, {a->xcoef_d, "xcoef_d"}, {a->ycoef_d, "ycoef_d"}, {a->curv_d, "curv_d"},
                             {a->start_d, "start_d"}, {a->pos_d, "pos_d"}, {a->val_d, "val_d"}, {a->status_d, "status_d"}};
    if (int rc = check_pointers(who, ptrs)) return rc;
    if (int rc = check_slice(who, a, a->nt)) return rc;
    if (a->n_chains < 1) return refuse(LEC_ERR_ARG, who, "n_chains must be >= 1");
    long long lds;
    if (int rc = check_window(who, a, &lds)) return rc;
    FollowParams p = slice_params(a, a->nt);
    p.sj = a->sj; p.si = a->si;
    p.pos = a->pos_d; p.val = a->val_d; p.status = a->status_d;
    hipStream_t st = (hipStream_t)a->stream;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)lec_follow_many_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return refuse(LEC_ERR_LAUNCH, who, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(lec_follow_many_kernel, dim3(a->n_chains), dim3(kThreads), (size_t)lds, st, p, a->start_d);
    return launched(who);
}

namespace {

// what lec_follow_seeds and lec_follow_seeds_series share: the checks (nt = 1 for the one slice) and the kernels' parameters of slice 0
template <class A>
int seed_params(const char* who, const A* a, int nt, SeedParams* out) {
    const NamedPtr ptrs[] = {{a->u_d, "u_d"}, {a->v_d, "v_d"}, {a->xcoef_d, "xcoef_d"}, {a->ycoef_d, "ycoef_d"}, {a->curv_d, "curv_d"},
                             {a->work_d, "work_d"}, {a->seed_pos_d, "seed_pos_d"}, {a->seed_val_d, "seed_val_d"}, {a->n_found_d, "n_found_d"}};
    if (int rc = check_pointers(who, ptrs)) return rc;
    if (int rc = check_slice(who, a, nt)) return rc;
    if (a->ej < 1 || a->ei < 1) return refuse(LEC_ERR_ARG, who, "ej and ei must be >= 1");
    if (a->k_max < 1 || a->k_max > 256) return refuse(LEC_ERR_ARG, who, "k_max must be 1..256");
    SeedParams q{};
    q.f = slice_params(a, 1);
    // a neighbourhood that reaches beyond the slice is the slice: the same points, and j + ej cannot overflow
    q.ej = a->ej < a->ny ? a->ej : a->ny; q.ei = a->ei < a->nx ? a->ei : a->nx; q.k_max = a->k_max;
    if (q.f.r > (a->ny > a->nx ? a->ny : a->nx)) q.f.r = a->ny > a->nx ? a->ny : a->nx;      // likewise the smoothing radius
    q.threshold = a->threshold;
    q.work = a->work_d; q.seed_pos = a->seed_pos_d; q.seed_val = a->seed_val_d; q.n_found = a->n_found_d;
    *out = q;
    return LEC_OK;
}

}  // namespace

extern "C" int lec_follow_seeds(const lec_follow_seeds_args* a) {
    const char* who = "lec_follow_seeds";
    if (!a) return refuse(LEC_ERR_ARG, who, "null args");
    SeedParams q;
    if (int rc = seed_params(who, a, 1, &q)) return rc;
    hipStream_t st = (hipStream_t)a->stream;
    const long long n_all = (long long)a->ny * a->nx, n_adm = (long long)(a->jhi - a->jlo + 1) * (a->ihi - a->ilo + 1);
    hipLaunchKernelGGL(lec_seeds_smooth_kernel, dim3((unsigned)((n_all + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, q);
    hipLaunchKernelGGL(lec_seeds_candidate_kernel, dim3((unsigned)((n_adm + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, q);
    hipLaunchKernelGGL(lec_seeds_select_kernel, dim3(1), dim3(kThreads), 0, st, q);
    return launched(who);
}

namespace {

int seeds_series(const lec_follow_seeds_series_args* a, const char* who, bool ring) {
    if (!a) return refuse(LEC_ERR_ARG, who, "null args");
    SeedParams q;
    if (int rc = seed_params(who, a, a->nt, &q)) return rc;
    if (ring) {
        if (int rc = check_ring(who, a, 2LL * a->ei + 1, "2 ei + 1")) return rc;
        if (int rc = check_ring(who, a, 2LL * a->smooth_r + 1, "2 smooth_r + 1")) return rc;
    }
    // nt * ny * nx doubles: the byte offsets into the series must fit 64 bits with room to spare
    const unsigned long long plane = (unsigned long long)a->ny * (unsigned long long)a->nx;
    if ((unsigned long long)a->nt > (1ULL << 59) / plane) return refuse(LEC_ERR_UNSUPPORTED, who, "series too large (nt * ny * nx)");
    hipStream_t st = (hipStream_t)a->stream;
    const unsigned long long n_all = plane * (unsigned long long)a->nt;
    const unsigned long long n_adm = (unsigned long long)(a->jhi - a->jlo + 1) * (unsigned long long)(a->ihi - a->ilo + 1) * (unsigned long long)a->nt;
    const auto grid = [](unsigned long long items) {
        const unsigned long long g = (items + kThreads - 1) / kThreads;
        return dim3((unsigned)(g < kSeriesGrid ? g : kSeriesGrid));
    };
    const dim3 steps((unsigned)((unsigned)a->nt < kSeriesGrid ? (unsigned)a->nt : kSeriesGrid));
    if (ring) {
        hipLaunchKernelGGL(lec_seeds_series_smooth_ring_kernel, grid(n_all), dim3(kThreads), 0, st, q, a->nt);
        hipLaunchKernelGGL(lec_seeds_series_candidate_ring_kernel, grid(n_adm), dim3(kThreads), 0, st, q, a->nt);
        hipLaunchKernelGGL(lec_seeds_series_select_ring_kernel, steps, dim3(kThreads), 0, st, q, a->nt);
    } else {
        hipLaunchKernelGGL(lec_seeds_series_smooth_kernel, grid(n_all), dim3(kThreads), 0, st, q, a->nt);
        hipLaunchKernelGGL(lec_seeds_series_candidate_kernel, grid(n_adm), dim3(kThreads), 0, st, q, a->nt);
        hipLaunchKernelGGL(lec_seeds_series_select_kernel, steps, dim3(kThreads), 0, st, q, a->nt);
    }
    return launched(who);
}

}  // namespace

extern "C" int lec_follow_seeds_series(const lec_follow_seeds_series_args* a) { return seeds_series(a, "lec_follow_seeds_series", false); }
extern "C" int lec_follow_seeds_series_ring(const lec_follow_seeds_series_args* a) { return seeds_series(a, "lec_follow_seeds_series_ring", true); }

extern "C" int lec_follow_spans(const lec_follow_spans_args* a) {
    const char* who = "lec_follow_spans";
    if (!a) return refuse(LEC_ERR_ARG, who, "null args");
    const NamedPtr ptrs[] = {{a->u_d, "u_d"}, {a->v_d, "v_d"}, {a->xcoef_d, "xcoef_d"}, {a->ycoef_d, "ycoef_d"}, {a->curv_d, "curv_d"},
                             {a->start_d, "start_d"}, {a->pos_d, "pos_d"}, {a->val_d, "val_d"}, {a->status_d, "status_d"}, {a->span_d, "span_d"}};
    if (int rc = check_pointers(who, ptrs)) return rc;
    if (int rc = check_slice(who, a, a->nt)) return rc;
    if (a->n_chains < 1) return refuse(LEC_ERR_ARG, who, "n_chains must be >= 1");
    if (a->patience < 1) return refuse(LEC_ERR_ARG, who, "patience must be >= 1");
    long long lds;
    if (int rc = check_window(who, a, &lds)) return rc;
    FollowParams p = slice_params(a, a->nt);
    p.sj = a->sj; p.si = a->si;
    p.pos = a->pos_d; p.val = a->val_d; p.status = a->status_d;
    hipStream_t st = (hipStream_t)a->stream;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)lec_follow_spans_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return refuse(LEC_ERR_LAUNCH, who, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(lec_follow_spans_kernel, dim3(a->n_chains), dim3(kThreads), (size_t)lds, st, p, a->start_d, a->end_threshold, a->patience, a->span_d);
    return launched(who);
}

namespace {

int spans_chunk_call(const lec_follow_chunk_args* a, const char* who, bool ring) {
    if (!a) return refuse(LEC_ERR_ARG, who, "null args");
    const NamedPtr ptrs[] = {{a->u_d, "u_d"}, {a->v_d, "v_d"}, {a->xcoef_d, "xcoef_d"}, {a->ycoef_d, "ycoef_d"}, {a->curv_d, "curv_d"},
                             {a->start_d, "start_d"}, {a->pos_d, "pos_d"}, {a->val_d, "val_d"}, {a->status_d, "status_d"}, {a->span_d, "span_d"},
                             {a->state_d, "state_d"}};
    if (int rc = check_pointers(who, ptrs)) return rc;
    if (int rc = check_slice(who, a, a->nt)) return rc;
    if (a->n_chains < 1) return refuse(LEC_ERR_ARG, who, "n_chains must be >= 1");
    if (a->patience < 0) return refuse(LEC_ERR_ARG, who, "patience must be >= 0 (0: the chains never stop)");
    if (a->t_base < 0) return refuse(LEC_ERR_ARG, who, "t_base must be >= 0");
    if ((long long)a->t_base + a->nt > 0x7fffffffLL) return refuse(LEC_ERR_ARG, who, "t_base + nt must fit a 32-bit series step");
    long long lds;
    if (int rc = check_window(who, a, &lds)) return rc;
    if (ring)
        if (int rc = check_ring(who, a, 2LL * a->si + 1 + 2LL * a->smooth_r, "2 si + 1 + 2 smooth_r")) return rc;
    FollowParams p = slice_params(a, a->nt);
    p.sj = a->sj; p.si = a->si;
    p.pos = a->pos_d; p.val = a->val_d; p.status = a->status_d;
    hipStream_t st = (hipStream_t)a->stream;
    const auto kernel = ring ? lec_follow_spans_chunk_ring_kernel : lec_follow_spans_chunk_kernel;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return refuse(LEC_ERR_LAUNCH, who, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kernel, dim3(a->n_chains), dim3(kThreads), (size_t)lds, st, p, a->start_d, a->end_threshold, a->patience,
                       a->span_d, a->t_base, a->state_d);
    return launched(who);
}

}  // namespace

extern "C" int lec_follow_spans_chunk(const lec_follow_chunk_args* a) { return spans_chunk_call(a, "lec_follow_spans_chunk", false); }
extern "C" int lec_follow_spans_chunk_ring(const lec_follow_chunk_args* a) { return spans_chunk_call(a, "lec_follow_spans_chunk_ring", true); }
