// lec_rowsweep.hip -- stage 1, single-sweep kernel: one wave per (time, level, box-latitude) row, ONE sweep over the row.
//
//  * One sweep per row.  Sums are formed about a shift c (the row's first element) instead of about
//    the row mean: with a = T - cT, b = u - cU, c = v - cV, d = w - cW, e = Phi - cP, f = Q the 20
//    weighted sums  <a> <b> <c> <d> <e> <f>  <aa> <bb> <cc> <ca> <da> <bc> <db> <dc> <de> <fa>
//    <caa> <daa> <(bb+cc)c> <(bb+cc)d>  give every centred statistic exactly, e.g.
//    [T'T'] = <aa> - <a>^2,  [vT'T'] = <caa> - 2<a><ca> + <a>^2<c> + cV [T'T'],
//    [Kv] = 2[u][u'v'] + [u]^2[v] + 2[v][v'v'] + [v]^3   (K = u^2+v^2-u'^2-v'^2 = 2u[u]-[u]^2+2v[v]-[v]^2).
//    The shift keeps the cancellation benign (|row mean - first element| is of the order of the eddy
//    amplitude).  Half the fp64 work of the two-sweep form (lec_rowstats.hip), one reduction instead of
//    two, and the fields need not stay in registers across it.
//  * One wave per row walks it in trips of 64 vectors inside a real (not unrolled) loop: the live state
//    is the 20 accumulators plus one vector of every operand, which fits 4 waves per SIMD.
//  * The helpers shared with the row-block kernel (lec_rowblock.hip) live in lec_sweep.h.
//  * The kernel template and its launch helpers live in lec_rowsweep_kernel.h: this file instantiates the limited-area rows,
//    lec_rowsweep_ring.hip the rows that are a closed circle of longitudes (a code object of its own).
//
// Output: the same LEC_NSTAT row records as lec_rowstats.hip (stage 2 is unchanged).
#include "lec_rowsweep_kernel.h"

namespace {

// Completes [Q] and [Q'T'] of the time-stencil mode from the row records: the time-derivative part of Q is linear in
// T(t-1), T(t), T(t+1), so  [Q] += cp (ta [T](t-1) + tb [T](t) + tc [T](t+1))  and
// [Q'T'] += cp (ta [T'(t)T'(t-1)] + tb [T'T'] + tc [T'(t)T'(t+1)]).  The backward pieces are the previous row's
// forward ones when that row was processed in this launch, else the row's own (slots 30, 31).  One fixed box only.
__global__ void __launch_bounds__(256) lec_qtime_kernel(const RowParams p) {
#pragma clang fp contract(off)
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per_t = (long long)p.nl * p.nyb_max;
    if (row >= per_t * p.t_count) return;
    const int tl = (int)(row / per_t);
    double* __restrict__ rec = p.rows + (size_t)row * LEC_NSTAT;
    const bool from_prev = tl > 0;
    const double* __restrict__ prev = rec - (size_t)per_t * LEC_NSTAT;
    const double mtb = from_prev ? prev[LEC_S_MT] : rec[LEC_S_SPARE + 3];
    const double cb = from_prev ? prev[LEC_S_SPARE + 0] : rec[LEC_S_SPARE + 2];
    const double* tcf = p.tcoef + (size_t)(p.t_begin + tl) * 3;
    const double ta = tcf[0], tb = tcf[1], tc = tcf[2];
    const double dm = (ta * mtb + tc * rec[LEC_S_SPARE + 1]) + tb * rec[LEC_S_MT];
    const double dc = (ta * cb + tc * rec[LEC_S_SPARE + 0]) + tb * rec[LEC_S_TT];
    rec[LEC_S_MQ] = rec[LEC_S_MQ] + kCp * dm;
    rec[LEC_S_QT] = rec[LEC_S_QT] + kCp * dc;
}

}  // namespace

// `aligned` = every cube base is 16-byte aligned and nx is a multiple of the 16-byte vector;
// `aligned8` (fp32 only) = 8-byte aligned bases and even nx.  fp32 storage uses float4 vectors when it can
// (four elements per lane and trip, operands kept as floats and converted at use, one element finished before the
// next starts: 141 VGPRs, 3 waves/SIMD, 10.5 ms per 64 steps) and float2 otherwise (11.0 ms; tuning.f32_vec = 2 forces it).
int lec_launch_rowsweep(const lec::RowParams& p, int dtype, bool aligned, bool aligned8, bool uniform, int mode, int f32_vec, hipStream_t st) {
    return launch_dtype<false>(p, dtype, aligned, aligned8, uniform, mode, f32_vec, st);
}

int lec_launch_qtime(const lec::RowParams& p, hipStream_t st) {
    const long long rows = (long long)p.t_count * p.nl * p.nyb_max;
    hipLaunchKernelGGL(lec_qtime_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, p);
    return LEC_OK;
}
