// lec_rowspecq.hip -- lec_rowspec_q_ring: the zonal-wavenumber shares C_n(Q, T) of the generation covariance [Q'T'] of every ring row
// (-f --periodic --wavenumbers N --wavenumbers-generation; include/lec_hip.h).  A translation unit of its own: its
// code object is loaded by calls that ask for Ge(n) only.
//
// The workgroup, the lane mapping, the twiddle table and the fixed-order sum over the column classes are lec_rowspec_core.h's, with
// kRows = 2 neighbouring (time, level, latitude) rows per workgroup.  The staging phase is the stencil of the diabatic-heating residual.
// Per trip of kChunk columns every thread forms Q / cp = dT/dt + u dT/dx + v dT/dy - S w of its columns from the row itself, its six
// neighbour rows in time, pressure and latitude (the row itself with coefficient 0 where a neighbour does not exist: nothing outside the
// band, the levels or the cube's steps is read) and u, v, w -- the expressions of sweep_one (lec_sweep.h) with the per-point dT/dt of its
// QMODE 1 -- and stores {T - T(column 0), Q / cp} as one double2.  The lambda neighbours are read from memory at wrapped column indices,
// so neither the ring's seam nor a trip's is a special case.  The projection then costs 4 fp64 FMAs per (row, column, n) and twiddle.
#include "lec_rowspec_core.h"
#include "lec_sweep.h"

namespace {

using namespace lec::spec;

constexpr int kRows = 2;               // rows per workgroup: one twiddle load feeds both (1 and 4 measured: 4 wins at N = 8 and 64, loses at 20)
constexpr int kChunk = 512;            // columns staged per trip: 8 KiB of LDS per row, which the 256 x 4 partial sums reuse afterwards
constexpr int kComp = 4;               // {T, Q / cp} x {cos, sin}
static_assert(kChunk * 2 >= kThreads * kComp, "the partial sums of a row reuse its staged columns");

struct SpecQParams {
    const void *T, *U, *V, *W;
    const double2* twid;               // [nx] {cos, sin}(2 pi m / nx)
    const double* lattab;              // [nyb][4]
    const double* levtab;              // [nl][3]
    const double* tcoef;               // [nt][3]
    double* qspec;                     // [t_count][nl][nyb][n_wave]
    double inv_hdeg;
    int nt, nl, ny, nx, t_begin, js, nyb, n_wave;
};

// columns [c0, c0 + cn) of one row -> dst[c - c0] = {T - T[0], Q / cp}.  Everything but the column is wave-uniform.
template <typename E>
__device__ __forceinline__ void stage_row(const SpecQParams& p, const long long row, const int c0, const int cn, double2* __restrict__ dst, const int tid) {
#pragma clang fp contract(off)
    const int nx = p.nx;
    const Row<E> r = decode_row<E>(p, row);
    const int jb = r.jb, k = r.k, t = r.t;
    const size_t plane = r.plane, cube = r.cube;
    const E* __restrict__ rT = r.T;
    const E* __restrict__ rU = r.U;
    const E* __restrict__ rV = r.V;
    const E* __restrict__ rW = r.W;
    // a neighbour that does not exist: the row itself, whose coefficient in the tables is 0
    const E* rTjm = jb > 0 ? rT - nx : rT;
    const E* rTjp = jb < p.nyb - 1 ? rT + nx : rT;
    const E* rTkm = k > 0 ? rT - plane : rT;
    const E* rTkp = k < p.nl - 1 ? rT + plane : rT;
    const E* rTtm = t > 0 ? rT - cube : rT;
    const E* rTtp = t < p.nt - 1 ? rT + cube : rT;
    const double* lt = p.lattab + (size_t)jb * 4;
    const double ga = lt[0], gb = lt[1], gc = lt[2];
    const double cx = 0.5 * p.inv_hdeg * lt[3];            // centred d/dlon -> d/dx
    const double* lv = p.levtab + (size_t)k * 3;
    const double al = lv[0], be = lv[1], gm = lv[2];
    const double* tcf = p.tcoef + (size_t)t * 3;
    const double ta = tcf[0], tb = tcf[1], tc = tcf[2];
    const double t0 = (double)rT[0];
    for (int c = tid; c < cn; c += kThreads) {
        const int i = c0 + c;
        const int il = i == 0 ? nx - 1 : i - 1, ir = i == nx - 1 ? 0 : i + 1;      // the circle closes: centred everywhere
        const double Tc = (double)rT[i];
        const double adv = ((double)rU[i] * cx) * ((double)rT[ir] - (double)rT[il]);
        const double sP = lec::stencil3(ga, (double)rTjm[i], gc, (double)rTjp[i], gb, Tc);
        const double sS = lec::stencil3(al, (double)rTkm[i], gm, (double)rTkp[i], be, Tc);
        const double rest = lec::stencil3(ta, (double)rTtm[i], tc, (double)rTtp[i], tb, Tc) + adv;
        const double f = fma(-(double)rW[i], sS, fma((double)rV[i], sP, rest));
        dst[c] = make_double2(Tc - t0, f);
    }
}

template <typename E, int R, bool TWLDS>
__global__ __launch_bounds__(kThreads) void lec_rowspec_q_kernel(const SpecQParams p, const long long nrows) {
    __shared__ __attribute__((aligned(16))) double fld[R][kChunk * 2];
    __shared__ double red[R][LEC_MAX_WAVENUMBERS * kComp];
    const int tid = threadIdx.x;
    const int N = p.n_wave, nx = p.nx;
    long long rows[R];
    wg_rows(nrows, rows);
    stage_twiddles<TWLDS>(p.twid, nx, tid);

    Lane lane(tid, N, nx);
    double acc[R][kComp] = {};

    for (int c0 = 0; c0 < nx; c0 += kChunk) {
        const int cn = min(kChunk, nx - c0);
        if (c0) __syncthreads();                   // the trip before has been read
#pragma unroll
        for (int r = 0; r < R; ++r) stage_row<E>(p, rows[r], c0, cn, (double2*)fld[r], tid);
        __syncthreads();
        if (lane.active)
            project<2, TWLDS>(lane, c0, c0 + cn, nx, p.twid, acc, [&](const int r, const int c, double (&x)[2]) {
                const double2 a = ((const double2*)fld[r])[c];
                x[0] = a.x; x[1] = a.y;
            });
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) spill(lane, tid, fld[r], acc[r]);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) class_sum<kComp>(lane, tid, N, fld[r], red[r]);
    __syncthreads();
    // C_n(Q, T) = w_n Re(Q^_n conj(T^_n)), Q = cp f: fields {T, Q / cp} = {0, 1}
    const double inv = lec::kCp / ((double)nx * (double)nx);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (row_repeated(rows, r)) break;
        for (int nn = tid; nn < N; nn += kThreads)
            p.qspec[(size_t)rows[r] * N + nn] = wave_weight(nn, nx) * cov(&red[r][kComp * nn], 1, 0) * inv;
    }
}

}  // namespace

extern "C" int lec_rowspec_q_ring(const lec_rowspec_q_args* a) {
    const Refusals R{"lec_rowspec_q_ring"};
    int rc, nyb;
    long long nrows;
    if (!a) return R.refuse(LEC_ERR_ARG, "null args");
    if ((rc = R.pointers(a, {}, {{a->lattab_d, "lattab_d"}, {a->levtab_d, "levtab_d"},
                                 {a->tcoef_d, "tcoef_d (a dT/dt cube is not supported: dT/dt comes from the cube's time axis)"},
                                 {a->qspec_d, "qspec_d"}})) != LEC_OK) return rc;
    if ((rc = R.dtype(a)) != LEC_OK) return rc;
    if (a->nt < 2) return R.refuse(LEC_ERR_ARG, "nt must be >= 2 (dT/dt by finite differences over the cube's time axis)");
    if (a->nl < 1 || a->ny < 2) return R.refuse(LEC_ERR_ARG, "cube needs nl >= 1, ny >= 2");
    if ((rc = R.ring_steps_band(a)) != LEC_OK) return rc;
    // (lec_rowstats_ring refuses a one-row band too: its box extents must be 2..ny rows)
    if (a->jn == a->js) return R.refuse(LEC_ERR_ARG, "jn must be > js (a band needs two rows for d/dlat)");
    if ((rc = R.wavenumbers(a)) != LEC_OK) return rc;
    if ((rc = R.aligned(a->qspec_d, 16, "qspec_d")) != LEC_OK) return rc;
    if ((rc = R.aligned(a->lattab_d, 8, "lattab_d")) != LEC_OK) return rc;
    if ((rc = R.aligned(a->levtab_d, 8, "levtab_d")) != LEC_OK) return rc;
    if ((rc = R.aligned(a->tcoef_d, 8, "tcoef_d")) != LEC_OK) return rc;
    if ((rc = R.cubes_rows(a, &nyb, &nrows)) != LEC_OK) return rc;

    SpecQParams p;
    common_params(p, a, nyb);
    p.lattab = a->lattab_d; p.levtab = a->levtab_d; p.tcoef = a->tcoef_d;
    p.qspec = a->qspec_d; p.inv_hdeg = a->inv_hdeg; p.nt = a->nt;
    hipStream_t st = (hipStream_t)a->stream;
    return R.launched(a->dtype == LEC_F64 ? launch(lec_rowspec_q_kernel<double, kRows, true>, lec_rowspec_q_kernel<double, kRows, false>, kRows, p, nrows, st)
                                          : launch(lec_rowspec_q_kernel<float, kRows, true>, lec_rowspec_q_kernel<float, kRows, false>, kRows, p, nrows, st));
}
