// lec_rowspec_b.hip -- lec_rowspec_b_ring: the zonal-wavenumber shares of the four triple products of a ring row that stage 2 reads for the
// boundary terms of the eddy budgets, BAe(n) and BKe(n) of -f --periodic --wavenumbers N --wavenumbers-budget (include/lec_hip.h, DESIGN.md
// section 4.2b).  A translation unit of its own: its code object is loaded by calls that ask for the budget only.
//
// A triple product [a b'b'] is the covariance of the pointwise product P = a b' with b, because [b'] = 0: [a b'b'] = [P'b'] = sum_n C_n(P, b).
// So with v and w the FULL fields and x' = x - [x] against the zonal means of the row's record
//   VTT(n) = C_n(v T', T)                     WTT(n) = C_n(w T', T)
//   EV(n)  = C_n(v u', u) + C_n(v v', v)      EW(n)  = C_n(w u', u) + C_n(w v', v)
// and the nx / 2 shares of a row sum to slots LEC_S_VTT, LEC_S_WTT, LEC_S_EV, LEC_S_EW of its record.
//
// The workgroup, the lane mapping, the twiddle table and the fixed-order sum over the column classes are lec_rowspec_core.h's, with one
// row per workgroup.  Per trip of kChunk columns every thread loads T, u, v, w at its columns (four loads per column: no neighbour row, no
// derivative) and stores nine doubles per column: {T', u'} {v', w T'} {w u', w v'} {v T', v u'} as double2 arrays and v v' as a double array (16-byte
// strides keep the 16-byte LDS accesses of neighbouring columns on neighbouring banks).  The projection runs the nine fields on cos and sin:
// 18 fp64 FMAs per (row, column, n) and twiddle.  Stage 2 reads VTT and EV at the band's first and last row only, so for every other row the
// three v products are neither formed nor projected (12 FMAs) -- the branch is uniform over the workgroup -- and slots 0 and 2 are written
// as 0.0.  WTT and EW are written for every row and level: _handle_nans can move "bottom" and "top" to any level.
//
// Trip length: kChunk = 576 columns, one row per workgroup (measured, profiles/spectrum_b_notes.md).  The staging phase is light here --
// four loads per column --, so what decides is how many workgroups a CU holds, and that is LDS: 576 columns x 72 B = 40.5 KiB of staged
// columns -- exactly the 256 x 18 partial sums that reuse them afterwards, so a shorter trip saves nothing -- + 9 KiB of sums per wavenumber
// + 16 nx bytes of twiddles when the table is staged (N >= 16, nx <= 4096).  At nx = 1440: 72 KiB with the staged table, two workgroups
// per CU of 160 KiB; 49.5 KiB without, three.  The sibling's 768 columns (63 KiB; 85.5 KiB with the table: ONE workgroup per CU) were
// a third slower at N = 20 and N = 64.  117 VGPRs, no scratch.
#include "lec_rowspec_core.h"

namespace {

using namespace lec::spec;

constexpr int kRows = 1;               // rows per workgroup: a wall row and an inner row stage and project different fields
constexpr int kChunk = 576;            // columns staged per trip: 40.5 KiB of LDS, all of it reused by the partial sums
constexpr int kComp = 18;              // {T', u', v', w T', w u', w v', v T', v u', v v'} x {cos, sin}
constexpr int kCompInner = 12;         // a row that is no wall: the first six fields
static_assert(kChunk * 8 >= kThreads * kComp, "the partial sums of the row reuse the staged columns");

struct SpecBParams {
    const void *T, *U, *V, *W;
    const double* rows;                // [t_count][nl][nyb][LEC_NSTAT]
    const double2* twid;               // [nx] {cos, sin}(2 pi m / nx)
    double* bspec;                     // [t_count][nl][nyb][n_wave][4]
    int nl, ny, nx, t_begin, js, nyb, n_wave;
};

// columns [c0, c0 + cn) of one row -> fa[c - c0] = {T', u'}, fb = {v', w T'}, fc = {w u', w v'} and, at a wall row, fd = {v T', v u'},
// fe = v v'.  Everything but the column is wave-uniform.
template <typename E, bool WALL>
__device__ __forceinline__ void stage_row(const SpecBParams& p, const long long row, const int c0, const int cn, double2* __restrict__ fa,
                                          double2* __restrict__ fb, double2* __restrict__ fc, double2* __restrict__ fd, double* __restrict__ fe,
                                          const int tid) {
#pragma clang fp contract(off)
    const Row<E> r = decode_row<E>(p, row);
    const E* __restrict__ rT = r.T;
    const E* __restrict__ rU = r.U;
    const E* __restrict__ rV = r.V;
    const E* __restrict__ rW = r.W;
    const double* rec = p.rows + (size_t)row * LEC_NSTAT;
    const double mT = rec[LEC_S_MT], mU = rec[LEC_S_MU], mV = rec[LEC_S_MV];
    for (int c = tid; c < cn; c += kThreads) {
        const int i = c0 + c;
        const double Vc = (double)rV[i], Wc = (double)rW[i];
        const double tp = (double)rT[i] - mT, up = (double)rU[i] - mU, vp = Vc - mV;
        fa[c] = make_double2(tp, up);
        fb[c] = make_double2(vp, Wc * tp);
        fc[c] = make_double2(Wc * up, Wc * vp);
        if (WALL) {
            fd[c] = make_double2(Vc * tp, Vc * up);
            fe[c] = Vc * vp;
        }
    }
}

template <typename E, bool TWLDS>
__global__ __launch_bounds__(kThreads) void lec_rowspec_b_kernel(const SpecBParams p, const long long nrows) {
    __shared__ __attribute__((aligned(16))) double2 fld[4][kChunk];
    __shared__ double fe[kChunk];
    __shared__ double red[LEC_MAX_WAVENUMBERS * kComp];
    const int tid = threadIdx.x;
    const int N = p.n_wave, nx = p.nx;
    long long rows[kRows];
    wg_rows(nrows, rows);
    const long long row = rows[0];
    const int jb = (int)(row % p.nyb);
    const bool wall = jb == 0 || jb == p.nyb - 1;  // the rows whose VTT and EV stage 2 reads; the same for every thread of the workgroup
    stage_twiddles<TWLDS>(p.twid, nx, tid);

    Lane lane(tid, N, nx);
    double acc[kRows][kComp] = {};

    for (int c0 = 0; c0 < nx; c0 += kChunk) {
        const int cn = min(kChunk, nx - c0);
        if (c0) __syncthreads();                   // the trip before has been read
        if (wall) stage_row<E, true>(p, row, c0, cn, fld[0], fld[1], fld[2], fld[3], fe, tid);
        else stage_row<E, false>(p, row, c0, cn, fld[0], fld[1], fld[2], fld[3], fe, tid);
        __syncthreads();
        if (lane.active) {
            if (wall)
                project<9, TWLDS>(lane, c0, c0 + cn, nx, p.twid, acc, [&](const int, const int c, double (&x)[9]) {
                    const double2 a = fld[0][c], b = fld[1][c], d = fld[2][c], e = fld[3][c];
                    x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y; x[4] = d.x; x[5] = d.y; x[6] = e.x; x[7] = e.y; x[8] = fe[c];
                });
            else
                project<6, TWLDS>(lane, c0, c0 + cn, nx, p.twid, acc, [&](const int, const int c, double (&x)[6]) {
                    const double2 a = fld[0][c], b = fld[1][c], d = fld[2][c];
                    x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y; x[4] = d.x; x[5] = d.y;
                });
        }
    }
    double* const part = (double*)&fld[0][0];
    __syncthreads();                                // the last trip has been read
    spill(lane, tid, part, acc[0]);
    __syncthreads();
    class_sum<kComp>(lane, tid, N, part, red, wall ? kComp : kCompInner);      // (an interior row's last six are 0 and are not summed)
    __syncthreads();
    // C_n(P, x) = w_n Re(P^_n conj(x^_n)) / nx^2: fields 0 T, 1 u, 2 v, 3 wT', 4 wu', 5 wv', 6 vT', 7 vu', 8 vv'.  slot 0 VTT, 1 WTT, 2 EV, 3 EW
    const double inv = 1.0 / ((double)nx * (double)nx);
    for (int o = tid; o < 4 * N; o += kThreads) {
        const int nn = o >> 2, s = o & 3;
        const double* q = &red[kComp * nn];
        const double wgt = wave_weight(nn, nx);
        double val = 0.0;
        if (s == 1) val = wgt * cov(q, 3, 0) * inv;
        else if (s == 3) val = wgt * (cov(q, 4, 1) + cov(q, 5, 2)) * inv;
        else if (wall && s == 0) val = wgt * cov(q, 6, 0) * inv;
        else if (wall) val = wgt * (cov(q, 7, 1) + cov(q, 8, 2)) * inv;
        p.bspec[((size_t)row * N + nn) * 4 + s] = val;
    }
}

}  // namespace

extern "C" int lec_rowspec_b_ring(const lec_rowspec_b_args* a) {
    const Refusals R{"lec_rowspec_b_ring"};
    int rc, nyb;
    long long nrows;
    if (!a) return R.refuse(LEC_ERR_ARG, "null args");
    if ((rc = R.pointers(a, {{a->rows_d, "rows_d"}}, {{a->bspec_d, "bspec_d"}})) != LEC_OK) return rc;
    if ((rc = R.dtype(a)) != LEC_OK) return rc;
    if (a->nt < 1) return R.refuse(LEC_ERR_ARG, "nt must be >= 1");
    if (a->nl < 1 || a->ny < 2) return R.refuse(LEC_ERR_ARG, "cube needs nl >= 1, ny >= 2");
    if ((rc = R.ring_steps_band(a)) != LEC_OK) return rc;
    if (a->jn == a->js) return R.refuse(LEC_ERR_ARG, "jn must be > js (a band has a south and a north wall row)");
    if ((rc = R.wavenumbers(a)) != LEC_OK) return rc;
    if ((rc = R.aligned(a->rows_d, 16, "rows_d")) != LEC_OK) return rc;
    if ((rc = R.aligned(a->bspec_d, 16, "bspec_d")) != LEC_OK) return rc;
    if ((rc = R.cubes_rows(a, &nyb, &nrows)) != LEC_OK) return rc;

    SpecBParams p;
    common_params(p, a, nyb);
    p.rows = a->rows_d; p.bspec = a->bspec_d;
    hipStream_t st = (hipStream_t)a->stream;
    return R.launched(a->dtype == LEC_F64 ? launch(lec_rowspec_b_kernel<double, true>, lec_rowspec_b_kernel<double, false>, kRows, p, nrows, st)
                                          : launch(lec_rowspec_b_kernel<float, true>, lec_rowspec_b_kernel<float, false>, kRows, p, nrows, st));
}
