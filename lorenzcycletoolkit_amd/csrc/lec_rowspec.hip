// lec_rowspec.hip -- lec_rowspec_ring: the zonal-wavenumber shares of the eight eddy covariances of every ring row (-f --periodic
// --wavenumbers; include/lec_hip.h).  A translation unit of its own: its code object is loaded by spectral calls only.
//
// The workgroup, the lane mapping, the twiddle table and the fixed-order sum over the column classes are lec_rowspec_core.h's, with
// kRows = 2 neighbouring (time, level, latitude) rows per workgroup.  The rows are staged in LDS in trips of kChunk columns as fp64
// {T, u, v, w} minus the row's column 0, so a lane reads a row's column with two 16-byte LDS loads -- lanes of one column class read one
// address (a broadcast), neighbouring classes neighbouring columns (other banks).  One twiddle serves both rows: 16 fp64 FMAs per 80
// bytes of operands.
#include "lec_rowspec_core.h"

namespace {

using namespace lec::spec;

constexpr int kRows = 2;               // rows per workgroup: one twiddle load feeds both (1, 3 and 4 measured slower)
constexpr int kChunk = 512;            // columns staged per trip: 16 KiB of LDS per row, which the 256 x 8 partial sums reuse afterwards
constexpr int kComp = 8;               // {T, u, v, w} x {cos, sin}
static_assert(kChunk * 4 >= kThreads * kComp, "the partial sums of a row reuse its staged columns");

struct SpecParams {
    const void *T, *U, *V, *W;
    const double2* twid;               // [nx] {cos, sin}(2 pi m / nx)
    double* spec;                      // [t_count][nl][nyb][n_wave][8]
    int nl, ny, nx, t_begin, js, nyb, n_wave;
};

template <typename E, int R, bool TWLDS>
__global__ __launch_bounds__(kThreads) void lec_rowspec_kernel(const SpecParams p, const long long nrows) {
    __shared__ __attribute__((aligned(16))) double fld[R][kChunk * 4];
    __shared__ double red[R][LEC_MAX_WAVENUMBERS * kComp];
    const int tid = threadIdx.x;
    const int N = p.n_wave, nx = p.nx;
    long long rows[R];
    wg_rows(nrows, rows);
    Row<E> row[R];
    double t0[R], u0[R], v0[R], w0[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        row[r] = decode_row<E>(p, rows[r]);
        // the reference value removed before projecting (T is ~288 K with eddies of ~1 K): the row's column 0; a constant has no share in n >= 1
        t0[r] = (double)row[r].T[0]; u0[r] = (double)row[r].U[0]; v0[r] = (double)row[r].V[0]; w0[r] = (double)row[r].W[0];
    }
    stage_twiddles<TWLDS>(p.twid, nx, tid);

    Lane lane(tid, N, nx);
    double acc[R][kComp] = {};

    for (int c0 = 0; c0 < nx; c0 += kChunk) {
        const int cn = min(kChunk, nx - c0);
        if (c0) __syncthreads();                   // the trip before has been read
#pragma unroll
        for (int r = 0; r < R; ++r)
            for (int c = tid; c < cn; c += kThreads) {
                double2* d = (double2*)&fld[r][4 * c];
                d[0] = make_double2((double)row[r].T[c0 + c] - t0[r], (double)row[r].U[c0 + c] - u0[r]);
                d[1] = make_double2((double)row[r].V[c0 + c] - v0[r], (double)row[r].W[c0 + c] - w0[r]);
            }
        __syncthreads();
        if (lane.active)
            project<4, TWLDS>(lane, c0, c0 + cn, nx, p.twid, acc, [&](const int r, const int c, double (&x)[4]) {
                const double2* f = (const double2*)&fld[r][4 * c];
                const double2 a = f[0], b = f[1];
                x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
            });
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) spill(lane, tid, fld[r], acc[r]);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) class_sum<kComp>(lane, tid, N, fld[r], red[r]);
    __syncthreads();
    // the eight shares in slot order LEC_S_TT .. LEC_S_WV: {T, u, v, w} = fields {0, 1, 2, 3}
    const double inv = 1.0 / ((double)nx * (double)nx);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (row_repeated(rows, r)) break;
        for (int o = tid; o < 8 * N; o += kThreads) {
            const int nn = o >> 3, s = o & 7;
            const int fa = (0x33132210 >> (4 * s)) & 15;     // first factor of slots 0 .. 7:  T u v v w u w w (a hex digit per slot, slot 0 lowest)
            const int fb = (0x21200210 >> (4 * s)) & 15;     // second factor:                 T u v T T v u v
            p.spec[((size_t)rows[r] * N + nn) * 8 + s] = wave_weight(nn, nx) * cov(&red[r][kComp * nn], fa, fb) * inv;
        }
    }
}

}  // namespace

extern "C" int lec_rowspec_ring(const lec_rowspec_args* a) {
    const Refusals R{"lec_rowspec_ring"};
    int rc, nyb;
    long long nrows;
    if (!a) return R.refuse(LEC_ERR_ARG, "null args");
    if ((rc = R.pointers(a, {}, {{a->spec_d, "spec_d"}})) != LEC_OK) return rc;
    if ((rc = R.dtype(a)) != LEC_OK) return rc;
    if (a->nt < 1 || a->nl < 1 || a->ny < 1) return R.refuse(LEC_ERR_ARG, "cube needs nt >= 1, nl >= 1, ny >= 1");
    if ((rc = R.ring_steps_band(a)) != LEC_OK) return rc;
    if ((rc = R.wavenumbers(a)) != LEC_OK) return rc;
    if ((rc = R.aligned(a->spec_d, 16, "spec_d")) != LEC_OK) return rc;
    if ((rc = R.cubes_rows(a, &nyb, &nrows)) != LEC_OK) return rc;

    SpecParams p;
    common_params(p, a, nyb);
    p.spec = a->spec_d;
    hipStream_t st = (hipStream_t)a->stream;
    return R.launched(a->dtype == LEC_F64 ? launch(lec_rowspec_kernel<double, kRows, true>, lec_rowspec_kernel<double, kRows, false>, kRows, p, nrows, st)
                                          : launch(lec_rowspec_kernel<float, kRows, true>, lec_rowspec_kernel<float, kRows, false>, kRows, p, nrows, st));
}
