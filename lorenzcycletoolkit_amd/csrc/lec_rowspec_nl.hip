// lec_rowspec_nl.hip -- lec_rowspec_nl_ring: the zonal-wavenumber shares -2 C_n(A_x, x), x = T, u, v, of the eddy-eddy advective
// tendencies of every ring row: the non-linear (triad) transfers S(n) and L(n) of -f --periodic --wavenumbers N
// --wavenumbers-interactions (include/lec_hip.h).  A translation unit of its own: its code object is loaded by
// calls that ask for the interactions only.
//
// The workgroup, the lane mapping, the twiddle table and the fixed-order sum over the column classes are lec_rowspec_core.h's, with
// kRows = 1 row per workgroup.  Per trip of kChunk columns every thread forms, for
// its columns, the eddies T', u', v', w' against the zonal means of the row's record and the three tendencies
//   A_x = u' D_lambda x + v' (D_phi x - D_phi [x]) + w' (D_p x - D_p [x])  (+ the metric terms of u and v)
// from the row itself, its four neighbour rows in latitude and pressure (the row itself with coefficient 0 where a neighbour does not
// exist: nothing outside the band or the levels is read) and the neighbour rows' records, and stores six doubles per column as three
// double2 arrays {T', u'} {v', A_T} {A_u, A_v}: a 16-byte stride per array keeps the 16-byte LDS accesses of neighbouring columns on
// neighbouring banks, which one array of 48-byte elements would not.  The projection costs 12 fp64 FMAs per (row, column, n) and
// twiddle.  The same staging pass sums A_x x', A_x and x' over the row's columns in physical space (per thread, then over the wave by a
// butterfly, then over the four waves in their order): nltot_d, the total the shares are judged against.
//
// Trip length and rows per workgroup: kChunk = 768, kRows = 1 (measured, profiles/spectrum_nl_notes.md).  The staging phase is bound by
// the latency of its 22 loads per column, and a barrier separates it from the projection: a trip has to give every thread several
// columns, whose loads are then in flight together -- three columns per thread and trip here, one at 256.  LDS per workgroup: 768
// columns x 48 B = 36 KiB of staged columns -- more than the 24 KiB the 256 x 12 partial sums need afterwards -- + 6 KiB of sums per
// wavenumber + 16 nx bytes of twiddles when the table is staged (N >= 16, nx <= 4096).  145 VGPRs: 3 waves per SIMD by registers.  At
// nx = 1440, N = 20: 65 KiB, two workgroups (8 waves, 2 per SIMD) per CU of 160 KiB; without the staged table 42 KiB, three workgroups;
// at nx = 4096 with it 106 KiB, one workgroup.  Two rows per workgroup (one twiddle load for both, the siblings' form) cost 164 to 190
// VGPRs and twice the LDS and were slower at every trip length tried; a trip of 2048 columns leaves one workgroup per CU and is twice
// as slow.
#include "lec_rowspec_core.h"
#include "lec_sweep.h"

namespace {

using namespace lec::spec;

constexpr int kWaves = kThreads / 64;
constexpr int kRows = 1;               // rows per workgroup (2 measured slower: registers and LDS cost more occupancy than the shared twiddle saves)
constexpr int kChunk = 768;            // columns staged per trip: 36 KiB of LDS per row
constexpr int kComp = 12;              // {T', u', v', A_T, A_u, A_v} x {cos, sin}
constexpr int kTot = 9;                // physical-space sums of a row: A_x x' (3), A_x (3), x' (3)
static_assert(kRows * kChunk * 6 >= kThreads * kComp, "the partial sums of one row reuse the staged columns");

struct SpecNlParams {
    const void *T, *U, *V, *W;
    const double* rows;                // [t_count][nl][nyb][LEC_NSTAT]
    const double2* twid;               // [nx] {cos, sin}(2 pi m / nx)
    const double* lattab;              // [nyb][5]
    const double* ptab;                // [nl][3]
    double* nlspec;                    // [t_count][nl][nyb][n_wave][8]
    double* nltot;                     // [t_count][nl][nyb][8]
    double inv_hdeg;
    int nl, ny, nx, t_begin, js, nyb, n_wave;
};

// columns [c0, c0 + cn) of one row -> fa[c - c0] = {T', u'}, fb = {v', A_T}, fc = {A_u, A_v}; tot += this thread's share of the row's
// physical-space sums.  Everything but the column is wave-uniform.
template <typename E>
__device__ __forceinline__ void stage_row(const SpecNlParams& p, const long long row, const int c0, const int cn, double2* __restrict__ fa,
                                          double2* __restrict__ fb, double2* __restrict__ fc, double (&tot)[kTot], const int tid) {
#pragma clang fp contract(off)
    const int nx = p.nx;
    const Row<E> r = decode_row<E>(p, row);
    const int jb = r.jb, k = r.k;
    const size_t plane = r.plane;
    const E* __restrict__ rT = r.T;
    const E* __restrict__ rU = r.U;
    const E* __restrict__ rV = r.V;
    const E* __restrict__ rW = r.W;
    // a neighbour that does not exist: the row itself, whose coefficient in the tables is 0
    const long long oj0 = jb > 0 ? -(long long)nx : 0, oj1 = jb < p.nyb - 1 ? (long long)nx : 0;
    const long long ok0 = k > 0 ? -(long long)plane : 0, ok1 = k < p.nl - 1 ? (long long)plane : 0;
    const double* rec = p.rows + (size_t)row * LEC_NSTAT;
    const double* recj0 = jb > 0 ? rec - LEC_NSTAT : rec;
    const double* recj1 = jb < p.nyb - 1 ? rec + LEC_NSTAT : rec;
    const double* reck0 = k > 0 ? rec - (size_t)p.nyb * LEC_NSTAT : rec;
    const double* reck1 = k < p.nl - 1 ? rec + (size_t)p.nyb * LEC_NSTAT : rec;
    const double* lt = p.lattab + (size_t)jb * 5;
    const double ga = lt[0], gb = lt[1], gc = lt[2];
    const double cx = 0.5 * p.inv_hdeg * lt[3];            // centred d/dlon -> d/dx
    const double mj = lt[4];                               // tan(lat) / Re
    const double* pt = p.ptab + (size_t)k * 3;
    const double pa = pt[0], pb = pt[1], pc = pt[2];
    const double mT = rec[LEC_S_MT], mU = rec[LEC_S_MU], mV = rec[LEC_S_MV], mW = rec[LEC_S_MW];
    // d/dlat and d/dp of the zonal means, from the neighbours' records
    const double yT = lec::stencil3(ga, recj0[LEC_S_MT], gc, recj1[LEC_S_MT], gb, mT);
    const double yU = lec::stencil3(ga, recj0[LEC_S_MU], gc, recj1[LEC_S_MU], gb, mU);
    const double yV = lec::stencil3(ga, recj0[LEC_S_MV], gc, recj1[LEC_S_MV], gb, mV);
    const double zT = lec::stencil3(pa, reck0[LEC_S_MT], pc, reck1[LEC_S_MT], pb, mT);
    const double zU = lec::stencil3(pa, reck0[LEC_S_MU], pc, reck1[LEC_S_MU], pb, mU);
    const double zV = lec::stencil3(pa, reck0[LEC_S_MV], pc, reck1[LEC_S_MV], pb, mV);
    for (int c = tid; c < cn; c += kThreads) {
        const int i = c0 + c;
        const int il = i == 0 ? nx - 1 : i - 1, ir = i == nx - 1 ? 0 : i + 1;      // the circle closes: centred everywhere
        const double Tc = (double)rT[i], Uc = (double)rU[i], Vc = (double)rV[i];
        const double tp = Tc - mT, up = Uc - mU, vp = Vc - mV, wp = (double)rW[i] - mW;
        const double xT = cx * ((double)rT[ir] - (double)rT[il]);
        const double xU = cx * ((double)rU[ir] - (double)rU[il]);
        const double xV = cx * ((double)rV[ir] - (double)rV[il]);
        const double dyT = lec::stencil3(ga, (double)rT[i + oj0], gc, (double)rT[i + oj1], gb, Tc) - yT;
        const double dyU = lec::stencil3(ga, (double)rU[i + oj0], gc, (double)rU[i + oj1], gb, Uc) - yU;
        const double dyV = lec::stencil3(ga, (double)rV[i + oj0], gc, (double)rV[i + oj1], gb, Vc) - yV;
        const double dpT = lec::stencil3(pa, (double)rT[i + ok0], pc, (double)rT[i + ok1], pb, Tc) - zT;
        const double dpU = lec::stencil3(pa, (double)rU[i + ok0], pc, (double)rU[i + ok1], pb, Uc) - zU;
        const double dpV = lec::stencil3(pa, (double)rV[i + ok0], pc, (double)rV[i + ok1], pb, Vc) - zV;
        const double aT = (up * xT + vp * dyT) + wp * dpT;
        const double aU = ((up * xU + vp * dyU) + wp * dpU) - mj * (up * vp);
        const double aV = ((up * xV + vp * dyV) + wp * dpV) + mj * (up * up);
        fa[c] = make_double2(tp, up);
        fb[c] = make_double2(vp, aT);
        fc[c] = make_double2(aU, aV);
        tot[0] += aT * tp; tot[1] += aU * up; tot[2] += aV * vp;
        tot[3] += aT; tot[4] += aU; tot[5] += aV;
        tot[6] += tp; tot[7] += up; tot[8] += vp;
    }
}

__device__ __forceinline__ double wave_sum(double x) {      // a butterfly: every lane ends with the same sum, formed in one order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

template <typename E, int R, bool TWLDS>
__global__ __launch_bounds__(kThreads) void lec_rowspec_nl_kernel(const SpecNlParams p, const long long nrows) {
    __shared__ __attribute__((aligned(16))) double2 fld[3][R][kChunk];
    __shared__ double red[R][LEC_MAX_WAVENUMBERS * kComp];
    __shared__ double wtot[R][kTot][kWaves];
    const int tid = threadIdx.x;
    const int N = p.n_wave, nx = p.nx;
    long long rows[R];
    wg_rows(nrows, rows);
    stage_twiddles<TWLDS>(p.twid, nx, tid);

    Lane lane(tid, N, nx);
    double acc[R][kComp] = {};
    double tot[R][kTot] = {};

    for (int c0 = 0; c0 < nx; c0 += kChunk) {
        const int cn = min(kChunk, nx - c0);
        if (c0) __syncthreads();                   // the trip before has been read
#pragma unroll
        for (int r = 0; r < R; ++r) stage_row<E>(p, rows[r], c0, cn, fld[0][r], fld[1][r], fld[2][r], tot[r], tid);
        __syncthreads();
        if (lane.active)
            project<6, TWLDS>(lane, c0, c0 + cn, nx, p.twid, acc, [&](const int r, const int c, double (&x)[6]) {
                const double2 a = fld[0][r][c], b = fld[1][r][c], d = fld[2][r][c];
                x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y; x[4] = d.x; x[5] = d.y;
            });
    }
    // the physical-space sums: over the wave, then over the waves in their order
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < kTot; ++q) {
            const double s = wave_sum(tot[r][q]);
            if ((tid & 63) == 0) wtot[r][q][tid >> 6] = s;
        }
    double* const part = (double*)&fld[0][0][0];    // the partial sums of ONE row
#pragma unroll
    for (int r = 0; r < R; ++r) {
        __syncthreads();                            // the last trip, or the row before, has been read
        spill(lane, tid, part, acc[r]);
        __syncthreads();
        class_sum<kComp>(lane, tid, N, part, red[r]);
    }
    __syncthreads();
    // slot s = 0, 1, 2: -2 C_n(A_x, x) = -2 w_n Re(A_x^_n conj(x^_n)), x = T, u, v: fields {x, A_x} = {s, 3 + s}; slots 3 .. 7: 0
    const double inv = 1.0 / ((double)nx * (double)nx);
    const double inx = 1.0 / (double)nx;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (row_repeated(rows, r)) break;
        for (int o = tid; o < 8 * N; o += kThreads) {
            const int nn = o >> 3, s = o & 7;
            double val = 0;
            if (s < 3) val = -2.0 * (wave_weight(nn, nx) * cov(&red[r][kComp * nn], 3 + s, s) * inv);
            p.nlspec[((size_t)rows[r] * N + nn) * 8 + s] = val;
        }
        if (tid < 8) {
            double val = 0;
            if (tid < 3) {
                double sax = 0, sa = 0, sx = 0;
#pragma unroll
                for (int w = 0; w < kWaves; ++w) { sax += wtot[r][tid][w]; sa += wtot[r][3 + tid][w]; sx += wtot[r][6 + tid][w]; }
                val = -2.0 * (sax * inx - (sa * inx) * (sx * inx));
            }
            p.nltot[(size_t)rows[r] * 8 + tid] = val;
        }
    }
}

}  // namespace

extern "C" int lec_rowspec_nl_ring(const lec_rowspec_nl_args* a) {
    const Refusals R{"lec_rowspec_nl_ring"};
    int rc, nyb;
    long long nrows;
    if (!a) return R.refuse(LEC_ERR_ARG, "null args");
    if ((rc = R.pointers(a, {{a->rows_d, "rows_d"}}, {{a->lattab_d, "lattab_d"}, {a->ptab_d, "ptab_d"}, {a->nlspec_d, "nlspec_d"},
                                                     {a->nltot_d, "nltot_d"}})) != LEC_OK) return rc;
    if ((rc = R.dtype(a)) != LEC_OK) return rc;
    if (a->nt < 1) return R.refuse(LEC_ERR_ARG, "nt must be >= 1");
    if (a->nl < 1 || a->ny < 2) return R.refuse(LEC_ERR_ARG, "cube needs nl >= 1, ny >= 2");
    if ((rc = R.ring_steps_band(a)) != LEC_OK) return rc;
    if (a->jn == a->js) return R.refuse(LEC_ERR_ARG, "jn must be > js (a band needs two rows for d/dlat)");
    if ((rc = R.wavenumbers(a)) != LEC_OK) return rc;
    if ((rc = R.aligned(a->rows_d, 16, "rows_d")) != LEC_OK) return rc;
    if ((rc = R.aligned(a->nlspec_d, 16, "nlspec_d")) != LEC_OK) return rc;
    if ((rc = R.aligned(a->nltot_d, 16, "nltot_d")) != LEC_OK) return rc;
    if ((rc = R.aligned(a->lattab_d, 8, "lattab_d")) != LEC_OK) return rc;
    if ((rc = R.aligned(a->ptab_d, 8, "ptab_d")) != LEC_OK) return rc;
    if ((rc = R.cubes_rows(a, &nyb, &nrows)) != LEC_OK) return rc;

    SpecNlParams p;
    common_params(p, a, nyb);
    p.rows = a->rows_d; p.lattab = a->lattab_d; p.ptab = a->ptab_d;
    p.nlspec = a->nlspec_d; p.nltot = a->nltot_d; p.inv_hdeg = a->inv_hdeg;
    hipStream_t st = (hipStream_t)a->stream;
    return R.launched(a->dtype == LEC_F64 ? launch(lec_rowspec_nl_kernel<double, kRows, true>, lec_rowspec_nl_kernel<double, kRows, false>, kRows, p, nrows, st)
                                          : launch(lec_rowspec_nl_kernel<float, kRows, true>, lec_rowspec_nl_kernel<float, kRows, false>, kRows, p, nrows, st));
}
