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
// The kernel is lec_rowspec_nl_kernel (lec_rowspec_nl.hip) with another staging phase: 256 threads per (time, level, latitude) row, thread
// tid on wavenumber n = 1 + tid % N and the columns i = seg, seg + nseg, ... (seg = tid / N, nseg = 256 / N), the twiddle {cos, sin}(2 pi m /
// nx) read from the host-built table with m = (n i) mod nx carried as an integer, the column classes of a wavenumber summed in a fixed
// order.  Per trip of kChunk columns every thread loads T, u, v, w at its columns (four loads per column: no neighbour row, no derivative)
// and stores nine doubles per column: {T', u'} {v', w T'} {w u', w v'} {v T', v u'} as double2 arrays and v v' as a double array (16-byte
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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lec_hip.h"
#include "lec_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 576;            // columns staged per trip: 40.5 KiB of LDS, all of it reused by the partial sums
constexpr int kComp = 18;              // {T', u', v', w T', w u', w v', v T', v u', v v'} x {cos, sin}
constexpr int kCompInner = 12;         // a row that is no wall: the first six fields
// the twiddle table in LDS: lec_rowspec_kernel's thresholds
constexpr int kTwidLdsMinWave = 16;
constexpr int kTwidLdsMaxRow = 4096;
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
    const int nx = p.nx;
    const int jb = (int)(row % p.nyb);
    const int k = (int)((row / p.nyb) % p.nl);
    const int t = p.t_begin + (int)(row / ((long long)p.nyb * p.nl));
    const size_t plane = (size_t)p.ny * nx, cube = plane * p.nl;
    const size_t base = (size_t)t * cube + (size_t)k * plane + (size_t)(p.js + jb) * nx;
    const E* __restrict__ rT = (const E*)p.T + base;
    const E* __restrict__ rU = (const E*)p.U + base;
    const E* __restrict__ rV = (const E*)p.V + base;
    const E* __restrict__ rW = (const E*)p.W + base;
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
__global__ __launch_bounds__(kThreads) void lec_rowspec_b_kernel(const SpecBParams p) {
    __shared__ __attribute__((aligned(16))) double2 fld[4][kChunk];
    __shared__ double fe[kChunk];
    __shared__ double red[LEC_MAX_WAVENUMBERS * kComp];
    extern __shared__ __attribute__((aligned(16))) double2 twl[];      // TWLDS: [nx]
    const int tid = threadIdx.x;
    const int N = p.n_wave, nx = p.nx;
    const long long row = blockIdx.x;
    const int jb = (int)(row % p.nyb);
    const bool wall = jb == 0 || jb == p.nyb - 1;  // the rows whose VTT and EV stage 2 reads; the same for every thread of the workgroup
    if (TWLDS)
        for (int c = tid; c < nx; c += kThreads) twl[c] = p.twid[c];       // (the first trip's barrier publishes it)

    const int nseg = kThreads / N;
    const bool active = tid < nseg * N;
    const int n = 1 + tid % N, seg = tid / N;
    int i = seg;                                   // this thread's next column
    int m = (int)(((long long)n * seg) % nx);      // (n i) mod nx, an integer throughout
    const int dm = (n * nseg) % nx;
    double acc[kComp];
#pragma unroll
    for (int q = 0; q < kComp; ++q) acc[q] = 0;

    for (int c0 = 0; c0 < nx; c0 += kChunk) {
        const int cn = min(kChunk, nx - c0);
        if (c0) __syncthreads();                   // the trip before has been read
        if (wall) stage_row<E, true>(p, row, c0, cn, fld[0], fld[1], fld[2], fld[3], fe, tid);
        else stage_row<E, false>(p, row, c0, cn, fld[0], fld[1], fld[2], fld[3], fe, tid);
        __syncthreads();
        if (active) {
            const int cend = c0 + cn;
            if (wall) {
#pragma unroll 2
                for (; i < cend; i += nseg) {
                    const double2 tw = TWLDS ? twl[m] : p.twid[m];
                    const double2 a = fld[0][i - c0], b = fld[1][i - c0], c = fld[2][i - c0], d = fld[3][i - c0];
                    const double e = fe[i - c0];
                    acc[0] = fma(a.x, tw.x, acc[0]); acc[1] = fma(a.x, tw.y, acc[1]);
                    acc[2] = fma(a.y, tw.x, acc[2]); acc[3] = fma(a.y, tw.y, acc[3]);
                    acc[4] = fma(b.x, tw.x, acc[4]); acc[5] = fma(b.x, tw.y, acc[5]);
                    acc[6] = fma(b.y, tw.x, acc[6]); acc[7] = fma(b.y, tw.y, acc[7]);
                    acc[8] = fma(c.x, tw.x, acc[8]); acc[9] = fma(c.x, tw.y, acc[9]);
                    acc[10] = fma(c.y, tw.x, acc[10]); acc[11] = fma(c.y, tw.y, acc[11]);
                    acc[12] = fma(d.x, tw.x, acc[12]); acc[13] = fma(d.x, tw.y, acc[13]);
                    acc[14] = fma(d.y, tw.x, acc[14]); acc[15] = fma(d.y, tw.y, acc[15]);
                    acc[16] = fma(e, tw.x, acc[16]); acc[17] = fma(e, tw.y, acc[17]);
                    m += dm;
                    if (m >= nx) m -= nx;
                }
            } else {
#pragma unroll 2
                for (; i < cend; i += nseg) {
                    const double2 tw = TWLDS ? twl[m] : p.twid[m];
                    const double2 a = fld[0][i - c0], b = fld[1][i - c0], c = fld[2][i - c0];
                    acc[0] = fma(a.x, tw.x, acc[0]); acc[1] = fma(a.x, tw.y, acc[1]);
                    acc[2] = fma(a.y, tw.x, acc[2]); acc[3] = fma(a.y, tw.y, acc[3]);
                    acc[4] = fma(b.x, tw.x, acc[4]); acc[5] = fma(b.x, tw.y, acc[5]);
                    acc[6] = fma(b.y, tw.x, acc[6]); acc[7] = fma(b.y, tw.y, acc[7]);
                    acc[8] = fma(c.x, tw.x, acc[8]); acc[9] = fma(c.x, tw.y, acc[9]);
                    acc[10] = fma(c.y, tw.x, acc[10]); acc[11] = fma(c.y, tw.y, acc[11]);
                    m += dm;
                    if (m >= nx) m -= nx;
                }
            }
        }
    }
    double* const part = (double*)&fld[0][0];       // partial sums [seg][wavenumber][18]: tid = seg N + (n - 1)
    const int ncomp = wall ? kComp : kCompInner;    // (an interior row's last six are 0 and are not summed)
    __syncthreads();                                // the last trip has been read
    if (active) {
#pragma unroll
        for (int q = 0; q < kComp; ++q) part[kComp * tid + q] = acc[q];
    }
    __syncthreads();
    for (int o = tid; o < kComp * N; o += kThreads) {      // one sum per (wavenumber, component), the column classes in their order
        double s = 0;
        if (o % kComp < ncomp)
            for (int g = 0; g < nseg; ++g) s += part[kComp * g * N + o];
        red[o] = s;
    }
    __syncthreads();
    // C_n(P, x) = w_n Re(P^_n conj(x^_n)) / nx^2 with the coefficients as {cos, sin} sums: components 0 T, 2 u, 4 v, 6 wT', 8 wu', 10 wv',
    // 12 vT', 14 vu', 16 vv'.  slot 0 VTT, 1 WTT, 2 EV, 3 EW
    const double inv = 1.0 / ((double)nx * (double)nx);
    for (int o = tid; o < 4 * N; o += kThreads) {
        const int nn = o >> 2, s = o & 3;
        const double* q = &red[kComp * nn];
        const double wgt = (2 * (nn + 1) == nx) ? 1.0 : 2.0;      // the Nyquist wavenumber of an even ring counts once
        double val = 0.0;
        if (s == 1) val = wgt * (q[6] * q[0] + q[7] * q[1]) * inv;
        else if (s == 3) val = wgt * ((q[8] * q[2] + q[9] * q[3]) + (q[10] * q[4] + q[11] * q[5])) * inv;
        else if (wall && s == 0) val = wgt * (q[12] * q[0] + q[13] * q[1]) * inv;
        else if (wall) val = wgt * ((q[14] * q[2] + q[15] * q[3]) + (q[16] * q[4] + q[17] * q[5])) * inv;
        p.bspec[((size_t)row * N + nn) * 4 + s] = val;
    }
}

template <typename E>
int launch(const SpecBParams& p, long long nrows, hipStream_t st) {
    const unsigned nb = (unsigned)nrows;
    if (p.n_wave >= kTwidLdsMinWave && p.nx <= kTwidLdsMaxRow) {
        const size_t lds = (size_t)p.nx * sizeof(double2);
        // (more than 64 KiB of LDS per workgroup, static and dynamic together, has to be asked for)
        if (hipFuncSetAttribute((const void*)lec_rowspec_b_kernel<E, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return LEC_ERR_LAUNCH;
        hipLaunchKernelGGL((lec_rowspec_b_kernel<E, true>), dim3(nb), dim3(kThreads), lds, st, p);
    } else {
        hipLaunchKernelGGL((lec_rowspec_b_kernel<E, false>), dim3(nb), dim3(kThreads), 0, st, p);
    }
    return LEC_OK;
}

}  // namespace

extern "C" int lec_rowspec_b_ring(const lec_rowspec_b_args* a) {
    if (!a) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: null args");
    if (!a->tair_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: null tair_d");
    if (!a->u_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: null u_d");
    if (!a->v_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: null v_d");
    if (!a->omega_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: null omega_d");
    if (!a->rows_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: null rows_d");
    if (!a->twid_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: null twid_d");
    if (!a->bspec_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: null bspec_d");
    if (a->dtype != LEC_F64 && a->dtype != LEC_F32) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: dtype must be LEC_F64 or LEC_F32");
    if (a->nt < 1) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: nt must be >= 1");
    if (a->nl < 1 || a->ny < 2) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: cube needs nl >= 1, ny >= 2");
    if (a->nx < 3) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: nx must be >= 3 (a ring has at least 3 columns)");
    if (a->t_begin < 0 || a->t_begin >= a->nt) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: t_begin outside the cube");
    if (a->t_count < 1 || a->t_count > a->nt - a->t_begin) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: t_count: [t_begin, t_begin + t_count) outside the cube");
    if (a->js < 0 || a->js >= a->ny) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: js outside the cube's latitudes");
    if (a->jn < a->js || a->jn >= a->ny) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: jn must be js .. ny - 1");
    if (a->jn == a->js) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: jn must be > js (a band has a south and a north wall row)");
    if (a->n_wave < 1) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: n_wave must be >= 1");
    if (a->n_wave > a->nx / 2) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: n_wave must be <= nx / 2 (a ring of nx columns holds the wavenumbers 1 .. nx / 2)");
    if (a->n_wave > LEC_MAX_WAVENUMBERS) return lec_set_error(LEC_ERR_UNSUPPORTED, "lec_rowspec_b_ring: n_wave above LEC_MAX_WAVENUMBERS");
    if ((uintptr_t)a->twid_d % 16) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: twid_d must be 16-byte aligned");
    if ((uintptr_t)a->rows_d % 16) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: rows_d must be 16-byte aligned");
    if ((uintptr_t)a->bspec_d % 16) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: bspec_d must be 16-byte aligned");
    const size_t esz = a->dtype == LEC_F32 ? 4 : 8;
    const void* cubes[4] = {a->tair_d, a->u_d, a->v_d, a->omega_d};
    for (const void* c : cubes)
        if ((uintptr_t)c % esz) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_b_ring: cube pointer (tair_d, u_d, v_d, omega_d) not aligned to its element size");
    const int nyb = a->jn - a->js + 1;
    const long long nrows = (long long)a->t_count * a->nl * nyb;
    if (nrows > 0x7fffffffLL) return lec_set_error(LEC_ERR_UNSUPPORTED, "lec_rowspec_b_ring: more than 2^31-1 rows in one call");

    SpecBParams p;
    p.T = a->tair_d; p.U = a->u_d; p.V = a->v_d; p.W = a->omega_d;
    p.rows = a->rows_d; p.twid = (const double2*)a->twid_d; p.bspec = a->bspec_d;
    p.nl = a->nl; p.ny = a->ny; p.nx = a->nx; p.t_begin = a->t_begin; p.js = a->js; p.nyb = nyb; p.n_wave = a->n_wave;
    hipStream_t st = (hipStream_t)a->stream;
    const int rc = a->dtype == LEC_F64 ? launch<double>(p, nrows, st) : launch<float>(p, nrows, st);
    if (rc != LEC_OK) return lec_set_error(rc, "lec_rowspec_b_ring: the kernel's LDS could not be reserved");
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}
