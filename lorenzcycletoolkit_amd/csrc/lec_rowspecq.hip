// lec_rowspecq.hip -- lec_rowspec_q_ring: the zonal-wavenumber shares C_n(Q, T) of the generation covariance [Q'T'] of every ring row
// (-f --periodic --wavenumbers N --wavenumbers-generation; include/lec_hip.h).  A translation unit of its own: its
// code object is loaded by calls that ask for Ge(n) only.
//
// The workgroup, the lane mapping, the twiddle table and the fixed-order sum over the column classes are lec_rowspec_kernel's
// (lec_rowspec.hip): 256 threads per kRows neighbouring (time, level, latitude) rows, thread tid on wavenumber n = 1 + tid % N and the
// columns i = seg, seg + nseg, ... (seg = tid / N, nseg = 256 / N), the twiddle {cos, sin}(2 pi m / nx) read from the host-built table
// with m = (n i) mod nx carried as an integer.  What differs is the staging phase: it is the stencil of the diabatic-heating residual.
// Per trip of kChunk columns every thread forms Q / cp = dT/dt + u dT/dx + v dT/dy - S w of its columns from the row itself, its six
// neighbour rows in time, pressure and latitude (the row itself with coefficient 0 where a neighbour does not exist: nothing outside the
// band, the levels or the cube's steps is read) and u, v, w -- the expressions of sweep_one (lec_sweep.h) with the per-point dT/dt of its
// QMODE 1 -- and stores {T - T(column 0), Q / cp} as one double2.  The lambda neighbours are read from memory at wrapped column indices,
// so neither the ring's seam nor a trip's is a special case.  The projection then costs 4 fp64 FMAs per (row, column, n) and twiddle.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lec_hip.h"
#include "lec_internal.h"
#include "lec_sweep.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 2;               // rows per workgroup: one twiddle load feeds both (1 and 4 measured: 4 wins at N = 8 and 64, loses at 20)
constexpr int kChunk = 512;            // columns staged per trip: 8 KiB of LDS per row, which the 256 x 4 partial sums reuse afterwards
// the twiddle table in LDS: lec_rowspec_kernel's thresholds (its staging pays once a workgroup serves 16 wavenumbers or more, and it
// fits beside the rows up to 4096 columns)
constexpr int kTwidLdsMinWave = 16;
constexpr int kTwidLdsMaxRow = 4096;

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
    const int jb = (int)(row % p.nyb);
    const int k = (int)((row / p.nyb) % p.nl);
    const int t = p.t_begin + (int)(row / ((long long)p.nyb * p.nl));
    const size_t plane = (size_t)p.ny * nx, cube = plane * p.nl;
    const size_t base = (size_t)t * cube + (size_t)k * plane + (size_t)(p.js + jb) * nx;
    const E* __restrict__ rT = (const E*)p.T + base;
    const E* __restrict__ rU = (const E*)p.U + base;
    const E* __restrict__ rV = (const E*)p.V + base;
    const E* __restrict__ rW = (const E*)p.W + base;
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
    __shared__ double red[R][LEC_MAX_WAVENUMBERS * 4];
    extern __shared__ __attribute__((aligned(16))) double2 twl[];      // TWLDS: [nx]
    const int tid = threadIdx.x;
    const int N = p.n_wave, nx = p.nx;
    long long rows[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long row = (long long)blockIdx.x * R + r;
        rows[r] = row < nrows ? row : nrows - 1;   // the last workgroup of a count R does not divide: the last row once more, written once
    }
    if (TWLDS)
        for (int c = tid; c < nx; c += kThreads) twl[c] = p.twid[c];       // (the first trip's barrier publishes it)

    const int nseg = kThreads / N;
    const bool active = tid < nseg * N;
    const int n = 1 + tid % N, seg = tid / N;
    int i = seg;                                   // this thread's next column
    int m = (int)(((long long)n * seg) % nx);      // (n i) mod nx, an integer throughout
    const int dm = (n * nseg) % nx;
    double acc[R][4];                              // {T, Q / cp} x {cos, sin} sums
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[r][q] = 0;

    for (int c0 = 0; c0 < nx; c0 += kChunk) {
        const int cn = min(kChunk, nx - c0);
        if (c0) __syncthreads();                   // the trip before has been read
#pragma unroll
        for (int r = 0; r < R; ++r) stage_row<E>(p, rows[r], c0, cn, (double2*)fld[r], tid);
        __syncthreads();
        if (active) {
            const int cend = c0 + cn;
#pragma unroll 2
            for (; i < cend; i += nseg) {
                const double2 tw = TWLDS ? twl[m] : p.twid[m];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double2 a = ((const double2*)fld[r])[i - c0];
                    acc[r][0] = fma(a.x, tw.x, acc[r][0]); acc[r][1] = fma(a.x, tw.y, acc[r][1]);
                    acc[r][2] = fma(a.y, tw.x, acc[r][2]); acc[r][3] = fma(a.y, tw.y, acc[r][3]);
                }
                m += dm;
                if (m >= nx) m -= nx;
            }
        }
    }
    __syncthreads();
    if (active) {                                   // partial sums [seg][wavenumber][4]: tid = seg N + (n - 1)
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) fld[r][4 * tid + q] = acc[r][q];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r)
        for (int o = tid; o < 4 * N; o += kThreads) {  // one sum per (wavenumber, component), the column classes in their order
            double s = 0;
            for (int g = 0; g < nseg; ++g) s += fld[r][4 * g * N + o];
            red[r][o] = s;
        }
    __syncthreads();
    // C_n(Q, T) = w_n Re(Q^_n conj(T^_n)), Q = cp f
    const double inv = lec::kCp / ((double)nx * (double)nx);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r && rows[r] == rows[r - 1]) break;
        for (int nn = tid; nn < N; nn += kThreads) {
            const double* q = &red[r][4 * nn];
            const double wgt = (2 * (nn + 1) == nx) ? 1.0 : 2.0;      // the Nyquist wavenumber of an even ring counts once
            p.qspec[(size_t)rows[r] * N + nn] = wgt * (q[2] * q[0] + q[3] * q[1]) * inv;
        }
    }
}

template <typename E>
int launch(const SpecQParams& p, long long nrows, hipStream_t st) {
    const unsigned nb = (unsigned)((nrows + kRows - 1) / kRows);
    if (p.n_wave >= kTwidLdsMinWave && p.nx <= kTwidLdsMaxRow) {
        const size_t lds = (size_t)p.nx * sizeof(double2);
        // (more than 64 KiB of LDS per workgroup, static and dynamic together, has to be asked for)
        if (hipFuncSetAttribute((const void*)lec_rowspec_q_kernel<E, kRows, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return LEC_ERR_LAUNCH;
        hipLaunchKernelGGL((lec_rowspec_q_kernel<E, kRows, true>), dim3(nb), dim3(kThreads), lds, st, p, nrows);
    } else {
        hipLaunchKernelGGL((lec_rowspec_q_kernel<E, kRows, false>), dim3(nb), dim3(kThreads), 0, st, p, nrows);
    }
    return LEC_OK;
}

}  // namespace

extern "C" int lec_rowspec_q_ring(const lec_rowspec_q_args* a) {
    if (!a) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: null args");
    if (!a->tair_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: null tair_d");
    if (!a->u_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: null u_d");
    if (!a->v_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: null v_d");
    if (!a->omega_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: null omega_d");
    if (!a->twid_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: null twid_d");
    if (!a->lattab_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: null lattab_d");
    if (!a->levtab_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: null levtab_d");
    if (!a->tcoef_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: null tcoef_d (a dT/dt cube is not supported: dT/dt comes from the cube's time axis)");
    if (!a->qspec_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: null qspec_d");
    if (a->dtype != LEC_F64 && a->dtype != LEC_F32) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: dtype must be LEC_F64 or LEC_F32");
    if (a->nt < 2) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: nt must be >= 2 (dT/dt by finite differences over the cube's time axis)");
    if (a->nl < 1 || a->ny < 2) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: cube needs nl >= 1, ny >= 2");
    if (a->nx < 3) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: nx must be >= 3 (a ring has at least 3 columns)");
    if (a->t_begin < 0 || a->t_begin >= a->nt) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: t_begin outside the cube");
    if (a->t_count < 1 || a->t_count > a->nt - a->t_begin) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: t_count: [t_begin, t_begin + t_count) outside the cube");
    if (a->js < 0 || a->js >= a->ny) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: js outside the cube's latitudes");
    if (a->jn < a->js || a->jn >= a->ny) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: jn must be js .. ny - 1");
    // (lec_rowstats_ring refuses a one-row band too: its box extents must be 2..ny rows)
    if (a->jn == a->js) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: jn must be > js (a band needs two rows for d/dlat)");
    if (a->n_wave < 1) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: n_wave must be >= 1");
    if (a->n_wave > a->nx / 2) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: n_wave must be <= nx / 2 (a ring of nx columns holds the wavenumbers 1 .. nx / 2)");
    if (a->n_wave > LEC_MAX_WAVENUMBERS) return lec_set_error(LEC_ERR_UNSUPPORTED, "lec_rowspec_q_ring: n_wave above LEC_MAX_WAVENUMBERS");
    if ((uintptr_t)a->twid_d % 16) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: twid_d must be 16-byte aligned");
    if ((uintptr_t)a->qspec_d % 16) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: qspec_d must be 16-byte aligned");
    if ((uintptr_t)a->lattab_d % 8) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: lattab_d must be 8-byte aligned");
    if ((uintptr_t)a->levtab_d % 8) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: levtab_d must be 8-byte aligned");
    if ((uintptr_t)a->tcoef_d % 8) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: tcoef_d must be 8-byte aligned");
    const size_t esz = a->dtype == LEC_F32 ? 4 : 8;
    const void* cubes[4] = {a->tair_d, a->u_d, a->v_d, a->omega_d};
    for (const void* c : cubes)
        if ((uintptr_t)c % esz) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_q_ring: cube pointer (tair_d, u_d, v_d, omega_d) not aligned to its element size");
    const int nyb = a->jn - a->js + 1;
    const long long nrows = (long long)a->t_count * a->nl * nyb;
    if (nrows > 0x7fffffffLL) return lec_set_error(LEC_ERR_UNSUPPORTED, "lec_rowspec_q_ring: more than 2^31-1 rows in one call");

    SpecQParams p;
    p.T = a->tair_d; p.U = a->u_d; p.V = a->v_d; p.W = a->omega_d;
    p.twid = (const double2*)a->twid_d; p.lattab = a->lattab_d; p.levtab = a->levtab_d; p.tcoef = a->tcoef_d;
    p.qspec = a->qspec_d; p.inv_hdeg = a->inv_hdeg;
    p.nt = a->nt; p.nl = a->nl; p.ny = a->ny; p.nx = a->nx; p.t_begin = a->t_begin; p.js = a->js; p.nyb = nyb; p.n_wave = a->n_wave;
    hipStream_t st = (hipStream_t)a->stream;
    const int rc = a->dtype == LEC_F64 ? launch<double>(p, nrows, st) : launch<float>(p, nrows, st);
    if (rc != LEC_OK) return lec_set_error(rc, "lec_rowspec_q_ring: the kernel's LDS could not be reserved");
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}
