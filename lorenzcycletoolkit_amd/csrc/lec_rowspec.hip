// lec_rowspec.hip -- lec_rowspec_ring: the zonal-wavenumber shares of the eight eddy covariances of every ring row (-f --periodic
// --wavenumbers; include/lec_hip.h).  A translation unit of its own: its code object is loaded by spectral calls only.
//
// One workgroup of 256 threads per kRows = 2 neighbouring (time, level, latitude) rows.  Thread tid serves wavenumber n = 1 + tid % N on
// the columns i = seg, seg + nseg, seg + 2 nseg, ... with seg = tid / N and nseg = 256 / N column classes (N = n_wave <= 64, so
// nseg >= 4; the 256 - nseg N threads left over stage data and take part in the barriers only).  The rows are staged in LDS in trips of
// kChunk columns as fp64 {T, u, v, w} minus the row's column 0, so a lane reads a row's column with two 16-byte LDS loads -- lanes of
// one column class read one address (a broadcast), neighbouring classes neighbouring columns (other banks) -- and the twiddle
// {cos, sin}(2 pi m / nx) with one 16-byte load from the host-built table, m = (n i) mod nx carried as an integer (m += (n nseg) mod nx,
// one conditional subtraction).  One twiddle serves both rows: 16 fp64 FMAs per 80 bytes of operands.  The table itself is copied to
// LDS first when that pays (TWLDS); it holds the same values, read in the same order.  The column classes of a wavenumber are summed in
// class order through LDS, so a row's record depends on (nx, N) and on nothing else -- not on the launch, the row's partner or TWLDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lec_hip.h"
#include "lec_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 2;               // rows per workgroup: one twiddle load feeds both (1, 3 and 4 measured slower)
constexpr int kChunk = 512;            // columns staged per trip: 16 KiB of LDS per row, which the 256 x 8 partial sums reuse afterwards
// the twiddle table in LDS: worth its staging once a workgroup serves 16 wavenumbers or more (measured), possible while the table fits
// beside the rows
constexpr int kTwidLdsMinWave = 16;
constexpr int kTwidLdsMaxRow = 4096;

struct SpecParams {
    const void *T, *U, *V, *W;
    const double2* twid;               // [nx] {cos, sin}(2 pi m / nx)
    double* spec;                      // [t_count][nl][nyb][n_wave][8]
    int nl, ny, nx, t_begin, js, nyb, n_wave;
};

template <typename E, int R, bool TWLDS>
__global__ __launch_bounds__(kThreads) void lec_rowspec_kernel(const SpecParams p, const long long nrows) {
    __shared__ __attribute__((aligned(16))) double fld[R][kChunk * 4];
    __shared__ double red[R][LEC_MAX_WAVENUMBERS * 8];
    extern __shared__ __attribute__((aligned(16))) double2 twl[];      // TWLDS: [nx]
    const int tid = threadIdx.x;
    const int N = p.n_wave, nx = p.nx;
    const E* T[R]; const E* U[R]; const E* V[R]; const E* W[R];
    double t0[R], u0[R], v0[R], w0[R];
    long long rows[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        long long row = (long long)blockIdx.x * R + r;
        if (row >= nrows) row = nrows - 1;         // the last workgroup of an odd count: the row once more, written once
        rows[r] = row;
        const int j = (int)(row % p.nyb);
        const int k = (int)((row / p.nyb) % p.nl);
        const long long t = row / ((long long)p.nyb * p.nl);
        const size_t base = ((((size_t)(p.t_begin + t)) * p.nl + k) * p.ny + (p.js + j)) * (size_t)nx;
        T[r] = (const E*)p.T + base; U[r] = (const E*)p.U + base; V[r] = (const E*)p.V + base; W[r] = (const E*)p.W + base;
        // the reference value removed before projecting (T is ~288 K with eddies of ~1 K): the row's column 0; a constant has no share in n >= 1
        t0[r] = (double)T[r][0]; u0[r] = (double)U[r][0]; v0[r] = (double)V[r][0]; w0[r] = (double)W[r][0];
    }
    if (TWLDS)
        for (int c = tid; c < nx; c += kThreads) twl[c] = p.twid[c];       // (the first trip's barrier publishes it)

    const int nseg = kThreads / N;
    const bool active = tid < nseg * N;
    const int n = 1 + tid % N, seg = tid / N;
    int i = seg;                                   // this thread's next column
    int m = (n * seg) % nx;                        // (n i) mod nx, an integer throughout
    const int dm = (n * nseg) % nx;
    double acc[R][8];                              // {T, u, v, w} x {cos, sin} sums
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[r][q] = 0;

    for (int c0 = 0; c0 < nx; c0 += kChunk) {
        const int cn = min(kChunk, nx - c0);
        if (c0) __syncthreads();                   // the trip before has been read
#pragma unroll
        for (int r = 0; r < R; ++r)
            for (int c = tid; c < cn; c += kThreads) {
                double2* d = (double2*)&fld[r][4 * c];
                d[0] = make_double2((double)T[r][c0 + c] - t0[r], (double)U[r][c0 + c] - u0[r]);
                d[1] = make_double2((double)V[r][c0 + c] - v0[r], (double)W[r][c0 + c] - w0[r]);
            }
        __syncthreads();
        if (active) {
            const int cend = c0 + cn;
#pragma unroll 2
            for (; i < cend; i += nseg) {
                const double2 tw = TWLDS ? twl[m] : p.twid[m];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double2* f = (const double2*)&fld[r][4 * (i - c0)];
                    const double2 a = f[0], b = f[1];
                    acc[r][0] = fma(a.x, tw.x, acc[r][0]); acc[r][1] = fma(a.x, tw.y, acc[r][1]);
                    acc[r][2] = fma(a.y, tw.x, acc[r][2]); acc[r][3] = fma(a.y, tw.y, acc[r][3]);
                    acc[r][4] = fma(b.x, tw.x, acc[r][4]); acc[r][5] = fma(b.x, tw.y, acc[r][5]);
                    acc[r][6] = fma(b.y, tw.x, acc[r][6]); acc[r][7] = fma(b.y, tw.y, acc[r][7]);
                }
                m += dm;
                if (m >= nx) m -= nx;
            }
        }
    }
    __syncthreads();
    if (active) {                                   // partial sums [seg][wavenumber][8]: tid = seg N + (n - 1)
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < 8; ++q) fld[r][8 * tid + q] = acc[r][q];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r)
        for (int o = tid; o < 8 * N; o += kThreads) {  // one sum per (wavenumber, component), the column classes in their order
            double s = 0;
            for (int g = 0; g < nseg; ++g) s += fld[r][8 * g * N + o];
            red[r][o] = s;
        }
    __syncthreads();
    // the eight shares in slot order LEC_S_TT .. LEC_S_WV: {T, u, v, w} = components {0, 1, 2, 3}
    const double inv = 1.0 / ((double)nx * (double)nx);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r && rows[r] == rows[r - 1]) break;
        for (int o = tid; o < 8 * N; o += kThreads) {
            const int nn = o >> 3, s = o & 7;
            const int fa = (0x33132210 >> (4 * s)) & 15;     // first factor of slots 0 .. 7:  T u v v w u w w (a hex digit per slot, slot 0 lowest)
            const int fb = (0x21200210 >> (4 * s)) & 15;     // second factor:                 T u v T T v u v
            const double* q = &red[r][8 * nn];
            const double wgt = (2 * (nn + 1) == nx) ? 1.0 : 2.0;      // the Nyquist wavenumber of an even ring counts once
            p.spec[((size_t)rows[r] * N + nn) * 8 + s] = wgt * (q[2 * fa] * q[2 * fb] + q[2 * fa + 1] * q[2 * fb + 1]) * inv;
        }
    }
}

template <typename E>
int launch(const SpecParams& p, long long nrows, hipStream_t st) {
    const unsigned nb = (unsigned)((nrows + kRows - 1) / kRows);
    if (p.n_wave >= kTwidLdsMinWave && p.nx <= kTwidLdsMaxRow) {
        const size_t lds = (size_t)p.nx * sizeof(double2);
        // (more than 64 KiB of LDS per workgroup, static and dynamic together, has to be asked for)
        if (hipFuncSetAttribute((const void*)lec_rowspec_kernel<E, kRows, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return LEC_ERR_LAUNCH;
        hipLaunchKernelGGL((lec_rowspec_kernel<E, kRows, true>), dim3(nb), dim3(kThreads), lds, st, p, nrows);
    } else {
        hipLaunchKernelGGL((lec_rowspec_kernel<E, kRows, false>), dim3(nb), dim3(kThreads), 0, st, p, nrows);
    }
    return LEC_OK;
}

}  // namespace

extern "C" int lec_rowspec_ring(const lec_rowspec_args* a) {
    if (!a) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: null args");
    if (!a->tair_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: null tair_d");
    if (!a->u_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: null u_d");
    if (!a->v_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: null v_d");
    if (!a->omega_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: null omega_d");
    if (!a->twid_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: null twid_d");
    if (!a->spec_d) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: null spec_d");
    if (a->dtype != LEC_F64 && a->dtype != LEC_F32) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: dtype must be LEC_F64 or LEC_F32");
    if (a->nt < 1 || a->nl < 1 || a->ny < 1) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: cube needs nt >= 1, nl >= 1, ny >= 1");
    if (a->nx < 3) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: nx must be >= 3 (a ring has at least 3 columns)");
    if (a->t_begin < 0 || a->t_begin >= a->nt) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: t_begin outside the cube");
    if (a->t_count < 1 || a->t_count > a->nt - a->t_begin) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: t_count: [t_begin, t_begin + t_count) outside the cube");
    if (a->js < 0 || a->js >= a->ny) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: js outside the cube's latitudes");
    if (a->jn < a->js || a->jn >= a->ny) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: jn must be js .. ny - 1");
    if (a->n_wave < 1) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: n_wave must be >= 1");
    if (a->n_wave > a->nx / 2) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: n_wave must be <= nx / 2 (a ring of nx columns holds the wavenumbers 1 .. nx / 2)");
    if (a->n_wave > LEC_MAX_WAVENUMBERS) return lec_set_error(LEC_ERR_UNSUPPORTED, "lec_rowspec_ring: n_wave above LEC_MAX_WAVENUMBERS");
    if ((uintptr_t)a->twid_d % 16) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: twid_d must be 16-byte aligned");
    if ((uintptr_t)a->spec_d % 16) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: spec_d must be 16-byte aligned");
    const size_t esz = a->dtype == LEC_F32 ? 4 : 8;
    const void* cubes[4] = {a->tair_d, a->u_d, a->v_d, a->omega_d};
    for (const void* c : cubes)
        if ((uintptr_t)c % esz) return lec_set_error(LEC_ERR_ARG, "lec_rowspec_ring: cube pointer (tair_d, u_d, v_d, omega_d) not aligned to its element size");
    const int nyb = a->jn - a->js + 1;
    const long long nrows = (long long)a->t_count * a->nl * nyb;
    if (nrows > 0x7fffffffLL) return lec_set_error(LEC_ERR_UNSUPPORTED, "lec_rowspec_ring: more than 2^31-1 rows in one call");

    SpecParams p;
    p.T = a->tair_d; p.U = a->u_d; p.V = a->v_d; p.W = a->omega_d;
    p.twid = (const double2*)a->twid_d; p.spec = a->spec_d;
    p.nl = a->nl; p.ny = a->ny; p.nx = a->nx; p.t_begin = a->t_begin; p.js = a->js; p.nyb = nyb; p.n_wave = a->n_wave;
    hipStream_t st = (hipStream_t)a->stream;
    const int rc = a->dtype == LEC_F64 ? launch<double>(p, nrows, st) : launch<float>(p, nrows, st);
    if (rc != LEC_OK) return lec_set_error(rc, "lec_rowspec_ring: the kernel's LDS could not be reserved");
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}
