// lec_rowspec_core.h -- what the four zonal-wavenumber passes of -f --periodic --wavenumbers share: lec_rowspec_ring (lec_rowspec.hip),
// lec_rowspec_q_ring (lec_rowspecq.hip), lec_rowspec_nl_ring (lec_rowspec_nl.hip) and lec_rowspec_b_ring (lec_rowspec_b.hip); DESIGN.md
// section 4.2b.  A member stages NF fields of its R rows in LDS, kChunk columns per trip, in a layout of its own; everything that
// projects them on the wavenumbers 1 .. N is written once, here:
//
// One workgroup of kThreads = 256 threads per R (time, level, latitude) rows.  Thread tid serves wavenumber n = 1 + tid % N on the
// columns i = seg, seg + nseg, seg + 2 nseg, ... with seg = tid / N and nseg = 256 / N column classes (N = n_wave <= 64, so nseg >= 4;
// the 256 - nseg N threads left over stage data and take part in the barriers only).  The twiddle {cos, sin}(2 pi m / nx) is one 16-byte
// load from the host-built table, m = (n i) mod nx carried as an integer (m += (n nseg) mod nx, one conditional subtraction), and serves
// all R rows: 2 NF fp64 FMAs per row.  The table itself is copied to LDS first when that pays (TWLDS); it holds the same values, read in
// the same order.  The column classes of a wavenumber are summed in class order through LDS, so a row's record depends on (nx, N) and
// on nothing else -- not on the launch, the row's partners or TWLDS.  The streamed, chunked and fused paths assert bit equality on that.
//
// The device pieces are __forceinline__ templates over values the compiler sees as constants: they are inlined before anything is
// optimised, so the loops of a member's kernel are the instructions they were with the pieces spelled out in it (registers, LDS and
// the comparison of the loops: DESIGN.md section 4.2b).  The kernels stay in the members' files: four translation units, four code
// objects, and a spectral call loads only what it uses.
#pragma once
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>

#include "../../include/lec_hip.h"
#include "lec_internal.h"

namespace lec {
namespace spec {

constexpr int kThreads = 256;
// the twiddle table in LDS: worth its staging once a workgroup serves 16 wavenumbers or more (measured), possible while the table fits
// beside the rows
constexpr int kTwidLdsMinWave = 16;
constexpr int kTwidLdsMaxRow = 4096;

// a workgroup's R rows; the last workgroup of a count R does not divide takes the last row once more
template <int R>
__device__ __forceinline__ void wg_rows(const long long nrows, long long (&rows)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long row = (long long)blockIdx.x * R + r;
        rows[r] = row < nrows ? row : nrows - 1;
    }
}
// ... and writes it once
template <int R>
__device__ __forceinline__ bool row_repeated(const long long (&rows)[R], const int r) { return r && rows[r] == rows[r - 1]; }

// a row of the call's band in the cubes: its step, level and band row, its first element in the four cubes.  P: a member's parameter
// struct (T U V W nl ny nx t_begin js nyb)
template <typename E>
struct Row {
    int t, k, jb;
    size_t plane, cube;                // elements from a row to the next level's, to the next step's
    const E *T, *U, *V, *W;
};
template <typename E, typename P>
__device__ __forceinline__ Row<E> decode_row(const P& p, const long long row) {
    Row<E> r;
    r.jb = (int)(row % p.nyb);
    r.k = (int)((row / p.nyb) % p.nl);
    r.t = p.t_begin + (int)(row / ((long long)p.nyb * p.nl));
    r.plane = (size_t)p.ny * p.nx;
    r.cube = r.plane * p.nl;
    const size_t base = (size_t)r.t * r.cube + (size_t)r.k * r.plane + (size_t)(p.js + r.jb) * p.nx;
    r.T = (const E*)p.T + base; r.U = (const E*)p.U + base; r.V = (const E*)p.V + base; r.W = (const E*)p.W + base;
    return r;
}

// a thread's wavenumber, column class, next column and twiddle index
struct Lane {
    int nseg, n, seg;
    bool active;
    int i;                             // this thread's next column
    int m, dm;                         // (n i) mod nx, an integer throughout (n <= 64, seg < 256: the products fit an int)

    __device__ __forceinline__ Lane(const int tid, const int N, const int nx)
        : nseg(kThreads / N), n(1 + tid % N), seg(tid / N), active(tid < nseg * N), i(seg), m((n * seg) % nx), dm((n * nseg) % nx) {}
    __device__ __forceinline__ void next(const int nx) {
        i += nseg;
        m += dm;
        if (m >= nx) m -= nx;
    }
};

// TWLDS: the table to the workgroup's dynamic LDS (the first trip's barrier publishes it)
template <bool TWLDS>
__device__ __forceinline__ void stage_twiddles(const double2* __restrict__ twid, const int nx, const int tid) {
    extern __shared__ __attribute__((aligned(16))) double2 twl[];      // [nx]
    if (TWLDS)
        for (int c = tid; c < nx; c += kThreads) twl[c] = twid[c];
}

// the columns [.., cend) of a trip that began at column c0, NF staged fields of R rows on one twiddle per column: acc[r][2 f] +=
// x_f cos, acc[r][2 f + 1] += x_f sin.  load(r, c, x) returns the NF values of row r at the trip's column c from the member's LDS
// layout.  For the lane's active threads only
template <int NF, bool TWLDS, int R, int NC, typename Load>
__device__ __forceinline__ void project(Lane& l, const int c0, const int cend, const int nx, const double2* __restrict__ twid,
                                        double (&acc)[R][NC], Load load) {
    static_assert(2 * NF <= NC, "a {cos, sin} pair per field");
    extern __shared__ __attribute__((aligned(16))) double2 twl[];      // TWLDS: [nx]
#pragma unroll 2
    for (; l.i < cend; l.next(nx)) {
        const double2 tw = TWLDS ? twl[l.m] : twid[l.m];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double x[NF];
            load(r, l.i - c0, x);
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                acc[r][2 * f] = fma(x[f], tw.x, acc[r][2 * f]);
                acc[r][2 * f + 1] = fma(x[f], tw.y, acc[r][2 * f + 1]);
            }
        }
    }
}

// a row's partial sums to part [seg][wavenumber][NC]: tid = seg N + (n - 1).  Between barriers: the staged columns that part reuses
// have been read, and class_sum follows the next one
template <int NC>
__device__ __forceinline__ void spill(const Lane& l, const int tid, double* part, const double (&acc)[NC]) {
    if (l.active) {
#pragma unroll
        for (int q = 0; q < NC; ++q) part[NC * tid + q] = acc[q];
    }
}
// one sum per (wavenumber, component) to red [wavenumber][NC], the column classes in their order; components from ncomp on are 0
template <int NC>
__device__ __forceinline__ void class_sum(const Lane& l, const int tid, const int N, const double* part, double* red, const int ncomp = NC) {
    for (int o = tid; o < NC * N; o += kThreads) {
        double s = 0;
        if (o % NC < ncomp)
            for (int g = 0; g < l.nseg; ++g) s += part[NC * g * N + o];
        red[o] = s;
    }
}

// w_n: the Nyquist wavenumber of an even ring counts once (nn = n - 1)
__device__ __forceinline__ double wave_weight(const int nn, const int nx) { return (2 * (nn + 1) == nx) ? 1.0 : 2.0; }
// Re(a^_n conj(b^_n)) of the fields a and b of a wavenumber's sums q = &red[NC nn], as {cos, sin} pairs
__device__ __forceinline__ double cov(const double* q, const int a, const int b) { return q[2 * a] * q[2 * b] + q[2 * a + 1] * q[2 * b + 1]; }

// the fields every member's parameter struct P has, from the call's argument struct
template <typename P, typename A>
void common_params(P& p, const A* a, const int nyb) {
    p.T = a->tair_d; p.U = a->u_d; p.V = a->v_d; p.W = a->omega_d;
    p.twid = (const double2*)a->twid_d;
    p.nl = a->nl; p.ny = a->ny; p.nx = a->nx; p.t_begin = a->t_begin; p.js = a->js; p.nyb = nyb; p.n_wave = a->n_wave;
}

// one workgroup per R rows; lds / mem: the member's kernel with the twiddle table in LDS / read from memory.  LEC_OK or LEC_ERR_LAUNCH
template <typename P>
int launch(void (*lds)(P, long long), void (*mem)(P, long long), const int R, const P& p, const long long nrows, hipStream_t st) {
    const unsigned nb = (unsigned)((nrows + R - 1) / R);
    if (p.n_wave >= kTwidLdsMinWave && p.nx <= kTwidLdsMaxRow) {
        const size_t bytes = (size_t)p.nx * sizeof(double2);
        // (more than 64 KiB of LDS per workgroup, static and dynamic together, has to be asked for)
        if (hipFuncSetAttribute((const void*)lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return LEC_ERR_LAUNCH;
        hipLaunchKernelGGL(lds, dim3(nb), dim3(kThreads), bytes, st, p, nrows);
    } else {
        hipLaunchKernelGGL(mem, dim3(nb), dim3(kThreads), 0, st, p, nrows);
    }
    return LEC_OK;
}

// the refusals the four calls have in common, under the call's name.  Each returns LEC_OK or the refusal's code; a call runs them between
// its own, in the order its messages have always come.  A: the call's argument struct, whose common fields are read by name
struct Refusals {
    const char* call;      // "lec_rowspec_ring" ...
    struct Ptr { const void* p; const char* name; };

    int refuse(int code, const char* what) const {
        char msg[320];
        snprintf(msg, sizeof(msg), "%s: %s", call, what);
        return lec_set_error(code, msg);
    }
    int null(const Ptr& q) const {
        char m[160];
        if (q.p) return LEC_OK;
        snprintf(m, sizeof(m), "null %s", q.name);
        return refuse(LEC_ERR_ARG, m);
    }
    int aligned(const void* p, int bytes, const char* name) const {
        char m[96];
        if ((uintptr_t)p % bytes == 0) return LEC_OK;
        snprintf(m, sizeof(m), "%s must be %d-byte aligned", name, bytes);
        return refuse(LEC_ERR_ARG, m);
    }
    // the cubes, the call's pointers that come before twid_d, twid_d, those that come after
    template <typename A>
    int pointers(const A* a, std::initializer_list<Ptr> before, std::initializer_list<Ptr> after) const {
        int rc;
        for (const Ptr& q : {Ptr{a->tair_d, "tair_d"}, Ptr{a->u_d, "u_d"}, Ptr{a->v_d, "v_d"}, Ptr{a->omega_d, "omega_d"}})
            if ((rc = null(q)) != LEC_OK) return rc;
        for (const Ptr& q : before)
            if ((rc = null(q)) != LEC_OK) return rc;
        if ((rc = null({a->twid_d, "twid_d"})) != LEC_OK) return rc;
        for (const Ptr& q : after)
            if ((rc = null(q)) != LEC_OK) return rc;
        return LEC_OK;
    }
    template <typename A>
    int dtype(const A* a) const {
        if (a->dtype != LEC_F64 && a->dtype != LEC_F32) return refuse(LEC_ERR_ARG, "dtype must be LEC_F64 or LEC_F32");
        return LEC_OK;
    }
    template <typename A>
    int ring_steps_band(const A* a) const {
        if (a->nx < 3) return refuse(LEC_ERR_ARG, "nx must be >= 3 (a ring has at least 3 columns)");
        if (a->t_begin < 0 || a->t_begin >= a->nt) return refuse(LEC_ERR_ARG, "t_begin outside the cube");
        if (a->t_count < 1 || a->t_count > a->nt - a->t_begin) return refuse(LEC_ERR_ARG, "t_count: [t_begin, t_begin + t_count) outside the cube");
        if (a->js < 0 || a->js >= a->ny) return refuse(LEC_ERR_ARG, "js outside the cube's latitudes");
        if (a->jn < a->js || a->jn >= a->ny) return refuse(LEC_ERR_ARG, "jn must be js .. ny - 1");
        return LEC_OK;
    }
    template <typename A>
    int wavenumbers(const A* a) const {
        if (a->n_wave < 1) return refuse(LEC_ERR_ARG, "n_wave must be >= 1");
        if (a->n_wave > a->nx / 2) return refuse(LEC_ERR_ARG, "n_wave must be <= nx / 2 (a ring of nx columns holds the wavenumbers 1 .. nx / 2)");
        if (a->n_wave > LEC_MAX_WAVENUMBERS) return refuse(LEC_ERR_UNSUPPORTED, "n_wave above LEC_MAX_WAVENUMBERS");
        return aligned(a->twid_d, 16, "twid_d");
    }
    // the cubes' alignment and the row count of the call: nyb rows per level, nrows in all
    template <typename A>
    int cubes_rows(const A* a, int* nyb, long long* nrows) const {
        const size_t esz = a->dtype == LEC_F32 ? 4 : 8;
        for (const void* c : {a->tair_d, a->u_d, a->v_d, a->omega_d})
            if ((uintptr_t)c % esz) return refuse(LEC_ERR_ARG, "cube pointer (tair_d, u_d, v_d, omega_d) not aligned to its element size");
        *nyb = a->jn - a->js + 1;
        *nrows = (long long)a->t_count * a->nl * *nyb;
        if (*nrows > 0x7fffffffLL) return refuse(LEC_ERR_UNSUPPORTED, "more than 2^31-1 rows in one call");
        return LEC_OK;
    }
    // rc: launch()'s
    int launched(int rc) const {
        if (rc != LEC_OK) return refuse(rc, "the kernel's LDS could not be reserved");
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
        return LEC_OK;
    }
};

}  // namespace spec
}  // namespace lec
