// lec_rowsweep_kernel.h -- the one-wave-per-row kernel template and its launch helpers, shared by the two translation units that
// instantiate it: lec_rowsweep.hip (limited-area rows) and lec_rowsweep_ring.hip (rows that are a closed circle of longitudes).  Each
// unit's code object holds only its own instantiations, so a process that never makes a ring call never loads the ring's kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/lec_hip.h"
#include "lec_internal.h"
#include "lec_rowcommon.h"
#include "lec_sweep.h"

using namespace lec;

namespace {

constexpr int kThreads = 64; // one wave per row: measured best (64 / 128 / 256 threads: 19.0 / 19.1 / 20.1 ms per 64 steps)
// one wave per (time, level, box-latitude) row, ONE sweep over the row (see the header comment)
// MODE: 0 no Q; 1 dT/dt from the cube's time neighbours per point; 2 dT/dt cube; 3 as 1 on one fixed box, through
// cross-time covariances (sweep_elems).  BOTH (MODE 3 only): the row also forms the covariance with T(t-1) -- the first
// processed time step of a launch.  RING: the box's columns are a closed circle of evenly spaced longitudes (lec_rowstats_ring; lec_sweep.h)
template <typename TIN, int VEC, bool UNIFORM, int MODE, bool ONE_TRIP, bool BOTH, bool RING = false>
__global__ void __launch_bounds__(kThreads, (sweep_min_waves<TIN, VEC, MODE>())) lec_rowsweep_kernel(const RowParams p) {
    constexpr int NTHR = kThreads;
    constexpr bool WITH_Q = MODE != 0;
    constexpr bool TIME_NB = (MODE == 1 || MODE == 3);      // reads T at t+1 (and t-1)
    constexpr int nthr = NTHR;
    __shared__ double red[kRound * red_stride(NTHR)];
    __shared__ double tot[24];

    const int tid = threadIdx.x;
    int jb, k, tl;
    if (ONE_TRIP) {
        // short rows are instruction-bound (a 61-point row is ~1000 instructions, a third of them index arithmetic): a 3-D
        // grid hands out (latitude, level, time step) without a single integer division
        jb = (int)(blockIdx.x & 7) * p.jchunk + (int)(blockIdx.x >> 3);      // blockIdx.x % 8 labels the XCD: contiguous latitude chunks
        k = blockIdx.y; tl = blockIdx.z;
        if (jb >= p.nyb_max || (int)(blockIdx.x >> 3) >= p.jchunk) return;
    } else if (p.order == 0) {
        int r = blockIdx.x;
        jb = r % p.nyb_max; r /= p.nyb_max;
        k = r % p.nl;
        tl = r / p.nl;
    } else {
        // XCD label (speed only): every XCD owns a contiguous latitude chunk.  Order 2 walks it latitude-fastest
        // per (time, level).  Order 7 (all terms, fixed box) walks tiles of tgroup time steps x jgroup latitudes
        // at one level, levels next: the ~500 one-wave workgroups resident on an XCD then cover a compact (t, k, j)
        // neighbourhood, so T rows at t+-1 as well as j+-1 / k+-1 are rows a sibling is fetching right now
        // (measured: fabric traffic 1.39 -> 1.29 x algorithmic, -8 % time).
        const int xcd = blockIdx.x & 7;
        int q = blockIdx.x >> 3;
        if (p.order == 7) {
            // tiles of tgroup time steps x jgroup latitudes at one level run together on the XCD, levels next
            const int tile = p.tgroup * p.jgroup;
            int tid_ = q / tile;
            const int within = q - tid_ * tile;
            const int t_in = within % p.tgroup, j_in = within / p.tgroup;
            k = tid_ % p.nl; tid_ /= p.nl;
            const int tgc = (p.t_count + p.tgroup - 1) / p.tgroup;
            const int tg = tid_ % tgc, jg = tid_ / tgc;
            tl = tg * p.tgroup + t_in;
            const int jl = jg * p.jgroup + j_in;
            jb = xcd * p.jchunk + jl;
            if (tl >= p.t_count || jl >= p.jchunk) return;
        } else {
            const int per_t = p.jchunk * p.nl;
            tl = q / per_t; q -= tl * per_t;
            k = q / p.jchunk;
            jb = xcd * p.jchunk + (q - k * p.jchunk);
        }
        if (jb >= p.nyb_max) return;
    }
    const int bi = (p.n_box == 1) ? 0 : tl;
    const int iw = p.box[4 * bi + 0], ie = p.box[4 * bi + 1], js = p.box[4 * bi + 2], jn = p.box[4 * bi + 3];
    const int nxb = ie - iw + 1, nyb = jn - js + 1;
    double* __restrict__ out = p.rows + ((size_t)(tl * p.nl + k) * p.nyb_max + jb) * LEC_NSTAT;
    if (jb >= nyb) {  // padding rows of a box smaller than nyb_max
        if (tid < LEC_NSTAT) out[tid] = 0.0;
        return;
    }
    const int j = js + jb, t = p.t_begin + tl;
    const size_t plane = (size_t)p.ny * p.nx;
    const size_t cube = plane * p.nl;
    const size_t rowoff = (size_t)t * cube + (size_t)k * plane + (size_t)j * p.nx + iw;
    const int shift = (VEC > 1) ? (int)(rowoff % VEC) : 0;
    const int e0_last = ((nxb - 1 + shift) / VEC) * VEC - shift;

    const TIN* __restrict__ rT = (const TIN*)p.T + rowoff;
    const TIN* __restrict__ rU = (const TIN*)p.U + rowoff;
    const TIN* __restrict__ rV = (const TIN*)p.V + rowoff;
    const TIN* __restrict__ rW = (const TIN*)p.W + rowoff;
    const TIN* __restrict__ rP = (const TIN*)(p.P ? p.P : p.T) + rowoff;
    const bool has_p = (MODE != 0) || (p.P != nullptr);

    const double inv_xlen = p.boxtab[4 * bi + 0];
    const double h_rad = p.boxtab[4 * bi + 1];
    const double inv_hdeg = p.boxtab[4 * bi + 2];
    const double* __restrict__ wl = UNIFORM ? nullptr : p.wlon + (size_t)bi * p.nxb_max;
    const double* __restrict__ gl = UNIFORM ? nullptr : p.glon + (size_t)bi * p.nxb_max * 3;

    const TIN *rTjm = rT, *rTjp = rT, *rTkm = rT, *rTkp = rT, *rTtm = rT, *rTtp = rT;
    double ga = 0, gb = 0, gc = 0, inv_dx = 0, al = 0, be = 0, gm = 0, ta = 0, tb = 0, tc = 0;
    if (WITH_Q) {
        if (jb > 0) rTjm = rT - p.nx;
        if (jb < nyb - 1) rTjp = rT + p.nx;
        if (k > 0) rTkm = rT - plane;
        if (k < p.nl - 1) rTkp = rT + plane;
        const double* lt = p.lattab + ((size_t)bi * p.nyb_max + jb) * 4;
        ga = lt[0]; gb = lt[1]; gc = lt[2]; inv_dx = lt[3];
        const double* lv = p.levtab + (size_t)k * 3;
        al = lv[0]; be = lv[1]; gm = lv[2];
        if (MODE == 2) {
            rTtm = (const TIN*)p.DT + rowoff;
        } else {
            if (t > 0) rTtm = rT - cube;
            if (t < p.nt - 1) rTtp = rT + cube;
            if (MODE == 1) {
                const double* tcf = p.tcoef + (size_t)t * 3;
                ta = tcf[0]; tb = tcf[1]; tc = tcf[2];
            }
        }
    }

    // shifts: the row's first box element (wave-uniform scalar loads)
    SweepRow r;
    r.nxb = nxb;
    r.cT = (double)rT[0]; r.cU = (double)rU[0]; r.cV = (double)rV[0]; r.cW = (double)rW[0];
    r.cP = (has_p && p.P) ? (double)rP[0] : 0.0;
    r.cx = 0.5 * inv_hdeg * inv_dx; r.inv_dx = inv_dx; r.wl = wl; r.gl = gl;
    r.cTf = (MODE == 3) ? (double)rTtp[0] : 0.0;
    r.cTb = (MODE == 3 && BOTH) ? (double)rTtm[0] : 0.0;
    // T, u, v at the east box column (boundary terms), fetched now so that the row does not end on a load
    const double eT = (double)rT[nxb - 1], eU = (double)rU[nxb - 1], eV = (double)rV[nxb - 1];
    r.eT = eT;

    double acc[kNA], xacc[kNX];
#pragma unroll
    for (int s = 0; s < kNA; ++s) acc[s] = 0.0;
#pragma unroll
    for (int s = 0; s < kNX; ++s) xacc[s] = 0.0;

    QCoef qc;
    qc.tb_ = ta; qc.tf_ = tc; qc.tm = tb; qc.k0 = al; qc.k1 = gm; qc.km = be; qc.j0 = ga; qc.j1 = gc; qc.jm = gb;

    // one trip = one vector of every row operand per lane; EDGE trips hold a row end or lanes past it.
    // Operands stay in their storage type (TIN) and are converted where they are used.
    auto trip = [&](auto edge_tag, const int it) {
        constexpr bool EDGE = decltype(edge_tag)::value;
        const int el = it * nthr * VEC - shift;              // box element of lane 0 (wave-uniform)
        const int e0 = el + tid * VEC;
        const bool lane_in = !EDGE || (e0 <= e0_last);
        const unsigned eo = (unsigned)((EDGE ? min(e0, e0_last) : e0) + shift);
        TIN fT[VEC], fU[VEC], fV[VEC], fW[VEC], fP[VEC];
        QRaw<TIN, VEC> qr;
        double tl_edge = 0.0, tr_edge = 0.0;
        load_vec<TIN, VEC, MODE == 0>(rT - shift, eo, fT);
        load_vec<TIN, VEC, true>(rU - shift, eo, fU);
        load_vec<TIN, VEC, true>(rV - shift, eo, fV);
        load_vec<TIN, VEC, true>(rW - shift, eo, fW);
        if (has_p) load_vec<TIN, VEC, true>(rP - shift, eo, fP);
        if (!has_p || !p.P) {                                // no geopotential cube: its statistics are written as 0
#pragma unroll
            for (int q = 0; q < VEC; ++q) fP[q] = (TIN)0;
        }
        if (WITH_Q) {
            load_vec<TIN, VEC, false>(rTjm - shift, eo, qr.j0);
            load_vec<TIN, VEC, false>(rTjp - shift, eo, qr.j1);
            load_vec<TIN, VEC, false>(rTkm - shift, eo, qr.k0);
            load_vec<TIN, VEC, false>(rTkp - shift, eo, qr.k1);
            // MODE 3: T(t+1) for the cross-time covariance (T(t-1) too when BOTH); MODE 1: both; MODE 2: the dT/dt cube (rTtm points into it).
            // Tiled order: the T(t+1) row is the own row of a sibling workgroup -> keep it cacheable
            if (TIME_NB) {
                if (p.order == 7) load_vec<TIN, VEC, false>(rTtp - shift, eo, qr.tf);
                else load_vec<TIN, VEC, true>(rTtp - shift, eo, qr.tf);
                if (MODE == 1 || BOTH) load_vec<TIN, VEC, true>(rTtm - shift, eo, qr.tb);
            } else {
                load_vec<TIN, VEC, true>(rTtm - shift, eo, qr.tf);
            }
            // in-row neighbours T[i-1], T[i+1]: from the adjacent lanes' registers (DPP); the elements beyond the
            // wave's two end lanes are at wave-uniform addresses: scalar loads
            const int il = EDGE ? min(max(el - 1, 0), nxb - 1) : el - 1;
            const int ir = EDGE ? min(max(el + nthr * VEC, 0), nxb - 1) : el + nthr * VEC;
            tl_edge = from_prev_lane((double)fT[VEC - 1], (double)rT[il]);
            tr_edge = from_next_lane((double)fT[0], (double)rT[ir]);
        }
        sweep_elems<VEC, UNIFORM, EDGE, MODE, BOTH, RING>(acc, xacc, r, e0, lane_in, fT, fU, fV, fW, fP, tl_edge, tr_edge, qr, qc);
    };

    // a real loop (not unrolled): the live state stays at the 20 accumulators plus one vector's worth of
    // operands, which is what lets 4 waves/SIMD fit.  Trips [1, mid_end) lie strictly inside the row.
    const int ntrips = ONE_TRIP ? 1 : p.ntrips;      // short rows (moving boxes): one trip, no loop
    trip(std::true_type{}, 0);
    if (!ONE_TRIP) {
        const int mid_end = min((nxb - 1 + shift) / (nthr * VEC), ntrips);
#pragma unroll 1
        for (int it = 1; it < mid_end; ++it) trip(std::false_type{}, it);
#pragma unroll 1
        for (int it = max(mid_end, 1); it < ntrips; ++it) trip(std::true_type{}, it);
    }

    finish_row<NTHR, kRound, MODE == 3>(acc, xacc, red, tot, tid, UNIFORM ? h_rad * inv_xlen : inv_xlen, r, out);
    // T, u, v at the west / east box columns (boundary terms): wave-uniform scalar loads
    if (tid == 0) {
        out[LEC_S_TW] = r.cT; out[LEC_S_UW] = r.cU; out[LEC_S_VW] = r.cV;
        // a ring's east column IS its west column: every east-minus-west difference of the boundary terms is exactly 0
        out[LEC_S_TE] = RING ? r.cT : eT; out[LEC_S_UE] = RING ? r.cU : eU; out[LEC_S_VE] = RING ? r.cV : eV;
    }
}

// workgroups (= rows, rounded up to whole XCD chunks / tiles) of a launch over p.t_count time steps; 0 = too many
long long grid_blocks(const RowParams& p) {
    long long n;
    if (p.order == 0) n = (long long)p.t_count * p.nl * p.nyb_max;
    else if (p.order == 7) {
        const long long tgc = (p.t_count + p.tgroup - 1) / p.tgroup, jgc = (p.jchunk + p.jgroup - 1) / p.jgroup;
        n = 8LL * jgc * tgc * p.nl * p.tgroup * p.jgroup;
    } else n = (long long)p.t_count * 8 * p.jchunk * p.nl;
    return n > 0x7fffffffLL ? 0 : n;
}

template <typename TIN, int VEC, bool BOTH, bool RING>
int launch_one(RowParams p, bool uniform, int mode, hipStream_t st) {
    // vectors needed to cover the longest row, plus one for the alignment shift; one wave walks them in trips of 64
    const int nvec = (p.nxb_max + VEC - 1) / VEC + (VEC > 1 ? 1 : 0);
    p.ntrips = (nvec + kThreads - 1) / kThreads;
    if (p.order == 7 && p.t_count < 2) p.order = 2;
    long long nblocks = grid_blocks(p);
    if (nblocks == 0) { p.order = 0; nblocks = grid_blocks(p); }
    if (nblocks == 0) return LEC_ERR_UNSUPPORTED;
    dim3 grid((unsigned)nblocks), block(kThreads);
    if (p.jchunk < 1) p.jchunk = (p.nyb_max + 7) / 8;
    dim3 grid3(8u * (unsigned)p.jchunk, (unsigned)p.nl, (unsigned)p.t_count);    // one-trip rows: (XCD x latitude, level, time step)
    if (p.ntrips == 1 && (p.nl > 65535 || p.t_count > 65535)) return LEC_ERR_UNSUPPORTED;
#define LEC_LAUNCH(U, M, R) do { if (p.ntrips == 1) hipLaunchKernelGGL((lec_rowsweep_kernel<TIN, VEC, U, M, true, BOTH && M == 3, R>), grid3, block, 0, st, p); \
                                 else hipLaunchKernelGGL((lec_rowsweep_kernel<TIN, VEC, U, M, false, BOTH && M == 3, R>), grid, block, 0, st, p); } while (0)
#define LEC_MODES(U) do { if (mode == 0) LEC_LAUNCH(U, 0, false); else if (mode == 1) LEC_LAUNCH(U, 1, false); else if (mode == 2) LEC_LAUNCH(U, 2, false); else LEC_LAUNCH(U, 3, false); } while (0)
    if constexpr (RING) {
        // a ring: evenly spaced longitudes and the dT/dt modes one fixed box reaches (none, a dT/dt cube, the time stencil through covariances)
        if (!uniform || mode == 1) return LEC_ERR_UNSUPPORTED;
        if (mode == 0) LEC_LAUNCH(true, 0, true); else if (mode == 2) LEC_LAUNCH(true, 2, true); else LEC_LAUNCH(true, 3, true);
    } else {
        if (uniform) LEC_MODES(true); else LEC_MODES(false);
    }
#undef LEC_MODES
#undef LEC_LAUNCH
    return LEC_OK;
}

// mode 3 (time stencil on one fixed box): the first time step of the launch forms both cross-time covariances, the
// others only the forward one
template <typename TIN, int VEC, bool RING>
int launch_vec(const RowParams& p, bool uniform, int mode, hipStream_t st) {
    if (mode != 3) return launch_one<TIN, VEC, false, RING>(p, uniform, mode, st);
    RowParams p0 = p;
    p0.t_count = 1;
    int rc = launch_one<TIN, VEC, true, RING>(p0, uniform, mode, st);
    if (rc != LEC_OK || p.t_count < 2) return rc;
    return launch_one<TIN, VEC, false, RING>(later_steps(p), uniform, mode, st);
}


// fp64: 16-byte vectors when every cube base is 16-byte aligned and nx even (`aligned`); fp32: float4 / float2 / scalar (see lec_launch_rowsweep)
template <bool RING>
int launch_dtype(const RowParams& p, int dtype, bool aligned, bool aligned8, bool uniform, int mode, int f32_vec, hipStream_t st) {
    if (dtype == LEC_F64) return aligned ? launch_vec<double, 2, RING>(p, uniform, mode, st) : launch_vec<double, 1, RING>(p, uniform, mode, st);
    if (aligned && f32_vec != 2) return launch_vec<float, 4, RING>(p, uniform, mode, st);
    return aligned8 ? launch_vec<float, 2, RING>(p, uniform, mode, st) : launch_vec<float, 1, RING>(p, uniform, mode, st);
}

}  // namespace
