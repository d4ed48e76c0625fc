// lec_level_core.h -- the level x latitude half of stage 2, written once ("The level stage").  Three kernels form the
// per-level sums of one (time step, level) from its row records:
//   lec_area_means_kernel<S>   {[X]}: the cos-weighted meridional means of the six zonal means             (calc_averages.py:46-78)
//   lec_level_terms_kernel<S>  any band height: 64-row staging trips through LDS, sigma, every per-level integrand and boundary piece
//                              (energy_contents.py:99-165, conversion_terms.py:103-245, boundary_terms.py:125-418,
//                               generation_and_dissipation_terms.py:122-152)
//   lec_level_small_kernel<S>  bands of at most 64 rows: one row per lane, the record in registers, no staging tile
// with what they share: the levraw record (V_*), wave_sum, the divisors, LaneSums, BAz's bottom-top repair.  The row arithmetic is
// lec_level_row.inc, included by both level kernels.  Formulas: SURVEY.md appendix A / F.
//
// The kernels are templates over a RECORD SOURCE S, which the including file supplies: lec_reduce.hip reads plain records
// (LevelRecords), lec_level_spec.hip records with a wavenumber's shares in some slots (SpecRecords<B>).  The kernels have internal
// linkage, so each file instantiates its own and remains a code object of its own.  The march over the rows IS each kernel's body and a
// source's members are a few lines that inline at once (lec_mapcol.h records why: a shared __device__ march is optimised on its own before
// it is inlined).  A source has:
//   Params                                 the file's launch struct, the kernel's argument.  The kernels read its rows, nl, nyb_max (rows of
//                                          the record buffer), box, lattab2, levtab2, phi_scale, am and levraw by name
//   kMeansInSmallKernel                    true: the small kernel forms the area means itself (no area-means launch for nyb_max <= 64);
//                                          false: it reads `am`, and the area-means kernel forms a band of at most 64 rows as the small
//                                          kernel would -- one product per lane, not a running sum from +0.0 (-0.0 would lose its sign)
//   S(p, block)                            decodes the level kernels' workgroup index into tl, k (and what else the source needs)
//   box_index(p, tl), band_rows(p, h)      the step's entry of box / lattab2, and its band height given the box's height h
//   out(p)                                 the workgroup's levraw record
//   Shares, load_shares(p, jbc), put(p, shares, r)
//                                          what replaces slots of the lane's own row jbc: loaded with the first load group, written over
//                                          r[] (the row in the LDS tile after the second barrier, or the register array)
//   wT(p, r, row)                          [w'T'] of record r (row index `row` of the buffer) at ANOTHER level, for BAz's repair
//   small_mean_T(p, am, lt, nyb, level)    {[T]} of another level for the small kernel's repair
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lec_hip.h"
#include "lec_internal.h"
#include "lec_rowcommon.h"

// The level kernels form the per-level sums from the same source lines (lec_level_row.inc), whichever kernel and whichever source.
// Contraction is off from here to the end of the including file so that they also give the same BITS: which products the compiler would
// fuse into multiply-adds depends on the surrounding code.
#pragma clang fp contract(off)

namespace lec {

constexpr double kG = LEC_G, kRe = LEC_RE, kRd = LEC_RD;       // (kCp: lec_rowcommon.h)
constexpr int kStageRows = 66;     // lec_level_terms_kernel: latitude rows staged through LDS at a time (64 + one either side)
constexpr int kPartStride = 65;    // partial sums of one statistic, one per lane (+1: conflict-free both ways)
constexpr int kRecStride = LEC_NSTAT + 1, kLatStride = 9;      // LDS row strides (doubles): odd, so a lane per row is conflict-free
constexpr int kSmallRows = 64;     // the tallest band of lec_level_small_kernel
constexpr int kSmallRound = 18;    // sums per reduction round of the small kernel (two rounds: 15 + 18)

// the levraw record
enum {
    V_AZ = 0, V_AE, V_KZ, V_KE, V_CZ2, V_CE2, V_CA1, V_CA2, V_CK1, V_CK2, V_CK3, V_CK4, V_CK5, V_GZ, V_GE,
    V_B1 = 15,  // BAz BAe BKz BKe BPhiZ BPhiE : east-west term, integrated over phi
    V_B2 = 21,  // north-south term
    V_B3 = 27,  // bottom-top term (area mean)
    V_SIG = 33,
    V_COUNT = 34
};
static_assert(V_COUNT <= LEC_NLEVRAW, "levraw record too small");
static_assert(V_SIG == LEC_LEVRAW_SIGMA, "lec_sections reads sigma from this slot");

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// what the sum of statistic s over the rows is divided by
__device__ __forceinline__ double level_divisor(int s, double sig) {
    double div = 1.0;
    const int b = (s >= V_B1) ? (s - V_B1) % 6 : -1;         // boundary pieces: Az Ae | Kz Ke | PhiZ PhiE
    if (s == V_AZ || s == V_AE || b == 0 || b == 1) div = 2 * sig;
    else if (b == 2 || b == 3) div = 2 * kG;
    else if (b == 4 || b == 5) div = kG;
    else if (s == V_CA1) div = 2 * kRe * sig;
    else if (s == V_CA2) div = sig;
    else if (s == V_GZ || s == V_GE) div = kCp * sig;
    return div;
}

// `acc[i] += x` of lec_level_row.inc, for a kernel in which every sum receives exactly one contribution per lane: the contribution goes
// straight to the lane's slot of the reduction buffer instead of waiting in a register (rows below the box contribute 0)
struct LaneSums {
    double* slot0; int first; bool in;
    struct Ref {
        double* q; bool in;
        __device__ __forceinline__ void operator+=(double x) const { *q = in ? x : 0.0; }
    };
    __device__ __forceinline__ Ref operator[](int i) const { return Ref{slot0 + (i - first) * kPartStride, in}; }
};

// the kernels: internal to the file that includes this header
namespace {

// grid (nl * t_count) -- level fastest: neighbouring workgroups are neighbouring levels of one time step --, block 64.  Like
// lec_level_terms_kernel: the record loads are addressed from the kernel arguments alone (nyb_max rows) and issued before the box
// height arrives; rows below a lower box are masked out afterwards.
template <class S>
__global__ void __launch_bounds__(64) lec_area_means_kernel(const typename S::Params p) {
    const int tl = blockIdx.x / p.nl, k = blockIdx.x - tl * p.nl, lane = threadIdx.x;
    const int bi = S::box_index(p, tl);
    const double* rec = p.rows + (size_t)(tl * p.nl + k) * p.nyb_max * LEC_NSTAT;
    const double* lt = p.lattab2 + (size_t)bi * p.nyb_max * 8;
    double a[6] = {0, 0, 0, 0, 0, 0};
    int nyb = 0;
    if (!S::kMeansInSmallKernel && p.nyb_max <= kSmallRows) {       // lec_level_small_kernel's own sums
        const int jc = min(lane, p.nyb_max - 1);
        const dbl2_t* r = reinterpret_cast<const dbl2_t*>(rec + (size_t)jc * LEC_NSTAT);
        const dbl2_t v0 = r[0], v1 = r[1], v2 = r[2];
        const double cw = lt[8 * jc + 0];
        nyb = S::band_rows(p, p.box[4 * bi + 3] - p.box[4 * bi + 2] + 1);
        const bool in = lane < nyb;
        a[0] = in ? cw * v0.x : 0.0; a[1] = in ? cw * v0.y : 0.0; a[2] = in ? cw * v1.x : 0.0;
        a[3] = in ? cw * v1.y : 0.0; a[4] = in ? cw * v2.x : 0.0; a[5] = in ? cw * v2.y : 0.0;
    } else {
        for (int j0 = 0; j0 < p.nyb_max; j0 += 64) {
            const int jb = j0 + lane, jc = min(jb, p.nyb_max - 1);
            const dbl2_t* r = reinterpret_cast<const dbl2_t*>(rec + (size_t)jc * LEC_NSTAT);
            const dbl2_t v0 = r[0], v1 = r[1], v2 = r[2];          // the six zonal means [T] [u] [v] [w] [Phi] [Q]
            const double cw = lt[8 * jc + 0];
            if (j0 == 0) nyb = S::band_rows(p, p.box[4 * bi + 3] - p.box[4 * bi + 2] + 1);
            if (jb < nyb) {
                a[0] += cw * v0.x; a[1] += cw * v0.y; a[2] += cw * v1.x; a[3] += cw * v1.y; a[4] += cw * v2.x; a[5] += cw * v2.y;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 6; ++s) a[s] = wave_sum(a[s]);
    if (lane == 0) {
        double* o = p.am + (size_t)(tl * p.nl + k) * 8;
        o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3];
        o[4] = a[4] * p.phi_scale; o[5] = a[5]; o[6] = 0.0; o[7] = 0.0;
    }
}

// BAz's bottom-top term before the area mean, one latitude row of ANOTHER level:  [2 w'T'] T* + [w] T*^2   (boundary_terms.py:165-168)
// am: the area means of the time step; the small kernel (SMALL) asks its source for {[T]} of that level
template <bool SMALL, class S>
__device__ __forceinline__ double baz3_row(const S& src, const typename S::Params& p, const double* am, const double* lt, int nyb, int level,
                                           int jb) {
    const size_t row = (size_t)(src.tl * p.nl + level) * p.nyb_max + jb;
    const double* r = p.rows + row * LEC_NSTAT;
    const double wt = src.wT(p, r, row);
    const double Ts = r[LEC_S_MT] - (SMALL ? src.small_mean_T(p, am, lt, nyb, level) : am[8 * level + 0]);
    return (2 * wt) * Ts + r[LEC_S_MW] * (Ts * Ts);
}

// The reference repairs THIS term per latitude, before the area mean and before the division by sigma
// (term3 = self._handle_nans(term3) on a [time, level, lat] array, boundary_terms.py:169): a NaN at (level, lat) is replaced by
// the linear interpolation in p between the nearest valid levels of the same latitude (interior gaps only, no
// extrapolation); what stays NaN makes the level's area mean NaN, and the level is then dropped (lec_vertical_kernel).
template <bool SMALL, class S>
__device__ double baz3_repaired(const S& src, const typename S::Params& p, const double* am, const double* lt, int nyb, int k, int jb) {
    int lo = k - 1, hi = k + 1;
    double yl = 0.0, yr = 0.0;
    for (; lo >= 0; --lo) { yl = baz3_row<SMALL>(src, p, am, lt, nyb, lo, jb); if (!isnan(yl)) break; }
    for (; hi < p.nl; ++hi) { yr = baz3_row<SMALL>(src, p, am, lt, nyb, hi, jb); if (!isnan(yr)) break; }
    if (lo < 0 || hi >= p.nl) return nan("");
    const double xl = p.levtab2[4 * lo], xr = p.levtab2[4 * hi];
    const double slope = (yr - yl) / (xr - xl);
    return slope * (p.levtab2[4 * k] - xl) + yl;
}

// grid (one workgroup per S(p, block): a (time step, level) of a record set, level fastest), block 64.  A wave's life here is a chain of
// memory round trips (a few hundred arithmetic instructions between them), so the kernel is arranged to have TWO: every global load --
// the level's records, the latitude table, the records of the levels above and below, the source's shares -- is addressed from the
// kernel arguments alone (the staging covers nyb_max rows; the rows below a lower box are zero records) and issued before anything waits
// for the area means or the box height.
template <class S>
__global__ void __launch_bounds__(64) lec_level_terms_kernel(const typename S::Params p) {
    const S src(p, blockIdx.x);
    const int tl = src.tl, k = src.k, lane = threadIdx.x;
    const int nl = p.nl, nyb_max = p.nyb_max;
    const int bi = S::box_index(p, tl);
    const int km = k > 0 ? k - 1 : k, kp = k < nl - 1 ? k + 1 : k;
    const size_t lstride = (size_t)nyb_max * LEC_NSTAT;
    const double* rec = p.rows + (size_t)(tl * nl + k) * lstride;
    const double* recm = p.rows + (size_t)(tl * nl + km) * lstride;
    const double* recp = p.rows + (size_t)(tl * nl + kp) * lstride;
    const double* lt = p.lattab2 + (size_t)bi * nyb_max * 8;
    const double ps = p.phi_scale;

    // The level's records (256 B each) and the latitude table are staged through LDS 64 rows (+ one row either side) at a time:
    // 16-byte-per-lane loads of consecutive addresses instead of ~45 loads that each touch one 128-byte line per lane.  Row strides of
    // 33 / 9 doubles keep the lane-per-row reads free of bank conflicts.  Same arithmetic and order as a direct read.
    __shared__ double tile[kStageRows * kRecStride];
    __shared__ double ltile[kStageRows * kLatStride];
    constexpr int kIt2 = (kStageRows * (LEC_NSTAT / 2) + 63) / 64, kIt8 = (kStageRows * 4 + 63) / 64;

    double acc[V_COUNT];
#pragma unroll
    for (int i = 0; i < V_COUNT; ++i) acc[i] = 0.0;
    int nyb = 0;
    double aT = 0, aW = 0, aP = 0, aQ = 0, aTm = 0, aTp = 0, pa = 0, pb = 0, pc = 0;
    const double* am = p.am + (size_t)tl * nl * 8;

    for (int j0 = 0; j0 < nyb_max; j0 += 64) {
        const int jlo = j0 > 0 ? j0 - 1 : 0, jhi = min(j0 + 64, nyb_max - 1);
        const int n2 = (jhi - jlo + 1) * (LEC_NSTAT / 2), n8 = (jhi - jlo + 1) * 4;
        const dbl2_t* rsrc = reinterpret_cast<const dbl2_t*>(rec + (size_t)jlo * LEC_NSTAT);
        const dbl2_t* lsrc = reinterpret_cast<const dbl2_t*>(lt + (size_t)jlo * 8);
        dbl2_t v2[kIt2], v8[kIt8];
#pragma unroll
        for (int it = 0; it < kIt2; ++it) v2[it] = rsrc[min(it * 64 + lane, n2 - 1)];
#pragma unroll
        for (int it = 0; it < kIt8; ++it) v8[it] = lsrc[min(it * 64 + lane, n8 - 1)];
        const int jb = j0 + lane, jbc = min(jb, nyb_max - 1);
        static_assert(LEC_S_MT == 0 && LEC_S_MU == 1, "the two means read from the neighbouring levels are one 16-byte load");
        const dbl2_t km2 = *reinterpret_cast<const dbl2_t*>(recm + (size_t)jbc * LEC_NSTAT);
        const dbl2_t kp2 = *reinterpret_cast<const dbl2_t*>(recp + (size_t)jbc * LEC_NSTAT);
        const typename S::Shares shares = src.load_shares(p, jbc);
        if (j0 == 0) {
            nyb = S::band_rows(p, p.box[4 * bi + 3] - p.box[4 * bi + 2] + 1);
            aT = am[8 * k + 0]; aW = am[8 * k + 3]; aP = am[8 * k + 4]; aQ = am[8 * k + 5];
            aTm = am[8 * km + 0]; aTp = am[8 * kp + 0];
            pa = p.levtab2[4 * k + 1]; pb = p.levtab2[4 * k + 2]; pc = p.levtab2[4 * k + 3];
        }
        __syncthreads();                                     // the previous chunk has been consumed
#pragma unroll
        for (int it = 0; it < kIt2; ++it) {
            const int i = it * 64 + lane;
            if (i < n2) { double* d = tile + (i >> 4) * kRecStride + 2 * (i & 15); d[0] = v2[it].x; d[1] = v2[it].y; }
        }
#pragma unroll
        for (int it = 0; it < kIt8; ++it) {
            const int i = it * 64 + lane;
            if (i < n8) { double* d = ltile + (i >> 2) * kLatStride + 2 * (i & 3); d[0] = v8[it].x; d[1] = v8[it].y; }
        }
        __syncthreads();
        if (jb >= nyb) continue;
        const int jm = jb > 0 ? jb - 1 : jb, jp = jb < nyb - 1 ? jb + 1 : jb;
        double* const row = tile + (jb - jlo) * kRecStride;
        src.put(p, shares, row);      // after the staging: only this lane reads these slots of this row
        const double* r = row;
        const double* rjm = tile + (jm - jlo) * kRecStride;
        const double* rjp = tile + (jp - jlo) * kRecStride;
        const double* l0 = ltile + (jb - jlo) * kLatStride;
        const double cw = l0[0], wphi = l0[1], c = l0[2], tn = l0[3];
        const double gra = l0[4], grb = l0[5], grc = l0[6];
        const double cm = ltile[(jm - jlo) * kLatStride + 2], cp = ltile[(jp - jlo) * kLatStride + 2];

#define LEC_BAZ3_REPAIR(jb_) baz3_repaired<false>(src, p, am, lt, nyb, k, (jb_))
#define LEC_ROW_COMMON
#define LEC_ROW_PART_A
#define LEC_ROW_PART_B
#include "lec_level_row.inc"
#undef LEC_ROW_COMMON
#undef LEC_ROW_PART_A
#undef LEC_ROW_PART_B
#undef LEC_BAZ3_REPAIR
    }
    // static stability (thermodynamics.py:55-70); the zonal/area mean commutes with the linear d/dp
    const double pk = p.levtab2[4 * k + 0];
    double sig = kG * aT / kCp - (pk * kG / kRd) * (pa * aTm + pb * aT + pc * aTp);
    sig = (sig > 0.03) ? sig : 0.03;

    // 64 partial sums per statistic -> one total, through LDS (the staging tile is free): lane s adds the partials of statistic s
    // in a fixed order (four chains), applies the statistic's divisor and stores it -- no lane-0 epilogue, no butterfly.
    static_assert(V_SIG * kPartStride <= kStageRows * kRecStride, "partial sums must fit the staging tile");
    __syncthreads();
#pragma unroll
    for (int i = 0; i < V_SIG; ++i) tile[i * kPartStride + lane] = acc[i];
    __syncthreads();
    if (lane < LEC_NLEVRAW) {
        const int s = lane;
        double tot = 0.0, div = 1.0;
        if (s < V_SIG) {
            const double* q = tile + s * kPartStride;
            double c0 = q[0], c1 = q[1], c2 = q[2], c3 = q[3];
#pragma unroll
            for (int l = 4; l < 64; l += 4) { c0 += q[l]; c1 += q[l + 1]; c2 += q[l + 2]; c3 += q[l + 3]; }
            tot = (c0 + c1) + (c2 + c3);
            div = level_divisor(s, sig);
        } else if (s == V_SIG) {
            tot = sig;
        }
        src.out(p)[s] = tot / div;        // x / 1.0 is x
    }
}

// Bands of at most 64 latitude rows (the moving framework's 61 x 61 boxes, every regional box on a 2.5-degree grid): one wave per
// (level, time step), one row per lane, the record in registers, neighbouring rows through lane shuffles, no staging tile.  Same row
// arithmetic (lec_level_row.inc), same butterfly for the area means, same four-chain reduction: the numbers are those of the general
// kernels, bit for bit.
// grid as lec_level_terms_kernel, block 64; requires nyb_max <= 64
// four waves per SIMD (rounds 2-5: 193 VGPRs, two waves per SIMD -- the hand-over's fully unrolled loop had sixty LDS values in flight
// at once.  Round 6: four waves per SIMD, and the SAME 85 us per 512 x 37 levels: the kernel is not bound by its occupancy; nor by its
// record loads -- staged through LDS as coalesced 16-byte loads: 86 us.  profiles/r06_stage2_pmc.txt)
template <class S>
__global__ void __launch_bounds__(64, 4) lec_level_small_kernel(const typename S::Params p) {
    __shared__ double part[kSmallRound * kPartStride];
    const S src(p, blockIdx.x);
    const int tl = src.tl, k = src.k, lane = threadIdx.x;
    const int nl = p.nl, nyb_max = p.nyb_max;
    const int bi = S::box_index(p, tl);
    const int km = k > 0 ? k - 1 : k, kp = k < nl - 1 ? k + 1 : k;
    const size_t lstride = (size_t)nyb_max * LEC_NSTAT;
    const double* lt = p.lattab2 + (size_t)bi * nyb_max * 8;
    const double ps = p.phi_scale;
    // every global load is addressed from the kernel arguments alone (rows below a lower box are zero records or are masked) ...
    const int jb = lane, jbc = min(jb, nyb_max - 1);
    const dbl2_t* rr = reinterpret_cast<const dbl2_t*>(p.rows + (size_t)(tl * nl + k) * lstride + (size_t)jbc * LEC_NSTAT);
    constexpr int kUsed = LEC_S_SPARE / 2;                  // the four spare slots of a record are not read
    dbl2_t R[kUsed];
#pragma unroll
    for (int i = 0; i < kUsed; ++i) R[i] = rr[i];
    const typename S::Shares shares = src.load_shares(p, jbc);
    static_assert(LEC_S_MT == 0 && LEC_S_MU == 1 && LEC_S_MV == 2, "the neighbour rows' [T] [u] [v] are read as r[0..2]");
    const dbl2_t km2 = *reinterpret_cast<const dbl2_t*>(p.rows + (size_t)(tl * nl + km) * lstride + (size_t)jbc * LEC_NSTAT);
    const dbl2_t kp2 = *reinterpret_cast<const dbl2_t*>(p.rows + (size_t)(tl * nl + kp) * lstride + (size_t)jbc * LEC_NSTAT);
    const dbl2_t* ll = reinterpret_cast<const dbl2_t*>(lt + (size_t)jbc * 8);
    const dbl2_t L0 = ll[0], L1 = ll[1], L2 = ll[2], L3 = ll[3];
    // ... and only now the values that arrive through the scalar cache
    const int nyb = S::band_rows(p, p.box[4 * bi + 3] - p.box[4 * bi + 2] + 1);
    const double pk = p.levtab2[4 * k + 0], pa = p.levtab2[4 * k + 1], pb = p.levtab2[4 * k + 2], pc = p.levtab2[4 * k + 3];
    const double* am = p.am + (size_t)tl * nl * 8;
    double aT, aW, aP, aQ, aTm, aTp;
    if constexpr (!S::kMeansInSmallKernel) {        // the area means ride with them (read further down, their scalar loads are issued later)
        aT = am[8 * k + 0]; aW = am[8 * k + 3]; aP = am[8 * k + 4]; aQ = am[8 * k + 5];
        aTm = am[8 * km + 0]; aTp = am[8 * kp + 0];
    }
    const bool in = jb < nyb;

    double r[LEC_S_SPARE];
#pragma unroll
    for (int i = 0; i < kUsed; ++i) { r[2 * i] = R[i].x; r[2 * i + 1] = R[i].y; }
    src.put(p, shares, r);
    const double cw = L0.x, wphi = L0.y, c = L1.x, tn = L1.y, gra = L2.x, grb = L2.y, grc = L3.x;

    if constexpr (S::kMeansInSmallKernel) {
        // lec_area_means_kernel's products and butterfly ({[u]} and {[v]} are not used by any term): no launch of it, no `am` round trip
        aT = wave_sum(in ? cw * r[0] : 0.0);
        aW = wave_sum(in ? cw * r[3] : 0.0);
        aP = wave_sum(in ? cw * r[4] : 0.0) * ps;
        aQ = wave_sum(in ? cw * r[5] : 0.0);
        aTm = (km == k) ? aT : wave_sum(in ? cw * km2.x : 0.0);
        aTp = (kp == k) ? aT : wave_sum(in ? cw * kp2.x : 0.0);
    }

    // rows j-1 / j+1 from the neighbouring lanes (the first and last row of the band see themselves, like the clamped indices of the
    // general kernel)
    const int lm = max(lane - 1, 0), lp = min(lane + 1, max(nyb - 1, 0));
    double rjm[3], rjp[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) { rjm[s] = __shfl(r[s], lm); rjp[s] = __shfl(r[s], lp); }
    const double cm = __shfl(c, lm), cp = __shfl(c, lp);

    // static stability (thermodynamics.py:55-70)
    double sig = kG * aT / kCp - (pk * kG / kRd) * (pa * aTm + pb * aT + pc * aTp);
    sig = (sig > 0.03) ? sig : 0.03;

    // The row's contributions (every lane computes; lanes below the box are masked where the sums are handed over), in two parts,
    // each followed by its reduction through one small LDS buffer: lane s adds the 64 partials of sum s in four chains (the general
    // kernel's order), applies the divisor and stores.
    double* const out = src.out(p);
    auto reduce_round = [&](const int s0, const int ns) {
        __syncthreads();
        if (lane < ns) {
            const int s = s0 + lane;
            const double* q = part + lane * kPartStride;
            double c0 = q[0], c1 = q[1], c2 = q[2], c3 = q[3];
#pragma unroll 4        // (sixteen partials in flight, not sixty: fully unrolled the loads alone hold 120 registers)
            for (int l = 4; l < 64; l += 4) { c0 += q[l]; c1 += q[l + 1]; c2 += q[l + 2]; c3 += q[l + 3]; }
            const double tot = (c0 + c1) + (c2 + c3);
            out[s] = tot / level_divisor(s, sig);
        }
        __syncthreads();
    };
    static_assert(V_B1 <= kSmallRound && V_SIG - V_B1 <= kSmallRound, "a reduction round must fit the buffer");
#define LEC_BAZ3_REPAIR(jb_) (in ? baz3_repaired<true>(src, p, am, lt, nyb, k, (jb_)) : 0.0)
#define LEC_ROW_COMMON
#include "lec_level_row.inc"
#undef LEC_ROW_COMMON
    {
        const LaneSums acc{part + lane, 0, in};
#define LEC_ROW_PART_A
#include "lec_level_row.inc"
#undef LEC_ROW_PART_A
    }
    reduce_round(0, V_B1);
    {
#pragma unroll
        for (int i = 0; i < V_SIG - V_B1; ++i) part[i * kPartStride + lane] = 0.0;      // the north-south sums take a row at either end only
        const LaneSums acc{part + lane, V_B1, in};
#define LEC_ROW_PART_B
#include "lec_level_row.inc"
#undef LEC_ROW_PART_B
    }
    reduce_round(V_B1, V_SIG - V_B1);
#undef LEC_BAZ3_REPAIR
    if (lane < LEC_NLEVRAW - V_SIG) out[V_SIG + lane] = (lane == 0) ? sig : 0.0;
}

}  // namespace

}  // namespace lec
