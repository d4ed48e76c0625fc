// lec_level_spec.hip -- lec_level_spec_ring: the level x latitude half of stage 2 for the zonal-wavenumber spectra of a ring
// (-f --periodic --wavenumbers; include/lec_hip.h).  A translation unit of its own: lec_reduce.hip and the bits of
// its kernels are not touched, and the code object is loaded by spectral calls only.
//
// X(n) is what stage 2 gives on the ring pass's row records with slots LEC_S_TT .. LEC_S_WV (6 .. 13) replaced by lec_rowspec_ring's
// shares of wavenumber n and slot LEC_S_QT (15) by lec_rowspec_q_ring's.  lec_reduce needs those records assembled in memory, N copies of
// every record; the kernels here are lec_reduce.hip's two level kernels -- the same source lines for a row (lec_level_row.inc), the same
// reductions, the same divisors -- with one workgroup per (wavenumber, time step, level) that loads the ring pass's record and takes the
// nine slots straight from spec_d / qspec_d:
//   lec_spec_area_means_kernel   the area means of the six zonal means, once per (time step, level): no replaced slot enters them
//   lec_spec_level_small_kernel  bands of at most 64 rows: the record in registers, the slots replaced in the register array
//   lec_spec_level_terms_kernel  taller bands: 64-row staging trips through LDS, the slots replaced in the LDS tile
// BAz's bottom-top term is repaired per latitude from OTHER levels' LEC_S_WT: a replaced slot, read from spec_d at that level.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/lec_hip.h"
#include "lec_internal.h"
#include "lec_rowcommon.h"

// as lec_reduce.hip: the same source lines must give the same bits in every kernel that includes them
#pragma clang fp contract(off)

namespace {
using lec::dbl2_t;

constexpr double kG = LEC_G, kRe = LEC_RE, kRd = LEC_RD, kCp = LEC_CP_D;
constexpr int kStageRows = 66;     // rows staged through LDS at a time (64 + one either side)
constexpr int kPartStride = 65;    // partial sums of one statistic, one per lane
constexpr int kRecStride = LEC_NSTAT + 1, kLatStride = 9;
constexpr int kSmallRows = 64;
constexpr int kSmallRound = 18;    // sums per reduction round of the small kernel (two rounds: 15 + 18)
constexpr int kSpecSlots = 8;      // LEC_S_TT .. LEC_S_WV
constexpr int kBudgetSlots = 4;    // lec_rowspec_b_ring's: LEC_S_VTT, LEC_S_WTT, LEC_S_EV, LEC_S_EW
static_assert(LEC_S_WV - LEC_S_TT + 1 == kSpecSlots && LEC_S_QT == LEC_S_WV + 2, "slots 6 .. 13 and 15 are the replaced ones");

// the levraw record of lec_reduce.hip
enum {
    V_AZ = 0, V_AE, V_KZ, V_KE, V_CZ2, V_CE2, V_CA1, V_CA2, V_CK1, V_CK2, V_CK3, V_CK4, V_CK5, V_GZ, V_GE,
    V_B1 = 15, V_B2 = 21, V_B3 = 27, V_SIG = 33, V_COUNT = 34
};
static_assert(V_COUNT <= LEC_NLEVRAW, "levraw record too small");

struct SpecLevParams {
    const double* rows;     // [t_count][nl][nyb][LEC_NSTAT]
    const double* spec;     // [t_count][nl][nyb][n_wave][8]
    const double* qspec;    // [t_count][nl][nyb][n_wave] or null
    int t_count, nl, nyb, n_wave;
    const int* box;
    const double* lattab2;
    const double* levtab2;
    double phi_scale;
    double* am;             // [t_count][nl][8]
    double* levraw;
    long long wstride;      // doubles between consecutive wavenumbers of levraw
    const double* bspec;    // [t_count][nl][nyb][n_wave][4], the instantiations of lec_level_spec_b_ring only
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int box_rows(const SpecLevParams& p) { return min(p.box[3] - p.box[2] + 1, p.nyb); }

// grid (nl * t_count), block 64.  The area means as the assembled path's kernels form them: lec_level_small_kernel's own butterfly of
// one product per lane for a band of at most 64 rows, lec_area_means_kernel's running sums over 64-row trips for a taller one.
__global__ void __launch_bounds__(64) lec_spec_area_means_kernel(const SpecLevParams p) {
    const int tl = blockIdx.x / p.nl, k = blockIdx.x - tl * p.nl, lane = threadIdx.x;
    const double* rec = p.rows + (size_t)(tl * p.nl + k) * p.nyb * LEC_NSTAT;
    const double* lt = p.lattab2;
    const int nyb = box_rows(p);
    double a[6] = {0, 0, 0, 0, 0, 0};
    if (p.nyb <= kSmallRows) {
        const int jc = min(lane, p.nyb - 1);
        const dbl2_t* r = reinterpret_cast<const dbl2_t*>(rec + (size_t)jc * LEC_NSTAT);
        const dbl2_t v0 = r[0], v1 = r[1], v2 = r[2];
        const double cw = lt[8 * jc + 0];
        const bool in = lane < nyb;
        a[0] = in ? cw * v0.x : 0.0; a[1] = in ? cw * v0.y : 0.0; a[2] = in ? cw * v1.x : 0.0;
        a[3] = in ? cw * v1.y : 0.0; a[4] = in ? cw * v2.x : 0.0; a[5] = in ? cw * v2.y : 0.0;
    } else {
        for (int j0 = 0; j0 < p.nyb; j0 += 64) {
            const int jb = j0 + lane, jc = min(jb, p.nyb - 1);
            const dbl2_t* r = reinterpret_cast<const dbl2_t*>(rec + (size_t)jc * LEC_NSTAT);
            const dbl2_t v0 = r[0], v1 = r[1], v2 = r[2];
            const double cw = lt[8 * jc + 0];
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

// BAz's bottom-top term before the area mean, one latitude row of ANOTHER level:  [2 w'T'] T* + [w] T*^2  with [w'T'] the wavenumber's
// share at that level (baz3_row of lec_reduce.hip on the assembled record)
__device__ __forceinline__ double baz3_row(const SpecLevParams& p, const double* am_t, int n, int tl, int level, int jb) {
    const size_t row = (size_t)(tl * p.nl + level) * p.nyb + jb;
    const double* r = p.rows + row * LEC_NSTAT;
    const double wt = p.spec[(row * p.n_wave + n) * kSpecSlots + (LEC_S_WT - LEC_S_TT)];
    const double Ts = r[LEC_S_MT] - am_t[8 * level + 0];
    return (2 * wt) * Ts + r[LEC_S_MW] * (Ts * Ts);
}

// baz3_repaired of lec_reduce.hip: linear in p between the nearest valid levels of the same latitude, interior gaps only
__device__ double baz3_repaired(const SpecLevParams& p, const double* am_t, int n, int tl, int k, int jb) {
    int lo = k - 1, hi = k + 1;
    double yl = 0.0, yr = 0.0;
    for (; lo >= 0; --lo) { yl = baz3_row(p, am_t, n, tl, lo, jb); if (!isnan(yl)) break; }
    for (; hi < p.nl; ++hi) { yr = baz3_row(p, am_t, n, tl, hi, jb); if (!isnan(yr)) break; }
    if (lo < 0 || hi >= p.nl) return nan("");
    const double xl = p.levtab2[4 * lo], xr = p.levtab2[4 * hi];
    const double slope = (yr - yl) / (xr - xl);
    return slope * (p.levtab2[4 * k] - xl) + yl;
}

// the statistic's divisor (lec_reduce.hip)
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

// grid (n_wave * t_count * nl) -- level fastest, then time step, then wavenumber --, block 64.  lec_level_terms_kernel with the nine
// slots of the lane's own row replaced in the LDS tile (the rows j - 1 / j + 1 are read for [T] [u] [v] only).
// B (lec_level_spec_b_ring): slots LEC_S_VTT, LEC_S_WTT, LEC_S_EV, LEC_S_EW likewise, from bspec_d; an instantiation of its own, the
// instantiation without it is the kernel lec_level_spec_ring has always launched.
template <bool B>
__global__ void __launch_bounds__(64) lec_spec_level_terms_kernel(const SpecLevParams p) {
    const int nl = p.nl, nyb_max = p.nyb, lane = threadIdx.x;
    const int per_wave = p.t_count * nl;
    const int n = blockIdx.x / per_wave, tk = blockIdx.x - n * per_wave;
    const int tl = tk / nl, k = tk - tl * nl;
    const int km = k > 0 ? k - 1 : k, kp = k < nl - 1 ? k + 1 : k;
    const size_t lstride = (size_t)nyb_max * LEC_NSTAT;
    const double* rec = p.rows + (size_t)(tl * nl + k) * lstride;
    const double* recm = p.rows + (size_t)(tl * nl + km) * lstride;
    const double* recp = p.rows + (size_t)(tl * nl + kp) * lstride;
    const double* lt = p.lattab2;
    const double ps = p.phi_scale;

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
        const dbl2_t* src = reinterpret_cast<const dbl2_t*>(rec + (size_t)jlo * LEC_NSTAT);
        const dbl2_t* lsrc = reinterpret_cast<const dbl2_t*>(lt + (size_t)jlo * 8);
        dbl2_t v2[kIt2], v8[kIt8];
#pragma unroll
        for (int it = 0; it < kIt2; ++it) v2[it] = src[min(it * 64 + lane, n2 - 1)];
#pragma unroll
        for (int it = 0; it < kIt8; ++it) v8[it] = lsrc[min(it * 64 + lane, n8 - 1)];
        const int jb = j0 + lane, jbc = min(jb, nyb_max - 1);
        const dbl2_t km2 = *reinterpret_cast<const dbl2_t*>(recm + (size_t)jbc * LEC_NSTAT);
        const dbl2_t kp2 = *reinterpret_cast<const dbl2_t*>(recp + (size_t)jbc * LEC_NSTAT);
        // the wavenumber's shares of the lane's own row
        const size_t srow = ((size_t)(tl * nl + k) * nyb_max + jbc) * p.n_wave + n;
        const dbl2_t* sp = reinterpret_cast<const dbl2_t*>(p.spec + srow * kSpecSlots);
        const dbl2_t s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
        const double sq = p.qspec ? p.qspec[srow] : 0.0;
        dbl2_t b0 = {0.0, 0.0}, b1 = {0.0, 0.0};
        if (B) {
            const dbl2_t* bp = reinterpret_cast<const dbl2_t*>(p.bspec + srow * kBudgetSlots);
            b0 = bp[0]; b1 = bp[1];
        }
        if (j0 == 0) {
            nyb = box_rows(p);
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
        {   // after the staging: only this lane reads these slots of this row
            double* d = tile + (jb - jlo) * kRecStride;
            d[LEC_S_TT + 0] = s0.x; d[LEC_S_TT + 1] = s0.y; d[LEC_S_TT + 2] = s1.x; d[LEC_S_TT + 3] = s1.y;
            d[LEC_S_TT + 4] = s2.x; d[LEC_S_TT + 5] = s2.y; d[LEC_S_TT + 6] = s3.x; d[LEC_S_TT + 7] = s3.y;
            if (p.qspec) d[LEC_S_QT] = sq;
            if (B) { d[LEC_S_VTT] = b0.x; d[LEC_S_WTT] = b0.y; d[LEC_S_EV] = b1.x; d[LEC_S_EW] = b1.y; }
        }
        const int jm = jb > 0 ? jb - 1 : jb, jp = jb < nyb - 1 ? jb + 1 : jb;
        const double* r = tile + (jb - jlo) * kRecStride;
        const double* rjm = tile + (jm - jlo) * kRecStride;
        const double* rjp = tile + (jp - jlo) * kRecStride;
        const double* l0 = ltile + (jb - jlo) * kLatStride;
        const double cw = l0[0], wphi = l0[1], c = l0[2], tn = l0[3];
        const double gra = l0[4], grb = l0[5], grc = l0[6];
        const double cm = ltile[(jm - jlo) * kLatStride + 2], cp = ltile[(jp - jlo) * kLatStride + 2];

#define LEC_BAZ3_REPAIR(jb_) baz3_repaired(p, am, n, tl, k, (jb_))
#define LEC_ROW_COMMON
#define LEC_ROW_PART_A
#define LEC_ROW_PART_B
#include "lec_level_row.inc"
#undef LEC_ROW_COMMON
#undef LEC_ROW_PART_A
#undef LEC_ROW_PART_B
#undef LEC_BAZ3_REPAIR
    }
    // static stability (thermodynamics.py:55-70)
    const double pk = p.levtab2[4 * k + 0];
    double sig = kG * aT / kCp - (pk * kG / kRd) * (pa * aTm + pb * aT + pc * aTp);
    sig = (sig > 0.03) ? sig : 0.03;

    // 64 partial sums per statistic -> one total, through LDS: lane s adds the partials of statistic s in four chains
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
        p.levraw[(size_t)n * (size_t)p.wstride + (size_t)(tl * nl + k) * LEC_NLEVRAW + s] = tot / div;        // x / 1.0 is x
    }
}

// `acc[i] += x` of lec_level_row.inc for a kernel in which every sum receives exactly one contribution per lane (lec_reduce.hip)
struct LaneSums {
    double* slot0; int first; bool in;
    struct Ref {
        double* q; bool in;
        __device__ __forceinline__ void operator+=(double x) const { *q = in ? x : 0.0; }
    };
    __device__ __forceinline__ Ref operator[](int i) const { return Ref{slot0 + (i - first) * kPartStride, in}; }
};

// grid (n_wave * t_count * nl), block 64; requires nyb <= 64.  lec_level_small_kernel with the nine slots replaced in the register
// array; the area means -- the same butterflies, formed once per (time step, level) by lec_spec_area_means_kernel -- come from `am`.
// B: as in lec_spec_level_terms_kernel.
template <bool B>
__global__ void __launch_bounds__(64, 4) lec_spec_level_small_kernel(const SpecLevParams p) {
    __shared__ double part[kSmallRound * kPartStride];
    const int nl = p.nl, nyb_max = p.nyb, lane = threadIdx.x;
    const int per_wave = p.t_count * nl;
    const int n = blockIdx.x / per_wave, tk = blockIdx.x - n * per_wave;
    const int tl = tk / nl, k = tk - tl * nl;
    const int km = k > 0 ? k - 1 : k, kp = k < nl - 1 ? k + 1 : k;
    const size_t lstride = (size_t)nyb_max * LEC_NSTAT;
    const double* lt = p.lattab2;
    const double ps = p.phi_scale;
    const int jb = lane, jbc = min(jb, nyb_max - 1);
    const dbl2_t* rr = reinterpret_cast<const dbl2_t*>(p.rows + (size_t)(tl * nl + k) * lstride + (size_t)jbc * LEC_NSTAT);
    constexpr int kUsed = LEC_S_SPARE / 2;                  // the four spare slots of a record are not read
    dbl2_t R[kUsed];
#pragma unroll
    for (int i = 0; i < kUsed; ++i) R[i] = rr[i];
    const size_t srow = ((size_t)(tl * nl + k) * nyb_max + jbc) * p.n_wave + n;
    const dbl2_t* sp = reinterpret_cast<const dbl2_t*>(p.spec + srow * kSpecSlots);
    const dbl2_t s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
    const double sq = p.qspec ? p.qspec[srow] : 0.0;
    dbl2_t b0 = {0.0, 0.0}, b1 = {0.0, 0.0};
    if (B) {
        const dbl2_t* bp = reinterpret_cast<const dbl2_t*>(p.bspec + srow * kBudgetSlots);
        b0 = bp[0]; b1 = bp[1];
    }
    const dbl2_t km2 = *reinterpret_cast<const dbl2_t*>(p.rows + (size_t)(tl * nl + km) * lstride + (size_t)jbc * LEC_NSTAT);
    const dbl2_t kp2 = *reinterpret_cast<const dbl2_t*>(p.rows + (size_t)(tl * nl + kp) * lstride + (size_t)jbc * LEC_NSTAT);
    const dbl2_t* ll = reinterpret_cast<const dbl2_t*>(lt + (size_t)jbc * 8);
    const dbl2_t L0 = ll[0], L1 = ll[1], L2 = ll[2], L3 = ll[3];
    const int nyb = box_rows(p);
    const double pk = p.levtab2[4 * k + 0], pa = p.levtab2[4 * k + 1], pb = p.levtab2[4 * k + 2], pc = p.levtab2[4 * k + 3];
    const double* am = p.am + (size_t)tl * nl * 8;
    const double aT = am[8 * k + 0], aW = am[8 * k + 3], aP = am[8 * k + 4], aQ = am[8 * k + 5];
    const double aTm = am[8 * km + 0], aTp = am[8 * kp + 0];
    const bool in = jb < nyb;

    double r[LEC_S_SPARE];
#pragma unroll
    for (int i = 0; i < kUsed; ++i) { r[2 * i] = R[i].x; r[2 * i + 1] = R[i].y; }
    r[LEC_S_TT + 0] = s0.x; r[LEC_S_TT + 1] = s0.y; r[LEC_S_TT + 2] = s1.x; r[LEC_S_TT + 3] = s1.y;
    r[LEC_S_TT + 4] = s2.x; r[LEC_S_TT + 5] = s2.y; r[LEC_S_TT + 6] = s3.x; r[LEC_S_TT + 7] = s3.y;
    if (p.qspec) r[LEC_S_QT] = sq;
    if (B) { r[LEC_S_VTT] = b0.x; r[LEC_S_WTT] = b0.y; r[LEC_S_EV] = b1.x; r[LEC_S_EW] = b1.y; }
    const double cw = L0.x, wphi = L0.y, c = L1.x, tn = L1.y, gra = L2.x, grb = L2.y, grc = L3.x;

    // rows j-1 / j+1 from the neighbouring lanes (the first and last row of the band see themselves)
    const int lm = max(lane - 1, 0), lp = min(lane + 1, max(nyb - 1, 0));
    double rjm[3], rjp[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) { rjm[s] = __shfl(r[s], lm); rjp[s] = __shfl(r[s], lp); }
    const double cm = __shfl(c, lm), cp = __shfl(c, lp);

    // static stability (thermodynamics.py:55-70)
    double sig = kG * aT / kCp - (pk * kG / kRd) * (pa * aTm + pb * aT + pc * aTp);
    sig = (sig > 0.03) ? sig : 0.03;

    double* const out = p.levraw + (size_t)n * (size_t)p.wstride + (size_t)(tl * nl + k) * LEC_NLEVRAW;
    auto reduce_round = [&](const int s0_, const int ns) {
        __syncthreads();
        if (lane < ns) {
            const int s = s0_ + lane;
            const double* q = part + lane * kPartStride;
            double c0 = q[0], c1 = q[1], c2 = q[2], c3 = q[3];
#pragma unroll 4
            for (int l = 4; l < 64; l += 4) { c0 += q[l]; c1 += q[l + 1]; c2 += q[l + 2]; c3 += q[l + 3]; }
            const double tot = (c0 + c1) + (c2 + c3);
            out[s] = tot / level_divisor(s, sig);
        }
        __syncthreads();
    };
    static_assert(V_B1 <= kSmallRound && V_SIG - V_B1 <= kSmallRound, "a reduction round must fit the buffer");
#define LEC_BAZ3_REPAIR(jb_) (in ? baz3_repaired(p, am, n, tl, k, (jb_)) : 0.0)
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

// a refusal of either call, under the call's own name
int refuse(int code, const char* who, const char* what) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return lec_set_error(code, msg);
}

// both calls: `who` names the call, `bspec` is lec_level_spec_b_ring's fourth input (checked by the caller) or null
int level_spec(const lec_level_spec_args* a, const double* bspec, const char* who) {
    if (!a) return refuse(LEC_ERR_ARG, who, "null args");
    if (!a->rows_d) return refuse(LEC_ERR_ARG, who, "null rows_d");
    if (!a->spec_d) return refuse(LEC_ERR_ARG, who, "null spec_d");
    if (!a->box_d) return refuse(LEC_ERR_ARG, who, "null box_d");
    if (!a->lattab2_d) return refuse(LEC_ERR_ARG, who, "null lattab2_d");
    if (!a->levtab2_d) return refuse(LEC_ERR_ARG, who, "null levtab2_d");
    if (!a->am_d) return refuse(LEC_ERR_ARG, who, "null am_d");
    if (!a->levraw_d) return refuse(LEC_ERR_ARG, who, "null levraw_d");
    if ((uintptr_t)a->rows_d % 16) return refuse(LEC_ERR_ARG, who, "rows_d must be 16-byte aligned");
    if ((uintptr_t)a->spec_d % 16) return refuse(LEC_ERR_ARG, who, "spec_d must be 16-byte aligned");
    if ((uintptr_t)a->lattab2_d % 16) return refuse(LEC_ERR_ARG, who, "lattab2_d must be 16-byte aligned");
    if (a->n_wave < 1) return refuse(LEC_ERR_ARG, who, "n_wave must be >= 1");
    if (a->t_count < 1) return refuse(LEC_ERR_ARG, who, "t_count must be >= 1");
    if (a->nl < 1) return refuse(LEC_ERR_ARG, who, "nl must be >= 1");
    if (a->nyb < 2) return refuse(LEC_ERR_ARG, who, "nyb must be >= 2 (a band needs two rows)");
    if (a->n_wave > LEC_MAX_WAVENUMBERS) return refuse(LEC_ERR_UNSUPPORTED, who, "n_wave above LEC_MAX_WAVENUMBERS");
    if (a->nl > LEC_MAX_LEVELS) return refuse(LEC_ERR_UNSUPPORTED, who, "nl above LEC_MAX_LEVELS");
    // one 64-lane workgroup per (n, t, k), and HIP takes fewer than 2^32 threads per launch
    if ((long long)a->n_wave * a->t_count * a->nl >= (1LL << 26))
        return refuse(LEC_ERR_UNSUPPORTED, who, "n_wave * t_count * nl must stay below 2^26 in one call (cut the series into several calls)");
    const long long dense = (long long)a->t_count * a->nl * LEC_NLEVRAW;
    if (a->wave_stride != 0 && a->wave_stride < dense)
        return refuse(LEC_ERR_ARG, who, "wave_stride must be 0 (dense) or at least t_count * nl * LEC_NLEVRAW");
    SpecLevParams p;
    p.rows = a->rows_d; p.spec = a->spec_d; p.qspec = a->qspec_d; p.bspec = bspec;
    p.t_count = a->t_count; p.nl = a->nl; p.nyb = a->nyb; p.n_wave = a->n_wave;
    p.box = a->box_d; p.lattab2 = a->lattab2_d; p.levtab2 = a->levtab2_d; p.phi_scale = a->phi_scale;
    p.am = a->am_d; p.levraw = a->levraw_d; p.wstride = a->wave_stride ? a->wave_stride : dense;
    hipStream_t st = (hipStream_t)a->stream;
    const dim3 grid_tk((unsigned)(a->t_count * a->nl)), grid((unsigned)(a->n_wave * a->t_count * a->nl));
    hipLaunchKernelGGL(lec_spec_area_means_kernel, grid_tk, dim3(64), 0, st, p);
    if (bspec) {
        if (a->nyb <= kSmallRows) hipLaunchKernelGGL(lec_spec_level_small_kernel<true>, grid, dim3(64), 0, st, p);
        else hipLaunchKernelGGL(lec_spec_level_terms_kernel<true>, grid, dim3(64), 0, st, p);
    } else {
        if (a->nyb <= kSmallRows) hipLaunchKernelGGL(lec_spec_level_small_kernel<false>, grid, dim3(64), 0, st, p);
        else hipLaunchKernelGGL(lec_spec_level_terms_kernel<false>, grid, dim3(64), 0, st, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lec_set_error(LEC_ERR_LAUNCH, hipGetErrorString(e));
    return LEC_OK;
}

}  // namespace

extern "C" int lec_level_spec_ring(const lec_level_spec_args* a) { return level_spec(a, nullptr, "lec_level_spec_ring"); }

extern "C" int lec_level_spec_b_ring(const lec_level_spec_b_args* a) {
    if (!a) return lec_set_error(LEC_ERR_ARG, "lec_level_spec_b_ring: null args");
    if (!a->bspec_d) return lec_set_error(LEC_ERR_ARG, "lec_level_spec_b_ring: null bspec_d");
    if ((uintptr_t)a->bspec_d % 16) return lec_set_error(LEC_ERR_ARG, "lec_level_spec_b_ring: bspec_d must be 16-byte aligned");
    return level_spec(&a->spec, a->bspec_d, "lec_level_spec_b_ring");
}
