// lec_zeta.h -- the 850-hPa relative vorticity at one grid point, shared by lec_diag.hip (extrema inside given boxes) and
// lec_follow.hip (the box that follows the extremum): ONE expression, so the two kernels see the same doubles.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

// running extremum with numpy's tie rule: the first in row-major order (lowest n) among equal values; NaN never enters
struct Best {
    double v; int n;
    __device__ __forceinline__ void take_min(double x, int m) { if (x < v || (x == v && m < n)) { v = x; n = m; } }
    __device__ __forceinline__ void take_max(double x, int m) { if (x > v || (x == v && m < n)) { v = x; n = m; } }
};

// zeta = dv/dx - du/dy + curv u with the three-point stencils of metpy.calc.first_derivative: the parabola through the point and its
// two neighbours (the three points nearest the edge at either end of the slice), coefficients in 1/m from the host's tables -- which
// metric the distances follow (and whether the sphere's curvature term is there) is the caller's choice, not the kernel's.
// P: a kernel's parameter block with xcoef [ny][nx][3], ycoef [ny][3], curv [ny], ny, nx; u, v: one [ny][nx] slice.
template <class P>
__device__ __forceinline__ double zeta_at(const P& p, const double* u, const double* v, int j, int i) {
    const int i0 = min(max(i - 1, 0), p.nx - 3), j0 = min(max(j - 1, 0), p.ny - 3);
    const double* cx = p.xcoef + 3 * ((size_t)j * p.nx + i);
    const double* cy = p.ycoef + 3 * (size_t)j;
    const double* vr = v + (size_t)j * p.nx + i0;
    const double dv = cx[0] * vr[0] + cx[1] * vr[1] + cx[2] * vr[2];
    const double* uc = u + (size_t)j0 * p.nx + i;
    const double du = cy[0] * uc[0] + cy[1] * uc[p.nx] + cy[2] * uc[2 * (size_t)p.nx];
    return dv - du + p.curv[j] * u[(size_t)j * p.nx + i];
}

// zeta_at on a RING of longitudes (lec_follow.hip's ring calls): the stencil at column i reads columns i - 1, i, i + 1 mod nx for every
// i, and xcoef holds the centred coefficients at all columns (the spacing from column nx - 1 to column 0 is the arc across the seam).
// The latitude stencil and curv are zeta_at's; so is the expression, term for term: an interior column gives zeta_at's double.
template <class P>
__device__ __forceinline__ double zeta_ring_at(const P& p, const double* u, const double* v, int j, int i) {
    const int j0 = min(max(j - 1, 0), p.ny - 3);
    const int iw = i == 0 ? p.nx - 1 : i - 1, ie = i == p.nx - 1 ? 0 : i + 1;
    const double* cx = p.xcoef + 3 * ((size_t)j * p.nx + i);
    const double* cy = p.ycoef + 3 * (size_t)j;
    const double* vr = v + (size_t)j * p.nx;
    const double dv = cx[0] * vr[iw] + cx[1] * vr[i] + cx[2] * vr[ie];
    const double* uc = u + (size_t)j0 * p.nx + i;
    const double du = cy[0] * uc[0] + cy[1] * uc[p.nx] + cy[2] * uc[2 * (size_t)p.nx];
    return dv - du + p.curv[j] * u[(size_t)j * p.nx + i];
}
