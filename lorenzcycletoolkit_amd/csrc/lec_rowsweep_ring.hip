// lec_rowsweep_ring.hip -- stage 1 of lec_rowstats_ring: the one-wave-per-row kernel (lec_rowsweep_kernel.h) with RING = true, for evenly
// spaced longitudes and the dT/dt modes one fixed box reaches.  A translation unit of its own: its code object is loaded by ring calls only.
#include "lec_rowsweep_kernel.h"

int lec_launch_rowsweep_ring(const lec::RowParams& p, int dtype, bool aligned, bool aligned8, bool uniform, int mode, int f32_vec, hipStream_t st) {
    return launch_dtype<true>(p, dtype, aligned, aligned8, uniform, mode, f32_vec, st);
}
