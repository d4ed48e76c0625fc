// lec_schedule.h -- workgroup -> (time cell, level cell, latitude cell) of the row-block kernel, for the kernel and for the host
// (the launch sizes its grid from it; tests/sched/ walks every block index of it).  No HIP types: it compiles as plain C++ too.
//
// Speed only.  Workgroups are dealt to the 8 XCDs round-robin, so blockIdx & 7 labels the XCD (the blocks that share an L2).  A cell
// is bt time steps x bk levels x bj latitudes, cut from row 0 of the box: one workgroup.  The C = ceil(nyb_max / bj) latitude cells
// are split in WHOLE cells, so no cell lies in two XCDs' chunks and only the cell that straddles row nyb_max - 1 (nyb_max no
// multiple of bj) has a wave without a row of its own:
//   own part   every XCD owns C / 8 consecutive cells for all time steps and levels.  The time cells are cut into time groups of
//              near-equal extent, at most tile_t cells; the chunk into latitude tiles of near-equal height about tile_j, at most
//              tile_j + 1 cells and of one height where that divides the chunk (45 cells at tile_j 4: nine tiles of 5; no
//              sliver).  A tile = one time group x one latitude tile at one level cell, time fastest; the XCD walks the tile
//              through the level cells, then the next time group, then the next latitude tile.
//   remainder  the C % 8 cells at the north end are cut into (cell, time group) units, each walked through its level cells like a
//              tile.  The units are dealt to the XCDs round-robin, the longer time groups first, so no XCD gets more than
//              ceil((C % 8) * time groups / 8) of them and the XCDs' work differs by less than one unit.
// Tiles and units are padded to the largest extent; a workgroup on the padding (or beyond the last unit) returns at once.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LEC_SCHED_HD __host__ __device__
#else
#define LEC_SCHED_HD
#endif

namespace lec {

constexpr int kSchedTileT = 2, kSchedTileJ = 4;   // default tile: 2 x 4 cells at one level cell (profiles/r01_notes.md)

struct BlockSchedule {
    int tcells, kcells, jcells;   // cells with at least one real row along time, level, latitude
    int jown, jrem;               // latitude cells every XCD owns; cells left at the north end (jcells = 8 jown + jrem)
    int tgc, tlo, textra;         // time groups: the first textra hold tlo + 1 cells, the others tlo
    int jgc, jlo, jextra;         // latitude tiles of a chunk, likewise (jgc = 0 when jown = 0)
    int tgmax, jgmax;             // the largest time group / latitude tile: the padded extents
    int own_slots;                // block slots per XCD for its own chunk
    int unit_slots;               // block slots of one (cell, time group) unit
    int units;                    // jrem * tgc
    long long blocks;             // the grid: 8 x (own_slots + slots of ceil(units / 8) units); 0 = beyond 2^31 - 1
};

// tile_t: the largest time group, tile_j: the latitude tile's height (one cell more where that cuts the chunk evenly), in cells; < 1 = the default
LEC_SCHED_HD inline BlockSchedule make_schedule(int nyb_max, int t_count, int nl, int bt, int bk, int bj, int tile_t, int tile_j) {
    BlockSchedule s;
    s.tcells = (t_count + bt - 1) / bt; s.kcells = (nl + bk - 1) / bk; s.jcells = (nyb_max + bj - 1) / bj;
    s.jown = s.jcells / 8; s.jrem = s.jcells % 8;
    if (tile_t < 1) tile_t = kSchedTileT;
    if (tile_j < 1) tile_j = kSchedTileJ;
    if (tile_t > s.tcells) tile_t = s.tcells;
    if (tile_j > s.jown) tile_j = s.jown;
    s.tgc = (s.tcells + tile_t - 1) / tile_t;
    s.tlo = s.tcells / s.tgc; s.textra = s.tcells % s.tgc; s.tgmax = s.tlo + (s.textra ? 1 : 0);
    s.jgc = s.jlo = s.jextra = s.jgmax = 0;
    if (s.jown) {
        // tiles of ONE height where the chunk divides by tile_j or by tile_j + 1; else the count nearest to jown / tile_j that keeps
        // them at tile_j + 1 cells or fewer.  (Measured at 45 cells, tile_j 4: nine tiles of 5 -1.2 .. -1.7 % against the parent
        // schedule, ten of 4 and one of 5 -0.1 .. -1.4 %, nine of 4 and three of 3 +1.6 .. +3.9 %: profiles/schedule_notes.md)
        if (s.jown % tile_j == 0) s.jgc = s.jown / tile_j;
        else if (s.jown % (tile_j + 1) == 0) s.jgc = s.jown / (tile_j + 1);
        else {
            const int nearest = (s.jown + tile_j / 2) / tile_j, fewest = (s.jown + tile_j) / (tile_j + 1);
            s.jgc = nearest > fewest ? nearest : fewest;
        }
        s.jlo = s.jown / s.jgc; s.jextra = s.jown % s.jgc; s.jgmax = s.jlo + (s.jextra ? 1 : 0);
    }
    s.units = s.jrem * s.tgc;
    const long long unit_slots = (long long)s.kcells * s.tgmax;
    const long long own_slots = (long long)s.jgc * s.tgc * s.jgmax * unit_slots;
    const long long blocks = 8 * (own_slots + (s.units + 7) / 8 * unit_slots);
    const bool fits = blocks <= 0x7fffffffLL;
    s.unit_slots = fits ? (int)unit_slots : 0; s.own_slots = fits ? (int)own_slots : 0;
    s.blocks = fits ? blocks : 0;
    return s;
}

// workgroup `block` of a grid of s.blocks -> its cell; false: the workgroup has no cell (padding)
LEC_SCHED_HD inline bool schedule_cell(const BlockSchedule& s, unsigned block, int& tc, int& kc, int& jc) {
    const int xcd = (int)(block & 7u);
    int q = (int)(block >> 3);
    int tg, t_in;
    if (q < s.own_slots) {
        const int tile = s.tgmax * s.jgmax;
        int tile_id = q / tile;
        const int within = q - tile_id * tile;
        const int j_in = within / s.tgmax;
        t_in = within - j_in * s.tgmax;
        kc = tile_id % s.kcells; tile_id /= s.kcells;
        const int jg = tile_id / s.tgc;
        tg = tile_id - jg * s.tgc;
        if (j_in >= s.jlo + (jg < s.jextra ? 1 : 0)) return false;
        jc = xcd * s.jown + jg * s.jlo + (jg < s.jextra ? jg : s.jextra) + j_in;
    } else {
        q -= s.own_slots;
        const int ul = q / s.unit_slots;
        const int w = q - ul * s.unit_slots;
        kc = w / s.tgmax;
        t_in = w - kc * s.tgmax;
        const int u = ul * 8 + xcd;
        if (u >= s.units) return false;
        tg = u / s.jrem;
        jc = 8 * s.jown + (u - tg * s.jrem);
    }
    if (t_in >= s.tlo + (tg < s.textra ? 1 : 0)) return false;
    tc = tg * s.tlo + (tg < s.textra ? tg : s.textra) + t_in;
    return true;
}

}  // namespace lec
