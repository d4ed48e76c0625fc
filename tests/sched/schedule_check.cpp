// schedule_check.cpp -- walks every workgroup index of the row-block kernel's grid through csrc/lec_schedule.h, the code the kernel
// runs, and checks what the launch relies on.  Plain C++ with its own main (tests/test_schedule_cpu.py builds it with
// -fsanitize=address,undefined and runs it).  Swept: nyb_max 1..130 and 721, t_count 1..9 and 64, nl 1, 2, 37, block shapes
// (bt, bj) = (2,2) (1,2) (2,1) (1,1) with bk = 1, tile_t and tile_j in {0, 1, 2, 3, 8}: every combination.
//
// Per combination:
//   * every (time cell, level cell, latitude cell) that holds at least one real row comes from exactly one workgroup, and no workgroup
//     names a cell outside those ranges;
//   * an XCD's own cells come from its workgroups only (blockIdx & 7), the chunks are whole cells, and at most one latitude cell --
//     the one that straddles row nyb_max - 1 -- has a row beyond the box;
//   * time groups are no larger than asked for, latitude tiles at most one cell higher, and either differ by at most one cell;
//   * the row walks of an XCD (waves of its workgroups that have a cell, the waves without a row of their own included: they walk
//     one too) differ from the mean over the XCDs by less than one (cell, time group) unit;
//   * no XCD has more than ceil(remainder cells x time groups / 8) units.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../lorenzcycletoolkit_amd/csrc/lec_schedule.h"

namespace {

struct Tally { long long combos = 0, same = 0, blocks = 0, failures = 0; };

void fail(Tally& ty, const char* what, int nyb, int t, int nl, int bt, int bj, int tt, int tj, long long a = 0, long long b = 0) {
    if (ty.failures++ < 5)
        std::fprintf(stderr, "FAIL %s: nyb_max %d t_count %d nl %d block %d1%d tile_t %d tile_j %d (%lld, %lld)\n", what, nyb, t, nl, bt, bj, tt, tj, a, b);
}

// `walked`: the schedules of this (nyb_max, t_count, nl, block shape) whose grids have been walked: tile extents beyond the cells
// there are, and 0 beside the default, give the same schedule, and the walk depends on nothing else
void check(Tally& ty, std::vector<unsigned char>& seen, std::vector<lec::BlockSchedule>& walked, int nyb, int t_count, int nl, int bt, int bj, int tt, int tj) {
    const int bk = 1;
    const lec::BlockSchedule s = lec::make_schedule(nyb, t_count, nl, bt, bk, bj, tt, tj);
#define FAIL(what, ...) fail(ty, what, nyb, t_count, nl, bt, bj, tt, tj, ##__VA_ARGS__)
    ty.combos++;
    const int tcells = (t_count + bt - 1) / bt, kcells = (nl + bk - 1) / bk, jcells = (nyb + bj - 1) / bj;
    if (s.tcells != tcells || s.kcells != kcells || s.jcells != jcells || s.blocks <= 0 || s.blocks % 8) { FAIL("extents / grid", s.blocks); return; }
    if (8 * s.jown + s.jrem != jcells || s.jrem < 0 || s.jrem > 7 || s.jown != jcells / 8) FAIL("chunks", s.jown, s.jrem);
    // time groups no larger than asked for (0 = the default), latitude tiles at most one cell higher; near-equal
    const int want_t = tt < 1 ? lec::kSchedTileT : tt, want_j = tj < 1 ? lec::kSchedTileJ : tj;
    if (s.tgmax > want_t || s.tgmax < 1 || s.tlo < s.tgmax - 1 || s.tlo < 1 || s.tgc * s.tlo + s.textra != tcells) FAIL("time groups", s.tgmax, s.tlo);
    if (s.jown && (s.jgmax > (want_j < s.jown ? want_j + 1 : s.jown) || s.jgmax < 1 || s.jlo < s.jgmax - 1 || s.jlo < 1 || s.jgc * s.jlo + s.jextra != s.jown)) FAIL("latitude tiles", s.jgmax, s.jlo);
    // at most one latitude cell reaches beyond the box, and it holds row nyb_max - 1
    if ((long long)jcells * bj - nyb >= bj) FAIL("dead rows");
    for (const lec::BlockSchedule& w : walked)
        if (w.tcells == s.tcells && w.kcells == s.kcells && w.jcells == s.jcells && w.jown == s.jown && w.jrem == s.jrem && w.tgc == s.tgc &&
            w.tlo == s.tlo && w.textra == s.textra && w.jgc == s.jgc && w.jlo == s.jlo && w.jextra == s.jextra && w.tgmax == s.tgmax &&
            w.jgmax == s.jgmax && w.own_slots == s.own_slots && w.unit_slots == s.unit_slots && w.units == s.units && w.blocks == s.blocks) {
            ty.same++;
            return;
        }
    walked.push_back(s);

    const size_t ncell = (size_t)tcells * kcells * jcells;
    seen.assign(ncell, 0);
    long long per_xcd[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rem_cells[8] = {0, 0, 0, 0, 0, 0, 0, 0}, produced = 0;
    for (long long b = 0; b < s.blocks; ++b) {
        int tc = -1, kc = -1, jc = -1;
        if (!lec::schedule_cell(s, (unsigned)b, tc, kc, jc)) continue;
        if (tc < 0 || tc >= tcells || kc < 0 || kc >= kcells || jc < 0 || jc >= jcells) { FAIL("cell outside the ranges", b, jc); continue; }
        const int xcd = (int)(b & 7);
        if (jc < 8 * s.jown) { if (jc / s.jown != xcd) FAIL("a cell of one XCD's chunk on another XCD", b, jc); }
        else rem_cells[xcd]++;
        unsigned char& c = seen[((size_t)jc * kcells + kc) * tcells + tc];
        if (c) FAIL("cell produced twice", b, jc);
        c = 1;
        per_xcd[xcd]++; produced++;
    }
    ty.blocks += s.blocks;
    if (produced != (long long)ncell) FAIL("cells missing", produced, (long long)ncell);
    // balance, in workgroups (every workgroup with a cell walks bt * bk * bj rows): |n_x - mean| < one unit = tgmax * kcells workgroups
    const long long unit = (long long)s.tgmax * kcells;
    for (int x = 0; x < 8; ++x) {
        const long long d = 8 * per_xcd[x] - produced;
        if ((d < 0 ? -d : d) >= 8 * unit) FAIL("XCD off the mean by a unit or more", x, per_xcd[x]);
        // units of an XCD: its remainder cells are at most ceil(jrem * tgc / 8) units of at most `unit` workgroups
        if (rem_cells[x] > (long long)((s.jrem * s.tgc + 7) / 8) * unit) FAIL("too many remainder units on an XCD", x, rem_cells[x]);
    }
#undef FAIL
}

std::atomic<int> next_box{131};       // box heights are handed out from the tallest down: the long walks start first

void sweep(Tally& ty) {
    static const int shapes[4][2] = {{2, 2}, {1, 2}, {2, 1}, {1, 1}}, tiles[5] = {0, 1, 2, 3, 8}, levels[3] = {1, 2, 37};
    std::vector<unsigned char> seen;
    std::vector<lec::BlockSchedule> walked;
    for (int i; (i = next_box.fetch_sub(1)) >= 1;) {
        const int nyb = i <= 130 ? i : 721;
        for (int ti = 1; ti <= 10; ++ti) {
            const int t_count = ti <= 9 ? ti : 64;
            for (int nl : levels)
                for (const auto& sh : shapes) {
                    walked.clear();
                    for (int tt : tiles)
                        for (int tj : tiles) check(ty, seen, walked, nyb, t_count, nl, sh[0], sh[1], tt, tj);
                }
        }
    }
}

}  // namespace

int main() {
    unsigned n = std::thread::hardware_concurrency();
    n = n < 1 ? 1 : (n > 8 ? 8 : n);
    std::vector<Tally> tallies(n);
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < n; ++w) pool.emplace_back([&, w] { sweep(tallies[w]); });
    for (auto& th : pool) th.join();
    Tally all;
    for (const Tally& ty : tallies) { all.combos += ty.combos; all.same += ty.same; all.blocks += ty.blocks; all.failures += ty.failures; }
    std::printf("%lld combinations (%lld with the schedule of another tile request), %lld workgroup indices, %lld failures\n", all.combos, all.same,
                all.blocks, all.failures);
    return all.failures ? 1 : 0;
}
