"""The cases of tests/follow_cases.py, checked on the CPU alone: every case reaches the seam it is named for -- the numbers that the
launch arithmetic of csrc/lec_follow.hip implies, restated in ``follow_cases.launch_numbers`` / ``place`` -- every hgt field is exact,
every zeta case clear of a near tie, and the tie cases can tell the rule from three wrong ones.  No kernel is built or run."""
import numpy as np
import pytest

from tests import follow_cases as fc

CHAINS = [fc.case(cid) for cid in fc.all_chain_ids()]
SEEDS = [fc.case(cid) for cid in fc.all_seed_ids()]


def _family(name):
    return [fc.case(cid) for cid in (fc.CHAIN_FAMILIES if name in fc.CHAIN_FAMILIES else fc.SEED_FAMILIES)[name]]


def test_case_counts():
    """The figures the pull request quotes."""
    assert {k: len(v) for k, v in fc.CHAIN_FAMILIES.items()} == {"partition": 120, "ties": 28, "clip": 80, "missing": 36, "ring": 16}
    assert sum(len(v) for v in fc.SEED_FAMILIES.values()) == 48


def test_hgt_fields_are_small_integers():
    for c in CHAINS + SEEDS:
        if c["field"] != "hgt":
            continue
        x = c["F"][np.isfinite(c["F"])]
        assert np.all(x == np.floor(x)) and np.all(x >= 0) and np.all(x < fc.HGT_LIMIT), c["id"]
    x = fc.capped_patterns()
    assert np.all(x == np.floor(x)) and x.min() >= 0 and x.max() < fc.HGT_LIMIT


def test_zeta_cases_are_clear_of_a_near_tie():
    """No case may be left out as a near tie: the restatement alone satisfies the margin."""
    zeta = [c for c in CHAINS if c["field"] == "zeta"]
    assert {(c["form"], c["expect"]["corner"], c["r"], c["sense"]) for c in zeta} == {
        (f, k, r, s) for f in ("metpy_no_crs", "spherical") for k in ("sw", "se", "nw", "ne") for r in (0, 1) for s in (fc.MIN, fc.MAX)}
    for c in zeta:
        ref = fc.reference(c["id"])
        assert ref["margin"].min() > fc.NEAR_TIE and not ref["status"].any(), c["id"]
        j0, j1, i0, i1 = ref["windows"][0]["window"]
        # the window lies on the slice's first or last row and column: the one-sided stencils i0 = clamp(i - 1, 0, nx - 3) are in play
        assert (j0 == 0 or j1 == fc.NY - 1) and (i0 == 0 or i1 == fc.NX - 1), c["id"]


def test_every_chain_is_safe_to_launch():
    """What the library validates, and what it relies on: the start is an admissible centre, every step's tile fits the LDS the launch
    declares (min(2 sj + 1 + 2 r, ny) x min(2 si + 1 + 2 r, nx) doubles), and that is below the 160 KiB limit."""
    for c in CHAINS:
        nt, ny, nx = c["F"].shape
        jlo, jhi, ilo, ihi = c["bounds"]
        assert 0 <= jlo <= jhi < ny and 0 <= ilo <= ihi < nx and c["sj"] >= 1 and c["si"] >= 1 and c["r"] >= 0
        assert tuple(c["start"]) == (-1, -1) or (jlo <= c["start"][0] <= jhi and ilo <= c["start"][1] <= ihi), c["id"]
        for ring in ({True, False} if c["family"] == "ties" else {c["ring"]}):
            for ln in fc.reference(c["id"], ring)["windows"]:
                assert ln["whole"] or ln["ntile"] <= ln["lds_doubles"], c["id"]
                assert fc.LDS_FIXED + 8 * ln["lds_doubles"] <= fc.LDS_LIMIT
                assert ln["npt"] >= 1


def test_partition_reaches_every_wave_and_trip():
    cases = _family("partition")
    assert not any(a * b == 257 for a in range(1, fc.NY + 1) for b in range(1, fc.NX + 1))          # 258 is the smallest count above 256
    assert {c["expect"]["npt"] for c in cases} == {9, 63, 64, 65, 255, 256, 258, 513}
    seen = set()
    for c in cases:
        ref, n, npt = fc.reference(c["id"]), c["expect"]["n"], c["expect"]["npt"]
        ln = ref["windows"][0]
        nostart = c["id"].endswith("nostart")
        assert ln["npt"] == npt and ln["whole"] == nostart and n < npt and c["r"] == 0
        if nostart:                                            # the admissible count IS the window: it crosses 256 and 512
            jlo, jhi, ilo, ihi = c["bounds"]
            assert (jhi - jlo + 1) * (ihi - ilo + 1) == npt
        elif npt in (64, 256, 258):                            # an odd x odd window cannot give these: the bounds cut it
            assert any(ln["window_cut"].values())
        else:
            assert not any(ln["window_cut"].values()) and npt == (2 * c["sj"] + 1) * (2 * c["si"] + 1)
        # the planted extremum is unique, everything else distinct, and the restatement finds it
        W = ref["W"][0].ravel()
        assert len(set(W.tolist())) == npt and fc.winners(ref["W"][0], c["sense"])["tied"] == [n]
        assert tuple(ref["pos"][0]) == fc._at(ln, n) and ref["val"][0] == fc.BEST[c["sense"]]
        p = fc.place(n)
        seen.add((c["sense"], nostart, p["wave"], p["lane"], p["trip"]))
    for sense in (fc.MIN, fc.MAX):
        for nostart in (False, True):
            got = {s[2:] for s in seen if s[:2] == (sense, nostart)}
            # n = 0, 63, 64, 255, 256, 511, 512: first and last lane of waves 0, 1 and 3 on trips 0, 1 and 2
            assert {(0, 0, 0), (0, 63, 0), (1, 0, 0), (3, 63, 0), (0, 0, 1), (3, 63, 1), (0, 0, 2)} <= got
    counts = sorted({c["expect"]["npt"] for c in cases if c["id"].endswith("nostart")})
    assert any(a <= 256 for a in counts) and any(256 < a <= 512 for a in counts) and any(a > 512 for a in counts)


LAYOUT = {  # layout -> what (place(n1), place(n2)) must look like
    "samewave": lambda a, b: a["trip"] == b["trip"] == 0 and a["wave"] == b["wave"] and a["lane"] != b["lane"],
    "waves": lambda a, b: a["trip"] == b["trip"] == 0 and a["wave"] != b["wave"],
    "wave3-trip1": lambda a, b: (a["trip"], a["wave"]) == (0, 3) and (b["trip"], b["wave"]) == (1, 0),
    "samethread": lambda a, b: a["thread"] == b["thread"] and (a["trip"], b["trip"]) == (0, 1),
    "trip1-trip2": lambda a, b: (a["trip"], b["trip"]) == (1, 2),
}


def test_tie_layouts_sit_where_they_are_named():
    for c in _family("ties"):
        pair, name = c["expect"]["pair"], c["expect"]["layout"]
        assert c["F"].shape[0] == 2                             # a cut in the middle is possible
        for ring in (False, True):
            ref = fc.reference(c["id"], ring)
            assert not ref["status"].any()
            for t, (ln, W) in enumerate(zip(ref["windows"], ref["W"])):
                w = fc.winners(W, c["sense"])
                assert tuple(ref["pos"][t]) == fc._at(ln, w["rule"], fc.NX if ring else None), c["id"]
                if pair is None:
                    nan0 = name.endswith("nan0") and c["r"] == 0
                    assert w["tied"] == list(range(1 if nan0 else 0, ln["npt"])) and ln["npt"] > 256, c["id"]
                    continue
                if ring and t == 1:
                    continue                                    # (the plants are laid out for the plain rule's second window)
                assert w["rule"] == pair[0] and pair[1] in w["tied"] and ln["npt"] == 513, c["id"]
                assert LAYOUT[name](fc.place(pair[0]), fc.place(pair[1])), c["id"]
                if c["r"] == 0:
                    assert w["tied"] == list(pair)
                else:                                           # two plateaus of nine equal means, each beginning at its index
                    assert len(w["tied"]) <= 18 and min(n for n in w["tied"] if n not in _block(pair[0], ln["nxw"])) == pair[1]
    # the two rules agree at step 0 and part at the slice's edge in the all-equal cases' second window
    c = fc.case("tie-allequal-r0-min")
    a, b = fc.reference(c["id"], False), fc.reference(c["id"], True)
    assert np.array_equal(a["pos"][0], b["pos"][0]) and not np.array_equal(a["pos"][1], b["pos"][1])


def _block(n, nxw):
    return {n + dj * nxw + di for dj in range(3) for di in range(3)}


@pytest.mark.parametrize("sense", [fc.MIN, fc.MAX])
def test_ties_tell_the_rule_from_wrong_ones(sense):
    """Last in row-major order; the lowest thread first; the lowest wave first: each is contradicted by at least one case, at r = 0 and at
    r = 1, and the all-equal cases contradict "last"."""
    for r in (0, 1):
        wrong = {"last": [], "thread": [], "wave": []}
        for c in _family("ties"):
            if c["sense"] != sense or c["r"] != r:
                continue
            for W in fc.reference(c["id"])["W"]:
                w = fc.winners(W, sense)
                for rule in wrong:
                    if w[rule] != w["rule"]:
                        wrong[rule].append(c["id"])
        assert all(wrong.values()), wrong
        assert any("allequal" in cid for cid in wrong["last"])
        assert any("wave3-trip1" in cid for cid in wrong["thread"]) and any("trip1-trip2" in cid for cid in wrong["wave"])


def test_clip_cuts_every_edge():
    cases = _family("clip")
    cut_w, cut_t, nb = set(), set(), set()
    for c in cases:
        ref = fc.reference(c["id"])
        ln = ref["windows"][0]
        e = c["expect"]
        if "on" in e:                                           # the centre ON a bound (a corner: on two)
            cuts = {k for k, v in ln["window_cut"].items() if v}
            assert cuts == {"south": {"south"}, "north": {"north"}, "west": {"west"}, "east": {"east"}, "sw": {"south", "west"},
                            "se": {"south", "east"}, "nw": {"north", "west"}, "ne": {"north", "east"}}[e["on"]], c["id"]
            assert not any(ln["tile_cut"].values())
            cut_w |= cuts
        if "corner" in e:                                       # bounds on the slice's edge: the tile is cut by the slice
            assert c["bounds"] == fc.FULL
            cuts = {k for k, v in ln["tile_cut"].items() if v}
            assert cuts == {"sw": {"south", "west"}, "se": {"south", "east"}, "nw": {"north", "west"}, "ne": {"north", "east"}}[e["corner"]] or c["r"] == 0
            cut_t |= cuts
            if c["r"] == 1 and c["field"] == "hgt":             # corner, edge and interior neighbourhoods: 4, 6 and 9 points
                j0, j1, i0, i1 = ln["window"]
                nb |= {(min(j + 1, fc.NY - 1) - max(j - 1, 0) + 1) * (min(i + 1, fc.NX - 1) - max(i - 1, 0) + 1)
                       for j in range(j0, j1 + 1) for i in range(i0, i1 + 1)}
        if e.get("whole"):                                      # sj >= ny, si >= nx: the window is all admissible centres, the tile the slice
            assert c["sj"] >= fc.NY and c["si"] >= fc.NX and ln["window"] == c["bounds"]
            assert ln["lds_doubles"] == fc.NY * fc.NX and (c["bounds"] != fc.FULL or ln["ntile"] == fc.NY * fc.NX)
        if e.get("band"):
            assert c["bounds"][0] == c["bounds"][1] and ln["window"][0] == ln["window"][1]
    assert cut_w == cut_t == {"south", "north", "west", "east"} and nb == {4, 6, 9}
    assert {c["r"] for c in cases if "corner" in c["expect"] and c["field"] == "hgt"} == {1, 2, 4} and all(c["sj"] == 2 for c in cases if c["r"] == 4)


def test_missing_plants_what_it_names():
    for c in _family("missing"):
        ref, F = fc.reference(c["id"]), c["F"]
        ln = ref["windows"][0]
        W = ref["W"][0]
        if "-inf-" in c["id"]:
            j0, j1, i0, i1 = ln["window"]
            raw = F[0][j0: j1 + 1, i0: i1 + 1]
            assert np.isinf(raw).sum() == 2 and np.isfinite(ref["val"]).all()
            n = int(np.argmax(raw) if c["sense"] == fc.MAX else np.argmin(raw))         # the infinity would win
            assert np.isinf(raw.ravel()[n])
            if c["r"] == 0:
                assert np.isnan(W.ravel()[n]) and fc.winners(W, c["sense"])["rule"] == 20
            else:                                               # S beside it is the mean of the finite rest: finite everywhere
                assert np.isfinite(W).all()
        if "-hole-" in c["id"]:
            assert np.isnan(W.ravel()[17]) and np.isfinite(W).sum() == ln["npt"] - 1
        if "-one-" in c["id"]:
            j0, j1, i0, i1 = ln["window"]
            assert np.isfinite(F[0][j0: j1 + 1, i0: i1 + 1]).sum() == 1
            assert np.isfinite(W).sum() == (1 if c["r"] == 0 else 9) and ref["val"][0] == 1234.0
        if "-blind-r" in c["id"]:
            assert ref["status"].tolist() == [0, 1, 0] and np.array_equal(ref["pos"][1], ref["pos"][0]) and np.isnan(ref["val"][1])
        if "-blind-first-" in c["id"]:
            kept = c["bounds"][0::2] if c["id"].endswith("nostart") else c["start"]
            assert ref["status"].tolist() == [1, 0] and tuple(ref["pos"][0]) == tuple(kept)
        assert ln["whole"] == c["id"].endswith("nostart")


def test_ring_tile_runs():
    seen = set()
    for c in _family("ring"):
        ref = fc.reference(c["id"])
        ln = ref["windows"][0]
        it0, it1 = ln["tile"][2:]
        run = c["expect"]["run"]
        assert it1 - it0 + 1 == 2 * c["si"] + 1 + 2 * c["r"] <= fc.RING_NX
        assert {"it0-neg": it0 < 0 and it1 < fc.RING_NX, "it0-zero": it0 == 0, "it1-last": it1 == fc.RING_NX - 1, "it1-over": it1 >= fc.RING_NX and it0 > 0,
                "whole": it1 - it0 + 1 == fc.RING_NX and c["start"][1] != 0, "seam-tie": ln["window"][2] < 0 or ln["window"][3] >= fc.RING_NX}[run], c["id"]
        assert ref["pos"][:, 1].min() >= 0 and ref["pos"][:, 1].max() < fc.RING_NX          # the reported column is i mod nx
        if run == "seam-tie":                                   # column nx - 1 is first in the window's order, and wins
            w = fc.winners(ref["W"][0], c["sense"])
            assert w["tied"] == [n for _, n in c["plants"]] and tuple(ref["pos"][0]) == (8, fc.RING_NX - 1)
            assert fc._at(ln, w["last"], fc.RING_NX) == (8, 0)
        seen.add(run)
    assert seen == {"it0-neg", "it0-zero", "it1-last", "it1-over", "whole", "seam-tie"}


def _owner(c, j, i):
    jlo, jhi, ilo, ihi = c["bounds"]
    return fc.place((j - jlo) * (ihi - ilo + 1) + (i - ilo))


def test_seeds_reach_the_selection_s_seams():
    nas, owners = set(), set()
    for c in SEEDS:
        ref = fc.reference(c["id"])
        jlo, jhi, ilo, ihi = c["bounds"]
        na = (jhi - jlo + 1) * (ihi - ilo + 1)
        assert 1 <= c["k_max"] <= 256 and c["ej"] >= 1 and c["ei"] >= 1
        assert not c["ring"] or (2 * c["ei"] + 1 <= fc.RING_NX and (ilo, ihi) == (0, fc.RING_NX - 1))
        assert np.all(ref["pos"][ref["n_found"]:] == -2) and np.all(np.isnan(ref["val"][ref["n_found"]:]))
        if c["family"] == "seeds-count":
            assert na == c["expect"]["na"]
            nas.add(na)
            found = {tuple(p) for p in ref["pos"][: ref["n_found"]]}
            assert set(c["plants"]) <= found, c["id"]            # every planted index is a seed
            owners |= {(a, _owner(c, *p)["thread"], _owner(c, *p)["trip"]) for a, p in zip(c["expect"]["index"], c["plants"])}
    assert nas == {50, 255, 256, 258, fc.NY * fc.NX}
    assert {(0, 0, 0), (255, 255, 0), (256, 0, 1)} <= owners and any(a == na - 1 for na in nas for a, _, _ in owners)
    # k_max: cuts between two equal candidates, equals the count, is 1, exceeds the count
    for sense, word in fc.SENSES:
        cands = fc.reference(f"seeds-order-k1-{word}")["candidates"]
        n = len(cands)
        assert n == fc.case(f"seeds-order-k1-{word}")["expect"]["ncand"] and cands[3][0] == cands[4][0]
        assert {fc.case(cid)["k_max"] for cid in fc.SEED_FAMILIES["seeds-order"] if cid.endswith(word)} == {1, 4, n, n + 3}
        # equal values are ordered by the slice's row-major index, and the cases can tell: "largest index first" gives another list
        wrong = sorted(cands, key=lambda q: (q[0], -q[1]))
        assert [q[1] for q in wrong[:4]] != [q[1] for q in cands[:4]] and [q[1] for q in wrong] != [q[1] for q in cands]
        lat = fc.reference(f"seeds-lattice-{word}")
        count = fc.case(f"seeds-lattice-{word}")["expect"]["count"]
        assert 190 <= count == lat["n_found"] == len(lat["candidates"]) < 256
        keys = [(q[0], q[1]) for q in lat["candidates"]]
        assert keys == sorted(keys) and len({q[0] for q in lat["candidates"]}) == 10        # many equal values: the index decides
        assert [q[1] for q in sorted(lat["candidates"], key=lambda q: (q[0], -q[1]))] != [q[1] for q in lat["candidates"]]
        for name, kept in (("equal", 3), ("beyond", 2), ("none", 3)):
            cid = f"seeds-thr-{name}-{word}"
            assert len([q for q in fc.reference(cid)["candidates"] if (q[2], q[3]) in fc.case(cid)["plants"]]) == kept == fc.case(cid)["expect"]["kept"]
        assert fc.case(f"seeds-thr-equal-{word}")["threshold"] == fc.reference(f"seeds-thr-equal-{word}")["candidates"][2][4]
        for cid in fc.SEED_FAMILIES["seeds-plateau"]:
            if cid.endswith(word):
                seeded = (15, 20) in {(q[2], q[3]) for q in fc.reference(cid)["candidates"]}
                plateau = {(q[2], q[3]) for q in fc.reference(cid)["candidates"]} & {(15 + dj, 20 + di) for dj in range(2) for di in range(3)}
                assert seeded == fc.case(cid)["expect"]["seeded"] and plateau == ({(15, 20)} if seeded else set()), cid
        edge = fc.reference(f"seeds-edge-{word}")
        got = {tuple(p) for p in edge["pos"][: edge["n_found"]]}
        assert {(0, 0), (0, fc.NX - 1), (fc.NY - 1, 0), (fc.NY - 1, fc.NX - 1), (18, 18)} <= got and (10, 30) not in got
        seam = fc.reference(f"seeds-ring-seam-{word}")
        got = [tuple(p) for p in seam["pos"][: seam["n_found"]]]
        assert (5, 0) in got and (5, fc.RING_NX - 1) not in got and (9, fc.RING_NX - 1) in got and (9, 0) not in got


def test_the_capped_grid_case_takes_the_strided_loop():
    cp = fc.CAPPED
    total = cp["nt"] * cp["ny"] * cp["nx"]
    cap = fc.SERIES_GRID * fc.THREADS
    assert cap == 1 << 24 and cap < total <= cap + cp["ny"] * cp["nx"]          # just above: the last step alone is strided
    assert (cp["nt"] - 1) * cp["ny"] * cp["nx"] <= cap                          # one step fewer would not take the loop
    assert fc.capped_steps() == [0, 4095, 4096]
    pats = fc.capped_patterns()
    assert len({p.tobytes() for p in pats}) == cp["patterns"] == 5
    refs = [fc.seeds(p, fc.MIN, 0, 1, 1, cp["k_max"], None, (0, cp["ny"] - 1, 0, cp["nx"] - 1)) for p in pats]
    assert all(2 <= r["n_found"] <= cp["k_max"] for r in refs) and len({r["pos"].tobytes() for r in refs}) == 5
