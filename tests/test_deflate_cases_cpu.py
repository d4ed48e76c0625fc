"""The hand-built deflate streams (tests/deflate_cases.py) are what they claim to be -- checked against zlib alone, without a GPU.

For every positive case the writer's own expansion of the tokens equals ``zlib.decompress``; every negative case makes zlib raise.  And
the coverage the GPU test (tests/test_gpu_inflate_conformance.py) relies on is computed from the token lists and bit positions the
writer recorded, not assumed.  These are conditions on the INPUTS: if one breaks, the case is built again, never the condition relaxed."""
import zlib

import pytest

from tests import deflate_cases as dc


def _blocks(name):
    return dc.INFO[name]["blocks"]


def _out_bytes(tok):
    return 1 if type(tok) is int else tok[0]


def test_every_family_has_cases_and_names_are_unique():
    names = [c.name for c in dc.positive() + dc.negative() + dc.neighbours()]
    assert len(names) == len(set(names))
    for f in dc.POSITIVE_FAMILIES:
        assert dc.family(f), f
    assert {c.family for c in dc.positive()} == set(dc.POSITIVE_FAMILIES)


@pytest.mark.parametrize("fam", dc.POSITIVE_FAMILIES + ("neighbour",))
def test_zlib_returns_the_writers_own_expansion(fam):
    cases = dc.neighbours() if fam == "neighbour" else dc.family(fam)
    for c in cases:
        assert c.status == 0 and c.size == len(c.expected)
        assert zlib.decompress(c.stream) == c.expected, c.name
        assert c.stream[:2] == b"\x78\x01" and c.stream[-4:] == zlib.adler32(c.expected).to_bytes(4, "big")


def test_zlib_refuses_every_negative_case():
    for c in dc.negative():
        assert c.expected is None and c.status != 0 and 0 not in (c.status if isinstance(c.status, frozenset) else ())
        if c.name in dc.SIZE_CASES:                  # a well-formed stream, the wrong size declared to the device
            assert abs(len(zlib.decompress(c.stream)) - c.size) == 1, c.name
            continue
        with pytest.raises(zlib.error):
            zlib.decompress(c.stream)
    sizes = {c.name: len(zlib.decompress(c.stream)) - c.size for c in dc.negative() if c.name in dc.SIZE_CASES}
    assert sizes == {"declared_size_one_less": 1, "declared_size_one_more": -1}
    # the kinds of fault, by the code the device has to report
    by_code = {}
    for c in dc.negative():
        by_code.setdefault(c.status, []).append(c.name)
    assert {k for k in by_code if isinstance(k, int)} == {1, 2, 3, 4, 5, 6, 7, 13}
    assert len(by_code[1]) == 4 and len(by_code[5]) == 3 and len(by_code[dc.TRUNCATED]) >= 10


def test_overlap_family_holds_every_distance_length_pair():
    pairs = []
    for c in dc.family("overlap"):
        blk, = _blocks(c.name)
        assert blk["kind"] == "fixed"
        toks = blk["tokens"]
        d = int(c.name.split("_d")[1])
        assert all(type(t) is int for t in toks[:d]) and type(toks[d]) is tuple          # d literals come first
        ms = [t for t in toks if type(t) is tuple]
        assert all(t[1] == d for t in ms)
        assert all(type(a) is not type(b) for a, b in zip(toks[d:], toks[d + 1:]))         # a literal between consecutive matches
        pairs += [(t[1], t[0]) for t in ms]
    want = {(d, n) for d in range(1, 260) for n in range(3, 259)}
    assert len(pairs) == len(set(pairs)) == 259 * 256 and set(pairs) == want
    assert sum(1 for d, n in want if d < n) == 33152                                      # the overlapping copy form
    assert all((n, n) in want and (n + 1, n) in want for n in range(3, 259))               # its two neighbours that take the plain form


def test_ring_family_aims_at_both_boundaries():
    want = set(range(2900, 4201)) | set(range(5900, 8301))
    ds = sorted(d for d in dc.RING_DISTANCES if d in want)
    assert ds[0] == 2900 and ds[-1] == 8300 and 4200 in ds and 5900 in ds
    assert max(b - a for a, b in zip(ds, ds[1:]) if not a <= 4200 < b) <= 7
    assert {4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768} <= set(dc.RING_DISTANCES)
    # the boundaries themselves: safe_lo lies kRing - kCap - 64 behind the round's start
    assert all(lo <= ring - ring // 4 - 64 <= hi for ring, (lo, hi) in zip(dc.RINGS, ((2900, 4200), (5900, 8300))))
    seen = set()
    for c in dc.family("ring"):
        blocks = _blocks(c.name)
        variant, length = c.name.split("_")[1], int(c.name.split("len")[1])
        history, last = blocks[:-1], blocks[-1]
        assert {b["kind"] for b in history} == {variant} and last["kind"] == ("fixed" if variant == "stored" else "dynamic")
        toks = last["tokens"]
        ms = [t for t in toks if type(t) is tuple]
        assert sorted(t[1] for t in ms) == list(dc.RING_DISTANCES) and {t[0] for t in ms} == {length}
        first_match_at = len(c.expected) - sum(_out_bytes(t) for t in toks)
        assert first_match_at >= 40000
        gaps, run = [], 0
        for t in toks[1:]:
            if type(t) is tuple:
                gaps.append(run); run = 0
            else:
                run += 1
        assert min(gaps) == 0 and max(gaps) == 70 and len(set(gaps)) > 60
        seen.add((variant, length))
    assert seen == {(v, n) for v in ("stored", "dynamic") for n in (3, 63, 64, 65, 257, 258)}


def test_long_code_family_uses_every_combination_at_least_50_times():
    info = dc.INFO["longcodes"]
    assert sorted(dc.LONG_LL.values()) == sorted(dc.LONG_D.values()) == list(range(1, 16)) + [15]
    counts = dict(long_literal=0, long_eob=0, long_len_short_dist=0, short_len_long_dist=0, both_long=0, both_short=0)
    widths = set()
    for blk in info["blocks"]:
        if blk["kind"] != "dynamic":
            continue
        ll, d = blk["ll"], blk["d"]
        assert blk["hlit"] == 286 and blk["hdist"] == 30 and blk["hclen"] == 19
        counts["long_eob"] += ll[256] > 10
        at = blk["token_at"] + [blk["eob_at"]]
        for i, t in enumerate(blk["tokens"]):
            if type(t) is int:
                counts["long_literal"] += ll[t] > 10
                continue
            lsym = 284 if t[2] else dc._LEN_SYM[t[0]][0]
            a, b = ll[lsym] > 10, d[dc._DIST_SYM[t[1]]] > 9
            counts["both_long" if a and b else "long_len_short_dist" if a else "short_len_long_dist" if b else "both_short"] += 1
            widths.add(at[i + 1] - at[i])
    assert all(counts[k] >= 50 for k in ("long_literal", "long_eob", "long_len_short_dist", "short_len_long_dist", "both_long")), counts
    assert max(widths) == 48                                                               # 15 + 5 + 15 + 13: the widest legal token
    # ... which starts at every bit phase of a dword and at every lane of a round (the c one-bit literals before it start the round)
    phases, lanes, spelled = set(), set(), set()
    for b, c in info["wide"]:
        blk = info["blocks"][b]
        at = blk["token_at"]
        assert blk["tokens"][:c] == [0] * c and blk["ll"][0] == 1 and at[c + 1] - at[c] == 48 and at[c] - at[0] == c
        phases.add(at[c] % 32); lanes.add(c); spelled.add(blk["tokens"][c][2])
    assert phases == set(range(32)) and lanes == set(range(64)) and spelled == {False, True}


def test_cap_family_sweeps_the_whole_window_of_both_caps():
    for cap in dc.CAPS:
        info = dc.INFO["cap_%d" % cap]
        first = info["blocks"][0]
        ll, d = first["ll"], first["d"]
        assert ll[285] == 1 and d[0] == 1 and ll[dc.CAP_MID] == 2
        run = best = 0
        for t in first["tokens"]:                       # runs of 40 two-bit matches of 258 bytes: 64 bits hold 32 of them, 8256 bytes
            run = run + 1 if t == dc.match(258, 1) else 0
            best = max(best, run)
        assert best >= 40
        totals = {}
        for b, decide, total in info["sweep"]:
            blk = info["blocks"][b]
            toks, at = blk["tokens"], blk["token_at"]
            assert sum(_out_bytes(t) for t in toks[:decide + 1]) == total and type(toks[decide]) is tuple
            assert at[decide] - at[0] < 64                                                  # the deciding match starts inside the block's first round
            p = next(i for i, t in enumerate(toks) if type(t) is tuple)
            assert all(type(t) is tuple for t in toks[p:decide + 1])                         # p literals, then matches
            totals.setdefault(total, set()).add(p)
        assert set(totals) == set(range(cap - 70, cap + 5))
        assert all(ps == {0, 1, 3} for ps in totals.values())


def test_block_structure_cases_hold_what_their_names_say():
    phases = {b["at"] % 8 for b in _blocks("stored_empty_phases") if b["kind"] == "stored"}
    kinds = [b["kind"] for b in _blocks("stored_empty_phases")]
    assert phases == set(range(8)) and all(kinds[i - 1] == "fixed" for i, k in enumerate(kinds) if k == "stored")
    sizes = [b["size"] for b in _blocks("stored_sizes") if b["kind"] == "stored"]
    assert tuple(sizes[:-1]) == dc.STORED_SIZES == (0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 65535)
    for n in dc.STORED_SIZES:
        assert [b["size"] for b in _blocks("stored_only_%d" % n)] == [n]
    assert [b["kind"] for b in _blocks("empty_fixed_300")][:300] == ["fixed"] * 300
    assert all(b["tokens"] == [] for b in _blocks("empty_fixed_300")[:300])
    assert _blocks("final_eob_only")[-1]["tokens"] == []
    blk, = _blocks("dyn_no_distance_code")
    assert blk["hdist"] == 1 and blk["d"] == (0,) and all(type(t) is int for t in blk["tokens"])
    blk, = _blocks("dyn_one_distance_code")
    assert blk["d"] == (1,) and sum(type(t) is tuple for t in blk["tokens"]) == 40
    assert _blocks("dyn_hclen5")[0]["hclen"] == 5 and _blocks("dyn_hclen19")[0]["hclen"] == 19
    for name, sym in (("dyn_repeat16_crosses", 16), ("dyn_repeat18_crosses", 18)):
        blk = _blocks(name)[-1]
        at, crossing = 0, []
        for s, _, rep in blk["cl_syms"]:
            if at < blk["hlit"] < at + rep:
                crossing.append(s)
            at += rep
        assert at == blk["hlit"] + blk["hdist"] and crossing == [sym], (name, crossing)
    blk = _blocks("dyn_hlit286_hdist30")[-1]
    assert blk["hlit"] == 286 and blk["hdist"] == 30 and blk["ll"][285] and blk["d"][29]
    for name in ("len258_as_284_fixed", "len258_as_284_dynamic"):
        assert sum(1 for t in _blocks(name)[0]["tokens"] if type(t) is tuple and t[2]) >= 3
    # a source in an earlier stored block
    assert any(b["kind"] == "fixed" and any(type(t) is tuple and t[1] >= 1000 for t in b["tokens"]) for b in _blocks("stored_sizes"))


def test_placement_cases():
    sizes = sorted(c.size for c in dc.family("placement") if c.name.startswith("out"))
    assert sizes == [0, 0, 1, 1, 15, 15, 16, 16, 17, 17]
    for c in dc.family("placement"):
        if not c.name.startswith("seek_reset"):
            continue
        blocks = _blocks(c.name)
        assert len(c.stream) > 1024
        assert any(a["kind"] == "stored" and a["size"] >= 600 and b["kind"] == "fixed" for a, b in zip(blocks, blocks[1:]))
