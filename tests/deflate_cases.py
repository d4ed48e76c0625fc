"""Hand-built zlib / deflate streams that cross the seams of lec_inflate.hip, and the token-level writer that makes them.

``zlib.compress`` decides by its own heuristics which tokens a stream holds; the decoder's seams (the 10 / 9-bit lookup tables with the
canonical decode behind them, the three forms of match copy and the ring boundary ``safe_lo``, the round's output cap, the stored-block
chunking, the dword view of the input) are crossed only by streams written token by token.  The writer here (RFC 1950 / 1951, nothing
imported from the package) takes blocks -- stored bytes, fixed-Huffman tokens, dynamic-Huffman tokens with prescribed code lengths and
a prescribed encoding of the header -- and expands the tokens itself, so every positive case carries two independent statements of
its bytes: the expansion and ``zlib.decompress`` (tests/test_deflate_cases_cpu.py holds them against each other, and asserts what
the GPU test relies on: which (distance, length) pairs, code widths, round totals and bit phases really occur).

Every stream is generated from a seeded generator; building all of them takes a few seconds."""
import functools
import zlib
from collections import namedtuple

import numpy as np

LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577)
DEXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = tuple([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_D = tuple([5] * 32)

# the decoder's constants the cases aim at (lec_inflate.hip): ring sizes, kCap = ring / 4, and how far back the ring serves a match
RINGS = (4096, 8192)
CAPS = (1024, 2048)

_LEN_SYM = {}
for _c in range(28):
    for _x in range(1 << LEXTRA[_c]):
        _LEN_SYM.setdefault(LBASE[_c] + _x, (257 + _c, LEXTRA[_c], _x))
_LEN_SYM[258] = (285, 0, 0)                 # (symbol 284 + extra 31 is the other spelling: match(258, d, as_284=True))
_DIST_SYM = np.zeros(32769, dtype=np.int64)
for _c in range(30):
    _DIST_SYM[DBASE[_c]: DBASE[_c] + (1 << DEXTRA[_c])] = _c
_DIST_SYM = _DIST_SYM.tolist()


def lit(b):
    return int(b)


def match(length, distance, as_284=False):
    assert 3 <= length <= 258 and 1 <= distance <= 32768 and (not as_284 or length == 258)
    return (length, distance, as_284)


def raw_ll(sym):
    """The literal/length code of ``sym`` and nothing else (bad-symbol cases)."""
    return ("ll", sym)


def raw_d(sym):
    return ("dd", sym)


def raw_bits(value, n):
    return ("x", value, n)


def kraft(lengths):
    """Sum of 2^-len in units of 2^-15: 32768 is a complete code."""
    return sum(1 << (15 - l) for l in lengths if l)


def canonical(lengths):
    """RFC 1951 3.2.2: per symbol (code bit-reversed for an LSB-first writer, length)."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        if l == 0:
            out.append((0, 0))
            continue
        c = nxt[l] & ((1 << l) - 1)
        nxt[l] += 1
        out.append((int(format(c, "0%db" % l)[::-1], 2), l))
    return out


class Bits:
    """LSB-first bit writer: bits gather in one integer and leave as whole bytes."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits
        if self.n >= 256:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def align(self):
        self.put(0, -self.n % 8)

    def put_bytes(self, data):
        self.align()
        k = self.n >> 3
        self.out += self.acc.to_bytes(k, "little")
        self.acc = self.n = 0
        self.out += data

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bytes(self):
        self.put_bytes(b"")
        return bytes(self.out)


def encode_lengths(seq, rle):
    """Code lengths -> symbols of the code-length alphabet, (symbol, extra value, repeat); ``rle`` uses 16 / 17 / 18 greedily over the
    WHOLE sequence (literal/length lengths followed by distance lengths: a run crosses from one into the other, as the format allows)."""
    if not rle:
        return [(l, 0, 1) for l in seq]
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11, r)); run -= r
            if run >= 3:
                out.append((17, run - 3, run)); run = 0
        else:
            out.append((v, 0, 1)); run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3, r)); run -= r
        out += [(v, 0, 1)] * run
        i = j
    return out


def balanced_code(n):
    """Lengths of a complete code of n >= 2 symbols (zlib refuses an incomplete code-length code)."""
    k = n.bit_length() - 1
    r = n - (1 << k)
    return [k + 1] * (2 * r) + [k] * (n - 2 * r)


class Stream:
    """One zlib stream under construction.  ``out`` is the writer's own expansion of the tokens; ``blocks`` records, per block, its
    kind, the bit position of its header, its tokens with the bit position of each, and its code lengths (what the coverage
    assertions are computed from)."""

    def __init__(self, header=b"\x78\x01"):
        self.bw = Bits()
        self.bw.put_bytes(header)
        self.out = bytearray()
        self.blocks = []
        self.broken = False             # a token that cannot be expanded (negative cases)

    # ---- blocks
    def stored(self, data, final=False, nlen=None):
        data = bytes(data)
        assert len(data) <= 65535
        self.blocks.append(dict(kind="stored", at=self.bw.bitpos, size=len(data)))
        self.bw.put(int(final), 3)
        self.bw.align()
        self.bw.put(len(data), 16)
        self.bw.put((len(data) ^ 0xffff) if nlen is None else nlen, 16)
        self.bw.put_bytes(data)
        self.out += data
        return self

    def fixed(self, tokens, final=False):
        self.blocks.append(dict(kind="fixed", at=self.bw.bitpos, ll=FIXED_LL, d=FIXED_D))
        self.bw.put(int(final) | 2, 3)
        self._tokens(tokens, canonical(FIXED_LL), canonical(FIXED_D))
        return self

    def dynamic(self, tokens, ll_lens, d_lens, final=False, rle=False, hclen=None, hlit=None, hdist=None, cl_syms=None, cl_lens=None,
                check=True, eob=True):
        """``ll_lens`` / ``d_lens``: code length per symbol (shorter lists are padded with 0).  ``hlit`` / ``hdist``: number of codes the
        header declares (default: up to the last used one); ``rle`` / ``cl_syms``: how the lengths are written; ``hclen``: number of
        code-length-code lengths (default: as few as the format allows); ``check=False`` switches the Kraft checks off (negative cases)."""
        ll_lens, d_lens = list(ll_lens), list(d_lens)
        if hlit is None:
            hlit = max(257, max((i + 1 for i, l in enumerate(ll_lens) if l), default=0))
        if hdist is None:
            hdist = max(1, max((i + 1 for i, l in enumerate(d_lens) if l), default=0))
        ll_lens = (ll_lens + [0] * 288)[:hlit]
        d_lens = (d_lens + [0] * 32)[:hdist]
        if check:
            assert 257 <= hlit <= 286 and 1 <= hdist <= 30
            assert kraft(ll_lens) <= 32768 and kraft(d_lens) <= 32768, "over-subscribed code"
        syms = encode_lengths(ll_lens + d_lens, rle) if cl_syms is None else list(cl_syms)
        if cl_lens is None:
            used = sorted({s for s, _, _ in syms})
            if len(used) < 2:
                used = sorted(set(used) | {0 if 0 not in used else 18})
            cl_lens = [0] * 19
            for s, l in zip(used, balanced_code(len(used))):
                cl_lens[s] = l
        if check:
            assert kraft(cl_lens) == 32768 and max(cl_lens) <= 7
        need = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        hclen = need if hclen is None else hclen
        assert need <= hclen <= 19 or not check
        self.blocks.append(dict(kind="dynamic", at=self.bw.bitpos, ll=tuple(ll_lens), d=tuple(d_lens), hlit=hlit, hdist=hdist, hclen=hclen,
                                cl_syms=syms))
        bw = self.bw
        bw.put(int(final) | 4, 3)
        bw.put(hlit - 257, 5); bw.put(hdist - 1, 5); bw.put(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            bw.put(cl_lens[s], 3)
        clc = canonical(cl_lens)
        for s, x, _ in syms:
            bw.put(*clc[s])
            if s >= 16:
                bw.put(x, (2, 3, 7)[s - 16])
        self._tokens(tokens, canonical(ll_lens + [0] * (288 - len(ll_lens))), canonical(d_lens + [0] * (32 - len(d_lens))), eob)
        return self

    def raw(self, value, nbits):
        self.bw.put(value, nbits)
        return self

    def _tokens(self, tokens, ll, dd, eob=True):
        bw, out, blk = self.bw, self.out, self.blocks[-1]
        put = bw.put
        at = []
        for t in tokens:
            at.append(bw.bitpos)
            if type(t) is int:
                c, l = ll[t]
                assert l, ("literal without a code", t)
                put(c, l)
                out.append(t)
            elif t[0] == "ll":
                put(*ll[t[1]]); self.broken = True
            elif t[0] == "dd":
                put(*dd[t[1]]); self.broken = True
            elif t[0] == "x":
                put(t[1], t[2]); self.broken = True
            else:
                length, dist, alt = t
                sym, nx, x = (284, 5, 31) if alt else _LEN_SYM[length]
                c, l = ll[sym]
                assert l, ("length symbol without a code", sym)
                put(c | (x << l), l + nx)
                ds = _DIST_SYM[dist]
                c, l = dd[ds]
                assert l, ("distance symbol without a code", ds)
                put(c | ((dist - DBASE[ds]) << l), l + DEXTRA[ds])
                n = len(out)
                if dist > n:
                    self.broken = True
                elif dist >= length:
                    out += out[n - dist: n - dist + length]
                else:
                    out += (out[n - dist:] * (length // dist + 1))[:length]
        blk["tokens"], blk["token_at"] = list(tokens), at
        blk["eob_at"] = bw.bitpos
        if eob:
            put(*ll[256])

    def finish(self, adler=None, trailer=4):
        a = zlib.adler32(bytes(self.out)) if adler is None else adler
        return self.bw.bytes() + a.to_bytes(4, "big")[:trailer]


# a case: ``expected`` None for a stream zlib refuses; ``status``: the code the device must report, or a frozenset of acceptable ones;
# ``size``: the output size declared to the device
Case = namedtuple("Case", "name family stream expected status size")
TRUNCATED = frozenset({8, 9, 10})

POSITIVE_FAMILIES = ("overlap", "ring", "longcodes", "cap", "blocks", "placement")
INFO = {}           # case name -> the Stream's block records (and, per family, what the coverage assertions need)


def _pos(family, name, s, **info):
    stream = s.finish()
    assert not s.broken
    INFO[name] = dict(blocks=s.blocks, **info)
    return Case(name, family, stream, bytes(s.out), 0, len(s.out))


def _rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


# ---------------------------------------------------------------------------------------------------------------- positive cases
def _overlap():
    """Every (distance, length) with 1 <= d <= 259, 3 <= len <= 258: one stream per distance, d random literals, then the matches in
    random order of length with a random literal between them (d < len: the overlapping copy form; d == len, len + 1: the plain one)."""
    rng = np.random.default_rng(101)
    cases = []
    for d in range(1, 260):
        toks = list(_rand(rng, d))
        lits = _rand(rng, 256)
        for k, length in enumerate(rng.permutation(np.arange(3, 259)).tolist()):
            toks.append(match(length, d))
            toks.append(lits[k])
        cases.append(_pos("overlap", "overlap_d%d" % d, Stream().fixed(toks, final=True)))
    return cases


RING_LENGTHS = (3, 63, 64, 65, 257, 258)
RING_DISTANCES = tuple(sorted(set(range(2900, 4201, 7)) | {4200} | set(range(5900, 8301, 7)) | {8300}
                              | {4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768}))
# literals 0..255 in 9 bits, end-of-block in 2, the four length symbols the ring lengths need in 4 bits each; 30 distance codes
_RING_LL = [9] * 256 + [2] + [0] * 29
for _s in {_LEN_SYM[n][0] for n in RING_LENGTHS}:
    _RING_LL[_s] = 4
_RING_D = [4, 4] + [5] * 28


def _ring():
    """Matches aimed at the band where a source stops being served from the LDS ring (6080 / 3008 bytes behind the ROUND's start): after
    40 KB of random bytes, every distance of RING_DISTANCES with one length each per stream, 0..70 random literals between matches so
    that a match falls early, mid and late in a round.  History in stored blocks, or in an earlier dynamic block."""
    rng = np.random.default_rng(102)
    cases = []
    for variant in ("stored", "dynamic"):
        for length in RING_LENGTHS:
            toks = []
            for d in rng.permutation(np.array(RING_DISTANCES)).tolist():
                toks.append(match(length, d))
                toks += list(_rand(rng, int(rng.integers(0, 71))))
            s = Stream()
            if variant == "stored":
                s.stored(_rand(rng, 30000)).stored(_rand(rng, 11000)).fixed(toks, final=True)
            else:
                s.dynamic(list(_rand(rng, 41000)), _RING_LL, _RING_D).dynamic(toks, _RING_LL, _RING_D, final=True, rle=True)
            cases.append(_pos("ring", "ring_%s_len%d" % (variant, length), s))
    return cases


# literal/length and distance codes with lengths 1, 2, ..., 14, 15, 15 (complete): symbol -> length
LONG_LL = {0: 1, 258: 2, 1: 3, 273: 4, 2: 5, 3: 6, 4: 7, 5: 8, 6: 9, 280: 10, 7: 11, 262: 12, 8: 13, 285: 14, 284: 15, 256: 15}
LONG_D = {0: 1, 5: 2, 10: 3, 3: 4, 12: 5, 14: 6, 16: 7, 18: 8, 20: 9, 22: 10, 24: 11, 26: 12, 1: 13, 2: 14, 29: 15, 28: 15}


def _lens(table, n):
    out = [0] * n
    for s, l in table.items():
        out[s] = l
    return out


def _longcodes():
    """Codes longer than the lookup widths (10 bits literal/length, 9 bits distance), reached on purpose: 256 dynamic blocks with the
    codes above (HLIT 286, HDIST 30, HCLEN 19).  Block (c, r) holds c one-bit literals, then the widest legal token -- 15 + 5 + 15 + 13 = 48
    bits -- at lane c of the block's first round, then a long literal, long length + short distance, short length + long distance, both
    long, a long literal and the 15-bit end-of-block.  0..3 empty fixed blocks before each block move its bit phase."""
    rng = np.random.default_rng(103)
    ll, dl = _lens(LONG_LL, 286), _lens(LONG_D, 30)
    s = Stream().stored(_rand(rng, 33000))
    wide = []
    for r in range(4):
        for c in range(64):
            for _ in range(int(rng.integers(0, 4))):
                s.fixed([])
            w = match(227 + int(rng.integers(0, 31)), 24577 + int(rng.integers(0, 8192))) if (c + r) % 5 else \
                match(258, 24577 + int(rng.integers(0, 8192)), as_284=True)
            toks = [0] * c + [w, 7, match(8, 1), match(4, 4097 + int(rng.integers(0, 2048))),
                              match(258, 16385 + int(rng.integers(0, 8192))), match(4, 2), 8, 3]
            s.dynamic(toks, ll, dl, rle=bool(c & 1))
            wide.append((len(s.blocks) - 1, c))
    s.fixed([], final=True)
    return [_pos("longcodes", "longcodes", s, wide=wide)]


CAP_MID = 281                              # lengths 131..162
CAP_LL = {285: 1, CAP_MID: 2, 0x41: 3, 0x42: 4, 256: 4}
CAP_D = {0: 1, 1: 1}


def _cap_plan(total, p):
    """``total`` output bytes as p literals, then a 258-matches, then mid-length matches, the last of which decides; fewest bits first."""
    for n258 in range(7, -1, -1):
        rest = total - p - 258 * n258
        for nmid in range(1, 7):
            if 131 * nmid <= rest <= 162 * nmid and 4 * p + 2 * n258 + 8 * (nmid - 1) <= 60:
                base, extra = divmod(rest, nmid)
                return n258, [base + (1 if k < extra else 0) for k in range(nmid)]
    raise AssertionError((total, p))


def _cap():
    """The round's output cap (kCap = 1024 / 2048): 1-bit codes for length 258 and distance 1, so 64 bits of stream hold far more
    output than a round may produce.  Runs of 40 such matches; then one block per (total, p): p literals, 258-matches and mid-length
    matches whose running total, through the deciding (last) match, is ``total`` -- every value from kCap - 70 to kCap + 4, all within
    the 64 lanes of the block's first round -- followed by tokens that read what the round wrote."""
    rng = np.random.default_rng(104)
    ll, dl = _lens(CAP_LL, 286), _lens(CAP_D, 2)
    cases = []
    for cap in CAPS:
        s = Stream()
        toks = [0x41, 0x42]
        for _ in range(3):
            toks += [match(258, 1)] * 40 + [0x42, 0x41, match(258, 2)] + [match(258, 1)] * 40 + [0x41]
        s.dynamic(toks, ll, dl)
        sweep = []
        for total in range(cap - 70, cap + 5):
            for p in (0, 1, 3):
                n258, mids = _cap_plan(total, p)
                toks = [int(rng.choice([0x41, 0x42])) for _ in range(p)] + [match(258, 1 + int(rng.integers(0, 2))) for _ in range(n258)]
                toks += [match(m, 1 + int(rng.integers(0, 2))) for m in mids]
                decide = len(toks) - 1
                toks += [0x42, match(150, 2), 0x41, 0x41, 0x42, match(258, 2), 0x41]
                s.dynamic(toks, ll, dl, rle=True)
                sweep.append((len(s.blocks) - 1, decide, total))
        s.fixed([], final=True)
        cases.append(_pos("cap", "cap_%d" % cap, s, sweep=sweep, cap=cap))
    return cases


ONE_LL = [8] * 253 + [0, 0, 0, 8, 8, 8]     # 253 literals, end-of-block, length symbols 257 and 258: complete
STORED_SIZES = (0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 65535)


def _blocks():
    rng = np.random.default_rng(105)
    cases = []
    # an empty stored block after a Huffman block, at every bit phase
    s = Stream()
    for k in range(24):                         # a fixed block after a byte boundary ends at bit 3 + 8 n + (9-bit literals) + 7
        toks = rng.integers(144, 256, k % 8).tolist() + rng.integers(0, 144, int(rng.integers(0, 4))).tolist()
        s.fixed([int(t) for t in rng.permutation(toks)]).stored(b"")
    s.fixed([1, 2, 3], final=True)
    cases.append(_pos("blocks", "stored_empty_phases", s))
    # stored blocks around kCap for both rings, the largest one, and matches whose source lies in the stored block before them
    s = Stream()
    for n in STORED_SIZES:
        s.stored(_rand(rng, n))
        have = len(s.out)
        if have:
            s.fixed([match(min(258, max(3, have)), d) for d in sorted({1, min(have, 2), min(have, 1000), min(have, 4000), min(have, 32768)})])
    s.stored(_rand(rng, 100), final=True)
    cases.append(_pos("blocks", "stored_sizes", s))
    for n in STORED_SIZES:                      # ... and each size alone, as the stream's only and final block
        cases.append(_pos("blocks", "stored_only_%d" % n, Stream().stored(_rand(rng, n), final=True)))
    s = Stream()
    for _ in range(300):
        s.fixed([])
    cases.append(_pos("blocks", "empty_fixed_300", s.fixed([5, 6, 7], final=True)))
    cases.append(_pos("blocks", "final_eob_only", Stream().fixed(list(_rand(rng, 40)) + [match(30, 7)]).fixed([], final=True)))
    # no distance code at all (HDIST = 1, its length 0): literals only
    flat = [8] * 255 + [0, 8]                   # 255 literals and end-of-block in 8 bits: complete
    body = [int(b) for b in rng.integers(0, 255, 500)]
    cases.append(_pos("blocks", "dyn_no_distance_code", Stream().dynamic(body, flat, [0], final=True)))
    # ... the same code at the smallest HCLEN a valid block can have (5: the code lengths 0 and 8; with 4 no symbol gets a code)
    cases.append(_pos("blocks", "dyn_hclen5", Stream().dynamic(body, flat, [0], final=True, rle=True, hclen=5)))
    # the single distance code of length 1 (an incomplete code the format allows), used 40 times
    one = ONE_LL
    toks = [int(b) for b in rng.integers(0, 253, 10)]
    for k in range(40):
        toks += [match(3 + (k & 1), 1), int(rng.integers(0, 253))]
    cases.append(_pos("blocks", "dyn_one_distance_code", Stream().dynamic(toks, one, [1], final=True)))
    cases.append(_pos("blocks", "dyn_hclen19", Stream().dynamic(toks, one, [1], final=True, hclen=19)))
    # repeat symbols that run from the literal/length lengths into the distance lengths: 16 (three 4s, then sixteen 4s) and 18 (28 + 14 zeros)
    ll16 = [8] * 192 + [0] * 64 + [4, 4, 4, 4]
    toks = [int(b) for b in rng.integers(0, 192, 300)]
    for k in range(30):
        toks += [match(3 + k % 3, 1 + k % 16), int(rng.integers(0, 192))]
    cases.append(_pos("blocks", "dyn_repeat16_crosses", Stream().dynamic(toks, ll16, [4] * 16, final=True, rle=True)))
    ll18 = [8] * 254 + [0, 0, 8, 7]             # 254 literals + end-of-block in 8, symbol 257 in 7: 255/256 + 2/256 -> see below
    ll18[0] = 0                                 # (one literal less keeps the code complete)
    toks = [int(b) for b in rng.integers(1, 254, 300)]
    for k in range(30):
        toks += [match(3, 20000 + 37 * k) if k > 26 else match(3, 129 + k), int(rng.integers(1, 254))]
    cases.append(_pos("blocks", "dyn_repeat18_crosses", Stream().stored(_rand(rng, 33000)).dynamic(toks, ll18, [0] * 14 + [4] * 16, final=True, rle=True, hlit=286)))
    # HLIT = 286 with HDIST = 30, in a small block
    cases.append(_pos("blocks", "dyn_hlit286_hdist30", Stream().stored(_rand(rng, 33000)).dynamic(
        [9, match(258, 30000), 10, match(258, 24577)], [8] * 254 + [0, 0, 8] + [0] * 28 + [8], [0] * 29 + [1], final=True, hlit=286, hdist=30)))
    # length 258 spelled as symbol 284 + extra 31, fixed and dynamic
    toks = [65, match(258, 1, as_284=True), 66, 67, match(258, 2, as_284=True), match(258, 258, as_284=True), match(258, 259), 68]
    cases.append(_pos("blocks", "len258_as_284_fixed", Stream().fixed(toks, final=True)))
    cases.append(_pos("blocks", "len258_as_284_dynamic", Stream().dynamic(toks[:-2] + [68], [8] * 254 + [0, 0, 8] + [0] * 27 + [8], _RING_D, final=True)))
    return cases


def _placement():
    rng = np.random.default_rng(106)
    cases = []
    for n in (0, 1, 15, 16, 17):
        data = list(_rand(rng, n))
        cases.append(_pos("placement", "out%d_fixed" % n, Stream().fixed(data, final=True)))
        cases.append(_pos("placement", "out%d_stored" % n, Stream().stored(bytes(data), final=True)))
    # a stored block of >= 600 bytes, then a Huffman block: the bit reader jumps more than 512 bytes (BitIn::seek's reset branch)
    for n in (600, 777, 5000):
        toks = list(_rand(rng, 50)) + [match(100, n), match(258, 3), 1, 2, match(7, 40)]
        cases.append(_pos("placement", "seek_reset_%d" % n, Stream().fixed(list(_rand(rng, 9))).stored(_rand(rng, n)).fixed(toks).stored(_rand(rng, n + 1)).fixed(toks, final=True)))
    return cases


@functools.lru_cache(maxsize=None)
def positive():
    return tuple(_overlap() + _ring() + _longcodes() + _cap() + _blocks() + _placement())


def family(name):
    return tuple(c for c in positive() if c.family == name)


@functools.lru_cache(maxsize=None)
def zlib_bytes(name):
    """What zlib returns for a positive case: the reference of the GPU test (computed once)."""
    return zlib.decompress({c.name: c for c in positive()}[name].stream)


# ---------------------------------------------------------------------------------------------------------------- negative cases
def _header(cm=8, cinfo=7, fdict=0, fcheck_off=0):
    cmf = cm | (cinfo << 4)
    flg = fdict << 5
    flg += (31 - ((cmf << 8) | flg) % 31) % 31
    return bytes([cmf, (flg + fcheck_off) & 0xff])


def _neg(name, stream, status, size=64):
    return Case(name, "negative", stream, None, status, size)


@functools.lru_cache(maxsize=None)
def negative():
    rng = np.random.default_rng(107)
    body = list(_rand(rng, 40)) + [match(20, 5)]
    flat = [8] * 255 + [0, 8]
    lits = [int(b) for b in rng.integers(0, 253, 60)]
    tail = lambda s: s.fixed(body, final=True).finish()         # a well-formed rest behind the fault
    cases = []
    # --- header
    for name, h in (("header_cm9", _header(cm=9)), ("header_cinfo8", _header(cinfo=8)), ("header_fcheck", _header(fcheck_off=1)),
                    ("header_fdict", _header(fdict=1))):
        cases.append(_neg(name, Stream(h).fixed(body, final=True).finish(), 1))
    # --- block type, stored length check
    cases.append(_neg("block_type_3", tail(Stream().fixed(body).raw(6, 3).raw(0x5a5a5a, 24)), 2))
    cases.append(_neg("block_type_3_first", tail(Stream().raw(7, 3).raw(0, 13)), 2))
    cases.append(_neg("stored_len_nlen", tail(Stream().fixed(body).stored(b"abcdefgh", nlen=0xfff6)), 3))
    # --- dynamic block headers
    big_ll, big_d = [8] * 255 + [0, 8] + [0] * 31, [1, 1] + [0] * 30
    for n in (287, 288):
        cases.append(_neg("dyn_hlit_%d" % n, tail(Stream().fixed(body).dynamic(lits, big_ll, big_d, hlit=n, check=False)), 4))
    for n in (31, 32):
        cases.append(_neg("dyn_hdist_%d" % n, tail(Stream().fixed(body).dynamic(lits, big_ll, big_d, hdist=n, check=False)), 4))
    plain = encode_lengths(flat + [0], False)
    cl = [0] * 19
    cl[0], cl[8], cl[16], cl[18] = 2, 2, 2, 2
    cases.append(_neg("dyn_repeat16_first", tail(Stream().dynamic(lits, flat, [0], cl_syms=[(16, 0, 3)] + plain[3:], cl_lens=cl, check=False)), 4))
    cases.append(_neg("dyn_repeat_overruns", tail(Stream().dynamic(lits, flat, [0], cl_syms=plain[:-5] + [(18, 0, 11)], cl_lens=cl, check=False)), 4))
    cases.append(_neg("dyn_repeat16_overruns", tail(Stream().dynamic(lits, flat, [0], cl_syms=plain[:-1] + [(16, 3, 6)], cl_lens=cl, check=False)), 4))
    no_eob = [8] * 256 + [0]
    cases.append(_neg("dyn_no_end_of_block", tail(Stream().dynamic(lits, no_eob, [0], hlit=257, eob=False)), 4))
    # HCLEN = 4 lists lengths for 16, 17, 18 and 0 only: every code length is then 0 and there is no end-of-block code -- not a valid block
    cl4 = [0] * 19
    cl4[16], cl4[17], cl4[18], cl4[0] = 2, 2, 2, 2
    cases.append(_neg("dyn_hclen4", tail(Stream().dynamic([], [0] * 257, [0], cl_syms=[(18, 127, 138), (18, 109, 120)], cl_lens=cl4, hclen=4,
                                                         check=False, eob=False)), 4))
    over = [0] * 19
    over[0], over[8], over[18] = 1, 1, 1
    cases.append(_neg("dyn_oversubscribed_code_length_code", tail(Stream().dynamic(lits, flat, [0], cl_syms=plain, cl_lens=over, check=False)), 5))
    cases.append(_neg("dyn_oversubscribed_literal_code", tail(Stream().dynamic([], [8] * 255 + [8, 8, 8], [0], check=False, eob=False)), 5))
    cases.append(_neg("dyn_oversubscribed_distance_code", tail(Stream().dynamic([], flat, [1, 1, 1], check=False, eob=False)), 5))
    # --- symbols that have a code but no meaning, and a bit pattern without a code
    for sym in (286, 287):
        cases.append(_neg("fixed_symbol_%d" % sym, tail(Stream().fixed(body + [raw_ll(sym)] + body)), 6, size=200))
    for sym in (30, 31):
        cases.append(_neg("fixed_distance_symbol_%d" % sym, tail(Stream().fixed(body + [raw_ll(260), raw_d(sym)] + body)), 6, size=200))
    one = ONE_LL
    cases.append(_neg("one_distance_code_other_bit", tail(Stream().dynamic([1, 2, 3, match(3, 1), raw_ll(257), raw_bits(1, 1), 4, 5, 6, 7], one, [1])), 6, size=200))
    # --- a distance that reaches before the start of the output
    cases.append(_neg("distance_1_at_0", Stream().fixed([match(3, 1), 1, 2], final=True).finish(), 7, size=5))
    cases.append(_neg("distance_5001_at_5000", Stream().stored(_rand(rng, 5000)).fixed([match(3, 5001), 1, 2], final=True).finish(), 7, size=5005))
    cases.append(_neg("distance_3_at_2_same_round", Stream().fixed([1, 2, match(5, 3), 1, 2], final=True).finish(), 7, size=9))
    # --- truncation after each structural piece, and the trailer
    s = Stream().dynamic(lits + [match(4, 1)] * 30 + lits, one, [1], final=True)
    good = s.finish()
    assert zlib.decompress(good) == bytes(s.out)
    n_out = len(s.out)
    blk = s.blocks[0]
    cuts = {"after_header": 2, "after_block_header": 3, "in_code_length_code": 6, "in_code_length_list": 20,
            "in_tokens": blk["token_at"][70] // 8, "in_last_tokens": blk["eob_at"] // 8 - 1, "before_trailer": len(good) - 4}
    assert 8 * cuts["in_code_length_list"] < blk["token_at"][0] - 64
    for name, n in cuts.items():
        cases.append(_neg("truncated_" + name, good[:n], TRUNCATED, size=n_out))
    st = Stream().fixed(body).stored(_rand(rng, 300), final=True)
    goods = st.finish()
    cases.append(_neg("truncated_in_stored_lengths", goods[: st.blocks[1]["at"] // 8 + 3], TRUNCATED, size=len(st.out)))
    cases.append(_neg("truncated_in_stored_bytes", goods[:-100], TRUNCATED, size=len(st.out)))
    for k in (1, 2, 3):
        cases.append(_neg("trailer_short_by_%d" % k, good[:-k], TRUNCATED, size=n_out))
    cases.append(_neg("adler_wrong", good[:-1] + bytes([good[-1] ^ 1]), 13, size=n_out))
    cases.append(_neg("adler_wrong_stored", Stream().stored(_rand(rng, 3000), final=True).finish(adler=1), 13, size=3000))
    cases.append(_neg("declared_size_one_less", good, TRUNCATED, size=n_out - 1))
    cases.append(_neg("declared_size_one_more", good, TRUNCATED, size=n_out + 1))
    return tuple(cases)


SIZE_CASES = ("declared_size_one_less", "declared_size_one_more")


@functools.lru_cache(maxsize=None)
def neighbours():
    """Small well-formed streams to put on either side of a bad one."""
    rng = np.random.default_rng(108)
    out = []
    for k in range(8):
        toks = list(_rand(rng, 30 + 11 * k)) + [match(40 + k, 7 + k), match(258, 1), 9]
        s = Stream().fixed(toks, final=True) if k & 1 else Stream().stored(_rand(rng, 50)).fixed(toks, final=True)
        out.append(_pos("neighbour", "neighbour_%d" % k, s))
    return tuple(out)
