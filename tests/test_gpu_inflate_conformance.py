"""lec_inflate against hand-built deflate streams (tests/deflate_cases.py) through the C ABI (GPU): tokens and block structures that
``zlib.compress`` never chooses, aimed at the decoder's seams, and malformed streams with the status each must end with.  zlib is the
oracle (tests/test_deflate_cases_cpu.py pins every case against it without a GPU); both history rings (flags 0 and 2) and both
layouts (streams at multiples of 16, and back to back with every value of ``src_off & 3``) run every case."""
import ctypes as C
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib
from tests import deflate_cases as dc
from tests.test_gpu_inflate import payload

DEV = "cuda:0"
FILL = 0xAA
COMBOS = [(flags, packed) for flags in (0, 2) for packed in (False, True)]


def launch(streams, sizes, *, flags=0, packed=False, first=0, pad=1024, offsets=None):
    """One lec_inflate launch.  Streams lie at multiples of 16, or (``packed``) back to back, stream i at the next offset with
    ``offset & 3 == (first + i) & 3`` (0..3 bytes of 0x55 between two streams), or at ``offsets``; ``pad`` bytes follow the last one.
    Outputs lie at multiples of 16 in a buffer filled with 0xAA.  Returns status, the whole output buffer, the descriptors."""
    lib = _lib.load()
    n = len(streams)
    desc = np.zeros((n, 4), dtype=np.int64)
    so = do = 0
    for i, (s, m) in enumerate(zip(streams, sizes)):
        if offsets is not None:
            so = offsets[i]
        elif packed:
            so += ((first + i) - so) & 3
        else:
            so = (so + 15) & ~15
        desc[i] = (so, len(s), do, m)
        so += len(s)
        do += (m + 15) & ~15
    src = np.full(so + pad, 0x55 if packed else 0, dtype=np.uint8)
    for i, s in enumerate(streams):
        src[desc[i, 0]: desc[i, 0] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    src_d, desc_d = torch.from_numpy(src).to(DEV), torch.from_numpy(desc).to(DEV)
    dst_d = torch.full((do + 16,), FILL, dtype=torch.uint8, device=DEV)
    status_d = torch.full((n, 4), -1, dtype=torch.int32, device=DEV)
    a = _lib.InflateArgs(src_d=src_d.data_ptr(), src_bytes=src.size, desc_d=desc_d.data_ptr(), n_streams=n, flags=flags, dst_d=dst_d.data_ptr(),
                         status_d=status_d.data_ptr(), stream=C.c_void_p(torch.cuda.current_stream().cuda_stream), dst_bytes=dst_d.numel())
    _lib.check(lib.lec_inflate(C.byref(a)), "lec_inflate")
    torch.cuda.synchronize()
    return status_d.cpu().numpy(), dst_d.cpu().numpy(), desc


def check_good(i, name, want, status, out, desc):
    off = int(desc[i, 2])
    assert status[i, 0] == 0, (i, name, status[i].tolist())
    assert status[i, 2] == len(want), (i, name, status[i].tolist())
    got = out[off: off + len(want)].tobytes()
    if got != want:
        at = next(k for k in range(len(want)) if got[k] != want[k])
        raise AssertionError((i, name, "first wrong byte at", at, "of", len(want)))


def check_untouched(out, desc, may_write):
    """Every byte outside the ranges the streams may write still holds the fill value (``may_write``: bytes per stream from its offset)."""
    free = np.ones(out.size, dtype=bool)
    for i, m in enumerate(may_write):
        free[desc[i, 2]: desc[i, 2] + m] = False
    bad = np.flatnonzero(free & (out != FILL))
    assert bad.size == 0, ("written outside any stream's output", bad[:8].tolist())


@pytest.mark.parametrize("flags,packed", COMBOS)
@pytest.mark.parametrize("fam", dc.POSITIVE_FAMILIES)
def test_hand_built_streams_inflate_to_what_zlib_returns(fam, flags, packed):
    """Every positive case of a family in one launch: status 0, zlib's bytes, the size in status[2], and the padding between a stream's
    end and its 16-byte boundary untouched."""
    cases = dc.family(fam)
    cases = cases * -(-4 // len(cases))                               # at least four streams: every src_off & 3 occurs when packed
    first = dc.POSITIVE_FAMILIES.index(fam) & 3
    status, out, desc = launch([c.stream for c in cases], [c.size for c in cases], flags=flags, packed=packed, first=first)
    if packed:
        assert set((desc[:, 0] & 3).tolist()) == {0, 1, 2, 3}
    else:
        assert not (desc[:, 0] & 15).any()
    for i, c in enumerate(cases):
        check_good(i, c.name, dc.zlib_bytes(c.name), status, out, desc)
    check_untouched(out, desc, [c.size for c in cases])


@pytest.mark.parametrize("flags,packed", COMBOS)
def test_refused_streams_end_with_their_status_and_leave_the_neighbours_alone(flags, packed):
    """Every stream zlib refuses, between two good ones: the device refuses it with the code of its fault (any of 8 / 9 / 10 where the
    stream is cut short or the declared size is wrong), the neighbours inflate, nothing is written outside the bad stream's own output."""
    lib = _lib.load()
    good = dc.neighbours()
    entries = []
    for i, bad in enumerate(dc.negative()):
        entries += [good[i % len(good)], bad, good[(i + 3) % len(good)]]
    status, out, desc = launch([c.stream for c in entries], [c.size for c in entries], flags=flags, packed=packed, first=1)
    wrong = []
    for i, c in enumerate(entries):
        if c.expected is not None:
            check_good(i, c.name, c.expected, status, out, desc)
            continue
        code = int(status[i, 0])
        ok = code in c.status if isinstance(c.status, frozenset) else code == c.status
        if not ok or code == 0:
            wrong.append((c.name, code, sorted(c.status) if isinstance(c.status, frozenset) else c.status))
        assert lib.lec_inflate_status_text(code)
    assert not wrong, wrong                                             # (name, the device's code, the code(s) asked for)
    check_untouched(out, desc, [c.size if c.expected is not None else (c.size + 15) & ~15 for c in entries])


def test_a_stream_that_ends_with_the_source_buffer():
    """``src`` sized to the byte, the last stream ending exactly at ``src_bytes`` with src_bytes % 4 = 0..3: the dword view of the input
    drops the buffer's trailing partial dword, where only trailer bytes (read bytewise) may lie.  Huffman and stored final blocks."""
    by_name = {c.name: c for c in dc.positive()}
    before = dc.neighbours()[0]
    lasts = [dc.neighbours()[1], by_name["out0_fixed"], by_name["out17_fixed"], by_name["stored_only_0"], by_name["stored_only_1"],
             by_name["stored_only_1025"], by_name["seek_reset_600"]]
    kinds = {dc.INFO[c.name]["blocks"][-1]["kind"] for c in lasts}
    assert kinds == {"fixed", "stored"}
    for flags in (0, 2):
        for last in lasts:
            for r in range(4):
                lead = (r - len(before.stream) - len(last.stream)) & 3
                offsets = [lead, lead + len(before.stream)]
                status, out, desc = launch([before.stream, last.stream], [before.size, last.size], flags=flags, pad=0, offsets=offsets)
                assert (desc[1, 0] + desc[1, 1]) % 4 == r                # = src_bytes: the stream ends where the buffer does
                check_good(0, before.name, before.expected, status, out, desc)
                check_good(1, last.name, last.expected, status, out, desc)
                check_untouched(out, desc, [before.size, last.size])


@pytest.mark.parametrize("flags", [0, 2])
def test_bit_flipped_streams_are_refused_wherever_zlib_refuses_them(flags):
    """40 zlib streams with 4 random bit flips each: where ``zlib.decompress`` raises the device status is non-zero, where it does not
    the device returns zlib's bytes."""
    rng = np.random.default_rng(77)
    streams, want = [], []
    for k in range(40):
        z = bytearray(zlib.compress(payload(rng, 20000, k % 6), int(rng.integers(1, 10))))
        for _ in range(4):
            z[int(rng.integers(2, len(z)))] ^= 1 << int(rng.integers(0, 8))
        try:
            d = zlib.decompress(bytes(z))
            want.append(d if len(d) == 20000 else None)
        except zlib.error:
            want.append(None)
        streams.append(bytes(z))
    assert sum(w is None for w in want) >= 30
    status, out, desc = launch(streams, [20000] * 40, flags=flags, packed=True)
    accepted = [k for k in range(40) if want[k] is None and status[k, 0] == 0]
    assert not accepted, ("zlib refuses these, the device does not", accepted)
    for k in range(40):
        assert 0 <= status[k, 0] <= 13
        if want[k] is not None:
            check_good(k, "flipped %d" % k, want[k], status, out, desc)
    check_untouched(out, desc, [20000] * 40)
