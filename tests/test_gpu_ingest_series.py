"""``lec_ingest_series``: the gather pass of ``lec_ingest`` with the packing constants of every SOURCE step taken from a device table
(a series that continues across files: each file packs with its own scale_factor / add_offset / fill value).  Bit for bit against the
per-step host decode of ``oracle/cf_decode.py``, for every source dtype, with and without a fill value and an add_offset (their
presence decides the decode dtype, ``dataset.decode_dtypes``), with and without a ``step_d`` table, and against ``lec_ingest`` itself.

The shape is the smallest that still walks a row and reads every table: 4 source steps, 2 levels through a reversing ``kmap``,
3 of 4 latitudes, 70 of 72 longitudes through a rolled ``imap`` -- one 128-thread workgroup per row with a partial second wave."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from lorenzcycletoolkit_amd import _lib
from lorenzcycletoolkit_amd import dataset as ds
from oracle import cf_decode as cf

pytestmark = pytest.mark.gpu

NT, NL, NY_IN, NX_IN, NY, NX = 4, 2, 4, 72, 3, 70
KMAP = np.array([1, 0], dtype=np.int32)
JMAP = np.array([3, 2, 1, 0], dtype=np.int32)                       # N -> S in the file
IMAP = np.roll(np.arange(NX_IN, dtype=np.int32), 17)                # a rolled longitude axis
SRC = {"i8": (np.int8, _lib.LEC_I8), "i16": (np.int16, _lib.LEC_I16), "i32": (np.int32, _lib.LEC_I32), "f32": (np.float32, _lib.LEC_F32),
       "f64": (np.float64, _lib.LEC_F64)}
CODE = {np.dtype(np.float32): _lib.LEC_F32, np.dtype(np.float64): _lib.LEC_F64}


def _case(kind, fill, offset, equal_rows=False):
    """(source [NT][NL][NY_IN][NX_IN], packing table [NT][3], per-step attributes for the oracle).  Every step has its own scale,
    offset and fill value; every step's data hold ALL the steps' fill values, so a value that is another step's fill must decode."""
    dtype = np.dtype(SRC[kind][0])
    rng = np.random.default_rng(11)
    shape = (NT, NL, NY_IN, NX_IN)
    if dtype.kind == "i":
        info = np.iinfo(dtype)
        src = rng.integers(max(info.min + 8, -30000), min(info.max, 30000), shape).astype(dtype)
        fills = [dtype.type(info.min + s) for s in range(NT)]
    else:
        src = (50.0 * rng.standard_normal(shape)).astype(dtype)
        fills = [dtype.type(9990.0 + s) for s in range(NT)]
    for s in range(NT):
        for q, fv in enumerate(fills):
            src[s, q % NL, (s + q) % NY_IN, 5 + 13 * q: 8 + 13 * q] = fv
    table, attrs = np.zeros((NT, 3)), []
    for s in range(NT):
        r = 0 if equal_rows else s
        scale, off = 0.0031 * (1.0 + 0.37 * r), (10.0 * r - 7.25 if offset else 0.0)
        table[s] = (scale, off, float(fills[r]) if fill else 0.0)
        a = {"scale_factor": np.float64(scale)}
        if offset:
            a["add_offset"] = np.float64(off)
        if fill:
            a["_FillValue"] = fills[r]
        attrs.append(a)
    return src, table, attrs


def _host(src, attrs):
    """Per-step host decode: the oracle's, checked against the package's own."""
    out = []
    for s in range(NT):
        a = cf.decode_cf_variable(src[s], attrs[s])
        fv = attrs[s].get("_FillValue")
        b = ds.decode_values(src[s], float(attrs[s]["scale_factor"]), None if "add_offset" not in attrs[s] else float(attrs[s]["add_offset"]),
                             None if fv is None else float(fv))
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
        out.append(a)
    return np.stack(out)


def _args(src_d, code, out, decode, fill, step=None, step_base=0, maps=None, table_row=None):
    kmap, jmap, imap = maps
    row = (1.0, 0.0, 0.0) if table_row is None else table_row
    return _lib.IngestArgs(
        src_d=src_d.data_ptr(), src_dtype=code, swap_bytes=0, nt=int(out.shape[0]), nl_in=NL, ny_in=NY_IN, nx_in=NX_IN, nl=NL, ny=NY, nx=NX,
        kmap_d=kmap.data_ptr(), jmap_d=jmap.data_ptr(), imap_d=imap.data_ptr(), has_packing=1, has_fill=int(fill),
        scale_factor=row[0], add_offset=row[1], fill_value=row[2], unit_scale=1.0,
        out_dtype=CODE[np.dtype(str(out.dtype).replace("torch.", ""))], decode_dtype=CODE[np.dtype(decode)], out_d=out.data_ptr(),
        stream=torch.cuda.current_stream().cuda_stream, step_d=None if step is None else step.data_ptr(), step_base=step_base,
        nt_src=0 if step is None else NT, jmap_len=0 if step is None else int(jmap.numel()), imap_len=0 if step is None else int(imap.numel()))


def _same(got, want, what):
    """Bit for bit; NaN where the reference has NaN."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    assert np.array_equal(got[~nan].view(u), want[~nan].view(u)), what


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("offset", [True, False], ids=["offset", "scale-only"])
@pytest.mark.parametrize("fill", [True, False], ids=["fill", "nofill"])
@pytest.mark.parametrize("kind", list(SRC))
def test_every_step_is_decoded_with_its_own_row(kind, fill, offset):
    lib = _lib.load()
    src, table, attrs = _case(kind, fill, offset)
    host = _host(src, attrs)                                      # [NT][NL][NY_IN][NX_IN] in the decode dtype of the rules
    decode = host.dtype
    assert decode == ds.decode_dtypes(src.dtype, 1.0, 1.0 if offset else None, 1.0 if fill else None)[1]
    if fill:
        assert all(np.isnan(host[s]).sum() == 3 for s in range(NT))          # that step's fill value alone is masked
    src_d, table_d = _dev(src), _dev(table)
    # --- output step t reads source step t
    maps = (_dev(KMAP), _dev(JMAP[:NY]), _dev(IMAP[:NX]))
    want = host[:, KMAP][:, :, JMAP[:NY]][:, :, :, IMAP[:NX]]
    for out_np in ([np.float32, np.float64] if decode == np.float32 else [np.float64, np.float32]):
        out = torch.full((NT, NL, NY, NX), -1.0, dtype=getattr(torch, np.dtype(out_np).name), device="cuda:0")
        ga = _args(src_d, SRC[kind][1], out, decode, fill, maps=maps)
        _lib.check(lib.lec_ingest_series(C.byref(ga), C.c_void_p(table_d.data_ptr()), NT), "lec_ingest_series")
        torch.cuda.synchronize()
        _same(out.cpu().numpy(), want.astype(out_np), (kind, fill, offset, out_np))
    # --- a step table: shifts -1 / 0 / +1 clipped at the ends, boxes that start elsewhere in the (longer) maps, one entry out of range
    base = 5
    rows = [(int(np.clip(t + shift, 0, NT - 1)), (t + shift) % 2, (t - shift) % 3) for shift in (-1, 0, 1) for t in range(NT)]
    bad = 6
    rows.insert(bad, (NT, 0, 0))                                  # one step past the source: NaN rows, nothing read
    step = _dev(np.array([(s + base, oj, oi) for s, oj, oi in rows], dtype=np.int32))
    maps = (_dev(KMAP), _dev(JMAP), _dev(IMAP))
    out = torch.full((len(rows), NL, NY, NX), -1.0, dtype=getattr(torch, np.dtype(decode).name), device="cuda:0")
    ga = _args(src_d, SRC[kind][1], out, decode, fill, step=step, step_base=base, maps=maps)
    _lib.check(lib.lec_ingest_series(C.byref(ga), C.c_void_p(table_d.data_ptr()), NT), "lec_ingest_series")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for t, (s, oj, oi) in enumerate(rows):
        if t == bad:
            assert np.isnan(got[t]).all()
        else:
            _same(got[t], host[s][KMAP][:, JMAP[oj: oj + NY]][:, :, IMAP[oi: oi + NX]], (kind, fill, offset, "step table", t))


@pytest.mark.parametrize("kind", list(SRC))
def test_equal_rows_give_the_bits_of_lec_ingest(kind):
    lib = _lib.load()
    src, table, attrs = _case(kind, True, True, equal_rows=True)
    assert (table == table[0]).all()
    decode = _host(src, attrs).dtype
    src_d, table_d = _dev(src), _dev(table)
    maps = (_dev(KMAP), _dev(JMAP), _dev(IMAP))
    step = _dev(np.array([(t, t % 2, t % 3) for t in (3, 1, 0, 2, 2)], dtype=np.int32))
    bits = torch.int32 if decode == np.float32 else torch.int64
    for st in (None, step):
        n = NT if st is None else int(st.shape[0])
        m = maps if st is not None else (maps[0], maps[1][:NY], maps[2][:NX])
        one = torch.full((n, NL, NY, NX), -1.0, dtype=getattr(torch, np.dtype(decode).name), device="cuda:0")
        two = torch.full_like(one, -2.0)
        _lib.check(lib.lec_ingest(C.byref(_args(src_d, SRC[kind][1], one, decode, True, step=st, maps=m, table_row=tuple(table[0])))), "lec_ingest")
        _lib.check(lib.lec_ingest_series(C.byref(_args(src_d, SRC[kind][1], two, decode, True, step=st, maps=m)),
                                         C.c_void_p(table_d.data_ptr()), NT), "lec_ingest_series")
        torch.cuda.synchronize()
        assert torch.equal(one.view(bits), two.view(bits)) and not bool((one == -1.0).any())
