"""``--series``: a time series that continues across files, on the host -- the command line, the opening rules of
``dataset._open_parts``, the host decode, the raw (streamed) view of the parts and the argument checks of ``lec_ingest_series``.
Comparisons are bit for bit: the merged file holds each part's values as ``oracle/cf_decode.py`` decodes them (tests/series_cases.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib
from lorenzcycletoolkit_amd import dataset as ds
from tests import series_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    root = tmp_path_factory.mktemp("series")
    parts, merged, packed, decoded = sc.standard_case(root)
    (root / "namelist").write_text(sc.NAMELIST)
    return dict(root=root, parts=parts, merged=merged, packed=packed, decoded=decoded, df=ds.read_namelist(str(root / "namelist")),
                namelist=str(root / "namelist"))


def same_bits(a, b) -> bool:
    """Bit for bit, NaN where the other has NaN (a NaN's payload is not data)."""
    nan = np.isnan(a)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def _parser():
    import lorenzcycletoolkit
    return lorenzcycletoolkit


def test_parser_accepts_series_and_series_paths_orders_the_parts(case):
    cli = _parser()
    p = case["parts"]
    args = cli.create_arg_parser().parse_args([p[2], "-r", "-f", "--series", p[1], p[2], p[0]])
    assert args.infile == p[2] and args.series == [p[1], p[2], p[0]]
    assert ds.series_paths(args, case["namelist"]) == p                    # by first time stamp; the repeated infile once
    link = str(case["root"] / "again.nc")
    os.symlink(p[1], link)
    args = cli.create_arg_parser().parse_args([p[0], "-r", "-f", "--series", link, p[2], p[1]])
    assert ds.series_paths(args, case["namelist"]) == [p[0], link, p[2]]   # duplicates by realpath: the first naming stays
    # without the option nothing is opened and the logged Namespace is what it was
    plain = cli.create_arg_parser().parse_args(["nowhere.nc", "-r", "-f"])
    assert not hasattr(plain, "series") and ds.series_paths(plain, "no/namelist") == ["nowhere.nc"]


def test_open_dataset_of_the_parts_equals_the_merged_file(case):
    p = case["parts"]
    got = ds.open_dataset([p[1], p[2], p[0]], case["df"])
    ref = ds.open_dataset(case["merged"], case["df"])
    assert np.array_equal(got.time, ref.time) and got.time.dtype == ref.time.dtype
    for a, b in ((got.lat, ref.lat), (got.lon, ref.lon), (got.level, ref.level)):
        assert np.array_equal(a, b)
    assert sorted(got.variables) == sorted(ref.variables)
    for name in sc.NAMES:
        a, b = got.variables[name], ref.variables[name]
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
        assert same_bits(a, b) and same_bits(a, case["decoded"][name]), name
    assert np.isnan(got.variables["v"][2, 7]).all() and np.isnan(got.variables["v"][4, 3, 10, 20])       # the fill points of two parts


def test_prepare_data_of_a_series_equals_the_merged_run(case, tmp_path, monkeypatch):
    """The host preparation end to end (``prepare_data``: gather_on_host step by step with every step's own packing)."""
    os.makedirs(tmp_path / "inputs")
    (tmp_path / "inputs" / "namelist").write_text(sc.NAMELIST)
    (tmp_path / "inputs" / "box_limits").write_text("min_lon;-60\nmax_lon;20\nmin_lat;-45\nmax_lat;30\n")
    monkeypatch.chdir(tmp_path)
    cli = _parser()
    p = case["parts"]
    got = ds.prepare_data(cli.create_arg_parser().parse_args([p[0], "-r", "-f", "--series", p[2], p[1]]))
    ref = ds.prepare_data(cli.create_arg_parser().parse_args([case["merged"], "-r", "-f"]))
    assert np.array_equal(got.time, ref.time) and np.array_equal(got.lon, ref.lon) and np.array_equal(got.level, ref.level)
    for name in sc.NAMES:
        assert got.variables[name].dtype == np.float32 and same_bits(got.variables[name], ref.variables[name]), name


def test_open_raw_of_the_parts_is_one_variable_with_a_packing_table(case, tmp_path):
    p, packed = case["parts"], case["packed"]
    raw = ds.open_raw([p[2], p[0], p[1]], case["df"])
    try:
        assert raw.time.size == 7 and np.all(np.diff(raw.time) == np.timedelta64(6, "h"))
        where = [(0, 0), (0, 1), (0, 2), (1, 0), (2, 0), (2, 1), (2, 2)]
        for name in sc.NAMES:
            v = raw.variables[name]
            assert tuple(v.data.shape) == (7, 9, 49, 144) and v.data.dtype == np.dtype(">i2") and not v.uniform_packing
            for ft, (k, t) in enumerate(where):
                block = v.data[ft]
                assert block.flags["C_CONTIGUOUS"] and np.array_equal(np.asarray(block).astype(np.int16), packed[k][name][0][t]), (name, ft)
            table = v.packing_table(np.arange(7))
            assert table.dtype == np.float64 and table.shape == (7, 3)
            for ft, (k, _) in enumerate(where):
                a = packed[k][name][1]
                assert table[ft].tolist() == [a["scale_factor"], a["add_offset"], float(sc.FILL)], (name, ft)
                assert v.packing_at(ft) == (a["scale_factor"], a["add_offset"], float(sc.FILL))
            assert np.array_equal(v.packing_table([5, 3]), table[[5, 3]])
            for attr in ("scale_factor", "add_offset", "fill_value"):
                with pytest.raises(ValueError, match="packed with other constants"):
                    getattr(v, attr)
            assert not hasattr(v.data, "chunk_streams")              # classic parts: nothing to inflate
            assert ds.decode_dtypes(v.data.dtype, *v.packing_at(0))[1] == np.float32
        ncs = list(raw._nc.ncs)
    finally:
        raw.close()
    assert len(ncs) == 3 and all(nc.variables == {} for nc in ncs)                     # close() closed every part
    # parts that share one packing: the scalar attributes answer, and the table repeats them
    same, _ = sc.write_series(tmp_path / "same", same_packing=True)
    raw = ds.open_raw(same, case["df"])
    try:
        for name in sc.NAMES:
            v = raw.variables[name]
            assert v.uniform_packing and v.fill_value == float(sc.FILL)
            assert np.array_equal(v.packing_table([0, 3, 6]), np.array([[v.scale_factor, v.add_offset, v.fill_value]] * 3))
    finally:
        raw.close()


def test_series_data_offers_what_a_chunked_part_offers_but_never_the_device_inflate():
    """Parts that are lazily inflated NetCDF-4 variables (stood in for here: ``read_step``, ``chunk_streams``, ``_filters``): the series
    reads only the wanted levels of the part that holds the step, says that there is something to inflate, and answers ``None`` where the
    device inflate asks for one file's chunk streams."""
    class Lazy:
        dtype, _filters = np.dtype("<i2"), [(1, (4,))]

        def __init__(self, a):
            self.a, self.shape = a, a.shape

        def __getitem__(self, t):
            return self.a[t]

        def read_step(self, t, levels):
            return self.a[t][levels] + 0

        def chunk_streams(self):
            return {"chunk": (1, 1, 2, 2)}

    a = np.arange(5 * 3 * 2 * 2, dtype="<i2").reshape(5, 3, 2, 2)
    lazy = ds._SeriesData([Lazy(a[:2]), a[2:3], Lazy(a[3:])], [0, 2, 3, 5])
    assert lazy.shape == (5, 3, 2, 2) and len(lazy) == 5 and [lazy.locate(t) for t in range(5)] == [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1)]
    for t in range(5):
        assert np.array_equal(lazy[t], a[t]) and np.array_equal(lazy.read_step(t, [2, 0]), a[t][[2, 0]])
    assert lazy.chunk_streams() is None and lazy._filters == [(1, (4,))]
    plain = ds._SeriesData([a[:2], a[2:]], [0, 2, 5])
    assert not hasattr(plain, "chunk_streams") and getattr(plain, "_filters", None) is None
    for bad in (-1, 5):
        with pytest.raises(IndexError):
            lazy[bad]
    with pytest.raises(TypeError):
        lazy[0:2]


def _rewrite(src, dst, change):
    """A copy of a classic file with ``change(name, variable values, attributes) -> (values, attributes) or None (drop)`` applied."""
    from scipy.io import netcdf_file
    a, b = netcdf_file(src, mmap=False), netcdf_file(dst, "w", version=2)
    for n, s in a.dimensions.items():
        b.createDimension(n, s)
    for name, v in a.variables.items():
        out = change(name, v.data.copy(), dict(v._attributes))
        if out is None:
            continue
        data, attrs = out
        w = b.createVariable(name, data.dtype.newbyteorder("="), v.dimensions)
        w[:] = data
        for k, x in attrs.items():
            setattr(w, k, x)
    a.close()
    b.close()
    return dst


def test_parts_that_do_not_continue_one_series_are_refused(case, tmp_path):
    p, df = case["parts"], case["df"]
    keep = lambda name, data, attrs: (data, attrs)

    def refused(change, match, others=(0,)):
        bad = _rewrite(p[1], str(tmp_path / "bad.nc"), change)
        for opener in (ds.open_raw, ds.open_dataset):
            with pytest.raises(ValueError, match=match) as e:
                opener([p[n] for n in others] + [bad], df)
            assert str(e.value).startswith("--series:") and bad in str(e.value) and p[others[-1]] in str(e.value), str(e.value)

    refused(lambda n, d, a: (d + np.float32(0.25), a) if n == "latitude" else keep(n, d, a), "differ in the latitude coordinate")
    refused(lambda n, d, a: None if n == "w" else keep(n, d, a), r"differ in their variables: .*Omega Velocity -> w")
    refused(lambda n, d, a: (d.astype(np.int32), a) if n == "u" else keep(n, d, a), "differ in the stored dtype of u")
    refused(lambda n, d, a: (d, {k: x for k, x in a.items() if k != "add_offset"}) if n == "z" else keep(n, d, a),
            "whether z has add_offset: present in the first, absent in the second")
    # time: part two starts at 2020-01-01 18:00; moved back by 6 h it repeats the first part's last stamp, by 9 h it lies inside it
    refused(lambda n, d, a: (d - 6, a) if n == "time" else keep(n, d, a), "both hold the time stamp 2020-01-01 12:00:00")
    refused(lambda n, d, a: (d - 9, a) if n == "time" else keep(n, d, a), r"overlap in time: .* begins at 2020-01-01 09:00:00, not after 2020-01-01 12:00:00")
    # uneven spacing across a seam is allowed: the d/dt coefficients take the real time axis
    late = _rewrite(p[2], str(tmp_path / "late.nc"), lambda n, d, a: (d + 1, a) if n == "time" else keep(n, d, a))
    raw = ds.open_raw([p[0], p[1], late], df)
    assert raw.time[4] - raw.time[3] == np.timedelta64(7, "h")
    raw.close()


def test_series_with_cdsapi_or_the_device_inflate_is_refused_in_words(case):
    cli = _parser()
    p = case["parts"]
    with pytest.raises(SystemExit, match="--cdsapi downloads one"):
        cli.main([p[0], "-r", "-f", "--cdsapi", "--series", p[1]])
    with pytest.raises(SystemExit, match="--inflate device is not supported with --series"):
        cli.main([p[0], "-r", "-f", "--ingest", "device", "--inflate", "device", "--series", p[1]])


def test_prefers_device_ingest_sums_the_parts_and_never_raises(case, monkeypatch, tmp_path):
    from lorenzcycletoolkit_amd import ingest
    cli = _parser()
    p = case["parts"]
    args = cli.create_arg_parser().parse_args([p[0], "-r", "-f", "--series", p[1], p[2]])
    assert ingest.prefers_device_ingest(args, case["namelist"]) is False          # 2.3 MB of parts: the host prepares them
    total = sum(os.path.getsize(x) for x in p)
    monkeypatch.setattr(ingest, "AUTO_DEVICE_BYTES", total)                       # no single part reaches it, together they do
    assert max(os.path.getsize(x) for x in p) < total
    verdict, raw = ingest.prefers_device_ingest(args, case["namelist"], keep_open=True)
    assert verdict is True and raw.time.size == 7
    raw.close()
    args.series = [p[1], str(tmp_path / "missing.nc")]
    assert ingest.prefers_device_ingest(args, case["namelist"]) is False


def test_lec_ingest_series_is_exported_and_checks_its_table_before_any_launch():
    hdr = open(os.path.join(ROOT, "include", "lec_hip.h")).read()
    assert re.search(r"^int lec_ingest_series\(const lec_ingest_args\* args, const double\* pack_d, int32_t pack_len\);", hdr, flags=re.M)
    assert "lec_ingest_series" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.lec_version() == 11 == _lib.LEC_ABI_VERSION
    g = _lib.IngestArgs()
    for f in ("src_d", "out_d", "kmap_d", "jmap_d", "imap_d"):
        setattr(g, f, 4096)
    g.src_dtype, g.out_dtype, g.decode_dtype = _lib.LEC_I16, _lib.LEC_F32, _lib.LEC_F32
    g.nt, g.nl_in, g.nl = 3, 1, 1
    g.ny_in = g.nx_in = 8
    g.ny = g.nx = 4
    table = ctypes.c_void_p(8192)
    assert lib.lec_ingest_series(None, table, 3) == 1 and b"null args" in lib.lec_last_error()
    assert lib.lec_ingest_series(ctypes.byref(g), None, 3) == 1 and b"null pack_d" in lib.lec_last_error()
    for n in (2, 4, 0):
        assert lib.lec_ingest_series(ctypes.byref(g), table, n) == 1 and b"pack_len must be" in lib.lec_last_error()
    g.step_d, g.nt_src, g.jmap_len, g.imap_len = 4096, 5, 6, 6                   # a step table: the table has a row per SOURCE step
    for n in (3, 4, 6):
        assert lib.lec_ingest_series(ctypes.byref(g), table, n) == 1 and b"pack_len must be nt_src" in lib.lec_last_error()
    # ... and what lec_ingest refuses is refused here too, first
    g.nt_src = 0
    assert lib.lec_ingest_series(ctypes.byref(g), table, 0) == 1 and b"nt_src >= 1" in lib.lec_last_error()


def test_deflated_netcdf4_parts_are_inflated_by_the_reader(tmp_path):
    """Two shuffled + deflated NetCDF-4 parts (the fixture and a copy that continues it 30 h later and packs T with another
    scale_factor): the whole-file decode and the step-by-step gather give each part's values with that part's constants."""
    src = os.path.join(ROOT, "tests", "golden", "hdf5", "packed_chunked_tracked.nc")
    later = sc.later_copy_of_hdf5(src, tmp_path / "parts" / "later.nc", 30, rescale_t=1.5)
    (tmp_path / "namelist").write_text(sc.NAMELIST)
    df = ds.read_namelist(str(tmp_path / "namelist"))
    one, single = ds.open_dataset(src, df), ds.open_raw(src, df)
    want = {}
    for name, v in single.variables.items():
        a = one.variables[name]
        b = a
        if name == "t":
            stored = np.stack([np.asarray(v.data[t]) for t in range(5)])
            b = ds.decode_values(stored.astype(stored.dtype.newbyteorder("=")), v.scale_factor * 1.5, v.add_offset, v.fill_value)
            assert not np.array_equal(a, b, equal_nan=True)
        want[name] = np.concatenate([a, b])
    single.close()
    got = ds.open_dataset([later, src], df)
    assert got.time.size == 10 and got.time[5] - got.time[4] == np.timedelta64(6, "h")
    raw = ds.open_raw([later, src], df)
    try:
        nt, nl, ny, nx = raw.variables["t"].data.shape
        plan = ds.IngestPlan(np.arange(nt), np.arange(nl, dtype=np.int32), np.arange(ny, dtype=np.int32), np.arange(nx, dtype=np.int32),
                             raw.lat, raw.lon, raw.level, raw.time)
        for name, v in raw.variables.items():
            assert v.uniform_packing == (name != "t") and v.data.chunk_streams() is None and v.data._filters
            assert same_bits(got.variables[name], want[name]), name
            assert same_bits(ds.gather_on_host(v, plan), want[name]), name
            assert same_bits(ds.gather_on_host(v, plan, (4, 7)), want[name][4:7]), name
    finally:
        raw.close()
