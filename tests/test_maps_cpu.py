"""Longitude-resolved maps without a GPU: the definition (the restatement of tests/maps_restatement.py closes on the sections'
restatement and on the oracle's scalars), the additive C call ``lec_maps`` (export, header, ABI 11, struct layout, every refusal on the
scalars before any HIP call), the engine's and the command line's refusals around maps and the writer's files on a hand-made result.

Bar of the definition: 1e-13 of each term's scale, the bar of tests/test_sections_cpu.py -- ``zonal_average`` is linear in its argument,
so the two sides differ by the order of a handful of fp64 sums (measured: the maps against the sections at most 3.9e-16, the Hovmoeller against the
scalars at most 9.8e-15; each case prints its figure)."""
import ctypes
import os
import types

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib
from oracle import lec_oracle as o
from tests import maps_restatement as mr
from tests import ring_restatement as rr
from tests import sections_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEC_IDX = [sr.TERMS.index(k) for k in mr.TERMS]


# -- the definition -----------------------------------------------------------------------------------------------------------------
def _box(kind, ny):
    dom = rr.ring_domain(3, 5, ny, 16, seed=ny)
    return rr.ring_box(dom, -60.0, 60.0) if kind == "ring" else o.make_box(dom, -100.0, 100.0, -60.0, 60.0)


@pytest.mark.parametrize("ny", [5, 65])
@pytest.mark.parametrize("kind", ["ring", "open"])
def test_restatement_closes_on_the_sections_and_the_oracle(kind, ny):
    b = _box(kind, ny)
    ring = kind == "ring"
    Y = mr.maps(b, ring)
    nxb = b.rlons.size - (1 if ring else 0)
    assert Y.shape == (3, 6, 5, b.rlats.size, nxb)
    X = sr.sections(b)[:, SEC_IDX]
    scale = np.abs(X).max(axis=(0, 2, 3), keepdims=True)
    err = (np.abs(mr.zonal_average(Y, b, ring) - X) / scale).max()
    print(f"{kind} {ny} rows: zonal average of the maps against the sections: {err:.3e}")
    assert err <= 1e-13
    # the columns close on the sections' columns, the Hovmoeller on the oracle's scalars
    C = mr.columns(Y, b.level)
    Cs = sr.columns(sr.sections(b), b.level)[:, SEC_IDX]
    assert (np.abs(mr.zonal_average(C, b, ring) - Cs) / np.abs(Cs).max(axis=(0, 2), keepdims=True)).max() <= 1e-13
    H = mr.hovmoller(C, sr.area_weights(b))
    scalars, _ = o.all_terms(b)
    for i, term in enumerate(mr.TERMS):
        sc = np.asarray(scalars[term], dtype=np.float64)
        e = np.abs(mr.zonal_average(H[:, i], b, ring) - sc).max() / np.abs(sc).max()
        print(f"{kind} {ny} rows {term}: zonal average of the Hovmoeller against the scalar: {e:.3e}")
        assert e <= 1e-13, term
    M = mr.time_mean(C)
    assert M.shape == (6, b.rlats.size, nxb) and np.allclose(M, C.mean(axis=0), rtol=1e-13, atol=0)


def test_column_nan_rule_per_point():
    p = np.array([100.0, 200.0, 400.0, 700.0, 1000.0])
    y = np.array([1.0, 2.0, 4.0, 7.0, 10.0])
    Y = np.broadcast_to(y[None, None, :, None, None], (1, 6, 5, 2, 4)).copy()
    Y[0, :, 2, 0, 1] = np.nan                  # an interior gap at one point: bridged (y is linear in p: nothing changes)
    Y[0, :, 0, 1, 2] = np.nan                  # a NaN top level at another: left out
    Y[0, :, :, 1, 3] = np.nan                  # no finite level at a third: NaN
    Y[0, :, :, 0, 3] = np.nan; Y[0, :, 3, 0, 3] = 2.0      # one finite level: an empty integral, 0
    C = mr.columns(Y, p)
    assert C.shape == (1, 6, 2, 4)
    for f, term in enumerate(mr.TERMS):
        s = sr.COLUMN_SCALE.get(term, 1.0)
        whole = o.trapz(y, p, axis=0) * s
        assert C[0, f, 0, 0] == pytest.approx(whole, rel=1e-15) and C[0, f, 0, 1] == pytest.approx(whole, rel=1e-15)
        assert C[0, f, 1, 2] == pytest.approx(o.trapz(y[1:], p[1:], axis=0) * s, rel=1e-15)
        assert np.isnan(C[0, f, 1, 3]) and C[0, f, 0, 3] == 0.0
    assert np.isnan(C).sum() == 6
    # the time mean is NaN where any step is; the Hovmoeller where any row is
    M = mr.time_mean(np.concatenate([C, np.ones_like(C)]))
    assert np.array_equal(np.isnan(M), np.isnan(C[0]))
    H = mr.hovmoller(C, np.array([0.25, 0.75]))
    assert np.array_equal(np.isnan(H[0]), np.isnan(C[0]).any(axis=1))


# -- the C call ---------------------------------------------------------------------------------------------------------------------
def test_maps_call_is_additive():
    lib = _lib.load()
    before = ["lec_version", "lec_last_error", "lec_max_row", "lec_rowstats", "lec_reduce", "lec_dropmask", "lec_ingest", "lec_track_diag",
              "lec_check_boxes", "lec_check_maps", "lec_host_register", "lec_host_unregister", "lec_copy_rows_async", "lec_inflate",
              "lec_inflate_status_text", "lec_chunk_scatter", "lec_format_csv_rows", "lec_dtdt", "lec_rowstats_steps", "lec_follow",
              "lec_follow_seeds", "lec_follow_many", "lec_follow_seeds_series", "lec_follow_spans", "lec_follow_spans_chunk",
              "lec_follow_seeds_series_ring", "lec_follow_spans_chunk_ring", "lec_rowstats_ring", "lec_ingest_series", "lec_rowspec_ring",
              "lec_rowspec_q_ring", "lec_level_spec_ring", "lec_rowspec_nl_ring", "lec_rowspec_b_ring", "lec_level_spec_b_ring",
              "lec_sections"]
    assert _lib.EXPORTS == before + ["lec_maps"]
    for name in _lib.EXPORTS:
        assert getattr(lib, name) is not None, name
    hdr = open(os.path.join(ROOT, "include", "lec_hip.h")).read()
    assert "int lec_maps(const lec_maps_args* args);" in hdr
    assert "#define LEC_NMAP 6" in hdr and "#define LEC_MAPS_NCOEF 16" in hdr
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11 and "#define LEC_ABI_VERSION 11" in hdr
    assert _lib.LEC_NMAP == 6 and _lib.LEC_MAPS_NCOEF == 16
    from lorenzcycletoolkit_amd.constants import MAP_TERMS
    assert MAP_TERMS == ["Ae", "Ke", "Ca", "Ce", "Ck", "Ge"] == mr.TERMS
    A = _lib.MapsArgs
    assert ctypes.sizeof(A) == 4 * 8 + 13 * 4 + 4 + 7 * 8 + 8 + 5 * 8 == 192
    offs = {n: getattr(A, n).offset for n, _ in A._fields_}
    assert [offs[n] for n in ("tair_d", "u_d", "v_d", "omega_d")] == [0, 8, 16, 24]
    assert [offs[n] for n in ("dtype", "nt", "nl", "ny", "nx", "t_begin", "t_count", "iw", "ie", "js", "jn", "ring", "reserved0")] \
        == list(range(32, 84, 4))
    assert [offs[n] for n in ("rows_d", "levraw_d", "lattab2_d", "levtab2_d", "lattab_d", "levtab_d", "tcoef_d", "inv_hdeg")] \
        == list(range(88, 152, 8))
    assert [offs[n] for n in ("coef_d", "col_d", "mapsum_d", "hov_d", "stream")] == list(range(152, 192, 8))
    # the existing structs are what they were
    assert ctypes.sizeof(_lib.SectionsArgs) == 128 and ctypes.sizeof(_lib.RowspecQArgs) == 4 * 8 + 10 * 4 + 4 * 8 + 8 + 2 * 8
    assert ctypes.sizeof(_lib.ReduceArgs) == 8 + 4 * 4 + 4 * 8 + 8 + 2 * 4 + 8 + 6 * 8 + 2 * 8


POINTERS = ["tair_d", "u_d", "v_d", "omega_d", "rows_d", "levraw_d", "lattab2_d", "levtab2_d", "lattab_d", "levtab_d", "tcoef_d",
            "coef_d", "col_d", "mapsum_d", "hov_d"]


def _valid_args():
    """Scalars of a valid call over fake (never dereferenced) pointers: every refusal is made on the scalars, before any HIP call."""
    a = _lib.MapsArgs()
    for n in POINTERS:
        setattr(a, n, 0x10000)
    a.dtype, a.nt, a.nl, a.ny, a.nx = _lib.LEC_F64, 5, 4, 9, 16
    a.t_begin, a.t_count, a.iw, a.ie, a.js, a.jn, a.ring = 1, 3, 2, 13, 1, 7, 0
    a.inv_hdeg = 1.0
    return a


def _set(**kw):
    return lambda a: [setattr(a, k, v) for k, v in kw.items()]


@pytest.mark.parametrize("field, change", [(n, _set(**{n: None})) for n in POINTERS] + [
    ("dtype", _set(dtype=_lib.LEC_I16)), ("ring", _set(ring=2)), ("ring", _set(ring=1)),     # a ring of part of the circle
    ("reserved0", _set(reserved0=1)), ("nt", _set(nt=1, t_begin=0, t_count=1)), ("nl", _set(nl=1)), ("ny", _set(ny=1)),
    ("nx", _set(nx=2)), ("t_begin", _set(t_begin=-1)), ("t_begin", _set(t_begin=5)), ("t_count", _set(t_count=0)),
    ("t_count", _set(t_count=5)), ("iw", _set(iw=-1)), ("iw", _set(iw=16)), ("ie", _set(ie=16)), ("ie", _set(ie=1)),
    ("ie", _set(ie=3)),                                                                       # two columns
    ("js", _set(js=-1)), ("js", _set(js=9)), ("jn", _set(jn=1)), ("jn", _set(jn=9)),
    ("rows_d", _set(rows_d=0x10008)), ("lattab2_d", _set(lattab2_d=0x10008)), ("coef_d", _set(coef_d=0x10008)),
    ("levraw_d", _set(levraw_d=0x10004)), ("levtab2_d", _set(levtab2_d=0x10004)), ("lattab_d", _set(lattab_d=0x10004)),
    ("levtab_d", _set(levtab_d=0x10004)), ("tcoef_d", _set(tcoef_d=0x10004)), ("col_d", _set(col_d=0x10004)),
    ("hov_d", _set(hov_d=0x10004)), ("mapsum_d", _set(mapsum_d=0x10004)), ("tair_d", _set(tair_d=0x10004)),
    ("omega_d", _set(omega_d=0x10002, dtype=_lib.LEC_F32)),
])
def test_c_call_refusals_name_the_field(field, change):
    lib = _lib.load()
    a = _valid_args()
    change(a)
    assert lib.lec_maps(ctypes.byref(a)) == 1          # LEC_ERR_ARG
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_maps") and field.encode() in msg, msg


@pytest.mark.parametrize("field, change", [
    ("nl", _set(nl=161)),                                                                  # LEC_MAX_LEVELS = 160
    ("t_count", _set(nt=1 << 20, nl=64, t_count=1 << 20, t_begin=0)),                      # 2^26 workgroups of the factors kernel
    ("rows", _set(nt=1 << 24, nl=2, t_count=1 << 24, t_begin=0, jn=4, js=1)),                # 2^26 workgroups of the column kernel
    ("columns", _set(ny=1 << 15, js=0, jn=(1 << 15) - 1, nx=1 << 15, iw=0, ie=(1 << 15) - 1)),      # 6 x 2^30 threads of the time sums
])
def test_c_call_beyond_the_limits(field, change):
    lib = _lib.load()
    a = _valid_args()
    change(a)
    assert lib.lec_maps(ctypes.byref(a)) == 2          # LEC_ERR_UNSUPPORTED
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_maps") and field.encode() in msg, msg


def test_c_call_null_args():
    lib = _lib.load()
    assert lib.lec_maps(None) == 1
    assert lib.lec_last_error().startswith(b"lec_maps") and b"null args" in lib.lec_last_error()


# -- the engine ---------------------------------------------------------------------------------------------------------------------
def test_engine_refusals_in_words():
    from lorenzcycletoolkit_amd.engine import LECEngine
    with pytest.raises(ValueError, match="ONE fixed box"):
        LECEngine._check_maps([(0, 3, 0, 3)] * 2, None)
    with pytest.raises(ValueError, match="ONE fixed box"):
        LECEngine._check_maps([(0, 3, 0, 3)], True)
    for kw in (dict(steps=object()), dict(tm=object()), dict(tp=object())):
        with pytest.raises(ValueError, match="ONE fixed box"):
            LECEngine._check_maps([(0, 3, 0, 3)], False, **kw)
    LECEngine._check_maps([(0, 3, 0, 3)], False)
    assert LECEngine.MAP_CHUNK_BYTES == 256 << 20
    # compute refuses before it touches the engine's tables, the library or a device: an engine that was never initialised will do
    import torch
    eng = object.__new__(LECEngine)
    t = torch.zeros((3, 2, 4, 4), dtype=torch.float64)
    box = [(0, 3, 0, 3)]
    for kw, words in [(dict(maps=True, out=torch.empty((3, 58), dtype=torch.float64)), "one process on one GPU"),
                      (dict(maps=True, merge_dropmask=lambda m: None), "one process on one GPU"),
                      (dict(maps=True, dTdt=t), "dTdt cube is not supported"),
                      (dict(maps=True, with_q=False), "maps need with_q"),
                      (dict(maps=True, per_step_boxes=True), "ONE fixed box"),
                      (dict(maps=True, steps=torch.zeros((3, 3), dtype=torch.int32)), "ONE fixed box"),
                      (dict(maps=True, tm=t, tp=t), "ONE fixed box"),
                      (dict(map_steps=True), "part of maps=True")]:
        with pytest.raises(ValueError, match=words):
            eng.compute(t, t, t, t, None, box, time_s=np.arange(3.0), **kw)
    with pytest.raises(ValueError, match="ONE fixed box"):
        eng.compute(t, t, t, t, None, box * 3, time_s=np.arange(3.0), maps=True)


# -- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags, text", [
    (["-t", "--maps"], "--maps goes with -f/--fixed"),
    (["-c", "--maps"], "--maps goes with -f/--fixed"),
    (["-f", "--maps", "--gpus", "2"], "--maps runs on one GPU"),
    (["-f", "--periodic", "--maps", "--gpus", "4"], "--maps runs on one GPU"),
    (["-f", "--maps", "--ingest", "device"], "--maps prepares the data on the host: --ingest device / --device-ingest is not supported"),
    (["-f", "--maps", "--device-ingest"], "--maps prepares the data on the host: --ingest device / --device-ingest is not supported"),
    (["-f", "--periodic", "--maps", "--wavenumbers", "4", "--wavenumbers-chunk", "2"], "--maps prepares the data on the host: --wavenumbers-chunk"),
])
def test_cli_refusals(tmp_path, monkeypatch, flags, text):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", *flags])
    assert text in str(e.value)
    assert not os.path.exists(tmp_path / "LEC_Results")          # refused before anything was created


def test_cli_help_names_the_flag(capsys):
    import lorenzcycletoolkit
    with pytest.raises(SystemExit):
        lorenzcycletoolkit.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--maps" in text and "results_maps/" in text and "<term>_lat_lon.csv" in text and "<term>_lon.csv" in text
    assert "--maps" in lorenzcycletoolkit.__doc__ and "--maps" in open(os.path.join(ROOT, "README.md")).read()


# -- the writer ---------------------------------------------------------------------------------------------------------------------
def test_writer_headers_and_labels(tmp_path):
    import pandas as pd
    from lorenzcycletoolkit_amd import frameworks as fw
    from lorenzcycletoolkit_amd.constants import MAP_TERMS
    nt, ny, nx = 3, 4, 5
    rng = np.random.default_rng(0)
    time = pd.date_range("2020-01-01", periods=nt, freq="6h")
    box = types.SimpleNamespace(
        map_mean=rng.standard_normal((6, ny, nx)), map_lon=rng.standard_normal((nt, 6, nx)),
        map_latitudes=np.array([-45.0, -15.0, 15.0, 45.0]), map_longitudes=np.array([-10.0, -7.5, -5.0, -2.5, 0.0]),
        time=time.values, row_labels=lambda method: fw.time_labels(time.values, method))
    box.map_mean[1, 2, 3] = np.nan
    out = tmp_path / "results_maps"
    fw.write_map_csvs(box, str(out), "time", "lat")
    assert sorted(os.listdir(out)) == sorted([f"{t}_lat_lon.csv" for t in MAP_TERMS] + [f"{t}_lon.csv" for t in MAP_TERMS])
    m = pd.read_csv(out / "Ke_lat_lon.csv", index_col=0, float_precision="round_trip")
    assert m.index.name == "lat" and list(m.index) == [-45.0, -15.0, 15.0, 45.0]
    assert [float(c) for c in m.columns] == [-10.0, -7.5, -5.0, -2.5, 0.0]
    assert np.array_equal(m.values, box.map_mean[1], equal_nan=True)            # repr(float): the values round-trip
    lines = open(out / "Ke_lat_lon.csv").read().splitlines()
    assert lines[0] == "lat,-10.0,-7.5,-5.0,-2.5,0.0" and lines[1].startswith("-45.0,") and lines[3].split(",")[4] == ""
    h = pd.read_csv(out / "Ck_lon.csv", index_col=0, float_precision="round_trip")
    assert h.index.name == "time" and list(h.index) == ["2020-01-01 00:00:00", "2020-01-01 06:00:00", "2020-01-01 12:00:00"]
    assert [float(c) for c in h.columns] == [-10.0, -7.5, -5.0, -2.5, 0.0]
    assert np.array_equal(h.values, box.map_lon[:, MAP_TERMS.index("Ck")])
