"""System-relative composites without a GPU: the definition (the restatement of tests/composite_restatement.py closes on the oracle's
moving-framework scalars), the additive C call ``lec_composite`` (export, extension header, ABI 11, struct layout, every refusal on the
scalars and on the host copy of the boxes before any HIP call), the engine's and the command line's refusals around composites and the
writer's files on a hand-made result.

Bar of the definition: 1e-13 of each term's scale, the bar of tests/test_maps_cpu.py -- ``zonal_average`` is linear in its argument, so
the two sides differ by the order of a handful of fp64 sums (measured: at most 3.5e-16; each case prints its figure)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib
from oracle import lec_oracle as o
from tests import composite_restatement as cr
from tests.helpers import synthetic_domain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the definition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nyb, nxb", [(5, 5), (7, 65)])
def test_restatement_closes_on_the_moving_oracle(nyb, nxb):
    nt, nl = 4, 5
    dom = synthetic_domain(nt, nl, nyb + 4, nxb + 6, seed=nyb + nxb)
    boxes = [(0, nxb - 1, 0, nyb - 1), (6, nxb + 5, 4, nyb + 3), (2, nxb + 1, 1, nyb), (3, nxb + 2, 3, nyb + 2)]
    C, H, M = cr.composites(dom, boxes)
    assert C.shape == (nt, 6, nyb, nxb) and H.shape == (nt, 6, nxb) and M.shape == (6, nyb, nxb) and np.isfinite(C).all()
    scalars, _ = o.lec_moving(dom, [cr.limits(dom, b) for b in boxes], residuals=False)
    za = cr.box_zonal_average(H, cr.step_boxes(dom, boxes))
    for i, term in enumerate(cr.TERMS):
        sc = np.asarray(scalars[term], dtype=np.float64)
        e = np.abs(za[:, i] - sc).max() / np.abs(sc).max()
        print(f"{nyb} x {nxb} {term}: the box's zonal average of the Hovmoeller against lec_moving's scalar: {e:.3e}")
        assert e <= 1e-13, term
    assert np.allclose(M, C.mean(axis=0), rtol=1e-13, atol=0)


# -- the C call ---------------------------------------------------------------------------------------------------------------------
def test_composite_call_is_an_extension():
    lib = _lib.load()
    assert _lib.EXT_EXPORTS == ["lec_composite"] and "lec_composite" not in _lib.EXPORTS
    assert lib.lec_composite is not None
    ext = open(os.path.join(ROOT, "include", "lec_hip_ext.h")).read()
    hdr = open(os.path.join(ROOT, "include", "lec_hip.h")).read()
    assert "int lec_composite(const lec_composite_args* args);" in ext and '#include "lec_hip.h"' in ext
    assert "lec_composite" not in hdr
    assert set(re.findall(r"^int (lec_\w+)\(", ext, flags=re.M)) == set(_lib.EXT_EXPORTS)
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11 and "#define LEC_ABI_VERSION 11" in hdr
    mk = open(os.path.join(ROOT, "lorenzcycletoolkit_amd", "csrc", "Makefile")).read()
    assert "lec_composite.hip" in mk and "lec_hip_ext.h" in mk and "lec_mapcol.h" in mk
    A = _lib.CompositeArgs
    assert ctypes.sizeof(A) == 7 * 8 + 10 * 4 + 15 * 8 == 216
    offs = {n: getattr(A, n).offset for n, _ in A._fields_}
    assert [offs[n] for n in ("tair_d", "u_d", "v_d", "omega_d", "dTdt_d", "tm_d", "tp_d")] == list(range(0, 56, 8))
    assert [offs[n] for n in ("dtype", "nt", "nl", "ny", "nx", "t_begin", "t_count", "nyb", "nxb", "reserved0")] == list(range(56, 96, 4))
    assert [offs[n] for n in ("box_h", "box_d", "boxtab_d", "lattab_d", "lattab2_d", "rows_d", "levraw_d", "levtab_d", "levtab2_d", "tcoef_d",
                              "coef_d", "col_d", "mapsum_d", "hov_d", "stream")] == list(range(96, 216, 8))
    assert ctypes.sizeof(_lib.MapsArgs) == 192            # the existing struct is what it was


def test_source_digest_covers_the_extension_header(tmp_path, monkeypatch):
    import inspect
    assert "lec_hip_ext.h" in inspect.getsource(_lib.source_digest)


POINTERS = ["tair_d", "u_d", "v_d", "omega_d", "box_d", "boxtab_d", "lattab_d", "lattab2_d", "rows_d", "levraw_d", "levtab_d",
            "levtab2_d", "coef_d", "col_d", "mapsum_d", "hov_d"]
T_COUNT, NYB, NXB = 3, 4, 7


def _valid_args(boxes=None):
    """Scalars of a valid call over fake (never dereferenced) device pointers and a real host copy of the boxes: every refusal is made on
    the scalars and on that copy, before any HIP call.  Returns (args, the host array, which must outlive the call)."""
    a = _lib.CompositeArgs()
    for n in POINTERS + ["dTdt_d", "tcoef_d"]:
        setattr(a, n, 0x10000)
    host = np.ascontiguousarray(boxes if boxes is not None else [(2, 8, 1, 4), (0, 6, 0, 3), (9, 15, 5, 8)], dtype=np.int32)
    a.box_h = host.ctypes.data
    a.dtype, a.nt, a.nl, a.ny, a.nx = _lib.LEC_F64, 5, 4, 9, 16
    a.t_begin, a.t_count, a.nyb, a.nxb = 1, T_COUNT, NYB, NXB
    return a, host


def _set(**kw):
    return lambda a: [setattr(a, k, v) for k, v in kw.items()]


@pytest.mark.parametrize("field, change", [(n, _set(**{n: None})) for n in POINTERS + ["box_h"]] + [
    ("dtype", _set(dtype=_lib.LEC_I16)), ("reserved0", _set(reserved0=1)),
    ("tp_d", _set(dTdt_d=None, tm_d=0x10000)),                              # tm_d without tp_d
    ("tm_d", _set(dTdt_d=None, tp_d=0x10000)),                              # ... and the reverse
    ("dTdt_d", _set(tm_d=0x10000, tp_d=0x10000)),                           # two sources of dT/dt
    ("tcoef_d", _set(dTdt_d=None, tcoef_d=None)),                           # no source of dT/dt
    ("tcoef_d", _set(dTdt_d=None, tm_d=0x10000, tp_d=0x10000, tcoef_d=None)),
    ("nt", _set(nt=0)), ("nt", _set(dTdt_d=None, nt=1, t_begin=0, t_count=1)),      # the cube's own neighbours need two steps
    ("nl", _set(nl=1)), ("nyb", _set(nyb=1)), ("nxb", _set(nxb=2)), ("ny", _set(ny=3)), ("nx", _set(nx=6)),
    ("t_begin", _set(t_begin=-1)), ("t_begin", _set(t_begin=5)), ("t_count", _set(t_count=0)), ("t_count", _set(t_count=5)),
    ("rows_d", _set(rows_d=0x10008)), ("lattab2_d", _set(lattab2_d=0x10008)), ("coef_d", _set(coef_d=0x10008)),
    ("box_d", _set(box_d=0x10002)),
    ("levraw_d", _set(levraw_d=0x10004)), ("levtab2_d", _set(levtab2_d=0x10004)), ("lattab_d", _set(lattab_d=0x10004)),
    ("levtab_d", _set(levtab_d=0x10004)), ("tcoef_d", _set(tcoef_d=0x10004)), ("boxtab_d", _set(boxtab_d=0x10004)),
    ("dTdt_d", _set(dTdt_d=0x10004)), ("col_d", _set(col_d=0x10004)), ("hov_d", _set(hov_d=0x10004)), ("mapsum_d", _set(mapsum_d=0x10004)),
    ("tair_d", _set(tair_d=0x10004)), ("omega_d", _set(omega_d=0x10002, dtype=_lib.LEC_F32)),
    ("tm_d", _set(dTdt_d=None, tm_d=0x10004, tp_d=0x10000)),
])
def test_c_call_refusals_name_the_field(field, change):
    lib = _lib.load()
    a, host = _valid_args()
    change(a)
    assert lib.lec_composite(ctypes.byref(a)) == 1          # LEC_ERR_ARG
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite") and field.encode() in msg, msg


@pytest.mark.parametrize("boxes, words", [
    ([(2, 8, 1, 4), (0, 7, 0, 3), (9, 15, 5, 8)], b"step 1 is 4 x 8 (rows x columns), the call's nyb x nxb is 4 x 7"),
    ([(2, 8, 1, 4), (0, 6, 0, 3), (9, 15, 4, 8)], b"step 2 is 5 x 7 (rows x columns), the call's nyb x nxb is 4 x 7"),
    ([(2, 8, 1, 4), (-1, 5, 0, 3), (9, 15, 5, 8)], b"step 1 {iw, ie, js, jn} = {-1, 5, 0, 3} lies outside the 9 x 16 cube"),
    ([(2, 8, 1, 4), (0, 6, 0, 3), (10, 16, 5, 8)], b"step 2 {iw, ie, js, jn} = {10, 16, 5, 8} lies outside"),
    ([(2, 8, 6, 9), (0, 6, 0, 3), (9, 15, 5, 8)], b"step 0 {iw, ie, js, jn} = {2, 8, 6, 9} lies outside"),
])
def test_c_call_checks_the_host_copy_of_the_boxes(boxes, words):
    lib = _lib.load()
    a, host = _valid_args(boxes)
    assert lib.lec_composite(ctypes.byref(a)) == 1
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite: box_h") and words in msg, msg


@pytest.mark.parametrize("field, change", [
    ("nl", _set(nl=161)),                                                                   # LEC_MAX_LEVELS = 160
])
def test_c_call_beyond_the_limits(field, change):
    lib = _lib.load()
    a, host = _valid_args()
    change(a)
    assert lib.lec_composite(ctypes.byref(a)) == 2          # LEC_ERR_UNSUPPORTED
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite") and field.encode() in msg, msg


def test_c_call_thread_count_limits():
    """lec_maps' limits, on a series long enough to reach them: the host copy of the boxes has one entry per step."""
    lib = _lib.load()
    n = 1 << 20
    host = np.ascontiguousarray(np.tile(np.array([(0, 6, 0, 3)], dtype=np.int32), (n, 1)))
    a, _ = _valid_args()
    a.box_h = host.ctypes.data
    a.nt, a.t_begin, a.t_count, a.nl = n, 0, n, 64                                          # 2^26 workgroups of the factors kernel
    assert lib.lec_composite(ctypes.byref(a)) == 2 and b"t_count * nl" in lib.lec_last_error()
    a.nl, a.ny, a.nyb = 4, 64, 64                                                           # 2^26 workgroups of the column kernel
    host[:, 3] = 63
    assert lib.lec_composite(ctypes.byref(a)) == 2 and b"t_count * rows" in lib.lec_last_error()


def test_c_call_null_args():
    lib = _lib.load()
    assert lib.lec_composite(None) == 1
    assert lib.lec_last_error().startswith(b"lec_composite") and b"null args" in lib.lec_last_error()


# -- the engine ---------------------------------------------------------------------------------------------------------------------
def test_engine_refusals_in_words():
    import torch
    from lorenzcycletoolkit_amd.engine import LECEngine
    boxes = [(0, 4, 0, 3), (1, 5, 2, 5), (2, 6, 1, 4)]
    assert LECEngine._check_composites(boxes, True) == (4, 5)
    assert LECEngine._check_composites(boxes, None) == (4, 5)
    with pytest.raises(ValueError, match="per_step_boxes=True"):
        LECEngine._check_composites(boxes, False)
    with pytest.raises(ValueError, match="per_step_boxes=True"):
        LECEngine._check_composites(boxes[:1], None)
    with pytest.raises(ValueError, match=r"step 2 has 4 x 6 points \(rows x columns\), that of step 0 has 4 x 5"):
        LECEngine._check_composites(boxes[:2] + [(2, 7, 1, 4)], True)
    with pytest.raises(ValueError, match="evenly spaced longitudes"):
        LECEngine._check_composites(boxes, True, None, False)
    with pytest.raises(ValueError, match="at least 3 box columns"):
        LECEngine._check_composites([(0, 1, 0, 3)] * 3, True)
    with pytest.raises(ValueError, match="step table"):
        LECEngine._check_composites(boxes, True, object())
    # compute refuses before it touches the engine's tables, the library or a device: an engine that was never initialised will do
    eng = object.__new__(LECEngine)
    t = torch.zeros((3, 2, 8, 8), dtype=torch.float64)
    for kw, words in [(dict(composites=True, per_step_boxes=True, out=torch.empty((3, 58), dtype=torch.float64)), "one process on one GPU"),
                      (dict(composites=True, per_step_boxes=True, merge_dropmask=lambda m: None), "one process on one GPU"),
                      (dict(composites=True, per_step_boxes=True, with_q=False), "composites need with_q"),
                      (dict(composites=True, per_step_boxes=False), "per_step_boxes=True"),
                      (dict(composites=True, steps=torch.zeros((3, 3), dtype=torch.int32)), "step table"),
                      (dict(composite_steps=True, per_step_boxes=True), "part of composites=True"),
                      (dict(maps=True, per_step_boxes=True), "ONE fixed box")]:
        with pytest.raises(ValueError, match=words):
            eng.compute(t, t, t, t, None, boxes, time_s=np.arange(3.0), **kw)


# -- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags, text", [
    (["-f", "--composites"], "--composites goes with -t / -c: ONE fixed box has --maps"),
    (["-t", "--trackfiles", "a", "b", "--composites"], "--composites follows ONE system: --trackfiles"),
    (["-c", "--choose-systems", "2", "--composites"], "--composites follows ONE system: -c --choose-systems / --choose-starts"),
    (["-t", "--composites", "--gpus", "2"], "--composites runs on one GPU"),
    (["-c", "--composites", "--gpus", "2"], "-c/--choose follows the system on one GPU"),       # (-c's own, earlier refusal)
    (["-t", "--composites", "--ingest", "device"], "--composites prepares the data on the host: --ingest device / --device-ingest is not supported"),
    (["-c", "--composites", "--device-ingest"], "--composites prepares the data on the host: --ingest device / --device-ingest is not supported"),
    (["-t", "--maps"], "--maps goes with -f/--fixed"),                     # as before, byte for byte
    (["-c", "--maps"], "--maps goes with -f/--fixed: a map lies on the points of ONE fixed box; the boxes of a -t / -c run move, "
                       "and their maps would be system-relative composites"),
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
    assert "--composites" in text and "results_composites/" in text and "<term>_dlat_dlon.csv" in text and "<term>_dlon.csv" in text
    assert "--composites" in lorenzcycletoolkit.__doc__ and "--composites" in open(os.path.join(ROOT, "README.md")).read()


def test_track_shapes_and_axes_are_checked_before_a_file_is_written():
    from lorenzcycletoolkit_amd import frameworks as fw
    lat, lon = np.linspace(-60.0, -10.0, 21), np.linspace(-80.0, -20.0, 25)
    same = [(0, 6, 0, 4), (3, 9, 2, 6)]
    assert fw.composites_check(lat, lon, same) == (5, 7)
    with pytest.raises(ValueError, match=r"--composites needs boxes of ONE shape: the box of step 1 has 5 x 8 points \(rows x columns\), "
                                         r"that of step 0 has 5 x 7"):
        fw.composites_check(lat, lon, [same[0], (3, 10, 2, 6)])
    with pytest.raises(ValueError, match="--composites needs evenly spaced longitudes"):
        fw.composites_check(lat, np.sort(lon + 0.3 * np.sin(np.arange(25.0))), same)
    with pytest.raises(ValueError, match="--composites needs evenly spaced latitudes"):
        fw.composites_check(np.sort(lat + 0.3 * np.sin(np.arange(21.0))), lon, same)
    with pytest.raises(ValueError, match="--composites needs boxes of at least 3 longitudes"):
        fw.composites_check(lat, lon, [(0, 1, 0, 4), (3, 4, 2, 6)])


# -- the writer ---------------------------------------------------------------------------------------------------------------------
def test_writer_headers_and_labels(tmp_path):
    import pandas as pd
    from lorenzcycletoolkit_amd import frameworks as fw
    from lorenzcycletoolkit_amd.constants import MAP_TERMS
    nt, ny, nx = 3, 4, 5
    rng = np.random.default_rng(0)
    time = pd.date_range("2020-01-01", periods=nt, freq="6h")
    box = types.SimpleNamespace(
        composite_mean=rng.standard_normal((6, ny, nx)), composite_lon=rng.standard_normal((nt, 6, nx)),
        composite_dlat=np.array([-3.75, -1.25, 1.25, 3.75]), composite_dlon=np.array([-5.0, -2.5, 0.0, 2.5, 5.0]),
        time=time.values, row_labels=lambda method: fw.time_labels(time.values, method))
    box.composite_mean[1, 2, 3] = np.nan
    out = tmp_path / "results_composites"
    fw.write_composite_csvs(box, str(out), "time")
    assert sorted(os.listdir(out)) == sorted([f"{t}_dlat_dlon.csv" for t in MAP_TERMS] + [f"{t}_dlon.csv" for t in MAP_TERMS])
    m = pd.read_csv(out / "Ke_dlat_dlon.csv", index_col=0, float_precision="round_trip")
    assert m.index.name == "dlat" and list(m.index) == [-3.75, -1.25, 1.25, 3.75]
    assert [float(c) for c in m.columns] == [-5.0, -2.5, 0.0, 2.5, 5.0]
    assert np.array_equal(m.values, box.composite_mean[1], equal_nan=True)            # repr(float): the values round-trip
    lines = open(out / "Ke_dlat_dlon.csv").read().splitlines()
    assert lines[0] == "dlat,-5.0,-2.5,0.0,2.5,5.0" and lines[1].startswith("-3.75,") and lines[3].split(",")[4] == ""
    h = pd.read_csv(out / "Ck_dlon.csv", index_col=0, float_precision="round_trip")
    assert h.index.name == "time" and list(h.index) == ["2020-01-01 00:00:00", "2020-01-01 06:00:00", "2020-01-01 12:00:00"]
    assert [float(c) for c in h.columns] == [-5.0, -2.5, 0.0, 2.5, 5.0]
    assert np.array_equal(h.values, box.composite_lon[:, MAP_TERMS.index("Ck")])


def test_offset_labels_are_taken_from_the_first_box():
    from lorenzcycletoolkit_amd import frameworks as fw
    lat, lon = np.arange(-60.0, -9.0, 2.5), np.arange(-80.0, -19.0, 2.5)
    dlat, dlon = fw.composite_offsets(lat, lon, (2, 8, 1, 5))
    assert np.array_equal(dlat, [-5.0, -2.5, 0.0, 2.5, 5.0]) and np.array_equal(dlon, [-7.5, -5.0, -2.5, 0.0, 2.5, 5.0, 7.5])
