"""Longitude x pressure sections without a GPU: the definition (the restatement of tests/lonsections_restatement.py closes on the
sections' restatement and on the maps' Hovmoeller), the additive C calls ``lec_lonsections`` / ``lec_composite_lonsections`` (the fourth
additive header, exports, struct layouts, every refusal on the scalars before any HIP call), the engine's and the command line's refusals
and the writers' files on a hand-made result.

Bar of the definition: 1e-13 of each term's scale, the bar of the project's restatement-closure tests on the CPU (tests/test_maps_cpu.py,
tests/test_sections_cpu.py): both sides are the same products summed in another order.  Measured: the zonal average against
``sum_j cw_j sections`` at most 2.4e-15 (65 rows on a ring), the vertical trapezoid against the maps' Hovmoeller at most 7.3e-16 (each
case prints its figure)."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib
from oracle import lec_oracle as o
from tests import lonsections_restatement as lr
from tests import maps_restatement as mr
from tests import ring_restatement as rr
from tests import sections_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEC_IDX = [sr.TERMS.index(k) for k in lr.TERMS]


# -- the definition -----------------------------------------------------------------------------------------------------------------
def _box(kind, ny):
    dom = rr.ring_domain(5, 5, ny, 16, seed=ny)
    return rr.ring_box(dom, -60.0, 60.0) if kind == "ring" else o.make_box(dom, dom.lon[2], dom.lon[13], -60.0, 60.0)


@pytest.mark.parametrize("ny", [5, 65])
@pytest.mark.parametrize("kind", ["ring", "open"])
def test_restatement_closes_on_the_sections_and_the_maps(kind, ny):
    b = _box(kind, ny)
    ring = kind == "ring"
    cw = sr.area_weights(b)
    Y = mr.maps(b, ring)
    X = lr.lon_sections(Y, cw)
    nxb = 16 if ring else 12
    assert X.shape == (5, 6, 5, nxb)
    # the box's own zonal average against sum_j cw_j of the latitude x pressure sections
    S = (sr.sections(b)[:, SEC_IDX] * cw[None, None, None, :]).sum(axis=3)
    scale = np.abs(S).max(axis=(0, 2), keepdims=True)
    err = (np.abs(mr.zonal_average(X, b, ring) - S) / scale).max()
    print(f"{kind} {ny} rows: zonal average of the lon-sections against sum_j cw_j sections: {err:.3e}")
    assert err <= 1e-13
    # s_f times the vertical trapezoid against the Hovmoeller rows of the maps
    H = mr.hovmoller(mr.columns(Y, b.level), cw)
    err = (np.abs(lr.columns(X, b.level) - H) / np.abs(H).max(axis=(0, 2), keepdims=True)).max()
    print(f"{kind} {ny} rows: vertical trapezoid of the lon-sections against the maps' Hovmoeller: {err:.3e}")
    assert err <= 1e-13
    M = lr.time_mean(X)
    assert M.shape == (6, 5, nxb) and np.allclose(M, X.mean(axis=0), rtol=1e-13, atol=0)


def test_nan_rule_of_the_restatement():
    Y = np.ones((2, 6, 3, 4, 5))
    Y[0, :, 1, 2, 3] = np.nan
    X = lr.lon_sections(Y, np.array([0.1, 0.2, 0.3, 0.4]))
    assert np.isnan(X[0, :, 1, 3]).all() and np.isnan(X).sum() == 6
    assert X[1, 0, 0, 0] == ((0.0 + 0.1) + 0.2 + 0.3) + 0.4
    assert np.array_equal(np.isnan(lr.time_mean(X)), np.isnan(X[0]))


# -- the C surface ------------------------------------------------------------------------------------------------------------------
def test_ext4_surface():
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    assert _lib.EXT4_EXPORTS == ["lec_lonsections", "lec_composite_lonsections"]
    assert not set(_lib.EXT4_EXPORTS) & set(_lib.EXPORTS + _lib.EXT_EXPORTS + _lib.EXT2_EXPORTS + _lib.EXT3_EXPORTS)
    ext4 = read("include", "lec_hip_ext4.h")
    assert set(re.findall(r"^int (lec_\w+)\(", ext4, flags=re.M)) == set(_lib.EXT4_EXPORTS) and '#include "lec_hip.h"' in ext4
    for name in ("lec_hip.h", "lec_hip_ext.h", "lec_hip_ext2.h", "lec_hip_ext3.h"):
        assert not set(re.findall(r"^int (lec_\w+)\(", read("include", name), flags=re.M)) & set(_lib.EXT4_EXPORTS), name
    lib = _lib.load()
    for name in _lib.EXT4_EXPORTS:
        assert getattr(lib, name) is not None
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11
    mk = read("lorenzcycletoolkit_amd", "csrc", "Makefile")
    assert "lec_lonsections.hip" in mk and "lec_hip_ext4.h" in mk
    assert "lec_hip_ext4.h" in inspect.getsource(_lib.source_digest)
    assert "EXT4_EXPORTS" in read("__graft_entry__.py")
    src = read("lorenzcycletoolkit_amd", "csrc", "lec_lonsections.hip")
    assert '#include "lec_mapcol.h"' in src and "lec_mapcol_coef_kernel" in src and "lec_mapcol_sum_kernel" in src
    assert "__shared__" not in src and "atomic" not in src
    # one text of the point integrand: the file both kernels include
    csrc = os.path.join(ROOT, "lorenzcycletoolkit_amd", "csrc")
    assert [n for n in sorted(os.listdir(csrc)) if re.search(r"\bdouble yGe\b", read(csrc, n))] == ["lec_mapcol_point.inc"]
    assert '#include "lec_mapcol_point.inc"' in src and '#include "lec_mapcol_point.inc"' in read(csrc, "lec_mapcol.h")


def test_struct_layouts():
    A = _lib.LonSectionsArgs
    assert ctypes.sizeof(A) == 4 * 8 + 13 * 4 + 4 + 7 * 8 + 8 + 4 * 8 == 184
    offs = {n: getattr(A, n).offset for n, _ in A._fields_}
    m = {n: getattr(_lib.MapsArgs, n).offset for n, _ in _lib.MapsArgs._fields_}
    for n in offs:          # lec_maps_args' inputs at lec_maps_args' places
        if n in m and n != "stream":
            assert offs[n] == m[n], n
    assert [offs[n] for n in ("coef_d", "lonsec_d", "lonsecsum_d", "stream")] == [152, 160, 168, 176]
    B = _lib.CompositeLonSectionsArgs
    c = {n: getattr(_lib.CompositeArgs, n).offset for n, _ in _lib.CompositeArgs._fields_}
    offs = {n: getattr(B, n).offset for n, _ in B._fields_}
    for n in offs:
        if n in c and n != "stream":
            assert offs[n] == c[n], n
    assert offs["lonsec_d"] == c["col_d"] and offs["lonsecsum_d"] == c["mapsum_d"] and ctypes.sizeof(B) == ctypes.sizeof(_lib.CompositeArgs) - 8
    # the existing structs are what they were
    assert ctypes.sizeof(_lib.MapsArgs) == 192 and ctypes.sizeof(_lib.CompositeArgs) == 7 * 8 + 10 * 4 + 15 * 8


FIXED_POINTERS = ["tair_d", "u_d", "v_d", "omega_d", "rows_d", "levraw_d", "lattab2_d", "levtab2_d", "lattab_d", "levtab_d", "tcoef_d",
                  "coef_d", "lonsec_d", "lonsecsum_d"]
MOVING_POINTERS = ["tair_d", "u_d", "v_d", "omega_d", "box_d", "boxtab_d", "lattab_d", "lattab2_d", "rows_d", "levraw_d", "levtab_d",
                   "levtab2_d", "coef_d", "lonsec_d", "lonsecsum_d"]


def fixed_args():
    """Scalars of a valid ``lec_lonsections`` call over fake (never dereferenced) pointers: every refusal is made on the scalars."""
    a = _lib.LonSectionsArgs()
    for n in FIXED_POINTERS:
        setattr(a, n, 0x10000)
    a.dtype, a.nt, a.nl, a.ny, a.nx = _lib.LEC_F64, 5, 4, 9, 16
    a.t_begin, a.t_count, a.iw, a.ie, a.js, a.jn, a.ring = 1, 3, 2, 13, 1, 7, 0
    a.inv_hdeg = 1.0
    return a


def moving_args(boxes=None):
    """The same for ``lec_composite_lonsections``: dT/dt from the cube's own neighbours; returns (args, the host boxes it points to)."""
    a = _lib.CompositeLonSectionsArgs()
    for n in MOVING_POINTERS + ["tcoef_d"]:
        setattr(a, n, 0x10000)
    a.dtype, a.nt, a.nl, a.ny, a.nx = _lib.LEC_F64, 5, 4, 9, 16
    a.t_begin, a.t_count, a.nyb, a.nxb = 1, 3, 4, 6
    box = np.ascontiguousarray([(1, 6, 2, 5), (2, 7, 3, 6), (10, 15, 5, 8)] if boxes is None else boxes, dtype=np.int32)
    a.box_h = box.ctypes.data
    return a, box


def _set(**kw):
    return lambda a: [setattr(a, k, v) for k, v in kw.items()]


FIXED_ARG = [(n, _set(**{n: None})) for n in FIXED_POINTERS] + [
    ("dtype", _set(dtype=_lib.LEC_I16)), ("ring", _set(ring=2)), ("ring", _set(ring=1)),     # a ring of part of the circle
    ("reserved0", _set(reserved0=1)), ("nt", _set(nt=1, t_begin=0, t_count=1)), ("nl", _set(nl=1)), ("ny", _set(ny=1)),
    ("nx", _set(nx=2)), ("t_begin", _set(t_begin=-1)), ("t_begin", _set(t_begin=5)), ("t_count", _set(t_count=0)),
    ("t_count", _set(t_count=5)), ("iw", _set(iw=-1)), ("iw", _set(iw=16)), ("ie", _set(ie=16)), ("ie", _set(ie=1)),
    ("nxb", _set(ie=3)),                                                                      # two columns
    ("js", _set(js=-1)), ("js", _set(js=9)), ("nyb", _set(jn=1)), ("jn", _set(jn=9)),          # jn = js: one row
    ("rows_d", _set(rows_d=0x10008)), ("lattab2_d", _set(lattab2_d=0x10008)), ("coef_d", _set(coef_d=0x10008)),
    ("levraw_d", _set(levraw_d=0x10004)), ("levtab2_d", _set(levtab2_d=0x10004)), ("lattab_d", _set(lattab_d=0x10004)),
    ("levtab_d", _set(levtab_d=0x10004)), ("tcoef_d", _set(tcoef_d=0x10004)), ("lonsec_d", _set(lonsec_d=0x10004)),
    ("lonsecsum_d", _set(lonsecsum_d=0x10004)), ("tair_d", _set(tair_d=0x10004)),
    ("omega_d", _set(omega_d=0x10002, dtype=_lib.LEC_F32)),
]
FIXED_UNSUPPORTED = [
    ("nl", _set(nl=161)),                                                                     # LEC_MAX_LEVELS = 160
    ("t_count * nl", _set(nt=1 << 20, nl=64, t_count=1 << 20, t_begin=0)),                    # 2^26 workgroups of the section kernel
    ("6 * nl * columns", _set(nl=160, nx=1 << 23, iw=0, ie=(1 << 23) - 1)),                   # 6 x 160 x 2^23 threads of the time sums
]
MOVING_ARG = [(n, _set(**{n: None})) for n in MOVING_POINTERS + ["box_h"]] + [
    ("dtype", _set(dtype=_lib.LEC_I16)), ("reserved0", _set(reserved0=1)),
    ("tm_d without tp_d", _set(tm_d=0x10000)), ("tp_d without tm_d", _set(tp_d=0x10000)),
    ("dTdt_d together", _set(dTdt_d=0x10000, tm_d=0x10000, tp_d=0x10000)), ("tcoef_d", _set(tcoef_d=None)),
    ("nt", _set(nt=0)), ("nt", _set(nt=1, t_begin=0, t_count=1)), ("nl", _set(nl=1)), ("nyb", _set(nyb=1)), ("nxb", _set(nxb=2)),
    ("ny", _set(ny=3)), ("nx", _set(nx=5)), ("t_begin", _set(t_begin=5)), ("t_count", _set(t_count=5)),
    ("rows_d", _set(rows_d=0x10008)), ("lattab2_d", _set(lattab2_d=0x10008)), ("coef_d", _set(coef_d=0x10008)),
    ("box_d", _set(box_d=0x10002)), ("boxtab_d", _set(boxtab_d=0x10004)), ("dTdt_d", _set(dTdt_d=0x10004)),
    ("lonsec_d", _set(lonsec_d=0x10004)), ("lonsecsum_d", _set(lonsecsum_d=0x10004)),
    ("tm_d", _set(tm_d=0x10004, tp_d=0x10000)),
]
MOVING_BOXES = [("step 1 is 4 x 5", [(1, 6, 2, 5), (2, 6, 3, 6), (10, 15, 5, 8)]), ("step 1 is 3 x 6", [(1, 6, 2, 5), (2, 7, 3, 5), (10, 15, 5, 8)]),
                ("step 2", [(1, 6, 2, 5), (2, 7, 3, 6), (11, 16, 5, 8)]), ("step 0", [(1, 6, -1, 2), (2, 7, 3, 6), (10, 15, 5, 8)])]

@pytest.mark.parametrize("field, change", FIXED_ARG)
def test_fixed_refusals_name_the_field(field, change):
    lib = _lib.load()
    a = fixed_args()
    change(a)
    assert lib.lec_lonsections(ctypes.byref(a)) == 1          # LEC_ERR_ARG
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_lonsections:") and field.encode() in msg, msg


@pytest.mark.parametrize("field, change", FIXED_UNSUPPORTED)
def test_fixed_beyond_the_limits(field, change):
    lib = _lib.load()
    a = fixed_args()
    change(a)
    assert lib.lec_lonsections(ctypes.byref(a)) == 2          # LEC_ERR_UNSUPPORTED
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_lonsections:") and field.encode() in msg, msg


@pytest.mark.parametrize("field, change", MOVING_ARG)
def test_moving_refusals_name_the_field(field, change):
    lib = _lib.load()
    a, box = moving_args()
    change(a)
    assert lib.lec_composite_lonsections(ctypes.byref(a)) == 1
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_lonsections:") and field.encode() in msg, msg


@pytest.mark.parametrize("words, boxes", MOVING_BOXES)
def test_moving_refuses_boxes_on_the_host_copy(words, boxes):
    lib = _lib.load()
    a, box = moving_args(boxes)
    assert lib.lec_composite_lonsections(ctypes.byref(a)) == 1
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_lonsections: box_h") and words.encode() in msg, msg


def test_moving_beyond_the_limits():
    lib = _lib.load()
    a, box = moving_args()
    a.nl = 161
    assert lib.lec_composite_lonsections(ctypes.byref(a)) == 2 and b"nl" in lib.lec_last_error()
    n = 1 << 14                                                 # 2^14 steps x 160 levels x 26 segments of 64 columns >= 2^26
    a, box = moving_args([(0, 1663, 0, 3)] * n)
    a.nt, a.nl, a.nx, a.nxb, a.t_begin, a.t_count = n, 160, 1664, 1664, 0, n
    assert lib.lec_composite_lonsections(ctypes.byref(a)) == 2
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_lonsections:") and b"t_count * nl" in msg and b"2^26" in msg, msg


def test_null_args():
    lib = _lib.load()
    for name in _lib.EXT4_EXPORTS:
        assert getattr(lib, name)(None) == 1
        assert lib.lec_last_error().startswith(name.encode() + b":") and b"null args" in lib.lec_last_error()


# -- the engine ---------------------------------------------------------------------------------------------------------------------
def test_engine_refusals_in_words():
    import torch
    from lorenzcycletoolkit_amd.engine import LECEngine
    with pytest.raises(ValueError, match="longitude-pressure sections exist for ONE fixed box"):
        LECEngine._check_lonsections([(0, 3, 0, 3)] * 2, None)
    with pytest.raises(ValueError, match="ONE fixed box"):
        LECEngine._check_lonsections([(0, 3, 0, 3)], True)
    for kw in (dict(steps=object()), dict(tm=object()), dict(tp=object())):
        with pytest.raises(ValueError, match="ONE fixed box"):
            LECEngine._check_lonsections([(0, 3, 0, 3)], False, **kw)
    LECEngine._check_lonsections([(0, 3, 0, 3)], False)
    # compute refuses before it touches the engine's tables, the library or a device: an engine that was never initialised will do
    eng = object.__new__(LECEngine)
    t = torch.zeros((3, 2, 4, 4), dtype=torch.float64)
    box = [(0, 3, 0, 3)]
    for kw, words in [(dict(lon_sections=True, out=torch.empty((3, 58), dtype=torch.float64)), "longitude-pressure sections run in one process"),
                      (dict(lon_sections=True, merge_dropmask=lambda m: None), "longitude-pressure sections run in one process"),
                      (dict(lon_sections=True, dTdt=t), "longitude-pressure sections: a dTdt cube is not supported"),
                      (dict(lon_sections=True, with_q=False), "longitude-pressure sections need with_q"),
                      (dict(lon_sections=True, per_step_boxes=True), "longitude-pressure sections exist for ONE fixed box"),
                      (dict(lon_sections=True, steps=torch.zeros((3, 3), dtype=torch.int32)), "ONE fixed box"),
                      (dict(lon_sections=True, tm=t, tp=t), "ONE fixed box"),
                      (dict(lon_section_steps=True), "part of lon_sections=True"),
                      (dict(composite_lon_section_steps=True), "part of composite_lon_sections=True"),
                      (dict(composite_lon_sections=True), "composite longitude-pressure sections exist for per-step boxes"),
                      (dict(composite_lon_sections=True, per_step_boxes=True, steps=torch.zeros((3, 3), dtype=torch.int32)),
                       "composite longitude-pressure sections: a step table"),
                      (dict(composite_lon_sections=True, per_step_boxes=True, with_q=False), "composite longitude-pressure sections need with_q"),
                      (dict(composite_lon_sections=True, per_step_boxes=True, merge_dropmask=lambda m: None),
                       "composite longitude-pressure sections run in one process")]:
        with pytest.raises(ValueError, match=words):
            eng.compute(t, t, t, t, None, box, time_s=np.arange(3.0), **kw)
    with pytest.raises(ValueError, match="ONE fixed box"):
        eng.compute(t, t, t, t, None, box * 3, time_s=np.arange(3.0), lon_sections=True)
    with pytest.raises(ValueError, match=r"composite longitude-pressure sections need boxes of ONE shape: the box of step 2 has 4 x 3 points "
                                         r"\(rows x columns\), that of step 0 has 4 x 4"):
        eng.compute(t, t, t, t, None, [(0, 3, 0, 3), (0, 3, 0, 3), (1, 3, 0, 3)], time_s=np.arange(3.0), composite_lon_sections=True)
    with pytest.raises(ValueError, match="composite longitude-pressure sections need at least 3 box columns"):
        eng.compute(t, t, t, t, None, [(0, 1, 0, 3)] * 3, time_s=np.arange(3.0), composite_lon_sections=True)
    eng.lon = np.array([0.0, 1.0, 2.5, 3.0])
    with pytest.raises(ValueError, match="composite longitude-pressure sections need evenly spaced longitudes"):
        eng.compute(t, t, t, t, None, box * 3, time_s=np.arange(3.0), composite_lon_sections=True)
    # the composites' own words are what they were
    with pytest.raises(ValueError, match="composites exist for per-step boxes .*ONE fixed box has maps=True"):
        LECEngine._check_composites(box, None)


# -- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags, text", [
    (["-t", "--lon-sections"], "--lon-sections goes with -f/--fixed"),
    (["-c", "--lon-sections"], "--lon-sections goes with -f/--fixed"),
    (["-f", "--lon-sections", "--gpus", "2"], "--lon-sections runs on one GPU"),
    (["-f", "--periodic", "--lon-sections", "--gpus", "4"], "--lon-sections runs on one GPU"),
    (["-f", "--lon-sections", "--ingest", "device"], "--lon-sections prepares the data on the host: --ingest device / --device-ingest is not supported"),
    (["-f", "--lon-sections", "--device-ingest"], "--lon-sections prepares the data on the host: --ingest device / --device-ingest is not supported"),
    (["-f", "--periodic", "--lon-sections", "--wavenumbers", "4", "--wavenumbers-chunk", "2"],
     "--lon-sections prepares the data on the host: --wavenumbers-chunk"),
    (["-f", "--composite-lon-sections"], "--composite-lon-sections goes with -t / -c"),
    (["-t", "--trackfiles", "a", "b", "--composite-lon-sections"], "--composite-lon-sections follows ONE system: --trackfiles"),
    (["-c", "--choose-systems", "2", "--composite-lon-sections"], "--composite-lon-sections follows ONE system: -c --choose-systems / --choose-starts"),
    (["-c", "--choose-starts", "starts.csv", "--composite-lon-sections"], "--composite-lon-sections follows ONE system: -c --choose-systems / --choose-starts"),
    (["-t", "--composite-lon-sections", "--gpus", "2"], "--composite-lon-sections runs on one GPU"),
    (["-t", "--composite-lon-sections", "--ingest", "device"], "--composite-lon-sections prepares the data on the host"),
    (["-c", "--composite-lon-sections", "--device-ingest"], "--composite-lon-sections prepares the data on the host"),
])
def test_cli_refusals(tmp_path, monkeypatch, flags, text):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    if "--choose-starts" in flags:              # (the file's presence is looked at first)
        (tmp_path / "starts.csv").write_text("time,lat,lon\n")
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", *flags])
    assert text in str(e.value)
    assert not os.path.exists(tmp_path / "LEC_Results")          # refused before anything was created


def test_cli_help_and_documents_name_the_flags(capsys):
    import lorenzcycletoolkit
    with pytest.raises(SystemExit):
        lorenzcycletoolkit.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    readme, design = open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "DESIGN.md")).read()
    for flag, where, name in (("--lon-sections", "results_lon_sections/", "<term>_lon_lv.csv"),
                              ("--composite-lon-sections", "results_composite_lon_sections/", "<term>_dlon_lv.csv")):
        assert flag in text and where in text and name in text
        assert flag in lorenzcycletoolkit.__doc__ and flag in readme and flag in design
    assert "4.2h" in design


# -- the writers --------------------------------------------------------------------------------------------------------------------
def test_writers_headers_and_labels(tmp_path):
    import pandas as pd
    from lorenzcycletoolkit_amd import frameworks as fw
    from lorenzcycletoolkit_amd.constants import MAP_TERMS
    nl, nx = 3, 5
    rng = np.random.default_rng(0)
    box = types.SimpleNamespace(
        lonsection_mean=rng.standard_normal((6, nl, nx)), lonsection_longitudes=np.array([-10.0, -7.5, -5.0, -2.5, 0.0]),
        composite_lonsection_mean=rng.standard_normal((6, nl, nx)), composite_lonsection_dlon=np.array([-5.0, -2.5, 0.0, 2.5, 5.0]),
        PressureData=np.array([10000.0, 50000.0, 100000.0]))
    box.lonsection_mean[1, 2, 3] = np.nan
    out = tmp_path / "results_lon_sections"
    fw.write_lon_section_csvs(box, str(out), "level")
    assert sorted(os.listdir(out)) == sorted(f"{t}_lon_lv.csv" for t in MAP_TERMS)
    m = pd.read_csv(out / "Ke_lon_lv.csv", index_col=0, float_precision="round_trip")
    assert m.index.name == "level" and list(m.index) == [10000.0, 50000.0, 100000.0]
    assert [float(c) for c in m.columns] == [-10.0, -7.5, -5.0, -2.5, 0.0]
    assert np.array_equal(m.values, box.lonsection_mean[1], equal_nan=True)            # repr(float): the values round-trip
    lines = open(out / "Ke_lon_lv.csv").read().splitlines()
    assert lines[0] == "level,-10.0,-7.5,-5.0,-2.5,0.0" and lines[1].startswith("10000.0,") and lines[3].split(",")[4] == ""
    # the number format is the --sections files'
    sec = types.SimpleNamespace(section_mean=np.broadcast_to(box.lonsection_mean[0], (10, nl, nx)), section_lat=np.zeros((1, 10, nx)),
                                section_spec_lat=None, section_latitudes=box.lonsection_longitudes, PressureData=box.PressureData,
                                time=pd.date_range("2020-01-01", periods=1).values,
                                row_labels=lambda method: fw.time_labels(pd.date_range("2020-01-01", periods=1).values, method))
    fw.write_section_csvs(sec, str(tmp_path / "sec"), "time", "level")
    assert open(tmp_path / "sec" / "Az_lat_lv.csv").read() == open(out / "Ae_lon_lv.csv").read()
    out = tmp_path / "results_composite_lon_sections"
    fw.write_composite_lon_section_csvs(box, str(out), "level")
    assert sorted(os.listdir(out)) == sorted(f"{t}_dlon_lv.csv" for t in MAP_TERMS)
    m = pd.read_csv(out / "Ge_dlon_lv.csv", index_col=0, float_precision="round_trip")
    assert m.index.name == "level" and list(m.index) == [10000.0, 50000.0, 100000.0]
    assert [float(c) for c in m.columns] == [-5.0, -2.5, 0.0, 2.5, 5.0]
    assert np.array_equal(m.values, box.composite_lonsection_mean[5])
