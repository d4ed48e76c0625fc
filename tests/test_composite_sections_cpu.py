"""System-relative latitude x pressure sections without a GPU: the definition (the restatement of tests/composite_sections_restatement.py
closes on the oracle's moving-framework per-level tables and scalars), the additive C call ``lec_composite_sections`` (export, second
extension header, ABI 11 and the first extension untouched, struct layout, every refusal on the scalars and on the host copy of the boxes
before any HIP call), the engine's and the command line's refusals, the writer's files on a hand-made result and the source digest.

Bar of the definition: 1e-13 of each term's scale, the bar of tests/test_sections_cpu.py for the fixed box -- ``area_average`` is linear in
its argument, so the two sides differ by the order of a handful of fp64 sums (each case prints its figure)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib
from oracle import lec_oracle as o
from tests import composite_restatement as cr
from tests import composite_sections_restatement as csr
from tests.helpers import synthetic_domain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the definition -----------------------------------------------------------------------------------------------------------------
def test_restatement_closes_on_the_moving_oracle():
    """9 x 9 boxes on 5 levels at 3 places, the first in a corner of the domain."""
    nt, nl, n = 3, 5, 9
    dom = synthetic_domain(nt, nl, n + 4, n + 6, seed=11)
    boxes = [(0, n - 1, 0, n - 1), (6, n + 5, 4, n + 3), (2, n + 1, 1, n)]
    X, C, M, cw = csr.composite_sections(dom, boxes)
    assert X.shape == (nt, 10, nl, n) and C.shape == (nt, 10, n) and M.shape == (10, nl, n) and cw.shape == (nt, n)
    assert np.isfinite(X).all() and np.isfinite(C).all()
    scalars, levels = o.lec_moving(dom, [cr.limits(dom, b) for b in boxes], residuals=False)
    for i, term in enumerate(csr.TERMS):
        lv = np.broadcast_to(np.asarray(levels[term], dtype=np.float64), (nt, nl))
        sc = np.asarray(scalars[term], dtype=np.float64)
        e_lv = np.abs((X[:, i] * cw[:, None, :]).sum(axis=-1) - lv).max() / np.abs(lv).max()
        e_sc = np.abs((C[:, i] * cw).sum(axis=-1) - sc).max() / np.abs(sc).max()
        print(f"{term}: sum_j cw_j(t) X against lec_moving's per-level table {e_lv:.3e}, sum_j cw_j(t) C against its scalar {e_sc:.3e}")
        assert e_lv <= 1e-13 and e_sc <= 1e-13, term
    assert np.allclose(M, X.mean(axis=0), rtol=1e-13, atol=0)


def test_restatement_refuses_different_row_counts():
    dom = synthetic_domain(2, 3, 12, 12, seed=1)
    with pytest.raises(ValueError, match="one row count"):
        csr.composite_sections(dom, [(0, 5, 0, 5), (1, 6, 1, 7)])


# -- the C call ---------------------------------------------------------------------------------------------------------------------
def test_call_is_a_second_extension():
    lib = _lib.load()
    assert _lib.EXT2_EXPORTS == ["lec_composite_sections"]
    assert "lec_composite_sections" not in _lib.EXPORTS and "lec_composite_sections" not in _lib.EXT_EXPORTS
    assert _lib.EXT_EXPORTS == ["lec_composite"] and "lec_sections" in _lib.EXPORTS
    assert lib.lec_composite_sections is not None
    ext2 = open(os.path.join(ROOT, "include", "lec_hip_ext2.h")).read()
    ext = open(os.path.join(ROOT, "include", "lec_hip_ext.h")).read()
    hdr = open(os.path.join(ROOT, "include", "lec_hip.h")).read()
    assert "int lec_composite_sections(const lec_composite_sections_args* args);" in ext2 and '#include "lec_hip.h"' in ext2
    assert "lec_composite_sections" not in hdr and "lec_composite_sections" not in ext
    assert set(re.findall(r"^int (lec_\w+)\(", ext2, flags=re.M)) == set(_lib.EXT2_EXPORTS)
    assert set(re.findall(r"^int (lec_\w+)\(", ext, flags=re.M)) == set(_lib.EXT_EXPORTS)
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11 and "#define LEC_ABI_VERSION 11" in hdr
    mk = open(os.path.join(ROOT, "lorenzcycletoolkit_amd", "csrc", "Makefile")).read()
    assert "lec_composite_sections.hip" in mk and "lec_hip_ext2.h" in mk and "lec_section_core.h" in mk
    A = _lib.CompositeSectionsArgs
    assert ctypes.sizeof(A) == 2 * 8 + 4 * 4 + 8 * 8 == 96
    offs = {n: getattr(A, n).offset for n, _ in A._fields_}
    assert [offs[n] for n in ("rows_d", "levraw_d")] == [0, 8]
    assert [offs[n] for n in ("t_count", "nl", "nyb", "reserved0")] == [16, 20, 24, 28]
    assert [offs[n] for n in ("box_h", "box_d", "lattab2_d", "levtab2_d", "sec_d", "col_d", "secsum_d", "stream")] == list(range(32, 96, 8))
    assert ctypes.sizeof(_lib.SectionsArgs) == 128 and ctypes.sizeof(_lib.CompositeArgs) == 216      # the existing structs are what they were


def test_both_code_objects_share_one_header():
    csrc = os.path.join(ROOT, "lorenzcycletoolkit_amd", "csrc")
    core = open(os.path.join(csrc, "lec_section_core.h")).read()
    assert "#pragma once" in core and "lec_section_rows_kernel" in core and "lec_section_fold_kernel" in core
    for name in ("lec_sections.hip", "lec_composite_sections.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "lec_section_core.h"' in text and "__global__" not in text, name


def test_source_digest_covers_the_second_extension_header(tmp_path, monkeypatch):
    """The digest changes when include/lec_hip_ext2.h changes: computed on a copy of the sources with one byte appended to the header."""
    import shutil
    before = _lib.source_digest()
    pkg = tmp_path / "lorenzcycletoolkit_amd"
    shutil.copytree(os.path.join(ROOT, "lorenzcycletoolkit_amd", "csrc"), pkg / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    monkeypatch.setattr(_lib, "_HERE", str(pkg))
    assert _lib.source_digest() == before
    with open(tmp_path / "include" / "lec_hip_ext2.h", "a") as f:
        f.write("\n")
    assert _lib.source_digest() != before


POINTERS = ["rows_d", "levraw_d", "box_d", "lattab2_d", "levtab2_d", "sec_d", "col_d", "secsum_d"]
T_COUNT, NL, NYB = 3, 4, 5


def _valid_args(boxes=None):
    """Scalars of a valid call over fake (never dereferenced) device pointers and a real host copy of the boxes: every refusal is made on
    the scalars and on that copy, before any HIP call.  Returns (args, the host array, which must outlive the call)."""
    a = _lib.CompositeSectionsArgs()
    for n in POINTERS:
        setattr(a, n, 0x10000)
    host = np.ascontiguousarray(boxes if boxes is not None else [(2, 8, 1, 5), (0, 3, 0, 4), (9, 15, 5, 9)], dtype=np.int32)
    a.box_h = host.ctypes.data
    a.t_count, a.nl, a.nyb, a.reserved0 = T_COUNT, NL, NYB, 0
    return a, host


def _set(**kw):
    return lambda a: [setattr(a, k, v) for k, v in kw.items()]


def _refused(a, code, field):
    lib = _lib.load()
    assert lib.lec_composite_sections(ctypes.byref(a)) == code
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_sections: ") and field.encode() in msg, msg


@pytest.mark.parametrize("field, change", [(n, _set(**{n: None})) for n in POINTERS + ["box_h"]] + [
    ("t_count", _set(t_count=0)), ("nl", _set(nl=1)), ("nyb", _set(nyb=1)), ("reserved0", _set(reserved0=1)),
    ("rows_d", _set(rows_d=0x10008)), ("lattab2_d", _set(lattab2_d=0x10008)),
    # two broken fields: one of them is named
    ("rows_d", _set(rows_d=None, nl=1)), ("t_count", _set(t_count=-1, reserved0=7)), ("nyb", _set(nyb=0, lattab2_d=0x10008)),
])
def test_c_call_refusals_name_the_field(field, change):
    a, host = _valid_args()
    change(a)
    _refused(a, 1, field)          # LEC_ERR_ARG


def test_c_call_beyond_the_limits():
    a, host = _valid_args()
    a.nl = 161                                                          # LEC_MAX_LEVELS = 160
    _refused(a, 2, "nl")           # LEC_ERR_UNSUPPORTED
    a, host = _valid_args()
    a.t_count, a.nl = 1 << 20, 64                                       # 2^26 workgroups of the rows kernel (refused before box_h is read)
    _refused(a, 2, "t_count * nl")
    a, host = _valid_args([(0, 1, 0, (1 << 29) - 1)])
    a.t_count, a.nyb = 1, 1 << 29                                       # 10 * 2^29 threads of the fold
    _refused(a, 2, "10 * nyb")


@pytest.mark.parametrize("boxes, words", [
    ([(2, 8, 1, 5), (0, 3, 0, 5), (9, 15, 5, 9)], b"step 1 has 6 rows, the call's nyb is 5"),
    ([(2, 8, 1, 5), (0, 3, 0, 4), (9, 15, 6, 9)], b"step 2 has 4 rows, the call's nyb is 5"),
    ([(2, 8, 1, 4), (0, 3, 0, 4), (9, 15, 5, 9)], b"step 0 has 4 rows, the call's nyb is 5"),
])
def test_c_call_checks_the_host_copy_of_the_boxes(boxes, words):
    lib = _lib.load()
    a, host = _valid_args(boxes)
    assert lib.lec_composite_sections(ctypes.byref(a)) == 1
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_sections: box_h") and words in msg, msg


def test_c_call_null_args():
    lib = _lib.load()
    assert lib.lec_composite_sections(None) == 1
    assert lib.lec_last_error().startswith(b"lec_composite_sections: ") and b"null args" in lib.lec_last_error()


# -- the engine ---------------------------------------------------------------------------------------------------------------------
def test_engine_refusals_in_words():
    import torch
    from lorenzcycletoolkit_amd.engine import LECEngine
    boxes = [(0, 4, 0, 3), (1, 7, 2, 5), (2, 6, 1, 4)]                  # one row count, two widths
    assert LECEngine._check_composite_sections(boxes, True) == 4
    assert LECEngine._check_composite_sections(boxes, None) == 4
    with pytest.raises(ValueError, match="per_step_boxes=True"):
        LECEngine._check_composite_sections(boxes, False)
    with pytest.raises(ValueError, match="per_step_boxes=True"):
        LECEngine._check_composite_sections(boxes[:1], None)
    with pytest.raises(ValueError, match="ONE row count: the box of step 2 has 5 rows, that of step 0 has 4"):
        LECEngine._check_composite_sections(boxes[:2] + [(2, 6, 1, 5)], True)
    # compute refuses before it touches the engine's tables, the library or a device: an engine that was never initialised will do
    eng = object.__new__(LECEngine)
    t = torch.zeros((3, 2, 8, 8), dtype=torch.float64)
    for bx, kw, words in [
            (boxes, dict(composite_sections=True, per_step_boxes=True, out=torch.empty((3, 58), dtype=torch.float64)), "one process on one GPU"),
            (boxes, dict(composite_sections=True, per_step_boxes=True, merge_dropmask=lambda m: None), "one process on one GPU"),
            (boxes, dict(composite_sections=True, per_step_boxes=False), "per_step_boxes=True"),
            (boxes[:1], dict(composite_sections=True), "per_step_boxes=True"),
            (boxes[:2] + [(2, 6, 1, 5)], dict(composite_sections=True, per_step_boxes=True), "the box of step 2 has 5 rows"),
            (boxes, dict(composite_section_steps=True, per_step_boxes=True), "part of composite_sections=True"),
            (boxes, dict(sections=True, per_step_boxes=True), "sections exist for ONE fixed box")]:       # as before
        with pytest.raises(ValueError, match=words):
            eng.compute(t, t, t, t, None, bx, time_s=np.arange(3.0), **kw)


# -- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags, text", [
    (["-f", "--composite-sections"], "--composite-sections goes with -t / -c: ONE fixed box has --sections"),
    (["-t", "--trackfiles", "a", "b", "--composite-sections"], "--composite-sections follows ONE system: --trackfiles"),
    (["-c", "--choose-systems", "2", "--composite-sections"], "--composite-sections follows ONE system: -c --choose-systems / --choose-starts"),
    (["-t", "--composite-sections", "--gpus", "2"], "--composite-sections runs on one GPU"),
    (["-t", "--sections"], "--sections goes with -f/--fixed: a section lies on the rows of ONE fixed box; the boxes of a -t / -c run "
                           "move, and their sections would be system-relative composites"),           # as before, byte for byte
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
    assert "--composite-sections" in text and "results_composite_sections/" in text
    assert "<term>_dlat_lv.csv" in text and "<term>_dlat.csv" in text
    assert "--composite-sections" in lorenzcycletoolkit.__doc__ and "--composite-sections" in open(os.path.join(ROOT, "README.md")).read()


def test_track_rows_and_latitudes_are_checked_before_a_file_is_written():
    from lorenzcycletoolkit_amd import frameworks as fw
    lat = np.linspace(-60.0, -10.0, 21)
    same = [(0, 6, 0, 4), (3, 12, 2, 6)]                                # one row count, two widths: accepted
    assert fw.composite_sections_check(lat, same) == 5
    with pytest.raises(ValueError, match="--composite-sections needs boxes of ONE row count: the box of step 1 has 6 rows, that of step 0 has 5"):
        fw.composite_sections_check(lat, [same[0], (3, 9, 2, 7)])
    with pytest.raises(ValueError, match="--composite-sections needs evenly spaced latitudes"):
        fw.composite_sections_check(np.sort(lat + 0.3 * np.sin(np.arange(21.0))), same)
    with pytest.raises(ValueError, match="--composite-sections needs boxes of at least 2 latitudes"):
        fw.composite_sections_check(lat, [(0, 4, 3, 3), (1, 5, 4, 4)])
    # BoxData's own check (any caller, before the GPU is touched) does not look at the spacing: it labels nothing
    assert fw.composite_sections_check(np.sort(lat + 0.3 * np.sin(np.arange(21.0))), same, flag="composite sections", lat_too=False) == 5


# -- the writer ---------------------------------------------------------------------------------------------------------------------
def test_writer_headers_and_labels(tmp_path):
    import pandas as pd
    from lorenzcycletoolkit_amd import frameworks as fw
    from lorenzcycletoolkit_amd.constants import SECTION_TERMS
    nt, nl, ny = 3, 4, 5
    rng = np.random.default_rng(0)
    time = pd.date_range("2020-01-01", periods=nt, freq="6h")
    level = np.array([100000.0, 85000.0, 50000.0, 2500.0])
    box = types.SimpleNamespace(
        composite_section_mean=rng.standard_normal((10, nl, ny)), composite_section_lat=rng.standard_normal((nt, 10, ny)),
        composite_section_dlat=np.array([-5.0, -2.5, 0.0, 2.5, 5.0]), PressureData=level,
        time=time.values, row_labels=lambda method: fw.time_labels(time.values, method))
    box.composite_section_mean[3, 2, 1] = np.nan
    out = tmp_path / "results_composite_sections"
    fw.write_composite_section_csvs(box, str(out), "time", "level")
    assert sorted(os.listdir(out)) == sorted([f"{t}_dlat_lv.csv" for t in SECTION_TERMS] + [f"{t}_dlat.csv" for t in SECTION_TERMS])
    m = pd.read_csv(out / "Ke_dlat_lv.csv", index_col=0, float_precision="round_trip")
    assert m.index.name == "level" and list(m.index) == list(level)
    assert [float(c) for c in m.columns] == [-5.0, -2.5, 0.0, 2.5, 5.0]
    assert np.array_equal(m.values, box.composite_section_mean[SECTION_TERMS.index("Ke")], equal_nan=True)      # repr(float): round trip
    lines = open(out / "Ke_dlat_lv.csv").read().splitlines()
    assert lines[0] == "level,-5.0,-2.5,0.0,2.5,5.0" and lines[1].startswith("100000.0,") and lines[4].startswith("2500.0,")
    assert lines[3].split(",")[2] == ""                                  # the NaN: an empty field, as the per-level tables have it
    h = pd.read_csv(out / "Ck_dlat.csv", index_col=0, float_precision="round_trip")
    assert h.index.name == "time" and list(h.index) == ["2020-01-01 00:00:00", "2020-01-01 06:00:00", "2020-01-01 12:00:00"]
    assert [float(c) for c in h.columns] == [-5.0, -2.5, 0.0, 2.5, 5.0]
    assert np.array_equal(h.values, box.composite_section_lat[:, SECTION_TERMS.index("Ck")])
    # the same labels and number formatting as write_section_csvs gives the fixed box
    fixed = types.SimpleNamespace(section_mean=box.composite_section_mean, section_lat=box.composite_section_lat, section_spec_lat=None,
                                  section_latitudes=box.composite_section_dlat, PressureData=level, time=time.values, row_labels=box.row_labels)
    fw.write_section_csvs(fixed, str(tmp_path / "fixed"), "time", "level")
    for t in SECTION_TERMS:
        assert open(out / f"{t}_dlat_lv.csv", "rb").read() == open(tmp_path / "fixed" / f"{t}_lat_lv.csv", "rb").read()
        assert open(out / f"{t}_dlat.csv", "rb").read() == open(tmp_path / "fixed" / f"{t}_lat.csv", "rb").read()
