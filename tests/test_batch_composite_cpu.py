"""Composites of a batch of tracks without a GPU: the definition (tests/batch_composite_restatement.py closes on the oracle's
moving-framework scalars track by track), the additive C calls ``lec_composite_steps`` / ``lec_composite_ensemble`` (exports, the third
extension header, ABI 11, struct layouts, every refusal on the scalars and on the host copies of the tables before any HIP call), the
engine's and the command line's refusals and the documentation.

Bar of the definition: 1e-13 of each term's scale, tests/test_composite_cpu.py's (each case prints its figure)."""
import ctypes
import os
import re

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib
from tests import batch_composite_restatement as br
from tests import composite_restatement as cr
from tests.helpers import synthetic_domain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the definition -----------------------------------------------------------------------------------------------------------------
def test_restatement_closes_on_the_moving_oracle_track_by_track():
    nyb, nxb, nl = 5, 7, 5
    dom = synthetic_domain(7, nl, nyb + 4, nxb + 6, seed=11, dt_s=10800.0)
    at = lambda i, j: (i, i + nxb - 1, j, j + nyb - 1)
    tracks = [(np.arange(7), [at(n % 7, n % 5) for n in range(7)]), (np.arange(0, 7, 2), [at(6 - n, 4 - n) for n in range(4)]),
              (np.array([3, 4]), [at(2, 1), at(3, 2)])]
    per, ens = br.composites(dom, tracks)
    assert ens.shape == (6, nyb, nxb) and np.isfinite(ens).all()
    assert np.allclose(ens, (per[0][2] + per[1][2] + per[2][2]) / 3, rtol=1e-14, atol=0)
    for k, (u, boxes) in enumerate(tracks):
        C, H, M = per[k]
        assert C.shape == (len(u), 6, nyb, nxb) and H.shape == (len(u), 6, nxb) and M.shape == (6, nyb, nxb)
        za, sc = br.closure(dom, u, boxes, H)
        for i, term in enumerate(cr.TERMS):
            e = np.abs(za[:, i] - sc[:, i]).max() / np.abs(sc[:, i]).max()
            print(f"track {k} {term}: the box's zonal average of the Hovmoeller against lec_moving's scalar: {e:.3e}")
            assert e <= 1e-13, (k, term)


# -- the C calls --------------------------------------------------------------------------------------------------------------------
def test_calls_are_the_third_extension():
    lib = _lib.load()
    assert _lib.EXT3_EXPORTS == ["lec_composite_steps", "lec_composite_ensemble"]
    assert not set(_lib.EXT3_EXPORTS) & set(_lib.EXPORTS + _lib.EXT_EXPORTS + _lib.EXT2_EXPORTS)
    read = lambda n: open(os.path.join(ROOT, "include", n)).read()
    ext3 = read("lec_hip_ext3.h")
    assert set(re.findall(r"^int (lec_\w+)\(", ext3, flags=re.M)) == set(_lib.EXT3_EXPORTS) and '#include "lec_hip.h"' in ext3
    for name in _lib.EXT3_EXPORTS:
        assert getattr(lib, name) is not None
        for old in ("lec_hip.h", "lec_hip_ext.h", "lec_hip_ext2.h"):
            assert name not in read(old), (name, old)
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11 and "#define LEC_ABI_VERSION 11" in read("lec_hip.h")
    mk = open(os.path.join(ROOT, "lorenzcycletoolkit_amd", "csrc", "Makefile")).read()
    assert "lec_composite_steps.hip" in mk and "lec_hip_ext3.h" in mk
    import inspect
    assert "lec_hip_ext3.h" in inspect.getsource(_lib.source_digest)
    assert "EXT3_EXPORTS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def _fields_of(header: str, struct: str):
    """[(type, name)] of the struct's members as the header declares them, in order."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, flags=re.S).group(1)
    out = []
    for line in body.splitlines():
        line = re.sub(r"/\*.*?\*/", "", line).strip().rstrip(";")
        if not line:
            continue
        if "," in line:                                  # int32_t a, b, c
            typ, rest = line.split(" ", 1)
            out += [(typ, n.strip()) for n in rest.split(",")]
        else:                                            # const double* name
            typ, name = line.rsplit(" ", 1)
            assert "*" not in name
            out.append((typ.strip(), name.strip()))
    return out


@pytest.mark.parametrize("struct, cls, size", [("lec_composite_steps_args", "CompositeStepsArgs", 4 * 8 + 10 * 4 + 19 * 8),
                                               ("lec_composite_ensemble_args", "CompositeEnsembleArgs", 3 * 8 + 4 * 4 + 3 * 8)])
def test_ctypes_structs_match_the_header(struct, cls, size):
    header = open(os.path.join(ROOT, "include", "lec_hip_ext3.h")).read()
    A = getattr(_lib, cls)
    declared = _fields_of(header, struct)
    assert [n for _, n in declared] == [n for n, _ in A._fields_]
    off = 0
    for (typ, name), (_, ctype) in zip(declared, A._fields_):
        want = 4 if typ == "int32_t" else 8
        assert ctypes.sizeof(ctype) == want, name
        off = (off + want - 1) // want * want
        assert getattr(A, name).offset == off, name
        off += want
    assert ctypes.sizeof(A) == size == (off + 7) // 8 * 8


POINTERS = ["tair_d", "u_d", "v_d", "omega_d", "step_d", "seg_d", "box_d", "boxtab_d", "lattab_d", "lattab2_d", "rows_d", "levraw_d", "levtab_d",
            "levtab2_d", "tcoef_d", "coef_d", "col_d", "mapsum_d", "hov_d"]
BOXES = [(2, 8, 1, 4), (0, 6, 0, 3), (9, 15, 5, 8), (3, 9, 2, 5)]
STEPS = [(0, 0, 2), (2, 0, 2), (1, 1, 4), (4, 1, 4)]
SEG = [0, 2, 4]


def _valid_args(boxes=BOXES, steps=STEPS, seg=SEG):
    """Scalars of a valid call over fake (never dereferenced) device pointers and real host copies of the three tables: every refusal is
    made on the scalars and on those copies, before any HIP call.  Returns (args, the host arrays, which must outlive the call)."""
    a = _lib.CompositeStepsArgs()
    for n in POINTERS:
        setattr(a, n, 0x10000)
    host = [np.ascontiguousarray(x, dtype=np.int32) for x in (boxes, steps, seg)]
    a.box_h, a.step_h, a.seg_h = (h.ctypes.data for h in host)
    a.dtype, a.nt, a.nl, a.ny, a.nx = _lib.LEC_F64, 5, 4, 9, 16
    a.s_count, a.nyb, a.nxb, a.n_seg = len(boxes), 4, 7, len(seg) - 1
    return a, host


def _set(**kw):
    return lambda a: [setattr(a, k, v) for k, v in kw.items()]


@pytest.mark.parametrize("field, change", [(n, _set(**{n: None})) for n in POINTERS + ["box_h", "step_h", "seg_h"]] + [
    ("dtype", _set(dtype=_lib.LEC_I16)), ("reserved0", _set(reserved0=1)), ("nt", _set(nt=0)), ("s_count", _set(s_count=0)),
    ("nl", _set(nl=1)), ("nyb", _set(nyb=1)), ("nxb", _set(nxb=2)), ("ny", _set(ny=3)), ("nx", _set(nx=6)), ("n_seg", _set(n_seg=0)),
    ("rows_d", _set(rows_d=0x10008)), ("lattab2_d", _set(lattab2_d=0x10008)), ("coef_d", _set(coef_d=0x10008)),
    ("box_d", _set(box_d=0x10002)), ("step_d", _set(step_d=0x10002)), ("seg_d", _set(seg_d=0x10002)),
    ("levraw_d", _set(levraw_d=0x10004)), ("levtab2_d", _set(levtab2_d=0x10004)), ("lattab_d", _set(lattab_d=0x10004)),
    ("levtab_d", _set(levtab_d=0x10004)), ("tcoef_d", _set(tcoef_d=0x10004)), ("boxtab_d", _set(boxtab_d=0x10004)),
    ("col_d", _set(col_d=0x10004)), ("hov_d", _set(hov_d=0x10004)), ("mapsum_d", _set(mapsum_d=0x10004)),
    ("tair_d", _set(tair_d=0x10004)), ("omega_d", _set(omega_d=0x10002, dtype=_lib.LEC_F32)),
])
def test_steps_call_refusals_name_the_field(field, change):
    lib = _lib.load()
    a, host = _valid_args()
    change(a)
    assert lib.lec_composite_steps(ctypes.byref(a)) == 1          # LEC_ERR_ARG
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_steps:") and field.encode() in msg, msg


@pytest.mark.parametrize("kw, words", [
    (dict(steps=[(0, 0, 2), (2, 0, 5), (1, 1, 4), (4, 1, 4)]), b"step_h: box 1 names cube step 5 as its t_next (entry 2), outside [0, 5)"),
    (dict(steps=[(0, 0, 2), (2, 0, 2), (1, -1, 4), (4, 1, 4)]), b"step_h: box 2 names cube step -1 as its t_prev (entry 1), outside [0, 5)"),
    (dict(steps=[(0, 0, 2), (2, 0, 2), (1, 1, 4), (7, 1, 4)]), b"step_h: box 3 names cube step 7 as its t (entry 0)"),
    (dict(seg=[1, 2, 4]), b"seg_h[0] must be 0"),
    (dict(seg=[0, 3, 2, 4]), b"seg_h: offsets must ascend and no segment may be empty: seg_h[1] = 3, seg_h[2] = 2"),
    (dict(seg=[0, 2, 2, 4]), b"no segment may be empty: seg_h[1] = 2, seg_h[2] = 2"),
    (dict(seg=[0, 2, 3]), b"seg_h[n_seg] = 3 must be s_count = 4"),
    (dict(seg=[0, 2, 5]), b"seg_h[n_seg] = 5 must be s_count = 4"),
    (dict(boxes=[(2, 8, 1, 4), (0, 7, 0, 3), (9, 15, 5, 8), (3, 9, 2, 5)]), b"box_h: box 1 is 4 x 8 (rows x columns), the call's nyb x nxb is 4 x 7"),
    (dict(boxes=[(2, 8, 1, 4), (0, 6, 0, 3), (10, 16, 5, 8), (3, 9, 2, 5)]), b"box_h: box 2 {iw, ie, js, jn} = {10, 16, 5, 8} lies outside the 9 x 16 cube"),
])
def test_steps_call_checks_the_host_copies_of_its_tables(kw, words):
    lib = _lib.load()
    a, host = _valid_args(**kw)
    assert lib.lec_composite_steps(ctypes.byref(a)) == 1
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_steps: ") and words in msg, msg


def test_steps_call_beyond_the_limits():
    lib = _lib.load()
    a, host = _valid_args()
    a.nl = 161
    assert lib.lec_composite_steps(ctypes.byref(a)) == 2 and b"nl above LEC_MAX_LEVELS" in lib.lec_last_error()
    # n_seg * 6 * nyb * nxb >= 2^32 - 256: 2^20 one-box segments of 32 x 32 points
    n = 1 << 20
    boxes = np.tile(np.array([(0, 31, 0, 31)], dtype=np.int32), (n, 1))
    a, host = _valid_args(boxes=boxes, steps=np.zeros((n, 3), dtype=np.int32), seg=np.arange(n + 1))
    a.ny, a.nx, a.nyb, a.nxb = 32, 32, 32, 32
    assert lib.lec_composite_steps(ctypes.byref(a)) == 2          # LEC_ERR_UNSUPPORTED
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_steps:") and b"n_seg * 6 * nyb * nxb" in msg, msg
    a.nl = 64                                                     # lec_maps' limits come first: 2^26 workgroups of the factors kernel
    assert lib.lec_composite_steps(ctypes.byref(a)) == 2 and b"t_count * nl" in lib.lec_last_error()


def test_null_args():
    lib = _lib.load()
    for call, name in ((lib.lec_composite_steps, b"lec_composite_steps:"), (lib.lec_composite_ensemble, b"lec_composite_ensemble:")):
        assert call(None) == 1
        assert lib.lec_last_error().startswith(name) and b"null args" in lib.lec_last_error()


def _valid_ensemble(counts=(3, 1, 2)):
    a = _lib.CompositeEnsembleArgs()
    for n in ("mapsum_d", "count_d", "mean_d", "ens_d"):
        setattr(a, n, 0x10000)
    host = np.ascontiguousarray(counts, dtype=np.int32)
    a.count_h = host.ctypes.data
    a.n_track, a.nyb, a.nxb = len(counts), 4, 7
    return a, host


@pytest.mark.parametrize("field, change", [(n, _set(**{n: None})) for n in ("mapsum_d", "count_h", "count_d", "mean_d", "ens_d")] + [
    ("reserved0", _set(reserved0=1)), ("n_track", _set(n_track=0)), ("nyb", _set(nyb=0)), ("nxb", _set(nxb=0)),
    ("count_d", _set(count_d=0x10002)), ("mapsum_d", _set(mapsum_d=0x10004)), ("mean_d", _set(mean_d=0x10004)), ("ens_d", _set(ens_d=0x10004)),
])
def test_ensemble_call_refusals_name_the_field(field, change):
    lib = _lib.load()
    a, host = _valid_ensemble()
    change(a)
    assert lib.lec_composite_ensemble(ctypes.byref(a)) == 1
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_composite_ensemble:") and field.encode() in msg, msg


def test_ensemble_call_checks_the_counts_and_the_limit():
    lib = _lib.load()
    a, host = _valid_ensemble((3, 0, 2))
    assert lib.lec_composite_ensemble(ctypes.byref(a)) == 1
    assert b"lec_composite_ensemble: count_h: track 1 has 0 steps" in lib.lec_last_error()
    a, host = _valid_ensemble()
    a.nyb, a.nxb = 1 << 15, 1 << 15
    assert lib.lec_composite_ensemble(ctypes.byref(a)) == 2 and b"6 * nyb * nxb" in lib.lec_last_error()


# -- the engine ---------------------------------------------------------------------------------------------------------------------
def test_engine_refusals_in_words():
    import torch
    from lorenzcycletoolkit_amd.engine import LECEngine
    boxes = [(0, 4, 0, 3), (1, 5, 2, 5), (2, 6, 1, 4)]
    assert LECEngine._check_batch_composites(boxes, 3, [2, 1]) == (4, 5)
    with pytest.raises(ValueError, match="sizes sum to 2, the step table has 3 rows and there are 3 boxes"):
        LECEngine._check_batch_composites(boxes, 3, [1, 1])
    with pytest.raises(ValueError, match=r"at least one box, the sizes are \[3, 0\]"):
        LECEngine._check_batch_composites(boxes, 3, [3, 0])
    with pytest.raises(ValueError, match=r"box 2 has 4 x 6 points \(rows x columns\), box 0 has 4 x 5"):
        LECEngine._check_batch_composites(boxes[:2] + [(2, 7, 1, 4)], 3, [3])
    with pytest.raises(ValueError, match="at least 3 box columns"):
        LECEngine._check_batch_composites([(0, 1, 0, 3)] * 3, 3, [3])
    with pytest.raises(ValueError, match="evenly spaced longitudes"):
        LECEngine._check_batch_composites(boxes, 3, [3], False)
    # compute refuses before it touches the engine's tables, the library or a device: an engine that was never initialised will do
    eng = object.__new__(LECEngine)
    t = torch.zeros((3, 2, 8, 8), dtype=torch.float64)
    st = torch.zeros((3, 3), dtype=torch.int32)
    for kw, words in [(dict(batch_composites=[3]), "need a step table"),
                      (dict(batch_composites=[2], steps=st), "sizes sum to 2"),
                      (dict(batch_composites=[3, 0], steps=st), "at least one box"),
                      (dict(batch_composites=[3], steps=st, with_q=False), "batch composites need with_q"),
                      (dict(batch_composites=[3], steps=st, out=torch.empty((3, 58), dtype=torch.float64)), "one process on one GPU"),
                      (dict(batch_composites=[3], steps=st, merge_dropmask=lambda m: None), "one process on one GPU"),
                      (dict(batch_composite_steps=True, steps=st), "part of batch_composites=sizes"),
                      (dict(composites=True, steps=st), "step table")]:          # as before: composites exist for ONE track
        with pytest.raises(ValueError, match=words):
            eng.compute(t, t, t, t, None, boxes, per_step_boxes=True, **kw)
    with pytest.raises(ValueError, match=r"box 1 has 4 x 6 points"):
        eng.compute(t, t, t, t, None, [boxes[0], (1, 6, 2, 5), boxes[2]], per_step_boxes=True, batch_composites=[3], steps=st)
    from lorenzcycletoolkit_amd import tables
    from lorenzcycletoolkit_amd.engine import PreparedBoxes
    lat, lon = np.linspace(-40.0, -33.0, 8), np.linspace(-60.0, -53.0, 8)
    tall = PreparedBoxes(boxes, tables.build_box_tables(lat, lon, boxes, nyb_min=6), {})
    with pytest.raises(ValueError, match="the boxes' own row count"):
        eng.compute(t, t, t, t, None, tall, per_step_boxes=True, batch_composites=[3], steps=st)
    uneven = PreparedBoxes(boxes, tables.build_box_tables(lat, np.sort(lon + 0.3 * np.sin(np.arange(8.0))), boxes), {})
    assert not uneven.bt.lon_uniform
    with pytest.raises(ValueError, match="evenly spaced longitudes"):
        eng.compute(t, t, t, t, None, uneven, per_step_boxes=True, batch_composites=[3], steps=st)


# -- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags, text", [
    (["-f", "--batch-composites"], "--batch-composites goes with -t --trackfiles or -c --choose-systems / --choose-starts"),
    (["-t", "--batch-composites"], "ONE system has --composites"),
    (["-t", "--trackfile", "a", "--batch-composites"], "ONE system has --composites (-t --trackfile FILE --composites"),
    (["-c", "--batch-composites"], "ONE system has --composites"),
    (["-t", "--trackfiles", "a", "b", "--batch-composites", "--gpus", "2"], "--batch-composites runs on one GPU"),
    (["-t", "--trackfiles", "a", "b", "--batch-composites", "--ingest", "device"], "--batch-composites prepares the data on the host"),
    (["-c", "--choose-systems", "2", "--batch-composites", "--device-ingest"],                 # (-c's own, earlier refusal)
     "-c --choose-systems / --choose-starts prepares the data on the host: --ingest device / --device-ingest is not supported"),
    (["-t", "--trackfiles", "a", "b", "--batch-composites", "--batch-chunk", "4"], "--batch-chunk streams the batch and never holds them"),
    (["-c", "--choose-systems", "2", "--batch-composites", "--batch-chunk", "4"], "--batch-chunk streams the batch and never holds them"),
    # the refusals of --composites for a batch stay word for word
    (["-t", "--trackfiles", "a", "b", "--composites"], "--composites follows ONE system: --trackfiles analyses a batch of tracks and has no composites "
                                                       "(run -t --trackfile FILE --composites for the track that matters)"),
    (["-c", "--choose-systems", "2", "--composites"], "--composites follows ONE system: -c --choose-systems / --choose-starts follows a batch and has no "
                                                      "composites (run -t --trackfile on a track it wrote, with --composites)"),
])
def test_cli_refusals(tmp_path, monkeypatch, flags, text):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", *flags])
    assert text in str(e.value)
    assert not os.path.exists(tmp_path / "LEC_Results")          # refused before anything was created


def test_tracks_on_two_longitude_axes_are_refused_and_only_the_log_is_left(tmp_path, monkeypatch, golden_dir):
    """Tracks on both sides of the +-180 meridian are two passes over the data and have no common ensemble.  The partition is known only
    once the file and the tracks have been read, so this refusal comes after the batch directory and its log exist: the log stays, no
    tree of a track is made."""
    import shutil
    import lorenzcycletoolkit
    from lorenzcycletoolkit_amd import batch
    os.makedirs(tmp_path / "inputs")
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_NCEP-R2"), tmp_path / "inputs" / "namelist")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(batch, "partition_by_origin", lambda args, trackfiles, *a, **k: [(0.0, [0]), (180.0, [1])])
    with pytest.raises(ValueError, match=r"--batch-composites: the tracks take two longitude axes \(-180..180: east; 0..360: west\).*run the two sets apart"):
        lorenzcycletoolkit.main(["nofile.nc", "-r", "-t", "--trackfiles", "east", "west", "--batch-composites"])
    assert os.listdir(tmp_path / "LEC_Results") == ["nofile_track_batch"]
    assert os.listdir(tmp_path / "LEC_Results" / "nofile_track_batch") == ["log.nofile"]


def test_a_track_that_changes_shape_is_refused_by_name_and_step():
    """``batch.composites_check``: ``frameworks.composites_check`` per track, on the track's own crop."""
    import pandas as pd
    from types import SimpleNamespace
    from lorenzcycletoolkit_amd import batch
    lat, lon = np.linspace(-60.0, -10.0, 21), np.linspace(-80.0, -20.0, 25)
    win = lambda self, la, lo: (la, lo)
    mk = lambda path, boxes: SimpleNamespace(path=path, boxes=boxes, window=lambda la, lo: (la, lo))
    good, small = mk("tracks/a", [(0, 6, 0, 4), (3, 9, 2, 6)]), mk("tracks/c", [(1, 5, 0, 2), (2, 6, 1, 3)])
    plan = SimpleNamespace(tracks=[good, small, mk("tracks/d", [(5, 11, 3, 7)])], lat=lat, lon=lon)
    assert batch.composites_check(plan) == {(5, 7): [0, 2], (3, 5): [1]}
    plan.tracks.append(mk("tracks/b", [(0, 6, 0, 4), (3, 9, 2, 6), (3, 10, 2, 6)]))
    with pytest.raises(batch.BatchRefusal, match=r"track file tracks/b: --batch-composites needs boxes of ONE shape: the box of step 2 has 5 x 8 "
                                                 r"points \(rows x columns\), that of step 0 has 5 x 7"):
        batch.composites_check(plan)
    plan.tracks[-1] = mk("tracks/e", [(0, 6, 0, 4)])
    plan.lon = np.sort(lon + 0.3 * np.sin(np.arange(25.0)))
    with pytest.raises(batch.BatchRefusal, match="track file tracks/a: --batch-composites needs evenly spaced longitudes"):
        batch.composites_check(plan)


def test_help_docstring_readme_and_design_name_the_flag(capsys):
    import lorenzcycletoolkit
    with pytest.raises(SystemExit):
        lorenzcycletoolkit.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--batch-composites" in text and "lec_composite_steps" in text and "composites.csv" in text
    assert "results_composites_<rows>x<columns>/" in text
    assert "--batch-composites" in lorenzcycletoolkit.__doc__
    assert "--batch-composites" in open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.2g" in design and "lec_composite_steps" in design and "lec_composite_ensemble" in design
