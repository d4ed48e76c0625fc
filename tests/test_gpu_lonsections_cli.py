"""--lon-sections and --composite-lon-sections on the command line (GPU).  On a small ring file written by the test, ``-f --periodic
--lon-sections --maps --sections``: the six files of results_lon_sections/ against the CPU restatement
(tests/lonsections_restatement.py) at print precision (repr(float) round-trips; 1e-9 of each term's scale, the project's parity bar),
every other file byte for byte what the run without the flag writes.  On the committed NCEP sample: ``-f`` with its preset box and
``-t`` with its preset track beside ``--composites``: the new files exist with the expected shapes and labels and every other file keeps
its bytes.
Measured on MI355X: the six files against the restatement 5.7e-13 (the test prints each term's figure)."""
import io
import os
import shutil

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd.constants import MAP_TERMS
from tests import lonsections_restatement as lr
from tests import maps_restatement as mr
from tests import ring_restatement as rr
from tests import sections_restatement as sr

TOL = 1e-9
SOUTH, NORTH = -30.0, 30.0


def _tree():
    """{relative path: bytes} of everything under LEC_Results but the logs; the tree is removed."""
    out = {}
    for base, _, files in os.walk("LEC_Results"):
        for f in files:
            if not f.startswith("log."):
                out[os.path.relpath(os.path.join(base, f), "LEC_Results")] = open(os.path.join(base, f), "rb").read()
    shutil.rmtree("LEC_Results")
    return out


def _main(argv):
    import lorenzcycletoolkit
    lorenzcycletoolkit.main(argv)
    return _tree()


def _table(blob):
    return pd.read_csv(io.BytesIO(blob), index_col=0, float_precision="round_trip")


def _split(tree, directory):
    """(the files of ``directory`` by name, every other file by path)."""
    d = directory + os.sep
    return {os.path.basename(k): v for k, v in tree.items() if k.startswith(d)}, {k: v for k, v in tree.items() if not k.startswith(d)}


def _levels(tree, base):
    """The per-level table of Ae: its columns are the levels as the per-level tables label them."""
    key = next(k for k in sorted(tree) if k.startswith(os.path.join(base, "results_vertical_levels", "Ae_")))
    return pd.read_csv(io.BytesIO(tree[key]), index_col=0)


def _same(one, two, what):
    assert sorted(one) == sorted(two), what
    for k in one:
        assert one[k] == two[k], f"{what}: {k} differs"


def test_ring_run_writes_the_lon_sections(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    (tmp_path / "inputs" / "namelist").write_text(rr.RING_NAMELIST)
    (tmp_path / "inputs" / "box_limits").write_text(f"min_lon;-180\nmax_lon;180\nmin_lat;{SOUTH}\nmax_lat;{NORTH}\n")
    monkeypatch.chdir(tmp_path)
    dom = rr.cli_domain()
    path = str(tmp_path / "ring.nc")
    rr.write_ring_file(path, dom)
    flags = ["-r", "-f", "--periodic", "--maps", "--sections"]
    plain = _main([path] + flags)
    got, other = _split(_main([path] + flags + ["--lon-sections"]), os.path.join("ring_fixed", "results_lon_sections"))
    assert sorted(got) == sorted(f"{t}_lon_lv.csv" for t in MAP_TERMS) and len(got) == 6
    _same(other, plain, "the run's other files")
    with np.errstate(invalid="ignore"):
        b = rr.ring_box(dom, SOUTH, NORTH)
        M = lr.time_mean(lr.lon_sections(mr.maps(b, True), sr.area_weights(b)))
    lat_lv = _table(plain[os.path.join("ring_fixed", "results_sections", "Ae_lat_lv.csv")])
    for i, term in enumerate(MAP_TERMS):
        m = _table(got[f"{term}_lon_lv.csv"])
        assert m.index.name == lat_lv.index.name and list(m.index) == list(lat_lv.index)          # labelled as _lat_lv.csv
        assert np.array_equal(np.asarray(m.index, dtype=float), dom.level) and np.array_equal([float(c) for c in m.columns], dom.lon)
        err = np.abs(m.values - M[i]).max() / np.abs(M[i]).max()
        print(f"{term}_lon_lv: max error / scale = {err:.3e}")
        assert m.values.shape == M[i].shape and err <= TOL, (term, err)


def test_ncep_sample_fixed_box(tmp_path, golden_dir, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_NCEP-R2"), tmp_path / "inputs" / "namelist")
    shutil.copy(os.path.join(golden_dir, "inputs", "box_limits_Reg1"), tmp_path / "inputs" / "box_limits")
    monkeypatch.chdir(tmp_path)
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    base = "testdata_NCEP-R2_fixed"
    plain = _main([infile, "-r", "-f", "--maps"])
    got, other = _split(_main([infile, "-r", "-f", "--maps", "--lon-sections"]), os.path.join(base, "results_lon_sections"))
    assert sorted(got) == sorted(f"{t}_lon_lv.csv" for t in MAP_TERMS)
    _same(other, plain, "the run's other files")
    hov = _table(plain[os.path.join(base, "results_maps", "Ae_lon.csv")])
    levels = _levels(plain, base)
    for term in MAP_TERMS:
        m = _table(got[f"{term}_lon_lv.csv"])
        assert list(m.columns) == list(hov.columns)                       # the box's longitudes in degrees, as the maps print them
        assert [float(p) for p in m.index] == [float(c) for c in levels.columns] and m.shape == (len(levels.columns), len(hov.columns))
        assert np.isfinite(m.values).all()


def test_ncep_sample_track(tmp_path, golden_dir, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_NCEP-R2"), tmp_path / "inputs" / "namelist")
    shutil.copy(os.path.join(golden_dir, "inputs", "track_testdata_NCEP-R2"), tmp_path / "inputs" / "track")
    monkeypatch.chdir(tmp_path)
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    base = "testdata_NCEP-R2_track"
    plain = _main([infile, "-r", "-t", "--composites"])
    got, other = _split(_main([infile, "-r", "-t", "--composite-lon-sections", "--composites"]),
                        os.path.join(base, "results_composite_lon_sections"))
    assert sorted(got) == sorted(f"{t}_dlon_lv.csv" for t in MAP_TERMS)
    _same(other, plain, "the run's other files")
    levels = _levels(plain, base)
    offs = [-7.5, -5.0, -2.5, 0.0, 2.5, 5.0, 7.5]
    for term in MAP_TERMS:
        m = _table(got[f"{term}_dlon_lv.csv"])
        assert [float(c) for c in m.columns] == offs and [float(p) for p in m.index] == [float(c) for c in levels.columns]
        assert m.shape == (len(levels.columns), 7) and np.isfinite(m.values).all()
