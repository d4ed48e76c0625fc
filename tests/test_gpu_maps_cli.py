"""-f [--periodic] --maps on the command line (GPU): the twelve files of results_maps/ against the CPU restatement
(tests/maps_restatement.py) at print precision, every other file of the run byte for byte what the run without --maps writes -- also
beside --sections and --wavenumbers --, a --series split in two with the same bytes, and the open box of the committed NCEP sample
whose Hovmoeller files reproduce the run's own results CSV under the box's zonal average (1e-9 of each term's scale)."""
import os
import shutil

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd.constants import MAP_TERMS
from oracle import lec_oracle as o
from tests import maps_restatement as mr
from tests import ring_restatement as rr
from tests import sections_restatement as sr

TOL = 1e-9
SOUTH, NORTH = -30.0, 30.0
FLAGS = ["-r", "-f", "--periodic"]
MAPS = os.path.join("ring_fixed", "results_maps")


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    (tmp_path / "inputs" / "namelist").write_text(rr.RING_NAMELIST)
    (tmp_path / "inputs" / "box_limits").write_text(f"min_lon;-180\nmax_lon;180\nmin_lat;{SOUTH}\nmax_lat;{NORTH}\n")
    monkeypatch.chdir(tmp_path)
    return tmp_path


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
    import io
    return pd.read_csv(io.BytesIO(blob), index_col=0, float_precision="round_trip")


def _maps_of(tree):
    return {k: v for k, v in tree.items() if k.startswith(MAPS + os.sep)}


def _same(one, two, what):
    assert sorted(one) == sorted(two), what
    for k in one:
        assert one[k] == two[k], f"{what}: {k} differs"


def _near(got, ref, what):
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max() / scale
    print(f"{what}: max error / scale = {err:.3e}")
    assert got.shape == ref.shape and err <= TOL, (what, err)


def test_ring_run_writes_the_maps(workdir):
    dom = rr.cli_domain()
    path = str(workdir / "ring.nc")
    rr.write_ring_file(path, dom)
    plain = _main([path] + FLAGS)
    got = _main([path] + FLAGS + ["--maps"])
    maps = _maps_of(got)
    names = [f"{t}_lat_lon.csv" for t in MAP_TERMS] + [f"{t}_lon.csv" for t in MAP_TERMS]
    assert sorted(maps) == sorted(os.path.join(MAPS, n) for n in names) and len(maps) == 12
    # every OTHER file of the run is what the run without --maps writes
    _same({k: v for k, v in got.items() if k not in maps}, plain, "the run's other files")

    # the numbers: the restatement on the same band
    with np.errstate(invalid="ignore"):
        b = rr.ring_box(dom, SOUTH, NORTH)
        C = mr.columns(mr.maps(b, True), b.level)
    M, H = mr.time_mean(C), mr.hovmoller(C, sr.area_weights(b))
    for i, term in enumerate(MAP_TERMS):
        m = _table(maps[os.path.join(MAPS, f"{term}_lat_lon.csv")])
        assert np.array_equal(np.asarray(m.index, dtype=float), b.lat) and np.array_equal([float(c) for c in m.columns], dom.lon)
        _near(m.values, M[i], term + "_lat_lon")
        h = _table(maps[os.path.join(MAPS, f"{term}_lon.csv")])
        assert h.index.name == "time" and len(h.index) == dom.time_s.size and str(h.index[1]) == "2020-01-01 06:00:00"
        assert np.array_equal([float(c) for c in h.columns], dom.lon)
        _near(h.values, H[:, i], term + "_lon")

    # beside --sections and --wavenumbers: the same maps, and the other files of that run unchanged
    more = ["--sections", "--wavenumbers", "4"]
    both = _main([path] + FLAGS + more + ["--maps"])
    _same(_maps_of(both), maps, "the maps beside --sections --wavenumbers")
    _same({k: v for k, v in both.items() if k not in maps}, _main([path] + FLAGS + more), "the other files beside --sections --wavenumbers")

    # ... and the series split in two files (2 + 2 steps) writes the same bytes
    os.makedirs(workdir / "parts")
    cut = lambda a, b_: o.Domain(dom.tair[a:b_], dom.u[a:b_], dom.v[a:b_], dom.omega[a:b_], dom.geopt[a:b_], dom.lat, dom.lon, dom.level,
                                 dom.time_s[a:b_])
    first, second = str(workdir / "parts" / "ring.nc"), str(workdir / "parts" / "ring_b.nc")
    rr.write_ring_file(first, cut(0, 2))
    rr.write_ring_file(second, cut(2, 4))
    _same(_maps_of(_main([first] + FLAGS + ["--maps", "--series", second])), maps, "--series")


def test_open_box_on_the_ncep_sample_closes_on_its_results(tmp_path, golden_dir, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_NCEP-R2"), tmp_path / "inputs" / "namelist")
    shutil.copy(os.path.join(golden_dir, "inputs", "box_limits_Reg1"), tmp_path / "inputs" / "box_limits")
    monkeypatch.chdir(tmp_path)
    tree = _main([os.path.join(golden_dir, "testdata_NCEP-R2.nc"), "-r", "-f", "--maps"])
    base = "testdata_NCEP-R2_fixed"
    maps = {os.path.basename(k): v for k, v in tree.items() if k.startswith(os.path.join(base, "results_maps") + os.sep)}
    assert sorted(maps) == sorted([f"{t}_lat_lon.csv" for t in MAP_TERMS] + [f"{t}_lon.csv" for t in MAP_TERMS])
    results = _table(tree[os.path.join(base, f"{base}_results.csv")])
    for term in MAP_TERMS:
        h = _table(maps[f"{term}_lon.csv"])                                                      # [time, lon]
        assert list(h.index) == list(results.index)
        rlon = np.deg2rad(np.array([float(c) for c in h.columns]))
        za = o.zonal_average(h.values, rlon, rlon[-1] - rlon[0])                                 # the open box's half-weight trapezoid
        _near(za, results[term].values, term + ": zonal average of the Hovmoeller against the results CSV")
