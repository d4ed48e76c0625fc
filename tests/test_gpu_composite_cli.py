"""-t / -c --composites on the command line (GPU): the twelve files of results_composites/ on the committed NCEP sample with its preset
track against the API's result (``BoxData(composites=True)`` on the same host-prepared data, both of its host routes; the files print
repr(float), which round-trips: the same numbers) and against the run's results CSV under the box's zonal average (1e-9 of each term's
scale, the project's parity bar); -c --choose-start writes them too; every other file of either run is byte for byte what the run
without --composites writes.
Measured on MI355X: the files equal the API's numbers (error 0); the unpacked route against the packed one 4.6e-16 for the five terms
without Q and 3.2e-8 for Ge; the Hovmoeller files against the results CSV 4.6e-16 (each test prints its own figure)."""
import io
import os
import shutil

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd.constants import MAP_TERMS
from oracle import lec_oracle as o

TOL = 1e-9
NAMES = [f"{t}_dlat_dlon.csv" for t in MAP_TERMS] + [f"{t}_dlon.csv" for t in MAP_TERMS]


@pytest.fixture
def workdir(tmp_path, golden_dir, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_NCEP-R2"), tmp_path / "inputs" / "namelist")
    shutil.copy(os.path.join(golden_dir, "inputs", "track_testdata_NCEP-R2"), tmp_path / "inputs" / "track")
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
    return pd.read_csv(io.BytesIO(blob), index_col=0, float_precision="round_trip")


def _split(tree, base):
    """(the composites' files by name, every other file by path)."""
    d = os.path.join(base, "results_composites") + os.sep
    return {os.path.basename(k): v for k, v in tree.items() if k.startswith(d)}, {k: v for k, v in tree.items() if not k.startswith(d)}


def _closes_on_results(comp, results, what):
    """The box's zonal average (the open box's half-weight trapezoid, over the offsets) of every Hovmoeller file is the results CSV."""
    for term in MAP_TERMS:
        h = _table(comp[f"{term}_dlon.csv"])
        assert list(h.index) == list(results.index)
        rl = np.deg2rad(np.array([float(c) for c in h.columns]))
        za = o.zonal_average(h.values, rl, rl[-1] - rl[0])
        ref = results[term].values
        err = np.abs(za - ref).max() / np.abs(ref).max()
        print(f"{what} {term}: zonal average of the Hovmoeller against the results CSV: {err:.3e}")
        assert err <= TOL, (what, term, err)


def test_track_run_writes_the_composites(workdir, golden_dir):
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    base = "testdata_NCEP-R2_track"
    plain = _main([infile, "-r", "-t"])
    comp, other = _split(_main([infile, "-r", "-t", "--composites"]), base)
    assert sorted(comp) == sorted(NAMES) and len(comp) == 12
    assert sorted(other) == sorted(plain)
    for k in plain:
        assert other[k] == plain[k], f"{k} differs from the run without --composites"

    # the API's result on the same host-prepared data: BoxData(composites=True), whose two host routes are the box-packed series
    # (no dTdt array: fp32 storage hands over tm / tp) and the unpacked crop (a dTdt array)
    import argparse
    from lorenzcycletoolkit_amd import dataset as ds
    from lorenzcycletoolkit_amd.frameworks import BoxData, get_limits, host_fields
    args = argparse.Namespace(fixed=False, track=True, trackfile="inputs/track", residuals=True)
    df = ds.read_namelist("inputs/namelist")
    host = ds.slice_domain(ds.process_data(ds.open_dataset(infile, df), args, df), args, df)
    track = ds.track_on_axis(ds.read_track("inputs/track"), host.lon)
    lims = [get_limits(track, t) for t in pd.DatetimeIndex(host.time)]
    limits = [(l["min_lon"], l["max_lon"], l["min_lat"], l["max_lat"]) for l in lims]
    api = BoxData(host, df, args=args, boxes_limits=limits, composites=True)
    M, H = api.composite_mean, api.composite_lon
    assert M.shape == (6, 7, 7) and H.shape == (5, 6, 7) and api.result.composite_steps is None
    # the unpacked route: the same series with dT/dt handed over as an array (np.gradient over the track's times; the fields' fp32
    # storage rounds it to fp32, so Ge agrees to that rounding only -- 2^-24 of dT/dt, which Q' may amplify by the cancellation of its
    # terms: 1e-4 of Ge's scale is asked; the five terms without Q read the same records and agree to fp64 rounding)
    T = np.asarray(host_fields(host, df)[0][0], dtype=np.float64)
    unpacked = BoxData(host, df, args=args, boxes_limits=limits, composites=True, dTdt=np.gradient(T, host.time_s, axis=0))
    for i, term in enumerate(MAP_TERMS):
        for got, ref, what in ((unpacked.composite_mean[i], M[i], "mean"), (unpacked.composite_lon[:, i], H[:, i], "lon")):
            err = np.abs(got - ref).max() / np.abs(ref).max()
            print(f"{term} composite_{what}: the unpacked route against the packed route: max error / scale = {err:.3e}")
            assert err <= (1e-4 if term == "Ge" else 1e-12), (term, what, err)
    offs = [-7.5, -5.0, -2.5, 0.0, 2.5, 5.0, 7.5]
    for i, term in enumerate(MAP_TERMS):
        m = _table(comp[f"{term}_dlat_dlon.csv"])
        assert m.index.name == "dlat" and list(m.index) == offs and [float(c) for c in m.columns] == offs
        h = _table(comp[f"{term}_dlon.csv"])
        assert len(h.index) == 5 and str(h.index[1]) == "2005-08-08 06:00:00" and [float(c) for c in h.columns] == offs
        for got, ref, what in ((m.values, M[i], term + "_dlat_dlon"), (h.values, H[:, i], term + "_dlon")):
            err = np.abs(got - ref).max() / np.abs(ref).max()
            print(f"{what}: the file against the API's result: max error / scale = {err:.3e}")
            assert np.array_equal(got, ref), what                     # repr(float) round-trips: the printed precision is the number
    _closes_on_results(comp, _table(other[os.path.join(base, f"{base}_results.csv")]), "-t")


def test_choose_run_writes_the_composites(workdir, golden_dir):
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    base = "testdata_NCEP-R2_choose"
    flags = ["-r", "-c", "--choose-start", "-22.5", "-45"]
    plain = _main([infile] + flags)
    comp, other = _split(_main([infile] + flags + ["--composites"]), base)
    assert sorted(comp) == sorted(NAMES) and len(comp) == 12
    assert sorted(other) == sorted(plain)
    for k in plain:
        assert other[k] == plain[k], f"{k} differs from the run without --composites"
    m = _table(comp["Ae_dlat_dlon.csv"])
    assert m.shape == (7, 7) and np.isfinite(m.values).all()
    _closes_on_results(comp, _table(other[os.path.join(base, f"{base}_results.csv")]), "-c")
