"""-t / -c --composite-sections on the command line (GPU): the twenty files of results_composite_sections/ on the committed NCEP sample
with its preset track against the API's result (``BoxData(composite_sections=True)`` on the same host-prepared data; the files print
repr(float), which round-trips: the same numbers) and, under every step's row weights, against the run's own results CSV (1e-9 of each
term's scale, the project's parity bar); the streamed route (--ingest device) writes the same files byte for byte; -c --choose-start
writes them too; every other file of either run is byte for byte what the run without --composite-sections writes.
Measured on MI355X (each test prints its own figure): the files equal the API's numbers (error 0); sum_j cw_j(t) of the column files
against the results CSV at most 8.0e-16 (Ck); the streamed route's twenty files are the host route's byte for byte (error 0), as the two
routes' results CSVs are for this sample."""
import io
import os
import shutil

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd.constants import SECTION_TERMS

TOL = 1e-9
NAMES = [f"{t}_dlat_lv.csv" for t in SECTION_TERMS] + [f"{t}_dlat.csv" for t in SECTION_TERMS]
OFFS = [-7.5, -5.0, -2.5, 0.0, 2.5, 5.0, 7.5]


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
    """(the system-relative sections' files by name, every other file by path)."""
    d = os.path.join(base, "results_composite_sections") + os.sep
    return {os.path.basename(k): v for k, v in tree.items() if k.startswith(d)}, {k: v for k, v in tree.items() if not k.startswith(d)}


def _same_other_files(other, plain):
    assert sorted(other) == sorted(plain)
    for k in plain:
        assert other[k] == plain[k], f"{k} differs from the run without --composite-sections"


def _host_data(infile):
    """(host-prepared data, namelist, args, the track's limits per step) as the command line prepares them for -t."""
    import argparse
    from lorenzcycletoolkit_amd import dataset as ds
    from lorenzcycletoolkit_amd.frameworks import get_limits
    args = argparse.Namespace(fixed=False, track=True, trackfile="inputs/track", residuals=True)
    df = ds.read_namelist("inputs/namelist")
    host = ds.slice_domain(ds.process_data(ds.open_dataset(infile, df), args, df), args, df)
    track = ds.track_on_axis(ds.read_track("inputs/track"), host.lon)
    lims = [get_limits(track, t) for t in pd.DatetimeIndex(host.time)]
    return host, df, args, [(l["min_lon"], l["max_lon"], l["min_lat"], l["max_lat"]) for l in lims]


def test_track_run_writes_the_sections(workdir, golden_dir):
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    base = "testdata_NCEP-R2_track"
    plain = _main([infile, "-r", "-t"])
    sec, other = _split(_main([infile, "-r", "-t", "--composite-sections"]), base)
    assert sorted(sec) == sorted(NAMES) and len(sec) == 20
    _same_other_files(other, plain)

    from lorenzcycletoolkit_amd.frameworks import BoxData
    from lorenzcycletoolkit_amd.tables import build_box_tables
    host, df, args, limits = _host_data(infile)
    api = BoxData(host, df, args=args, boxes_limits=limits, composite_sections=True)
    M, L = api.composite_section_mean, api.composite_section_lat
    nl = len(host.level)
    assert M.shape == (10, nl, 7) and L.shape == (5, 10, 7) and api.result.composite_section_steps is None
    assert list(api.composite_section_dlat) == OFFS
    results = _table(other[os.path.join(base, f"{base}_results.csv")])
    cw = np.asarray(build_box_tables(host.lat, host.lon, api.boxes).lattab2)[:, :7, 0]            # [T, 7]: every step's own row weights
    for i, term in enumerate(SECTION_TERMS):
        m = _table(sec[f"{term}_dlat_lv.csv"])
        assert list(m.index) == [float(p) for p in host.level] and [float(c) for c in m.columns] == OFFS
        h = _table(sec[f"{term}_dlat.csv"])
        assert len(h.index) == 5 and str(h.index[1]) == "2005-08-08 06:00:00" and [float(c) for c in h.columns] == OFFS
        for got, ref, what in ((m.values, M[i], term + "_dlat_lv"), (h.values, L[:, i], term + "_dlat")):
            err = np.nanmax(np.abs(got - ref)) / np.nanmax(np.abs(ref))
            print(f"{what}: the file against the API's result: max error / scale = {err:.3e}")
            assert np.array_equal(got, ref, equal_nan=True), what         # repr(float) round-trips: the printed precision is the number
        ref = results[term].values
        err = np.abs((h.values * cw).sum(axis=-1) - ref).max() / np.abs(ref).max()
        print(f"{term}: sum_j cw_j(t) of the column file against the results CSV: {err:.3e}")
        assert err <= TOL, (term, err)


def test_streamed_run_writes_the_same_files(workdir, golden_dir):
    """--ingest device against the host route: the files of results_composite_sections/ byte for byte (both routes hand stage 1 the same
    box-packed series, and the call reads nothing but its row records)."""
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    base = "testdata_NCEP-R2_track"
    host_sec, host_other = _split(_main([infile, "-r", "-t", "--ingest", "host", "--composite-sections"]), base)
    plain = _main([infile, "-r", "-t", "--ingest", "device"])
    dev_sec, dev_other = _split(_main([infile, "-r", "-t", "--ingest", "device", "--composite-sections"]), base)
    assert sorted(dev_sec) == sorted(NAMES) == sorted(host_sec)
    _same_other_files(dev_other, plain)
    key = os.path.join(base, f"{base}_results.csv")
    print(f"results CSV of the two routes byte-identical: {dev_other[key] == host_other[key]}")
    for name in NAMES:
        a, b = _table(host_sec[name]).values, _table(dev_sec[name]).values
        err = np.nanmax(np.abs(a - b)) / np.nanmax(np.abs(a))
        print(f"{name}: the streamed route against the host route: max error / scale = {err:.3e}")
    for name in NAMES:
        assert dev_sec[name] == host_sec[name], f"{name}: the streamed route's file differs from the host route's"


def test_choose_run_writes_the_sections(workdir, golden_dir):
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    base = "testdata_NCEP-R2_choose"
    flags = ["-r", "-c", "--choose-start", "-22.5", "-45"]
    plain = _main([infile] + flags)
    sec, other = _split(_main([infile] + flags + ["--composite-sections"]), base)
    assert sorted(sec) == sorted(NAMES) and len(sec) == 20
    _same_other_files(other, plain)
    m = _table(sec["Ae_dlat_lv.csv"])
    assert m.shape[1] == 7 and [float(c) for c in m.columns] == OFFS and m.index.name is not None and np.isfinite(m.values).all()
    h = _table(sec["Ae_dlat.csv"])
    assert h.shape[1] == 7 and [float(c) for c in h.columns] == OFFS and np.isfinite(h.values).all()
