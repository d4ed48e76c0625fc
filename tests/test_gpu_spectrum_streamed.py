"""The zonal-wavenumber spectra of a streamed series: ``ingest.lec_streamed(..., ring=True, wavenumbers=N)`` computes them chunk by
chunk (``rowspec`` / ``rowspec_q`` beside the ring pass, ``lec_level_spec_ring`` into one levraw buffer of the series) and gives, bit
for bit, what the resident ``LECEngine.compute`` gives on the same domain with its assembled records; the command line's
--wavenumbers-chunk writes the bytes of the host run, over one file and over the file split in two (--series).

Five steps in chunks of one and two: T's halo for Ge's dT/dt crosses chunk edges.  4 levels x 5 latitudes (the small form of stage 2)
and x 70 (the general form); rings of 24 and 130 longitudes; fp64 and fp32 storage."""
import argparse
import os
import shutil

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import dataset as ds
from lorenzcycletoolkit_amd import ingest
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests import series_cases as sc

DEV = "cuda:0"
NT, NL = 5, 4
SOUTH, NORTH = -60.0, 60.0
RESULT_FIELDS = ("scalars", "levels", "spectrum", "spectrum_rest", "spectrum_levels", "spectrum_ge", "spectrum_ge_rest", "spectrum_ge_levels")

_resident = {}


def _dom(ny, nx, dtype, nan=False):
    dom = rr.ring_domain(NT, NL, ny, nx, seed=nx + ny, dtype=dtype, lat0=SOUTH, lat1=NORTH)
    if nan:
        for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt):
            a[:, NL - 1, 1:3, 2:4] = np.nan
    return dom


def _same_bits(a, b):
    if a.dtype == torch.int32:
        return torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _compute_resident(key, dom, n):
    """The resident call (assembled records) of one case, computed once and shared."""
    if key not in _resident:
        eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
        pb = eng.prepare_boxes([(0, dom.lon.size - 1, 0, dom.lat.size - 1)], ring=True)
        _resident[key] = eng.compute(*[_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)], pb, time_s=dom.time_s,
                                     wavenumbers=n, spectrum_generation=True)
    return _resident[key]


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    (tmp_path / "inputs" / "namelist").write_text(rr.RING_NAMELIST)
    (tmp_path / "inputs" / "box_limits").write_text(f"min_lon;-180\nmax_lon;180\nmin_lat;{SOUTH}\nmax_lat;{NORTH}\n")
    monkeypatch.chdir(tmp_path)
    return tmp_path


def _streamed(workdir, dom, n, chunk_steps, **kw):
    path = str(workdir / "ring.nc")
    rr.write_ring_file(path, dom)
    df = ds.read_namelist("inputs/namelist")
    raw = ds.open_raw(path, df)
    try:
        plan = ingest.make_plan(raw, argparse.Namespace(fixed=True, track=False, trackfile=None, residuals=True))
        assert np.array_equal(plan.lon, dom.lon) and np.array_equal(plan.lat, dom.lat) and np.array_equal(plan.level, dom.level)
        stats = {}
        res = ingest.lec_streamed(raw, plan, df, [(-180.0, 180.0, SOUTH, NORTH)], device=DEV, chunk_steps=chunk_steps, stats=stats, ring=True,
                                  wavenumbers=n, **kw)
        torch.cuda.synchronize()
    finally:
        raw.close()
    return res, stats


def _assert_same(st, whole, what):
    for name in RESULT_FIELDS:
        assert _same_bits(getattr(st, name), getattr(whole, name)), f"{what}: {name} differs from the resident call"
    assert torch.equal(st.nanflag, whole.nanflag), what


CASES = [(5, 24, 4, np.float64, 1), (5, 24, 4, np.float64, 2), (5, 130, 20, np.float64, 1), (5, 130, 20, np.float64, 2),
         (70, 24, 4, np.float64, 2), (5, 24, 4, np.float32, 2)]


@pytest.mark.parametrize("ny, nx, n, dtype, chunk_steps", CASES, ids=[f"ny{c[0]}-nx{c[1]}-N{c[2]}-{np.dtype(c[3]).name}-chunks-of-{c[4]}" for c in CASES])
def test_streamed_equals_resident(ny, nx, n, dtype, chunk_steps, workdir, monkeypatch):
    dom = _dom(ny, nx, dtype)
    whole = _compute_resident((ny, nx, n, np.dtype(dtype).name), dom, n)
    st, stats = _streamed(workdir, dom, n, chunk_steps, spectrum_generation=True)
    assert stats["chunks"] >= 2 and stats["chunk_steps"] == chunk_steps
    assert stats["spectrum_levraw_bytes"] == n * NT * NL * 320
    assert stats["spectrum_buffer_bytes"] == chunk_steps * NL * ny * n * (64 + 8)
    _assert_same(st, whole, f"chunks of {chunk_steps}")
    # the spectral records of ONE step at a time: a sub-chunk of two steps runs its spectral calls in pieces
    monkeypatch.setattr(LECEngine, "SPECTRUM_CHUNK_BYTES", 1)
    st, stats = _streamed(workdir, dom, n, chunk_steps, spectrum_generation=True)
    assert stats["spectrum_buffer_bytes"] == NL * ny * n * (64 + 8)
    _assert_same(st, whole, f"chunks of {chunk_steps}, spectral records of one step")


def test_streamed_without_generation(workdir):
    dom = _dom(5, 24, np.float64)
    whole = _compute_resident((5, 24, 4, "float64"), dom, 4)
    st, stats = _streamed(workdir, dom, 4, 2)
    assert st.spectrum_ge is None and st.spectrum_ge_rest is None and st.spectrum_ge_levels is None
    assert stats["spectrum_buffer_bytes"] == 2 * NL * 5 * 4 * 64
    for name in ("scalars", "levels", "spectrum", "spectrum_rest", "spectrum_levels"):
        assert _same_bits(getattr(st, name), getattr(whole, name)), name


@pytest.mark.parametrize("ny", [5, 70])
def test_streamed_nan_level(ny, workdir):
    """NaN at the bottom level: dropped from every step's integrals, for the totals and for every (n, t) of the spectra."""
    dom = _dom(ny, 24, np.float64, nan=True)
    whole = _compute_resident((ny, 24, 4, "float64", "nan"), dom, 4)
    st, _ = _streamed(workdir, dom, 4, 2, spectrum_generation=True)
    assert int(whole.nanflag.sum()) > 0
    _assert_same(st, whole, "NaN at the bottom level")


def test_streamed_refusals(workdir):
    """Said before anything is allocated (the file is not even read)."""
    kw = dict(device=DEV, wavenumbers=4)
    lim = [(-180.0, 180.0, SOUTH, NORTH)]
    for bad, text in ((dict(ring=False), "ring"), (dict(per_step_boxes=True), "per_step_boxes"),
                      (dict(ring=True, t_range=(0, 2)), "t_range"), (dict(ring=True, merge_dropmask=lambda m: None), "merge_dropmask"),
                      (dict(ring=True, out=torch.empty(1)), "out"), (dict(ring=True, spectrum_generation=True, with_q=False), "with_q")):
        with pytest.raises(ValueError) as e:
            ingest.lec_streamed(None, None, None, lim, **kw, **bad)
        assert text in str(e.value), (bad, str(e.value))
    with pytest.raises(ValueError):
        ingest.lec_streamed(None, None, None, lim, device=DEV, ring=True, spectrum_generation=True)


# -- the command line -------------------------------------------------------------------------------------------------------------
def _tree():
    """({relative path: bytes} of everything under LEC_Results but the logs, the logs); the tree is removed."""
    out = {}
    for base, _, files in os.walk("LEC_Results"):
        for f in files:
            if not f.startswith("log."):
                out[os.path.relpath(os.path.join(base, f), "LEC_Results")] = open(os.path.join(base, f), "rb").read()
    logs = "".join(open(os.path.join(base, f)).read() for base, _, files in os.walk("LEC_Results") for f in files if f.startswith("log."))
    shutil.rmtree("LEC_Results")
    return out, logs


def _main(argv):
    import lorenzcycletoolkit
    lorenzcycletoolkit.main(argv)
    return _tree()


def _same(one, two, what):
    assert sorted(one) == sorted(two), what
    for k in one:
        assert one[k] == two[k], f"{what}: {k} differs from the host run's"


SPECTRA = ["-r", "-f", "--periodic", "--wavenumbers", "4", "--wavenumbers-generation"]


def test_cli_wavenumbers_chunk(workdir):
    (workdir / "inputs" / "box_limits").write_text("min_lon;-180\nmax_lon;180\nmin_lat;-30\nmax_lat;30\n")
    path = str(workdir / "ring.nc")
    rr.write_ring_file(path, rr.cli_domain())
    want, log = _main([path] + SPECTRA)
    assert "--ingest auto resolves to host" in log and "lec_level_spec_ring" not in log
    assert len([k for k in want if k.startswith(os.path.join("ring_fixed", "results_wavenumbers"))]) == 6
    for extra in ([], ["--ingest", "device"], ["--device-ingest"]):
        got, log = _main([path] + SPECTRA + ["--wavenumbers-chunk", "2"] + extra)
        _same(want, got, "--wavenumbers-chunk 2 " + " ".join(extra))
        assert "lec_level_spec_ring" in log and "--wavenumbers-chunk 2" in log and "resolves to host" not in log
    with pytest.raises(SystemExit) as e:
        _main([path, "-r", "-f", "--periodic", "--wavenumbers-chunk", "2"])
    assert "--wavenumbers-chunk goes with --wavenumbers" in str(e.value) and not os.path.exists("LEC_Results")


def test_cli_wavenumbers_chunk_over_a_series(tmp_path, monkeypatch):
    """The file split in two (4 + 3 steps, each part packed with its own constants): the bytes of the host run over the merged file."""
    cuts = (4, 3)
    parts, packed = sc.write_series(tmp_path / "parts", cuts=cuts)
    merged = str(tmp_path / "merged" / os.path.basename(parts[0]))
    sc.write_merged(merged, packed, cuts=cuts)
    os.makedirs(tmp_path / "inputs")
    (tmp_path / "inputs" / "namelist").write_text(sc.NAMELIST)
    (tmp_path / "inputs" / "box_limits").write_text("min_lon;-180\nmax_lon;180\nmin_lat;-45\nmax_lat;30\n")
    monkeypatch.chdir(tmp_path)
    want, _ = _main([merged] + SPECTRA)
    got, log = _main([parts[0]] + SPECTRA + ["--wavenumbers-chunk", "2", "--series", parts[1]])
    _same(want, got, "--wavenumbers-chunk 2 --series")
    assert len([k for k in got if "results_wavenumbers" in k]) == 6 and "lec_level_spec_ring" in log
