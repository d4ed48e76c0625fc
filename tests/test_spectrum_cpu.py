"""-f --periodic --wavenumbers without a GPU: the additive C call ``lec_rowspec_ring`` (export, header, ABI 11, struct layout, every
refusal before any HIP call), the host-built twiddle table, the command line's refusals, and the CPU restatement's own closure and
rotation invariance (tests/spectrum_restatement.py).

Bars of the restatement's own checks: the N = nx / 2 shares of a term sum to its total to 1e-12 of scale (a sum of at most 65 terms of
rounding error a few ulp of scale each; measured 3e-15), and a rotation of the ring moves no share by more than 1e-11 of scale (the
bar of the GPU test; measured 9e-15)."""
import ctypes
import os
import re

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib, tables
from tests import ring_restatement as rr
from tests import spectrum_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the C call -------------------------------------------------------------------------------------------------------------------
def test_rowspec_call_is_additive():
    lib = _lib.load()
    assert "lec_rowspec_ring" in _lib.EXPORTS and lib.lec_rowspec_ring is not None
    hdr = open(os.path.join(ROOT, "include", "lec_hip.h")).read()
    assert "int lec_rowspec_ring(const lec_rowspec_args* args);" in hdr
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11 and "#define LEC_ABI_VERSION 11" in hdr
    m = re.search(r"#define LEC_MAX_WAVENUMBERS (\d+)", hdr)
    assert m and int(m.group(1)) == _lib.LEC_MAX_WAVENUMBERS >= 64
    A = _lib.RowspecArgs
    assert ctypes.sizeof(A) == 4 * 8 + 10 * 4 + 3 * 8
    offs = {n: getattr(A, n).offset for n, _ in A._fields_}
    assert offs["tair_d"] == 0 and offs["dtype"] == 32 and offs["nx"] == 48 and offs["t_begin"] == 52 and offs["js"] == 60
    assert offs["n_wave"] == 68 and offs["twid_d"] == 72 and offs["spec_d"] == 80 and offs["stream"] == 88
    # the existing structs are what they were
    assert ctypes.sizeof(_lib.RowstatsArgs) == 6 * 8 + 14 * 4 + 9 * 8 + 8 * 4 + 2 * 8
    assert ctypes.sizeof(_lib.ReduceArgs) == 8 + 4 * 4 + 4 * 8 + 8 + 2 * 4 + 8 + 6 * 8 + 2 * 8


def _valid_args():
    """Scalars of a valid call over fake (never dereferenced) pointers: every refusal is made on the scalars, before any HIP call."""
    fake = ctypes.c_void_p(0x10000)
    a = _lib.RowspecArgs()
    a.tair_d = a.u_d = a.v_d = a.omega_d = a.twid_d = a.spec_d = fake
    a.dtype = _lib.LEC_F64
    a.nt, a.nl, a.ny, a.nx, a.t_begin, a.t_count = 3, 4, 5, 16, 0, 3
    a.js, a.jn, a.n_wave = 0, 4, 8
    return a


@pytest.mark.parametrize("field, change", [
    ("tair_d", lambda a: setattr(a, "tair_d", None)),
    ("u_d", lambda a: setattr(a, "u_d", None)),
    ("v_d", lambda a: setattr(a, "v_d", None)),
    ("omega_d", lambda a: setattr(a, "omega_d", None)),
    ("twid_d", lambda a: setattr(a, "twid_d", None)),
    ("spec_d", lambda a: setattr(a, "spec_d", None)),
    ("dtype", lambda a: setattr(a, "dtype", _lib.LEC_I16)),
    ("nx", lambda a: (setattr(a, "nx", 2), setattr(a, "n_wave", 1))),
    ("n_wave", lambda a: setattr(a, "n_wave", 0)),
    ("n_wave", lambda a: setattr(a, "n_wave", 9)),                   # nx / 2 = 8
    ("n_wave", lambda a: (setattr(a, "nx", 17), setattr(a, "n_wave", 9))),      # nx / 2 = 8 on an odd ring too
    ("js", lambda a: setattr(a, "js", -1)),
    ("js", lambda a: (setattr(a, "js", 5), setattr(a, "jn", 5))),
    ("jn", lambda a: setattr(a, "jn", 5)),
    ("jn", lambda a: (setattr(a, "js", 3), setattr(a, "jn", 2))),
    ("spec_d", lambda a: setattr(a, "spec_d", 0x10008)),
    ("twid_d", lambda a: setattr(a, "twid_d", 0x10008)),
    ("tair_d", lambda a: setattr(a, "tair_d", 0x10004)),
    ("t_begin", lambda a: setattr(a, "t_begin", -1)),
    ("t_begin", lambda a: setattr(a, "t_begin", 3)),
    ("t_count", lambda a: setattr(a, "t_count", 0)),
    ("t_count", lambda a: (setattr(a, "t_begin", 1), setattr(a, "t_count", 3))),
])
def test_c_call_refusals_name_the_field(field, change):
    lib = _lib.load()
    a = _valid_args()
    change(a)
    assert lib.lec_rowspec_ring(ctypes.byref(a)) == 1          # LEC_ERR_ARG
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_rowspec_ring") and field.encode() in msg, msg


def test_c_call_null_and_beyond_the_limit():
    lib = _lib.load()
    assert lib.lec_rowspec_ring(None) == 1 and b"null args" in lib.lec_last_error()
    a = _valid_args()
    a.nx, a.n_wave = 1440, _lib.LEC_MAX_WAVENUMBERS + 1
    assert lib.lec_rowspec_ring(ctypes.byref(a)) == 2          # LEC_ERR_UNSUPPORTED
    msg = lib.lec_last_error()
    assert b"lec_rowspec_ring" in msg and b"n_wave" in msg and b"LEC_MAX_WAVENUMBERS" in msg, msg


# -- the twiddle table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [3, 4, 17, 130, 1440])
def test_twiddle_table(nx):
    t = tables.twiddle_table(nx)
    ang = 2.0 * np.pi * np.arange(nx) / nx
    assert t.shape == (nx, 2) and t.dtype == np.float64 and t.flags["C_CONTIGUOUS"]
    assert np.array_equal(t[:, 0], np.cos(ang)) and np.array_equal(t[:, 1], np.sin(ang))
    assert t[0, 0] == 1.0 and t[0, 1] == 0.0
    with pytest.raises(ValueError):
        tables.twiddle_table(2)


# -- the restatement's own closure and rotation invariance ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dom():
    return rr.ring_domain(3, 5, 9, 16, seed=1)


@pytest.mark.parametrize("nx", [3, 4, 16, 17, 130])
def test_restatement_closes_on_the_totals(nx):
    d = rr.ring_domain(3, 5, 9, nx, seed=1)
    spec, rest, levels, tot = sr.spectrum_terms(d, -60, 60, nx // 2)
    assert spec.shape == (3, 5, nx // 2) and rest.shape == (3, 5) and levels.shape == (3, 14, nx // 2, 5)
    scale = np.abs(spec).max(axis=(0, 2))
    err = np.abs(rest).max(axis=0) / scale
    print(f"nx={nx}: closure {err.max():.2e} of scale")
    assert err.max() <= 1e-12, dict(zip(sr.TERMS, err))
    # the tables' pressure integrals are the scalars' own pieces: the shares of the per-level tables close on the ring's tables too
    _, lv = rr.ring_terms(d, -60, 60)
    for i, name in enumerate(sr.LEVEL_TERMS):
        if name == "Ce_1":
            continue                    # (a function of level alone: the same for every n)
        s = np.abs(levels[:, i]).max()
        assert np.abs(levels[:, i].sum(axis=1) - lv[name]).max() <= 1e-12 * s, name


def test_restatement_is_rotation_invariant(dom):
    spec, _, levels, _ = sr.spectrum_terms(dom, -60, 60, 8)
    spec2, _, levels2, _ = sr.spectrum_terms(rr.rolled(dom, 5), -60, 60, 8)
    err = np.abs(spec2 - spec).max(axis=(0, 2)) / np.abs(spec).max(axis=(0, 2))
    print(f"rotation by 5: {err.max():.2e} of scale")
    assert err.max() <= 1e-11
    lerr = np.abs(levels2 - levels).max(axis=(0, 2, 3)) / np.abs(levels).max(axis=(0, 2, 3))
    assert lerr.max() <= 1e-11


def test_row_shares_are_the_covariances(dom):
    """The NumPy form of the row records (``row_shares``) sums to the plain covariances of the rows."""
    f = [a[..., :] for a in (dom.tair, dom.u, dom.v, dom.omega)]
    sh = sr.row_shares(*f, 8).sum(axis=-2)
    dev = [a - a.mean(axis=-1, keepdims=True) for a in f]
    pairs = [(0, 0), (1, 1), (2, 2), (2, 0), (3, 0), (1, 2), (3, 1), (3, 2)]
    for s, (a, b) in enumerate(pairs):
        cov = (dev[a] * dev[b]).mean(axis=-1)
        assert np.abs(sh[..., s] - cov).max() <= 1e-12 * np.abs(cov).max(), s


# -- the command line -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags, text", [
    (["-f", "--wavenumbers", "4"], "--wavenumbers goes with -f --periodic"),
    (["-t", "--wavenumbers", "4"], "--wavenumbers goes with -f --periodic"),
    (["-f", "--periodic", "--wavenumbers", "0"], "--wavenumbers must be >= 1"),
    (["-f", "--periodic", "--wavenumbers", "-3"], "--wavenumbers must be >= 1"),
    (["-f", "--periodic", "--wavenumbers", "65"], "--wavenumbers must be <= 64"),
    (["-f", "--periodic", "--wavenumbers", "4", "--gpus", "2"], "--wavenumbers runs on one GPU"),
    (["-f", "--periodic", "--wavenumbers", "4", "--ingest", "device"], "--wavenumbers prepares the data on the host"),
    (["-f", "--periodic", "--wavenumbers", "4", "--device-ingest"], "--wavenumbers prepares the data on the host"),
])
def test_cli_refusals(tmp_path, monkeypatch, flags, text):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", *flags])
    assert text in str(e.value)
    assert not os.path.exists(tmp_path / "LEC_Results")          # refused before anything was created


def test_cli_refuses_more_wavenumbers_than_the_ring_holds(tmp_path, monkeypatch):
    """N > nx / 2 needs the file's longitudes: refused once they are read, before a result file is written or the GPU is touched."""
    import logging

    import lorenzcycletoolkit
    os.makedirs(tmp_path / "inputs")
    (tmp_path / "inputs" / "namelist").write_text(rr.RING_NAMELIST)
    (tmp_path / "inputs" / "box_limits").write_text("min_lon;-180\nmax_lon;180\nmin_lat;-30\nmax_lat;30\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(logging.getLogger("lorenzcycletoolkit"), "handlers", [])
    rr.write_ring_file(str(tmp_path / "ring.nc"), rr.cli_domain())          # 24 longitudes: wavenumbers 1 .. 12
    with pytest.raises(ValueError) as e:
        lorenzcycletoolkit.main([str(tmp_path / "ring.nc"), "-r", "-f", "--periodic", "--wavenumbers", "13"])
    assert "--wavenumbers 13" in str(e.value) and "1 .. 12" in str(e.value)
    results = tmp_path / "LEC_Results" / "ring_fixed"
    assert not os.path.isdir(results / "results_wavenumbers") and not os.path.isdir(results / "results_vertical_levels")
