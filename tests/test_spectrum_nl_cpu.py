"""-f --periodic --wavenumbers N --wavenumbers-interactions without a GPU: the additive C call ``lec_rowspec_nl_ring`` (export, header, ABI
11, struct layout, every refusal before any HIP call), its two host tables, the command line's, the framework's and the engine's
refusals, ``write_spectrum_csvs`` on a hand-made result, and the CPU restatement's own identities (tests/spectrum_nl_restatement.py).

Bars of the restatement's own checks, on grids of 3 steps x 4 levels x 5 latitudes.  Closure: the N = nx / 2 shares of a row sum to the
physical-space covariance, and S(n), L(n) to their totals, to 1e-12 of the largest share (a sum of at most 64 terms with a rounding
error of a few ulp of scale each; measured: rows 1.8e-15, terms 2.2e-14 at worst over nx = 8, 65, 128, 129).  A single wavenumber: the
advection of a wave of wavenumber m by a wave of wavenumber m holds the wavenumbers 0 and 2 m only, so every share vanishes: at most
1e-12 of max|A| max|x'| (measured 7.6e-15).  The two routes through the energy operator: the polarised one subtracts two energies of
the size of max|c a| max|b| to get a covariance that is a small part of it, so it is judged against that size, max over n of the
energies it subtracts: 1e-12 (measured 1.3e-16); against the largest share itself it reaches 2.6e-15, in the tables 8.4e-16 (bar 1e-11)."""
import ctypes
import os

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib, tables
from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests import spectrum_nl_restatement as nr
from tests.spectrum_restatement import wave_part

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the C call -------------------------------------------------------------------------------------------------------------------
def test_rowspec_nl_call_is_additive():
    lib = _lib.load()
    assert "lec_rowspec_nl_ring" in _lib.EXPORTS and lib.lec_rowspec_nl_ring is not None
    hdr = open(os.path.join(ROOT, "include", "lec_hip.h")).read()
    assert "int lec_rowspec_nl_ring(const lec_rowspec_nl_args* args);" in hdr
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11 and "#define LEC_ABI_VERSION 11" in hdr
    A = _lib.RowspecNlArgs
    assert ctypes.sizeof(A) == 4 * 8 + 10 * 4 + 8 * 8
    offs = {n: getattr(A, n).offset for n, _ in A._fields_}
    assert offs["tair_d"] == 0 and offs["dtype"] == 32 and offs["nx"] == 48 and offs["n_wave"] == 68 and offs["rows_d"] == 72
    assert offs["twid_d"] == 80 and offs["lattab_d"] == 88 and offs["ptab_d"] == 96 and offs["inv_hdeg"] == 104
    assert offs["nlspec_d"] == 112 and offs["nltot_d"] == 120 and offs["stream"] == 128
    # the sibling calls' structs are what they were
    assert ctypes.sizeof(_lib.RowspecArgs) == 4 * 8 + 10 * 4 + 3 * 8 and ctypes.sizeof(_lib.RowspecQArgs) == 4 * 8 + 10 * 4 + 7 * 8


POINTERS = ["tair_d", "u_d", "v_d", "omega_d", "rows_d", "twid_d", "lattab_d", "ptab_d", "nlspec_d", "nltot_d"]


def _valid_args():
    """Scalars of a valid call over fake (never dereferenced) pointers: every refusal is made on the scalars, before any HIP call."""
    a = _lib.RowspecNlArgs()
    for name in POINTERS:
        setattr(a, name, 0x10000)
    a.dtype = _lib.LEC_F64
    a.nt, a.nl, a.ny, a.nx, a.t_begin, a.t_count = 3, 4, 5, 16, 0, 3
    a.js, a.jn, a.n_wave = 0, 4, 8
    a.inv_hdeg = 16 / 360.0
    return a


@pytest.mark.parametrize("field, change", [(name, lambda a, name=name: setattr(a, name, None)) for name in POINTERS] + [
    ("dtype", lambda a: setattr(a, "dtype", _lib.LEC_I16)),
    ("nx", lambda a: (setattr(a, "nx", 2), setattr(a, "n_wave", 1))),
    ("nl", lambda a: setattr(a, "nl", 0)),
    ("ny", lambda a: (setattr(a, "ny", 1), setattr(a, "js", 0), setattr(a, "jn", 0))),
    ("n_wave", lambda a: setattr(a, "n_wave", 0)),
    ("n_wave", lambda a: setattr(a, "n_wave", 9)),                   # nx / 2 = 8
    ("n_wave", lambda a: (setattr(a, "nx", 17), setattr(a, "n_wave", 9))),      # nx / 2 = 8 on an odd ring too
    ("js", lambda a: setattr(a, "js", -1)),
    ("js", lambda a: (setattr(a, "js", 5), setattr(a, "jn", 5))),
    ("jn", lambda a: setattr(a, "jn", 5)),
    ("jn", lambda a: (setattr(a, "js", 3), setattr(a, "jn", 2))),
    ("jn", lambda a: (setattr(a, "js", 2), setattr(a, "jn", 2))),     # one row: no d/dlat
    ("nlspec_d", lambda a: setattr(a, "nlspec_d", 0x10008)),
    ("nltot_d", lambda a: setattr(a, "nltot_d", 0x10008)),
    ("rows_d", lambda a: setattr(a, "rows_d", 0x10008)),
    ("twid_d", lambda a: setattr(a, "twid_d", 0x10008)),
    ("lattab_d", lambda a: setattr(a, "lattab_d", 0x10004)),
    ("ptab_d", lambda a: setattr(a, "ptab_d", 0x10004)),
    ("tair_d", lambda a: setattr(a, "tair_d", 0x10004)),
    ("omega_d", lambda a: (setattr(a, "dtype", _lib.LEC_F32), setattr(a, "omega_d", 0x10002))),
    ("t_begin", lambda a: setattr(a, "t_begin", -1)),
    ("t_begin", lambda a: setattr(a, "t_begin", 3)),
    ("t_count", lambda a: setattr(a, "t_count", 0)),
    ("t_count", lambda a: (setattr(a, "t_begin", 1), setattr(a, "t_count", 3))),
])
def test_c_call_refusals_name_the_field(field, change):
    lib = _lib.load()
    a = _valid_args()
    change(a)
    assert lib.lec_rowspec_nl_ring(ctypes.byref(a)) == 1          # LEC_ERR_ARG
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_rowspec_nl_ring") and field.encode() in msg, msg


def test_c_call_null_and_beyond_the_limits():
    lib = _lib.load()
    assert lib.lec_rowspec_nl_ring(None) == 1 and b"null args" in lib.lec_last_error()
    a = _valid_args()
    a.nx, a.n_wave = 1440, _lib.LEC_MAX_WAVENUMBERS + 1
    assert lib.lec_rowspec_nl_ring(ctypes.byref(a)) == 2          # LEC_ERR_UNSUPPORTED
    msg = lib.lec_last_error()
    assert b"lec_rowspec_nl_ring" in msg and b"n_wave" in msg and b"LEC_MAX_WAVENUMBERS" in msg, msg
    a = _valid_args()
    a.nt = a.t_count = 60000
    a.nl, a.ny, a.jn = 200, 200, 199                             # 2.4e9 rows
    assert lib.lec_rowspec_nl_ring(ctypes.byref(a)) == 2
    assert b"rows" in lib.lec_last_error()


# -- the host tables --------------------------------------------------------------------------------------------------------------
def test_pressure_coefs_are_np_gradient():
    p = np.array([20000.0, 30000.0, 50000.0, 85000.0, 100000.0])
    co = tables.pressure_coefs(p)
    f = np.random.default_rng(0).standard_normal(p.size)
    fm, fp = np.concatenate([f[:1], f[:-1]]), np.concatenate([f[1:], f[-1:]])
    assert np.allclose(co[:, 0] * fm + co[:, 1] * f + co[:, 2] * fp, np.gradient(f, p, edge_order=1), rtol=1e-13, atol=0)
    assert co[0, 0] == 0 and co[-1, 2] == 0                      # one-sided at the top and bottom level
    one = tables.pressure_coefs(np.array([50000.0]))
    assert one.shape == (1, 3) and not one.any()                 # one level: no pressure derivative


def test_nl_lat_table():
    lat = np.array([-90.0, -45.0, 0.0, 60.0, 90.0])
    bt = tables.build_box_tables(lat, -180.0 + 15.0 * np.arange(24), [(0, 23, 0, 4)], ring=True)
    t5 = tables.nl_lat_table(bt.lattab[0], lat)
    assert t5.shape == (5, 5) and np.array_equal(t5[:, :4], bt.lattab[0])       # lec_rowspec_q_ring's table, untouched
    assert t5[0, 4] == 0 and t5[4, 4] == 0                       # the pole rows
    assert np.allclose(t5[1:4, 4], np.tan(np.deg2rad(lat[1:4])) / o.RE, rtol=1e-15, atol=0)
    with pytest.raises(ValueError):
        tables.nl_lat_table(bt.lattab[0], lat[:4])


# -- the command line, the framework and the engine -------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["-f", "--periodic", "--wavenumbers-interactions"], ["-f", "--wavenumbers-interactions"],
                                   ["-t", "--wavenumbers-interactions"]])
def test_cli_refuses_interactions_without_wavenumbers(tmp_path, monkeypatch, flags):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", *flags])
    assert "--wavenumbers-interactions goes with --wavenumbers" in str(e.value)
    assert not os.path.exists(tmp_path / "LEC_Results")          # refused before anything was created


@pytest.mark.parametrize("flags, text", [
    (["-f", "--periodic", "--wavenumbers", "4", "--wavenumbers-interactions", "--gpus", "2"], "--wavenumbers runs on one GPU"),
    (["-f", "--periodic", "--wavenumbers", "4", "--wavenumbers-interactions", "--ingest", "device"], "--wavenumbers prepares the data on the host"),
    (["-f", "--wavenumbers", "4", "--wavenumbers-interactions"], "--wavenumbers goes with -f --periodic"),
])
def test_cli_refusals_of_wavenumbers_cover_the_flag(tmp_path, monkeypatch, flags, text):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", *flags])
    assert text in str(e.value)


def test_cli_namespace_of_other_runs_is_unchanged():
    """default=argparse.SUPPRESS: a run without the flag logs the Namespace it always logged."""
    src = open(os.path.join(ROOT, "lorenzcycletoolkit.py")).read()
    line = [ln for ln in src.splitlines() if '"--wavenumbers-interactions"' in ln and "add_argument" in ln]
    assert len(line) == 1 and "default=argparse.SUPPRESS" in line[0] and 'action="store_true"' in line[0]


class _NoGpu:
    """Stands where the engine would be built: the refusals below must come before it."""
    def __init__(self, *a, **k):
        raise AssertionError("the refusal must precede the engine")


def test_framework_refusal(monkeypatch):
    import pandas as pd

    from lorenzcycletoolkit_amd import frameworks
    monkeypatch.setattr(frameworks, "LECEngine", _NoGpu)
    dom = rr.cli_domain()

    class Data:
        lat, lon, level, time = dom.lat, dom.lon, dom.level, None
    with pytest.raises(ValueError, match="spectrum_interactions.*wavenumbers"):
        frameworks.BoxData(Data, pd.DataFrame(), -180, 180, -30, 30, periodic=True, spectrum_interactions=True)


def test_engine_and_ingest_refusals_precede_the_fields():
    from lorenzcycletoolkit_amd import ingest
    from lorenzcycletoolkit_amd.engine import LECEngine
    eng = object.__new__(LECEngine)            # no device: the refusal uses nothing of the engine
    with pytest.raises(ValueError, match="spectrum_interactions.*wavenumbers"):
        eng.compute(None, None, None, None, None, None, spectrum_interactions=True)
    with pytest.raises(ValueError, match="spectrum_interactions.*wavenumbers"):
        ingest.lec_streamed(None, None, None, None, spectrum_interactions=True)


# -- the CSVs ---------------------------------------------------------------------------------------------------------------------
def test_write_spectrum_csvs_writes_s_and_l(tmp_path):
    import pandas as pd

    from lorenzcycletoolkit_amd import frameworks
    nt, n = 3, 4
    rng = np.random.default_rng(1)

    class Box:
        time = pd.date_range("2020-01-01", periods=nt, freq="6h").values
        spectrum = rng.standard_normal((nt, 5, n))
        spectrum_rest = rng.standard_normal((nt, 5))
        spectrum_ge = None
        spectrum_nl = rng.standard_normal((nt, 2, n))
        spectrum_nl_rest = rng.standard_normal((nt, 2))

        def row_labels(self, method):
            return frameworks.time_labels(self.time, method)
    box = Box()
    frameworks.write_spectrum_csvs(box, str(tmp_path / "w"), "time")
    assert sorted(os.listdir(tmp_path / "w")) == sorted(f"{t}_n.csv" for t in ["Ae", "Ke", "Ca", "Ce", "Ck", "S", "L"])
    ae = open(tmp_path / "w" / "Ae_n.csv").read().splitlines()
    for i, term in enumerate(("S", "L")):
        lines = open(tmp_path / "w" / f"{term}_n.csv").read().splitlines()
        assert lines[0] == "time,1,2,3,4,rest" and len(lines) == 1 + nt
        assert [ln.split(",")[0] for ln in lines] == [ln.split(",")[0] for ln in ae]       # the time labels of its siblings
        df = pd.read_csv(tmp_path / "w" / f"{term}_n.csv", index_col=0, float_precision="round_trip")
        assert np.array_equal(df.values[:, :n], box.spectrum_nl[:, i]) and np.array_equal(df["rest"].values, box.spectrum_nl_rest[:, i])
    # without the interactions the two files are not written
    box.spectrum_nl = None
    frameworks.write_spectrum_csvs(box, str(tmp_path / "v"), "time")
    assert sorted(os.listdir(tmp_path / "v")) == sorted(f"{t}_n.csv" for t in ["Ae", "Ke", "Ca", "Ce", "Ck"])


# -- the restatement's own identities ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [8, 65, 128, 129])
def test_restatement_closes_on_the_physical_space_covariance(nx):
    d = rr.ring_domain(3, 4, 5, nx, seed=nx, lat0=-60.0, lat1=60.0)
    n = nx // 2
    shares, totals = nr.row_shares(d, -60, 60, n)
    nl_, rest, levels, total = nr.nl_terms(d, -60, 60, n)
    assert shares.shape == (3, 4, 5, n, 3) and totals.shape == (3, 4, 5, 3)
    assert nl_.shape == (3, 2, n) and rest.shape == (3, 2) and levels.shape == (3, 2, n, 4) and total.shape == (3, 2)
    e_rows = np.abs(shares.sum(axis=3) - totals).max() / np.abs(shares).max()
    e_terms = (np.abs(rest).max(axis=0) / np.abs(nl_).max(axis=(0, 2))).max()
    print(f"nx={nx}: rows close to {e_rows:.2e}, S and L to {e_terms:.2e} of the largest share")
    assert e_rows <= 1e-12 and e_terms <= 1e-12


def test_one_wavenumber_alone_has_no_share():
    """Eddies of one single wavenumber m: A_x holds the wavenumbers 0 and 2 m, x' the wavenumber m: every share vanishes."""
    nx, m = 24, 3
    d = nr.planted_domain(nx, [m])
    _, X, A = nr.tendencies(d, -60, 60)
    shares, totals = nr.row_shares(d, -60, 60, nx // 2)
    scale = max(np.abs(a).max() * np.abs(x).max() for a, x in zip(A, X))
    worst = max(np.abs(shares).max(), np.abs(totals).max()) / scale
    print(f"one wavenumber alone: largest share {worst:.2e} of max|A| max|x'|")
    assert scale > 0 and worst <= 1e-12


@pytest.mark.parametrize("nx, n", [(16, 8), (65, 20)])
def test_the_two_routes_agree(nx, n):
    d = rr.ring_domain(3, 4, 5, nx, seed=nx, lat0=-60.0, lat1=60.0)
    nl_, _, levels, _ = nr.nl_terms(d, -60, 60, n)
    pol, pol_levels = nr.nl_terms_polarised(d, -60, 60, n)
    assert pol.shape == nl_.shape and pol_levels.shape == levels.shape
    # the size of the energies the polarised route subtracts: E[(c a) ** 2 + b ** 2] / 2 / c >= |E[a b]|, per term
    b, X, A = nr.tendencies(d, -60, 60)
    size = np.zeros(2)
    for k in range(1, n + 1):
        wx, wa = [wave_part(x, k) for x in X], [wave_part(a, k) for a in A]
        cT, cK = nr._pow2(wa[0], wx[0]), nr._pow2(np.stack(wa[1:]), np.stack(wx[1:]))
        S, L, _, _ = nr._operators(b, rr._close(((cT * wa[0]) ** 2 + wx[0] ** 2) / cT),
                                   rr._close(((cK * wa[1]) ** 2 + wx[1] ** 2 + (cK * wa[2]) ** 2 + wx[2] ** 2) / cK))
        size = np.maximum(size, [np.abs(S).max(), np.abs(L).max()])
    err = np.abs(pol - nl_).max(axis=(0, 2))
    e_size, e_share = (err / size).max(), (err / np.abs(nl_).max(axis=(0, 2))).max()
    e_lev = (np.abs(pol_levels - levels).max(axis=(0, 2, 3)) / np.abs(levels).max(axis=(0, 2, 3))).max()
    print(f"nx={nx} N={n}: the two routes agree to {e_size:.2e} of the energies subtracted, {e_share:.2e} of the largest share; tables {e_lev:.2e}")
    assert e_size <= 1e-12 and e_share <= 1e-11 and e_lev <= 1e-11
