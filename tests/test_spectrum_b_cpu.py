"""-f --periodic --wavenumbers N --wavenumbers-budget without a GPU: the additive C calls ``lec_rowspec_b_ring`` and
``lec_level_spec_b_ring`` (exports, header, ABI 11, struct layouts, every refusal before any HIP call), the command line's, the
framework's and the engine's refusals, ``tables.spectrum_budgets``, ``write_spectrum_csvs`` on a hand-made result, and the CPU
restatement's own closure (tests/spectrum_b_restatement.py).

Bars.  Closure of the restatement: with N = nx / 2 the shares of BAe(n), BKe(n) sum to the oracle's ``boundary_terms`` and the residuals
to its RGe, RKe to 1e-11 of scale (the largest share, or the total where it is larger): sums of at most 64 terms with a rounding error
of a few ulp of scale each -- the siblings' bar for closures (tests/test_spectrum_nl_cpu.py)."""
import ctypes
import os

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib, tables
from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests import spectrum_b_restatement as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the C calls ------------------------------------------------------------------------------------------------------------------
def test_calls_are_additive():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lec_hip.h")).read()
    for name in ("lec_rowspec_b_ring", "lec_level_spec_b_ring"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert "int lec_rowspec_b_ring(const lec_rowspec_b_args* args);" in hdr
    assert "int lec_level_spec_b_ring(const lec_level_spec_b_args* args);" in hdr
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11 and "#define LEC_ABI_VERSION 11" in hdr
    A = _lib.RowspecBArgs
    assert ctypes.sizeof(A) == 4 * 8 + 10 * 4 + 4 * 8
    offs = {n: getattr(A, n).offset for n, _ in A._fields_}
    assert offs["tair_d"] == 0 and offs["dtype"] == 32 and offs["nx"] == 48 and offs["n_wave"] == 68 and offs["rows_d"] == 72
    assert offs["twid_d"] == 80 and offs["bspec_d"] == 88 and offs["stream"] == 96
    B = _lib.LevelSpecBArgs
    assert B.spec.offset == 0 and B.bspec_d.offset == ctypes.sizeof(_lib.LevelSpecArgs) and ctypes.sizeof(B) == ctypes.sizeof(_lib.LevelSpecArgs) + 8
    # the sibling calls' structs are what they were
    assert ctypes.sizeof(_lib.RowspecArgs) == 4 * 8 + 10 * 4 + 3 * 8 and ctypes.sizeof(_lib.RowspecNlArgs) == 4 * 8 + 10 * 4 + 8 * 8
    assert ctypes.sizeof(_lib.LevelSpecArgs) == 3 * 8 + 4 * 4 + 3 * 8 + 8 + 2 * 8 + 8 + 8


POINTERS = ["tair_d", "u_d", "v_d", "omega_d", "rows_d", "twid_d", "bspec_d"]


def _valid_args():
    """Scalars of a valid call over fake (never dereferenced) pointers: every refusal is made on the scalars, before any HIP call."""
    a = _lib.RowspecBArgs()
    for name in POINTERS:
        setattr(a, name, 0x10000)
    a.dtype = _lib.LEC_F64
    a.nt, a.nl, a.ny, a.nx, a.t_begin, a.t_count = 3, 4, 5, 16, 0, 3
    a.js, a.jn, a.n_wave = 0, 4, 8
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
    ("jn", lambda a: (setattr(a, "js", 2), setattr(a, "jn", 2))),     # one row: no south and north wall
    ("bspec_d", lambda a: setattr(a, "bspec_d", 0x10008)),
    ("rows_d", lambda a: setattr(a, "rows_d", 0x10008)),
    ("twid_d", lambda a: setattr(a, "twid_d", 0x10008)),
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
    assert lib.lec_rowspec_b_ring(ctypes.byref(a)) == 1           # LEC_ERR_ARG
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_rowspec_b_ring") and field.encode() in msg, msg


def test_c_call_null_and_beyond_the_limits():
    lib = _lib.load()
    assert lib.lec_rowspec_b_ring(None) == 1 and b"null args" in lib.lec_last_error()
    a = _valid_args()
    a.nx, a.n_wave = 1440, _lib.LEC_MAX_WAVENUMBERS + 1
    assert lib.lec_rowspec_b_ring(ctypes.byref(a)) == 2           # LEC_ERR_UNSUPPORTED
    msg = lib.lec_last_error()
    assert b"lec_rowspec_b_ring" in msg and b"n_wave" in msg and b"LEC_MAX_WAVENUMBERS" in msg, msg
    a = _valid_args()
    a.nt = a.t_count = 60000
    a.nl, a.ny, a.jn = 200, 200, 199                              # 2.4e9 rows
    assert lib.lec_rowspec_b_ring(ctypes.byref(a)) == 2
    assert b"rows" in lib.lec_last_error()


def _valid_level_args():
    b = _lib.LevelSpecBArgs()
    for name in ("rows_d", "spec_d", "box_d", "lattab2_d", "levtab2_d", "am_d", "levraw_d"):
        setattr(b.spec, name, 0x10000)
    b.spec.t_count, b.spec.nl, b.spec.nyb, b.spec.n_wave = 2, 3, 5, 4
    b.bspec_d = 0x10000
    return b


@pytest.mark.parametrize("field, change, code", [
    ("bspec_d", lambda b: setattr(b, "bspec_d", None), 1),
    ("bspec_d", lambda b: setattr(b, "bspec_d", 0x10008), 1),
    ("rows_d", lambda b: setattr(b.spec, "rows_d", None), 1),
    ("spec_d", lambda b: setattr(b.spec, "spec_d", 0x10008), 1),
    ("nyb", lambda b: setattr(b.spec, "nyb", 1), 1),
    ("wave_stride", lambda b: setattr(b.spec, "wave_stride", 8), 1),
    ("n_wave", lambda b: setattr(b.spec, "n_wave", _lib.LEC_MAX_WAVENUMBERS + 1), 2),
])
def test_level_call_refusals_carry_its_own_name(field, change, code):
    lib = _lib.load()
    b = _valid_level_args()
    change(b)
    assert lib.lec_level_spec_b_ring(ctypes.byref(b)) == code
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_level_spec_b_ring: ") and field.encode() in msg, msg
    assert lib.lec_level_spec_b_ring(None) == 1 and b"null args" in lib.lec_last_error()


def test_level_spec_ring_keeps_its_messages():
    lib = _lib.load()
    a = _valid_level_args().spec
    a.nyb = 1
    assert lib.lec_level_spec_ring(ctypes.byref(a)) == 1
    assert lib.lec_last_error() == b"lec_level_spec_ring: nyb must be >= 2 (a band needs two rows)"


# -- the command line, the framework and the engine -------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["-f", "--periodic", "--wavenumbers-budget"], ["-f", "--wavenumbers-budget"], ["-t", "--wavenumbers-budget"]])
def test_cli_refuses_budget_without_wavenumbers(tmp_path, monkeypatch, flags):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", *flags])
    assert "--wavenumbers-budget goes with --wavenumbers" in str(e.value)
    assert not os.path.exists(tmp_path / "LEC_Results")          # refused before anything was created


@pytest.mark.parametrize("flags, text", [
    (["-f", "--periodic", "--wavenumbers", "4", "--wavenumbers-budget", "--gpus", "2"], "--wavenumbers runs on one GPU"),
    (["-f", "--periodic", "--wavenumbers", "4", "--wavenumbers-budget", "--ingest", "device"], "--wavenumbers prepares the data on the host"),
    (["-f", "--wavenumbers", "4", "--wavenumbers-budget"], "--wavenumbers goes with -f --periodic"),
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
    line = [ln for ln in src.splitlines() if '"--wavenumbers-budget"' in ln and "add_argument" in ln]
    assert len(line) == 1 and "default=argparse.SUPPRESS" in line[0] and 'action="store_true"' in line[0]


class _NoGpu:
    """Stands where the engine would be built: the refusals below must come before it."""
    def __init__(self, *a, **k):
        raise AssertionError("the refusal must precede the engine")


def test_framework_refusals(monkeypatch):
    import pandas as pd

    from lorenzcycletoolkit_amd import frameworks
    monkeypatch.setattr(frameworks, "LECEngine", _NoGpu)
    dom = rr.cli_domain()

    class Data:
        lat, lon, level, time = dom.lat, dom.lon, dom.level, np.arange(1)
    with pytest.raises(ValueError, match="spectrum_budget.*wavenumbers"):
        frameworks.BoxData(Data, pd.DataFrame(), -180, 180, -30, 30, periodic=True, spectrum_budget=True)
    with pytest.raises(ValueError, match="spectrum_budget.*at least 2 time steps"):          # a series of one time step
        frameworks.BoxData(Data, pd.DataFrame(), -180, 180, -30, 30, periodic=True, wavenumbers=4, spectrum_budget=True)


def test_engine_and_ingest_refusals_precede_the_fields():
    import torch

    from lorenzcycletoolkit_amd import ingest
    from lorenzcycletoolkit_amd.engine import LECEngine
    eng = object.__new__(LECEngine)            # no device: the refusal uses nothing of the engine
    with pytest.raises(ValueError, match="spectrum_budget.*wavenumbers"):
        eng.compute(None, None, None, None, None, None, spectrum_budget=True)
    with pytest.raises(ValueError, match="spectrum_budget needs time_s"):
        eng.compute(None, None, None, None, None, None, wavenumbers=4, spectrum_budget=True)
    one = torch.zeros((1, 2, 3, 8))
    with pytest.raises(ValueError, match="spectrum_budget.*at least 2 time steps"):
        eng.compute(one, one, one, one, None, None, wavenumbers=4, spectrum_budget=True, time_s=np.zeros(1))
    two = torch.zeros((2, 2, 3, 8))
    with pytest.raises(ValueError, match="spectrum_budget.*at least 2 time steps"):          # one PROCESSED step of a longer cube
        eng.compute(two, two, two, two, None, None, wavenumbers=4, spectrum_budget=True, time_s=np.arange(2.0), t_begin=1)
    with pytest.raises(ValueError, match="spectrum_budget.*wavenumbers"):
        ingest.lec_streamed(None, None, None, None, spectrum_budget=True)


# -- the host arithmetic ----------------------------------------------------------------------------------------------------------
def test_spectrum_budgets_is_the_totals_function_column_by_column():
    rng = np.random.default_rng(2)
    nt, n = 5, 3
    spec, rest = rng.standard_normal((nt, 5, n)), rng.standard_normal((nt, 5))
    b, b_rest = rng.standard_normal((nt, 2, n)), rng.standard_normal((nt, 2))
    time_s = 21600.0 * np.arange(nt)
    got = tables.spectrum_budgets(spec, rest, b, b_rest, time_s)
    assert got["tendency"].shape == (nt, 2, n) and got["residual"].shape == (nt, 2, n)
    assert got["tendency_rest"].shape == (nt, 2) and got["residual_rest"].shape == (nt, 2)
    for i in range(n):
        dAe, dKe = np.gradient(spec[:, 0, i], 21600.0), np.gradient(spec[:, 1, i], 21600.0)
        assert np.array_equal(got["tendency"][:, 0, i], dAe) and np.array_equal(got["tendency"][:, 1, i], dKe)
        assert np.array_equal(got["residual"][:, 0, i], dAe - spec[:, 2, i] + spec[:, 3, i] - b[:, 0, i])       # RGe = dAe/dt - Ca + Ce - BAe
        assert np.array_equal(got["residual"][:, 1, i], dKe - spec[:, 3, i] + spec[:, 4, i] - b[:, 1, i])       # RKe = dKe/dt - Ce + Ck - BKe
    assert np.array_equal(got["residual_rest"][:, 0], np.gradient(rest[:, 0], 21600.0) - rest[:, 2] + rest[:, 3] - b_rest[:, 0])
    # the restatement's columns (the oracle's function) are the same numbers
    t, tr, r, rr_ = br.budget_columns(spec, rest, b, b_rest, time_s)
    assert np.array_equal(t, got["tendency"]) and np.array_equal(r, got["residual"]) and np.array_equal(rr_, got["residual_rest"])
    with pytest.raises(ValueError, match="at least 2 time steps"):
        tables.spectrum_budgets(spec[:1], rest[:1], b[:1], b_rest[:1], time_s[:1])


# -- the CSVs ---------------------------------------------------------------------------------------------------------------------
def test_write_spectrum_csvs_writes_the_six_files(tmp_path):
    import pandas as pd

    from lorenzcycletoolkit_amd import frameworks
    nt, n = 3, 4
    rng = np.random.default_rng(1)

    class Box:
        time = pd.date_range("2020-01-01", periods=nt, freq="6h").values
        spectrum = rng.standard_normal((nt, 5, n))
        spectrum_rest = rng.standard_normal((nt, 5))
        spectrum_ge = None
        spectrum_nl = None
        spectrum_b, spectrum_b_rest = rng.standard_normal((nt, 2, n)), rng.standard_normal((nt, 2))
        spectrum_tendency, spectrum_tendency_rest = rng.standard_normal((nt, 2, n)), rng.standard_normal((nt, 2))
        spectrum_residual, spectrum_residual_rest = rng.standard_normal((nt, 2, n)), rng.standard_normal((nt, 2))

        def row_labels(self, method):
            return frameworks.time_labels(self.time, method)
    box = Box()
    frameworks.write_spectrum_csvs(box, str(tmp_path / "w"), "time")
    new = {"BAe": ("spectrum_b", 0), "BKe": ("spectrum_b", 1), "dAedt": ("spectrum_tendency", 0), "dKedt": ("spectrum_tendency", 1),
           "RGe": ("spectrum_residual", 0), "RKe": ("spectrum_residual", 1)}
    assert sorted(os.listdir(tmp_path / "w")) == sorted(f"{t}_n.csv" for t in ["Ae", "Ke", "Ca", "Ce", "Ck", *new])
    ae = open(tmp_path / "w" / "Ae_n.csv").read().splitlines()
    for term, (field, i) in new.items():
        lines = open(tmp_path / "w" / f"{term}_n.csv").read().splitlines()
        assert lines[0] == "time,1,2,3,4,rest" and len(lines) == 1 + nt
        assert [ln.split(",")[0] for ln in lines] == [ln.split(",")[0] for ln in ae]       # the time labels of its siblings
        df = pd.read_csv(tmp_path / "w" / f"{term}_n.csv", index_col=0, float_precision="round_trip")
        assert np.array_equal(df.values[:, :n], getattr(box, field)[:, i]) and np.array_equal(df["rest"].values, getattr(box, field + "_rest")[:, i])
    box.spectrum_b = None           # without the budget the six files are not written
    frameworks.write_spectrum_csvs(box, str(tmp_path / "v"), "time")
    assert sorted(os.listdir(tmp_path / "v")) == sorted(f"{t}_n.csv" for t in ["Ae", "Ke", "Ca", "Ce", "Ck"])


# -- the restatement's closure ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [8, 65, 128, 129])
def test_rows_close_on_the_triple_products(nx):
    d = rr.ring_domain(3, 4, 5, nx, seed=nx, lat0=-60.0, lat1=60.0)
    sh = br.row_shares(d.tair, d.u, d.v, d.omega, nx // 2)
    tot = br.row_totals(d.tair, d.u, d.v, d.omega)
    assert sh.shape == (3, 4, 5, nx // 2, 4) and tot.shape == (3, 4, 5, 4)
    err = (np.abs(sh.sum(axis=3) - tot).max(axis=(0, 1, 2)) / np.abs(sh).max(axis=(0, 1, 2, 3))).max()
    print(f"nx={nx}: the nx / 2 shares of a row sum to the triple products to {err:.2e} of the largest share")
    assert err <= 1e-11


@pytest.mark.parametrize("nx", [16, 65])
def test_restatement_closes_on_the_oracle(nx):
    """N = nx / 2: sum_n BAe(n), BKe(n) = ``boundary_terms``' BAe, BKe of the ring box; the summed residuals = the oracle's RGe, RKe."""
    d = rr.ring_domain(4, 4, 5, nx, seed=nx, lat0=-60.0, lat1=60.0)
    n = nx // 2
    got = br.budget_terms(d, -60, 60, n)
    assert got["b"].shape == (4, 2, n) and got["residual"].shape == (4, 2, n)
    scale = np.maximum(np.abs(got["b"]).max(axis=(0, 2)), np.abs(got["b_total"]).max(axis=0))
    e_b = (np.abs(got["b"].sum(axis=2) - got["b_total"]).max(axis=0) / scale).max()
    scalars, _ = rr.ring_terms(d, -60, 60)
    ref = o.budgets_and_residuals(scalars, d.time_s)
    assert np.array_equal(got["b_total"][:, 0], ref["BAe"]) and np.array_equal(got["b_total"][:, 1], ref["BKe"])
    want = np.stack([ref["RGe"], ref["RKe"]], axis=1)
    # the shares alone (the rest is what the spectra leave, by construction a rounding error here)
    rscale = np.maximum(np.abs(got["residual"]).max(axis=(0, 2)), np.abs(want).max(axis=0))
    e_r = (np.abs(got["residual"].sum(axis=2) - want).max(axis=0) / rscale).max()
    e_t = (np.abs(got["residual"].sum(axis=2) + got["residual_rest"] - want).max(axis=0) / rscale).max()
    print(f"nx={nx}: sum BAe(n), BKe(n) closes to {e_b:.2e}, the summed residuals to {e_r:.2e} (with the rest: {e_t:.2e}) of scale")
    assert e_b <= 1e-11 and e_r <= 1e-11 and e_t <= 1e-11
