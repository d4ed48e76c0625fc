"""-f --periodic --wavenumbers N --wavenumbers-generation without a GPU: the additive C call ``lec_rowspec_q_ring`` (export, header, ABI
11, struct layout, every refusal before any HIP call), the command line's and the framework's refusals, and the CPU restatement's own
closure (tests/spectrum_ge_restatement.py).

Bar of the restatement's own check: the N = nx / 2 shares of [Q'T'] of a row sum to the oracle's zonal mean of Q'T', and the Ge(n) to
the oracle's Ge, to 1e-12 of the largest share (a sum of at most 65 terms with a rounding error of a few ulp of scale each; measured
3.4e-14 and 2.7e-15)."""
import ctypes
import os

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib
from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests import spectrum_ge_restatement as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the C call -------------------------------------------------------------------------------------------------------------------
def test_rowspec_q_call_is_additive():
    lib = _lib.load()
    assert "lec_rowspec_q_ring" in _lib.EXPORTS and lib.lec_rowspec_q_ring is not None
    hdr = open(os.path.join(ROOT, "include", "lec_hip.h")).read()
    assert "int lec_rowspec_q_ring(const lec_rowspec_q_args* args);" in hdr
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11 and "#define LEC_ABI_VERSION 11" in hdr
    A = _lib.RowspecQArgs
    assert ctypes.sizeof(A) == 4 * 8 + 10 * 4 + 7 * 8
    offs = {n: getattr(A, n).offset for n, _ in A._fields_}
    assert offs["tair_d"] == 0 and offs["dtype"] == 32 and offs["nx"] == 48 and offs["n_wave"] == 68 and offs["twid_d"] == 72
    assert offs["lattab_d"] == 80 and offs["levtab_d"] == 88 and offs["tcoef_d"] == 96 and offs["inv_hdeg"] == 104
    assert offs["qspec_d"] == 112 and offs["stream"] == 120
    # the sibling call's struct is what it was
    assert ctypes.sizeof(_lib.RowspecArgs) == 4 * 8 + 10 * 4 + 3 * 8


POINTERS = ["tair_d", "u_d", "v_d", "omega_d", "twid_d", "lattab_d", "levtab_d", "tcoef_d", "qspec_d"]


def _valid_args():
    """Scalars of a valid call over fake (never dereferenced) pointers: every refusal is made on the scalars, before any HIP call."""
    a = _lib.RowspecQArgs()
    for name in POINTERS:
        setattr(a, name, 0x10000)
    a.dtype = _lib.LEC_F64
    a.nt, a.nl, a.ny, a.nx, a.t_begin, a.t_count = 3, 4, 5, 16, 0, 3
    a.js, a.jn, a.n_wave = 0, 4, 8
    a.inv_hdeg = 16 / 360.0
    return a


@pytest.mark.parametrize("field, change", [(name, lambda a, name=name: setattr(a, name, None)) for name in POINTERS] + [
    ("dtype", lambda a: setattr(a, "dtype", _lib.LEC_I16)),
    ("nt", lambda a: (setattr(a, "nt", 1), setattr(a, "t_count", 1))),
    ("nx", lambda a: (setattr(a, "nx", 2), setattr(a, "n_wave", 1))),
    ("n_wave", lambda a: setattr(a, "n_wave", 0)),
    ("n_wave", lambda a: setattr(a, "n_wave", 9)),                   # nx / 2 = 8
    ("n_wave", lambda a: (setattr(a, "nx", 17), setattr(a, "n_wave", 9))),      # nx / 2 = 8 on an odd ring too
    ("js", lambda a: setattr(a, "js", -1)),
    ("js", lambda a: (setattr(a, "js", 5), setattr(a, "jn", 5))),
    ("jn", lambda a: setattr(a, "jn", 5)),
    ("jn", lambda a: (setattr(a, "js", 3), setattr(a, "jn", 2))),
    ("jn", lambda a: (setattr(a, "js", 2), setattr(a, "jn", 2))),     # one row: no d/dlat
    ("qspec_d", lambda a: setattr(a, "qspec_d", 0x10008)),
    ("twid_d", lambda a: setattr(a, "twid_d", 0x10008)),
    ("lattab_d", lambda a: setattr(a, "lattab_d", 0x10004)),
    ("levtab_d", lambda a: setattr(a, "levtab_d", 0x10004)),
    ("tcoef_d", lambda a: setattr(a, "tcoef_d", 0x10004)),
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
    assert lib.lec_rowspec_q_ring(ctypes.byref(a)) == 1          # LEC_ERR_ARG
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_rowspec_q_ring") and field.encode() in msg, msg


def test_c_call_null_and_beyond_the_limits():
    lib = _lib.load()
    assert lib.lec_rowspec_q_ring(None) == 1 and b"null args" in lib.lec_last_error()
    a = _valid_args()
    a.nx, a.n_wave = 1440, _lib.LEC_MAX_WAVENUMBERS + 1
    assert lib.lec_rowspec_q_ring(ctypes.byref(a)) == 2          # LEC_ERR_UNSUPPORTED
    msg = lib.lec_last_error()
    assert b"lec_rowspec_q_ring" in msg and b"n_wave" in msg and b"LEC_MAX_WAVENUMBERS" in msg, msg
    a = _valid_args()
    a.nt = a.t_count = 60000
    a.nl, a.ny, a.jn = 200, 200, 199                             # 2.4e9 rows
    assert lib.lec_rowspec_q_ring(ctypes.byref(a)) == 2
    assert b"rows" in lib.lec_last_error()


# -- the command line and the framework -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["-f", "--periodic", "--wavenumbers-generation"], ["-f", "--wavenumbers-generation"],
                                   ["-t", "--wavenumbers-generation"]])
def test_cli_refuses_generation_without_wavenumbers(tmp_path, monkeypatch, flags):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", *flags])
    assert "--wavenumbers-generation goes with --wavenumbers" in str(e.value)
    assert not os.path.exists(tmp_path / "LEC_Results")          # refused before anything was created


@pytest.mark.parametrize("flags, text", [
    (["-f", "--periodic", "--wavenumbers", "4", "--wavenumbers-generation", "--gpus", "2"], "--wavenumbers runs on one GPU"),
    (["-f", "--periodic", "--wavenumbers", "4", "--wavenumbers-generation", "--ingest", "device"], "--wavenumbers prepares the data on the host"),
])
def test_cli_refusals_of_wavenumbers_cover_the_flag(tmp_path, monkeypatch, flags, text):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", *flags])
    assert text in str(e.value)


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
        lat, lon, level, time = dom.lat, dom.lon, dom.level, None
    df = pd.DataFrame()
    with pytest.raises(ValueError, match="spectrum_generation.*wavenumbers"):
        frameworks.BoxData(Data, df, -180, 180, -30, 30, periodic=True, spectrum_generation=True)
    with pytest.raises(ValueError, match="spectrum_generation.*dTdt"):
        frameworks.BoxData(Data, df, -180, 180, -30, 30, periodic=True, wavenumbers=4, spectrum_generation=True, dTdt=np.zeros(1))


def test_engine_refusals_precede_the_fields():
    """``compute`` refuses the flag without wavenumbers, with with_q=False and with a dTdt cube before it looks at a field or a box."""
    from lorenzcycletoolkit_amd.engine import LECEngine
    eng = object.__new__(LECEngine)            # no device: the refusals use nothing of the engine
    for kw, text in (({}, "wavenumbers"), ({"wavenumbers": 4, "with_q": False}, "with_q"), ({"wavenumbers": 4, "dTdt": object()}, "dTdt")):
        with pytest.raises(ValueError, match="spectrum_generation.*" + text):
            eng.compute(None, None, None, None, None, None, spectrum_generation=True, **kw)


# -- the restatement's own closure ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [8, 65, 128, 129])
def test_restatement_closes_on_the_oracle(nx):
    d = rr.ring_domain(3, 4, 5, nx, seed=nx, lat0=-60.0, lat1=60.0)
    n = nx // 2
    shares = gr.row_shares_q(d, -60, 60, n)
    ge, rest, levels, total = gr.ge_terms(d, -60, 60, n)
    assert shares.shape == (3, 4, 5, n) and ge.shape == (3, n) and rest.shape == (3,) and levels.shape == (3, n, 4) and total.shape == (3,)
    b = rr.ring_box(d, -60, 60)
    qt = o.zonal_average(b.f["Q_ZE"] * b.f["tair_ZE"], b.rlons, b.xlength)          # the oracle's [Q'T']
    e_rows = np.abs(shares.sum(axis=-1) - qt).max() / np.abs(shares).max()
    e_ge = np.abs(rest).max() / np.abs(ge).max()
    # the two ways of restating Ge(n): single-wavenumber fields through generation_terms, and C_n through the area mean
    s = b.sigma_AA
    lv = np.stack([o.area_average(shares[..., i], b.rlats, b.coslats) / (o.CP_D * s) for i in range(n)], axis=1)
    e_two = np.abs(lv - levels).max() / np.abs(levels).max()
    print(f"nx={nx}: rows close to {e_rows:.2e}, Ge to {e_ge:.2e}, the two restatements agree to {e_two:.2e} of scale")
    assert e_rows <= 1e-12 and e_ge <= 1e-12 and e_two <= 1e-12
