"""Latitude x pressure sections without a GPU: the definition (the restatement of tests/sections_restatement.py closes on the oracle's own
per-level tables and scalars), the additive C call ``lec_sections`` (export, header, ABI 11, struct layout, every refusal on the scalars
before any HIP call), the command line's refusals around --sections and the writer's files on a hand-made result.

Bar of the definition: 1e-13 of each term's scale -- ``area_average`` is linear in its argument, so the two sides differ by the order of
a handful of fp64 sums (measured: at most 1.5e-15)."""
import ctypes
import os
import types

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib
from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests import sections_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the definition -----------------------------------------------------------------------------------------------------------------
def _boxes():
    dom = rr.ring_domain(3, 5, 9, 16)
    return {"ring": rr.ring_box(dom, -60.0, 60.0), "open": o.make_box(dom, -100.0, 100.0, -45.0, 45.0)}


@pytest.mark.parametrize("kind", ["ring", "open"])
def test_restatement_closes_on_the_oracle(kind):
    b = _boxes()[kind]
    X = sr.sections(b)
    C = sr.columns(X, b.level)
    scalars, levels = o.all_terms(b)
    cw = sr.area_weights(b)
    assert X.shape == (3, 10, 5, b.rlats.size) and C.shape == (3, 10, b.rlats.size)
    for i, term in enumerate(sr.TERMS):
        lv = np.broadcast_to(np.asarray(levels[term], dtype=np.float64), (3, 5))
        sc = np.asarray(scalars[term], dtype=np.float64)
        # through the oracle's own area average, and through the row weights
        assert np.abs(o.area_average(X[:, i], b.rlats, b.coslats) - lv).max() <= 1e-13 * np.abs(lv).max(), term
        assert np.abs((X[:, i] * cw).sum(axis=-1) - lv).max() <= 1e-13 * np.abs(lv).max(), term
        assert np.abs((C[:, i] * cw).sum(axis=-1) - sc).max() <= 1e-13 * np.abs(sc).max(), term


def test_spectral_restatement_closes_on_the_totals():
    b = _boxes()["ring"]
    X = sr.sections(b)
    Xn = sr.spectral_sections(b, 8, generation=True)               # N = nx / 2: Parseval leaves nothing
    tot = X[:, [sr.TERMS.index(k) for k in sr.SPEC_TERMS]]
    assert Xn.shape == (3, 6, 8, 5, 9)
    assert (np.abs(Xn.sum(axis=2) - tot).max(axis=(0, 2, 3)) <= 1e-13 * np.abs(tot).max(axis=(0, 2, 3))).all()
    M = sr.spectral_columns_mean(b, 8, generation=True)
    assert M.shape == (6, 9, 9) and (np.abs(M[:, 8]).max(axis=1) <= 1e-13 * np.abs(M[:, :8]).max(axis=(1, 2))).all()


def test_column_nan_rule():
    p = np.array([100.0, 200.0, 400.0, 700.0, 1000.0])
    y = np.array([1.0, 2.0, 4.0, 7.0, 10.0])
    col = lambda v: sr.columns(np.asarray(v, dtype=np.float64)[None, None, :, None], p, ["Az"])[0, 0, 0]
    whole = col(y)
    bridged = y.copy(); bridged[2] = np.nan
    assert col(bridged) == pytest.approx(whole, rel=1e-15)           # y is linear in p: bridging an interior gap changes nothing
    top = y.copy(); top[0] = np.nan
    assert col(top) == pytest.approx(o.trapz(y[1:], p[1:], axis=0), rel=1e-15)      # a NaN end level is left out
    assert np.isnan(col(np.full(5, np.nan)))                          # no finite level: NaN, not the 0.0 of an empty integral
    one = np.full(5, np.nan); one[3] = 2.0
    assert col(one) == 0.0


# -- the C call ---------------------------------------------------------------------------------------------------------------------
def test_sections_call_is_additive():
    lib = _lib.load()
    assert "lec_sections" in _lib.EXPORTS and lib.lec_sections is not None
    hdr = open(os.path.join(ROOT, "include", "lec_hip.h")).read()
    assert "int lec_sections(const lec_sections_args* args);" in hdr
    assert "#define LEC_LEVRAW_SIGMA 33" in hdr and "#define LEC_NSECTION 10" in hdr
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11 and "#define LEC_ABI_VERSION 11" in hdr
    A = _lib.SectionsArgs
    assert ctypes.sizeof(A) == 8 + 4 * 4 + 9 * 8 + 2 * 4 + 3 * 8 == 128
    offs = {n: getattr(A, n).offset for n, _ in A._fields_}
    assert offs["rows_d"] == 0 and offs["t_count"] == 8 and offs["nl"] == 12 and offs["n_box"] == 16 and offs["nyb"] == 20
    assert offs["box_d"] == 24 and offs["lattab2_d"] == 32 and offs["levtab2_d"] == 40 and offs["levraw_d"] == 48
    assert offs["sec_d"] == 56 and offs["col_d"] == 64 and offs["secsum_d"] == 72 and offs["spec_d"] == 80 and offs["qspec_d"] == 88
    assert offs["n_wave"] == 96 and offs["reserved0"] == 100 and offs["specsec_d"] == 104 and offs["speccolsum_d"] == 112
    assert offs["stream"] == 120
    # the existing structs are what they were
    assert ctypes.sizeof(_lib.ReduceArgs) == 8 + 4 * 4 + 4 * 8 + 8 + 2 * 4 + 8 + 6 * 8 + 2 * 8
    assert ctypes.sizeof(_lib.LevelSpecArgs) == 3 * 8 + 4 * 4 + 3 * 8 + 8 + 2 * 8 + 8 + 8


def _valid_args(spectral=False):
    """Scalars of a valid call over fake (never dereferenced) pointers: every refusal is made on the scalars, before any HIP call."""
    fake = ctypes.c_void_p(0x10000)
    a = _lib.SectionsArgs()
    a.rows_d = a.box_d = a.lattab2_d = a.levtab2_d = a.levraw_d = a.sec_d = a.col_d = a.secsum_d = fake
    a.t_count, a.nl, a.n_box, a.nyb = 3, 4, 1, 5
    if spectral:
        a.spec_d = a.qspec_d = a.specsec_d = a.speccolsum_d = fake
        a.n_wave = 8
    return a


def _set(**kw):
    return lambda a: [setattr(a, k, v) for k, v in kw.items()]


@pytest.mark.parametrize("field, spectral, change", [
    ("rows_d", False, _set(rows_d=None)), ("box_d", False, _set(box_d=None)), ("lattab2_d", False, _set(lattab2_d=None)),
    ("levtab2_d", False, _set(levtab2_d=None)), ("levraw_d", False, _set(levraw_d=None)), ("sec_d", False, _set(sec_d=None)),
    ("col_d", False, _set(col_d=None)), ("secsum_d", False, _set(secsum_d=None)),
    ("n_box", False, _set(n_box=3)), ("n_box", False, _set(n_box=0)),
    ("t_count", False, _set(t_count=0)), ("nl", False, _set(nl=1)), ("nyb", False, _set(nyb=1)),
    ("n_wave", False, _set(n_wave=-1)), ("reserved0", False, _set(reserved0=1)),
    ("qspec_d", True, _set(spec_d=None, n_wave=0)),                     # qspec_d without spec_d
    ("spec_d", False, _set(n_wave=4)),                                  # n_wave without spec_d
    ("n_wave", True, _set(n_wave=0)),                                   # spec_d without n_wave
    ("specsec_d", True, _set(specsec_d=None)), ("speccolsum_d", True, _set(speccolsum_d=None)),
    ("rows_d", False, _set(rows_d=0x10008)), ("lattab2_d", False, _set(lattab2_d=0x10008)), ("spec_d", True, _set(spec_d=0x10008)),
])
def test_c_call_refusals_name_the_field(field, spectral, change):
    lib = _lib.load()
    a = _valid_args(spectral)
    change(a)
    assert lib.lec_sections(ctypes.byref(a)) == 1          # LEC_ERR_ARG
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_sections") and field.encode() in msg, msg


@pytest.mark.parametrize("field, spectral, change", [
    ("nl", False, _set(nl=161)),                                        # LEC_MAX_LEVELS = 160
    ("n_wave", True, _set(n_wave=_lib.LEC_MAX_WAVENUMBERS + 1)),
    ("t_count", False, _set(nl=64, t_count=1 << 20)),                   # 2^26 workgroups of 64 threads
    ("t_count", True, _set(n_wave=63, nl=64, t_count=1 << 14)),
    ("nyb", True, _set(n_wave=64, nyb=(1 << 31) - 1)),                  # 384 functions x nyb threads in the fold
])
def test_c_call_beyond_the_limits(field, spectral, change):
    lib = _lib.load()
    a = _valid_args(spectral)
    change(a)
    assert lib.lec_sections(ctypes.byref(a)) == 2          # LEC_ERR_UNSUPPORTED
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_sections") and field.encode() in msg, msg


def test_c_call_null_args():
    lib = _lib.load()
    assert lib.lec_sections(None) == 1
    assert lib.lec_last_error().startswith(b"lec_sections") and b"null args" in lib.lec_last_error()


# -- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags, text", [
    (["-t", "--sections"], "--sections goes with -f/--fixed"),
    (["-c", "--sections"], "--sections goes with -f/--fixed"),
    (["-f", "--sections", "--gpus", "2"], "--sections runs on one GPU"),
    (["-f", "--periodic", "--sections", "--gpus", "4"], "--sections runs on one GPU"),
])
def test_cli_refusals(tmp_path, monkeypatch, flags, text):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", *flags])
    assert text in str(e.value)
    assert not os.path.exists(tmp_path / "LEC_Results")          # refused before anything was created


def test_cli_help_names_the_flag(capsys):
    import lorenzcycletoolkit
    with pytest.raises(SystemExit):
        lorenzcycletoolkit.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--sections" in text and "results_sections/" in text and "<term>_lat_lv.csv" in text


def test_engine_refusals_in_words():
    from lorenzcycletoolkit_amd.engine import LECEngine
    with pytest.raises(ValueError, match="ONE fixed box"):
        LECEngine._check_sections([(0, 3, 0, 3)] * 2, None)
    with pytest.raises(ValueError, match="ONE fixed box"):
        LECEngine._check_sections([(0, 3, 0, 3)], True)
    LECEngine._check_sections([(0, 3, 0, 3)], False)


# -- the writer ---------------------------------------------------------------------------------------------------------------------
def test_writer_headers_and_labels(tmp_path):
    import pandas as pd
    from lorenzcycletoolkit_amd import frameworks as fw
    from lorenzcycletoolkit_amd.constants import SECTION_TERMS
    nt, nl, ny, n = 3, 2, 4, 2
    rng = np.random.default_rng(0)
    time = pd.date_range("2020-01-01", periods=nt, freq="6h")
    box = types.SimpleNamespace(
        section_mean=rng.standard_normal((10, nl, ny)), section_lat=rng.standard_normal((nt, 10, ny)),
        section_spec_lat=rng.standard_normal((6, n + 1, ny)), section_latitudes=np.array([-45.0, -15.0, 15.0, 45.0]),
        PressureData=np.array([50000.0, 100000.0]), time=time.values, row_labels=lambda method: fw.time_labels(time.values, method))
    box.section_mean[3, 1, 2] = np.nan
    out = tmp_path / "results_sections"
    fw.write_section_csvs(box, str(out), "time", "level")
    names = sorted(os.listdir(out))
    assert names == sorted([f"{t}_lat_lv.csv" for t in SECTION_TERMS] + [f"{t}_lat.csv" for t in SECTION_TERMS]
                           + [f"{t}_n_lat.csv" for t in ("Ae", "Ke", "Ca", "Ce", "Ck", "Ge")])
    lv = pd.read_csv(out / "Ke_lat_lv.csv", index_col=0, float_precision="round_trip")
    assert lv.index.name == "level" and list(lv.index) == [50000.0, 100000.0]
    assert [float(c) for c in lv.columns] == [-45.0, -15.0, 15.0, 45.0]
    assert np.array_equal(lv.values, box.section_mean[3], equal_nan=True)            # repr(float): the values round-trip
    lines = open(out / "Ke_lat_lv.csv").read().splitlines()
    assert lines[0] == "level,-45.0,-15.0,15.0,45.0" and lines[1].startswith("50000.0,") and lines[2].split(",")[3] == ""
    lat = pd.read_csv(out / "Ck_lat.csv", index_col=0, float_precision="round_trip")
    assert lat.index.name == "time" and list(lat.index) == ["2020-01-01 00:00:00", "2020-01-01 06:00:00", "2020-01-01 12:00:00"]
    assert np.array_equal(lat.values, box.section_lat[:, SECTION_TERMS.index("Ck")])
    sp = pd.read_csv(out / "Ge_n_lat.csv", index_col=0, float_precision="round_trip")
    assert sp.index.name == "n" and [str(x) for x in sp.index] == ["1", "2", "rest"]
    assert np.array_equal(sp.values, box.section_spec_lat[5])
    # without spectra: the twenty files
    box.section_spec_lat = None
    fw.write_section_csvs(box, str(tmp_path / "plain"), "time", "level")
    assert len(os.listdir(tmp_path / "plain")) == 20
