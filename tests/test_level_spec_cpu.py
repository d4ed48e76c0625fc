"""Stage 2 of the spectra without assembled records, without a GPU: the additive C call ``lec_level_spec_ring`` (export, header, ABI 11,
struct layout, every refusal on the scalars before any HIP call) and the command line's refusals around --wavenumbers-chunk."""
import ctypes
import os

import pytest

from lorenzcycletoolkit_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_level_spec_call_is_additive():
    lib = _lib.load()
    assert "lec_level_spec_ring" in _lib.EXPORTS and lib.lec_level_spec_ring is not None
    hdr = open(os.path.join(ROOT, "include", "lec_hip.h")).read()
    assert "int lec_level_spec_ring(const lec_level_spec_args* args);" in hdr
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11 and "#define LEC_ABI_VERSION 11" in hdr
    A = _lib.LevelSpecArgs
    assert ctypes.sizeof(A) == 3 * 8 + 4 * 4 + 3 * 8 + 8 + 2 * 8 + 8 + 8
    offs = {n: getattr(A, n).offset for n, _ in A._fields_}
    assert offs["rows_d"] == 0 and offs["spec_d"] == 8 and offs["qspec_d"] == 16
    assert offs["t_count"] == 24 and offs["nl"] == 28 and offs["nyb"] == 32 and offs["n_wave"] == 36
    assert offs["box_d"] == 40 and offs["lattab2_d"] == 48 and offs["levtab2_d"] == 56 and offs["phi_scale"] == 64
    assert offs["am_d"] == 72 and offs["levraw_d"] == 80 and offs["wave_stride"] == 88 and offs["stream"] == 96
    # the existing structs are what they were
    assert ctypes.sizeof(_lib.RowstatsArgs) == 6 * 8 + 14 * 4 + 9 * 8 + 8 * 4 + 2 * 8
    assert ctypes.sizeof(_lib.ReduceArgs) == 8 + 4 * 4 + 4 * 8 + 8 + 2 * 4 + 8 + 6 * 8 + 2 * 8
    assert ctypes.sizeof(_lib.RowspecArgs) == 4 * 8 + 10 * 4 + 3 * 8
    assert ctypes.sizeof(_lib.RowspecQArgs) == 4 * 8 + 10 * 4 + 4 * 8 + 8 + 2 * 8


def _valid_args():
    """Scalars of a valid call over fake (never dereferenced) pointers: every refusal is made on the scalars, before any HIP call."""
    fake = ctypes.c_void_p(0x10000)
    a = _lib.LevelSpecArgs()
    a.rows_d = a.spec_d = a.qspec_d = a.box_d = a.lattab2_d = a.levtab2_d = a.am_d = a.levraw_d = fake
    a.t_count, a.nl, a.nyb, a.n_wave = 3, 4, 5, 8
    a.phi_scale, a.wave_stride = 1.0, 0
    return a


@pytest.mark.parametrize("field, change", [
    ("rows_d", lambda a: setattr(a, "rows_d", None)),
    ("spec_d", lambda a: setattr(a, "spec_d", None)),
    ("box_d", lambda a: setattr(a, "box_d", None)),
    ("lattab2_d", lambda a: setattr(a, "lattab2_d", None)),
    ("levtab2_d", lambda a: setattr(a, "levtab2_d", None)),
    ("am_d", lambda a: setattr(a, "am_d", None)),
    ("levraw_d", lambda a: setattr(a, "levraw_d", None)),
    ("rows_d", lambda a: setattr(a, "rows_d", 0x10008)),
    ("spec_d", lambda a: setattr(a, "spec_d", 0x10008)),
    ("lattab2_d", lambda a: setattr(a, "lattab2_d", 0x10008)),
    ("n_wave", lambda a: setattr(a, "n_wave", 0)),
    ("t_count", lambda a: setattr(a, "t_count", 0)),
    ("nl", lambda a: setattr(a, "nl", 0)),
    ("nyb", lambda a: setattr(a, "nyb", 1)),
    ("wave_stride", lambda a: setattr(a, "wave_stride", 3 * 4 * _lib.LEC_NLEVRAW - 1)),
    ("wave_stride", lambda a: setattr(a, "wave_stride", -1)),
])
def test_c_call_refusals_name_the_field(field, change):
    lib = _lib.load()
    a = _valid_args()
    change(a)
    assert lib.lec_level_spec_ring(ctypes.byref(a)) == 1          # LEC_ERR_ARG
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_level_spec_ring") and field.encode() in msg, msg


@pytest.mark.parametrize("field, change", [
    ("n_wave", lambda a: setattr(a, "n_wave", _lib.LEC_MAX_WAVENUMBERS + 1)),
    ("nl", lambda a: setattr(a, "nl", 161)),                                       # LEC_MAX_LEVELS = 160
    ("t_count", lambda a: (setattr(a, "n_wave", 64), setattr(a, "nl", 64), setattr(a, "t_count", 1 << 14))),      # 2^26 workgroups
])
def test_c_call_beyond_the_limits(field, change):
    lib = _lib.load()
    a = _valid_args()
    change(a)
    assert lib.lec_level_spec_ring(ctypes.byref(a)) == 2          # LEC_ERR_UNSUPPORTED
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_level_spec_ring") and field.encode() in msg, msg


def test_c_call_null_args():
    lib = _lib.load()
    assert lib.lec_level_spec_ring(None) == 1
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_level_spec_ring") and b"null args" in msg


# -- the command line -------------------------------------------------------------------------------------------------------------
SPECTRA = ["-f", "--periodic", "--wavenumbers", "4"]


@pytest.mark.parametrize("flags, text", [
    (["-f", "--periodic", "--wavenumbers-chunk", "2"], "--wavenumbers-chunk goes with --wavenumbers"),
    (["-f", "--wavenumbers-chunk", "2"], "--wavenumbers-chunk goes with --wavenumbers"),
    (SPECTRA + ["--wavenumbers-chunk", "0"], "--wavenumbers-chunk must be >= 1"),
    (SPECTRA + ["--wavenumbers-chunk", "-2"], "--wavenumbers-chunk must be >= 1"),
    (SPECTRA + ["--wavenumbers-chunk", "2", "--ingest", "host"], "give one of the two"),
    (SPECTRA + ["--wavenumbers-chunk", "2", "--gpus", "2"], "--wavenumbers runs on one GPU"),
    (["-f", "--wavenumbers", "4", "--wavenumbers-chunk", "2"], "--wavenumbers goes with -f --periodic"),
    (SPECTRA + ["--wavenumbers-chunk", "2", "--series", "b.nc", "--inflate", "device"], "--inflate device is not supported with --series"),
    # without the flag the device ingest of the spectra stays refused, in the words it was refused with, and names the flag
    (SPECTRA + ["--ingest", "device"], "--wavenumbers prepares the data on the host: --ingest device / --device-ingest is not supported for the spectra"),
    (SPECTRA + ["--device-ingest"], "--wavenumbers-chunk N"),
])
def test_cli_refusals(tmp_path, monkeypatch, flags, text):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", *flags])
    assert text in str(e.value)
    assert not os.path.exists(tmp_path / "LEC_Results")          # refused before anything was created
