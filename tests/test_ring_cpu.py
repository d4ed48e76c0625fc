"""-f --periodic without a GPU: the CPU restatement of the closed axis (tests/ring_restatement.py) is rotation-invariant and exact on
an analytic wave where the limited-area evaluation is not, its east-west boundary pieces are exactly 0; the ring's host tables, the
additive C call ``lec_rowstats_ring`` (export, ABI 11, unchanged struct, every refusal before any HIP call) and the command line's
refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

from lorenzcycletoolkit_amd import _lib, tables
from lorenzcycletoolkit_amd.constants import RE
from lorenzcycletoolkit_amd.follow import ring_error
from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests.helpers import SCALARS, scale_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9          # of each term's scale: the bar of the fixed-box parity tests


@pytest.fixture(scope="module")
def dom():
    return rr.ring_domain(3, 5, 9, 16, seed=1)


@pytest.fixture(scope="module")
def ring(dom):
    return rr.ring_terms(dom, -60, 60)


@pytest.mark.parametrize("k", [1, 5, 8, 15])
def test_restatement_is_rotation_invariant(dom, ring, k):
    s, lv = rr.ring_terms(rr.rolled(dom, k), -60, 60)
    worst = {n: scale_err(s[n], ring[0][n]) for n in SCALARS}
    worst.update({"lv:" + n: scale_err(lv[n], ring[1][n]) for n in lv})
    print(f"rotation by {k}: worst {max(worst.values()):.2e}")
    assert max(worst.values()) <= TOL, {n: e for n, e in worst.items() if e > TOL}


def test_ring_differs_from_the_limited_area_evaluation(dom, ring):
    """The ring changes the answers, not the last digits: every integrated term moves by more than 1e-3 of its scale."""
    s, _ = o.all_terms(o.make_box(dom, -180, 180, -60, 60))
    moved = {n: scale_err(s[n], ring[0][n]) for n in SCALARS}
    print({n: f"{e:.3f}" for n, e in moved.items()})
    assert min(moved.values()) > 1e-3, moved


@pytest.mark.parametrize("m", [1, 2, 5])
def test_zonal_mean_of_a_wave_is_its_constant(dom, m):
    a, b = 250.0, 7.0
    lam = np.deg2rad(dom.lon)
    wave = np.broadcast_to(a + b * np.cos(m * lam), dom.tair.shape).copy()
    d = o.Domain(wave, dom.u, dom.v, dom.omega, dom.geopt, dom.lat, dom.lon, dom.level, dom.time_s)
    za = rr.ring_box(d, -60, 60).f["tair_ZA"]
    assert np.max(np.abs(za - a)) <= 1e-13 * a
    limited = o.make_box(d, -180, 180, -60, 60).f["tair_ZA"]
    assert np.max(np.abs(limited - a)) > 1e-3 * b          # the seam's missing interval and half weights


def test_east_west_pieces_are_exactly_zero(dom):
    b = rr.ring_box(dom, -60, 60)
    f = b.f
    ew = lambda X: X[..., -1] - X[..., 0]
    for name, X in f.items():
        if X.ndim == 4:
            assert np.all(ew(X) == 0.0), name
    tae4 = f["tair_AE"][..., None]
    K = f["u"] ** 2 + f["v"] ** 2 - f["u_ZE"] ** 2 - f["v_ZE"] ** 2
    E = f["u_ZE"] ** 2 + f["v_ZE"] ** 2
    pieces = {"BAz": (2 * tae4 * f["tair_ZE"] * f["u"]) + (tae4 ** 2 * f["u"]), "BAe": f["u"] * f["tair_ZE"] ** 2, "BKz": f["u"] * K,
              "BKe": f["u"] * E, "BΦE": f["v_ZE"] * f["geopt_AE"][..., None] / o.G}
    for name, X in pieces.items():
        d = ew(X)
        assert d.shape == X.shape[:-1] and np.all(d == 0.0), name


def test_ring_tables():
    lat = np.linspace(-50.0, 50.0, 5)
    lon = -180.0 + 15.0 * np.arange(24)
    t = tables.build_box_tables(lat, lon, [(0, 23, 0, 4)], ring=True)
    xlen = np.deg2rad(lon[-1] + 15.0) - np.deg2rad(lon[0])
    ylen = np.sin(np.deg2rad(50.0)) - np.sin(np.deg2rad(-50.0))
    assert t.ring and t.lon_uniform and t.nxb_max == 24 and t.nyb_max == 5
    assert np.allclose(t.boxtab[0], [1.0 / xlen, xlen / 24, 24 / 360.0, 0.0], rtol=1e-15, atol=0)
    assert np.allclose(t.boxtab2[0], [-1.0 / (RE * xlen * ylen), -1.0 / (RE * ylen), xlen, ylen], rtol=1e-15, atol=0)
    assert abs(xlen - 2 * np.pi) < 1e-14
    assert not t.wlon.any() and not t.glon.any()
    plain = tables.build_box_tables(lat, lon, [(0, 23, 0, 4)])
    assert not plain.ring and np.array_equal(plain.lattab, t.lattab) and np.array_equal(plain.lattab2, t.lattab2)
    assert plain.boxtab[0, 0] != t.boxtab[0, 0]            # the limited area's xlength leaves out the closing interval
    # the two refusals: an axis that is no ring (ring_error's text), a box that is not the whole axis
    short = -180.0 + 10.0 * np.arange(24)
    with pytest.raises(ValueError) as e:
        tables.build_box_tables(lat, short, [(0, 23, 0, 4)], ring=True)
    assert ring_error(short) and ring_error(short) in str(e.value)
    for box in ([(1, 23, 0, 4)], [(0, 22, 0, 4)], [(0, 23, 0, 4), (0, 23, 0, 4)]):
        with pytest.raises(ValueError) as e:
            tables.build_box_tables(lat, lon, box, ring=True)
        assert "whole longitude axis" in str(e.value)


def test_ring_call_is_additive():
    lib = _lib.load()
    assert "lec_rowstats_ring" in _lib.EXPORTS and lib.lec_rowstats_ring is not None
    hdr = open(os.path.join(ROOT, "include", "lec_hip.h")).read()
    assert "int lec_rowstats_ring(const lec_rowstats_args* args);" in hdr
    assert _lib.LEC_ABI_VERSION == 11 and lib.lec_version() == 11 and "#define LEC_ABI_VERSION 11" in hdr
    A = _lib.RowstatsArgs
    assert ctypes.sizeof(A) == 6 * 8 + 14 * 4 + 9 * 8 + 8 * 4 + 2 * 8
    offs = {n: getattr(A, n).offset for n, _ in A._fields_}
    assert offs["tair_d"] == 0 and offs["dtype"] == 48 and offs["box_per_step"] == 96 and offs["reserved0"] == 100 and offs["box_d"] == 104
    assert offs["rows_d"] == 160 and offs["stream"] == 168 and offs["tuning"] == 176 and offs["tm_d"] == 208 and offs["tp_d"] == 216
    assert re.search(r"int32_t reserved0;\s*/\* must be 0 \*/", hdr)


def _valid_ring_args():
    """Scalars of a valid ring call over fake (never dereferenced) pointers: every refusal is made on the scalars, before any HIP call."""
    fake = ctypes.c_void_p(0x10000)
    a = _lib.RowstatsArgs()
    a.tair_d = a.u_d = a.v_d = a.omega_d = a.geopt_d = a.rows_d = a.box_d = a.boxtab_d = a.lattab_d = a.levtab_d = a.tcoef_d = fake
    a.dtype, a.with_q = _lib.LEC_F64, 1
    a.nt, a.nl, a.ny, a.nx, a.t_begin, a.t_count = 3, 4, 5, 16, 0, 3
    a.n_box, a.nxb_max, a.nyb_max, a.lon_uniform, a.box_per_step = 1, 16, 5, 1, 0
    return a, fake


@pytest.mark.parametrize("field, change", [
    ("box_per_step", lambda a, f: (setattr(a, "box_per_step", 1), setattr(a, "n_box", 3))),
    ("n_box", lambda a, f: setattr(a, "n_box", 2)),
    ("lon_uniform", lambda a, f: setattr(a, "lon_uniform", 0)),
    ("tm_d", lambda a, f: setattr(a, "tm_d", f)),
    ("tp_d", lambda a, f: setattr(a, "tp_d", f)),
    ("nxb_max", lambda a, f: setattr(a, "nxb_max", 2)),
])
def test_c_call_refuses_what_a_ring_is_not(field, change):
    lib = _lib.load()
    a, fake = _valid_ring_args()
    change(a, fake)
    assert lib.lec_rowstats_ring(ctypes.byref(a)) == 1          # LEC_ERR_ARG
    msg = lib.lec_last_error()
    assert msg.startswith(b"lec_rowstats_ring") and field.encode() in msg, msg


def test_c_call_refuses_other_kernel_families_and_null():
    lib = _lib.load()
    assert lib.lec_rowstats_ring(None) == 1 and b"null args" in lib.lec_last_error()
    for k in (_lib.KERNEL_TWO_SWEEP, _lib.KERNEL_ROW_BLOCK, _lib.KERNEL_BOX_TILE, _lib.KERNEL_BOX_PLANE):
        a, _ = _valid_ring_args()
        a.tuning.kernel = k
        assert lib.lec_rowstats_ring(ctypes.byref(a)) == 2      # LEC_ERR_UNSUPPORTED
        msg = lib.lec_last_error()
        assert b"lec_rowstats_ring" in msg and b"ring form" in msg and b"tuning.kernel" in msg, msg
    a, _ = _valid_ring_args()                                    # what lec_rowstats checks is checked here too
    a.reserved0 = 1
    assert lib.lec_rowstats_ring(ctypes.byref(a)) == 1 and b"reserved0" in lib.lec_last_error()


# -- the command line -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["-t"], ["-c"], ["-t", "--trackfiles", "a"], ["-c", "--choose-systems", "2"]])
def test_cli_refuses_periodic_outside_the_fixed_framework(tmp_path, monkeypatch, flags):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", "--periodic", *flags])
    assert "--periodic goes with -f" in str(e.value)
    assert not os.path.exists(tmp_path / "LEC_Results")          # refused before anything was created


def _cli_workdir(tmp_path, monkeypatch, limits):
    import logging
    os.makedirs(tmp_path / "inputs")
    (tmp_path / "inputs" / "namelist").write_text(rr.RING_NAMELIST)
    (tmp_path / "inputs" / "box_limits").write_text("min_lon;%s\nmax_lon;%s\nmin_lat;-30\nmax_lat;30\n" % limits)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(logging.getLogger("lorenzcycletoolkit"), "handlers", [])


def _level_tables(tmp_path, stem):
    d = tmp_path / "LEC_Results" / f"{stem}_fixed" / "results_vertical_levels"
    return os.listdir(d) if os.path.isdir(d) else []


def test_cli_refuses_a_file_that_is_no_ring(tmp_path, monkeypatch):
    import lorenzcycletoolkit
    _cli_workdir(tmp_path, monkeypatch, (-180, 180))
    rr.write_ring_file(str(tmp_path / "arc.nc"), rr.cli_domain(step=10.0))      # 24 columns of 10 degrees: 240, not 360
    with pytest.raises(ValueError) as e:
        lorenzcycletoolkit.main([str(tmp_path / "arc.nc"), "-r", "-f", "--periodic", "--ingest", "host"])
    assert "--periodic needs a full ring of longitudes" in str(e.value) and "240.0 degrees" in str(e.value)
    assert not _level_tables(tmp_path, "arc")                    # nothing that looks like a result is left


def test_cli_refuses_limits_that_do_not_span_the_ring(tmp_path, monkeypatch):
    """The crop of the fixed framework follows inputs/box_limits, so limits short of the axis leave an arc: no ring.  Limits that the
    crop spans but the box does not (--box_limits FILE) name the two longitudes found."""
    import lorenzcycletoolkit
    _cli_workdir(tmp_path, monkeypatch, (-180, 180))
    rr.write_ring_file(str(tmp_path / "ring.nc"), rr.cli_domain())
    (tmp_path / "part").write_text("min_lon;-150\nmax_lon;120\nmin_lat;-30\nmax_lat;30\n")
    with pytest.raises(ValueError) as e:
        lorenzcycletoolkit.main([str(tmp_path / "ring.nc"), "-r", "-f", "--periodic", "--ingest", "host", "--box_limits", str(tmp_path / "part")])
    assert "-150.0 and 120.0" in str(e.value) and "part of a circle does not exist" in str(e.value)
    assert not _level_tables(tmp_path, "ring")
    (tmp_path / "inputs" / "box_limits").write_text("min_lon;-150\nmax_lon;120\nmin_lat;-30\nmax_lat;30\n")
    with pytest.raises(ValueError) as e:
        lorenzcycletoolkit.main([str(tmp_path / "ring.nc"), "-r", "-f", "--periodic", "--ingest", "host"])
    assert "--periodic needs a full ring of longitudes" in str(e.value)
