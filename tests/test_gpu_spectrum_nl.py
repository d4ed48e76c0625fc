"""-f --periodic --wavenumbers N --wavenumbers-interactions on the GPU: ``lec_rowspec_nl_ring`` against NumPy's FFT of the restatement's
tendencies and eddies of the same rows (tests/spectrum_nl_restatement.py), the closure of its shares on the total it sums in physical
space, and ``LECEngine.compute(..., wavenumbers=N, spectrum_interactions=True)`` / the command line against the CPU restatement.  Grids
of 3 steps x 4 levels (the top, interior and bottom d/dp) x 5 latitudes (both one-sided d/dlat rows) on ``ring_restatement.ring_domain``
from -60 to 60 degrees.

Widths and N of the record test.  The list of tests/test_gpu_spectrum_ge.py: 3 / 1, 4 / 2 (Nyquist, weight 1), 8 / 4, 65 / 32, 128 / 64,
129 / 64, 130 / 5, 130 / 33 (N divides 256 and N does not), 130 / 15 and 130 / 16 and 2050 / 20 and 4096 / 16 (the twiddle table in LDS
from N = 16 up to 4096 columns).  The kernel stages a row in trips of L = 768 columns and reads a column's lambda neighbours at wrapped
indices: 768 (one full trip), 769 (one column into a second), 1542 / 7 (three trips).  fp32 storage: 256, 257 (the restatement is fed
the float32-rounded fields as fp64).  45 rows: an odd count, for a kernel form that serves two rows per workgroup.  One level (no engine exists
for one level: the C call itself, over records that carry the rows' means; every d/dp coefficient is 0) and two levels (both d/dp
one-sided).  A band of rows 1 .. 5 in a cube of 7 latitudes whose rows 0 and 6 are NaN: the one-sided rows read nothing outside the band.

Bars.  Records: 1e-9 of the largest |share| of the case (the project's record bar).  Closure of the shares on the total and of S(n),
L(n) on theirs: 1e-11 of the largest share (the project's bar for term closure; the restatement alone, on the CPU, closes its rows to
1.8e-15 and its terms to 2.2e-14, well inside it; its two routes through the energy operator agree to 2.6e-15 of the largest share:
tests/test_spectrum_nl_cpu.py).  Terms against the restatement: 1e-9 of scale.  Rotation: 1e-11.  Triads: 1e-12 of the largest share;
one wavenumber alone: 1e-12 of max|A| max|x'| (the restatement alone: 7.6e-15)."""
import ctypes as C
import os
import shutil

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib, tables
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests import spectrum_nl_restatement as nr
from tests import spectrum_restatement as sr
from tests.helpers import as_f64

DEV = "cuda:0"
NT, NL, NY = 3, 4, 5
SOUTH, NORTH = -60.0, 60.0
TOL = 1e-9
TRIP = 768                  # kChunk of lec_rowspec_nl.hip
RECORD_CASES = [(3, 1, np.float64), (4, 2, np.float64), (8, 4, np.float64), (65, 32, np.float64), (128, 64, np.float64), (129, 64, np.float64),
                (130, 5, np.float64), (130, 33, np.float64), (130, 15, np.float64), (130, 16, np.float64), (2050, 20, np.float64),
                (4096, 16, np.float64), (TRIP, 20, np.float64), (TRIP + 1, 20, np.float64), (2 * TRIP + 6, 7, np.float64),
                (256, 20, np.float32), (257, 20, np.float32)]
RECORD_IDS = [f"{nx}-N{n}-{np.dtype(d).name}" for nx, n, d in RECORD_CASES]

_doms, _refs = {}, {}


def _dom(nx, dtype=np.float64):
    key = (nx, np.dtype(dtype).name)
    if key not in _doms:
        _doms[key] = rr.ring_domain(NT, NL, NY, nx, seed=nx, dtype=dtype, lat0=SOUTH, lat1=NORTH)
    return _doms[key]


def _reference(nx, n, dtype=np.float64):
    """The restatement's (nl, rest, levels, total) of one case, computed once and shared."""
    key = (nx, n, np.dtype(dtype).name)
    if key not in _refs:
        _refs[key] = nr.nl_terms(as_f64(_dom(nx, dtype)), SOUTH, NORTH, n)
    return _refs[key]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _engine(dom, band=None):
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    js, jn = band or (0, dom.lat.size - 1)
    return eng, eng.prepare_boxes([(0, dom.lon.size - 1, js, jn)], ring=True)


def _fields(dom):
    return [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]


def _compute(dom, n, interactions=True, **kw):
    eng, pb = _engine(dom)
    return eng.compute(*_fields(dom), pb, time_s=dom.time_s, keep_rows=True, wavenumbers=n, spectrum_interactions=interactions, **kw)


def _rowspec_nl(dom, n, band=None):
    """(nlspec [.., N, 8], nltot [.., 8]) of the engine's call over the ring pass's own records."""
    eng, pb = _engine(dom, band)
    f = _fields(dom)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    spec, tot = eng.rowspec_nl(*f[:4], rows, pb, n)
    return spec.cpu().numpy(), tot.cpu().numpy()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _record_err(got, ref, what):
    """Worst |difference| of the shares and of the totals, of the largest |share|; slots 3 .. 7 must be 0."""
    (spec, tot), (shares, totals) = got, ref
    assert spec.shape == shares.shape[:-1] + (8,) and tot.shape == totals.shape[:-1] + (8,), what
    assert not spec[..., 3:].any() and not tot[..., 3:].any(), what
    scale = np.abs(shares).max()
    err, terr = np.abs(spec[..., :3] - shares).max() / scale, np.abs(tot[..., :3] - totals).max() / scale
    print(f"records {what}: shares {err:.2e}, totals {terr:.2e} of the largest share")
    return max(err, terr)


# -- 1. records -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx, n, dtype", RECORD_CASES, ids=RECORD_IDS)
def test_records(nx, n, dtype):
    """nlspec_d and nltot_d against NumPy: rfft of the restatement's A_x and x', C_n as defined."""
    dom = _dom(nx, dtype)
    got = _rowspec_nl(dom, n)
    assert got[0].shape == (NT, NL, NY, n, 8) and got[1].shape == (NT, NL, NY, 8)
    assert _record_err(got, nr.row_shares(as_f64(dom), SOUTH, NORTH, n), f"nx={nx} N={n} {np.dtype(dtype).name}") <= TOL


@pytest.mark.parametrize("n", [7, 20])
def test_records_odd_row_count(n):
    """3 steps x 3 levels x 5 latitudes = 45 rows: with two rows per workgroup (kRows = 2) the last workgroup serves one row."""
    dom = rr.ring_domain(NT, 3, NY, 65, seed=3, lat0=SOUTH, lat1=NORTH)
    assert _record_err(_rowspec_nl(dom, n), nr.row_shares(dom, SOUTH, NORTH, n), f"45 rows, N={n}") <= TOL


def test_records_two_levels():
    """nl = 2: d/dp is one-sided at both levels."""
    dom = rr.ring_domain(NT, 2, NY, 65, seed=4, lat0=SOUTH, lat1=NORTH)
    assert _record_err(_rowspec_nl(dom, 20), nr.row_shares(dom, SOUTH, NORTH, 20), "two levels") <= TOL


def test_records_one_level():
    """nl = 1: the pressure derivative vanishes (``tables.pressure_coefs``: all 0).  No engine exists for one level, so this is the C
    call itself; its records carry the zonal means of the rows (the plain mean over the ring's columns, what the ring pass writes)."""
    nx, n = 65, 20
    dom = rr.ring_domain(NT, 1, NY, nx, seed=8, lat0=SOUTH, lat1=NORTH)
    bt = tables.build_box_tables(dom.lat, dom.lon, [(0, nx - 1, 0, NY - 1)], ring=True)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega)]
    rows = torch.zeros((NT, 1, NY, _lib.LEC_NSTAT), dtype=torch.float64, device=DEV)
    for s, a in enumerate(f):
        rows[..., s] = a.mean(dim=-1)
    twid, lattab = _dev(tables.twiddle_table(nx)), _dev(tables.nl_lat_table(bt.lattab[0], dom.lat))
    ptab = _dev(tables.pressure_coefs(dom.level))
    assert not tables.pressure_coefs(dom.level).any()
    spec = torch.full((NT, 1, NY, n, 8), np.nan, dtype=torch.float64, device=DEV)
    tot = torch.full((NT, 1, NY, 8), np.nan, dtype=torch.float64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    a = _lib.RowspecNlArgs(tair_d=p(f[0]), u_d=p(f[1]), v_d=p(f[2]), omega_d=p(f[3]), dtype=_lib.LEC_F64, nt=NT, nl=1, ny=NY, nx=nx, t_begin=0,
                           t_count=NT, js=0, jn=NY - 1, n_wave=n, rows_d=p(rows), twid_d=p(twid), lattab_d=p(lattab), ptab_d=p(ptab),
                           inv_hdeg=float(bt.boxtab[0, 2]), nlspec_d=p(spec), nltot_d=p(tot),
                           stream=C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    _lib.check(_lib.load().lec_rowspec_nl_ring(C.byref(a)), "lec_rowspec_nl_ring")
    torch.cuda.synchronize()
    assert _record_err((spec.cpu().numpy(), tot.cpu().numpy()), nr.row_shares(dom, SOUTH, NORTH, n), "one level") <= TOL


def test_records_band_inside_a_taller_cube():
    """Rows 1 .. 5 of a cube of 7 latitudes whose rows 0 and 6 are NaN: finite, and the restatement's on the cropped domain."""
    nx, n = 130, 20
    full = rr.ring_domain(NT, NL, 7, nx, seed=6, lat0=-75.0, lat1=75.0)
    crop = o.Domain(*[np.ascontiguousarray(a[:, :, 1:6]) for a in (full.tair, full.u, full.v, full.omega, full.geopt)],
                    full.lat[1:6], full.lon, full.level, full.time_s)
    holed = [a.copy() for a in (full.tair, full.u, full.v, full.omega, full.geopt)]
    for a in holed:
        a[:, :, 0] = np.nan
        a[:, :, 6] = np.nan
    dom = o.Domain(*holed, full.lat, full.lon, full.level, full.time_s)
    got = _rowspec_nl(dom, n, band=(1, 5))
    assert got[0].shape == (NT, NL, 5, n, 8) and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert _record_err(got, nr.row_shares(crop, float(crop.lat[0]), float(crop.lat[-1]), n), "band 1..5 of 7 rows") <= TOL


# -- 2. closure on the shipped kernel ---------------------------------------------------------------------------------------------
def _check_closure(res, spec, tot, what):
    """The shares of a row sum to the total the kernel formed in physical space, and S(n), L(n) to theirs, on the finite entries; NaN
    sits at the same places."""
    s3, t3 = spec[..., :3], tot[..., :3]
    assert np.array_equal(np.isnan(s3), np.broadcast_to(np.isnan(t3)[..., None, :], s3.shape)), what
    with np.errstate(invalid="ignore"):
        err = np.nanmax(np.abs(s3.sum(axis=3) - t3)) / np.nanmax(np.abs(s3))
    nl_, rest, total = res.spectrum_nl.cpu().numpy(), res.spectrum_nl_rest.cpu().numpy(), res.spectrum_nl_total.cpu().numpy()
    assert np.array_equal(np.isnan(rest), np.isnan(total)), what
    with np.errstate(invalid="ignore"):
        rerr = (np.nanmax(np.abs(rest), axis=0) / np.nanmax(np.abs(nl_), axis=(0, 2))).max()
    print(f"{what}: rows close to {err:.2e}, S and L to {rerr:.2e} of the largest share")
    assert err <= 1e-11, (what, err)
    assert rerr <= 1e-11, (what, rerr)


@pytest.mark.parametrize("nx", [8, 65, 128, 129])
def test_closure(nx):
    """With N = nx // 2 the shares of every row sum to nltot_d (Parseval: the kernel checks itself) and S(n), L(n) to their totals."""
    dom = _dom(nx)
    spec, tot = _rowspec_nl(dom, nx // 2)
    _check_closure(_compute(dom, nx // 2), spec, tot, f"closure nx={nx}")


# -- 3. terms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx, n, dtype", [(16, 8, np.float64), (130, 20, np.float64), (260, 20, np.float32)], ids=["16-N8", "130-N20", "260-N20-float32"])
def test_terms(nx, n, dtype):
    """spectrum_nl, spectrum_nl_rest and spectrum_nl_levels (and the total) against the restatement."""
    res = _compute(_dom(nx, dtype), n)
    nl_, rest, levels, total = _reference(nx, n, dtype)
    got, got_rest = res.spectrum_nl.cpu().numpy(), res.spectrum_nl_rest.cpu().numpy()
    got_levels, got_total = res.spectrum_nl_levels.cpu().numpy(), res.spectrum_nl_total.cpu().numpy()
    assert got.shape == (NT, 2, n) and got_rest.shape == (NT, 2) and got_levels.shape == (NT, 2, n, NL) and got_total.shape == (NT, 2)
    assert np.isfinite(got).all() and np.isfinite(got_levels).all() and np.isfinite(got_rest).all()
    for i, term in enumerate(nr.TERMS):
        scale = max(np.abs(nl_[:, i]).max(), np.abs(total[:, i]).max())
        e_nl = np.abs(got[:, i] - nl_[:, i]).max() / scale
        # the rest is a difference of the total and the shares: judged against the scale of what is subtracted
        e_rest = max(np.abs(got_rest[:, i] - rest[:, i]).max(), np.abs(got_total[:, i] - total[:, i]).max()) / scale
        e_lev = np.abs(got_levels[:, i] - levels[:, i]).max() / np.abs(levels[:, i]).max()
        print(f"terms nx={nx} N={n} {np.dtype(dtype).name}: {term}(n) {e_nl:.2e}, rest {e_rest:.2e}, levels {e_lev:.2e} of scale")
        assert e_nl <= TOL and e_rest <= TOL and e_lev <= TOL


# -- 4. triads --------------------------------------------------------------------------------------------------------------------
def test_planted_triad():
    """Eddies at the wavenumbers 2, 3 and 5 on 24 columns (2 + 3 = 5: a triad): the tendencies hold many wavenumbers, yet x' has power
    at 2, 3 and 5 only, so every share elsewhere vanishes, in the records and in S(n), L(n)."""
    nx, waves = 24, [2, 3, 5]
    dom = nr.planted_domain(nx, waves)
    res = _compute(dom, nx // 2)
    spec, _ = _rowspec_nl(dom, nx // 2)
    own = [m - 1 for m in waves]
    for name, a, axis in (("records", spec[..., :3], 3), ("S, L", res.spectrum_nl.cpu().numpy(), 2)):
        mine, other = np.abs(np.take(a, own, axis=axis)), np.abs(np.delete(a, own, axis=axis)).max()
        assert (mine.max(axis=tuple(k for k in range(a.ndim) if k != axis)) > 0).all(), name
        print(f"planted triad, {name}: shares outside 2, 3, 5 at most {other / mine.max():.2e} of the largest")
        assert other <= 1e-12 * mine.max(), name


def test_one_wavenumber_alone():
    """Eddies of one wavenumber m alone: A_x holds 0 and 2 m, x' holds m: no wavenumber receives anything."""
    nx, m = 24, 3
    dom = nr.planted_domain(nx, [m])
    _, X, A = nr.tendencies(dom, SOUTH, NORTH)
    scale = max(np.abs(a).max() * np.abs(x).max() for a, x in zip(A, X))
    spec, tot = _rowspec_nl(dom, nx // 2)
    worst = max(np.abs(spec).max(), np.abs(tot).max()) / scale
    print(f"one wavenumber alone: largest share {worst:.2e} of max|A| max|x'|")
    assert worst <= 1e-12


# -- 5. rotation ------------------------------------------------------------------------------------------------------------------
def test_rotation():
    """Rolled by 5 columns, every share stays: the ring's seam moves through the lambda stencil and the staging trips."""
    dom = _dom(130)
    a, b = _compute(dom, 20), _compute(rr.rolled(dom, 5), 20)
    for name in ("spectrum_nl", "spectrum_nl_levels", "spectrum_nl_total"):
        x, y = getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()
        err = np.abs(y - x).max() / np.abs(x).max()
        print(f"rotation by 5: {name} {err:.2e} of scale")
        assert err <= 1e-11, name


# -- 6. NaN -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["interior level of one step", "bottom level"])
def test_nan(where):
    """T is NaN on a few columns (the two cases of test_gpu_spectrum_ge.test_nan, six levels): the shares are NaN exactly at the rows
    the restatement's are -- the row, its latitude neighbours and its pressure neighbours, for T's share and, through nothing, for no
    other --, slots 3 .. 7 stay 0, and the closure holds on what is finite."""
    nx, nl = 65, 6
    src = rr.ring_domain(NT, nl, NY, nx, seed=nx, lat0=SOUTH, lat1=NORTH)
    T = src.tair.copy()
    if where == "bottom level":
        T[:, nl - 1, 1:3, 10:14] = np.nan
    else:
        T[1, 2, 1:3, 10:14] = np.nan
    dom = o.Domain(T, src.u, src.v, src.omega, src.geopt, src.lat, src.lon, src.level, src.time_s)
    spec, tot = _rowspec_nl(dom, nx // 2)
    shares, totals = nr.row_shares(dom, SOUTH, NORTH, nx // 2)
    assert np.isnan(shares).any() and np.isfinite(shares).any()
    assert np.array_equal(np.isnan(spec[..., :3]), np.isnan(shares)) and np.array_equal(np.isnan(tot[..., :3]), np.isnan(totals))
    assert not spec[..., 3:].any() and not tot[..., 3:].any()
    # the rows, spelled out: T's share is NaN at the rows 0 .. 3 (1, 2 and their latitude neighbours) of the levels around the hole
    bad = np.isnan(spec[..., 0, 0])
    want = np.zeros_like(bad)
    if where == "bottom level":
        want[:, nl - 1, 0:4] = True
        want[:, nl - 2, 1:3] = True
    else:
        want[1, 2, 0:4] = True
        want[1, 1, 1:3] = True
        want[1, 3, 1:3] = True
    assert np.array_equal(bad, want) and not np.isnan(spec[..., 1:3]).any()
    with np.errstate(invalid="ignore"):
        assert np.nanmax(np.abs(spec[..., :3] - shares)) <= TOL * np.nanmax(np.abs(shares))
    res = _compute(dom, nx // 2)
    assert int(res.nanflag.sum()) > 0
    _check_closure(res, spec, tot, f"NaN at the {where}")


# -- 7. nothing else moves --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generation", [False, True], ids=["plain", "with-generation"])
@pytest.mark.parametrize("nx, dtype", [(130, np.float64), (260, np.float32)], ids=["130", "260-float32"])
def test_nothing_else_moves(nx, dtype, generation):
    dom = _dom(nx, dtype)
    res, plain = _compute(dom, 20, spectrum_generation=generation), _compute(dom, 20, interactions=False, spectrum_generation=generation)
    for name in ("spectrum_nl", "spectrum_nl_total", "spectrum_nl_rest", "spectrum_nl_levels"):
        assert getattr(plain, name) is None and getattr(res, name) is not None, name
    assert _same_bits(res.scalars, plain.scalars) and _same_bits(res.levels, plain.levels) and torch.equal(res.nanflag, plain.nanflag)
    assert _same_bits(res.rows[..., :28], plain.rows[..., :28])       # (slots 28..31 are stage 1's scratch, not an interface)
    assert _same_bits(res.spectrum, plain.spectrum) and _same_bits(res.spectrum_rest, plain.spectrum_rest)
    assert _same_bits(res.spectrum_levels, plain.spectrum_levels)
    if generation:
        assert _same_bits(res.spectrum_ge, plain.spectrum_ge) and _same_bits(res.spectrum_ge_rest, plain.spectrum_ge_rest)
        assert _same_bits(res.spectrum_ge_levels, plain.spectrum_ge_levels)
    else:
        assert res.spectrum_ge is None and plain.spectrum_ge is None
    eng, pb = _engine(dom)
    with pytest.raises(ValueError):
        eng.compute(*_fields(dom), pb, time_s=dom.time_s, spectrum_interactions=True)


# -- 8. time chunks ---------------------------------------------------------------------------------------------------------------
def test_time_chunks_give_the_same_bits(monkeypatch):
    """The interactions run in time chunks of their own records ([tc, nl, nyb, N + 1, 8]): one step per chunk, and two steps and a
    shorter last chunk, give the bits of the whole series at once."""
    dom = _dom(130)
    whole = _compute(dom, 20)
    eng, _ = _engine(dom)
    assert eng.spectrum_nl_chunk_steps(NT, NL, NY, 20) == NT
    for chunk, steps in ((1, 1), (2 * NL * NY * 21 * 64, 2)):
        monkeypatch.setattr(LECEngine, "SPECTRUM_CHUNK_BYTES", chunk)
        assert eng.spectrum_nl_chunk_steps(NT, NL, NY, 20) == steps
        parts = _compute(dom, 20)
        for name in ("spectrum_nl", "spectrum_nl_total", "spectrum_nl_rest", "spectrum_nl_levels", "spectrum"):
            assert _same_bits(getattr(parts, name), getattr(whole, name)), (chunk, name)


# -- 9, 10. the command line, resident and streamed -------------------------------------------------------------------------------
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


@pytest.fixture
def ring_file(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    (tmp_path / "inputs" / "namelist").write_text(rr.RING_NAMELIST)
    (tmp_path / "inputs" / "box_limits").write_text("min_lon;-180\nmax_lon;180\nmin_lat;-30\nmax_lat;30\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    dom = rr.cli_domain()
    path = str(tmp_path / "ring.nc")
    rr.write_ring_file(path, dom)
    return path, dom


FLAGS = ["-r", "-f", "--periodic", "--wavenumbers", "4"]
NEW = [os.path.join("ring_fixed", "results_wavenumbers", f"{t}_n.csv") for t in ("L", "S")]


def test_cli_streamed_writes_the_resident_bytes(ring_file):
    """--wavenumbers-chunk 2: S_n.csv and L_n.csv (and every other file) byte for byte those of the resident run."""
    path, _ = ring_file
    want, _ = _main([path] + FLAGS + ["--wavenumbers-interactions"])
    got, log = _main([path] + FLAGS + ["--wavenumbers-interactions", "--wavenumbers-chunk", "2"])
    assert "lec_level_spec_ring" in log and "lec_rowspec_nl_kernel: N = 4, nx = 24" in log
    assert sorted(got) == sorted(want) and all(k in got for k in NEW)
    for k in want:
        assert got[k] == want[k], f"{k} differs from the resident run's"


def test_cli_wavenumbers_interactions(ring_file):
    """-r -f --periodic --wavenumbers 4 --wavenumbers-interactions: S_n.csv and L_n.csv beside their five siblings, their shape, header,
    time labels and the restatement's numbers; every other file of the tree is byte-identical to the run with --wavenumbers 4 alone."""
    path, dom = ring_file
    plain, plain_log = _main([path] + FLAGS)
    tree, log = _main([path] + FLAGS + ["--wavenumbers-interactions"])
    assert sorted(k for k in tree if "results_wavenumbers" in k) == sorted(
        os.path.join("ring_fixed", "results_wavenumbers", f"{t}_n.csv") for t in sr.TERMS + nr.TERMS)
    assert sorted(set(tree) - set(plain)) == NEW and set(plain) <= set(tree)
    for k in plain:
        assert tree[k] == plain[k], f"{k} differs from the run without --wavenumbers-interactions"
    assert "lec_rowspec_nl_kernel: N = 4, nx = 24" in log and "lec_rowspec_kernel: N = 4, nx = 24" in log
    assert "lec_rowspec_nl_kernel" not in plain_log and "wavenumbers_interactions" not in plain_log
    crop = o.crop_domain(dom, -180, 180, -30, 30)
    nl_, rest, _, _ = nr.nl_terms(crop, -30, 30, 4)
    labels = [line.split(",")[0] for line in tree[os.path.join("ring_fixed", "results_vertical_levels", "Ae_level.csv")].decode().splitlines()]
    for i, term in enumerate(nr.TERMS):
        name = os.path.join("ring_fixed", "results_wavenumbers", f"{term}_n.csv")
        lines = tree[name].decode().splitlines()
        assert lines[0] == "time,1,2,3,4,rest" and len(lines) == 1 + len(dom.time_s)
        assert [line.split(",")[0] for line in lines[1:]] == labels[1:]                  # the time labels of the per-level tables
        import io
        df = pd.read_csv(io.BytesIO(tree[name]), index_col=0)
        assert df.shape == (len(dom.time_s), 5)
        worst = max(np.abs(df.values[:, :4] - nl_[:, i]).max(), np.abs(df["rest"].values - rest[:, i]).max()) / np.abs(nl_[:, i]).max()
        print(f"cli --wavenumbers-interactions: {term}_n.csv worst {worst:.2e} of scale")
        assert worst <= TOL
