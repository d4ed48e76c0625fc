"""-f --periodic --wavenumbers on the GPU: ``lec_rowspec_ring`` against NumPy's FFT of the same rows, the closure of its shares on
the records ``lec_rowstats_ring`` writes, and ``LECEngine.compute(..., wavenumbers=N)`` / the command line against the CPU restatement
(tests/spectrum_restatement.py).  Grids of 3 steps x 4 levels x 5 latitudes on ``ring_restatement.ring_domain``.

Widths and N of the record test.  The issue's list: 3 / 1, 4 / 2 (Nyquist, weight 1), 7, 8, 64, 65, 128 / 64 (whole spectrum with
Nyquist), 129 / 64 (whole, odd), 130 / 64 (partial), 130 / 1, 130 / 5.  The kernel's own: a workgroup of 256 threads gives wavenumber n
the 256 // N column classes i = seg (mod 256 // N), so the lane mapping changes with N -- N that divides 256 (1, 2, 4, 32, 64: no idle
thread) and N that does not (3, 5, 7, 20, 33: 256 - N (256 // N) threads only stage data), fewer columns than classes (nx = 3, 130 with
N = 1: 256 classes) -- and the row is staged in LDS in trips of 512 columns: 512 (one full trip), 513 (one column into a second), 1030
(three trips, a class stride of 36 that divides neither 512 nor 1030).  The twiddle table is read from LDS when N >= 16 and nx <= 4096,
from memory otherwise (same values, same order): N = 15 / 16 at 130 columns, 2050 columns with N = 20 (more than 64 KiB of LDS per
workgroup), 4096 / 4098 with N = 16.  A workgroup serves two rows: ``test_records_odd_row_count`` runs 45 rows, so the last
workgroup has one.  fp32 storage: 256, 257, 258, 260 (the comparison is fed the float32-rounded fields as fp64).

Bars.  Records: 1e-9 of each slot's scale (the largest |C_n| of the slot over the case), the bar of tests/test_gpu_ring.py.  Closure
of the shares on the ring pass's covariances: 1e-12 of the same scale; of the terms: |rest| <= 1e-11 of the term's scale (the largest
|value| over time and n).  Terms against the restatement: 1e-9 of scale.  Rotation: 1e-11.  Planted wave: 1e-12 of the n = 3 share."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd.constants import SCALAR_TERMS, LEVEL_TERMS
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests import spectrum_restatement as sr
from tests.helpers import as_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lorenzcycletoolkit.py")
DEV = "cuda:0"
NT, NL, NY = 3, 4, 5
SOUTH, NORTH = -60.0, 60.0
TOL = 1e-9
RECORD_CASES = [(3, 1, np.float64), (4, 2, np.float64), (7, 3, np.float64), (8, 4, np.float64), (64, 32, np.float64), (65, 32, np.float64),
                (128, 64, np.float64), (129, 64, np.float64), (130, 64, np.float64), (130, 1, np.float64), (130, 5, np.float64),
                (65, 7, np.float64), (130, 33, np.float64), (512, 20, np.float64), (513, 20, np.float64), (1030, 7, np.float64),
                (130, 15, np.float64), (130, 16, np.float64), (2050, 20, np.float64), (4096, 16, np.float64), (4098, 16, np.float64),
                (256, 20, np.float32), (257, 20, np.float32), (258, 64, np.float32), (260, 64, np.float32)]
RECORD_IDS = [f"{nx}-N{n}-{np.dtype(d).name}" for nx, n, d in RECORD_CASES]
TERM_IDX = [SCALAR_TERMS.index(x) for x in sr.TERMS]
TABLE_IDX = [LEVEL_TERMS.index(x) for x in sr.LEVEL_TERMS]

_doms, _refs = {}, {}


def _dom(nx, dtype=np.float64):
    key = (nx, np.dtype(dtype).name)
    if key not in _doms:
        _doms[key] = rr.ring_domain(NT, NL, NY, nx, seed=nx, dtype=dtype, lat0=SOUTH, lat1=NORTH)
    return _doms[key]


def _reference(nx, n, dtype=np.float64):
    """The restatement's (spectrum, rest, spectrum_levels, totals) of one case, computed once and shared."""
    key = (nx, n, np.dtype(dtype).name)
    if key not in _refs:
        _refs[key] = sr.spectrum_terms(as_f64(_dom(nx, dtype)), SOUTH, NORTH, n)
    return _refs[key]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _engine(dom):
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    return eng, eng.prepare_boxes([(0, dom.lon.size - 1, 0, dom.lat.size - 1)], ring=True)


def _compute(dom, n, **kw):
    eng, pb = _engine(dom)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    return eng.compute(*f, pb, time_s=dom.time_s, keep_rows=True, wavenumbers=n, **kw)


def _rowspec(dom, n):
    eng, pb = _engine(dom)
    return eng.rowspec(*[_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega)], pb, n).cpu().numpy()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _slot_scale(spec):
    """The largest |C_n| of every slot over the case ([8])."""
    return np.nanmax(np.abs(spec), axis=tuple(range(spec.ndim - 1)))


def _term_errs(got, ref, axes):
    """max |got - ref| over ``axes`` relative to the largest |ref| there (per term); NaN must sit at the same places."""
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    with np.errstate(invalid="ignore"):
        return np.nanmax(np.abs(got - ref), axis=axes) / np.nanmax(np.abs(ref), axis=axes)


# -- 1. records -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx, n, dtype", RECORD_CASES, ids=RECORD_IDS)
def test_records(nx, n, dtype):
    """spec_d against NumPy: rfft of the fp64 fields, C_n as defined."""
    dom = _dom(nx, dtype)
    got = _rowspec(dom, n)
    d64 = as_f64(dom)
    ref = sr.row_shares(d64.tair, d64.u, d64.v, d64.omega, n)
    assert got.shape == (NT, NL, NY, n, 8) == ref.shape
    err = np.abs(got - ref).max(axis=(0, 1, 2, 3)) / _slot_scale(ref)
    print(f"records nx={nx} N={n} {np.dtype(dtype).name}: worst {err.max():.2e} of scale (slot {6 + int(err.argmax())})")
    assert err.max() <= TOL, err


@pytest.mark.parametrize("n", [7, 20])
def test_records_odd_row_count(n):
    """3 steps x 3 levels x 5 latitudes = 45 rows: the last workgroup serves one row, not two."""
    dom = rr.ring_domain(NT, 3, NY, 65, seed=3, lat0=SOUTH, lat1=NORTH)
    got = _rowspec(dom, n)
    ref = sr.row_shares(dom.tair, dom.u, dom.v, dom.omega, n)
    assert got.shape == (NT, 3, NY, n, 8)
    err = np.abs(got - ref).max(axis=(0, 1, 2, 3)) / _slot_scale(ref)
    print(f"records, 45 rows, N={n}: worst {err.max():.2e} of scale")
    assert err.max() <= TOL, err


# -- 2. closure on the shipped kernel ---------------------------------------------------------------------------------------------
def _check_closure(res, spec, what):
    rows = res.rows.cpu().numpy()
    total = spec.sum(axis=3)                                # [t, k, j, 8]
    cov = rows[..., 6:14]
    assert np.array_equal(np.isnan(total), np.isnan(cov)), what
    with np.errstate(invalid="ignore"):
        err = np.nanmax(np.abs(total - cov), axis=(0, 1, 2)) / _slot_scale(spec)
    spectrum, rest = res.spectrum.cpu().numpy(), res.spectrum_rest.cpu().numpy()
    tot = res.scalars.cpu().numpy()[:, TERM_IDX]
    assert np.array_equal(np.isnan(rest), np.isnan(tot)), what
    with np.errstate(invalid="ignore"):
        rerr = np.nanmax(np.abs(rest), axis=0) / np.nanmax(np.abs(spectrum), axis=(0, 2))
    print(f"{what}: rows close to {err.max():.2e}, terms to {rerr.max():.2e} of scale")
    assert err.max() <= 1e-12, (what, err)
    assert rerr.max() <= 1e-11, (what, dict(zip(sr.TERMS, rerr)))


@pytest.mark.parametrize("nx", [8, 65, 128, 129])
def test_closure(nx):
    """With N = nx // 2 the shares sum to the covariances ``lec_rowstats_ring`` writes and the spectra to the totals."""
    dom = _dom(nx)
    res = _compute(dom, nx // 2)
    _check_closure(res, _rowspec(dom, nx // 2), f"closure nx={nx}")


# -- 3. terms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx, n, dtype", [(16, 8, np.float64), (130, 20, np.float64), (260, 20, np.float32)], ids=["16-N8", "130-N20", "260-N20-float32"])
def test_terms(nx, n, dtype):
    """spectrum, spectrum_rest and spectrum_levels against the restatement."""
    res = _compute(_dom(nx, dtype), n)
    spec, rest, levels, _ = _reference(nx, n, dtype)
    got = res.spectrum.cpu().numpy()
    assert got.shape == (NT, 5, n) and res.spectrum_rest.shape == (NT, 5) and res.spectrum_levels.shape == (NT, 14, n, NL)
    e_spec = _term_errs(got, spec, (0, 2))
    # the rest is a difference of the total and the shares: judged against the scale of what is subtracted
    e_rest = np.abs(res.spectrum_rest.cpu().numpy() - rest).max(axis=0) / np.abs(spec).max(axis=(0, 2))
    e_lev = _term_errs(res.spectrum_levels.cpu().numpy(), levels, (0, 2, 3))
    print(f"terms nx={nx} N={n} {np.dtype(dtype).name}: spectrum {e_spec.max():.2e}, rest {e_rest.max():.2e}, levels {e_lev.max():.2e} of scale")
    assert e_spec.max() <= TOL, dict(zip(sr.TERMS, e_spec))
    assert e_rest.max() <= TOL, dict(zip(sr.TERMS, e_rest))
    assert e_lev.max() <= TOL, dict(zip(sr.LEVEL_TERMS, e_lev))


# -- 4. rotation ------------------------------------------------------------------------------------------------------------------
def test_rotation():
    """A ring has no preferred meridian: rolled by 5 columns, every share stays."""
    dom = _dom(130)
    a, b = _compute(dom, 20), _compute(rr.rolled(dom, 5), 20)
    sa, sb = a.spectrum.cpu().numpy(), b.spectrum.cpu().numpy()
    err = np.abs(sb - sa).max(axis=(0, 2)) / np.abs(sa).max(axis=(0, 2))
    la, lb = a.spectrum_levels.cpu().numpy(), b.spectrum_levels.cpu().numpy()
    lerr = np.abs(lb - la).max(axis=(0, 2, 3)) / np.abs(la).max(axis=(0, 2, 3))
    print(f"rotation by 5: spectrum {err.max():.2e}, levels {lerr.max():.2e} of scale")
    assert err.max() <= 1e-11 and lerr.max() <= 1e-11


# -- 5. a planted wave ------------------------------------------------------------------------------------------------------------
def test_planted_wave():
    """Eddies of one wavenumber, m = 3 on 24 columns, no noise, smooth zonal means: every other share vanishes."""
    nx, m = 24, 3
    base = rr.ring_domain(NT, NL, NY, nx, seed=5, lat0=SOUTH, lat1=NORTH, noise=0.0)
    lam = np.deg2rad(base.lon)[None, None, None, :]
    phi = np.deg2rad(base.lat)[None, None, :, None]
    p = base.level[None, :, None, None] / 1e5
    tt = (np.arange(NT) / NT)[:, None, None, None]
    zm = lambda a: a.mean(axis=-1, keepdims=True)
    wave = lambda amp, ph: amp * np.cos(m * lam + ph + 0.3 * p + tt) * np.cos(phi)
    f = [np.ascontiguousarray(zm(a) + w) for a, w in ((base.tair, wave(4.0, 0.0)), (base.u, wave(6.0, 0.7)), (base.v, wave(5.0, 1.9)),
                                                     (base.omega, wave(0.2, 2.6)))]
    dom = o.Domain(f[0], f[1], f[2], f[3], base.geopt, base.lat, base.lon, base.level, base.time_s)
    res = _compute(dom, nx // 2)
    s = res.spectrum.cpu().numpy()
    own = np.abs(s[:, :, m - 1]).max(axis=0)
    other = np.abs(np.delete(s, m - 1, axis=2)).max(axis=(0, 2))
    assert np.all(own > 0)
    print(f"planted wave: other shares at most {(other / own).max():.2e} of the n = {m} share")
    assert np.all(other <= 1e-12 * own), dict(zip(sr.TERMS, other / own))
    rows = _rowspec(dom, nx // 2)
    scale = np.abs(rows[..., m - 1, :]).max(axis=(0, 1, 2))
    assert np.all(np.abs(np.delete(rows, m - 1, axis=3)).max(axis=(0, 1, 2, 3)) <= 1e-12 * scale)


# -- 6. NaN -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["interior level of one step", "bottom level"])
def test_nan(where):
    """T is NaN on a few columns: the shares are finite exactly where the totals are, the closure holds, and nothing of the totals moves.
    Six levels here: d/dp spreads a NaN level to its two neighbours, which on four levels leaves one level for _handle_nans and makes
    Ca 0 at every step -- nothing to close on."""
    nx, nl = 65, 6
    src = rr.ring_domain(NT, nl, NY, nx, seed=nx, lat0=SOUTH, lat1=NORTH)
    T = src.tair.copy()
    if where == "bottom level":
        T[:, nl - 1, 1:3, 10:14] = np.nan
    else:
        T[1, 2, 1:3, 10:14] = np.nan
    dom = o.Domain(T, src.u, src.v, src.omega, src.geopt, src.lat, src.lon, src.level, src.time_s)
    res = _compute(dom, nx // 2)
    eng, pb = _engine(dom)
    plain = eng.compute(*[_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)], pb, time_s=dom.time_s, keep_rows=True)
    assert torch.equal(res.nanflag, plain.nanflag) and int(res.nanflag.sum()) > 0
    assert _same_bits(res.scalars, plain.scalars) and _same_bits(res.levels, plain.levels) and _same_bits(res.rows[..., :28], plain.rows[..., :28])
    tot = res.scalars.cpu().numpy()[:, TERM_IDX]
    s = res.spectrum.cpu().numpy()
    assert np.array_equal(np.isfinite(s), np.broadcast_to(np.isfinite(tot)[:, :, None], s.shape))
    lv = res.levels.cpu().numpy()[:, TABLE_IDX]
    sl = res.spectrum_levels.cpu().numpy()
    assert np.array_equal(np.isfinite(sl), np.broadcast_to(np.isfinite(lv)[:, :, None, :], sl.shape))
    spec = _rowspec(dom, nx // 2)
    assert np.isnan(spec).any()
    _check_closure(res, spec, f"NaN at the {where}")


# -- 7. nothing else moves --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx, dtype", [(130, np.float64), (260, np.float32)], ids=["130", "260-float32"])
def test_nothing_else_moves(nx, dtype):
    dom = _dom(nx, dtype)
    res = _compute(dom, 20)
    eng, pb = _engine(dom)
    plain = eng.compute(*[_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)], pb, time_s=dom.time_s, keep_rows=True)
    assert plain.spectrum is None and plain.spectrum_rest is None and plain.spectrum_levels is None
    assert _same_bits(res.scalars, plain.scalars) and _same_bits(res.levels, plain.levels) and torch.equal(res.nanflag, plain.nanflag)
    assert _same_bits(res.rows[..., :28], plain.rows[..., :28])       # (slots 28..31 are stage 1's scratch, not an interface)
    with pytest.raises(ValueError):                                  # a spectrum exists on a ring only
        eng.compute(*[_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)], [(0, nx - 1, 0, NY - 1)], time_s=dom.time_s, wavenumbers=4)
    with pytest.raises(ValueError):
        eng.compute(*[_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)], pb, time_s=dom.time_s, wavenumbers=nx // 2 + 1)


def test_time_chunks_give_the_same_bits(monkeypatch):
    """Stage 2 of the spectra runs in time chunks: one step per chunk gives the bits of the whole series at once."""
    dom = _dom(130)
    whole = _compute(dom, 20)
    monkeypatch.setattr(LECEngine, "SPECTRUM_CHUNK_BYTES", 1)
    parts = _compute(dom, 20)
    assert _same_bits(parts.spectrum, whole.spectrum) and _same_bits(parts.spectrum_levels, whole.spectrum_levels)
    monkeypatch.setattr(LECEngine, "SPECTRUM_CHUNK_BYTES", 2 * 20 * NL * NY * 32 * 8)       # two steps, then a shorter last chunk
    parts = _compute(dom, 20)
    assert _same_bits(parts.spectrum, whole.spectrum) and _same_bits(parts.spectrum_levels, whole.spectrum_levels)


# -- 8. the command line ----------------------------------------------------------------------------------------------------------
def _run(argv, timeout=600):
    env = dict(os.environ, LEC_DIST_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "LEC_FORCE_SHARD"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, CLI] + argv, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r


def _tree(d):
    out = {}
    for base, _, files in os.walk(d):
        for f in files:
            if not f.startswith("log."):
                p = os.path.join(base, f)
                out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def test_cli_wavenumbers(tmp_path, monkeypatch):
    """-r -f --periodic --wavenumbers 4: the five files, their shape and header, the restatement's numbers; every other file of the tree
    is byte-identical to the run without the flag."""
    os.makedirs(tmp_path / "inputs")
    (tmp_path / "inputs" / "namelist").write_text(rr.RING_NAMELIST)
    (tmp_path / "inputs" / "box_limits").write_text("min_lon;-180\nmax_lon;180\nmin_lat;-30\nmax_lat;30\n")
    monkeypatch.chdir(tmp_path)
    dom = rr.cli_domain()
    path = str(tmp_path / "ring.nc")
    rr.write_ring_file(path, dom)
    results = tmp_path / "LEC_Results" / "ring_fixed"
    _run([path, "-r", "-f", "--periodic"])
    plain = _tree(results)
    shutil.rmtree(results)
    _run([path, "-r", "-f", "--periodic", "--wavenumbers", "4"])
    tree = _tree(results)
    new = sorted(set(tree) - set(plain))
    assert new == sorted(os.path.join("results_wavenumbers", f"{t}_n.csv") for t in sr.TERMS) and set(plain) <= set(tree)
    for k in plain:
        assert tree[k] == plain[k], f"{k} differs from the run without --wavenumbers"
    log = open(results / "log.ring").read()
    assert "lec_rowspec_kernel: N = 4, nx = 24" in log and "--ingest auto resolves to host" in log
    crop = o.crop_domain(dom, -180, 180, -30, 30)
    spec, rest, _, _ = sr.spectrum_terms(crop, -30, 30, 4)
    labels = [line.split(",")[0] for line in tree[os.path.join("results_vertical_levels", "Ae_level.csv")].decode().splitlines()]
    worst = {}
    for i, term in enumerate(sr.TERMS):
        text = tree[os.path.join("results_wavenumbers", f"{term}_n.csv")].decode()
        lines = text.splitlines()
        assert lines[0] == "time,1,2,3,4,rest" and len(lines) == 1 + len(dom.time_s)
        assert [line.split(",")[0] for line in lines[1:]] == labels[1:], term          # the time labels of the per-level tables
        df = pd.read_csv(results / "results_wavenumbers" / f"{term}_n.csv", index_col=0)
        assert df.shape == (len(dom.time_s), 5)
        scale = np.abs(spec[:, i]).max()
        worst[term] = max(np.abs(df.values[:, :4] - spec[:, i]).max(), np.abs(df["rest"].values - rest[:, i]).max()) / scale
    print(f"cli --wavenumbers: worst {max(worst.values()):.2e} of scale")
    assert max(worst.values()) <= TOL, worst
