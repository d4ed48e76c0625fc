"""-f --periodic --wavenumbers N --wavenumbers-budget on the GPU: ``lec_rowspec_b_ring`` against NumPy's FFT of the same rows' products
(tests/spectrum_b_restatement.py), the closure of its shares on slots 16, 17, 20, 21 of the ring pass's records, ``lec_level_spec_b_ring``
against the assembled form, and ``LECEngine.compute(..., wavenumbers=N, spectrum_budget=True)``, the streamed path and the command line
against the CPU restatement and the run's own totals.  Grids of 3 or 4 steps x 4 levels x 5 latitudes on
``ring_restatement.ring_domain`` from -60 to 60 degrees; bands of 66 rows for the level kernel of tall bands.

Widths and N of the record test.  The kernel stages a row in trips of L = 576 columns: 576 (one full trip), 577 (one column into a
second), 1158 (three trips).  nx odd (65, 129), 8 / 4 (Nyquist, weight 1), 130 / 15 and 130 / 16 (the twiddle table in LDS from N = 16),
130 / 5 and 130 / 33 (N divides 256 and N does not), 128 / 64, 4100 / 16 (past the 4096 columns of the LDS table; two rows, one level),
fp32 storage 256 and 257.  One and three levels; a band of exactly two rows (both walls); a band inside a taller cube whose outer rows
are NaN.  At every interior row slots 0 and 2 must be exactly 0.0.

Bars (the siblings', tests/test_gpu_spectrum_nl.py).  Against the restatement: 1e-9 of the largest share.  Closures -- the shares of a
row on the record's slot, sum_n X(n) + rest on the run's totals --, rotation and the planted waves' product identity: 1e-11 of the largest
share; what must vanish: 1e-12 of the largest."""
import argparse
import ctypes as C
import io
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
from tests import spectrum_b_restatement as br
from tests import spectrum_nl_restatement as nr
from tests.helpers import as_f64

DEV = "cuda:0"
NT, NL, NY = 3, 4, 5
SOUTH, NORTH = -60.0, 60.0
TOL, CLOSE = 1e-9, 1e-11
TRIP = 576                  # kChunk of lec_rowspec_b.hip
SLOTS = (16, 17, 20, 21)
RECORD_CASES = [(8, 4, np.float64), (65, 32, np.float64), (128, 64, np.float64), (129, 64, np.float64), (130, 5, np.float64),
                (130, 33, np.float64), (130, 15, np.float64), (130, 16, np.float64), (TRIP, 20, np.float64), (TRIP + 1, 20, np.float64),
                (2 * TRIP + 6, 7, np.float64), (256, 20, np.float32), (257, 20, np.float32)]
RECORD_IDS = [f"{nx}-N{n}-{np.dtype(d).name}" for nx, n, d in RECORD_CASES]
BUDGET_FIELDS = ("spectrum_b", "spectrum_b_rest", "spectrum_tendency", "spectrum_tendency_rest", "spectrum_residual", "spectrum_residual_rest")

_doms, _refs, _runs = {}, {}, {}


def _dom(nx, dtype=np.float64, nt=NT, ny=NY):
    key = (nx, np.dtype(dtype).name, nt, ny)
    if key not in _doms:
        _doms[key] = rr.ring_domain(nt, NL, ny, nx, seed=nx, dtype=dtype, lat0=SOUTH, lat1=NORTH)
    return _doms[key]


def _reference(nx, n, nt=NT):
    """The restatement's budget of one case, computed once and shared."""
    if (nx, n, nt) not in _refs:
        _refs[(nx, n, nt)] = br.budget_terms(_dom(nx, nt=nt), SOUTH, NORTH, n)
    return _refs[(nx, n, nt)]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _engine(dom, band=None):
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    js, jn = band or (0, dom.lat.size - 1)
    return eng, eng.prepare_boxes([(0, dom.lon.size - 1, js, jn)], ring=True)


def _fields(dom):
    return [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]


def _compute(dom, n, budget=True, **kw):
    eng, pb = _engine(dom)
    return eng.compute(*_fields(dom), pb, time_s=dom.time_s, keep_rows=True, wavenumbers=n, spectrum_budget=budget, **kw)


def _shared_run(nx, n, nt=NT):
    """compute(..., spectrum_budget=True) of one case (the assembled form), run once and shared; nothing changes it."""
    if (nx, n, nt) not in _runs:
        _runs[(nx, n, nt)] = _compute(_dom(nx, nt=nt), n)
    return _runs[(nx, n, nt)]


def _rowspec_b(dom, n, band=None):
    """(bspec [.., N, 4], the ring pass's records) of the engine's call."""
    eng, pb = _engine(dom, band)
    f = _fields(dom)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    return eng.rowspec_b(*f[:4], rows, pb, n).cpu().numpy(), rows.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _record_err(bspec, shares, what):
    """Worst |difference| of the four slots of the largest |share| of the slot: every slot at the band's first and last row, slots 1
    and 3 elsewhere, where slots 0 and 2 must be exactly 0.0."""
    assert bspec.shape == shares.shape, what
    inner = bspec[:, :, 1:-1]
    assert not inner[..., 0].any() and not inner[..., 2].any() and not np.signbit(inner[..., 0]).any() and not np.signbit(inner[..., 2]).any(), what
    err = 0.0
    for s in range(4):
        rows = slice(None) if s in (1, 3) else [0, bspec.shape[2] - 1]
        got, ref = bspec[..., s][:, :, rows], shares[..., s][:, :, rows]
        err = max(err, np.abs(got - ref).max() / np.abs(ref).max())
    print(f"records {what}: {err:.2e} of the largest share")
    return err


def _band(dom, js=0, jn=None):
    jn = dom.lat.size - 1 if jn is None else jn
    return [as_f64_array(a[:, :, js:jn + 1]) for a in (dom.tair, dom.u, dom.v, dom.omega)]


def as_f64_array(a):
    return np.asarray(a, dtype=np.float64)


# -- 1. records -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx, n, dtype", RECORD_CASES, ids=RECORD_IDS)
def test_records(nx, n, dtype):
    """bspec_d against NumPy: rfft of the products and fields of the same rows, C_n as defined."""
    dom = _dom(nx, dtype)
    bspec, _ = _rowspec_b(dom, n)
    assert bspec.shape == (NT, NL, NY, n, 4)
    assert _record_err(bspec, br.row_shares(*_band(dom), n), f"nx={nx} N={n} {np.dtype(dtype).name}") <= TOL


def _direct(dom, n, band):
    """The C call itself over records that carry the rows' zonal means (no engine exists for one level)."""
    nt, nl, ny, nx = dom.tair.shape
    js, jn = band
    nyb = jn - js + 1
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega)]
    rows = torch.zeros((nt, nl, nyb, _lib.LEC_NSTAT), dtype=torch.float64, device=DEV)
    for s, a in enumerate(f):
        rows[..., s] = a[:, :, js:jn + 1].mean(dim=-1)
    twid = _dev(tables.twiddle_table(nx))
    bspec = torch.full((nt, nl, nyb, n, 4), np.nan, dtype=torch.float64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    a = _lib.RowspecBArgs(tair_d=p(f[0]), u_d=p(f[1]), v_d=p(f[2]), omega_d=p(f[3]), dtype=_lib.LEC_F64, nt=nt, nl=nl, ny=ny, nx=nx, t_begin=0,
                          t_count=nt, js=js, jn=jn, n_wave=n, rows_d=p(rows), twid_d=p(twid), bspec_d=p(bspec),
                          stream=C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    _lib.check(_lib.load().lec_rowspec_b_ring(C.byref(a)), "lec_rowspec_b_ring")
    torch.cuda.synchronize()
    return bspec.cpu().numpy()


def test_records_one_level():
    dom = rr.ring_domain(NT, 1, NY, 65, seed=8, lat0=SOUTH, lat1=NORTH)
    assert _record_err(_direct(dom, 20, (0, NY - 1)), br.row_shares(*_band(dom), 20), "one level") <= TOL


def test_records_past_the_lds_table():
    """4100 columns: the twiddle table stays in memory at N = 16 (the LDS table ends at 4096); two rows, one level, eight trips."""
    dom = rr.ring_domain(2, 1, 2, 4100, seed=9, lat0=-10.0, lat1=10.0)
    assert _record_err(_direct(dom, 16, (0, 1)), br.row_shares(*_band(dom), 16), "nx=4100 N=16") <= TOL


def test_records_three_levels():
    dom = rr.ring_domain(NT, 3, NY, 65, seed=4, lat0=SOUTH, lat1=NORTH)
    bspec, _ = _rowspec_b(dom, 20)
    assert _record_err(bspec, br.row_shares(*_band(dom), 20), "three levels") <= TOL


def test_records_band_of_two_rows():
    """A band of exactly two rows: both are walls, every slot is computed."""
    dom = _dom(130)
    bspec, _ = _rowspec_b(dom, 20, band=(2, 3))
    assert bspec.shape == (NT, NL, 2, 20, 4) and (bspec != 0).all()
    assert _record_err(bspec, br.row_shares(*_band(dom, 2, 3), 20), "band of two rows") <= TOL


def test_records_band_inside_a_taller_cube():
    """Rows 1 .. 5 of a cube of 7 latitudes whose rows 0 and 6 are NaN: finite, and the shares of the band's own rows."""
    nx, n = 130, 20
    full = rr.ring_domain(NT, NL, 7, nx, seed=6, lat0=-75.0, lat1=75.0)
    holed = [a.copy() for a in (full.tair, full.u, full.v, full.omega, full.geopt)]
    for a in holed:
        a[:, :, 0] = np.nan
        a[:, :, 6] = np.nan
    dom = o.Domain(*holed, full.lat, full.lon, full.level, full.time_s)
    bspec, _ = _rowspec_b(dom, n, band=(1, 5))
    assert bspec.shape == (NT, NL, 5, n, 4) and np.isfinite(bspec).all()
    assert _record_err(bspec, br.row_shares(*_band(full, 1, 5), n), "band 1..5 of 7 rows") <= TOL


# -- 2. Parseval ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [8, 65, 128, 129])
def test_parseval(nx):
    """With N = nx // 2 the shares of a row sum to slots 16, 17, 20, 21 of the ring pass's record: the kernel's own check."""
    bspec, rows = _rowspec_b(_dom(nx), nx // 2)
    err = 0.0
    for s, slot in enumerate(SLOTS):
        r = slice(None) if s in (1, 3) else [0, NY - 1]
        err = max(err, np.abs(bspec[..., s][:, :, r].sum(axis=3) - rows[:, :, r, slot]).max() / np.abs(bspec[..., s][:, :, r]).max())
    print(f"parseval nx={nx}: the shares sum to the record's slots to {err:.2e} of the largest share")
    assert err <= CLOSE


# -- 3. stage 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny", [5, 66], ids=["band-of-5-small-kernel", "band-of-66-tall-kernel"])
def test_fused_equals_assembled(ny):
    """``lec_level_spec_b_ring`` against the assembled records through ``lec_reduce``: every result field, bit for bit."""
    dom = _dom(24, ny=ny)
    asm, fused = _compute(dom, 8, spectrum_generation=True), _compute(dom, 8, spectrum_generation=True, spectrum_fused=True)
    for name in BUDGET_FIELDS + ("spectrum", "spectrum_rest", "spectrum_levels", "spectrum_ge", "scalars", "levels"):
        assert _same_bits(getattr(fused, name), getattr(asm, name)), name
    assert np.isfinite(asm.spectrum_b.cpu().numpy()).all() and (asm.spectrum_b != 0).all()


@pytest.mark.parametrize("ny", [5, 66], ids=["band-of-5-small-kernel", "band-of-66-tall-kernel"])
def test_replicated_slots_reproduce_level_spec_ring(ny):
    """bspec_d holding the records' own slots 16, 17, 20, 21 for every n: the bits of ``lec_level_spec_ring``."""
    dom, n = _dom(24, ny=ny), 8
    eng, pb = _engine(dom)
    f = _fields(dom)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    spec = eng.rowspec(*f[:4], pb, n)
    own = rows[..., list(SLOTS)].unsqueeze(3).expand(-1, -1, -1, n, -1).contiguous()
    f64 = dict(dtype=torch.float64, device=DEV)
    want, got = torch.zeros((n, NT, NL, _lib.LEC_NLEVRAW), **f64), torch.ones((n, NT, NL, _lib.LEC_NLEVRAW), **f64)
    eng.spectrum_level_stage(rows, spec, None, pb, want)
    eng.spectrum_level_stage(rows, spec, None, pb, got, bspec=own)
    assert _same_bits(got, want)
    # ... and the shares move the boundary sums alone
    other = torch.ones_like(got)
    eng.spectrum_level_stage(rows, spec, None, pb, other, bspec=eng.rowspec_b(*f[:4], rows, pb, n))
    assert not _same_bits(other, want) and _same_bits(other[..., :15], want[..., :15])
    with pytest.raises(ValueError, match="bspec"):
        eng.spectrum_level_stage(rows, spec, None, pb, got, bspec=own[..., :3])


# -- 4. terms ---------------------------------------------------------------------------------------------------------------------
def _term_errs(res, ref, what):
    worst = 0.0
    for field, key in (("spectrum_b", "b"), ("spectrum_tendency", "tendency"), ("spectrum_residual", "residual")):
        got, got_rest = getattr(res, field).cpu().numpy(), getattr(res, field + "_rest").cpu().numpy()
        want, want_rest = ref[key], ref[key + "_rest"]
        assert got.shape == want.shape and got_rest.shape == want_rest.shape, field
        for i in range(2):
            scale = max(np.abs(want[:, i]).max(), np.abs(want[:, i].sum(axis=1) + want_rest[:, i]).max())
            e, e_rest = np.abs(got[:, i] - want[:, i]).max() / scale, np.abs(got_rest[:, i] - want_rest[:, i]).max() / scale
            print(f"{what}: {field}[{i}] {e:.2e}, rest {e_rest:.2e} of scale")
            worst = max(worst, e, e_rest)
    return worst


def _totals_errs(res, time_s, what):
    """sum_n X(n) + rest against the run's own totals: BAe, BKe, the tendencies of Ae and Ke, RGe and RKe."""
    tot = tables.budgets_and_residuals({k: v for k, v in res.scalars_dict().items()}, time_s)
    worst = 0.0
    for field, names in (("spectrum_b", ("BAe", "BKe")), ("spectrum_tendency", ("∂Ae/∂t (finite diff.)", "∂Ke/∂t (finite diff.)")),
                         ("spectrum_residual", ("RGe", "RKe"))):
        got, rest = getattr(res, field).cpu().numpy(), getattr(res, field + "_rest").cpu().numpy()
        for i, name in enumerate(names):
            scale = max(np.abs(got[:, i]).max(), np.abs(tot[name]).max())
            e = np.abs(got[:, i].sum(axis=1) + rest[:, i] - tot[name]).max() / scale
            print(f"{what}: sum_n + rest closes on {name} to {e:.2e} of scale")
            worst = max(worst, e)
    return worst


@pytest.mark.parametrize("nx, n, nt", [(16, 8, 4), (130, 20, 3)], ids=["16-N8", "130-N20"])
def test_terms(nx, n, nt):
    res = _shared_run(nx, n, nt)
    for name in BUDGET_FIELDS:
        assert np.isfinite(getattr(res, name).cpu().numpy()).all(), name
    assert res.spectrum_b.shape == (nt, 2, n) and res.spectrum_residual_rest.shape == (nt, 2)
    assert _term_errs(res, _reference(nx, n, nt), f"terms nx={nx} N={n}") <= TOL
    assert _totals_errs(res, _dom(nx, nt=nt).time_s, f"terms nx={nx} N={n}") <= CLOSE


def test_terms_float32_storage():
    dom = _dom(260, np.float32)
    res = _compute(dom, 20)
    ref = br.budget_terms(as_f64(dom), SOUTH, NORTH, 20)
    assert _term_errs(res, ref, "terms nx=260 N=20 float32") <= TOL
    assert _totals_errs(res, dom.time_s, "terms nx=260 N=20 float32") <= CLOSE


# -- 5. NaN -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["lowest level", "wall row"])
def test_nan(where):
    """A NaN point at the lowest level: [w T'T'] and the shares of that row are NaN, _handle_nans drops the level and the bottom-minus-top
    difference moves to the level above, as for the totals.  A NaN row at the south wall of an interior level: the wall's shares are NaN
    there and the level is repaired along p.  The four slots are NaN for every n exactly where the record's slot is."""
    nx, nl, n = 65, 6, 20
    src = rr.ring_domain(4, nl, NY, nx, seed=nx, lat0=SOUTH, lat1=NORTH)
    T, v = src.tair.copy(), src.v.copy()
    if where == "lowest level":
        T[:, nl - 1, 2, 10] = np.nan
    else:
        v[1, 2, 0, :] = np.nan
    dom = o.Domain(T, src.u, v, src.omega, src.geopt, src.lat, src.lon, src.level, src.time_s)
    bspec, rows = _rowspec_b(dom, n)
    for s, slot in enumerate(SLOTS):
        r = slice(None) if s in (1, 3) else [0, NY - 1]
        bad = np.isnan(rows[:, :, r, slot])
        assert np.array_equal(np.isnan(bspec[..., s][:, :, r]), np.broadcast_to(bad[..., None], bad.shape + (n,))), (where, slot)
    assert not bspec[:, :, 1:-1, :, 0].any() and not bspec[:, :, 1:-1, :, 2].any()
    assert np.isnan(bspec).any() and np.isfinite(bspec).any()
    res = _compute(dom, n)
    assert int(res.nanflag.sum()) > 0
    for name in BUDGET_FIELDS:
        assert np.isfinite(getattr(res, name).cpu().numpy()).all(), name
    with np.errstate(invalid="ignore"):
        ref = br.budget_terms(dom, SOUTH, NORTH, n)
    assert _term_errs(res, ref, f"NaN at the {where}") <= TOL
    assert _totals_errs(res, dom.time_s, f"NaN at the {where}") <= CLOSE


# -- 6. rotation ------------------------------------------------------------------------------------------------------------------
def test_rotation():
    """Rolled by 5 columns, every share stays: the ring's seam moves through the staging trips."""
    a, b = _shared_run(130, 20), _compute(rr.rolled(_dom(130), 5), 20)
    for name in ("spectrum_b", "spectrum_tendency", "spectrum_residual"):
        x, y = getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()
        err = (np.abs(y - x).max(axis=(0, 2)) / np.abs(x).max(axis=(0, 2))).max()
        print(f"rotation by 5: {name} {err:.2e} of scale")
        assert err <= CLOSE, name


# -- 7. planted waves -------------------------------------------------------------------------------------------------------------
def test_planted_waves():
    """Eddies of T and u at the wavenumbers 2, 3 and 5 on 24 columns, v and w zonally uniform: VTT(n) = [v] C_n(T, T), WTT(n) =
    [w] C_n(T, T), EV(n) = [v] C_n(u, u), EW(n) = [w] C_n(u, u) (v' = 0), and nothing at any other n."""
    nx, waves = 24, [2, 3, 5]
    p = nr.planted_domain(nx, waves)
    zm = lambda a: np.ascontiguousarray(np.broadcast_to(a.mean(axis=-1, keepdims=True), a.shape))
    dom = o.Domain(p.tair, p.u, zm(p.v), zm(p.omega), p.geopt, p.lat, p.lon, p.level, p.time_s)
    eng, pb = _engine(dom)
    f = _fields(dom)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    bspec = eng.rowspec_b(*f[:4], rows, pb, nx // 2).cpu().numpy()
    spec = eng.rowspec(*f[:4], pb, nx // 2).cpu().numpy()
    mV, mW = dom.v[..., 0][..., None], dom.omega[..., 0][..., None]
    want = np.stack([mV * spec[..., 0], mW * spec[..., 0], mV * (spec[..., 1] + spec[..., 2]), mW * (spec[..., 1] + spec[..., 2])], axis=-1)
    want[:, :, 1:-1, :, 0] = 0.0
    want[:, :, 1:-1, :, 2] = 0.0
    own = [m - 1 for m in waves]
    for s in range(4):
        r = slice(None) if s in (1, 3) else [0, NY - 1]
        got, ref = bspec[..., s][:, :, r], want[..., s][:, :, r]
        big = np.abs(ref).max()
        err, other = np.abs(got - ref).max() / big, np.abs(np.delete(got, own, axis=3)).max() / big
        print(f"planted waves, {br.SLOTS[s]}: the product identity to {err:.2e}, outside 2, 3, 5 at most {other:.2e} of the largest")
        assert big > 0 and (np.abs(np.take(got, own, axis=3)).max(axis=(0, 1, 2)) > 0).all()
        assert err <= CLOSE and other <= 1e-12


# -- 8. chunks, and nothing else moves --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["assembled", "fused"])
def test_time_chunks_give_the_same_bits(fused, monkeypatch):
    """One step per chunk, and two steps and a shorter last chunk, give the bits of the whole series at once."""
    dom, n = _dom(130), 20
    whole = _shared_run(130, 20)
    per_step = NL * NY * n * (96 if fused else _lib.LEC_NSTAT * 8)
    eng, _ = _engine(dom)
    assert eng.spectrum_chunk_steps(NT, NL, NY, n, True) == NT
    for chunk, steps in ((1, 1), (2 * per_step, 2)):
        monkeypatch.setattr(LECEngine, "SPECTRUM_CHUNK_BYTES", chunk)
        if fused:
            assert eng.spectrum_chunk_steps(NT, NL, NY, n, True) == steps
        parts = _compute(dom, n, spectrum_fused=fused)
        for name in BUDGET_FIELDS + ("spectrum", "spectrum_rest", "spectrum_levels"):
            assert _same_bits(getattr(parts, name), getattr(whole, name)), (chunk, name)


@pytest.mark.parametrize("fused", [False, True], ids=["assembled", "fused"])
def test_nothing_else_moves(fused):
    dom = _dom(130)
    res = _compute(dom, 20, spectrum_generation=True, spectrum_interactions=True, spectrum_fused=fused)
    plain = _compute(dom, 20, budget=False, spectrum_generation=True, spectrum_interactions=True, spectrum_fused=fused)
    for name in BUDGET_FIELDS:
        assert getattr(plain, name) is None and getattr(res, name) is not None, name
    assert torch.equal(res.nanflag, plain.nanflag) and _same_bits(res.rows[..., :28], plain.rows[..., :28])
    for name in ("scalars", "levels", "spectrum", "spectrum_rest", "spectrum_levels", "spectrum_ge", "spectrum_ge_rest", "spectrum_ge_levels",
                 "spectrum_nl", "spectrum_nl_total", "spectrum_nl_rest", "spectrum_nl_levels"):
        assert _same_bits(getattr(res, name), getattr(plain, name)), name
    eng, pb = _engine(dom)
    with pytest.raises(ValueError, match="spectrum_budget"):
        eng.compute(*_fields(dom), pb, time_s=dom.time_s, spectrum_budget=True)


# -- 9. the streamed series -------------------------------------------------------------------------------------------------------
@pytest.fixture
def workdir(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    (tmp_path / "inputs" / "namelist").write_text(rr.RING_NAMELIST)
    (tmp_path / "inputs" / "box_limits").write_text(f"min_lon;-180\nmax_lon;180\nmin_lat;{SOUTH}\nmax_lat;{NORTH}\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return tmp_path


@pytest.mark.parametrize("chunk_steps", [1, 2])
def test_streamed_equals_resident(chunk_steps, workdir):
    """``ingest.lec_streamed(..., ring=True, wavenumbers=N, spectrum_budget=True)``: the bits of the resident run."""
    from lorenzcycletoolkit_amd import dataset as ds
    from lorenzcycletoolkit_amd import ingest
    nx, n, nt = 130, 20, 5
    dom = _dom(nx, nt=nt)
    whole = _shared_run(nx, n, nt)
    path = str(workdir / "ring.nc")
    rr.write_ring_file(path, dom)
    df = ds.read_namelist("inputs/namelist")
    raw = ds.open_raw(path, df)
    try:
        plan = ingest.make_plan(raw, argparse.Namespace(fixed=True, track=False, trackfile=None, residuals=True))
        stats = {}
        st = ingest.lec_streamed(raw, plan, df, [(-180.0, 180.0, SOUTH, NORTH)], device=DEV, chunk_steps=chunk_steps, stats=stats, ring=True,
                                 wavenumbers=n, spectrum_budget=True)
        torch.cuda.synchronize()
    finally:
        raw.close()
    assert stats["chunks"] >= 2 and stats["spectrum_buffer_bytes"] == chunk_steps * NL * NY * n * (64 + 32)
    for name in BUDGET_FIELDS + ("scalars", "levels", "spectrum", "spectrum_rest", "spectrum_levels"):
        assert _same_bits(getattr(st, name), getattr(whole, name)), f"chunks of {chunk_steps}: {name} differs from the resident call"


# -- 10. the command line ---------------------------------------------------------------------------------------------------------
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
def ring_file(workdir):
    (workdir / "inputs" / "box_limits").write_text("min_lon;-180\nmax_lon;180\nmin_lat;-30\nmax_lat;30\n")
    dom = rr.cli_domain()
    path = str(workdir / "ring.nc")
    rr.write_ring_file(path, dom)
    return path, dom


FLAGS = ["-r", "-f", "--periodic", "--wavenumbers", "4"]
FILES = {"BAe": ("b", 0), "BKe": ("b", 1), "dAedt": ("tendency", 0), "dKedt": ("tendency", 1), "RGe": ("residual", 0), "RKe": ("residual", 1)}
NEW = sorted(os.path.join("ring_fixed", "results_wavenumbers", f"{t}_n.csv") for t in FILES)


def test_cli_wavenumbers_budget(ring_file):
    """-r -f --periodic --wavenumbers 4 --wavenumbers-budget: the six files beside their five siblings, their shape, header, time labels
    and the restatement's numbers; every other file of the tree is byte-identical to the run with --wavenumbers 4 alone; the streamed
    run (--wavenumbers-chunk 2) writes the resident run's bytes."""
    path, dom = ring_file
    plain, plain_log = _main([path] + FLAGS)
    tree, log = _main([path] + FLAGS + ["--wavenumbers-budget"])
    assert sorted(set(tree) - set(plain)) == NEW and set(plain) <= set(tree)
    for k in plain:
        assert tree[k] == plain[k], f"{k} differs from the run without --wavenumbers-budget"
    assert "lec_rowspec_b_kernel: N = 4, nx = 24" in log and "lec_rowspec_kernel: N = 4, nx = 24" in log
    assert "lec_rowspec_b_kernel" not in plain_log and "wavenumbers_budget=" not in plain_log        # (the Namespace line; the work directory carries the test's name)
    streamed, slog = _main([path] + FLAGS + ["--wavenumbers-budget", "--wavenumbers-chunk", "2"])
    assert "lec_rowspec_b_kernel: N = 4, nx = 24" in slog and sorted(streamed) == sorted(tree)
    for k in tree:
        assert streamed[k] == tree[k], f"{k} of the streamed run differs from the resident run's"
    crop = o.crop_domain(dom, -180, 180, -30, 30)
    ref = br.budget_terms(crop, -30, 30, 4)
    labels = [line.split(",")[0] for line in tree[os.path.join("ring_fixed", "results_vertical_levels", "Ae_level.csv")].decode().splitlines()]
    for term, (key, i) in FILES.items():
        name = os.path.join("ring_fixed", "results_wavenumbers", f"{term}_n.csv")
        lines = tree[name].decode().splitlines()
        assert lines[0] == "time,1,2,3,4,rest" and len(lines) == 1 + len(dom.time_s)
        assert [line.split(",")[0] for line in lines[1:]] == labels[1:]                  # the time labels of the per-level tables
        df = pd.read_csv(io.BytesIO(tree[name]), index_col=0)
        assert df.shape == (len(dom.time_s), 5)
        want, want_rest = ref[key][:, i], ref[key + "_rest"][:, i]
        scale = max(np.abs(want).max(), np.abs(want.sum(axis=1) + want_rest).max())
        worst = max(np.abs(df.values[:, :4] - want).max(), np.abs(df["rest"].values - want_rest).max()) / scale
        print(f"cli --wavenumbers-budget: {term}_n.csv worst {worst:.2e} of scale")
        assert worst <= TOL


def test_cli_refuses_a_series_of_one_step(workdir):
    (workdir / "inputs" / "box_limits").write_text("min_lon;-180\nmax_lon;180\nmin_lat;-30\nmax_lat;30\n")
    dom = rr.cli_domain(nt=1)
    path = str(workdir / "one.nc")
    rr.write_ring_file(path, dom)
    import lorenzcycletoolkit
    with pytest.raises((SystemExit, ValueError)) as e:
        lorenzcycletoolkit.main([path] + FLAGS + ["--wavenumbers-budget"])
    assert "at least 2 time steps" in str(e.value)
    shutil.rmtree("LEC_Results", ignore_errors=True)
