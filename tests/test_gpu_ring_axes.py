"""The ring pass, the four spectra, the fused level-spectrum kernels, ``lec_sections`` and ``lec_maps`` on UNEVEN latitudes, levels and time
steps, on a band INSIDE a taller cube whose outer rows (and, for the open box, outer columns) are NaN, and with NaNs in u, omega and T at
once: the cases of tests/ring_axes_cases.py against the CPU restatements the sibling tests use (tests/test_gpu_ring.py,
test_gpu_spectrum*.py, test_gpu_sections.py, test_gpu_maps.py, test_gpu_rowstats_records.py).  On the siblings' even axes the middle
coefficient of every gradient triple is 0 and all interior triples are alike, so ``gb`` / ``be`` / ``tb`` of the Q stencils, ``grb`` / ``pb`` of
the maps' factors kernel, ``ptab`` and ``nl_lat_table`` multiply by zero and a table read at the wrong row, level or step goes unnoticed;
tests/test_ring_axes_cpu.py shows that the references used here move by 2e-3 to 1 of scale under such a defect.

Shapes (tests/ring_axes_cases.py): ``narrow`` 9 x 70 with the band on rows 1 .. 7 (a ring of 70: the maps' 64-column wave seam; the open
box is columns 3 .. 67), ``tall`` 68 x 16 with rows 1 .. 66 (a second 64-row trip, the tall level kernels), ``levels17`` 7 x 16 with 17
levels (two level batches of 8 plus one); 4 steps at hours 0, 1, 4, 6.  N = 8 wavenumbers, on ``narrow`` also 20 (the twiddle table in
LDS) and 35 = nx / 2 (Parseval).  One engine per domain and one compute per case, shared by the tests.

Bars, the siblings': 1e-9 of the term's scale (or of the largest share) against a restatement, 1e-11 for closures, bit for bit for the
fused form, the chunkings and the terms a NaN cannot reach, NaN patterns exactly the restatement's; the records by the measure of
tests/test_gpu_rowstats_records.py.  Every test prints its worst figure.
Measured on MI355X (worst over the cases): totals 7.1e-13; rowspec 1.1e-13, spectrum 3.3e-13, its levels 4.0e-13; rowspec_q 1.2e-14, Ge(n)
6.7e-15, its levels 2.0e-14; rowspec_nl 1.8e-14, S(n) 8.5e-14, L(n) 3.2e-15; rowspec_b 3.9e-13, BAe(n) 8.3e-14, tendencies and residuals
4.7e-13, their sums on the totals 2.3e-14; sections 2.0e-13, columns 1.9e-13 (with NaNs 3.9e-13), means 2.5e-13, closure on levels 1.4e-15, on
scalars 1.9e-15; spectral columns 2.4e-14, Parseval at N = 35 3.6e-15; map_steps 9.0e-14, map_lon 1.1e-13, map_mean 4.8e-14, closure on
section_lat 3.8e-15, on the scalars 8.1e-15; records 0.026 of the 1e-11 bar, means 0.027 of their bound; the fused form, the chunkings and
the 70 (field, term, step) slabs a NaN cannot reach: the same bits.  The module takes 5.9 s (39 tests, the slowest 0.8 s)."""
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib
from lorenzcycletoolkit_amd.constants import LEVEL_TERMS, MAP_TERMS, SCALAR_TERMS, SECTION_TERMS
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import maps_restatement as mr
from tests import ring_axes_cases as ra
from tests import ring_restatement as rr
from tests import sections_restatement as sr
from tests import spectrum_b_restatement as br
from tests import spectrum_ge_restatement as gr
from tests import spectrum_nl_restatement as nr
from tests import spectrum_restatement as spr
from tests import test_gpu_rowstats_records as rec
from tests import test_gpu_spectrum_b as tb
from tests import test_gpu_spectrum_nl as tn
from tests.helpers import as_f64, compare

DEV = "cuda:0"
TOL, CLOSE = 1e-9, 1e-11
N = 8
NT = ra.NT
WAVE_CASES = [("narrow", 8), ("narrow", 20), ("tall", 8), ("levels17", 8)]
WAVE_IDS = [f"{c}-N{n}" for c, n in WAVE_CASES]
SPEC_IDX = [SECTION_TERMS.index(k) for k in sr.SPEC_TERMS]

_engines, _setups, _runs = {}, {}, {}


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _engine(name):
    """One engine per domain (the axes are the domain's: every case on it shares them)."""
    if name not in _engines:
        dom = ra.clean(name)
        _engines[name] = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    return _engines[name]


def _setup(case_id):
    """(domain, its fp64 twin, box, engine, prepared box, the framed fields on the device), uploaded once per case."""
    if case_id not in _setups:
        dom, box, exp = ra.build(case_id)
        eng = _engine(ra.parse(case_id)[0])
        pb = eng.prepare_boxes([box], ring=True) if exp["ring"] else eng.prepare_boxes([box])
        _setups[case_id] = (dom, as_f64(dom), box, eng, pb, [_dev(getattr(dom, n)) for n in ra.FIELDS])
    return _setups[case_id]


def _run(case_id, n=N, fused=False):
    """``compute`` with everything the case can carry, run once per (case, N, form) and shared; nothing changes it."""
    key = (case_id, n, fused)
    if key not in _runs:
        dom, _, _, eng, pb, f = _setup(case_id)
        kw = dict(time_s=dom.time_s, keep_rows=True, sections=True, section_steps=True, maps=True, map_steps=True)
        if ra.build(case_id)[2]["ring"]:
            kw.update(wavenumbers=n, spectrum_generation=True, spectrum_interactions=True, spectrum_budget=True, spectrum_fused=fused)
        _runs[key] = eng.compute(*f, pb, **kw)
    return _runs[key]


def _band(case_id):
    """T, u, v, omega of the band as fp64 [T, nl, nyb, nx]."""
    _, d64, box, _, _, _ = _setup(case_id)
    return [a[:, :, box[2]:box[3] + 1] for a in (d64.tair, d64.u, d64.v, d64.omega)]


def _scale(ref, axes):
    """The term's scale: its largest finite |value| over ``axes`` (1.0 where the term has none)."""
    a = np.where(np.isnan(ref), -np.inf, np.abs(ref)).max(axis=axes, keepdims=True)
    return np.where(np.isfinite(a), a, 1.0)


def _close(got, ref, axes, what, tol=TOL):
    """|got - ref| <= tol * the term's scale, the NaN patterns equal; returns the largest error over scale."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern"
    err = np.nanmax(np.abs(got - ref) / _scale(ref, axes)) if np.isfinite(ref).any() else 0.0
    print(f"{what}: max error / scale = {err:.3e}")
    assert err <= tol, (what, err)
    return err


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


# -- 1. totals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ra.CLEAN_IDS)
def test_totals(name):
    """All scalars, level tables, budgets and residuals against ``ring_restatement.ring_terms`` of the band."""
    dom, d64, box, _, _, _ = _setup(name)
    res = _run(name)
    ref_s, ref_l = rr.ring_terms(d64, *ra.limits_of(dom, box))
    worst = compare(res.scalars_dict(), res.levels_dict(), o.budgets_and_residuals(ref_s, dom.time_s), ref_l, TOL, f"{name} totals", time_s=dom.time_s)
    print(f"{name} totals: worst {max(worst.values()):.2e} of scale ({max(worst, key=worst.get)})")
    assert int(res.nanflag.sum()) == 0 and np.isfinite(res.rows.cpu().numpy()[..., :28]).all()


# -- 2. the spectra ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, n", WAVE_CASES, ids=WAVE_IDS)
def test_linear_spectra(name, n):
    """``rowspec`` against NumPy's FFT of the band's rows; spectrum, rest and spectrum_levels against ``spectrum_terms``."""
    dom, d64, box, eng, pb, f = _setup(name)
    got = eng.rowspec(*f[:4], pb, n).cpu().numpy()
    ref = spr.row_shares(*_band(name), n)
    assert got.shape == ref.shape
    err = np.abs(got - ref).max(axis=(0, 1, 2, 3)) / np.abs(ref).max(axis=(0, 1, 2, 3))
    print(f"{name} N={n} rowspec: worst {err.max():.2e} of the slot's scale")
    assert err.max() <= TOL, err
    res = _run(name, n)
    spec, rest, levels, _ = spr.spectrum_terms(d64, *ra.limits_of(dom, box), n)
    _close(res.spectrum, spec, (0, 2), f"{name} N={n} spectrum")
    e_rest = (np.abs(res.spectrum_rest.cpu().numpy() - rest).max(axis=0) / np.abs(spec).max(axis=(0, 2))).max()
    print(f"{name} N={n} spectrum_rest: {e_rest:.2e} of the shares' scale")
    assert e_rest <= TOL
    _close(res.spectrum_levels, levels, (0, 2, 3), f"{name} N={n} spectrum_levels")


@pytest.mark.parametrize("name, n", WAVE_CASES, ids=WAVE_IDS)
def test_generation_spectrum(name, n):
    """``rowspec_q`` (gb, be, tb of its Q stencils) against the oracle's Q and T of the band's rows; Ge(n) against ``ge_terms``."""
    dom, d64, box, eng, pb, f = _setup(name)
    south, north = ra.limits_of(dom, box)
    got = eng.rowspec_q(*f[:4], pb, n, time_s=dom.time_s).cpu().numpy()
    ref = gr.row_shares_q(d64, south, north, n)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{name} N={n} rowspec_q: worst {err:.2e} of the largest share")
    assert err <= TOL
    res = _run(name, n)
    ge, rest, levels, _ = gr.ge_terms(d64, south, north, n)
    e_ge = np.abs(res.spectrum_ge.cpu().numpy() - ge).max() / np.abs(ge).max()
    e_rest = np.abs(res.spectrum_ge_rest.cpu().numpy() - rest).max() / np.abs(ge).max()
    e_lev = np.abs(res.spectrum_ge_levels.cpu().numpy() - levels).max() / np.abs(levels).max()
    print(f"{name} N={n}: Ge(n) {e_ge:.2e}, rest {e_rest:.2e}, levels {e_lev:.2e} of scale")
    assert e_ge <= TOL and e_rest <= TOL and e_lev <= TOL


@pytest.mark.parametrize("name, n", WAVE_CASES, ids=WAVE_IDS)
def test_interaction_spectra(name, n):
    """``rowspec_nl`` (ptab, nl_lat_table) against the restatement's tendencies and eddies; S(n), L(n) against ``nl_terms``."""
    dom, d64, box, eng, pb, f = _setup(name)
    south, north = ra.limits_of(dom, box)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    spec, tot = eng.rowspec_nl(*f[:4], rows, pb, n)
    assert tn._record_err((spec.cpu().numpy(), tot.cpu().numpy()), nr.row_shares(d64, south, north, n), f"{name} N={n} rowspec_nl") <= TOL
    res = _run(name, n)
    nl_, rest, levels, total = nr.nl_terms(d64, south, north, n)
    got, got_rest = res.spectrum_nl.cpu().numpy(), res.spectrum_nl_rest.cpu().numpy()
    got_levels, got_total = res.spectrum_nl_levels.cpu().numpy(), res.spectrum_nl_total.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(got_levels).all() and np.isfinite(got_rest).all()
    for i, term in enumerate(nr.TERMS):
        scale = max(np.abs(nl_[:, i]).max(), np.abs(total[:, i]).max())
        e_nl = np.abs(got[:, i] - nl_[:, i]).max() / scale
        e_rest = max(np.abs(got_rest[:, i] - rest[:, i]).max(), np.abs(got_total[:, i] - total[:, i]).max()) / scale
        e_lev = np.abs(got_levels[:, i] - levels[:, i]).max() / np.abs(levels[:, i]).max()
        print(f"{name} N={n}: {term}(n) {e_nl:.2e}, rest {e_rest:.2e}, levels {e_lev:.2e} of scale")
        assert e_nl <= TOL and e_rest <= TOL and e_lev <= TOL


@pytest.mark.parametrize("name, n", WAVE_CASES, ids=WAVE_IDS)
def test_budget_spectra(name, n):
    """``rowspec_b`` against NumPy's FFT of the band's rows' products; BAe(n), BKe(n), tendencies and residuals against ``budget_terms``,
    and their sums on the run's own totals."""
    dom, d64, box, eng, pb, f = _setup(name)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    bspec = eng.rowspec_b(*f[:4], rows, pb, n).cpu().numpy()
    assert tb._record_err(bspec, br.row_shares(*_band(name), n), f"{name} N={n} rowspec_b") <= TOL
    res = _run(name, n)
    for field in tb.BUDGET_FIELDS:
        assert np.isfinite(getattr(res, field).cpu().numpy()).all(), field
    assert tb._term_errs(res, br.budget_terms(d64, *ra.limits_of(dom, box), n), f"{name} N={n}") <= TOL
    assert tb._totals_errs(res, dom.time_s, f"{name} N={n}") <= CLOSE


@pytest.mark.parametrize("name", ["narrow", "tall"], ids=["narrow-small-kernels", "tall-tall-kernels"])
def test_fused_equals_assembled(name):
    """``spectrum_fused=True`` (lec_level_spec*_ring) against the assembled form: every field of the result, bit for bit."""
    asm, fused = _run(name), _run(name, fused=True)
    seen = 0
    for fld in dataclasses.fields(asm):
        a, b = getattr(asm, fld.name), getattr(fused, fld.name)
        assert (a is None) == (b is None), fld.name
        if isinstance(a, torch.Tensor) and a.dtype == torch.float64 and fld.name != "rows":
            assert _same_bits(a, b), fld.name
            seen += 1
    assert _same_bits(asm.rows[..., :28], fused.rows[..., :28])
    assert (asm.spectrum_b != 0).all() and torch.isfinite(asm.spectrum_levels).all()
    print(f"{name}: {seen} result fields of the fused form carry the assembled form's bits")
    assert seen >= 20


# -- 3. sections ------------------------------------------------------------------------------------------------------------------
def _check_sections(case_id, res, tag):
    _, r = ra.reference(case_id)
    _, _, _, _, pb, _ = _setup(case_id)
    steps, lat = res.section_steps.cpu().numpy(), res.section_lat.cpu().numpy()
    _close(steps, r["X"], (0, 2, 3), tag + " sections")
    _close(lat, r["Xc"], (0, 2), tag + " columns")
    _close(res.section_mean, r["Xm"], (1, 2), tag + " mean")
    return steps, lat, pb.bt.lattab2[0, :steps.shape[-1], 0]


@pytest.mark.parametrize("name", ra.CLEAN_IDS)
def test_sections(name):
    """Sections, columns and means against the restatement; sum_j cw_j of them closes on the run's own level tables and scalars."""
    res = _run(name)
    steps, lat, cw = _check_sections(name, res, name)
    levels, scalars = res.levels.cpu().numpy(), res.scalars.cpu().numpy()
    own_lv = np.stack([levels[:, LEVEL_TERMS.index(t)] for t in SECTION_TERMS], axis=1)
    own_sc = np.stack([scalars[:, SCALAR_TERMS.index(t)] for t in SECTION_TERMS], axis=1)
    _close((steps * cw).sum(axis=-1), own_lv, (0, 2), name + " closure on levels", CLOSE)
    _close((lat * cw).sum(axis=-1), own_sc, (0,), name + " closure on scalars", CLOSE)


def test_spectral_sections():
    """``narrow``: the spectral columns of N = 8 with Ge against the restatement, their N + 1 entries on the time mean of the columns, and
    with N = nx / 2 = 35 the Parseval closure of the spectral sections on the sections."""
    dom, _, _, eng, pb, f = _setup("narrow")
    b, r = ra.reference("narrow")
    res = _run("narrow")
    got = res.section_spec_lat.cpu().numpy()
    with np.errstate(invalid="ignore"):
        ref = sr.spectral_columns_mean(b, N, generation=True, total_columns=r["Xc"])
    scale = np.abs(ref[:, :N]).max(axis=(1, 2), keepdims=True)
    err = (np.abs(got - ref).max(axis=(1, 2), keepdims=True) / scale).max()
    print(f"narrow N={N} spectral columns: {err:.2e} of the largest share")
    assert got.shape == ref.shape == (6, N + 1, ra.build("narrow")[2]["nyb"]) and err <= TOL
    tot = sr.time_mean(res.section_lat.cpu().numpy())[SPEC_IDX]
    _close(got.sum(axis=1), tot, (1,), f"narrow N={N}: shares + rest against the columns' time mean", CLOSE)
    n = dom.lon.size // 2
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    levraw = torch.empty((NT, rows.shape[1], _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
    eng.level_stage(rows, pb, levraw)
    sp, qs = eng.rowspec(*f[:4], pb, n).clone(), eng.rowspec_q(*f[:4], pb, n, time_s=dom.time_s).clone()
    st = eng.section_begin(NT, int(rows.shape[2]), DEV, n_wave=n, generation=True, keep_steps=True)
    eng.section_stage(rows, pb, levraw, st, 0, spec=sp, qspec=qs)
    torch.cuda.synchronize()
    total = st["steps"].cpu().numpy()[:, :, SPEC_IDX]                       # [T, nl, 6, ny]
    shares = st["specwork"][:NT].cpu().numpy().sum(axis=2)                  # [T, nl, N, 6, ny] summed over n
    _close(shares, total, (0, 1, 3), f"narrow N={n}: sum over n of X_f^n against X_f", CLOSE)


# -- 4. maps ----------------------------------------------------------------------------------------------------------------------
def _check_maps(case_id, res, tag):
    _, r = ra.reference(case_id)
    steps = res.map_steps.cpu().numpy()
    _close(steps, r["C"], (0, 2, 3), tag + " map_steps")
    _close(res.map_lon, r["H"], (0, 2), tag + " map_lon")
    _close(res.map_mean, r["M"], (1, 2), tag + " map_mean")
    return steps


@pytest.mark.parametrize("case_id", list(ra.CLEAN_IDS) + ["narrow_open", "narrow_f32_open"])
def test_maps(case_id):
    """map_steps, map_lon and map_mean against the restatement; the box's zonal average of a map row closes on the run's own
    ``section_lat``, that of the Hovmoeller on its scalars."""
    res = _run(case_id)
    b, _ = ra.reference(case_id)
    ring = ra.build(case_id)[2]["ring"]
    steps = _check_maps(case_id, res, case_id)
    lat = res.section_lat.cpu().numpy()[:, [SECTION_TERMS.index(t) for t in MAP_TERMS]]
    _close(mr.zonal_average(steps, b, ring), lat, (0, 2), case_id + " zonal average of map_steps against section_lat", CLOSE)
    own_sc = res.scalars.cpu().numpy()[:, [SCALAR_TERMS.index(t) for t in MAP_TERMS]]
    _close(mr.zonal_average(res.map_lon.cpu().numpy(), b, ring), own_sc, (0,), case_id + " zonal average of map_lon against the scalars", CLOSE)


# -- 5. NaNs in u, omega and T at once ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("suffix", ["", "_open"], ids=["ring", "open"])
def test_nan_case(suffix):
    """``narrow_nan``: NaN patterns and values of the sections and maps are the restatement's, every column value is finite, and a term is
    bit-equal to the clean run of the same engine at every step outside its own changed set."""
    case_id = ra.NAN_ID + suffix
    res, plain = _run(case_id), _run("narrow" + suffix)
    _check_sections(case_id, res, case_id)
    _check_maps(case_id, res, case_id)
    changed = ra.build(case_id)[2]["changed"]
    assert torch.isnan(res.section_steps).any()
    same = moved = 0
    for terms, fields in ((SECTION_TERMS, ("section_steps", "section_lat")), (MAP_TERMS, ("map_steps", "map_lon"))):
        for name in fields:
            a, c = getattr(res, name), getattr(plain, name)
            if name != "section_steps":            # (the sections hold the NaN levels themselves; their columns bridge or trim them)
                assert torch.isfinite(a).all(), name
            for t in range(NT):
                for i, term in enumerate(terms):
                    if t in changed[term]:
                        assert not _same_bits(a[t, i], c[t, i]), (name, term, t)
                        moved += 1
                    else:
                        assert _same_bits(a[t, i], c[t, i]), f"{name}: {term} at step {t} differs from the clean run"
                        same += 1
    print(f"{case_id}: {same} (field, term, step) slabs carry the clean run's bits, {moved} moved")


# -- 6. chunks on uneven time ------------------------------------------------------------------------------------------------------
def test_chunk_independence_on_uneven_time(monkeypatch):
    """``map_stage`` / ``section_stage`` in chunks of 1, 2 and 4 steps with ``t_begin`` / ``t_offset`` advancing, and under a
    ``MAP_CHUNK_BYTES`` cap of 2 steps: the whole run's bits -- and the whole run is the restatement's (test_maps, test_sections), so
    'every chunking equally wrong' does not pass: on uneven steps tcoef differs from step to step."""
    dom, _, box, eng, pb, f = _setup("narrow")
    nyb, nxb, nl = box[3] - box[2] + 1, box[1] - box[0] + 1, dom.level.size
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    levraw = torch.empty((NT, nl, _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
    eng.level_stage(rows, pb, levraw)
    sp, qs = eng.rowspec(*f[:4], pb, N).clone(), eng.rowspec_q(*f[:4], pb, N, time_s=dom.time_s).clone()
    out = {}
    for name, chunk, cap in (("1", 1, None), ("2", 2, None), ("4", 4, None), ("cap", 4, 2)):
        if cap is not None:
            monkeypatch.setattr(LECEngine, "MAP_CHUNK_BYTES", cap * 8 * (6 * nyb * nxb + nl * nyb * _lib.LEC_MAPS_NCOEF))
        mp = eng.map_begin(NT, pb, DEV, keep_steps=True)
        sc = eng.section_begin(NT, nyb, DEV, n_wave=N, generation=True, keep_steps=True)
        for a in range(0, NT, chunk):
            b = min(a + chunk, NT)
            eng.map_stage(*f[:4], rows[a:b], pb, levraw[a:b], mp, a, time_s=dom.time_s, t_begin=a)
            eng.section_stage(rows[a:b], pb, levraw[a:b], sc, a, spec=sp[a:b], qspec=qs[a:b])
        if cap is not None:
            assert mp["coef"].shape[0] == cap
        res = eng.vertical_stage(levraw, pb)
        eng.map_finish(res, mp)
        eng.section_finish(res, sc)
        out[name] = res
        monkeypatch.undo()
    whole = _run("narrow")
    names = ("map_steps", "map_lon", "map_mean", "section_steps", "section_lat", "section_mean", "section_spec_lat")
    for name, res in out.items():
        for fld in names:
            x, y = getattr(res, fld), getattr(whole, fld)
            assert not torch.isnan(y).any()
            assert _same_bits(x, y), (name, fld)
    _, r = ra.reference("narrow")
    _close(out["1"].map_steps, r["C"], (0, 2, 3), "narrow, one step per chunk: map_steps")
    _close(out["1"].section_steps, r["X"], (0, 2, 3), "narrow, one step per chunk: sections")
    print(f"chunks of 1, 2, 4 steps and a cap of 2: {len(names)} fields carry the whole run's bits")


# -- 7. records -------------------------------------------------------------------------------------------------------------------
def _records(case_id):
    dom, boxes, kw, _ = ra.records_build(case_id)
    if dom.tair.dtype == np.float64:
        rec._engines.setdefault(id(dom), (dom, _engine("narrow")))
    judge = rec._Judge(case_id, kw["family"])
    rec._fixed(judge, dom, rec._dom_fields(dom), rec._engine(dom), boxes, kw, ra.records_reference(case_id))
    judge.finish()


@pytest.mark.parametrize("case_id", ra.RECORD_IDS)
def test_records(case_id):
    """lec_rowstats_ring on ``narrow`` (fp64 and fp32 storage; modes 0, 2, 3; the whole series and steps 1, 2 of it) against the
    extended-precision restatement, by the judge and the measure of tests/test_gpu_rowstats_records.py."""
    rec._guarded(_records, case_id)
