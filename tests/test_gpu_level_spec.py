"""``lec_level_spec_ring`` on the GPU: stage 2 of the spectra without assembled records (``compute(..., spectrum_fused=True)``) against
the assembled form of the same call, as int64 bits -- no tolerance: X(n) is DEFINED as what ``lec_reduce`` gives on the assembled
records.  Grids of 3 steps x 4 levels on ``ring_restatement.ring_domain``.

Band heights: 5 rows (the small form: the record in registers), 70 (the general form: two staging trips through LDS, the rows j - 1 /
j + 1 across the trip edge) and 130 (three trips).  Rings / N: 8 / 4 (the Nyquist share), 7 / 3 (odd), 130 / 20, and N = 1.  NaN at an
interior level of one step: BAz's bottom-top term is repaired per latitude from the OTHER levels' [w'T'], a replaced slot; NaN at the
bottom level: the level is dropped, with the any-time mask over the (n, t) batch.  One parity case against the CPU restatement at the
bar of tests/test_gpu_spectrum.py (1e-9 of scale), so that the bit identity is not the only anchor."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests import spectrum_restatement as sr

DEV = "cuda:0"
NT, NL = 3, 4
SOUTH, NORTH = -60.0, 60.0
TOL = 1e-9
FIELDS = ("spectrum", "spectrum_rest", "spectrum_levels")
GE_FIELDS = ("spectrum_ge", "spectrum_ge_rest", "spectrum_ge_levels")

_doms = {}


def _dom(ny, nx):
    if (ny, nx) not in _doms:
        _doms[(ny, nx)] = rr.ring_domain(NT, NL, ny, nx, seed=ny + nx, lat0=SOUTH, lat1=NORTH)
    return _doms[(ny, nx)]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _engine(dom):
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    return eng, eng.prepare_boxes([(0, dom.lon.size - 1, 0, dom.lat.size - 1)], ring=True)


def _compute(dom, n, **kw):
    eng, pb = _engine(dom)
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    return eng.compute(*f, pb, time_s=dom.time_s, keep_rows=True, wavenumbers=n, **kw)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _assert_same(fused, ref, generation, what):
    for name in FIELDS + (GE_FIELDS if generation else ()):
        assert _same_bits(getattr(fused, name), getattr(ref, name)), f"{what}: {name} differs from the assembled form"
    if not generation:
        assert fused.spectrum_ge is None and fused.spectrum_ge_rest is None and fused.spectrum_ge_levels is None
    # ... and nothing of the totals moves
    assert _same_bits(fused.scalars, ref.scalars) and _same_bits(fused.levels, ref.levels) and torch.equal(fused.nanflag, ref.nanflag)


# -- 1. both forms, every ring ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generation", [False, True], ids=["", "Ge"])
@pytest.mark.parametrize("ny, nx, n", [(5, 8, 4), (5, 7, 3), (5, 130, 20), (5, 130, 1), (70, 8, 4), (70, 7, 3), (70, 130, 20), (70, 130, 1),
                                       (130, 8, 4), (130, 7, 3), (130, 130, 20)])
def test_fused_equals_assembled(ny, nx, n, generation):
    dom = _dom(ny, nx)
    ref = _compute(dom, n, spectrum_generation=generation)
    fused = _compute(dom, n, spectrum_generation=generation, spectrum_fused=True)
    assert fused.spectrum.shape == (NT, 5, n) and torch.isfinite(fused.spectrum).all()
    _assert_same(fused, ref, generation, f"ny={ny} nx={nx} N={n}")


def test_fused_needs_wavenumbers():
    dom = _dom(5, 8)
    eng, pb = _engine(dom)
    with pytest.raises(ValueError):
        eng.compute(*[_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)], pb, time_s=dom.time_s, spectrum_fused=True)


# -- 2. NaN -----------------------------------------------------------------------------------------------------------------------
def _with_nan(dom, where):
    f = [a.copy() for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    ny = dom.lat.size
    rows = [1, 2] + ([ny - 4] if ny > 64 else [])       # (a taller band: a row of the second staging trip too)
    for a in f:
        for j in rows:
            if where == "bottom":
                a[:, NL - 1, j, 2:4] = np.nan
            else:
                a[1, 2, j, 2:4] = np.nan
    return o.Domain(*f, dom.lat, dom.lon, dom.level, dom.time_s)


@pytest.mark.parametrize("where", ["interior", "bottom"])
@pytest.mark.parametrize("ny", [5, 70])
def test_nan(ny, where):
    dom = _with_nan(_dom(ny, 16), where)
    ref = _compute(dom, 8, spectrum_generation=True)
    fused = _compute(dom, 8, spectrum_generation=True, spectrum_fused=True)
    assert int(ref.nanflag.sum()) > 0
    _assert_same(fused, ref, True, f"NaN at the {where} level, ny={ny}")
    # BAz itself has no spectrum, so its repaired bottom-top term shows in the level records only: compare them too
    eng, pb = _engine(dom)
    cubes = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega)]
    spec = eng.rowspec(*cubes, pb, 8)
    asm = ref.rows.unsqueeze(0).repeat(8, 1, 1, 1, 1)
    asm[..., 6:14] = spec.permute(3, 0, 1, 2, 4)
    want = torch.empty((8 * NT, NL, _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
    eng.level_stage(asm.view(8 * NT, NL, ny, _lib.LEC_NSTAT), pb, want)
    got = torch.empty((8, NT, NL, _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
    eng.spectrum_level_stage(ref.rows, spec, None, pb, got)
    assert _same_bits(got.view(8 * NT, NL, _lib.LEC_NLEVRAW), want)
    baz3 = got[:, 1, :, 27]                             # the repaired term of the step with the NaN level
    if where == "interior":
        assert torch.isfinite(baz3).all()                # repaired per latitude from the levels above and below
    else:
        assert torch.isnan(baz3[:, NL - 1]).all() and torch.isfinite(baz3[:, :NL - 1]).all()


# -- 3. time chunks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny", [5, 70])
def test_time_chunks_give_the_same_bits(ny, monkeypatch):
    """One step per chunk, and two steps plus a shorter last chunk: strided ``levraw_out`` slices through ``wave_stride``."""
    n = 20
    dom = _dom(ny, 130)
    ref = _compute(dom, n, spectrum_generation=True)
    eng, _ = _engine(dom)
    monkeypatch.setattr(LECEngine, "SPECTRUM_CHUNK_BYTES", 1)
    assert eng.spectrum_chunk_steps(NT, NL, ny, n) == 1
    _assert_same(_compute(dom, n, spectrum_generation=True, spectrum_fused=True), ref, True, "one step per chunk")
    monkeypatch.setattr(LECEngine, "SPECTRUM_CHUNK_BYTES", 2 * NL * ny * n * 64)
    assert eng.spectrum_chunk_steps(NT, NL, ny, n) == 2
    _assert_same(_compute(dom, n, spectrum_generation=True, spectrum_fused=True), ref, True, "two steps, then one")


# -- 4. the stage itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny", [5, 70])
def test_level_stage_dense_and_sliced(ny):
    n = 4
    dom = _dom(ny, 8)
    eng, pb = _engine(dom)
    res = _compute(dom, n)
    cubes = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega)]
    spec = eng.rowspec(*cubes, pb, n)
    qspec = eng.rowspec_q(*cubes, pb, n, time_s=dom.time_s)
    f64 = dict(dtype=torch.float64, device=DEV)
    dense = torch.full((n, NT, NL, _lib.LEC_NLEVRAW), -1.0, **f64)
    eng.spectrum_level_stage(res.rows, spec, qspec, pb, dense)
    longer = torch.full((n, NT + 3, NL, _lib.LEC_NLEVRAW), -1.0, **f64)
    eng.spectrum_level_stage(res.rows, spec, qspec, pb, longer[:, 1:1 + NT])
    assert _same_bits(longer[:, 1:1 + NT], dense)
    assert bool((longer[:, :1] == -1.0).all()) and bool((longer[:, 1 + NT:] == -1.0).all())       # nothing beside the slice is written
    # the assembled records through lec_reduce's level half: the definition
    asm = res.rows.unsqueeze(0).repeat(n, 1, 1, 1, 1)
    asm[..., 6:14] = spec.permute(3, 0, 1, 2, 4)
    asm[..., 15] = qspec.permute(3, 0, 1, 2)
    want = torch.empty((n * NT, NL, _lib.LEC_NLEVRAW), **f64)
    eng.level_stage(asm.view(n * NT, NL, ny, _lib.LEC_NSTAT), pb, want)
    assert _same_bits(dense.view(n * NT, NL, _lib.LEC_NLEVRAW), want)
    # without qspec slot 15 stays the ring pass's: Ge's level sums are the totals' for every n
    plain = torch.empty((n, NT, NL, _lib.LEC_NLEVRAW), **f64)
    eng.spectrum_level_stage(res.rows, spec, None, pb, plain)
    tot = torch.empty((NT, NL, _lib.LEC_NLEVRAW), **f64)
    eng.level_stage(res.rows, pb, tot)
    assert _same_bits(plain[..., 14], tot[..., 14].unsqueeze(0).expand(n, NT, NL))
    with pytest.raises(ValueError):
        eng.spectrum_level_stage(res.rows, spec, qspec, pb, dense[:, :, :, :39])
    with pytest.raises(ValueError):
        eng.spectrum_level_stage(res.rows, spec, qspec, pb, longer[:, ::2][:, :NT])
    with pytest.raises(ValueError):
        eng.spectrum_level_stage(res.rows, spec[:, :, :, :2], qspec, pb, dense)


# -- 5. the restatement -----------------------------------------------------------------------------------------------------------
def test_fused_terms_against_the_restatement():
    """The general form (70 rows) against the CPU restatement: spectrum, rest and level tables to 1e-9 of scale."""
    ny, nx, n = 70, 24, 4
    dom = _dom(ny, nx)
    res = _compute(dom, n, spectrum_fused=True)
    spec, rest, levels, _ = sr.spectrum_terms(dom, SOUTH, NORTH, n)
    got = res.spectrum.cpu().numpy()
    e_spec = np.abs(got - spec).max(axis=(0, 2)) / np.abs(spec).max(axis=(0, 2))
    e_rest = np.abs(res.spectrum_rest.cpu().numpy() - rest).max(axis=0) / np.abs(spec).max(axis=(0, 2))
    e_lev = np.abs(res.spectrum_levels.cpu().numpy() - levels).max(axis=(0, 2, 3)) / np.abs(levels).max(axis=(0, 2, 3))
    print(f"fused terms ny={ny} nx={nx} N={n}: spectrum {e_spec.max():.2e}, rest {e_rest.max():.2e}, levels {e_lev.max():.2e} of scale")
    assert e_spec.max() <= TOL, dict(zip(sr.TERMS, e_spec))
    assert e_rest.max() <= TOL, dict(zip(sr.TERMS, e_rest))
    assert e_lev.max() <= TOL, dict(zip(sr.LEVEL_TERMS, e_lev))
