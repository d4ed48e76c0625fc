"""-f [--periodic] --sections on the GPU: ``lec_sections`` through ``LECEngine.compute(..., sections=True)`` / ``section_stage`` against the
CPU restatement (tests/sections_restatement.py) and against the engine's own per-level tables and scalars.

Shapes.  Bands of 5, 64, 65 and 130 rows (the small and the tall stage-2 path, the 64-row trip seam, a third trip), nx = 16, nl = 5 and once
nl = 70, T = 5; a ring and an open regional box; fp64 storage and fp32 storage once (the restatement is fed the float32-rounded fields as
fp64).

Bars.  1e-9 of the term's scale (the largest |value| of the term in the case) for every section, column and mean against the
restatement, for the closure of sum_j cw_j X_f on the engine's per-level tables, of sum_j cw_j C_f on its scalars, and for the Parseval
closure of the spectral sections: the project's parity bar.  Chunk independence and ``sections=False`` are bit for bit.
Measured on MI355X: sections 2.3e-13, columns 1.2e-13, means 1.5e-13, closure on levels 3.1e-15, on scalars 2.8e-15, Parseval 4.8e-15,
spectral columns 2.9e-14 (each test prints its own figure).
Uneven axes, inner bands (js > 0, NaN rows and columns around the box) and NaNs in the other fields: tests/test_gpu_ring_axes.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib
from lorenzcycletoolkit_amd.constants import LEVEL_TERMS, SCALAR_TERMS, SECTION_TERMS
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests import sections_restatement as sr
from tests.helpers import as_f64

DEV = "cuda:0"
NT, NX = 5, 16
TOL = 1e-9
SOUTH, NORTH = -60.0, 60.0
OPEN_IW, OPEN_IE = 2, 13            # the open box's columns on the 16-column axis
# (kind, rows, levels, storage)
CASES = [("ring", 5, 5, np.float64), ("ring", 64, 5, np.float64), ("ring", 65, 5, np.float64), ("ring", 130, 5, np.float64),
         ("open", 5, 5, np.float64), ("open", 64, 5, np.float64), ("open", 65, 5, np.float64), ("open", 130, 5, np.float64),
         ("ring", 65, 70, np.float64), ("open", 64, 5, np.float32)]
IDS = [f"{k}-{ny}rows-{nl}lev-{np.dtype(d).name}" for k, ny, nl, d in CASES]
SPEC_IDX = [SECTION_TERMS.index(k) for k in sr.SPEC_TERMS]

_cache = {}


def _dom(ny, nl, dtype=np.float64):
    key = ("dom", ny, nl, np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = rr.ring_domain(NT, nl, ny, NX, seed=ny + nl, dtype=dtype, lat0=SOUTH, lat1=NORTH)
    return _cache[key]


def _box(kind, dom):
    """The oracle's Box of the case (whole latitude axis; the ring, or the columns OPEN_IW .. OPEN_IE as a limited area)."""
    d = as_f64(dom)
    with np.errstate(invalid="ignore"):
        if kind == "ring":
            return rr.ring_box(d, SOUTH, NORTH)
        return o.make_box(d, dom.lon[OPEN_IW], dom.lon[OPEN_IE], SOUTH, NORTH)


def _reference(kind, ny, nl, dtype):
    """(X [T, 10, nl, ny], C [T, 10, ny], M [10, nl, ny]) of the restatement, computed once per case and shared."""
    key = ("ref", kind, ny, nl, np.dtype(dtype).name)
    if key not in _cache:
        b = _box(kind, _dom(ny, nl, dtype))
        with np.errstate(invalid="ignore"):
            X = sr.sections(b)
        _cache[key] = (X, sr.columns(X, b.level), sr.time_mean(X))
    return _cache[key]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _fields(dom):
    return [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]


def _engine(kind, dom):
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    if kind == "ring":
        return eng, eng.prepare_boxes([(0, dom.lon.size - 1, 0, dom.lat.size - 1)], ring=True)
    return eng, eng.prepare_boxes([(OPEN_IW, OPEN_IE, 0, dom.lat.size - 1)])


def _scale(ref, axes):
    """The term's scale: its largest finite |value| over ``axes`` (1.0 where the term has none)."""
    a = np.where(np.isnan(ref), -np.inf, np.abs(ref)).max(axis=axes, keepdims=True)
    return np.where(np.isfinite(a), a, 1.0)


def _close(got, ref, axes, what):
    """|got - ref| <= TOL * the term's scale, the NaN patterns equal; returns the largest error over scale."""
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern"
    err = np.nanmax(np.abs(got - ref) / _scale(ref, axes)) if np.isfinite(ref).any() else 0.0
    print(f"{what}: max error / scale = {err:.3e}")
    assert err <= TOL, (what, err)
    return err


@pytest.mark.parametrize("kind, ny, nl, dtype", CASES, ids=IDS)
def test_sections_match_restatement_and_close(kind, ny, nl, dtype):
    dom = _dom(ny, nl, dtype)
    X, Cc, M = _reference(kind, ny, nl, dtype)
    eng, pb = _engine(kind, dom)
    res = eng.compute(*_fields(dom), pb, time_s=dom.time_s, sections=True, section_steps=True)
    steps, lat, mean = res.section_steps.cpu().numpy(), res.section_lat.cpu().numpy(), res.section_mean.cpu().numpy()
    tag = f"{kind} {ny}x{nl} {np.dtype(dtype).name}"
    _close(steps, X, (0, 2, 3), tag + " sections")
    _close(lat, Cc, (0, 2), tag + " columns")
    _close(mean, M, (1, 2), tag + " mean")
    # closure on the engine's own per-level tables and scalars, with the row weight the level stage uses
    cw = pb.bt.lattab2[0, :ny, 0]
    levels, scalars = res.levels.cpu().numpy(), res.scalars.cpu().numpy()
    own_lv = np.stack([levels[:, LEVEL_TERMS.index(t)] for t in SECTION_TERMS], axis=1)        # [T, 10, nl]
    own_sc = np.stack([scalars[:, SCALAR_TERMS.index(t)] for t in SECTION_TERMS], axis=1)       # [T, 10]
    _close((steps * cw).sum(axis=-1), own_lv, (0, 2), tag + " closure on levels")
    _close((lat * cw).sum(axis=-1), own_sc, (0,), tag + " closure on scalars")


def _records(dom, n_wave):
    """(engine, ring box, rows, levraw, spec, qspec) of the whole series."""
    eng, pb = _engine("ring", dom)
    f = _fields(dom)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    levraw = torch.empty((rows.shape[0], rows.shape[1], _lib.LEC_NLEVRAW), dtype=torch.float64, device=DEV)
    eng.level_stage(rows, pb, levraw)
    sp = eng.rowspec(*f[:4], pb, n_wave).clone()
    qs = eng.rowspec_q(*f[:4], pb, n_wave, time_s=dom.time_s).clone()
    return eng, pb, rows, levraw, sp, qs


@pytest.mark.parametrize("ny", [5, 65])
def test_parseval_closure_of_the_spectral_sections(ny):
    dom = _dom(ny, 5)
    n = NX // 2
    eng, pb, rows, levraw, sp, qs = _records(dom, n)
    st = eng.section_begin(NT, ny, DEV, n_wave=n, generation=True, keep_steps=True)
    eng.section_stage(rows, pb, levraw, st, 0, spec=sp, qspec=qs)
    torch.cuda.synchronize()
    total = st["steps"].cpu().numpy()[:, :, SPEC_IDX]                       # [T, nl, 6, ny]
    shares = st["specwork"][:NT].cpu().numpy().sum(axis=2)                  # [T, nl, N, 6, ny] summed over n
    _close(shares, total, (0, 1, 3), f"ring {ny} rows: sum over n of X_f^n against X_f")
    # ... and the spectral columns against the restatement; at N = nx / 2 nothing is left for the rest
    res = eng.compute(*_fields(dom), pb, time_s=dom.time_s, sections=True, wavenumbers=n, spectrum_generation=True)
    got = res.section_spec_lat.cpu().numpy()
    b = _box("ring", dom)
    with np.errstate(invalid="ignore"):
        ref = sr.spectral_columns_mean(b, n, generation=True)
    scale = np.abs(ref[:, :n]).max(axis=(1, 2), keepdims=True)
    err = np.abs(got - ref).max(axis=(1, 2), keepdims=True) / scale
    print("spectral columns: max error / scale =", err.ravel())
    assert got.shape == (6, n + 1, ny) and err.max() <= TOL
    assert (np.abs(got[:, n]) / scale[:, 0]).max() <= TOL


def test_chunk_independence_bit_for_bit():
    ny, n = 65, 4
    dom = _dom(ny, 5)
    eng, pb, rows, levraw, sp, qs = _records(dom, n)
    out = {}
    for chunk in (1, 2, 5):
        st = eng.section_begin(NT, ny, DEV, n_wave=n, generation=True)
        for a in range(0, NT, chunk):
            b = min(a + chunk, NT)
            eng.section_stage(rows[a:b], pb, levraw[a:b], st, a, spec=sp[a:b], qspec=qs[a:b])
        res = eng.vertical_stage(levraw, pb)
        eng.section_finish(res, st)
        out[chunk] = (res.section_mean, res.section_lat, res.section_spec_lat)
    whole = eng.compute(*_fields(dom), pb, time_s=dom.time_s, sections=True, wavenumbers=n, spectrum_generation=True)
    fused = eng.compute(*_fields(dom), pb, time_s=dom.time_s, sections=True, wavenumbers=n, spectrum_generation=True, spectrum_fused=True)
    for name, got in (("1", out[1]), ("2", out[2]), ("compute", (whole.section_mean, whole.section_lat, whole.section_spec_lat)),
                      ("fused", (fused.section_mean, fused.section_lat, fused.section_spec_lat))):
        for x, y, what in zip(got, out[5], ("section_mean", "section_lat", "section_spec_lat")):
            assert not torch.isnan(y).any()
            assert torch.equal(x, y), (name, what)


NAN_CASES = {"interior level": dict(t=2, k=[2], rows=[3, 4, 5]), "top level": dict(t=2, k=[0], rows=[3, 4, 5]),
             "one row at every level": dict(t=2, k=[0, 1, 2, 3, 4], rows=[4])}


@pytest.mark.parametrize("case", list(NAN_CASES))
def test_nan_patterns_are_the_restatements(case):
    ny, nl = 9, 5
    c = NAN_CASES[case]
    base = _dom(ny, nl)
    T = base.tair.copy()
    for k in c["k"]:
        T[c["t"], k, c["rows"], 5:9] = np.nan
    dom = o.Domain(T, base.u, base.v, base.omega, base.geopt, base.lat, base.lon, base.level, base.time_s)
    with np.errstate(invalid="ignore"):
        b = rr.ring_box(dom, SOUTH, NORTH)
        X = sr.sections(b)
    Cc, M = sr.columns(X, b.level), sr.time_mean(X)
    eng, pb = _engine("ring", dom)
    res = eng.compute(*_fields(dom), pb, time_s=dom.time_s, sections=True, section_steps=True)
    _close(res.section_steps.cpu().numpy(), X, (0, 2, 3), case + ": sections")
    lat = res.section_lat.cpu().numpy()
    _close(lat, Cc, (0, 2), case + ": columns")
    _close(res.section_mean.cpu().numpy(), M, (1, 2), case + ": mean")
    ae = SECTION_TERMS.index("Ae")              # Ae reads [T'T'] of its own row and level only (sigma is clamped where it is NaN)
    if case == "one row at every level":        # the column of the row is NaN at that step, and its neighbours' are not
        assert np.isnan(lat[c["t"], ae, 4]) and np.isfinite(lat[c["t"], ae, [3, 5]]).all()
    else:                                        # bridged or trimmed: the columns stay finite, the mean is NaN at the patch only
        assert np.isfinite(lat[:, ae]).all()
        m = np.isnan(res.section_mean.cpu().numpy()[ae])
        assert m[c["k"][0], c["rows"]].all() and m.sum() == len(c["rows"])


def test_without_sections_nothing_changes():
    dom = _dom(65, 5)
    eng, pb = _engine("ring", dom)
    kw = dict(time_s=dom.time_s, wavenumbers=4, spectrum_generation=True)
    plain, again = eng.compute(*_fields(dom), pb, **kw), eng.compute(*_fields(dom), pb, sections=False, **kw)
    with_sec = eng.compute(*_fields(dom), pb, sections=True, **kw)
    import dataclasses
    for f in dataclasses.fields(plain):
        a, b, c = getattr(plain, f.name), getattr(again, f.name), getattr(with_sec, f.name)
        if f.name.startswith("section_"):
            assert a is None and b is None, f.name
            continue
        assert (a is None) == (b is None) == (c is None), f.name
        if a is not None:
            assert torch.equal(a, b) and torch.equal(a, c), f.name
    assert with_sec.section_mean is not None and with_sec.section_steps is None


def test_refused_in_words():
    dom = _dom(5, 5)
    eng, _ = _engine("open", dom)
    boxes = [(OPEN_IW, OPEN_IE, 0, 4)] * NT
    with pytest.raises(ValueError, match="ONE fixed box"):
        eng.compute(*_fields(dom), boxes, time_s=dom.time_s, sections=True)
    with pytest.raises(ValueError, match="one process on one GPU"):
        eng.compute(*_fields(dom), [boxes[0]], time_s=dom.time_s, sections=True, merge_dropmask=lambda m: None)
