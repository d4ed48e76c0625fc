"""Stage-1 conformance: the row records of every kernel family against tests/rowstats_restatement.py (the 28 interface statistics of a
row, evaluated in np.longdouble from the oracle's own functions), on the cases of tests/rowstats_cases.py -- the smallest shapes at
which each family's control flow changes, with every grid point outside the box NaN.  ``LECEngine.rowstats`` only: stage 2 is not
involved, and ``tuning={"kernel": ...}`` is passed explicitly.  The engine cannot tell which instantiation ran.  The library refuses a
box-tile / box-plane request it cannot serve, but it quietly runs one wave per row for a row-block request that lacks a geopotential
cube, the time stencil or a second step: tests/test_rowstats_cases_cpu.py asserts that every block case meets those conditions, and
that the tile cases reach both forms of lec_boxtile_kernel (the launch picks by the call's widest box).

The measure (per case):
  slots 5..21   per statistic, max over the case's rows |got - ref| <= 1e-11 x max over the rows |ref|;
  slots 0..4    per row, |got - ref| <= (nxb + 4) 2^-53 max |X| over the row's box elements;
  slots 22..27  bit-equal to the stored element as fp64;
  zeroed slots  ([Q], [Q'T'] without Q; [Phi], [w'Phi'] without a geopotential cube) exactly 0; every record finite -- in the nan cases:
                NaN at the reference's places, in all 28 slots, and nowhere else.
Every case prints its worst ratio to the two bars; the module prints the worst per family at its end."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import rowstats_cases as rc
from tests import rowstats_restatement as rs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_fields, _engines, _worst, _dead = {}, {}, {}, []


def _up(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _dom_fields(dom):
    """The clean fields of a domain on the device, uploaded once per module."""
    if id(dom) not in _fields:
        _fields[id(dom)] = (dom, [_up(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)])
    return _fields[id(dom)][1]


def _engine(dom):
    from lorenzcycletoolkit_amd.engine import LECEngine
    if id(dom) not in _engines:
        _engines[id(dom)] = (dom, LECEngine(dom.lat, dom.lon, dom.level, device=DEV))
    return _engines[id(dom)][1]


def _framed(t, mask):
    """NaN wherever ``mask`` (bool, broadcast over [steps, level, lat, lon]) is False."""
    return torch.where(mask, t, torch.full((), float("nan"), dtype=t.dtype, device=t.device)).contiguous()


def _box_mask(dom, box, ring=False):
    m = np.zeros((1, 1, dom.lat.size, dom.lon.size), dtype=bool)
    m[..., box[2]:box[3] + 1, :] = True
    if not ring:
        m[..., :box[0]] = False
        m[..., box[1] + 1:] = False
    return _up(m)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


class _Judge:
    """Collects the rows of a case and judges them by the measure.  ``nans``: the case plants NaNs -- they must sit at the reference's
    places in all 28 slots and nowhere else, and the other values agree."""

    def __init__(self, case_id, family, nans=False):
        self.case_id, self.family, self.nans, self.got, self.ref, self.bad, self.mean = case_id, family, nans, [], [], [], 0.0

    def rows(self, got, ref, xmax, nxb, what, with_q=True, with_phi=True):
        got = np.asarray(got)[..., :rs.NSLOT]
        odd = np.isinf(got) | (np.isnan(got) != np.isnan(ref))
        if odd.any():
            self.bad.append(f"{what}: {int(odd.sum())} values in slots {sorted(set(np.nonzero(odd)[-1].tolist()))} are "
                            + ("NaN where the reference is not, or the reverse, or infinite" if self.nans else "not finite"))
            return
        e = ~np.isnan(ref[..., rs.EDGES])
        if not _same_bits(got[..., rs.EDGES][e], ref[..., rs.EDGES][e]):
            self.bad.append(f"{what}: edge values are not the stored elements")
        zero = ([] if with_q else list(rs.Q_SLOTS)) + ([] if with_phi else list(rs.PHI_SLOTS))
        if zero and np.any(got[..., zero] != 0.0):
            self.bad.append(f"{what}: slots {zero} are not exactly 0")
        m = rc.mean_error(got, ref, xmax, nxb)
        self.mean = max(self.mean, m)
        if not m <= 1.0:
            self.bad.append(f"{what}: a mean is {m:.2f} x its bound")
        self.got.append(got.reshape(-1, rs.NSLOT))
        self.ref.append(ref.reshape(-1, rs.NSLOT))

    def finish(self):
        ratio = float("inf")
        if self.got:
            err = rc.moment_error(np.concatenate(self.got), np.concatenate(self.ref)) / rc.GPU_BAR
            ratio = float(err.max())
            if not ratio <= 1.0:
                self.bad.append("slots beyond 1e-11 of their largest value: " + ", ".join(f"{5 + s}: {e:.2f} x" for s, e in enumerate(err) if not e <= 1.0))
        print(f"{self.case_id}: moments {ratio:.3f} of the bar, means {self.mean:.3f} of the bound")
        w = _worst.setdefault(self.family, [0.0, 0.0])
        w[0], w[1] = max(w[0], ratio), max(w[1], self.mean)
        assert not self.bad, f"{self.case_id}: " + "; ".join(self.bad[:12]) + (f" ... ({len(self.bad)} in all)" if len(self.bad) > 12 else "")


def _guarded(run, case_id):
    """A case that ends in anything but a failed assertion (a HIP error) stops the module: nothing more is started on the device."""
    if _dead:
        pytest.fail(f"case {_dead[0]} ended in an error of the device or the library: not run")
    try:
        run(case_id)
    except AssertionError:
        raise
    except BaseException:
        _dead.append(case_id)
        raise


def _fixed(judge, dom, clean, eng, boxes, kw, ref, label=""):
    """One call per box and run: the fields NaN outside the box (a ring: outside the band's rows)."""
    ring = kw["kind"] == "ring"
    cubes = {c: (_up(rc.dtdt_cube(rc.steps_of(dom, *c))) if kw["dtdt"] else None) for c in ref}
    for i, box in enumerate(boxes):
        mask = _box_mask(dom, box, ring)
        f = [_framed(t, mask) for t in clean]
        pb = eng.prepare_boxes([box], ring=True) if ring else [box]
        for h0, h1, tb, tc in kw["runs"]:
            d = None if cubes[(h0, h1)] is None else _framed(cubes[(h0, h1)], mask)
            got = eng.rowstats(*[t[h0:h1] for t in f[:4]], f[4][h0:h1] if kw["with_phi"] else None, pb, time_s=dom.time_s[h0:h1], dTdt=d,
                               t_begin=tb, t_count=tc, with_q=kw["with_q"], tuning=kw["tuning"]).cpu().numpy()
            judge.rows(got, ref[(h0, h1)][i][tb:tb + tc], rc.row_max(dom, box, h0 + tb, h0 + tb + tc), box[1] - box[0] + 1,
                       f"{label}width {box[1] - box[0] + 1}, steps {tb}..{tb + tc - 1} of {h1 - h0}", kw["with_q"], kw["with_phi"])


def _moving(judge, dom, clean, eng, boxes, kw, ref, label=""):
    """One call with a box per step: a cube NaN outside the boxes (of steps t - 1 .. t + 1 where T's time neighbours are read from the
    cube), or a box-packed series with NaN beside every box in its slab."""
    nt, ny, nx = len(boxes), dom.lat.size, dom.lon.size
    if kw["kind"] == "packed":
        slab = kw["slab"]
        pk = [_up(rc.pack(a, boxes, slab)) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
        tm, tp = _up(rc.pack(dom.tair, boxes, slab, -1)), _up(rc.pack(dom.tair, boxes, slab, +1))
        pb, tc = eng.prepare_boxes(boxes, packed=True), eng.time_coefs_device(dom.time_s)
        args, dkw = pk + [pb], eng.packed_dtdt(tm, pk[0], tp, tc)
        assert ("dTdt" in dkw) == (dom.tair.dtype == np.float64)
    else:
        mask = _up(rc.cover(boxes, nt, ny, nx, 1 if kw["mode"] == "nb" else 0)[:, None])
        args = [_framed(t, mask) for t in clean] + [boxes]
        dkw = {"dTdt": _framed(_up(rc.dtdt_cube(dom)), mask)} if kw["mode"] == "cube" else {"time_s": dom.time_s}
    for tuning in kw["tunings"]:
        got = eng.rowstats(*args, per_step_boxes=True, tuning=tuning, **dkw).cpu().numpy()
        for t, box in enumerate(boxes):
            h = box[3] - box[2] + 1
            judge.rows(got[t:t + 1, :, :h], ref[t:t + 1, :, :h], rc.row_max(dom, box, t, t + 1), box[1] - box[0] + 1,
                       f"{label}step {t} box {box} tile_j {tuning.get('tile_j', 0)}")
            if np.any(got[t, :, h:, :rs.NSLOT] != 0.0):
                judge.bad.append(f"{label}step {t}: padding rows are not 0")


def _steps(judge, dom, clean, eng, boxes, kw, ref):
    """lec_rowstats_steps: one call for the boxes of all tracks; every track against the records of its own sub-series."""
    table = np.asarray(kw["table"], dtype=np.int32)
    mask = _up(rc.steps_cover(kw["table"], boxes, dom.tair.shape[0], dom.lat.size, dom.lon.size)[:, None])
    tcoef = torch.cat([eng.time_coefs_device(dom.time_s[list(s)]) for s, _ in kw["tracks"]]).contiguous()
    got = eng.rowstats(*[_framed(t, mask) for t in clean], boxes, steps=_up(table), tcoef=tcoef, tuning=kw["tuning"]).cpu().numpy()
    at = 0
    for (steps, bs), r in zip(kw["tracks"], ref):
        sub = rc.track_domain(dom, steps)
        for i, box in enumerate(bs):
            h = box[3] - box[2] + 1
            judge.rows(got[at:at + 1, :, :h], r[i:i + 1, :, :h], rc.row_max(sub, box, i, i + 1), box[1] - box[0] + 1, f"table row {at} box {box}")
            at += 1


def _run(case_id):
    dom, boxes, kw, _ = rc.build(case_id)
    ref = rc.reference(case_id)
    eng = _engine(dom)
    judge = _Judge(case_id, kw["family"], nans="plants" in kw)
    run = {"fixed": _fixed, "ring": _fixed, "moving": _moving, "packed": _moving, "steps": _steps}[kw["kind"]]
    if "plants" in kw:          # one NaN at a time: the planted fields are uploaded per plant (small), the engine is the domain's
        for plant in kw["plants"]:
            d = rc.planted(dom, plant)
            run(judge, d, [_up(a) for a in (d.tair, d.u, d.v, d.omega, d.geopt)], eng, boxes, kw, ref[plant[0]], label=plant[0] + ": ")
    else:
        run(judge, dom, _dom_fields(dom), eng, boxes, kw, ref)
    judge.finish()


@pytest.mark.parametrize("case_id", rc.FAMILY_IDS["sweep"])
def test_sweep(case_id):
    """One wave per row: every vector form x alignment shift, widths across every change of the trip structure; five launch modes."""
    _guarded(_run, case_id)


@pytest.mark.parametrize("case_id", rc.FAMILY_IDS["block"])
def test_block(case_id):
    """lec_rowblock_kernel: block shapes 212 / 222 / 122 with partial blocks along time, level and latitude; whole and as a shard."""
    _guarded(_run, case_id)


@pytest.mark.parametrize("case_id", rc.FAMILY_IDS["tile"])
def test_tile(case_id):
    """lec_boxtile_kernel: a box per step on a cube; and the boxes of three tracks over one cube through a step table."""
    _guarded(_run, case_id)


@pytest.mark.parametrize("case_id", rc.FAMILY_IDS["plane"])
def test_plane(case_id):
    """lec_boxplane_kernel: a box-packed series, NaN beside every box in its slab."""
    _guarded(_run, case_id)


def test_ring_shapes_are_the_ring_tests():
    from tests import test_gpu_ring
    assert [(nx, np.dtype(d).name, v) for nx, d, v in test_gpu_ring.SHAPES] == [tuple(s) for s in rc.RING_SHAPES]


@pytest.mark.parametrize("case_id", rc.FAMILY_IDS["ring"])
def test_ring(case_id):
    """lec_rowstats_ring at the widths of tests/test_gpu_ring.py; the latitudes outside the band are NaN."""
    _guarded(_run, case_id)


@pytest.mark.parametrize("case_id", rc.FAMILY_IDS["axes"])
def test_axes(case_id):
    """Uneven latitudes, levels and time steps: the coefficient triples of lattab, levtab and tcoef are asymmetric."""
    _guarded(_run, case_id)


@pytest.mark.parametrize("case_id", rc.FAMILY_IDS["conditioning"])
def test_conditioning(case_id):
    """Rows that strain the shift of the single-sweep form: eddies of a thousandth of the mean, and a west column (the shift) 30 row
    standard deviations away from the row."""
    _guarded(_run, case_id)


@pytest.mark.parametrize("case_id", rc.FAMILY_IDS["nan"])
def test_nan(case_id):
    """One NaN at a time inside the box: at the row's first, a middle-trip and last element, and in T one row, level and step away."""
    _guarded(_run, case_id)


def test_zz_worst_ratios():
    """Prints the worst ratio to the bars per family (the figures DESIGN.md section 4.1 quotes); runs last in the module."""
    for fam, (m, mean) in _worst.items():
        print(f"{fam}: worst moments {m:.3f} of the 1e-11 bar, worst mean {mean:.3f} of its bound")
