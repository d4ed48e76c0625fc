"""Follow conformance: the kernels of csrc/lec_follow.hip (and lec_diag.hip's LDS tree) against the index-level restatement of
tests/follow_cases.py, on the cases that module names -- the workgroup partition of the window, the tie rule across lanes, waves and
trips, every kind of clipping, missing values, the ring's tile runs, the seeds' selection and the capped grid of the series kernels.
tests/test_follow_cases_cpu.py proves that every case reaches the seam it is named for.

The C ABI is driven directly through the ``_lib`` structs (``_chain_call``, ``_seeds_call``): follow.py's degree-based wrappers cannot
state ``hgt`` with LEC_FOLLOW_MAX or bounds on the slice's edge.  The vorticity tables come from ``diagnostics.vorticity_tables``.

The measure.  hgt cases: positions, status, span, state, n_found and the (-2, -2) / NaN marks EQUAL, values equal bit for bit (the
fields are small integers: every sum is exact, every mean one division).  zeta cases: positions equal, values within VALUE_BAR of the
tile's scale, the restatement's margin above NEAR_TIE (both from tests/test_gpu_follow.py).  No other tolerance."""
import ctypes as C
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from lorenzcycletoolkit_amd import _lib
from lorenzcycletoolkit_amd import diagnostics as dg
from tests import follow_cases as fc
from tests import test_gpu_follow as tgf

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WALKING = 1
_dead, _tables, _zeros, _t0 = [], {}, {}, [None]


def _guarded(run, *what):
    """A case that ends in anything but a failed assertion (a HIP error) stops the module: nothing more is started on the device."""
    if _dead:
        pytest.fail(f"{_dead[0]} ended in an error of the device or the library: not run")
    if _t0[0] is None:
        _t0[0] = time.perf_counter()
    try:
        run(*what)
    except (AssertionError, pytest.skip.Exception):
        raise
    except BaseException:
        _dead.append(str(what))
        raise


def _up(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tabs(ny, nx, ring=False, form="metpy_no_crs"):
    """The vorticity tables of a plain 1-degree grid (the ring grid: its own axes), uploaded once; hgt calls need them too."""
    key = (ny, nx, ring, form)
    if key not in _tables:
        lat, lon = (fc.RING_LAT, fc.RING_LON) if (ny, nx) == (fc.RING_NY, fc.RING_NX) else (fc.LAT[0] + np.arange(ny), fc.LON[0] + np.arange(nx))
        _tables[key] = [_up(a) for a in dg.vorticity_tables(lat, lon, form, periodic=ring)]
    return _tables[key]


def _zero(n):
    """One shared zero array: u_d and v_d of every hgt call."""
    if _zeros.get("n", 0) < n:
        _zeros["z"], _zeros["n"] = torch.zeros(n, dtype=torch.float64, device=DEV), n
    return _zeros["z"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_values(got, want):
    """Bit for bit where the reference is a number, NaN where it is NaN."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


# ---------------------------------------------------------------------------------------------------------------------------------
# the chain calls
# ---------------------------------------------------------------------------------------------------------------------------------
def _fields(c, ring):
    """(u, v, h) of a case on the device, [nt][ny][nx]; hgt cases share one zero array for u and v."""
    if c["field"] == "zeta":
        return _up(c["u"]), _up(c["v"]), None
    z = _zero(c["F"].size)
    return z, z, _up(c["F"])


def _scalars(c, nt, ny, nx, ring):
    xc, yc, cv = _tabs(ny, nx, ring, c.get("form", "metpy_no_crs"))
    jlo, jhi, ilo, ihi = c["bounds"]
    return dict(nt=nt, ny=ny, nx=nx, field=_lib.FOLLOW_ZETA if c["field"] == "zeta" else _lib.FOLLOW_HGT, xcoef_d=_ptr(xc), ycoef_d=_ptr(yc),
                curv_d=_ptr(cv), sense=c["sense"], smooth_r=c["r"], sj=c["sj"], si=c["si"], jlo=jlo, jhi=jhi, ilo=ilo, ihi=ihi, stream=_stream())


def _chain_call(entry, c):
    """One case through one entry point -> dict(pos [nt][2], val [nt], status [nt], and span / state where the call has them)."""
    lib = _lib.load()
    ring = entry.startswith("ring")
    nt, ny, nx = c["F"].shape
    u, v, h = _fields(c, ring)
    start = tuple(int(x) for x in c["start"])
    nch = 2 if entry == "many" else 1                          # lec_follow_many: the same chain twice -- its bits do not depend on its company
    pos = torch.full((nch, nt, 2), -7, dtype=torch.int32, device=DEV)
    val = torch.full((nch, nt), -7.0, dtype=torch.float64, device=DEV)
    status = torch.full((nch, nt), -7, dtype=torch.int32, device=DEV)
    span = torch.full((nch, 2), -7, dtype=torch.int32, device=DEV)
    out = {}

    if entry == "follow":
        args = _lib.FollowArgs(u_d=_ptr(u), v_d=_ptr(v), hgt_d=_ptr(h), j_start=start[0], i_start=start[1], pos_d=_ptr(pos), val_d=_ptr(val),
                               status_d=_ptr(status), **_scalars(c, nt, ny, nx, ring))
        _lib.check(lib.lec_follow(C.byref(args)), "lec_follow")
    elif entry == "many":
        st = _up([start, start], np.int32)
        args = _lib.FollowManyArgs(u_d=_ptr(u), v_d=_ptr(v), hgt_d=_ptr(h), n_chains=nch, reserved0=0, start_d=_ptr(st), pos_d=_ptr(pos),
                                   val_d=_ptr(val), status_d=_ptr(status), **_scalars(c, nt, ny, nx, ring))
        _lib.check(lib.lec_follow_many(C.byref(args)), "lec_follow_many")
    elif entry == "spans":
        st = _up([(0,) + start], np.int32)
        args = _lib.FollowSpansArgs(u_d=_ptr(u), v_d=_ptr(v), hgt_d=_ptr(h), n_chains=1, patience=nt + 1, start_d=_ptr(st),
                                    end_threshold=float("nan"), pos_d=_ptr(pos), val_d=_ptr(val), status_d=_ptr(status), span_d=_ptr(span),
                                    **_scalars(c, nt, ny, nx, ring))
        _lib.check(lib.lec_follow_spans(C.byref(args)), "lec_follow_spans")
        out["span"] = span
    else:                                                      # "chunk", "ring", "ring-cut": the resumed form, patience 0: never stops
        fn = lib.lec_follow_spans_chunk if entry == "chunk" else lib.lec_follow_spans_chunk_ring
        cuts = [0, nt] if entry == "ring" or nt < 2 else [0, nt // 2, nt]      # a cut in the middle wherever there are two steps
        st = _up([(0,) + start], np.int32)
        state = torch.zeros((1, 8), dtype=torch.int32, device=DEV)
        keep = []
        for a, b in zip(cuts, cuts[1:]):
            p = torch.full((1, b - a, 2), -7, dtype=torch.int32, device=DEV)
            w = torch.full((1, b - a), -7.0, dtype=torch.float64, device=DEV)
            s = torch.full((1, b - a), -7, dtype=torch.int32, device=DEV)
            plane = ny * nx
            cut = lambda t: None if t is None else _ptr(t.reshape(-1)[a * plane:])
            args = _lib.FollowChunkArgs(u_d=cut(u), v_d=cut(v), hgt_d=cut(h), n_chains=1, patience=0, start_d=_ptr(st), end_threshold=float("nan"),
                                        pos_d=_ptr(p), val_d=_ptr(w), status_d=_ptr(s), span_d=_ptr(span), t_base=a, state_d=_ptr(state),
                                        **_scalars(c, b - a, ny, nx, ring))
            _lib.check(fn(C.byref(args)), "lec_follow_spans_chunk" + ("" if entry == "chunk" else "_ring"))
            keep.append((p, w, s))
        pos, val, status = (torch.cat([k[q] for k in keep], dim=1) for q in range(3))
        out["span"], out["state"] = span, state
    torch.cuda.synchronize()
    out = {k: t.cpu().numpy() for k, t in out.items()}
    pos, val, status = pos.cpu().numpy(), val.cpu().numpy(), status.cpu().numpy()
    if nch == 2:
        assert np.array_equal(pos[0], pos[1]) and np.array_equal(_bits(val[0]), _bits(val[1])) and np.array_equal(status[0], status[1]), \
            f"{c['id']}: two chains of one start differ"
    out.update(pos=pos[0], val=val[0], status=status[0])
    return out


def _judge_chain(c, entry, got, ref):
    """-> a list of what is wrong (empty: nothing)."""
    bad, what = [], f"{c['id']} [{entry}]"
    if not np.array_equal(got["status"], ref["status"]):
        return [f"{what}: status {got['status'].tolist()} != {ref['status'].tolist()}"]
    if not np.array_equal(got["pos"], ref["pos"]):
        bad.append(f"{what}: pos {got['pos'].tolist()} != {ref['pos'].tolist()}")
    if c["field"] == "hgt":
        if not _same_values(got["val"], ref["val"]):
            bad.append(f"{what}: val {got['val'].tolist()} != {ref['val'].tolist()} (bit for bit)")
    else:
        ok = ref["status"] == 0
        err = np.abs(got["val"][ok] - ref["val"][ok]) / ref["tile_scale"][ok]
        print(f"{what}: margin {ref['margin'].min():.3e}, value error / tile scale {err.max() if err.size else 0.0:.3e}")
        assert ref["margin"].min() > tgf.NEAR_TIE, (what, ref["margin"])
        if not (np.all(np.isnan(got["val"][~ok])) and np.all(err <= tgf.VALUE_BAR)):
            bad.append(f"{what}: val {got['val'].tolist()} beyond {tgf.VALUE_BAR} of {ref['val'].tolist()}")
    if "span" in got:
        span, weak = fc.spans_of(ref["status"])
        if tuple(got["span"][0]) != span:
            bad.append(f"{what}: span {got['span'][0].tolist()} != {span}")
        if "state" in got:
            want = [WALKING, int(ref["pos"][-1][0]), int(ref["pos"][-1][1]), weak, span[0], span[1], 0, 0]
            if got["state"][0].tolist() != want:
                bad.append(f"{what}: state {got['state'][0].tolist()} != {want}")
    return bad


def _run_family(family, entries, sense):
    bad, n = [], 0
    for cid in fc.CHAIN_FAMILIES[family]:
        c = fc.case(cid)
        if c["sense"] != sense:
            continue
        for entry in entries:
            if entry in ("spans", "chunk") and tuple(c["start"]) == (-1, -1):
                continue                                       # a born chain always has a start
            ref = fc.reference(cid, True) if entry.startswith("ring") else fc.reference(cid)
            bad += _judge_chain(c, entry, _chain_call(entry, c), ref)
            n += 1
    print(f"{family}, sense {sense}: {n} chains")
    assert not bad, "\n".join(bad[:20]) + (f"\n... ({len(bad)} in all)" if len(bad) > 20 else "")


def test_constants_are_the_follow_tests():
    assert (fc.NEAR_TIE, fc.VALUE_BAR) == (tgf.NEAR_TIE, tgf.VALUE_BAR)


@pytest.mark.parametrize("sense", [fc.MIN, fc.MAX])
def test_partition(sense):
    """Windows of 9 .. 513 points, the unique extremum at the first and last index of every wave and trip: lec_follow with a start (the
    tile path) and without one (the strided scan of all admissible centres), and the same through lec_follow_many."""
    _guarded(_run_family, "partition", ("follow", "many"), sense)


@pytest.mark.parametrize("sense", [fc.MIN, fc.MAX])
def test_ties(sense):
    """Equal extremes across lanes, waves, a thread's trips: all five chain entry points (kPlain twice, kSpans, kResume with a cut in the
    middle, kRing -- whose second window is not cut at the slice's edge, and is judged by the ring rule)."""
    _guarded(_run_family, "ties", ("follow", "many", "spans", "chunk", "ring", "ring-cut"), sense)


@pytest.mark.parametrize("sense", [fc.MIN, fc.MAX])
def test_clip(sense):
    """Windows cut by the bounds, tiles cut by the slice, r > sj, the window that is all admissible centres, a one-row band; zeta at the
    slice's corners in both formulations."""
    _guarded(_run_family, "clip", ("follow", "chunk"), sense)


@pytest.mark.parametrize("sense", [fc.MIN, fc.MAX])
def test_missing(sense):
    """+-inf never wins and never enters a mean; an all-NaN neighbourhood is skipped; one finite point; a blind step keeps the centre."""
    _guarded(_run_family, "missing", ("follow", "many", "chunk"), sense)


@pytest.mark.parametrize("sense", [fc.MIN, fc.MAX])
def test_ring(sense):
    """lec_follow_spans_chunk_ring: every kind of tile run, the tile that is the whole ring, the tie across the seam."""
    _guarded(_run_family, "ring", ("ring", "ring-cut"), sense)


def _ring_rolled():
    """Kernel against kernel: the first step of every ring case equals lec_follow_spans_chunk on the data rolled until the window and
    its tile lie inside the slice (the centre in column 12), with the column rolled back."""
    bad = []
    for cid in fc.CHAIN_FAMILIES["ring"]:
        c = fc.case(cid)
        shift = 12 - c["start"][1]
        flat = dict(c, id=cid + "-rolled", F=np.roll(c["F"][:1], shift, axis=2), start=(c["start"][0], 12), ring=False)
        ln = fc.launch_numbers(fc.RING_NY, fc.RING_NX, c["r"], c["sj"], c["si"], c["bounds"], flat["start"])
        assert not (ln["window_cut"]["west"] or ln["window_cut"]["east"] or ln["tile_cut"]["west"] or ln["tile_cut"]["east"])
        one = dict(c, F=c["F"][:1])
        a, b = _chain_call("ring", one), _chain_call("chunk", flat)
        back = [int(b["pos"][0][0]), int((b["pos"][0][1] - shift) % fc.RING_NX)]
        if a["pos"][0].tolist() != back or not np.array_equal(_bits(a["val"]), _bits(b["val"])) or a["status"][0] != b["status"][0]:
            bad.append(f"{cid}: ring {a['pos'][0].tolist()} {a['val']} != rolled {back} {b['val']}")
    assert not bad, "\n".join(bad)


def test_ring_is_the_plain_kernel_on_rolled_data():
    _guarded(_ring_rolled)


# ---------------------------------------------------------------------------------------------------------------------------------
# lec_track_diag: its LDS tree is a separate implementation of the same tie rule
# ---------------------------------------------------------------------------------------------------------------------------------
def _diag_cross_check():
    ids = [cid for fam in ("partition", "ties", "missing") for cid in fc.CHAIN_FAMILIES[fam] if fc.case(cid)["r"] == 0]
    boxes, fields = zip(*(fc.diag_inputs(cid) for cid in ids))
    box, F = _up(np.concatenate(boxes)), _up(np.concatenate(fields))
    n = int(F.shape[0])
    xc, yc, cv = _tabs(fc.NY, fc.NX)
    val = torch.full((n, 5), -7.0, dtype=torch.float64, device=DEV)
    pos = torch.full((n, 8), -7, dtype=torch.int32, device=DEV)
    zero = _zero(F.numel())
    # height minimum: h = the field; wind-speed maximum: u = the (non-negative integer) field, v = 0 -- sqrt(u u) = u exactly
    args = _lib.DiagArgs(u_d=_ptr(F), v_d=_ptr(zero), hgt_d=_ptr(F), nt=n, ny=fc.NY, nx=fc.NX, reserved0=0, box_d=_ptr(box), xcoef_d=_ptr(xc),
                         ycoef_d=_ptr(yc), curv_d=_ptr(cv), val_d=_ptr(val), pos_d=_ptr(pos), stream=_stream())
    _lib.check(_lib.load().lec_track_diag(C.byref(args)), "lec_track_diag")
    torch.cuda.synchronize()
    val, pos = val.cpu().numpy(), pos.cpu().numpy()
    bad, at = [], 0
    for cid in ids:
        c, ref = fc.case(cid), fc.reference(cid)
        nt = c["F"].shape[0]
        q = 2 if c["sense"] == fc.MIN else 3                   # val[2] / pos[4:6]: height minimum; val[3] / pos[6:8]: wind maximum
        gv, gp = val[at: at + nt, q], pos[at: at + nt, 2 * q: 2 * q + 2]
        want = np.where((ref["status"] == 0)[:, None], ref["pos"], -1)          # a blind box: no position here, a kept centre there
        if not (_same_values(gv, ref["val"]) and np.array_equal(gp, want)):
            bad.append(f"{cid}: lec_track_diag {gp.tolist()} {gv.tolist()} != {want.tolist()} {ref['val'].tolist()}")
        at += nt
    print(f"lec_track_diag: {len(ids)} cases, {n} boxes")
    assert not bad, "\n".join(bad[:20]) + (f"\n... ({len(bad)} in all)" if len(bad) > 20 else "")


def test_lec_track_diag_agrees_on_the_windows():
    """Every partition, ties and missing case with r = 0: the box equal to the window gives the MIN case's value and position as the
    height minimum and the MAX case's as the wind-speed maximum, bit for bit."""
    _guarded(_diag_cross_check)


# ---------------------------------------------------------------------------------------------------------------------------------
# seeds
# ---------------------------------------------------------------------------------------------------------------------------------
def _seeds_call(c, F, series, ring=False):
    """F [ny][nx] through lec_follow_seeds, or [nt][ny][nx] through a series call -> (pos [nt][k][2], val [nt][k], n_found [nt])."""
    lib = _lib.load()
    nt = int(F.shape[0]) if series else 1
    ny, nx = (int(x) for x in F.shape[-2:])
    k = c["k_max"]
    z = _zero(F.numel())
    xc, yc, cv = _tabs(ny, nx, ring)
    jlo, jhi, ilo, ihi = c["bounds"]
    work = torch.empty(nt * ny * nx, dtype=torch.float64, device=DEV)
    pos = torch.full((nt, k, 2), -7, dtype=torch.int32, device=DEV)
    val = torch.full((nt, k), -7.0, dtype=torch.float64, device=DEV)
    nf = torch.full((nt,), -7, dtype=torch.int32, device=DEV)
    kw = dict(u_d=_ptr(z), v_d=_ptr(z), hgt_d=_ptr(F), ny=ny, nx=nx, field=_lib.FOLLOW_HGT, sense=c["sense"], xcoef_d=_ptr(xc), ycoef_d=_ptr(yc),
              curv_d=_ptr(cv), smooth_r=c["r"], ej=c["ej"], ei=c["ei"], k_max=k, jlo=jlo, jhi=jhi, ilo=ilo, ihi=ihi,
              threshold=float("nan") if c["threshold"] is None else c["threshold"], work_d=_ptr(work), seed_pos_d=_ptr(pos), seed_val_d=_ptr(val),
              n_found_d=_ptr(nf), stream=_stream())
    if series:
        fn, name = (lib.lec_follow_seeds_series_ring, "lec_follow_seeds_series_ring") if ring else (lib.lec_follow_seeds_series, "lec_follow_seeds_series")
        _lib.check(fn(C.byref(_lib.FollowSeedsSeriesArgs(nt=nt, reserved0=0, **kw))), name)
    else:
        assert not ring
        _lib.check(lib.lec_follow_seeds(C.byref(_lib.FollowSeedsArgs(**kw))), "lec_follow_seeds")
    return pos, val, nf


def _judge_seeds(what, got, ref):
    pos, val, nf = got
    if int(nf) != ref["n_found"] or not np.array_equal(pos, ref["pos"]) or not _same_values(val, ref["val"]):
        k = max(int(nf), ref["n_found"]) + 1
        return [f"{what}: n_found {int(nf)} != {ref['n_found']}, or seeds {pos[:k].tolist()} {val[:k].tolist()} != {ref['pos'][:k].tolist()} {ref['val'][:k].tolist()}"]
    return []


def _run_seeds(family):
    """Every case alone (lec_follow_seeds; on the ring a series of one step) against the restatement; then the cases that share their
    scalars stacked as the steps of ONE series call, there and back, bit for bit against the single calls, marks included."""
    bad, single, groups = [], {}, {}
    for cid in fc.SEED_FAMILIES[family]:
        c = fc.case(cid)
        F = _up(c["F"])
        pos, val, nf = _seeds_call(c, F[None] if c["ring"] else F, c["ring"], c["ring"])
        torch.cuda.synchronize()
        single[cid] = (pos[0].cpu().numpy(), val[0].cpu().numpy(), nf[0].cpu().numpy())
        bad += _judge_seeds(cid, single[cid], fc.reference(cid))
        key = (c["sense"], c["r"], c["ej"], c["ei"], c["k_max"], c["threshold"], c["bounds"], c["ring"])
        groups.setdefault(key, []).append(cid)
    for ids in groups.values():
        steps = ids + ids[::-1]
        c = fc.case(ids[0])
        pos, val, nf = _seeds_call(c, _up(np.stack([fc.case(i)["F"] for i in steps])), True, c["ring"])
        torch.cuda.synchronize()
        pos, val, nf = pos.cpu().numpy(), val.cpu().numpy(), nf.cpu().numpy()
        for t, cid in enumerate(steps):
            p, v, n = single[cid]
            if not (np.array_equal(pos[t], p) and np.array_equal(_bits(val[t]), _bits(v)) and nf[t] == n):
                bad.append(f"{cid} as step {t} of {len(steps)}: the series call differs from the single call")
    print(f"{family}: {len(single)} slices, {len(groups)} series calls")
    assert not bad, "\n".join(bad[:20]) + (f"\n... ({len(bad)} in all)" if len(bad) > 20 else "")


@pytest.mark.parametrize("family", sorted(fc.SEED_FAMILIES))
def test_seeds(family):
    _guarded(_run_seeds, family)


def _capped_grid():
    """lec_follow_seeds_series with nt ny nx = 2^24 + 4096: the smooth and the candidate kernel run out of their 2^16 workgroups and
    stride.  Every step against lec_follow_seeds on its pattern (on the device); four steps against the restatement."""
    free = torch.cuda.mem_get_info()[0]
    if free < 1 << 30:
        pytest.skip(f"the capped-grid case allocates about 400 MB in arrays of 134 MB: {free >> 20} MiB of device memory are free")
    cp = fc.CAPPED
    c = dict(sense=fc.MIN, r=0, ej=1, ei=1, k_max=cp["k_max"], threshold=None, bounds=(0, cp["ny"] - 1, 0, cp["nx"] - 1))
    pats = fc.capped_patterns()
    P = len(pats)
    assert cp["nt"] * cp["ny"] * cp["nx"] > fc.SERIES_GRID * fc.THREADS
    series = np.tile(pats, (cp["nt"] // P + 1, 1, 1))[: cp["nt"]]
    pos, val, nf = _seeds_call(c, _up(series), True)
    one = [_seeds_call(c, _up(p), False) for p in pats]
    torch.cuda.synchronize()
    idx = torch.arange(cp["nt"], device=DEV) % P
    spos, sval, snf = (torch.cat([o[q] for o in one]) for q in range(3))
    assert torch.equal(nf, snf[idx]), "n_found of some step differs from lec_follow_seeds on its pattern"
    assert torch.equal(pos, spos[idx]), "seed positions of some step differ from lec_follow_seeds on its pattern"
    assert torch.equal(val.view(torch.int64), sval[idx].view(torch.int64)), "seed values (or marks) of some step differ bit for bit"
    bad = []
    for t in fc.capped_steps():
        ref = fc.seeds(pats[t % P], fc.MIN, 0, 1, 1, cp["k_max"], None, c["bounds"])
        bad += _judge_seeds(f"capped grid, step {t}", (pos[t].cpu().numpy(), val[t].cpu().numpy(), nf[t].cpu().numpy()), ref)
    assert not bad, "\n".join(bad)
    _zeros.clear()                                             # (the 134 MB zero array is given back)


def test_series_beyond_the_capped_grid():
    _guarded(_capped_grid)


def test_zz_wall_time():
    """Prints the module's wall time from its first device call (the figure DESIGN.md section 4.7 quotes); runs last."""
    if _t0[0] is not None:
        torch.cuda.synchronize()
        print(f"follow conformance: {time.perf_counter() - _t0[0]:.1f} s")
