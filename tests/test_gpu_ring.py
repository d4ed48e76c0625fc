"""-f --periodic on the GPU: ``lec_rowstats_ring`` (one wave per row with the RING parameter) against the CPU restatement of the
closed axis (tests/ring_restatement.py), at the row widths where the edge trips and the vector forms change.  A trip is 64 lanes x
VEC: VEC 2 for aligned fp64 rows, else 1; fp32 storage 4 / 2 / 1.  Grids of 3 steps x 4 levels x 5 latitudes.

Tolerance: 1e-9 of each term's scale, the bar of the fixed-box parity tests, for scalars and level tables alike;
for fp32 storage the restatement is fed the float32-rounded fields as fp64."""
import argparse
import os
import shutil
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import _lib
from lorenzcycletoolkit_amd import dataset as ds
from lorenzcycletoolkit_amd import ingest
from lorenzcycletoolkit_amd.engine import LECEngine
from oracle import lec_oracle as o
from tests import ring_restatement as rr
from tests.helpers import SCALARS, as_f64, scale_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lorenzcycletoolkit.py")
TOL = 1e-9
DEV = "cuda:0"
NT, NL, NY = 3, 4, 5
SOUTH, NORTH = -60.0, 60.0
# (columns, storage, tuning.f32_vec): fp64 -- 7 / 8: one trip, odd / even; 64 / 65: one element into a second trip with VEC 1; 128: the
# last element in the last lane of a trip (its eastern neighbour takes the scalar path); 129, 130.  fp32 -- 256, 260 (float4), 258
# (float2), 257 (scalar), 260 again with float2 forced.
SHAPES = [(7, np.float64, 0), (8, np.float64, 0), (64, np.float64, 0), (65, np.float64, 0), (128, np.float64, 0), (129, np.float64, 0),
          (130, np.float64, 0), (256, np.float32, 0), (260, np.float32, 0), (258, np.float32, 0), (257, np.float32, 0), (260, np.float32, 2)]
IDS = [f"{nx}-{np.dtype(d).name}" + ("-f32vec2" if v else "") for nx, d, v in SHAPES]
NO_Q = ["Az", "Ae", "Kz", "Ke", "Cz", "Ca", "Ck", "Ce", "BAz", "BAe", "BKz", "BKe", "BΦZ", "BΦE"]
BOUNDARY = ["BAz", "BAe", "BKz", "BKe"]

_cache = {}


def _case(nx, dtype):
    """(domain, its fp64 twin for the restatement, a dT/dt cube in the storage dtype) of one shape -- built once per module."""
    key = (nx, np.dtype(dtype).name)
    if key not in _cache:
        dom = rr.ring_domain(NT, NL, NY, nx, seed=nx, dtype=dtype, lat0=SOUTH, lat1=NORTH)
        d64 = as_f64(dom)
        dtdt = np.ascontiguousarray(o.differentiate(d64.tair, dom.time_s, axis=0).astype(dtype))
        _cache[key] = {"dom": dom, "d64": d64, "dtdt": dtdt, "ref": {}}
    return _cache[key]


def _reference(c, mode):
    """The restatement's (scalars, level tables) of one dT/dt mode, computed once and shared."""
    if mode not in c["ref"]:
        kw = {"cube": dict(dTdt=c["dtdt"].astype(np.float64)), "no_geopt": dict(with_geopt=False)}.get(mode, {})
        c["ref"][mode] = rr.ring_terms(c["d64"], SOUTH, NORTH, **kw)
    return c["ref"][mode]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _engine(dom):
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    return eng, eng.prepare_boxes([(0, dom.lon.size - 1, 0, dom.lat.size - 1)], ring=True)


def _compute(eng, pb, dom, mode, dtdt=None, tuning=None, **kw):
    f = [_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega)]
    geopt = None if mode == "no_geopt" else _dev(dom.geopt)
    if mode == "no_q":
        return eng.compute(*f, geopt, pb, with_q=False, keep_rows=True, tuning=tuning, **kw)
    if mode == "cube":
        return eng.compute(*f, geopt, pb, dTdt=_dev(dtdt), keep_rows=True, tuning=tuning, **kw)
    return eng.compute(*f, geopt, pb, time_s=dom.time_s, keep_rows=True, tuning=tuning, **kw)


def _check(res, ref, what, names=SCALARS, skip_levels=()):
    got_s, got_l = res.scalars_dict(), res.levels_dict()
    worst = {n: scale_err(got_s[n], ref[0][n]) for n in names}
    for n, r in ref[1].items():
        if n in skip_levels:
            continue
        r = np.asarray(r, dtype=np.float64)
        worst["lv:" + n] = scale_err(got_l[n], np.broadcast_to(r, got_l[n].shape) if r.ndim == 1 else r)
    print(f"{what}: worst {max(worst.values()):.2e} of scale ({max(worst, key=worst.get)})")
    bad = {k: v for k, v in worst.items() if not v <= TOL}
    assert not bad, f"{what}: beyond {TOL:g} of scale: {bad}"
    return worst


def _same_bits(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("nx, dtype, vec", SHAPES, ids=IDS)
def test_parity_and_edge_values(nx, dtype, vec):
    """All 16 scalars and 21 level tables against the restatement in every dT/dt mode a fixed box reaches, through the AUTO and the
    ROW_SWEEP request (bit-identical records); the east columns of every record carry the west columns' bits."""
    c = _case(nx, dtype)
    dom = c["dom"]
    eng, pb = _engine(dom)
    for mode in ("no_q", "stencil", "cube", "no_geopt"):
        ref = _reference(c, "stencil" if mode == "no_q" else mode)
        res = {}
        for kernel in ("auto", "row_sweep"):
            tuning = dict(kernel=kernel, f32_vec=vec)
            res[kernel] = r = _compute(eng, pb, dom, mode, dtdt=c["dtdt"], tuning=tuning)
            what = f"ring nx={nx} {np.dtype(dtype).name} vec={vec} {mode} {kernel}"
            if mode == "no_q":
                _check(r, ref, what, names=NO_Q, skip_levels=("Gz", "Ge"))
                got = r.scalars_dict()
                assert np.all(got["Gz"] == 0) and np.all(got["Ge"] == 0)
            else:
                worst = _check(r, ref, what)
                assert all(worst[n] <= TOL for n in BOUNDARY)      # the restatement's east-west parts are exactly 0
            rows = r.rows
            assert rows.shape == (NT, NL, NY, _lib.LEC_NSTAT)
            for w, e in ((22, 23), (24, 25), (26, 27)):          # LEC_S_TW / TE, UW / UE, VW / VE (include/lec_hip.h)
                assert _same_bits(rows[..., e], rows[..., w]), (what, e)
            assert int(r.nanflag.sum()) == 0
        assert _same_bits(res["auto"].rows, res["row_sweep"].rows), f"nx={nx} {mode}: AUTO and ROW_SWEEP records differ"
        assert _same_bits(res["auto"].packed, res["row_sweep"].packed)


@pytest.mark.parametrize("nx, dtype, vec", SHAPES, ids=IDS)
def test_rotation(nx, dtype, vec):
    """A ring has no preferred meridian: the fields rolled by 1, nx / 2 and nx - 1 columns give every term of the unrolled restatement."""
    c = _case(nx, dtype)
    eng, pb = _engine(c["dom"])
    ref = _reference(c, "stencil")
    for k in (1, nx // 2, nx - 1):
        res = _compute(eng, pb, rr.rolled(c["dom"], k), "stencil", tuning=dict(f32_vec=vec))
        _check(res, ref, f"ring nx={nx} {np.dtype(dtype).name} vec={vec} rolled by {k}")


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    (tmp_path / "inputs" / "namelist").write_text(rr.RING_NAMELIST)
    (tmp_path / "inputs" / "box_limits").write_text(f"min_lon;-180\nmax_lon;180\nmin_lat;{SOUTH}\nmax_lat;{NORTH}\n")
    monkeypatch.chdir(tmp_path)
    return tmp_path


@pytest.mark.parametrize("nx, dtype, vec", SHAPES, ids=IDS)
def test_time_split_and_streamed_chunks(nx, dtype, vec, workdir):
    """The series split at every step by t_begin / t_count gives the whole series' row records bit for bit; the streamed ingest, chunk
    by chunk (one step per chunk), gives its packed results bit for bit."""
    c = _case(nx, dtype)
    dom = c["dom"]
    eng, pb = _engine(dom)
    tuning = dict(f32_vec=vec)
    for mode in ("stencil", "cube", "no_q"):
        whole = _compute(eng, pb, dom, mode, dtdt=c["dtdt"], tuning=tuning)
        for t in range(NT):
            part = _compute(eng, pb, dom, mode, dtdt=c["dtdt"], tuning=tuning, t_begin=t, t_count=1)
            # (slots 28..31 are stage 1's scratch, not an interface: the first step of a launch leaves its backward covariance there)
            assert _same_bits(part.rows[..., :28], whole.rows[t:t + 1, ..., :28]), f"nx={nx} {mode}: step {t} alone differs from the whole series"
            assert _same_bits(part.scalars, whole.scalars[t:t + 1]) and _same_bits(part.levels, whole.levels[t:t + 1]), (nx, mode, t)
    if vec:
        return                      # (the streamed path takes the library's own vector choice)
    whole = _compute(eng, pb, dom, "stencil")
    path = str(workdir / "ring.nc")
    rr.write_ring_file(path, dom)
    df = ds.read_namelist("inputs/namelist")
    raw = ds.open_raw(path, df)
    try:
        plan = ingest.make_plan(raw, argparse.Namespace(fixed=True, track=False, trackfile=None, residuals=True))
        assert np.array_equal(plan.lon, dom.lon) and np.array_equal(plan.lat, dom.lat) and np.array_equal(plan.level, dom.level)
        stats = {}
        st = ingest.lec_streamed(raw, plan, df, [(-180.0, 180.0, SOUTH, NORTH)], device=DEV, chunk_steps=1, stats=stats, ring=True)
        torch.cuda.synchronize()
    finally:
        raw.close()
    assert stats["chunks"] >= 2
    assert _same_bits(st.scalars, whole.scalars) and _same_bits(st.levels, whole.levels) and torch.equal(st.nanflag, whole.nanflag)


@pytest.mark.parametrize("nx, dtype, vec", SHAPES, ids=IDS)
def test_nan_patch_across_the_seam(nx, dtype, vec):
    """A below-ground NaN patch over the columns nx - 2 .. 1, across the seam, at the lowest level: the restatement's numbers, NaN at
    the same levels.  nanflag: lec_reduce is untouched and counts per level function; the patch covers both seam columns, so every
    level function is NaN at the same levels in the ring and in the limited-area evaluation of the same cubes -- the same counts."""
    c = _case(nx, dtype)
    cut = lambda a: a.copy()
    dom = o.Domain(cut(c["dom"].tair), cut(c["dom"].u), cut(c["dom"].v), cut(c["dom"].omega), cut(c["dom"].geopt), c["dom"].lat,
                   c["dom"].lon, c["dom"].level, c["dom"].time_s)
    for f in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt):
        f[1:, NL - 1, 1:3, nx - 2:] = np.nan
        f[1:, NL - 1, 1:3, :2] = np.nan
    eng, pb = _engine(dom)
    res = _compute(eng, pb, dom, "stencil", tuning=dict(f32_vec=vec))
    with np.errstate(invalid="ignore"):
        ref = rr.ring_terms(as_f64(dom), SOUTH, NORTH)
    _check(res, ref, f"ring nx={nx} {np.dtype(dtype).name} vec={vec} NaN patch across the seam")
    got = res.scalars_dict()
    assert all(np.isfinite(got[k]).all() for k in SCALARS)
    plain = eng.compute(*[_dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)], [(0, nx - 1, 0, NY - 1)], time_s=dom.time_s,
                        tuning=dict(f32_vec=vec))
    assert int(res.nanflag.min()) > 0 and torch.equal(res.nanflag, plain.nanflag)


# -- the command line -------------------------------------------------------------------------------------------------------------
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


def test_cli_periodic(workdir):
    """-r -f --periodic on a synthetic ring file with host ingest, device ingest and two ranks on one card: three byte-identical trees,
    the restatement's numbers; the plain -f run of the same file differs and logs the hint."""
    dom = rr.cli_domain()
    (workdir / "inputs" / "box_limits").write_text("min_lon;-180\nmax_lon;180\nmin_lat;-30\nmax_lat;30\n")
    path = str(workdir / "ring.nc")
    rr.write_ring_file(path, dom)
    results = workdir / "LEC_Results" / "ring_fixed"
    trees = {}
    for name, extra in (("host", ["--ingest", "host"]), ("device", ["--ingest", "device"]), ("two ranks", ["--ingest", "host", "--gpus", "2"])):
        if os.path.isdir(results):
            shutil.rmtree(results)
        _run([path, "-r", "-f", "--periodic"] + extra)
        trees[name] = _tree(results)
        log = open(results / "log.ring").read()
        assert "a ring of 24 longitudes" in log and "lec_rowstats_ring" in log, name
    assert len(trees["host"]) == 22 and "ring_fixed_results.csv" in trees["host"]
    for name in ("device", "two ranks"):
        assert sorted(trees[name]) == sorted(trees["host"]), name
        for k in trees["host"]:
            assert trees[name][k] == trees["host"][k], f"{name}: {k} differs from the host-ingest run"
    # the numbers: the restatement on the crop the run makes (latitudes -30 .. 30)
    crop = o.crop_domain(dom, -180, 180, -30, 30)
    ref_s, ref_l = rr.ring_terms(crop, -30, 30)
    df = pd.read_csv(results / "ring_fixed_results.csv", index_col=0)
    worst = {n: scale_err(df[n].values, ref_s[n]) for n in ("Az", "Ae", "Kz", "Ke", "Cz", "Ca", "Ck", "Ce", "BAz", "BAe", "BKz", "BKe", "Gz", "Ge")}
    for n in o.LEVEL_TERMS:
        if n in ("Cz_1", "Ce_1"):
            continue                # (level-only, written transposed)
        t = pd.read_csv(results / "results_vertical_levels" / f"{n}_level.csv", index_col=0).values
        worst["lv:" + n] = scale_err(t, ref_l[n])
    print(f"cli --periodic: worst {max(worst.values()):.2e} of scale")
    assert max(worst.values()) <= TOL, {k: v for k, v in worst.items() if v > TOL}
    # the plain run: a limited area with a seam -- other numbers, and one line that names --periodic
    shutil.rmtree(results)
    _run([path, "-r", "-f", "--ingest", "host"])
    plain = pd.read_csv(results / "ring_fixed_results.csv", index_col=0)
    assert scale_err(plain["Ae"].values, df["Ae"].values) > 1e-3 and scale_err(plain["BKe"].values, df["BKe"].values) > 1e-3
    log = open(results / "log.ring").read()
    assert "--periodic closes the circle" in log and "lec_rowstats_ring" not in log
