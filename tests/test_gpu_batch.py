"""Many tracks over one data set in one pass (GPU): the records of ``lec_rowstats_steps`` against each track's own single-track
computation, bit for bit; the terms against the oracle; and the command line -- every file a ``--trackfiles`` run writes for a track
is byte for byte the file its own ``-t --trackfile`` run writes."""
import filecmp
import os
import shutil

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from lorenzcycletoolkit_amd import tables                      # noqa: E402
from lorenzcycletoolkit_amd.engine import LECEngine           # noqa: E402
from lorenzcycletoolkit_amd.synthetic import write_classic_nc  # noqa: E402
from oracle import lec_oracle as o                            # noqa: E402
from tests.helpers import SCALARS, scale_err, synthetic_domain  # noqa: E402

DEV = "cuda:0"


def _same(a, b):
    a, b = a[..., :28], b[..., :28]
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _drift(n, w, h, i0, j0, rng, nx, ny):
    out, i, j = [], i0, j0
    for _ in range(n):
        i = int(np.clip(i + rng.integers(-1, 3), 0, nx - w))
        j = int(np.clip(j + rng.integers(-1, 2), 0, ny - h))
        out.append((i, i + w - 1, j, j + h - 1))
    return out


def _batch_case(dtype, with_nan, seed=3):
    """A union cube of 12 (3-hourly) steps and three tracks: a 6-hourly one, a 3-hourly one whose boxes change size (width / length
    columns), and a 6-hourly one on the first track's steps (repeated source steps)."""
    rng = np.random.default_rng(seed)
    nt, nl, ny, nx = 12, 7, 44, 52
    dom = synthetic_domain(nt, nl, ny, nx, seed=seed, dtype=dtype, dt_s=10800.0)
    if with_nan:                              # below-ground points at the lowest levels (NaN, as a decoded fill value)
        for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt):
            a[:, -1, 5:14, 8:20] = np.nan
            a[3:6, -2, 30:33, 30:34] = np.nan
    tracks = [
        (np.arange(0, 12, 2), _drift(6, 15, 15, 4, 3, rng, nx, ny)),
        (np.arange(1, 9), [(b[0], b[0] + 9 + (k % 3), b[2], b[2] + 11 - (k % 2)) for k, b in enumerate(_drift(8, 12, 12, 20, 10, rng, nx, ny))]),
        (np.arange(2, 12, 2), _drift(5, 15, 15, 30, 20, rng, nx, ny)),
    ]
    return dom, tracks


def _single(eng, cubes, ustep, boxes, time_s):
    """The track alone, as the host-prepared moving framework computes it (frameworks.BoxData._compute_resident_packed)."""
    own = [c[torch.as_tensor(ustep, device=DEV)].contiguous() for c in cubes]
    nyb = max(b[3] - b[2] + 1 for b in boxes)
    tcoef = eng.time_coefs_device(time_s)
    pk = eng.pack_series(*own, boxes, tcoef)
    pb = eng.prepare_boxes(boxes, nyb_min=nyb, packed=True)
    kw = dict(dTdt=pk["dTdt"]) if "dTdt" in pk else dict(tm=pk["tm"], tp=pk["tp"], tcoef=tcoef)
    return eng.compute(pk["tair"], pk["u"], pk["v"], pk["omega"], pk["geopt"], pb, per_step_boxes=True, drop_any_time=False,
                       keep_rows=True, **kw)


@pytest.mark.parametrize("dtype,with_nan", [(np.float64, True), (np.float32, True), (np.float64, False)])
def test_step_table_records_equal_each_tracks_own_run(dtype, with_nan):
    dom, tracks = _batch_case(dtype, with_nan)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    cubes = [torch.as_tensor(a).to(DEV) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    groups = {}
    for k, (ustep, boxes) in enumerate(tracks):
        groups.setdefault((max(b[3] - b[2] + 1 for b in boxes), max(b[1] - b[0] + 1 for b in boxes)), []).append(k)
    assert len(groups) == 2
    for (nyb, _), members in groups.items():
        steps, tcoef, boxes = [], [], []
        for k in members:
            u, bx = tracks[k]
            n = len(u)
            steps.append(np.stack([u, u[np.maximum(np.arange(n) - 1, 0)], u[np.minimum(np.arange(n) + 1, n - 1)]], 1))
            tcoef.append(tables.time_coefs(dom.time_s[u] - dom.time_s[u[0]]))
            boxes += bx
        st = torch.as_tensor(np.concatenate(steps).astype(np.int32)).to(DEV)
        tc = torch.as_tensor(np.concatenate(tcoef)).to(DEV)
        got = eng.compute(*cubes, eng.prepare_boxes(boxes, nyb_min=nyb), steps=st, tcoef=tc, per_step_boxes=True, drop_any_time=False,
                          keep_rows=True)
        torch.cuda.synchronize()
        a = 0
        for k in members:
            u, bx = tracks[k]
            ref = _single(eng, cubes, u, bx, dom.time_s[u] - dom.time_s[u[0]])
            b = a + len(u)
            assert _same(got.rows[a:b], ref.rows), f"track {k}: records"
            assert torch.equal(torch.nan_to_num(got.packed[a:b], nan=7.0), torch.nan_to_num(ref.packed, nan=7.0)), f"track {k}: terms"
            if not with_nan:
                sub = o.Domain(*(np.ascontiguousarray(x[u].astype(np.float64)) for x in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)),
                               dom.lat, dom.lon, dom.level, dom.time_s[u] - dom.time_s[u[0]])
                limits = [(dom.lon[q[0]], dom.lon[q[1]], dom.lat[q[2]], dom.lat[q[3]]) for q in bx]
                sc, _ = o.lec_moving(sub, limits)
                mine = {n: got.scalars[a:b, i].cpu().numpy() for i, n in enumerate(SCALARS)}
                for n in SCALARS:
                    assert scale_err(mine[n], np.asarray(sc[n])) <= 1e-11, (k, n)
            a = b


def test_identity_table_gives_the_records_of_the_t_pm_1_kernel():
    dom, tracks = _batch_case(np.float64, True, seed=9)
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    cubes = [torch.as_tensor(a).to(DEV) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    nt = dom.tair.shape[0]
    rng = np.random.default_rng(1)
    boxes = _drift(nt, 15, 15, 5, 5, rng, dom.lon.size, dom.lat.size)
    u = np.arange(nt)
    st = torch.as_tensor(np.stack([u, np.maximum(u - 1, 0), np.minimum(u + 1, nt - 1)], 1).astype(np.int32)).to(DEV)
    tc = eng.time_coefs_device(dom.time_s)
    ref = eng.rowstats(*cubes, boxes, time_s=dom.time_s, per_step_boxes=True, tuning={"kernel": "box_tile"})
    got = eng.rowstats(*cubes, boxes, steps=st, tcoef=tc)
    torch.cuda.synchronize()
    assert _same(got, ref)


# ---------------------------------------------------------------------------------------------------------------------------- CLI
def _track_file(path, rows, sizes=None):
    head = "time;Lat;Lon" + (";width;length" if sizes else "")
    lines = [head]
    for k, (t, la, lo) in enumerate(rows):
        lines.append(f"{t};{la};{lo}" + (f";{sizes[k][0]};{sizes[k][1]}" if sizes else ""))
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def _main(argv):
    import lorenzcycletoolkit
    lorenzcycletoolkit.main(argv)


def _tree_files(d):
    out = []
    for root, dirs, files in os.walk(d):
        rel = os.path.relpath(root, d)
        out += [os.path.join(rel, x) + "/" for x in dirs]
        out += [os.path.join(rel, x) for x in files if not x.startswith("log.")]
    return sorted(out)


def _check_batch_equals_single_runs(workdir, infile, trackfiles, extra):
    stem = os.path.basename(infile).split(".nc")[0]
    res = workdir / "LEC_Results"
    singles = {}
    for tf in trackfiles:
        _main([infile, "-r", "-t", "--trackfile", tf, *extra])
        tstem = os.path.splitext(os.path.basename(tf))[0]
        dst = workdir / f"single_{tstem}"
        shutil.move(str(res / f"{stem}_track"), str(dst))
        singles[tstem] = dst
    _main([infile, "-r", "-t", "--trackfiles", *trackfiles, *extra])
    listing = pd.read_csv(res / f"{stem}_track_batch" / "batch.csv")
    assert list(listing["trackfile"]) == list(trackfiles)
    assert os.path.exists(res / f"{stem}_track_batch" / f"log.{stem}")
    for tstem, single in singles.items():
        tree = res / f"{stem}_{tstem}_track"
        files = _tree_files(single)
        assert files == _tree_files(tree), tstem
        assert f"./{stem}_track_results.csv" in files and f"./{stem}_track_trackfile" in files
        for f in files:
            if not f.endswith("/"):
                assert filecmp.cmp(single / f, tree / f, shallow=False), (tstem, f)


@pytest.fixture
def workdir(tmp_path, golden_dir, monkeypatch):
    os.makedirs(tmp_path / "inputs")
    monkeypatch.chdir(tmp_path)
    return tmp_path


@pytest.mark.parametrize("dtype,extra", [(np.float32, []), (np.float64, ["-z"])])
def test_cli_batch_matches_single_runs_synthetic(workdir, golden_dir, dtype, extra):
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_ERA5"), workdir / "inputs" / "namelist")
    infile = str(workdir / f"synth_{np.dtype(dtype).name}.nc")
    write_classic_nc(infile, dtype)
    t = lambda k: (pd.Timestamp("2020-01-01") + pd.Timedelta(hours=3 * k)).strftime("%Y-%m-%d-%H%M")
    tracks = [
        _track_file(workdir / "six_hourly.csv", [(t(k), -30.0 + 0.4 * k, -55.0 + 0.7 * k) for k in range(0, 12, 2)]),
        _track_file(workdir / "sized.csv", [(t(k), -25.0, -45.0 - 0.5 * k) for k in range(2, 9)],
                    sizes=[(8 + (k % 3), 10 + (k % 2)) for k in range(7)]),
        _track_file(workdir / "edge.csv", [(t(k), -52.4, -72.3 + 0.5 * k) for k in range(4, 11)]),     # its box meets the data's edge
    ]
    _check_batch_equals_single_runs(workdir, infile, tracks, extra)


def test_cli_batch_matches_single_runs_ncep(workdir, golden_dir):
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_NCEP-R2"), workdir / "inputs" / "namelist")
    infile = os.path.join(golden_dir, "testdata_NCEP-R2.nc")
    base = pd.read_csv(os.path.join(golden_dir, "inputs", "track_testdata_NCEP-R2"), sep=";")
    tracks = [str(shutil.copy(os.path.join(golden_dir, "inputs", "track_testdata_NCEP-R2"), workdir / "track_testdata"))]
    for name, dlat, dlon, rows in (("north_east", 5.0, 7.5, slice(None)), ("south", -7.5, 0.0, slice(1, 4))):
        tr = base.iloc[rows].copy()
        tr["Lat"] += dlat
        tr["Lon"] += dlon
        p = workdir / f"track_{name}"
        tr.to_csv(p, sep=";", index=False)
        tracks.append(str(p))
    _check_batch_equals_single_runs(workdir, infile, tracks, [])


def test_cli_batch_matches_single_runs_on_a_partly_stretched_grid(workdir, golden_dir):
    """Evenly spaced west of 45 W, stretched east of it: a track in the west has an evenly spaced crop of its own (its single run takes
    the uniform-longitude formulation) while the union crop is not; the batch must keep each track's own formulation."""
    from types import SimpleNamespace
    from lorenzcycletoolkit_amd import batch
    shutil.copy(os.path.join(golden_dir, "inputs", "namelist_ERA5"), workdir / "inputs" / "namelist")
    lon = np.r_[np.arange(-80.0, -44.5, 1.0), -45.0 + np.cumsum(1.0 + 0.04 * np.arange(1, 25))]
    infile = str(workdir / "stretched.nc")
    write_classic_nc(infile, np.float32, lon=lon)
    t = lambda k: (pd.Timestamp("2020-01-01") + pd.Timedelta(hours=3 * k)).strftime("%Y-%m-%d-%H%M")
    tracks = [
        _track_file(workdir / "west.csv", [(t(k), -30.0 - 0.3 * k, -70.0 + 0.3 * k) for k in range(0, 10, 2)]),
        _track_file(workdir / "east.csv", [(t(k), -35.0, -30.0 + 0.5 * k) for k in range(1, 8)]),
    ]
    _, plan = batch.prepare_union(SimpleNamespace(infile=infile, mpas=False), tracks, "inputs/namelist")
    assert plan.tracks[0].lon_uniform and not plan.tracks[1].lon_uniform and not tables.is_uniform(plan.lon)
    _check_batch_equals_single_runs(workdir, infile, tracks, [])


def test_step_table_cut_into_launches_gives_the_same_records():
    """More boxes than MAX_STEPS_PER_LAUNCH: the table, tcoef, boxes and records are cut into launches (same bits)."""
    dom, tracks = _batch_case(np.float64, True)
    whole = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    cut = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    cut.MAX_STEPS_PER_LAUNCH = 5
    cubes = [torch.as_tensor(a).to(DEV) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    boxes, steps, tcoef = [], [], []
    for k in (0, 2):                        # one group: 11 boxes -> launches of 5, 5, 1
        u, bx = tracks[k]
        n = len(u)
        steps.append(np.stack([u, u[np.maximum(np.arange(n) - 1, 0)], u[np.minimum(np.arange(n) + 1, n - 1)]], 1))
        tcoef.append(tables.time_coefs(dom.time_s[u] - dom.time_s[u[0]]))
        boxes += bx
    st = torch.as_tensor(np.concatenate(steps).astype(np.int32)).to(DEV)
    tc = torch.as_tensor(np.concatenate(tcoef)).to(DEV)
    calls = []
    ref = whole.compute(*cubes, boxes, steps=st, tcoef=tc, drop_any_time=False, keep_rows=True)
    got = cut.compute(*cubes, boxes, steps=st, tcoef=tc, drop_any_time=False, keep_rows=True, timing=calls)
    torch.cuda.synchronize()
    assert len(calls) == 3
    assert _same(got.rows, ref.rows)
    assert torch.equal(torch.nan_to_num(got.packed, nan=7.0), torch.nan_to_num(ref.packed, nan=7.0))
