"""Batches of tracks over one data set (lorenzcycletoolkit_amd/batch.py, ``-t --trackfiles``) without a GPU: the plan -- union of
times, each track's own crop, boxes, slice table and d/dt coefficients --, every refusal naming its track file, the host check of a
step table, the command line's refusals, and the C ABI of lec_rowstats_steps."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from lorenzcycletoolkit_amd import _lib, batch, tables
from lorenzcycletoolkit_amd import dataset as ds

LAT = np.arange(0.0, -62.6, -2.5)                      # file order N -> S, as the NCEP files
LON = np.arange(-100.0, 0.1, 2.5)
LEV = np.array([600, 700, 850, 925, 1000])             # hPa
TIME = np.datetime64("2005-08-08T00:00", "ns") + np.arange(16) * np.timedelta64(3, "h")      # 3-hourly
NAMES = {"Vertical Level": "lev"}


def _write(path, rows, width=None):
    """A track file: rows of (time string, lat, lon[, width, length])."""
    head = "time;Lat;Lon" + (";width;length" if width else "")
    lines = [head] + [";".join(str(x) for x in r) for r in rows]
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def _stamp(k):
    return pd.Timestamp(TIME[k]).strftime("%Y-%m-%d-%H%M")


@pytest.fixture
def tracks(tmp_path):
    a = _write(tmp_path / "a.csv", [(_stamp(k), -30.0 + 0.5 * k, -50.0 + k) for k in range(0, 12, 2)])          # 6-hourly
    b = _write(tmp_path / "b.csv", [(_stamp(k), -20.0, -60.0 - 0.5 * k, 10, 12) for k in range(3, 9)], width=True)  # 3-hourly, 10 x 12
    return a, b


def _plan(paths):
    return batch.plan_batch(LAT, LON, LEV, TIME, "hPa", NAMES, paths)


def test_union_windows_boxes_and_slice_tables(tracks):
    plan = _plan(list(tracks))
    px = ds.process_index(LAT, LON, LEV, TIME, "hPa", NAMES, SimpleNamespace(track=False))
    want = sorted(set(range(0, 12, 2)) | set(range(3, 9)))
    assert plan.tpos.tolist() == want
    assert [str(t) for t in plan.time] == [str(TIME[k]) for k in want]
    for tr, path in zip(plan.tracks, tracks):
        # the track's own crop is what a single run of it crops
        js, is_ = ds.domain_slices(px.lat, px.lon, SimpleNamespace(track=True, trackfile=path))
        assert (tr.js, tr.is_) == (js, is_)
        assert plan.js.start <= js.start and js.stop <= plan.js.stop and plan.is_.start <= is_.start and is_.stop <= plan.is_.stop
        assert (tr.joff, tr.ioff) == (js.start - plan.js.start, is_.start - plan.is_.start)
        wlat, wlon = tr.window(plan.lat, plan.lon)
        assert np.array_equal(wlat, px.lat[js]) and np.array_equal(wlon, px.lon[is_])
        # boxes: the single run's grid points, shifted into the union crop
        for b, l in zip(tr.boxes, tr.limits):
            iw, ie, jsb, jn = tables.box_indices(px.lat[js], px.lon[is_], l["min_lon"], l["max_lon"], l["min_lat"], l["max_lat"])
            assert b == (iw + tr.ioff, ie + tr.ioff, jsb + tr.joff, jn + tr.joff)
        # slice table in union steps; ends name the step itself; d/dt coefficients of the track's own times, exactly
        tt = ds.select_track_times(px.time, ds.read_track(path))
        u = np.searchsorted(plan.tpos, tt)
        assert tr.steps.dtype == np.int32 and tr.steps[:, 0].tolist() == u.tolist()
        assert tr.steps[0, 1] == tr.steps[0, 0] and tr.steps[-1, 2] == tr.steps[-1, 0]
        assert tr.steps[1:, 1].tolist() == u[:-1].tolist() and tr.steps[:-1, 2].tolist() == u[1:].tolist()
        own = (px.time[tt] - px.time[tt].min()) / np.timedelta64(1, "s")
        assert np.array_equal(tr.tcoef, tables.time_coefs(own))
    # the 6-hourly track over the 3-hourly union: its neighbours are two union steps away where the other track fills the gap
    a = plan.tracks[0]
    assert any(a.steps[i, 2] - a.steps[i, 0] == 2 for i in range(a.n - 1))
    assert not all(a.steps[i, 2] - a.steps[i, 0] == 1 for i in range(a.n - 1))
    # groups: by the single run's record extents (default 15 x 15 boxes vs 10 x 12)
    assert len(plan.groups) == 2 and sorted(sum(plan.groups.values(), [])) == [0, 1]


def test_one_track_plans_like_its_single_run(tracks):
    plan = _plan([tracks[0]])
    tr = plan.tracks[0]
    assert (tr.joff, tr.ioff) == (0, 0) and (plan.js, plan.is_) == (tr.js, tr.is_)
    assert tr.steps[:, 0].tolist() == list(range(tr.n))


@pytest.mark.parametrize("case", ["hourly", "late", "between", "lat", "one_step", "no_time_col"])
def test_refusals_name_the_track_file(tmp_path, tracks, case):
    rows = {
        "hourly": [(_stamp(0), -30, -50), (pd.Timestamp(TIME[0] + np.timedelta64(1, "h")).strftime("%Y-%m-%d-%H%M"), -30, -50)],
        "late": [(_stamp(14), -30, -50), ("2005-08-10-0000", -30, -50)],
        "between": [(_stamp(0), -30, -50), ("2005-08-08-0430", -30, -50)],
        "lat": [(_stamp(0), -63.0, -50), (_stamp(1), -63.0, -50)],
        "one_step": [(_stamp(0), -30, -50)],
    }
    bad = tmp_path / f"bad_{case}.csv"
    if case == "no_time_col":
        bad.write_text("when;Lat;Lon\n2005-08-08-0000;-30;-50\n")
    else:
        _write(bad, rows[case])
    with pytest.raises(ValueError) as e:
        _plan([tracks[0], str(bad)])
    assert str(bad) in str(e.value)


def test_missing_850_hpa_is_refused_by_name(tracks):
    with pytest.raises(ValueError) as e:
        batch.plan_batch(LAT, LON, np.array([500, 700, 1000]), TIME, "hPa", NAMES, [tracks[1]])
    assert tracks[1] in str(e.value)


def test_trackfile_expansion_and_duplicate_stems(tmp_path, tracks):
    d = tmp_path / "dir"
    d.mkdir()
    for n in ("z_track", "a_track"):
        (d / n).write_text("time;Lat;Lon\n")
    (d / "sub").mkdir()
    assert batch.expand_trackfiles([str(d)]) == [str(d / "a_track"), str(d / "z_track")]
    other = tmp_path / "other"
    other.mkdir()
    (other / "a.csv").write_text("time;Lat;Lon\n")
    with pytest.raises(ValueError) as e:
        batch.expand_trackfiles([tracks[0], str(other / "a.csv")])
    assert tracks[0] in str(e.value) and str(other / "a.csv") in str(e.value)


def test_engine_refuses_a_malformed_step_table_before_launching():
    torch = pytest.importorskip("torch")
    from lorenzcycletoolkit_amd.engine import LECEngine
    eng = object.__new__(LECEngine)          # check_steps is host work only
    good = torch.tensor([[0, 0, 1], [1, 0, 2], [2, 1, 2]], dtype=torch.int32)
    tc = torch.zeros((3, 3), dtype=torch.float64)
    assert eng.check_steps(good, tc, 3, "cpu") == 3
    bad = [
        (good.to(torch.int64), tc), (good[:, :2].contiguous(), tc), (good.t().contiguous().t(), tc),
        (torch.tensor([[0, 0, 1], [3, 2, 3]], dtype=torch.int32), tc[:2].contiguous()),       # a step outside [0, nt)
        (torch.tensor([[0, -1, 1]], dtype=torch.int32), tc[:1].contiguous()),                 # a negative neighbour
        (good, tc[:2].contiguous()), (good, tc.to(torch.float32)), (good, None),
    ]
    for steps, tcoef in bad:
        with pytest.raises(ValueError):
            eng.check_steps(steps, tcoef, 3, "cpu")


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--ingest", "device"], ["--device-ingest"]])
def test_cli_refuses_what_a_batch_does_not_do(tmp_path, monkeypatch, tracks, extra):
    import lorenzcycletoolkit
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        lorenzcycletoolkit.main(["nofile.nc", "-r", "-t", "--trackfiles", *tracks, *extra])
    assert "--trackfiles" in str(e.value)
    assert not os.path.exists(tmp_path / "LEC_Results")          # refused before anything was created


def test_rowstats_args_size_is_unchanged_and_steps_entry_validates():
    assert ctypes.sizeof(_lib.RowstatsArgs) == 6 * 8 + 14 * 4 + 9 * 8 + 8 * 4 + 2 * 8
    lib = _lib.load()
    assert lib.lec_version() == _lib.LEC_ABI_VERSION == 11 and "lec_rowstats_steps" in _lib.EXPORTS
    a = _lib.RowstatsArgs()
    assert lib.lec_rowstats_steps(ctypes.byref(a), None) == 1 and b"step_d" in lib.lec_last_error()
    fake = ctypes.c_void_p(0x1000)                  # never dereferenced: the calls are refused on their scalars
    assert lib.lec_rowstats_steps(ctypes.byref(a), fake) == 1          # box_per_step = 0
    a.box_per_step, a.n_box, a.t_count, a.with_q, a.tcoef_d = 1, 4, 4, 1, fake
    a.dTdt_d = fake
    assert lib.lec_rowstats_steps(ctypes.byref(a), fake) == 1 and b"NULL" in lib.lec_last_error()
    a.dTdt_d = None
    a.tuning.kernel = _lib.KERNEL_BOX_PLANE
    assert lib.lec_rowstats_steps(ctypes.byref(a), fake) == 2
    a.tuning.kernel = _lib.KERNEL_ROW_SWEEP
    assert lib.lec_rowstats_steps(ctypes.byref(a), fake) == 2
    a.tuning.kernel = _lib.KERNEL_AUTO
    a.t_begin = 1
    assert lib.lec_rowstats_steps(ctypes.byref(a), fake) == 1


def test_partly_stretched_grid_keeps_each_tracks_own_formulation(tmp_path):
    """A track whose own crop is evenly spaced keeps the uniform-longitude formulation of its single run, although the union crop
    is stretched: its box tables in the union equal those of its own crop, flag included."""
    lon = np.r_[np.arange(-100.0, -44.9, 2.5), -45.0 + np.cumsum(2.5 + 0.1 * np.arange(1, 18))]
    west = _write(tmp_path / "west.csv", [(_stamp(k), -30.0, -85.0 + 0.5 * k) for k in range(0, 8, 2)])
    east = _write(tmp_path / "east.csv", [(_stamp(k), -30.0, -20.0) for k in range(0, 4)])
    plan = batch.plan_batch(LAT, lon, LEV, TIME, "hPa", NAMES, [west, east])
    w, e = plan.tracks
    assert not tables.is_uniform(plan.lon)
    assert w.lon_uniform and not e.lon_uniform
    assert w.group_key != e.group_key and len(plan.groups) == 2
    for tr in plan.tracks:
        wlat, wlon = tr.window(plan.lat, plan.lon)
        own = [(b[0] - tr.ioff, b[1] - tr.ioff, b[2] - tr.joff, b[3] - tr.joff) for b in tr.boxes]
        single = tables.build_box_tables(wlat, wlon, own)
        union = tables.build_box_tables(plan.lat, plan.lon, tr.boxes, lon_uniform=tr.lon_uniform)
        assert single.lon_uniform == union.lon_uniform == tr.lon_uniform
        for f in ("boxtab", "wlon", "glon", "lattab", "boxtab2", "lattab2"):
            assert np.array_equal(getattr(single, f), getattr(union, f)), (tr.stem, f)
    with pytest.raises(ValueError):                       # the uniform formulation on stretched boxes is refused
        tables.build_box_tables(plan.lat, plan.lon, e.boxes, lon_uniform=True)


def test_device_estimate_counts_cubes_records_and_results(tracks):
    plan = _plan(list(tracks))
    m = batch.device_bytes(plan, 5, 4)
    nl = 5
    assert m["cubes"] == 5 * 4 * len(plan.tpos) * nl * len(plan.lat) * len(plan.lon)
    biggest = max(8 * sum(plan.tracks[k].n for k in mem) * nl * (key[0] * 32 + 48) for key, mem in plan.groups.items())
    assert m["records"] == biggest and m["results"] > 0 and m["total"] == m["cubes"] + m["records"] + m["results"]
