"""Return code and ``lec_last_error()`` of the six calls on csrc/lec_mapcol.h -- ``lec_maps``, ``lec_composite``, ``lec_composite_steps``,
``lec_composite_ensemble``, ``lec_lonsections``, ``lec_composite_lonsections`` -- for the valid argument set, for every argument broken
singly (null, misaligned, each range check, each ``box_h`` / ``step_h`` / ``seg_h`` / ``count_h`` fault, each launch limit) and for every
PAIR of breaks, which pins the order of the refusals.  One JSON line per case.  For a change to the calls' host side that must keep
every refusal's code, message and place: run it once per library (``LEC_LIB=/path/to/other/liblec_hip.so`` selects a build of the same
ABI) and compare the files.

Needs no GPU and uses none: every refusal comes before any HIP call, the device pointers are made-up aligned addresses that nothing
dereferences, and the process hides the devices from the HIP runtime before the library loads, so the valid set ends in the launch's own
error wherever it runs.

    python tools/probes/mapcol_refusals.py --out FILE
    python tools/probes/mapcol_refusals.py --compare FILE_A FILE_B"""
import argparse
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

os.environ["HIP_VISIBLE_DEVICES"] = os.environ["ROCR_VISIBLE_DEVICES"] = "-1"      # before the runtime loads: see above

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from lorenzcycletoolkit_amd import _lib  # noqa: E402

PTR = 0x10000
HOST = {"box_h": 4, "step_h": 3, "seg_h": 1, "count_h": 1}      # host tables: int32 per row
BIG = 1 << 20


def put(**kw):
    return lambda s: s.update(kw)


def row(table, i, values):
    """Row ``i`` of a host table replaced."""
    def f(s):
        t = np.array(s[table], dtype=np.int32).reshape(-1, HOST[table])
        if i < len(t):
            t[i] = values
        s[table] = t
    return f


def rows_needed(s, table):
    if table == "box_h":
        return s.get("t_count", s.get("s_count", 0))
    return {"step_h": s.get("s_count", 0), "seg_h": s.get("n_seg", 0) + 1, "count_h": s.get("n_track", 0)}[table]


def build(struct, s, keep):
    """The args struct of the state ``s``.  A host table is padded with copies of its last row to the rows the call may read, so that
    every combination of breaks stays inside the probe's own memory."""
    a = struct()
    for name, _ in struct._fields_:
        if name in HOST:
            if s[name] is None:
                continue
            t = np.array(s[name], dtype=np.int32).reshape(-1, HOST[name])
            need = min(max(rows_needed(s, name), 1), 1 << 21)
            if len(t) < need:
                t = np.concatenate([t, np.repeat(t[-1:], need - len(t), axis=0)])
            buf = np.zeros(t.nbytes + 32, dtype=np.uint8)
            off = (-buf.ctypes.data) % 16 + s.get(name + "_off", 0)
            buf[off: off + t.nbytes] = t.view(np.uint8).reshape(-1)
            keep.append(buf)
            setattr(a, name, buf.ctypes.data + off)
        elif name != "stream":
            setattr(a, name, s[name])
    return a


def pointer_breaks(struct):
    out = []
    for name, typ in struct._fields_:
        if typ is not C.c_void_p or name == "stream":
            continue
        out.append((f"{name} null", put(**{name: None})))
        for off in (8, 4, 2):
            out.append((f"{name} + {off}", put(**{name + "_off": off}) if name in HOST else put(**{name: PTR + off})))
    return out


# -- the six calls: (struct, the valid state, the breaks of its scalars, tables and limits) ---------------------------------------------
def pointers(struct, but=()):
    return {n: PTR for n, t in struct._fields_ if t is C.c_void_p and n not in HOST and n != "stream" and n not in but}


CUBE = dict(dtype=_lib.LEC_F64, nt=5, nl=4, ny=9, nx=16)
COMMON = [("dtype i16", put(dtype=_lib.LEC_I16)), ("dtype f32 (valid)", put(dtype=_lib.LEC_F32)), ("reserved0", put(reserved0=1)),
          ("nl 1", put(nl=1)), ("nl 161", put(nl=161))]
STEPS = [("t_begin -1", put(t_begin=-1)), ("t_begin nt", put(t_begin=5)), ("t_count 0", put(t_count=0)), ("t_count 5", put(t_count=5))]


def fixed(struct, lonsec):
    s = dict(CUBE, t_begin=1, t_count=3, iw=2, ie=13, js=1, jn=7, ring=0, reserved0=0, inv_hdeg=1.0, **pointers(struct))
    br = COMMON + STEPS + [
        ("ring 2", put(ring=2)), ("ring of a part", put(ring=1)), ("ring (valid)", put(ring=1, iw=0, ie=15)), ("nt 1", put(nt=1, t_begin=0, t_count=1)),
        ("ny 1", put(ny=1)), ("nx 2", put(nx=2)), ("iw -1", put(iw=-1)), ("iw nx", put(iw=16)), ("ie nx", put(ie=16)), ("ie < iw", put(ie=1)),
        ("two columns", put(ie=3)), ("js -1", put(js=-1)), ("js ny", put(js=9)), ("one row", put(jn=1)), ("jn ny", put(jn=9))]
    if lonsec:
        br += [("limit t_count * nl * segments", put(nt=BIG, t_count=BIG, t_begin=0, nl=64)),
               ("limit 6 * nl * columns", put(nl=160, nx=1 << 23, iw=0, ie=(1 << 23) - 1))]
    else:
        br += [("limit t_count * nl", put(nt=BIG, t_count=BIG, t_begin=0, nl=64)),
               ("limit t_count * rows * segments", put(nt=BIG, t_count=BIG, t_begin=0, ny=65, js=0, jn=63)),
               ("limit 6 * rows * columns", put(ny=1 << 15, nx=1 << 15, js=0, jn=(1 << 15) - 1, iw=0, ie=(1 << 15) - 1)),
               ("limit t_count * 6 * columns", put(nt=BIG, t_count=BIG, t_begin=0, nx=1024, iw=0, ie=1023, js=1, jn=2))]
    return struct, s, br


BOXES = [(1, 6, 2, 5), (2, 7, 3, 6), (10, 15, 5, 8)]
BOX_FAULTS = [("box 1 narrow", row("box_h", 1, (2, 6, 3, 6))), ("box 1 low", row("box_h", 1, (2, 7, 3, 5))),
              ("box 0 wide and tall", row("box_h", 0, (1, 7, 2, 6))), ("box 2 east", row("box_h", 2, (11, 16, 5, 8))),
              ("box 0 west", row("box_h", 0, (-1, 4, 2, 5))), ("box 0 south", row("box_h", 0, (1, 6, -1, 2))),
              ("box 2 north", row("box_h", 2, (10, 15, 6, 9)))]
SHAPE = [("nyb 1", put(nyb=1)), ("nxb 2", put(nxb=2)), ("ny < nyb", put(ny=3)), ("nx < nxb", put(nx=5))]


def moving(struct, lonsec):
    s = dict(CUBE, t_begin=1, t_count=3, nyb=4, nxb=6, reserved0=0, box_h=BOXES, **pointers(struct, but=("dTdt_d", "tm_d", "tp_d")),
             dTdt_d=None, tm_d=None, tp_d=None)
    br = COMMON + STEPS + SHAPE + BOX_FAULTS + [
        ("tm_d alone", put(tm_d=PTR)), ("tp_d alone", put(tp_d=PTR)), ("tm_d tp_d (valid)", put(tm_d=PTR, tp_d=PTR)),
        ("dTdt_d (valid)", put(dTdt_d=PTR)), ("dTdt_d and tm_d tp_d", put(dTdt_d=PTR, tm_d=PTR, tp_d=PTR)), ("nt 0", put(nt=0)),
        ("nt 1", put(nt=1, t_begin=0, t_count=1))]
    big = dict(nt=BIG, t_count=BIG, t_begin=0)
    if lonsec:
        br += [("limit t_count * nl * segments", put(nl=64, **big)),
               ("limit 6 * nl * columns", put(nl=160, nx=1 << 23, nxb=1 << 23, box_h=[(0, (1 << 23) - 1, 2, 5)]))]
    else:
        br += [("limit t_count * nl", put(nl=64, **big)),
               ("limit t_count * rows * segments", put(ny=64, nyb=64, box_h=[(1, 6, 0, 63)], **big)),
               ("limit 6 * rows * columns", put(ny=1 << 15, nx=1 << 15, nyb=1 << 15, nxb=1 << 15, box_h=[(0, (1 << 15) - 1, 0, (1 << 15) - 1)])),
               ("limit t_count * 6 * columns", put(nx=1024, nxb=1024, nyb=2, box_h=[(0, 1023, 2, 3)], **big))]
    return struct, s, br


def steps():
    struct = _lib.CompositeStepsArgs
    s = dict(CUBE, s_count=3, nyb=4, nxb=6, n_seg=2, reserved0=0, box_h=BOXES, step_h=[(0, 0, 1), (1, 0, 2), (4, 3, 4)], seg_h=[0, 2, 3],
             **pointers(struct))
    br = COMMON + SHAPE + BOX_FAULTS + [
        ("nt 0", put(nt=0)), ("s_count 0", put(s_count=0)), ("n_seg 0", put(n_seg=0)),
        ("step 1 t -1", row("step_h", 1, (-1, 0, 2))), ("step 1 t_prev nt", row("step_h", 1, (1, 5, 2))), ("step 2 t_next nt", row("step_h", 2, (4, 3, 5))),
        ("seg_h[0] 1", row("seg_h", 0, 1)), ("seg_h descends", row("seg_h", 1, 4)), ("segment 0 empty", row("seg_h", 1, 0)),
        ("segment 1 empty", row("seg_h", 2, 2)), ("seg_h[n_seg] 4", row("seg_h", 2, 4)), ("one segment (valid)", put(n_seg=1, seg_h=[0, 3])),
        ("limit s_count * nl", put(s_count=BIG, nl=64, n_seg=1, seg_h=[0, BIG])),
        ("limit s_count * rows * segments", put(s_count=BIG, ny=64, nyb=64, box_h=[(1, 6, 0, 63)], n_seg=1, seg_h=[0, BIG])),
        ("limit 6 * rows * columns", put(ny=1 << 15, nx=1 << 15, nyb=1 << 15, nxb=1 << 15, box_h=[(0, (1 << 15) - 1, 0, (1 << 15) - 1)])),
        ("limit s_count * 6 * columns", put(s_count=BIG, nx=1024, nxb=1024, nyb=2, box_h=[(0, 1023, 2, 3)], n_seg=1, seg_h=[0, BIG])),
        ("limit n_seg * 6 * rows * columns", put(s_count=1 << 16, n_seg=1 << 16, seg_h=np.arange((1 << 16) + 1), ny=128, nx=128, nyb=128, nxb=128,
                                                 box_h=[(0, 127, 0, 127)]))]
    return struct, s, br


def ensemble():
    struct = _lib.CompositeEnsembleArgs
    s = dict(n_track=3, nyb=4, nxb=6, reserved0=0, count_h=[9, 5, 2], **pointers(struct))
    br = [("reserved0", put(reserved0=1)), ("n_track 0", put(n_track=0)), ("nyb 0", put(nyb=0)), ("nxb 0", put(nxb=0)),
          ("track 0 empty", row("count_h", 0, 0)), ("track 2 negative", row("count_h", 2, -1)), ("mean_d aliases mapsum_d (valid)", put()),
          ("limit 6 * rows * columns", put(nyb=1 << 15, nxb=1 << 15))]
    return struct, s, br


CALLS = {"lec_maps": lambda: fixed(_lib.MapsArgs, False), "lec_composite": lambda: moving(_lib.CompositeArgs, False),
         "lec_composite_steps": steps, "lec_composite_ensemble": ensemble, "lec_lonsections": lambda: fixed(_lib.LonSectionsArgs, True),
         "lec_composite_lonsections": lambda: moving(_lib.CompositeLonSectionsArgs, True)}


def run(out):
    lib = _lib.load()
    lines = []
    for call, make in CALLS.items():
        struct, valid, breaks = make()
        breaks = breaks + pointer_breaks(struct)
        fn = getattr(lib, call)
        fn.restype = C.c_int
        rc = fn(None)
        lines.append({"call": call, "case": "null args", "code": rc, "error": lib.lec_last_error().decode("utf-8", "replace")})
        cases = [()] + [(b,) for b in breaks] + list(itertools.combinations(breaks, 2))
        for case in cases:
            s, keep = dict(valid), []
            for _, change in case:
                change(s)
            rc = fn(C.byref(build(struct, s, keep)))
            lines.append({"call": call, "case": " & ".join(n for n, _ in case) or "valid", "code": rc,
                          "error": lib.lec_last_error().decode("utf-8", "replace") if rc else ""})
    text = "".join(json.dumps(x) + "\n" for x in lines)
    with open(out, "w") as fh:
        fh.write(text)
    per = {call: sum(1 for x in lines if x["call"] == call) for call in CALLS}
    print(json.dumps({"library": os.environ.get("LEC_LIB") or "in-tree", "cases": len(lines), "per_call": per,
                      "refused": sum(1 for x in lines if x["code"] in (1, 2)), "distinct_messages": len({x["error"] for x in lines}),
                      "sha256": hashlib.sha256(text.encode()).hexdigest()}))


def compare(a, b):
    la, lb = open(a).read().splitlines(), open(b).read().splitlines()
    diff = [(x, y) for x, y in itertools.zip_longest(la, lb) if x != y]
    for x, y in diff[:20]:
        print("A:", x, "\nB:", y)
    print(json.dumps({"cases": len(la), "differences": len(diff)}))
    return 1 if diff else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    ns = ap.parse_args()
    if ns.compare:
        sys.exit(compare(*ns.compare))
    run(ns.out or os.devnull)
