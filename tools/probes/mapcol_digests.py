"""sha256 of what the calls on csrc/lec_mapcol.h return -- ``lec_maps`` and ``lec_composite`` (the column values, the time mean and the
Hovmoeller), ``lec_lonsections`` and ``lec_composite_lonsections`` (the sections and their time mean), ``lec_composite_steps`` with
``lec_composite_ensemble`` (the column values, the tracks' means, the Hovmoeller and the ensemble) -- at the shapes of their GPU tests
(tests/test_gpu_maps.py, test_gpu_composite.py, test_gpu_lonsections.py, test_gpu_composite_lonsections.py, test_gpu_batch_composite.py),
one JSON line per case.  For a change to csrc/lec_mapcol.h that must keep the calls' bits: run it once per library in one GPU session
(``LEC_LIB=/path/to/other/liblec_hip.so`` selects a build of the same ABI) and compare the lines, the ``library`` key aside.

    python tools/probes/mapcol_digests.py [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from lorenzcycletoolkit_amd import _lib  # noqa: E402
from lorenzcycletoolkit_amd.engine import LECEngine  # noqa: E402
from tests import test_gpu_batch_composite as tb  # noqa: E402
from tests import test_gpu_composite as tc  # noqa: E402
from tests import test_gpu_composite_lonsections as tcl  # noqa: E402
from tests import test_gpu_lonsections as tl  # noqa: E402
from tests import test_gpu_maps as tm  # noqa: E402


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for (kind, nx, cols, ny, nl, dtype), name in zip(tm.CASES, tm.IDS):
        dom = tm._dom(nx, ny, nl, dtype)
        eng, pb = tm._engine(cols, dom)
        res = eng.compute(*tm._fields(dom), pb, time_s=dom.time_s, maps=True, map_steps=True)
        lines.append({"call": "lec_maps", "case": name, "col": _sha(res.map_steps), "mapsum": _sha(res.map_mean), "hov": _sha(res.map_lon)})
    for (nxb, nyb, nl, layout, dtype), name in zip(tc.CASES, tc.IDS):
        res = tc._run(tc._dom(nxb, nyb, nl, dtype), tc._boxes(nxb, nyb), layout, composites=True, composite_steps=True)
        lines.append({"call": "lec_composite", "case": name, "col": _sha(res.composite_steps), "mapsum": _sha(res.composite_mean),
                      "hov": _sha(res.composite_lon)})
    for (kind, nx, cols, ny, nl, dtype), name in zip(tl.CASES, tl.IDS):
        dom = tl._dom(nx, ny, nl, dtype)
        eng, pb = tl._engine(cols, dom)
        res = eng.compute(*tl._fields(dom), pb, time_s=dom.time_s, lon_sections=True, lon_section_steps=True)
        lines.append({"call": "lec_lonsections", "case": name, "lonsec": _sha(res.lonsection_steps), "lonsecsum": _sha(res.lonsection_mean)})
    for (nxb, nyb, nl, layout, dtype), name in zip(tcl.CASES, tcl.IDS):
        res = tcl._run(tcl._dom(nxb, nyb, nl, dtype), tcl._boxes(nxb, nyb), layout, composite_lon_sections=True,
                       composite_lon_section_steps=True)
        lines.append({"call": "lec_composite_lonsections", "case": name, "lonsec": _sha(res.composite_lonsection_steps),
                      "lonsecsum": _sha(res.composite_lonsection_mean)})
    for (nyb, nxb, nl, dtype, ny, nx), name in zip(tb.CASES, tb.IDS):
        dom = tb._dom(nl, ny, nx, dtype)
        eng = LECEngine(dom.lat, dom.lon, dom.level, device=tb.DEV)
        cubes = [tb._dev(x) for x in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
        res = tb._batch(eng, cubes, dom, tb._tracks(nyb, nxb, ny, nx), batch_composite_steps=True)
        lines.append({"call": "lec_composite_steps", "case": name, "col": _sha(res.batch_composite_steps),
                      "mapsum": _sha(res.batch_composite_mean), "hov": _sha(res.batch_composite_lon),
                      "ensemble": _sha(res.batch_composite_ensemble)})
    for line in lines:
        line["library"] = os.environ.get("LEC_LIB") or "in-tree"
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
