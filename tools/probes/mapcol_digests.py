"""sha256 of what ``lec_maps`` and ``lec_composite`` return -- the column values, the time mean and the Hovmoeller -- at the shapes of
tests/test_gpu_maps.py and tests/test_gpu_composite.py, one JSON line per case.  For a change to csrc/lec_mapcol.h that must keep the
two calls' bits: run it once per library in one GPU session (``LEC_LIB=/path/to/other/liblec_hip.so`` selects a build of the same ABI)
and compare the lines.

    python tools/probes/mapcol_digests.py [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from lorenzcycletoolkit_amd import _lib  # noqa: E402
from tests import test_gpu_composite as tc  # noqa: E402
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
    for line in lines:
        line["library"] = os.environ.get("LEC_LIB") or "in-tree"
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
