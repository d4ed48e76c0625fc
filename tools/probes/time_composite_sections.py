"""Times ``lec_composite_sections`` on the geometry of ``bench.py --moving``: a box-packed series of 61 x 61 x 37 boxes, 512 steps, fp64
storage (dT/dt as a cube) and fp32 storage (tm / tp), next to stage 1 + stage 2 (``rowstats`` + ``reduce``) on the same series in the same
run.  The call reads row records only, so the storage dtype matters to the yardstick, not to the call.

Method.  HIP events on the launch stream around each call, which ends in ``event.synchronize()``; two warm-up passes of every shape, then
``--repeat`` timed passes of stage 1 + 2 and of the sections ALTERNATING; the figure is the median, the spread is min .. max.  The
fields are smooth waves plus noise made on the device from a seed (the time of these kernels does not depend on the values); the boxes
drift over a 0.25-degree grid a column or a row per step, as a track does, so every step has tables of its own.

    python tools/probes/time_composite_sections.py [--steps 512] [--repeat 7] [--out FILE]

Prints one JSON line per storage dtype (and appends them to ``--out``)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from lorenzcycletoolkit_amd import _lib  # noqa: E402
from lorenzcycletoolkit_amd.engine import LECEngine  # noqa: E402
from tools.probes.time_composite import NL, NXB, NYB, series, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_composite_sections.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    lat, lon = np.arange(-60.0, 0.25, 0.25), np.arange(-100.0, 20.25, 0.25)
    level = np.linspace(1000.0, 100000.0, NL)
    time_s = np.arange(a.steps) * 21600.0
    eng = LECEngine(lat, lon, level, device=dev)
    boxes = [((t // 2) % 300, (t // 2) % 300 + NXB - 1, (t // 3) % 150, (t // 3) % 150 + NYB - 1) for t in range(a.steps)]
    pb = eng.prepare_boxes(boxes, packed=True)
    tcoef = eng.time_coefs_device(time_s)
    stream = torch.cuda.current_stream(dev)
    # what the call moves, counted from the shapes: the records read once, the sections written and read twice by the fold (the scan of
    # the levels, the time sums)
    call_bytes = a.steps * NL * NYB * 8 * (_lib.LEC_NSTAT + 3 * _lib.LEC_NSECTION)
    for dtype in (torch.float64, torch.float32):
        f = series(a.steps, dtype, dev)
        kw = eng.packed_dtdt(f["tm"], f["tair"], f["tp"], tcoef)
        fields = (f["tair"], f["u"], f["v"], f["omega"])

        def totals():
            rows = eng.rowstats(*fields, f["geopt"], pb, per_step_boxes=True, **kw)
            res = eng.reduce(rows, pb, drop_any_time=False)
            return rows, res

        rows, _ = totals()
        levraw = eng._workspace(a.steps, NL, dev)[1].clone()

        def sections():
            st = eng.composite_section_begin(a.steps, pb, dev)
            eng.composite_section_stage(rows, pb, levraw, st, 0)
            return st

        for _ in range(2):
            totals()
            sections()
        torch.cuda.synchronize(dev)
        t12, ts = [], []
        for _ in range(a.repeat):
            t12.append(timed(totals, stream)[0])
            ts.append(timed(sections, stream)[0])
        med12, meds = statistics.median(t12), statistics.median(ts)
        line = {"probe": "time_composite_sections", "storage": str(dtype).replace("torch.", ""), "dTdt": "cube" if "dTdt" in kw else "tm/tp",
                "box": [NL, NYB, NXB], "steps": a.steps, "repeat": a.repeat, "source_digest": _lib.source_digest(),
                "stage1_plus_stage2_ms": {"median": med12, "min": min(t12), "max": max(t12), "per_step_us": 1e3 * med12 / a.steps},
                "composite_sections_ms": {"median": meds, "min": min(ts), "max": max(ts), "per_step_us": 1e3 * meds / a.steps},
                "composite_sections_over_stage1_plus_stage2": meds / med12,
                "composite_sections_bytes": call_bytes, "composite_sections_GBps": call_bytes / (meds * 1e-3) / 1e9}
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")
        del f, kw, rows, levraw


if __name__ == "__main__":
    main()
