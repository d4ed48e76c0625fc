"""SHA-256 of every output tensor of the level x latitude half of stage 2 and of what reads its record -- ``lec_reduce`` / ``lec_dropmask``,
``lec_level_spec_ring`` / ``lec_level_spec_b_ring``, ``lec_sections`` -- over the shapes at which their kernels take different paths.  Two
builds of the library give the same numbers exactly when the digests are equal: run it once per library (``LEC_LIB`` selects the library)
and compare the files.

    LEC_LIB=/path/to/liblec_hip.so python tools/probes/level_digests.py --out FILE

Every output and workspace is zero-filled before its call, so what a path does not write (``am`` of a box of at most 64 rows, the mask of
a moving series, the rows of a record buffer below a lower box) compares equal.

``lec_reduce`` (am, levraw, dropmask, the packed scalars + level tables, nanflag; then the two halves -- LEC_STAGE_LEVELS, LEC_STAGE_VERTICAL --
and the ``lec_dropmask`` path, on the same records): one fixed box of 2, 5, 63, 64, 65, 66, 128, 129 and 130 rows on a grid of 8 columns, 3
steps, 4 levels (the small kernel's first rows and last lane, the general kernel's one trip + 1, + 2, two exact trips, + 1, + 2); every
fixed case of tests/stage2_cases.py (tall boxes clean and with NaNs, 64 ... 160 levels, the many-NaN case, the uneven axes) and its two
moving cases of mixed heights (one box per step, lower than the record buffer).

``lec_level_spec_ring`` and ``lec_level_spec_b_ring`` (am, levraw of every n): the (ny, nx, N) of tests/test_gpu_level_spec.py at 5 and 70 rows,
each with and without ``qspec``, into a dense tensor and into a time slice of a longer one (``wave_stride``); that module's interior and
bottom NaN patterns (BAz's repair reads ``spec`` at another level); and a band INSIDE the record buffer (box rows 1 .. ny - 2 of ny: the
full band's records under the inner band's tables -- the kernels only compute with them), at 5 and 70 rows.

``lec_sections`` (sec, col, secsum, specsec, speccolsum): the CASES of tests/test_gpu_sections.py, the rings with the shares of 4 wavenumbers.
Prints one JSON object {case: {tensor: sha256}}."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from lorenzcycletoolkit_amd import _lib  # noqa: E402
from lorenzcycletoolkit_amd.engine import LECEngine  # noqa: E402
from tests import stage2_cases as sc  # noqa: E402
from tests import test_gpu_level_spec as tls  # noqa: E402
from tests import test_gpu_sections as tgs  # noqa: E402
from tests.helpers import synthetic_domain  # noqa: E402

DEV = "cuda:0"
HEIGHTS = (2, 5, 63, 64, 65, 66, 128, 129, 130)
SPEC_SHAPES = [(ny, nx, n) for ny, nx, n in [(5, 8, 4), (5, 7, 3), (5, 130, 20), (5, 130, 1), (70, 8, 4), (70, 7, 3), (70, 130, 20), (70, 130, 1)]]
F64 = dict(dtype=torch.float64, device=DEV)


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def fields(dom):
    return [dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]


def zeroed_workspace(eng, t_count, nl):
    """The engine's stage-2 scratch of this shape (am, levraw, dropmask), zero-filled: the calls below write into it."""
    work = eng._workspace(t_count, nl, torch.device(DEV))
    for w in work:
        w.zero_()
    return work


def reduce_calls(dom, boxes):
    """{tensor: sha256} of stage 2 on the row records of ``boxes`` (one, or one per step): whole, in its two halves, and with the mask formed
    by ``lec_dropmask``."""
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    rows = eng.rowstats(*fields(dom), boxes, time_s=dom.time_s)
    t_count, nl = int(rows.shape[0]), int(rows.shape[1])
    out = {"rows": sha(rows)}

    def packed():
        return torch.zeros((t_count, eng.packed_width(nl)), **F64), torch.zeros((t_count,), dtype=torch.int32, device=DEV)

    am, levraw, mask = zeroed_workspace(eng, t_count, nl)
    buf, flag = packed()
    eng.reduce(rows, boxes, out=buf, nanflag_out=flag)
    out.update(am=sha(am), levraw=sha(levraw), dropmask=sha(mask), packed=sha(buf), nanflag=sha(flag))

    am, _, _ = zeroed_workspace(eng, t_count, nl)
    lev = torch.zeros((t_count, nl, _lib.LEC_NLEVRAW), **F64)
    eng.level_stage(rows, boxes, lev)
    buf, flag = packed()
    eng.vertical_stage(lev, boxes, out=buf, nanflag_out=flag)
    out.update({"halves am": sha(am), "halves levraw": sha(lev), "halves packed": sha(buf), "halves nanflag": sha(flag)})

    am, levraw, mask = zeroed_workspace(eng, t_count, nl)
    buf, flag = packed()
    seen = []
    eng.reduce(rows, boxes, drop_any_time=True, merge_dropmask=lambda m: seen.append(sha(m)), out=buf, nanflag_out=flag)
    out.update({"lec_dropmask mask": seen[0], "lec_dropmask levraw": sha(levraw), "lec_dropmask packed": sha(buf), "lec_dropmask nanflag": sha(flag)})
    return out


def spec_calls(dom, n, band=None):
    """{tensor: sha256} of the two spectral level calls on a ring's records, with and without qspec, dense and sliced."""
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    ny, nx = dom.lat.size, dom.lon.size
    pb = eng.prepare_boxes([(0, nx - 1, 0, ny - 1)], ring=True)
    f = fields(dom)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    spec = eng.rowspec(*f[:4], pb, n)
    qspec = eng.rowspec_q(*f[:4], pb, n, time_s=dom.time_s)
    bspec = eng.rowspec_b(*f[:4], rows, pb, n)
    if band is not None:        # the same records under the tables of a lower band of the same buffer
        pb = eng.prepare_boxes([(0, nx - 1, band[0], band[1])], nyb_min=ny, ring=True)
    t_count, nl = int(rows.shape[0]), int(rows.shape[1])
    out = {}
    for call, b in (("spec", None), ("spec_b", bspec)):
        for qname, q in (("", None), (" q", qspec)):
            am = zeroed_workspace(eng, t_count, nl)[0]
            dense = torch.zeros((n, t_count, nl, _lib.LEC_NLEVRAW), **F64)
            eng.spectrum_level_stage(rows, spec, q, pb, dense, bspec=b)
            out[f"{call}{qname} am"] = sha(am)
            out[f"{call}{qname} levraw"] = sha(dense)
            longer = torch.zeros((n, t_count + 3, nl, _lib.LEC_NLEVRAW), **F64)
            eng.spectrum_level_stage(rows, spec, q, pb, longer[:, 1:1 + t_count], bspec=b)
            out[f"{call}{qname} levraw sliced"] = sha(longer)
    return out


def section_calls(kind, ny, nl, dtype, n=4):
    """{tensor: sha256} of ``lec_sections`` on a case of tests/test_gpu_sections.py; a ring also with the shares of ``n`` wavenumbers."""
    dom = tgs._dom(ny, nl, dtype)
    eng, pb = tgs._engine(kind, dom)
    f = fields(dom)
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    t_count = int(rows.shape[0])
    levraw = torch.zeros((t_count, nl, _lib.LEC_NLEVRAW), **F64)
    eng.level_stage(rows, pb, levraw)
    ring = kind == "ring"
    state = eng.section_begin(t_count, ny, torch.device(DEV), n_wave=n if ring else 0, generation=ring, keep_steps=True)
    state["col"].zero_()
    state["steps"].zero_()
    spec = qspec = None
    if ring:
        state["specwork"] = torch.zeros((t_count, nl, n, state["nf"], ny), **F64)
        spec = eng.rowspec(*f[:4], pb, n)
        qspec = eng.rowspec_q(*f[:4], pb, n, time_s=dom.time_s)
    eng.section_stage(rows, pb, levraw, state, 0, spec=spec, qspec=qspec)
    out = {"sec": sha(state["steps"]), "col": sha(state["col"]), "secsum": sha(state["secsum"])}
    if ring:
        out.update(specsec=sha(state["specwork"]), speccolsum=sha(state["speccolsum"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cases = {}
    for h in HEIGHTS:
        dom = synthetic_domain(3, 4, h + 3, 8, seed=h, lat0=-70.0, lat1=-5.0)
        cases[f"reduce box of {h} rows"] = reduce_calls(dom, [(1, 6, 2, h + 1)])
    for cid in sc.FIXED_IDS + sc.MOVING_IDS:
        dom, limits, _ = sc.build(cid)
        eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
        boxes = [eng.box_from_limits(*lim) for lim in limits] if cid in sc.MOVING_IDS else [eng.box_from_limits(*limits)]
        cases[f"reduce {cid}"] = reduce_calls(dom, boxes)
    for ny, nx, n in SPEC_SHAPES:
        cases[f"level_spec {ny} rows nx={nx} N={n}"] = spec_calls(tls._dom(ny, nx), n)
    for ny in (5, 70):
        for where in ("interior", "bottom"):
            cases[f"level_spec {ny} rows NaN {where}"] = spec_calls(tls._with_nan(tls._dom(ny, 16), where), 8)
        cases[f"level_spec band rows 1..{ny - 2} of {ny}"] = spec_calls(tls._dom(ny, 16), 8, band=(1, ny - 2))
    for (kind, ny, nl, dtype), cid in zip(tgs.CASES, tgs.IDS):
        cases[f"sections {cid}"] = section_calls(kind, ny, nl, dtype)
    out = {"library": os.path.basename(_lib.LIB_PATH), "sha256": cases}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
