"""SHA-256 of every output tensor of the four ring spectral passes -- ``lec_rowspec_ring``, ``lec_rowspec_q_ring``, ``lec_rowspec_nl_ring``
(two tensors), ``lec_rowspec_b_ring`` -- over the shapes at which their kernels take different paths.  Two builds of the library give
the same records exactly when the digests are equal: run it once per library (``LEC_LIB`` selects the library) and compare the files.

    LEC_LIB=/path/to/liblec_hip.so python tools/probes/rowspec_digests.py --out FILE

Cases, each for all four calls: every (nx, N, dtype) of the four GPU test modules' ``RECORD_CASES`` on their 3 x 4 x 5 domains; their
45-row case (an odd row count, N = 7 and 20); a band inside a taller cube (js > 0, jn < ny - 1); a band of two rows (both walls for
``lec_rowspec_b_ring``); and nx = 4100 and 4098 with N = 16 on two rows of one level -- no engine exists for one level, so these go to
the C calls directly, with tables and records of seeded random numbers (the kernels only compute with them).  Together: nseg N < 256 and = 256, N on both sides of
the LDS-table threshold, nx on both sides of 4096, one trip, an exact trip, a trip + 1 and three trips of each file's kChunk, odd and
even nx (Nyquist), both storages.  Prints one JSON object {case: {tensor: sha256}}."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from lorenzcycletoolkit_amd import _lib, tables  # noqa: E402
from lorenzcycletoolkit_amd.engine import LECEngine  # noqa: E402
from tests import ring_restatement as rr  # noqa: E402
from tests import test_gpu_spectrum, test_gpu_spectrum_b, test_gpu_spectrum_ge, test_gpu_spectrum_nl  # noqa: E402

DEV = "cuda:0"
NT, NL, NY = 3, 4, 5
SOUTH, NORTH = -60.0, 60.0
MODULES = (test_gpu_spectrum, test_gpu_spectrum_ge, test_gpu_spectrum_nl, test_gpu_spectrum_b)


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def engine_calls(dom, n, band=None):
    """{tensor: sha256} of the four calls through the engine, over the ring pass's own records."""
    eng = LECEngine(dom.lat, dom.lon, dom.level, device=DEV)
    js, jn = band or (0, dom.lat.size - 1)
    pb = eng.prepare_boxes([(0, dom.lon.size - 1, js, jn)], ring=True)
    f = [dev(a) for a in (dom.tair, dom.u, dom.v, dom.omega, dom.geopt)]
    rows = eng.rowstats(*f, pb, time_s=dom.time_s)
    nlspec, nltot = eng.rowspec_nl(*f[:4], rows, pb, n)
    return {"spec": sha(eng.rowspec(*f[:4], pb, n)), "qspec": sha(eng.rowspec_q(*f[:4], pb, n, time_s=dom.time_s)), "nlspec": sha(nlspec),
            "nltot": sha(nltot), "bspec": sha(eng.rowspec_b(*f[:4], rows, pb, n))}


def direct_calls(nx, n, nt=2, nl=1, ny=2):
    """{tensor: sha256} of the four C calls on a cube of one level and two rows, tables and records of seeded random numbers."""
    lib = _lib.load()
    rng = np.random.default_rng(nx)
    rnd = lambda *shape: dev(rng.standard_normal(shape))
    T, U, V, W = 280.0 + rnd(nt, nl, ny, nx), rnd(nt, nl, ny, nx), rnd(nt, nl, ny, nx), rnd(nt, nl, ny, nx)
    rows = rnd(nt, nl, ny, _lib.LEC_NSTAT)
    twid = dev(tables.twiddle_table(nx))
    lattab, lattab5, levtab, ptab, tcoef = rnd(ny, 4), rnd(ny, 5), rnd(nl, 3), rnd(nl, 3), rnd(nt, 3)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    common = dict(tair_d=ptr(T), u_d=ptr(U), v_d=ptr(V), omega_d=ptr(W), dtype=_lib.LEC_F64, nt=nt, nl=nl, ny=ny, nx=nx, t_begin=0, t_count=nt,
                  js=0, jn=ny - 1, n_wave=n, twid_d=ptr(twid), stream=C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream))
    new = lambda *tail: torch.empty((nt, nl, ny) + tail, dtype=torch.float64, device=DEV)
    spec, qspec, nlspec, nltot, bspec = new(n, 8), new(n), new(n, 8), new(8), new(n, 4)
    sa = _lib.RowspecArgs(spec_d=ptr(spec), **common)
    _lib.check(lib.lec_rowspec_ring(C.byref(sa)), "lec_rowspec_ring")
    qa = _lib.RowspecQArgs(lattab_d=ptr(lattab), levtab_d=ptr(levtab), tcoef_d=ptr(tcoef), inv_hdeg=nx / 360.0, qspec_d=ptr(qspec), **common)
    _lib.check(lib.lec_rowspec_q_ring(C.byref(qa)), "lec_rowspec_q_ring")
    na = _lib.RowspecNlArgs(rows_d=ptr(rows), lattab_d=ptr(lattab5), ptab_d=ptr(ptab), inv_hdeg=nx / 360.0, nlspec_d=ptr(nlspec),
                            nltot_d=ptr(nltot), **common)
    _lib.check(lib.lec_rowspec_nl_ring(C.byref(na)), "lec_rowspec_nl_ring")
    ba = _lib.RowspecBArgs(rows_d=ptr(rows), bspec_d=ptr(bspec), **common)
    _lib.check(lib.lec_rowspec_b_ring(C.byref(ba)), "lec_rowspec_b_ring")
    return {"spec": sha(spec), "qspec": sha(qspec), "nlspec": sha(nlspec), "nltot": sha(nltot), "bspec": sha(bspec)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cases = {}
    for nx, n, dtype in sorted({(nx, n, np.dtype(d).name) for m in MODULES for nx, n, d in m.RECORD_CASES}):
        dom = rr.ring_domain(NT, NL, NY, nx, seed=nx, dtype=np.dtype(dtype), lat0=SOUTH, lat1=NORTH)
        cases[f"{nx}-N{n}-{dtype}"] = engine_calls(dom, n)
    for n in (7, 20):
        cases[f"45 rows N{n}"] = engine_calls(rr.ring_domain(NT, 3, NY, 65, seed=3, lat0=SOUTH, lat1=NORTH), n)
    tall = rr.ring_domain(NT, NL, 9, 130, seed=9, lat0=SOUTH, lat1=NORTH)
    cases["inner band rows 2..6 of 9, 130-N20"] = engine_calls(tall, 20, band=(2, 6))
    cases["two-row band rows 3..4 of 9, 130-N20"] = engine_calls(tall, 20, band=(3, 4))
    for nx in (4100, 4098):
        cases[f"{nx}-N16 two rows, one level"] = direct_calls(nx, 16)
    out = {"library": os.path.basename(_lib.LIB_PATH), "sha256": cases}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
