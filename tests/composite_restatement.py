"""The system-relative composites of the six eddy terms (-t / -c --composites), restated on the CPU from the
oracle.  Nothing of the kernel is restated here: for every time step the oracle's own per-step ``Box`` is built exactly as
``oracle.lec_moving`` builds it (``make_box(sub_t, *boxes[t], dTdt=moving_dTdt(dom)[t:t+1], fixed=False)``), the integrands are those of
``tests/maps_restatement.maps`` on that box taken as an open box, the column integrals ``maps_restatement.columns``, the Hovmoeller is
formed with that box's own ``sections_restatement.area_weights``, and the time mean runs in time order.

Order of the terms: Ae Ke Ca Ce Ck Ge (``maps_restatement.TERMS``).  Boxes are inclusive index quadruples (iw, ie, js, jn) on ``dom``'s
grid and must all have one shape."""
from __future__ import annotations

import numpy as np

from oracle import lec_oracle as o
from tests import maps_restatement as mr
from tests import sections_restatement as sr

TERMS = mr.TERMS


def limits(dom: o.Domain, box):
    """(west, east, south, north) in degrees of the index box: the grid's own coordinates, which ``make_box`` selects back exactly."""
    iw, ie, js, jn = box
    return dom.lon[iw], dom.lon[ie], dom.lat[js], dom.lat[jn]


def step_boxes(dom: o.Domain, boxes):
    """The oracle's ``Box`` of every time step, as ``oracle.lec_moving`` builds them."""
    dTdt = o.moving_dTdt(dom)
    out = []
    for t, box in enumerate(boxes):
        sub = o.Domain(dom.tair[t:t + 1], dom.u[t:t + 1], dom.v[t:t + 1], dom.omega[t:t + 1], dom.geopt[t:t + 1], dom.lat, dom.lon,
                       dom.level, dom.time_s[t:t + 1])
        b = o.make_box(sub, *limits(dom, box), dTdt=dTdt[t:t + 1], fixed=False)
        assert tuple(b.idx) == tuple(int(x) for x in box), (t, b.idx, box)
        out.append(b)
    return out


def composites(dom: o.Domain, boxes, with_integrands: bool = False):
    """(C [T, 6, nyb, nxb], H [T, 6, nxb], M [6, nyb, nxb]) -- the per-step columns, the Hovmoeller and the time-mean composite; with
    ``with_integrands`` also Y [T, 6, level, nyb, nxb], the integrands the columns were taken of."""
    C, H, Y = [], [], []
    for b in step_boxes(dom, boxes):
        y = mr.maps(b, ring=False)
        c = mr.columns(y, b.level)
        C.append(c[0])
        H.append(mr.hovmoller(c, sr.area_weights(b))[0])
        Y.append(y[0])
    C = np.stack(C)
    if C.shape[2:] != C[0].shape[1:]:
        raise ValueError("boxes of one shape")
    out = (C, np.stack(H), mr.time_mean(C))
    return out + (np.stack(Y),) if with_integrands else out


def box_zonal_average(H: np.ndarray, bs) -> np.ndarray:
    """[T, ...] -> the zonal average over the LAST axis of H[t] with step t's own ``Box`` ``bs[t]`` (``maps_restatement.zonal_average``
    on an open box)."""
    return np.stack([mr.zonal_average(H[t], b, False) for t, b in enumerate(bs)])
