"""The composites of a BATCH of tracks over one union domain, restated on the CPU with nothing of its own: every track is cut out of the
union as the ``oracle.Domain`` of its own steps -- the data set of the track's single run -- and handed to
``composite_restatement.composites``; the ensemble is the NumPy mean of the tracks' time-mean composites.  No kernel logic is restated
here."""
import numpy as np

from oracle import lec_oracle as o
from tests import composite_restatement as cr


def track_domain(dom: o.Domain, ustep) -> o.Domain:
    """The union domain restricted to the track's steps, its time axis starting at 0 (the track's single run)."""
    u = np.asarray(ustep)
    c = lambda a: np.ascontiguousarray(a[u])
    return o.Domain(c(dom.tair), c(dom.u), c(dom.v), c(dom.omega), c(dom.geopt), dom.lat, dom.lon, dom.level,
                    np.asarray(dom.time_s)[u] - np.asarray(dom.time_s)[u[0]])


def composites(dom: o.Domain, tracks):
    """``tracks``: [(union steps, boxes)].  Returns ([(C, H, M) per track], E): ``composite_restatement.composites`` of every track's own
    domain, and E [6, nyb, nxb] the mean over the tracks of their M."""
    per = []
    with np.errstate(invalid="ignore"):
        for ustep, boxes in tracks:
            per.append(cr.composites(track_domain(dom, ustep), boxes))
        ens = np.mean(np.stack([m for _, _, m in per]), axis=0)
    return per, ens


def closure(dom: o.Domain, ustep, boxes, H: np.ndarray):
    """(za, sc), both [steps, 6]: the zonal average over every step's own box of the track's Hovmoeller ``H``, and ``oracle.lec_moving``'s
    scalars of the track alone, in ``composite_restatement.TERMS``' order."""
    d = track_domain(dom, ustep)
    sc, _ = o.lec_moving(d, [cr.limits(d, b) for b in boxes], residuals=False)
    za = cr.box_zonal_average(H, cr.step_boxes(d, boxes))
    return za, np.stack([np.asarray(sc[t], dtype=np.float64) for t in cr.TERMS], axis=1)
