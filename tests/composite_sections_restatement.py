"""The system-relative latitude x pressure sections of the ten terms (-t / -c --composite-sections), restated on
the CPU from the oracle.  Nothing of the kernel is restated here: for every time step the oracle's own per-step ``Box`` is built exactly as
``oracle.lec_moving`` builds it (``composite_restatement.step_boxes``), the sections are ``sections_restatement.sections`` of that box, the
columns ``sections_restatement.columns``, and the time mean runs in time order (``sections_restatement.time_mean``).

Order of the terms: Az Ae Kz Ke Cz Ca Ck Ce Gz Ge (``sections_restatement.TERMS``).  Boxes are inclusive index quadruples (iw, ie, js, jn)
on ``dom``'s grid and must all have one ROW COUNT; their widths may differ."""
from __future__ import annotations

import numpy as np

from oracle import lec_oracle as o
from tests import composite_restatement as cr
from tests import sections_restatement as sr

TERMS = sr.TERMS


def composite_sections(dom: o.Domain, boxes):
    """(X [T, 10, level, nyb], C [T, 10, nyb], M [10, level, nyb], cw [T, nyb]) -- the per-step sections on box-relative rows, their
    columns, the time-mean section and every step's own area weights."""
    X, C, W = [], [], []
    for b in cr.step_boxes(dom, boxes):
        x = sr.sections(b)
        if X and x.shape[-1] != X[0].shape[-1]:
            raise ValueError("boxes of one row count")
        X.append(x[0])
        C.append(sr.columns(x, b.level)[0])
        W.append(sr.area_weights(b))
    X = np.stack(X)
    return X, np.stack(C), sr.time_mean(X), np.stack(W)
