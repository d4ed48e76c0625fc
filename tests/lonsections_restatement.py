"""The longitude x pressure sections of the six eddy terms (-f [--periodic] --lon-sections, -t / -c --composite-lon-sections; DESIGN.md
section 4.2h), restated on the CPU from the oracle.  Nothing of the kernel is restated here: a section is the integrand of
``tests/maps_restatement.maps`` -- the sections' integrand with the zonal average left off -- summed over the box's rows with the
oracle's own area weights (``sections_restatement.area_weights``), rows ascending in a plain running sum.  ``area_average`` and
``zonal_average`` are linear, so the box's zonal average of a section is ``sum_j cw_j`` of ``sections_restatement.sections``, and its
vertical trapezoid (``sections_restatement.columns``) the Hovmoeller of the maps.

Order of the terms: Ae Ke Ca Ce Ck Ge (``maps_restatement.TERMS``)."""
from __future__ import annotations

import numpy as np

from tests import composite_restatement as cr
from tests import maps_restatement as mr
from tests import sections_restatement as sr

TERMS = mr.TERMS


def lon_sections(Y: np.ndarray, cw: np.ndarray) -> np.ndarray:
    """X [time, 6, level, lon] = sum_j cw_j Y[time, 6, level, j, lon], rows ascending from 0.0 (``Y``: ``maps_restatement.maps``,
    ``cw``: ``sections_restatement.area_weights``); NaN propagates."""
    X = np.zeros(Y.shape[:3] + Y.shape[4:])
    for j in range(Y.shape[3]):
        X = X + cw[j] * Y[:, :, :, j]
    return X


def composite_lon_sections(dom, boxes) -> np.ndarray:
    """X [T, 6, level, nxb] over per-step boxes of one shape: step t's integrands on the oracle's own ``Box`` of that step
    (``composite_restatement.composites(..., with_integrands=True)``) with that step's ``area_weights``."""
    Y = cr.composites(dom, boxes, with_integrands=True)[3]
    bs = cr.step_boxes(dom, boxes)
    return np.stack([lon_sections(Y[t: t + 1], sr.area_weights(b))[0] for t, b in enumerate(bs)])


def time_mean(X: np.ndarray) -> np.ndarray:
    """(1 / T) sum_t X[t], summed in time order; NaN at any step gives NaN."""
    return sr.time_mean(X)


def columns(X: np.ndarray, level: np.ndarray) -> np.ndarray:
    """H [time, 6, lon]: s_f times the trapezoid of X [time, 6, level, lon] over the levels (``sections_restatement.columns``)."""
    return sr.columns(X, level, TERMS)
