"""The phase-aligned ensembles of a batch's composites, restated in NumPy with nothing of the kernels': from the per-step columns that
``tests/batch_composite_restatement.composites`` returns and a range table [K, B, 2] of every track's own steps, the mean of every
(track, bin) cell, and per bin the ensemble and the n - 1 spread over the tracks that have a step in it."""
import numpy as np


def phases(per, ranges):
    """``per``: [(C, H, M) per track], C [steps, 6, nyb, nxb]; ``ranges`` int [K, B, 2].  Returns (mean [K, B, 6, nyb, nxb] -- NaN for an empty
    cell --, ens [B, 6, nyb, nxb], spread [B, 6, nyb, nxb], count [K, B], members [B]).  ens is NaN without a member, spread below two."""
    ranges = np.asarray(ranges)
    K, B = ranges.shape[:2]
    shape = per[0][0].shape[1:]
    mean = np.full((K, B) + shape, np.nan)
    count = (ranges[:, :, 1] - ranges[:, :, 0]).astype(np.int64)
    with np.errstate(invalid="ignore"):
        for k in range(K):
            for b in range(B):
                lo, hi = ranges[k, b]
                if hi > lo:
                    mean[k, b] = np.mean(per[k][0][lo:hi], axis=0)
        members = (count >= 1).sum(axis=0)
        ens, spread = np.full((B,) + shape, np.nan), np.full((B,) + shape, np.nan)
        for b in range(B):
            who = np.flatnonzero(count[:, b] >= 1)
            if who.size:
                ens[b] = np.mean(mean[who, b], axis=0)
            if who.size >= 2:
                spread[b] = np.std(mean[who, b], axis=0, ddof=1)
    return mean, ens, spread, count, members
