"""Case builders for the seams of csrc/lec_follow.hip (and lec_diag.hip's LDS tree)  --  TEST INFRASTRUCTURE ONLY; no GPU, no torch.

A case is stated in GRID INDICES -- slice [ny][nx], field, sense, r, (sj, si) or (ej, ei, k_max, threshold), the admissible bounds
(jlo, jhi, ilo, ihi) and the start -- which is what the C ABI takes; nothing is imported from lorenzcycletoolkit_amd/follow.py, whose
degree-based wrappers cannot state most of them.  The index-level restatement (``chain``, ``seeds``) is written from the rule text in
include/lec_hip.h on top of what exists: follow_restatement.smoothed, follow_many_restatement.candidates_of and
follow_ring_restatement.smoothed_at / smoothed.

Exact fields.  Apart from the zeta cases every field is ``hgt`` with small non-negative integers (< 2^20): every row-major sum of at
most (2 r + 1)^2 of them is exact and sum / cnt is ONE correctly rounded division on both sides, so positions, status AND value bits
must be equal, and ties among smoothed values can be planted on purpose (r = 0: equal values; r = 1: one dip in a constant field gives
a 3 x 3 plateau of equal means whose first point in row-major order is (j - 1, i - 1)).

The launch arithmetic, restated (``launch_numbers``, ``place``): one workgroup of 256 threads; window point n (row-major in the window)
is scanned by thread n % 256 -- wave (n % 256) // 64 -- on trip n // 256; the LDS tile is the window grown by r and cut by the slice
(on a ring: never cut along longitude).  ``lec_follow_seeds``' selection scans admissible index a = (j - jlo) nxa + (i - ilo) the same
way and strikes a winner through thread a % 256.

Families (``CHAIN_FAMILIES`` / ``SEED_FAMILIES``: family -> case ids; ``case(id)`` -> dict; ``reference(id)`` -> the restatement's answer):
  partition  hgt, r = 0, MIN and MAX: windows of 9, 63, 64, 65, 255, 256, 258 (257 is prime: no window of a 40 x 48 slice has 257
             points) and 513 points, the unique extremum at window index 0, 63, 64, 255, 256, 511, 512, npt - 1 wherever it exists, all
             other values distinct; each with a start, and without one on bounds equal to the window (the strided scan of all admissible
             centres through smooth_global).
  ties       a 513-point window, two steps: equal extremes at (3, 40), (70, 200), (200, 261), (7, 263), (386, 512), every point equal, and
             every point equal except NaN at n = 0; r = 0 by equal values, r = 1 by plateaus; MIN and MAX.  Every case also has the ring
             rule's answer (the bounds span all columns), which differs where the second window meets the slice's edge.
  clip       centres on the bounds and in their corners, bounds on the slice's edge with r in {1, 2, sj + 2}, sj >= ny and si >= nx,
             a one-row band, and zeta in both formulations at the slice's corners (the one-sided stencils).
  missing    -inf / +inf at the would-be extremum (r = 0) and beside it (r = 1), a point whose whole neighbourhood is NaN, a window
             with one finite point, a blind step between two finite ones and a blind first step; each with a start and without.
  ring       lec_follow_spans_chunk_ring on a 16 x 25 ring: tile runs with it0 < 0, it0 == 0, it1 == nx - 1, it1 >= nx, the tile that
             is the whole ring (2 si + 1 + 2 r is odd, hence the odd nx), and equal values at columns nx - 1 and 0 of one row.
  seeds-*    lec_follow_seeds and the two series calls: see ``_seed_cases``.
"""
import functools

import numpy as np

from tests import follow_many_restatement as fmr
from tests import follow_restatement as fr
from tests import follow_ring_restatement as frr

NY, NX = 40, 48
RING_NY, RING_NX = 16, 25
LAT, LON = -50.0 + np.arange(NY), -70.0 + np.arange(NX)                     # a plain 1-degree grid: the vorticity tables
RING_LAT, RING_LON = -30.0 + 4.0 * np.arange(RING_NY), (360.0 / RING_NX) * np.arange(RING_NX)
THREADS, WAVE = 256, 64
MIN, MAX = 0, 1
FORMS = ("metpy_no_crs", "spherical")
HGT_LIMIT = 2 ** 20
FULL = (0, NY - 1, 0, NX - 1)
RING_BOUNDS = (2, RING_NY - 3, 0, RING_NX - 1)
BEST = {MIN: 5.0, MAX: 900000.0}             # a planted extremum: better than every background value
LDS_FIXED, LDS_LIMIT = 64, 160 * 1024
NEAR_TIE, VALUE_BAR = 1e-9, 1e-11            # tests/test_gpu_follow.py's (the GPU test asserts that they are)
SERIES_GRID = 1 << 16                        # workgroups per launch of the series kernels at the most
CAPPED = dict(ny=64, nx=64, nt=4097, patterns=5, k_max=8)


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch arithmetic, restated (follow_chain, seeds_select, check_window in csrc/lec_follow.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def launch_numbers(ny, nx, r, sj, si, bounds, centre, ring=False):
    """What one step of follow_chain does around ``centre`` (None: step 0 without a start)."""
    jlo, jhi, ilo, ihi = bounds
    if centre is None:
        j0, j1, i0, i1 = jlo, jhi, ilo, ihi
    else:
        j0, j1 = max(jlo, centre[0] - sj), min(jhi, centre[0] + sj)
        i0, i1 = (centre[1] - si, centre[1] + si) if ring else (max(ilo, centre[1] - si), min(ihi, centre[1] + si))
    nxw = i1 - i0 + 1
    jt0, jt1 = max(j0 - r, 0), min(j1 + r, ny - 1)
    it0, it1 = (i0 - r, i1 + r) if ring else (max(i0 - r, 0), min(i1 + r, nx - 1))
    th, tw = min(2 * sj + 1 + 2 * r, ny), (2 * si + 1 + 2 * r if ring else min(2 * si + 1 + 2 * r, nx))
    return dict(window=(j0, j1, i0, i1), nxw=nxw, npt=nxw * (j1 - j0 + 1), whole=centre is None, tile=(jt0, jt1, it0, it1),
                ntile=(it1 - it0 + 1) * (jt1 - jt0 + 1), lds_doubles=th * tw,
                tile_cut=dict(south=j0 - r < 0, north=j1 + r > ny - 1, west=(not ring) and i0 - r < 0, east=(not ring) and i1 + r > nx - 1),
                window_cut=dict(south=centre is not None and centre[0] - sj < jlo, north=centre is not None and centre[0] + sj > jhi,
                                west=centre is not None and not ring and centre[1] - si < ilo,
                                east=centre is not None and not ring and centre[1] + si > ihi))


def place(n):
    """Who scans point n of a window (or admissible index n of the seeds' selection)."""
    return dict(thread=n % THREADS, wave=(n % THREADS) // WAVE, lane=n % WAVE, trip=n // THREADS)


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule, restated by index
# ---------------------------------------------------------------------------------------------------------------------------------
def chain(F, sense, r, sj, si, bounds, start, ring=False):
    """lec_follow's chain on F [nt][ny][nx] from ``start`` ((-1, -1): none) -> dict(pos [nt][2], val [nt], status [nt], windows: the
    launch_numbers of every step, W: every step's smoothed window (NaN where S is not finite), margin [nt]: the distance from the best
    to the nearest DIFFERENT value of the window over max |finite F| of the series (inf for a tie or a lone value), tile_scale [nt])."""
    F = np.asarray(F, dtype=np.float64)
    nt, ny, nx = F.shape
    jlo, jhi, ilo, ihi = bounds
    want_max = sense == MAX
    centre = None if tuple(start) == (-1, -1) else (int(start[0]), int(start[1]))
    assert centre is None or (jlo <= centre[0] <= jhi and ilo <= centre[1] <= ihi)
    assert not ring or (centre is not None and (ilo, ihi) == (0, nx - 1) and 2 * si + 1 + 2 * r <= nx)
    fin = np.isfinite(F)
    scale = float(np.max(np.abs(F[fin]))) if fin.any() else 0.0
    pos, val, status, windows, Ws, margin, tile_scale = [], [], [], [], [], [], []
    for t in range(nt):
        ln = launch_numbers(ny, nx, r, sj, si, bounds, centre, ring)
        j0, j1, i0, i1 = ln["window"]
        if ring:
            cols = [(i0 + k) % nx for k in range(ln["nxw"])]                       # west to east, never cut
            W = np.array([[frr.smoothed_at(F[t], r, j, i) for i in cols] for j in range(j0, j1 + 1)])
            tcols = [(i0 - r + k) % nx for k in range(ln["nxw"] + 2 * r)]
        else:
            cols = list(range(i0, i1 + 1))
            W = fr.smoothed(F[t], r, (j0, j1, i0, i1))[j0: j1 + 1, i0: i1 + 1]
            tcols = list(range(ln["tile"][2], ln["tile"][3] + 1))
        T = F[t][ln["tile"][0]: ln["tile"][1] + 1][:, tcols]
        tile_scale.append(float(np.max(np.abs(T[np.isfinite(T)]))) if np.isfinite(T).any() else 0.0)
        ok = np.isfinite(W)
        windows.append(ln); Ws.append(W)
        if not ok.any():
            if centre is None:
                centre = (jlo, ilo)
            pos.append(centre); val.append(np.nan); status.append(1); margin.append(np.inf)
            continue
        key = np.where(ok, W, -np.inf if want_max else np.inf)
        n = int(np.argmax(key) if want_max else np.argmin(key))                    # the first in row-major order of the window
        centre = (j0 + n // ln["nxw"], cols[n % ln["nxw"]])
        best = float(W.ravel()[n])
        others = W[ok & (W != best)]
        margin.append(float(np.min(np.abs(others - best))) / scale if others.size else np.inf)
        pos.append(centre); val.append(best); status.append(0)
    return dict(pos=np.array(pos, dtype=np.int64), val=np.array(val), status=np.array(status, dtype=np.int64), windows=windows, W=Ws,
                margin=np.array(margin), tile_scale=np.array(tile_scale), scale=scale)


def spans_of(status, t_base=0):
    """(span, weak) of a chain that never stops under a NaN end threshold: a walked step is good when its status is 0."""
    good = [t_base + t for t, s in enumerate(status) if s == 0]
    weak = 0
    for s in status:
        weak = 0 if s == 0 else weak + 1
    return ((good[0], good[-1]) if good else (-1, -1)), weak


def winners(W, sense):
    """The window indices a tie could go to: dict(rule = first in row-major order, last, thread = lowest thread first, wave = lowest
    wave first, tied = every index that holds the best value)."""
    flat = W.ravel()
    ok = np.isfinite(flat)
    best = flat[ok].max() if sense == MAX else flat[ok].min()
    tied = [int(n) for n in np.flatnonzero(ok & (flat == best))]
    return dict(rule=min(tied), last=max(tied), thread=min(tied, key=lambda n: (n % THREADS, n)),
                wave=min(tied, key=lambda n: ((n % THREADS) // WAVE, n)), tied=tied)


def _ring_candidates(S, bounds, ej, ei, want_max, threshold):
    """follow_many_restatement.candidates_of with the ring's neighbourhood (ring distance <= ei); the tie clause keeps the slice's
    absolute row-major index."""
    ny, nx = S.shape
    sgn = -1.0 if want_max else 1.0
    out = []
    for j in range(bounds[0], bounds[1] + 1):
        for i in range(nx):
            s = S[j, i]
            if not np.isfinite(s) or (threshold is not None and sgn * s > sgn * threshold):
                continue
            ok = True
            for jj in range(max(j - ej, 0), min(j + ej, ny - 1) + 1):
                for d in range(-ei, ei + 1):
                    ii = (i + d) % nx
                    if (jj, ii) == (j, i) or not np.isfinite(S[jj, ii]):
                        continue
                    diff = sgn * (S[jj, ii] - s)
                    if diff < 0 or (diff == 0 and (jj, ii) < (j, i)):
                        ok = False
            if ok:
                out.append((sgn * s, j * nx + i, j, i, float(s), np.inf))
    out.sort()
    return out


def seeds(F, sense, r, ej, ei, k_max, threshold, bounds, ring=False):
    """lec_follow_seeds on one slice F [ny][nx] -> dict(pos [k_max][2] with (-2, -2) marks, val [k_max] with NaN marks, n_found,
    candidates: all of them, best first, as (key, row-major index, j, i, S, gap))."""
    F = np.asarray(F, dtype=np.float64)
    if ring:
        assert 2 * ei + 1 <= F.shape[1] and (bounds[2], bounds[3]) == (0, F.shape[1] - 1)
        cands = _ring_candidates(frr.smoothed(F, r), bounds, ej, ei, sense == MAX, threshold)
    else:
        cands = fmr.candidates_of(fr.smoothed(F, r), bounds, ej, ei, sense == MAX, threshold)
    pos, val = np.full((k_max, 2), -2, dtype=np.int64), np.full(k_max, np.nan)
    for k, c in enumerate(cands[:k_max]):
        pos[k], val[k] = (c[2], c[3]), c[4]
    return dict(pos=pos, val=val, n_found=min(len(cands), k_max), candidates=cands)


# ---------------------------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------------------------
def _background(seed, shape=(NY, NX)):
    """Distinct integers 1000 .. 1000 + ny nx - 1 in a random order: worse than BEST in either sense."""
    n = int(np.prod(shape))
    return 1000.0 + np.random.default_rng(seed).permutation(n).reshape(shape).astype(np.float64)


def _ramp(sense, shape=(NY, NX)):
    """Monotone in row-major order, worse and worse: no point but (0, 0) is an extremum of its neighbourhood."""
    k = np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)
    return 1000.0 + k if sense == MIN else 500000.0 - k


def _at(ln, n, nx=None):
    """Grid position of window index n (``nx``: on a ring)."""
    j, i = ln["window"][0] + n // ln["nxw"], ln["window"][2] + n % ln["nxw"]
    return (j, i % nx) if nx else (j, i)


_CASES, CHAIN_FAMILIES, SEED_FAMILIES = {}, {}, {}


def _add(fam, cid, **kw):
    assert cid not in _CASES, cid
    kw.setdefault("field", "hgt"); kw.setdefault("ring", False); kw.setdefault("plants", [])
    _CASES[cid] = dict(kw, id=cid, family=fam)
    (SEED_FAMILIES if fam.startswith("seeds") else CHAIN_FAMILIES).setdefault(fam, []).append(cid)


SENSES = ((MIN, "min"), (MAX, "max"))
CENTRE = (20, 24)
# npt -> (sj, si, bounds): windows around CENTRE; an odd x odd window cannot give 64, 256 or 258, the bounds cut those
PARTITION = {9: (1, 1, FULL), 63: (3, 4, FULL), 64: (4, 4, (0, 23, 0, 27)), 65: (2, 6, FULL), 255: (7, 8, FULL),
             256: (8, 8, (0, 27, 0, 31)), 258: (3, 21, (0, 22, 0, 47)), 513: (9, 13, FULL)}
PLANT_AT = (0, 63, 64, 255, 256, 511, 512)


def _partition_cases():
    for npt, (sj, si, bounds) in PARTITION.items():
        ln = launch_numbers(NY, NX, 0, sj, si, bounds, CENTRE)
        assert ln["npt"] == npt
        for sense, word in SENSES:
            bg = _background(100 + npt + sense)
            for n in sorted({m for m in PLANT_AT if m < npt} | {npt - 1}):
                F = bg.copy()
                F[_at(ln, n)] = BEST[sense]
                common = dict(F=F[None], sense=sense, r=0, sj=sj, si=si, plants=[(0, n)], expect=dict(npt=npt, n=n))
                _add("partition", f"part-{npt}-n{n}-{word}", bounds=bounds, start=CENTRE, **common)
                _add("partition", f"part-{npt}-n{n}-{word}-nostart", bounds=ln["window"], start=(-1, -1), **common)


TIE_WINDOW = dict(sj=9, si=13, start=(20, 25))           # 19 x 27 = 513 points, three trips
TIE_LAYOUTS = {"samewave": (3, 40), "waves": (70, 200), "wave3-trip1": (200, 261), "samethread": (7, 263), "trip1-trip2": (386, 512),
               "allequal": None, "allequal-nan0": None}


def _tie_cases():
    sj, si, start = TIE_WINDOW["sj"], TIE_WINDOW["si"], TIE_WINDOW["start"]
    for name, pair in TIE_LAYOUTS.items():
        for r in (0, 1):
            for sense, word in SENSES:
                centre, steps, plants = start, [], []
                for t in range(2):
                    ln = launch_numbers(NY, NX, r, sj, si, FULL, centre)
                    if pair is None:
                        F = np.full((NY, NX), 1000.0)
                        if name.endswith("nan0"):
                            F[_at(ln, 0)] = np.nan
                            plants.append((t, 0))
                    elif r == 0:
                        F = _background(300 + 7 * t + sense)
                        for n in pair:
                            F[_at(ln, n)] = BEST[sense]
                    else:                                   # one dip at (j + 1, i + 1): the 3 x 3 of equal means begins at (j, i)
                        F = np.full((NY, NX), 1000.0)
                        for n in pair:
                            j, i = _at(ln, n)
                            assert j + 1 < NY and i + 1 < NX
                            F[j + 1, i + 1] = 100.0 if sense == MIN else 10000.0
                    if pair is not None:
                        assert pair[1] < ln["npt"]
                        plants += [(t, pair[0]), (t, pair[1])]
                        centre = _at(ln, pair[0])
                    else:                                   # every S equal: the window's first point (r = 1 heals the NaN at n = 0)
                        centre = _at(ln, 1 if name.endswith("nan0") and r == 0 else 0)
                    steps.append(F)
                _add("ties", f"tie-{name}-r{r}-{word}", F=np.stack(steps), sense=sense, r=r, sj=sj, si=si, bounds=FULL, start=start,
                     plants=plants, expect=dict(pair=pair, layout=name))


CLIP_BOUNDS = (5, 30, 6, 40)


def _uv(seed):
    rng = np.random.default_rng(seed)
    return 10.0 * rng.standard_normal((2, 2, NY, NX))


def _clip_cases():
    jlo, jhi, ilo, ihi = CLIP_BOUNDS
    on = {"south": (jlo, 20), "north": (jhi, 20), "west": (17, ilo), "east": (17, ihi), "sw": (jlo, ilo), "se": (jlo, ihi),
          "nw": (jhi, ilo), "ne": (jhi, ihi)}
    corners = {"sw": (0, 0), "se": (0, NX - 1), "nw": (NY - 1, 0), "ne": (NY - 1, NX - 1)}
    k = 0
    for sense, word in SENSES:
        for name, c in on.items():
            k += 1
            _add("clip", f"clip-bound-{name}-{word}", F=np.stack([_background(400 + k), _background(450 + k)]), sense=sense, r=1, sj=2, si=3,
                 bounds=CLIP_BOUNDS, start=c, expect=dict(on=name))
        for name, c in corners.items():
            for r in (1, 2, 4):                             # 4 = sj + 2: r > sj
                k += 1
                _add("clip", f"clip-edge-{name}-r{r}-{word}", F=np.stack([_background(500 + k), _background(550 + k)]), sense=sense, r=r,
                     sj=2, si=3, bounds=FULL, start=c, expect=dict(corner=name))
        for name, b in (("full", FULL), ("inner", CLIP_BOUNDS)):
            k += 1
            _add("clip", f"clip-whole-{name}-{word}", F=np.stack([_background(600 + k), _background(650 + k)]), sense=sense, r=1, sj=NY, si=NX,
                 bounds=b, start=CENTRE, expect=dict(whole=True))
        for r in (0, 1):
            k += 1
            _add("clip", f"clip-band-r{r}-{word}", F=np.stack([_background(700 + k), _background(750 + k)]), sense=sense, r=r, sj=2, si=3,
                 bounds=(17, 17, ilo, ihi), start=(17, 20), expect=dict(band=True))
        for form in FORMS:
            for name, c in corners.items():
                for r in (0, 1):
                    k += 1
                    u, v = _uv(800 + k)
                    _add("clip", f"clip-zeta-{form}-{name}-r{r}-{word}", field="zeta", form=form, u=u, v=v,
                         F=fr.field_of(u, v, None, LAT, LON, "zeta", form), sense=sense, r=r, sj=2, si=3, bounds=FULL, start=c,
                         expect=dict(corner=name))


MISS = dict(sj=2, si=3, start=CENTRE)                        # a 5 x 7 window, rows 18..22, columns 21..27


def _missing_cases():
    sj, si = MISS["sj"], MISS["si"]
    ln = launch_numbers(NY, NX, 0, sj, si, FULL, CENTRE)
    inf = np.inf

    def both(cid, F, sense, r, plants):
        _add("missing", cid, F=F, sense=sense, r=r, sj=sj, si=si, bounds=FULL, start=CENTRE, plants=plants, expect={})
        _add("missing", cid + "-nostart", F=F, sense=sense, r=r, sj=sj, si=si, bounds=ln["window"], start=(-1, -1), plants=plants, expect={})

    for sense, word in SENSES:
        F = _background(900 + sense)                        # r = 0: the infinity at n = 10 would win, the true extremum is n = 20
        F[_at(ln, 10)] = -inf if sense == MIN else inf
        F[_at(ln, 24)] = inf if sense == MIN else -inf
        F[_at(ln, 20)] = BEST[sense]
        both(f"miss-inf-r0-{word}", F[None], sense, 0, [(0, 10), (0, 20), (0, 24)])
        F = _background(910 + sense)                        # r = 1: neither may enter a mean
        F[_at(ln, 10)], F[_at(ln, 22)] = -inf, inf
        both(f"miss-inf-r1-{word}", F[None], sense, 1, [(0, 10), (0, 22)])
        F = _background(920 + sense)                        # the centre's whole neighbourhood is NaN: that window point is skipped
        F[CENTRE[0] - 1: CENTRE[0] + 2, CENTRE[1] - 1: CENTRE[1] + 2] = np.nan
        both(f"miss-hole-r1-{word}", F[None], sense, 1, [(0, 17)])
        for r in (0, 1):
            F = np.full((NY, NX), np.nan)                   # one finite point (r = 1: a plateau of nine equal means)
            F[_at(ln, 12)] = 1234.0
            both(f"miss-one-r{r}-{word}", F[None], sense, r, [(0, 12)])
            F = np.stack([_background(930 + sense), np.full((NY, NX), np.nan), _background(940 + sense)])
            both(f"miss-blind-r{r}-{word}", F, sense, r, [])
            F = np.stack([np.full((NY, NX), np.nan), _background(950 + sense)])       # blind at once: the start (none: jlo, ilo) is kept
            both(f"miss-blind-first-r{r}-{word}", F, sense, r, [])


def _ring_cases():
    sj = 2
    k = 0
    for sense, word in SENSES:
        for name, ic in (("it0-neg", 2), ("it0-zero", 4), ("it1-last", 20), ("it1-over", 22)):
            k += 1
            _add("ring", f"ring-{name}-{word}", ring=True, F=np.stack([_background(1000 + k, (RING_NY, RING_NX)), _background(1050 + k, (RING_NY, RING_NX))]),
                 sense=sense, r=1, sj=sj, si=3, bounds=RING_BOUNDS, start=(8, ic), expect=dict(run=name))
        k += 1
        _add("ring", f"ring-whole-{word}", ring=True, F=np.stack([_background(1100 + k, (RING_NY, RING_NX)), _background(1150 + k, (RING_NY, RING_NX))]),
             sense=sense, r=2, sj=sj, si=10, bounds=RING_BOUNDS, start=(8, 7), expect=dict(run="whole"))
        for ic in (0, 24, 2):                               # the window straddles the seam: column nx - 1 comes first
            F = _background(1200 + k + ic, (RING_NY, RING_NX))
            F[8, RING_NX - 1] = F[8, 0] = BEST[sense]
            ln = launch_numbers(RING_NY, RING_NX, 0, sj, 3, RING_BOUNDS, (8, ic), True)
            n1 = 2 * ln["nxw"] + (RING_NX - 1 - ln["window"][2]) % RING_NX
            _add("ring", f"ring-seam-tie-c{ic}-{word}", ring=True, F=np.stack([F, _background(1250 + k + ic, (RING_NY, RING_NX))]), sense=sense, r=0,
                 sj=sj, si=3, bounds=RING_BOUNDS, start=(8, ic), plants=[(0, n1), (0, n1 + 1)], expect=dict(run="seam-tie"))


# seeds ---------------------------------------------------------------------------------------------------------------------------
# admissible counts: below 64, 255, 256, the next above (258), the whole slice
SEED_BOUNDS = {50: (10, 14, 10, 19), 255: (12, 26, 15, 31), 256: (12, 27, 16, 31), 258: (17, 22, 3, 45), NY * NX: FULL}


def _seed(fam, cid, F, sense, **kw):
    kw = dict(dict(r=0, ej=1, ei=1, k_max=8, threshold=None, bounds=FULL, ring=False), **kw)
    _add(fam, cid, F=F, sense=sense, **kw)


def _lows(sense, at, values, shape=(NY, NX)):
    F = _ramp(sense, shape)
    for (j, i), x in zip(at, values):
        F[j, i] = x if sense == MIN else 600000.0 - x
    return F


def _seed_cases():
    for sense, word in SENSES:
        # admissible counts: seeds at admissible index 0, 255, 256 and na - 1 (wherever they exist) and one in the middle
        for na, b in SEED_BOUNDS.items():
            nxa = b[3] - b[2] + 1
            assert nxa * (b[1] - b[0] + 1) == na
            for variant, want in (("a", (0, 255, na // 2, na - 1)), ("b", (256, 3))):       # 255 and 256 are neighbours: a slice each
                idx = sorted({a for a in want if a < na})
                if variant == "b" and 256 >= na:
                    continue
                at = [(b[0] + a // nxa, b[2] + a % nxa) for a in idx]
                assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) > 1 for n, p in enumerate(at) for q in at[:n])
                _seed("seeds-count", f"seeds-na{na}{variant}-{word}", _lows(sense, at, [10 + 3 * n for n in range(len(at))]), sense, bounds=b,
                      plants=at, expect=dict(na=na, index=idx))
        # equal values far apart, ordered by the slice's row-major index; k_max cuts between two of them, equals the count, is 1
        at = [(30, 40), (5, 7), (5, 30), (20, 3), (33, 10), (12, 44), (25, 25)]
        F = _lows(sense, at, [7, 7, 3, 7, 3, 7, 7])
        ncand = len(seeds(F, sense, 0, 1, 1, 256, None, FULL)["candidates"])
        for k in (1, 4, ncand, ncand + 3):
            _seed("seeds-order", f"seeds-order-k{k}-{word}", F, sense, k_max=k, plants=at, expect=dict(ncand=ncand))
        # a lattice of isolated lows, k_max = 256: value-then-index order over many equal values, the rest marked
        at = [(j, i) for j in range(1, NY, 3) for i in range(1, NX, 3)]
        _seed("seeds-lattice", f"seeds-lattice-{word}", _lows(sense, at, [(7 * j + 3 * i) % 10 for j, i in at]), sense, k_max=256, plants=at,
              expect=dict(count=len(at)))
        # threshold: equal keeps, one beyond rejects
        at = [(8, 8), (20, 30), (31, 12)]
        F = _lows(sense, at, [3, 7, 9])
        worst = F[31, 12]
        for name, thr in (("equal", worst), ("beyond", worst - 1 if sense == MIN else worst + 1), ("none", None)):
            _seed("seeds-threshold", f"seeds-thr-{name}-{word}", F, sense, threshold=None if thr is None else float(thr), plants=at,
                  expect=dict(kept={"equal": 3, "beyond": 2, "none": 3}[name]))
        # neighbourhoods cut by the slice's edge, and holding NaN and +-inf
        at = [(0, 0), (0, NX - 1), (NY - 1, 0), (NY - 1, NX - 1), (0, 20), (22, 0), (18, 18), (10, 30)]
        F = _lows(sense, at, [10, 11, 12, 13, 14, 15, 16, 17])
        F[18, 19], F[17, 18], F[19, 17] = np.nan, np.inf, -np.inf
        F[10, 30] = -np.inf if sense == MIN else np.inf      # an infinity is no seed
        _seed("seeds-edge", f"seeds-edge-{word}", F, sense, ej=2, ei=2, plants=at, expect={})
        # plateaus: 2 x 3 points of one value; the first point admissible, and not
        F = _lows(sense, [(15 + dj, 20 + di) for dj in range(2) for di in range(3)] + [(30, 30)], [4] * 6 + [9])
        for name, b in (("admissible", FULL), ("first-row-out", (16, NY - 1, 0, NX - 1)), ("first-column-out", (0, NY - 1, 21, NX - 1))):
            _seed("seeds-plateau", f"seeds-plateau-{name}-{word}", F, sense, bounds=b, plants=[(15, 20)], expect=dict(seeded=name == "admissible"))
        # r = 1: corner S (means of 4) enter the neighbourhoods of the corner centres
        _seed("seeds-smooth", f"seeds-r1-{word}", _background(1300 + sense), sense, r=1, ej=2, ei=2, expect={})
        _seed("seeds-smooth", f"seeds-r1-inner-{word}", _background(1310 + sense), sense, r=1, ej=2, ei=3, bounds=CLIP_BOUNDS, expect={})
        # the ring: lows on either side of the seam (equal: the absolute index decides), r = 0 and r = 1
        shape = (RING_NY, RING_NX)
        at = [(5, 0), (5, RING_NX - 1), (9, RING_NX - 1), (9, 0), (12, 12), (3, 6)]
        _seed("seeds-ring", f"seeds-ring-seam-{word}", _lows(sense, at, [6, 6, 4, 8, 6, 6], shape), sense, bounds=RING_BOUNDS, ring=True, plants=at, expect={})
        _seed("seeds-ring", f"seeds-ring-wide-{word}", _lows(sense, at, [6, 6, 4, 8, 6, 6], shape), sense, ej=2, ei=12, bounds=RING_BOUNDS, ring=True,
              plants=at, expect={})
        _seed("seeds-ring", f"seeds-ring-r1-{word}", _background(1320 + sense, shape), sense, r=1, ej=1, ei=2, bounds=RING_BOUNDS, ring=True, expect={})


_partition_cases()
_tie_cases()
_clip_cases()
_missing_cases()
_ring_cases()
_seed_cases()


def case(cid):
    return _CASES[cid]


def all_chain_ids():
    return [c for ids in CHAIN_FAMILIES.values() for c in ids]


def all_seed_ids():
    return [c for ids in SEED_FAMILIES.values() for c in ids]


@functools.lru_cache(maxsize=None)
def reference(cid, ring=None):
    """The restatement's answer, computed once and never written to.  ``ring``: for a chain case, the ring rule instead of the case's own
    (the tie cases run through lec_follow_spans_chunk_ring too)."""
    c = _CASES[cid]
    if c["family"].startswith("seeds"):
        return seeds(c["F"], c["sense"], c["r"], c["ej"], c["ei"], c["k_max"], c["threshold"], c["bounds"], c["ring"])
    return chain(c["F"], c["sense"], c["r"], c["sj"], c["si"], c["bounds"], c["start"], c["ring"] if ring is None else ring)


def diag_inputs(cid):
    """lec_track_diag's view of an r = 0 hgt case: boxes [nt][6] equal to the chain's windows, and the field with +-inf made NaN --
    lec_track_diag's rule skips NaN only, lec_follow's everything that is not finite."""
    c, ref = _CASES[cid], reference(cid)
    assert c["r"] == 0 and c["field"] == "hgt" and not c["ring"]
    boxes = [(ln["window"][2], ln["window"][3], ln["window"][0], ln["window"][1], ln["window"][0], ln["window"][2]) for ln in ref["windows"]]
    return np.array(boxes, dtype=np.int32), np.where(np.isfinite(c["F"]), c["F"], np.nan)


# the capped grid of the series kernels -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def capped_patterns():
    """Five distinct 64 x 64 integer slices: a ramp with a few lows of partly equal values, moved from pattern to pattern."""
    ny, nx = CAPPED["ny"], CAPPED["nx"]
    out = []
    for p in range(CAPPED["patterns"]):
        at = [((7 + 11 * q + 5 * p) % ny, (3 + 17 * q + 9 * p) % nx) for q in range(6)]
        out.append(_lows(MIN, at, [4, 9, 4, 6, 9, 2], (ny, nx)))
    return np.stack(out)


def capped_steps():
    """The steps checked against the restatement: the first, the last, and those on either side of series point 2^24."""
    plane = CAPPED["ny"] * CAPPED["nx"]
    edge = (1 << 24) // plane
    return sorted({0, edge - 1, edge, CAPPED["nt"] - 1})
