"""Input planes for the sorted-tile walks of etopo1_ice (k_et_tiles) and make_topoO (k_to_tiles<false> / <true>), a named case per
tile, with a table of what every tile is meant to reach: the land count, the padded sort size, where the walk stops and how.  The
builders need no GPU and no library: the areas are make_topoo_restatement.make_dxyp's, plain Python.  Whether a case reaches what
its name says is decided by the restatements alone (tests/test_tile_walk_cases.py); tests/test_gpu_tile_walks.py then compares the
kernels with the restatements on these planes, bit for bit.

Within a case tile every land cell has its own elevation (a seeded choice of distinct int16 values, both extremes in some tiles),
unless the case is about ties: so the sorted order and the index where a walk stops are visible in the output."""
import functools
import math
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_topoo_restatement as mr  # noqa: E402

Grid = namedtuple("Grid", "im jm")      # what the restatements read of an HntrSpec


def pow2(n):
    n2 = 1
    while n2 < n:
        n2 <<= 1
    return n2


def distinct(rng, n, extremes=False):
    """n distinct int16 values in random order; with `extremes` (n >= 2) -32768 and 32767 are among them"""
    if extremes and n >= 2:
        v = rng.choice(np.arange(-32767, 32767), n - 2, replace=False)
        v = np.concatenate([v, [-32768, 32767]])
        return rng.permutation(v).astype(np.int16)
    return rng.choice(np.arange(-32767, 32767), n, replace=False).astype(np.int16)


# ================================================================================================================================
# A. etopo1_ice: k_et_tiles
# ================================================================================================================================
# name -> (coarse, fine).  walk: tiles of 20 x 20 = 400 cells (n2 up to 512: six full 64-cell steps and one of 16), coarse rows 4..6
# lie south of the 78N band row 160 * 14 // 15 = 149; 48 columns give the 144 tiles the cases need.  limit: tiles of exactly MAX_TILE
# = 8192 cells (128 x 64), coarse row 2 south of the band row 238.
ET_GEOM = {"walk": ((48, 8), (960, 160)), "limit": ((4, 4), (512, 256))}
ET_STOPS = (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192)         # and n - 2, n - 1
ET_SORT_N = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 399, 400)
ET_LIMIT_N = (4096, 4097, 8191, 8192)
ET_OUTCOMES = ("quarter", "three_quarters", "exact")        # of cell k's area left: not rounded in; rounded in; `<=` holds

EtCase = namedtuple("EtCase", "name j1 i1 n n2 k outcome taken")


def et_grids(name):
    c, f = ET_GEOM[name]
    return Grid(*f), Grid(*c)


def et_trace(areas, remain):
    """The walk of etopo1_ice.cpp:190-207 over areas in sorted order: (cells taken, index of the first cell that fails
    `area <= remain` or None, whether that cell was rounded in)."""
    for k, a in enumerate(areas):
        if a <= remain:
            remain -= a
        else:
            r = remain >= a * .5
            return k + (1 if r else 0), k, r
    return len(areas), None, False


def et_walk_order(fo_t, zt_t):
    """the tile's land cells as traversal positions, in the reference's order (-elev, j, i)"""
    pos = np.flatnonzero(fo_t.reshape(-1) == 0)
    z = zt_t.reshape(-1)[pos].astype(np.int64)
    return pos[np.lexsort((pos, -z))]


def et_fraction(areas, k, outcome, dC):
    """The coarse fraction that makes the walk over `areas` fail first at sorted cell k with `outcome` (the way
    test_gpu_etopo1_ice's first_cell_fraction does: the areas before k summed in walk order, plus the share, over dxypC).  For
    "exact" the fraction is moved up ulp by ulp until `<=` holds at cell k (the division and the product by dxypC both round)."""
    s = 0.
    for a in areas[:k]:
        s += a
    share = {"quarter": .25, "three_quarters": .75, "exact": 1.}[outcome]
    f = (s + share * areas[k]) / dC
    if outcome == "exact":
        for _ in range(64):
            stop = et_trace(areas, f * dC)[1]
            if stop is None or stop > k:
                break
            f = math.nextafter(f, math.inf)
    return f


def _et_specs():
    """(name, n, what, k, outcome, extremes) for the walk geometry, one per tile"""
    specs = []
    for q, n in enumerate(ET_SORT_N):           # sort sizes: stopped at n // 2 without rounding
        specs.append(("sort n=%d" % n, n, "stop", n // 2, "quarter", q % 3 == 0))
    for n in (400, 128, 129):                   # stop positions
        for k in sorted({k for k in ET_STOPS if k < n} | {n - 2, n - 1}):
            for oc in ET_OUTCOMES:
                specs.append(("stop n=%d k=%d %s" % (n, k, oc), n, "stop", k, oc, k % 2 == 1))
    for n in (64, 128):                         # the loop ends on a step boundary with the prefetch reaching past n
        specs.append(("never stops n=%d" % n, n, "never", None, None, False))
    specs.append(("ties: one elevation", 400, "tie_one", 190, "quarter", False))
    specs.append(("ties: two elevations alternating", 400, "tie_two", 250, "quarter", False))
    specs.append(("ties: stop between equal cells of two rows", 400, "tie_pair", 100, "quarter", False))
    return specs


def _et_background(I, Cg, rng):
    """random planes in the manner of test_gpu_etopo1_ice.make_planes, with Greenland (2) in the south half only"""
    shape = (I.jm, I.im)
    fo = rng.integers(0, 4, shape).astype(np.int16)
    north = fo[I.jm // 2:]
    north[north == 2] = 3
    zt = (rng.integers(-3, 4, shape) * 100).astype(np.int16)
    zt[rng.random(shape) < 0.03] = -32768
    zt[rng.random(shape) < 0.03] = 32767
    zs = np.clip(zt.astype(np.int64) - rng.integers(0, 100, shape), -32768, 32767).astype(np.int16)
    fC = np.where(rng.random((Cg.jm, Cg.im)) < 1 / 3, 0., rng.random((Cg.jm, Cg.im)) * 1.2)
    return fo, zt, zs, fC


def _et_fill_tile(rng, fo_t, zt_t, n, what, extremes):
    """n land cells at seeded positions, the rest ocean (1 or 3); the elevations by `what`"""
    ncell = fo_t.size
    pos = np.sort(rng.choice(ncell, n, replace=False)) if n < ncell else np.arange(ncell)
    f = rng.choice(np.array([1, 3], np.int16), ncell)
    f[pos] = 0
    fo_t[:] = f.reshape(fo_t.shape)
    z = zt_t.reshape(-1).copy()
    if what == "tie_one":
        z[pos] = 777
    elif what == "tie_two":
        z[pos] = np.where(np.arange(n) % 2 == 0, 500, -500)
    else:
        z[pos] = distinct(rng, n, extremes)
    zt_t[:] = z.reshape(zt_t.shape)


@functools.lru_cache(maxsize=None)
def et_cases(name):
    """((focean, zictop, zsolid, fgiceC), table of EtCase) of geometry `name`; all read-only"""
    I, Cg = et_grids(name)
    mi, mj = I.im // Cg.im, I.jm // Cg.jm
    rng = np.random.default_rng(sum(map(ord, "et" + name)))
    fo, zt, zs, fC = _et_background(I, Cg, rng)
    dI, dC = mr.make_dxyp(I.im, I.jm), mr.make_dxyp(Cg.im, Cg.jm)
    jband = I.jm * 14 // 15
    rows = [j1 for j1 in range(Cg.jm // 2, Cg.jm) if (j1 + 1) * mj <= jband]
    tiles = [(j1, i1) for j1 in rows for i1 in range(Cg.im)]
    if name == "walk":
        specs = _et_specs()
    else:
        specs = [("limit n=%d" % n, n, "stop", n // 2, "quarter", n == 8192) for n in ET_LIMIT_N]
    assert len(specs) <= len(tiles), (len(specs), len(tiles))
    table = []
    for (label, n, what, k, oc, extremes), (j1, i1) in zip(specs, tiles):
        sl = (slice(j1 * mj, (j1 + 1) * mj), slice(i1 * mi, (i1 + 1) * mi))
        _et_fill_tile(rng, fo[sl], zt[sl], n, what, extremes)
        order = et_walk_order(fo[sl], zt[sl])
        if what == "tie_pair":          # sorted cells k - 1 and k get one elevation; they sit in different rows
            a, b = sorted((int(order[k - 1]), int(order[k])))
            assert a // mi != b // mi
            t = zt[sl].reshape(-1).copy()
            t[b] = t[a] = max(t[a], t[b])
            zt[sl] = t.reshape(mj, mi)
            order = et_walk_order(fo[sl], zt[sl])
            assert [int(order[k - 1]), int(order[k])] == [a, b]
        areas = [dI[j1 * mj + int(c) // mi] for c in order]
        if what == "never":
            fC[j1, i1], taken = 1.5, n
        else:
            fC[j1, i1] = et_fraction(areas, k, oc, dC[j1])
            taken = et_trace(areas, fC[j1, i1] * dC[j1])[0]
        table.append(EtCase(label, j1, i1, n, pow2(n), k, oc, taken))
    for a in (fo, zt, zs, fC):
        a.setflags(write=False)
    return (fo, zt, zs, fC), tuple(table)


def et_case_at(name, j, i):
    """the case whose tile holds fine cell (j, i), or None: for the message of a mismatch"""
    I, Cg = et_grids(name)
    mi, mj = I.im // Cg.im, I.jm // Cg.jm
    for c in et_cases(name)[1]:
        if (c.j1, c.i1) == (j // mj, i // mi):
            return c
    return None


# ================================================================================================================================
# B, C. make_topoO: k_to_tiles<false> (short) and k_to_tiles<true> (long)
# ================================================================================================================================
# name -> (ocean, fine); FLAKES is given on the ocean grid itself, so a requested p / 256 arrives at std::round as it is.
# short: tiles of 64 x 4 = 256 cells, pole tiles of 3072: the LDS sort everywhere.  long: tiles of MAX_TILE + 1 = 8193 cells
# (2731 x 3) on the narrowest ocean grid the library takes, so every interior tile and both pole tiles take the counting sort.
TO_GEOM = {"short": ((12, 12), (768, 48)), "long": ((2, 12), (5462, 36))}
TO_MAX_TILE = 8192

# a land case: ocean cell (I, J) 1-based; n land cells; p: FLAKES = p / 256; ice: ice cells; walk: the (NLAKE, NGRND) the case is
# steered onto (None: only n is pinned); tags: what the coverage test counts
ToCase = namedtuple("ToCase", "name I J n p ice walk tags")
ToOcean = namedtuple("ToOcean", "name I J ncell lowest_at")


def to_grids(name):
    o, f = TO_GEOM[name]
    return Grid(*f), Grid(*o)


def to_tile_slices(I, O, Ic, J):
    """the fine cells of ocean cell (Ic, J), 1-based; a pole row's tile is the whole row (IMAX = 1)"""
    mi, mj = I.im // O.im, I.jm // O.jm
    if J in (1, O.jm):
        return slice((J - 1) * mj, J * mj), slice(0, I.im)
    return slice((J - 1) * mj, J * mj), slice((Ic - 1) * mi, Ic * mi)


def regrid_nested(I, O, wta, a):
    """Hntr's regrid (mean_polar) where the fine grid nests in the coarse one: per tile sum(w * area * a) / sum(w * area), 0 where
    no weight, the pole rows one mean over the whole row.  This is the regrid's value, not its bits: the cases below are chosen
    with room to spare, and the CPU test shows that by moving FGICE."""
    d = np.asarray(mr.make_dxyp(I.im, I.jm))[:, None]
    w = np.broadcast_to(np.asarray(wta, np.float64), (I.jm, I.im)) * d
    wa = w * np.asarray(a, np.float64)
    mi, mj = I.im // O.im, I.jm // O.jm
    W = w.reshape(O.jm, mj, O.im, mi).sum(axis=(1, 3))
    V = wa.reshape(O.jm, mj, O.im, mi).sum(axis=(1, 3))
    for r in (0, O.jm - 1):
        W[r], V[r] = W[r].sum(), V[r].sum()
    with np.errstate(all="ignore"):
        return np.where(W != 0, V / np.where(W != 0, W, 1.), 0.)


def to_six(I, O, planes):
    """the six regridded planes of make_topoO's step 1 for the planes (fg, zt, zs, fo, flakes), by regrid_nested"""
    fg, zt, zs, fo, fl = planes
    return [regrid_nested(I, O, 1., fo), regrid_nested(I, O, 1., fg), np.array(fl, np.float64), regrid_nested(I, O, fo, zs),
            regrid_nested(I, O, fg, zt), regrid_nested(I, O, fg, zs)]


def to_fractions(p, land_area, ice_area, tile_area):
    """(FLAKE, FGRND, how far p / fcontf lies from a half: the room std::round has) of a continental cell as topo_base.cpp:506-641
    gives them, from the requested p / 256 and the areas"""
    fcontf = land_area / tile_area
    FLAKE = mr.std_round(p / 256. * 1. / (fcontf + 1e-20) * 256.) / 256.
    FGICE = min(max((ice_area / tile_area) * (1. / fcontf), 0.), 1.)
    if FLAKE + FGICE > 1:
        FLAKE = 1. - FGICE
    FGRND = 1. - FLAKE - FGICE
    v = p / fcontf
    return FLAKE, (0. if abs(FGRND) < 1e-14 else FGRND), abs(v - math.floor(v) - .5)


def to_predict(depth, area, FLAKE, FGRND):
    """(NLAKE, NGRND, margin) of callZ's two walks (:164-172, :192-203) over the land cells in traversal order; margin: how far, in
    mean cells, the nearest partial sum lies from the threshold it is compared with where a walk ends"""
    n = len(depth)
    order = np.argsort(depth, kind="stable")
    cs = np.cumsum(np.asarray(area)[order])
    SAREA = float(np.cumsum(area)[-1])
    mean = SAREA / n
    out, margin, start = [], math.inf, 0
    for thr in (SAREA * FLAKE, SAREA * (FLAKE + FGRND)):
        over = np.flatnonzero(cs[start:] > thr)
        k = start + int(over[0]) if over.size else n - 1
        if k > start:
            margin = min(margin, (thr - cs[k - 1]) / mean)
        if over.size and k < n - 1:     # (on the last cell the walk ends there whether the sum exceeds or not)
            margin = min(margin, (cs[k] - thr) / mean)
        out.append(k)
        start = k
    return out[0], out[1], margin


def to_walk_detail(depth, area, FLAKE, FGRND):
    """callZ's two walks over the land cells (traversal order) in the restatement's own arithmetic, with how each ended:
    (NLAKE, NGRND, the lake walk ended by the clamp of :165-168, the ground walk ended by exceeding its threshold)"""
    n = len(depth)
    SAREA = 0.
    for a in area:
        SAREA += a
    cells = [(float(area[k]), float(depth[k])) for k in sorted(range(n), key=lambda k: depth[k])]
    ANSUM, NLAKE, clamped = 0., 0, False
    while True:
        if NLAKE == n:
            NLAKE, clamped = NLAKE - 1, True
            break
        ANSUM += cells[NLAKE][0]
        if ANSUM > SAREA * FLAKE:
            break
        NLAKE += 1
    ANSUM -= cells[NLAKE][0]
    NGRND, exceeded = NLAKE, True
    while True:
        if NGRND == n:
            NGRND, exceeded = NGRND - 1, False
            break
        ANSUM += cells[NGRND][0]
        if ANSUM > SAREA * (FLAKE + FGRND):
            break
        NGRND += 1
    return NLAKE, NGRND, clamped, exceeded


def _to_fill_tile(rng, sl, P, n, ice, depths="distinct", extremes=False):
    """One tile: n land cells (FOCEAN1m 0) at seeded positions, the rest ocean; `ice` of the land cells carry FGICE1m = 1 with
    ZSOLG1m 10 m below ZICETOP1m (never a cell within 10 m of -32768, so the difference cannot wrap)."""
    fg, zt, zs, fo = P
    shape = fo[sl].shape
    ncell = shape[0] * shape[1]
    pos = np.sort(rng.choice(ncell, n, replace=False)) if n < ncell else np.arange(ncell)
    f = np.ones(ncell, np.int16)
    f[pos] = 0
    z = rng.integers(-3000, 3000, ncell).astype(np.int16)       # the ocean cells' depths: any
    if depths == "distinct":
        z[pos] = distinct(rng, n, extremes)
    elif depths == "one":
        z[pos] = -123
    elif depths == "two":
        z[pos] = np.where(np.arange(n) % 2 == 0, 250, -250)
    elif depths == "last_chunk":        # the tile's last cell, alone in its chunk of 256, holds the only copy of the lowest depth
        assert n == ncell
        v = distinct(rng, n, False)
        v[-1] = -32768
        z[pos] = v
    elif depths == "every_chunk":       # one depth once in every chunk of 256, at a varying place
        assert n == ncell
        v = distinct(rng, n, False)
        v[v == 4242] = -32768               # (distinct() without extremes never gives -32768)
        for c0 in range(0, ncell, 256):
            v[c0 + (c0 // 256 * 37) % min(256, ncell - c0)] = 4242
        z[pos] = v
    else:
        raise ValueError(depths)
    g = np.zeros(ncell, np.int16)
    if ice:
        cand = pos[z[pos] >= -32758]
        g[rng.choice(cand, ice, replace=False)] = 1
    s = z.copy()
    s[g == 1] -= 10
    fo[sl], zt[sl], fg[sl], zs[sl] = f.reshape(shape), z.reshape(shape), g.reshape(shape), s.reshape(shape)


def _to_tile_walk(I, sl, P, p, flag=None):
    """what to_predict says of the tile as it stands: (NLAKE, NGRND, margin, flag holds)"""
    fg, zt, zs, fo = P
    d = np.asarray(mr.make_dxyp(I.im, I.jm))[sl[0]]
    area = np.repeat(d, fo[sl].shape[1])
    land = fo[sl].reshape(-1) == 0
    ice = land & (fg[sl].reshape(-1) != 0)
    FLAKE, FGRND, room = to_fractions(p, float(area[land].sum()), float(area[ice].sum()), float(area.sum()))
    depth = zt[sl].reshape(-1)[land].astype(np.float64)
    a, b, margin = to_predict(depth, area[land], FLAKE, FGRND)
    if p and not land.all():
        margin = min(margin, room)
    ok = True
    if flag:        # (exact: these cases have no ice or a whole cell to spare, and FLAKE = p / 256 as it is)
        _, _, clamped, exceeded = to_walk_detail(depth.tolist(), area[land].tolist(), FLAKE, FGRND)
        ok = {"clamp": clamped, "ground_last_exceeded": exceeded, "ground_never": not exceeded}[flag]
    return a, b, margin, ok


def _to_steer(rng, I, sl, P, n, want, p0, ice0, flag=None, **kw):
    """Fill the tile, over seeds and the neighbours of (p0, ice0), until the predicted walks are `want` = (NLAKE, NGRND) (None: any)
    with at least a twentieth of a cell to spare; returns (p, ice)."""
    for attempt in range(400):
        for p in ([p0 + attempt % 5 if p0 else 0] if want is None else [p0, p0 - 1, p0 + 1]):
            for ice in ([ice0] if want is None else [ice0, ice0 - 1, ice0 + 1, ice0 - 2, ice0 + 2]):
                if not (0 <= p <= 256 and 0 <= ice <= max(n - 1, 0)):
                    continue
                state = rng.bit_generator.state
                _to_fill_tile(rng, sl, P, n, ice, **kw)
                a, b, margin, ok = _to_tile_walk(I, sl, P, p, flag)
                if ok and margin >= .05 and (want is None or (a, b) == want):
                    return p, ice
                if want is not None:
                    rng.bit_generator.state = state     # the same cells for the next (p, ice); a new seed only in the outer loop
        rng.random()
    raise AssertionError("no tile found for %r from (%d, %d)" % (want, p0, ice0))


# short geometry: (NLAKE, NGRND) targets on all-land tiles of 256 distinct depths, with the tags the coverage test looks for
_SHORT_WALKS = [(0, 63), (62, 64), (63, 63), (63, 64), (64, 64), (64, 65), (65, 128), (127, 128), (128, 128), (128, 129), (127, 191),
                (128, 192), (0, 0), (62, 127), (65, 193)]
_SHORT_N = (1, 2, 63, 64, 65, 128, 129, 255)        # land counts below the tile, forced to land by SET_TO (256: every case above)
_OCEAN_AT = (0, 63, 64, 255)                        # the lowest ocean fine cell's traversal position; the north pole tile: its last


@functools.lru_cache(maxsize=None)
def to_cases(name):
    """((FGICE1m, ZICETOP1m, ZSOLG1m, FOCEAN1m, FLAKES), set_to_land, table of ToCase, table of ToOcean) of geometry `name`"""
    I, O = to_grids(name)
    rng = np.random.default_rng(sum(map(ord, "to" + name)))
    shape = (I.jm, I.im)
    P = tuple(np.zeros(shape, np.int16) for _ in range(4))      # fg, zt, zs, fo
    fl = np.zeros((O.jm, O.im))
    mi, mj = I.im // O.im, I.jm // O.jm
    ncell = mi * mj
    # every tile first: all land, distinct depths, some ice, some lake; the pole tiles too (the south pole row is continental by
    # :498-502 with FGICE = 1, so it needs ice for dZGICE not to come from pow)
    for J in range(1, O.jm + 1):
        for Ic in range(1, (1 if J in (1, O.jm) else O.im) + 1):
            sl = to_tile_slices(I, O, Ic, J)
            nc = P[0][sl].size
            _to_fill_tile(rng, sl, P, nc, int(rng.integers(1, nc // 2)), extremes=(Ic + J) % 3 == 0 and nc < 65536)
            fl[J - 1, Ic - 1] = int(rng.integers(0, 200)) / 256.
    # the case tiles: J = 3..8, whose 2 x 2 blocks lie in J = 3..8 too and hold no ocean cell, outside FLAKE's zero bands
    free = [(Ic, J) for J in range(3, 9) for Ic in range(1, O.im + 1)]
    land, table, oceans = [], [], []

    def add(label, n, want, p0, ice0, tags, **kw):
        Ic, J = free.pop(0)
        sl = to_tile_slices(I, O, Ic, J)
        flag = tags[0] if tags[0] in ("clamp", "ground_last_exceeded", "ground_never") else None
        p, ice = _to_steer(rng, I, sl, P, n, want, p0, ice0, flag=flag, **kw)
        fl[J - 1, Ic - 1] = p / 256.
        if n < ncell:
            land.append((Ic, J))
        table.append(ToCase(label, Ic, J, n, p, ice, want, tuple(tags)))

    if name == "short":
        for q, (a, b) in enumerate(_SHORT_WALKS):
            add("walk NLAKE=%d NGRND=%d" % (a, b), 256, (a, b), a, max(0, 256 - b - 1), ["steered"], extremes=q % 2 == 0 and b > 0)
        add("lake to the last cell by the clamp", 256, (255, 255), 256, 0, ["clamp"])
        add("ground exceeded on the last cell", 256, (64, 255), 64, 1, ["ground_last_exceeded"])
        add("ground never exceeded", 256, (64, 255), 64, 0, ["ground_never"])
        for n in _SHORT_N:
            add("n=%d" % n, n, None, 0 if n < 63 else 40, n // 3, ["n"], extremes=n >= 2)
        add("all one depth", 256, None, 100, 60, ["ties"], depths="one")
        add("two depths alternating", 256, None, 100, 60, ["ties"], depths="two")
        # ocean cells: one 2 x 2 block of their own (its lakes go to the ground, no case is beside them), and the north pole tile
        block = [(11, 9), (12, 9), (11, 10), (12, 10)]
        fg, zt, zs, fo = P
        for (Ic, J), at in list(zip(block, _OCEAN_AT)) + [((1, O.jm), None)]:
            sl = to_tile_slices(I, O, Ic, J)
            nc = fo[sl].size
            at = nc - 1 if at is None else at
            f = np.ones(nc, np.int16)
            landpos = rng.choice(np.setdiff1d(np.arange(nc), [at]), nc // 5, replace=False)
            f[landpos] = 0
            z = distinct(rng, nc, False)
            z[z < -20000] += 15000                  # the ocean cells stay above -20000 ...
            z[at] = -30000                          # ... but for the one that is the lowest
            z[landpos[:3]] = [-32768, -31000, -30001]       # land below it, which :80 must not take
            g = np.zeros(nc, np.int16)
            g[landpos[3::2]] = 1
            s = z.copy()
            s[g == 1] -= 10
            shp = fo[sl].shape
            fo[sl], zt[sl], fg[sl], zs[sl] = f.reshape(shp), z.reshape(shp), g.reshape(shp), s.reshape(shp)
            oceans.append(ToOcean("ocean, lowest ocean cell at %d of %d" % (at, nc), Ic, J, nc, at))
    else:
        # NLAKE ~ 32.004 p on 8193 nearly equal cells: p = 32, 64, 96 land beside multiples of 64, the seed does the rest
        for a, b, p0 in ((1023, 4096, 32), (2048, 4097, 64), (3073, 6143, 96)):
            add("permutation NLAKE=%d NGRND=%d" % (a, b), ncell, (a, b), p0, ncell - b - 1, ["steered", "full"], extremes=True)
        add("all one depth", ncell, None, 100, 2000, ["ties", "one"], depths="one")
        add("two depths alternating", ncell, None, 100, 2000, ["ties", "two"], depths="two")
        add("a depth in the last chunk only", ncell, None, 50, 1000, ["last_chunk"], depths="last_chunk")
        add("a depth once in every chunk", ncell, None, 50, 1000, ["every_chunk"], depths="every_chunk")
        add("n=8000 of 8193", 8000, None, 40, 3000, ["n"], extremes=True)
        add("n=257 of 8193", 257, None, 0, 64, ["n"], extremes=True)
        # the north pole tile (scratch placed after the interior tiles'): FLAKE is 0 there, the ground walk ends on a multiple of 64
        sl = to_tile_slices(I, O, 1, O.jm)
        nc = P[0][sl].size
        _to_steer(rng, I, sl, P, nc, (0, 8192), 0, nc - 8193)
        fl[O.jm - 1, :] = 0.
        table.append(ToCase("north pole NGRND=8192", 1, O.jm, nc, 0, None, (0, 8192), ("pole", "steered")))
    planes = (P[0], P[1], P[2], P[3], fl)
    for a in planes:
        a.setflags(write=False)
    return planes, tuple(land), tuple(table), tuple(oceans)


def to_case_at(name, Ic, J):
    """the case of ocean cell (Ic, J), 1-based, or None"""
    _, _, table, oceans = to_cases(name)
    for c in table + oceans:
        if c.J == J and (c.I == Ic or J in (1, to_grids(name)[1].jm)):
            return c
    return None


def to_walks(name, six):
    """Every land case's (_walk, the dict callZ_cell returns) from the restatement, fed the six regridded planes `six`:
    {(I, J): (walk, o, FLAKE, FGRND)}.  Valid because a case tile's 2 x 2 block holds no ocean cell: the FLAKE and FGRND planes
    are then what callZ was called with."""
    I, O = to_grids(name)
    p, land, table, _ = to_cases(name)
    planes, counts, pow_cells = mr.make_topoO(I.im, I.jm, O.im, O.jm, p[0], p[1], p[2], p[3], *six, set_to_land=land)
    d = mr.make_dxyp(I.im, I.jm)
    out = {}
    for c in table:
        sl = to_tile_slices(I, O, c.I, c.J)
        FLAKE, FGRND = float(planes["FLAKE"][c.J - 1, c.I - 1]), float(planes["FGRND"][c.J - 1, c.I - 1])
        o = mr.callZ_cell(p[0][sl].tolist(), p[3][sl].tolist(), p[1][sl].tolist(), d[sl[0]], False, FLAKE, FGRND)
        out[(c.I, c.J)] = (o["_walk"], o, FLAKE, FGRND)
    return out, planes, counts, pow_cells
