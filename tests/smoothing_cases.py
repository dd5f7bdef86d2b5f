"""Which device form a smoothed build must take, decided on the CPU from the oracle's matrices: a numpy transcription of the bin
arithmetic (icebin_amd/csrc/smooth_plan.h smooth_grid, smooth.hip smooth_bin / k_smt_bincols) gives the quantities the forms' limits
are about, so that a test first asserts that its input lies on the intended side of a limit and only then which form ran
(linear_Weighted.smoothed_by): an input that drifts fails loudly instead of testing another form.

Below the grid legs: scene builders that put the forms' bin, wave and table limits where a leg wants them (one-bin clusters, a lattice
with pairs at the cut, a pair across two bins of two sigmas, degenerate bin grids, cells without area), the facts about them (members
per bin, neighbours per row, pairs at the cut), a long-double reference of the smoother's definition and the entry bound derived for
it.  CPU and numpy only."""
import functools

import numpy as np

from icebin_amd import synthetic as syn
from oracle import oracle as orc

NONE, TRIPLET, DIRECT, TILE = 0, 1, 2, 3        # SmoothForm, as ibh_weighted_smoothed_by reports it
SMT_KMAX, SMT_ROWMAX, SMD_MAXCOL = 128, 8, 128  # the limits (smooth_plan.h)
MAX_BINS = 4096
SMD_HITS = 1024
BIN_MARGIN = 1e-9                               # SMOOTH_BIN_MARGIN: how much wider than two sigmas a bin is


def _bin_axis(extent, sig):
    w = max(2.0 * sig, extent / float(MAX_BINS)) * (1.0 + BIN_MARGIN)
    return w, int(min(float(MAX_BINS), np.floor(extent / w) + 1.0))


def smooth_grid(cmin, cmax, sigma):
    """(x0, y0, bw, bh, nbx, nby): bins a margin wider than two sigmas over the centroids' bounding box, at most MAX_BINS per axis"""
    bw, nbx = _bin_axis(cmax[0] - cmin[0], sigma[0])
    bh, nby = _bin_axis(cmax[1] - cmin[1], sigma[1])
    return cmin[0], cmin[1], bw, bh, nbx, nby


def neighbourhood_facts(g, em, plain, sigma):
    """plain: the oracle's UNSMOOTHED I-row matrix.  Returns (the most distinct columns the rows of any non-empty bin's 3 x 3
    neighbourhood hold -- the tile form's column table, limit SMT_KMAX --, the longest row of `plain` -- limit SMT_ROWMAX)."""
    cen = np.asarray(g["I_centroid_xy"], np.float64).reshape(-1, 2)
    x0, y0, bw, bh, nbx, nby = smooth_grid(cen.min(axis=0), cen.max(axis=0), sigma)
    s = np.asarray(plain.dims[0], np.int64)                 # dense row -> ice cell
    live = ~np.isnan(np.asarray(em, np.float64)[s])         # masked cells are no tuples
    bx = np.clip(((cen[s, 0] - x0) / bw).astype(np.int64), 0, nbx - 1)      # (C's cast truncates; the operands are >= 0)
    by = np.clip(((cen[s, 1] - y0) / bh).astype(np.int64), 0, nby - 1)
    rowbin = by * nbx + bx
    cols = [set() for _ in range(nbx * nby)]                # the distinct columns of each bin's member rows
    occupied = np.zeros(nbx * nby, bool)
    occupied[rowbin[live]] = True
    keep = live[plain.row]
    for b, c in np.unique(np.stack([rowbin[plain.row[keep]], plain.col[keep].astype(np.int64)], axis=1), axis=0):
        cols[b].add(int(c))
    widest = 0
    for b in np.nonzero(occupied)[0]:
        x, y = b % nbx, b // nbx
        around = set()
        for yy in range(max(y - 1, 0), min(y + 1, nby - 1) + 1):
            for xx in range(max(x - 1, 0), min(x + 1, nbx - 1) + 1):
                around |= cols[yy * nbx + xx]
        widest = max(widest, len(around))
    longest = int(np.bincount(plain.row, minlength=plain.nrow).max()) if plain.nnz else 0
    return widest, longest


@functools.lru_cache(maxsize=None)
def grids(config):
    g = syn.make_grids(config)
    return g, syn.dome_elevmask(g)


@functools.lru_cache(maxsize=None)
def oracle_case(config, name, sigma, scale=True, correctA=True):
    """(the oracle's unsmoothed matrix, its smoothed one, columns around the widest bin, longest unsmoothed row, longest smoothed row):
    computed once, shared by the tests, never modified"""
    g, em = grids(config)
    rg = orc.Regridder(g)
    plain = rg.matrix_d(name, em, scale=scale, correctA=correctA)
    smoothed = rg.matrix_d(name, em, scale=scale, correctA=correctA, sigma=sigma)
    widest, longest = neighbourhood_facts(g, em, plain, sigma)
    return plain, smoothed, widest, longest, int(np.bincount(smoothed.row, minlength=smoothed.nrow).max())


def form_served(tile_tried, direct_tried, widest, longest, longest_smoothed):
    """the first form tried whose tables hold the input"""
    tile_fits = widest <= SMT_KMAX and longest <= SMT_ROWMAX
    direct_fits = longest_smoothed <= SMD_MAXCOL
    return TILE if tile_tried and tile_fits else DIRECT if direct_tried and direct_fits else TRIPLET


def assert_input_side(form, tile_tried, direct_tried, widest, longest, longest_smoothed):
    """the input lies where the knobs (which forms are tried) make `form` the one that builds the matrix"""
    want = form_served(tile_tried, direct_tried, widest, longest, longest_smoothed)
    assert want == form, ("the input left the side of the limits this leg is about", dict(
        form=form, tile_tried=tile_tried, direct_tried=direct_tried, widest=widest, longest=longest, longest_smoothed=longest_smoothed))


# The small legs (50 km: 793 unmasked rows, unsmoothed rows of at most 8 entries, so only the column limits are in play):
# (sigma, matrix, (smooth_direct, smooth_tile), the form that must build it, the knobs whose build it must equal bitwise or None)
G50_LEGS = (
    ((60e3, 60e3, 250.0), "IvE", (0, 1), TILE, None),           # 125 columns around the widest bin: at the edge of SMT_KMAX; raised LDS
    ((60e3, 60e3, 250.0), "IvA", (0, 1), TILE, None),           # 18
    ((120e3, 120e3, 400.0), "IvE", (1, 1), DIRECT, (1, 0)),     # 365 around a bin, rows of <= 92: the tiles overflow, the direct form serves
    ((200e3, 200e3, 1500.0), "IvE", (1, 1), TRIPLET, (0, 0)),   # 665, rows of up to 315: both overflow
    ((200e3, 200e3, 1500.0), "IvA", (1, 1), TILE, None),        # 85
)


# ---- scenes that put the forms' bin, wave and table limits where a test wants them (tests/test_smoothing_cases.py asserts on the CPU
# that they do, tests/test_gpu_smoothing.py builds them on the device) ---------------------------------------------------------------
SIGMA_C = (60e3, 45e3, 250.0)                   # sx != sy: the cluster and lattice scenes
_ORIGIN = (310000.1, -730000.3)                 # the scenes lie away from the plane's origin


def _scene(cen, elev, K, rowlen, seed):
    """The `g` dict from_synthetic and orc.Regridder take, and em: len(elev) ice cells, all unmasked, ice cell i under the rowlen GCM
    cells (i + e) % K of K realised ones; overlaps 1e6 * (0.5 + U), all positive, sorted by (iA, iI)"""
    rng = np.random.default_rng(seed)
    n = len(elev)
    assert 1 <= rowlen <= K
    im, jm = 16, 12
    nA = im * jm
    A_to_sparse = np.sort(rng.choice(nA, K, replace=False)).astype(np.int64)
    iI = np.repeat(np.arange(n), rowlen)
    iA = A_to_sparse[(iI + np.tile(np.arange(rowlen), n)) % K]
    o = np.lexsort((iI, iA))
    iA, iI = iA[o], iI[o]
    area = 1e6 * (0.5 + rng.random(len(iA)))
    proj = 1e9 * (1.0 + rng.random(K))
    g = dict(config="scene", nx=n, ny=1, dx=1.0, x_fastest=False, nI=n, nA=nA, im=im, jm=jm,
             ex_indices=np.stack([iA, iI], axis=1).astype(np.int32), ex_area=area, A_to_sparse=A_to_sparse,
             A_native_area=proj * (1.0 + 0.05 * rng.random(K)), A_proj_area=proj, hcdefs=np.array([-50.0, 1000.0, 2000.0, 3000.0]),
             hc_stride_A=1, hc_stride_HC=nA, interp_style=0, I_centroid_xy=np.ascontiguousarray(cen, np.float64))
    return g, np.ascontiguousarray(elev, np.float64)


def cluster_scene(n, K, rowlen, sigma=SIGMA_C, seed=0):
    """n cells in a box of 0.9 sigma_x x 0.9 sigma_y x 0.9 sigma_z: every cell is every cell's neighbour, all share one bin"""
    rng = np.random.default_rng(7000 + seed)
    cen = np.stack([_ORIGIN[0] + 0.9 * sigma[0] * rng.random(n), _ORIGIN[1] + 0.9 * sigma[1] * rng.random(n)], axis=1)
    elev = 1500.0 + 0.9 * sigma[2] * rng.random(n)
    return _scene(cen, elev, K, rowlen, 8000 + seed)


LATTICE = (8, 8, 4)
_LATTICE_ORIGIN = (500000.3, 470000.7, 900.1)
LATTICE_STEPS = ((5, 0, 0), (3, 4, 0), (0, 4, 3), (4, 0, 3))     # index steps of length 5 * 0.4 = 2 sigmas: nds within ulps of 4


def lattice_scene(sigma=SIGMA_C):
    """8 x 8 x 4 cells at (x0 + 0.4 sx i, y0 + 0.4 sy j, z0 + 0.4 sz k), one GCM cell of 16 under each: pairs at the cut nds == 4"""
    ni, nj, nk = LATTICE
    I, J, Kk = np.meshgrid(np.arange(ni), np.arange(nj), np.arange(nk), indexing="ij")
    # The steps are whole numbers, so sums within one binade are exact and every such nds is exactly 4: the origin has a fraction and
    # lies just below a power of two on each axis (2^19, 2^19, 2^10), the sums above it round, and the steps fall on both sides
    x0, y0, z0 = _LATTICE_ORIGIN
    cen = np.stack([x0 + 0.4 * sigma[0] * I.ravel(), y0 + 0.4 * sigma[1] * J.ravel()], axis=1)
    elev = z0 + 0.4 * sigma[2] * Kk.ravel()
    return _scene(cen, elev, 16, 1, 8100)


FAR_SIGMA = (50e3, 50e3, 1e6)
FAR_X0, FAR_A, FAR_B = -1234500.0, -234500.0000000001, -134500.00000000012


def far_pair_scene():
    """50 km, the x centroids shifted so that their minimum is FAR_X0; two unmasked cells -- b from elsewhere on the sheet, so that its
    columns are its own -- get one y, one elevation and the x centroids FAR_A and FAR_B: (FAR_B - FAR_A) / sigma_x < 2, yet with bins
    of exactly two sigmas their truncated quotients differ by two.  Returns (g, em, ice cell a, ice cell b)."""
    g, em = grids("g50")
    g, em = dict(g), em.copy()
    cen = np.array(g["I_centroid_xy"], np.float64).reshape(-1, 2)
    cen[:, 0] += FAR_X0 - cen[:, 0].min()
    iy = g["ny"] // 2
    a, b = 20 * g["ny"] + iy, 15 * g["ny"] + iy + 10            # (y fastest; x = FAR_X0 + 50e3 * ix)
    assert cen[a, 0] == -234500.0 and not np.isnan(em[a]) and not np.isnan(em[b])
    cen[a, 0], cen[b, 0] = FAR_A, FAR_B
    cen[b, 1] = cen[a, 1]
    em[b] = em[a]
    g["I_centroid_xy"] = cen
    return g, em, a, b


def far_pair_facts(g, em, plain, a, b, sigma=FAR_SIGMA):
    """(the truncated quotients of a and b under bins of exactly two sigmas from the bounding box -- not the library's grid, so that
    the fact stays true after a fix --, whether b is a's neighbour, the columns b alone brings to a's smoothed row)"""
    cen = np.asarray(g["I_centroid_xy"], np.float64).reshape(-1, 2)
    x0, bw = cen[:, 0].min(), 2.0 * sigma[0]
    qa, qb = int((cen[a, 0] - x0) / bw), int((cen[b, 0] - x0) / bw)
    N, nb = neighbour_lists(g, em, plain, sigma)
    s = np.asarray(plain.dims[0], np.int64)
    da, db = int(np.nonzero(s == a)[0][0]), int(np.nonzero(s == b)[0][0])
    cols = lambda d: set(plain.col[plain.row == d].tolist())
    others = set()
    for j in nb[da]:
        if j != db:
            others |= cols(int(j))
    return (qa, qb), db in nb[da].tolist(), sorted(cols(db) - others)


# ---- facts from the oracle's matrices and numpy alone ------------------------------------------------------------------------------
def _tuples(g, em, plain):
    """(dense rows that are tuples -- unmasked --, their (x, y, elevation))"""
    cen = np.asarray(g["I_centroid_xy"], np.float64).reshape(-1, 2)
    s = np.asarray(plain.dims[0], np.int64)
    e = np.asarray(em, np.float64)[s]
    live = np.nonzero(~np.isnan(e))[0]
    return live, np.stack([cen[s[live], 0], cen[s[live], 1], e[live]], axis=1)


def _nds(c, lo, hi, sigma):
    """nds[i - lo, j] in the reference's division form and summation order (smoother.cpp:29-33), float64"""
    nds = np.zeros((hi - lo, len(c)))
    for k in range(3):
        d = (c[None, :, k] - c[lo:hi, None, k]) / sigma[k]
        nds = nds + d * d
    return nds


def neighbour_lists(g, em, plain, sigma, chunk=512):
    """(N[d] = neighbours of dense row d, itself included, 0 for a masked row; the neighbours' dense rows, ascending, per dense row):
    brute force over all pairs"""
    live, c = _tuples(g, em, plain)
    N = np.zeros(plain.nrow, np.int64)
    nb = [np.zeros(0, np.int64)] * plain.nrow
    for lo in range(0, len(live), chunk):
        hi = min(lo + chunk, len(live))
        hit = _nds(c, lo, hi, sigma) < 4.0
        for i in range(lo, hi):
            nb[live[i]] = np.sort(live[hit[i - lo]])
        N[live[lo:hi]] = hit.sum(axis=1)
    return N, nb


def neighbour_counts(g, em, plain, sigma, chunk=512):
    live, c = _tuples(g, em, plain)
    N = np.zeros(plain.nrow, np.int64)
    for lo in range(0, len(live), chunk):
        hi = min(lo + chunk, len(live))
        N[live[lo:hi]] = (_nds(c, lo, hi, sigma) < 4.0).sum(axis=1)
    return N


def cut_pairs(g, em, plain, sigma, eps=1e-9):
    """ordered pairs with |nds - 4| < eps: (inside the cut, outside it)"""
    live, c = _tuples(g, em, plain)
    nds = _nds(c, 0, len(live), sigma)
    near = np.abs(nds - 4.0) < eps
    return int((near & (nds < 4.0)).sum()), int((near & ~(nds < 4.0)).sum())


def bin_members(g, em, plain, sigma):
    """(members of every bin [nby, nbx], (nbx, nby)) under the library's bin grid"""
    cen = np.asarray(g["I_centroid_xy"], np.float64).reshape(-1, 2)
    x0, y0, bw, bh, nbx, nby = smooth_grid(cen.min(axis=0), cen.max(axis=0), sigma)
    _, c = _tuples(g, em, plain)
    bx = np.clip(((c[:, 0] - x0) / bw).astype(np.int64), 0, nbx - 1)
    by = np.clip(((c[:, 1] - y0) / bh).astype(np.int64), 0, nby - 1)
    return np.bincount(by * nbx + bx, minlength=nbx * nby).reshape(nby, nbx), (nbx, nby)


def reference_ld(g, em, plain, sigma):
    """The definition in long double: w_ij = exp(-nds / 2) * wM_j over nds < 4, row i = sum_j w_ij M_j / sum_j w_ij, M and wM the oracle's
    unsmoothed matrix; the cut is the reference's (float64, division form).  Returns (row, col, val long double) in (row, col) order."""
    ld = np.longdouble
    live, c = _tuples(g, em, plain)
    M = np.zeros((plain.nrow, plain.ncol), ld)
    S = np.zeros((plain.nrow, plain.ncol), bool)
    M[plain.row, plain.col] = plain.val
    S[plain.row, plain.col] = True
    Ml, Sl = M[live], S[live].astype(np.int64)
    hit = _nds(c, 0, len(live), sigma) < 4.0
    cl, nds = c.astype(ld), np.zeros(hit.shape, ld)
    for k in range(3):
        d = (cl[None, :, k] - cl[:, None, k]) / ld(sigma[k])
        nds = nds + d * d
    W = np.where(hit, np.exp(-nds / ld(2)) * plain.wM[live].astype(ld)[None, :], ld(0))
    val = (W @ Ml) / W.sum(axis=1)[:, None]
    r, col = np.nonzero((hit.astype(np.int64) @ Sl) > 0)
    return live[r].astype(np.int32), col.astype(np.int32), val[r, col]


def entry_bound(N, row, ref):
    """|v - ref| <= (2 N_i + 64) 2^-53 |ref|: all terms are positive (all overlaps are), the numerator and the denominator cost up to
    N_i roundings each; exp, the three quotients (or reciprocal products) and the final factor cost the constant"""
    return (2.0 * N[row] + 64.0) * 2.0 ** -53 * np.abs(ref)


def assert_entries_within_bound(val, N, row, ref):
    err = np.abs(np.asarray(val).astype(np.longdouble) - ref)
    bound = entry_bound(N, row, ref)
    worst = float(np.max(err / bound)) if len(ref) else 0.0
    assert worst <= 1.0, ("an entry outside the derived bound", worst)
    return worst


@functools.lru_cache(maxsize=None)
def scene(kind, *args):
    """(g, em) of a named scene, built once: "cluster" (n, K, rowlen), "lattice", "far", and the degenerate ones"""
    if kind == "cluster":
        return cluster_scene(*args)
    if kind == "lattice":
        return lattice_scene()
    if kind == "far":
        return far_pair_scene()[:2]
    g, em = cluster_scene(65, 3, 1)
    g, em = dict(g), em.copy()
    cen = np.array(g["I_centroid_xy"])
    if kind == "one_column":            # nbx == 1 with a y extent
        cen[:, 0] = cen[0, 0]
    elif kind == "one_point":           # zero extent: one bin
        cen[:] = cen[0]
    elif kind == "one_cell":            # one tuple
        em[np.arange(len(em)) != 31] = np.nan
    elif kind == "all_masked":
        em[:] = np.nan
    else:
        raise KeyError(kind)
    g["I_centroid_xy"] = cen
    return g, em


def capped_sigma(g):
    """the cap on one axis only: sigma_x = extent_x / 1e5 (nbx == MAX_BINS), sigma_y = 10 extent_y (nby == 1)"""
    cen = np.asarray(g["I_centroid_xy"]).reshape(-1, 2)
    ext = cen.max(axis=0) - cen.min(axis=0)
    return (float(ext[0]) / 1e5, 10.0 * float(ext[1]), 250.0)


@functools.lru_cache(maxsize=None)
def scene_case(name, sigma, kind, *args):
    """(g, em, plain, smoothed, facts) of a scene: the oracle's two matrices and what the limits are about, computed once"""
    g, em = scene(kind, *args)
    rg = orc.Regridder(g)
    plain = rg.matrix_d(name, em, scale=True, correctA=True)
    smoothed = rg.matrix_d(name, em, scale=True, correctA=True, sigma=sigma)
    widest, longest = neighbourhood_facts(g, em, plain, sigma)
    members, (nbx, nby) = bin_members(g, em, plain, sigma)
    facts = dict(widest=widest, longest=longest, longest_smoothed=int(np.bincount(smoothed.row, minlength=max(smoothed.nrow, 1)).max()),
                 N=neighbour_counts(g, em, plain, sigma), members=members, nbx=nbx, nby=nby)
    return g, em, plain, smoothed, facts


@functools.lru_cache(maxsize=None)
def scene_reference(name, sigma, kind, *args):
    """reference_ld of a scene_case, computed once"""
    g, em, plain, _, _ = scene_case(name, sigma, kind, *args)
    return reference_ld(g, em, plain, sigma)


def serving_form(knobs, facts):
    """the form assert_input_side lets these knobs (smooth_direct, smooth_tile) build this input with"""
    return form_served(knobs[1] > 0, knobs[0] > 0, facts["widest"], facts["longest"], facts["longest_smoothed"])


def cluster_form(K, rowlen, knobs):
    """the form a cluster leg is written for, from the scene's parameters: the tiles hold 128 columns and member rows of 8, the direct
    form 128 columns"""
    direct, tile = knobs
    if tile and K <= SMT_KMAX and rowlen <= SMT_ROWMAX:
        return TILE
    return DIRECT if direct and K <= SMD_MAXCOL else TRIPLET


# (n, K, rowlen): slots and lanes 63 / 64, 128 columns in both tables and 129, member rows of 8 and 9, a hit list exactly full at 1024 and
# drained at 1025, bins of 1, 64, 65 and 32 x 64 + 1 members
CLUSTERS_IVA = ((1, 1, 1), (64, 1, 1), (65, 1, 1), (64, 64, 1), (130, 65, 2), (128, 128, 3), (257, 128, 8), (129, 129, 1), (130, 65, 9),
                (1024, 3, 1), (1025, 3, 1), (2049, 3, 1))
CLUSTERS_IVE = ((129, 40, 1), (130, 64, 1))                  # 80 and 128 columns, rows of 2
KNOBS = ((0, 1), (1, 0), (0, 0))                             # (smooth_direct, smooth_tile): the tiles, the direct form, the triplets


# Grids with several waves in a bin of the tile form: (id, config, matrix, sigma, what the oracle and numpy measure)
BIG_LEGS = (
    # bins of up to 400 members (7 waves, the last with 16 live lanes), rows of up to 1138 neighbours (the direct form's hit list drains)
    ("g20-IvA-200km", "g20", "IvA", (200e3, 200e3, 1500.0),
     dict(rows=4870, bins=(4, 7), fullest=400, widest=76, longest=4, longest_smoothed=40, neighbours=1138)),
    # exactly SMT_KMAX columns around the widest bin, bins of up to 204 members (4 waves, the last with 12 live lanes)
    ("g50-IvA-400km", "g50", "IvA", (400e3, 400e3, 1e5),
     dict(rows=793, bins=(2, 4), fullest=204, widest=128, longest=4, longest_smoothed=110, neighbours=641)),
)
ZERO_AREA_ONE = 17
ZERO_AREA_PAIR = (1, 5)                        # (the smaller index, the larger): the larger one's dense row comes first


def zero_area_scene(cells):
    """the cluster (65, 5, 1) with a second exchange cell over each given ice cell, under the same GCM cell and of the opposite overlap:
    the cell stays a row of IvE and its area, the row's weight wM, is exactly 0.  (An overlap that is 0 itself leaves no row at all,
    and GvAp -- IvA -- keeps positive overlaps only, IceRegridder_L0.cpp:209: neither reaches the smoother's refusal.)"""
    g, em = cluster_scene(65, 5, 1)
    g = dict(g)
    ex, area = g["ex_indices"], g["ex_area"]
    q = np.nonzero(np.isin(ex[:, 1], cells))[0]
    ex, area = np.concatenate([ex, ex[q]]), np.concatenate([area, -area[q]])
    o = np.lexsort((ex[:, 1], ex[:, 0]))
    g["ex_indices"], g["ex_area"] = np.ascontiguousarray(ex[o]), area[o]
    return g, em
