"""Which device form a smoothed build must take, decided on the CPU from the oracle's matrices: a numpy transcription of the bin
arithmetic (icebin_amd/csrc/smooth_plan.h smooth_grid, assemble.hip smooth_bin / k_smt_bincols) gives the quantities the forms' limits
are about, so that a test first asserts that its input lies on the intended side of a limit and only then which form ran
(linear_Weighted.smoothed_by): an input that drifts fails loudly instead of testing another form."""
import functools

import numpy as np

from icebin_amd import synthetic as syn
from oracle import oracle as orc

NONE, TRIPLET, DIRECT, TILE = 0, 1, 2, 3        # SmoothForm, as ibh_weighted_smoothed_by reports it
SMT_KMAX, SMT_ROWMAX, SMD_MAXCOL = 128, 8, 128  # the limits (smooth_plan.h)
MAX_BINS = 4096


def smooth_grid(cmin, cmax, sigma):
    """(x0, y0, bw, bh, nbx, nby): bins of two sigmas over the centroids' bounding box, at most MAX_BINS per axis"""
    bw, bh = 2.0 * sigma[0], 2.0 * sigma[1]
    nbx = int(min(float(MAX_BINS), np.floor((cmax[0] - cmin[0]) / bw) + 1.0))
    nby = int(min(float(MAX_BINS), np.floor((cmax[1] - cmin[1]) / bh) + 1.0))
    if nbx == MAX_BINS:
        bw = (cmax[0] - cmin[0]) / float(MAX_BINS) * (1 + 1e-12)
    if nby == MAX_BINS:
        bh = (cmax[1] - cmin[1]) / float(MAX_BINS) * (1 + 1e-12)
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


def assert_input_side(form, tile_tried, direct_tried, widest, longest, longest_smoothed):
    """the input lies where the knobs (which forms are tried) make `form` the one that builds the matrix"""
    tile_fits = widest <= SMT_KMAX and longest <= SMT_ROWMAX
    direct_fits = longest_smoothed <= SMD_MAXCOL
    want = TILE if tile_tried and tile_fits else DIRECT if direct_tried and direct_fits else TRIPLET
    assert want == form, ("the input left the side of the limits this leg is about", dict(
        form=form, tile_tried=tile_tried, direct_tried=direct_tried, widest=widest, longest=longest, longest_smoothed=longest_smoothed))


# The small legs (50 km: 793 unmasked rows, unsmoothed rows of at most 8 entries, so only the column limits are in play):
# (sigma, matrix, (smooth_direct, smooth_tile), the form that must build it, the knobs whose build it must equal bitwise or None)
G50_LEGS = (
    ((60e3, 60e3, 250.0), "IvE", (0, 1), TILE, None),           # 127 columns around the widest bin: at the edge of SMT_KMAX; raised LDS
    ((60e3, 60e3, 250.0), "IvA", (0, 1), TILE, None),           # 18
    ((120e3, 120e3, 400.0), "IvE", (1, 1), DIRECT, (1, 0)),     # 347 around a bin, rows of <= 92: the tiles overflow, the direct form serves
    ((200e3, 200e3, 1500.0), "IvE", (1, 1), TRIPLET, (0, 0)),   # 604, rows of up to 315: both overflow
    ((200e3, 200e3, 1500.0), "IvA", (1, 1), TILE, None),        # 76
)
