"""Elevations at the edges of the class table, on every kind of exchange cell.

A plain module (no tests, no fixtures).  One small sorted grid (assembly_limit_cases.build_grid) whose ice cells take their
elevations cell by cell from a table of edge values, ice cell i the row i % len(rows), so that every row lands on plain cells, on
straddlers, in duplicate runs, on ice cells of several ranges, and on exchange cells without and with negative area.
tests/test_class_edge_cases.py checks that with numpy (the class pattern as test_assembly_limit_cases.class_pattern restates it) and
that the oracle builds or refuses every scene as claimed; tests/test_gpu_class_edges.py builds every scene through the general
pipeline, the per-range build and the streamed build and compares every matrix with the oracle bit for bit.
"""
import numpy as np

import assembly_limit_cases as alc

# 863 exchange cells: 33 straddlers in four groups, 24 ice cells in three ranges each, 32 duplicate runs of three and of two cells
GRID = dict(ranges=[60, 110, 300, 17, 256, 120], straddle=[(0, 1, 6, 1), (1, 3, 4, 2), (2, 4, 20, 0), (0, 5, 3, 3)],
            dups=[(2, 3, 16), (4, 2, 16)], multi=[(0, 3, 24)], area=dict(zero_every=11, neg_every=7))
TABLES = {"from_zero": np.array([0.0, 100.0, 200.0, 300.0]), "above_zero": np.array([100.0, 200.0, 300.0, 400.0])}
# hc_stride_A, hc_stride_HC as functions of (nA, nhc): classes outermost (the default), classes innermost
STRIDES = {"class_major": lambda nA, nhc: (1, nA), "cell_major": lambda nA, nhc: (nhc, 1)}


def rows_of(table, interp_style, tiny):
    """The elevations of a scene.  Z_INTERP: every one legal (the oracle builds all of EvI, IvE, EvX, XvE, AvE, EvA).  `tiny`: with
    1e-300, whose upper weight over a table from zero is 1e-302 -- the streamed build hands such a mask on (weights below 1e-30)."""
    hc = TABLES[table]
    top = hc[-1]
    rows = [0.0, -0.0, -5.0, 5e-324, np.nextafter(100.0, 0.0), 100.0, np.nextafter(100.0, 200.0), 150.0, 250.0,
            np.nextafter(300.0, 0.0), 300.0, np.nextafter(top, 0.0), top, np.nan]
    if tiny:
        rows.insert(4, 1e-300)
    if interp_style == 1:
        # ELEV_CLASS_INTERP: the exact tie between two classes (the lower one wins) and the first value past it, for both tables;
        # above the top class and below the lowest are legal there
        rows += [50.0, np.nextafter(50.0, 100.0), 150.0 + 0.0, np.nextafter(150.0, 200.0), top + 50.0, 1e300, hc[0] - 50.0]
    out = []
    for v in rows:                                          # (a value listed twice -- 300 is the top of one table -- once)
        if not any(np.array_equal(np.float64(v).view(np.uint64), np.float64(u).view(np.uint64)) for u in out):
            out.append(v)
    return np.array(out, np.float64)


def scene(table="from_zero", interp_style=0, strides="class_major", tiny=False, cells=None, hcdefs=None, spare_ice=None):
    """(grid dict, elevation mask) of one scene.  cells: {ice cell: elevation} on top of the table; hcdefs: a class table of its
    own; spare_ice: an elevation for one more ice cell that no exchange cell names."""
    g, _ = alc.build_grid(GRID)
    hc = TABLES[table] if hcdefs is None else np.asarray(hcdefs, np.float64)
    rows = rows_of(table, interp_style, tiny)
    em = rows[np.arange(g["nI"]) % len(rows)].copy()
    for ice, v in (cells or {}).items():
        em[ice] = v
    if spare_ice is not None:
        g["nI"] += 1
        g["nx"] += 1
        g["I_centroid_xy"] = np.zeros((g["nI"], 2))
        em = np.r_[em, spare_ice]
    g["hcdefs"] = hc
    g["interp_style"] = interp_style
    g["hc_stride_A"], g["hc_stride_HC"] = STRIDES[strides](g["nA"], len(hc))
    return g, em


def kinds(g):
    """Per exchange cell: the kinds it belongs to, as boolean arrays by name."""
    ex = g["ex_indices"].astype(np.int64)
    iA, iI, area = ex[:, 0], ex[:, 1], g["ex_area"]
    mult = np.bincount(iI, minlength=g["nI"])
    nranges = np.zeros(g["nI"], np.int64)
    seen = np.unique(np.stack([iI, iA], axis=1), axis=0)
    np.add.at(nranges, seen[:, 0], 1)
    return {"plain": mult[iI] == 1, "straddler": nranges[iI] == 2, "multi": nranges[iI] >= 3,
            "duplicate": (mult[iI] > 1) & (nranges[iI] == 1), "zero_area": area == 0, "negative_area": area < 0}


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------
# name -> scene arguments.  stream_path: the path the streamed-build knob must end on (2, or 1 where the mask holds a weight below
# 1e-30 and the streamed build hands the matrix to the per-range build)
LEGAL = {}
for _style in (0, 1):
    for _strides in STRIDES:
        for _table in TABLES:
            LEGAL["%s-%s-style%d" % (_table, _strides, _style)] = dict(args=dict(table=_table, interp_style=_style, strides=_strides), stream_path=2)
    LEGAL["from_zero-tiny-style%d" % _style] = dict(args=dict(table="from_zero", interp_style=_style, tiny=True), stream_path=1 if _style == 0 else 2)
LEGAL["above_zero-tiny-style0"] = dict(args=dict(table="above_zero", interp_style=0, tiny=True), stream_path=2)
# "An offending cell that is masked elsewhere must not raise", read two ways.  Here: an elevation beyond the top class on an ice cell
# that no exchange cell names -- nobody evaluates it, nothing is refused.  In the refusal test: the offending ice cells of a
# refused scene under the mask (NaN) -- the scene builds, through the same path.
LEGAL["spare_ice_beyond_top"] = dict(args=dict(spare_ice=np.nextafter(300.0, np.inf)), stream_path=2)

TOP = 300.0
# ice cells of GRID: 0 .. 32 the straddlers (6 .. 9 first seen in range 1), 33 .. 56 in three ranges, 57 .. 88 the duplicate runs,
# 89 .. the plain cells in range order.  PLAIN0 is a plain cell of range 0: its exchange cell comes before every cell of range 1.
STRADDLER1, PLAIN0 = 7, 93
# name -> (scene arguments, the ice cell whose elevation the refusal names)
REFUSED = {
    "one_ulp_beyond_top": (dict(cells={PLAIN0: np.nextafter(TOP, np.inf)}), PLAIN0),
    "one_ulp_beyond_top_on_a_straddler": (dict(cells={STRADDLER1: np.nextafter(TOP, np.inf)}), STRADDLER1),
    # two offenders: the one whose exchange cell comes first is reported, not the one with the lower ice index
    "two_offenders": (dict(cells={STRADDLER1: 301.0, PLAIN0: 350.0}), PLAIN0),
    "two_offenders_cell_major": (dict(cells={STRADDLER1: 301.0, PLAIN0: 350.0}, strides="cell_major"), PLAIN0),
    # one class: linterp_1d_b has no interval at all, the first unmasked exchange cell is refused
    "one_class": (dict(hcdefs=[0.0]), None),
}
E_MATRICES = ("EvI", "IvE", "EvX", "XvE", "AvE", "EvA")
