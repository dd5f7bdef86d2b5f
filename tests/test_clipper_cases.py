"""CPU checks that the cases of tests/clipper_cases.py reach the limits they are named for -- read from the vertex counter and
the exact clipper, never from the GPU.  tests/test_gpu_clippers.py runs the same cases on the device."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clipper_cases as cc            # noqa: E402
import lonlat_restatement as llr      # noqa: E402


def convex_ccw(poly):
    P = np.asarray(poly, float)
    e = np.roll(P, -1, 0) - P
    f = np.roll(e, -1, 0)
    return bool(np.all(e[:, 0] * f[:, 1] - e[:, 1] * f[:, 0] > 0))


# ---- gridgen -------------------------------------------------------------------------------------------------------------------
def test_g20_fills_the_arrays_exactly():
    g = cc.g20()
    counts, _ = cc.gg_counts(g["poly"], -0.96, 0.96, -0.96, 0.96)
    assert counts == [16, 17, 18, 19, 20] and counts[-1] == cc.GG_CLIPV
    assert cc.gg_worst_counts(*g["three"], g["poly"]) == [16, 17, 18, 19, 20]
    keys, areas = cc.exact_gridgen(*g["three"], [g["poly"]], g["iA"])
    assert keys == [(5, 1), (5, 3), (5, 4), (5, 5), (5, 7)]                 # the centre and the four tips, no corner cell
    assert np.all(areas[[0, 1, 3, 4]] < 0.01) and areas[2] > 3.0
    assert cc.exact_gridgen(*g["one"], [g["poly"]], g["iA"])[0] == [(5, 0)]


def test_gnc_needs_more_than_the_arrays_hold():
    c = cc.gnc()
    counts, _ = cc.gg_counts(cc.ZIGZAG, 0., 2.5, -1.5, 4.25)
    print("zigzag: vertex counts %s" % counts)
    assert len(cc.ZIGZAG) == 16 and counts[1] == 23 > cc.GG_CLIPV
    assert max(cc.gg_worst_counts(*c["zigzag"])) == 23
    assert len(cc.U_SHAPE) == 8 and max(cc.gg_worst_counts(*c["u"])) <= cc.GG_CLIPV      # the U is no overflow, only not convex
    star = c["star"][2]
    assert len(star) == 16 and convex_ccw(star) and max(cc.gg_worst_counts(*c["star"])) > cc.GG_CLIPV
    assert not convex_ccw(cc.ZIGZAG) and not convex_ccw(cc.U_SHAPE)
    for name in ("zigzag", "u"):
        assert len(cc.exact_gridgen_poly(*c[name])) >= 9


def test_gr_ranges_ties_and_block_edges():
    G = cc.gr()
    xe, ye, polys = G["xe"], G["ye"], G["polys"]
    assert len(xe) - 1 == 9 and len(ye) - 1 == 7 and len(polys) == 257
    ncand = []
    for p in polys:
        ncand.append(cc.cell_range(xe, p[:, 0].min(), p[:, 0].max())[1] * cc.cell_range(ye, p[:, 1].min(), p[:, 1].max())[1])
    ncand = np.array(ncand)
    assert tuple(np.nonzero(ncand == 0)[0]) == cc.GR_ZERO_CANDIDATES         # first, two in a row, the boundary-sharers, last
    assert ncand[12] == 1 and G["per_poly"][12] == []                        # touches the grid in one corner: a candidate, no cell
    assert G["per_poly"][11] == [] and G["per_poly"][13] == []
    # a vertex exactly on interior ice edges, and as the box's minimum: the searches' ties
    sp = polys[1]
    assert sp[0, 0] == xe[3] == sp[:, 0].min() and sp[1, 1] == ye[1] == sp[:, 1].min() and (sp[2, 0], sp[2, 1]) == (xe[5], ye[3])
    assert (polys[2][0, 0], polys[2][0, 1]) == (xe[5], ye[4])
    w = polys[3]
    assert (w[:, 0].min(), w[:, 0].max(), w[:, 1].min(), w[:, 1].max()) == (xe[0], xe[-1], ye[0], ye[-1]) and ncand[3] == 63
    for k, side in ((4, 0), (5, 1), (6, 2), (9, 3)):                  # out of the left, right, bottom and top
        p = polys[k]
        out = (p[:, 0].min() < xe[0], p[:, 0].max() > xe[-1], p[:, 1].min() < ye[0], p[:, 1].max() > ye[-1])
        assert out[side] and G["per_poly"][k], k
    for npoly in cc.GR_NPOLY:
        ps, iA, pos = cc.gr_variant(npoly)
        total = int(ncand[pos].sum())
        assert len(ps) == npoly and np.all(np.diff(iA) > 0) and total > 2 * 256 and total % 256 != 0
        assert ncand[pos[-1]] == 0 and ncand[pos[0]] == 0
    # every polygon is convex and stays within n + 4; every piece is large enough for the 1e-12 bar: the array kernel's shoelace in
    # absolute coordinates and the streamed one, restated in floats, are within 1e-13 of the exact areas
    worst = 0.0
    for p, cells in zip(polys, G["per_poly"]):
        assert convex_ccw(p)
        assert all(c <= len(p) + k for k, c in enumerate(cc.gg_worst_counts(xe, ye, p)))
        for ix, iy, a in cells:
            arr = cc.gg_counts(p, xe[ix], xe[ix + 1], ye[iy], ye[iy + 1])[1]
            st = llr.clip_area(p[:, 0], p[:, 1], xe[ix], xe[ix + 1], ye[iy], ye[iy + 1])
            worst = max(worst, abs(arr - a) / a, abs(st - a) / a)
    print("GR: restated kernels vs exact, worst relative area error %.2e over %d cells" % (worst, sum(len(c) for c in G["per_poly"])))
    assert worst <= 1e-13


# ---- L1 ------------------------------------------------------------------------------------------------------------------------
def test_l19_fills_the_piece_exactly():
    L = cc.l19()
    T = [(L["vx"][v], L["vy"][v]) for v in L["tri"][0]]
    counts = cc.l1_counts(T, L["polys"][0])
    assert counts == list(range(3, 20)) and counts[-1] == cc.L1_CLIPV
    ex = cc.exact_l1(L["vx"], L["vy"], L["tri"], L["polys"], L["iA"])
    assert sorted(ex) == [(3, 0), (3, 1), (3, 2), (3, 3), (8, 3), (8, 4)]
    assert ex[(3, 0)][1] == 19 and [ex[(3, t)][1] for t in (1, 2, 3)] == [3, 3, 3]
    e = L["tri"]
    x, y = L["vx"], L["vy"]
    assert np.all((x[e[:, 1]] - x[e[:, 0]]) * (y[e[:, 2]] - y[e[:, 0]]) - (y[e[:, 1]] - y[e[:, 0]]) * (x[e[:, 2]] - x[e[:, 0]]) > 0)


def test_lb_bins_clamp_shared_bins_and_sub_meshes():
    B = cc.lb()
    g = cc.l1_bins(B["polys"])
    assert len(B["polys"]) == 257 and g[6] == 17 and g[:4] == (0., 0., 24., 16.)
    assert cc.l1_bins(B["polys"][-1:])[6] == 1 and cc.l1_bins(B["polys"][:256])[6] == 16
    big = cc.l1_bin_range(g, B["polys"][-1])
    assert big == (11, 16, 0, 16)                                  # (24, 16) is the box's maximum: f == nb, clamped to nb - 1
    vx, vy, tri = B["vx"], B["vy"], B["tri"]
    bw, bh = 1.0 / g[4], 1.0 / g[5]
    ext = np.stack([vx[tri].max(1) - vx[tri].min(1), vy[tri].max(1) - vy[tri].min(1)], 1)
    assert np.sum((ext[:, 0] < bw) & (ext[:, 1] < bh)) >= 20 and np.sum((ext[:, 0] > 2 * bw) & (ext[:, 1] > 2 * bh)) >= 20
    outside = (vx[tri].max(1) < 0) | (vx[tri].min(1) > 24) | (vy[tri].max(1) < 0) | (vy[tri].min(1) > 16)
    assert outside.sum() >= 10
    for lo, v in ((0., vx), (24., vx), (0., vy), (16., vy)):      # astride each side of the box
        assert np.any((v[tri].min(1) < lo) & (v[tri].max(1) > lo))
    # pairs whose bin ranges share more than one bin in each axis, and that do overlap: the "once" rule has something to do
    iA_pos = {int(a): k for k, a in enumerate(B["iA"])}
    shared = 0
    for (a, t) in B["exact"]:
        pr = big if iA_pos[a] == 256 else None
        if pr is None:
            continue
        tr = cc.l1_bin_range(g, np.stack([vx[tri[t]], vy[tri[t]]], 1))
        if min(pr[1], tr[1]) - max(pr[0], tr[0]) >= 1 and min(pr[3], tr[3]) - max(pr[2], tr[2]) >= 1:
            shared += 1
    assert shared >= 10
    # unit cells astride a bin edge (24/17 and 16/17 do not divide 1) are listed in two bins an axis, too
    assert sum(1 for p in B["polys"][:256] if (lambda r: r[1] > r[0] and r[3] > r[2])(cc.l1_bin_range(g, p))) >= 50
    for n in cc.LB_NTRI:
        assert sum(1 for k in B["exact"] if k[1] < n) >= 3, n
    assert len(tri) >= 257 and len(B["exact"]) > 1000
    # convex cells: a piece never needs more than 3 + pn vertices, and the pieces are large enough for the 1e-12 bar -- k_l1_clip
    # restated in floats is within 2e-13 of the exact areas (the jitter's seed was picked among a few for that margin)
    worst = 0.0
    for (a, t), (area, nv, per) in B["exact"].items():
        p = B["polys"][iA_pos[a]]
        counts, fa = cc.l1_clip([(vx[v], vy[v]) for v in tri[t]], p)
        assert all(c <= 3 + k for k, c in enumerate(counts)) and max(counts) <= 3 + len(p) <= cc.L1_CLIPV
        worst = max(worst, abs(fa - area) / area)
    print("LB: restated kernel vs exact, worst relative area error %.2e over %d cells" % (worst, len(B["exact"])))
    assert worst <= 2e-13
    # the cells tile: every GCM cell lies inside the mesh, so its pieces add up to its area
    tot = np.zeros(257)
    for (a, t), v in B["exact"].items():
        tot[iA_pos[a]] += v[0]
    assert np.max(np.abs(tot[:256] - 1.0)) <= 1e-13 and abs(tot[256] - 128.0) <= 1e-11


def test_lnc_margins():
    N = cc.lnc()
    far = cc.l1_turns(N["far"])
    worst = min(c / tol for c, tol in far)
    print("far quad: worst turn / bound = %.3e (refused below -1)" % worst)
    assert len(N["far"]) == 12 and min(c for c, _ in far) < 0 and worst > -0.1          # really bent by rounding, well inside the bound
    assert np.abs(N["far"]).max() > 2e6
    for name in ("reflex", "clockwise"):
        assert min(c / tol for c, tol in cc.l1_turns(N[name])) < -1e12, name
    assert cc.l1_turns(N["reflex"])[2][0] == -10.0                                      # the turn at vertex 3
    assert min(c / tol for c, tol in cc.l1_turns(N["star"])) > 1e12                    # the star turns left everywhere: its winding refuses it
    e = np.roll(N["star"], -1, 0) - N["star"]
    for a in (0, 1):
        s = np.sign(e[:, a])
        assert np.sum(s != np.roll(s, -1)) == 14
    m = N["far_mesh"]
    ex = cc.exact_l1(m["vx"], m["vy"], m["tri"], [N["far"]], [4])
    assert sorted(ex) == [(4, 0), (4, 1), (4, 2), (4, 3)]
