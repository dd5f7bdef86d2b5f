"""Pins tests/topo_restatement.py (the plain-Python restatement of merge_topoO and make_topoA that tests/test_gpu_topo.py
compares the device with) on the CPU: a hand-computed case with every number written out, the reference's own sanity
conditions, what mergemaskOm marks, the single-cell-ocean pass (sequential against one-shot), the DBL_MIN quirk and the
ghost ranges; and records how far the restatement's sequential row sums lie from math.fsum on the GPU fixtures."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_ave_restatement as gr  # noqa: E402
import topo_cases as tc  # noqa: E402
import topo_restatement as tr  # noqa: E402
from test_gpu_hntr import regrid_ref  # noqa: E402
from test_gpu_hntr_matrix import triplets_ref  # noqa: E402

R = tc.R
NaN = float("nan")

# The largest relative deviation |sequential - fsum| / |fsum| of a row sum OvI . elevmaskI (the products rounded, as both add
# them) over the rows of every raw build of a fixture, measured on the CPU.  The GPU sums the same products in another order:
# tests/test_gpu_topo.py holds the device to the project's apply gate, 1e-12, and prints its deviation beside these.
MEASURED_SEQ_VS_FSUM = {"t1": 4.9e-16, "t2": 3.9e-16}


def allowed(measured):
    tol = 16 * measured
    assert tol <= 1e-12
    return tol


def same(a, b):
    """bitwise, NaN positions included"""
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def hand_sheet(orc):
    """A 4 x 4 ocean (iO = i + 4 j), every cell of native area 4.  One sheet of 6 ice cells: (O cell, ice cell, overlap)."""
    ex = [(5, 0, 1.), (5, 1, 1.), (6, 2, 2.), (6, 3, 2.), (9, 4, 1.)]
    g = dict(nA=16, nI=6, nhc=2, hcdefs=np.asarray([0., 400.]), hc_stride_A=1, hc_stride_HC=16,
             ex_indices=np.asarray([(a, i) for a, i, _ in ex], np.int32), ex_area=np.asarray([v for _, _, v in ex]),
             A_to_sparse=np.arange(16, dtype=np.int64), A_native_area=np.full(16, 4.), A_proj_area=np.full(16, 4.), interp_style=0)
    land = np.asarray([100., 300., 200., -50., 1000., NaN])
    ice = np.asarray([100., NaN, 200., NaN, NaN, NaN])
    return [(orc.Regridder(g), land, ice)]


def ocean_planes(n):
    """every cell ModelE ocean"""
    z, o = np.zeros(n), np.ones(n)
    return dict(foceanOp=o.copy(), fgiceOp=z.copy(), zatmoOp=z.copy(), foceanOm=o.copy(), flakeOm=z.copy(), fgrndOm=z.copy(), fgiceOm=z.copy(),
                zatmoOm=z.copy(), zicetopO=z.copy())


def test_hand_computed_4x4_ocean():
    """Land: O5 holds ice cells of 100 m and 300 m (overlap 1 each: half of the O cell), O6 of 200 m and -50 m (2 each: all of
    it), O9 one of 1000 m (a quarter).  Ice: the 100 m cell of O5 and the 200 m cell of O6.
      OvI . elev     land O5 (100 + 300) / 2 = 200, O6 (200 - 50) / 2 = 75, O9 1000;   ice O5 100, O6 200
      da_zicetopO    O5 100 * 4, O6 200 * 4;   da_giceO O5 1, O6 2;   da_zatmoO O5 800, O6 300, O9 4000;   da_contO O5 2, O6 4, O9 1
      O5   fgiceOp 1/4, foceanOp 1 - 2/4 = 1/2 (not below 1/2: stays ModelE ocean), zatmoOp 200, zicetopO (400/4 * 1/4) / (1/4) = 100
      O6   fgiceOp 1/2, foceanOp 0 -> land: fact 1, fgiceOm 1/2, fgrndOm 1/2, zatmoOm = zatmoOp = 75, zicetopO (800/4 * 1/2) / (1/2) = 200
      O9   foceanOp 3/4, zatmoOp 1000, no ice: mergemaskOm stays 0 and zland_* NaN (the mask follows the ICE build alone)
      zland_min / zland_max   O5 (100, 300), O6 (-50, 200)
    make_topoA under the 2 x 2 atmosphere A0 = O{0, 1, 4, 5}, A1 = O{2, 3, 6, 7}, A2 = O{8, 9, 12, 13}, A3 = O{10, 11, 14, 15}:
    a polar O row weighs 1 - s, the row beside it s = sin 45; both A rows are pole rows and take their row's mean.
      focean   A1 = 1 - s/2, row 0 -> 1 - s/4, row 1 -> 1;   fgice = fgrnd: A1 = s/4, row 0 -> s/8;   zatmo A1 = 75 s/2, row 0 -> 75 s/4
      zicetop (weight fgiceOm)   A1 = 200, A0 = DATMIS = 0, row 0 -> 100
      mergemask (1, 1, 0, 0);   zland_min (100, -50) -> 25, zland_max (300, 200) -> 250, row 1 NaN
      AAmvEAm by hand, classes (0, 400): A0 (1/2, 1/2), A1 (1, 0); the south-pole mean gives row 0 (3/4, 1/4)
      underice   class 0 (1, 1, 0, 0), class 1 (1, 0, 0, 0): A1's class 1 has a mean fhc but no entry;  sea-land class: row 0
      elevE      class k = hcdefs[k] everywhere, the sea-land class = zatmoA;   no ghosts: both classes of row 0 hold ice"""
    from icebin_amd import HntrSpec
    from oracle import oracle as orc
    out, errors = tr.merge_topoO(orc, hand_sheet(orc), [4.] * 16, ocean_planes(16), 4, 4)
    assert errors == []

    def plane(dflt, **cells):
        p = [dflt] * 16
        for k, v in cells.items():
            p[int(k[1:])] = v
        return p
    assert out["fgiceOp"] == plane(0., O5=.25, O6=.5) and out["foceanOp"] == plane(1., O5=.5, O6=0., O9=.75)
    assert out["zatmoOp"] == plane(0., O5=200., O6=75., O9=1000.) and out["zicetopO"] == plane(0., O5=100., O6=200.)
    assert out["foceanOm"] == plane(1., O6=0.) and out["fgiceOm"] == plane(0., O6=.5) and out["fgrndOm"] == plane(0., O6=.5)
    assert out["flakeOm"] == [0.] * 16 and out["zatmoOm"] == plane(0., O6=75.)
    assert out["mergemaskOm"] == plane(0, O5=1, O6=1)
    assert same(out["zland_minO"], plane(NaN, O5=100., O6=-50.)) and same(out["zland_maxO"], plane(NaN, O5=300., O6=200.))

    O, A = HntrSpec(4, 4, 0., 2700.), HntrSpec(2, 2, 0., 5400.)
    out["zlakeOm"] = [0.] * 16
    entries = [(0, 0, .5), (0, 4, .5), (1, 1, 1.)]
    a, errors = tr.make_topoA(out, out["mergemaskOm"], O, A, (1, 4), [0., 400.], [1, 1], entries, regrid_ref, triplets_ref)
    assert errors == []
    s = math.sin(math.pi / 4)
    rt = dict(rtol=1e-14, atol=0)
    np.testing.assert_allclose(a["focean"], [1 - s / 4, 1 - s / 4, 1., 1.], **rt)
    np.testing.assert_allclose(a["fgice"], [s / 8, s / 8, 0., 0.], **rt)
    np.testing.assert_allclose(a["fgrnd"], [s / 8, s / 8, 0., 0.], **rt)
    np.testing.assert_allclose(a["zatmo"], [75 * s / 4, 75 * s / 4, 0., 0.], **rt)
    np.testing.assert_allclose(a["zicetop"], [100., 100., 0., 0.], **rt)     # (w * 200) / w is 200 to an ulp
    assert a["flake"] == [0.] * 4 and a["zlake"] == [0.] * 4
    assert a["mergemask"] == [1, 1, 0, 0]
    assert same(a["zland_min"], [25., 25., NaN, NaN]) and same(a["zland_max"], [250., 250., NaN, NaN])
    assert a["fhc"] == [.75, .75, 0., 0., .25, .25, 0., 0., 1e-30, 1e-30, 0., 0.]
    assert a["underice"] == [1, 1, 0, 0, 1, 0, 0, 0, 5, 5, 0, 0]
    assert a["elevE"][:8] == [0.] * 4 + [400.] * 4 and a["elevE"][8:] == a["zatmo"]


class Case:
    def __init__(self, name):
        from oracle import oracle as orc
        self.orc, self.name = orc, name
        self.c = getattr(tc, name)()
        self.O = self.c["O"]
        self.sums = []
        self.out, self.errors = tr.merge_topoO(orc, tc.oracle_sheets(orc, self.c), tc.native_area(self.c), self.c["planes"], self.O.im,
                                               self.O.jm, sums=self.sums)


@pytest.fixture(scope="module", params=["t1", "t2"])
def case(request):
    return Case(request.param)


def test_land_fractions_sum_to_one_and_nothing_is_nan(case):
    assert case.errors == []
    o = case.out
    dev = max(abs(o["foceanOm"][c] + o["fgrndOm"][c] + o["flakeOm"][c] + o["fgiceOm"][c] - 1.) for c in range(case.O.size))
    assert dev <= 1e-13
    # the fixtures do what they are for: cells turn to land, and cells keep their ocean
    before = np.asarray(case.c["planes"]["foceanOm"])
    after = np.asarray(o["foceanOm"])
    assert np.sum((before == 1.) & (after == 0.)) >= 4 and np.sum(after == 1.) >= 2 and set(after.tolist()) == {0., 1.}


def test_mergemask_marks_the_ice_build_and_changed_ice(case):
    """mergemaskOm is 1 exactly on the cells of the ice build (scale = 1, correctA = 0), on cells with diff_fgiceOp != 0 and on
    cells the update turned to land; zland_* are NaN exactly where it is 0."""
    orc = case.orc
    want = np.zeros(case.O.size, bool)
    for rg, _, em_ice in tc.oracle_sheets(orc, case.c):
        want[tr.sheet_elevO(orc, rg, em_ice, True, False)[0]] = True
    ice_cells = want.copy()
    o = case.out
    flipped = (np.asarray(case.c["planes"]["foceanOm"]) == 1.) & (np.asarray(o["foceanOm"]) == 0.)
    changed_ice = np.asarray(o["fgiceOp"]) != np.asarray(case.c["planes"]["fgiceOp"])
    assert not np.any(changed_ice & ~ice_cells)                     # diff_fgiceOp != 0 only under the ice build
    mask = np.asarray(o["mergemaskOm"]) != 0
    assert np.all(mask[ice_cells]) and not np.any(mask & ~ice_cells & ~flipped)
    assert np.array_equal(np.isnan(o["zland_minO"]), ~mask) and np.array_equal(np.isnan(o["zland_maxO"]), ~mask)
    assert 4 <= mask.sum() < case.O.size
    # land masks are supersets of the ice masks: a merged cell's range holds every ice elevation under it
    assert np.all(np.asarray(o["zland_minO"])[mask] <= np.asarray(o["zland_maxO"])[mask])


def test_sequential_row_sums_against_fsum(case):
    dev = 0.
    n = 0
    for w_ice, em_ice, elev_ice, w_land, em_land, elev_land in case.sums:
        for w, em, elev in ((w_ice, em_ice, elev_ice), (w_land, em_land, elev_land)):
            x = np.asarray(em, np.float64).tolist()
            terms = [[] for _ in range(w.nrow)]
            for r, c, v in zip(w.row.tolist(), w.col.tolist(), w.val.tolist()):
                terms[r].append(v * x[c])
            for r in range(w.nrow):
                exact = math.fsum(terms[r])
                assert exact != 0 and not math.isnan(exact)
                dev = max(dev, abs(elev[r] - exact) / abs(exact))
                n += 1
    print("%s: %d row sums, sequential against fsum %.3e" % (case.name, n, dev))
    assert n >= 20 and dev <= MEASURED_SEQ_VS_FSUM[case.name] * 1.0001
    assert allowed(MEASURED_SEQ_VS_FSUM[case.name]) <= 1e-12


def test_t2_is_arranged_as_promised():
    c = Case("t2")
    O = c.O
    at = lambda ij: ij[1] * O.im + ij[0]   # noqa: E731
    before, after = np.asarray(c.c["planes"]["foceanOm"]), np.asarray(c.out["foceanOm"])
    op = np.asarray(c.out["foceanOp"])
    crossed = (before == 1.) & (op < 0.5)
    assert crossed.sum() >= 10 and np.all(after[crossed] == 0.)
    # the interior single-cell ocean: still ModelE ocean after the per-cell update (foceanOp >= 0.5), land after the pass
    s = at(tc.T2_SINGLE)
    assert before[s] == 1. and 0.5 <= op[s] < 1. and after[s] == 0.
    assert c.out["fgiceOm"][s] == c.out["fgiceOp"][s] * (1. / (1. - op[s]))
    # the edge candidate has the same surroundings and is skipped; of two adjacent candidates neither qualifies
    e = at(tc.T2_EDGE)
    assert before[e] == 1. and 0.5 <= op[e] < 1. and after[e] == 1.
    assert all(after[k] == 0. for k in (e - O.im, e + O.im, e + 1))
    for k in map(at, tc.T2_PAIR):
        assert before[k] == 1. and 0.5 <= op[k] < 1. and after[k] == 1.


def test_single_cell_pass_sequential_equals_one_shot():
    """An 8 x 8 pattern with isolated, diagonal and adjacent candidates and candidates on every edge.  A cell changes only if it
    is 1 and its four neighbours are 0: two adjacent cells never both qualify, and a changed cell (1 -> 0) cannot make a
    neighbour qualify (that neighbour would have needed the changed cell to be 0 before): the in-place loop and the one-shot
    pass agree."""
    rows = ["00000000",
            "01000100",     # (1,1) isolated; (5,1) diagonal to (6,2) and (4,2)
            "00001010",
            "01100000",     # (1,3), (2,3) adjacent: neither
            "00000010",     # (6,4) isolated
            "10000001",     # edges
            "00010000",     # (3,6): isolated, but foceanOp == 1 keeps it
            "00100100"]     # the last row is an edge
    om = np.asarray([[float(ch) for ch in r] for r in rows]).reshape(-1)
    rng = np.random.default_rng(3)

    def fresh():
        p = ocean_planes(64)
        p["foceanOm"] = om.copy()
        p["foceanOp"] = np.where(om == 1., 0.8, 0.1)
        p["foceanOp"][6 * 8 + 3] = 1.
        p["fgiceOp"] = rng.uniform(0., .2, 64)
        p["flakeOm"] = np.full(64, .125)
        p["zatmoOp"] = rng.uniform(0., 500., 64)
        return {k: v.tolist() for k, v in p.items()}
    rng = np.random.default_rng(3)
    seq = fresh()
    rng = np.random.default_rng(3)
    one = fresh()
    tr.single_cell_oceans(seq, 8, 8, one_shot=False)
    tr.single_cell_oceans(one, 8, 8, one_shot=True)
    assert seq == one
    changed = [k for k in range(64) if seq["foceanOm"][k] != om[k]]
    assert changed == [1 * 8 + 1, 1 * 8 + 5, 2 * 8 + 4, 2 * 8 + 6, 4 * 8 + 6]
    k = 8 + 1
    assert seq["fgiceOm"][k] == seq["fgiceOp"][k] * (1. / (1. - .8)) and seq["fgrndOm"][k] == 1.0 - seq["fgiceOm"][k] - .125


def test_dbl_min_quirk():
    """zland_maxO starts at numeric_limits<double>::min(), the smallest positive NORMAL number, not at the lowest double: a
    merged cell whose land lies entirely below sea level keeps it."""
    from oracle import oracle as orc
    rg, land, ice = hand_sheet(orc)[0]
    land, ice = land.copy(), ice.copy()
    land[[0, 1]] = [-30., -10.]
    ice[0] = -30.
    out, errors = tr.merge_topoO(orc, [(rg, land, ice)], [4.] * 16, ocean_planes(16), 4, 4)
    assert errors == [] and out["mergemaskOm"][5] == 1
    assert out["zland_minO"][5] == -30. and out["zland_maxO"][5] == tr.DBL_MIN == 2.2250738585072014e-308
    assert out["zland_maxO"][6] == 200.
    # make_topoA takes the value for "unset" on the A cell that holds nothing else
    from icebin_amd import HntrSpec
    out["zlakeOm"] = [0.] * 16
    out["mergemaskOm"][6] = 0
    a, _ = tr.make_topoA(out, out["mergemaskOm"], HntrSpec(4, 4, 0., 2700.), HntrSpec(2, 2, 0., 5400.), (1, 4), [0., 400.], [1, 1], [],
                         regrid_ref, triplets_ref)
    assert a["mergemask"] == [1, 0, 0, 0] and math.isnan(a["zland_max"][0]) and math.isnan(a["zland_min"][0])      # (-30 + NaN) / 2


def test_ghost_ranges():
    hc = [0., 500., 1000., 1500., 2000.]
    # inside the table: the largest class below zland_min, less one, to the largest class at or below zland_max, plus two
    assert tr.ghost_range(hc, 5, 600., 1100.) == (0, 4)
    assert tr.ghost_range(hc, 5, 1600., 1700.) == (2, 4)
    assert tr.ghost_range(hc, 5, 1000., 1000.) == (0, 4)            # zland_min == a class: that class is not "below" it
    assert tr.ghost_range(hc, 5, 1001., 1001.) == (1, 4)
    # below the table: no class lies below zland_min, the int sentinel survives and the range is empty
    lo, hi = tr.ghost_range(hc, 5, -50., 700.)
    assert (lo, hi) == (tr.INT_MAX - 1, 3) and lo > hi
    lo, hi = tr.ghost_range(hc, 5, -50., -20.)
    assert (lo, hi) == (tr.INT_MAX - 1, tr.INT_MIN + 2)
    # above the table
    assert tr.ghost_range(hc, 5, 2500., 2600.) == (3, 4)
    # NaN (an A cell no merged O cell lies under): every comparison is false
    assert tr.ghost_range(hc, 5, NaN, NaN) == (tr.INT_MAX - 1, tr.INT_MIN + 2)
    # only the leading local classes count
    assert tr.ghost_range(hc, 2, 600., 1100.) == (0, 1) and tr.ghost_range(hc, 0, 600., 1100.) == (tr.INT_MAX - 1, tr.INT_MIN + 2)


class TopoA:
    """make_topoA of a fixture's merged planes under the restated global AvE (local classes 0 / 1500 / 3000 and the base ice of
    tests/global_ave_cases.py)."""

    def __init__(self, case):
        orc, c, O = case.orc, case.c, case.O
        sheets = [(rg, em_ice) for rg, _, em_ice in tc.oracle_sheets(orc, c)]
        ice = np.unique(np.concatenate([tr.sheet_elevO(orc, rg, em, True, False)[0] for rg, em in sheets]))
        self.base = tc.base(c, ice)
        self.merged = gr.merged(orc, sheets, O.size, 3, tc.HC, self.base)
        self.AvE = gr.AAmvEAm(self.merged, O, R, case.out["foceanOp"], case.out["foceanOm"], triplets_ref, scale=True)
        self.hspecA = gr.make_hntrA(O)
        self.entries = [(int(self.AvE["dims"][0][r]), int(self.AvE["dims"][1][k]), v) for r, row in enumerate(self.AvE["M"]) for k, v in row]
        planes = dict(case.out, zlakeOm=c["planes"]["zlakeOm"])
        self.out, self.errors = tr.make_topoA(planes, case.out["mergemaskOm"], O, self.hspecA, (1, self.hspecA.size), self.merged["hcdefs"],
                                              self.merged["underice"], self.entries, regrid_ref, triplets_ref)


def test_make_topoA_sanity_and_ghosts(case):
    """fhc sums to 0 or 1 within 1e-13 (T2 keeps its ice off the pole rows: the south-pole mean of fhc, :735-740, would leave
    other sums where only a part of the row's cells holds ice)."""
    t = TopoA(case)
    assert len(t.entries) >= 10
    a, nA, nhc = t.out, t.hspecA.size, len(t.merged["hcdefs"])
    assert nhc == 5 and t.merged["underice"] == [1, 1, 1, 2, 2]
    assert t.errors == []
    ghosts = land = 0
    for c in range(nA):
        frac = a["focean"][c] + a["fgrnd"][c] + a["flake"][c] + a["fgice"][c]
        assert abs(frac - 1.) <= 1e-13
        s = math.fsum(a["fhc"][k * nA + c] for k in range(nhc + 1))
        assert s == 0. or abs(s) <= (nhc + 1) * 1e-30 or abs(s - 1.) <= 1e-13, (c, s)
        col = [a["underice"][k * nA + c] for k in range(nhc + 1)]
        if a["focean"][c] == 1.:
            assert tr.UI_VGHOST not in col                          # no ghosts over pure ocean
        else:
            land += 1
        for k in range(nhc + 1):
            if col[k] == tr.UI_VGHOST:
                ghosts += 1
                assert k < 3 and a["fhc"][k * nA + c] == 1e-30      # only local classes, only where there was no ice
        assert all(not math.isnan(a["elevE"][k * nA + c]) for k in range(nhc + 1))
        assert (col[nhc] == tr.UI_SEALAND) == (a["fgice"][c] > 0)
    assert land >= 4
    if case.name == "t2":
        assert ghosts >= 1
        assert sum(1 for c in range(nA) if a["focean"][c] == 1.) >= 1
