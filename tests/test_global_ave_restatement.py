"""Pins tests/global_ave_restatement.py (the plain-Python restatement of compute_EOpvAOp_merged, squash_ECs and
_compute_AAmvEAm_EIGEN that tests/test_gpu_global_ave.py compares the device builds with, bit for bit) on the CPU: a
hand-computed case, the reference's identity M_unscaled == diag(wM) * M_scaled, the three invariants of the row-normalised
factors, and what squash_ECs and the choice of nhc do."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_ave_cases as gc  # noqa: E402
import global_ave_restatement as gr  # noqa: E402
import modele_restatement as mr  # noqa: E402
from test_gpu_hntr_matrix import triplets_ref  # noqa: E402

R = gc.R

# The largest relative deviations of the restatement on the fixtures (F1 + F2, every ocean pattern that keeps wEOm != 0),
# measured on the CPU; each test allows 16 times its figure and never more than the project's 1e-12.
MEASURED_IDENTITY = 4.4e-16         # |M_unscaled - wM * M_scaled| / |M_unscaled|
MEASURED_ROWSUM = 3.4e-16           # |sum of a non-empty scaled row - 1|
MEASURED_WEIGHTS = 1.2e-16          # |sum wAAm - sum wAOm|, |sum wEAm - sum wEOm|, |sum wEOm - sum wAOm|, relative


def allowed(measured):
    tol = 16 * measured
    assert tol <= 1e-12
    return tol


def dense(res, n0, n1):
    """The matrix by SPARSE indices."""
    D = np.zeros((n0, n1))
    for r, row in enumerate(res["M"]):
        for c, v in row:
            D[res["dims"][0][r], res["dims"][1][c]] = v
    return D


def test_hand_computed_4x2_ocean():
    """A 4 x 2 ocean grid (O = i + 4 j) under a 2 x 1 atmosphere: A0 = O{0, 1, 4, 5}, A1 = O{2, 3, 6, 7}; all O cells have the
    same area a.  One sheet, classes (0, 200), every ice cell at 100 m: half of its area in either class.  Ice per O cell
        O0 4   O1 4   O2 3   O3 5   O4 4   O5 1
    One base class (500 m), offsetE = 8 * 2 = 16, the stream (iE, iO, v) = (6, 6, 3) (1, 1, 6) (4, 4, 2) (6, 6, 1): O6 lies outside
    the sheet and appears twice (3 + 1 = 4), O1 also carries local ice, O4 is ModelE ocean.
      EOpvAOp   rows (iO + 8 ihc) first-seen by columns of the sheet, then the base: (O, class 0) = (O, class 1) = ice / 2;
                (22, O6) = 4, (17, O1) = 6, (20, O4) = 2
      wAOp      (4, 4 + 6, 3, 5, 4 + 2, 1, 4)
      foceanAOm[4] = 1 drops O4; foceanAOp[2] = 0.25: wAOm = (4, 10, 3 / 0.75 = 4, 5, -, 1, 4)
      wAAm      A0 = 4 + 10 + 1 = 15, A1 = 4 + 5 + 4 = 13
      wEOm      a row of EOmvAOm scaled to its column's wAOm: O0 (2, 2), O1 (2, 2, 6), O2 1.5 / 3 * 4 = (2, 2), O3 (2.5, 2.5), O5
                (0.5, 0.5), O6 (-, -, 4)
      wEAm      (A, class) = the sum of its O cells' wEOm: A0 (4.5, 4.5, 6), A1 (4.5, 4.5, 4)
      M scaled  M(A, (A, class)) = 1/3 * sum over the three O cells of EOpvAOp((O, class), O) / wAOp[O]
                A0: (2/4 + 2/10 + 0.5/1) / 3 = 0.4 twice, (6/10) / 3 = 0.2;   A1: (1.5/3 + 2.5/5) / 3 = 1/3 twice, (4/4) / 3 = 1/3
      M unscaled = diag(wAAm) * M scaled."""
    from icebin_amd import HntrSpec
    from oracle import oracle as orc
    ex = [(0, 0, 2.), (0, 1, 2.), (1, 1, 1.), (1, 2, 3.), (2, 2, 1.), (2, 4, 2.), (3, 5, 5.), (4, 3, 4.), (5, 3, 1.)]
    g = dict(nA=8, nI=6, nhc=2, hcdefs=np.asarray([0., 200.]), hc_stride_A=1, hc_stride_HC=8,
             ex_indices=np.asarray([(a, i) for a, i, _ in ex], np.int32), ex_area=np.asarray([v for _, _, v in ex]),
             A_to_sparse=np.arange(6, dtype=np.int64), A_native_area=np.ones(6), A_proj_area=np.ones(6), interp_style=0)
    sheets = [(orc.Regridder(g), np.full(6, 100.))]
    base = ([500.], ([6, 1, 4, 6], [6, 1, 4, 6], [3., 6., 2., 1.]), (8, 8))
    res = gr.merged(orc, sheets, 8, 2, [0., 200.], base)
    assert res["dims"] == [[0, 8, 1, 9, 2, 10, 3, 11, 4, 12, 5, 13, 22, 17, 20], [0, 1, 2, 3, 4, 5, 6]]
    assert res["M"] == [[(0, 2.)], [(0, 2.)], [(1, 2.)], [(1, 2.)], [(2, 1.5)], [(2, 1.5)], [(3, 2.5)], [(3, 2.5)], [(4, 2.)], [(4, 2.)],
                        [(5, .5)], [(5, .5)], [(6, 4.)], [(1, 6.)], [(4, 2.)]]
    assert res["wM"] == [2., 2., 2., 2., 1.5, 1.5, 2.5, 2.5, 2., 2., .5, .5, 4., 6., 2.] and res["Mw"] == [4., 10., 3., 5., 6., 1., 4.]
    assert (res["extents"], res["offsetE"], res["hcdefs"], res["underice"], res["strides"]) == ([24, 8], 16, [0., 200., 500.], [1, 1, 2], (1, 8))
    fp, fm = np.zeros(8), np.zeros(8)
    fm[4], fp[4] = 1., 1.
    fp[2] = 0.25
    O = HntrSpec(4, 2, 0., 5400.)
    want = np.zeros((2, 6))                         # columns: A + 2 * class
    want[0, [0, 2, 4]] = [0.4, 0.4, 0.2]
    want[1, [1, 3, 5]] = [1 / 3, 1 / 3, 1 / 3]
    wAAm = np.asarray([15., 13.])
    for scale in (True, False):
        parts = {}
        a = gr.AAmvEAm(res, O, R, fp, fm, triplets_ref, scale=scale, parts=parts)
        assert a["dims"][0].tolist() == [0, 1] and a["dims"][1].tolist() == [0, 2, 4, 1, 3, 5] and a["extents"] == [2, 6]
        assert [[c for c, _ in row] for row in a["M"]] == [[0, 1, 2], [3, 4, 5]]
        np.testing.assert_allclose(dense(a, 2, 6), want if scale else wAAm[:, None] * want, rtol=1e-14, atol=0)
        np.testing.assert_allclose(a["wM"], wAAm, rtol=1e-14)
        np.testing.assert_allclose(a["Mw"], [4.5, 4.5, 6., 4.5, 4.5, 4.], rtol=1e-14)
        assert not a["conservative"] and a["scaled"] == scale
        assert parts["dimAOm"] == [0, 1, 2, 3, 5, 6] and parts["dimEOm"] == [0, 8, 1, 9, 17, 2, 10, 3, 11, 5, 13, 22]
        np.testing.assert_allclose(parts["wAOm"], [4., 10., 4., 5., 1., 4.], rtol=1e-14)
        np.testing.assert_allclose(parts["wEOm"], [2., 2., 2., 2., 6., 2., 2., 2.5, 2.5, .5, .5, 4.], rtol=1e-14)
    # a fractional ModelE ocean on an ice-bearing cell is the reference's error, naming the cell
    fm[1] = 0.5
    with pytest.raises(ValueError, match=r"fcont_m\[1\] = 0.5"):
        gr.AAmvEAm(res, O, R, fp, fm, triplets_ref)


class F1:
    """Two sheets on the 8 x 6 ocean (tests/global_ave_cases.py), restated on the host, and the base F2."""

    def __init__(self):
        from oracle import oracle as orc
        self.orc = orc
        self.O, Is = gc.specs()
        self.ems = gc.masks()
        self.grids = [mr.hntr_grids(self.O, I, em, gc.HC, R) for I, em in zip(Is, self.ems)]
        self.sheets = [(orc.Regridder(g), em) for g, em in zip(self.grids, self.ems)]
        ice = gc.ice_cells(self.grids)
        self.ice = np.union1d(ice[0], ice[1])
        self.both = np.intersect1d(ice[0], ice[1])
        self.kids = gc.ocean("zero", self.both, self.O)[2]
        self.base = gc.base(self.ice, self.kids, self.O)

    def merged(self, **kw):
        kw.setdefault("base", self.base)
        return gr.merged(self.orc, self.sheets, self.O.size, 3, gc.HC, **kw)


@pytest.fixture(scope="module")
def f1():
    return F1()


def test_fixture_has_two_sheets_in_one_class_of_one_cell(f1):
    """At least one O cell carries ice of both sheets in the same elevation class: the merge sums such duplicates."""
    rows = []
    for rg, em in f1.sheets:
        dE = f1.orc.SparseSet()
        rg.matrix_d("EvA", em, dims=(dE, f1.orc.SparseSet()), scale=False, correctA=False)
        rows.append(set(dE.to_sparse().tolist()))
    shared = rows[0] & rows[1]
    assert len(shared) > 10
    res = f1.merged(base=None)
    assert len(res["dims"][0]) == len(rows[0] | rows[1]) and sum(len(r) for r in res["M"]) == len(rows[0] | rows[1])
    assert len(np.setdiff1d(np.arange(f1.O.size), f1.ice)) >= 4         # cells outside every sheet


# the ocean patterns whose ice-bearing cells keep wEOm != 0 (no foceanAOp == 1 on an ice-bearing cell that ModelE calls land)
INVARIANT_PATTERNS = ("zero", "om1", "om2", "om4", "frac")


@pytest.mark.parametrize("pattern", INVARIANT_PATTERNS)
def test_identity_and_invariants(f1, pattern):
    """topo.cpp:335: M_unscaled == diag(wM) * M_scaled; and, because the three factors are row-normalised: every non-empty row of
    the scaled M sums to 1, sum wAAm == sum wAOm, sum wEAm == sum wEOm == sum wAOm (math.fsum)."""
    fp, fm, _ = gc.ocean(pattern, f1.both, f1.O)
    res = f1.merged()
    parts = {}
    s = gr.AAmvEAm(res, f1.O, R, fp, fm, triplets_ref, scale=True, parts=parts)
    u = gr.AAmvEAm(res, f1.O, R, fp, fm, triplets_ref, scale=False)
    assert np.array_equal(s["wM"], u["wM"]) and np.array_equal(s["Mw"], u["Mw"])
    assert all(np.array_equal(a, b) for a, b in zip(s["dims"], u["dims"]))
    dev_id = dev_row = 0.
    n = 0
    for r, (rs, ru) in enumerate(zip(s["M"], u["M"])):
        assert [c for c, _ in rs] == [c for c, _ in ru]
        for (_, vs), (_, vu) in zip(rs, ru):
            dev_id = max(dev_id, abs(vu - s["wM"][r] * vs) / abs(vu))
            n += 1
        if rs:
            dev_row = max(dev_row, abs(math.fsum(v for _, v in rs) - 1.))
    assert n >= 40
    tAOm, tEOm = math.fsum(parts["wAOm"]), math.fsum(parts["wEOm"])
    dev_w = max(abs(math.fsum(s["wM"]) - tAOm) / tAOm, abs(math.fsum(s["Mw"]) - tEOm) / tEOm, abs(tEOm - tAOm) / tAOm)
    print("%s: identity %.3e, row sums %.3e, weights %.3e" % (pattern, dev_id, dev_row, dev_w))
    assert dev_id <= allowed(MEASURED_IDENTITY), dev_id
    assert dev_row <= allowed(MEASURED_ROWSUM), dev_row
    assert dev_w <= allowed(MEASURED_WEIGHTS), dev_w


def test_squash_of_distinct_classes_only_renumbers(f1):
    """With every class elevation distinct, squash_ECs keeps every entry and weight; rows are numbered by the column-major
    visit instead of the stream, under keys that are the old ones with the class index replaced by its rank."""
    hc_b, trip, shape = f1.base
    base = (np.asarray([1700., 4000.]), trip, shape)
    m0, m1 = f1.merged(base=base), f1.merged(base=base, squash_ecs=True)
    assert m1["hcdefs"] == [0., 1500., 1700., 3000., 4000.] and m0["hcdefs"] == [0., 1500., 3000., 1700., 4000.]
    assert m1["underice"] == [2] * 5 and m0["underice"] == [1, 1, 1, 2, 2] and m1["strides"] == m0["strides"] == (1, 48)
    assert m1["extents"] == [48 * 5, 48] and m1["dims"][1] == m0["dims"][1] and m1["Mw"] == m0["Mw"]
    to_new = [0, 1, 3, 2, 4]
    key1 = {k: (k % 48) + 48 * to_new[k // 48] for k in m0["dims"][0]}
    by_key0 = {k: (row, w) for k, row, w in zip(m0["dims"][0], m0["M"], m0["wM"])}
    by_key1 = {k: (row, w) for k, row, w in zip(m1["dims"][0], m1["M"], m1["wM"])}
    assert {key1[k]: v for k, v in by_key0.items()} == by_key1
    assert m1["dims"][0] != [key1[k] for k in m0["dims"][0]]            # (the numbering did move)


def test_squash_sums_equal_classes_into_one_row(f1):
    """The base's 1500 m class is the sheets' class 1: squashed, a cell's local and base ice of that class share a row."""
    m0, m1 = f1.merged(), f1.merged(squash_ecs=True)
    assert m0["hcdefs"] == [0., 1500., 3000., 1500., 4000.] and m1["hcdefs"] == [0., 1500., 3000., 4000.]
    nO = 48
    local = {k for k in m0["dims"][0] if k // nO == 1}
    basek = {k - 2 * nO for k in m0["dims"][0] if k // nO == 3}
    assert local & basek
    assert len(m1["dims"][0]) == len(m0["dims"][0]) - len(local & basek)
    w0 = dict(zip(m0["dims"][0], m0["wM"]))
    w1 = dict(zip(m1["dims"][0], m1["wM"]))
    for k in local & basek:
        assert w1[k] == w0[k] + w0[k + 2 * nO]            # column-major visit: the local row (dense ids are older) first
    assert math.fsum(m1["Mw"]) == pytest.approx(math.fsum(m0["Mw"]), rel=1e-15)


def test_nhc_local_drops_every_base_class(f1):
    """The snapshot's global_AvE passes indexings whose class extent is the LOCAL count: raw_EOvEA then never reaches a base
    class, and no column of the result has a class index >= nhc_local (DESIGN.md 16 composes the functions as the offline
    tools do instead, with nhc = every merged class)."""
    fp, fm, _ = gc.ocean("om1", f1.both, f1.O)
    res = f1.merged()
    nA = f1.O.size // 4
    lit = gr.AAmvEAm(res, f1.O, R, fp, fm, triplets_ref, nhc=3)
    full = gr.AAmvEAm(res, f1.O, R, fp, fm, triplets_ref)
    assert lit["extents"] == [nA, nA * 3] and full["extents"] == [nA, nA * 5]
    assert max(lit["dims"][1]) // nA <= 2 and set(np.asarray(full["dims"][1]) // nA) == {0, 1, 2, 3, 4}
    assert set(lit["dims"][1].tolist()) == {k for k in full["dims"][1].tolist() if k // nA <= 2}
