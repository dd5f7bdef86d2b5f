"""Pins tests/modele_restatement.py (the numpy restatement of GCMRegridder_ModelE::regrid_matrices that
tests/test_gpu_modele.py compares the device builds with, bit for bit) on the CPU: a hand-computed case, the reference's
own identity M_unscaled == diag(wM) * M_scaled, and a cross-check against the oracle on the atmosphere grid."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modele_restatement as mr  # noqa: E402
from test_gpu_hntr_matrix import triplets_ref  # noqa: E402

R = 6371000.
NAMES = ("AvI", "EvI", "AvX", "EvX", "IvA", "IvE", "XvA", "XvE")


def ctx(g, em, hspecO, fp, fm):
    from oracle import oracle as orc
    return mr.Ctx(orc, orc.Regridder(g), em, hspecO, R, fp, fm, triplets_ref)


def dense(res, n0, n1):
    """The matrix by SPARSE indices."""
    D = np.zeros((n0, n1))
    for r, row in enumerate(res["M"]):
        for c, v in row:
            D[res["dims"][0][r], res["dims"][1][c]] = v
    return D


def test_hand_computed_4x2_ocean():
    """A 4 x 2 ocean grid (O = i + 4 j) under a 2 x 1 atmosphere: A0 = O{0, 1, 4, 5}, A1 = O{2, 3, 6, 7}; all O cells have the
    same area.  Ice cells and overlap areas:
        O0: I0 2, I1 2    O1: I1 1, I2 3    O2: I2 1, I4 2    O3: I5 5    O4: I3 4    O5: I3 1
    foceanAOm[4] = 1 (ModelE calls O4 ocean: dropped), foceanAOp[2] = 0.25, foceanAOp[3] = 1 (no ice weight left).
        wAOp = (4, 4, 3, 5, 4, 1);  wAOm = (4, 4, 3 / 0.75 = 4, 0, -, 1);  wAAm = (4 + 4 + 1, 4 + 0) = (9, 4)
        AvI(A0, .) = 1/3 * (rows of O0, O1, O5 scaled by 1 / wAOp) = I0 1/6, I1 1/3 * (2/4 + 1/4) = 1/4, I2 1/4, I3 1/3
        AvI(A1, .) = 1/2 * (rows of O2, O3)                        = I2 1/6, I4 1/3, I5 1/2
    Mw = the ice cells' total overlap (2, 3, 4, 5, 2, 5); the unscaled matrix is diag(wAAm) times the scaled one."""
    from icebin_amd import HntrSpec
    ex = [(0, 0, 2.), (0, 1, 2.), (1, 1, 1.), (1, 2, 3.), (2, 2, 1.), (2, 4, 2.), (3, 5, 5.), (4, 3, 4.), (5, 3, 1.)]
    g = dict(nA=8, nI=6, nhc=2, hcdefs=np.asarray([0., 200.]), hc_stride_A=1, hc_stride_HC=8,
             ex_indices=np.asarray([(a, i) for a, i, _ in ex], np.int32), ex_area=np.asarray([v for _, _, v in ex]),
             A_to_sparse=np.arange(6, dtype=np.int64), A_native_area=np.ones(6), A_proj_area=np.ones(6), interp_style=0)
    fp, fm = np.zeros(8), np.zeros(8)
    fm[4], fp[4] = 1., 1.
    fp[2] = 0.25
    fp[3] = 1.
    cx = ctx(g, np.full(6, 100.), HntrSpec(4, 2, 0., 5400.), fp, fm)
    want = np.zeros((2, 6))
    want[0, :4] = [1 / 6, 1 / 4, 1 / 4, 1 / 3]
    want[1, [2, 4, 5]] = [1 / 6, 1 / 3, 1 / 2]
    wAAm = np.asarray([9., 4.])
    for scale in (True, False):
        res = mr.regrid_matrix(cx, "AvI", scale)
        assert res["dims"][0].tolist() == [0, 1] and res["dims"][1].tolist() == [0, 1, 2, 4, 5, 3]
        np.testing.assert_allclose(dense(res, 2, 6), want if scale else wAAm[:, None] * want, rtol=1e-14, atol=0)
        np.testing.assert_allclose(res["wM"], wAAm, rtol=1e-14)
        np.testing.assert_allclose(res["Mw"][np.argsort(res["dims"][1])], [2., 3., 4., 5., 2., 5.], rtol=1e-14)
        assert not res["conservative"] and res["scaled"] == scale
        tr = mr.regrid_matrix(cx, "IvA", scale)
        assert tr["dims"][1].tolist() == [0, 1] and tr["dims"][0].tolist() == [0, 1, 2, 4, 5, 3]
        np.testing.assert_allclose(tr["Mw"], wAAm, rtol=1e-14)
    # IvA scaled: an ice cell takes the value of the atmosphere cell(s) above its ModelE-land O cells, weighted by overlap
    tr = dense(mr.regrid_matrix(cx, "IvA", True), 6, 2)
    np.testing.assert_allclose(tr, [[1, 0], [1, 0], [3 / 4, 1 / 4], [1 / 5, 0], [0, 1], [0, 1]], rtol=1e-14, atol=0)
    # a fractional ModelE ocean on an ice-bearing cell is the reference's error, naming the cell
    fm[1] = 0.5
    with pytest.raises(ValueError, match=r"fcont_m\[1\] = 0.5"):
        mr.regrid_matrix(ctx(g, np.full(6, 100.), HntrSpec(4, 2, 0., 5400.), fp, fm), "AvI", True)


@pytest.fixture(scope="module")
def straddle():
    """Ocean 8 x 6, ice 48 x 36 shifted by half a cell (ice cells straddle O cells inside one parent and across parents), a
    random mask, three elevation classes; every ocean pattern at once on parents that carry ice."""
    from icebin_amd import HntrSpec
    O, I = HntrSpec(8, 6, 0., 1800.), HntrSpec(48, 36, 0.5, 300.)
    rng = np.random.default_rng(11)
    em = rng.uniform(0., 3000., I.size)
    em[rng.random(I.size) < 0.4] = np.nan
    g = mr.hntr_grids(O, I, em, [0., 1500., 3000.], R)
    fp, fm = np.zeros(O.size), np.zeros(O.size)
    ice = g["A_to_sparse"]
    fm[ice[::5]] = 1.
    fp[ice[::5]] = 1.
    fp[ice[1::5]] = rng.uniform(0.1, 0.9, len(ice[1::5]))
    fp[ice[2::7]] = 1.
    return ctx(g, em, O, fp, fm)


@pytest.mark.parametrize("name", NAMES)
def test_unscaled_is_wM_times_scaled(straddle, name):
    """GCMRegridder_ModelE.cpp:356-358: M_unscaled == diag(wM) * M_scaled.  rel 1e-12: the two sides differ by a few roundings
    per entry ((w * s) * x against w * (s * x)), and in the GpvXAm group by the few-term summation order of IpvXOp.wM against
    XOpvIp.Mw."""
    s, u = mr.regrid_matrix(straddle, name, True), mr.regrid_matrix(straddle, name, False)
    assert len(s["M"]) == len(u["M"]) and np.array_equal(s["dims"][0], u["dims"][0]) and np.array_equal(s["dims"][1], u["dims"][1])
    assert np.array_equal(s["wM"], u["wM"]) and np.array_equal(s["Mw"], u["Mw"])
    n = 0
    for r, (rs, ru) in enumerate(zip(s["M"], u["M"])):
        assert [c for c, _ in rs] == [c for c, _ in ru]
        for (_, vs), (_, vu) in zip(rs, ru):
            if s["wM"][r] == 0:
                continue                         # (0 * inf: the reference's NaN, on both sides)
            assert abs(vu - s["wM"][r] * vs) <= 1e-12 * abs(vu), (name, r, vu, s["wM"][r] * vs)
            n += 1
    assert n > 100


# largest relative difference of the cross-check below, measured on the CPU; the test allows 16 times that
CROSS_MEASURED = 1.51e-15     # 7.8e-16 (straddling ice grid, unmasked) and 1.504e-15 (nested ice grid, whole O cells masked)


def cross_check(O, I, em):
    from oracle import oracle as orc
    A = mr.make_hntrA(O)
    hc = [0., 1500., 3000.]
    cx = ctx(mr.hntr_grids(O, I, em, hc, R), em, O, np.zeros(O.size), np.zeros(O.size))
    res = mr.regrid_matrix(cx, "AvI", True)
    direct = orc.Regridder(mr.hntr_grids(A, I, em, hc, R, unit_area=True)).matrix_d("AvI", em, scale=True, correctA=False)
    want = {(int(direct.dims[0][r]), int(direct.dims[1][c])): v for r, c, v in zip(direct.row, direct.col, direct.val)}
    got = {(int(res["dims"][0][r]), int(res["dims"][1][c])): v for r, row in enumerate(res["M"]) for c, v in row}
    assert set(got) == set(want) and len(got) > 100
    return max(abs(got[k] - want[k]) / abs(want[k]) for k in want)


def test_focean_zero_AvI_equals_the_atmosphere_grids_own_AvI():
    """With no ocean, AvI (scaled) through the ModelE regridder is, per (iA_sparse, iI_sparse), the oracle's AvI of a regridder
    built directly on make_hntrA(hspecO) from the same ice grid and mask.  The two agree when every O cell is either free of
    ice or wholly covered (the ModelE form averages its O cells' means by CELL area, the direct form by ICE area), so: the
    straddling ice grid with every cell unmasked, and a nested ice grid (6 x 6 ice cells per O cell) with whole O cells masked
    at random, parents partly covered included.  Measured: CROSS_MEASURED; allowed: 16 times that, and below 1e-9."""
    from icebin_amd import HntrSpec
    O = HntrSpec(8, 6, 0., 1800.)
    rng = np.random.default_rng(3)
    I1 = HntrSpec(48, 36, 0.5, 300.)
    e1 = cross_check(O, I1, rng.uniform(0., 3000., I1.size))
    I2 = HntrSpec(48, 36, 0., 300.)
    em = rng.uniform(0., 3000., I2.size).reshape(36, 48)
    off = rng.random((6, 8)) < 0.5
    em[np.repeat(np.repeat(off, 6, axis=0), 6, axis=1)] = np.nan
    e2 = cross_check(O, I2, em.reshape(-1))
    print("cross-check: largest relative difference %.3e (straddling, unmasked), %.3e (nested, whole cells masked)" % (e1, e2))
    allowed = 16 * CROSS_MEASURED
    assert allowed < 1e-9
    assert max(e1, e2) <= allowed, (e1, e2, allowed)
