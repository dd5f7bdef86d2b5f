"""Smoothed IvA / IvE (sigma != 0) through GCMRegridder.to_modele (ibh_modele_matrices_matrix_d_sigma): the composition bitwise
against the numpy restatement (tests/modele_restatement.py) fed the device's own smoothed O-grid matrix; end to end against the
oracle's smoothed O-grid matrix within a derived bound; the row-local composition against the generic product, bit for bit; the
coupler's sequence of four matrices on one object; the refusals; the Python surface."""
import math
import os
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modele_restatement as mr  # noqa: E402
import smoothing_cases as smc  # noqa: E402
import test_gpu_modele as tgm  # noqa: E402
from test_gpu_hntr_matrix import triplets_ref  # noqa: E402
from test_gpu_modele import PATTERNS, Case, bits, g50_case, same  # noqa: E402,F401

R = tgm.R
SIGMA = smc.SIGMA_C                     # (60 km, 45 km, 250 m): 793 ice rows on g50, smoothed IvE rows of up to 33 entries
SIGMA_B = (50e3, 50e3, 100.)
I_NAMES = ("IvA", "IvE", "IpvAAm", "IpvEAm")
BASE = {"IvA": "IvA", "IvE": "IvE", "IpvAAm": "IvA", "IpvEAm": "IvE"}       # the restatement knows the aliases by their base names
SMOOTHED_RTOL = 1e-12                   # what tests/test_gpu_smoothing.py (check_leg) allows an O-grid smoothed entry against the oracle

_g50 = []


@pytest.fixture
def g50():
    if not _g50:
        _g50.append(g50_case())
    return _g50[0]


@pytest.fixture
def rowlocal():
    """Sets ibh_set_tuning("modele_rowlocal", v) and puts the default back."""
    from icebin_amd.linear import set_tuning
    yield lambda v: set_tuning("modele_rowlocal", v)
    set_tuning("modele_rowlocal", -1)


class OracleSmoothCtx(mr.Ctx):
    """The restatement's context whose I-row O-grid matrix (IpvXOp) is the ORACLE's smoothed build."""

    def __init__(self, case, fp, fm, sigma):
        super().__init__(case.orc, case.rgO, case.em, case.hspecO, R, fp, fm, triplets_ref)
        self.sigma = sigma

    def o_matrix(self, name, dims, correctA):
        if name[0] != "I":
            return super().o_matrix(name, dims, correctA)
        return self.rgO.matrix_d(name, self.em, dims=dims, scale=False, correctA=correctA, sigma=self.sigma)


class DeviceSmoothCtx(mr.Ctx):
    """The restatement's context whose I-row O-grid matrix is the DEVICE's own smoothed build: the same name, scale = False,
    correctA = False, the same sigma and the keys already in the two sets; the oracle's sets are advanced by what it appended."""

    def __init__(self, case, fp, fm, sigma):
        super().__init__(case.orc, case.rgO, case.em, case.hspecO, R, fp, fm, triplets_ref)
        self.sigma = sigma
        self.rmO = case.gcm.regrid_matrices(case.sheet, case.em)

    def o_matrix(self, name, dims, correctA):
        if name[0] != "I":
            return super().o_matrix(name, dims, correctA)
        from icebin_amd import SparseSet
        assert not correctA
        dev = [SparseSet(-1, d.to_sparse()) for d in dims]
        w = self.rmO.matrix_d(name, tuple(dev), scale=False, correctA=False, sigma=self.sigma)
        assert w.smoothed_by() != 0
        for d, s in zip(dims, dev):
            for key in s.to_sparse()[d.dense_extent:].tolist():
                d.add_dense(key)
        row, col, val = w.coo_dense()
        return types.SimpleNamespace(row=row, col=col, val=val, nrow=w.nrow_d, wM=w.wM, Mw=w.Mw)


def restated(cx, name, scale, **kw):
    return mr.regrid_matrix(cx, BASE[name], scale, **kw)


def csr_bits(w):
    rp, ci, v = w.csr_dense()
    return [rp, ci, bits(v), bits(w.wM), bits(w.Mw), w.dim(0), w.dim(1), np.asarray([w.conservative, w.scaled])]


def same_matrix(a, b, what):
    for k, (x, y) in enumerate(zip(csr_bits(a), csr_bits(b))):
        assert np.array_equal(x, y), (what, k)


# ---- 1: the composition, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_composition_bitwise_on_the_devices_own_smoothed_matrix(g50, pattern):
    """The smoother's three forms agree with each other and with the oracle only to rounding, so the bitwise statement is about
    the composition: the restatement takes the device's own smoothed O-grid IvA / IvE and must give every bit of the ModelE
    matrix -- both sets, structure, values, wM, Mw and flags."""
    fp, fm = g50.ocean(pattern)
    rm = g50.modele(fp, fm).regrid_matrices(g50.sheet, g50.em)
    cx = DeviceSmoothCtx(g50, fp, fm, SIGMA)
    longest = 0
    for name in I_NAMES:
        for scale in (False, True):
            w = rm.matrix_d(name, scale=scale, sigma=SIGMA)
            same(w, restated(cx, name, scale), (name, scale))
            assert w.composed_by() == 2 and w.smoothed_by() != 0
            longest = max(longest, int(np.diff(w.csr_dense()[0]).max()))
    assert longest > 8          # longer than any unsmoothed row: the smoothing went through


def test_composition_bitwise_at_a_second_sigma(g50):
    fp, fm = g50.ocean("frac")
    rm = g50.modele(fp, fm).regrid_matrices(g50.sheet, g50.em)
    cx = DeviceSmoothCtx(g50, fp, fm, SIGMA_B)
    for name in ("IvA", "IvE"):
        same(rm.matrix_d(name, scale=True, sigma=SIGMA_B), restated(cx, name, True), name)


# ---- 2: end to end against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["zero", "om2", "frac"])
def test_end_to_end_against_the_oracle(g50, pattern, monkeypatch):
    """The same comparison with the ORACLE's smoothed O-grid matrix as the restatement's input: dims, rowptr, colind, wM and Mw
    are exact (the smoother changes no structure and neither weight vector), the values are close.

    The bound.  A composed entry is C(i, c) = sum of T terms t = ((rs[i] * v) * cs[k]) * r, v an entry of the smoothed O-grid
    matrix; rs, cs and r come from matrices and weights that are bitwise the oracle's (wM of a smoothed matrix is the unsmoothed
    one's), so the device's term differs from the oracle's only through v, by at most SMOOTHED_RTOL = 1e-12 relative -- what
    tests/test_gpu_smoothing.py allows a smoothed entry -- plus three roundings of 2^-53 on either side.  Every factor is
    positive (asserted: all values > 0), so the terms do not cancel and the T - 1 additions add at most (T - 1) * 2^-53 relative
    on either side: |dev - ref| <= (1e-12 + (2 T + 4) * 1.2e-16) * |ref|.  The issue's bound is T_max * 1e-12 * |ref| with
    T_max the largest number of terms one composed entry sums in the case, counted from the restatement's own product; it
    covers the line above once T_max >= 2 (asserted), since 1e-12 then exceeds (2 T + 4) * 1.2e-16 for every T below 4000."""
    fp, fm = g50.ocean(pattern)
    rm = g50.modele(fp, fm).regrid_matrices(g50.sheet, g50.em)
    cx = OracleSmoothCtx(g50, fp, fm, SIGMA)
    terms = []
    product = mr.product

    def counting_product(L, Rm):
        worst = 0
        for row in L:
            n = {}
            for k, _ in row:
                for c, _ in Rm[k]:
                    n[c] = n.get(c, 0) + 1
            worst = max(worst, max(n.values(), default=0))
        terms.append(worst)
        return product(L, Rm)

    monkeypatch.setattr(mr, "product", counting_product)
    for name in ("IvA", "IvE"):
        for scale in (False, True):
            w = rm.matrix_d(name, scale=scale, sigma=SIGMA)
            del terms[:]
            res = restated(cx, name, scale)
            tmax = terms[0]
            assert len(terms) == 1 and 2 <= tmax < 4000
            for k in (0, 1):
                assert np.array_equal(w.dim(k), res["dims"][k]), (name, scale, "dims", k)
            rp, ci, v = mr.csr(res)
            wrp, wci, wv = w.csr_dense()
            assert np.array_equal(wrp, rp) and np.array_equal(wci, ci), (name, scale, "structure")
            assert np.array_equal(bits(w.wM), bits(res["wM"])) and np.array_equal(bits(w.Mw), bits(res["Mw"])), (name, scale)
            assert (w.conservative, w.scaled) == (False, scale)
            assert (v > 0).all()
            dev = np.abs(wv - v) / v
            print("%s scale=%d %s: T_max %d, largest deviation %.3g of the bound %.3g" % (name, scale, pattern, tmax, dev.max(),
                                                                                         tmax * SMOOTHED_RTOL))
            assert dev.max() <= tmax * SMOOTHED_RTOL, (name, scale, dev.max(), tmax)


# ---- 3: both compositions, the same bits ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_rowlocal_and_product_give_the_same_bits(g50, pattern, rowlocal):
    fp, fm = g50.ocean(pattern)
    rm = g50.modele(fp, fm).regrid_matrices(g50.sheet, g50.em)
    for name in I_NAMES:
        for scale in (False, True):
            rowlocal(0)
            a = rm.matrix_d(name, scale=scale, sigma=SIGMA)
            rowlocal(1)
            b = rm.matrix_d(name, scale=scale, sigma=SIGMA)
            rowlocal(-1)
            c = rm.matrix_d(name, scale=scale, sigma=SIGMA)
            assert (a.composed_by(), b.composed_by(), c.composed_by()) == (1, 2, 2), (name, scale)
            same_matrix(a, b, (name, scale))
            same_matrix(a, c, (name, scale))
            assert a.nnz > 1000
    # sigma = 0 goes where it always went, and AvI is the generic product whatever the knob
    assert rm.matrix_d("IvE").composed_by() == 1 and rm.matrix_d("AvI").composed_by() == 1
    rowlocal(1)
    assert rm.matrix_d("IvE").composed_by() == 2 and rm.matrix_d("AvI").composed_by() == 1
    assert rm.matrix_d("AOmvAAm").composed_by() == 0


@pytest.mark.parametrize("pattern", PATTERNS)
def test_unsmoothed_rows_through_the_rowlocal_form(tgm_case, pattern, rowlocal):
    """modele_rowlocal = 1: the unsmoothed IvA / IvE of test_bitwise_against_the_restatement's inputs, through the row-local form."""
    case = tgm_case
    fp, fm = case.ocean(pattern)
    rm = case.modele(fp, fm).regrid_matrices(case.sheet, case.em)
    cx = case.ctx(fp, fm)
    rowlocal(1)
    for name in ("IvA", "IvE", "XvA", "XvE"):
        for scale in (False, True):
            w = rm.matrix_d(name, scale=scale)
            assert w.composed_by() == 2 and w.smoothed_by() == 0
            same(w, mr.regrid_matrix(cx, name, scale), (name, scale))


@pytest.fixture(params=["hntr-Z", "hntr-EC", "g50"])
def tgm_case(request, g50):
    k = request.param
    if k == "g50":
        return g50
    if k not in tgm._cases:
        tgm._cases[k] = tgm.hntr_case("Z_INTERP" if k == "hntr-Z" else "ELEV_CLASS_INTERP")
    return tgm._cases[k]


# ---- 4: the coupler's sequence (IceCoupler.cpp:361-468) on one object ------------------------------------------------------------
def test_the_couplers_sequence_on_one_object(g50):
    from icebin_amd import SparseSet
    fp, fm = g50.ocean("om2")
    rm = g50.modele(fp, fm).regrid_matrices(g50.sheet, g50.em)
    nI = int(g50.rgO.nI)
    dimE, dimA, dimI = SparseSet(), SparseSet(), SparseSet.identity(nI)
    EvI = rm.matrix_d("EvI", (dimE, dimI), scale=True)
    keys = dimE.to_sparse()
    assert len(keys) > 0 and np.array_equal(dimI.to_sparse(), np.arange(nI))
    AvI = rm.matrix_d("AvI", (dimA, dimI), scale=True)
    IvE = rm.matrix_d("IvE", (dimI, dimE), scale=True, sigma=SIGMA)
    assert np.array_equal(dimE.to_sparse(), keys) and np.array_equal(dimI.to_sparse(), np.arange(nI))
    XvE = rm.matrix_d("XvE", (None, dimE), scale=True)
    assert np.array_equal(dimE.to_sparse(), keys)
    assert (EvI.nrow_d, AvI.ncol_d, IvE.ncol_d, XvE.ncol_d) == (len(keys), nI, len(keys), len(keys))
    cx = DeviceSmoothCtx(g50, fp, fm, SIGMA)
    same(IvE, restated(cx, "IvE", True, dim0=np.arange(nI), dim1=keys), "IvE after EvI and AvI")
    same(XvE, mr.regrid_matrix(g50.ctx(fp, fm), "XvE", True, dim1=keys), "XvE")


# ---- 5: refusals leave the sets alone ------------------------------------------------------------------------------------------
def untouched(dims):
    return (dims[0].to_sparse().tolist() == [1, 0] and dims[0].sparse_extent() == -1 and dims[1].dense_extent() == 0
            and dims[1].sparse_extent() == -1)


def test_refusals_leave_the_sets_alone(g50):
    from icebin_amd import SparseSet, _capi
    fp, fm = g50.ocean("om1")
    rm = g50.modele(fp, fm).regrid_matrices(g50.sheet, g50.em)
    for name in ("XvE", "XvA"):
        dims = (SparseSet(-1, [1, 0]), SparseSet())
        with pytest.raises(_capi.IcebinHipError, match="rows on the exchange grid") as ei:
            rm.matrix_d(name, dims, sigma=SIGMA)
        assert ei.value.code == _capi.IBH_ENOTIMPL and untouched(dims)
    for name in ("IvE", "IvA"):
        dims = (SparseSet(-1, [1, 0]), SparseSet())
        with pytest.raises(_capi.IcebinHipError, match="three positive sigmas") as ei:
            rm.matrix_d(name, dims, sigma=(5e4, 0, 100))
        assert ei.value.code == _capi.IBH_EINVAL and untouched(dims)
    # AvI / EvI never read sigma, a bad one included; sigma[0] == 0 is no smoothing at all
    for name in ("AvI", "EvI"):
        plain = rm.matrix_d(name)
        same_matrix(rm.matrix_d(name, sigma=SIGMA), plain, name)
        same_matrix(rm.matrix_d(name, sigma=(5e4, 0, 100)), plain, name)
    same_matrix(rm.matrix_d("IvE", sigma=(0, 45e3, 250.)), rm.matrix_d("IvE"), "sigma[0] == 0")
    assert rm.matrix_d("IvE", sigma=(0, 45e3, 250.)).composed_by() == 1


def test_a_grid_without_centroids_gives_the_smoothers_message():
    from icebin_amd import SparseSet, _capi
    if "hntr-Z" not in tgm._cases:
        tgm._cases["hntr-Z"] = tgm.hntr_case("Z_INTERP")
    case = tgm._cases["hntr-Z"]
    rm = case.modele(*case.ocean("zero")).regrid_matrices(case.sheet, case.em)
    dims = (SparseSet(-1, [1, 0]), SparseSet())
    with pytest.raises(_capi.IcebinHipError, match="needs the ice grid's centroid_xy") as ei:
        rm.matrix_d("IvE", dims, sigma=SIGMA)
    assert ei.value.code == _capi.IBH_EINVAL and untouched(dims)
    same_matrix(rm.matrix_d("EvI", sigma=SIGMA), rm.matrix_d("EvI"), "EvI")


# ---- 6: the surface ----------------------------------------------------------------------------------------------------------
def test_python_surface(g50):
    fp, fm = g50.ocean("frac")
    m = g50.modele(fp, fm)
    rm = m.regrid_matrices(g50.sheet, g50.em, scale=True, sigma=SIGMA)
    plain = m.regrid_matrices(g50.sheet, g50.em, scale=True)
    same_matrix(rm.matrix("IvE"), plain.matrix_d("IvE", scale=True, sigma=SIGMA), "matrix(IvE)")
    same_matrix(rm.matrix("EvI"), plain.matrix("EvI"), "matrix(EvI)")
    assert rm.matrix("IvE").nnz > plain.matrix("IvE").nnz
    with pytest.raises(NotImplementedError):
        m.wA(g50.sheet, "native")
    # the project's gate (test_gpu_modele.py: test_apply_M_conserves) on the smoothed IvA
    w = rm.matrix("IvA")
    assert not w.conservative and w.smoothed_by() != 0
    x = np.random.default_rng(2).uniform(1., 2., w.ncol_d)
    y = w.apply(x, fill=0., force_conservation=True)
    lhs = math.fsum(float(a) * float(b) for a, b in zip(w.wM, y) if a != 0)
    rhs = math.fsum(float(a) * float(b) for a, b in zip(w.Mw, x))
    assert abs(lhs - rhs) / abs(rhs) < 1e-13, (lhs, rhs)
