"""GCMRegridder.to_modele on the GPU (ibh_modele_matrices_*): every matrix bitwise against the numpy restatement
(tests/modele_restatement.py, pinned by tests/test_modele_restatement.py) -- both sets, rowptr, colind, value bit patterns,
wM, Mw and flags -- over two grid families and every ocean pattern; the product primitive alone; pre-populated sets; the
conservation gate of apply_M; the error paths."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modele_restatement as mr  # noqa: E402
from test_gpu_hntr_matrix import triplets_ref  # noqa: E402

R = 6371000.
NAMES = ("AvI", "EvI", "AvX", "EvX", "IvA", "IvE", "XvA", "XvE")
PATTERNS = ("zero", "om1", "om2", "om4", "frac", "op1")


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class Case:
    """One O-grid regridder on the device, its oracle twin, the ice mask and the ocean HntrSpec."""

    def __init__(self, gcm, sheet, g, em, hspecO, kwargs):
        from oracle import oracle as orc
        self.gcm, self.sheet, self.em, self.hspecO, self.kwargs = gcm, sheet, em, hspecO, kwargs
        self.orc, self.rgO = orc, orc.Regridder(g)
        self.realised = np.asarray(g["A_to_sparse"], np.int64)      # agridA of the O-grid regridder
        self.ice = np.sort(self.rgO.matrix_d("AvI", em).dims[0])    # O cells that carry unmasked ice

    def ocean(self, pattern):
        """(foceanAOp, foceanAOm) of one pattern, on a parent whose four children all carry ice."""
        O = self.hspecO
        fp, fm = np.zeros(O.size), np.zeros(O.size)
        has = np.zeros(O.size, bool)
        has[self.ice] = True
        kids = None
        for ja in range(O.jm // 2):
            for ia in range(O.im // 2):
                k = [(2 * ja + dj) * O.im + 2 * ia + di for dj in (0, 1) for di in (0, 1)]
                if kids is None and all(has[k]):
                    kids = k
        assert kids is not None
        rng = np.random.default_rng(5)
        if pattern in ("om1", "om2", "om4"):
            n = int(pattern[2])
            fm[kids[:n]] = 1.
            fp[kids[:n]] = 1.
        elif pattern == "frac":
            fp[self.ice] = rng.uniform(0.05, 0.95, len(self.ice))
        elif pattern == "op1":
            fp[kids[1]] = 1.
            fp[self.ice[::3]] = 1.
        return fp, fm

    def ctx(self, fp, fm):
        return mr.Ctx(self.orc, self.rgO, self.em, self.hspecO, R, fp, fm, triplets_ref)

    def modele(self, fp, fm):
        return self.gcm.to_modele((fp, fm), **self.kwargs)


def hntr_case(interp):
    from icebin_amd import HntrSpec, global_ec
    O, I = HntrSpec(8, 6, 0., 1800.), HntrSpec(48, 36, 0.5, 300.)
    rng = np.random.default_rng(11)
    em = rng.uniform(0., 3000., I.size)
    em[rng.random(I.size) < 0.4] = np.nan
    hc = np.asarray([0., 1500., 3000.])
    gcm = global_ec.gcm_from_hntr(O, I, em, hc, True, R, interp)
    idx, area, proj = gcm._sheets["globalI"].arrays
    g = dict(nA=O.size, nI=I.size, nhc=3, hcdefs=hc, hc_stride_A=1, hc_stride_HC=O.size, ex_indices=idx.reshape(-1, 2), ex_area=area,
             A_to_sparse=gcm._A_to_sparse, A_native_area=gcm._A_native, A_proj_area=proj, interp_style=0 if interp == "Z_INTERP" else 1)
    return Case(gcm, "globalI", g, em, O, {})


def g50_case():
    from icebin_amd import HntrSpec, from_synthetic, synthetic
    g = synthetic.make_grids("g50")
    em = synthetic.dome_elevmask(g)
    return Case(from_synthetic(g), "greenland", g, em, HntrSpec(144, 90, 0., 120.), dict(hspecO=HntrSpec(144, 90, 0., 120.), eq_rad=R))


_cases = {}


@pytest.fixture(params=["hntr-Z", "hntr-EC", "g50"])
def case(request):
    k = request.param
    if k not in _cases:
        _cases[k] = g50_case() if k == "g50" else hntr_case("Z_INTERP" if k == "hntr-Z" else "ELEV_CLASS_INTERP")
    return _cases[k]


def same(w, res, what):
    for k in (0, 1):
        assert np.array_equal(w.dim(k), res["dims"][k]), (what, "dims", k)
    rp, ci, v = mr.csr(res)
    wrp, wci, wv = w.csr_dense()
    assert np.array_equal(wrp, rp) and np.array_equal(wci, ci), (what, "structure")
    assert np.array_equal(bits(wv), bits(v)), (what, "values", int(np.sum(bits(wv) != bits(v))), len(v))
    assert np.array_equal(bits(w.wM), bits(res["wM"])), (what, "wM")
    assert np.array_equal(bits(w.Mw), bits(res["Mw"])), (what, "Mw")
    assert (w.conservative, w.scaled) == (res["conservative"], res["scaled"]), (what, "flags")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_bitwise_against_the_restatement(case, pattern):
    fp, fm = case.ocean(pattern)
    rm = case.modele(fp, fm).regrid_matrices(case.sheet, case.em)
    cx = case.ctx(fp, fm)
    nnz = 0
    for name in NAMES:
        for scale in (False, True):
            w = rm.matrix_d(name, scale=scale)
            same(w, mr.regrid_matrix(cx, name, scale), (name, scale))
            nnz += w.nnz
    assert nnz > 1000


def test_prepopulated_dimE_shared_by_EvI_then_IvE(case):
    from icebin_amd import SparseSet
    fp, fm = case.ocean("om2")
    rm = case.modele(fp, fm).regrid_matrices(case.sheet, case.em)
    cx = case.ctx(fp, fm)
    dimE = SparseSet()
    EvI = rm.matrix_d("EvI", (dimE, None), scale=True)
    r1 = mr.regrid_matrix(cx, "EvI", True)
    same(EvI, r1, "EvI")
    keys = dimE.to_sparse()
    assert np.array_equal(keys, r1["dims"][0]) and dimE.sparse_extent() == rm._keep[1].nE
    # the second matrix finds every class already numbered -- in an order of its own had the set been fresh
    IvE = rm.matrix_d("IvE", (None, dimE), scale=False)
    same(IvE, mr.regrid_matrix(cx, "IvE", False, dim1=keys), "IvE")
    assert np.array_equal(dimE.to_sparse(), keys)
    # a set that holds keys the matrix never meets keeps them, and the matrix numbers its own after them
    extra = SparseSet(-1, [int(keys[-1]), 1])
    IvE2 = rm.matrix_d("IvE", (None, extra), scale=True)
    same(IvE2, mr.regrid_matrix(cx, "IvE", True, dim1=[int(keys[-1]), 1]), "IvE after extra keys")


def to_weighted(M, ncol):
    from icebin_amd import linear_Weighted
    rp, ci, v = mr.csr(dict(M=M))
    return linear_Weighted.from_csr((len(M), ncol), rp, ci, v, np.zeros(len(M)), np.zeros(ncol))


def random_rows(rng, nrow, ncol, lengths):
    M = []
    for r in range(nrow):
        n = min(int(lengths[r % len(lengths)]), ncol)
        cols = np.sort(rng.choice(ncol, n, replace=False))
        M.append([(int(c), float(x)) for c, x in zip(cols, rng.uniform(-1., 1., n))])
    return M


@pytest.mark.parametrize("shape", ["long_R_rows", "short_R_rows", "empty_L", "empty_R"])
def test_product_primitive(shape):
    """C = L * R alone (ibh_selftest_csr_product): rows of L with 1, 2 and 65 entries and none; (r, c) reached through several
    k (the columns of R are few, so rows of R overlap); an empty result row; an empty operand; both emit forms (a wave or a
    thread per row of L, chosen by the terms per row)."""
    from icebin_amd import linear_Weighted
    from icebin_amd._capi import check, lib
    rng = np.random.default_rng(17)
    nk = 70
    if shape == "long_R_rows":
        L = random_rows(rng, 9, nk, [1, 2, 65, 0, 3])
        Rm = random_rows(rng, nk, 40, [30, 0, 17, 40])
        nc = 40
    elif shape == "short_R_rows":
        L = random_rows(rng, 700, nk, [1, 2, 0, 1])
        Rm = random_rows(rng, nk, 5, [1, 2, 0, 3])
        nc = 5
    elif shape == "empty_L":
        L, Rm, nc = [[] for _ in range(4)], random_rows(rng, nk, 6, [2]), 6
    else:
        L, Rm, nc = random_rows(rng, 5, nk, [3]), [[] for _ in range(nk)], 6
    want = mr.product(L, Rm)
    if shape in ("long_R_rows", "short_R_rows"):
        terms = sum(len(Rm[k]) for row in L for k, _ in row)
        assert (terms >= 8 * len(L)) == (shape == "long_R_rows")
        assert any(not row for row in want) and terms > sum(len(r) for r in want)      # an empty row; duplicates were summed
    wl, wr = to_weighted(L, nk), to_weighted(Rm, nc)
    h = C.c_void_p()
    check(lib().ibh_selftest_csr_product(wl._h, wr._h, C.byref(h)))
    w = linear_Weighted(h)
    rp, ci, v = mr.csr(dict(M=want))
    wrp, wci, wv = w.csr_dense()
    assert (w.nrow_d, w.ncol_d) == (len(L), nc)
    assert np.array_equal(wrp, rp) and np.array_equal(wci, ci) and np.array_equal(bits(wv), bits(v))


def own_dims_matrix(maker):
    """One matrix with dims of its own from `maker`, on the smallest input its own tests build -> (matrix, identity sets promised)."""
    import icebin_amd
    from icebin_amd import linear_Weighted
    from icebin_amd._capi import check, lib
    rng = np.random.default_rng(3)
    if maker in ("from_csr", "from_coo", "csr_product"):
        L, Rm = random_rows(rng, 5, 7, [2, 0, 3]), random_rows(rng, 7, 4, [1, 2])
        if maker == "from_csr":
            return to_weighted(L, 7), True
        if maker == "from_coo":
            row = np.repeat(np.arange(5), [len(r) for r in L])
            col, val = [c for r in L for c, _ in r], [x for r in L for _, x in r]
            return linear_Weighted.from_coo((5, 7), row, col, val, np.zeros(5), np.zeros(7)), True
        wl, wr = to_weighted(L, 7), to_weighted(Rm, 4)
        h = C.c_void_p()
        check(lib().ibh_selftest_csr_product(wl._h, wr._h, C.byref(h)))
        return linear_Weighted(h), True
    if maker == "e1ve0":
        from icebin_amd import from_synthetic, synthetic
        g = synthetic.make_grids("g20")
        XvE = from_synthetic(g).regrid_matrices("greenland", synthetic.dome_elevmask(g), scale=False,
                                               correctA=True).matrix_d("XvE", scale=False, correctA=True)
        return icebin_amd.compute_E1vE0c([XvE], [XvE], g["nA"] * len(g["hcdefs"])), True
    if maker == "l1":
        import l1_restatement
        from icebin_amd import l1
        c = l1_restatement.load_case("four_tri_a1")
        ex = l1.exchange_grid_from_polygons(c["ex_iA"], c["ex_iTri"], vptr=c["ex_vptr"], qx=c["ex_qx"], qy=c["ex_qy"])
        return l1.compute_AvI(ex, int(c["nA"]), l1.Mesh(c["vx"], c["vy"], c["tri"]), scale=True), True
    if maker == "hntr":
        from test_gpu_hntr_matrix import hntr
        return hntr("8x4", "16x8").matrix_d("overlap", R), True
    if "hntr-Z" not in _cases:
        _cases["hntr-Z"] = hntr_case("Z_INTERP")
    case = _cases["hntr-Z"]
    return case.modele(*case.ocean("om1")).regrid_matrices(case.sheet, case.em).matrix_d("AvI"), False


@pytest.mark.parametrize("maker", ["from_csr", "from_coo", "e1ve0", "csr_product", "l1", "hntr", "modele"])
def test_every_maker_hands_out_readable_own_dims(maker):
    """A matrix made without caller's sets owns its two: they read back with the dense extents (nrow, ncol), as arange where
    the maker promises identity sets and as distinct keys inside the sparse extent otherwise, and destroying the handle (which
    deletes them) and building the same matrix again gives the same sets."""
    from icebin_amd._capi import check, lib
    seen = None
    for _ in range(2):
        w, identity = own_dims_matrix(maker)
        dims = []
        for k, n in enumerate((w.nrow_d, w.ncol_d)):
            dense = C.c_int32(-1)
            check(lib().ibh_weighted_dim(w._h, k, None, C.byref(dense)))
            d = w.dim(k)
            assert dense.value == n == len(d) and n > 0
            if identity:
                assert np.array_equal(d, np.arange(n)) and w.sparse_extent(k) == n
            else:
                assert len(np.unique(d)) == n and d.min() >= 0 and d.max() < w.sparse_extent(k)
            dims.append(d.copy())
        assert seen is None or all(np.array_equal(a, b) for a, b in zip(seen, dims))
        seen = dims
        del w


@pytest.mark.parametrize("name", ["AvI", "IvA"])
def test_apply_M_conserves(case, name):
    """The project's gate: |sum wM y - sum Mw x| / |sum Mw x| < 1e-13 (math.fsum) with force_conservation."""
    fp, fm = case.ocean("frac")
    w = case.modele(fp, fm).regrid_matrices(case.sheet, case.em).matrix(name)
    assert not w.conservative
    x = np.random.default_rng(2).uniform(1., 2., w.ncol_d)
    y = w.apply(x, fill=0., force_conservation=True)
    wM, Mw = w.wM, w.Mw
    lhs = math.fsum(float(a) * float(b) for a, b in zip(wM, y) if a != 0)
    rhs = math.fsum(float(a) * float(b) for a, b in zip(Mw, x))
    assert abs(lhs - rhs) / abs(rhs) < 1e-13, (lhs, rhs)


def test_test_matrices_AOmvAAm(case):
    """compute_AOmvAAm (:92-121): Hntr's overlap clipped by the caller's dimAOm, {TO_DENSE_IGNORE_MISSING, ADD_DENSE}."""
    from icebin_amd import SparseSet
    rm = case.modele(*case.ocean("zero")).regrid_matrices(case.sheet, case.em)
    keysO = case.ice[::2][::-1].copy()
    mask = np.zeros(case.hspecO.size, bool)
    mask[keysO] = True
    iO, iA, v = triplets_ref(case.hspecO, mr.make_hntrA(case.hspecO), "overlap", R, mask=mask)
    toO = {int(s): d for d, s in enumerate(keysO)}
    dimA, toA = [], {}
    for a in iA.tolist():
        if a not in toA:
            toA[a] = len(dimA)
            dimA.append(a)
    rows, cols = [toO[int(o)] for o in iO], [toA[int(a)] for a in iA]
    for name, M in (("AOmvAAm", mr.from_triplets(len(keysO), rows, cols, v.tolist())),
                    ("AAmvAOm", mr.from_triplets(len(dimA), cols, rows, v.tolist()))):
        dO, dAset = SparseSet(-1, keysO), SparseSet()
        w = rm.matrix_d(name, (dO, dAset))
        rp, ci, val = mr.csr(dict(M=M))
        wrp, wci, wv = w.csr_dense()
        assert np.array_equal(wrp, rp) and np.array_equal(wci, ci) and np.array_equal(bits(wv), bits(val)), name
        assert np.array_equal(dO.to_sparse(), keysO) and np.array_equal(dAset.to_sparse(), dimA), name
        assert w.conservative


def test_python_surface(case):
    from icebin_amd import GCMRegridder_ModelE, from_synthetic, synthetic
    m = case.gcm.to_modele(**case.kwargs)           # focean=None: no ocean
    assert isinstance(m, GCMRegridder_ModelE)
    O = case.hspecO
    assert (m.nA, m.nhc, m.nE) == (O.size // 4, case.gcm.nhc, O.size // 4 * case.gcm.nhc)
    assert not m.foceanOp.any() and not m.foceanOm.any() and len(m.foceanOm) == O.size
    with pytest.raises(NotImplementedError):
        m.wA(case.sheet, "native")
    rm = m.regrid_matrices(case.sheet, case.em, scale=False)
    same(rm.matrix("AvI"), mr.regrid_matrix(case.ctx(np.zeros(O.size), np.zeros(O.size)), "AvI", False), "matrix(AvI)")
    same(rm.matrix_d("AAmvIp", scale=False), mr.regrid_matrix(case.ctx(np.zeros(O.size), np.zeros(O.size)), "AvI", False), "AAmvIp")
    # make_agridA: the atmosphere cells above the realised O cells, first-seen in Hntr's stream order
    mask = np.zeros(O.size, bool)
    mask[case.realised] = True
    _, iA, _ = triplets_ref(O, mr.make_hntrA(O), "overlap", R, mask=mask)
    _, first = np.unique(iA, return_index=True)
    assert np.array_equal(m.agridA(case.sheet), iA[np.sort(first)])
    if not case.kwargs:
        return
    with pytest.raises(RuntimeError, match="requires specO have a Hntr source"):
        from_synthetic(synthetic.make_grids("tiny")).to_modele()


def test_errors_leave_the_sets_alone(case):
    from icebin_amd import SparseSet, _capi
    from icebin_amd._capi import lib, ptr
    O = case.hspecO
    fp, fm = case.ocean("zero")
    bad = int(case.ice[3])
    fm[bad] = 0.25
    rm = case.modele(fp, fm).regrid_matrices(case.sheet, case.em)
    for name, k in (("AvI", 0), ("IvE", 1)):
        dims = [SparseSet(), SparseSet()]
        dims[k] = SparseSet(-1, [1, 0])
        with pytest.raises(_capi.IcebinHipError, match=r"fcont_m\[%d\] = 0.75" % bad) as ei:
            rm.matrix_d(name, tuple(dims))
        assert ei.value.code == _capi.IBH_EINVAL
        assert dims[k].to_sparse().tolist() == [1, 0] and dims[k].sparse_extent() == -1
        assert dims[1 - k].dense_extent() == 0 and dims[1 - k].sparse_extent() == -1
    with pytest.raises(_capi.IcebinHipError) as ei:
        rm.matrix_d("AvE")
    assert ei.value.code == _capi.IBH_ENOKEY
    with pytest.raises(_capi.IcebinHipError, match="sparse extent") as ei:
        rm.matrix_d("AvI", (SparseSet(7), None))
    assert ei.value.code == _capi.IBH_EINVAL
    # refused before anything is allocated: an odd imO, a grid or focean arrays of the wrong size, smoothing
    rmO = case.gcm.regrid_matrices(case.sheet, case.em)
    z = np.zeros(O.size + 1)
    h = C.c_void_p()

    def create(rm_, im, jm, n):
        return lib().ibh_modele_matrices_create(rm_._h, im, jm, O.offi, O.dlat, R, ptr(z), ptr(z), n, C.byref(h))
    assert create(rmO, O.im + 1, O.jm, O.size) == _capi.IBH_EINVAL and not h.value
    assert b"even number" in lib().ibh_last_error()
    assert create(rmO, O.im + 2, O.jm, O.size) == _capi.IBH_EINVAL and not h.value
    assert create(rmO, O.im, O.jm, O.size + 1) == _capi.IBH_EINVAL and not h.value
    assert create(rmO, O.im, O.jm, O.size) == _capi.IBH_OK and h.value
    lib().ibh_modele_matrices_destroy(h)
    h = C.c_void_p()
    rmS = case.gcm.regrid_matrices(case.sheet, case.em, sigma=(50000., 50000., 100.))
    assert create(rmS, O.im, O.jm, O.size) == _capi.IBH_ENOTIMPL and not h.value
