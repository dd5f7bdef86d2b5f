"""global_AvE on the GPU (ibh_modele_merge_EOpvAOp, ibh_modele_AAmvEAm): the merged / squashed EOpvAOp and AAmvEAm bitwise
against the plain-Python restatement (tests/global_ave_restatement.py, pinned by tests/test_global_ave_restatement.py) --
both sets of every result, rowptr, colind, value bit patterns, wM, Mw, flags, offsetE, hcdefs, underice_hc, strides -- on
two sheets sharing one 8 x 6 ocean (F1) with a base ice matrix (F2), over every ocean pattern, every combination of local
and global ice, squash_ecs, pre-populated sets, an empty sheet, no sheet at all and a 144 x 90 ocean; the error paths."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_ave_cases as gc  # noqa: E402
import global_ave_restatement as gr  # noqa: E402
import modele_restatement as mr  # noqa: E402
from test_global_ave_restatement import MEASURED_ROWSUM, allowed  # noqa: E402
from test_gpu_hntr_matrix import triplets_ref  # noqa: E402

R = gc.R
# (use_local_ice, use_global_ice); "global" leaves the sheets out by the flag, "base" has no sheets at all (offsetE = 0)
COMBOS = {"both": (True, True), "local": (True, False), "global": (False, True), "base": (True, True)}


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_matrix(w, res, what):
    rp, ci, v = mr.csr(res)
    wrp, wci, wv = w.csr_dense()
    assert np.array_equal(wrp, rp) and np.array_equal(wci, ci), (what, "structure")
    assert np.array_equal(bits(wv), bits(v)), (what, "values", int(np.sum(bits(wv) != bits(v))), len(v))
    assert np.array_equal(bits(w.wM), bits(res["wM"])), (what, "wM")
    assert np.array_equal(bits(w.Mw), bits(res["Mw"])), (what, "Mw")
    for k in (0, 1):
        assert np.array_equal(w.dim(k), np.asarray(res["dims"][k], np.int64)), (what, "dims", k)
        assert w.sparse_extent(k) == res["extents"][k], (what, "extent", k, w.sparse_extent(k), res["extents"][k])


def same_merge(r, res, what):
    same_matrix(r.EOpvAOp, res, what)
    assert np.array_equal(r.dimEOp.to_sparse(), np.asarray(res["dims"][0], np.int64)) and r.dimEOp.sparse_extent() == res["extents"][0], what
    assert np.array_equal(r.dimAOp.to_sparse(), np.asarray(res["dims"][1], np.int64)) and r.dimAOp.sparse_extent() == res["extents"][1], what
    assert (r.EOpvAOp.conservative, r.EOpvAOp.scaled) == (False, False), what
    assert r.offsetE == res["offsetE"] and tuple(r.indexingHC) == tuple(res["strides"]), (what, r.offsetE, r.indexingHC)
    assert np.array_equal(bits(r.hcdefs), bits(res["hcdefs"])) and r.underice_hc.tolist() == res["underice"], what


def same_AvE(w, res, what):
    same_matrix(w, res, what)
    assert (w.conservative, w.scaled) == (res["conservative"], res["scaled"]), (what, "flags")


class F1:
    """Two sheets in ONE GCMRegridder whose every O cell is realised; the exchange grids come from the Hntr exchange-grid
    builder on the device, and the oracle twins are fed the same arrays."""

    def __init__(self):
        from icebin_amd import GCMRegridder, global_ec
        from oracle import oracle as orc
        self.orc = orc
        self.O, self.Is = gc.specs()
        self.ems = gc.masks()
        allO = np.arange(self.O.size, dtype=np.int64)
        nat = global_ec.native_area(self.O, allO, R)
        self.gcm = GCMRegridder(dict(nA=self.O.size, to_sparse=allO, native_area=nat), gc.HC, True)
        self.grids = []
        for k, (I, em) in enumerate(zip(self.Is, self.ems)):
            idx, area = global_ec.gcm_from_hntr(self.O, I, em, gc.HC, True, R).exgrid()
            idx, area = idx.copy(), area.copy()
            self.gcm.add_sheet("sheet%d" % k, dict(nI=I.size), dict(indices=idx, overlaps=area))
            self.grids.append(dict(nA=self.O.size, nI=I.size, nhc=3, hcdefs=np.asarray(gc.HC), hc_stride_A=1, hc_stride_HC=self.O.size,
                                   ex_indices=idx, ex_area=area, A_to_sparse=allO, A_native_area=nat, A_proj_area=nat, interp_style=0))
        self.rgs = [orc.Regridder(g) for g in self.grids]
        ice = gc.ice_cells(self.grids)
        self.ice, self.both = np.union1d(ice[0], ice[1]), np.intersect1d(ice[0], ice[1])
        self.kids = gc.ocean("zero", self.both, self.O)[2]
        self.bases = {n: gc.base(self.ice, self.kids, self.O, n) for n in (2, 72)}
        hc1, (iE, iO, val), _ = self.bases[2]
        one = iE < self.O.size                       # the entries of class 0 alone: a base with one class
        self.bases[1] = (hc1[:1], (iE[one], iO[one], val[one]), (self.O.size, self.O.size))
        # the fixture's premises (CPU): an O cell with ice of both sheets in one class; cells outside every sheet
        rows = []
        for rg, em in zip(self.rgs, self.ems):
            dE = orc.SparseSet()
            rg.matrix_d("EvA", em, dims=(dE, orc.SparseSet()), scale=False, correctA=False)
            rows.append(set(dE.to_sparse().tolist()))
        assert rows[0] & rows[1] and len(np.setdiff1d(allO, self.ice)) >= 4
        self._dev, self._ref = {}, {}

    def rmOs(self, ems=None):
        ems = self.ems if ems is None else ems
        return [self.gcm.regrid_matrices("sheet%d" % k, em) for k, em in enumerate(ems)]

    def merged(self, nbase=2, combo="both", squash=False):
        """(device result, restatement) of one merge, built once."""
        from icebin_amd import compute_EOpvAOp_merged
        key = (nbase, combo, squash)
        if key not in self._dev:
            ul, ug = COMBOS[combo]
            rmOs, sheets = (self.rmOs(), list(zip(self.rgs, self.ems))) if combo != "base" else ([], [])
            self._dev[key] = compute_EOpvAOp_merged(rmOs, self.bases[nbase], use_global_ice=ug, use_local_ice=ul, squash_ecs=squash)
            self._ref[key] = gr.merged(self.orc, sheets, self.O.size, 3 if sheets else 0, gc.HC if sheets else [], self.bases[nbase],
                                       use_global_ice=ug, use_local_ice=ul, squash_ecs=squash)
        return self._dev[key], self._ref[key]


@pytest.fixture(scope="module")
def f1():
    return F1()


# squash_ECs after a merge of the base alone is left out while there are sheets: its row keys start at offsetE = nO * nhc_local,
# classes the merged hcdefs do not have (test_squash_refuses_classes_outside_hcdefs)
MERGES = [(nbase, combo, squash) for nbase in (1, 2, 72) for combo in COMBOS for squash in (False, True) if not (combo == "global" and squash)]


@pytest.mark.parametrize("nbase,combo,squash", MERGES)
def test_merge_bitwise(f1, nbase, combo, squash):
    r, res = f1.merged(nbase, combo, squash)
    same_merge(r, res, (nbase, combo, squash))
    assert r.EOpvAOp.nnz > (5 if combo in ("global", "base") else 50)
    if combo == "both" and not squash:
        assert len(res["hcdefs"]) == 3 + nbase and r.nhc == 3 + nbase and r.offsetE == 3 * f1.O.size


@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("pattern", gc.PATTERNS)
def test_AAmvEAm_bitwise_every_ocean_pattern(f1, pattern, scale):
    from icebin_amd import compute_AAmvEAm
    fp, fm, _ = gc.ocean(pattern, f1.both, f1.O)
    r, res = f1.merged()
    w = compute_AAmvEAm(r, f1.O, R, fp, fm, scale=scale)
    same_AvE(w, gr.AAmvEAm(res, f1.O, R, fp, fm, triplets_ref, scale=scale), (pattern, scale))
    assert w.nnz >= 30


def test_squash_refuses_classes_outside_hcdefs(f1):
    """use_local_ice = false with sheets present: the base's rows sit at offsetE = nO * 3 and name classes 3.. of an hcdefs that
    holds the base's alone.  The reference indexes to_new out of bounds there; here it is IBH_EINVAL, the sets untouched."""
    from icebin_amd import SparseSet, _capi, compute_EOpvAOp_merged
    dimAOp = SparseSet(-1, [5])
    with pytest.raises(_capi.IcebinHipError, match="squash_ECs: rows") as ei:
        compute_EOpvAOp_merged(f1.rmOs(), f1.bases[2], use_local_ice=False, squash_ecs=True, dimAOp=dimAOp)
    assert ei.value.code == _capi.IBH_EINVAL and dimAOp.to_sparse().tolist() == [5] and dimAOp.sparse_extent() == -1
    with pytest.raises(IndexError):
        gr.merged(f1.orc, list(zip(f1.rgs, f1.ems)), f1.O.size, 3, gc.HC, f1.bases[2], use_local_ice=False, squash_ecs=True)


@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("combo,nbase,squash", [("both", 2, False), ("both", 2, True), ("local", 2, False), ("local", 2, True),
                                                ("base", 2, False), ("base", 2, True), ("base", 1, False), ("both", 72, False),
                                                ("both", 72, True)])
def test_AAmvEAm_bitwise_every_merge(f1, combo, nbase, squash, scale):
    """The base alone with one class has rows of at most 4 terms (the product's thread-per-row emit form), the full merge its
    wave form; with 72 base classes one O cell carries 75 rows of EOmvAOm, so a row of AOmvEOm takes a wave two passes."""
    from icebin_amd import compute_AAmvEAm
    fp, fm, _ = gc.ocean("om2", f1.both, f1.O)
    r, res = f1.merged(nbase, combo, squash)
    parts = {}
    want = gr.AAmvEAm(res, f1.O, R, fp, fm, triplets_ref, scale=scale, parts=parts)
    terms = [len(row) for row in parts["P1"]]
    if (combo, nbase) == ("base", 1):
        assert max(terms) <= 4
    if nbase == 72:
        assert max(terms) > 64
    same_AvE(compute_AAmvEAm(r, f1.O, R, fp, fm, scale=scale), want, (combo, nbase, squash, scale))


def test_prepopulated_sets(f1):
    """dimAOp, dimAAm and dimEAm that hold keys already (permuted, incomplete): the builds append behind them."""
    from icebin_amd import SparseSet, compute_AAmvEAm, compute_EOpvAOp_merged
    _, res0 = f1.merged()
    preO = [int(k) for k in res0["dims"][1][::-2]]
    preO.append(max(set(range(48)) - set(res0["dims"][1])))         # and a cell the merge never meets
    dimAOp = SparseSet(-1, preO)
    r = compute_EOpvAOp_merged(f1.rmOs(), f1.bases[2], dimAOp=dimAOp)
    res = gr.merged(f1.orc, list(zip(f1.rgs, f1.ems)), f1.O.size, 3, gc.HC, f1.bases[2], dimAOp=preO)
    same_merge(r, res, "pre-populated dimAOp")
    assert r.dimAOp is dimAOp and dimAOp.to_sparse().tolist()[:len(preO)] == preO
    fp, fm, _ = gc.ocean("om1", f1.both, f1.O)
    full = gr.AAmvEAm(res, f1.O, R, fp, fm, triplets_ref)
    preA, preE = [int(k) for k in full["dims"][0][::-3]], [int(k) for k in full["dims"][1][::-2]]
    preE.append(max(set(range(60)) - set(full["dims"][1].tolist())))
    dA, dE = SparseSet(-1, preA), SparseSet(-1, preE)
    w = compute_AAmvEAm(r, f1.O, R, fp, fm, dims=(dA, dE))
    same_AvE(w, gr.AAmvEAm(res, f1.O, R, fp, fm, triplets_ref, dimAAm=preA, dimEAm=preE), "pre-populated dimAAm, dimEAm")
    assert dA.to_sparse().tolist()[:len(preA)] == preA and dE.to_sparse().tolist()[:len(preE)] == preE
    assert dA.sparse_extent() == 12 and dE.sparse_extent() == 12 * 5


def test_empty_sheet_and_no_sheet(f1):
    from icebin_amd import compute_AAmvEAm, compute_EOpvAOp_merged
    fp, fm, _ = gc.ocean("frac", f1.both, f1.O)
    # one sheet whose mask is all NaN: an empty EvA between the other sheet and the base
    ems = [f1.ems[0], np.full(f1.Is[1].size, np.nan)]
    r = compute_EOpvAOp_merged(f1.rmOs(ems), f1.bases[2])
    res = gr.merged(f1.orc, list(zip(f1.rgs, ems)), f1.O.size, 3, gc.HC, f1.bases[2])
    same_merge(r, res, "empty sheet")
    same_AvE(compute_AAmvEAm(r, f1.O, R, fp, fm), gr.AAmvEAm(res, f1.O, R, fp, fm, triplets_ref), "empty sheet")
    # no sheet at all: the base alone, offsetE = 0
    r = compute_EOpvAOp_merged([], f1.bases[2])
    res = gr.merged(f1.orc, [], f1.O.size, 0, [], f1.bases[2])
    same_merge(r, res, "no sheet")
    assert r.offsetE == 0 and r.nhc == 2
    same_AvE(compute_AAmvEAm(r, f1.O, R, fp, fm, scale=False), gr.AAmvEAm(res, f1.O, R, fp, fm, triplets_ref, scale=False), "no sheet")


def test_nhc_local_drops_every_base_class(f1):
    """The low-level entry takes nhc explicitly: with nhc = nhc_local (what the snapshot's global_AvE passes) no base class survives."""
    from icebin_amd import compute_AAmvEAm
    fp, fm, _ = gc.ocean("om1", f1.both, f1.O)
    r, res = f1.merged()
    w = compute_AAmvEAm(r, f1.O, R, fp, fm, nhc=3)
    same_AvE(w, gr.AAmvEAm(res, f1.O, R, fp, fm, triplets_ref, nhc=3), "nhc = nhc_local")
    assert w.dim(1).max() // 12 <= 2 and w.sparse_extent(1) == 36


def test_global_AvE_is_the_two_calls(f1):
    from icebin_amd import compute_AAmvEAm
    fp, fm, _ = gc.ocean("om2", f1.both, f1.O)
    m = f1.gcm.to_modele((fp, fm), hspecO=f1.O, eq_rad=R, global_ec=f1.bases[2])
    assert np.array_equal(m.hcdefs, [0., 1500., 3000., 1500., 4000.]) and [m.underice(k) for k in range(5)] == [1, 1, 1, 2, 2]
    with pytest.raises(NotImplementedError):
        m.wA("sheet0", "native")
    r, res = f1.merged()
    for scale in (True, False):
        w, offsetE = m.global_AvE(None, f1.ems, fp, fm, scale=scale)
        assert offsetE == r.offsetE == 3 * f1.O.size
        two = compute_AAmvEAm(r, f1.O, R, fp, fm, scale=scale)
        for a, b in zip(w.csr_dense() + (w.wM, w.Mw, w.dim(0), w.dim(1)), two.csr_dense() + (two.wM, two.Mw, two.dim(0), two.dim(1))):
            assert a.tobytes() == b.tobytes()
        same_AvE(w, gr.AAmvEAm(res, f1.O, R, fp, fm, triplets_ref, scale=scale), ("global_AvE", scale))
    # to_coo / get_weights: the reference's to_tuple form, in sparse indices
    coo = w.to_coo()
    assert coo.shape == (12, 60) and coo.nnz == w.nnz and w.get_weights(0).shape == (12,) and w.get_weights(1).shape == (60,)


def test_scaled_result_maps_one_to_one(f1):
    """apply_M of the scaled AAmvEAm takes the constant 1 over E to 1 over every atmosphere cell it reaches."""
    from icebin_amd import compute_AAmvEAm
    fp, fm, _ = gc.ocean("frac", f1.both, f1.O)
    r, _ = f1.merged()
    w = compute_AAmvEAm(r, f1.O, R, fp, fm, scale=True)
    y = w.apply_M(np.ones(w.sparse_extent(1)), fill=np.nan, force_conservation=False)
    reached = w.dim(0)
    assert len(reached) >= 8 and np.all(np.isnan(np.delete(y, reached)))
    dev = np.max(np.abs(y[reached] - 1.))
    print("apply_M(1): largest deviation from 1 %.3e" % dev)
    assert dev <= allowed(MEASURED_ROWSUM), dev


def test_g50_under_the_144x90_ocean():
    """The synthetic Greenland sheet with global_ec's own EvA of a second mask (scale = false, correctA = true) as the base."""
    from icebin_amd import HntrSpec, compute_AAmvEAm, compute_EOpvAOp_merged, from_synthetic, synthetic
    from oracle import oracle as orc
    g = synthetic.make_grids("g50")
    em = synthetic.dome_elevmask(g)
    em2 = np.where(np.random.default_rng(4).random(len(em)) < 0.5, np.nan, em * 0.8)
    gcm, rg = from_synthetic(g), orc.Regridder(g)
    O = HntrSpec(144, 90, 0., 120.)
    EvA = gcm.regrid_matrices("greenland", em2, scale=False, correctA=True).matrix_d("EvA", scale=False, correctA=True)
    coo = EvA.to_coo()
    base = (np.asarray(g["hcdefs"], np.float64), (coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data), coo.shape)
    strides = (int(g["hc_stride_A"]), int(g["hc_stride_HC"]))
    assert strides == (1, O.size) and coo.shape == (O.size * len(g["hcdefs"]), O.size)
    r = compute_EOpvAOp_merged([gcm.regrid_matrices("greenland", em)], base)
    res = gr.merged(orc, [(rg, em)], O.size, len(g["hcdefs"]), g["hcdefs"], base)
    same_merge(r, res, "g50")
    ice = np.unique(np.asarray(res["dims"][1]))
    fp, fm = np.zeros(O.size), np.zeros(O.size)
    fp[ice[::4]] = 0.3
    fm[ice[1::7]] = fp[ice[1::7]] = 1.
    for scale in (True, False):
        same_AvE(compute_AAmvEAm(r, O, R, fp, fm, scale=scale), gr.AAmvEAm(res, O, R, fp, fm, triplets_ref, scale=scale), ("g50", scale))


def test_errors_leave_the_sets_alone(f1):
    from icebin_amd import SparseSet, _capi, compute_AAmvEAm, compute_EOpvAOp_merged
    hc, (iE, iO, val), shape = f1.bases[2]
    # a base index outside its shape, named
    badE = iE.copy()
    badE[5] = shape[0]
    dimAOp = SparseSet(-1, [3, 1])
    for base, what in (((hc, (badE, iO, val), shape), r"base entry 5 = \(%d, %d\)" % (shape[0], iO[5])),
                       ((hc, (iE, iO, val), (shape[0], shape[1] + 2)), "nO=48")):       # a base on another ocean grid
        with pytest.raises(_capi.IcebinHipError, match=what) as ei:
            compute_EOpvAOp_merged(f1.rmOs(), base, dimAOp=dimAOp, nO=f1.O.size)
        assert ei.value.code == _capi.IBH_EINVAL
        assert dimAOp.to_sparse().tolist() == [3, 1] and dimAOp.sparse_extent() == -1
    # sheets on an ocean grid of another size
    with pytest.raises(_capi.IcebinHipError, match="sheet 0 lives on an ocean grid of 48 cells") as ei:
        compute_EOpvAOp_merged(f1.rmOs(), None, dimAOp=dimAOp, nO=50)
    assert ei.value.code == _capi.IBH_EINVAL and dimAOp.to_sparse().tolist() == [3, 1]
    # fcont_m neither 0 nor 1 on an ice-bearing cell
    r, _ = f1.merged()
    fp, fm, _ = gc.ocean("zero", f1.both, f1.O)
    bad = int(f1.both[3])
    fm[bad] = 0.25
    dA, dE = SparseSet(-1, [2, 0]), SparseSet()
    with pytest.raises(_capi.IcebinHipError, match=r"fcont_m\[%d\] = 0.75" % bad) as ei:
        compute_AAmvEAm(r, f1.O, R, fp, fm, dims=(dA, dE))
    assert ei.value.code == _capi.IBH_EINVAL
    assert dA.to_sparse().tolist() == [2, 0] and dA.sparse_extent() == -1 and dE.dense_extent() == 0 and dE.sparse_extent() == -1
    with pytest.raises(_capi.IcebinHipError, match="sparse extent") as ei:
        compute_AAmvEAm(r, f1.O, R, np.zeros(48), np.zeros(48), dims=(SparseSet(7), None))
    assert ei.value.code == _capi.IBH_EINVAL
