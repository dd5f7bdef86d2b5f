"""Parity of the HIP path (through the C-ABI) against the CPU oracle, on a real MI355X.

Bar: dims / CSR structure / wM / Mw / M bit-exact; regridded fp64 fields within
1e-12 relative L-inf; conservation residual < 1e-13."""
import math

import numpy as np
import pytest

import os
import sys

import icebin_amd
from icebin_amd import synthetic as syn
from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import smoothing_cases as smc
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

ALL = ("AvI", "IvA", "AvX", "XvA", "EvI", "IvE", "EvX", "XvE", "EvA", "AvE")
FIELD_RTOL = 1e-12        # relative L-inf tolerance for regridded fields (BASELINE.json north_star)


def rel_linf(a, b):
    m = np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return np.max(np.abs(a[m] - b[m])) / max(np.max(np.abs(b[m])), 1e-300)


def assert_same_weighted(w, o, name=""):
    assert (w.nrow_d, w.ncol_d, w.nnz) == (o.nrow, o.ncol, o.nnz), name
    assert w.conservative == o.conservative and w.scaled == o.scaled
    np.testing.assert_array_equal(w.dim(0), o.dims[0], err_msg=name + " dims[0]")
    np.testing.assert_array_equal(w.dim(1), o.dims[1], err_msg=name + " dims[1]")
    assert w.shape == (o.sparse_extents[0], o.sparse_extents[1])
    row, col, val = w.coo_dense()
    np.testing.assert_array_equal(row, o.row, err_msg=name + " row")
    np.testing.assert_array_equal(col, o.col, err_msg=name + " col")
    # bit-exact, not merely close: compare the raw 64-bit patterns
    np.testing.assert_array_equal(val.view(np.uint64), o.val.view(np.uint64), err_msg=name + " M")
    np.testing.assert_array_equal(w.wM.view(np.uint64), o.wM.view(np.uint64), err_msg=name + " wM")
    np.testing.assert_array_equal(w.Mw.view(np.uint64), o.Mw.view(np.uint64), err_msg=name + " Mw")


def setup(config, **kw):
    g = syn.make_grids(config, **kw)
    em = syn.dome_elevmask(g)
    return g, em, icebin_amd.from_synthetic(g), orc.Regridder(g)


@pytest.mark.parametrize("variant", ["sorted", "shuffled", "zero_area", "negative_area", "elev_class"])
def test_assembly_bit_exact_all_matrices(variant):
    kw = {}
    if variant == "shuffled":
        kw["order"] = "shuffled"
    if variant == "zero_area":
        kw["zero_area_every"] = 7
    g = syn.make_grids("g50", **kw)
    if variant == "negative_area":
        g["ex_area"] = g["ex_area"].copy()
        g["ex_area"][::11] *= -1.0
    if variant == "elev_class":
        g["interp_style"] = 1
    em = syn.dome_elevmask(g)
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    rm = mm.regrid_matrices("greenland", em)
    for name in ALL:
        for scale in (True, False):
            for correctA in (True, False):
                w = rm.matrix_d(name, scale=scale, correctA=correctA)
                o = rg.matrix_d(name, em, scale=scale, correctA=correctA)
                assert_same_weighted(w, o, "%s scale=%d correctA=%d %s" % (name, scale, correctA, variant))


@pytest.mark.parametrize("config", ["g50", "g20"])
def test_fast_and_general_assembly_paths_agree_with_the_oracle(config):
    # sorted exchange grids take the plan-based fast path (fastasm.inl) for the A/E-row, I/X-row and EvA/AvE families; the
    # general pipeline (forced with assemble_fast=0) must give the same bits.  Own dims, identity I / X dims, and the
    # coupler's shared dimE (IceCoupler.cpp:361-468).
    g, em, mm, rg = setup(config)
    nI, nX, nE = g["nI"], len(g["ex_area"]), g["nA"] * len(g["hcdefs"])
    try:
        for fast in (1, 0):
            icebin_amd.set_tuning("assemble_fast", fast)
            for scale, correctA in ((True, True), (False, False), (True, False), (False, True)):
                rm = mm.regrid_matrices("greenland", em, scale=scale, correctA=correctA)
                for name in ALL:
                    w = rm.matrix(name)
                    assert w.built_fast() == bool(fast), (name, fast)          # EvA / AvE too (fresh sets: fast_build_eva)
                    assert_same_weighted(w, rg.matrix_d(name, em, scale=scale, correctA=correctA), "%s fast=%d" % (name, fast))
            # the coupler's step: EvI / AvI with identity dimI, then IvE / XvE on the dimE that EvI numbered
            rm = mm.regrid_matrices("greenland", em)
            dimI, dimX, dimE = icebin_amd.SparseSet.identity(nI), icebin_amd.SparseSet.identity(nX), icebin_amd.SparseSet(nE)
            oI, oX, oE = orc.SparseSet(nI, init=np.arange(nI)), orc.SparseSet(nX, init=np.arange(nX)), orc.SparseSet(nE)
            for name, dims, odims, sc, cA in (("EvI", (dimE, dimI), (oE, oI), False, False), ("AvI", (None, dimI), (None, oI), False, True),
                                              ("IvE", (dimI, dimE), (oI, oE), True, True), ("XvE", (dimX, dimE), (oX, oE), False, True)):
                w = rm.matrix_d(name, dims, scale=sc, correctA=cA)
                assert w.built_fast() == bool(fast), (name, fast)
                assert_same_weighted(w, rg.matrix_d(name, em, dims=odims, scale=sc, correctA=cA), "coupler %s fast=%d" % (name, fast))
            # a shared dimE that numbers the classes in some OTHER order (and holds keys this mask never touches): the
            # rows' columns are no longer ascending in visiting order -> the per-row selection branch of the fast path
            E_keys = dimE.to_sparse()
            extra = np.setdiff1d(np.arange(nE), E_keys)[:7]
            perm = np.random.default_rng(5).permutation(np.concatenate([E_keys, extra]))
            for name, rowset, orow in (("IvE", dimI, oI), ("XvE", dimX, oX)):
                dE2, oE2 = icebin_amd.SparseSet(nE, perm), orc.SparseSet(nE, init=perm)
                w = rm.matrix_d(name, (rowset, dE2), scale=True, correctA=True)
                assert w.built_fast() == bool(fast)
                assert_same_weighted(w, rg.matrix_d(name, em, dims=(orow, oE2), scale=True, correctA=True), "permuted dimE %s fast=%d" % (name, fast))
            # ... and one that lacks a key: the fast path hands over to the general pipeline, which appends it
            dE3, oE3 = icebin_amd.SparseSet(nE, E_keys[:-3]), orc.SparseSet(nE, init=E_keys[:-3])
            w = rm.matrix_d("IvE", (dimI, dE3), scale=True, correctA=True)
            assert not w.built_fast() and dE3.dense_extent() == len(E_keys)
            assert_same_weighted(w, rg.matrix_d("IvE", em, dims=(oI, oE3), scale=True, correctA=True), "incomplete dimE")
    finally:
        icebin_amd.set_tuning("assemble_fast", 1)


@pytest.mark.parametrize("config,kw", [("g5", {}), ("g20", {}), ("g20", dict(x_fastest=True))])
def test_fused_pair_evi_then_ave_is_the_two_applies(config, kw, rowgroup_form):
    """ibh_weighted_apply_pair_device: E = EvI * I and A = AvE * E in one launch (BASELINE config 3's chain) against the two
    separate applies and the oracle: B1 bitwise the EvI apply, B2 within 1e-12 of AvE applied to it; NaN fields, fill for rows
    without weight, 1..40 fields, matrices with their own dims (different numberings of E: paired through sparse indices) and
    with a shared dimE; graph capture; matrices that do not pair are refused."""
    import torch
    g = syn.make_grids(config, **kw)
    em = syn.dome_elevmask(g)
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    nE = g["nA"] * len(g["hcdefs"])
    for shared in (False, True):
        if shared:
            dimE = icebin_amd.SparseSet(nE)
            EvI = rm.matrix_d("EvI", (dimE, None), scale=True, correctA=True)
            AvE = rm.matrix_d("AvE", (None, dimE), scale=True, correctA=True)
        else:
            EvI, AvE = rm.matrix("EvI"), rm.matrix("AvE")
        oE, oA = rg.matrix_d("EvI", em, scale=True, correctA=True), rg.matrix_d("AvE", em, scale=True, correctA=True)
        EvI.pair_prepare(AvE, 16)
        for nvar in (16, 1, 7, 40):
            x = torch.from_numpy(syn.fields(nvar, EvI.ncol_d, seed=90 + nvar)).cuda()
            x[nvar // 2, ::9] = float("nan")
            EvI.set_kernel("rowgroup")
            e_sep = EvI.apply_device(x, fill=-1.0, force_conservation=False).clone()
            EvI.set_kernel("auto")
            perm = np.argsort(EvI.dim(0))[np.searchsorted(np.sort(EvI.dim(0)), AvE.dim(1))]        # AvE's column order of E
            a_sep = AvE.apply_device(e_sep[:, torch.from_numpy(perm).cuda()].contiguous(), fill=-1.0, force_conservation=False)
            b1, b2 = EvI.apply_pair_device(AvE, x, fill=-1.0)
            torch.cuda.synchronize()
            assert EvI.last_kernel() == "rowgroup"
            assert np.array_equal(b1.cpu().numpy().view(np.uint64), e_sep.cpu().numpy().view(np.uint64)), (config, shared, nvar)
            assert rel_linf(b2.cpu().numpy(), a_sep.cpu().numpy()) <= FIELD_RTOL, (config, shared, nvar)
            # ... and the oracle's two applies
            ref_e = oE.apply(x.cpu().numpy(), fill=-1.0, force_conservation=False)
            operm = np.argsort(oE.dims[0])[np.searchsorted(np.sort(oE.dims[0]), oA.dims[1])]
            ref_a = oA.apply(ref_e[:, operm], fill=-1.0, force_conservation=False)
            order_a = np.argsort(AvE.dim(0))[np.searchsorted(np.sort(AvE.dim(0)), oA.dims[0])]
            assert rel_linf(b2.cpu().numpy()[:, order_a], ref_a) <= FIELD_RTOL, (config, shared, nvar)
        # the chain of BASELINE config 3 in one call: the pair, then IvA on its result -- bitwise the pair apply followed by the
        # IvA apply, call after call into the same outputs (new inputs every call; the outputs poisoned with NaN before it)
        if not shared:
            IvA = rm.matrix("IvA")
            permA = np.argsort(AvE.dim(0))[np.searchsorted(np.sort(AvE.dim(0)), IvA.dim(1))]
            assert np.array_equal(permA, np.arange(len(permA)))      # (both numbered by first sight of the GCM cells: the same order)
            for nvar in (16, 3, 40):
                out1, out2, out3 = (torch.empty((nvar, n), dtype=torch.float64, device="cuda") for n in (EvI.nrow_d, AvE.nrow_d, IvA.nrow_d))
                for rep in range(3):
                    x = torch.from_numpy(syn.fields(nvar, EvI.ncol_d, seed=70 + 3 * nvar + rep)).cuda()
                    x[(nvar // 2 + rep) % nvar, rep::9] = float("nan")
                    b1, b2 = EvI.apply_pair_device(AvE, x, fill=-1.0)
                    b3 = IvA.apply_device(b2, fill=-1.0, force_conservation=False)
                    for o in (out1, out2, out3):
                        o.fill_(float("nan"))
                    c1, c2, c3 = EvI.apply_chain_device(AvE, IvA, x, out1=out1, out2=out2, out3=out3, fill=-1.0)
                    torch.cuda.synchronize()
                    assert c1 is out1 and c2 is out2 and c3 is out3
                    for a, b in ((c1, b1), (c2, b2), (c3, b3)):
                        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (config, nvar, rep)
        # inside a hipGraph
        x = torch.from_numpy(syn.fields(16, EvI.ncol_d, seed=5)).cuda()
        o1, o2 = EvI.apply_pair_device(AvE, x, fill=-1.0)
        keep1, keep2 = o1.clone(), o2.clone()
        o1.zero_(); o2.zero_()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            EvI.apply_pair_device(AvE, x, out1=o1, out2=o2, fill=-1.0)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(o1.view(torch.int64), keep1.view(torch.int64)) and torch.equal(o2.view(torch.int64), keep2.view(torch.int64))
    # matrices that do not pair: IvE's rows are ice cells (no row groups); AvI after EvI reads ice cells, not classes
    with pytest.raises(icebin_amd.IcebinHipError):
        rm.matrix("IvE").pair_prepare(rm.matrix("AvE"))
    with pytest.raises(icebin_amd.IcebinHipError):
        rm.matrix("EvI").pair_prepare(rm.matrix("AvI"))
    with pytest.raises(icebin_amd.IcebinHipError, match="pair_prepare"):
        a, b = rm.matrix("EvI"), rm.matrix("AvE")
        a.apply_pair_device(b, torch.zeros((2, a.ncol_d), dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("shape", [0, 1, 2, 3])
def test_assembly_range_kernel_shapes_are_bit_identical(shape):
    # the per-range kernels of the plan-based build exist in four workgroup shapes (128 x 2, 256 x 4, 1024 x 4, 1024 x 1 cells per
    # pass, chosen by the size and number of the ranges: fastasm.inl fa_range_shape); every shape must give the oracle's bits --
    # ranges shorter and longer than one pass (g50: ~20 cells, g5: ~720, up to ~1 500), duplicates, zero areas, both interpolation styles
    try:
        icebin_amd.set_tuning("assemble_range_shape", shape)
        # (shape 1 also with the row counts of the I-row builds taken by VISITING the exchange cells instead of from the plan's
        # static per-ice-cell counts: the path a grid with underflow-sized areas takes)
        icebin_amd.set_tuning("assemble_static_count", 0 if shape == 1 else 1)
        # (shape 2 also with the STREAMED count of the one-class matrices -- k_fa_count_stream, the default from 2^20 exchange
        # cells on -- forced on these small grids)
        icebin_amd.set_tuning("assemble_stream_count", 1 if shape == 2 else -2 ** 31)
        for config, kw, style in (("g50", {}, 0), ("g50", dict(zero_area_every=7), 0), ("g50", {}, 1), ("g20", {}, 0)):
            g = syn.make_grids(config, **kw)
            g["interp_style"] = style
            em = syn.dome_elevmask(g)
            mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
            for scale, correctA in ((True, True), (False, False)):
                rm = mm.regrid_matrices("greenland", em, scale=scale, correctA=correctA)
                for name in ALL:
                    w = rm.matrix(name)
                    assert w.built_fast(), name
                    assert_same_weighted(w, rg.matrix_d(name, em, scale=scale, correctA=correctA), "%s shape=%d %s" % (name, shape, config))
        # 5 km: ranges of ~1 500 cells (several passes of the small shapes), against the default shape's bits
        g = syn.make_grids("g5")
        em = syn.dome_elevmask(g)
        rm = icebin_amd.from_synthetic(g).regrid_matrices("greenland", em, scale=True, correctA=True)
        for name in ("AvI", "IvA", "EvI", "IvE", "EvA", "XvE"):
            icebin_amd.set_tuning("assemble_range_shape", shape)
            w = rm.matrix(name)
            icebin_amd.set_tuning("assemble_range_shape", 1)
            w1 = rm.matrix(name)
            assert np.array_equal(w.dim(0), w1.dim(0)) and np.array_equal(w.dim(1), w1.dim(1)), name
            for a, b in zip(w.csr_dense() + (w.wM, w.Mw), w1.csr_dense() + (w1.wM, w1.Mw)):
                assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), name
    finally:
        icebin_amd.set_tuning("assemble_range_shape", -1)
        icebin_amd.set_tuning("assemble_static_count", 1)
        icebin_amd.set_tuning("assemble_stream_count", -2 ** 31)


@pytest.mark.parametrize("fast", [1, 0])
def test_matrix_batch_equals_sequential_builds(fast):
    # ibh_regrid_matrices_matrix_batch: the coupler's per-step set (IceCoupler.cpp:361-468) in one call; independent builds
    # run concurrently on the library's worker threads.  Results (matrices AND dims) are those of matrix_d calls in order.
    g, em, mm, rg = setup("g20")
    nI, nX, nE = g["nI"], len(g["ex_area"]), g["nA"] * len(g["hcdefs"])
    try:
        icebin_amd.set_tuning("assemble_fast", fast)
        rm = mm.regrid_matrices("greenland", em)
        for rep in range(3):            # repeated steps reuse the worker threads and their workspaces
            dimI, dimX, dimE, dimA = (icebin_amd.SparseSet.identity(nI), icebin_amd.SparseSet.identity(nX), icebin_amd.SparseSet(nE),
                                      icebin_amd.SparseSet(g["nA"]))
            jobs = [("EvI", (dimE, dimI), False, False), ("AvI", (dimA, dimI), False, True), ("IvE", (dimI, dimE), True, True),
                    ("XvE", (dimX, dimE), False, True), ("EvA", (dimE, dimA), True, True), ("IvA", (None, None), True, False)]
            ws = rm.matrix_batch(jobs)
            oI, oX, oE, oA = (orc.SparseSet(nI, init=np.arange(nI)), orc.SparseSet(nX, init=np.arange(nX)), orc.SparseSet(nE),
                              orc.SparseSet(g["nA"]))
            odims = [(oE, oI), (oA, oI), (oI, oE), (oX, oE), (oE, oA), (None, None)]
            for (name, _, sc, cA), od, w in zip(jobs, odims, ws):
                assert_same_weighted(w, rg.matrix_d(name, em, dims=od, scale=sc, correctA=cA), "batch %s fast=%d" % (name, fast))
                if fast:
                    assert w.built_fast() == (name != "EvA")
            assert np.array_equal(dimE.to_sparse(), ws[0].dim(0)) and np.array_equal(dimA.to_sparse(), ws[1].dim(0))
        # a shared set that lacks a key: the concurrent fast-only attempt declines, the job is redone by the general pipeline
        # (which appends), and the later job that shares the set is redone after it -- sequential semantics
        E_keys = ws[0].dim(0)
        dE3, oE3 = icebin_amd.SparseSet(nE, E_keys[:-3]), orc.SparseSet(nE, init=E_keys[:-3])
        dI2, dX2 = icebin_amd.SparseSet.identity(nI), icebin_amd.SparseSet.identity(nX)
        w1, w2 = rm.matrix_batch([("IvE", (dI2, dE3), True, True), ("XvE", (dX2, dE3), False, True)])
        assert_same_weighted(w1, rg.matrix_d("IvE", em, dims=(orc.SparseSet(nI, init=np.arange(nI)), oE3), scale=True, correctA=True), "redo IvE")
        assert_same_weighted(w2, rg.matrix_d("XvE", em, dims=(orc.SparseSet(nX, init=np.arange(nX)), oE3), scale=False, correctA=True), "redo XvE")
        assert dE3.dense_extent() == len(E_keys)
        # an error in one job: nothing is returned, the message is the job's
        with pytest.raises(icebin_amd.IcebinHipError, match="unknown regrid matrix 'BvA'"):
            rm.matrix_batch([("AvI", (None, None), True, True), ("BvA", (None, None), True, True)])
        assert rm.matrix_batch([]) == []
    finally:
        icebin_amd.set_tuning("assemble_fast", 1)


def test_config1_real_mask_bit_exact(elev_mask_g20):
    # BASELINE config 1: 20 km Greenland, the reference's own PISM mask fixture, all six matrices
    g = syn.make_grids("g20")
    _, em = orc.elevmask_pism(elev_mask_g20["mask"], elev_mask_g20["thk"], elev_mask_g20["topg"])
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    for name in ("AvI", "IvA", "EvI", "IvE", "EvA", "AvE"):
        assert_same_weighted(rm.matrix(name), rg.matrix_d(name, em, scale=True, correctA=True), name)
    # Python default correctA=True (_icebin.pyx:165) vs C++ default false (RegridMatrices.hpp:33)
    rm2 = mm.regrid_matrices("greenland", em)
    assert_same_weighted(rm2.matrix("AvI"), rg.matrix_d("AvI", em, scale=True, correctA=True))


def test_prepopulated_and_shared_dims():
    # IceCoupler.cpp:366-371,462,467: identity dimI, one dimE shared by EvI / IvE / XvE
    g, em, mm, rg = setup("g50")
    rm = mm.regrid_matrices("greenland", em)
    dimI, dimE = icebin_amd.SparseSet.identity(g["nI"]), icebin_amd.SparseSet(g["nA"] * 40)
    odimI, odimE = orc.SparseSet(g["nI"], init=np.arange(g["nI"])), orc.SparseSet(g["nA"] * 40)
    w1 = rm.matrix_d("EvI", (dimE, dimI), scale=False, correctA=False)
    o1 = rg.matrix_d("EvI", em, (odimE, odimI), scale=False, correctA=False)
    assert_same_weighted(w1, o1, "EvI shared")
    w2 = rm.matrix_d("IvE", (dimI, dimE), scale=True, correctA=True)
    o2 = rg.matrix_d("IvE", em, (odimI, odimE), scale=True, correctA=True)
    assert_same_weighted(w2, o2, "IvE shared")
    dimX, odimX = icebin_amd.SparseSet.identity(len(g["ex_area"])), orc.SparseSet(len(g["ex_area"]), init=np.arange(len(g["ex_area"])))
    w3 = rm.matrix_d("XvE", (dimX, dimE), scale=False, correctA=True)
    o3 = rg.matrix_d("XvE", em, (odimX, odimE), scale=False, correctA=True)
    assert_same_weighted(w3, o3, "XvE shared")
    np.testing.assert_array_equal(dimE.to_sparse(), odimE.to_sparse())
    # a partially pre-populated, non-identity set is appended to in first-seen order
    some = o1.dims[0][::3][::-1].copy()
    dimE2, odimE2 = icebin_amd.SparseSet(g["nA"] * 40, some), orc.SparseSet(g["nA"] * 40, init=some)
    assert_same_weighted(rm.matrix_d("EvA", (dimE2, None)), rg.matrix_d("EvA", em, (odimE2, None)), "EvA prepopulated")
    np.testing.assert_array_equal(dimE2.to_sparse()[:len(some)], some)


def test_prepopulated_dimE_grown_on_the_host_between_builds():
    """The coupler's dimE numbered on the device by EvI, then grown on the host, then read as a pre-populated set by IvE and
    XvE (through its device sparse -> dense table, which must follow the host's growth)."""
    g, em, mm, rg = setup("g50")
    rm = mm.regrid_matrices("greenland", em)
    nE = g["nA"] * 40
    dimI, dimE = icebin_amd.SparseSet.identity(g["nI"]), icebin_amd.SparseSet(nE)
    odimI, odimE = orc.SparseSet(g["nI"], init=np.arange(g["nI"])), orc.SparseSet(nE)
    assert_same_weighted(rm.matrix_d("EvI", (dimE, dimI), scale=False, correctA=False),
                         rg.matrix_d("EvI", em, (odimE, odimI), scale=False, correctA=False), "EvI")
    k = int(np.setdiff1d(np.arange(nE), dimE.to_sparse())[0])
    assert dimE.add_dense(k) == odimE.add_dense(k) == dimE.dense_extent() - 1
    w = rm.matrix_d("IvE", (dimI, dimE), scale=True, correctA=True)
    assert_same_weighted(w, rg.matrix_d("IvE", em, (odimI, odimE), scale=True, correctA=True), "IvE after the host's add_dense")
    assert w.ncol_d == dimE.dense_extent()
    dimX, odimX = icebin_amd.SparseSet.identity(len(g["ex_area"])), orc.SparseSet(len(g["ex_area"]), init=np.arange(len(g["ex_area"])))
    assert_same_weighted(rm.matrix_d("XvE", (dimX, dimE), scale=False, correctA=True),
                         rg.matrix_d("XvE", em, (odimX, odimE), scale=False, correctA=True), "XvE after the host's add_dense")
    np.testing.assert_array_equal(dimE.to_sparse(), odimE.to_sparse())


def test_errors_mirror_reference():
    g, em, mm, rg = setup("tiny")
    rm = mm.regrid_matrices("greenland", em)
    with pytest.raises(icebin_amd.IcebinHipError, match="unknown regrid matrix"):
        rm.matrix("BvA")                                  # regrids.at() throws, RegridMatrices_Dynamic.cpp:419
    with pytest.raises(icebin_amd.IcebinHipError, match="elevmaskI has"):
        mm.regrid_matrices("greenland", em[:-1])          # np_to_blitz shape check, icebin_cython.cpp:231
    with pytest.raises(KeyError):
        mm.regrid_matrices("antarctica", em)
    hi = em.copy(); hi[np.isfinite(hi).argmax()] = 3900.0   # above the last height class 3850 m
    rmh = mm.regrid_matrices("greenland", hi)
    with pytest.raises(icebin_amd.IcebinHipError, match=r"Elevation 3900 out of bounds \(-50, 3850\)") as ei:
        rmh.matrix("EvI")                                 # linterp_1d_b, IceRegridder_L0.cpp:84-85
    assert ei.value.code == -4
    with pytest.raises(orc.OracleError, match=r"Elevation 3900 out of bounds \(-50, 3850\)"):
        rg.matrix_d("EvI", hi)
    assert rmh.matrix("AvI").nnz > 0                      # matrices that never call GvEp are unaffected
    with pytest.raises(icebin_amd.IcebinHipError) as ei:
        mm.regrid_matrices("greenland", em, sigma=(50e3, 50e3, 100.)).matrix("XvA")    # smoothing needs ice-grid rows
    assert ei.value.code == -5
    with pytest.raises(icebin_amd.IcebinHipError, match="three positive sigmas"):
        mm.regrid_matrices("greenland", em, sigma=(50e3, 0., 0.)).matrix("IvA")


@pytest.mark.parametrize("nvar", [1, 2, 3, 5, 8, 16, 17, 64])
@pytest.mark.parametrize("name", ["AvI", "IvA", "EvI", "IvE", "EvA", "AvE"])
def test_apply_parity(name, nvar):
    from icebin_amd.linear import set_tuning
    g, em, mm, rg = setup("g20")
    set_tuning("assemble_bands", 1)          # opt-in structure behind the "rowdual" kernel (EvI/EvX only)
    try:
        w = mm.regrid_matrices("greenland", em, scale=True, correctA=True).matrix(name)
    finally:
        set_tuning("assemble_bands", 0)
    o = rg.matrix_d(name, em, scale=True, correctA=True)
    x = syn.fields(nvar, w.ncol_d)
    for kernel in ("auto", "rowblock", "shortrow", "rowdual"):
        w.set_kernel(kernel)
        y = w.apply(x, fill=np.nan, force_conservation=False)
        ref = o.apply(x, fill=np.nan, force_conservation=False)
        assert rel_linf(y, ref) <= FIELD_RTOL, (name, nvar, kernel)
        assert w.last_kernel() in ("rowblock", "shortrow", "rowdual")
        if kernel == "rowdual":          # only E-row matrices over ice/exchange columns carry bands
            assert w.last_kernel() == ("rowdual" if name == "EvI" else "rowblock")
    y1 = w.apply(x[0])
    assert y1.shape == (w.nrow_d,) and rel_linf(y1, o.apply(x[0])) <= FIELD_RTOL


def test_apply_fill_nan_and_identity_dims():
    # merge_topo.cpp:48-65: identity dimI, the field applied is elevmaskI itself (NaN in masked cells);
    # NaNs sit in empty columns and must not leak; rows with wM == 0 get `fill`.
    g, em, mm, rg = setup("g20")
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=False)
    dimI, odimI = icebin_amd.SparseSet.identity(g["nI"]), orc.SparseSet(g["nI"], init=np.arange(g["nI"]))
    w = rm.matrix_d("AvI", (None, dimI), scale=True, correctA=False)
    o = rg.matrix_d("AvI", em, (None, odimI), scale=True, correctA=False)
    assert_same_weighted(w, o)
    y = w.apply(em, fill=np.nan, force_conservation=False)
    assert np.all(np.isfinite(y)) and rel_linf(y, o.apply(em)) <= FIELD_RTOL
    wi = rm.matrix_d("IvA", (dimI, None), scale=True, correctA=False)
    oi = rg.matrix_d("IvA", em, (odimI, None), scale=True, correctA=False)
    for kernel in ("rowblock", "shortrow"):
        wi.set_kernel(kernel)
        yi = wi.apply(syn.fields(3, wi.ncol_d), fill=-1.5)
        ref = oi.apply(syn.fields(3, wi.ncol_d), fill=-1.5)
        assert np.all(yi[:, np.isnan(em)] == -1.5)
        assert rel_linf(yi, ref) <= FIELD_RTOL


def test_python_surface_apply_M_and_weights():
    # matrix_formats.rst:149-195
    g, em, mm, rg = setup("g20")
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    AvI, IvA = rm.matrix("AvI"), rm.matrix("IvA")
    oA = rg.matrix_d("AvI", em, scale=True, correctA=True)
    assert AvI.shape == (g["nA"], g["nI"]) and mm.nA == g["nA"] and mm.nE == g["nA"] * 40 and mm.nhc == 40
    valI = np.ones(g["nI"])
    valA = AvI.apply_M(valI)
    assert valA.shape == (g["nA"],) and np.isnan(valA).sum() == g["nA"] - AvI.nrow_d
    back = IvA.apply_M(np.nan_to_num(valA))
    ok = ~np.isnan(back)
    assert ok.sum() == np.isfinite(em).sum() and np.all(np.abs(back[ok] - 1) < 1e-12)   # constant survives I->A->I
    two = AvI.apply_M(np.stack([valI, 2 * valI]))
    assert two.shape == (2, g["nA"]) and np.allclose(two[1], 2 * two[0], equal_nan=True)
    # conservation: sum(x*Mw) == sum(Mx * wM)  (test_conserv.py:174-205)
    xi = syn.fields(1, g["nI"])[0]
    lhs, rhs = AvI.apply_Mw(xi), AvI.apply_wM(np.nan_to_num(AvI.apply_M(xi)))
    assert abs(lhs - rhs) / abs(lhs) < 1e-12
    np.testing.assert_array_equal(AvI.get_weights(0)[AvI.dim(0)], oA.wM)
    M = AvI.to_coo()
    assert M.shape == (g["nA"], g["nI"]) and M.nnz == oA.nnz
    np.testing.assert_array_equal(mm.wA("greenland", "native")[g["A_to_sparse"]], g["A_native_area"])
    assert np.all(mm.wA("greenland", "proj", fill=-1.0)[np.setdiff1d(np.arange(g["nA"]), g["A_to_sparse"])] == -1.0)


def test_from_coo_duplicates_bit_exact():
    # Eigen setFromTriplets: duplicates summed in input order (to_eigen_M, eigen_types.cpp:9-34)
    rng = np.random.default_rng(5)
    nrow, ncol, n = 300, 5000, 200000
    r, c = rng.integers(0, nrow, n), rng.integers(0, ncol, n)
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    wM, Mw = rng.random(nrow) + 0.5, rng.random(ncol) + 0.5
    w = icebin_amd.linear_Weighted.from_coo((nrow, ncol), r, c, v, wM, Mw)
    o = orc.Weighted.from_coo(nrow, ncol, r, c, v, wM, Mw)
    assert_same_weighted(w, o, "from_coo")
    x = rng.standard_normal((4, ncol))
    assert rel_linf(w.apply(x), o.apply(x)) <= FIELD_RTOL


def test_force_conservation_branch():
    # non-conservative matrices only arise from smoothing; exercised through from_coo(conservative=False)
    rng = np.random.default_rng(6)
    nrow, ncol, n = 40, 900, 5000
    r, c, v = rng.integers(0, nrow, n), rng.integers(0, ncol, n), rng.random(n)
    wM, Mw = rng.random(nrow) + 0.5, rng.random(ncol) + 0.5
    wM[3] = 0.0
    w = icebin_amd.linear_Weighted.from_coo((nrow, ncol), r, c, v, wM, Mw, conservative=False)
    o = orc.Weighted.from_coo(nrow, ncol, r, c, v, wM, Mw, conservative=False)
    x = rng.random((3, ncol))
    for fc in (False, True):
        y, ref = w.apply(x, fill=-2.0, force_conservation=fc), o.apply(x, fill=-2.0, force_conservation=fc)
        assert np.all(y[:, 3] == -2.0) and rel_linf(y, ref) <= 1e-12


def test_5km_headline_shape_parity_and_conservation():
    # BASELINE config 2/metric shape: 5 km Greenland -> 2x2.5, AvI + IvA, 64 fields
    g, em, mm, rg = setup("g5")
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=False)
    AvI, IvA = rm.matrix("AvI"), rm.matrix("IvA")
    oA, oI = rg.matrix_d("AvI", em), rg.matrix_d("IvA", em)
    assert_same_weighted(AvI, oA, "AvI g5")
    assert_same_weighted(IvA, oI, "IvA g5")
    x = syn.fields(64, AvI.ncol_d)
    y = AvI.apply(x)
    assert rel_linf(y, oA.apply(x)) <= FIELD_RTOL
    wM, Mw = AvI.wM, AvI.Mw
    for k in (0, 17, 63):     # conservation residual with compensated summation
        a = math.fsum((Mw * x[k]).tolist())
        b = math.fsum((wM * y[k]).tolist())
        assert abs(a - b) / abs(a) < 1e-13
    xa = syn.fields(64, IvA.ncol_d)
    assert rel_linf(IvA.apply(xa), oI.apply(xa)) <= FIELD_RTOL


def test_config3_chain_5km_16_fields():
    """BASELINE config 3: 5 km, nhc = 40: 16 fields through EvI, then AvE, then IvA (ice -> elevation
    classes -> atmosphere -> ice), plus IvE on the intermediate; matrices bit-exact, every stage of the
    chain within the field tolerance of the oracle run on the oracle's own intermediates, and the
    round trip conserves the integral (constant field stays constant where defined)."""
    g, em, mm, rg = setup("g5")
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    W = {n: rm.matrix(n) for n in ("EvI", "AvE", "IvA", "IvE")}
    O = {n: rg.matrix_d(n, em, scale=True, correctA=True) for n in W}
    for n in W:
        assert_same_weighted(W[n], O[n], n + " g5")
    xI = syn.fields(16, W["EvI"].ncol_d)
    yE, oE = W["EvI"].apply(xI), O["EvI"].apply(xI)
    assert rel_linf(yE, oE) <= FIELD_RTOL
    # the E and A spaces of independently built matrices are numbered alike here (same emission order)
    np.testing.assert_array_equal(W["AvE"].dim(1), W["EvI"].dim(0))
    np.testing.assert_array_equal(W["IvA"].dim(1), W["AvE"].dim(0))
    yA, oA = W["AvE"].apply(yE), O["AvE"].apply(oE)
    assert rel_linf(yA, oA) <= 4 * FIELD_RTOL
    yI, oI = W["IvA"].apply(yA), O["IvA"].apply(oA)
    assert rel_linf(yI, oI) <= 8 * FIELD_RTOL
    zI, oz = W["IvE"].apply(yE), O["IvE"].apply(oE)
    assert rel_linf(zI, oz) <= 4 * FIELD_RTOL
    ones = np.ones((1, W["EvI"].ncol_d))
    back = W["IvA"].apply(W["AvE"].apply(W["EvI"].apply(ones)))
    m = np.isfinite(back)
    assert m.any() and np.max(np.abs(back[m] - 1.0)) < 1e-12


def test_device_resident_apply_torch():
    import torch
    g, em, mm, rg = setup("g20")
    w = mm.regrid_matrices("greenland", em, scale=True, correctA=False).matrix("AvI")
    o = rg.matrix_d("AvI", em)
    x = syn.fields(16, w.ncol_d)
    dx = torch.from_numpy(x).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dy = w.apply_device(dx, force_conservation=False)
    s.synchronize()
    assert rel_linf(dy.cpu().numpy(), o.apply(x)) <= FIELD_RTOL


_BIG = {}


def _big_grids(config):
    """Full-size synthetic grids, one kept at a time (the Antarctic ones take a minute to generate)."""
    if config not in _BIG:
        _BIG.clear()
        _BIG[config] = syn.make_grids(config)
    return _BIG[config]


def _conservation(W, x, y):
    a = math.fsum((W.Mw * x).tolist())
    b = math.fsum((W.wM * y).tolist())
    return abs(a - b) / abs(a)


def test_config4_full_size_1km_properties_and_parity():
    # BASELINE config 4 at full size: Greenland 1 km (4 204 301 cells) <-> 1x1 deg; oracle parity on the
    # matrices (seconds on one core) and size-independent properties on the fields.
    g, em, mm, rg = setup("g1")
    assert g["nI"] == 4204301
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    AvI, IvA = rm.matrix("AvI"), rm.matrix("IvA")
    assert_same_weighted(AvI, rg.matrix_d("AvI", em, scale=True, correctA=True), "AvI g1")
    assert_same_weighted(IvA, rg.matrix_d("IvA", em, scale=True, correctA=True), "IvA g1")
    x = syn.fields(4, AvI.ncol_d)
    y = AvI.apply(x)
    for k in range(4):
        assert _conservation(AvI, x[k], y[k]) < 1e-13
    # linearity and the constant: M(a*x + b) == a*Mx + b*M1
    ones = np.ones((1, AvI.ncol_d))
    y1 = AvI.apply(ones)
    z = AvI.apply(2.5 * x[:1] - 3.0 * ones)
    assert rel_linf(z, 2.5 * y[:1] - 3.0 * y1) <= 1e-12
    # with correctA the constant is scaled by proj/native per GCM cell; I -> A -> I returns it
    back = IvA.apply(y1)
    assert np.all(np.abs(back - 1.0) < 1e-11)


def test_config2_5km_avi_iva_one_to_three_fields():
    """BASELINE config 2: 5 km Greenland <-> 2x2.5, AvI + IvA, ONE field (and 2, 3) on one GPU, against the oracle at full
    size, for every kernel the dispatcher can pick there -- rowblock with the row split over the four waves (WK = 4 for one
    field, 2 for two or three), shortrow with its 4-field groups -- through the host call, the device call and a batched
    launch; NaN-carrying inputs (merge_topo.cpp:65 applies elevmaskI itself) and `fill` in rows with wM == 0 (identity
    dimI: masked ice cells are empty rows of IvA)."""
    import torch
    g, em, mm, rg = setup("g5")
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    dimI, odimI = icebin_amd.SparseSet.identity(g["nI"]), orc.SparseSet(g["nI"], init=np.arange(g["nI"]))
    cases = [("AvI", (None, None), (None, None)), ("IvA", (None, None), (None, None)),
             ("AvI", (None, dimI), (None, odimI)), ("IvA", (dimI, None), (odimI, None))]
    for name, dims, odims in cases:
        w = rm.matrix_d(name, dims, scale=True, correctA=True)
        o = rg.matrix_d(name, em, dims=odims, scale=True, correctA=True)
        assert_same_weighted(w, o, "config 2 " + name)
        ident = dims != (None, None)
        for nvar in (1, 2, 3):
            x = syn.fields(nvar, w.ncol_d, seed=40 + nvar)
            if name == "AvI":
                cols = np.flatnonzero(np.isfinite(em))[1000:1003] if ident else np.arange(1000, 1003)
                x[0, cols] = np.nan                         # a few ice cells: the NaN stays in the rows that read them
                if ident:
                    x[nvar - 1, np.isnan(em)] = np.nan      # masked cells are empty columns: their NaN must not leak at all
            else:
                x[nvar - 1, 7] = np.nan
            ref = o.apply(x, fill=-3.0, force_conservation=False)
            if name == "AvI":
                assert np.isnan(ref).sum() in range(1, 8 * nvar)
            if name == "IvA" and ident:
                assert np.all(ref[:, np.isnan(em)] == -3.0)
            for kernel in ("auto", "rowblock", "shortrow"):
                w.set_kernel(kernel)
                y = w.apply(x, fill=-3.0, force_conservation=False)
                assert rel_linf(y, ref) <= FIELD_RTOL, (name, nvar, kernel, ident)
                used = w.last_kernel()
                assert used == (kernel if kernel != "auto" else ("rowblock" if name == "AvI" else "shortrow")), (name, kernel, used)
                dx = torch.from_numpy(x).cuda()
                yd = w.apply_device(dx, fill=-3.0, force_conservation=False)
                ym = w.apply_many_device([dx, dx, dx, dx, dx], fill=-3.0, force_conservation=False)
                torch.cuda.synchronize()
                assert rel_linf(yd.cpu().numpy(), ref) <= FIELD_RTOL, (name, nvar, kernel, "device")
                for q in (0, 4):
                    assert np.array_equal(ym[q].cpu().numpy().view(np.uint64), yd.cpu().numpy().view(np.uint64)), (name, nvar, kernel, q)
            w.set_kernel("auto")
            # the 1-D form of apply() (a single field as a vector)
            y1 = w.apply(x[0], fill=-3.0, force_conservation=False)
            assert y1.shape == (w.nrow_d,) and rel_linf(y1, ref[0]) <= FIELD_RTOL
        if name == "AvI" and not ident:                     # conservation of the one-field regrid, compensated sums
            x = syn.fields(1, w.ncol_d, seed=44)
            y = w.apply(x)
            assert _conservation(w, x[0], y[0]) < 1e-13


def test_config4_1km_64_fields_benched_kernels_against_the_oracle():
    """BASELINE config 4 at the field count and through the kernels the 1 km bench lines time, against the oracle's apply
    (1.2e8..2.5e8 multiply-adds on the host): AvI on the column sweep in a batched launch (one entry per column: the
    IDENT variant) and on rowblock; EvI on the row groups (single and batched), on the column sweep and on rowblock; IvA on shortrow with
    the transposed-input / 16-fields-per-thread plan of GB-sized results, with 512-byte planes and with the reference's
    contiguous planes (odd leading dimension: the re-aligning variant)."""
    import torch
    g, em, mm, rg = setup("g1")
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    for name in ("AvI", "EvI"):
        w, o = rm.matrix(name), rg.matrix_d(name, em, scale=True, correctA=True)
        assert_same_weighted(w, o, name + " g1")
        x = syn.fields(64, w.ncol_d, seed=3)
        x[7, ::100003] = np.nan
        ref = o.apply(x, fill=-1.0, force_conservation=False)
        dx = torch.from_numpy(x).cuda()
        w.set_kernel("rowblock")
        y = w.apply_device(dx, fill=-1.0, force_conservation=False)
        torch.cuda.synchronize()
        assert w.last_kernel() == "rowblock" and rel_linf(y.cpu().numpy(), ref) <= FIELD_RTOL, name
        w.set_kernel("auto")
        w.prepare(64, 4)                                 # what bench.py's W.prepare does: the sweep structure, scratch for 4 deep
        ys = w.apply_many_device([dx] * 4, fill=-1.0, force_conservation=False)
        torch.cuda.synchronize()
        assert w.last_kernel() == ("rowgroup" if name == "EvI" else "colsweep"), name
        for q in range(4):
            assert rel_linf(ys[q].cpu().numpy(), ref) <= FIELD_RTOL, (name, q)
        y1 = w.apply_device(dx, fill=-1.0, force_conservation=False)
        torch.cuda.synchronize()
        assert w.last_kernel() == ("rowgroup" if name == "EvI" else "rowblock")      # AvI: the sweep in batched launches only
        if name == "EvI":                                # the sweep serves batched launches of fewer fields: also against the oracle
            w.set_kernel("colsweep")
            yc = w.apply_many_device([dx] * 2, fill=-1.0, force_conservation=False)
            torch.cuda.synchronize()
            assert w.last_kernel() == "colsweep" and rel_linf(yc[1].cpu().numpy(), ref) <= FIELD_RTOL
            w.set_kernel("auto")
        assert rel_linf(y1.cpu().numpy(), ref) <= FIELD_RTOL, name
        for k in (0, 33):
            if not np.isnan(x[k]).any():
                assert _conservation(w, x[k], y1[k].cpu().numpy()) < 1e-13
        del dx, ys, y, y1
    w, o = rm.matrix("IvA"), rg.matrix_d("IvA", em, scale=True, correctA=True)
    assert_same_weighted(w, o, "IvA g1")
    x = syn.fields(64, w.ncol_d, seed=4)
    x[5, 17] = np.nan
    ref = o.apply(x, fill=-1.0, force_conservation=False)
    dx = torch.from_numpy(x).cuda()
    y = w.apply_device(dx, fill=-1.0, force_conservation=False)                       # planes padded to 512 bytes
    torch.cuda.synchronize()
    assert w.last_kernel() == "shortrow" and rel_linf(y.cpu().numpy(), ref) <= FIELD_RTOL
    yc = torch.empty((64, w.nrow_d), dtype=torch.float64, device="cuda")              # the reference's layout: ldb = nrow_d (odd)
    assert w.nrow_d % 8 != 0
    w.apply_device(dx, out=yc, fill=-1.0, force_conservation=False)
    ym = w.apply_many_device([dx, dx], fill=-1.0, force_conservation=False)
    torch.cuda.synchronize()
    assert np.array_equal(yc.cpu().numpy().view(np.uint64), y.cpu().numpy().view(np.uint64))
    assert np.array_equal(ym[1].cpu().numpy().view(np.uint64), y.cpu().numpy().view(np.uint64))


def test_config5_antarctica_1km_assembly_and_apply_properties():
    # BASELINE config 5 (the Antarctic sheet, 36 012 001 ice cells, 1/2 deg GCM): COO -> CSR assembly +
    # apply at full size, through size-independent properties (the bit-level comparison with the oracle at this size is
    # test_config5_full_size_assembly_is_the_oracle_bitwise below).
    g = _big_grids("a1h")
    assert g["nI"] == 36012001
    em = syn.dome_elevmask(g)
    mm = icebin_amd.from_synthetic(g)
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=False)
    AvI = rm.matrix("AvI")
    n_unmasked = int(np.isfinite(em).sum())
    assert AvI.ncol_d == n_unmasked and AvI.nnz >= n_unmasked
    # dims: first-seen order over an (iA, iI)-sorted exchange grid -> the dense->sparse table of I is a
    # permutation of the unmasked cells; of A strictly ascending
    dI, dA = AvI.dim(1), AvI.dim(0)
    assert np.array_equal(np.sort(dI), np.flatnonzero(np.isfinite(em)))
    assert np.all(np.diff(dA) > 0)
    rowptr, col, val = AvI.csr_dense()
    assert rowptr[-1] == AvI.nnz and np.all(np.diff(rowptr) >= 0)
    # scaled rows sum to 1 (M = diag(1/wM) * ApvI), weights are areas: sum(wM) == sum(Mw) == unmasked overlap area
    rs = np.add.reduceat(val, rowptr[:-1][np.diff(rowptr) > 0])
    assert np.all(np.abs(rs - 1.0) < 1e-12)
    wM, Mw = AvI.wM, AvI.Mw
    ok = np.isfinite(em[g["ex_indices"][:, 1]])
    total = math.fsum(g["ex_area"][ok].tolist())
    assert abs(math.fsum(wM.tolist()) - total) / total < 1e-13
    assert abs(math.fsum(Mw.tolist()) - total) / total < 1e-13
    x = syn.fields(2, AvI.ncol_d)
    y = AvI.apply(x)
    for k in range(2):
        assert _conservation(AvI, x[k], y[k]) < 1e-13
    IvA = rm.matrix("IvA")
    assert IvA.nnz == AvI.nnz and IvA.last_kernel() == "none"
    back = IvA.apply(AvI.apply(np.ones((1, AvI.ncol_d))))
    assert IvA.last_kernel() == "shortrow" and np.all(np.abs(back - 1.0) < 1e-11)


def _sheet_properties(config, names, nI_expected):
    """Size-independent checks of a full-size sheet (the oracle comparison at this size goes through committed hashes:
    test_config5_full_size_assembly_is_the_oracle_bitwise): structure,
    scaled rows sum to 1, sum(wM) == sum(Mw) == unmasked overlap area, conservation < 1e-13, and the
    constant field survives the round trips."""
    g = _big_grids(config)
    assert g["nI"] == nI_expected
    em = syn.dome_elevmask(g)
    rm = icebin_amd.from_synthetic(g).regrid_matrices("greenland", em, scale=True, correctA=False)
    ok = np.isfinite(em[g["ex_indices"][:, 1]])
    total = math.fsum(g["ex_area"][ok].tolist())
    n_unmasked = int(np.isfinite(em).sum())
    W = {}
    for name in names:
        w = W[name] = rm.matrix(name)
        rowptr, col, val = w.csr_dense()
        assert rowptr[0] == 0 and rowptr[-1] == w.nnz and np.all(np.diff(rowptr) >= 0), name
        assert col.min() >= 0 and col.max() < w.ncol_d, name
        # columns ascending inside every row
        inner = np.ones(w.nnz, bool); inner[rowptr[:-1][np.diff(rowptr) > 0]] = False
        assert np.all(np.diff(col)[inner[1:]] > 0), name
        nz = np.diff(rowptr) > 0
        rs = np.add.reduceat(val, rowptr[:-1][nz])
        assert np.all(np.abs(rs - 1.0) < 1e-12), name                       # M = diag(1/wM) * (unscaled)
        wM, Mw = w.wM, w.Mw
        assert np.all(wM[nz] > 0) and np.all(Mw >= 0), name
        assert abs(math.fsum(wM.tolist()) - total) / total < 1e-13, name
        assert abs(math.fsum(Mw.tolist()) - total) / total < 1e-13, name
        if name[0] in "AE":
            assert w.ncol_d == n_unmasked and np.array_equal(np.sort(w.dim(1)), np.flatnonzero(np.isfinite(em))), name
        else:
            assert w.nrow_d == n_unmasked, name
        x = syn.fields(2, w.ncol_d)
        y = w.apply(x)
        for k in range(2):
            assert _conservation(w, x[k], y[k]) < 1e-13, name
    return W


def test_config5_antarctica_1km_elevation_class_matrices():
    # the shapes recorded in a faulting scratch run of round 1 (a1h EvI; DESIGN.md "the a1h EvI fault"):
    # EvI and IvE of the Antarctic sheet at full size, through the same properties
    W = _sheet_properties("a1h", ("EvI", "IvE"), 36012001)
    EvI, IvE = W["EvI"], W["IvE"]
    assert EvI.nnz == IvE.nnz and EvI.nrow_d == IvE.ncol_d
    # every ice cell lies between two classes: at most two entries per column of EvI / row of IvE
    rowptr = IvE.csr_dense()[0]
    assert np.diff(rowptr).max() <= 2 * 4        # <= 4 GCM cells under one ice cell, two classes each
    # dims of the shared E space agree as sets (first-seen orders differ between the two generators)
    assert np.array_equal(np.sort(EvI.dim(0)), np.sort(IvE.dim(1)))
    one = np.ones((1, EvI.ncol_d))
    back = IvE.apply(EvI.apply(one)[:, np.argsort(EvI.dim(0))[np.searchsorted(np.sort(EvI.dim(0)), IvE.dim(1))]])
    assert np.all(np.abs(back - 1.0) < 1e-11)


@pytest.mark.parametrize("config", ["g1h", "a1h"])
def test_config5_full_size_assembly_is_the_oracle_bitwise(config):
    """BASELINE config 5 at FULL size against the oracle, bit for bit: both sheets (Antarctica 1 km and
    Greenland 1 km under the 1/2 deg GCM grid), all ten matrices, all four (scale, correctA) branches of
    RegridMatrices_Dynamic.cpp:50-332.  The oracle's side was computed in the build container (16-30 s and 6 GB per Antarctic
    matrix on one core: tests/golden/make_config5_hashes.py) and is committed as SHA-256 of dims / row / col / val / wM / Mw in
    tests/golden/config5_oracle_hashes.json; here the same seeded inputs (their hashes are pinned too) go through the C-ABI and
    the hashes of what comes back must be equal."""
    import importlib.util
    import json
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_config5_hashes", os.path.join(here, "golden", "make_config5_hashes.py"))
    # (only its hashing helpers are used: importing the module imports the oracle wrapper but calls nothing in it)
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    gold = json.load(open(os.path.join(here, "golden", "config5_oracle_hashes.json")))[config]
    g = _big_grids(config)
    em = syn.dome_elevmask(g)
    assert mk.input_hashes(g, em) == gold["inputs"], "the synthetic inputs changed: regenerate tests/golden/config5_oracle_hashes.json"
    mm = icebin_amd.from_synthetic(g)
    n = 0
    for scale, correctA in mk.BRANCHES:
        rm = mm.regrid_matrices("greenland", em, scale=scale, correctA=correctA)
        for name in ALL:
            key = "%s scale=%d correctA=%d" % (name, scale, correctA)
            want = {k: v for k, v in gold["matrices"][key].items() if k != "oracle_seconds"}
            w = rm.matrix(name)
            assert w.built_fast(), key                       # the plan-based build is what the bench times
            row, col, val = w.coo_dense()
            got = mk.weighted_hashes(w.nrow_d, w.ncol_d, w.nnz, w.dim(0), w.dim(1), row, col, val, w.wM, w.Mw)
            assert got == want, (config, key, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
            n += 1
            del w, row, col, val
    assert n == 40


def test_config5_antarctica_eva_ave_fast_build_is_the_general_pipeline_bitwise():
    # EvA / AvE of the Antarctic sheet (tens of thousands of atmosphere cells: the device-wide scans of fast_build_eva, which
    # the oracle-sized grids never reach): the plan-based build against the general pipeline (itself pinned to the oracle on
    # the small grids), all four (scale, correctA) branches, every bit of the matrix, its weights and its dims
    g = _big_grids("a1h")
    em = syn.dome_elevmask(g)
    mm = icebin_amd.from_synthetic(g)
    try:
        for name in ("EvA", "AvE"):
            for scale, correctA in ((True, True), (False, False), (True, False), (False, True)):
                rm = mm.regrid_matrices("greenland", em, scale=scale, correctA=correctA)
                icebin_amd.set_tuning("assemble_fast_eva", 1)
                wf = rm.matrix(name)
                icebin_amd.set_tuning("assemble_fast_eva", 0)
                wg = rm.matrix(name)
                assert wf.built_fast() and not wg.built_fast()
                assert (wf.nrow_d, wf.ncol_d, wf.nnz) == (wg.nrow_d, wg.ncol_d, wg.nnz) and wf.nnz > 4096
                assert np.array_equal(wf.dim(0), wg.dim(0)) and np.array_equal(wf.dim(1), wg.dim(1))
                for a, b in zip(wf.csr_dense(), wg.csr_dense()):
                    assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), name
                assert np.array_equal(wf.wM.view(np.uint64), wg.wM.view(np.uint64)) and np.array_equal(wf.Mw.view(np.uint64), wg.Mw.view(np.uint64))
    finally:
        icebin_amd.set_tuning("assemble_fast_eva", 1)


def test_config5_antarctica_colsweep_agrees_with_rowblock_at_64_fields():
    # full-size cross-check of the two EvI kernels (8.4 GB of fields; the oracle is out of reach at this size): the column
    # sweep and the row-by-row kernel evaluate the same sums in different orders -- 1e-12 of each other, same NaN pattern,
    # constants reproduced (rows of the scaled matrix sum to 1)
    import torch
    g = _big_grids("a1h")
    em = syn.dome_elevmask(g)
    w = icebin_amd.from_synthetic(g).regrid_matrices("greenland", em, scale=True, correctA=False).matrix("EvI")    # (the synthetic sheet's name)
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((64, w.ncol_d), dtype=torch.float64, device="cuda", generator=gen)
    x[3, ::1000003] = float("nan")
    x[5].fill_(1.0)
    w.set_kernel("rowblock")
    y_row = w.apply_device(x, fill=-1.0, force_conservation=False).cpu().numpy()
    w.set_kernel("colsweep")
    y_col = w.apply_device(x, fill=-1.0, force_conservation=False)
    torch.cuda.synchronize()
    assert w.last_kernel() == "colsweep"
    y_col = y_col.cpu().numpy()
    assert rel_linf(y_col, y_row) <= FIELD_RTOL
    live = w.wM != 0
    assert np.all(np.abs(y_col[5][live] - 1.0) < 1e-11)
    # ... and against the ORACLE's apply (ColMajor Eigen order) fed the GPU-built matrix: a full oracle build of this sheet is
    # out of reach on one core, its apply is not (16 fields x 3.3e7 entries).  16 fields = config 5's per-GPU share at 8 GPUs.
    row, col, val = w.coo_dense()
    o = orc.Weighted.from_coo(w.nrow_d, w.ncol_d, row, col, val, w.wM, w.Mw)
    del row, col, val
    x16 = x[:16].contiguous()
    ref = o.apply(x16.cpu().numpy(), fill=-1.0, force_conservation=False)
    for kernel in ("auto", "rowblock", "colsweep", "rowgroup", "auto"):        # (auto: one launch of 16 fields now takes the row groups)
        w.set_kernel(kernel)
        y = w.apply_device(x16, fill=-1.0, force_conservation=False)
        torch.cuda.synchronize()
        assert rel_linf(y.cpu().numpy(), ref) <= FIELD_RTOL, kernel
    w.set_kernel("auto")
    ys = w.apply_many_device([x16] * 4, fill=-1.0, force_conservation=False)          # batched launch of few fields: the tiled row groups (round 5)
    torch.cuda.synchronize()
    assert w.last_kernel() == "rowgroup" and "grouptile" in w.last_launch()
    for q in (0, 3):
        assert rel_linf(ys[q].cpu().numpy(), ref) <= FIELD_RTOL
    icebin_amd.set_tuning("rowgroup_form", 0)                                         # ... and the (batch, field) lanes of the sweep
    try:
        ys = w.apply_many_device([x16] * 4, fill=-1.0, force_conservation=False)
        torch.cuda.synchronize()
        assert w.last_kernel() == "colsweep"
        for q in (0, 3):
            assert rel_linf(ys[q].cpu().numpy(), ref) <= FIELD_RTOL
    finally:
        icebin_amd.set_tuning("rowgroup_form", -2 ** 31)
    assert rel_linf(y_col[:16], ref) <= FIELD_RTOL


def test_config5_antarctica_128_fields_in_one_launch_against_the_oracle():
    """Config 5 at the shape bench.py times it (128 fields in ONE launch, the Antarctic sheet), every family of the hot path:
    the first and the last 16 fields against the ORACLE's apply fed the GPU-built matrix (whose bits are the oracle's: the hash
    test above), the 96 between them against 16-field applies -- the per-GPU share, oracle-checked here and in the test
    above.  NaN inputs, fill and the constant field ride along."""
    import torch
    g = _big_grids("a1h")
    em = syn.dome_elevmask(g)
    rm = icebin_amd.from_synthetic(g).regrid_matrices("greenland", em, scale=True, correctA=False)
    for name, expect in (("AvI", "colsweep"), ("IvA", "shortrow"), ("EvI", "grouptile"), ("IvE", "shortrow")):
        w = rm.matrix(name)
        w.prepare(128)                                      # (as bench.py does: the apply structures built before the first apply)
        gen = torch.Generator(device="cuda").manual_seed(17)
        x = torch.randn((128, w.ncol_d), dtype=torch.float64, device="cuda", generator=gen)
        x[2, ::999983] = float("nan")
        x[127, 5::1000003] = float("nan")
        x[120].fill_(1.0)
        y = w.apply_device(x, fill=-1.0, force_conservation=False)
        torch.cuda.synchronize()
        assert expect in w.last_kernel() + " " + w.last_launch(), (name, w.last_kernel(), w.last_launch())
        row, col, val = w.coo_dense()
        o = orc.Weighted.from_coo(w.nrow_d, w.ncol_d, row, col, val, w.wM, w.Mw)
        del row, col, val
        for b in (0, 7):
            ref = o.apply(x[16 * b:16 * b + 16].cpu().numpy(), fill=-1.0, force_conservation=False)
            assert rel_linf(y[16 * b:16 * b + 16].cpu().numpy(), ref) <= FIELD_RTOL, (name, b)
            del ref
        del o
        for b in range(1, 7):
            y16 = w.apply_device(x[16 * b:16 * b + 16].contiguous(), fill=-1.0, force_conservation=False)
            torch.cuda.synchronize()
            assert rel_linf(y[16 * b:16 * b + 16].cpu().numpy(), y16.cpu().numpy()) <= FIELD_RTOL, (name, b)
        live = torch.from_numpy(w.wM != 0).cuda()
        assert bool(torch.all(torch.abs(y[120][:w.nrow_d][live] - 1.0) < 1e-11)), name          # scaled rows sum to 1
        del x, y, w


def test_config5_greenland_1km_half_degree_sheet():
    # the other sheet of config 5: Greenland 1 km <-> 1/2 deg
    W = _sheet_properties("g1h", ("AvI", "IvA"), 4204301)
    AvI, IvA = W["AvI"], W["IvA"]
    assert IvA.nnz == AvI.nnz
    back = IvA.apply(AvI.apply(np.ones((1, AvI.ncol_d))))
    assert np.all(np.abs(back - 1.0) < 1e-11)


def test_config5_two_sheets_on_one_regridder():
    # combined Greenland + Antarctica: two sheets on ONE GCMRegridder (GCMRegridder.hpp:249, per-sheet
    # regridders); each sheet's matrices are those of the sheet alone (reduced sizes: g20 grids, the two
    # domains placed on the same GCM grid)
    g1 = syn.make_grids("g20")
    g2 = syn.make_grids(dict(sheet="antarctica", dx_km=100, gcm="2x2.5"))
    assert g1["nA"] == g2["nA"]
    # one A grid covering both sheets' realised cells
    allA = np.union1d(g1["A_to_sparse"], g2["A_to_sparse"])
    native = np.zeros(len(allA)); proj = np.zeros(len(allA))
    for g in (g2, g1):
        pos = np.searchsorted(allA, g["A_to_sparse"])
        native[pos], proj[pos] = g["A_native_area"], g["A_proj_area"]
    mm = icebin_amd.GCMRegridder(dict(nA=g1["nA"], to_sparse=allA, native_area=native), g1["hcdefs"], True)
    for name, g in (("greenland", g1), ("antarctica", g2)):
        mm.add_sheet(name, dict(nI=g["nI"]), dict(indices=g["ex_indices"], overlaps=g["ex_area"]), "Z_INTERP", proj)
    for name, g in (("greenland", g1), ("antarctica", g2)):
        em = syn.dome_elevmask(g)
        g = dict(g, A_to_sparse=allA, A_native_area=native, A_proj_area=proj)
        rg = orc.Regridder(g)
        rm = mm.regrid_matrices(name, em, scale=True, correctA=True)
        for spec in ("AvI", "IvA", "EvI", "IvE", "EvA"):
            assert_same_weighted(rm.matrix(spec), rg.matrix_d(spec, em, scale=True, correctA=True), name + " " + spec)


def test_on_disk_formats_roundtrip(tmp_path):
    # the IceBin input file (GCMRegridder_Standard::ncio, GCMRegridder.cpp:104-150) and the
    # "Eigen format" of Weighted_Eigen (matrix_formats.rst:9-63).  GCMRegridder(fname) -- the 1-arg form of
    # _icebin.pyx:81-88 -- on a file the writer produced builds bit-identical matrices; a Weighted survives
    # write -> read bit-exact and applies identically.
    from icebin_amd import ncio
    g, em, mm, rg = setup("g20")
    fn = str(tmp_path / "icebin_in.nc")
    mm.ncio_write(fn)
    ds = ncio.Dataset.read(fn)
    for v in ("m.info", "m.agridA.dim", "m.agridA.native_area", "m.indexingHC", "m.hcdefs", "m.greenland.info",
              "m.greenland.gridA_proj_area", "m.greenland.agridI.dim", "m.greenland.agridI.centroid_xy",
              "m.greenland.aexgrid.indices", "m.greenland.aexgrid.overlaps"):
        assert v in ds.variables, v
    assert ds.dims["m.greenland.aexgrid.nindices"] == 2 * len(g["ex_area"]) and ds.dims["m.nhc"] == 40
    mm2 = icebin_amd.GCMRegridder(fn)
    assert (mm2.nA, mm2.nhc, mm2.nE, mm2.correctA) == (mm.nA, mm.nhc, mm.nE, mm.correctA)
    assert np.array_equal(mm2.wA("greenland", "proj"), mm.wA("greenland", "proj"))
    rm2 = mm2.regrid_matrices("greenland", em, scale=True, correctA=True)
    for spec in ("AvI", "IvE", "EvA"):
        assert_same_weighted(rm2.matrix(spec), rg.matrix_d(spec, em, scale=True, correctA=True), "from file " + spec)
    # sigma != 0 needs the centroids the file carries
    w_s = mm2.regrid_matrices("greenland", em, scale=True, correctA=True, sigma=(30e3, 30e3, 100.)).matrix("IvA")
    assert not w_s.conservative
    # 4-arg form: A grid from a grid file
    fa = str(tmp_path / "gridA.nc")
    dsA = ncio.Dataset()
    ncio.put_abbr_grid(dsA, "grid", g["A_to_sparse"], g["nA"], g["A_native_area"])
    dsA.write(fa)
    mm4 = icebin_amd.GCMRegridder(fa, "grid", g["hcdefs"], True)
    assert mm4.nA == mm.nA and mm4.nhc == 40
    # the other indexingHC layout survives the file too
    g2 = syn.make_grids("g50")
    g2["hc_stride_A"], g2["hc_stride_HC"] = 40, 1
    em2 = syn.dome_elevmask(g2)
    f2 = str(tmp_path / "hcfast.nc")
    icebin_amd.from_synthetic(g2).ncio_write(f2)
    assert_same_weighted(icebin_amd.GCMRegridder(f2).regrid_matrices("greenland", em2, scale=True, correctA=True).matrix("EvI"),
                         orc.Regridder(g2).matrix_d("EvI", em2, scale=True, correctA=True), "hc-fastest from file")

    # Eigen format: two matrices sharing dimI in one file (IceCoupler.cpp:473-488 writes dims once)
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    AvI, EvI = rm.matrix("AvI"), rm.matrix("EvI")
    out = ncio.Dataset()
    AvI.ncio(out, "AvI", ("dimA", "dimI"))
    EvI.ncio(out, "EvI", ("dimE", "dimI"))
    fm = str(tmp_path / "matrices.nc")
    out.write(fm)
    for name, w in (("AvI", AvI), ("EvI", EvI)):
        r = icebin_amd.nc_read_weighted(fm, name)
        assert (r.nrow_d, r.ncol_d, r.nnz, r.conservative, r.scaled) == (w.nrow_d, w.ncol_d, w.nnz, w.conservative, w.scaled)
        assert r.shape == w.shape and np.array_equal(r.dim(0), w.dim(0)) and np.array_equal(r.dim(1), w.dim(1))
        for a, b in zip(r.coo_dense(), w.coo_dense()):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
        assert np.array_equal(r.wM.view(np.uint64), w.wM.view(np.uint64)) and np.array_equal(r.Mw.view(np.uint64), w.Mw.view(np.uint64))
        x = syn.fields(3, g["nI"])
        x[:, ~np.isfinite(em)] = np.nan
        a, b = r.apply_M(x), w.apply_M(x)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b))


def test_cython_module_icebin_on_gpu(tmp_path):
    # `import icebin` (the reference's module name, pylib/_icebin.pyx) over the C++ host mirror: the script of
    # tests/test_conserv/test_conserv.py -- GCMRegridder(fname), regrid_matrices(sheet, elevmaskI, correctA=...),
    # matrix(name), to_coo(), coo_multiply -- against the oracle
    # (import-only: the extension is compiled by __graft_entry__.build() and travels to the GPU box with the snapshot --
    # no compile inside a GPU test; a box without it skips rather than builds)
    import os, sys
    from icebin_amd.cython.build_ext import ext_path
    if not os.path.exists(ext_path()):
        pytest.skip("Cython module not prebuilt (run __graft_entry__.build())")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "icebin_amd", "cython"))
    import icebin
    g, em, mm, rg = setup("g20")
    fn = str(tmp_path / "icebin_in.nc")
    mm.ncio_write(fn)
    mm2 = icebin.GCMRegridder(fn)
    assert (mm2.nA, mm2.nhc, mm2.nE) == (mm.nA, 40, mm.nA * 40)
    assert np.array_equal(mm2.wA("greenland", "native"), mm.wA("greenland", "native"))
    rm = mm2.regrid_matrices("greenland", em.reshape(g["nx"], g["ny"]))        # defaults: scale=True, correctA=True
    mats = {}
    for name in ("AvI", "IvA", "EvI", "IvE", "AvE", "EvA"):
        w = mats[name] = rm.matrix(name)
        o = rg.matrix_d(name, em, scale=True, correctA=True)
        assert w.shape == (o.sparse_extents[0], o.sparse_extents[1]) and w.shape_d == (o.nrow, o.ncol)
        assert np.array_equal(w.dim(0), o.dims[0]) and np.array_equal(w.dim(1), o.dims[1])
        assert np.array_equal(w.wM.view(np.uint64), o.wM.view(np.uint64)) and np.array_equal(w.Mw.view(np.uint64), o.Mw.view(np.uint64))
        M = w.to_coo()
        assert np.array_equal(M.data.view(np.uint64), o.val.view(np.uint64))
        assert np.array_equal(M.row, o.dims[0][o.row]) and np.array_equal(M.col, o.dims[1][o.col])
    # test_conserv.py:132-172: a constant survives I -> A -> I and I -> E -> I (coo_multiply) ...
    AvI, IvA, EvI, IvE = (mats[k].to_coo() for k in ("AvI", "IvA", "EvI", "IvE"))
    valI = np.ones(g["nI"])
    valIAI = icebin.coo_multiply(IvA, icebin.coo_multiply(AvI, valI, fill=np.nan), fill=np.nan, ignore_nan=True)
    m = np.isfinite(valIAI)
    assert m.sum() == np.isfinite(em).sum() and np.all(np.abs(valIAI[m] - 1.0) < 1e-11)
    # ... and apply_M on 2-D input + conservation sum(x*Mw) == sum(Mx*wM) (test_conserv.py:174-205)
    x = syn.fields(2, g["nI"])
    y = mats["AvI"].apply_M(x)
    ref = rg.matrix_d("AvI", em, scale=True, correctA=True)
    yd = ref.apply(x[:, ref.dims[1]])
    assert rel_linf(y[:, ref.dims[0]], yd) <= FIELD_RTOL and np.isnan(y[:, 0]).all()
    for k in range(2):
        a, b = mats["AvI"].apply_Mw(x[k]), mats["AvI"].apply_wM(np.nan_to_num(y[k]))
        assert abs(a - b) / abs(a) < 1e-12
    with pytest.raises(RuntimeError, match="unknown regrid matrix"):
        rm.matrix("BvA")
    with pytest.raises(KeyError):
        mm2.regrid_matrices("antarctica", em)


def _clip_numpy(poly, x0, x1, y0, y1):
    """Independent Sutherland-Hodgman + shoelace in numpy (checker for the device clipper)."""
    def clip(pts, axis, bound, lower):
        out = []
        for k in range(len(pts)):
            a, b = pts[k], pts[(k + 1) % len(pts)]
            ina = a[axis] >= bound if lower else a[axis] <= bound
            inb = b[axis] >= bound if lower else b[axis] <= bound
            if ina:
                out.append(a)
            if ina != inb:
                t = (bound - a[axis]) / (b[axis] - a[axis])
                out.append(a + t * (b - a))
        return out
    pts = [np.asarray(p, float) for p in poly]
    for axis, bound, lower in ((0, x0, True), (0, x1, False), (1, y0, True), (1, y1, False)):
        pts = clip(pts, axis, bound, lower)
        if len(pts) < 3:
            return 0.0
    P = np.array(pts)
    return 0.5 * float(np.sum(P[:, 0] * np.roll(P[:, 1], -1) - np.roll(P[:, 0], -1) * P[:, 1]))


def test_exchange_grid_generation():
    # make_exchange_grid (gridgen/GridGen_Exchange.cpp:175-284) for the rectilinear case, SURVEY.md 8f rank 4
    from icebin_amd import gridgen
    # (1) tests/test_grid.cpp:200-201: unit squares have area 1 -- two unit ice cells under one 2 x 1 GCM cell
    ex = gridgen.make_exchange_grid([0., 1., 2.], [0., 1.], [[(0, 0), (2, 0), (2, 1), (0, 1)]], [7])
    assert ex["indices"].tolist() == [[7, 0], [7, 1]] and ex["overlaps"].tolist() == [1.0, 1.0]
    # (2) the synthetic configurations' exact interval products (icebin_amd/synthetic.py), both index orders
    for cfg, xf in (("g50", False), ("g20", True), ("g5", False)):
        g = syn.make_grids(cfg, x_fastest=xf)
        axe, aye = g["A_xedges"], g["A_yedges"]
        polys, iA = [], []
        for ky in range(len(aye) - 1):
            for kx in range(len(axe) - 1):
                polys.append([(axe[kx], aye[ky]), (axe[kx + 1], aye[ky]), (axe[kx + 1], aye[ky + 1]), (axe[kx], aye[ky + 1])])
                iA.append((g["A_j0"] + ky) * g["im"] + g["A_i0"] + kx)
        order = np.argsort(iA)
        ex = gridgen.make_exchange_grid(np.arange(g["nx"] + 1) * g["dx"], np.arange(g["ny"] + 1) * g["dx"],
                                        [polys[k] for k in order], np.asarray(iA)[order], x_fastest=xf)
        assert np.array_equal(ex["indices"], g["ex_indices"]), cfg
        assert np.max(np.abs(ex["overlaps"] - g["ex_area"]) / g["ex_area"]) <= 1e-12, cfg
        # the generated grid drives the regridder to the same matrices (values to rounding: areas differ in the last bit)
    em = syn.dome_elevmask(g)
    g2 = dict(g, ex_indices=ex["indices"], ex_area=ex["overlaps"])
    a = icebin_amd.from_synthetic(g2).regrid_matrices("greenland", em).matrix("AvI")
    b = icebin_amd.from_synthetic(g).regrid_matrices("greenland", em).matrix("AvI")
    assert np.array_equal(a.dim(1), b.dim(1)) and np.array_equal(a.coo_dense()[1], b.coo_dense()[1])
    assert np.max(np.abs(a.coo_dense()[2] - b.coo_dense()[2])) <= 1e-12 * np.max(b.coo_dense()[2])
    # (3) general convex polygons (a projected lon/lat box is a skewed quadrilateral): against an independent numpy clipper,
    #     cell by cell, and area conservation -- the overlaps of a polygon inside the domain add up to its area
    rng = np.random.default_rng(11)
    xe, ye = np.cumsum(rng.uniform(0.5, 1.5, 41)), np.cumsum(rng.uniform(0.5, 1.5, 31))
    polys, iA = [], []
    for k in range(12):
        c = np.array([rng.uniform(xe[8], xe[-9]), rng.uniform(ye[8], ye[-9])])
        ang = np.sort(rng.uniform(0, 2 * np.pi, rng.integers(3, 9)))
        rad = rng.uniform(2.0, 5.0)
        polys.append(c + rad * np.stack([np.cos(ang), np.sin(ang)], axis=1))       # convex, counter-clockwise
        iA.append(100 + 3 * k)
    ex = gridgen.make_exchange_grid(xe, ye, polys, iA)
    ny = len(ye) - 1
    assert np.all(np.diff(ex["indices"][:, 0].astype(np.int64) * 10 ** 6 + ex["indices"][:, 1]) > 0)      # sorted by (iA, iI), unique
    for k, poly in enumerate(polys):
        sel = ex["indices"][:, 0] == iA[k]
        P = np.asarray(poly)
        full = 0.5 * float(np.sum(P[:, 0] * np.roll(P[:, 1], -1) - np.roll(P[:, 0], -1) * P[:, 1]))
        assert abs(ex["overlaps"][sel].sum() - full) <= 1e-12 * full
        for iI, a_dev in zip(ex["indices"][sel, 1], ex["overlaps"][sel]):
            ix, iy = divmod(int(iI), ny)
            ref = _clip_numpy(poly, xe[ix], xe[ix + 1], ye[iy], ye[iy + 1])
            assert abs(a_dev - ref) <= 1e-12 * max(ref, 1e-3), (k, iI)
    # errors: clockwise polygons give no cells (negative areas are not overlaps); unsorted iA is refused
    assert len(gridgen.make_exchange_grid([0., 1.], [0., 1.], [[(0, 0), (0, 1), (1, 1), (1, 0)]], [0])["overlaps"]) == 0
    with pytest.raises(icebin_amd.IcebinHipError, match="ascending iA"):
        gridgen.make_exchange_grid([0., 1.], [0., 1.], [[(0, 0), (1, 0), (1, 1)]] * 2, [5, 5])


def test_e1ve0_bit_exact_against_oracle():
    # compute_E1vE0c (slib/icebin/e1ve0.cpp:55-106) on the device assembly machinery vs the oracle's SpGEMM restatement:
    # one sheet and two sheets (the second one a different mask pair on the same grids), identity and own X dims
    g = syn.make_grids("g50")
    nX, nE = len(g["ex_area"]), g["nA"] * len(g["hcdefs"])
    em0 = syn.dome_elevmask(g)
    em1 = np.where(np.isfinite(syn.dome_elevmask(g, frac=0.80)), syn.dome_elevmask(g, frac=0.80) + 35.0, np.nan)
    em2 = np.where(np.isfinite(em0), em0 * 0.9 + 10.0, np.nan)
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)

    def pair(em, identity_x):
        dX = icebin_amd.SparseSet.identity(nX) if identity_x else None
        w = mm.regrid_matrices("greenland", em, scale=False, correctA=True).matrix_d("XvE", (dX, None), scale=False, correctA=True)
        oX = orc.SparseSet(nX, init=np.arange(nX)) if identity_x else None
        o = rg.matrix_d("XvE", em, dims=(oX, None), scale=False, correctA=True)
        assert_same_weighted(w, o, "XvE")
        return w, o
    for identity_x in (True, False):
        (w1, o1), (w0, o0), (w2, o2) = pair(em1, identity_x), pair(em0, identity_x), pair(em2, identity_x)
        for ws, os_ in ((([w1], [w0]), ([o1], [o0])), (([w1, w2], [w0, w0]), ([o1, o2], [o0, o0]))):
            E = icebin_amd.compute_E1vE0c(ws[0], ws[1], nE)
            i, j, v = orc.e1ve0c(os_[0], os_[1], nE)
            M = E.to_coo()
            assert M.shape == (nE, nE) and len(M.data) == len(v)
            assert np.array_equal(M.row, i) and np.array_equal(M.col, j)
            assert np.array_equal(M.data.view(np.uint64), v.view(np.uint64)), (identity_x, len(ws[0]))
    # E1 == E0 -> exact zeros
    Z = icebin_amd.compute_E1vE0c([w0], [w0], nE).to_coo()
    assert len(Z.data) > 0 and not np.any(Z.data)


def test_coo_multiply_legacy_contract():
    # icebin.coo_multiply(M, x, fill, ignore_nan) (coo_matvec, pylib/icebin_cython.cpp:158-192): rows with no
    # (surviving) entry keep `fill`; NaN inputs are skipped with ignore_nan, propagate without
    g, em, mm, rg = setup("g20")
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    for name in ("AvI", "IvA", "IvE"):
        w = rm.matrix(name)
        M = w.to_coo()
        rng = np.random.default_rng(3)
        x = rng.standard_normal(M.shape[1])
        x[rng.random(M.shape[1]) < 0.3] = np.nan
        for ignore_nan in (False, True):
            for fill in (np.nan, -5.0):
                got = icebin_amd.coo_multiply(M, x, fill=fill, ignore_nan=ignore_nan)
                ref = orc.coo_matvec(M, x, fill=fill, ignore_nan=ignore_nan)
                assert np.array_equal(np.isnan(got), np.isnan(ref)), (name, ignore_nan, fill)
                m = np.isfinite(ref)
                assert np.max(np.abs(got[m] - ref[m])) <= FIELD_RTOL * max(np.max(np.abs(ref[m])), 1e-300)
        # shuffled triplets with duplicates: same result up to rounding
        perm = rng.permutation(len(M.data))
        import scipy.sparse
        M2 = scipy.sparse.coo_matrix((np.concatenate([M.data[perm] * 0.25, M.data * 0.75]),
                                      (np.concatenate([M.row[perm], M.row]), np.concatenate([M.col[perm], M.col]))), shape=M.shape)
        a = icebin_amd.coo_multiply(M2, np.nan_to_num(x), fill=np.nan)
        b = orc.coo_matvec(M, np.nan_to_num(x), fill=np.nan)
        m = np.isfinite(b)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.max(np.abs(a[m] - b[m])) <= 1e-12 * np.max(np.abs(b[m]))


def test_field_sharded_apply_rccl_world1():
    # the bench's N>1 path (field shard + grouped RCCL all-gather on a second stream), rehearsed at world_size 1
    import socket
    import torch
    import torch.distributed as dist
    from icebin_amd.distributed import FieldShardedApply
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        g, em, mm, rg = setup("g20")
        w = mm.regrid_matrices("greenland", em, scale=True, correctA=False).matrix("AvI")
        o = rg.matrix_d("AvI", em)
        xs = [syn.fields(8, w.ncol_d, seed=100 + i) for i in range(7)]
        dxs = [torch.from_numpy(x).cuda() for x in xs]
        for G in (1, 4):
            sh = FieldShardedApply(w, 8, None, torch.device("cuda", 0), steps_per_gather=G)
            handles = []
            for i, dx in enumerate(dxs):
                if G == 4 and i < 4:       # the first whole group through ONE batched launch
                    if i == 0:
                        grp, _ = sh.apply_many_ptr([d.data_ptr() for d in dxs[:4]], w.ncol_d)
                    handles.append((grp, i))
                else:
                    handles.append(sh.apply(dx))
                if G == 4 and i == 3:      # first full group gathered: check it before its buffers are reused
                    sh.wait(); torch.cuda.synchronize()
                    for j in range(4):
                        y = sh.result(*handles[j]).reshape(8, -1).cpu().numpy()
                        assert rel_linf(y, o.apply(xs[j])) <= FIELD_RTOL
            sh.flush(); sh.wait(); torch.cuda.synchronize()
            last = range(4, 7) if G == 4 else range(5, 7)     # results still held in the double buffers
            for j in last:
                y = sh.result(*handles[j]).reshape(8, -1).cpu().numpy()
                assert rel_linf(y, o.apply(xs[j])) <= FIELD_RTOL, (G, j)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name", ["IvE", "AvI", "EvI"])
def test_coupler_shaped_fused_apply(name):
    # IceCoupler.cpp:203-252 (ice_ivalsI = IvE0 * (gcm_ovalsE0*T + b)) and :445 (gcm_ivalsX = M * (ice_ovalsI*T + b)):
    # the small dense variable transform is applied on the small side of M; result vs the oracle's
    # reference-order evaluation (transform first, then M).
    g, em, mm, rg = setup("g20")
    w = mm.regrid_matrices("greenland", em, scale=True, correctA=True).matrix(name)
    o = rg.matrix_d(name, em, scale=True, correctA=True)
    rng = np.random.default_rng(11)
    nin, nout = 5, 3
    V = syn.fields(nin, w.ncol_d)
    V[4, ::7] = np.nan                       # an input variable no output uses may carry NaN (contracts::ALLOW_NAN)
    T = np.zeros((nin, nout))
    T[0, 0], T[1, 0], T[2, 1], T[3, 2], T[0, 2] = 1.0, 0.5, 917.0, -2.0, 0.25     # sparse: row 4 is all structural zeros
    b = np.array([0.0, 273.15, -1.0])
    y = w.apply_transformed(V, T, b, fill=-9.0)
    ref = o.apply_transformed(V, T, b, fill=-9.0)
    assert y.shape == (nout, w.nrow_d) and np.all(np.isfinite(y))
    assert rel_linf(y, ref) <= FIELD_RTOL
    # second call reuses the handle's scratch and cached M*1
    assert rel_linf(w.apply_transformed(2 * V, T, b, fill=-9.0), o.apply_transformed(2 * V, T, b, fill=-9.0)) <= FIELD_RTOL
    # a NaN in a USED variable propagates exactly where the reference puts it
    V2 = V.copy(); V2[2, 5] = np.nan
    y2, r2 = w.apply_transformed(V2, T, b), o.apply_transformed(V2, T, b)
    assert np.array_equal(np.isnan(y2), np.isnan(r2)) and np.isnan(y2).any()


def test_empty_and_degenerate_inputs():
    # everything masked -> empty matrices; one unmasked cell; zero fields; nX == 0
    g = syn.make_grids("tiny")
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    em = np.full(g["nI"], np.nan)
    rm = mm.regrid_matrices("greenland", em)
    for name in ALL:
        w = rm.matrix(name)
        o = rg.matrix_d(name, em, scale=True, correctA=True)
        assert (w.nrow_d, w.ncol_d, w.nnz) == (0, 0, 0) == (o.nrow, o.ncol, o.nnz), name
        assert w.apply(np.zeros((3, 0))).shape == (3, 0)
        assert w.shape == (o.sparse_extents[0], o.sparse_extents[1])
    em1 = em.copy(); em1[g["nI"] // 2] = 1234.5          # a single ice cell
    rm1 = mm.regrid_matrices("greenland", em1)
    for name in ALL:
        assert_same_weighted(rm1.matrix_d(name, scale=True, correctA=True), rg.matrix_d(name, em1, scale=True, correctA=True), name + " one cell")
    w = rm1.matrix("AvI")
    assert w.apply(np.zeros((0, w.ncol_d))).shape == (0, w.nrow_d)
    # identity dims on an empty matrix: every row exists, all weights zero -> apply returns fill everywhere
    dimI = icebin_amd.SparseSet.identity(g["nI"])
    wi = rm.matrix_d("IvA", (dimI, None))
    assert wi.nrow_d == g["nI"] and wi.ncol_d == 0 and wi.nnz == 0
    assert np.all(wi.apply(np.zeros((2, 0)), fill=-3.0) == -3.0)
    # an exchange grid with no cells at all
    g0 = dict(g); g0["ex_indices"] = np.zeros((0, 2), np.int32); g0["ex_area"] = np.zeros(0)
    w0 = icebin_amd.from_synthetic(g0).regrid_matrices("greenland", syn.dome_elevmask(g)).matrix("EvI")
    assert (w0.nrow_d, w0.ncol_d, w0.nnz) == (0, 0, 0)


def test_alternate_indexingHC_and_proj_alias():
    # a file-loaded regridder may carry indexingHC with HC as the FASTEST index (iE = iA*nhc + ihc);
    # and sproj == "" aliases proj_area to native_area (IceRegridder.cpp:106-108) -> correctA is a no-op
    g = syn.make_grids("g50")
    g["hc_stride_A"], g["hc_stride_HC"] = 40, 1
    em = syn.dome_elevmask(g)
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    rm = mm.regrid_matrices("greenland", em)
    for name in ("EvI", "IvE", "EvA", "AvE", "XvE", "EvX"):
        for correctA in (True, False):
            assert_same_weighted(rm.matrix_d(name, scale=True, correctA=correctA),
                                 rg.matrix_d(name, em, scale=True, correctA=correctA), name + " HC-fastest")
    g2 = syn.make_grids("g50")
    g2["A_proj_area"] = g2["A_native_area"]
    mm2, rg2 = icebin_amd.from_synthetic(g2), orc.Regridder(g2)
    rm2 = mm2.regrid_matrices("greenland", em)
    for name in ("AvI", "IvA", "EvA"):
        a, b = rm2.matrix_d(name, scale=True, correctA=True), rm2.matrix_d(name, scale=True, correctA=False)
        assert_same_weighted(a, rg2.matrix_d(name, em, scale=True, correctA=True), name + " proj alias")
        np.testing.assert_allclose(a.coo_dense()[2], b.coo_dense()[2], rtol=1e-15)
    with pytest.raises(icebin_amd.IcebinHipError, match="neither"):
        g3 = syn.make_grids("tiny"); g3["hc_stride_A"], g3["hc_stride_HC"] = 3, 7
        icebin_amd.from_synthetic(g3)


def test_unsorted_prepopulated_and_reused_matrices_object():
    # one RegridMatrices serves many matrix_d calls with different params (IceCoupler.cpp:361-468), in any order
    g, em, mm, rg = setup("g50", order="shuffled")
    rm = mm.regrid_matrices("greenland", em, scale=False, correctA=False)
    calls = [("XvE", False, True), ("AvI", False, True), ("EvI", False, False), ("IvE", True, True), ("AvI", True, False)]
    for name, scale, correctA in calls + calls[::-1]:
        assert_same_weighted(rm.matrix_d(name, scale=scale, correctA=correctA),
                             rg.matrix_d(name, em, scale=scale, correctA=correctA), "%s %d %d" % (name, scale, correctA))
    # RegridMatrices.matrix() uses the params given to regrid_matrices (RegridMatrices_Dynamic.cpp:433)
    assert_same_weighted(rm.matrix("IvA"), rg.matrix_d("IvA", em, scale=False, correctA=False), "matrix() params")


@pytest.mark.parametrize("name", ["IvA", "IvE"])
def test_smoothing_sigma_nonzero(name):
    # RegridMatrices_Dynamic.cpp:237-248 + smoother.cpp: M <- smoothI * M, conservative = false, and the
    # conservation correction of apply().  Structure is exact; entries agree to rounding (device exp()
    # and the neighbour order of the absent RTree are not bit-reproducible: parity unpinned at 1e-13).
    # All three device forms are checked: the wave-per-row direct build (small grids), the spatial tiles (larger grids) and the
    # triplet pipeline (their fallback).
    from icebin_amd.linear import set_tuning
    g, em, mm, rg = setup("g20")
    sigma = (60e3, 60e3, 250.0)
    # The form that builds each leg, from the CPU (tests/smoothing_cases.py).  IvA: 18 columns around the widest bin, the tile legs run
    # the tiles.  IvE at 20 km: 145 columns around the widest bin, more than SMT_KMAX = 128 -- the column tables overflow and the
    # smooth_tile = 1 legs are served by the triplet pipeline (the tiles are checked against the oracle at 50 km, where IvE has 125:
    # test_smoothing_forms_and_their_fallthroughs).
    _, _, widest, longest, longest_smoothed = smc.oracle_case("g20", name, sigma)
    tile_form = {"IvA": smc.TILE, "IvE": smc.TRIPLET}[name]
    for (scale, correctA), direct, tile, form in (((True, True), 1, 0, smc.DIRECT), ((False, False), 0, 0, smc.TRIPLET), ((True, True), 0, 0, smc.TRIPLET),
                                                  ((True, True), 0, 1, tile_form), ((False, True), 0, 1, tile_form)):
        smc.assert_input_side(form, tile > 0, direct > 0, widest, longest, longest_smoothed)
        set_tuning("smooth_direct", direct)
        set_tuning("smooth_tile", tile)           # 1: the spatial-tile form (taken by itself for grids beyond the direct form's size)
        try:
            w = mm.regrid_matrices("greenland", em, scale=scale, correctA=correctA, sigma=sigma).matrix(name)
        finally:
            set_tuning("smooth_direct", -1)
            set_tuning("smooth_tile", -1)
        assert w.smoothed_by() == form
        o = rg.matrix_d(name, em, scale=scale, correctA=correctA, sigma=sigma)
        plain = rg.matrix_d(name, em, scale=scale, correctA=correctA)
        assert not w.conservative and not o.conservative and w.scaled == scale
        assert (w.nrow_d, w.ncol_d, w.nnz) == (o.nrow, o.ncol, o.nnz) and o.nnz > 3 * plain.nnz
        np.testing.assert_array_equal(w.dim(0), o.dims[0])
        np.testing.assert_array_equal(w.dim(1), o.dims[1])
        row, col, val = w.coo_dense()
        np.testing.assert_array_equal(row, o.row)
        np.testing.assert_array_equal(col, o.col)
        np.testing.assert_allclose(val, o.val, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(w.wM.view(np.uint64), plain.wM.view(np.uint64))     # weights are those of the unsmoothed matrix
        np.testing.assert_array_equal(w.Mw.view(np.uint64), plain.Mw.view(np.uint64))
        x = syn.fields(3, w.ncol_d) + 2.0
        for fc in (False, True):
            y, ref = w.apply(x, force_conservation=fc), o.apply(x, force_conservation=fc)
            assert rel_linf(y, ref) <= FIELD_RTOL
        y = w.apply(x, force_conservation=True)          # the correction restores sum(wM*y) == sum(Mw*x)
        for k in range(3):
            assert _conservation(w, x[k], y[k]) < 1e-13
    # matrices whose build never smooths ignore sigma (compute_AEvI, compute_EvA)
    a = mm.regrid_matrices("greenland", em, sigma=sigma).matrix("AvI")
    assert a.conservative and a.smoothed_by() == smc.NONE
    assert_same_weighted(a, rg.matrix_d("AvI", em, scale=True, correctA=True), "AvI with sigma")


def _smoothed_build(mm, em, name, sigma, knobs):
    from icebin_amd.linear import set_tuning
    set_tuning("smooth_direct", knobs[0])
    set_tuning("smooth_tile", knobs[1])
    try:
        return mm.regrid_matrices("greenland", em, scale=True, correctA=True, sigma=sigma).matrix(name)
    finally:
        set_tuning("smooth_direct", -1)
        set_tuning("smooth_tile", -1)


def _same_bits(a, b):
    if (a.nrow_d, a.ncol_d, a.nnz, a.conservative) != (b.nrow_d, b.ncol_d, b.nnz, b.conservative):
        return False
    return all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
               for x, y in zip(a.csr_dense() + (a.wM, a.Mw), b.csr_dense() + (b.wM, b.Mw)))


def check_smoothing_leg(mm, sigma, name, knobs, form, same_as, assert_form=True):
    """One leg of smc.G50_LEGS: the input lies on the intended side of the forms' limits (decided on the CPU), the form that built the
    matrix is the intended one, the matrix is the oracle's (structure exact, entries to 1e-12) and, where another knob setting must
    give the same form, bitwise that build.  assert_form=False: a library without smoothed_by (a parent build, measured by hand)."""
    g, em = smc.grids("g50")
    plain, o, widest, longest, longest_smoothed = smc.oracle_case("g50", name, sigma)
    smc.assert_input_side(form, knobs[1] > 0, knobs[0] > 0, widest, longest, longest_smoothed)
    w = _smoothed_build(mm, em, name, sigma, knobs)
    if assert_form:
        assert w.smoothed_by() == form
    assert not w.conservative and not o.conservative
    assert (w.nrow_d, w.ncol_d, w.nnz) == (o.nrow, o.ncol, o.nnz)
    np.testing.assert_array_equal(w.dim(0), o.dims[0])
    np.testing.assert_array_equal(w.dim(1), o.dims[1])
    row, col, val = w.coo_dense()
    np.testing.assert_array_equal(row, o.row)
    np.testing.assert_array_equal(col, o.col)
    np.testing.assert_allclose(val, o.val, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(w.wM.view(np.uint64), plain.wM.view(np.uint64))
    np.testing.assert_array_equal(w.Mw.view(np.uint64), plain.Mw.view(np.uint64))
    if same_as is not None:
        other = _smoothed_build(mm, em, name, sigma, same_as)
        if assert_form:
            assert other.smoothed_by() == form
        assert _same_bits(w, other)


@pytest.mark.parametrize("leg", range(len(smc.G50_LEGS)), ids=["%s-%dkm-%d%d" % (l[1], l[0][0] / 1e3, l[2][0], l[2][1]) for l in smc.G50_LEGS])
def test_smoothing_forms_and_their_fallthroughs(leg):
    # 50 km (793 rows): the tile form at the edge of its column table (IvE, 125 of SMT_KMAX = 128 columns: the raised-LDS launch), the
    # tiles overflowing into the direct form, both overflowing into the triplet pipeline, and the tiles serving IvA at a sigma where
    # they cannot serve IvE -- each against the oracle; a fall-through is bitwise the build that asks for the serving form alone
    g, em = smc.grids("g50")
    check_smoothing_leg(icebin_amd.from_synthetic(g), *smc.G50_LEGS[leg])


def test_smoothing_refusals_are_decided_before_any_smoothing_work():
    # smooth_check: "three positive sigmas" and the centroids, IBH_EINVAL both, after the unsmoothed build and before the first bin
    g, em = smc.grids("g50")
    mm = icebin_amd.from_synthetic(g)
    # (RegridParams::smooth() is sigma.x != 0: a zero x component asks for no smoothing at all)
    plain = mm.regrid_matrices("greenland", em, sigma=(0.0, 60e3, 250.0)).matrix("IvA")
    assert plain.conservative and plain.smoothed_by() == smc.NONE
    for sigma in ((60e3, 60e3, 0.0), (60e3, -1.0, 250.0), (-60e3, 60e3, 250.0)):
        for name in ("IvA", "IvE"):
            with pytest.raises(icebin_amd.IcebinHipError, match="three positive sigmas") as ei:
                mm.regrid_matrices("greenland", em, sigma=sigma).matrix(name)
            assert ei.value.code == icebin_amd._capi.IBH_EINVAL
    bare = dict(g)
    bare["I_centroid_xy"] = None
    mb = icebin_amd.from_synthetic(bare)
    assert mb.regrid_matrices("greenland", em).matrix("IvA").nnz > 0              # unsmoothed builds do not need them
    for name in ("IvA", "IvE"):
        with pytest.raises(icebin_amd.IcebinHipError, match="centroid_xy") as ei:
            mb.regrid_matrices("greenland", em, sigma=(60e3, 60e3, 250.0)).matrix(name)
        assert ei.value.code == icebin_amd._capi.IBH_EINVAL


def test_apply_is_graph_capturable():
    # the device-resident apply only enqueues kernels (no allocation, no sync): it can be captured in a
    # hipGraph together with the caller's own work and replayed
    import torch
    g, em, mm, rg = setup("g20")
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=False)
    AvI, IvA = rm.matrix("AvI"), rm.matrix("IvA")
    oA, oI = rg.matrix_d("AvI", em), rg.matrix_d("IvA", em)
    x = torch.from_numpy(syn.fields(8, AvI.ncol_d)).cuda()
    y = torch.empty((8, AvI.nrow_d), dtype=torch.float64, device="cuda")
    z = torch.empty((8, IvA.nrow_d), dtype=torch.float64, device="cuda")
    AvI.apply_device(x, out=y, force_conservation=False); IvA.apply_device(y, out=z, force_conservation=False)   # warm-up outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        AvI.apply_device(x, out=y, force_conservation=False)      # I -> A
        IvA.apply_device(y, out=z, force_conservation=False)      # A -> I
    for rep in range(3):
        x.copy_(torch.from_numpy(syn.fields(8, AvI.ncol_d, seed=50 + rep)).cuda())
        y.zero_(); z.zero_()
        graph.replay()
        torch.cuda.synchronize()
        xr = x.cpu().numpy()
        yr = oA.apply(xr)
        assert rel_linf(y.cpu().numpy(), yr) <= FIELD_RTOL
        assert rel_linf(z.cpu().numpy(), oI.apply(yr)) <= 10 * FIELD_RTOL


@pytest.mark.parametrize("name", ["AvI", "EvI", "IvA", "IvE"])
@pytest.mark.parametrize("nbatch,nvar", [(1, 5), (2, 3), (5, 8), (16, 16), (19, 64), (35, 4)])
def test_apply_many_is_bitwise_separate_applies(name, nbatch, nvar):
    # ibh_weighted_apply_many_device: ONE launch over several field batches (the staged row segment is
    # reused across the batches of a workgroup); results must be bitwise those of separate applies, for
    # every batches-per-workgroup setting, including more batches than one launch takes (IBH_MAX_BATCH)
    import torch
    g, em, mm, rg = setup("g20")
    w = mm.regrid_matrices("greenland", em, scale=True, correctA=True).matrix(name)
    o = rg.matrix_d(name, em, scale=True, correctA=True)
    xs = [torch.from_numpy(syn.fields(nvar, w.ncol_d, seed=100 + q)).cuda() for q in range(nbatch)]
    xs[0][0, ::7] = float("nan")              # NaN inputs stay confined to the rows that read them
    ref = [w.apply_device(x, force_conservation=False).clone() for x in xs]
    torch.cuda.synchronize()
    assert rel_linf(ref[-1].cpu().numpy(), o.apply(xs[-1].cpu().numpy())) <= FIELD_RTOL
    try:
        for qi in (0, 1, 2, 3, 16):
            icebin_amd.set_tuning("rowblock_many_qi", qi)
            outs = w.apply_many_device(xs, force_conservation=False)
            torch.cuda.synchronize()
            for q in range(nbatch):
                a, b = outs[q].cpu().numpy(), ref[q].cpu().numpy()
                np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64), err_msg="%s batch %d qi %d" % (name, q, qi))
    finally:
        icebin_amd.set_tuning("rowblock_many_qi", 0)


def test_apply_many_long_rows_and_graph_capture():
    # rows longer than one staged segment (1024 entries) re-stage per batch; the batched launch is
    # capturable (pointer table travels in the kernel arguments)
    import torch
    rng = np.random.default_rng(5)
    nrow, ncol = 7, 6000
    rowlen = [0, 1, 1023, 1024, 1025, 2500, 3000]
    rowptr = np.concatenate([[0], np.cumsum(rowlen)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(ncol, n, replace=False)) for n in rowlen]).astype(np.int32)
    val = rng.standard_normal(len(col))
    wM = np.ones(nrow); wM[0] = 0.0
    w = icebin_amd.linear_Weighted.from_csr((nrow, ncol), rowptr, col, val, wM, np.ones(ncol))
    w.set_kernel("rowblock")
    import scipy.sparse
    M = scipy.sparse.csr_matrix((val, col, rowptr), shape=(nrow, ncol))
    xs = [torch.from_numpy(rng.standard_normal((6, ncol))).cuda() for _ in range(5)]
    outs = [torch.empty((6, nrow), dtype=torch.float64, device="cuda") for _ in range(5)]
    w.apply_many_device(xs, outs, fill=-7.0, force_conservation=False)      # warm-up outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        w.apply_many_device(xs, outs, fill=-7.0, force_conservation=False)
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, o in zip(xs, outs):
        ref = (M @ x.cpu().numpy().T).T
        ref[:, 0] = -7.0
        got = o.cpu().numpy()
        assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))


# ---- the ordering primitive behind the assembly (prims.hip "adaptive ordering") ---------------------
def _selftest_sort(keys, lo_bits, hi_bits):
    import ctypes as C
    from icebin_amd import _capi
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    perm = np.empty(len(keys), np.uint32)
    path = C.c_int(-1)
    _capi.check(_capi.lib().ibh_selftest_sort(keys.ctypes.data, len(keys), lo_bits, hi_bits, perm.ctypes.data, C.byref(path)))
    return perm, path.value


def _pieces(rng, n, max_piece, lo_bits, disorder):
    """Keys whose high field grows piece by piece (cuts between pieces); inside a piece the low
    field is ascending except for a `disorder` fraction of out-of-place entries and duplicates."""
    keys = np.empty(n, np.uint64)
    k, hi = 0, 0
    while k < n:
        m = int(min(n - k, rng.integers(1, max_piece + 1)))
        lo = np.sort(rng.integers(0, 1 << lo_bits, m, dtype=np.uint64))
        j = rng.random(m) < disorder
        lo[j] = rng.integers(0, 1 << lo_bits, int(j.sum()), dtype=np.uint64)
        nrows = int(rng.integers(1, 4))               # a piece may span a few rows, interleaved
        keys[k:k + m] = ((hi + rng.integers(0, nrows, m).astype(np.uint64)) << np.uint64(32)) | lo
        hi += nrows
        k += m
    return keys


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["empty", "one", "two", "sorted", "all_equal", "small_pieces", "mid_pieces",
                                  "cap_piece", "over_cap", "random", "lo_sorted_hi_random", "tile_edges"])
def test_ordering_primitive_equals_stable_sort(case):
    rng = np.random.default_rng(20240501)
    lo_bits, hi_bits, want_path = 20, 12, None
    if case == "empty":
        keys = np.zeros(0, np.uint64)
    elif case == "one":
        keys = np.array([5], np.uint64)
    elif case == "two":
        keys = np.array([7, 3], np.uint64); want_path = 1
    elif case == "sorted":
        keys = np.sort(rng.integers(0, 1 << 20, 300001, dtype=np.uint64)); want_path = 0
    elif case == "all_equal":
        keys = np.full(100000, 9, np.uint64); want_path = 0
    elif case == "small_pieces":
        keys = _pieces(rng, 500000, 300, lo_bits, 0.1); want_path = 1
    elif case == "mid_pieces":
        keys = _pieces(rng, 700000, 7000, lo_bits, 0.05); want_path = 1
    elif case == "cap_piece":       # one piece of exactly 8192 and one of 2048 (the size-class edges), rest in order
        a = np.arange(8192, dtype=np.uint64)[::-1].copy()
        b = (np.uint64(1) << np.uint64(32)) | np.arange(2048, dtype=np.uint64)[::-1]
        c = (np.uint64(2) << np.uint64(32)) | np.arange(5000, dtype=np.uint64)
        keys = np.concatenate([a, b, c]); want_path = 1
    elif case == "over_cap":        # a piece of 8193 -> nothing may be touched by the piece kernels; radix sort
        a = np.arange(8193, dtype=np.uint64)[::-1].copy()
        b = (np.uint64(1) << np.uint64(32)) | np.array([3, 1, 2], np.uint64)
        keys = np.concatenate([a, b]); want_path = 2
    elif case == "random":
        keys = (rng.integers(0, 1 << hi_bits, 1 << 20, dtype=np.uint64) << np.uint64(32)) | rng.integers(0, 1 << lo_bits, 1 << 20, dtype=np.uint64)
        want_path = 2
    elif case == "lo_sorted_hi_random":   # the low field never decreases: only the high field is radix-sorted
        n = 400000
        keys = (rng.integers(0, 1 << hi_bits, n, dtype=np.uint64) << np.uint64(32)) | np.sort(rng.integers(0, 1 << lo_bits, n, dtype=np.uint64))
        want_path = 2
    else:                           # disorder straddling the 2048-element analysis tiles
        keys = np.arange(3 * 2048 + 5, dtype=np.uint64)
        for e in (2047, 2048, 4095, 4096, 6143):
            keys[e], keys[e + 1] = keys[e + 1], keys[e]
        want_path = 1
    perm, path = _selftest_sort(keys, lo_bits, hi_bits)
    ref = np.argsort(keys, kind="stable").astype(np.uint32)
    assert np.array_equal(perm, ref)
    if want_path is not None:
        assert path == want_path


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["IvA", "IvE"])
def test_shortrow_realigned_result_planes(name):
    """Result planes that do not start on 64-byte lines go through the LDS re-alignment of the
    shortrow kernel (spmm.hip): same arithmetic, so bit-identical to the plain store path, for every
    combination of odd leading dimension and base offset; nothing outside the planes is written."""
    import torch
    from icebin_amd.linear import set_tuning
    g = syn.make_grids("g5")
    W = icebin_amd.from_synthetic(g).regrid_matrices("greenland", syn.dome_elevmask(g)).matrix(name)
    nf, nrow, ncol = 7, W.nrow_d, W.ncol_d
    x = torch.from_numpy(syn.fields(nf, ncol)).cuda()
    try:
        set_tuning("shortrow_realign", 0)
        set_tuning("shortrow_xt", 0)
        ref = W.apply_device(x, out=torch.empty((nf, nrow), dtype=torch.float64, device="cuda")).cpu().numpy()
        # the transposed-input variant (16-byte loads of XT[c, f0:f0+G]) does the same arithmetic in the same order
        for xt, ra in ((1, 0), (1, 1)):
            set_tuning("shortrow_xt", xt); set_tuning("shortrow_realign", ra)
            got = W.apply_device(x, out=torch.empty((nf, nrow), dtype=torch.float64, device="cuda")).cpu().numpy()
            assert np.array_equal(got, ref, equal_nan=True), (xt, ra)
        set_tuning("shortrow_xt", -1)
        set_tuning("shortrow_realign", 1)
        for ld in (nrow, nrow + 1, nrow + 3, nrow + 8):
            for off in (0, 1, 5):
                buf = torch.full((nf * ld + 16,), -7.0, dtype=torch.float64, device="cuda")
                out = buf[off:off + nf * ld].view(nf, ld)[:, :nrow]
                W.apply_device(x, out=out)
                got = buf.cpu().numpy()
                planes = got[off:off + nf * ld].reshape(nf, ld)
                assert np.array_equal(planes[:, :nrow], ref, equal_nan=True)
                assert np.all(planes[:, nrow:] == -7.0) and np.all(got[:off] == -7.0) and np.all(got[off + nf * ld:] == -7.0)
    finally:
        set_tuning("shortrow_realign", -1)
        set_tuning("shortrow_xt", -1)


@pytest.mark.parametrize("nrow", [1, 7, 247, 248, 249, 255, 256, 257, 495, 496, 497, 1000])
def test_shortrow_variants_on_edge_sizes(nrow):
    """Plain / re-aligned / transposed-input shortrow launches on row counts around the 248-row step
    and the 256-thread workgroup, 0-3 entries per row, a dead (wM == 0) row, against numpy."""
    import torch
    from icebin_amd.linear import linear_Weighted, set_tuning
    rng = np.random.default_rng(nrow)
    ncol, nf = 5, 6
    cnt = rng.integers(0, 4, nrow)
    rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    colind = np.concatenate([np.sort(rng.choice(ncol, c, replace=False)) for c in cnt] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = rng.standard_normal(len(colind))
    wM = np.ones(nrow); wM[nrow // 2] = 0.0
    W = linear_Weighted.from_csr((nrow, ncol), rowptr, colind, val, wM, np.ones(ncol))
    W.set_kernel("shortrow")
    x = rng.standard_normal((nf, ncol))
    dense = np.zeros((nrow, ncol))
    for r in range(nrow):
        dense[r, colind[rowptr[r]:rowptr[r + 1]]] = val[rowptr[r]:rowptr[r + 1]]
    ref = x @ dense.T
    ref[:, nrow // 2] = -3.0
    xd = torch.from_numpy(x).cuda()
    try:
        for xt in (0, 1):
            for ra in (0, 1):
                set_tuning("shortrow_xt", xt); set_tuning("shortrow_realign", ra)
                for off in (0, 3):
                    buf = torch.full((nf * (nrow + 5) + 8,), 9.0, dtype=torch.float64, device="cuda")
                    out = buf[off:off + nf * (nrow + 5)].view(nf, nrow + 5)[:, :nrow]
                    W.apply_device(xd, out=out, fill=-3.0)
                    got = buf.cpu().numpy()
                    planes = got[off:off + nf * (nrow + 5)].reshape(nf, nrow + 5)
                    assert np.max(np.abs(planes[:, :nrow] - ref)) <= 1e-13 * max(1.0, np.max(np.abs(ref))), (xt, ra, off)
                    assert np.all(planes[:, nrow:] == 9.0) and np.all(got[:off] == 9.0) and np.all(got[off + nf * (nrow + 5):] == 9.0)
    finally:
        set_tuning("shortrow_realign", -1)
        set_tuning("shortrow_xt", -1)


@pytest.mark.parametrize("pattern", ["cell_by_cell", "two_columns", "scattered", "long_rows"])
def test_shortrow_shared_columns_are_bitwise_the_gather_form(pattern):
    """The I-row kernel with groups of four fields takes, wave by wave, the X values of the <= 2 columns per entry slot that its
    lanes share through scalar loads (spmm.hip "SHARED"); groups of eight never do.  Rows numbered cell by cell with edge rows of
    2-4 entries (the Antarctic IvA / IvE shape), waves with exactly two columns per slot, scattered columns (every wave falls
    back), rows of more than four entries (fallback), NaN fields, a dead row, a partial last wave: the two forms agree bit for bit
    and with numpy."""
    import torch
    from icebin_amd.linear import linear_Weighted
    rng = np.random.default_rng({"cell_by_cell": 1, "two_columns": 2, "scattered": 3, "long_rows": 4}[pattern])
    nrow, ncol, nf = 64 * 37 + 19, 300, 20
    r = np.arange(nrow)
    if pattern == "cell_by_cell":       # runs of 45 rows per "GCM cell" x 2 classes, the first and last row of a run with four entries
        cell = r // 45
        cols = [[2 * c, 2 * c + 1] if (k % 45) not in (0, 44) else ([2 * c - 2, 2 * c - 1, 2 * c, 2 * c + 1] if k % 45 == 0 and c > 0 else [2 * c, 2 * c + 1, 2 * c + 2, 2 * c + 3])
                for k, c in zip(r, cell)]
    elif pattern == "two_columns":      # every wave: lanes < 40 one column pair, the others another
        cols = [[(k // 64) % 100, 100 + (k // 64) % 100] if k % 64 < 40 else [(k // 64) % 100 + 1, 200 + (k // 64) % 90] for k in r]
    elif pattern == "scattered":
        cols = [sorted(rng.choice(ncol, rng.integers(0, 5), replace=False).tolist()) for _ in r]
    else:                               # most rows one entry in the wave's column, one row in 50 with seven
        cols = [[(k // 64) % ncol] if k % 50 else sorted(rng.choice(ncol, 7, replace=False).tolist()) for k in r]
    cnt = np.array([len(c) for c in cols])
    rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    colind = np.array([c for cc in cols for c in cc], np.int32)
    val = rng.standard_normal(len(colind))
    wM = np.ones(nrow); wM[777] = 0.0
    W = linear_Weighted.from_csr((nrow, ncol), rowptr, colind, val, wM, np.ones(ncol))
    W.set_kernel("shortrow")
    x = rng.standard_normal((nf, ncol)); x[3, ::7] = np.nan
    xd = torch.from_numpy(x).cuda()
    out = {}
    for grp in (4, 8):
        W.set_option("shortrow_xt", 1); W.set_option("shortrow_group", grp); W.set_option("shortrow_fper", 8)
        out[grp] = W.apply_device(xd, fill=-3.0).cpu().numpy().copy()
    assert np.array_equal(out[4], out[8], equal_nan=True)
    ref = np.full((nf, nrow), 0.0)
    for k in range(nrow):
        acc = np.zeros(nf)
        for j in range(rowptr[k], rowptr[k + 1]):
            acc = (val[j] * x[:, colind[j]]) if j == rowptr[k] else acc + val[j] * x[:, colind[j]]
        ref[:, k] = acc
    ref[:, 777] = -3.0
    ok = np.isfinite(ref)
    assert np.array_equal(np.isnan(out[4]), np.isnan(ref))
    assert np.max(np.abs(out[4][ok] - ref[ok])) <= 1e-13 * max(1.0, np.max(np.abs(ref[ok])))


def test_column_sums_with_long_columns():
    """Mw (column sums in ascending row order) when a few ice cells are overlapped by MANY atmosphere
    cells: the short-column path (csrbuild.hip k_col_sums) takes its selection branch (3..64 entries)
    and its one-wave-per-column branch (> 64), still bit-exact against the oracle."""
    g = syn.make_grids("g20")
    em = syn.dome_elevmask(g)
    ok = np.flatnonzero(np.isfinite(em))
    iA_all = np.unique(g["ex_indices"][:, 0])
    rng = np.random.default_rng(11)
    extra = []
    for iI, k in ((ok[10], 100), (ok[200], 40), (ok[500], 9)):           # 100, 40 and 9 extra atmosphere cells
        for a in rng.choice(iA_all, min(k, len(iA_all)), replace=False):
            extra.append((a, iI))
    extra = np.array(extra, np.int32)
    g = dict(g)
    g["ex_indices"] = np.concatenate([g["ex_indices"], extra]).astype(np.int32)
    g["ex_area"] = np.concatenate([g["ex_area"], 1e6 * (1.0 + rng.random(len(extra)))])
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    # IvA / IvE: the same cells are ROWS of 100 / 40 / 9 contributions: the per-row-slot build gives up
    # (> 32 in a row) and the sort-based path takes over
    for name in ("AvI", "EvI", "AvX", "IvA", "IvE"):
        assert_same_weighted(rm.matrix(name), rg.matrix_d(name, em, scale=True, correctA=True), name + " long columns")


def test_device_resident_elevation_mask():
    """regrid_matrices() from an elevation mask that is already in HBM builds the same matrices."""
    import torch
    g, em, mm, rg = setup("g20")
    emd = torch.from_numpy(em).cuda()
    rm = mm.regrid_matrices("greenland", emd, scale=True, correctA=True)
    for name in ("AvI", "EvI", "IvE"):
        assert_same_weighted(rm.matrix(name), rg.matrix_d(name, em, scale=True, correctA=True), name + " device mask")
    with pytest.raises(icebin_amd.IcebinHipError, match="elements"):
        mm.regrid_matrices("greenland", emd[:-1])


@pytest.mark.parametrize("variant", ["sorted", "shuffled", "elev_class"])
def test_rowdual_bands_on_grid_variants(variant):
    """The band structure (one entry per (GCM cell, ice cell) with both class weights) applied by the
    rowdual kernel, on the grid variants that change the pairing: shuffled exchange cells, straddling
    cells, one class per cell (ELEV_CLASS_INTERP: no partners at all)."""
    from icebin_amd.linear import set_tuning
    kw = dict(sorted={}, shuffled=dict(order="shuffled"), elev_class={})[variant]
    g = syn.make_grids("g50", **kw)
    if variant == "elev_class":
        g["interp_style"] = 1
    em = syn.dome_elevmask(g)
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    set_tuning("assemble_bands", 1)
    try:
        rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
        for name in ("EvI", "EvX"):
            w, o = rm.matrix(name), rg.matrix_d(name, em, scale=True, correctA=True)
            assert_same_weighted(w, o, name)
            x = syn.fields(9, w.ncol_d)
            x[3, ::7] = np.nan                      # NaN in a field must stay in the rows that use those cells
            w.set_kernel("rowdual")
            y = w.apply(x, fill=-1.0, force_conservation=False)
            assert w.last_kernel() == "rowdual"
            assert rel_linf(y, o.apply(x, fill=-1.0, force_conservation=False)) <= FIELD_RTOL
    finally:
        set_tuning("assemble_bands", 0)


@pytest.mark.parametrize("variant", ["sorted", "shuffled"])
def test_lazy_bands_on_repeated_applies_and_batched_rowdual(variant):
    # an E-row matrix that is applied again gets its band structure from its own CSR (either assembly path) and the
    # rowdual kernel takes over; batched launches serve it too, bitwise like separate rowdual applies
    import torch
    from icebin_amd.linear import set_tuning
    g = syn.make_grids("g20", **(dict(order="shuffled") if variant == "shuffled" else {}))
    em = syn.dome_elevmask(g)
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    set_tuning("rowdual_min_work", 1)
    try:
        rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
        for name in ("EvI", "EvX"):
            w, o = rm.matrix(name), rg.matrix_d(name, em, scale=True, correctA=True)
            assert w.built_fast() == (variant == "sorted")
            xs = [torch.from_numpy(syn.fields(6, w.ncol_d, seed=40 + q)).cuda() for q in range(5)]
            xs[1][2, ::5] = float("nan")
            y0 = w.apply_device(xs[0], fill=-1.0, force_conservation=False)
            torch.cuda.synchronize()
            assert w.last_kernel() == "rowblock"                     # first apply: no bands yet
            y1 = w.apply_device(xs[0], fill=-1.0, force_conservation=False)
            torch.cuda.synchronize()
            assert w.last_kernel() == "rowdual"                      # second apply: bands built from the CSR
            ref = o.apply(xs[0].cpu().numpy(), fill=-1.0, force_conservation=False)
            assert rel_linf(y0.cpu().numpy(), ref) <= FIELD_RTOL and rel_linf(y1.cpu().numpy(), ref) <= FIELD_RTOL
            sep = [w.apply_device(x, fill=-1.0, force_conservation=False).clone() for x in xs]
            outs = w.apply_many_device(xs, fill=-1.0, force_conservation=False)
            torch.cuda.synchronize()
            assert w.last_kernel() == "rowdual"
            for a, b, x in zip(outs, sep, xs):
                assert np.array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64))
                assert rel_linf(a.cpu().numpy(), o.apply(x.cpu().numpy(), fill=-1.0, force_conservation=False)) <= FIELD_RTOL
        # matrices of other shapes never grow bands
        w = rm.matrix("AvI")
        x = torch.from_numpy(syn.fields(6, w.ncol_d)).cuda()
        w.apply_device(x); w.apply_device(x)
        assert w.last_kernel() == "rowblock"
    finally:
        set_tuning("rowdual_min_work", 128 << 20)


@pytest.mark.parametrize("variant", ["sorted", "shuffled", "elev_class", "x_fastest"])
def test_colsweep_on_grid_variants(variant):
    """The column-sweep apply (sweep_kernel.inl: lanes = fields, every X element read once) of the E-row matrices against
    the oracle: full and partial field blocks (64, 40, 130, 7 fields), NaN-carrying fields, fill, both interpolation
    styles, both ice index orders, shuffled exchange cells (general assembly path)."""
    kw = dict(sorted={}, shuffled=dict(order="shuffled"), elev_class={}, x_fastest=dict(x_fastest=True))[variant]
    g = syn.make_grids("g5", **kw)      # (a 20 km grid is too coarse: 64 columns span several GCM cells, > 32 rows)
    if variant == "elev_class":
        g["interp_style"] = 1
    em = syn.dome_elevmask(g)
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    for name in ("EvI", "EvX"):
        w, o = rm.matrix(name), rg.matrix_d(name, em, scale=True, correctA=True)
        w.set_kernel("colsweep")
        for nvar in (64, 40, 130, 7):
            x = syn.fields(nvar, w.ncol_d, seed=7 + nvar)
            x[nvar // 2, ::7] = np.nan              # NaN in a field must stay in the rows that use those cells
            y = w.apply(x, fill=-1.0, force_conservation=False)
            # (a shuffled exchange grid scatters a GCM cell's ice cells over the dense numbering, and with x fastest 64
            # consecutive cells of this 5 km grid cross the steep side of the dome: 64 columns touch > 32 rows, the structure
            # is declined and the request falls back)
            expect = dict(sorted=("colsweep",), elev_class=("colsweep",), shuffled=("rowblock",), x_fastest=("colsweep", "rowblock"))[variant]
            assert w.last_kernel() in expect, (name, nvar)
            assert rel_linf(y, o.apply(x, fill=-1.0, force_conservation=False)) <= FIELD_RTOL, (name, nvar)
    # the structure is generic (entries by column, paired): any matrix with short columns can be swept on request ...
    w, o = rm.matrix("AvI"), rg.matrix_d("AvI", em, scale=True, correctA=True)
    w.set_kernel("colsweep")
    x = syn.fields(64, w.ncol_d)
    assert rel_linf(w.apply(x, force_conservation=False), o.apply(x, force_conservation=False)) <= FIELD_RTOL
    assert w.last_kernel() == ("colsweep" if variant != "shuffled" else "rowblock")      # AvI: one entry per column, few rows per block
    # ... one whose columns are long (64 items touch more rows than the kernel's table holds) falls back
    w, o = rm.matrix("IvA"), rg.matrix_d("IvA", em, scale=True, correctA=True)
    w.set_kernel("colsweep")
    x = syn.fields(64, w.ncol_d)
    assert rel_linf(w.apply(x, force_conservation=False), o.apply(x, force_conservation=False)) <= FIELD_RTOL
    assert w.last_kernel() in ("rowblock", "shortrow")


@pytest.fixture(params=["atomics", "tiles256", "tiles128"])
def rowgroup_form(request):
    """Both forms of the row-group apply (spmm.hip): the class sums in LDS tables through ds_add_f64 (spmm_rowgroup_kernel), and
    the tiled form with register sums (spmm_grouptile_kernel) in its two tile sizes -- whatever the automatic choice would be."""
    form = request.param
    icebin_amd.set_tuning("rowgroup_form", 0 if form == "atomics" else 1)
    if form != "atomics":
        icebin_amd.set_tuning("grouptile_seg", int(form[5:]))
    yield form
    icebin_amd.set_tuning("rowgroup_form", -2 ** 31)
    icebin_amd.set_tuning("grouptile_seg", -2 ** 31)


@pytest.mark.parametrize("variant", ["sorted", "shuffled", "elev_class", "x_fastest", "g20", "fine_classes"])
def test_rowgroup_on_grid_variants(variant, rowgroup_form):
    """The row-group apply of the E-row matrices (spmm.hip rowgroup / grouptile: the elevation classes of one GCM cell form a
    group whose columns are gathered once) against the oracle: 1..130 fields, NaN-carrying fields, fill, both interpolation
    styles, both ice index orders, shuffled exchange cells (general assembly path), a coarse grid (few cells per class), batched
    launches bitwise equal to separate applies, inside a hipGraph, and a shared dimE in a scrambled order (the rows of a group
    are not consecutive)."""
    import torch
    kw = dict(sorted={}, shuffled=dict(order="shuffled"), elev_class={}, x_fastest=dict(x_fastest=True), g20={}, fine_classes=dict(nhc=64))[variant]
    g = syn.make_grids("g20" if variant == "g20" else "g5", **kw)
    if variant == "elev_class":
        g["interp_style"] = 1
    if variant == "fine_classes":           # 64 classes 60 m apart: GCM cells with 17..32 classes (the kernels' second instantiation)
        g["hcdefs"] = np.arange(64, dtype=np.float64) * 60.0 - 30.0
    em = syn.dome_elevmask(g)
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    for name in ("EvI", "EvX"):
        w, o = rm.matrix(name), rg.matrix_d(name, em, scale=True, correctA=True)
        w.set_kernel("rowgroup")
        if variant == "fine_classes" and rowgroup_form != "atomics":
            w.apply(syn.fields(4, w.ncol_d), fill=-1.0, force_conservation=False)
            assert "grouptile_kernel<16, 32," in w.last_launch(), w.last_launch()      # groups of 17..32 rows
        for nvar in (64, 40, 130, 7, 1):
            x = syn.fields(nvar, w.ncol_d, seed=7 + nvar)
            x[nvar // 2, ::7] = np.nan              # NaN in a field must stay in the rows that use those cells
            ref = o.apply(x, fill=-1.0, force_conservation=False)
            # class tables of half width (two lanes per entry: the default below 2^20 entries) and of full width
            for tw in (None, 64, 32) if nvar in (64, 7) else (None,):
                if tw is not None:
                    icebin_amd.set_tuning("rowgroup_tw", tw)
                try:
                    y = w.apply(x, fill=-1.0, force_conservation=False)
                finally:
                    icebin_amd.set_tuning("rowgroup_tw", -2 ** 31)
                assert w.last_kernel() == "rowgroup", (name, nvar)
                assert ("grouptile" in w.last_launch()) == (rowgroup_form != "atomics"), w.last_launch()
                assert rel_linf(y, ref) <= FIELD_RTOL, (name, nvar, tw)
        if name == "EvI":
            xs = [torch.from_numpy(syn.fields(16, w.ncol_d, seed=400 + q)).cuda() for q in range(5)]
            xs[2][3, ::5] = float("nan")
            sep = [w.apply_device(x, fill=-1.0, force_conservation=False).clone() for x in xs]
            outs = [torch.zeros_like(sep[0]) for _ in xs]
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                w.apply_many_device(xs, outs, fill=-1.0, force_conservation=False)
            gr.replay()
            torch.cuda.synchronize()
            assert w.last_kernel() == "rowgroup"
            for a, b, x in zip(outs, sep, xs):
                assert np.array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64))
                assert rel_linf(a.cpu().numpy(), o.apply(x.cpu().numpy(), fill=-1.0, force_conservation=False)) <= FIELD_RTOL
    # a shared dimE in a scrambled order, holding keys this mask never touches (rows without entries: 0, or fill when wM == 0)
    o = rg.matrix_d("EvI", em, scale=True, correctA=True)
    nE = g["nA"] * len(g["hcdefs"])
    extra = np.setdiff1d(np.arange(nE), o.dims[0])[:5]
    perm = np.random.default_rng(5).permutation(np.concatenate([o.dims[0], extra]))
    dimE, odimE = icebin_amd.SparseSet(nE, perm), orc.SparseSet(nE, init=perm)
    w2 = rm.matrix_d("EvI", (dimE, None), scale=True, correctA=True)
    o2 = rg.matrix_d("EvI", em, (odimE, None), scale=True, correctA=True)
    assert_same_weighted(w2, o2, "EvI scrambled dimE")
    w2.set_kernel("rowgroup")
    x = syn.fields(24, w2.ncol_d)
    y = w2.apply(x, fill=-1.0, force_conservation=False)
    assert w2.last_kernel() == "rowgroup"
    assert rel_linf(y, o2.apply(x, fill=-1.0, force_conservation=False)) <= FIELD_RTOL
    # automatic choice: a matrix below the column sweep's size gets its row groups from ibh_weighted_prepare -- or, on request
    # (rowgroup_after), lazily from the n-th apply on; without either every apply runs row by row
    if variant == "sorted":
        x = syn.fields(16, o.ncol, seed=9)
        ref = o.apply(x, fill=-1.0, force_conservation=False)
        for after, expect in ((None, ["rowblock"] * 5), (3, ["rowblock"] * 3 + ["rowgroup"] * 2)):
            if after is not None:
                icebin_amd.set_tuning("rowgroup_after", after)
            try:
                w4 = rm.matrix("EvI")
                kernels = []
                for _ in range(5):
                    y = w4.apply(x, fill=-1.0, force_conservation=False)
                    kernels.append(w4.last_kernel())
                    assert rel_linf(y, ref) <= FIELD_RTOL
                assert kernels == expect, kernels
            finally:
                icebin_amd.set_tuning("rowgroup_after", -2 ** 31)
        w5 = rm.matrix("EvI")
        w5.prepare(16, 4)
        assert rel_linf(w5.apply(x, fill=-1.0, force_conservation=False), ref) <= FIELD_RTOL and w5.last_kernel() == "rowgroup"
        y1 = w5.apply(x[:1], fill=-1.0, force_conservation=False)            # fewer than 4 fields: the row kernel splits the row over the waves
        assert w5.last_kernel() == "rowblock" and rel_linf(y1, ref[:1]) <= FIELD_RTOL
    # matrices without elevation-class rows have no groups: the request falls back
    w3 = rm.matrix("AvI")
    w3.set_kernel("rowgroup")
    w3.apply(syn.fields(8, w3.ncol_d), force_conservation=False)
    assert w3.last_kernel() == "rowblock"


def test_colsweep_lazy_build_batched_and_shared_dims():
    # with >= 32 fields an E-row matrix that is applied again gets the column-sweep structure from its CSR; batched launches
    # are bitwise separate applies (also inside a hipGraph once the structure exists); a shared dimE in a permuted order
    # (rows of one GCM cell no longer consecutive: small groups) stays correct
    import torch
    from icebin_amd.linear import set_tuning
    g, em, mm, rg = setup("g5")
    set_tuning("sweep_min_work", 1)
    set_tuning("rowgroup_auto", 0)          # (with >= 32 fields the automatic choice for an E-row matrix is the row groups now)
    try:
        rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
        w, o = rm.matrix("EvI"), rg.matrix_d("EvI", em, scale=True, correctA=True)
        xs = [torch.from_numpy(syn.fields(64, w.ncol_d, seed=60 + q)).cuda() for q in range(5)]
        xs[1][2, ::5] = float("nan")
        y0 = w.apply_device(xs[0], fill=-1.0, force_conservation=False)
        torch.cuda.synchronize()
        assert w.last_kernel() == "rowblock"                     # first apply: nothing built yet
        y1 = w.apply_device(xs[0], fill=-1.0, force_conservation=False)
        torch.cuda.synchronize()
        assert w.last_kernel() == "colsweep"                     # second apply: structure built from the CSR
        ref = o.apply(xs[0].cpu().numpy(), fill=-1.0, force_conservation=False)
        assert rel_linf(y0.cpu().numpy(), ref) <= FIELD_RTOL and rel_linf(y1.cpu().numpy(), ref) <= FIELD_RTOL
        sep = [w.apply_device(x, fill=-1.0, force_conservation=False).clone() for x in xs]
        outs = w.apply_many_device(xs, fill=-1.0, force_conservation=False)
        torch.cuda.synchronize()
        assert w.last_kernel() == "colsweep"
        for a, b, x in zip(outs, sep, xs):
            assert np.array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64))
            assert rel_linf(a.cpu().numpy(), o.apply(x.cpu().numpy(), fill=-1.0, force_conservation=False)) <= FIELD_RTOL
        # stream capture (scratch is sized: the batch above was larger)
        out = torch.empty_like(sep[0])
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            w.apply_device(xs[2], out=out, fill=-1.0, force_conservation=False)
        out.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), sep[2].cpu().numpy().view(np.uint64))
        # fewer than 32 fields keep the row-by-row kernels
        w.apply_device(xs[0][:8].contiguous(), force_conservation=False)
        assert w.last_kernel() in ("rowblock", "rowdual")
        # shared dimE in a scrambled order
        perm = np.random.default_rng(5).permutation(o.dims[0])
        dimE, odimE = icebin_amd.SparseSet(g["nA"] * 40, perm), orc.SparseSet(g["nA"] * 40, init=perm)
        w2 = rm.matrix_d("EvI", (dimE, None), scale=True, correctA=True)
        o2 = rg.matrix_d("EvI", em, (odimE, None), scale=True, correctA=True)
        assert_same_weighted(w2, o2, "EvI scrambled dimE")
        w2.set_kernel("colsweep")
        x = syn.fields(64, w2.ncol_d)
        y = w2.apply(x, fill=-1.0, force_conservation=False)
        assert w2.last_kernel() == "colsweep"
        assert rel_linf(y, o2.apply(x, fill=-1.0, force_conservation=False)) <= FIELD_RTOL
    finally:
        set_tuning("sweep_min_work", 64 << 20)
        set_tuning("rowgroup_auto", 1)


def test_prepare_makes_applies_pure_enqueues():
    # ibh_weighted_prepare(w, nvar, nbatch): the structure an apply would build lazily on its second call exists before the
    # FIRST one, scratch is sized for the batch depth, so a batched apply can be captured right away and equals the eager
    # one bitwise; with lazy_structures = 0 an unprepared matrix never builds inside an apply
    import torch
    from icebin_amd.linear import set_tuning
    g, em, mm, rg = setup("g5")
    set_tuning("sweep_min_work", 1)
    try:
        rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
        o = rg.matrix_d("EvI", em, scale=True, correctA=True)
        xs = [torch.from_numpy(syn.fields(64, o.ncol, seed=80 + q)).cuda() for q in range(6)]
        xs[3][5, ::11] = float("nan")
        # unprepared, lazy builds off: every apply stays on the row-by-row kernel
        set_tuning("lazy_structures", 0)
        w0 = rm.matrix("EvI")
        for _ in range(3):
            w0.apply_device(xs[0], fill=-1.0, force_conservation=False)
        torch.cuda.synchronize()
        assert w0.last_kernel() == "rowblock"
        set_tuning("lazy_structures", 1)
        # prepared: the row groups from the first apply on, single and batched, eager == captured
        w = rm.matrix("EvI")
        w.prepare(64, len(xs))
        y = w.apply_device(xs[0], fill=-1.0, force_conservation=False)
        torch.cuda.synchronize()
        assert w.last_kernel() == "rowgroup"
        assert rel_linf(y.cpu().numpy(), o.apply(xs[0].cpu().numpy(), fill=-1.0, force_conservation=False)) <= FIELD_RTOL
        outs = [torch.zeros((64, w.nrow_d), dtype=torch.float64, device="cuda") for _ in xs]
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):                       # no warm-up apply_many before the capture: prepare() sized the scratch
            w.apply_many_device(xs, outs, fill=-1.0, force_conservation=False)
        gr.replay()
        torch.cuda.synchronize()
        assert w.last_kernel() == "rowgroup"
        eager = w.apply_many_device(xs, fill=-1.0, force_conservation=False)
        torch.cuda.synchronize()
        for a, b, x in zip(outs, eager, xs):
            assert np.array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64))
            assert rel_linf(a.cpu().numpy(), o.apply(x.cpu().numpy(), fill=-1.0, force_conservation=False)) <= FIELD_RTOL
        # fewer than 32 fields in batched launches: the column sweep (batches share its lanes), scratch sized for the depth
        ws = rm.matrix("EvI")
        x16 = [x[:16].contiguous() for x in xs[:4]]
        ws.prepare(16, 4)
        o16 = [torch.zeros((16, ws.nrow_d), dtype=torch.float64, device="cuda") for _ in x16]
        gr3 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr3):
            ws.apply_many_device(x16, o16, fill=-1.0, force_conservation=False)
        gr3.replay()
        torch.cuda.synchronize()
        assert ws.last_kernel() == "colsweep"
        for a, x in zip(o16, x16):
            assert rel_linf(a.cpu().numpy(), o.apply(x.cpu().numpy(), fill=-1.0, force_conservation=False)) <= FIELD_RTOL
        # an I-row matrix: the transposed-input scratch of a deep launch is sized too
        wi, oi = rm.matrix("IvE"), rg.matrix_d("IvE", em, scale=True, correctA=True)
        xe = [torch.from_numpy(syn.fields(16, wi.ncol_d, seed=90 + q)).cuda() for q in range(8)]
        wi.prepare(16, len(xe))
        oute = [torch.zeros((16, wi.nrow_d), dtype=torch.float64, device="cuda") for _ in xe]
        gr2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr2):
            wi.apply_many_device(xe, oute, fill=-1.0, force_conservation=False)
        gr2.replay()
        torch.cuda.synchronize()
        for a, x in zip(oute, xe):
            assert rel_linf(a.cpu().numpy(), oi.apply(x.cpu().numpy(), fill=-1.0, force_conservation=False)) <= FIELD_RTOL
        # a structure the sweep declines (long columns: 64 items touch more rows than its table holds) fails neither
        # prepare() nor the applies, which stay on the row kernel
        wl = rm.matrix("IvA")
        wl.set_kernel("colsweep")
        wl.prepare(64, 2)
        wl.apply_device(torch.from_numpy(syn.fields(64, wl.ncol_d)).cuda(), force_conservation=False)
        torch.cuda.synchronize()
        assert wl.last_kernel() in ("rowblock", "shortrow")
        from icebin_amd import _capi
        _capi.check(_capi.lib().ibh_release_cached_memory())       # all threads' workspaces; handles stay valid
        y2 = w.apply_device(xs[0], fill=-1.0, force_conservation=False)
        torch.cuda.synchronize()
        assert np.array_equal(y2.cpu().numpy().view(np.uint64), y.cpu().numpy().view(np.uint64))
    finally:
        set_tuning("sweep_min_work", 64 << 20)
        set_tuning("lazy_structures", 1)


@pytest.mark.parametrize("nvar,nbatch", [(16, 4), (16, 5), (8, 9), (12, 8), (24, 3), (32, 2), (5, 33)])
def test_colsweep_batches_share_lanes(nvar, nbatch):
    # fewer than 33 fields per batch: the 64 lanes of the sweep are (batch, field) pairs -- 64 / nfl batches of a batched launch
    # share a wave (they sweep the same columns and feed the same rows); ragged last slices, field counts that are not powers of
    # two, more than 32 batches; automatic choice: taken on the second apply once enough lanes carry data
    import torch
    from icebin_amd.linear import set_tuning
    g, em, mm, rg = setup("g5")
    set_tuning("sweep_min_work", 1)
    set_tuning("rowgroup_auto", 0)          # (32 fields would go to the row groups)
    try:
        rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
        w, o = rm.matrix("EvI"), rg.matrix_d("EvI", em, scale=True, correctA=True)
        xs = [torch.from_numpy(syn.fields(nvar, w.ncol_d, seed=300 + q)).cuda() for q in range(nbatch)]
        xs[nbatch // 2][nvar - 1, ::9] = float("nan")
        w.apply_many_device(xs, fill=-2.0, force_conservation=False)         # first apply: nothing built yet
        outs = w.apply_many_device(xs, fill=-2.0, force_conservation=False)
        torch.cuda.synchronize()
        lanes = 64 if nvar > 32 else nvar * min(nbatch, 64 // (8 if nvar <= 8 else 16 if nvar <= 16 else 32))
        assert w.last_kernel() == ("colsweep" if lanes >= 32 else "rowblock")
        for q in (0, nbatch // 2, nbatch - 1):
            assert rel_linf(outs[q].cpu().numpy(), o.apply(xs[q].cpu().numpy(), fill=-2.0, force_conservation=False)) <= FIELD_RTOL
        w.set_kernel("colsweep")                                             # on request also with few lanes
        y = w.apply_device(xs[0], fill=-2.0, force_conservation=False)
        torch.cuda.synchronize()
        assert w.last_kernel() == "colsweep"
        assert rel_linf(y.cpu().numpy(), o.apply(xs[0].cpu().numpy(), fill=-2.0, force_conservation=False)) <= FIELD_RTOL
    finally:
        set_tuning("sweep_min_work", 64 << 20)
        set_tuning("rowgroup_auto", 1)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_colsweep_on_random_structures(seed):
    """The column sweep on request for matrices it was not designed around: random columns with 0..5 entries (empty columns:
    column != item index; more than two entries: several items per column), rows from a window that drifts along the columns
    (few rows per 64 items), wM == 0 rows (fill), 33 batches in one call (> 32: two launches), 1..70 fields."""
    import torch
    rng = np.random.default_rng(100 + seed)
    nrow, ncol = 400, 9000 + 37 * seed
    rows, cols = [], []
    for c in range(ncol):
        k = int(rng.integers(0, 6)) if c % 11 else 0          # every 11th column is empty
        base = c * (nrow - 12) // ncol
        for r in rng.choice(12, size=k, replace=False):
            rows.append(base + int(r)); cols.append(c)
    rows, cols = np.array(rows), np.array(cols)
    vals = rng.standard_normal(len(rows))
    wM = rng.random(nrow) + 0.5
    wM[::17] = 0.0
    Mw = rng.random(ncol) + 0.5
    w = icebin_amd.linear_Weighted.from_coo((nrow, ncol), rows, cols, vals, wM, Mw)
    o = orc.Weighted.from_coo(nrow, ncol, rows, cols, vals, wM, Mw)
    w.set_kernel("colsweep")
    for nvar in (64, 70, 1):
        x = rng.standard_normal((nvar, ncol))
        x[0, ::13] = np.nan
        y = w.apply(x, fill=-3.0, force_conservation=False)
        assert w.last_kernel() == "colsweep"
        assert rel_linf(y, o.apply(x, fill=-3.0, force_conservation=False)) <= FIELD_RTOL
    xs = [torch.from_numpy(rng.standard_normal((64, ncol))).cuda() for _ in range(33)]
    outs = w.apply_many_device(xs, fill=-3.0, force_conservation=False)
    torch.cuda.synchronize()
    for q in (0, 31, 32):
        assert rel_linf(outs[q].cpu().numpy(), o.apply(xs[q].cpu().numpy(), fill=-3.0, force_conservation=False)) <= FIELD_RTOL


def _random_grid(seed, force_sorted=False):
    rng = np.random.default_rng(1000 + seed)
    nA_real, nI, nhc = int(rng.integers(3, 40)), int(rng.integers(20, 600)), int(rng.integers(2, 12))
    im, jm = 12, 8
    nA = im * jm
    A_to_sparse = np.sort(rng.choice(nA, nA_real, replace=False)).astype(np.int64)
    nX = int(rng.integers(50, 3000))
    iA = rng.choice(A_to_sparse, nX)
    iI = rng.integers(0, nI, nX)
    if force_sorted:
        # inside the limits of the plan-based build: <= 8 exchange cells per ice cell, <= 3 cells with the same (iA, iI)
        o = np.lexsort((iA, iI)); iA, iI = iA[o], iI[o]
        first = np.r_[True, iI[1:] != iI[:-1]]
        rank_in_ice = np.arange(nX) - np.maximum.accumulate(np.where(first, np.arange(nX), 0))
        firstp = np.r_[True, (iI[1:] != iI[:-1]) | (iA[1:] != iA[:-1])]
        rank_in_pair = np.arange(nX) - np.maximum.accumulate(np.where(firstp, np.arange(nX), 0))
        keep = (rank_in_ice < 8) & (rank_in_pair < 3)
        iA, iI = iA[keep], iI[keep]
        nX = len(iA)
    if seed % 3 == 0 or force_sorted:    # a sorted grid (the reference's normal case), else arbitrary order
        o = np.lexsort((iI, iA)); iA, iI = iA[o], iI[o]
    area = 1e6 * (0.5 + rng.random(nX))
    area[rng.random(nX) < 0.03] = 0.0
    if seed % 4 == 1:
        area[rng.random(nX) < 0.05] *= -1.0
    hcdefs = np.sort(rng.random(nhc)) * 3000.0
    hcdefs[0] = -50.0
    em = rng.random(nI) * (hcdefs[-1] - 1.0)
    em[rng.random(nI) < 0.3] = np.nan
    em[rng.random(nI) < 0.05] = hcdefs[int(rng.integers(0, nhc))]     # exactly on a class boundary (weight 0 dropped)
    proj = 1e9 * (1.0 + rng.random(nA_real))
    g = dict(config="random", nx=nI, ny=1, dx=1.0, x_fastest=False, nI=nI, nA=nA, im=im, jm=jm,
             ex_indices=np.stack([iA, iI], axis=1).astype(np.int32), ex_area=area, A_to_sparse=A_to_sparse,
             A_native_area=proj * (1.0 + 0.05 * rng.random(nA_real)), A_proj_area=proj, hcdefs=hcdefs,
             hc_stride_A=1 if seed % 2 == 0 else nhc, hc_stride_HC=nA if seed % 2 == 0 else 1,
             interp_style=1 if seed % 5 == 4 else 0, I_centroid_xy=np.zeros((nI, 2)))
    return g, em


@pytest.mark.parametrize("seed", list(range(10)))
def test_random_exchange_grids_bit_exact(seed):
    """Randomised differential test of the whole assembly against the oracle: arbitrary (iA, iI) pairs
    (duplicates, any order, ice cells under many atmosphere cells), random masks, zero / negative
    overlaps, both interpolation styles, both indexingHC layouts -- every ordering path (in order,
    pieces, radix, optimistic row-only sort and its failed check), both column-sum paths."""
    g, em = _random_grid(seed)
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    rm = mm.regrid_matrices("greenland", em)
    for name in ALL:
        for scale, correctA in ((True, True), (False, False)):
            w = rm.matrix_d(name, scale=scale, correctA=correctA)
            o = rg.matrix_d(name, em, scale=scale, correctA=correctA)
            assert_same_weighted(w, o, "%s scale=%d correctA=%d seed=%d" % (name, scale, correctA, seed))
            if w.nnz and name in ("AvI", "IvE", "EvI"):
                x = syn.fields(3, w.ncol_d, seed=seed)
                assert rel_linf(w.apply(x, fill=-9.0), o.apply(x, fill=-9.0)) <= FIELD_RTOL


@pytest.mark.parametrize("seed", list(range(10)))
def test_random_sorted_grids_on_every_variant_of_the_plan_based_build(seed):
    """The same random grids, sorted (so the plan-based build takes them when its limits allow: duplicates, ice cells under many
    atmosphere cells, zero / negative areas, masks, cells exactly on a class boundary), with the variants that large grids
    select forced on: the streamed count of the one-class matrices, every workgroup shape of the per-range kernels, the static
    and the visiting row count -- all against the oracle's bits."""
    g, em = _random_grid(seed, force_sorted=True)
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    rm = mm.regrid_matrices("greenland", em)
    try:
        icebin_amd.set_tuning("assemble_stream_count", 1)
        icebin_amd.set_tuning("assemble_range_shape", seed % 4)
        icebin_amd.set_tuning("assemble_static_count", seed % 2)
        icebin_amd.set_tuning("assemble_stream_rowsl", (seed // 2) % 2)        # (the lane-parallel row kernel of the streamed build ...
        icebin_amd.set_tuning("assemble_stream_rowsl_r", (1, 3, 16, 5, 2)[seed % 5])      # ... and its ranges per wave)
        for stream in (0, 1):                   # the per-range kernels (fastasm.inl), then the streamed build (streamasm.inl)
            icebin_amd.set_tuning("assemble_stream", stream)
            fast = streamed = 0
            for name in ALL:
                for scale, correctA in ((True, True), (False, False)):
                    w = rm.matrix_d(name, scale=scale, correctA=correctA)
                    fast += int(w.built_fast())
                    streamed += int(w.built_streamed())
                    assert_same_weighted(w, rg.matrix_d(name, em, scale=scale, correctA=correctA), "%s seed=%d stream=%d" % (name, seed, stream))
            assert fast >= 12, fast             # (EvA / AvE with negative areas, and little else, go to the general pipeline)
            assert streamed == (16 if stream else 0), (stream, streamed)       # all but EvA / AvE
    finally:
        for k in ("assemble_stream_count", "assemble_range_shape", "assemble_static_count", "assemble_stream", "assemble_stream_rowsl", "assemble_stream_rowsl_r"):
            icebin_amd.set_tuning(k, -2 ** 31)


@pytest.mark.parametrize("rowsl", [0, 1])
@pytest.mark.parametrize("config,variant", [("g50", "sorted"), ("g50", "zero_area"), ("g50", "negative_area"), ("g50", "elev_class"),
                                            ("g20", "sorted"), ("g20", "x_fastest"), ("g5", "sorted")])
def test_streamed_build_is_the_oracle_bitwise(config, variant, rowsl):
    """The streamed build (streamasm.inl: what grids of 2^20 exchange cells and more take) forced on the oracle-sized grids:
    the eight matrices it serves x the four (scale, correctA) branches, own dims; identity I / X sets where it serves them;
    the coupler's shared dimE, also permuted and incomplete -- every bit of dims / CSR / wM / Mw against the oracle."""
    kw = {}
    if variant == "zero_area":
        kw["zero_area_every"] = 7
    if variant == "x_fastest":
        kw["x_fastest"] = True
    g = syn.make_grids(config, **kw)
    if variant == "negative_area":
        g["ex_area"] = g["ex_area"].copy()
        g["ex_area"][::11] *= -1.0
    if variant == "elev_class":
        g["interp_style"] = 1
    em = syn.dome_elevmask(g)
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    nI, nX, nE = g["nI"], len(g["ex_area"]), g["nA"] * len(g["hcdefs"])
    names = [n for n in ALL if n not in ("EvA", "AvE")]
    try:
        icebin_amd.set_tuning("assemble_stream", 1)
        # waves per range of the byte pass (by default chosen by the mean range length): every shape is walked
        icebin_amd.set_tuning("assemble_stream_wpr", {("g20", "sorted"): 4, ("g20", "x_fastest"): 16, ("g50", "negative_area"): 16,
                                                      ("g50", "elev_class"): 4}.get((config, variant), -2 ** 31))
        icebin_amd.set_tuning("assemble_stream_oldseg", 512 if variant in ("x_fastest", "zero_area") else -2 ** 31)   # (the table size of the straddler sort)
        icebin_amd.set_tuning("assemble_stream_rows4", {"sorted": 1, "negative_area": 0, "elev_class": 1}.get(variant, -2 ** 31))   # (segments per wave of the row kernel)
        icebin_amd.set_tuning("assemble_stream_rowsl", rowsl)       # (1: the lane-parallel row kernel, sixteen chains per wave)
        for scale, correctA in ((True, True), (False, False), (True, False), (False, True)):
            rm = mm.regrid_matrices("greenland", em, scale=scale, correctA=correctA)
            for name in names:
                w = rm.matrix(name)
                assert w.built_streamed(), name
                assert_same_weighted(w, rg.matrix_d(name, em, scale=scale, correctA=correctA), "%s %s scale=%d correctA=%d" % (name, variant, scale, correctA))
        rm = mm.regrid_matrices("greenland", em)
        # the coupler's step (IceCoupler.cpp:361-468): EvI / AvI on an identity dimI, IvE on it and the dimE EvI numbered (its rows lie
        # in ice-cell order: row lengths scattered by ice cell, scanned over the ice cells), XvE on that dimE and an identity dimX
        dimI, dimX, dimE = icebin_amd.SparseSet.identity(nI), icebin_amd.SparseSet.identity(nX), icebin_amd.SparseSet(nE)
        oI, oX, oE = orc.SparseSet(nI, init=np.arange(nI)), orc.SparseSet(nX, init=np.arange(nX)), orc.SparseSet(nE)
        for name, dims, odims, sc, cA, streamed in (("EvI", (dimE, dimI), (oE, oI), False, False, True), ("AvI", (None, dimI), (None, oI), False, True, True),
                                                    ("IvE", (dimI, dimE), (oI, oE), True, True, True), ("XvE", (dimX, dimE), (oX, oE), False, True, True),
                                                    ("IvE", (None, dimE), (None, oE), True, True, True), ("AvX", (None, dimX), (None, oX), True, True, True),
                                                    ("IvA", (dimI, None), (oI, None), True, False, True), ("IvE", (dimI, None), (oI, None), False, False, True)):
            w = rm.matrix_d(name, dims, scale=sc, correctA=cA)
            assert w.built_fast() and w.built_streamed() == streamed, name
            assert_same_weighted(w, rg.matrix_d(name, em, dims=odims, scale=sc, correctA=cA), "coupler %s %s" % (name, variant))
        E_keys = dimE.to_sparse()
        extra = np.setdiff1d(np.arange(nE), E_keys)[:7]
        perm = np.random.default_rng(5).permutation(np.concatenate([E_keys, extra]))
        for name, rowset, orow in (("IvE", None, None), ("XvE", dimX, oX), ("XvE", None, None), ("IvE", dimI, oI)):
            dE2, oE2 = icebin_amd.SparseSet(nE, perm), orc.SparseSet(nE, init=perm)
            w = rm.matrix_d(name, (rowset, dE2), scale=True, correctA=True)
            assert w.built_streamed(), name
            assert_same_weighted(w, rg.matrix_d(name, em, dims=(orow, oE2), scale=True, correctA=True), "permuted dimE %s %s" % (name, variant))
        dE3, oE3 = icebin_amd.SparseSet(nE, E_keys[:-3]), orc.SparseSet(nE, init=E_keys[:-3])
        w = rm.matrix_d("XvE", (dimX, dE3), scale=True, correctA=True)              # a key is missing: the general pipeline appends it
        assert not w.built_fast() and dE3.dense_extent() == len(E_keys)
        assert_same_weighted(w, rg.matrix_d("XvE", em, dims=(oX, oE3), scale=True, correctA=True), "incomplete dimE " + variant)
    finally:
        icebin_amd.set_tuning("assemble_stream", -2 ** 31)
        icebin_amd.set_tuning("assemble_stream_wpr", -2 ** 31)
        icebin_amd.set_tuning("assemble_stream_oldseg", -2 ** 31)
        icebin_amd.set_tuning("assemble_stream_rows4", -2 ** 31)
        icebin_amd.set_tuning("assemble_stream_rowsl", -2 ** 31)


@pytest.mark.parametrize("nA_real,nX", [(12, 150000), (60, 200000)])
def test_random_exchange_grids_large_pieces(nA_real, nX):
    """Same, at sizes where a GCM cell's contributions exceed the LDS piece classes (2048 / 4096 /
    8192: the first case falls back to the radix sort for AvI, the second lands in the upper classes)."""
    rng = np.random.default_rng(77 + nA_real)
    nI, nhc, im, jm = 60000, 8, 12, 8
    nA = im * jm
    A_to_sparse = np.sort(rng.choice(nA, nA_real, replace=False)).astype(np.int64)
    iA = rng.choice(A_to_sparse, nX)
    iI = rng.integers(0, nI, nX)
    o = np.lexsort((iI, iA)); iA, iI = iA[o], iI[o]
    hcdefs = np.linspace(-50.0, 3000.0, nhc)
    em = rng.random(nI) * 2900.0
    em[rng.random(nI) < 0.3] = np.nan
    proj = 1e9 * (1.0 + rng.random(nA_real))
    g = dict(config="random", nx=nI, ny=1, dx=1.0, x_fastest=False, nI=nI, nA=nA, im=im, jm=jm,
             ex_indices=np.stack([iA, iI], axis=1).astype(np.int32), ex_area=1e6 * (0.5 + rng.random(nX)),
             A_to_sparse=A_to_sparse, A_native_area=proj * 1.01, A_proj_area=proj, hcdefs=hcdefs,
             hc_stride_A=1, hc_stride_HC=nA, interp_style=0, I_centroid_xy=np.zeros((nI, 2)))
    mm, rg = icebin_amd.from_synthetic(g), orc.Regridder(g)
    rm = mm.regrid_matrices("greenland", em)
    for name in ("AvI", "EvI", "IvE", "EvA", "XvE"):
        assert_same_weighted(rm.matrix_d(name, scale=True, correctA=True), rg.matrix_d(name, em, scale=True, correctA=True),
                             "%s nA=%d" % (name, nA_real))


def test_per_handle_options_do_not_leak_between_matrices():
    """ibh_weighted_set_option: a launch option set on ONE matrix changes the kernel its applies take and nothing about another
    matrix's -- the process-wide ibh_set_tuning map is for experiments; the result stays within the documented tolerance."""
    import torch
    g, em, mm, rg = setup("g5")
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    a, b = rm.matrix("EvI"), rm.matrix("EvI")
    x = torch.from_numpy(syn.fields(16, a.ncol_d, seed=3)).cuda()
    a.set_option("rowgroup_auto", 0)                       # this handle: no row groups
    for w in (a, b):
        w.prepare(16, 1)
    ya, yb = a.apply_device(x, force_conservation=False), b.apply_device(x, force_conservation=False)
    torch.cuda.synchronize()
    assert b.last_kernel() == "rowgroup" and a.last_kernel() != "rowgroup", (a.last_kernel(), b.last_kernel())
    assert rel_linf(ya.cpu().numpy(), yb.cpu().numpy()) <= FIELD_RTOL
    a.set_option("rowgroup_auto", None)                    # removed: back to the default choice
    a.prepare(16, 1)
    a.apply_device(x, force_conservation=False)
    torch.cuda.synchronize()
    assert a.last_kernel() == "rowgroup"
