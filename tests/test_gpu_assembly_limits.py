"""The sorted-grid builds at every path threshold and fallback limit (tests/assembly_limit_cases.py), on a real MI355X: every case
asserts the path that built each matrix (ibh_weighted_built_fast) and compares the matrix bit for bit with the oracle -- or, for
the 8 M-cell case, with the general pipeline -- and, after a build that was discarded, that the caller's sets are the oracle's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import icebin_amd
from icebin_amd import _capi
from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import assembly_limit_cases as alc
    from test_gpu_parity import assert_same_weighted
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

KNOBS = ("assemble_fast", "assemble_stream", "assemble_stream_wpr", "assemble_stream_oldseg", "assemble_stream_rowsl",
         "assemble_stream_rows4", "assemble_range_shape", "assemble_static_count")


def path_of(w):
    v = C.c_int()
    _capi.check(_capi.lib().ibh_weighted_built_fast(w._h, C.byref(v)))
    return v.value


def reset_knobs():
    for k in KNOBS:
        icebin_amd.set_tuning(k, -2 ** 31)


def host_copy(w):
    """dims, CSR, wM and Mw of a matrix on the host (the reference of the case built by the general pipeline)."""
    rowptr, colind, val = w.csr_dense()
    return dict(shape=(w.nrow_d, w.ncol_d, w.nnz), dims=(w.dim(0).copy(), w.dim(1).copy()), rowptr=rowptr.copy(), colind=colind.copy(),
                val=val.view(np.uint64).copy(), wM=w.wM.view(np.uint64).copy(), Mw=w.Mw.view(np.uint64).copy())


def assert_same_host(w, ref, what):
    got = host_copy(w)
    assert got["shape"] == ref["shape"], what
    for k in ("rowptr", "colind", "val", "wM", "Mw"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (what, k))
    for i in (0, 1):
        np.testing.assert_array_equal(got["dims"][i], ref["dims"][i], err_msg="%s dims[%d]" % (what, i))


def identity_dims(name, g, mine):
    """the identity set on the I / X side of `name` (the coupler's dimI / dimX), for the library (mine) or the oracle"""
    rows, cols = name[0], name[2]
    n = {"I": g["nI"], "X": len(g["ex_area"])}
    make = (lambda k: icebin_amd.SparseSet.identity(n[k])) if mine else (lambda k: orc.SparseSet(n[k], init=np.arange(n[k])))
    return (make(rows) if rows in n else None, make(cols) if cols in n else None)


@pytest.mark.parametrize("case", alc.CASES, ids=[c["name"] for c in alc.CASES])
def test_sorted_grid_limits(case):
    g, em = alc.build_grid(case["grid"])
    mm = icebin_amd.from_synthetic(g)
    general = case.get("reference", "oracle") == "general"
    rg = None if general else orc.Regridder(g)
    paths = case["path"] if isinstance(case["path"], list) else [case["path"]] * len(case["knobs"])
    refs = {}
    try:
        if general:                                        # the general pipeline's bits first (itself pinned to the oracle elsewhere)
            icebin_amd.set_tuning("assemble_fast", 0)
            rm = mm.regrid_matrices("greenland", em)
            for name, branches, dims in case["builds"]:
                for sc, cA in branches:
                    w = rm.matrix_d(name, identity_dims(name, g, True) if dims == "identity" else (None, None), scale=sc, correctA=cA)
                    assert path_of(w) == 0
                    refs[(name, sc, cA, dims)] = host_copy(w)
                    del w
            reset_knobs()
        for knobs, path in zip(case["knobs"], paths):
            reset_knobs()
            for k, v in knobs.items():
                icebin_amd.set_tuning(k, v)
            rm = mm.regrid_matrices("greenland", em)
            for name, branches, dims in case["builds"]:
                for sc, cA in branches:
                    what = "%s %s scale=%d correctA=%d dims=%s knobs=%s" % (case["name"], name, sc, cA, dims, knobs)
                    w = rm.matrix_d(name, identity_dims(name, g, True) if dims == "identity" else (None, None), scale=sc, correctA=cA)
                    assert path_of(w) == path, (what, path_of(w))
                    if general:
                        assert_same_host(w, refs[(name, sc, cA, dims)], what)
                    else:
                        od = identity_dims(name, g, False) if dims == "identity" else (None, None)
                        assert_same_weighted(w, rg.matrix_d(name, em, dims=od, scale=sc, correctA=cA), what)
                    del w
            if case.get("discard"):
                # the discarded build on caller-owned sets: a fresh dimE that the build numbers, then a pre-populated one (its keys
                # reversed, and seven keys this mask never touches): nothing of the discarded attempt may stay behind in either
                nE = g["nA"] * len(g["hcdefs"])
                dimE, oE = icebin_amd.SparseSet(nE), orc.SparseSet(nE)
                w = rm.matrix_d("EvI", (dimE, None), scale=False, correctA=False)
                assert path_of(w) == path, (case["name"], "EvI fresh dimE", path_of(w))
                assert_same_weighted(w, rg.matrix_d("EvI", em, dims=(oE, None), scale=False, correctA=False), case["name"] + " EvI fresh dimE")
                np.testing.assert_array_equal(dimE.to_sparse(), oE.to_sparse())
                keys = dimE.to_sparse()
                pre = np.concatenate([keys[::-1], np.setdiff1d(np.arange(nE), keys)[:7]])
                dE2, oE2 = icebin_amd.SparseSet(nE, pre), orc.SparseSet(nE, init=pre)
                w = rm.matrix_d("IvE", (None, dE2), scale=True, correctA=True)
                assert path_of(w) == path, (case["name"], "IvE pre-populated dimE", path_of(w))
                assert_same_weighted(w, rg.matrix_d("IvE", em, dims=(None, oE2), scale=True, correctA=True), case["name"] + " IvE pre-populated dimE")
                np.testing.assert_array_equal(dE2.to_sparse(), oE2.to_sparse())
                assert dE2.dense_extent() == len(pre)
    finally:
        reset_knobs()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_streamed_build_of_32_bit_positions(world):
    """ibh_regrid_matrices_matrix_d_sharded of a grid with 32-bit positions (a range of 65 536 cells), 2 and 3 ranks sharing the
    GPU over the host-staged transport of test_distributed_gloo.py: every rank's slice is rounded to 64-cell waves and the emit
    pass walks 4 cells per thread there -- every matrix bitwise the single-rank build."""
    import multiprocessing as mp
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    try:
        from test_distributed_gloo import _free_port, _worker_asm_sharded
    finally:
        sys.path.pop(0)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_asm_sharded, args=(r, world, port, q, ("limits:" + alc.SHARDED_CASE,))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    got = sorted(q.get(timeout=5) for _ in range(world))
    assert all(ok for _, ok, _, _ in got), got
