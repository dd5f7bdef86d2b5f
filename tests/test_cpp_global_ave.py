"""Compiles the C++ test of global_AvE (tests/cpp/test_global_ave.cpp: compute_EOpvAOp_merged, _compute_AAmvEAm[_EIGEN] and
GCMRegridder_ModelE::global_AvE of icebin_amd/host/icebin_hip.hpp) against libicebin_hip.so (g++, no HIP headers needed), runs
it, and compares its matrices with the Python surface, bitwise."""
import numpy as np
import pytest

import cpp_programs as cpp
from cpp_programs import bits, read


def test_cpp_global_ave_compiles_and_fails_loudly_without_gpu(tmp_path):
    cpp.fails_loudly_without_gpu("test_global_ave", tmp_path, timeout=300)


def same(tmp_path, name, w):
    row, col, val = w.coo_dense()
    assert len(val) > 20, name
    p = lambda ext: tmp_path / (name + ext)       # noqa: E731
    assert np.array_equal(read(p(".row"), np.int32), row), name
    assert np.array_equal(read(p(".col"), np.int32), col), name
    assert np.array_equal(bits(read(p(".val"), np.float64)), bits(val)), name
    assert np.array_equal(bits(read(p(".wM"), np.float64)), bits(w.wM)), name
    assert np.array_equal(bits(read(p(".Mw"), np.float64)), bits(w.Mw)), name
    assert np.array_equal(read(p(".dim0"), np.int64), w.dim(0)), name
    assert np.array_equal(read(p(".dim1"), np.int64), w.dim(1)), name
    assert read(p(".extent"), np.int64).tolist() == [w.sparse_extent(0), w.sparse_extent(1)], name


def same_classes(tmp_path, name, r):
    assert np.array_equal(bits(read(tmp_path / (name + ".hcdefs"), np.float64)), bits(r.hcdefs)), name
    assert np.array_equal(read(tmp_path / (name + ".underice"), np.int16), r.underice_hc), name
    assert read(tmp_path / (name + ".meta"), np.int64).tolist() == [r.offsetE, r.indexingHC[0], r.indexingHC[1], r.nO, r.nhc], name


@pytest.mark.gpu
def test_cpp_global_ave_on_gpu(tmp_path):
    from icebin_amd import GCMRegridder, HntrSpec, SparseSet, compute_AAmvEAm, compute_EOpvAOp_merged, global_ec
    r = cpp.run(cpp.exe("test_global_ave", allow_compile=False), tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    R = 6371000.
    O, Is = HntrSpec(8, 6, 0., 1800.), (HntrSpec(48, 36, 0.5, 300.), HntrSpec(24, 18, 0.25, 600.))
    i0, i1 = np.arange(Is[0].size), np.arange(Is[1].size)
    ems = [np.where((i0 * 7) % 5 == 0, np.nan, (i0 % 3000).astype(np.float64)),
           np.where((i1 * 3) % 4 == 0, np.nan, ((i1 * 5) % 3000).astype(np.float64))]
    o = np.arange(O.size)
    fm = np.where(o % 5 == 0, 1., 0.)
    fp = np.where(o % 5 == 0, 1., np.where(o % 5 == 1, 0.25, 0.))
    c = np.arange(1, O.size, 4)
    iE, iO, val = c + O.size * (c % 3 == 0), c, 1e9 * (c + 1.)
    iE, iO, val = np.append(iE, iE[2]), np.append(iO, iO[2]), np.append(val, 2.5e9)
    base = ([1500., 4000.], (iE, iO, val), (2 * O.size, O.size))
    hc = [0., 1500., 3000.]
    gcm = GCMRegridder(dict(nA=O.size, to_sparse=o, native_area=np.ones(O.size)), hc, True)
    for k in (0, 1):
        idx, area = global_ec.gcm_from_hntr(O, Is[k], ems[k], hc, True, R).exgrid()
        gcm.add_sheet("sheet%d" % k, dict(nI=Is[k].size), dict(indices=idx.copy(), overlaps=area.copy()))
    rmOs = [gcm.regrid_matrices("sheet%d" % k, ems[k]) for k in (0, 1)]
    eo = compute_EOpvAOp_merged(rmOs, base)
    same(tmp_path, "EOpvAOp", eo.EOpvAOp)
    same_classes(tmp_path, "EOpvAOp", eo)
    sq = compute_EOpvAOp_merged(rmOs, base, squash_ecs=True)
    same(tmp_path, "EOpvAOp_sq", sq.EOpvAOp)
    same_classes(tmp_path, "EOpvAOp_sq", sq)
    same(tmp_path, "AvE_s", compute_AAmvEAm(eo, O, R, fp, fm, scale=True))
    same(tmp_path, "AvE_sq", compute_AAmvEAm(sq, O, R, fp, fm, scale=False, dims=(SparseSet(), SparseSet())))
    w, offsetE = gcm.to_modele((fp, fm), hspecO=O, eq_rad=R, global_ec=base).global_AvE(None, ems, fp, fm, scale=False)
    assert offsetE == 3 * O.size
    same(tmp_path, "AvE_u", w)
