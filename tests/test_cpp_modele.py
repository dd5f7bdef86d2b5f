"""Compiles the C++ test of the ModelE regridder (tests/cpp/test_modele.cpp: GCMRegridder_ModelE / GCMRegridder_WrapE of
icebin_amd/host/icebin_hip.hpp) against libicebin_hip.so (g++, no HIP headers needed), runs it, and compares its EvI, AvI,
IvE and XvE with the Python surface (GCMRegridder.to_modele), bitwise."""
import os

import numpy as np
import pytest

import cpp_programs as cpp
from cpp_programs import ROOT, bits, read


def test_cpp_modele_compiles_and_fails_loudly_without_gpu(tmp_path):
    cpp.fails_loudly_without_gpu("test_modele", tmp_path, timeout=300)


@pytest.mark.gpu
def test_cpp_modele_on_gpu(tmp_path):
    from icebin_amd import HntrSpec, SparseSet, global_ec
    r = cpp.run(cpp.exe("test_modele", allow_compile=False), tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    O, I = HntrSpec(8, 6, 0., 1800.), HntrSpec(48, 36, 0.5, 300.)
    i = np.arange(I.size)
    em = np.where((i * 7) % 5 == 0, np.nan, (i % 3000).astype(np.float64))
    o = np.arange(O.size)
    fm = np.where(o % 5 == 0, 1., 0.)
    fp = np.where(o % 5 == 0, 1., np.where(o % 5 == 1, 0.25, 0.))
    gcmO = global_ec.gcm_from_hntr(O, I, em, [0., 1500., 3000.], True, 6371000.)
    gcmA = gcmO.to_modele((fp, fm))
    assert np.array_equal(read(tmp_path / "agridA.dim", np.int64), gcmA.agridA("globalI"))
    rm = gcmA.regrid_matrices("globalI", em)
    dimE = SparseSet()
    mats = (("EvI", rm.matrix_d("EvI", (dimE, None), scale=True)), ("AvI", rm.matrix("AvI")),
            ("IvE", rm.matrix_d("IvE", (None, dimE), scale=False)), ("XvE", rm.matrix_d("XvE", (None, dimE), scale=False)))
    for name, w in mats:
        row, col, val = w.coo_dense()
        assert len(val) > 100, name
        p = lambda ext: tmp_path / (name + ext)       # noqa: E731
        assert np.array_equal(read(p(".row"), np.int32), row), name
        assert np.array_equal(read(p(".col"), np.int32), col), name
        assert np.array_equal(bits(read(p(".val"), np.float64)), bits(val)), name
        assert np.array_equal(bits(read(p(".wM"), np.float64)), bits(w.wM)), name
        assert np.array_equal(bits(read(p(".Mw"), np.float64)), bits(w.Mw)), name
        assert np.array_equal(read(p(".dim0"), np.int64), w.dim(0)), name
        assert np.array_equal(read(p(".dim1"), np.int64), w.dim(1)), name


def cython_icebin():
    import sys
    from icebin_amd.cython.build_ext import build
    build()
    sys.path.insert(0, os.path.join(ROOT, "icebin_amd", "cython"))
    import icebin
    return icebin


def test_cython_to_modele_has_the_reference_surface():
    # pylib/_icebin.pyx:128-147: GCMRegridder.to_modele(focean=None) returns an object with nA, nE, nhc, regrid_matrices
    icebin = cython_icebin()
    g = icebin.GCMRegridder(dict(nA=48, to_sparse=[0, 1], native_area=[1., 1.]), [0., 100.], True)
    with pytest.raises(RuntimeError, match="requires specO have a Hntr source"):
        g.to_modele()
    m = g.to_modele(hspecO=icebin.HntrSpec(8, 6, 0., 1800.), eq_rad=6371000.)
    assert (m.nA, m.nE, m.nhc) == (12, 24, 2) and hasattr(m, "regrid_matrices")
    with pytest.raises(NotImplementedError):
        m.wA("s", "native")
    with pytest.raises(RuntimeError, match="even number"):
        icebin.GCMRegridder(dict(nA=35, to_sparse=[0], native_area=[1.]), [0.], True).to_modele(
            hspecO=icebin.HntrSpec(7, 5, 0., 1800.), eq_rad=6371000.)


@pytest.mark.gpu
def test_cython_to_modele_equals_the_ctypes_surface():
    from icebin_amd import HntrSpec, from_synthetic, synthetic
    icebin = cython_icebin()
    g = synthetic.make_grids("g50")
    em = synthetic.dome_elevmask(g)
    fp, fm = np.zeros(g["nA"]), np.zeros(g["nA"])
    ice = np.unique(g["ex_indices"][:, 0])
    fm[ice[::4]] = fp[ice[::4]] = 1.
    fp[ice[1::4]] = 0.5
    O = (144, 90, 0., 120.)
    c = icebin.GCMRegridder(dict(nA=g["nA"], to_sparse=g["A_to_sparse"], native_area=g["A_native_area"]), g["hcdefs"], True)
    c.add_sheet("greenland", dict(nI=g["nI"]), dict(indices=g["ex_indices"], overlaps=g["ex_area"]), "Z_INTERP", g["A_proj_area"])
    rc = c.to_modele((fp, fm), hspecO=icebin.HntrSpec(*O), eq_rad=6371000.).regrid_matrices("greenland", em)
    rp = from_synthetic(g).to_modele((fp, fm), hspecO=HntrSpec(*O), eq_rad=6371000.).regrid_matrices("greenland", em)
    for name in ("AvI", "EvI", "IvA", "IvE"):
        a, b = rc.matrix(name), rp.matrix(name)
        assert np.array_equal(bits(a.wM), bits(b.wM)) and np.array_equal(bits(a.Mw), bits(b.Mw)), name
        ca, cb = a.to_coo().tocsr(), b.to_coo().tocsr()
        assert np.array_equal(ca.indptr, cb.indptr) and np.array_equal(ca.indices, cb.indices), name
        assert np.array_equal(bits(ca.data), bits(cb.data)) and len(ca.data) > 100, name
