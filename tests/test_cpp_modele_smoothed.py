"""Compiles the C++ test of the smoothed ModelE matrices (tests/cpp/test_modele_smoothed.cpp: RegridMatrices_ModelE::matrix_d with
RegridParams(true, true, sigma), icebin_amd/host/icebin_hip.hpp) against libicebin_hip.so, runs it on the synthetic grid g50 and
compares its EvI, IvE and IvA with the ctypes surface, bitwise; the Cython module's to_modele(...).regrid_matrices(..., sigma=)
.matrix("IvE") gives the same."""
import os
import sys

import numpy as np
import pytest

import cpp_programs as cpp
from cpp_programs import ROOT, bits, read, write

SIGMA = (60e3, 45e3, 250.)
O = (144, 90, 0., 120.)
R = 6371000.


def inputs(indir):
    """g50 with its dome mask; ModelE ocean on every 4th ice-bearing O cell, a fractional ice-model ocean on every 4th + 1."""
    from icebin_amd import synthetic
    g = synthetic.make_grids("g50")
    em = synthetic.dome_elevmask(g)
    fp, fm = np.zeros(g["nA"]), np.zeros(g["nA"])
    ice = np.unique(np.asarray(g["ex_indices"]).reshape(-1, 2)[:, 0])
    fm[ice[::4]] = fp[ice[::4]] = 1.
    fp[ice[1::4]] = 0.5
    os.makedirs(indir, exist_ok=True)
    p = lambda n: os.path.join(str(indir), n + ".bin")     # noqa: E731
    write(p("sizes"), [g["nA"], g["nI"], O[0], O[1]], np.int64)
    write(p("hspec"), [O[2], O[3]], np.float64)
    write(p("sigma"), SIGMA, np.float64)
    write(p("A_to_sparse"), g["A_to_sparse"], np.int64)
    for k in ("A_native_area", "A_proj_area", "ex_area", "hcdefs", "I_centroid_xy"):
        write(p(k), g[k], np.float64)
    write(p("ex_indices"), g["ex_indices"], np.int32)
    write(p("elevmaskI"), em, np.float64)
    write(p("foceanOp"), fp, np.float64)
    write(p("foceanOm"), fm, np.float64)
    return g, em, fp, fm


def test_cpp_modele_smoothed_compiles_and_fails_loudly_without_gpu(tmp_path):
    inputs(tmp_path / "in")
    os.makedirs(tmp_path / "out")
    cpp.fails_loudly_without_gpu("test_modele_smoothed", tmp_path / "in", tmp_path / "out", timeout=300)


def same_as_files(w, outdir, name):
    row, col, val = w.coo_dense()
    assert len(val) > 100, name
    p = lambda ext: os.path.join(str(outdir), name + ext)       # noqa: E731
    assert np.array_equal(read(p(".row"), np.int32), row), name
    assert np.array_equal(read(p(".col"), np.int32), col), name
    assert np.array_equal(bits(read(p(".val"), np.float64)), bits(val)), name
    assert np.array_equal(bits(read(p(".wM"), np.float64)), bits(w.wM)), name
    assert np.array_equal(bits(read(p(".Mw"), np.float64)), bits(w.Mw)), name
    assert np.array_equal(read(p(".dim0"), np.int64), w.dim(0)), name
    assert np.array_equal(read(p(".dim1"), np.int64), w.dim(1)), name


@pytest.mark.gpu
def test_cpp_modele_smoothed_on_gpu(tmp_path):
    from icebin_amd import HntrSpec, SparseSet, from_synthetic
    g, em, fp, fm = inputs(tmp_path / "in")
    os.makedirs(tmp_path / "out")
    r = cpp.run(cpp.exe("test_modele_smoothed", allow_compile=False), tmp_path / "in", tmp_path / "out", timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    rm = from_synthetic(g).to_modele((fp, fm), hspecO=HntrSpec(*O), eq_rad=R).regrid_matrices("greenland", em)
    dimE = SparseSet()
    same_as_files(rm.matrix_d("EvI", (dimE, None), scale=True), tmp_path / "out", "EvI")
    IvE = rm.matrix_d("IvE", (None, dimE), scale=True, sigma=SIGMA)
    assert IvE.smoothed_by() != 0 and IvE.composed_by() == 2
    same_as_files(IvE, tmp_path / "out", "IvE")
    IvA = rm.matrix_d("IvA", scale=True, sigma=SIGMA)
    same_as_files(IvA, tmp_path / "out", "IvA")
    same_as_files(IvA, tmp_path / "out", "IvA_matrix")


def cython_icebin():
    from icebin_amd.cython.build_ext import build
    build()
    sys.path.insert(0, os.path.join(ROOT, "icebin_amd", "cython"))
    import icebin
    return icebin


@pytest.mark.gpu
def test_cython_smoothed_to_modele_equals_the_ctypes_surface(tmp_path):
    from icebin_amd import HntrSpec, from_synthetic
    icebin = cython_icebin()
    g, em, fp, fm = inputs(tmp_path / "in")
    c = icebin.GCMRegridder(dict(nA=g["nA"], to_sparse=g["A_to_sparse"], native_area=g["A_native_area"]), g["hcdefs"], True)
    c.add_sheet("greenland", dict(nI=g["nI"], centroid_xy=g["I_centroid_xy"]), dict(indices=g["ex_indices"], overlaps=g["ex_area"]),
                "Z_INTERP", g["A_proj_area"])
    rc = c.to_modele((fp, fm), hspecO=icebin.HntrSpec(*O), eq_rad=R).regrid_matrices("greenland", em, sigma=SIGMA)
    rp = from_synthetic(g).to_modele((fp, fm), hspecO=HntrSpec(*O), eq_rad=R).regrid_matrices("greenland", em, sigma=SIGMA)
    plain = from_synthetic(g).to_modele((fp, fm), hspecO=HntrSpec(*O), eq_rad=R).regrid_matrices("greenland", em)
    for name in ("IvE", "IvA", "EvI"):
        a, b = rc.matrix(name), rp.matrix(name)
        assert np.array_equal(bits(a.wM), bits(b.wM)) and np.array_equal(bits(a.Mw), bits(b.Mw)), name
        ca, cb = a.to_coo().tocsr(), b.to_coo().tocsr()
        assert np.array_equal(ca.indptr, cb.indptr) and np.array_equal(ca.indices, cb.indices), name
        assert np.array_equal(bits(ca.data), bits(cb.data)) and len(ca.data) > 100, name
        assert (b.nnz > plain.matrix(name).nnz) == (name[0] == "I"), name
