"""Compiles the C++ test of global_ec (tests/cpp/test_global_ec.cpp) against libicebin_hip.so (g++, no HIP headers needed),
runs it, and compares its regridder, AvI, IvE and I2vE with the Python surface (icebin_amd.global_ec), bitwise."""
import numpy as np
import pytest

import cpp_programs as cpp
from cpp_programs import bits, read


def test_cpp_global_ec_compiles_and_fails_loudly_without_gpu(tmp_path):
    cpp.fails_loudly_without_gpu("test_global_ec", tmp_path, timeout=300)


@pytest.mark.gpu
def test_cpp_global_ec_on_gpu(tmp_path):
    from icebin_amd import HntrSpec, SparseSet, global_ec
    r = cpp.run(cpp.exe("test_global_ec", allow_compile=False), tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    A, I, I2 = HntrSpec(72, 46, 0., 240.), HntrSpec(360, 180, 0., 60.), HntrSpec(144, 90, 0., 120.)
    i = np.arange(I.size)
    em = np.where((i * 7) % 3 == 0, np.nan, (i % 3000).astype(np.float64))
    hc = global_ec.hcdefs(0., 3000., 500.)
    gcm = global_ec.gcm_from_hntr(A, I, em, hc, True, 6371000.)
    assert np.array_equal(read(tmp_path / "agridA.dim", np.int64), gcm._A_to_sparse)
    assert np.array_equal(bits(read(tmp_path / "agridA.native_area", np.float64)), bits(gcm._A_native))
    assert np.array_equal(bits(read(tmp_path / "wA", np.float64)), bits(gcm.wA("globalI", "native")))

    rm = gcm.regrid_matrices("globalI", em, scale=False, correctA=True)
    dimA, dimI, dimE, dimI2 = SparseSet(), SparseSet(), SparseSet(), SparseSet(I2.size)
    AvI = rm.matrix_d("AvI", (dimA, dimI), scale=False, correctA=True)
    IvE = rm.matrix_d("IvE", (dimI, dimE), scale=False, correctA=True)
    I2vE = global_ec.make_I2vX(IvE, I, I2, em, dimI2, 6371000.)
    for name, w in (("AvI", AvI), ("IvE", IvE), ("I2vE", I2vE)):
        row, col, val = w.coo_dense()
        p = lambda ext: tmp_path / (name + ext)       # noqa: E731
        assert np.array_equal(read(p(".row"), np.int32), row), name
        assert np.array_equal(read(p(".col"), np.int32), col), name
        assert np.array_equal(bits(read(p(".val"), np.float64)), bits(val)), name
        assert np.array_equal(bits(read(p(".wM"), np.float64)), bits(w.wM)), name
        assert np.array_equal(bits(read(p(".Mw"), np.float64)), bits(w.Mw)), name
        assert np.array_equal(read(p(".dim0"), np.int64), w.dim(0)), name
        assert np.array_equal(read(p(".dim1"), np.int64), w.dim(1)), name
