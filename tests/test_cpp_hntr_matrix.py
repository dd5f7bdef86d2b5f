"""Compiles the C++ test of Hntr's matrix forms (tests/cpp/test_hntr_matrix.cpp) against libicebin_hip.so (g++, no HIP headers
needed), runs it, and compares what its accumulators and matrix_d produced with the Python surface, bitwise."""
import numpy as np
import pytest

import cpp_programs as cpp


def read(path):
    """the program's own format, three arrays under one count (its four-argument dump)"""
    with open(path, "rb") as f:
        n = int(np.frombuffer(f.read(8), np.int64)[0])
        a = np.frombuffer(f.read(4 * n), np.int32)
        b = np.frombuffer(f.read(4 * n), np.int32)
        v = np.frombuffer(f.read(8 * n), np.float64)
    return a, b, v


def test_cpp_hntr_matrix_compiles_and_fails_loudly_without_gpu(tmp_path):
    cpp.fails_loudly_without_gpu("test_hntr_matrix", tmp_path, timeout=300)


@pytest.mark.gpu
def test_cpp_hntr_matrix_on_gpu(tmp_path):
    from icebin_amd import Hntr, HntrSpec, SparseSet
    r = cpp.run(cpp.exe("test_hntr_matrix", allow_compile=False), tmp_path, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    B, A = HntrSpec(72, 46, 0.5, 240.), HntrSpec(144, 90, 0.25, 120.)
    h = Hntr(17.17, B, A)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64)   # noqa: E731

    for got, ref in ((read(tmp_path / "overlap.bin"), h.overlap(6371000.)),):
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(bits(got[2]), bits(ref[2]))
    clip = (np.arange(B.size) * 7) % 3 != 0
    got, ref = read(tmp_path / "scaled_clip.bin"), h.scaled_regrid_matrix(clip)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(bits(got[2]), bits(ref[2]))

    dimB, dimA = SparseSet(B.size, np.nonzero(clip)[0]), SparseSet()
    w = h.matrix_d("overlap", 6371000., includeB=clip, dims=(dimB, dimA), transforms=(2, 0), transpose=True)
    row, col, val = w.coo_dense()
    got = read(tmp_path / "matrix_T.bin")
    assert np.array_equal(got[0], row) and np.array_equal(got[1], col) and np.array_equal(bits(got[2]), bits(val))
    assert np.array_equal(read(tmp_path / "dimA.bin")[0], dimA.to_sparse())
