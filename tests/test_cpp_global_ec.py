"""Compiles the C++ test of global_ec (tests/cpp/test_global_ec.cpp) against libicebin_hip.so (g++, no HIP headers needed),
runs it, and compares its regridder, AvI, IvE and I2vE with the Python surface (icebin_amd.global_ec), bitwise."""
import os
import subprocess

import numpy as np
import pytest

from icebin_amd import _capi
from icebin_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_global_ec")


def compile_exe():
    lib = build_library()
    src = os.path.join(ROOT, "tests", "cpp", "test_global_ec.cpp")
    hdrs = [os.path.join(ROOT, "icebin_amd", "host", h) for h in ("icebin_hip.hpp", "ncio.hpp")]
    libdir = os.path.dirname(lib)
    if (not os.path.exists(EXE)) or os.path.getmtime(EXE) < max(os.path.getmtime(f) for f in [src, lib] + hdrs):
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", EXE, src, "-L" + libdir, "-licebin_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def read(path, dtype):
    with open(path, "rb") as f:
        n = int(np.frombuffer(f.read(8), np.int64)[0])
        return np.frombuffer(f.read(np.dtype(dtype).itemsize * n), dtype)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def test_cpp_global_ec_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = compile_exe()
    if _capi.device_count() > 0:
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3, r.stdout + r.stderr
    assert "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_cpp_global_ec_on_gpu(tmp_path):
    from icebin_amd import HntrSpec, SparseSet, global_ec
    r = subprocess.run([compile_exe(), str(tmp_path)], capture_output=True, text=True, timeout=600)
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
