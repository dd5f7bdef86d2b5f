"""Compiles the C++ host-API test against libicebin_hip.so (g++, no HIP headers needed) and runs it."""
import numpy as np
import pytest

import cpp_programs as cpp


def test_cpp_host_api_compiles_and_fails_loudly_without_gpu():
    cpp.fails_loudly_without_gpu("test_host_api")


@pytest.mark.gpu
def test_cpp_host_api_on_gpu(tmp_path):
    fn = str(tmp_path / "host_api.nc")
    r = cpp.run(cpp.exe("test_host_api", allow_compile=False), fn)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    # the file the C++ host wrote (GCMRegridder_Standard::ncio + two Weighted::ncio appends) through the Python side:
    # the same regridder builds the same matrix as the one stored beside it
    import icebin_amd
    mm = icebin_amd.GCMRegridder(fn)
    assert (mm.nA, mm.nhc) == (32, 40)
    stored = icebin_amd.nc_read_weighted(fn, "AvI")
    nx, ny = 12, 10
    em = np.array([[np.nan if (ix == 0 or iy == ny - 1) else 100.0 * ix + 37.0 * iy for iy in range(ny)] for ix in range(nx)]).reshape(-1)
    w = mm.regrid_matrices("greenland", em, scale=True, correctA=False).matrix("AvI")
    for a, b in zip(w.coo_dense(), stored.coo_dense()):
        assert np.array_equal(a, b)
    assert np.array_equal(w.wM.view(np.uint64), stored.wM.view(np.uint64)) and np.array_equal(w.dim(1), stored.dim(1))
    assert stored.shape == w.shape
