"""Compiles the C++ test of etopo1_ice (tests/cpp/test_etopo1_ice.cpp) against libicebin_hip.so (g++, no HIP headers needed),
runs it, and compares its planes with the Python surface (icebin_amd.etopo1), bitwise."""
import numpy as np
import pytest

import cpp_programs as cpp
from cpp_programs import read


def test_cpp_etopo1_ice_compiles_and_fails_loudly_without_gpu(tmp_path):
    cpp.fails_loudly_without_gpu("test_etopo1_ice", tmp_path, timeout=300)


@pytest.mark.gpu
def test_cpp_etopo1_ice_on_gpu(tmp_path):
    from icebin_amd import HntrSpec, etopo1
    r = cpp.run(cpp.exe("test_etopo1_ice", allow_compile=False), tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    Cg, I, H = HntrSpec(8, 4, 0., 2700.), HntrSpec(32, 16, 0., 675.), HntrSpec(16, 8, 0., 1350.)
    x = np.arange(I.size)
    fo = ((x * 7 + x // 13) % 4).astype(np.int16).reshape(I.jm, I.im)
    zt = (((x * 37) % 7) * 100 - 300).astype(np.int16).reshape(I.jm, I.im)
    zs = (zt.reshape(-1) - (x * 11) % 100).astype(np.int16).reshape(I.jm, I.im)
    k = np.arange(Cg.size)
    fC = np.where(k % 3 == 0, 0., (k % 7) / 6.0).reshape(Cg.jm, Cg.im)
    for incl in (0, 1):
        res = etopo1.etopo1_ice(I, Cg, fo, zt, zs, fC, include_greenland=bool(incl), hspecH=H)
        for n in etopo1.PLANES:
            assert np.array_equal(read(tmp_path / ("g%d.%s" % (incl, n)), np.int16), getattr(res, n).cpu().numpy().reshape(-1)), (incl, n)
        for n in etopo1.PLANES_H:
            got = read(tmp_path / ("g%d.%s" % (incl, n)), np.float64)
            assert np.array_equal(got.view(np.uint64), getattr(res, n).cpu().numpy().reshape(-1).view(np.uint64)), (incl, n)
