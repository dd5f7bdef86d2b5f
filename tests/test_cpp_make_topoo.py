"""Compiles the C++ test of make_topoO (tests/cpp/test_make_topoo.cpp) against libicebin_hip.so (g++, no HIP headers needed),
runs it, and compares its planes with the Python surface (icebin_amd.topoo), bitwise."""
import numpy as np
import pytest

import cpp_programs as cpp
from icebin_amd import _capi


def test_cpp_make_topoo_compiles_and_fails_loudly_without_gpu(tmp_path):
    """the refusals that need no device run either way; without a GPU the first call that needs one says so.  (Not
    cpp.fails_loudly_without_gpu, which skips where there is a device: this one runs there too and must pass.)"""
    r = cpp.run(cpp.exe("test_make_topoo"), tmp_path, timeout=300)
    if _capi.device_count() > 0:
        assert r.returncode == 0, r.stdout + r.stderr
    else:
        assert r.returncode == 3, r.stdout + r.stderr
        assert "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_cpp_make_topoo_on_gpu(tmp_path):
    from icebin_amd import HntrSpec, topoo
    r = cpp.run(cpp.exe("test_make_topoo", allow_compile=False), tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    O, I, S = HntrSpec(12, 12, 0., 900.), HntrSpec(48, 48, 0., 225.), HntrSpec(18, 9, 0., 1200.)
    x = np.arange(I.size)
    fo = (((x * 7 + x // 13) % 5) < 2).astype(np.int16)
    fg = (((x * 5 + x // 7) % 3) == 0).astype(np.int16)
    zt = (((x * 37) % 7) * 100 - 300).astype(np.int16)
    zs = (zt - np.where(x % 48 < 24, (x * 11) % 100, 0)).astype(np.int16)
    k = np.arange(S.size)
    fl = np.where(k % 4 == 0, 0., (k % 9) / 16.0)
    res = topoo.make_topoO(I, O, fg, zt, zs, fo, S, fl, set_to_land=[(3, 4)], set_to_ocean=[(7, 6)], resets=[(-30., [(5, 5)]), (53., [(6, 7)])])
    for n in topoo.PLANES:
        assert np.array_equal(cpp.read(tmp_path / n, np.float64).view(np.uint64), getattr(res, n).cpu().numpy().reshape(-1).view(np.uint64)), n
    assert cpp.read(tmp_path / "counts", np.float64).astype(np.int64).tolist() == list(res.counts.values())
