"""Compiles the C++ test of the path from grid specs (tests/cpp/test_lonlat.cpp) against libicebin_hip.so (g++, no HIP headers
needed) and runs it; on the GPU its sizes and exchange-cell count must be the Python path's."""
import os
import re
import sys

import numpy as np
import pytest

import cpp_programs as cpp


def test_cpp_lonlat_compiles_and_fails_loudly_without_gpu():
    cpp.fails_loudly_without_gpu("test_lonlat", timeout=300)


@pytest.mark.gpu
def test_cpp_lonlat_on_gpu():
    r = cpp.run(cpp.exe("test_lonlat", allow_compile=False), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout)}
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import lonlat_cases as llc
    from icebin_amd import gridgen as gg
    spec = llc.small_spec(6, 2, south_pole=False, north_pole=True)
    realised = llc.all_cells(spec)
    xe, ye = -0.24e6 + 2e4 * np.arange(25), -0.7e6 + 2e4 * np.arange(31)
    mm = gg.regridder_from_specs(spec, realised, xe, ye, llc.SPROJ["searise_north"], [0., 500., 1500., 3000.])
    idx, area, _ = mm._sheets["ice"].arrays
    assert got == dict(nA=mm.nA, nE=mm.nE, nI=24 * 30, nX=len(area), ncell=len(realised)), (got, r.stdout)
