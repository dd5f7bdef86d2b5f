"""Compiles the C++ test of HcIndexing (tests/cpp/test_hc_indexing.cpp: the indexingHC tuple of common.h, host code only) with the
host compiler and runs it: split / index / with_nhc for both orders at the smallest grids."""
import cpp_programs as cpp


def test_cpp_hc_indexing():
    r = cpp.run(cpp.exe("test_hc_indexing"), timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
