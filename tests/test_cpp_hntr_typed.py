"""Compiles the C++ test of the typed Hntr regrid (tests/cpp/test_hntr_typed.cpp) against libicebin_hip.so (g++, no HIP headers needed) and runs it."""
import pytest

import cpp_programs as cpp


def test_cpp_hntr_typed_compiles_and_fails_loudly_without_gpu():
    cpp.fails_loudly_without_gpu("test_hntr_typed", timeout=300)


@pytest.mark.gpu
def test_cpp_hntr_typed_on_gpu():
    r = cpp.run(cpp.exe("test_hntr_typed", allow_compile=False), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
