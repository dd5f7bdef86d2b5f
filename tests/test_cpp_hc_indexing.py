"""Compiles the C++ test of HcIndexing (tests/cpp/test_hc_indexing.cpp: the indexingHC tuple of common.h, host code only) with the
host compiler and runs it: split / index / with_nhc for both orders at the smallest grids."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_hc_indexing(tmp_path):
    exe = str(tmp_path / "test_hc_indexing")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_hc_indexing.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
