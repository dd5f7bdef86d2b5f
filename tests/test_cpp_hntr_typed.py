"""Compiles the C++ test of the typed Hntr regrid (tests/cpp/test_hntr_typed.cpp) against libicebin_hip.so (g++, no HIP headers needed) and runs it."""
import os
import subprocess

import pytest

from icebin_amd import _capi
from icebin_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_hntr_typed")


def compile_exe(allow_compile=True):
    """__graft_entry__.build() builds the executable, which travels to the GPU box: the GPU test only compiles when it is
    missing altogether."""
    lib = build_library()
    src = os.path.join(ROOT, "tests", "cpp", "test_hntr_typed.cpp")
    hdrs = [os.path.join(ROOT, "icebin_amd", "host", h) for h in ("icebin_hip.hpp", "ncio.hpp")]
    libdir = os.path.dirname(lib)
    stale = (not os.path.exists(EXE)) or os.path.getmtime(EXE) < max(os.path.getmtime(f) for f in [src, lib] + hdrs)
    if stale and (allow_compile or not os.path.exists(EXE)):
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", EXE, src, "-L" + libdir, "-licebin_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cpp_hntr_typed_compiles_and_fails_loudly_without_gpu():
    exe = compile_exe()
    if _capi.device_count() > 0:
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3, r.stdout + r.stderr
    assert "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_cpp_hntr_typed_on_gpu():
    r = subprocess.run([compile_exe(allow_compile=False)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
