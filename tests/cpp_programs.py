"""The stand-alone C++ test programs under tests/cpp/: which exist, how each is compiled, where its executable lies and when it
may be recompiled, written down once.  __graft_entry__.build() builds the ones that link the library, so that they travel with
the tree to the GPU machine; the tests in tests/test_cpp_*.py and tests/test_ncio.py run them and read their files back."""
import os
import subprocess
import sys

import numpy as np

from icebin_amd import _capi
from icebin_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(SRC, "bin")
HOST_HEADERS = [os.path.join(ROOT, "icebin_amd", "host", h) for h in ("icebin_hip.hpp", "ncio.hpp", "hdf5.hpp")]

# the kinds: each fixes the compile line and what, besides its source, a program is stale against
HOST = "host"                   # the host API of icebin_hip.hpp, linked with libicebin_hip.so
NCIO = "ncio"                   # ncio.hpp / hdf5.hpp alone, no library
HEADER_ONLY = "header-only"     # a header of icebin_amd/csrc alone, no library, warnings are errors; compiled afresh every time
HEADER_ONLY_HIP = "header-only, with HIP's host headers"

# name -> kind; one entry per tests/cpp/test_*.cpp
PROGRAMS = {
    "test_host_api": HOST,
    "test_hntr": HOST,
    "test_hntr_typed": HOST,
    "test_hntr_matrix": HOST,
    "test_lonlat": HOST,
    "test_multivec": HOST,
    "test_modele": HOST,
    "test_modele_smoothed": HOST,
    "test_global_ec": HOST,
    "test_global_ec_chunks": HOST,
    "test_global_ave": HOST,
    "test_topo": HOST,
    "test_topo_pack": HOST,
    "test_etopo1_ice": HOST,
    "test_make_topoo": HOST,
    "test_ncio": NCIO,
    "test_apply_plan": HEADER_ONLY,         # apply_plan.h
    "test_asm_plan": HEADER_ONLY,           # asm_plan.h
    "test_smooth_plan": HEADER_ONLY,        # smooth_plan.h
    "test_plane_split": HEADER_ONLY,        # plane_split.h
    "test_hc_indexing": HEADER_ONLY_HIP,    # common.h
}
SHIPPED = [name for name, kind in PROGRAMS.items() if kind in (HOST, NCIO)]      # what build() builds ahead of the GPU run


def _recipe(kind):
    """g++'s flags in front of -o, those behind the source, and the files besides the source that make an executable stale
    (None: always stale.  The header-only programs compile in seconds, and so no list of what their headers include can go
    out of date)"""
    if kind == HOST:
        lib = build_library()
        libdir = os.path.dirname(lib)
        return (["-std=c++14", "-O1", "-Wall"], ["-L" + libdir, "-licebin_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"],
                [lib, os.path.join(ROOT, "include", "icebin_hip.h"), os.path.join(SRC, "host_test.h")] + HOST_HEADERS)
    if kind == NCIO:
        return ["-std=c++14", "-O1", "-Wall", "-DICEBIN_NCIO_HDF5"], ["-lz"], HOST_HEADERS[1:]
    flags = ["-std=c++17", "-O1", "-Wall", "-Werror"]
    if kind == HEADER_ONLY_HIP:
        flags += ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")]
    return flags, [], None


def exe(name, allow_compile=True, programs=PROGRAMS, srcdir=SRC, bindir=BIN):
    """The path of a program's executable, compiled first if it is missing or older than what it was made from.  The GPU-marked
    tests pass allow_compile=False: the executable was built beforehand and travels with the tree, so there it is compiled only
    if it is missing altogether.  `programs`, `srcdir` and `bindir` (here and in build_many) exist for
    tests/test_cpp_programs.py alone, which builds throw-away sources; nothing else passes them."""
    path, source = os.path.join(bindir, name), os.path.join(srcdir, name + ".cpp")
    if os.path.exists(path) and not allow_compile:
        return path
    flags, link, deps = _recipe(programs[name])
    if deps is None or not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(f) for f in [source] + deps):
        os.makedirs(bindir, exist_ok=True)
        r = subprocess.run(["g++"] + flags + ["-o", path, source] + link, capture_output=True, text=True)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            raise RuntimeError("g++ failed on %s.cpp:\n%s" % (name, r.stderr))
    return path


def build_many(names, **where):
    """Builds every one of the programs and returns {name: error} of those that failed: one failure does not stop the others."""
    failed = {}
    for name in names:
        try:
            exe(name, **where)
        except Exception as e:      # noqa: BLE001
            failed[name] = "%s: %s" % (type(e).__name__, e)
    return failed


def run(path, *args, timeout=None):
    return subprocess.run([path] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)


def fails_loudly_without_gpu(name, *args, timeout=None):
    """The body of every test_cpp_*_compiles_and_fails_loudly_without_gpu: without a device the program says that there is no
    CPU fallback and exits with 3."""
    import pytest       # here, not at the top: build() imports this module too
    path = exe(name)
    if _capi.device_count() > 0:
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = run(path, *args, timeout=timeout)
    assert r.returncode == 3, r.stdout + r.stderr
    assert "no CPU fallback" in r.stdout


# ---- the programs' array files: <int64 n><n values> (dump<T> of tests/cpp/host_test.h) ----
def read(path, dtype):
    with open(path, "rb") as f:
        n = int(np.frombuffer(f.read(8), np.int64)[0])
        return np.frombuffer(f.read(np.dtype(dtype).itemsize * n), dtype)


def write(path, a, dtype):
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    with open(path, "wb") as f:
        f.write(np.asarray([a.size], np.int64).tobytes())
        f.write(a.tobytes())


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
