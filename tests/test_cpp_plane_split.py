"""Compiles the C++ test of the int16 planes' 16-byte split (tests/cpp/test_plane_split.cpp: plane_split.h alone) with the host compiler
and runs it: head, pieces, tail and the loose-index map at every start address within a 16-byte block against every length 0..40, and
overlap on touching, nested and disjoint ranges -- the arithmetic globalec.hip, etopo1.hip and topoo.hip share on the host and in kernels."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_plane_split(tmp_path):
    exe = str(tmp_path / "test_plane_split")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_plane_split.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
