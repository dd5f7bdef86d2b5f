"""Compiles the C++ test of the int16 planes' 16-byte split (tests/cpp/test_plane_split.cpp: plane_split.h alone) with the host compiler
and runs it: head, pieces, tail and the loose-index map at every start address within a 16-byte block against every length 0..40, and
overlap on touching, nested and disjoint ranges -- the arithmetic globalec.hip, etopo1.hip and topoo.hip share on the host and in kernels."""
import cpp_programs as cpp


def test_cpp_plane_split():
    r = cpp.run(cpp.exe("test_plane_split"), timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
