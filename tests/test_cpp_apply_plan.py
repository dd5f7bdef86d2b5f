"""Compiles the C++ test of the launch choice (tests/cpp/test_apply_plan.cpp: apply_plan.h alone, with its own get_tuning) with the
host compiler and runs it: the rules for matrices of 2^23 rows / 2^24 entries, which no test builds on a GPU."""
import cpp_programs as cpp


def test_cpp_apply_plan():
    r = cpp.run(cpp.exe("test_apply_plan"), timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
