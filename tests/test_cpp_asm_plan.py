"""Compiles the C++ test of the sorted-grid builds' decisions (tests/cpp/test_asm_plan.cpp: asm_plan.h alone, with its own get_tuning)
with the host compiler and runs it: both sides of every host-decided threshold, the knobs, the gate, and invariants over a sweep of
facts up to 2^31 - 1 exchange cells, which no test builds on a GPU."""
import cpp_programs as cpp


def test_cpp_asm_plan():
    r = cpp.run(cpp.exe("test_asm_plan"), timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
