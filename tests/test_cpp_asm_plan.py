"""Compiles the C++ test of the sorted-grid builds' decisions (tests/cpp/test_asm_plan.cpp: asm_plan.h alone, with its own get_tuning)
with the host compiler and runs it: both sides of every host-decided threshold, the knobs, the gate, and invariants over a sweep of
facts up to 2^31 - 1 exchange cells, which no test builds on a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_asm_plan(tmp_path):
    exe = str(tmp_path / "test_asm_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_asm_plan.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
