"""Compiles the C++ test of the launch choice (tests/cpp/test_apply_plan.cpp: apply_plan.h alone, with its own get_tuning) with the
host compiler and runs it: the rules for matrices of 2^23 rows / 2^24 entries, which no test builds on a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_apply_plan(tmp_path):
    exe = str(tmp_path / "test_apply_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_apply_plan.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
