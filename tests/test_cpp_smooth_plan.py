"""Compiles the C++ test of a smoothed build's decisions (tests/cpp/test_smooth_plan.cpp: smooth_plan.h alone, with its own get_tuning)
with the host compiler and runs it: the bin geometry and its cap, the order of the device forms under every knob setting, the LDS
layout of the tile kernel, and the split of a shared tile build among 1..8 ranks over thousands of bin histograms -- arithmetic that
otherwise runs only inside the multi-process GPU tests."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_smooth_plan(tmp_path):
    exe = str(tmp_path / "test_smooth_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_smooth_plan.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
