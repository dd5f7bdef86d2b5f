"""Compiles the C++ test of a smoothed build's decisions (tests/cpp/test_smooth_plan.cpp: smooth_plan.h alone, with its own get_tuning)
with the host compiler and runs it: the bin geometry and its cap, the order of the device forms under every knob setting, the LDS
layout of the tile kernel, and the split of a shared tile build among 1..8 ranks over thousands of bin histograms -- arithmetic that
otherwise runs only inside the multi-process GPU tests."""
import cpp_programs as cpp


def test_cpp_smooth_plan():
    r = cpp.run(cpp.exe("test_smooth_plan"), timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
