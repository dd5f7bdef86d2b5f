"""The table of C++ test programs (tests/cpp_programs.py) names every program there is, and building many of them goes on past
one that does not compile."""
import glob
import os

import cpp_programs as cpp


def test_every_cpp_program_is_in_the_table():
    stems = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(cpp.SRC, "test_*.cpp")))
    assert sorted(cpp.PROGRAMS) == stems


def test_one_failed_compile_does_not_stop_the_others(tmp_path):
    (tmp_path / "bad.cpp").write_text("int main() { return undeclared_name; }\n")
    (tmp_path / "good.cpp").write_text("int main() { return 0; }\n")
    programs = {"bad": cpp.HEADER_ONLY, "good": cpp.HEADER_ONLY}
    failed = cpp.build_many(["bad", "good"], programs=programs, srcdir=str(tmp_path), bindir=str(tmp_path / "bin"))
    assert list(failed) == ["bad"] and "undeclared_name" in failed["bad"]
    assert not os.path.exists(tmp_path / "bin" / "bad")
    good = str(tmp_path / "bin" / "good")       # built by build_many, after the one that failed: run as it lies, not through exe()
    assert os.path.exists(good)
    assert cpp.run(good).returncode == 0
