"""CPU checks of the L1 arithmetic as tests/l1_restatement.py restates it (icebin_amd/csrc/l1.hip computes the same bits on
the GPU, tests/test_gpu_l1.py): against exact rational arithmetic on every case of tests/golden/l1_reference.npz, against the
reference's own pylib/icebin/element_l1.py where that is sound, and against the known answers of the reference's test."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import l1_restatement as R  # noqa: E402


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in R.CASES:
        c = R.load_case(name)
        c["restated"] = R.cell_terms(c["vx"], c["vy"], c["tri"], c["ex_iTri"], c["ex_vptr"], c["ex_qx"], c["ex_qy"])
        c["exact"] = [[Fraction(float(c["exact_hi"][x, k])) + Fraction(float(c["exact_lo"][x, k])) for k in range(3)]
                      for x in range(len(c["ex_iTri"]))]
        out[name] = c
    return out


def test_fixture_holds_the_cases_the_tolerances_refer_to(cases):
    assert len(cases["jit9"]["ex_iA"]) == 241 and int(cases["jit9"]["nnz"]) == 224
    assert len(cases["jit9_far"]["ex_iA"]) == 241
    assert len(cases["jit24"]["tri"]) == 1058 and len(cases["jit24"]["tri"]) % 64 != 0
    for name in R.CASES:
        c = cases[name]
        assert np.isfinite(c["ref_err"]) and np.isfinite(c["restate_err"]), name
        nv = np.diff(c["ex_vptr"])
        assert nv.min() >= 3 and nv.max() <= 19 and np.all(c["poly_area"] > 0), name
    assert set(np.diff(cases["jit9"]["ex_vptr"]).tolist()) == {3, 4, 5}
    # the fixture builds cells triangle by triangle: the (iA, iTri) sort has work to do
    assert np.any(np.diff(R.sort_cells(cases["jit9"]["ex_iA"], cases["jit9"]["ex_iTri"])) < 0)
    # where the reference is not sound its terms are kept for the record only
    assert cases["jit9_far"]["ref_err"] > 1e-5 and cases["jit9"]["ref_err"] < 1e-10


@pytest.mark.parametrize("name", R.CASES)
def test_terms_within_1e15_of_element_area_of_exact(cases, name):
    # every restated term within 1e-15 x the element's area of the exact term (measured worst: 1.9e-16, jit24)
    c = cases[name]
    elem = [Fraction(float(a)) for a in c["elem_area"]]
    worst = R.max_err_over(c["restated"], c["exact"], elem)
    print("%s: worst |restated - exact| / element area = %.3e (fixture recorded %.3e)" % (name, worst, float(c["restate_err"])))
    assert worst <= 1e-15, (name, worst)


@pytest.mark.parametrize("name", ["four_tri_a1", "four_tri_a2", "jit9"])
def test_terms_within_4_ref_err_of_the_reference(cases, name):
    # per polygon area; the reference's own distance from exact sets the scale, x4 covers the two errors adding
    c = cases[name]
    d = np.max(np.abs(c["restated"] - c["ref_terms"]) / c["poly_area"][:, None])
    print("%s: max |restated - reference| / polygon area = %.3e, ref_err = %.3e" % (name, d, float(c["ref_err"])))
    assert d <= 4 * float(c["ref_err"]), (name, d, float(c["ref_err"]))


def test_known_answers_of_the_references_test(cases):
    # pylib/icebin/tests/test_regrid_l1.py test_A1: vertex weights 2/3 x4 and 4/3; weightsA = [4]
    c = cases["four_tri_a1"]
    p = R.sort_cells(c["ex_iA"], c["ex_iTri"])
    row, col, val = R.triplets(c["tri"], c["ex_iA"][p], c["ex_iTri"][p], c["restated"][p])
    rowptr, ocol, oval, wM, Mw = R.assemble(row, col, val, 1, 5)
    assert np.max(np.abs(Mw - np.array([2 / 3, 2 / 3, 2 / 3, 2 / 3, 4 / 3]))) <= 1e-15
    assert np.max(np.abs(wM - 4.0)) <= 1e-15
    assert ocol.tolist() == [0, 1, 2, 3, 4] and np.max(np.abs(oval - Mw)) <= 1e-15
    assert np.max(np.abs(c["ref_weightsI"] - Mw)) <= 1e-14 and abs(c["ref_weightsA"][0] - 4.0) <= 1e-14
    # test_A2: the two cells share the weight
    c = cases["four_tri_a2"]
    p = R.sort_cells(c["ex_iA"], c["ex_iTri"])
    row, col, val = R.triplets(c["tri"], c["ex_iA"][p], c["ex_iTri"][p], c["restated"][p])
    _, _, _, wM, Mw = R.assemble(row, col, val, 2, 5)
    assert np.max(np.abs(wM - 2.0)) <= 1e-15 and abs(wM.sum() - Mw.sum()) <= 1e-15


@pytest.mark.parametrize("name", R.CASES)
def test_assembly_order_and_transpose(cases, name):
    # IvA is AvI with the roles swapped: the same values, wM and Mw exchanged, bit for bit
    c = cases[name]
    p = R.sort_cells(c["ex_iA"], c["ex_iTri"])
    nA, nI = int(c["nA"]), len(c["vx"])
    a = R.assemble(*R.triplets(c["tri"], c["ex_iA"][p], c["ex_iTri"][p], c["restated"][p], "AvI"), nA, nI)
    t = R.assemble(*R.triplets(c["tri"], c["ex_iA"][p], c["ex_iTri"][p], c["restated"][p], "IvA"), nI, nA)
    assert len(a[2]) == int(c["nnz"]) == len(t[2])
    assert np.array_equal(a[3].view(np.uint64), t[4].view(np.uint64)) and np.array_equal(a[4].view(np.uint64), t[3].view(np.uint64))
    rows_a = np.repeat(np.arange(nA), np.diff(a[0]))
    rows_t = np.repeat(np.arange(nI), np.diff(t[0]))
    o = np.lexsort((rows_t, t[1]))
    assert np.array_equal(t[1][o], rows_a) and np.array_equal(rows_t[o], a[1])
    assert np.array_equal(t[2][o].view(np.uint64), a[2].view(np.uint64))
