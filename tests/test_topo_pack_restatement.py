"""Pins tests/topo_pack_restatement.py by hand on a 2 x 2 atmosphere grid with two elevation classes (and the sea-land class
behind them, which is never packed): the indices, the order of the entries, the initialisation step's aliasing of mergemaskA0
and the two-step unit conversion.  CPU only."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topo_pack_restatement as pr  # noqa: E402

IM, JM, NHC = 2, 2, 2
A0 = [10., 11., 12., 13.]
A1 = [20., 21., 22., 23.]
FHC = [.1, .2, .3, .4, .5, .6, .7, .8, 9., 9., 9., 9.]          # (ihc, j, i); the last four: the sea-land class
UNDERICE = [1, 0, 0, 2, 2, 0, 1, 1, 5, 5, 5, 5]


def indexingA(i, j):
    return j * IM + i


def slowest(i, j, ihc):         # indexingE with the class slowest: strides (1, nA)
    return (j * IM + i) + ihc * IM * JM


def fastest(i, j, ihc):         # the class fastest: strides (nhc, 1)
    return (j * IM + i) * NHC + ihc


def step(c, run_ice, mask, indexingE=slowest, **kw):
    return c.pack(run_ice, mask, [A0, A1], [FHC, pr.underice_d(UNDERICE)], NHC, IM, JM, indexingA, indexingE, **kw)


def test_underice_d_is_the_int16_plane_as_doubles():
    d = pr.underice_d(UNDERICE)
    assert d == [1., 0., 0., 2., 2., 0., 1., 1., 5., 5., 5., 5.] and all(type(x) is float for x in d)


def test_initialisation_step_uses_its_own_mask():
    c = pr.Coupler()
    A, E = step(c, False, [1, 0, 0, 7])
    assert A.index == [0, 3] and A.weights == [1., 1.] and A.vals == [10., 20., 13., 23.]
    # the classes outermost, the cells ascending inside each; the sea-land class is not there
    assert E.index == [0, 3, 4, 7] and E.weights == [1.] * 4
    assert E.vals == [.1, 1., .4, 2., .5, 2., .8, 1.]
    assert c.mergemaskA0 == [1, 0, 0, 7]


def test_second_step_keeps_the_cells_of_the_previous_mask():
    c = pr.Coupler()
    step(c, False, [1, 0, 0, 7])
    A, E = step(c, True, [0, -1, 0, 0])
    # cell 1 by the new mask, cells 0 and 3 by the previous one alone, cell 2 by neither
    assert A.index == [0, 1, 3] and A.vals == [10., 20., 11., 21., 13., 23.]
    assert E.index == [0, 1, 3, 4, 5, 7]
    assert E.vals == [.1, 1., .2, 0., .4, 2., .5, 2., .6, 0., .8, 1.]
    assert c.mergemaskA0 == [0, -1, 0, 0]
    # the third step no longer sees the first mask
    A, _ = step(c, True, [0, 0, 1, 0])
    assert A.index == [1, 2]


def test_initialisation_aliases_whatever_was_stored():
    c = pr.Coupler()
    step(c, False, [1, 1, 1, 1])
    A, E = step(c, False, [0, 0, 1, 0])         # run_ice = False again: the stored mask is replaced before it is read (:1017)
    assert A.index == [2] and E.index == [2, 6]


def test_class_fastest_indexing():
    c = pr.Coupler()
    _, E = step(c, False, [1, 0, 0, 7], indexingE=fastest)
    assert E.index == [0, 6, 1, 7]              # still the classes outermost: the ORDER does not follow the index


def test_empty_mask_packs_nothing():
    c = pr.Coupler()
    A, E = step(c, False, [0, 0, 0, 0])
    assert A.size() == 0 and E.size() == 0 and A.vals == [] and E.vals == []


def test_unit_conversion_is_a_product_then_an_add():
    v = pr.VectorMultivec(2)
    x = 1. + 2. ** -30
    v.add(5, [x, 3.], 1.0)
    v.add(6, [2., -0.], 1.0)
    pr.convert_units(v, [x, 2.], [-1., .5])
    # x * x = 1 + 2^-29 + 2^-60 rounds to 1 + 2^-29 before the add; a fused multiply-add would leave 2^-29 + 2^-60
    assert v.vals == [2. ** -29, 6.5, 2. * x - 1., .5]
    assert v.vals[0] != 2. ** -29 + 2. ** -60
    assert v.index == [5, 6] and v.weights == [1., 1.]


def test_conversion_runs_after_the_mask_is_stored_and_over_both_vectors():
    c = pr.Coupler()
    A, E = step(c, False, [0, 1, 0, 0], unitsA=([1., 2.], [.5, 0.]), unitsE=([10., 1.], [0., 1.]))
    assert A.vals == [11.5, 42.] and E.vals == [2., 1., 6., 1.]
