"""CPU-only: the scenes of tests/class_edge_cases.py are what they claim -- every elevation of a table lands on every kind of
exchange cell, the class pattern of every row is the one the table's comment gives (restated in
test_assembly_limit_cases.class_pattern), and the oracle builds every legal scene and refuses every other with the claimed cell."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import class_edge_cases as cec
    from test_assembly_limit_cases import ElevationOutOfBounds, cell_entries, class_pattern
finally:
    sys.path.pop(0)


def test_the_grid_is_small_and_has_every_kind_of_cell():
    g, _ = cec.scene()
    assert len(g["ex_area"]) < 1000
    for name, k in cec.kinds(g).items():
        assert k.any(), name


@pytest.mark.parametrize("name", list(cec.LEGAL))
def test_every_elevation_lands_on_every_kind_of_cell(name):
    g, em = cec.scene(**cec.LEGAL[name]["args"])
    args = cec.LEGAL[name]["args"]
    rows = cec.rows_of(args.get("table", "from_zero"), args.get("interp_style", 0), args.get("tiny", False))
    iI = g["ex_indices"][:, 1].astype(np.int64)
    row_of_x = iI % len(rows)
    np.testing.assert_array_equal(em[:len(em) - (1 if "spare_ice" in args else 0)].view(np.uint64),
                                  rows[np.arange(g["nI"] - (1 if "spare_ice" in args else 0)) % len(rows)].view(np.uint64))
    for kind, k in cec.kinds(g).items():
        assert set(row_of_x[k].tolist()) == set(range(len(rows))), (kind, sorted(set(range(len(rows))) - set(row_of_x[k].tolist())))


def pattern_of(hc, e, style=0):
    i0, i1, w0, w1 = class_pattern(hc, np.array([e]), style)
    return int(i0[0]), int(i1[0]), float(w0[0]), float(w1[0])


def test_the_rows_have_the_class_patterns_the_table_is_there_for():
    a, b = cec.TABLES["from_zero"], cec.TABLES["above_zero"]
    # Z_INTERP over a table from zero: zero, minus zero and a negative elevation sit on class 0 (the clamp), and so does the
    # smallest subnormal (its ratio underflows); 1e-300 is between 0 and 1 with an upper weight of 1e-302
    for e in (0.0, -0.0, -5.0, 5e-324):
        i0, i1, w0, w1 = pattern_of(a, e)
        assert (i0, i1, w0) == (0, 1, 1.0) and w1 == 0
    assert pattern_of(a, 1e-300) == (0, 1, 1.0, 1e-302)
    # around a class: one ulp below -> two classes, the upper weight rounds to 1 - 2^-53 or so; on it -> lower_bound names it as the
    # UPPER index with weight 1; one ulp above -> the next interval
    i0, i1, w0, w1 = pattern_of(a, np.nextafter(100.0, 0.0))
    assert (i0, i1) == (0, 1) and 0 < w0 < 1e-15 and 0 < w1 < 1
    assert pattern_of(a, 100.0) == (0, 1, 0.0, 1.0)
    i0, i1, w0, w1 = pattern_of(a, np.nextafter(100.0, 200.0))
    assert (i0, i1) == (1, 2) and 0 < w1 < 1e-15 and w0 == 1.0 - w1
    assert pattern_of(a, 150.0) == (1, 2, 0.5, 0.5) and pattern_of(a, 250.0) == (2, 3, 0.5, 0.5)
    # the top class: exactly on it is legal (upper index nhc - 1), one ulp beyond is not
    assert pattern_of(a, 300.0) == (2, 3, 0.0, 1.0)
    i0, i1, w0, w1 = pattern_of(a, np.nextafter(300.0, 0.0))
    assert (i0, i1) == (2, 3) and w0 > 0 and w1 > 0
    with pytest.raises(ElevationOutOfBounds):
        pattern_of(a, np.nextafter(300.0, np.inf))
    with pytest.raises(ElevationOutOfBounds):
        pattern_of(np.array([0.0]), 0.0)                          # one class: no interval
    # a table whose lowest class is above zero: the clamped elevation extrapolates below it
    for e in (0.0, -0.0, -5.0, 5e-324, 1e-300):
        assert pattern_of(b, e) == (0, 1, 2.0, -1.0)
    assert pattern_of(b, 100.0) == (0, 1, 1.0, 0.0)               # (the lowest class exactly: lower_bound 0, raised to 1)
    assert pattern_of(b, 400.0) == (2, 3, 0.0, 1.0)
    # ELEV_CLASS_INTERP: the nearest class, the lower one on a tie; beyond either end the end class
    assert pattern_of(a, 50.0, 1)[0] == 0 and pattern_of(a, np.nextafter(50.0, 100.0), 1)[0] == 1
    assert pattern_of(b, 150.0, 1)[0] == 0 and pattern_of(b, np.nextafter(150.0, 200.0), 1)[0] == 1
    assert pattern_of(a, 1e300, 1)[0] == 3 and pattern_of(a, 350.0, 1)[0] == 3 and pattern_of(b, 50.0, 1)[0] == 0 and pattern_of(a, -50.0, 1)[0] == 0
    # NaN is the mask
    assert pattern_of(a, np.nan) == (-1, -1, 0.0, 0.0)


@pytest.mark.parametrize("name", list(cec.LEGAL))
def test_the_oracle_builds_every_legal_scene(name):
    g, em = cec.scene(**cec.LEGAL[name]["args"])
    rg = orc.Regridder(g)
    em_named = em.copy()
    if "spare_ice" in cec.LEGAL[name]["args"]:                    # (the restatement walks ice cells: without the one nobody names)
        assert g["nI"] - 1 not in g["ex_indices"][:, 1]
        with pytest.raises(ElevationOutOfBounds):
            class_pattern(g["hcdefs"], em, 0)
        em_named[-1] = np.nan
    ce = cell_entries(g, em_named)
    for m in cec.E_MATRICES:
        w = rg.matrix_d(m, em, scale=False, correctA=False)
        assert w.nnz > 0, m
        if m in ("EvX", "XvE"):                                   # nothing merges on X: the restatement's entries
            assert w.nnz == int(np.count_nonzero(ce["has0"]) + np.count_nonzero(ce["has1"])), m
    # the mask of a scene that hands the streamed build on has a weight below 1e-30 and no underflow; the others have neither
    i0, i1, w0, w1 = class_pattern(g["hcdefs"], em_named, g["interp_style"])
    smallest = min(np.abs(w[w != 0]).min() for w in (w0, w1) if np.any(w != 0))
    assert (smallest < 1e-30) == (cec.LEGAL[name]["stream_path"] == 1), smallest
    assert not np.any(ce["under0"] | ce["under1"])


@pytest.mark.parametrize("name", list(cec.REFUSED))
def test_the_oracle_refuses_the_other_scenes_with_the_first_offender(name):
    args, ice = cec.REFUSED[name]
    g, em = cec.scene(**args)
    rg = orc.Regridder(g)
    iI = g["ex_indices"][:, 1].astype(np.int64)
    hc = g["hcdefs"]
    if ice is None:                                               # every unmasked cell offends: the first exchange cell of one
        ice = int(iI[np.flatnonzero(~np.isnan(em[iI]))[0]])
    else:
        # the claimed cell is the offender whose exchange cell comes first
        off = np.flatnonzero(np.maximum(em, 0.0) > hc[-1])
        first_x = {int(i): int(np.flatnonzero(iI == i)[0]) for i in off}
        assert ice == min(first_x, key=first_x.get), first_x
        if len(off) > 1:
            assert ice != int(off.min())                           # (... and not the one with the lowest ice index)
    with pytest.raises(ElevationOutOfBounds):
        class_pattern(hc, em, 0)
    text = "Elevation %g out of bounds (%g, %g)" % (max(em[ice], 0.0), hc[0], hc[-1])
    for m in cec.E_MATRICES:
        with pytest.raises(orc.OracleError) as ei:
            rg.matrix_d(m, em)
        assert str(ei.value) == text, (m, str(ei.value))
    assert rg.matrix_d("AvI", em).nnz > 0                          # a matrix without classes is built all the same
    if "cells" in args:                                           # ... and with the offenders under the mask so is every other
        masked = em.copy()
        masked[list(args["cells"])] = np.nan
        class_pattern(hc, masked, 0)
        for m in cec.E_MATRICES:
            assert rg.matrix_d(m, masked).nnz > 0, m
