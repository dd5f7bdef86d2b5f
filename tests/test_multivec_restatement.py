"""Pins tests/multivec_restatement.py -- what the GPU tests compare with bitwise -- on cases small enough to work out by hand."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multivec_restatement as mr  # noqa: E402


def mv_of(nvar, entries):
    mv = mr.Multivec(nvar)
    for ix, val, w in entries:
        mv.add(ix, val, w)
    return mv


def test_layout_is_entry_major():
    mv = mv_of(2, [(5, [1.0, 2.0], 0.5), (3, [3.0, 4.0], 0.25)])
    index, weights, vals = mv.arrays()
    assert index.tolist() == [5, 3] and weights.tolist() == [0.5, 0.25]
    assert vals.tolist() == [[1.0, 2.0], [3.0, 4.0]]
    assert mv.val(1, 0) == 2.0 and mv.val(0, 1) == 3.0       # vals[ix * nvar + ivar]


def test_two_sheets_sharing_a_cell_give_the_weighted_mean():
    # an unscaled product holds sum(M x): weight * mean.  Sheet 1: weight 3, mean 10; sheet 2: weight 1, mean 2.
    mv = mv_of(1, [(4, [30.0], 3.0), (4, [2.0], 1.0), (1, [8.0], 2.0)])
    scale = mr.to_dense_scale(mv, 6)
    assert scale[4] == 0.25 and scale[1] == 0.5
    out = mr.to_dense(mv, scale, -1.0)
    assert out[0, 4] == 30.0 * 0.25 + 2.0 * 0.25 == 8.0        # (3*10 + 1*2) / 4
    assert out[0, 1] == 4.0
    assert out[0, [0, 2, 3, 5]].tolist() == [-1.0] * 4


def test_untouched_cells_have_infinite_scale():
    scale = mr.to_dense_scale(mv_of(1, [(2, [1.0], 4.0)]), 4)
    assert scale.tolist() == [np.inf, np.inf, 0.25, np.inf]
    assert np.all(mr.to_dense_scale(mr.Multivec(3), 2) == np.inf)


def test_nan_rule_three_cases():
    nan = np.nan
    #  cell 0: NaN then 6   -> the NaN is forgotten: 6 * 0.5 = 3
    #  cell 1: 6 then NaN   -> NaN at the end: fill
    #  cell 2: the weights sum to zero -> scale 1/0 = inf, and the term 0 * inf = NaN -> fill
    #  cell 3: NaN, 2, 4    -> 2*0.25 + 4*0.25 = 1.5
    mv = mv_of(1, [(0, [nan], 1.0), (0, [6.0], 1.0),
                   (1, [6.0], 1.0), (1, [nan], 1.0),
                   (2, [0.0], 0.0),
                   (3, [nan], 1.0), (3, [2.0], 1.0), (3, [4.0], 2.0)])
    scale = mr.to_dense_scale(mv, 5)
    assert scale.tolist() == [0.5, 0.5, np.inf, 0.25, np.inf]
    out = mr.to_dense(mv, scale, -9.0)
    assert out[0].tolist() == [3.0, -9.0, -9.0, 1.5, -9.0]


def test_update_dense_clears_touched_cells_only_and_starts_from_zero():
    mv = mv_of(2, [(1, [2.0, -0.0], 2.0), (1, [4.0, -0.0], 2.0), (3, [1.0, 1.0], 1.0)])
    scale = mr.to_dense_scale(mv, 4)
    out = np.full((2, 4), 7.0)
    mr.update_dense(mv, scale, out)
    assert out[0].tolist() == [7.0, 1.5, 7.0, 1.0]
    assert out[1].tolist() == [7.0, 0.0, 7.0, 1.0]
    assert not np.signbit(out[1, 1])         # 0.0 + (-0.0 * 0.25) = +0.0


def test_first_seen_numbering_with_duplicates_and_a_prepopulated_set():
    mv = mv_of(1, [(9, [1.0], 0), (4, [2.0], 0), (9, [3.0], 0), (7, [4.0], 0), (4, [5.0], 0), (2, [6.0], 0)])
    assert mr.add_dense([], mv) == [9, 4, 7, 2]
    assert mr.add_dense([7, 100], mv) == [7, 100, 9, 4, 2]
    out = mr.densify(mv, [7, 100, 9, 4, 2])
    assert out.tolist() == [[4.0, 0.0, 4.0, 7.0, 6.0]]
    with pytest.raises(KeyError, match="entry 3: index 7"):
        mr.densify(mv, [9, 4, 2])


def test_append_weighted_transposes():
    mv = mr.Multivec(3)
    B = np.arange(6, dtype=np.float64).reshape(3, 2)       # B[ivar, row]
    mr.append_weighted(mv, [11, 5], [0.5, 1.5], B)
    index, weights, vals = mv.arrays()
    assert index.tolist() == [11, 5] and weights.tolist() == [0.5, 1.5]
    assert vals.tolist() == [[0.0, 2.0, 4.0], [1.0, 3.0, 5.0]]
    with pytest.raises(ValueError, match="Inconsistant nvar"):
        mr.append_weighted(mv, [1], [1.0], np.zeros((2, 1)))


def test_concatenate_and_refusals():
    a, b = mv_of(1, [(1, [1.0], 1.0)]), mv_of(1, [(0, [2.0], 3.0), (1, [4.0], 5.0)])
    c = mr.concatenate([a, b])
    assert c.index == [1, 0, 1] and c.weights == [1.0, 3.0, 5.0] and c.vals == [1.0, 2.0, 4.0]
    with pytest.raises(ValueError, match="at least one"):
        mr.concatenate([])
    with pytest.raises(ValueError, match="Inconsistant nvar"):
        mr.concatenate([a, mr.Multivec(2)])
    with pytest.raises(IndexError, match="entry 1: Index out of range: 4 vs. 4"):
        mr.to_dense_scale(mv_of(1, [(0, [0.0], 1.0), (4, [0.0], 1.0)]), 4)
    with pytest.raises(IndexError, match="entry 0: Index out of range: -1"):
        mr.to_dense(mv_of(1, [(-1, [0.0], 1.0)]), np.ones(4), 0.0)
