"""The inputs of tests/test_gpu_apply_sidepaths.py, checked on the CPU: every case lies where its path needs it -- the coefficient counts
on both sides of the inline table, the entry counts on both sides of the wave form, the chunk counts of the weight dots, the row counts
around the longest-rows-first limit -- every NaN-pattern case has NaN rows and other rows, the exact cases are exact in any order, and
the plain references of apply_sidepath_cases agree with the CPU oracle within the bounds that the GPU test gates with."""
import math
import os
import sys

import numpy as np
import pytest

from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import apply_sidepath_cases as asc
finally:
    sys.path.pop(0)


def oracle_of(m, conservative=True):
    return orc.Weighted.from_coo(m.nrow, m.ncol, m.row, m.colind, m.val, m.wM, m.Mw, conservative=conservative)


def both_kinds_of_rows(ref):
    nan_rows = np.isnan(ref).any(axis=0)
    return nan_rows.any() and (~np.isnan(ref)).all(axis=0).any()


# ---- the matrices ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", asc.SHAPES_A + ((asc.NROW_B, asc.NCOL_B),))
def test_side_matrix_has_the_rows_the_issue_lists(shape):
    nrow, ncol = shape
    m = asc.side_matrix(nrow, ncol, seed=nrow + ncol)
    assert (m.nrow, m.ncol, len(m.wM), len(m.Mw)) == (nrow, ncol, nrow, ncol)
    for n in asc.LENGTHS:
        assert m.cnt[m.where["len%d" % n]] == min(n, ncol - 1) and m.wM[m.where["len%d" % n]] != 0.0
    assert m.cnt[m.where["dead_entries"]] == min(66, ncol - 1) and m.wM[m.where["dead_entries"]] == 0.0
    assert m.cnt[m.where["dead_empty"]] == 0 and m.wM[m.where["dead_empty"]] == 0.0
    assert np.sum(m.wM == 0.0) == 2 and np.sum(m.cnt == 0) == 2
    rest = np.delete(m.cnt, list(m.where.values()))
    assert set(rest.tolist()) == {2, 3, 4}
    assert not np.any(m.val == 0.0) and ncol - 1 not in set(m.colind.tolist())
    for r in range(nrow):                                    # a CSR row names a column once, in ascending order
        assert np.all(np.diff(m.colind[m.entries(r)]) > 0)


# ---- A --------------------------------------------------------------------------------------------------------------------------------
def test_transform_sizes_sit_on_both_sides_of_the_inline_table():
    counts = {s: asc.coefficient_count(*s) for s in asc.SIZES_A}
    assert counts[(23, 16)] == counts[(31, 12)] == asc.TB_MAX == 384 and counts[(24, 16)] == 400
    assert all(c <= asc.TB_MAX for s, c in counts.items() if s != (24, 16))
    sides = {s: asc.transforms_inputs_side(*s) for s in asc.SHAPES_A}
    assert sides == {(400, 255): True, (400, 256): True, (400, 257): True, (256, 256): True, (255, 400): False, (256, 400): False,
                     (257, 400): False}
    small = sorted(min(s) for s in asc.SHAPES_A)
    assert small == [255, 255, 256, 256, 256, 257, 257]                    # one block, exactly one block, two blocks of 256
    T, b = asc.transform(5, 3, 0)
    assert not T[2].any() and all(np.count_nonzero(T[:, k]) == 2 for k in range(3))
    for s in asc.SIZES_A:
        for seed in (0, 1):
            T, b = asc.transform(*s, seed)
            assert np.all(b != 0.0) and len(set(b.tolist())) == len(b)
    assert not np.array_equal(asc.transform(24, 16, 0)[0], asc.transform(24, 16, 1)[0])


@pytest.mark.parametrize("size", asc.SIZES_A, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("shape", asc.SHAPES_A, ids=lambda s: "%dx%d" % s)
def test_transformed_reference_is_the_oracle(shape, size):
    m = asc.side_matrix(*shape, seed=sum(shape))
    o = oracle_of(m)
    T, b = asc.transform(*size, 0)
    V = asc.transform_inputs(m, size[0], seed=11, T=T)
    worst = 0.0
    for fill in (asc.FILL, np.nan):
        y = o.apply_transformed(V, T, b, fill=fill)
        worst = max(worst, asc.check_transformed(m, y, V, T, b, fill, "oracle %s %s" % (shape, size)))
    print("transformed %s %s: oracle err/bound %.3f" % (shape, size, worst))
    # the NaN of variable 0 at one column reaches exactly the rows that store it, in the outputs that use variable 0
    ref, _ = asc.transformed_ref(m, V, T, b, asc.FILL)
    stores = np.zeros(m.nrow, bool)
    stores[m.row[m.colind == asc.nan_column(m)]] = True
    stores &= m.wM != 0.0
    assert stores.any() and not stores.all()
    np.testing.assert_array_equal(np.isnan(ref), (T[0] != 0.0)[:, None] & stores[None, :])
    assert both_kinds_of_rows(ref)
    if size == (5, 3):
        assert np.all(np.isnan(V[2])) and np.isnan(ref[0]).any() and not np.isnan(ref[1]).any()


# ---- B --------------------------------------------------------------------------------------------------------------------------------
def test_matvec_matrices_straddle_the_wave_form():
    thread, wave = asc.matvec_matrices()
    assert thread.nrow == wave.nrow == asc.NROW_B > 256                    # more than one block of threads
    assert thread.nnz == 8 * thread.nrow - 1 and wave.nnz == 8 * wave.nrow
    differ = np.flatnonzero(thread.cnt != wave.cnt)
    assert len(differ) == 1 and thread.cnt[differ[0]] == 3 and wave.cnt[differ[0]] == 4
    assert thread.where == wave.where
    for r in range(thread.nrow):
        a, b = thread.colind[thread.entries(r)], wave.colind[wave.entries(r)]
        assert set(a.tolist()) <= set(b.tolist())
        keep = np.isin(b, a)
        np.testing.assert_array_equal(thread.val[thread.entries(r)], wave.val[wave.entries(r)][keep])
    assert thread.cnt[thread.where["len1025"]] == 1025


@pytest.mark.parametrize("ignore_nan", [0, 1])
@pytest.mark.parametrize("nvar", [1, 3])
@pytest.mark.parametrize("form", [0, 1], ids=["thread", "wave"])
def test_matvec_reference_is_the_oracle(form, nvar, ignore_nan):
    import scipy.sparse
    m = asc.matvec_matrices()[form]
    X = asc.matvec_inputs(m, nvar, seed=5)
    Y0 = np.full((nvar, m.nrow), asc.FILL)
    ref, tol, written = asc.matvec_ref(m, X, Y0, ignore_nan)
    M = scipy.sparse.coo_matrix((m.val, (m.row, m.colind)), shape=(m.nrow, m.ncol))
    trip = asc.shuffled_duplicate_triplets(m, seed=9)
    M2 = scipy.sparse.coo_matrix((trip[2], (trip[0], trip[1])), shape=(m.nrow, m.ncol))
    merged = asc.csr_from_coo(m.nrow, m.ncol, *trip, m.wM, m.Mw)
    np.testing.assert_array_equal(merged.colind, m.colind)
    assert asc.same_bits(merged.val, m.val)                                # the halves add up exactly: the same matrix
    for f in range(nvar):
        for MM in (M, M2):
            y = orc.coo_matvec(MM, X[f], fill=asc.FILL, ignore_nan=bool(ignore_nan))
            assert np.all(y[~written[f]] == asc.FILL)
            r = asc.gate(y, ref[f], tol[f], "oracle coo_matvec")
        print("matvec form %d var %d ignore_nan %d: oracle err/bound %.3f" % (form, f, ignore_nan, r))
    r63, r64, r65, r130, r1025, r0 = (m.where[k] for k in ("len63", "len64", "len65", "len130", "len1025", "len0"))
    gone = asc.matvec_all_nan_rows(m)
    assert len(gone) == 2 and m.cnt[gone[0]] == 1 and 2 <= m.cnt[gone[1]] <= 4
    assert not written[:, r0].any()                                         # the empty row keeps its canary in both modes
    k = m.entries(r130)
    alive = np.flatnonzero(~np.isnan(X[0, m.colind[k]]))
    assert {3, 64, 129} <= set(alive.tolist()) and 3 <= len(alive) < 65     # survivors at entries 64 and 129 of the 130-entry row
    if ignore_nan:
        assert not written[0, gone].any()                                   # every input NaN: nothing survives
        assert written[0, r130] and not np.isnan(ref).any()
        want = (m.val[k][alive].astype(asc.LD) * X[0, m.colind[k]][alive].astype(asc.LD)).sum()
        assert abs(ref[0, r130] - want) <= 4 * asc.U * abs(want)
        assert written[0].sum() == (m.cnt > 0).sum() - 2
    else:
        assert np.isnan(ref[0, gone + [r130, r1025]]).all() and written[0, gone + [r130]].all()
        assert both_kinds_of_rows(ref[:1]) and both_kinds_of_rows(ref)
        assert not np.isnan(ref[0, [r63, r64, r65]]).any()                  # rows on both sides of the wave's 64 lanes stay finite
        if nvar == 3:
            assert not np.isnan(ref[1]).any() and both_kinds_of_rows(ref[2:])


# ---- C --------------------------------------------------------------------------------------------------------------------------------
def test_weight_dot_sizes_have_the_chunks_the_issue_lists():
    want = {1: (1, 1), 64: (1, 64), 1024: (1, 1024), 1025: (1, 1025), 4096: (1, 4096), 4097: (2, 2049), 8193: (3, 2731),
            1 << 20: (256, 4096), (1 << 20) + 1: (256, 4097)}
    assert {n: asc.weight_dot_chunks(n) for n in asc.SIZES_C} == want
    for n, (c, ln) in want.items():
        assert (c - 1) * ln < n <= c * ln                                   # every chunk holds an element, the chunks cover n


@pytest.mark.parametrize("n", asc.SIZES_C)
def test_weight_dot_references(n):
    for exact in (False, True):
        m = asc.empty_matrix(n, seed=n, exact=exact)
        o = oracle_of(m)
        for dim, w in ((0, m.wM), (1, m.Mw)):
            assert n < 10 or np.sum(w == 0.0) == n // 10
            A = asc.weight_fields(w, 3, seed=n + dim, exact=exact)
            assert np.all(np.isnan(A[:, w == 0.0])) and not np.isnan(A[:, w != 0.0]).any()
            assert not any(np.array_equal(A[0], A[k]) for k in (1, 2)) or n == 1
            ref, tol = asc.weight_dot_ref(w, A)
            assert np.all(np.isfinite(ref.astype(np.float64)))
            y = o.apply_weight(dim, np.nan_to_num(A))                      # the oracle multiplies by the zero weights: NaN taken out
            r = asc.gate(y, ref, tol, "oracle apply_weight n=%d dim=%d" % (n, dim))
            if exact:                                                      # the premise of the bitwise check: any order, the same bits
                for k in range(3):
                    t = (w * np.nan_to_num(A[k]))
                    assert float(np.cumsum(t)[-1]) == math.fsum(t) == float(ref[k]) == y[k]
            else:
                print("weight dot n=%d dim=%d: oracle err/bound %.3f" % (n, dim, r))


# ---- D --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrow", [4096, 4097])
def test_correction_reference_is_the_oracle(nrow):
    ncol = 900
    assert asc.weight_dot_chunks(nrow)[0] == (1 if nrow == 4096 else 2) and asc.weight_dot_chunks(ncol)[0] == 1
    row, col, val, wM, Mw, nan_cols = asc.random_coo(nrow, ncol, 8, seed=nrow)
    assert len(nan_cols) and np.all(Mw[nan_cols] == 0.0) and not np.isin(nan_cols, col).any()
    m = asc.csr_from_coo(nrow, ncol, row, col, val, wM, Mw)
    o = orc.Weighted.from_coo(nrow, ncol, row, col, val, wM, Mw, conservative=False)
    X = asc.correction_fields(3, ncol, nan_cols)
    y0 = o.apply(X, fill=asc.FILL, force_conservation=False)
    r0 = asc.check_product(m, y0, X, asc.FILL, "oracle uncorrected")
    y1 = o.apply(X, fill=asc.FILL, force_conservation=True)
    exact, tol, _ = asc.correction_ref(y0, X, wM, Mw)
    assert np.all(y1[:, wM == 0.0] == asc.FILL)
    r1 = asc.gate(y1, exact, tol, "oracle corrected")
    print("correction %d x %d: oracle err/bound %.3f uncorrected, %.3f corrected" % (nrow, ncol, r0, r1))
    assert np.max(np.abs(y1 / y0 - 1.0)) > 1e-3                             # the matrix is not conservative: the factor is not 1


@pytest.mark.parametrize("nbatch", [2, 33])
def test_correction_batches_differ_in_every_batch_and_variable(nbatch):
    assert asc.IBH_MAX_BATCH == 32 and (nbatch > asc.IBH_MAX_BATCH) == (nbatch == 33)        # 33: two launches
    row, col, val, wM, Mw, nan_cols = asc.random_coo(4097, 900, 8, seed=4097)
    Xs = asc.batch_fields(asc.correction_fields(3, 900, nan_cols), nbatch)
    assert len(Xs) == nbatch and all(X.shape == (3, 900) for X in Xs)
    o = orc.Weighted.from_coo(4097, 900, row, col, val, wM, Mw, conservative=False)
    live = wM != 0.0
    factors = []
    for X in Xs:                                       # a factor of its own per (batch, variable): a mixed-up one misses the bound
        y0, y1 = (o.apply(X, fill=asc.FILL, force_conservation=fc) for fc in (False, True))
        factors += (y1[:, live][:, 0] / y0[:, live][:, 0]).tolist()
    f = np.sort(factors)
    assert np.min(np.diff(f) / f[1:]) > 1e-9, "two (batch, variable) factors closer than 1e-9"


def test_exact_correction_case_is_exact_in_any_order():
    m = asc.side_matrix(400, 1100, seed=77, exact=True)
    X = asc.exact_fields(3, m.ncol, seed=8)
    for a in (m.val, m.wM[m.wM != 0.0], m.Mw[:-1]):
        e = np.log2(a)
        assert np.all(e == np.round(e)) and e.min() >= -3 and e.max() <= 3
    assert m.Mw[-1] == 0.0
    assert np.all(X[:, :-1] == np.round(X[:, :-1])) and X[:, :-1].min() >= 1 and np.all(np.isnan(X[:, -1]))
    o = oracle_of(m, conservative=False)
    y0 = o.apply(X, fill=asc.FILL, force_conservation=False)
    for f in range(3):
        for r in (m.where["len1025"], m.where["len130"], m.where["len65"], m.where["len1"]):
            t = m.val[m.entries(r)] * X[f, m.colind[m.entries(r)]]
            assert asc.sequential_sum(t) == math.fsum(t) == asc.sequential_sum(t[::-1]) == y0[f, r]
    ref, tol = asc.product_ref(m, X)
    live = m.wM != 0.0
    assert np.array_equal(y0[:, live].astype(asc.LD), ref[:, live])         # every row: the long-double sum is the float64 one
    exact, _, factor = asc.correction_ref(y0, X, m.wM, m.Mw)
    for f in range(3):
        ta, tb = m.Mw[:-1] * X[f, :-1], m.wM[live] * y0[f, live]
        assert asc.sequential_sum(ta) == math.fsum(ta) and asc.sequential_sum(tb) == math.fsum(tb)
        assert factor[f] == math.fsum(ta) / math.fsum(tb) and factor[f] != 1.0
    y1 = o.apply(X, fill=asc.FILL, force_conservation=True)
    want = y0.copy()
    want[:, live] = y0[:, live] * factor[:, None]
    assert asc.same_bits(y1, want)
    assert np.all(y1[:, ~live] == asc.FILL)


# ---- E --------------------------------------------------------------------------------------------------------------------------------
def test_lpt_matrices_straddle_the_row_limit_with_ties():
    assert asc.LPT_MAX_ROWS == 8192
    for nrow in (8192, 8193, 1):
        m = asc.lpt_matrix(nrow, seed=nrow)
        assert m.nrow == nrow and m.ncol == 2000
        if nrow > 1:
            assert np.sum(m.cnt == 3) > 7000 and {0, 1, 2, 5, 65, 130, 1025} <= set(m.cnt.tolist())
            order = np.lexsort((np.arange(nrow), -m.cnt))                  # longest first, ties by index: a permutation
            assert order[0] == m.where["len1025"] and np.array_equal(np.sort(order), np.arange(nrow))
