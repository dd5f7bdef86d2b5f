"""CPU-only: the cases of tests/csr_build_cases.py lie on the side of every selector they claim (measured here with numpy, no
library), the restatement there is the oracle (bit for bit against oracle.Weighted.from_coo and modele_restatement.product), and
the values can tell a wrong sum from the right one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import csr_build_cases as cbc
    import modele_restatement as mr
finally:
    sys.path.pop(0)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


_measured = {}


def measured(c):
    if c.name not in _measured:
        _measured[c.name] = cbc.measure(c)
    return _measured[c.name]


CASES = cbc.cases()


# ---- (a) the side of every selector ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_case_lies_where_it_claims(c):
    m = measured(c)
    assert c.forms and set(c.forms) <= {0, 1}, c.name
    for mode, claimed in c.forms.items():
        want = cbc.predict(m, mode)
        assert set(claimed) <= set(cbc.INFO)
        for k, v in claimed.items():
            assert want[k] == v, (c.name, mode, k, "claimed", v, "the selectors give", want[k])
    for sel, v in c.at.items():
        where, what, a, b = cbc.SELECTORS[sel]
        assert m[what] == v and v in (a, b), (c.name, sel, what, m[what], v)
    assert np.all((c.row >= 0) & (c.row < max(c.nrow, 1))) and np.all((c.col >= 0) & (c.col < max(c.ncol, 1)))


def test_every_selector_has_a_case_on_each_side():
    seen = {s: set() for s in cbc.SELECTORS}
    for c in CASES:
        for sel, v in c.at.items():
            seen[sel].add(v)
    for p in cbc.product_cases().values():
        seen["prod_emit"].add(cbc.product_total(p[0], p[1]) - 8 * p[0]["nrow"])
    for sel, (where, what, a, b) in cbc.SELECTORS.items():
        assert {a, b} <= seen[sel], (sel, where, "no case at", {a, b} - seen[sel])


def test_run_length_matrix_is_the_one_asked_for():
    m = measured(cbc.case("runs_alone"))
    assert (m["n"], m["nnz"]) == (964, 10) and m["runs"] == set(cbc.RUN_LENGTHS)
    m = measured(cbc.case("runs_thread"))
    assert m["nnz"] - 10 >= 127 and set(cbc.RUN_LENGTHS) <= m["runs"] and m["n"] < 8 * m["nnz"]
    assert measured(cbc.case("runs_8nnz"))["n_minus_8nnz"] == 0 and measured(cbc.case("runs_8nnz_minus_1"))["n_minus_8nnz"] == -1
    for name in ("runs_alone", "runs_thread", "runs_8nnz", "runs_8nnz_minus_1"):
        c = cbc.case(name)
        # the terms of a key are interleaved with other keys: no long run is contiguous in the input
        key = (c.row.astype(np.int64) << 32) | c.col
        longest_block = max(len(list(g)) for g in np.split(key, np.flatnonzero(key[1:] != key[:-1]) + 1))
        assert longest_block < 20, (name, longest_block)
        assert sorted(c.special.values()) == sorted([cbc.NEG_ZEROS, cbc.ZERO_PAIR])


def test_order_cases_hold_the_same_triplets():
    names = ["order_sorted", "order_short_pieces", "order_%d" % cbc.CS_BIG, "order_%d" % (cbc.CS_BIG + 1)]
    first = cbc.case(names[0])
    assert first.n == 9000 and measured(first)["nnz"] == 3000
    o0 = cbc.runs_of(first.row, first.col)[0]
    for name in names[1:]:
        c = cbc.case(name)
        o = cbc.runs_of(c.row, c.col)[0]          # the stable order by key: the same terms, every key's in the same emission order
        assert np.array_equal(c.row[o], first.row[o0]) and np.array_equal(c.col[o], first.col[o0])
        assert np.array_equal(bits(c.val[o]), bits(first.val[o0])), name
    assert measured(cbc.case("order_short_pieces"))["maxpiece"] <= 37 and measured(cbc.case("order_sorted"))["maxpiece"] == 1
    assert measured(cbc.case(names[2]))["maxpiece"] == cbc.CS_BIG and measured(cbc.case(names[3]))["maxpiece"] == cbc.CS_BIG + 1


def test_weight_and_extent_cases_hold_what_the_issue_lists():
    for name in ("wM_wave", "wM_thread", "wM_8nrow", "wM_8nrow_minus_1"):
        c = cbc.case(name)
        m = measured(c)
        assert set(cbc.ROW_LENGTHS) <= m["row_lengths"] and m["n"] == m["nnz"], name
        M, wM, Mw = cbc.reference(c)
        r = c.neg_zero_row
        rowvals = M["val"][M["rowptr"][r]:M["rowptr"][r + 1]]
        assert len(rowvals) >= 1 and np.all(bits(rowvals) == bits(-0.0)) and bits(wM[r:r + 1])[0] == bits(0.0)
    for name in ("Mw_slots_4ncol", "Mw_sort_4ncol_plus_1", "Mw_sort_wave", "Mw_slots_wide"):
        m = measured(cbc.case(name))
        assert set(cbc.COL_LENGTHS) <= m["col_lengths"] and m["n"] == m["nnz"], name
    assert measured(cbc.case("Mw_slots_wide"))["ncol"] >= 65536
    for nrow in (65535, 65536):
        c = cbc.case("tall_%d_gaps" % nrow)
        rows = np.unique(c.row)
        assert rows[0] >= 1000 and rows[-1] < 60000 and np.diff(rows).max() > 256 and 2000 <= c.n <= 5000
        assert set(cbc.case("tall_%d_first_row" % nrow).row.tolist()) == {0}
        assert set(cbc.case("tall_%d_last_row" % nrow).row.tolist()) == {nrow - 1}
        assert cbc.case("tall_%d_empty" % nrow).n == 0
        assert int(cbc.case("tall_%d_dense" % nrow).row.max()) == nrow - 1
    for nrow, ncol in ((1, 1), (1, 300), (300, 1), (256, 256), (257, 257), (3, 65536)):
        c = cbc.case("extent_%dx%d" % (nrow, ncol))
        assert np.any((c.row == nrow - 1) & (c.col == ncol - 1)), c.name
    for name, longest in (("srb_taken_32", 32), ("srb_declined_33", 33)):
        c = cbc.case(name)
        m = measured(c)
        assert m["maxrow_contrib"] == longest and m["n"] > m["nnz"] and 0 in m["row_lengths"]     # duplicates inside the rows


# ---- (b) the restatement is the oracle ---------------------------------------------------------------------------------------------------
FROM_COO_SHAPED = [c for c in CASES if c.nrow and c.ncol]


@pytest.mark.parametrize("c", FROM_COO_SHAPED, ids=[c.name for c in FROM_COO_SHAPED])
def test_restatement_equals_the_oracle_from_coo(c):
    from oracle import oracle as orc
    M = cbc.from_triplets(c.nrow, c.ncol, c.row, c.col, c.val)
    o = orc.Weighted.from_coo(c.nrow, c.ncol, c.row, c.col, c.val, np.ones(c.nrow), np.ones(c.ncol))
    assert o.nnz == len(M["val"])
    assert np.array_equal(o.row, cbc.rows_of(M)) and np.array_equal(o.col, M["colind"])
    assert np.array_equal(bits(o.val), bits(M["val"])), (c.name, int(np.sum(bits(o.val) != bits(M["val"]))))


def as_rows(M):
    return [[(int(c), float(x)) for c, x in zip(M["colind"][b:e], M["val"][b:e])] for b, e in zip(M["rowptr"][:-1], M["rowptr"][1:])]


@pytest.mark.parametrize("name", sorted(cbc.product_cases()))
def test_restatement_equals_the_modele_product(name):
    L, R, lanes = cbc.product_cases()[name]
    want = mr.product(as_rows(L), as_rows(R))
    rp, ci, v = mr.csr(dict(M=want))
    P = cbc.product(L, R)
    assert np.array_equal(P["rowptr"], rp) and np.array_equal(P["colind"], ci) and np.array_equal(bits(P["val"]), bits(v))
    total = cbc.product_total(L, R)
    assert (64 if total >= 8 * L["nrow"] else 1) == lanes
    if name == "long":
        row, col, term = cbc.product_terms(L, R)
        order, ks, starts, ends = cbc.runs_of(row, col)
        assert (ends - starts).max() >= 65                                  # an (r, c) reached by 65 or more terms
        assert {63, 64, 65, 129} <= set(np.diff(R["rowptr"]).tolist())
        assert L["rowptr"][1] == 0 and L["rowptr"][-1] == L["rowptr"][-2]      # an empty first and an empty last row of L
        for b, e in zip(starts, ends):
            assert cbc.is_sensitive(term[order[b:e]]), (int(b), int(e))


def test_restatement_transpose_and_weights_against_the_modele_restatement():
    M = cbc.algebra_matrix()
    T = mr.transpose(as_rows(M), M["ncol"])
    rp, ci, v = mr.csr(dict(M=T))
    mine = cbc.transpose(M)
    assert np.array_equal(mine["rowptr"], rp) and np.array_equal(mine["colind"], ci) and np.array_equal(bits(mine["val"]), bits(v))
    rs, cs = mr.sums(as_rows(M), M["ncol"])
    wM, Mw = cbc.weights(M)
    assert np.array_equal(bits(wM), bits(rs)) and np.array_equal(bits(Mw), bits(cs))


# ---- (c) the inputs can tell a wrong kernel from a right one --------------------------------------------------------------------------------
def groups_by(labels_major, labels_minor, val):
    order = np.lexsort((labels_minor, labels_major))
    lab = np.asarray(labels_major)[order]
    cuts = np.flatnonzero(lab[1:] != lab[:-1]) + 1
    return [g.tolist() for g in np.split(np.asarray(val)[order], cuts)] if len(lab) else []


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_values_are_sensitive(c):
    order, ks, starts, ends = cbc.runs_of(c.row, c.col)
    v = c.val[order]
    nspecial = 0
    for b, e in zip(starts.tolist(), ends.tolist()):
        run = v[b:e].tolist()
        key = (int(ks[b] >> 32), int(ks[b] & 0xffffffff))
        right = cbc.sum_assigned(run)
        if c.special.get(key) == cbc.NEG_ZEROS:
            # a run of two or more that opens with -0.0: started at 0.0 the sum is +0.0, assigned it stays -0.0
            assert len(run) >= 2 and bits(right) == bits(-0.0) and bits(cbc.sum_from_zero(run)) == bits(0.0)
            assert bits(cbc.chunked64(run, False)) != bits(right)
            nspecial += 1
        elif c.special.get(key) == cbc.ZERO_PAIR:
            assert bits(np.asarray(run)).tolist() == bits(np.asarray([-0.0, 0.0])).tolist()
            assert bits(right) == bits(0.0) and bits(run[0]) != bits(right)           # the first term alone is not the sum
            nspecial += 1
        elif len(run) >= 3:
            wrong = cbc.wrong_sums(run, True)
            assert (len(run) <= 65 or "chunked64" in wrong) and (len(run) <= 64 or "swap_63_64" in wrong)
            for how, w in wrong.items():
                assert bits(w) != bits(right), (c.name, key, len(run), how)
    assert nspecial == len(c.special)
    if c.weight_groups:
        M = cbc.from_triplets(c.nrow, c.ncol, c.row, c.col, c.val)
        rows = cbc.rows_of(M)
        major, minor = (rows, M["colind"]) if c.weight_groups == "rows" else (M["colind"], rows)
        checked = 0
        for g in groups_by(major, minor, M["val"]):
            if len(g) >= 3 and not all(bits(x) == bits(-0.0) for x in g):
                right = cbc.sum_from_zero(g)
                for how, w in cbc.wrong_sums(g, False).items():
                    assert bits(w) != bits(right), (c.name, len(g), how)
                checked += 1
        assert checked >= 4


def test_a_wrong_restatement_would_be_caught():
    # the conditions above in action: three wrong builders differ from the right one on the run-length matrix
    c = cbc.case("runs_alone")
    right = cbc.from_triplets(c.nrow, c.ncol, c.row, c.col, c.val)["val"]
    order, ks, starts, ends = cbc.runs_of(c.row, c.col)
    v = c.val[order].tolist()
    from_zero = np.asarray([cbc.sum_from_zero(v[b:e]) for b, e in zip(starts, ends)])
    unstable = np.asarray([cbc.sum_assigned(v[b:e][::-1]) for b, e in zip(starts, ends)])
    chunked = np.asarray([cbc.chunked64(v[b:e], True) for b, e in zip(starts, ends)])
    lengths = (ends - starts)
    drawn = np.asarray([(int(k >> 32), int(k & 0xffffffff)) not in c.special for k in ks[starts]])
    assert np.count_nonzero(bits(from_zero) != bits(right)) == 1                    # only the run of negative zeros sees the start
    assert np.array_equal(bits(unstable) != bits(right), (lengths >= 3) & drawn)
    assert np.array_equal(bits(chunked) != bits(right), (lengths > 65) & drawn)         # (65: the second chunk is one term)
