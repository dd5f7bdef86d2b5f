"""The triplets -> CSR builder and the CSR algebra on the GPU, at their form edges (tests/csr_build_cases.py: the cases and the exact
restatement; tests/test_csr_build_cases.py pins both on the CPU).  Every test first asserts the form it is about from what the
library reports (ibh_selftest_triplets' info_out), then the bits: rowptr and colind equal as integers, val / wM / Mw equal as
uint64 views.  There is no tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import csr_build_cases as cbc
finally:
    sys.path.pop(0)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def ptr(a):
    return None if a is None or len(a) == 0 else a.ctypes.data_as(C.c_void_p)


def triplets(c, mode):
    """The case through ibh_selftest_triplets -> (the matrix handle, the forms that ran by name)."""
    from icebin_amd import linear_Weighted
    from icebin_amd._capi import check, lib
    h, info = C.c_void_p(), np.full(len(cbc.INFO), -1, np.int32)
    check(lib().ibh_selftest_triplets(c.nrow, c.ncol, c.n, ptr(c.row), ptr(c.col), ptr(c.val), mode, C.byref(h), info.ctypes.data))
    return linear_Weighted(h), dict(zip(cbc.INFO, info.tolist()))


_reference = {}


def reference(c):
    if c.name not in _reference:
        _reference[c.name] = cbc.reference(c)
    return _reference[c.name]


def same_csr(w, M, what):
    rp, ci, v = w.csr_dense()
    assert (w.nrow_d, w.ncol_d, w.nnz) == (M["nrow"], M["ncol"], len(M["val"])), what
    assert np.array_equal(rp, M["rowptr"]) and np.array_equal(ci, M["colind"]), (what, "structure")
    assert np.array_equal(bits(v), bits(M["val"])), (what, "values", np.flatnonzero(bits(v) != bits(M["val"]))[:8].tolist())


def run(c, mode):
    """Form first, then bits."""
    w, info = triplets(c, mode)
    for k, v in c.forms.get(mode, {}).items():
        assert info[k] == v, (c.name, mode, "form", k, "ran", info[k], "the case is about", v, info)
    assert info == cbc.predict(cbc.measure(c), mode), (c.name, mode, info)
    M, wM, Mw = reference(c)
    same_csr(w, M, (c.name, mode))
    assert np.array_equal(bits(w.wM), bits(wM)), (c.name, mode, "wM", np.flatnonzero(bits(w.wM) != bits(wM))[:8].tolist())
    assert np.array_equal(bits(w.Mw), bits(Mw)), (c.name, mode, "Mw", np.flatnonzero(bits(w.Mw) != bits(Mw))[:8].tolist())
    return w, info


def named(prefixes):
    return [c.name for c in cbc.cases() if c.name.startswith(prefixes)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", named("runs_"))
def test_run_lengths(name, mode):
    """Runs of 1, 2, 63, 64, 65, 127, 128, 129, 192 and 193 terms of one key, interleaved with the other keys in the input, one of
    them [-0.0, +0.0] and one all -0.0: alone (a wave per entry), among 127 single-term keys (a thread per entry), and at
    n == 8 * nnz and one below."""
    c = cbc.case(name)
    assert c.forms[mode]["seg"] in (cbc.WAVE, cbc.THREAD)
    w, info = run(c, mode)
    M = reference(c)[0]
    for (r, col), kind in c.special.items():
        e = M["rowptr"][r] + int(np.searchsorted(M["colind"][M["rowptr"][r]:M["rowptr"][r + 1]], col))
        got = bits(w.csr_dense()[2][e:e + 1])[0]
        assert got == (bits(-0.0)[0] if kind == cbc.NEG_ZEROS else bits(0.0)[0]), (name, kind)


@pytest.mark.parametrize("name", named("runs_"))
def test_run_lengths_through_from_coo(name):
    from icebin_amd import linear_Weighted
    c = cbc.case(name)
    w = linear_Weighted.from_coo((c.nrow, c.ncol), c.row, c.col, c.val, np.ones(c.nrow), np.ones(c.ncol))
    same_csr(w, reference(c)[0], name)


@pytest.mark.parametrize("name", named("order_"))
def test_order_forms(name):
    """The same triplets already sorted, disordered inside short pieces, in one piece of 8192 (sorted in LDS) and of 8193 (the radix
    sort): every key's emission order is kept, so the matrices are the same."""
    c = cbc.case(name)
    assert "order" in c.forms[0]
    run(c, 0)
    run(c, 1)           # (no local disorder expected: in order, or the radix sort)


def test_order_forms_give_one_matrix():
    def arrays(name):
        w, _ = triplets(cbc.case(name), 0)
        return [x.view(np.uint64) if x.dtype == np.float64 else x for x in w.csr_dense() + (w.wM, w.Mw)]
    first = arrays("order_sorted")
    for name in named("order_")[1:]:
        for x, y in zip(first, arrays(name)):
            assert np.array_equal(x, y), name


@pytest.mark.parametrize("name", named("optimistic_"))
def test_optimistic_row_sort(name):
    c = cbc.case(name)
    assert c.forms[1]["optimistic"] in (cbc.HELD, cbc.FAILED)
    run(c, 1)
    run(c, 0)


@pytest.mark.parametrize("name", named("srb_"))
def test_short_rows(name):
    """Per-row slots (mode 1): the longest row at 32 contributions and at 33, duplicate columns inside the rows, n == 8 * nrow and
    one more."""
    c = cbc.case(name)
    assert "short_rows" in c.forms[1]
    run(c, 1)
    run(c, 0)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", named(("extent_", "tall_", "empty_")))
def test_extents(name, mode):
    c = cbc.case(name)
    w, info = run(c, mode)
    if c.nrow >= 65535 and c.n and mode == 0:
        assert info["rowptr"] == (cbc.SEARCH if c.nrow < 65536 else cbc.HEADS_FILL)


@pytest.mark.parametrize("name", named(("wM_", "Mw_")))
def test_weights(name):
    c = cbc.case(name)
    assert set(c.forms[0]) & {"wM", "Mw"}
    w, info = run(c, 0)
    if name.startswith("wM_"):
        assert bits(w.wM[c.neg_zero_row:c.neg_zero_row + 1])[0] == bits(0.0)[0]           # a row of -0.0 alone sums to +0.0 from 0.0


# ---- the product -----------------------------------------------------------------------------------------------------------------
def to_weighted(M):
    from icebin_amd import linear_Weighted
    return linear_Weighted.from_csr((M["nrow"], M["ncol"]), M["rowptr"], M["colind"], M["val"], np.zeros(M["nrow"]), np.zeros(M["ncol"]))


@pytest.mark.parametrize("name", ["long", "edge", "edge_minus_1"])
def test_product(name):
    """total == 8 * n against 8 * n - 1 (64 lanes or one per row of L), an (r, c) reached by 65 and more terms, rows of R with 63,
    64, 65 and 129 entries under the 64-lane emit, an empty first and last row of L.  (The emit form is a pure function of the
    term count, asserted here from the operands; the library reports no form for the product.)"""
    from icebin_amd import linear_Weighted
    from icebin_amd._capi import check, lib
    L, R, lanes = cbc.product_cases()[name]
    assert (64 if cbc.product_total(L, R) >= 8 * L["nrow"] else 1) == lanes
    wl, wr = to_weighted(L), to_weighted(R)
    h = C.c_void_p()
    check(lib().ibh_selftest_csr_product(wl._h, wr._h, C.byref(h)))
    same_csr(linear_Weighted(h), cbc.product(L, R), name)


# ---- the algebra -------------------------------------------------------------------------------------------------------------------
def factors(rng, n):
    """Scale factors over sixteen decades, none of them zero."""
    return rng.standard_normal(n) * 10. ** rng.uniform(-8, 8, n)


def csr_op(op, M=None, idx=None, a=None, b=None, nout=0):
    from icebin_amd import linear_Weighted
    from icebin_amd._capi import check, lib
    idx = None if idx is None else np.ascontiguousarray(idx, np.int32)
    a = None if a is None else np.ascontiguousarray(a, np.float64)
    b = None if b is None else np.ascontiguousarray(b, np.float64)
    w = to_weighted(M) if M is not None else None
    h = C.c_void_p()
    code = cbc.OPS[op]
    vec = None
    if op == "expand_rows":
        vec = np.full(len(M["val"]), -7, np.int32)
    elif code >= cbc.OPS["recip"]:
        vec = np.full(nout, np.nan)
    n = lambda x: 0 if x is None else len(x)
    check(lib().ibh_selftest_csr_op(code, w._h if w else None, ptr(idx), n(idx), ptr(a), n(a), ptr(b), n(b), nout, C.byref(h),
                                    None if vec is None or len(vec) == 0 else vec.ctypes.data))
    return vec if vec is not None else linear_Weighted(h)


def test_crop_rows():
    """src with -1, a source row taken twice, rows of 0 / 1 / 63 / 64 / 65 / 129 entries, rs null and given, nout == 0, all -1."""
    M = cbc.algebra_matrix()
    rng = np.random.default_rng(1)
    rs = factors(rng, M["nrow"])
    src = np.asarray([5, -1, 0, 2, 3, 3, 4, -1, 7, 1, 11, 5, 6])
    assert {0, 1, 63, 64, 65, 129} <= set(np.diff(M["rowptr"])[src[src >= 0]].tolist())
    for s in (src, np.zeros(0, np.int32), np.full(5, -1)):
        for scale in (None, rs):
            same_csr(csr_op("crop_rows", M, idx=s, a=scale, nout=len(s)), cbc.crop_rows(M, s, scale), ("crop_rows", len(s), scale is not None))


def test_crop_cols():
    """Dropped columns, a map that reverses the order inside rows of 1 to 12 entries, a row dropped whole, and the four null / given
    combinations of rs / cs."""
    M = cbc.short_matrix()
    rng = np.random.default_rng(2)
    ncol_out = 50
    cmap = (ncol_out - 1 - np.arange(M["ncol"])).astype(np.int32)            # reversing: every row is re-sorted back to front
    cmap[::7] = -1
    whole = 9                                                                # row 9 loses every column
    cmap[M["colind"][M["rowptr"][whole]:M["rowptr"][whole + 1]]] = -1
    rs, cs = factors(rng, M["nrow"]), factors(rng, ncol_out)
    want = cbc.crop_cols(M, cmap, ncol_out)
    assert set(range(1, 13)) <= set(np.diff(M["rowptr"]).tolist()) and want["rowptr"][whole] == want["rowptr"][whole + 1]
    assert len(want["val"]) < len(M["val"]) and M["rowptr"][whole + 1] > M["rowptr"][whole]
    for r in (None, rs):
        for c in (None, cs):
            got = csr_op("crop_cols", M, idx=cmap, a=r, b=c, nout=ncol_out)
            same_csr(got, cbc.crop_cols(M, cmap, ncol_out, r, c), ("crop_cols", r is not None, c is not None))
    # the long rows as well (insertion over 129 entries), and a matrix without rows
    A = cbc.algebra_matrix()
    amap = rng.permutation(A["ncol"]).astype(np.int32)
    same_csr(csr_op("crop_cols", A, idx=amap, nout=A["ncol"]), cbc.crop_cols(A, amap, A["ncol"]), "crop_cols, long rows")


def test_transpose_and_expand_rows():
    """A matrix with empty rows and columns, and a 3 x 70 000 one (its transpose has 70 000 rows: the heads + fill row pointer)."""
    for M in (cbc.algebra_matrix(), cbc.wide_matrix()):
        T = cbc.transpose(M)
        assert np.any(np.diff(M["rowptr"]) == 0) and np.any(np.diff(T["rowptr"]) == 0)
        same_csr(csr_op("transpose", M), T, ("transpose", M["nrow"], M["ncol"]))
        assert np.array_equal(csr_op("expand_rows", M), cbc.rows_of(M))
    empty = cbc.matrix(4, 3, np.zeros(5), [], [])
    same_csr(csr_op("transpose", empty), cbc.transpose(empty), "transpose, no entries")
    assert len(csr_op("expand_rows", empty)) == 0


VECTOR_LENGTHS = (0, 1, 255, 256, 257)


@pytest.mark.parametrize("n", VECTOR_LENGTHS)
def test_vector_ops(n):
    rng = np.random.default_rng(3 + n)
    a, b = rng.standard_normal(n) * 10. ** rng.uniform(-8, 8, n), rng.standard_normal(n) * 10. ** rng.uniform(-8, 8, n)
    assert np.array_equal(bits(csr_op("recip", a=a, nout=n)), bits(1. / a))
    assert np.array_equal(bits(csr_op("mul", a=a, b=b, nout=n)), bits(a * b))
    src = rng.standard_normal(37)
    idx = rng.integers(0, 37, n)
    if n:
        idx[-1] = 36
    assert np.array_equal(bits(csr_op("gather", idx=idx, a=src, nout=n)), bits(src[idx]))


@pytest.mark.parametrize("nrow", VECTOR_LENGTHS)
def test_scalings(nrow):
    """diag(s) * M, M * diag(d) and diag(1 / sum) * M over 0, 1, 255, 256 and 257 rows (and as many columns)."""
    rng = np.random.default_rng(40 + nrow)
    lengths = [int(x) for x in rng.integers(0, min(nrow, 9) + 1, nrow)]
    if nrow:
        lengths[0], lengths[-1] = 0, min(nrow, 5)                            # (an empty first row where there are two; a last one with entries)
    M = cbc.random_matrix(rng, nrow, max(nrow, 1), lengths)
    assert len(M["val"]) > 0 or nrow == 0
    s, d = factors(rng, nrow), factors(rng, M["ncol"])
    same_csr(csr_op("scale_rows", M, a=s), cbc.scale_rows(M, s), "scale_rows")
    same_csr(csr_op("scale_cols", M, a=d), cbc.scale_cols(M, d), "scale_cols")
    same_csr(csr_op("scale_rows_recip", M, a=s), cbc.scale_rows_recip(M, s), "scale_rows_recip")


def test_scale_rows_recip_skips_empty_rows():
    """Rows without entries whose sum is 0: no inf or NaN appears, and every value is its own times one reciprocal."""
    M = cbc.algebra_matrix()
    wM, _ = cbc.weights(M)
    empty = np.diff(M["rowptr"]) == 0
    assert empty.sum() >= 2 and np.all(wM[empty] == 0.) and np.all(wM[~empty] != 0.)
    got = csr_op("scale_rows_recip", M, a=wM)
    same_csr(got, cbc.scale_rows_recip(M, wM), "scale_rows_recip")
    assert np.all(np.isfinite(got.csr_dense()[2]))


def test_csr_op_checks_lengths_against_the_matrix():
    from icebin_amd._capi import IBH_EINVAL, IcebinHipError
    M = cbc.short_matrix()
    one = np.ones(M["nrow"] + 1)
    twice = np.zeros(M["ncol"], np.int32)                                    # every column onto column 0
    for kw in (dict(op="crop_rows", idx=[0, M["nrow"]], nout=2), dict(op="crop_rows", idx=[0, 1], a=one, nout=2),
               dict(op="crop_cols", idx=[0, 1], nout=5), dict(op="crop_cols", idx=twice, nout=5), dict(op="scale_rows", a=one),
               dict(op="scale_cols", a=one[:3]), dict(op="scale_rows_recip", a=one), dict(op="transpose", a=one)):
        with pytest.raises(IcebinHipError) as e:
            csr_op(M=M, **kw)
        assert e.value.code == IBH_EINVAL, kw
