"""The composition of the I-row ModelE matrices alone (ibh_selftest_compose_cols; csrops.h: compose_cols): crop_cols(L) * R by
both forms -- 1 crop_cols + the generic product, 2 the row-local kernel -- against a plain-Python restatement, bit for bit, at the
row-local form's edges: rows of 0, 1, COMPOSE_LANES -1 / +0 / +1, 63 / 64 / 65, COMPOSE_ROWCAP and COMPOSE_ROWCAP + 1 kept entries
(the last declines to form 1), maps that keep, drop and reverse, an R with empty rows, with one output column and with a row of two
entries (declines), each scaling present and absent, a lone -0.0, sums that depend on their order, and empty operands."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LANES, ROWCAP = 32, 128             # COMPOSE_LANES, COMPOSE_ROWCAP (icebin_amd/csrc/csrops.h)
PRODUCT, ROWLOCAL = 1, 2


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def restate(L, mp, rs, cs, Rm):
    """Per entry (i, p, v) of L: k = map[p], dropped when k < 0; a term ((rs[i] * v) * cs[k]) * r for every entry (c, r) of row k
    of R, each factor optional, each product one IEEE operation; C(i, c) = its terms in ascending k, the first assigned."""
    out = []
    for i, row in enumerate(L):
        kept = []
        for p, v in row:
            k = int(mp[p])
            if k < 0:
                continue
            if rs is not None:
                v = float(rs[i]) * v
            if cs is not None:
                v = v * float(cs[k])
            kept.append((k, v))
        acc = {}
        for k, v in sorted(kept, key=lambda kv: kv[0]):
            for c, r in Rm[k]:
                t = v * r
                acc[c] = acc[c] + t if c in acc else t
        out.append(sorted(acc.items()))
    return out


def csr_arrays(M):
    rp = np.zeros(len(M) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in M])
    return rp, np.asarray([c for r in M for c, _ in r], np.int32), np.asarray([v for r in M for _, v in r], np.float64)


def to_weighted(M, ncol):
    from icebin_amd import linear_Weighted
    rp, ci, v = csr_arrays(M)
    return linear_Weighted.from_csr((len(M), ncol), rp, ci, v, np.zeros(len(M)), np.zeros(ncol))


def rows_of_lengths(rng, lengths, ncol):
    M = []
    for n in lengths:
        cols = np.sort(rng.choice(ncol, n, replace=False))
        M.append([(int(c), float(x)) for c, x in zip(cols, rng.uniform(-1., 1., n))])
    return M


def one_entry_rows(rng, nrow, ncol, empty_every=0):
    return [[] if empty_every and k % empty_every == 2 else [(int(rng.integers(ncol)), float(rng.uniform(0.5, 2.)))] for k in range(nrow)]


def run(L, nk, mp, rs, cs, Rm, nc, form, ncol_L=None):
    from icebin_amd import linear_Weighted
    from icebin_amd._capi import check, lib, ptr
    wl, wr = to_weighted(L, len(mp) if ncol_L is None else ncol_L), to_weighted(Rm, nc)
    assert len(Rm) == nk
    mp = np.ascontiguousarray(mp, np.int32)
    rs = None if rs is None else np.ascontiguousarray(rs, np.float64)
    cs = None if cs is None else np.ascontiguousarray(cs, np.float64)
    h = C.c_void_p()
    check(lib().ibh_selftest_compose_cols(wl._h, ptr(mp) if len(mp) else None, len(mp), None if rs is None else ptr(rs),
                                          None if cs is None else ptr(cs), wr._h, form, C.byref(h)))
    return linear_Weighted(h)


def check_both(L, mp, rs, cs, Rm, nc, served=True):
    """Both forms against the restatement; the row-local request reports 2 when it can serve and 1 when it declines."""
    want = restate(L, mp, rs, cs, Rm)
    rp, ci, v = csr_arrays(want)
    for form in (PRODUCT, ROWLOCAL):
        w = run(L, len(Rm), mp, rs, cs, Rm, nc, form)
        assert w.composed_by() == (ROWLOCAL if form == ROWLOCAL and served else PRODUCT), form
        wrp, wci, wv = w.csr_dense()
        assert (w.nrow_d, w.ncol_d) == (len(L), nc)
        assert np.array_equal(wrp, rp) and np.array_equal(wci, ci), form
        assert np.array_equal(bits(wv), bits(v)), (form, int(np.sum(bits(wv) != bits(v))), len(v))
    return want


LENGTHS = [0, 1, LANES - 1, LANES, LANES + 1, 63, 64, 65, ROWCAP, 2, 0, 7]
MAPS = ("keep", "drop_all", "drop_some", "reverse")


def make_map(kind, rng, np_, nk):
    """np_ columns of L into nk >= np_ rows of R, one-to-one."""
    if kind == "keep":
        return rng.permutation(nk)[:np_].astype(np.int32)
    if kind == "drop_all":
        return np.full(np_, -1, np.int32)
    if kind == "reverse":
        return (nk - 1 - np.arange(np_)).astype(np.int32)
    mp = rng.permutation(nk)[:np_].astype(np.int32)
    mp[rng.random(np_) < 0.3] = -1
    return mp


@pytest.mark.parametrize("scalings", ["rs_cs", "rs", "cs", "none"])
@pytest.mark.parametrize("kind", MAPS)
def test_row_lengths_maps_and_scalings(kind, scalings):
    rng = np.random.default_rng(100 + MAPS.index(kind))
    np_, nk, nc = ROWCAP + 20, ROWCAP + 40, 9
    L = rows_of_lengths(rng, LENGTHS * 2, np_)          # 24 rows: three workgroups of eight
    mp = make_map(kind, rng, np_, nk)
    Rm = one_entry_rows(rng, nk, nc)
    rs = rng.uniform(0.5, 2., len(L)) if "rs" in scalings else None
    cs = rng.uniform(0.5, 2., nk) if "cs" in scalings else None
    want = check_both(L, mp, rs, cs, Rm, nc)
    if kind in ("keep", "reverse"):
        assert max(len(r) for r in want) == nc and sum(len(r) for r in want) < sum(len(r) for r in L)    # equal columns were merged
        assert not want[0] and len(want[1]) == 1
    if kind == "drop_all":
        assert not any(want)


@pytest.mark.parametrize("kept", [ROWCAP, ROWCAP + 1])
def test_the_row_cap_counts_kept_entries(kept):
    """A row of ROWCAP + 1 entries of which the map drops one is served; with none dropped the row-local form declines, the
    generic product builds the matrix and the bits are the same."""
    rng = np.random.default_rng(7)
    np_, nc = ROWCAP + 1, 11
    L = rows_of_lengths(rng, [np_, 3, 0, np_], np_)
    mp = rng.permutation(np_).astype(np.int32)
    if kept == ROWCAP:
        mp[5] = -1
    Rm = one_entry_rows(rng, np_, nc)
    check_both(L, mp, rng.uniform(0.5, 2., len(L)), rng.uniform(0.5, 2., np_), Rm, nc, served=kept == ROWCAP)


@pytest.mark.parametrize("shape", ["empty_rows", "one_column", "two_entries", "two_entries_unreached"])
def test_shapes_of_R(shape):
    rng = np.random.default_rng(21)
    np_, nk, nc = 80, 90, 6
    L = rows_of_lengths(rng, [5, 0, 40, 64, 1, 80, 33, 12, 9], np_)
    mp = rng.permutation(nk)[:np_].astype(np.int32)
    served = True
    if shape == "empty_rows":
        Rm = one_entry_rows(rng, nk, nc, empty_every=3)
    elif shape == "one_column":
        Rm = [[(4, float(rng.uniform(0.5, 2.)))] for _ in range(nk)]
    else:
        Rm = one_entry_rows(rng, nk, nc)
        k = int(mp[3]) if shape == "two_entries" else int(np.setdiff1d(np.arange(nk), mp)[0])      # a row L reaches / does not reach
        Rm[k] = [(1, 0.75), (4, 1.5)]
        served = False
    want = check_both(L, mp, rng.uniform(0.5, 2., len(L)), rng.uniform(0.5, 2., nk), Rm, nc, served=served)
    if shape == "one_column":
        assert all(len(r) == (1 if l else 0) for r, l in zip(want, L))
    if shape == "empty_rows":
        assert sum(len(r) for r in want) > 0


def test_a_lone_negative_zero_and_sums_that_depend_on_their_order():
    """Row 0: one term, -0.0, which must stay -0.0 (the first term is assigned, not added to +0.0).  Row 1: three terms of one
    output column, 1, 1e16 and -1e16 by ascending k, whose sum is 0.0 in that order and 1.0 in the order of L's columns (the map
    reverses the columns, so the order of k is not the order of L).  Row 2: 2^-53, 2^-53 and 1 by ascending k give 1 + 2^-52, and
    1.0 in the order of L's columns."""
    L = [[(2, -0.0)], [(0, -1e16), (1, 1e16), (2, 1.0)], [(0, 1.0), (1, 2.0 ** -53), (2, 2.0 ** -53)]]
    mp = np.asarray([2, 1, 0], np.int32)
    Rm = [[(0, 1.0)], [(0, 1.0)], [(0, 1.0)]]
    want = check_both(L, mp, None, None, Rm, 1)
    assert np.signbit(want[0][0][1]) and want[0][0][1] == 0.0
    assert want[1][0][1] == 0.0 and want[2][0][1] == 1.0 + 2.0 ** -52


@pytest.mark.parametrize("shape", ["no_rows", "no_entries", "no_columns_of_R"])
def test_empty_operands(shape):
    rng = np.random.default_rng(3)
    if shape == "no_rows":
        L, np_ = [], 5
    elif shape == "no_entries":
        L, np_ = [[] for _ in range(10)], 5
    else:
        L, np_ = rows_of_lengths(rng, [3, 5], 5), 5
    nk = 6
    mp = rng.permutation(nk)[:np_].astype(np.int32)
    Rm = [[] for _ in range(nk)] if shape == "no_columns_of_R" else one_entry_rows(rng, nk, 4)
    want = check_both(L, mp, np.ones(len(L)), np.ones(nk), Rm, 4)
    assert not any(want)


def test_bad_arguments_are_refused():
    from icebin_amd import _capi
    rng = np.random.default_rng(5)
    L, Rm = rows_of_lengths(rng, [2, 3], 4), one_entry_rows(rng, 5, 3)
    good = np.asarray([0, 1, 2, 3], np.int32)
    for mp, form in ((good[:3], 2), (np.asarray([0, 1, 2, 5], np.int32), 2), (np.asarray([0, 1, 1, 3], np.int32), 2),
                     (np.asarray([0, -2, 1, 3], np.int32), 2), (good, 0), (good, 3)):
        with pytest.raises(_capi.IcebinHipError) as ei:
            run(L, 5, mp, None, None, Rm, 3, form, ncol_L=4)
        assert ei.value.code == _capi.IBH_EINVAL
