"""Hntr's matrix forms on the GPU (ibh_hntr_triplets / ibh_hntr_matrix_d) against an exact numpy restatement of
Hntr::matrix with OverlapMatAccum / ScaledRegridMatAccum (hntr.hpp:205-338), MakeDenseEigenT and setFromTriplets: indices
and value bit patterns equal, wM / Mw bitwise, dims equal; then the reference's own invariants (test_hntr.cpp:310-380) and
the applies against Hntr::regrid."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hntr import GRIDS, PAIRS  # noqa: E402
from test_hntr_matrix import dxyp_restated  # noqa: E402

R_EARTH = 6371000.


def spec(name):
    from icebin_amd import HntrSpec
    return HntrSpec(*GRIDS[name]) if isinstance(name, str) else HntrSpec(*name)


def triplets_ref(Bspec, Aspec, kind, eq_rad, mask=None):
    """Stream order: JB, IB ascending (skipping excluded cells); JA outer, IAREV inner.  WEIGHT by a sequential sum."""
    from icebin_amd.hntr import partition
    P = partition(Bspec, Aspec)
    imA, imB = Aspec.im, Bspec.im
    dx = dxyp_restated(Bspec.im, Bspec.jm)
    R2 = eq_rad * eq_rad
    out_b, out_a, out_v = [], [], []
    for JB in range(1, Bspec.jm + 1):
        jmn, jmx = int(P["JMIN"][JB - 1]), int(P["JMAX"][JB - 1])
        JA = np.arange(jmn, jmx + 1)
        G = P["SINA"][JA] - P["SINA"][JA - 1]
        G[0] -= P["GMIN"][JB - 1]
        G[-1] -= P["GMAX"][JB - 1]
        area = R2 * dx[JB - 1]
        for IB in range(1, imB + 1):
            IJB = IB + imB * (JB - 1)
            if mask is not None and not mask[IJB - 1]:
                continue
            imn, imx = int(P["IMIN"][IB - 1]), int(P["IMAX"][IB - 1])
            IAREV = np.arange(imn, imx + 1)
            F = np.ones(len(IAREV))
            F[0] -= P["FMIN"][IB - 1]
            F[-1] -= P["FMAX"][IB - 1]
            FG = (F[None, :] * G[:, None]).reshape(-1)
            WEIGHT = np.add.accumulate(np.concatenate([[0.], FG]))[-1]
            v = FG * (1. / WEIGHT)
            if kind == "overlap":
                v = v * area
            IA = 1 + (IAREV - 1) % imA
            out_b.append(np.full(len(FG), IJB - 1, np.int64))
            out_a.append(((IA[None, :] + imA * (JA[:, None] - 1)) - 1).reshape(-1))
            out_v.append(v)
    cat = lambda x, t: np.concatenate(x).astype(t) if x else np.zeros(0, t)   # noqa: E731
    return cat(out_b, np.int64), cat(out_a, np.int64), cat(out_v, np.float64)


def seq_sums(keys, val, n):
    """sum from 0 in the given (already ordered) sequence per key, one rounded add at a time."""
    order = np.argsort(keys, kind="stable")
    k, v = keys[order], val[order]
    cnt = np.bincount(k, minlength=n)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    s = np.zeros(n)
    for j in range(int(cnt.max()) if len(cnt) and cnt.size else 0):
        live = cnt > j
        s[live] = s[live] + v[start[live] + j]
    return s


def dense_ref(iB, iA, val, nB, nA, dims, transforms, transpose):
    """MakeDenseEigenT + setFromTriplets + the column-major sums.  dims: two lists (dense -> sparse), appended to.  An entry's
    indices are transformed in order (B, then A) and the entry stops at the first one TO_DENSE_IGNORE_MISSING drops."""
    dmaps = [{s: d for d, s in enumerate(dims[0])}, {s: d for d, s in enumerate(dims[1])}]
    keep, rows, cols = [], [], []
    for p, (b, a) in enumerate(zip(iB.tolist(), iA.tolist())):
        ids = []
        for k, key in ((0, b), (1, a)):
            d = dmaps[k].get(key, -1)
            if d < 0 and transforms[k] == 0:
                d = len(dims[k]); dims[k].append(key); dmaps[k][key] = d
            if d < 0 and transforms[k] == 1:
                raise KeyError(key)
            ids.append(d)
            if d < 0:
                break
        if len(ids) == 2 and ids[0] >= 0 and ids[1] >= 0:
            keep.append(p); rows.append(ids[0]); cols.append(ids[1])
    r, c, v = np.array(rows, np.int64), np.array(cols, np.int64), val[np.array(keep, np.int64)]
    if transpose:
        r, c = c, r
    nrow, ncol = (len(dims[1]), len(dims[0])) if transpose else (len(dims[0]), len(dims[1]))
    order = np.lexsort((c, r))          # stable: duplicates stay in input order
    r, c, v = r[order], c[order], v[order]
    head = np.ones(len(r), bool)
    head[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    ur, uc, uv = r[head], c[head], v[head].copy()
    gid = np.cumsum(head) - 1
    for p in np.nonzero(~head)[0]:
        uv[gid[p]] = uv[gid[p]] + v[p]
    wM = seq_sums(ur, uv, nrow)
    Mw = seq_sums(uc, uv, ncol)     # ur ascends inside each column after the stable sort by column
    return ur, uc, uv, wM, Mw


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def check_matrix(w, ref, dims_ref=None):
    ur, uc, uv, wM, Mw = ref
    r, c, v = w.coo_dense()
    assert np.array_equal(r, ur) and np.array_equal(c, uc)
    assert np.array_equal(bits(v), bits(uv))
    assert np.array_equal(bits(w.wM), bits(wM))
    assert np.array_equal(bits(w.Mw), bits(Mw))
    if dims_ref is not None:
        assert np.array_equal(w.dim(0), dims_ref[0]) and np.array_equal(w.dim(1), dims_ref[1])


def hntr(b, a):
    from icebin_amd import Hntr
    return Hntr(17.17, spec(b), spec(a))


ALL_PAIRS = PAIRS + [(a, b) for b, a in PAIRS]


@pytest.mark.parametrize("b,a", ALL_PAIRS, ids=lambda x: x)
def test_triplets_bitwise(b, a):
    h = hntr(b, a)
    for kind, R in (("overlap", 1.), ("overlap", R_EARTH), ("scaled", 1.)):
        got = h.triplets(kind, R)
        ref = triplets_ref(spec(b), spec(a), kind, R)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        assert np.array_equal(bits(got[2]), bits(ref[2])), (kind, R)
    iB, iA, v = h.overlap(R_EARTH)
    assert np.array_equal(bits(v), bits(triplets_ref(spec(b), spec(a), "overlap", R_EARTH)[2]))
    assert np.array_equal(bits(h.scaled_regrid_matrix()[2]), bits(triplets_ref(spec(b), spec(a), "scaled", 1.)[2]))


def test_triplets_bitwise_from_2_minutes():
    from icebin_amd import Hntr, HntrSpec
    A, B = HntrSpec(10800, 5400, 0., 2.), HntrSpec(72, 36, 0., 300.)
    m = (np.arange(B.size) // B.im) % 6 == 1          # every sixth row of B cells: 9.7 M entries
    got = Hntr(17.17, B, A).overlap(R_EARTH, m)
    ref = triplets_ref(B, A, "overlap", R_EARTH, m)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert np.array_equal(bits(got[2]), bits(ref[2]))


def test_includeB_masks():
    b, a = "72x46_east", "360x180"
    h = hntr(b, a)
    nB = spec(b).size
    m = np.random.default_rng(5).random(nB) < 0.4
    for kind in ("overlap", "scaled"):
        got = h.triplets(kind, R_EARTH, m)
        ref = triplets_ref(spec(b), spec(a), kind, R_EARTH, m)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(bits(got[2]), bits(ref[2]))
        w = h.matrix_d(kind, R_EARTH, includeB=m)
        check_matrix(w, dense_ref(*ref, nB, spec(a).size, [list(range(nB)), list(range(spec(a).size))], (0, 0), False))
    # all false: a valid empty matrix
    w = h.matrix_d("overlap", includeB=np.zeros(nB, bool))
    assert w.nnz == 0 and (w.nrow_d, w.ncol_d) == (nB, spec(a).size)
    assert not w.wM.any() and not w.Mw.any()
    assert len(h.overlap(1., np.zeros(nB, bool))[0]) == 0
    # all true == NULL
    w1, w2 = h.matrix_d("scaled", includeB=np.ones(nB, bool)), h.matrix_d("scaled")
    for x, y in zip(w1.coo_dense() + (w1.wM, w1.Mw), w2.coo_dense() + (w2.wM, w2.Mw)):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


@pytest.mark.parametrize("b,a", ALL_PAIRS, ids=lambda x: x)
def test_matrix_d_null_dims_bitwise(b, a):
    h = hntr(b, a)
    nB, nA = spec(b).size, spec(a).size
    for kind in ("overlap", "scaled"):
        w = h.matrix_d(kind, R_EARTH)
        assert w.conservative and w.scaled == (kind == "scaled")
        ref = dense_ref(*triplets_ref(spec(b), spec(a), kind, R_EARTH), nB, nA, [list(range(nB)), list(range(nA))], (0, 0), False)
        check_matrix(w, ref, (np.arange(nB), np.arange(nA)))


def make_set(kind, n, rng):
    from icebin_amd import SparseSet
    if kind == "empty":
        return SparseSet(), []
    if kind == "pre":           # a pre-populated set holding some of the keys, in ascending order
        keys = np.sort(rng.choice(n, n // 2, replace=False))
    else:                       # permuted: every key, shuffled
        keys = rng.permutation(n)
    return SparseSet(n, keys), keys.tolist()


@pytest.mark.parametrize("transpose", [False, True])
def test_matrix_d_transforms_and_sets(transpose):
    from icebin_amd import IcebinHipError
    b, a = "72x46_east", "144x90_east"
    h = hntr(b, a)
    nB, nA = spec(b).size, spec(a).size
    trip = triplets_ref(spec(b), spec(a), "overlap", R_EARTH)
    rng = np.random.default_rng(11)
    for tB in (0, 1, 2):
        for tA in (0, 1, 2):
            for sB in ("empty", "pre", "perm"):
                for sA in ("empty", "pre", "perm"):
                    dB, lB = make_set(sB, nB, rng)
                    dA, lA = make_set(sA, nA, rng)
                    try:
                        ref = dense_ref(*trip, nB, nA, [list(lB), list(lA)], (tB, tA), transpose)
                        ref_dims = None
                    except KeyError:
                        with pytest.raises(IcebinHipError) as e:
                            h.matrix_d("overlap", R_EARTH, dims=(dB, dA), transforms=(tB, tA), transpose=transpose)
                        assert e.value.code == -1
                        assert np.array_equal(dB.to_sparse(), lB) and np.array_equal(dA.to_sparse(), lA), "sets changed on error"
                        continue
                    ref_l = [list(lB), list(lA)]
                    ref = dense_ref(*trip, nB, nA, ref_l, (tB, tA), transpose)
                    w = h.matrix_d("overlap", R_EARTH, dims=(dB, dA), transforms=(tB, tA), transpose=transpose)
                    ref_dims = (ref_l[1], ref_l[0]) if transpose else (ref_l[0], ref_l[1])
                    check_matrix(w, ref, ref_dims)
                    assert np.array_equal(dB.to_sparse(), ref_l[0]) and np.array_equal(dA.to_sparse(), ref_l[1])
                    assert dB.sparse_extent() == nB and dA.sparse_extent() == nA


@pytest.mark.parametrize("transpose", [False, True])
def test_failed_matrix_d_leaves_both_sets_alone(transpose):
    """A key missing from a TO_DENSE set is found after dimA's ADD_DENSE numbering was prepared and before either set adopts
    anything: both sets keep their entries and their unset (-1) sparse extent."""
    from icebin_amd import IcebinHipError, SparseSet
    from icebin_amd.hntr import ADD_DENSE, TO_DENSE
    h = hntr("8x4", "16x8")
    dimB, dimA = SparseSet(-1, [3, 17]), SparseSet(-1, [5])
    with pytest.raises(IcebinHipError, match="missing from a TO_DENSE set") as e:
        h.matrix_d("overlap", R_EARTH, dims=(dimB, dimA), transforms=(TO_DENSE, ADD_DENSE), transpose=transpose)
    assert e.value.code == -1       # IBH_EINVAL
    assert np.array_equal(dimB.to_sparse(), [3, 17]) and np.array_equal(dimA.to_sparse(), [5])
    assert dimB.sparse_extent() == -1 and dimA.sparse_extent() == -1


def test_ignore_missing_b_stops_the_entry():
    """B dropped by TO_DENSE_IGNORE_MISSING: the entry's A index is neither numbered (ADD_DENSE) nor looked up (TO_DENSE)."""
    from icebin_amd import SparseSet
    b, a = "72x46_east", "144x90_east"
    h = hntr(b, a)
    nB, nA = spec(b).size, spec(a).size
    keepB = np.arange(0, nB, 5)
    w = h.matrix_d("scaled", dims=(SparseSet(nB, keepB), SparseSet()), transforms=(2, 0))
    trip = triplets_ref(spec(b), spec(a), "scaled", 1.)
    usedA = trip[1][np.isin(trip[0], keepB)]
    _, first = np.unique(usedA, return_index=True)
    assert np.array_equal(w.dim(1), usedA[np.sort(first)])
    # A holds only the keys of the kept B cells: TO_DENSE on A succeeds
    w2 = h.matrix_d("scaled", dims=(SparseSet(nB, keepB), SparseSet(nA, w.dim(1))), transforms=(2, 1))
    assert w2.nnz == w.nnz


def test_one_set_grown_and_read_every_way():
    """One SparseSet through every way it is grown and read: looked up on the device (which builds and caches its device
    sparse -> dense table), grown on the device, grown on the host, looked up on the device again.  The last lookup must
    see the host's key at dense id dense_extent - 1."""
    from icebin_amd import SparseSet
    b, a = "72x46_east", "144x90_east"
    h = hntr(b, a)
    nB, nA = spec(b).size, spec(a).size
    trip = triplets_ref(spec(b), spec(a), "overlap", R_EARTH)
    keys = sorted(np.random.default_rng(23).choice(nA, nA // 4, replace=False).tolist())
    S, L = SparseSet(nA, keys), list(keys)

    def build(includeB, tA):
        t = trip if includeB is None else triplets_ref(spec(b), spec(a), "overlap", R_EARTH, includeB)
        ref_l = [[], L]
        ref = dense_ref(*t, nB, nA, ref_l, (0, tA), False)          # appends to L under ADD_DENSE
        w = h.matrix_d("overlap", R_EARTH, includeB=includeB, dims=(SparseSet(), S), transforms=(0, tA))
        check_matrix(w, ref, (ref_l[0], L))
        assert np.array_equal(S.to_sparse(), L) and S.dense_extent() == len(L)
        return w

    build(None, 2)                                  # 1. TO_DENSE_IGNORE_MISSING on the pre-populated set
    south = np.arange(nB) < nB // 2
    n1 = len(L)
    build(south, 0)                                 # 2. ADD_DENSE on the device, the southern half of B only
    assert len(L) > n1
    have = set(L)
    k = next(int(x) for x in trip[1] if int(x) not in have)         # an A cell only the northern half reaches
    assert S.add_dense(k) == len(L)                 # 3. on the host
    L.append(k)
    assert np.array_equal(S.to_sparse(), L)
    w = build(None, 2)                              # 4. TO_DENSE_IGNORE_MISSING again: entries of k land in the last column
    _, c, _ = w.coo_dense()
    assert np.any(c == S.dense_extent() - 1)


@pytest.mark.parametrize("transpose", [False, True])
def test_caller_owned_identity_sets(transpose):
    """SparseSet.identity(n) over the whole grid, passed in: the in-place build (no transpose) or the general one; the
    result is the NULL-dims matrix and the sets keep their identity."""
    from icebin_amd import SparseSet
    b, a = "144x90_east", "288x180"
    h = hntr(b, a)
    nB, nA = spec(b).size, spec(a).size
    for tB, tA in ((0, 0), (1, 1), (2, 0)):
        dB, dA = SparseSet.identity(nB), SparseSet.identity(nA)
        w = h.matrix_d("overlap", R_EARTH, dims=(dB, dA), transforms=(tB, tA), transpose=transpose)
        ref = dense_ref(*triplets_ref(spec(b), spec(a), "overlap", R_EARTH), nB, nA, [list(range(nB)), list(range(nA))],
                        (0, 0), transpose)
        check_matrix(w, ref, (np.arange(nA), np.arange(nB)) if transpose else (np.arange(nB), np.arange(nA)))
        assert dB.sparse_extent() == nB and dA.sparse_extent() == nA
        assert np.array_equal(dB.to_sparse(), np.arange(nB)) and np.array_equal(dA.to_sparse(), np.arange(nA))


def test_modele_shape():
    """compute_AOmvAAm: B = 1 deg ocean clipped to a pre-populated dimAOm (TO_DENSE_IGNORE_MISSING), A = 2x2.5 deg
    (ADD_DENSE), transposed; DimClip(&dimAOm) as the includeB mask."""
    from icebin_amd import Hntr, HntrSpec, SparseSet
    B, A = HntrSpec(360, 180, 0., 60.), HntrSpec(144, 90, 0., 120.)
    rng = np.random.default_rng(3)
    ocean = np.nonzero(rng.random(B.size) < 0.7)[0]
    dimAOm, dimAAm = SparseSet(B.size, ocean), SparseSet()
    clip = np.zeros(B.size, bool)
    clip[ocean] = True
    h = Hntr(17.17, B, A)
    w = h.matrix_d("overlap", R_EARTH, includeB=clip, dims=(dimAOm, dimAAm), transforms=(2, 0), transpose=True)
    dims = [ocean.tolist(), []]
    ref = dense_ref(*triplets_ref(B, A, "overlap", R_EARTH, clip), B.size, A.size, dims, (2, 0), True)
    check_matrix(w, ref, (dims[1], dims[0]))
    w2 = h.matrix_d("overlap", R_EARTH, includeB=clip, dims=(SparseSet(B.size, ocean), SparseSet()), transforms=(2, 0),
                    transpose=True)
    for x, y in zip(w.coo_dense() + (w.wM, w.Mw), w2.coo_dense() + (w2.wM, w2.Mw)):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), "two builds differ"


@pytest.mark.parametrize("B,A", [((1, 4, 0.3, 2700.), (8, 4, 0., 2700.)), ((1, 2, 0.3, 5400.), (16, 8, 0.25, 1350.)),
                                 ((3, 4, 0.5, 2700.), (8, 4, 0., 2700.))], ids=str)
def test_duplicate_columns(B, A):
    """imB = 1 with an offset: the window is one cell wider than imA and visits one A column twice."""
    from icebin_amd.hntr import partition
    Bs, As = spec(B), spec(A)
    P = partition(Bs, As)
    if B[0] == 1:
        assert P["IMAX"][0] - P["IMIN"][0] + 1 > A[0]
    h = hntr(B, A)
    for kind in ("overlap", "scaled"):
        trip = triplets_ref(Bs, As, kind, R_EARTH)
        got = h.triplets(kind, R_EARTH)
        assert np.array_equal(got[1], trip[1]) and np.array_equal(bits(got[2]), bits(trip[2]))
        for transpose in (False, True):
            w = h.matrix_d(kind, R_EARTH, transpose=transpose)
            check_matrix(w, dense_ref(*trip, Bs.size, As.size, [list(range(Bs.size)), list(range(As.size))], (0, 0), transpose))


# global grids of uniform rows and even jm: make_dxyp takes jm/2 in integer division, so odd jm (91x45) shifts its rows
UNIFORM = ["4x2", "8x4", "16x8", "144x90", "288x180", "360x180", "100x50"]


@pytest.mark.parametrize("b,a", [(b, a) for b, a in ALL_PAIRS if b in UNIFORM and a in UNIFORM], ids=lambda x: x)
def test_reference_invariants(b, a):
    """test_hntr.cpp:310-380: row sums of the overlap are R^2 dxyp(jB), column sums R^2 dxyp(jA)."""
    h = hntr(b, a)
    Bs, As = spec(b), spec(a)
    for R in (1., 2.):
        w = h.matrix_d("overlap", R)
        rs = np.repeat(R * R * dxyp_restated(Bs.im, Bs.jm), Bs.im)
        cs = np.repeat(R * R * dxyp_restated(As.im, As.jm), As.im)
        assert np.max(np.abs(w.wM - rs) / rs) < 1e-12
        assert np.max(np.abs(w.Mw - cs) / cs) < 1e-12


def apply_checks(h, Bs, As, X, kernels=("auto",)):
    ov, sc = h.matrix_d("overlap", R_EARTH), h.matrix_d("scaled")
    ref = h.regrid(np.ones(As.size), X)
    tol = 1e-12 * np.max(np.abs(X))
    for k in kernels:
        ov.set_kernel(k)
        sc.set_kernel(k)
        y1 = ov.apply(X, force_conservation=False) / ov.wM
        y2 = sc.apply(X, force_conservation=False)
        assert np.max(np.abs(y1 - ref)) <= tol, k
        assert np.max(np.abs(y2 - ref)) <= tol, k
    return ov, sc


@pytest.mark.parametrize("b,a", [("72x46_east", "360x180"), ("360x180", "72x46_east"), ("100x50", "144x90"), ("144x90_east", "288x180")],
                         ids=lambda x: x)
def test_apply_equals_regrid(b, a):
    Bs, As = spec(b), spec(a)
    X = np.random.default_rng(1).standard_normal(As.size) * 300.
    apply_checks(hntr(b, a), Bs, As, X)
    ov = hntr(b, a).matrix_d("overlap", R_EARTH)
    Xs = np.random.default_rng(2).standard_normal((3, As.size))
    y = ov.apply_M(Xs, force_conservation=False)
    assert y.shape == (3, Bs.size)


def test_apply_long_rows_every_kernel():
    """2' -> 4x5 deg: 18 000 entries per row, auto dispatch and every kernel ibh_weighted_set_kernel accepts."""
    from icebin_amd import Hntr, HntrSpec
    A, B = HntrSpec(10800, 5400, 0., 2.), HntrSpec(72, 46, 0., 240.)
    h = Hntr(17.17, B, A)
    X = np.random.default_rng(4).standard_normal(A.size)
    apply_checks(h, B, A, X, ("auto", "rowblock", "shortrow", "rowdual", "colsweep", "rowgroup"))


def test_size_limit_refused_before_allocation():
    """More than INT32_MAX entries is IBH_EINVAL.  A 15'' A grid (86 400 x 43 200) has more than 2^31-1 cells, which
    ibh_hntr_create itself refuses; a 30'' A onto a 30'' B shifted by half a cell both ways gives ~4 entries per A cell."""
    from icebin_amd import Hntr, HntrSpec, IcebinHipError
    with pytest.raises(IcebinHipError) as e:
        Hntr(17.17, HntrSpec(72, 46, 0., 240.), HntrSpec(86400, 43200, 0., .25))
    assert e.value.code == -1
    h = Hntr(17.17, HntrSpec(43200, 21599, 0.5, .5), HntrSpec(43200, 21600, 0., .5))
    for transpose in (False, True):
        with pytest.raises(IcebinHipError) as e:
            h.matrix_d("overlap", transpose=transpose)
        assert e.value.code == -1 and "INT32_MAX" in str(e.value)
    with pytest.raises(IcebinHipError) as e:
        h.overlap(1.)
    assert e.value.code == -1


def test_bad_arguments_with_a_handle():
    from icebin_amd import IcebinHipError, SparseSet
    h = hntr("8x4", "16x8")
    for kw in (dict(kind=7), dict(kind="overlap", transforms=(0, 5))):
        with pytest.raises(IcebinHipError) as e:
            h.matrix_d(**kw)
        assert e.value.code == -1
    with pytest.raises(IcebinHipError) as e:       # sparse extent of another grid
        h.matrix_d("overlap", dims=(SparseSet(99), None))
    assert e.value.code == -1
    s = SparseSet()
    with pytest.raises(IcebinHipError):
        h.matrix_d("overlap", dims=(s, s))
    rc = h._h and __import__("icebin_amd")._capi.lib().ibh_hntr_matrix_d(h._h, 0, 1., None, None, 0, None, 0, 0, None)
    assert rc == -1
