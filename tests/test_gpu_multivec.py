"""ibh_multivec (include/icebin_hip.h) on the GPU against tests/multivec_restatement.py, BITWISE: the device code sums in entry
order with separate products and adds, so no tolerance applies.

Sizes: n around the rows of an append block (64) and the threads of a walk / key block (256); nvar around the variables a
walk thread holds (4) and the append tile's variable chunk (32); ld equal to the extent and extent + 3."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multivec_restatement as mr  # noqa: E402

pytestmark = pytest.mark.gpu

NS = [0, 1, 63, 64, 65, 255, 256, 257]
NVARS = [1, 2, 3, 4, 5, 7, 16, 17, 31, 32, 33]


@pytest.fixture(scope="module")
def env():
    import torch
    from icebin_amd import _capi
    assert torch.cuda.is_available()
    return _capi.lib(), _capi, torch


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Dev:
    """An ibh_multivec driven through the C-ABI, with its restatement twin kept in step."""

    def __init__(self, env, nvar):
        self.L, self.capi, self.torch = env
        self.h = C.c_void_p()
        self.capi.check(self.L.ibh_multivec_create(nvar, C.byref(self.h)))
        self.nvar = nvar
        self.twin = mr.Multivec(nvar)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.ibh_multivec_destroy(self.h)
            self.h = None

    def add(self, index, weights, vals):
        index = np.ascontiguousarray(index, np.int64)
        weights = np.ascontiguousarray(weights, np.float64)
        vals = np.ascontiguousarray(vals, np.float64).reshape(len(index), self.nvar)
        self.capi.check(self.L.ibh_multivec_add_host(self.h, len(index), self.capi.ptr(index), self.capi.ptr(weights), self.capi.ptr(vals)))
        for i in range(len(index)):
            self.twin.add(index[i], vals[i], weights[i])

    def size(self):
        n, nvar = C.c_int64(), C.c_int32()
        self.capi.check(self.L.ibh_multivec_size(self.h, C.byref(n), C.byref(nvar)))
        assert nvar.value == self.nvar
        return n.value

    def get(self):
        n = self.size()
        index, weights, vals = np.empty(n, np.int64), np.empty(n, np.float64), np.empty((n, self.nvar), np.float64)
        self.capi.check(self.L.ibh_multivec_get(self.h, self.capi.ptr(index), self.capi.ptr(weights), self.capi.ptr(vals)))
        return index, weights, vals

    def view(self):
        v = self.capi.MultivecDeviceView()
        self.capi.check(self.L.ibh_multivec_device_view_get(self.h, C.byref(v)))
        return v.n, v.nvar, v.index, v.weights, v.vals

    def matches_twin(self):
        index, weights, vals = self.get()
        ti, tw, tv = self.twin.arrays()
        return np.array_equal(index, ti) and same(weights, tw) and same(vals, tv)

    # the merge calls: return (status, host copy of the output)
    def to_dense_scale(self, nE):
        t = self.torch
        d = t.full((nE + 3,), -7.0, dtype=t.float64, device="cuda")
        rc = self.L.ibh_multivec_to_dense_scale(self.h, nE, C.c_void_p(d.data_ptr()), None)
        t.cuda.synchronize()
        out = d.cpu().numpy()
        assert rc != 0 or np.all(out[nE:] == -7.0), "to_dense_scale wrote past nE"
        return rc, out[:nE]

    def to_dense(self, scale, fill, pad):
        t = self.torch
        nE = len(scale)
        ds = t.from_numpy(np.ascontiguousarray(scale)).cuda()
        d = t.full((self.nvar, nE + pad), -7.0, dtype=t.float64, device="cuda")
        rc = self.L.ibh_multivec_to_dense(self.h, C.c_void_p(ds.data_ptr()), float(fill), C.c_void_p(d.data_ptr()), nE + pad, nE, None)
        t.cuda.synchronize()
        out = d.cpu().numpy()
        assert rc != 0 or np.all(out[:, nE:] == -7.0), "to_dense wrote into the row padding"
        return rc, out[:, :nE]

    def update_dense(self, scale, prefill, pad):
        t = self.torch
        nE = len(scale)
        ds = t.from_numpy(np.ascontiguousarray(scale)).cuda()
        h = np.full((self.nvar, nE + pad), -7.0)
        h[:, :nE] = prefill
        d = t.from_numpy(h).cuda()
        rc = self.L.ibh_multivec_update_dense(self.h, C.c_void_p(ds.data_ptr()), C.c_void_p(d.data_ptr()), nE + pad, nE, None)
        t.cuda.synchronize()
        out = d.cpu().numpy()
        assert rc != 0 or np.all(out[:, nE:] == -7.0), "update_dense wrote into the row padding"
        return rc, out[:, :nE]

    def densify(self, sset, pad):
        t = self.torch
        nd = sset.dense_extent()
        d = t.full((self.nvar, nd + pad), -7.0, dtype=t.float64, device="cuda")
        rc = self.L.ibh_multivec_densify_device(self.h, sset._h, C.c_void_p(d.data_ptr()), nd + pad, None)
        t.cuda.synchronize()
        out = d.cpu().numpy()
        assert rc != 0 or np.all(out[:, nd:] == -7.0), "densify wrote into the row padding"
        return rc, out[:, :nd]


def check_merges(dev, nE, fill=-3.25, seed=0):
    """to_dense_scale, to_dense and update_dense of dev against its twin, ld = nE and nE + 3, every call twice."""
    ref_scale = mr.to_dense_scale(dev.twin, nE)
    ref_dense = mr.to_dense(dev.twin, ref_scale, fill)
    prefill = np.random.default_rng(seed + 99).standard_normal((dev.nvar, nE))
    ref_upd = mr.update_dense(dev.twin, ref_scale, prefill.copy())
    for rep in range(2):
        rc, scale = dev.to_dense_scale(nE)
        assert rc == 0 and same(scale, ref_scale), "to_dense_scale (call %d)" % rep
        for pad in (0, 3):
            rc, dense = dev.to_dense(scale, fill, pad)
            assert rc == 0 and same(dense, ref_dense), "to_dense pad=%d (call %d)" % (pad, rep)
            rc, upd = dev.update_dense(scale, prefill, pad)
            assert rc == 0 and same(upd, ref_upd), "update_dense pad=%d (call %d)" % (pad, rep)
    touched = np.zeros(nE, bool)
    touched[np.array(dev.twin.index, np.int64)] = True
    assert same(ref_upd[:, ~touched], prefill[:, ~touched])          # (of the restatement: untouched cells keep their contents)
    assert np.all(np.isinf(ref_scale[~touched]))


def random_entries(rng, n, nE, nvar):
    index = rng.integers(0, nE, n)
    if n >= 2:
        index[rng.choice(n, 2, replace=False)] = (0, nE - 1)
    return index, rng.random(n) + 0.5, rng.standard_normal((n, nvar))


@pytest.mark.parametrize("nvar", NVARS)
def test_merges_bitwise_over_sizes(env, nvar):
    rng = np.random.default_rng(1000 + nvar)
    for n in NS:
        nE = max(4, n // 3)                      # about three entries a cell, unsorted
        dev = Dev(env, nvar)
        index, weights, vals = random_entries(rng, n, nE, nvar)
        dev.add(index, weights, vals)
        assert dev.size() == n and dev.matches_twin()
        if n >= 2:
            assert 0 in dev.twin.index and nE - 1 in dev.twin.index
        check_merges(dev, nE, seed=n)


@pytest.mark.parametrize("order", ["shuffled", "descending", "ascending"])
def test_duplicate_runs_of_1_2_3_and_70(env, order):
    nvar, nE = 5, 12
    rng = np.random.default_rng(7)
    index = np.concatenate([np.full(1, 0), np.full(2, 5), np.full(3, nE - 1), np.full(70, 8)])     # 70: longer than a wave
    if order == "shuffled":
        index = rng.permutation(index)
    elif order == "descending":
        index = np.sort(index)[::-1]
    else:
        index = np.sort(index)
    dev = Dev(env, nvar)
    dev.add(index, rng.random(len(index)) + 0.5, rng.standard_normal((len(index), nvar)) * 10.0 ** rng.integers(-8, 8, (len(index), 1)))
    check_merges(dev, nE)


def test_all_entries_on_one_index(env):
    rng = np.random.default_rng(8)
    for cell, nE in ((0, 1), (0, 9), (8, 9)):
        dev = Dev(env, 3)
        dev.add(np.full(300, cell), rng.random(300), rng.standard_normal((300, 3)))
        check_merges(dev, nE)


def test_nan_rule_on_the_device(env):
    nan = np.nan
    dev = Dev(env, 2)
    rows = [(0, [nan, 1.0], 1.0), (0, [6.0, nan], 1.0),            # leading NaN forgotten | trailing NaN -> fill
            (1, [6.0, 1.0], 1.0), (1, [nan, 2.0], 1.0),
            (2, [0.0, 5.0], 0.0),                                  # zero weight sum: 0 * inf = NaN -> fill | 5 * inf = inf
            (3, [nan, nan], 1.0), (3, [2.0, nan], 1.0), (3, [4.0, 1.0], 2.0)]
    dev.add([r[0] for r in rows], [r[2] for r in rows], [r[1] for r in rows])
    rc, scale = dev.to_dense_scale(5)
    assert rc == 0 and scale.tolist() == [0.5, 0.5, np.inf, 0.25, np.inf]
    rc, out = dev.to_dense(scale, -9.0, 0)
    assert rc == 0
    assert out[0].tolist() == [3.0, -9.0, -9.0, 1.5, -9.0]
    assert out[1].tolist() == [-9.0, 1.5, np.inf, 0.25, -9.0]
    check_merges(dev, 5, fill=-9.0)
    check_merges(dev, 5, fill=np.nan)


def test_negative_zero_through_update_dense(env):
    dev = Dev(env, 1)
    dev.add([2, 2], [1.0, 1.0], [[-0.0], [-0.0]])
    rc, scale = dev.to_dense_scale(4)
    rc2, out = dev.update_dense(scale, np.full((1, 4), -0.0), 0)
    assert rc == 0 and rc2 == 0
    assert out[0, 2] == 0.0 and not np.signbit(out[0, 2])          # 0.0 + (-0.0): the sum starts from +0.0
    assert np.all(np.signbit(out[0, [0, 1, 3]]))                   # untouched cells keep their -0.0
    check_merges(dev, 4)


# ---- append_weighted ----------------------------------------------------------------------------------------------------------
def append_and_check(env, dev, w, B, pad):
    """Append the rows of linear_Weighted w from the host product B through a device copy of row stride nrow + pad."""
    L, capi, torch = env
    nrow = w.nrow_d
    h = np.full((B.shape[0], nrow + pad), -7.0)
    h[:, :nrow] = B
    d = torch.from_numpy(h).cuda()
    rc = L.ibh_multivec_append_weighted_device(dev.h, w._h, C.c_void_p(d.data_ptr()), B.shape[0], nrow + pad, None)
    torch.cuda.synchronize()
    if rc == 0:
        mr.append_weighted(dev.twin, w.dim(0), w.wM, B)
    return rc


@pytest.fixture(scope="module")
def sheets(env):
    """name -> (GCMRegridder, elevmask) of the small synthetic grids."""
    import icebin_amd
    from icebin_amd import synthetic as syn
    out = {}
    for name in ("tiny", "g50"):
        g = syn.make_grids(name)
        out[name] = (icebin_amd.from_synthetic(g), syn.dome_elevmask(g), g)
    return out


@pytest.mark.parametrize("grid", ["tiny", "g50"])
@pytest.mark.parametrize("spec", ["AvI", "EvI"])
def test_append_weighted_after_apply_transformed(env, sheets, grid, spec):
    from icebin_amd import synthetic as syn
    mm, em, g = sheets[grid]
    w = mm.regrid_matrices("greenland", em).matrix_d(spec, scale=False, correctA=(spec == "AvI"))
    assert w.nrow_d > 0
    V = syn.fields(3, w.ncol_d)
    rng = np.random.default_rng(5)
    for nvar in (1, 2, 7, 16, 17, 33):
        T, b = rng.standard_normal((3, nvar)), rng.standard_normal(nvar)
        B = w.apply_transformed(V, T, b, fill=0.0)
        assert B.shape == (nvar, w.nrow_d)
        for pad in (0, 3):
            dev = Dev(env, nvar)
            for rep in range(2):            # the second append lands behind the first
                assert append_and_check(env, dev, w, B, pad) == 0
            assert dev.size() == 2 * w.nrow_d and dev.matches_twin()
    index, weights, _ = dev.get()
    assert np.array_equal(index[:w.nrow_d], w.dim(0)) and same(weights[:w.nrow_d], w.wM)


@pytest.mark.parametrize("nrow", [1, 63, 64, 65, 129])
def test_append_weighted_at_the_row_tile_edges(env, nrow):
    from icebin_amd import linear_Weighted
    rng = np.random.default_rng(nrow)
    r = np.arange(nrow, dtype=np.int32)
    w = linear_Weighted.from_coo((nrow, nrow), r, r, np.ones(nrow), rng.random(nrow), np.ones(nrow))
    for nvar in (1, 4, 31, 32, 33):
        B = rng.standard_normal((nvar, nrow))
        dev = Dev(env, nvar)
        dev.add([5], [0.5], [np.arange(nvar)])             # the append starts at an odd entry
        assert append_and_check(env, dev, w, B, 3) == 0 and append_and_check(env, dev, w, B, 0) == 0
        assert dev.size() == 1 + 2 * nrow and dev.matches_twin()


def test_growth_and_reserve(env):
    from icebin_amd import linear_Weighted
    L, capi, torch = env
    nrow, nvar = 200, 3
    r = np.arange(nrow, dtype=np.int32)
    w = linear_Weighted.from_coo((nrow, nrow), r, r, np.ones(nrow), np.arange(nrow) + 1.0, np.ones(nrow))
    B = np.random.default_rng(3).standard_normal((nvar, nrow))
    dev = Dev(env, nvar)
    assert append_and_check(env, dev, w, B, 0) == 0
    first = dev.view()
    assert append_and_check(env, dev, w, B, 0) == 0              # no reserve in between: the buffers grow, the entries move along
    assert dev.size() == 2 * nrow and dev.matches_twin()
    capi.check(L.ibh_multivec_reserve(dev.h, 3 * nrow))
    before = dev.view()
    assert append_and_check(env, dev, w, B, 0) == 0
    after = dev.view()
    assert before[2:] == after[2:] and after[0] == 3 * nrow, "an append within the reserved capacity moved the buffers"
    assert first[0] == nrow and dev.matches_twin()
    capi.check(L.ibh_multivec_clear(dev.h))
    assert dev.size() == 0 and dev.view()[2:] == after[2:]       # clear keeps the capacity
    rc, scale = dev.to_dense_scale(3)
    assert rc == 0 and np.all(np.isinf(scale))                   # and the grouping of the old entries is gone


# ---- two ice sheets merged into the GCM's arrays ------------------------------------------------------------------------------
def two_sheets(env, g):
    """The g50 grids twice, under a dome and a shifted dome: spec -> (vector of the transformed fields, vector of the constant
    field 1 under the identity transform, cells both sheets name, extent of the GCM's index space)."""
    import icebin_amd
    from icebin_amd import SparseSet, synthetic as syn
    mm = icebin_amd.from_synthetic(g)
    mm.add_sheet("second", dict(nI=g["nI"], centroid_xy=g["I_centroid_xy"]), dict(indices=g["ex_indices"], overlaps=g["ex_area"]),
                 "Z_INTERP", g["A_proj_area"])
    dome = syn.dome_elevmask(g)
    shifted = np.roll(dome.reshape(g["nx"], g["ny"]), (4, -6), axis=(0, 1)).reshape(-1)
    T = np.array([[1.0, 0.5], [-2.0, 0.25], [0.125, 3.0]])
    b = np.array([0.5, -1.0])
    V = syn.fields(3, g["nI"])
    out = {}
    for spec, nE, correctA in (("AvI", mm.nA, True), ("EvI", mm.nE, False)):
        dev, ones = Dev(env, 2), Dev(env, 2)
        per_sheet = []
        for name, em in (("greenland", dome), ("second", shifted)):
            rm = mm.regrid_matrices(name, em)
            w = rm.matrix_d(spec, (SparseSet(nE) if spec == "EvI" else SparseSet(), SparseSet.identity(g["nI"])), scale=False,
                            correctA=correctA)
            assert append_and_check(env, dev, w, w.apply_transformed(V, T, b, fill=0.0), 0) == 0
            assert append_and_check(env, ones, w, w.apply_transformed(np.ones((2, g["nI"])), np.eye(2), np.zeros(2), fill=0.0), 3) == 0
            per_sheet.append(set(w.dim(0).tolist()))
        assert dev.matches_twin() and ones.matches_twin()
        shared = np.array(sorted(per_sheet[0] & per_sheet[1]), np.int64)
        assert len(shared) >= 1, "%s: the two sheets share no cell: the merge is not tested" % spec
        assert len(shared) < min(len(per_sheet[0]), len(per_sheet[1])), "%s: no cell belongs to one sheet alone" % spec
        out[spec] = (dev, ones, shared, nE)
    return out


def merged_ones_error(ones, shared, nE):
    rc, scale = ones.to_dense_scale(nE)
    rc2, merged = ones.to_dense(scale, 0.0, 0)
    assert rc == 0 and rc2 == 0
    assert same(merged, mr.to_dense(ones.twin, mr.to_dense_scale(ones.twin, nE), 0.0))
    return np.max(np.abs(merged[:, shared] - 1.0))


def test_two_sheets_merge(env):
    """Both sheets' unscaled AvI (correctA) and EvI products appended, then to_dense_scale, to_dense and update_dense onto a
    prefilled array: bitwise the restatement, untouched cells unchanged (check_merges)."""
    from icebin_amd import synthetic as syn
    for spec, (dev, ones, shared, nE) in two_sheets(env, syn.make_grids("g50")).items():
        check_merges(dev, nE)
        check_merges(ones, nE)


def test_two_sheets_constant_field_merges_to_one(env):
    """Constant 1 on both sheets under the identity transform: every shared cell merges to 1 within 1e-15.

    The merged value is sum(M 1) / sum(wM) over the sheets.  For EvI, and for AvI without a projection correction, wM is the
    row sum of the unscaled M, so this is 1 up to rounding.  With correctA the reference weights AvI by the NATIVE cell areas
    while the unscaled M keeps the PROJECTED ones (RegridMatrices_Dynamic.cpp:103-129: wM = sum(wAvAp * wApvI), M = ApvI), so
    there the merged value is the cell's projected / native area ratio -- up to 1 +- 0.03 on the synthetic grids' default
    ratio_amp, measured 2.477e-2 off 1 -- and equals 1 only where the two areas agree.  The AvI (correctA) case therefore
    runs on the g50 grids made with ratio_amp = 0 (native == projected: the correction is exactly 1.0); EvI runs on both."""
    from icebin_amd import synthetic as syn
    errs = {}
    for label, g in (("ratio_amp=0", syn.make_grids("g50", ratio_amp=0.0)), ("default", syn.make_grids("g50"))):
        for spec, (dev, ones, shared, nE) in two_sheets(env, g).items():
            errs[(label, spec)] = merged_ones_error(ones, shared, nE)
            print("%s %s: %d shared cells, max |merged - 1| = %.3e" % (label, spec, len(shared), errs[(label, spec)]))
    assert errs[("ratio_amp=0", "AvI")] <= 1e-15
    assert errs[("ratio_amp=0", "EvI")] <= 1e-15
    assert errs[("default", "EvI")] <= 1e-15


# ---- the other direction: dimE0 and the densified GCM vector ------------------------------------------------------------------
@pytest.mark.parametrize("nvar", [1, 5, 33])
def test_add_dense_multivec_and_densify(env, nvar):
    from icebin_amd import SparseSet
    L, capi, torch = env
    rng = np.random.default_rng(40 + nvar)
    for n in (1, 64, 257, 600):
        index = rng.integers(0, 10 ** 11, max(1, n // 3))[rng.integers(0, max(1, n // 3), n)]      # keys beyond 32 bits, repeated
        dev = Dev(env, nvar)
        dev.add(index, rng.random(n), rng.standard_normal((n, nvar)))
        for pre in ([], [int(index[n // 2]), 12345678901234, 7]):
            sset = SparseSet(-1, pre) if pre else SparseSet()
            for rep in range(2):            # the second call finds every key present
                capi.check(L.ibh_sparse_set_add_dense_multivec(sset._h, dev.h, None))
                ref_table = mr.add_dense(pre, dev.twin)
                assert sset.to_sparse().tolist() == ref_table, "first-seen numbering (n=%d, call %d)" % (n, rep)
            assert sset.to_dense(int(index[0])) == ref_table.index(int(index[0]))
            ref = mr.densify(dev.twin, ref_table)
            for pad in (0, 3):
                for rep in range(2):
                    rc, out = dev.densify(sset, pad)
                    assert rc == 0 and same(out, ref), "densify n=%d pad=%d (call %d)" % (n, pad, rep)
    ident = SparseSet.identity(12)          # an identity set serves as it is: every key below its extent is present
    dev = Dev(env, nvar)
    dev.add([9, 2, 9, 5], np.ones(4), rng.standard_normal((4, nvar)))
    capi.check(L.ibh_sparse_set_add_dense_multivec(ident._h, dev.h, None))
    assert ident.to_sparse().tolist() == list(range(12))
    rc, out = dev.densify(ident, 3)
    assert rc == 0 and same(out, mr.densify(dev.twin, list(range(12))))


# ---- concatenate ----------------------------------------------------------------------------------------------------------------
def test_append_and_concatenate(env):
    L, capi, torch = env
    rng = np.random.default_rng(11)
    parts = []
    for n in (3, 0, 70):
        d = Dev(env, 4)
        d.add(rng.integers(0, 9, n), rng.random(n), rng.standard_normal((n, 4)))
        parts.append(d)
    arr = (C.c_void_p * 3)(*[p.h.value for p in parts])
    cat = Dev(env, 4)
    L.ibh_multivec_destroy(cat.h)
    cat.h = C.c_void_p()
    capi.check(L.ibh_multivec_concatenate(3, arr, C.byref(cat.h)))
    cat.twin = mr.concatenate([p.twin for p in parts])
    assert cat.size() == 73 and cat.matches_twin()
    capi.check(L.ibh_multivec_append(parts[0].h, parts[2].h))
    capi.check(L.ibh_multivec_append(parts[0].h, parts[0].h))        # onto itself
    t = mr.concatenate([parts[0].twin, parts[2].twin])
    parts[0].twin = mr.concatenate([t, t])
    assert parts[0].size() == 146 and parts[0].matches_twin()
    check_merges(cat, 9)


# ---- refusals: argument errors reported through a status word ------------------------------------------------------------------
def last_error(env):
    return env[0].ibh_last_error().decode()


def test_refusals(env):
    from icebin_amd import SparseSet, linear_Weighted
    L, capi, torch = env
    h = C.c_void_p()
    assert L.ibh_multivec_create(0, C.byref(h)) == capi.IBH_EINVAL and "nvar" in last_error(env)
    nE = 6
    for bad, where in ((nE, 3), (-1, 0), (nE, 0), (-1, 4)):
        dev = Dev(env, 2)
        index = np.array([1, 2, 3, 4, 5])
        index[where] = bad
        dev.add(index, np.ones(5), np.ones((5, 2)))
        good_scale = np.ones(nE)
        for call in (lambda: dev.to_dense_scale(nE), lambda: dev.to_dense(good_scale, 0.0, 0),
                     lambda: dev.update_dense(good_scale, np.zeros((2, nE)), 0)):
            for rep in range(2):
                rc, _ = call()
                assert rc == capi.IBH_EINVAL
                msg = last_error(env)
                assert "entry %d" % where in msg and "%d vs. %d" % (bad, nE) in msg, msg
        if bad > 0:                          # the same vector is fine for a longer array: the handle is unchanged
            check_merges(dev, nE + 1)
            rc, _ = dev.to_dense_scale(nE)   # and a refusal after the grouping exists names the entry as well
            assert rc == capi.IBH_EINVAL and "entry %d" % where in last_error(env)
        ok = Dev(env, 2)                     # a valid call after a refusal
        ok.add([0, nE - 1], [1.0, 2.0], np.ones((2, 2)))
        check_merges(ok, nE)

    dev = Dev(env, 2)
    dev.add([4, 8, 15, 8], np.ones(4), np.arange(8.0).reshape(4, 2))
    sset = SparseSet(-1, [8, 4])
    rc, _ = dev.densify(sset, 0)
    assert rc == capi.IBH_EINVAL
    assert "entry 2" in last_error(env) and "15" in last_error(env), last_error(env)
    rc, out = dev.densify(SparseSet(-1, [15, 8, 4]), 0)
    assert rc == 0 and same(out, mr.densify(dev.twin, [15, 8, 4]))
    bounded = SparseSet(10, [8])             # add_dense beyond the set's sparse extent: refused, the set as it was
    assert L.ibh_sparse_set_add_dense_multivec(bounded._h, dev.h, None) == capi.IBH_EINVAL
    assert "entry 2" in last_error(env) and bounded.to_sparse().tolist() == [8]
    ident = SparseSet.identity(6)            # (an identity set's sparse extent is its size)
    assert L.ibh_sparse_set_add_dense_multivec(ident._h, dev.h, None) == capi.IBH_EINVAL
    assert "entry 1" in last_error(env) and ident.to_sparse().tolist() == list(range(6))

    r = np.arange(4, dtype=np.int32)
    w = linear_Weighted.from_coo((4, 4), r, r, np.ones(4), np.ones(4), np.ones(4))
    assert append_and_check(env, dev, w, np.ones((3, 4)), 0) == capi.IBH_EINVAL
    assert "nvar" in last_error(env) and dev.size() == 4
    assert append_and_check(env, dev, w, np.ones((2, 4)), 0) == 0 and dev.matches_twin()

    other = Dev(env, 3)
    arr = (C.c_void_p * 2)(dev.h.value, other.h.value)
    out = C.c_void_p()
    assert L.ibh_multivec_concatenate(2, arr, C.byref(out)) == capi.IBH_EINVAL and "nvar" in last_error(env) and not out.value
    assert L.ibh_multivec_concatenate(0, arr, C.byref(out)) == capi.IBH_EINVAL and "at least one" in last_error(env) and not out.value
    assert L.ibh_multivec_append(dev.h, other.h) == capi.IBH_EINVAL and "nvar" in last_error(env)
    assert L.ibh_multivec_concatenate(1, arr, C.byref(out)) == 0 and out.value
    L.ibh_multivec_destroy(out)


# ---- the Python class ---------------------------------------------------------------------------------------------------------
def test_python_vector_multivec(env, sheets):
    import icebin_amd
    from icebin_amd import SparseSet, VectorMultivec, concatenate
    L, capi, torch = env
    mm, em, g = sheets["tiny"]
    w = mm.regrid_matrices("greenland", em).matrix_d("AvI", scale=False, correctA=True)
    B = w.apply_transformed(np.ones((2, w.ncol_d)), np.eye(2), np.zeros(2), fill=0.0)
    a, twin = VectorMultivec(2), mr.Multivec(2)
    a.append_weighted(w, torch.from_numpy(B).cuda())
    a.append_weighted(w, B)
    mr.append_weighted(twin, w.dim(0), w.wM, B)
    mr.append_weighted(twin, w.dim(0), w.wM, B)
    a.add(int(w.dim(0)[0]), [3.0, 4.0], 0.5)
    twin.add(int(w.dim(0)[0]), [3.0, 4.0], 0.5)
    ti, tw, tv = twin.arrays()
    assert a.nvar == 2 and a.size() == len(a) == 2 * w.nrow_d + 1
    assert np.array_equal(a.index, ti) and same(a.weights, tw) and same(a.vals, tv)
    ref_scale = mr.to_dense_scale(twin, mm.nA)
    scale = a.to_dense_scale(mm.nA)
    assert same(scale.cpu().numpy(), ref_scale)
    ref = mr.to_dense(twin, ref_scale, -1.0)
    assert same(a.to_dense(scale, -1.0).cpu().numpy(), ref) and same(a.to_dense(ref_scale, -1.0), ref)
    pre = np.full((2, mm.nA), 9.0)
    ref_upd = mr.update_dense(twin, ref_scale, pre.copy())
    assert same(a.update_dense(ref_scale, pre.copy()), ref_upd)
    assert same(a.update_dense(scale, torch.from_numpy(pre).cuda()).cpu().numpy(), ref_upd)
    s = SparseSet()
    s.add_dense_multivec(a)
    assert s.to_sparse().tolist() == mr.add_dense([], twin)
    assert same(a.densify(s).cpu().numpy(), mr.densify(twin, s.to_sparse()))
    c = concatenate([a, a])
    assert c.size() == 2 * a.size() and c.nvar == 2 and np.array_equal(c.index, np.concatenate([ti, ti]))
    with pytest.raises(icebin_amd.IcebinHipError, match="at least one"):
        concatenate([])
    with pytest.raises(icebin_amd.IcebinHipError, match="nvar"):
        VectorMultivec(0)
