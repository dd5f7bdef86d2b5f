"""global_ec on the GPU: the masked-overlap exchange grid and the regridder built from it in place
(ibh_regridder_create_hntr), make_I2vX, the round trips through the IceBin input file and the Eigen-format matrix file, and
the error paths.  Everything is compared bitwise with a numpy restatement or with the regridder ibh_regridder_create builds
from the same host arrays."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from global_ec_ref import exgrid_ref, i2vx_ref  # noqa: E402
from test_gpu_hntr_matrix import triplets_ref  # noqa: E402

R = 6371000.
G = {"4x5": (72, 46, 0., 240.), "1deg": (360, 180, 0., 60.), "2x2.5": (144, 90, 0., 120.), "30min": (720, 360, 0., 30.),
     "halfdeg": (720, 360, 0., 30.), "2min": (10800, 5400, 0., 2.), "72x46_east": (72, 46, 0.5, 240.),
     "144x90_east": (144, 90, 0.25, 120.), "wide": (1, 2, 0.3, 5400.), "4x2": (4, 2, 0., 5400.)}
# (GCM, ice)
PAIRS = [("4x5", "1deg"), ("2x2.5", "30min"), ("72x46_east", "144x90_east"), ("wide", "4x2")]
MATRICES = ("AvI", "IvA", "EvI", "IvE", "AvE", "EvA", "AvX", "XvA", "EvX", "XvE")


def spec(name):
    from icebin_amd import HntrSpec
    return HntrSpec(*G[name])


def mask(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    em = rng.uniform(0., 3000., n)
    if kind == "random":
        em[rng.random(n) < 0.5] = np.nan
    elif kind == "all_nan":
        em[:] = np.nan
    return em


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def check_exgrid(gcm, A, I, em, trip=None):
    if trip is None:
        iB, iA, v = triplets_ref(A, I, "overlap", R)
    else:
        iB, iA, v = trip
    idx, area, dimA, dimI = exgrid_ref(iB, iA, v, em)
    gi, ga = gcm.exgrid()
    assert gi.shape == idx.shape and np.array_equal(gi, idx)
    assert np.array_equal(bits(ga), bits(area))
    assert np.array_equal(gcm.dimA.to_sparse(), dimA) and gcm.dimA.sparse_extent() == A.size
    assert np.array_equal(gcm.dimI.to_sparse(), dimI) and gcm.dimI.sparse_extent() == I.size
    return idx, area, dimA


def check_agridA(gcm, A, dimA):
    from icebin_amd import global_ec
    nat = global_ec.native_area(A, dimA, R)
    assert np.array_equal(gcm._A_to_sparse, dimA)
    assert np.array_equal(bits(gcm._A_native), bits(nat))
    assert np.array_equal(bits(gcm._sheets["globalI"].arrays[2]), bits(nat))
    for kind in ("native", "proj"):
        ref = np.zeros(A.size)
        ref[dimA] = nat
        assert np.array_equal(bits(gcm.wA("globalI", kind)), bits(ref))


def host_twin(gcm, interp_style):
    """ibh_regridder_create from the host arrays read back from the new regridder."""
    from icebin_amd import GCMRegridder
    idx, area, proj = gcm._sheets["globalI"].arrays
    mm = GCMRegridder(dict(nA=gcm.nA, to_sparse=gcm._A_to_sparse, native_area=gcm._A_native), gcm._hcdefs, gcm.correctA)
    mm.add_sheet("globalI", dict(nI=gcm._sheets["globalI"].nI), dict(indices=idx.reshape(-1, 2), overlaps=area), interp_style, proj)
    return mm


def same_matrix(w1, w2):
    for k in (0, 1):
        assert np.array_equal(w1.dim(k), w2.dim(k))
    r1, c1, v1 = w1.coo_dense()
    r2, c2, v2 = w2.coo_dense()
    assert np.array_equal(r1, r2) and np.array_equal(c1, c2) and np.array_equal(bits(v1), bits(v2))
    assert np.array_equal(bits(w1.wM), bits(w2.wM)) and np.array_equal(bits(w1.Mw), bits(w2.Mw))


@pytest.mark.parametrize("a,i", PAIRS, ids=lambda x: x)
@pytest.mark.parametrize("kind", ["random", "none_nan", "all_nan"])
def test_exgrid_bitwise(a, i, kind):
    import torch
    from icebin_amd import global_ec
    A, I = spec(a), spec(i)
    em = mask(kind, I.size)
    hc = global_ec.hcdefs(0., 3000., 500.)
    gcm = global_ec.gcm_from_hntr(A, I, em, hc, True, R)
    idx, _, dimA = check_exgrid(gcm, A, I, em)
    if kind == "all_nan":
        assert len(idx) == 0
    if a == "wide" and kind == "none_nan":      # a window wider than imA: one ice column, two exchange cells
        pairs = [tuple(p) for p in idx]
        assert len(pairs) > len(set(pairs))
    assert global_ec.exgrid_count(A, I, em, R) == len(idx)
    check_agridA(gcm, A, dimA)
    # the device mask gives the same regridder
    gd = global_ec.gcm_from_hntr(A, I, torch.from_numpy(em).cuda(), hc, True, R)
    gi, ga = gd.exgrid()
    hi, ha = gcm.exgrid()
    assert np.array_equal(gi, hi) and np.array_equal(bits(ga), bits(ha))
    assert np.array_equal(gd.dimI.to_sparse(), gcm.dimI.to_sparse())


@pytest.mark.parametrize("interp", ["Z_INTERP", "ELEV_CLASS_INTERP"])
@pytest.mark.parametrize("a,i", [("4x5", "1deg"), ("72x46_east", "144x90_east")], ids=lambda x: x)
def test_matrices_equal_host_built(a, i, interp):
    from icebin_amd import global_ec
    A, I = spec(a), spec(i)
    em = mask("random", I.size, 3)
    gcm = global_ec.gcm_from_hntr(A, I, em, global_ec.hcdefs(0., 3000., 500.), True, R, interp)
    twin = host_twin(gcm, interp)
    for scale in (False, True):
        for correctA in (False, True):
            r1 = gcm.regrid_matrices("globalI", em, scale=scale, correctA=correctA)
            r2 = twin.regrid_matrices("globalI", em, scale=scale, correctA=correctA)
            for name in MATRICES:
                same_matrix(r1.matrix_d(name, scale=scale, correctA=correctA), r2.matrix_d(name, scale=scale, correctA=correctA))


def test_matrices_equal_oracle():
    """One small pair: bitwise oracle.Regridder built from the same arrays."""
    from icebin_amd import global_ec
    from oracle import oracle as orc
    A, I = spec("4x5"), spec("1deg")
    em = mask("random", I.size, 5)
    hc = global_ec.hcdefs(0., 3000., 500.)
    gcm = global_ec.gcm_from_hntr(A, I, em, hc, True, R)
    idx, area, proj = gcm._sheets["globalI"].arrays
    g = dict(nA=A.size, nI=I.size, nhc=len(hc), hcdefs=hc, hc_stride_A=1, hc_stride_HC=A.size,
             ex_indices=idx.reshape(-1, 2), ex_area=area, A_to_sparse=gcm._A_to_sparse, A_native_area=gcm._A_native,
             A_proj_area=proj, interp_style=0)
    rg = orc.Regridder(g)
    rm = gcm.regrid_matrices("globalI", em, scale=True, correctA=True)
    for name in ("AvI", "IvA", "EvI", "IvE", "AvE", "EvA"):
        w = rm.matrix(name)
        o = rg.matrix_d(name, em, scale=True, correctA=True)
        r, c, v = w.coo_dense()
        assert np.array_equal(r, o.row) and np.array_equal(c, o.col) and np.array_equal(bits(v), bits(o.val)), name
        assert np.array_equal(bits(w.wM), bits(o.wM)) and np.array_equal(bits(w.Mw), bits(o.Mw)), name
        assert np.array_equal(w.dim(0), o.dims[0]) and np.array_equal(w.dim(1), o.dims[1]), name


@pytest.mark.parametrize("kind", ["random", "none_nan", "all_nan"])
def test_streamed_2min_to_halfdeg(kind):
    """The 2' pair: every mask, host and device; with the random mask the matrices, large enough for the streamed
    assembly (built_fast code 2; IBH_DEBUG_SORT=1 reports the path)."""
    import torch
    from icebin_amd import Hntr, global_ec
    from icebin_amd._capi import check, lib
    A, I = spec("halfdeg"), spec("2min")
    em = mask(kind, I.size, 7)
    hc = global_ec.hcdefs(0., 3000., 250.)
    gcm = global_ec.gcm_from_hntr(A, I, em, hc, True, R)
    trip = Hntr(17.17, A, I).overlap(R)         # stream-order overlap (checked against the restatement by the Hntr tests)
    idx, _, dimA = check_exgrid(gcm, A, I, em, trip=(trip[0].astype(np.int64), trip[1].astype(np.int64), trip[2]))
    del trip
    check_agridA(gcm, A, dimA)
    gd = global_ec.gcm_from_hntr(A, I, torch.from_numpy(em).cuda(), hc, True, R)
    gi, ga = gd.exgrid()
    hi, ha = gcm.exgrid()
    assert np.array_equal(gi, hi) and np.array_equal(bits(ga), bits(ha))
    assert np.array_equal(gd.dimA.to_sparse(), gcm.dimA.to_sparse()) and np.array_equal(gd.dimI.to_sparse(), gcm.dimI.to_sparse())
    del gd
    if kind != "random":
        return
    twin = host_twin(gcm, "Z_INTERP")
    os.environ["IBH_DEBUG_SORT"] = "1"
    codes = {}
    try:
        r1 = gcm.regrid_matrices("globalI", em, scale=False, correctA=True)
        r2 = twin.regrid_matrices("globalI", em, scale=False, correctA=True)
        for name in ("AvI", "IvA", "EvI", "IvE"):
            w1 = r1.matrix_d(name, scale=False, correctA=True)
            code = C.c_int()
            check(lib().ibh_weighted_built_fast(w1._h, C.byref(code)))
            codes[name] = code.value
            print("global_ec 2min %s: built_fast code %d" % (name, code.value))
            same_matrix(w1, r2.matrix_d(name, scale=False, correctA=True))
    finally:
        del os.environ["IBH_DEBUG_SORT"]
    assert 2 in codes.values(), codes           # the streamed assembly served this grid


def i2vx_check(gcm, I, I2, em, name, dimI2, eq_rad=R):
    from icebin_amd import SparseSet, global_ec
    rm = gcm.regrid_matrices("globalI", em, scale=False, correctA=True)
    dimI, dimX = SparseSet(), SparseSet()
    IvX = rm.matrix_d(name, (dimI, dimX), scale=False, correctA=True)
    before = dimI2.to_sparse()
    trip = triplets_ref(I, I2, "overlap", eq_rad, ~np.isnan(em))
    r, c, v = IvX.coo_dense()
    ref = i2vx_ref(trip, dimI.to_sparse(), before, r, c, v, IvX.wM, IvX.Mw, IvX.shape[1])
    out = global_ec.make_I2vX(IvX, I, I2, em, dimI2, eq_rad)
    ro, co, vo = out.coo_dense()
    assert np.array_equal(ro, ref[0]) and np.array_equal(co, ref[1]) and np.array_equal(bits(vo), bits(ref[2]))
    assert np.array_equal(bits(out.wM), bits(ref[3])) and np.array_equal(bits(out.Mw), bits(ref[4]))
    assert np.array_equal(dimI2.to_sparse(), ref[5]) and np.array_equal(out.dim(1), dimX.to_sparse())
    assert out.conservative == IvX.conservative and not out.scaled
    s1, s0 = out.wM.sum(), IvX.wM.sum()
    assert abs(s1 - s0) <= 1e-13 * abs(s0)
    return out


@pytest.mark.parametrize("name", ["IvE", "IvA"])
def test_make_I2vX_bitwise(name):
    from icebin_amd import SparseSet, global_ec
    A, I, I2 = spec("4x5"), spec("1deg"), spec("2x2.5")
    em = mask("random", I.size, 11)
    gcm = global_ec.gcm_from_hntr(A, I, em, global_ec.hcdefs(0., 3000., 500.), True, R)
    dimI2 = SparseSet(I2.size)
    i2vx_check(gcm, I, I2, em, name, dimI2)
    # a second product onto the same, now populated, dimI2 appends to it
    i2vx_check(gcm, I, I2, em, "IvA" if name == "IvE" else "IvE", dimI2)


def test_I2vX_outlives_the_IvX_it_was_made_from():
    """IvX made with dims of its own owns its X set, so I2vX takes a copy of it and not the pointer: with IvX destroyed,
    I2vX's columns still read back and the matrix applies; they are the columns of the same build on a caller's X set,
    which I2vX shares."""
    import gc
    from icebin_amd import SparseSet, global_ec
    A, I, I2 = spec("4x5"), spec("1deg"), spec("2x2.5")
    em = mask("random", I.size, 11)
    rm = global_ec.gcm_from_hntr(A, I, em, global_ec.hcdefs(0., 3000., 500.), True, R).regrid_matrices("globalI", em, scale=False,
                                                                                                      correctA=True)
    IvX = rm.matrix_d("IvA", (None, None), scale=False, correctA=True)
    out = global_ec.make_I2vX(IvX, I, I2, em, None, R)
    out._keep = ()          # the wrapper's own reference to IvX
    del IvX
    gc.collect()
    dimX = SparseSet()
    out2 = global_ec.make_I2vX(rm.matrix_d("IvA", (SparseSet(), dimX), scale=False, correctA=True), I, I2, em, None, R)
    assert out.ncol_d == out2.ncol_d > 0
    assert np.array_equal(out.dim(1), out2.dim(1)) and np.array_equal(out2.dim(1), dimX.to_sparse())
    x = np.random.default_rng(2).random(out.ncol_d)
    assert np.array_equal(bits(out.apply(x)), bits(out2.apply(x)))


def test_ncio_round_trip(tmp_path):
    from icebin_amd import GCMRegridder, global_ec
    A, I = spec("72x46_east"), spec("144x90_east")
    em = mask("random", I.size, 13)
    gcm = global_ec.gcm_from_hntr(A, I, em, global_ec.hcdefs(0., 3000., 500.), True, R)
    f = str(tmp_path / "gcm.nc")
    gcm.ncio_write(f)
    back = GCMRegridder(f)
    r1 = gcm.regrid_matrices("globalI", em, scale=True, correctA=True)
    r2 = back.regrid_matrices("globalI", em, scale=True, correctA=True)
    for name in MATRICES:
        same_matrix(r1.matrix_d(name, scale=True, correctA=True), r2.matrix_d(name, scale=True, correctA=True))


@pytest.mark.parametrize("Achar", ["A", "O"])
def test_write_matrices_round_trip(tmp_path, Achar):
    from icebin_amd import global_ec, nc_read_weighted
    A, I, I2 = spec("4x5"), spec("1deg"), spec("2x2.5")
    em = mask("random", I.size, 17)
    gcm = global_ec.gcm_from_hntr(A, I, em, global_ec.hcdefs(0., 3000., 500.), True, R)
    f = str(tmp_path / "ec.nc")
    built = global_ec.write_matrices(gcm, em, I2, f, Achar=Achar)
    assert sorted(built) == sorted(n.replace("A", Achar) for n in ["AvI", "EvI", "IvE", "I2vE", "IvA", "I2vA", "AvE", "EvA"])
    for name, w in built.items():
        r = nc_read_weighted(f, name)
        same_matrix(r, w)


def test_check_negative():
    from icebin_amd import global_ec, linear_Weighted
    ok = linear_Weighted.from_coo((2, 2), [0, 1], [0, 1], [1., 2.], [1., 2.], [1., 2.])
    global_ec.check_negative(ok, "ok")
    bad = linear_Weighted.from_coo((2, 2), [0, 1], [0, 1], [1., -2.], [1., 2.], [1., 2.])
    with pytest.raises(RuntimeError, match="Negative values"):
        global_ec.check_negative(bad, "bad")


def _desc(A, I, em, hc):
    from icebin_amd import Hntr, global_ec
    h = Hntr(17.17, A, I)
    d, keep = global_ec._desc(h, em, hc, R, "Z_INTERP")
    return h, d, keep


def _create_fails(d, match):
    from icebin_amd import SparseSet
    from icebin_amd._capi import check, lib
    dA, dI = SparseSet(), SparseSet()
    h = C.c_void_p(1)
    with pytest.raises(RuntimeError, match=match):
        check(lib().ibh_regridder_create_hntr(C.byref(d), dA._h, dI._h, C.byref(h)))
    assert not h.value
    assert dA.dense_extent() == 0 and dI.dense_extent() == 0 and dA.sparse_extent() == -1 and dI.sparse_extent() == -1


def test_error_wrong_mask_length():
    A, I = spec("4x5"), spec("1deg")
    h, d, keep = _desc(A, I, np.zeros(I.size - 1), np.zeros(1))
    _create_fails(d, "elevmaskI has")


def test_error_nE_overflow():
    A, I = spec("halfdeg"), spec("1deg")
    hc = np.arange(8300, dtype=np.float64)             # 259200 * 8300 >= 2^31
    h, d, keep = _desc(A, I, np.zeros(I.size), hc)
    _create_fails(d, "overflows int32")


def test_error_int32_limit_before_allocation():
    """A GCM grid of 2.147e9 cells over a 3 x 3 ice grid: more than INT32_MAX exchange cells.  The count query answers
    without building; the create refuses before allocating."""
    from icebin_amd import HntrSpec
    from icebin_amd._capi import check, lib
    A, I = HntrSpec(46340, 46340, 0., 10800. / 46340), HntrSpec(3, 3, 0., 3600.)
    h, d, keep = _desc(A, I, np.zeros(I.size), np.zeros(1))
    n = C.c_int64()
    check(lib().ibh_hntr_exgrid_count(C.byref(d), C.byref(n)))
    assert n.value > 2**31 - 1
    _create_fails(d, "exceed the regridder's limit")


def test_error_I2vX_grid_mismatch():
    from icebin_amd import SparseSet, global_ec
    A, I, I2 = spec("4x5"), spec("1deg"), spec("2x2.5")
    em = mask("random", I.size, 19)
    gcm = global_ec.gcm_from_hntr(A, I, em, global_ec.hcdefs(0., 3000., 500.), True, R)
    rm = gcm.regrid_matrices("globalI", em, scale=False, correctA=True)
    IvE = rm.matrix_d("IvE", (SparseSet(), SparseSet()), scale=False, correctA=True)
    dimI2 = SparseSet(I2.size)
    dimI2.add_dense(5)
    with pytest.raises(RuntimeError, match="sparse extent"):
        global_ec.make_I2vX(IvE, spec("30min"), I2, mask("random", spec("30min").size), dimI2, R)   # hspecI is not IvE's grid
    assert dimI2.to_sparse().tolist() == [5]
