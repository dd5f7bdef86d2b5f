"""Hntr's typed regrid on the GPU: int16 / float32 / float64 planes and a constant weight (ibh_hntr_regrid_typed_*,
Hntr.regrid / regrid_device / regrid_shape).  An int16 or float32 element converts to double exactly, so every typed result must
be bitwise both the numpy restatement of tests/test_gpu_hntr.py on the same arrays (regrid_ref widens with np.asarray(..,
float64)) and the double path on the widened planes; a constant weight c is bitwise a plane filled with c.  Zero tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_hntr import regrid_ref, same, spec  # noqa: E402
from test_hntr import GRIDS, PAIRS  # noqa: E402,F401

DATMIS = -1e30
F64, I16, F32 = 0, 1, 2
DT = {"f64": np.float64, "f32": np.float32, "i16": np.int16}
PAIRS_T = [("4x2", "8x4"), ("72x46", "360x180"), ("72x46_east", "360x180"), ("144x90_east", "288x180"), ("91x45", "100x50")]
assert all(p in PAIRS for p in PAIRS_T)


def last_error():
    from icebin_amd import _capi
    return _capi.lib().ibh_last_error().decode(errors="replace")


def zero_block(sp):
    """fields(zeros=True) of tests/test_gpu_hntr.py: a rectangular block and the whole southern polar row."""
    jj, ii = np.meshgrid(np.arange(sp.jm), np.arange(sp.im), indexing="ij")
    z = ((ii >= sp.im // 4) & (ii < sp.im // 2) & (jj >= sp.jm // 4) & (jj < sp.jm // 2)) | (jj == 0)
    return z.reshape(-1)


def sources(sp, nvar, seed):
    """Source planes per element type: int16 elevations in [-11000, 8850], float32 / float64 normal variates."""
    rng = np.random.default_rng(seed)
    return {"i16": rng.integers(-11000, 8851, (nvar, sp.size)).astype(np.int16),
            "f32": rng.standard_normal((nvar, sp.size)).astype(np.float32),
            "f64": rng.standard_normal((nvar, sp.size))}


def weights(sp, nvar, seed):
    """Weight planes per element type, each with the zero block (DATMIS cells occur); "i16" in {0, 1}, "focean" (int16) in
    {0, 1, 2}."""
    rng = np.random.default_rng(seed + 1000)
    z = zero_block(sp)
    w = {"i16": rng.integers(0, 2, (nvar, sp.size)).astype(np.int16),
         "focean": rng.integers(0, 3, (nvar, sp.size)).astype(np.int16),
         "f32": rng.uniform(0.1, 1.0, (nvar, sp.size)).astype(np.float32),
         "f64": rng.uniform(0.1, 1.0, (nvar, sp.size))}
    for v in w.values():
        v[:, z] = 0
    return w


def plane_of(c, sp):
    return np.full(sp.size, float(c))


def wide(x):
    return x if np.isscalar(x) else x.astype(np.float64)


@pytest.mark.parametrize("b,a", PAIRS_T + [(a, b) for b, a in PAIRS_T], ids=lambda x: x)
def test_type_combinations_on_grid_pairs(b, a):
    from icebin_amd import Hntr
    B, A = spec(b), spec(a)
    h = Hntr(17.17, B, A, DATMIS)
    S, W = sources(A, 3, 11), weights(A, 3, 11)
    forms = [("c1", 1.0), ("c037", 0.37), ("c0", 0.0)] + [(k, W[k]) for k in ("f64", "f32", "i16", "focean")]
    for wname, w in forms:
        const = np.isscalar(w)
        wplane = plane_of(w, A) if const else w[0]
        for sname, X in S.items():
            tag = (b, a, wname, sname)
            # one weight shared by three fields
            got = h.regrid(w if const else w[0], X)
            assert got.shape == (3, B.size) and got.dtype == np.float64, tag
            assert same(got, h.regrid(wide(wplane), wide(X))), tag
            for k in range(3):
                ref, wref = regrid_ref(B, A, wplane, X[k], DATMIS)
                assert same(got[k], ref), tag + (k,)
            assert np.array_equal(got[0] == DATMIS, wref == 0), tag
            if wname == "c0":
                assert np.all(wref == 0) and np.all(got == DATMIS), tag
            if const:
                continue
            # one weight per field, two fields
            got = h.regrid(w[:2], X[:2])
            assert same(got, h.regrid(wide(w[:2]), wide(X[:2]))), tag
            for k in range(2):
                assert same(got[k], regrid_ref(B, A, w[k], X[k], DATMIS)[0]), tag + (k,)
            if wname == "i16":      # 1 - FOCEAN
                got = h.regrid(w[1], X[1], wtm=-1., wtb=1.)
                assert same(got, regrid_ref(B, A, w[1], X[1], DATMIS, wtm=-1., wtb=1.)[0]), tag
                assert same(got, h.regrid(wide(w[1]), wide(X[1]), wtm=-1., wtb=1.)), tag
    # a constant weight under wtm / wtb: wta = wtm*c + wtb, as for a plane of c
    got = h.regrid(0.37, S["i16"][0], wtm=-1., wtb=1.)
    assert same(got, regrid_ref(B, A, plane_of(0.37, A), S["i16"][0], DATMIS, wtm=-1., wtb=1.)[0])


def to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda:0"))


def odd_planes(x, nA):
    """The planes of x [n, nA] as a view with row stride nA + 1 that starts one element into a larger tensor: the plane bases
    are aligned to the element only."""
    import torch
    n = x.shape[0]
    big = torch.zeros(n * (nA + 1) + 1, dtype=to_dev(x[:1, :1]).dtype, device=torch.device("cuda:0"))
    v = big[1:].view(n, nA + 1)[:, :nA]
    v.copy_(to_dev(x))
    assert v.stride(0) == nA + 1 and v.data_ptr() == big.data_ptr() + big.element_size()
    return v


@pytest.mark.parametrize("wname,sname", [("const", "i16"), ("i16", "i16"), ("f32", "f32")])
def test_grouping_and_plane_layout(wname, sname):
    import torch
    from icebin_amd import Hntr
    A, B = spec("360x180"), spec("72x46_east")
    h = Hntr(17.17, B, A, DATMIS)
    X = sources(A, 17, 21)[sname]
    w = 0.37 if wname == "const" else to_dev(weights(A, 17, 21)[wname])
    shared = w if wname == "const" else w[0]
    wplane = plane_of(0.37, A) if wname == "const" else weights(A, 17, 21)[wname][0]
    singles = [h.regrid_device(shared, to_dev(X[k:k + 1])).cpu().numpy()[0] for k in range(17)]
    for k in (0, 8, 16):
        assert same(singles[k], regrid_ref(B, A, wplane, X[k], DATMIS)[0]), k
    ldb = B.size + 11
    for nvar in (1, 2, 3, 5, 9, 17):
        Ap = odd_planes(X[:nvar], A.size)
        Wp = shared if wname == "const" else odd_planes(weights(A, 17, 21)[wname][:1], A.size)[0]
        Bp = torch.full((nvar, ldb), float("nan"), dtype=torch.float64, device=Ap.device)
        out = h.regrid_device(Wp, Ap, out=Bp[:, :B.size])
        torch.cuda.synchronize()
        got = Bp.cpu().numpy()
        assert out.data_ptr() == Bp.data_ptr() and out.dtype == torch.float64
        for k in range(nvar):
            assert same(got[k, :B.size], singles[k]), (nvar, k)
        assert np.all(np.isnan(got[:, B.size:])), nvar
    if wname == "const":
        return
    # one weight per field, weights and fields both on odd strides
    Wn = weights(A, 17, 21)[wname]
    got = h.regrid_device(odd_planes(Wn[:5], A.size), odd_planes(X[:5], A.size)).cpu().numpy()
    for k in range(5):
        assert same(got[k], regrid_ref(B, A, Wn[k], X[k], DATMIS)[0]), k
    # weight and source of different types
    other = "f64" if sname != "f64" else "f32"
    got = h.regrid_device(w[0], to_dev(sources(A, 2, 21)[other])).cpu().numpy()
    for k in range(2):
        assert same(got[k], regrid_ref(B, A, wplane, sources(A, 2, 21)[other][k], DATMIS)[0]), k


# Column chunks.  The planes are staged into LDS as doubles, so K depends on the number of staged planes (weight + fields, or the
# fields alone under a constant weight), not on the element size.  From the 2' grid of test_bitwise_from_2_minutes onto 1 degree
# the windows are 30 columns wide and a constant weight's K covers them, so the chunked case takes the nearest larger A grid that
# still chunks under both weight forms: 1' in longitude (21600 columns, windows of 60) and 30' in latitude (360 rows, which keeps
# the planes at 7.8 M cells).
CHUNK_A, CHUNK_B = (21600, 360, 0., 30.), (360, 180, 0., 60.)


def widest_window(B, A):
    from icebin_amd.hntr import partition
    p = partition(B, A)
    return int((p["IMAX"] - p["IMIN"] + 1).max())


@pytest.fixture(scope="module")
def chunk_case():
    from icebin_amd import HntrSpec
    A, B = HntrSpec(*CHUNK_A), HntrSpec(*CHUNK_B)
    rng = np.random.default_rng(31)
    X = {"i16": rng.integers(-11000, 8851, A.size).astype(np.int16), "f32": rng.standard_normal(A.size).astype(np.float32)}
    X["f64"] = rng.standard_normal(A.size)
    W = rng.integers(0, 3, A.size).astype(np.int16)
    W[zero_block(A)] = 0
    refs = {(wn, sn): regrid_ref(B, A, plane_of(1.0, A) if wn == "const" else W, x, DATMIS)[0] for sn, x in X.items()
            for wn in ("const", "shared")}
    return A, B, W, X, refs


@pytest.mark.parametrize("sname", ["f64", "f32", "i16"])
@pytest.mark.parametrize("wname", ["shared", "const"])
def test_column_chunks(chunk_case, wname, sname):
    from icebin_amd import Hntr
    # several chunks per step
    A, B, W, X, refs = chunk_case
    h = Hntr(17.17, B, A, DATMIS)
    wdt = None if wname == "const" else np.int16
    shape = h.regrid_shape(1, wdt, DT[sname])
    assert shape["K"] < widest_window(B, A), shape
    got = h.regrid(1.0 if wname == "const" else W, X[sname])
    assert same(got, refs[(wname, sname)])
    assert same(got, h.regrid(plane_of(1.0, A) if wname == "const" else wide(W), wide(X[sname])))
    # one chunk per step
    B2, A2 = spec("72x46"), spec("360x180")
    h2 = Hntr(17.17, B2, A2, DATMIS)
    shape = h2.regrid_shape(1, wdt, DT[sname])
    assert shape["K"] >= widest_window(B2, A2), shape
    x, w = sources(A2, 1, 32)[sname][0], weights(A2, 1, 32)["focean"][0]
    got = h2.regrid(1.0 if wname == "const" else w, x)
    assert same(got, regrid_ref(B2, A2, plane_of(1.0, A2) if wname == "const" else w, x, DATMIS)[0])


@pytest.mark.parametrize("wname", ["const", "i16"])
@pytest.mark.parametrize("b,a", [("72x46", "360x180"), ("4x2", "8x4")], ids=lambda x: x)
def test_mean_polar_and_nan_datmis(b, a, wname):
    import math
    from icebin_amd import Hntr
    from icebin_amd.hntr import partition
    B, A = spec(b), spec(a)
    X = sources(A, 1, 41)["i16"][0]
    if wname == "const":
        w, wplane = 1.0, plane_of(1.0, A)
    else:
        w = weights(A, 1, 41)["i16"][0]
        w.reshape(A.jm, A.im)[partition(B, A)["JMAX"][0]:, :] |= 1     # weight everywhere else: the northern row has a mean
        w.reshape(A.jm, A.im)[:partition(B, A)["JMAX"][0], :] = 0      # none under B's southern polar row: DATMIS there
        wplane = w
    for datmis in (DATMIS, float("nan")):
        h = Hntr(17.17, B, A, datmis)
        for mp in (False, True):
            got = h.regrid(w, X, mean_polar=mp)
            assert same(got, regrid_ref(B, A, wplane, X, datmis, mean_polar=mp)[0]), (datmis, mp)
            assert same(got, h.regrid(wide(wplane), wide(X), mean_polar=mp)), (datmis, mp)
        got = h.regrid(w, X, mean_polar=True)
        north = got[-B.im:]
        assert np.all(north == north[0]) and np.isfinite(north[0])
        south = got[:B.im]
        if wname == "const":
            assert np.all(south == south[0]) and np.isfinite(south[0])
        else:
            assert np.all(np.isnan(south)) if math.isnan(datmis) else np.all(south == datmis)


def typed_host(h, w, wta_type, wta_ld, wconst, X, a_type, nvar, lda, out, ldb, mean_polar=0, wtm=1., wtb=0.):
    from icebin_amd import _capi
    return _capi.lib().ibh_hntr_regrid_typed_host(h._h, None if w is None else w.ctypes.data, wta_type, wta_ld, wconst,
                                                  None if X is None else X.ctypes.data, a_type, nvar, lda, out.ctypes.data, ldb,
                                                  mean_polar, wtm, wtb)


@pytest.mark.parametrize("wname,sname", [("const", "i16"), ("i16", "i16"), ("f64", "f32")])
def test_host_form_is_the_device_form(wname, sname):
    from icebin_amd import Hntr, _capi
    code = {"f64": F64, "i16": I16, "f32": F32}
    A, B = spec("360x180"), spec("72x46_east")
    h = Hntr(17.17, B, A, DATMIS)
    X = sources(A, 3, 51)[sname]
    Wn = None if wname == "const" else weights(A, 3, 51)[wname]
    dev = h.regrid_device(0.37 if Wn is None else to_dev(Wn[0]), to_dev(X), mean_polar=True).cpu().numpy()
    assert same(h.regrid(0.37 if Wn is None else Wn[0], X, mean_polar=True), dev)
    # the C entry on padded host planes (lda, ldb in elements of the plane's own type); gaps of B stay as they were
    lda, ldb = A.size + 3, B.size + 5
    Xp = np.zeros((3, lda), X.dtype)
    Xp[:, :A.size] = X
    out = np.full((3, ldb), 7.5)
    rc = typed_host(h, None if Wn is None else Wn[0], code.get(wname, 0), 0, 0.37, Xp, code[sname], 3, lda, out, ldb, mean_polar=1)
    assert rc == _capi.IBH_OK, last_error()
    assert same(out[:, :B.size], dev) and np.all(out[:, B.size:] == 7.5)
    if Wn is not None:      # one weight per field
        Wp = np.zeros((3, lda), Wn.dtype)
        Wp[:, :A.size] = Wn
        rc = typed_host(h, Wp, code[wname], lda, 0., Xp, code[sname], 3, lda, out, ldb)
        assert rc == _capi.IBH_OK, last_error()
        assert same(out[:, :B.size], h.regrid_device(to_dev(Wn), to_dev(X)).cpu().numpy())


def test_refusals():
    import torch
    from icebin_amd import Hntr, HntrSpec, _capi
    A, B = spec("360x180"), spec("72x46_east")
    h = Hntr(17.17, B, A, DATMIS)
    X, W = sources(A, 3, 61), weights(A, 3, 61)
    out = np.full((3, B.size), 7.5)
    # an unknown type code, of the source or of the weight plane; a constant weight ignores wta_type
    for wt, at, bad in ((I16, 3, 3), (7, I16, 7), (-1, F64, -1)):
        assert typed_host(h, W["i16"][0], wt, 0, 0., X["i16"], at, 3, A.size, out, B.size) == _capi.IBH_EINVAL
        assert "type code %d" % bad in last_error(), last_error()
    assert typed_host(h, None, 99, 12345, 1.0, X["i16"], I16, 3, A.size, out, B.size) == _capi.IBH_OK
    assert same(out, h.regrid(1.0, X["i16"]))
    out[:] = 7.5
    # wta_ld inside (0, nA); a null A; lda < nA
    assert typed_host(h, W["i16"], I16, 5, 0., X["i16"], I16, 3, A.size, out, B.size) == _capi.IBH_EINVAL
    assert "wta_ld=5" in last_error()
    assert typed_host(h, W["i16"], I16, A.size - 1, 0., X["i16"], I16, 3, A.size, out, B.size) == _capi.IBH_EINVAL
    assert typed_host(h, W["i16"][0], I16, 0, 0., None, I16, 3, A.size, out, B.size) == _capi.IBH_EINVAL
    assert typed_host(h, None, 0, 0, 1.0, None, I16, 3, A.size, out, B.size) == _capi.IBH_EINVAL
    assert typed_host(h, None, 0, 0, 1.0, X["i16"], I16, 3, A.size - 1, out, B.size) == _capi.IBH_EINVAL
    assert np.all(out == 7.5)
    # the device entry refuses the same before it launches anything
    dX, dout = to_dev(X["i16"]), torch.full((3, B.size), 7.5, dtype=torch.float64, device=torch.device("cuda:0"))
    lib = _capi.lib()
    rc = lib.ibh_hntr_regrid_typed_device(h._h, None, 0, 0, 1.0, dX.data_ptr(), 5, 3, A.size, dout.data_ptr(), B.size, 0, 1., 0., None)
    assert rc == _capi.IBH_EINVAL and "type code 5" in last_error()
    rc = lib.ibh_hntr_regrid_typed_device(h._h, dX.data_ptr(), I16, 7, 0., dX.data_ptr(), I16, 3, A.size, dout.data_ptr(), B.size, 0, 1.,
                                          0., None)
    assert rc == _capi.IBH_EINVAL
    # mean_polar on a one-row B grid
    one = Hntr(17.17, HntrSpec(8, 1, 0., 10800.), A, DATMIS)
    assert one.regrid(1.0, X["i16"][0]).shape == (8,)
    with pytest.raises(_capi.IcebinHipError, match="mean_polar needs jmB >= 2") as ei:
        one.regrid(1.0, X["i16"][0], mean_polar=True)
    assert ei.value.code == _capi.IBH_EINVAL
    # overlapping planes through regrid_device, typed and under a constant weight
    with pytest.raises(ValueError, match="A planes overlap"):
        h.regrid_device(1.0, dX[0].expand(3, -1), out=dout)
    with pytest.raises(ValueError, match="WTA planes overlap"):
        h.regrid_device(torch.as_strided(dX, (3, A.size), (A.size - 1, 1)), dX, out=dout)
    with pytest.raises(ValueError, match="out planes overlap"):
        h.regrid_device(1.0, dX, out=torch.zeros(B.size, dtype=torch.float64, device=dX.device).expand(3, -1))
    torch.cuda.synchronize()
    assert torch.all(dout == 7.5)
    # any other dtype goes through float64, as before
    for dt in (np.float16, np.int32):
        x, w = X["i16"][:2].astype(dt), W["i16"][0].astype(dt)
        assert same(h.regrid(w, x), h.regrid(w.astype(np.float64), x.astype(np.float64)))
        assert same(h.regrid(1.0, x), h.regrid(plane_of(1.0, A), x.astype(np.float64)))


def test_regrid_shape():
    from icebin_amd import Hntr, HntrSpec, _capi
    budget = 40 * 1024
    for bdef, adef in ((GRIDS["72x46_east"], GRIDS["360x180"]), (CHUNK_B, CHUNK_A), (GRIDS["8x4"], GRIDS["4x2"]),
                       ((720, 360, 0., 30.), CHUNK_A)):
        B, A = HntrSpec(*bdef), HntrSpec(*adef)
        h = Hntr(17.17, B, A, DATMIS)
        wmax = widest_window(B, A)
        for nvar in (1, 2, 3, 5, 9, 17):
            for wdt in (None, np.float64, np.float32, np.int16):
                for adt in (np.float64, np.float32, np.int16):
                    for per_field in (False, True) if wdt is not None else (False,):
                        s = h.regrid_shape(nvar, wdt, adt, per_field=per_field)
                        assert s == h.regrid_shape(nvar, wdt, adt, per_field=per_field)
                        assert set(s) == {"NV", "L", "K", "lds_bytes"}
                        assert 1 <= s["NV"] <= 8 and (s["NV"] == 1 or not per_field)
                        assert 1 <= s["L"] <= 64 and s["L"] & (s["L"] - 1) == 0
                        assert 1 <= s["K"] <= wmax
                        planes = s["NV"] + (wdt is not None)
                        assert s["lds_bytes"] == 8 * planes * s["L"] * (s["K"] | 1) <= budget, s
                        # staged as doubles: the element types change nothing
                        assert s == h.regrid_shape(nvar, None if wdt is None else np.float64, np.float64, per_field=per_field)
            # a constant weight stages one plane fewer: out of the same LDS budget its chunks are never narrower.  The budget is
            # 20 KiB while that leaves 16 columns; otherwise it is 40 KiB with a weight plane and 32 KiB under
            # a constant weight, so only launches that both stay within 20 KiB compare.
            c, w = h.regrid_shape(nvar, None, np.int16), h.regrid_shape(nvar, np.int16, np.int16)
            small = 20 * 1024
            assert c["lds_bytes"] <= 32 * 1024, c
            if w["lds_bytes"] <= small:
                assert c["lds_bytes"] <= small and c["K"] >= w["K"], (c, w)
            if c["lds_bytes"] > small:
                assert w["lds_bytes"] > small, (c, w)
    rc = _capi.lib().ibh_hntr_regrid_shape(h._h, 1, 0, 9, 0, 0, None, None, None, None)
    assert rc == _capi.IBH_EINVAL and "type code 9" in last_error()


def test_byte_swapped_arrays_equal_the_native_ones():
    # arrays in the other byte order (netCDF-3, Fortran and ETOPO1's MSB int16 files give them) are converted to native float64 on
    # the host, as every input was before the typed regrid; only native int16 / float32 / float64 memory reaches the library
    from icebin_amd import Hntr
    from icebin_amd.hntr import _code
    B, A = spec("72x46_east"), spec("360x180")
    h = Hntr(17.17, B, A, DATMIS)
    S, W = sources(A, 2, 71), weights(A, 2, 71)
    other = ">" if sys.byteorder == "little" else "<"
    for sname, wname in (("f64", "f64"), ("i16", "i16"), ("f32", "f32"), ("i16", "focean")):
        X, w = S[sname], W[wname]
        Xs, ws = X.astype(X.dtype.newbyteorder(other)), w.astype(w.dtype.newbyteorder(other))
        assert not Xs.dtype.isnative and Xs.dtype.name == X.dtype.name and np.array_equal(Xs, X)
        assert Xs.tobytes() != X.tobytes()
        native = h.regrid(w[0], X)
        assert same(native[0], regrid_ref(B, A, w[0], X[0], DATMIS)[0])
        assert same(h.regrid(ws[0], Xs), native), (sname, wname)
        assert same(h.regrid(w[0], Xs), native) and same(h.regrid(ws[0], X), native), (sname, wname)
        assert same(h.regrid(ws, Xs, mean_polar=True), h.regrid(w, X, mean_polar=True)), (sname, wname)
        assert same(h.regrid(1.0, Xs[0].reshape(A.jm, A.im)), h.regrid(1.0, X[0].reshape(A.jm, A.im))), sname
        with pytest.raises(KeyError):
            _code(Xs.dtype)
    with pytest.raises(KeyError):
        import torch
        h.regrid_shape(1, None, torch.float16)
