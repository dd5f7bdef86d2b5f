"""Hntr on the GPU against an exact numpy restatement of the reference's regrid loop (hntr.hpp:260-296 matrix,
RegridAccum :322-338, mean_polar :404-423).  The restatement runs across all B cells at once but keeps every cell's
term order (JA outer, IAREV inner) and the reference's expressions, so the comparison is bitwise."""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hntr import GRIDS, PAIRS  # noqa: E402

DATMIS = -1e30


def regrid_ref(Bspec, Aspec, WTA, A, datmis, mean_polar=False, wtm=1., wtb=0.):
    """B and the per-cell WEIGHT of Hntr::regrid, one field; the partition comes from ibh_hntr_partition (bitwise the
    independent restatement of tests/test_hntr.py)."""
    from icebin_amd.hntr import partition
    p = partition(Bspec, Aspec)
    imA, jmA = Aspec.im, Aspec.jm
    W2, A2 = np.asarray(WTA, np.float64).reshape(jmA, imA), np.asarray(A, np.float64).reshape(jmA, imA)
    JMIN, JMAX, GMIN, GMAX, SINA = p["JMIN"], p["JMAX"], p["GMIN"], p["GMAX"], p["SINA"]
    IMIN, IMAX, FMIN, FMAX = p["IMIN"], p["IMAX"], p["FMIN"], p["FMAX"]
    WEIGHT = np.zeros((Bspec.jm, Bspec.im))
    VALUE = np.zeros((Bspec.jm, Bspec.im))
    with np.errstate(all="ignore"):
        for r in range(int((JMAX - JMIN).max()) + 1):
            JA = JMIN + r
            rv = JA <= JMAX
            JA = np.minimum(JA, JMAX)
            G = SINA[JA] - SINA[JA - 1]
            G = np.where(JA == JMIN, G - GMIN, G)
            G = np.where(JA == JMAX, G - GMAX, G)
            for k in range(int((IMAX - IMIN).max()) + 1):
                IAREV = IMIN + k
                cv = IAREV <= IMAX
                IAREV = np.minimum(IAREV, IMAX)
                IA = (IAREV - 1) % imA
                F = np.ones(Bspec.im)
                F = np.where(IAREV == IMIN, F - FMIN, F)
                F = np.where(IAREV == IMAX, F - FMAX, F)
                FG = F[None, :] * G[:, None]
                wta = wtm * W2[np.ix_(JA - 1, IA)] + wtb
                wt = FG * wta
                valid = rv[:, None] & cv[None, :]
                WEIGHT = np.where(valid, WEIGHT + wt, WEIGHT)
                VALUE = np.where(valid, VALUE + wt * A2[np.ix_(JA - 1, IA)], VALUE)
        B = np.where(WEIGHT == 0, datmis, VALUE / WEIGHT)
        if mean_polar:
            for JB in (0, Bspec.jm - 1):
                BMEAN, n, s = datmis, 0., 0.
                for IB in range(Bspec.im):
                    if B[JB, IB] == datmis:
                        break
                    n += 1
                    s += B[JB, IB]
                else:
                    if n != 0:
                        BMEAN = s / n
                B[JB, :] = BMEAN
    return B.reshape(-1), WEIGHT.reshape(-1)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def fields(spec, nvar, seed, zeros=True):
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(spec.jm), np.arange(spec.im), indexing="ij")
    A = np.stack([np.sin(0.3 * ii * (1 + k) / spec.im * 8) * np.cos(2.0 * jj / spec.jm * (k + 1)) + rng.standard_normal(ii.shape)
                  for k in range(nvar)]).reshape(nvar, -1)
    W = rng.uniform(0.1, 1.0, (nvar, spec.size))
    if zeros:      # a block of zero weight, and the whole southern polar row
        z = ((ii >= spec.im // 4) & (ii < spec.im // 2) & (jj >= spec.jm // 4) & (jj < spec.jm // 2)) | (jj == 0)
        W[:, z.reshape(-1)] = 0.
    return W, A


def spec(name):
    from icebin_amd import HntrSpec
    return HntrSpec(*GRIDS[name])


@pytest.mark.parametrize("b,a", PAIRS + [(a, b) for b, a in PAIRS], ids=lambda x: x)
def test_bitwise_on_grid_pairs(b, a):
    from icebin_amd import Hntr
    B, A = spec(b), spec(a)
    h = Hntr(17.17, B, A, DATMIS)
    W, X = fields(A, 3, 1)
    # one weight shared by three fields
    got = h.regrid(W[0], X)
    for k in range(3):
        ref, wref = regrid_ref(B, A, W[0], X[k], DATMIS)
        assert same(got[k], ref), (b, a, k)
    # DATMIS exactly where the covered weight is 0
    assert np.array_equal(got[0] == DATMIS, wref == 0)
    # one weight per field; and the weight 1 - WTA (wtm=-1, wtb=1)
    got = h.regrid(W[:2], X[:2])
    got_m = h.regrid(W[1], X[1], wtm=-1., wtb=1.)
    for k in range(2):
        assert same(got[k], regrid_ref(B, A, W[k], X[k], DATMIS)[0]), (b, a, k)
    assert same(got_m, regrid_ref(B, A, W[1], X[1], DATMIS, wtm=-1., wtb=1.)[0])


@pytest.mark.parametrize("b,a", [("72x46", "360x180"), ("144x90_east", "288x180"), ("4x2", "8x4")], ids=lambda x: x)
def test_mean_polar_and_nan_datmis(b, a):
    from icebin_amd import Hntr
    B, A = spec(b), spec(a)
    from icebin_amd.hntr import partition
    W, X = fields(A, 1, 2)
    W.reshape(A.jm, A.im)[:partition(B, A)["JMAX"][0], :] = 0.      # no weight under B's southern polar row: DATMIS there
    for datmis in (DATMIS, float("nan")):
        h = Hntr(17.17, B, A, datmis)
        for mp in (False, True):
            got = h.regrid(W[0], X[0], mean_polar=mp)
            ref, wref = regrid_ref(B, A, W[0], X[0], datmis, mean_polar=mp)
            assert same(got, ref), (datmis, mp)
        got = h.regrid(W[0], X[0], mean_polar=True)
        # south row: a DATMIS cell stops the mean, the row stays DATMIS (a NaN DATMIS never compares equal: NaNs average in)
        assert np.all(np.isnan(got[:B.im])) if math.isnan(datmis) else np.all(got[:B.im] == datmis)
        # north row: no DATMIS, one mean
        north = got[-B.im:]
        assert np.all(north == north[0]) and np.isfinite(north[0])


def test_mean_polar_on_one_row_is_einval():
    from icebin_amd import Hntr, HntrSpec, _capi
    h = Hntr(17.17, HntrSpec(8, 1, 0., 10800.), spec("360x180"), DATMIS)
    W, X = fields(spec("360x180"), 1, 3)
    assert h.regrid(W[0], X[0]).shape == (8,)
    with pytest.raises(_capi.IcebinHipError, match="mean_polar needs jmB >= 2") as ei:
        h.regrid(W[0], X[0], mean_polar=True)
    assert ei.value.code == _capi.IBH_EINVAL


@pytest.mark.parametrize("Bdef", [(720, 360, 0., 30.), (360, 180, 0., 60.)], ids=["2min_to_halfdeg", "2min_to_1deg"])
def test_bitwise_from_2_minutes(Bdef):
    from icebin_amd import Hntr, HntrSpec
    A, B = HntrSpec(10800, 5400, 0., 2.), HntrSpec(*Bdef)
    h = Hntr(17.17, B, A, DATMIS)
    W, X = fields(A, 2, 4)
    got = h.regrid(W[0], X)
    for k in range(2):
        ref, wref = regrid_ref(B, A, W[0], X[k], DATMIS)
        assert same(got[k], ref), k
    got = h.regrid(W, X, mean_polar=True)
    assert same(got[1], regrid_ref(B, A, W[1], X[1], DATMIS, mean_polar=True)[0])


def test_batching_is_bitwise_single_launches_and_gaps_stay_untouched():
    import torch
    from icebin_amd import Hntr
    A, B = spec("360x180"), spec("72x46_east")
    h = Hntr(17.17, B, A, DATMIS)
    W, X = fields(A, 64, 5)
    dev = torch.device("cuda:0")
    singles = [h.regrid_device(torch.from_numpy(W[0]).to(dev), torch.from_numpy(X[k:k + 1]).to(dev)).cpu().numpy()[0] for k in range(64)]
    singles_pf = [h.regrid(W[k], X[k]) for k in range(7)]
    lda, ldb = A.size + 37, B.size + 11
    for nvar in (1, 7, 64):
        Ap = torch.full((nvar, lda), float("nan"), dtype=torch.float64, device=dev)
        Ap[:, :A.size] = torch.from_numpy(X[:nvar]).to(dev)
        Bp = torch.full((nvar, ldb), 12345.5, dtype=torch.float64, device=dev)
        out = h.regrid_device(torch.from_numpy(W[0]).to(dev), Ap[:, :A.size], out=Bp[:, :B.size])
        torch.cuda.synchronize()
        got = Bp.cpu().numpy()
        for k in range(nvar):
            assert same(got[k, :B.size], singles[k]), (nvar, k)
        assert np.all(got[:, B.size:] == 12345.5), nvar
        assert out.data_ptr() == Bp.data_ptr()
    # per-field weights in one launch, padded planes
    Wp = torch.full((7, lda), float("nan"), dtype=torch.float64, device=dev)
    Wp[:, :A.size] = torch.from_numpy(W[:7]).to(dev)
    Ap = torch.full((7, lda), float("nan"), dtype=torch.float64, device=dev)
    Ap[:, :A.size] = torch.from_numpy(X[:7]).to(dev)
    got = h.regrid_device(Wp[:, :A.size], Ap[:, :A.size]).cpu().numpy()
    for k in range(7):
        assert same(got[k], singles_pf[k]) and same(got[k], regrid_ref(B, A, W[k], X[k], DATMIS)[0]), k
    # run to run
    again = h.regrid_device(torch.from_numpy(W[0]).to(dev), torch.from_numpy(X).to(dev)).cpu().numpy()
    assert all(same(again[k], singles[k]) for k in range(64))


@pytest.mark.parametrize("b,a", [("72x46_east", "360x180"), ("288x180", "144x90"), ("91x45", "100x50")], ids=lambda x: x)
def test_invariants(b, a):
    from icebin_amd import Hntr
    from icebin_amd.hntr import partition
    B, A = spec(b), spec(a)
    h = Hntr(17.17, B, A, DATMIS)
    W, X = fields(A, 1, 6)
    got = h.regrid(W[0], X[0])
    ref, WEIGHT = regrid_ref(B, A, W[0], X[0], DATMIS)
    assert same(got, ref)
    # conservation: the weighted integral over B is the weighted integral over A (F summed over B columns is 1)
    p = partition(B, A)
    dsin = np.diff(p["SINA"])
    lhs = math.fsum((WEIGHT * np.where(WEIGHT == 0, 0., got)).tolist())
    rhs = math.fsum((W[0].reshape(A.jm, A.im) * X[0].reshape(A.jm, A.im) * dsin[:, None]).reshape(-1).tolist())
    assert abs(lhs - rhs) <= 1e-13 * abs(rhs), (lhs, rhs)
    # a constant field comes back (the two chains round independently, so to 1e-13, not exactly)
    c = h.regrid(W[0], np.full(A.size, 3.25))
    ok = c != DATMIS
    assert ok.sum() > 0 and np.max(np.abs(c[ok] - 3.25)) <= 1e-13 * 3.25


def test_the_other_surfaces():
    import torch
    from icebin_amd import Hntr, HntrSpec
    from icebin_amd.cython.build_ext import build
    build()
    sys.path.insert(0, os.path.join(ROOT, "icebin_amd", "cython"))
    import icebin
    B, A = spec("72x46_east"), spec("360x180")
    W, X = fields(A, 1, 7)
    ref = regrid_ref(B, A, W[0], X[0], DATMIS, mean_polar=True)[0]
    # Cython: the reference's float32 rounding of offi / dlat / DATMIS (all exact here) and regrid(WTA, A, mean_polar)
    hc = icebin.Hntr(17.17, icebin.HntrSpec(*GRIDS["72x46_east"]), icebin.HntrSpec(*GRIDS["360x180"]), DATMIS)
    got = hc.regrid(W[0], X[0], True)
    assert same(got, regrid_ref(B, A, W[0], X[0], float(np.float32(DATMIS)), mean_polar=True)[0])
    with pytest.raises(ValueError):
        hc.regrid(W[0][:10], X[0], False)
    # Python: (jm, im) in, (jm, im) out; torch tensors on the device
    h = Hntr(17.17, B, A, DATMIS)
    got2 = h.regrid(W[0].reshape(A.jm, A.im), X[0].reshape(A.jm, A.im), mean_polar=True)
    assert got2.shape == (B.jm, B.im) and same(got2.reshape(-1), ref)
    dev = torch.device("cuda:0")
    got3 = h.regrid_device(torch.from_numpy(W[0]).to(dev), torch.from_numpy(X[:1]).to(dev), mean_polar=True)
    assert same(got3.cpu().numpy()[0], ref)
    with pytest.raises(TypeError):
        HntrSpec(72, 46)                            # the reference's four arguments, no defaults


def test_device_strides_refuse_broadcast_planes():
    import torch
    from icebin_amd import Hntr, _capi
    A, B = spec("360x180"), spec("72x46_east")
    h = Hntr(17.17, B, A, DATMIS)
    W, X = fields(A, 3, 8)
    dev = torch.device("cuda:0")
    dW, dX = torch.from_numpy(W).to(dev), torch.from_numpy(X).to(dev)
    # a weight broadcast to every field is the shared weight
    got = h.regrid_device(dW[0].expand(3, -1), dX).cpu().numpy()
    assert all(same(got[k], regrid_ref(B, A, W[0], X[k], DATMIS)[0]) for k in range(3))
    # a broadcast A or out would read or write past its one plane: refused, and out is left as it was
    out = torch.full((3, B.size), 7.0, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="A planes overlap"):
        h.regrid_device(dW[0], dX[0].expand(3, -1), out=out)
    with pytest.raises(ValueError, match="out planes overlap"):
        h.regrid_device(dW[0], dX, out=torch.zeros(B.size, dtype=torch.float64, device=dev).expand(3, -1))
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)
    # the C-ABI refuses the same strides by itself
    rc = _capi.lib().ibh_hntr_regrid_device(h._h, dW.data_ptr(), 0, dX.data_ptr(), 3, 0, out.data_ptr(), B.size, 0, 1.0, 0.0, None)
    assert rc == _capi.IBH_EINVAL
    rc = _capi.lib().ibh_hntr_regrid_device(h._h, dW.data_ptr(), 5, dX.data_ptr(), 3, A.size, out.data_ptr(), B.size, 0, 1.0, 0.0, None)
    assert rc == _capi.IBH_EINVAL
