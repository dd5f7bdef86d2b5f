"""Numpy / plain-Python restatement of GCMRegridder_ModelE::regrid_matrices (slib/icebin/modele/GCMRegridder_ModelE.cpp:
92-121, 168-433) and the topo.cpp helpers it calls (:50-240), line by line, in the canonical order of DESIGN.md 15:

  * C = L * R: C(r, c) = sum_k L(r, k) * R(k, c), terms added in ascending dense k starting from the first term; each operand
    is evaluated first (diag(s) * X gives s[r] * X(r, k); (A * diag(d)) * B gives (A(i, k) * d[k]) * B(k, c));
  * y = (X * diag(d)) * w: per column k ascending, y[r] += (X(r, k) * d[k]) * w[k], from 0;
  * sum(M, dim, '+' | '-'): the column-major visit (column ascending, rows ascending inside), from 0; '-' inverts.

The O-grid matrices come from the oracle (oracle/oracle.py: Regridder.matrix_d), the Hntr stream from a triplets function
(tests/test_gpu_hntr_matrix.py: triplets_ref).  Every scalar operation is one IEEE double operation on Python floats.
A matrix is a list of rows, each a list of (column, value) with columns ascending."""
import numpy as np


def recip(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1. / np.asarray(x, np.float64)).tolist()


def from_triplets(nrow, rows, cols, vals):
    """Eigen setFromTriplets: duplicates summed in stream order, the first assigned."""
    acc = [dict() for _ in range(nrow)]
    for r, c, v in zip(rows, cols, vals):
        a = acc[r]
        a[c] = a[c] + v if c in a else v
    return [sorted(a.items()) for a in acc]


def transpose(M, ncol):
    T = [[] for _ in range(ncol)]
    for r, row in enumerate(M):
        for c, v in row:
            T[c].append((r, v))
    return T


def sums(M, ncol):
    """(sum(M, 0, '+'), sum(M, 1, '+')) of the column-major visit: row sums add over ascending columns, column sums over
    ascending rows, both from 0."""
    rs, cs = [0.] * len(M), [0.] * ncol
    for r, row in enumerate(M):
        for c, v in row:
            rs[r] = rs[r] + v
            cs[c] = cs[c] + v
    return rs, cs


def scaled_matvec(M, d, w):
    y = []
    for row in M:
        s = 0.
        for k, v in row:
            s = s + (v * d[k]) * w[k]
        y.append(s)
    return y


def product(L, R):
    out = []
    for row in L:
        acc = {}
        for k, l in row:                    # k ascending
            for c, v in R[k]:
                t = l * v
                acc[c] = acc[c] + t if c in acc else t
        out.append(sorted(acc.items()))
    return out


def rows_of(w):
    """The oracle's Weighted as a list of rows."""
    order = np.lexsort((w.col, w.row))
    M = [[] for _ in range(w.nrow)]
    for r, c, v in zip(w.row[order].tolist(), w.col[order].tolist(), w.val[order].tolist()):
        M[r].append((c, v))
    return M


def make_hntrA(hspecO):
    from icebin_amd import HntrSpec
    assert hspecO.im % 2 == 0 and hspecO.jm % 2 == 0
    return HntrSpec(hspecO.im // 2, hspecO.jm // 2, hspecO.offi * 0.5, hspecO.dlat * 2.)


class Ctx:
    """What a GCMRegridder_ModelE holds: the O-grid oracle regridder and mask, the ocean HntrSpec, the two ocean fractions."""

    def __init__(self, orc, rgO, elevmaskI, hspecO, eq_rad, foceanAOp, foceanAOm, triplets):
        self.orc, self.rgO, self.em, self.hspecO, self.eq_rad = orc, rgO, elevmaskI, hspecO, eq_rad
        self.hspecA = make_hntrA(hspecO)
        self.fp, self.fm = np.asarray(foceanAOp, np.float64).tolist(), np.asarray(foceanAOm, np.float64).tolist()
        self.triplets = triplets
        self.nO, self.nA, self.nhc = hspecO.size, self.hspecA.size, rgO.nhc
        sA, sHC = int(rgO.c.hc_stride_A), int(rgO.c.hc_stride_HC)
        self.sO = (sA, sHC)
        self.sA = (1, self.nA) if (sA, sHC) == (1, self.nO) else (self.nhc, 1)      # GCMRegridder_ModelE.cpp:451-456

    def o_matrix(self, name, dims, correctA):
        return self.rgO.matrix_d(name, self.em, dims=dims, scale=False, correctA=correctA)

    def stream(self, dimAOm):
        mask = np.zeros(self.nO, bool)
        mask[np.asarray(dimAOm, np.int64)] = True
        iO, iA, v = self.triplets(self.hspecO, self.hspecA, "overlap", self.eq_rad, mask=mask)
        return iO.tolist(), iA.tolist(), v.tolist()


def helper(cx, gridX, gridG, dimXAm, dimGp_set):
    """ComputeXAmvGp_Helper (:168-280).  dimXAm: list of sparse keys (appended to); dimGp_set: oracle SparseSet."""
    orc = cx.orc
    dimAOp = orc.SparseSet()
    AOpvIp_c = cx.o_matrix("Av" + gridG, (dimAOp, dimGp_set), True)
    wAOp = AOpvIp_c.wM.tolist()
    keysAOp = dimAOp.to_sparse().tolist()
    # compute_wAOm (topo.cpp:84-109)
    dimAOm = [s for s in keysAOp if cx.fm[s] == 0]
    toAOm = {s: k for k, s in enumerate(dimAOm)}
    wAOm = [0.] * len(dimAOm)
    for d, s in enumerate(keysAOp):             # scaled_AOmvAOp (topo.cpp:50-81)
        fcont_p, fcont_m = 1.0 - cx.fp[s], 1.0 - cx.fm[s]
        if fcont_m == 0.0:
            continue
        if fcont_m != 1.0:
            raise ValueError("fcont_m[%d] = %g, must be 0 or 1" % (s, fcont_m))
        if fcont_p == 0.0:
            continue
        wAOm[toAOm[s]] = 0. + (1. / fcont_p) * wAOp[d]
    toXAm = {s: k for k, s in enumerate(dimXAm)}

    def add_XAm(s):
        if s not in toXAm:
            toXAm[s] = len(dimXAm)
            dimXAm.append(s)
        return toXAm[s]

    sO, sA, v = cx.stream(dimAOm)
    if gridX == "E":
        dimXOp = orc.SparseSet()
        XOpvIp = cx.o_matrix("Ev" + gridG, (dimXOp, dimGp_set), False)
        dimEOp2, dimAOp2 = orc.SparseSet(), orc.SparseSet()
        EOpvAOp = cx.o_matrix("EvA", (dimEOp2, dimAOp2), False)
        kE2, kA2 = dimEOp2.to_sparse().tolist(), dimAOp2.to_sparse().tolist()
        # compute_EOmvAOm_unscaled (topo.cpp:211-240): column-major visit
        order = np.lexsort((EOpvAOp.row, EOpvAOp.col))
        dimXOm, toEOm = [], {}
        tr, tc, tv = [], [], []
        for r, c, val in zip(EOpvAOp.row[order].tolist(), EOpvAOp.col[order].tolist(), EOpvAOp.val[order].tolist()):
            k = toAOm.get(kA2[c])
            if k is None:
                continue
            s = kE2[r]
            if s not in toEOm:
                toEOm[s] = len(dimXOm)
                dimXOm.append(s)
            tr.append(toEOm[s]); tc.append(k); tv.append(val)
        EOmvAOm = from_triplets(len(dimXOm), tr, tc, tv)
        EOmvAOms = recip(sums(EOmvAOm, len(dimAOm))[1])
        wXOm = scaled_matvec(EOmvAOm, EOmvAOms, wAOm)
        # raw_EOvEA (topo.cpp:112-204)
        tr, tc, tv = [], [], []
        for iO, iA, val in zip(sO, sA, v):
            if abs(val) < 1e-8:
                raise ValueError("Found a stray overlap; what should we do about it?")
            for ihc in range(cx.nhc):
                d = toEOm.get(iO * cx.sO[0] + ihc * cx.sO[1])
                if d is None or wXOm[d] == 0:
                    continue
                tr.append(d); tc.append(add_XAm(iA * cx.sA[0] + ihc * cx.sA[1])); tv.append(wXOm[d])
        toXOm = toEOm
    else:
        dimXOp = dimAOp
        XOpvIp = cx.o_matrix("Av" + gridG, (dimAOp, dimGp_set), False)
        dimXOm, toXOm, wXOm = dimAOm, toAOm, wAOm
        tr, tc, tv = [], [], []
        for iO, iA, val in zip(sO, sA, v):      # {TO_DENSE_IGNORE_MISSING, ADD_DENSE}
            d = toAOm.get(iO)
            if d is None:
                continue
            tr.append(d); tc.append(add_XAm(iA)); tv.append(val)
    XOmvXAm = from_triplets(len(dimXOm), tr, tc, tv)        # the reference's XAmvXOm, by its columns
    nXAm = len(dimXAm)
    rs, cs = sums(XOmvXAm, nXAm)
    XAmvXOms, sXAm = recip(rs), recip(cs)       # sum(XAmvXOm, 1, '-'), sum(XAmvXOm, 0, '-')
    XAmvXOm = transpose(XOmvXAm, nXAm)
    wXAm = scaled_matvec(XAmvXOm, XAmvXOms, wXOm)
    return dict(dimXOp=dimXOp, dimXOm=dimXOm, toXOm=toXOm, XOpvIp=XOpvIp, XOmvXAm=XOmvXAm, XAmvXOm=XAmvXOm, XAmvXOms=XAmvXOms,
                sXAm=sXAm, wXAm=wXAm)


SPECS = {"AvI": (0, "A", "I"), "EvI": (0, "E", "I"), "AvX": (0, "A", "X"), "EvX": (0, "E", "X"),
         "IvA": (1, "A", "I"), "IvE": (1, "E", "I"), "XvA": (1, "A", "X"), "XvE": (1, "E", "X")}


def regrid_matrix(cx, name, scale, dim0=(), dim1=()):
    """compute_XAmvGp (:318-368) / compute_GpvXAm (:379-433).  dim0 / dim1: the keys the caller's sets hold already.  Returns
    dict(M = list of rows, wM, Mw, dims = [keys, keys], conservative, scaled)."""
    kind, gridX, gridG = SPECS[name]
    dimXAm = [int(s) for s in (dim0 if kind == 0 else dim1)]
    dimGp = cx.orc.SparseSet(-1, np.asarray(dim1 if kind == 0 else dim0, np.int64))
    h = helper(cx, gridX, gridG, dimXAm, dimGp)
    XOpvIp = h["XOpvIp"]
    keysXOp = h["dimXOp"].to_sparse().tolist()
    if kind == 0:
        sXOpvIp = recip(XOpvIp.wM)
        rowsXOp = rows_of(XOpvIp)
        src = {s: d for d, s in enumerate(keysXOp)}
        R = []                                  # crop_mvp(dimXOm, dimXOp, 0, diag(sXOpvIp) * XOpvIp.M)
        for s in h["dimXOm"]:
            p = src.get(s)
            R.append([] if p is None else [(c, sXOpvIp[p] * v) for c, v in rowsXOp[p]])
        ls = h["sXAm"] if scale else [w * s for w, s in zip(h["wXAm"], h["sXAm"])]
        L = [[(k, ls[r] * v) for k, v in row] for r, row in enumerate(h["XAmvXOm"])]
        M = product(L, R)
        wM, Mw = h["wXAm"], XOpvIp.Mw.tolist()
        dims = [dimXAm, dimGp.to_sparse().tolist()]
    else:
        IpvXOp = cx.o_matrix(gridG + "v" + gridX, (dimGp, h["dimXOp"]), False)
        assert h["dimXOp"].to_sparse().tolist() == keysXOp
        sIpvXOp = recip(IpvXOp.wM)
        d = h["XAmvXOms"]
        L = []                                  # crop_mvp(dimXOm, dimXOp, 1, [diag(sIpvXOp) *] IpvXOp.M) * diag(sXOmvXAm)
        for i, row in enumerate(rows_of(IpvXOp)):
            out = []
            for c, v in row:
                k = h["toXOm"].get(keysXOp[c])
                if k is None:
                    continue
                out.append((k, ((sIpvXOp[i] * v) if scale else v) * d[k]))
            L.append(sorted(out))
        M = product(L, h["XOmvXAm"])
        wM, Mw = XOpvIp.Mw.tolist(), h["wXAm"]
        dims = [dimGp.to_sparse().tolist(), dimXAm]
    return dict(M=M, wM=np.asarray(wM, np.float64), Mw=np.asarray(Mw, np.float64), dims=[np.asarray(x, np.int64) for x in dims],
                conservative=False, scaled=bool(scale))


def csr(res):
    M = res["M"]
    rowptr = np.zeros(len(M) + 1, np.int32)
    rowptr[1:] = np.cumsum([len(r) for r in M])
    col = np.asarray([c for r in M for c, _ in r], np.int32)
    val = np.asarray([v for r in M for _, v in r], np.float64)
    return rowptr, col, val


def hntr_grids(hspecG, hspecI, elevmaskI, hcdefs, eq_rad, interp_style=0, unit_area=False):
    """The arrays of new_gcmA_standard's regridder (global_ec.cpp:384-432), restated on the host, in the oracle's layout.
    unit_area: native = projected = 1 instead of make_abbr_grid's areas (a grid with an odd jm has no grid spec; the areas
    only enter through correctA, as their ratio)."""
    from icebin_amd import global_ec
    from global_ec_ref import exgrid_ref
    from test_gpu_hntr_matrix import triplets_ref
    iB, iA, v = triplets_ref(hspecG, hspecI, "overlap", eq_rad)
    idx, area, dimA, _ = exgrid_ref(iB, iA, v, elevmaskI)
    nat = np.ones(len(dimA)) if unit_area else global_ec.native_area(hspecG, dimA, eq_rad)
    return dict(nA=hspecG.size, nI=hspecI.size, nhc=len(hcdefs), hcdefs=np.asarray(hcdefs, np.float64), hc_stride_A=1,
                hc_stride_HC=hspecG.size, ex_indices=idx, ex_area=area, A_to_sparse=dimA, A_native_area=nat, A_proj_area=nat,
                interp_style=interp_style)
