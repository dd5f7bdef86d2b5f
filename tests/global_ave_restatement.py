"""Plain-Python restatement of the three library functions behind GCMRegridder_ModelE::global_AvE, line by line:
compute_EOpvAOp_merged and squash_ECs (slib/icebin/modele/merge_topo.cpp:375-527) and _compute_AAmvEAm_EIGEN
(slib/icebin/modele/topo.cpp:242-347), in the canonical order of DESIGN.md 16 (the rules of tests/modele_restatement.py):

  * one triplet stream in SPARSE indices, numbered first-seen and summed as setFromTriplets sums it;
  * M = diag(lead) * AAmvAOm * diag(EOmvAOms) * AOmvEOm * diag(EAmvEOms) * EOmvEAm, left-associated, each operand rounded
    before it is used: X1 = diag(lead) * AAmvAOm, X2 = X1 * diag(EOmvAOms), P1 = X2 * AOmvEOm, P2 = P1 * diag(EAmvEOms),
    M = P2 * EOmvEAm; every product sums its terms over ascending dense inner index, the first assigned.

The sheets' EvA come from the oracle (oracle/oracle.py: Regridder.matrix_d), the Hntr stream from a triplets function
(tests/test_gpu_hntr_matrix.py: triplets_ref).  Every scalar operation is one IEEE double operation on Python floats."""
import numpy as np

from modele_restatement import from_triplets, make_hntrA, product, recip, scaled_matvec, sums, transpose

UI_LOCALICE, UI_GLOBALICE = 1, 2            # modele/grids.hpp:44-46


class Numbering:
    """spsparse::SparseSet: dense ids handed out first-seen, behind the keys the set holds already."""

    def __init__(self, keys=()):
        self.keys = [int(k) for k in keys]
        self.inv = {k: d for d, k in enumerate(self.keys)}

    def add(self, k):
        if k not in self.inv:
            self.inv[k] = len(self.keys)
            self.keys.append(k)
        return self.inv[k]


def weighted(nrow, ncol, rows, cols, vals):
    M = from_triplets(nrow, rows, cols, vals)
    wM, Mw = sums(M, ncol)
    return M, wM, Mw


def change_nhc(strides, nhc):
    """indexingHC_change_nhc (:364-372) on (stride_A, stride_HC): the class-slowest order keeps its strides."""
    return strides if strides[1] >= strides[0] else (nhc, 1)


def split(key, strides):
    sA, sHC = strides
    if sHC >= sA:
        return (key % sHC) // sA, key // sHC
    return key // sA, (key % sA) // sHC


def merged(orc, sheets, nO, nhc_local, hcdefs_local, base=None, use_global_ice=True, use_local_ice=True, squash_ecs=False,
           dimAOp=(), strides_base=None):
    """compute_EOpvAOp_merged (:375-466).  sheets: [(oracle Regridder, elevmaskI)] in sheet order; base: None or
    (hcdefs_base, (iE, iO, val), shape) in sparse indices, the order of the arrays being the order of the stream; dimAOp: the keys
    the caller's set holds already.  Returns dict(M rows, wM, Mw, dims [dimEOp, dimAOp], extents, offsetE, hcdefs, underice,
    strides)."""
    use_global_ice = use_global_ice and base is not None
    kE, kA, v = [], [], []
    hcdefs, underice = [], []
    if use_local_ice:
        for rg, em in sheets:
            dE, dA = orc.SparseSet(), orc.SparseSet()
            w = rg.matrix_d("EvA", em, dims=(dE, dA), scale=False, correctA=False)
            tsE, tsA = dE.to_sparse().tolist(), dA.to_sparse().tolist()
            order = np.lexsort((w.row, w.col))          # begin(M)...end(M) of a column-major matrix
            for r, c, x in zip(w.row[order].tolist(), w.col[order].tolist(), w.val[order].tolist()):
                kE.append(tsE[r]); kA.append(tsA[c]); v.append(x)
        if sheets:
            hcdefs += [float(h) for h in hcdefs_local]
            underice += [UI_LOCALICE] * nhc_local
    offsetE = 0
    extents = [nO * (nhc_local if sheets else 0), nO]   # (the reference leaves 0 here without global ice: DESIGN.md 16)
    if use_global_ice:
        hc_b, (iE, iO, val), shape = base
        offsetE = nO * (nhc_local if sheets else 0)
        for e, o, x in zip(np.asarray(iE).tolist(), np.asarray(iO).tolist(), np.asarray(val, np.float64).tolist()):
            kE.append(e + offsetE); kA.append(o); v.append(x)
        hcdefs += [float(h) for h in hc_b]
        underice += [UI_GLOBALICE] * len(hc_b)
        extents = [offsetE + int(shape[0]), int(shape[1])]
    nE, nA = Numbering(), Numbering(dimAOp)
    rows, cols = [], []
    for e, a in zip(kE, kA):                            # one entry at a time: {ADD_DENSE, ADD_DENSE}
        rows.append(nE.add(e)); cols.append(nA.add(a))
    M, wM, Mw = weighted(len(nE.keys), len(nA.keys), rows, cols, v)
    strides = change_nhc(strides_base if strides_base is not None else (1, nO), len(hcdefs))
    res = dict(M=M, wM=wM, Mw=Mw, dims=[nE.keys, nA.keys], extents=extents, offsetE=offsetE, hcdefs=hcdefs, underice=underice,
               strides=strides)
    return squash(res) if squash_ecs else res


def squash(res0):
    """squash_ECs (:470-527), in Python's unbounded integers (the reference uses int)."""
    hc1 = sorted(set(res0["hcdefs"]))
    to_new = [hc1.index(h) for h in res0["hcdefs"]]
    s0, s1 = res0["strides"], change_nhc(res0["strides"], len(hc1))
    nE = Numbering()
    rows, cols, v = [], [], []
    keysE0 = res0["dims"][0]
    nA = len(res0["dims"][1])
    for c, col in enumerate(transpose(res0["M"], nA)):  # column-major visit
        for r, x in col:
            iO, ihc0 = split(keysE0[r], s0)
            rows.append(nE.add(iO * s1[0] + to_new[ihc0] * s1[1])); cols.append(c); v.append(x)
    M, wM, Mw = weighted(len(nE.keys), nA, rows, cols, v)
    return dict(M=M, wM=wM, Mw=Mw, dims=[nE.keys, res0["dims"][1]], extents=[res0["extents"][1] * len(hc1), res0["extents"][1]],
                offsetE=res0["offsetE"], hcdefs=hc1, underice=[UI_GLOBALICE] * len(hc1), strides=s1)


def AAmvEAm(res, hspecO, eq_rad, foceanAOp, foceanAOm, triplets, scale=True, nhc=None, stridesO=None, stridesA=None, dimAAm=(),
            dimEAm=(), parts=None):
    """_compute_AAmvEAm_EIGEN (topo.cpp:242-347) on a result of merged().  nhc / strides default to the offline tools' choice:
    len(merged hcdefs) on both indexings.  parts: a dict that receives wAOm, wEOm (the invariants' witnesses)."""
    hspecA = make_hntrA(hspecO)
    nO, nA = hspecO.size, hspecA.size
    nhc = len(res["hcdefs"]) if nhc is None else nhc
    sO = res["strides"] if stridesO is None else stridesO
    sA = ((1, nA) if sO[1] >= sO[0] else (nhc, 1)) if stridesA is None else stridesA
    fp, fm = np.asarray(foceanAOp, np.float64).tolist(), np.asarray(foceanAOm, np.float64).tolist()
    keysE, keysA = res["dims"]
    wAOp = res["Mw"]                                    # sum(EOpvAOp, 1, '+')
    # compute_wAOm (topo.cpp:84-109)
    dimAOm = [s for s in keysA if fm[s] == 0]
    toAOm = {s: k for k, s in enumerate(dimAOm)}
    wAOm = [0.] * len(dimAOm)
    for d, s in enumerate(keysA):                       # scaled_AOmvAOp (topo.cpp:50-81)
        fcont_p, fcont_m = 1.0 - fp[s], 1.0 - fm[s]
        if fcont_m == 0.0:
            continue
        if fcont_m != 1.0:
            raise ValueError("fcont_m[%d] = %g, must be 0 or 1" % (s, fcont_m))
        if fcont_p == 0.0:
            continue
        wAOm[toAOm[s]] = 0. + (1. / fcont_p) * wAOp[d]
    # AAmvAOm (:286-295): Hntr's overlap clipped by dimAOm, {TO_DENSE_IGNORE_MISSING, ADD_DENSE}, transposed
    mask = np.zeros(nO, bool)
    mask[np.asarray(dimAOm, np.int64)] = True
    iO_s, iA_s, ov = triplets(hspecO, hspecA, "overlap", eq_rad, mask=mask)
    iO_s, iA_s, ov = iO_s.tolist(), iA_s.tolist(), ov.tolist()
    nAA = Numbering(dimAAm)
    tr, tc, tv = [], [], []
    for o, a, x in zip(iO_s, iA_s, ov):
        d = toAOm.get(o)
        if d is None:
            continue
        tr.append(d); tc.append(nAA.add(a)); tv.append(x)
    AOmvAAm = from_triplets(len(dimAOm), tr, tc, tv)
    nAAm = len(nAA.keys)
    rs, cs = sums(AOmvAAm, nAAm)
    AAmvAOms, sAAmvAOm = recip(rs), recip(cs)           # sum(AAmvAOm, 1, '-'), sum(AAmvAOm, 0, '-')
    AAmvAOm = transpose(AOmvAAm, nAAm)
    wAAm = scaled_matvec(AAmvAOm, AAmvAOms, wAOm)
    # compute_EOmvAOm_unscaled (topo.cpp:211-240) on the GIVEN EOpvAOp: column-major visit
    nEO = Numbering()
    tr, tc, tv = [], [], []
    for c, col in enumerate(transpose(res["M"], len(keysA))):
        k = toAOm.get(keysA[c])
        if k is None:
            continue
        for r, x in col:
            tr.append(nEO.add(keysE[r])); tc.append(k); tv.append(x)
    EOmvAOm = from_triplets(len(nEO.keys), tr, tc, tv)
    EOmvAOms = recip(sums(EOmvAOm, len(dimAOm))[1])
    wEOm = scaled_matvec(EOmvAOm, EOmvAOms, wAOm)
    # raw_EOvEA (topo.cpp:112-204)
    nEA = Numbering(dimEAm)
    tr, tc, tv = [], [], []
    for o, a, x in zip(iO_s, iA_s, ov):
        if abs(x) < 1e-8:
            raise ValueError("Found a stray overlap; what should we do about it?")
        for ihc in range(nhc):
            d = nEO.inv.get(o * sO[0] + ihc * sO[1])
            if d is None or wEOm[d] == 0:
                continue
            tr.append(d); tc.append(nEA.add(a * sA[0] + ihc * sA[1])); tv.append(wEOm[d])
    EOmvEAm = from_triplets(len(nEO.keys), tr, tc, tv)
    nEAm = len(nEA.keys)
    EAmvEOms = recip(sums(EOmvEAm, nEAm)[0])            # sum(EOmvEAm, 0, '-')
    wEAm = scaled_matvec(transpose(EOmvEAm, nEAm), EAmvEOms, wEOm)
    # the composition (:326-343)
    lead = sAAmvAOm if scale else [w * s for w, s in zip(wAAm, sAAmvAOm)]
    X1 = [[(k, lead[r] * x) for k, x in row] for r, row in enumerate(AAmvAOm)]
    X2 = [[(k, x * EOmvAOms[k]) for k, x in row] for row in X1]
    P1 = product(X2, transpose(EOmvAOm, len(dimAOm)))
    P2 = [[(k, x * EAmvEOms[k]) for k, x in row] for row in P1]
    M = product(P2, EOmvEAm)
    if parts is not None:
        parts.update(wAOm=wAOm, wEOm=wEOm, dimAOm=dimAOm, dimEOm=nEO.keys, P1=P1)
    return dict(M=M, wM=np.asarray(wAAm, np.float64), Mw=np.asarray(wEAm, np.float64),
                dims=[np.asarray(nAA.keys, np.int64), np.asarray(nEA.keys, np.int64)], extents=[nA, nA * nhc], conservative=False,
                scaled=bool(scale))
