"""Plain-Python restatement of the two library functions behind GCMCoupler_ModelE::update_topo, line by line: merge_topoO
(slib/icebin/modele/merge_topo.cpp:84-360) and make_topoA (slib/icebin/modele/topo.cpp:538-888).  Every scalar operation is
one IEEE double operation on Python floats, in the order the reference writes it; the loops are the reference's loops.

What it stands on: the oracle's AvI (oracle/oracle.py: Regridder.matrix_d), applied as Eigen applies a column-major matrix
(columns ascending, y[row] += val * x[col], from 0); Hntr::regrid as tests/test_gpu_hntr.py restates it (regrid_ref) and the
stream of Hntr::scaled_regrid_matrix as tests/test_gpu_hntr_matrix.py does (triplets_ref)."""
import math

import numpy as np

NaN = float("nan")
DBL_MAX = float(np.finfo(np.float64).max)       # std::numeric_limits<double>::max()
DBL_MIN = float(np.finfo(np.float64).tiny)      # std::numeric_limits<double>::min(): the smallest positive NORMAL number
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
UI_UNUSED, UI_LOCALICE, UI_GLOBALICE, UI_VGHOST, UI_HGHOST, UI_SEALAND = 0, 1, 2, 3, 4, 5   # modele/grids.hpp:44-49

MERGE_PLANES = ("foceanOp", "fgiceOp", "zatmoOp", "foceanOm", "flakeOm", "fgrndOm", "fgiceOm", "zatmoOm", "zicetopO")
TOPOA_PLANES = ("focean", "flake", "fgrnd", "fgice", "zatmo", "zlake", "zicetop", "zland_min", "zland_max")


def cmin(a, b):
    """std::min(a, b)"""
    return b if b < a else a


def cmax(a, b):
    """std::max(a, b)"""
    return b if a < b else a


def apply_colmajor(w, x):
    """Eigen's M * x for a column-major sparse M: columns ascending, the rows of a column ascending."""
    y = [0.0] * w.nrow
    order = np.lexsort((w.row, w.col))
    for r, c, v in zip(w.row[order].tolist(), w.col[order].tolist(), w.val[order].tolist()):
        y[r] += v * x[c]
    return y


def sheet_elevO(orc, rg, em, scale, correctA):
    """get_sheet_elevO (:36-69): (dimO's to_sparse, the Weighted OvI, elev_areaO)."""
    dimO, dimI = orc.SparseSet(), orc.SparseSet(rg.nI, np.arange(rg.nI))
    w = rg.matrix_d("AvI", em, dims=(dimO, dimI), scale=scale, correctA=correctA)
    assert w.ncol == rg.nI and np.array_equal(w.dims[1], np.arange(rg.nI))      # dense and sparse are the same for the ice grid
    return dimO.to_sparse().tolist(), w, apply_colmajor(w, np.asarray(em, np.float64).tolist())


def sanity_nonan(label, var, im, jm, errors):
    for j in range(jm):
        for i in range(im):
            if math.isnan(var[j * im + i]):
                errors.append("(%d, %d): %s is NaN" % (i + 1, j + 1, label))


def sanity_check_land_fractions(focean, flake, fgrnd, fgice, im, jm, errors):
    for j in range(jm):
        for i in range(im):
            c = j * im + i
            all_frac = focean[c] + fgrnd[c] + flake[c] + fgice[c]
            if abs(all_frac - 1.0) > 1.e-13:
                errors.append("(%d, %d): FOCEAN(%g) + FGRND(%g) + FLAKE(%g) + FGICE(%g)  = %g" % (i + 1, j + 1, focean[c], fgrnd[c], flake[c],
                                                                                                 fgice[c], all_frac))


def single_cell_oceans(p, IM, JM, one_shot=False):
    """(:291-313) in place on the planes p; one_shot: every cell reads the foceanOm the pass started with."""
    foceanOm = list(p["foceanOm"]) if one_shot else p["foceanOm"]
    for j in range(JM):
        for i in range(IM):
            if i == 0 or i == IM - 1 or j == 0 or j == JM - 1:
                continue
            iO = j * IM + i
            if (foceanOm[iO - IM] == 0. and foceanOm[iO + IM] == 0. and foceanOm[iO - 1] == 0. and foceanOm[iO + 1] == 0.
                    and foceanOm[iO] == 1. and p["foceanOp"][iO] != 1.):
                denom = 1. - p["foceanOp"][iO]
                fact = 1. / denom
                p["foceanOm"][iO] = 0.0
                p["fgiceOm"][iO] = p["fgiceOp"][iO] * fact
                p["fgrndOm"][iO] = 1.0 - p["fgiceOm"][iO] - p["flakeOm"][iO]
                p["zatmoOm"][iO] = p["zatmoOp"][iO] * fact


def merge_topoO(orc, sheets, native_area, planes, IM, JM, one_shot=False, sums=None):
    """merge_topoO (:142-336).  sheets: [(oracle Regridder, emI_land, emI_ice)] in sheet order; native_area[iO]: the O cell's
    native area by SPARSE index; planes: dict of the nine in/out planes (flat, iO = j * IM + i; not changed).  sums: a list that
    receives every sheet's (elev_areaO of the ice build, of the land build) with the matrices, for the tests that measure the
    order of the sums.  Returns (dict of the twelve planes as lists, errors)."""
    nO = IM * JM
    p = {k: [float(v) for v in np.asarray(planes[k], np.float64).reshape(-1)] for k in MERGE_PLANES}
    assert all(len(v) == nO for v in p.values())
    mergemaskOm = [0] * nO
    errors = []
    for k in MERGE_PLANES:
        sanity_nonan(k + "2-0", p[k], IM, JM, errors)
    da_giceO, da_zicetopO, da_contO, da_zatmoO = [0.] * nO, [0.] * nO, [0.] * nO, [0.] * nO
    zland_minO, zland_maxO = [DBL_MAX] * nO, [DBL_MIN] * nO
    for rg, em_land, em_ice in sheets:
        tsO, w_ice, elev = sheet_elevO(orc, rg, em_ice, True, False)
        for d, iO in enumerate(tsO):
            da_zicetopO[iO] += elev[d] * native_area[iO]
            mergemaskOm[iO] = 1
        tsO, w, _ = sheet_elevO(orc, rg, em_ice, False, True)
        for d, iO in enumerate(tsO):
            da_giceO[iO] += float(w.wM[d])
        elevI = np.asarray(em_land, np.float64).tolist()
        tsO, w_land, elev_land = sheet_elevO(orc, rg, em_land, True, False)
        for d, iO in enumerate(tsO):
            da_zatmoO[iO] += elev_land[d] * native_area[iO]
        for r, c in zip(w_land.row.tolist(), w_land.col.tolist()):
            iO = tsO[r]
            zland_minO[iO] = cmin(zland_minO[iO], elevI[c])
            zland_maxO[iO] = cmax(zland_maxO[iO], elevI[c])
        if sums is not None:
            sums.append((w_ice, em_ice, elev, w_land, em_land, elev_land))
        tsO, w, _ = sheet_elevO(orc, rg, em_land, False, True)
        for d, iO in enumerate(tsO):
            da_contO[iO] += float(w.wM[d])
    for iO in range(nO):
        if da_contO[iO] == 0.:
            continue
        by_areaO = 1. / native_area[iO]
        fgiceOp0 = p["fgiceOp"][iO]
        diff_fgiceOp = da_giceO[iO] * by_areaO
        if diff_fgiceOp != 0:
            mergemaskOm[iO] = 1
        p["fgiceOp"][iO] = p["fgiceOp"][iO] + diff_fgiceOp
        p["foceanOp"][iO] = p["foceanOp"][iO] - da_contO[iO] * by_areaO
        p["zatmoOp"][iO] += da_zatmoO[iO] * by_areaO
        if p["fgiceOp"][iO] != 0:
            p["zicetopO"][iO] = (p["zicetopO"][iO] * fgiceOp0 + da_zicetopO[iO] * by_areaO * diff_fgiceOp) / p["fgiceOp"][iO]
        if p["foceanOp"][iO] < 0.5 and p["foceanOm"][iO] == 1.0:
            fact = 1. / (1. - p["foceanOp"][iO])
            p["foceanOm"][iO] = 0.0
            p["fgiceOm"][iO] = p["fgiceOp"][iO] * fact
            mergemaskOm[iO] = 1
            p["fgrndOm"][iO] = 1.0 - p["fgiceOm"][iO] - p["flakeOm"][iO]
            p["zatmoOm"][iO] = p["zatmoOp"][iO] * fact
    single_cell_oceans(p, IM, JM, one_shot)
    for k in MERGE_PLANES:
        sanity_nonan(k + "2", p[k], IM, JM, errors)
    sanity_check_land_fractions(p["foceanOm"], p["flakeOm"], p["fgrndOm"], p["fgiceOm"], IM, JM, errors)
    for iO in range(nO):
        if not mergemaskOm[iO]:
            zland_minO[iO] = NaN
            zland_maxO[iO] = NaN
    p.update(zland_minO=zland_minO, zland_maxO=zland_maxO, mergemaskOm=mergemaskOm)
    return p, errors


def merge_poles(var, im, jm):
    """(:538-550)"""
    for j in (0, jm - 1):
        s = 0.
        for i in range(im):
            s += var[j * im + i]
        mean = s / float(im)
        for i in range(im):
            var[j * im + i] = mean


def split(iE, strides):
    """indexingHCA.index_to_tuple on (stride_A, stride_HC) -> (iA2, ihc)"""
    sA, sHC = strides
    if sHC >= sA:
        return (iE % sHC) // sA, iE // sHC
    return iE // sA, (iE % sA) // sHC


def ghost_range(hcdefs, nhc_local, zland_min, zland_max):
    """(:750-761, :775-776) -> (minghost, maxghost), in the reference's int arithmetic"""
    zland_minhc, zland_maxhc = INT_MAX, INT_MIN
    for ihc in range(nhc_local):
        if hcdefs[ihc] < zland_min:
            zland_minhc = ihc
        if hcdefs[ihc] <= zland_max:
            zland_maxhc = ihc
    minghost = max(0, zland_minhc - 1)
    maxghost = min(zland_maxhc + 2, nhc_local - 1)
    assert INT_MIN <= minghost <= INT_MAX and INT_MIN <= maxghost <= INT_MAX
    return minghost, maxghost


def make_topoA(planesO, mergemaskOm, hspecO, hspecA, strides, hcdefs, underice_hc, entries, regrid_ref, triplets_ref):
    """make_topoA (:621-852).  planesO: dict of foceanOm flakeOm fgrndOm fgiceOm zatmoOm zlakeOm zicetopO zland_minO zland_maxO
    (flat); entries: AAmvEAm as (iA, iE, value) in SPARSE indices; strides: (stride_A, stride_HC) of indexingHCA.  Returns (dict of
    the nine A planes, mergemask, fhc, elevE, underice as flat lists, errors)."""
    imA, jmA, nA, nO = hspecA.im, hspecA.jm, hspecA.size, hspecO.size
    src = ("foceanOm", "flakeOm", "fgrndOm", "fgiceOm", "zatmoOm", "zlakeOm", "zicetopO")
    O = {k: np.asarray(planesO[k], np.float64).reshape(-1) for k in src + ("zland_minO", "zland_maxO")}
    assert all(len(v) == nO for v in O.values())
    A = {}
    WTO = np.ones(nO)
    for kO, kA in zip(src[:6], TOPOA_PLANES[:6]):
        A[kA] = regrid_ref(hspecA, hspecO, WTO, O[kO], 0.)[0].tolist()
    A["zicetop"] = regrid_ref(hspecA, hspecO, O["fgiceOm"], O["zicetopO"], 0.)[0].tolist()
    mergemaskA = [0] * nA
    zland_minA, zland_maxA = [DBL_MAX] * nA, [DBL_MIN] * nA
    mO = np.asarray(mergemaskOm).reshape(-1).tolist()
    zminO, zmaxO = O["zland_minO"].tolist(), O["zland_maxO"].tolist()
    iB, iA_, _ = triplets_ref(hspecA, hspecO, "scaled", 1.)
    for iA, iO in zip(iB.tolist(), iA_.tolist()):        # _RegridMinMax::add (:565-578)
        if mO[iO]:
            mergemaskA[iA] = 1
            zland_minA[iA] = cmin(zland_minA[iA], zminO[iO])
            zland_maxA[iA] = cmax(zland_maxA[iA], zmaxO[iO])
    for c in range(nA):
        if zland_minA[c] == DBL_MAX:
            zland_minA[c] = NaN
        if zland_maxA[c] == DBL_MIN:
            zland_maxA[c] = NaN
    A["zland_min"], A["zland_max"] = zland_minA, zland_maxA
    for k in TOPOA_PLANES:
        merge_poles(A[k], imA, jmA)
    nhc_icebin = len(hcdefs)
    nhc_local = 0
    while nhc_local < nhc_icebin and underice_hc[nhc_local] == UI_LOCALICE:
        nhc_local += 1
    nhc_gcm = nhc_icebin + 1
    fhc, elevE, underice = [0.] * (nhc_gcm * nA), [NaN] * (nhc_gcm * nA), [UI_UNUSED] * (nhc_gcm * nA)
    for iA, iE, v in entries:
        iA2, ihc = split(iE, strides)
        if iA2 != iA:
            raise ValueError("Matrix is non-local: iA=%d, iE=%d, iA2=%d" % (iA, iE, iA2))
        if ihc < 0 or ihc >= nhc_icebin:
            raise ValueError("ihc out of range [0,%d): %d" % (nhc_icebin, ihc))
        if iA < 0 or iA >= nA:
            raise ValueError("iA out of range [0,%d): %d" % (nA, iA))
        fhc[ihc * nA + iA] += v
        underice[ihc * nA + iA] = underice_hc[ihc]
    for ihc in range(nhc_icebin):
        fhc_sum = 0.
        for i in range(imA):
            fhc_sum += fhc[ihc * nA + i]
        fhc_mean = fhc_sum / float(imA)
        for i in range(imA):
            fhc[ihc * nA + i] = fhc_mean
    for c in range(nA):
        for ihc in range(nhc_local):
            elevE[ihc * nA + c] = hcdefs[ihc]
        if abs(A["focean"][c] - 1.0) > 1.e-14:
            minghost, maxghost = ghost_range(hcdefs, nhc_local, zland_minA[c], zland_maxA[c])
            for ihc in range(minghost, maxghost + 1):
                if fhc[ihc * nA + c] == 0:
                    fhc[ihc * nA + c] = 1.e-30
                    underice[ihc * nA + c] = UI_VGHOST
        for ihc in range(nhc_local, nhc_icebin):
            elevE[ihc * nA + c] = hcdefs[ihc]
    ec_base = nhc_icebin
    for c in range(nA):
        if A["fgice"][c] > 0:
            fhc[ec_base * nA + c] = 0 if A["fgice"][c] == 0 else 1e-30
            underice[ec_base * nA + c] = UI_SEALAND
        elevE[ec_base * nA + c] = A["zatmo"][c]
    errors = []
    sanity_check_land_fractions(A["focean"], A["flake"], A["fgrnd"], A["fgice"], imA, jmA, errors)
    for j in range(jmA):
        for i in range(imA):
            all_fhc = 0.
            for ihc in range(nhc_gcm):
                all_fhc += fhc[ihc * nA + j * imA + i]
            all_fhc += 1.0
            if all_fhc != 1.0 and abs(all_fhc - 2.0) > 1.e-13:
                errors.append("(%d, %d): sum(FHC) = %g" % (i + 1, j + 1, all_fhc - 1.0))
    A.update(mergemask=mergemaskA, fhc=fhc, elevE=elevE, underice=underice)
    return A, errors
