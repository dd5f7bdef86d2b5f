"""update_topo's field handling on the GPU (ibh_weighted_row_stats_device, ibh_modele_merge_topoO, ibh_modele_make_topoA,
GCMRegridder_ModelE.update_topo) against the plain-Python restatement (tests/topo_restatement.py, pinned by
tests/test_topo_restatement.py): the planes that depend on the matrices' weights and on min / max alone bitwise, the planes
that carry a row sum OvI . elevmaskI within the project's apply gate (rel Linf <= 1e-12), make_topoA bitwise."""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topo_cases as tc  # noqa: E402
import topo_restatement as tr  # noqa: E402
from test_gpu_hntr import regrid_ref  # noqa: E402
from test_gpu_hntr_matrix import triplets_ref  # noqa: E402
from test_topo_restatement import MEASURED_SEQ_VS_FSUM  # noqa: E402

R = tc.R
GATE = 1e-12
DBL_MAX, DBL_MIN = tr.DBL_MAX, tr.DBL_MIN
# the launch shapes of k_topo_row_stats (icebin_amd/csrc/topo.hip): a workgroup of 4 waves per row, 16 when the matrix holds more
# than 16384 entries per row on average; each lane takes 4 entries per pass while the row lasts, then one
UNROLL, THREADS, THREADS_LONG, LONG_ROWS = 4, 256, 1024, 16384

TOPOO = dict(foceanOp="FOCEANF", fgiceOp="FGICEF", zatmoOp="ZATMOF", foceanOm="FOCEAN", flakeOm="FLAKE", fgrndOm="FGRND", fgiceOm="FGICE",
             zatmoOm="ZATMO", zicetopO="ZICETOP", zlakeOm="ZLAKE", zland_minO="ZLAND_MIN", zland_maxO="ZLAND_MAX")
BITWISE_O = ("foceanOp", "fgiceOp", "foceanOm", "flakeOm", "fgrndOm", "fgiceOm", "zland_minO", "zland_maxO")
GATED_O = ("zatmoOp", "zatmoOm", "zicetopO")
TOPOA = dict(zip(tr.TOPOA_PLANES, ("focean", "flake", "fgrnd", "fgice", "zatmo", "hlake", "zicetop", "zland_min", "zland_max")))


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1)).view(np.uint64)


def rel_linf(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    scale = np.max(np.abs(want[ok])) if ok.any() else 0.
    return float(np.max(np.abs(got[ok] - want[ok])) / scale) if scale else float(np.max(np.abs(got[ok]), initial=0.))


# ---- row statistics ---------------------------------------------------------------------------------------------------------
def stats_matrix(lengths, ncol, seed, exact):
    """A Weighted whose row r holds lengths[r] entries in distinct shuffled columns, and an x that is NaN in every column no
    entry names.  exact: values are powers of two and x small integers, so every partial sum is exact."""
    from icebin_amd import linear_Weighted
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)
    cols = np.concatenate([rng.choice(ncol, n, replace=False) for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
    nnz = len(rows)
    if exact:
        val = 2.0 ** rng.integers(-3, 4, nnz)
        xs = rng.integers(-8, 9, ncol).astype(np.float64)
    else:
        val = rng.uniform(-1., 2., nnz)
        xs = rng.uniform(-500., 3000., ncol)
    p = rng.permutation(nnz)
    w = linear_Weighted.from_coo((len(lengths), ncol), rows[p], cols[p], val[p], np.ones(len(lengths)), np.ones(ncol))
    x = np.full(ncol, np.nan)
    x[np.unique(cols)] = xs[np.unique(cols)]
    return w, x


def stats_ref(w, x):
    """(sequential sum in CSR order, fsum of the rounded products, min, max) per row"""
    rp, ci, v = w.csr_dense()
    seq, exact, lo, hi = [], [], [], []
    xl, vl, cl = x.tolist(), v.tolist(), ci.tolist()
    for r in range(len(rp) - 1):
        terms = [vl[e] * xl[cl[e]] for e in range(rp[r], rp[r + 1])]
        s = 0.
        for t in terms:
            s += t
        seq.append(s)
        exact.append(math.fsum(terms))
        xs = [xl[cl[e]] for e in range(rp[r], rp[r + 1])]
        lo.append(min(xs + [DBL_MAX]))
        hi.append(max(xs + [DBL_MIN]))
    return np.asarray(seq), np.asarray(exact), np.asarray(lo), np.asarray(hi)


def run_stats(w, x, **kw):
    import torch
    out = w.row_stats_device(torch.from_numpy(x).cuda(), **kw)
    torch.cuda.synchronize()
    return [None if o is None else o.cpu().numpy() for o in out]


SHORT = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 3 * THREADS - 1, 3 * THREADS, 3 * THREADS + 1, UNROLL * THREADS - 1, UNROLL * THREADS,
         UNROLL * THREADS + 1, 300, 0, 5000, 2 * UNROLL * THREADS + 5]
LONG = [3 * THREADS_LONG, 3 * THREADS_LONG + 1, UNROLL * THREADS_LONG - 1, UNROLL * THREADS_LONG, UNROLL * THREADS_LONG + 1, 0, 200000]
SHAPES = {"short": (SHORT, 6000), "long": (LONG, 220000), "at": ([LONG_ROWS], 20000), "over": ([LONG_ROWS + 1], 20000),
          "under": ([LONG_ROWS - 1], 20000)}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_row_stats(shape):
    """Rows of every length at which the kernel takes another path: below, at and above a wave, the first unrolled pass of the
    first lane (3 T + 1 entries) and of the last (4 T), an empty row between full ones, 5 000 and 200 000 entries; the 4-wave
    and the 16-wave workgroup ("long": more than 16 384 entries per row on average; "under" / "at" / "over": one row around
    that threshold)."""
    lengths, ncol = SHAPES[shape]
    if shape == "long":
        assert sum(lengths) > LONG_ROWS * len(lengths)
    if shape == "short":
        assert sum(lengths) <= LONG_ROWS * len(lengths)
    # (a) every partial sum exact: the sum is bitwise the sequential one whatever the order
    w, x = stats_matrix(lengths, ncol, 7, exact=True)
    seq, exact, lo, hi = stats_ref(w, x)
    s, mn, mx = run_stats(w, x)
    assert np.array_equal(seq, exact) and np.array_equal(bits(s), bits(seq)), shape
    assert np.array_equal(mn, lo) and np.array_equal(mx, hi), shape
    # (b) random values: the project's apply gate against fsum; min / max exact
    w, x = stats_matrix(lengths, ncol, 8, exact=False)
    seq, exact, lo, hi = stats_ref(w, x)
    s, mn, mx = run_stats(w, x)
    dev, dev_seq = rel_linf(s, exact), rel_linf(seq, exact)
    print("%s: rel Linf of the row sums against fsum: device %.3e, sequential %.3e" % (shape, dev, dev_seq))
    assert dev <= GATE, (shape, dev)
    assert np.array_equal(mn, lo) and np.array_equal(mx, hi), shape
    assert not np.any(np.isnan(s)) and not np.any(np.isnan(mn)) and not np.any(np.isnan(mx))        # no NaN of an unreferenced column
    empty = [r for r, n in enumerate(lengths) if n == 0]
    for r in empty:
        assert s[r] == 0. and mn[r] == DBL_MAX and mx[r] == DBL_MIN


def test_row_stats_null_outputs_and_quirk():
    w, x = stats_matrix([5, 0, 70, 300], 400, 9, exact=True)
    x = np.where(np.isnan(x), x, -np.abs(x) - 1.)              # every referenced x negative: max keeps DBL_MIN (the reference's quirk)
    seq, _, lo, hi = stats_ref(w, x)
    full = run_stats(w, x)
    assert np.array_equal(full[2], np.full(4, DBL_MIN)) and np.array_equal(full[2], hi)
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, False, False)):
        out = run_stats(w, x, want_sum=want[0], want_min=want[1], want_max=want[2])
        for o, f, wanted in zip(out, full, want):
            assert (o is None) == (not wanted) and (o is None or np.array_equal(bits(o), bits(f)))


def test_row_stats_refuses_bad_arguments():
    import ctypes as C
    from icebin_amd import _capi
    w, _ = stats_matrix([3, 4], 10, 1, exact=True)
    L = _capi.lib()
    out = np.zeros(2)           # never written: the calls are refused before anything is launched
    assert L.ibh_weighted_row_stats_device(None, None, None, None, None, None) == _capi.IBH_EINVAL
    assert "null Weighted handle" in L.ibh_last_error().decode()
    assert L.ibh_weighted_row_stats_device(w._h, None, C.c_void_p(out.ctypes.data), None, None, None) == _capi.IBH_EINVAL
    assert "null x" in L.ibh_last_error().decode()
    assert np.all(out == 0)


# ---- merge_topoO ------------------------------------------------------------------------------------------------------------
class G:
    """One fixture of tests/topo_cases.py: the GCMRegridder on the device, the oracle twins, the restatement's merge (once)."""

    def __init__(self, name):
        from icebin_amd import GCMRegridder
        from oracle import oracle as orc
        self.orc, self.name = orc, name
        self.c = c = getattr(tc, name)()
        self.O = O = c["O"]
        g0 = c["grids"][0]
        self.gcm = self.new_gcm()
        self.empty = GCMRegridder(dict(nA=O.size, to_sparse=g0["A_to_sparse"], native_area=g0["A_native_area"]), tc.HC, True)
        self.ref, self.ref_errors = tr.merge_topoO(orc, tc.oracle_sheets(orc, c), tc.native_area(c), c["planes"], O.im, O.jm)
        ice = np.unique(np.concatenate([tr.sheet_elevO(orc, rg, em, True, False)[0] for rg, _, em in tc.oracle_sheets(orc, c)]))
        self.base = tc.base(c, ice)

    def new_gcm(self):
        from icebin_amd import GCMRegridder
        g0 = self.c["grids"][0]
        gcm = GCMRegridder(dict(nA=self.O.size, to_sparse=g0["A_to_sparse"], native_area=g0["A_native_area"]), tc.HC, True)
        for k, g in enumerate(self.c["grids"]):
            gcm.add_sheet("sheet%d" % k, dict(nI=g["nI"]), dict(indices=g["ex_indices"].copy(), overlaps=g["ex_area"].copy()))
        return gcm

    def topoo(self, planes=None, device=False):
        planes = self.c["planes"] if planes is None else planes
        t = {TOPOO[k]: np.array(planes[k], np.float64) for k in planes if k in TOPOO}
        if device:
            import torch
            t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
        return t


_G = {}


def get_G(name):
    if name not in _G:
        _G[name] = G(name)
    return _G[name]


@pytest.fixture(params=["t1", "t2"])
def g(request):
    return get_G(request.param)


def host(x):
    return x.cpu().numpy() if hasattr(x, "is_cuda") else np.asarray(x)


def same_merge(g, topoo, mask, ref, what):
    devs = {}
    for k in BITWISE_O:
        got = host(topoo[TOPOO[k]])
        assert got.shape == (g.O.jm, g.O.im) and np.array_equal(bits(got), bits(ref[k])), (what, k)
    assert np.array_equal(host(mask).reshape(-1), np.asarray(ref["mergemaskOm"], np.int16)), (what, "mergemaskOm")
    for k in GATED_O:
        devs[k] = rel_linf(host(topoo[TOPOO[k]]), ref[k])
        assert devs[k] <= GATE, (what, k, devs[k])
    return devs


@pytest.mark.parametrize("device", [False, True])
def test_merge_topoO(g, device):
    from icebin_amd import merge_topoO
    c = g.c
    topoo = g.topoo(device=device)
    lands, ices = c["lands"], c["ices"]
    if device:
        import torch
        lands, ices = [torch.from_numpy(e).cuda() for e in lands], [torch.from_numpy(e).cuda() for e in ices]
    mask, errors = merge_topoO(topoo, g.gcm, lands, ices, g.O, R)
    assert errors == [] == g.ref_errors
    devs = same_merge(g, topoo, mask, g.ref, (g.name, device))
    print("%s (%s): rel Linf against the restatement %s; its sequential sums lie %.1e from fsum" % (
        g.name, "device" if device else "host", ", ".join("%s %.3e" % kv for kv in devs.items()), MEASURED_SEQ_VS_FSUM[g.name]))
    ref_mask = np.asarray(g.ref["mergemaskOm"])
    assert 4 <= ref_mask.sum() < g.O.size and np.isnan(g.ref["zland_minO"]).sum() == g.O.size - ref_mask.sum()


def test_merge_topoO_empty_sheet_and_no_sheet(g):
    from icebin_amd import merge_topoO
    c, orc = g.c, g.orc
    # a sheet whose two masks are all NaN: four empty builds
    lands = [np.full(len(e), np.nan) for e in c["lands"][:1]] + list(c["lands"][1:])
    ices = [np.full(len(e), np.nan) for e in c["ices"][:1]] + list(c["ices"][1:])
    ref, ref_errors = tr.merge_topoO(orc, tc.oracle_sheets(orc, c, lands, ices), tc.native_area(c), c["planes"], g.O.im, g.O.jm)
    topoo = g.topoo()
    mask, errors = merge_topoO(topoo, g.gcm, lands, ices, g.O, R)
    assert errors == ref_errors == []
    same_merge(g, topoo, mask, ref, (g.name, "empty sheet"))
    # no sheet: mergemask 0, zland NaN, and the fields unchanged -- but for the single-cell-ocean pass, which the reference runs
    # whatever was merged: it finds nothing once foceanOp == 1 on every ModelE ocean cell
    ref, ref_errors = tr.merge_topoO(orc, [], tc.native_area(c), c["planes"], g.O.im, g.O.jm)
    topoo = g.topoo()
    mask, errors = merge_topoO(topoo, g.empty, [], [], g.O, R)
    assert errors == ref_errors == [] and not mask.any()
    for k in tr.MERGE_PLANES:
        assert np.array_equal(bits(topoo[TOPOO[k]]), bits(ref[k])), k
    assert np.all(np.isnan(topoo["ZLAND_MIN"])) and np.all(np.isnan(topoo["ZLAND_MAX"]))
    planes = dict(c["planes"], foceanOp=np.where(np.asarray(c["planes"]["foceanOm"]) == 1., 1., c["planes"]["foceanOp"]))
    topoo = g.topoo(planes)
    mask, errors = merge_topoO(topoo, g.empty, [], [], g.O, R)
    assert errors == [] and not mask.any()
    for k in tr.MERGE_PLANES:
        assert np.array_equal(bits(topoo[TOPOO[k]]), bits(planes[k])), k
    assert np.all(np.isnan(topoo["ZLAND_MIN"])) and np.all(np.isnan(topoo["ZLAND_MAX"]))


@pytest.mark.parametrize("device", [False, True])
def test_merge_topoO_error_strings(g, device):
    """NaN planted in three input planes and a land fraction off by 1e-10: the reference's strings in the reference's order
    (check by check, then j, then i); the call itself succeeds."""
    from icebin_amd import merge_topoO
    c = g.c
    planes = {k: np.array(v, np.float64) for k, v in c["planes"].items()}
    n = g.O.size
    planes["zatmoOp"][[n - 2, 3]] = np.nan
    planes["foceanOp"][7] = np.nan
    planes["flakeOm"][n // 2] = np.nan
    land = np.flatnonzero(planes["foceanOm"] == 0.)            # a cell the update never recomputes
    planes["fgrndOm"][land[land > 10][0]] += 1e-10
    ref, ref_errors = tr.merge_topoO(g.orc, tc.oracle_sheets(g.orc, c), tc.native_area(c), planes, g.O.im, g.O.jm)
    topoo = g.topoo(planes, device=device)
    mask, errors = merge_topoO(topoo, g.gcm, c["lands"], c["ices"], g.O, R)
    assert errors == ref_errors and len(errors) >= 9, errors
    assert errors[0] == "(8, 1): foceanOp2-0 is NaN" and errors[1] == "(4, 1): zatmoOp2-0 is NaN"
    assert any(e.endswith("foceanOp2 is NaN") for e in errors) and any("FOCEAN(" in e and ") + FGRND(" in e for e in errors)
    assert errors[-1].startswith("(") and "  = " in errors[-1]
    same = [k for k in BITWISE_O if np.array_equal(bits(host(topoo[TOPOO[k]])), bits(ref[k]))]
    assert same == list(BITWISE_O)


def test_merge_topoO_refusals_leave_the_planes_alone(g):
    from icebin_amd import _capi
    from icebin_amd.modele import merge_topoO_rm
    c = g.c
    names = list(g.gcm._sheets)
    lands = [g.gcm.regrid_matrices(n, e, scale=False, correctA=True) for n, e in zip(names, c["lands"])]
    ices = [g.gcm.regrid_matrices(n, e, scale=False, correctA=True) for n, e in zip(names, c["ices"])]
    other = get_G("t2" if g.name == "t1" else "t1")
    foreign = other.gcm.regrid_matrices("sheet0", other.c["ices"][0], scale=False, correctA=True)
    twin = g.new_gcm()          # the same grid in another regridder: the two masks of a sheet must share one
    twin_land = twin.regrid_matrices("sheet0", c["lands"][0], scale=False, correctA=True)
    smooth = g.gcm.regrid_matrices("sheet0", c["ices"][0], scale=False, correctA=True, sigma=(50000., 50000., 100.))
    from icebin_amd import HntrSpec
    cases = [(lands, ices[:-1] if len(ices) > 1 else [], g.O, r"%d land masks \(emI_lands\) for %d ice masks" % (len(lands), len(ices) - 1)),
             ([foreign] + lands[1:], [foreign] + ices[1:], g.O, r"sheet 0: imO\*jmO = %d but its ocean grid has nA=%d" % (g.O.size, other.O.size)),
             (lands, ices, HntrSpec(g.O.im, g.O.jm + 2, 0., 10800. / (g.O.jm + 2)), r"imO\*jmO = %d" % (g.O.im * (g.O.jm + 2))),
             ([twin_land] + lands[1:], ices, g.O, "sheet 0: emI_lands and emI_ices belong to different ice regridders"),
             (lands, [smooth] + ices[1:], g.O, "sheet 0 has a non-zero sigma")]
    for la, ic, spec, msg in cases:
        topoo = g.topoo()
        topoo["ZLAND_MIN"] = np.full((spec.jm, spec.im), 7.)
        keep = {k: v.copy() for k, v in topoo.items()}
        if spec is not g.O:     # planes of the (wrong) size asked for, so that the C entry is what refuses
            topoo = {k: np.resize(v, spec.size) for k, v in topoo.items()}
            keep = {k: v.copy() for k, v in topoo.items()}
        with pytest.raises(_capi.IcebinHipError, match=msg) as ei:
            merge_topoO_rm(topoo, la, ic, spec, R)
        assert ei.value.code == _capi.IBH_EINVAL
        for k in keep:
            assert np.array_equal(bits(topoo[k]), bits(keep[k])), (msg, k)


# ---- make_topoA -------------------------------------------------------------------------------------------------------------
def device_AvE(g, classes, fp, fm):
    """(AAmvEAm, hcdefs, underice_hc) of global_AvE's two library calls on the fixture: the sheets' local classes, the base ice's,
    or both."""
    from icebin_amd import compute_AAmvEAm, compute_EOpvAOp_merged
    names = list(g.gcm._sheets)
    rmOs = [g.gcm.regrid_matrices(n, e, scale=False, correctA=False) for n, e in zip(names, g.c["ices"])]
    if classes == "local":
        r = compute_EOpvAOp_merged(rmOs, None, nO=g.O.size)
    elif classes == "base":
        r = compute_EOpvAOp_merged([], g.base)
    else:
        r = compute_EOpvAOp_merged(rmOs, g.base)
    return compute_AAmvEAm(r, g.O, R, fp, fm, scale=True), r.hcdefs, r.underice_hc.tolist()


def entries_of(w):
    rp, ci, v = w.csr_dense()
    dA, dE = w.dim(0).tolist(), w.dim(1).tolist()
    return [(dA[r], dE[ci[e]], float(v[e])) for r in range(len(rp) - 1) for e in range(rp[r], rp[r + 1])]


def same_topoA(got, ref, hspecA, nhc, what):
    shape2, shape3 = (hspecA.jm, hspecA.im), (nhc + 1, hspecA.jm, hspecA.im)
    for kr, kg in TOPOA.items():
        x = host(got[kg])
        assert x.shape == shape2 and np.array_equal(bits(x), bits(ref[kr])), (what, kg)
    assert np.array_equal(host(got["mergemask"]).reshape(-1), np.asarray(ref["mergemask"], np.int16)), (what, "mergemask")
    for k in ("fhc", "elevE"):
        x = host(got[k])
        assert x.shape == shape3 and np.array_equal(bits(x), bits(ref[k])), (what, k)
    assert np.array_equal(host(got["underice"]).reshape(-1), np.asarray(ref["underice"], np.int16)), (what, "underice")


def tampered(g):
    """The restatement's merged planes with the land range of two merged cells moved below the first and above the last class."""
    p = {k: list(v) for k, v in g.ref.items()}
    p["zlakeOm"] = list(g.c["planes"]["zlakeOm"])
    merged = np.flatnonzero(np.asarray(p["mergemaskOm"]))
    merged = merged[(merged // g.O.im >= 2) & (merged // g.O.im < g.O.jm - 2)]      # under atmosphere rows that are no pole rows
    lo, hi = int(merged[0]), int(merged[-1])
    assert (lo // g.O.im // 2, lo % g.O.im // 2) != (hi // g.O.im // 2, hi % g.O.im // 2)
    p["zland_minO"][lo], p["zland_maxO"][lo] = -20., -5.
    p["zland_maxO"][hi] = 3500.
    return p


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("classes", ["both", "local", "base"])
def test_make_topoA_bitwise(g, classes, device):
    from icebin_amd import make_hntrA, make_topoA
    p = tampered(g)
    w, hcdefs, underice_hc = device_AvE(g, classes, g.ref["foceanOp"], g.ref["foceanOm"])
    hspecA = make_hntrA(g.O)
    strides = (1, hspecA.size)
    ref, ref_errors = tr.make_topoA(p, p["mergemaskOm"], g.O, hspecA, strides, hcdefs.tolist(), underice_hc, entries_of(w), regrid_ref,
                                    triplets_ref)
    topoo = g.topoo(p, device=device)
    mask = np.asarray(p["mergemaskOm"], np.int16)
    if device:
        import torch
        mask = torch.from_numpy(mask).cuda()
    got, errors = make_topoA(topoo, mask, g.O, hspecA, strides, hcdefs, underice_hc, w)
    same_topoA(got, ref, hspecA, len(hcdefs), (g.name, classes, device))
    assert errors == ref_errors
    # what the fixture is for
    nA, nhc = hspecA.size, len(hcdefs)
    ui = np.asarray(ref["underice"]).reshape(nhc + 1, nA)
    assert hspecA.jm >= 3 and (np.asarray(ref["fgice"]) > 0).any() and (ui[nhc] == tr.UI_SEALAND).any()
    assert np.nanmin(ref["zland_min"]) < 0. and np.nanmax(ref["zland_max"]) > 3000.
    if classes != "base":
        assert (ui[:3] == tr.UI_LOCALICE).any()
    if g.name == "t2":
        assert (np.asarray(ref["focean"]) == 1.).any()
        if classes != "base":
            assert (ui == tr.UI_VGHOST).any()


def test_make_topoA_errors(g):
    from icebin_amd import _capi, linear_Weighted, make_hntrA, make_topoA
    hspecA = make_hntrA(g.O)
    nA = hspecA.size
    p = tampered(g)
    mask = np.asarray(p["mergemaskOm"], np.int16)
    # land fractions perturbed by 1e-10: the reference's string for every cell, then nothing else
    p["fgrndOm"] = [v + 1e-10 for v in p["fgrndOm"]]
    w, hcdefs, underice_hc = device_AvE(g, "both", g.ref["foceanOp"], g.ref["foceanOm"])
    ref, ref_errors = tr.make_topoA(p, p["mergemaskOm"], g.O, hspecA, (1, nA), hcdefs.tolist(), underice_hc, entries_of(w), regrid_ref, triplets_ref)
    got, errors = make_topoA(g.topoo(p), mask, g.O, hspecA, (1, nA), hcdefs, underice_hc, w)
    assert errors == ref_errors and len(errors) == nA and errors[0].startswith("(1, 1): FOCEAN(") and "  = 1" in errors[0]
    same_topoA(got, ref, hspecA, len(hcdefs), (g.name, "perturbed"))
    # a matrix entry that names another A cell, a class outside the table, an A cell outside the grid: dims are the identity
    nhc = 3
    good = [(0, 0, .5), (0, nA, .5), (2, 2 + 2 * nA, 1.)]
    for bad, msg in (((1, 2, .25), r"Matrix is non-local: iA=1, iE=2, iA2=2"),
                     ((1, 1 + nhc * nA, .25), r"ihc out of range \[0,3\): 3")):
        r, c_, v = zip(*(good[:2] + [bad] + good[2:]))
        ncol = nA * (nhc + 1)
        m = linear_Weighted.from_coo((nA, ncol), r, c_, v, np.ones(nA), np.ones(ncol))
        with pytest.raises(_capi.IcebinHipError, match=msg) as ei:
            make_topoA(g.topoo(p), mask, g.O, hspecA, (1, nA), tc.HC, [1, 1, 1], m)
        assert ei.value.code == _capi.IBH_EINVAL
        with pytest.raises(ValueError, match=msg):
            tr.make_topoA(p, p["mergemaskOm"], g.O, hspecA, (1, nA), tc.HC, [1, 1, 1], list(zip(r, c_, v)), regrid_ref, triplets_ref)


# ---- update_topo ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_update_topo(g, device):
    """Against the three calls made separately (bitwise: the same kernels) and against the restatement end to end: the planes
    that carry no row sum bitwise, zatmo / zicetop and the sea-land elevation (= zatmoA) within the gate."""
    import global_ave_restatement as gr
    from icebin_amd import make_topoA, merge_topoO
    c = g.c
    m = g.gcm.to_modele((c["planes"]["foceanOp"], c["planes"]["foceanOm"]), hspecO=g.O, eq_rad=R, global_ec=g.base)
    lands, ices = c["lands"], c["ices"]
    if device:
        import torch
        lands, ices = [torch.from_numpy(e).cuda() for e in lands], [torch.from_numpy(e).cuda() for e in ices]
    topoo = g.topoo(device=device)
    out = m.update_topo(topoo, lands, ices, run_ice=True)
    assert np.array_equal(bits(m.foceanOp), bits(host(topoo["FOCEANF"]))) and np.array_equal(bits(m.foceanOm), bits(c["planes"]["foceanOm"]))
    # the three calls
    t3 = g.topoo(device=device)
    mask, errors = merge_topoO(t3, g.gcm, lands, ices, g.O, R)
    assert errors == []
    for k in t3:
        assert np.array_equal(bits(host(t3[k])), bits(host(topoo[k]))), k
    fp, fm = host(t3["FOCEANF"]).reshape(-1), host(t3["FOCEAN"]).reshape(-1)
    w, offsetE = m.global_AvE(lands, ices, fp, fm, scale=True)
    nhc = len(m.hcdefs)
    sep, errors = make_topoA(t3, mask, g.O, m.hspecA, (1, m.hspecA.size), m.hcdefs, [m.underice(k) for k in range(nhc)], w)
    assert errors == [] and offsetE == out["offsetE"] == 3 * g.O.size
    for k in sep:
        assert host(sep[k]).tobytes() == host(out[k]).tobytes(), k
    iE, Mw = w.dim(1), w.Mw
    assert np.array_equal(out["wEAm_base"][0], iE[iE >= offsetE]) and np.array_equal(bits(out["wEAm_base"][1]), bits(Mw[iE >= offsetE]))
    # (offsetE counts rows of the OCEAN grid's E space, Mw's keys those of the atmosphere's, four times smaller: DESIGN.md 17)
    assert len(out["wEAm_base"][0]) == 0 and iE.max() < nhc * m.hspecA.size <= offsetE
    # the restatement end to end
    sheets = [(rg, em) for rg, _, em in tc.oracle_sheets(g.orc, c)]
    merged = gr.merged(g.orc, sheets, g.O.size, 3, tc.HC, g.base)
    AvE = gr.AAmvEAm(merged, g.O, R, g.ref["foceanOp"], g.ref["foceanOm"], triplets_ref, scale=True)
    entries = [(int(AvE["dims"][0][r]), int(AvE["dims"][1][k]), v) for r, row in enumerate(AvE["M"]) for k, v in row]
    planes = dict(g.ref, zlakeOm=c["planes"]["zlakeOm"])
    ref, ref_errors = tr.make_topoA(planes, g.ref["mergemaskOm"], g.O, m.hspecA, (1, m.hspecA.size), merged["hcdefs"], merged["underice"], entries,
                                    regrid_ref, triplets_ref)
    assert ref_errors == []
    nA = m.hspecA.size
    devs = {}
    for kr, kg in TOPOA.items():
        if kr in ("zatmo", "zicetop"):
            devs[kg] = rel_linf(host(out[kg]), ref[kr])
            assert devs[kg] <= GATE, (kg, devs[kg])
        else:
            assert np.array_equal(bits(host(out[kg])), bits(ref[kr])), kg
    assert np.array_equal(host(out["mergemask"]).reshape(-1), np.asarray(ref["mergemask"], np.int16))
    assert np.array_equal(bits(host(out["fhc"])), bits(ref["fhc"])) and np.array_equal(host(out["underice"]).reshape(-1), ref["underice"])
    eE, rE = host(out["elevE"]).reshape(-1), np.asarray(ref["elevE"])
    assert np.array_equal(bits(eE[:nhc * nA]), bits(rE[:nhc * nA]))
    devs["elevE[sea-land]"] = rel_linf(eE[nhc * nA:], rE[nhc * nA:])
    assert devs["elevE[sea-land]"] <= GATE
    print("%s (%s): update_topo against the restatement, rel Linf %s" % (g.name, "device" if device else "host",
                                                                         ", ".join("%s %.3e" % kv for kv in devs.items())))


def test_update_topo_halts_on_failed_checks(g):
    c = g.c
    m = g.gcm.to_modele((c["planes"]["foceanOp"], c["planes"]["foceanOm"]), hspecO=g.O, eq_rad=R, global_ec=g.base)
    planes = {k: np.array(v, np.float64) for k, v in c["planes"].items()}
    planes["zicetopO"][9] = np.nan
    at = r"\(%d, %d\)" % (9 % g.O.im + 1, 9 // g.O.im + 1)
    with pytest.raises(RuntimeError, match=r"halting!\nERROR: %s: zicetopO2-0 is NaN\nERROR: %s: zicetopO2 is NaN" % (at, at)) as ei:
        m.update_topo(g.topoo(planes), c["lands"], c["ices"])
    assert str(ei.value).count("ERROR: ") == 2
