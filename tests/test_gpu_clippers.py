"""The two polygon clippers on the GPU at their vertex-count, bin and lane limits: gridgen.hip's k_gg_clip / k_gg_clip_stream and
l1.hip's k_l1_clip behind its uniform-bin candidate search, on the cases of tests/clipper_cases.py (tests/test_clipper_cases.py
checks on the CPU that the cases reach those limits).  References: exact Sutherland-Hodgman in Fractions of the float inputs,
and tests/lonlat_restatement.py for the streamed kernel's bits.  Areas: 1e-12 relative, the bar of test_exchange_grid_generation
and test_gpu_l1.py."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clipper_cases as cc                  # noqa: E402
import lonlat_restatement as llr            # noqa: E402
import test_lonlat_restatement as cpu       # noqa: E402
from icebin_amd import _capi                # noqa: E402
from icebin_amd import gridgen as gg        # noqa: E402
from icebin_amd._capi import check, lib     # noqa: E402

pytestmark = pytest.mark.gpu
u64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)     # noqa: E731
RTOL = 1e-12


@pytest.fixture
def stream_clip():
    def force(v):
        check(lib().ibh_set_tuning(b"gridgen_stream_clip", v))
    yield force
    force(-1)


@pytest.fixture(scope="module")
def l1():
    from icebin_amd import l1 as mod
    return mod


def three_ways(stream_clip, xe, ye, polys, iA, xf=False):
    out = []
    for v in (-1, 0, 1):
        stream_clip(v)
        out.append(gg.make_exchange_grid(xe, ye, polys, iA, x_fastest=xf))
    stream_clip(-1)
    return out


def restated(xe, ye, polys, iA, xf=False):
    polyptr = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int32)
    v = np.concatenate(polys)
    return llr.exchange_grid(xe, ye, polyptr, v[:, 0], v[:, 1], iA, xf)


def same(a, b):
    return np.array_equal(a["indices"], b["indices"]) and np.array_equal(u64(a["overlaps"]), u64(b["overlaps"]))


def check_convex_gridgen(stream_clip, xe, ye, polys, iA, xf, keys, exact, what):
    dflt, arr, st = three_ways(stream_clip, xe, ye, polys, iA, xf)
    assert [tuple(k) for k in arr["indices"].tolist()] == keys, what                     # the exact set, in (iA, iI) order
    err_a, err_s = np.max(np.abs(arr["overlaps"] - exact) / exact), np.max(np.abs(st["overlaps"] - exact) / exact)
    print("%s: %d cells, array kernel within %.2e of exact, streamed within %.2e" % (what, len(keys), err_a, err_s))
    assert err_a <= RTOL and err_s <= RTOL, what
    assert same(dflt, arr), what + ": the default call is not the array kernel's"
    idx, area = restated(xe, ye, polys, iA, xf)
    assert np.array_equal(st["indices"], idx) and np.array_equal(u64(st["overlaps"]), u64(area)), what + ": streamed vs restatement"
    # streamed vs array as test_old_path_untouched measures it: relative to the ice cell's area
    nx, ny = len(xe) - 1, len(ye) - 1
    iI = arr["indices"][:, 1]
    ix, iy = (iI % nx, iI // nx) if xf else (iI // ny, iI % ny)
    cell = np.diff(xe)[ix] * np.diff(ye)[iy]
    r = max(np.abs(xe).max(), np.abs(ye).max()) / min(np.diff(xe).min(), np.diff(ye).min())
    bound = cpu.stream_clip_bound(r) + cpu.array_clip_bound(r)
    err = np.max(np.abs(st["overlaps"] - arr["overlaps"]) / cell)
    print("%s: streamed vs array kernel, worst difference / ice-cell area = %.3e (bound %.3e)" % (what, err, bound))
    assert err <= bound, what


# ---- gridgen: G20 and GR ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["one", "three"])
@pytest.mark.parametrize("xf", [False, True])
def test_g20_array_limit(stream_clip, grid, xf):
    g = cc.g20()
    xe, ye = g[grid]
    keys, exact = cc.exact_gridgen(xe, ye, [g["poly"]], g["iA"], xf)
    assert len(keys) == (1 if grid == "one" else 5)
    check_convex_gridgen(stream_clip, xe, ye, [g["poly"]], g["iA"], xf, keys, exact, "G20/" + grid)


@pytest.mark.parametrize("npoly", cc.GR_NPOLY)
@pytest.mark.parametrize("xf", [False, True])
def test_gr_candidate_ranges_and_ties(stream_clip, npoly, xf):
    G = cc.gr()
    polys, iA, pos = cc.gr_variant(npoly)
    keys, exact = cc.assemble_gridgen(G["xe"], G["ye"], [G["per_poly"][k] for k in pos], iA, xf)
    assert len(keys) > 500
    check_convex_gridgen(stream_clip, G["xe"], G["ye"], polys, iA, xf, keys, exact, "GR/%d" % npoly)


# ---- gridgen: GNC ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zigzag", "u", "star"])
def test_gnc_non_convex_takes_the_streamed_kernel(stream_clip, name):
    xe, ye, poly = cc.gnc()[name]
    iA = [7]
    for xf in (False, True):
        stream_clip(-1)
        dflt = gg.make_exchange_grid(xe, ye, [poly], iA, x_fastest=xf)
        stream_clip(1)
        st = gg.make_exchange_grid(xe, ye, [poly], iA, x_fastest=xf)
        idx, area = restated(xe, ye, [poly], iA, xf)
        assert same(dflt, st) and np.array_equal(st["indices"], idx) and np.array_equal(u64(st["overlaps"]), u64(area))
        assert len(area) >= 9
        if name != "star":      # self-intersecting: no exact area to hold it to
            keys, exact = cc.exact_gridgen(xe, ye, [poly], iA, xf)
            assert [tuple(k) for k in dflt["indices"].tolist()] == keys
            err = np.max(np.abs(dflt["overlaps"] - exact) / exact)
            print("GNC/%s: %d cells, within %.2e of exact" % (name, len(keys), err))
            assert err <= RTOL
    # the array kernel refuses it, naming the polygon -- here the second of two
    stream_clip(0)
    square = np.array([(0., 0.), (1., 0.), (1., 1.), (0., 1.)])
    with pytest.raises(_capi.IcebinHipError, match="gridgen_stream_clip=0: polygon 1 is not convex") as ei:
        gg.make_exchange_grid(xe, ye, [square, poly], [3, 7])
    assert ei.value.code == _capi.IBH_EINVAL
    # the library works afterwards, and a convex call still runs the array kernel
    ok = gg.make_exchange_grid(xe, ye, [square], [3])
    stream_clip(-1)
    ok2 = gg.make_exchange_grid(xe, ye, [square], [3])
    assert same(ok, ok2) and len(ok["overlaps"]) >= 1 and abs(ok["overlaps"].sum() - 1.0) <= 1e-15
    # mixed with convex polygons the whole call is streamed
    both = gg.make_exchange_grid(xe, ye, [square, poly], [3, 7])
    idx, area = restated(xe, ye, [square, poly], [3, 7])
    assert np.array_equal(both["indices"], idx) and np.array_equal(u64(both["overlaps"]), u64(area))
    # a clockwise convex polygon still gives no cells
    assert len(gg.make_exchange_grid(xe, ye, [square[::-1]], [3])["overlaps"]) == 0


# ---- L1 ------------------------------------------------------------------------------------------------------------------------
def check_l1(ex, want, what, slack=0.0):
    keys = sorted(want)
    assert [tuple(k) for k in ex.indices.tolist()] == keys, what             # every pair once, none missed, in (iA, iTri) order
    ref = np.array([want[k][0] for k in keys])
    err = np.abs(ex.areas - ref)
    print("%s: %d exchange cells, areas within %.2e relative of the exact ones" % (what, len(keys), np.max(err / ref) if len(keys) else 0.0))
    assert np.all(err <= RTOL * ref + slack), what
    assert np.all(ex.areas > 0) and ex.vptr[0] == 0 and ex.vptr[-1] == len(ex.qx)
    return keys


def test_l19_piece_limit(l1):
    L = cc.l19()
    mesh = l1.Mesh(L["vx"], L["vy"], L["tri"])
    ex = l1.make_exchange_grid(mesh, L["polys"], L["iA"])
    want = cc.exact_l1(L["vx"], L["vy"], L["tri"], L["polys"], L["iA"])
    keys = check_l1(ex, want, "L19")
    nv = np.diff(ex.vptr)
    assert nv.tolist() == [want[k][1] for k in keys] and nv[0] == cc.L1_CLIPV and np.sum(nv == cc.L1_CLIPV) == 1
    w = l1.compute_AvI(ex, 9, mesh)
    assert abs(math.fsum(w.wM) - math.fsum(ex.areas)) <= 1e-13 * math.fsum(ex.areas)


@pytest.fixture(scope="module")
def lb_built(l1):
    B = cc.lb()
    mesh = l1.Mesh(B["vx"], B["vy"], B["tri"])
    return B, mesh, l1.make_exchange_grid(mesh, B["polys"], B["iA"])


def test_lb_every_pair_once(l1, lb_built):
    B, mesh, ex = lb_built
    keys = check_l1(ex, B["exact"], "LB")
    assert np.diff(ex.vptr).max() <= 7
    again = l1.make_exchange_grid(mesh, B["polys"], B["iA"])
    for k in ("indices", "areas", "vptr", "qx", "qy"):
        assert getattr(ex, k).tobytes() == getattr(again, k).tobytes(), k
    # every GCM cell lies inside the mesh: its pieces add up to its area (each within 1e-12 of its own)
    worst = 0.0
    for n, (poly, a) in enumerate(zip(B["polys"], B["iA"])):
        area = 1.0 if n < 256 else 128.0
        tot = math.fsum(ex.areas[ex.indices[:, 0] == a])
        worst = max(worst, abs(tot - area) / area)
    print("LB: per GCM cell, |sum of pieces - area| <= %.2e x area" % worst)
    assert worst <= RTOL and len(keys) > 1000


@pytest.mark.parametrize("ntri", cc.LB_NTRI)
def test_lb_sub_meshes(l1, ntri):
    B = cc.lb()
    mesh = l1.Mesh(B["vx"], B["vy"], B["tri"][:ntri])
    ex = l1.make_exchange_grid(mesh, B["polys"], B["iA"])
    check_l1(ex, {k: v for k, v in B["exact"].items() if k[1] < ntri}, "LB/ntri=%d" % ntri)


def test_lb_one_polygon_one_bin(l1, lb_built):
    B, mesh, _ = lb_built
    for n in (256, 0):
        ex = l1.make_exchange_grid(mesh, [B["polys"][n]], [B["iA"][n]])
        keys = check_l1(ex, {k: v for k, v in B["exact"].items() if k[0] == B["iA"][n]}, "LB/npoly=1 (polygon %d)" % n)
        assert len(keys) >= 1


# ---- L1: LNC -------------------------------------------------------------------------------------------------------------------
def test_lnc_refusals_and_the_near_collinear_quad(l1):
    N = cc.lnc()
    B = cc.l19()
    mesh = l1.Mesh(B["vx"], B["vy"], B["tri"])
    square = np.array([(0., 0.), (1., 0.), (1., 1.), (0., 1.)])
    for name, words in (("reflex", "polygon 1 is not counter-clockwise convex: the turn at vertex 3 is reflex"),
                        ("clockwise", "polygon 1 is not counter-clockwise convex: the turn at vertex "),
                        ("star", "polygon 1 is not convex: its edges wind more than once")):
        with pytest.raises(_capi.IcebinHipError, match=words) as ei:
            l1.make_exchange_grid(mesh, [square, N[name]], [2, 5])
        assert ei.value.code == _capi.IBH_EINVAL, name
    # straight to rounding at 2e6: accepted.  The bar is test_gpu_l1.py's for jit9_far: 1e-12, and the area a piece gains when
    # every vertex moves by one ulp of the largest coordinate (the polygon is stored in doubles at 2e6): perimeter x ulp
    m = N["far_mesh"]
    far_mesh = l1.Mesh(m["vx"], m["vy"], m["tri"])
    ex = l1.make_exchange_grid(far_mesh, [N["far"]], [4])
    want = cc.exact_l1(m["vx"], m["vy"], m["tri"], [N["far"]], [4])
    keys = sorted(want)
    slack = np.array([want[k][2] for k in keys]) * np.spacing(np.abs(N["far"]).max())
    assert check_l1(ex, want, "LNC/far", slack) == [(4, 0), (4, 1), (4, 2), (4, 3)]
    # compute_AvI works afterwards
    w = l1.compute_AvI(ex, 5, far_mesh)
    assert w.nnz == 5 and abs(math.fsum(w.wM) - math.fsum(ex.areas)) <= 1e-13 * math.fsum(ex.areas)
