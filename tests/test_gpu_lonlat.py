"""GPU tests of the path from grid specs: lonlat.hip's projection and cells against the 50-digit golden file and the float64
restatement, gridgen.hip's streamed clip bit for bit against its restatement, and regridder_from_specs against
ibh_regridder_create fed with the copied-out arrays."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lonlat_cases as llc              # noqa: E402
import lonlat_restatement as llr        # noqa: E402
import test_lonlat_restatement as cpu   # noqa: E402
from icebin_amd import _capi, GCMRegridder      # noqa: E402
from icebin_amd import gridgen as gg    # noqa: E402
from icebin_amd._capi import check, lib, ptr    # noqa: E402

pytestmark = pytest.mark.gpu
u64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)     # noqa: E731


@pytest.fixture(scope="module")
def tol():
    """4 x the restatement's own measured error against the golden file: (coordinates / a, areas / area)."""
    coord, area = cpu.restatement_errors()
    return 4 * coord, 4 * area


@pytest.fixture
def stream_clip():
    def force(v):
        check(lib().ibh_set_tuning(b"gridgen_stream_clip", v))
    yield force
    force(-1)


def test_projection_and_areas_against_golden(tol):
    g = np.load(llc.GOLDEN)
    worst = 0.0
    for name, s in llc.SPROJ.items():
        x, y = gg.project(s, g[name + "/lon"], g[name + "/lat"])
        a = gg.parse_sproj(s)["a"]
        err = max(np.max(np.abs(x - g[name + "/x"])), np.max(np.abs(y - g[name + "/y"]))) / a
        print("%s: device vs golden, worst coordinate error / a = %.3e (tolerance %.3e)" % (name, err, tol[0]))
        worst = max(worst, err)
    worst_area = 0.0
    for tag, spec, pname in (("north", llc.small_spec(points_in_side=2), "searise_north"), ("south", llc.south_spec(points_in_side=2), "searise_south")):
        c = gg.lonlat_cells(spec, g["areas_%s/cells" % tag], llc.SPROJ[pname]).get()
        for key, ref in (("native_area", g["areas_%s/native" % tag]), ("proj_area", g["areas_%s/proj" % tag])):
            worst_area = max(worst_area, np.max(np.abs(c[key] - ref) / np.abs(ref)))
    print("device vs golden, worst area error / area = %.3e (tolerance %.3e)" % (worst_area, tol[1]))
    assert worst <= tol[0] and worst_area <= tol[1]


CELL_CASES = [(6, 1, (1, 0)), (6, 2, (0, 1)), (6, 4, (1, 0)), (6, 5, (0, 1)), (6, 3, (1, 0)), (4, 2, (0, 1))]


@pytest.mark.parametrize("nlon,n,indices", CELL_CASES)
@pytest.mark.parametrize("south", [False, True])
def test_cells_order_lonlat_and_areas(nlon, n, indices, south, tol):
    spec = (llc.south_spec if south else llc.small_spec)(nlon, n, indices)
    sproj = llc.SPROJ["searise_south" if south else "searise_north"]
    realised = llc.all_cells(spec)
    if nlon == 6 and n != 3:
        realised = realised[[0, 2, 3, 7, 11, 12, 20, len(realised) - 1]]      # a subset that skips cells; both caps stay
    c = gg.lonlat_cells(spec, realised, sproj, keep_lonlat=True).get(lonlat=True)
    r = llr.cells(spec, realised, llr.stere_setup(gg.parse_sproj(sproj)))
    assert np.array_equal(c["iA"], realised) and np.array_equal(c["polyptr"], r["polyptr"])
    nv = np.diff(c["polyptr"])
    assert nv[0] == nv[-1] == nlon * n and set(nv[1:-1].tolist()) == {4 * n}
    assert realised[0] == 0 and realised[-1] == spec.nlat * nlon + nlon - 1
    # vertex generation uses no libm: order and values bit for bit
    assert np.array_equal(u64(c["lon"]), u64(r["lon"])) and np.array_equal(u64(c["lat"]), u64(r["lat"]))
    a = gg.parse_sproj(sproj)["a"]
    assert max(np.max(np.abs(c["vx"] - r["vx"])), np.max(np.abs(c["vy"] - r["vy"]))) / a <= 2 * tol[0]
    assert np.max(np.abs(c["native_area"] - r["native_area"]) / np.abs(r["native_area"])) <= 2 * tol[1]
    # proj_area: the reference's shoelace of the device's own vertices, bit for bit
    mine = [llr.proj_area(c["vx"][c["polyptr"][k]:c["polyptr"][k + 1]], c["vy"][c["polyptr"][k]:c["polyptr"][k + 1]]) for k in range(len(realised))]
    assert np.array_equal(u64(c["proj_area"]), u64(mine))
    # counter-clockwise in the plane, in both hemispheres; the cap of the OTHER pole (these specs carry both caps over 40
    # degrees of one hemisphere) is walked the other way round and is left out
    own = slice(0, -1) if south else slice(1, None)
    assert np.all(c["proj_area"][own] > 0) and np.all(c["native_area"] > 0)


def hand_polygons():
    """3, 16, 17 and 40 vertices; a concave one; one with an edge on an ice-cell edge; one inside a single ice cell; one outside
    the grid.  Ice grid: 7 x 5 cells of 2 x 3 from (-7, -6)."""
    xe, ye = -7. + 2. * np.arange(8), -6. + 3. * np.arange(6)
    def ring(n, cx, cy, rx, ry, ph=0.1):
        t = ph + np.linspace(0, 2 * np.pi, n, endpoint=False)
        return np.stack([cx + rx * np.cos(t), cy + ry * np.sin(t)], 1)
    polys = [np.array([[-6.3, -5.2], [1.7, -4.1], [-2.2, 2.9]]), ring(16, 1.1, 0.4, 4.3, 3.7), ring(17, -1.3, 1.2, 5.1, 2.2), ring(40, 0.2, -0.3, 6.1, 5.3),
             np.array([[-5., -4.], [4., -4.], [4., 5.], [0.5, 5.], [0.5, -1.], [-0.5, -1.], [-0.5, 5.], [-5., 5.]]),       # concave (a U)
             np.array([[-3., -3.], [1., -3.], [1., 3.], [-3., 3.]]),      # edges on ice-cell edges
             np.array([[-0.7, 0.3], [0.6, 0.5], [0.1, 2.4]]),             # inside cell [-1, 1] x [0, 3]
             ring(5, 40., 40., 3., 3.)]                                   # outside the grid
    return xe, ye, polys


def test_stream_clip_bitwise_on_hand_polygons(stream_clip):
    xe, ye, polys = hand_polygons()
    polyptr = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int32)
    v = np.concatenate(polys)
    iA = np.arange(len(polys)) * 3 + 1
    stream_clip(1)
    for xf in (False, True):
        ex = gg.make_exchange_grid(xe, ye, polys, iA, x_fastest=xf)
        idx, area = llr.exchange_grid(xe, ye, polyptr, v[:, 0], v[:, 1], iA, xf)
        assert np.array_equal(ex["indices"], idx) and np.array_equal(u64(ex["overlaps"]), u64(area))
        got = {int(a): ex["overlaps"][ex["indices"][:, 0] == a] for a in iA}
        assert len(got[int(iA[6])]) == 1 and len(got[int(iA[7])]) == 0 and len(got[int(iA[5])]) == 4
    stream_clip(-1)      # above 16 vertices the default call runs the streamed kernel: same bytes
    ex2 = gg.make_exchange_grid(xe, ye, polys, iA, x_fastest=True)
    assert np.array_equal(ex2["indices"], ex["indices"]) and np.array_equal(u64(ex2["overlaps"]), u64(ex["overlaps"]))
    stream_clip(0)
    with pytest.raises(_capi.IcebinHipError, match="gridgen_stream_clip=0"):
        gg.make_exchange_grid(xe, ye, polys, iA)


def ice_grid(shift=False):
    """24 x 30 cells of 20 km under the 6 x 4 grid (SeaRISE north puts lon -99..-36, lat 48..88 at x -3.5e6..0.2e6, y -3.3e6..-0.2e6)."""
    x0, y0 = (-2.2e6, -2.6e6) if shift else (-0.24e6, -0.7e6)
    return x0 + 2e4 * np.arange(25), y0 + 2e4 * np.arange(31)


@pytest.mark.parametrize("n", [1, 5])
def test_stream_clip_bitwise_on_cells_and_invariant(n, stream_clip):
    spec = llc.small_spec(6, n)
    sproj = llc.SPROJ["searise_north"]
    cells = gg.lonlat_cells(spec, llc.all_cells(spec), sproj)
    c = cells.get()
    for shift in (False, True):
        xe, ye = ice_grid(shift)
        ex = gg.make_exchange_grid_lonlat(cells, xe, ye)
        idx, area = llr.exchange_grid(xe, ye, c["polyptr"], c["vx"], c["vy"], c["iA"])
        assert len(area) > 100 and np.array_equal(ex["indices"], idx) and np.array_equal(u64(ex["overlaps"]), u64(area))
        polys = [np.stack([c["vx"][c["polyptr"][k]:c["polyptr"][k + 1]], c["vy"][c["polyptr"][k]:c["polyptr"][k + 1]]], 1) for k in range(cells.ncell)]
        stream_clip(1)
        ex1 = gg.make_exchange_grid(xe, ye, polys, c["iA"])
        stream_clip(-1)
        assert np.array_equal(ex1["indices"], idx) and np.array_equal(u64(ex1["overlaps"]), u64(area))
    # invariant (K9's 1e-12): a cell whose polygon lies inside the ice domain is tiled by its overlaps.  A finer, wider ice grid so
    # that several cells do: near the origin of the plane (lat ~ 88) and far from it (lat ~ 50)
    for x0, y0, nx, ny in ((-0.3e6, -0.6e6, 40, 40), (-3.6e6, -3.6e6, 190, 130)):
        xe, ye = x0 + 2e4 * np.arange(nx + 1), y0 + 2e4 * np.arange(ny + 1)
        ex = gg.make_exchange_grid_lonlat(cells, xe, ye)
        inside = 0
        for k in range(cells.ncell):
            px, py = c["vx"][c["polyptr"][k]:c["polyptr"][k + 1]], c["vy"][c["polyptr"][k]:c["polyptr"][k + 1]]
            if px.min() > xe[0] and px.max() < xe[-1] and py.min() > ye[0] and py.max() < ye[-1]:
                inside += 1
                tot = ex["overlaps"][ex["indices"][:, 0] == c["iA"][k]].sum()
                assert abs(tot - c["proj_area"][k]) <= 1e-12 * c["proj_area"][k], (k, tot, c["proj_area"][k])
        assert inside >= 1, (x0, y0)


def test_old_path_untouched(stream_clip):
    """Convex, <= 16 vertices (test_gpu_parity.py's general convex polygons, and the CPU test's grid pair near the origin): the
    default call and the forced array kernel give the same bytes; the streamed kernel gives the same indices, and areas within
    the CPU test's bound for it plus the array kernel's own rounding (absolute coordinates), relative to the ice cell's area.
    The grid pair's octagon has a concave side: the array kernel is not for it (its arrays hold n + 4 vertices, a convex
    polygon's count), so with it the default call is the streamed kernel's and forcing the array kernel is refused."""
    def turns(p):
        e = np.roll(p, -1, 0) - p
        return e[:, 0] * np.roll(e[:, 1], -1) - e[:, 1] * np.roll(e[:, 0], -1)
    rng = np.random.default_rng(11)
    xe, ye = np.cumsum(rng.uniform(0.5, 1.5, 41)), np.cumsum(rng.uniform(0.5, 1.5, 31))
    polys = []
    for k in range(12):
        c = np.array([rng.uniform(xe[8], xe[-9]), rng.uniform(ye[8], ye[-9])])
        ang = np.sort(rng.uniform(0, 2 * np.pi, rng.integers(3, 9)))
        polys.append(c + rng.uniform(2.0, 5.0) * np.stack([np.cos(ang), np.sin(ang)], axis=1))
    xe2, ye2, polys2 = cpu.clip_pair()
    small = [p for p in polys2 if len(p) <= 16]
    concave = [k for k, p in enumerate(small) if np.any(turns(p) < 0)]
    assert len(small) == 7 and concave == [6]
    iA = np.arange(len(small)) * 3 + 100
    stream_clip(0)
    with pytest.raises(_capi.IcebinHipError, match="gridgen_stream_clip=0: polygon 6 is not convex"):
        gg.make_exchange_grid(xe2, ye2, small, iA)
    stream_clip(-1)
    dflt = gg.make_exchange_grid(xe2, ye2, small, iA)
    stream_clip(1)
    st = gg.make_exchange_grid(xe2, ye2, small, iA)
    assert np.array_equal(dflt["indices"], st["indices"]) and np.array_equal(u64(dflt["overlaps"]), u64(st["overlaps"]))
    for xe, ye, polys in ((xe, ye, polys), (xe2, ye2, small[:6])):
        assert all(np.all(turns(p) > 0) for p in polys)
        iA = np.arange(len(polys)) * 3 + 100
        stream_clip(-1)
        dflt = gg.make_exchange_grid(xe, ye, polys, iA)
        stream_clip(0)
        arr = gg.make_exchange_grid(xe, ye, polys, iA)
        stream_clip(1)
        st = gg.make_exchange_grid(xe, ye, polys, iA)
        stream_clip(-1)
        assert np.array_equal(dflt["indices"], arr["indices"]) and np.array_equal(u64(dflt["overlaps"]), u64(arr["overlaps"]))
        assert np.array_equal(st["indices"], arr["indices"]) and len(arr["overlaps"]) > 50
        ny = len(ye) - 1
        ix, iy = arr["indices"][:, 1] // ny, arr["indices"][:, 1] % ny
        cell = np.diff(xe)[ix] * np.diff(ye)[iy]
        err = np.max(np.abs(st["overlaps"] - arr["overlaps"]) / cell)
        r = max(np.abs(xe).max(), np.abs(ye).max()) / min(np.diff(xe).min(), np.diff(ye).min())
        bound = cpu.stream_clip_bound(r) + cpu.array_clip_bound(r)
        print("streamed vs array kernel: worst difference / ice-cell area = %.3e (bound %.3e)" % (err, bound))
        assert err <= bound


def test_end_to_end_against_regridder_create():
    spec = llc.small_spec(6, 2, north_pole=True, south_pole=False)
    sproj = llc.SPROJ["searise_north"]
    realised = llc.all_cells(spec)
    xe, ye = ice_grid()
    hcdefs = np.array([0., 500., 1500., 3000.])
    mm = gg.regridder_from_specs(spec, realised, xe, ye, sproj, hcdefs)
    cells = gg.lonlat_cells(spec, realised, sproj)
    c = cells.get()
    ex = gg.make_exchange_grid_lonlat(cells, xe, ye)
    assert realised[-1] == spec.north_cap_index and spec.north_cap_index in ex["indices"][:, 0]
    ref = GCMRegridder(dict(nA=cells.nA, to_sparse=c["iA"], native_area=c["native_area"]), hcdefs, True)
    ref.add_sheet("ice", dict(nI=24 * 30, centroid_xy=gg.ice_centroids(xe, ye)), ex, "Z_INTERP", c["proj_area"])
    sheet = mm._sheets["ice"]
    idx, area, proj = sheet.arrays
    assert np.array_equal(idx.reshape(-1, 2), ex["indices"]) and np.array_equal(u64(area), u64(ex["overlaps"]))
    assert np.array_equal(mm._A_to_sparse, c["iA"]) and np.array_equal(u64(mm._A_native), u64(c["native_area"]))
    assert np.array_equal(u64(proj), u64(c["proj_area"]))
    for which in ("native", "proj"):
        assert np.array_equal(u64(mm.wA("ice", which)), u64(ref.wA("ice", which)))
    em = 100. + 10. * np.arange(24 * 30, dtype=np.float64) % 2500.
    rm, rr = mm.regrid_matrices("ice", em, scale=True, correctA=True), ref.regrid_matrices("ice", em, scale=True, correctA=True)
    mats = {}
    for name in ("AvI", "IvA"):
        w, o = rm.matrix(name), rr.matrix(name)
        a, b = w.coo_dense(), o.coo_dense()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(u64(a[2]), u64(b[2])), name
        assert np.array_equal(u64(w.wM), u64(o.wM)) and np.array_equal(u64(w.Mw), u64(o.Mw))
        assert np.array_equal(w.dim(0), o.dim(0)) and np.array_equal(w.dim(1), o.dim(1))
        mats[name] = w
    ones = mats["AvI"].apply(np.ones((1, mats["AvI"].ncol_d)), force_conservation=False)
    back = mats["IvA"].apply(ones, force_conservation=False)
    seen = np.isfinite(back)      # ice cells under no realised GCM cell keep the fill value
    assert seen.sum() > 100 and np.max(np.abs(back[seen] - 1.0)) <= 1e-12


def test_end_to_end_south():
    """SeaRISE's southern projection: the south cap (18 vertices) and its neighbours over a 30 x 30 ice grid round the pole."""
    spec = llc.south_spec(6, 3, north_pole=False, south_pole=True)
    realised = llc.all_cells(spec)
    xe = ye = -0.3e6 + 2e4 * np.arange(31)
    mm = gg.regridder_from_specs(spec, realised, xe, ye, llc.SPROJ["searise_south"], [0., 2000., 4000.])
    idx, area, proj = mm._sheets["ice"].arrays
    assert np.all(proj > 0) and np.all(area > 0) and spec.south_cap_index in idx.reshape(-1, 2)[:, 0]
    cells = gg.lonlat_cells(spec, realised, llc.SPROJ["searise_south"]).get()
    r = llr.exchange_grid(xe, ye, cells["polyptr"], cells["vx"], cells["vy"], cells["iA"])
    assert np.array_equal(idx.reshape(-1, 2), r[0]) and np.array_equal(u64(area), u64(r[1]))
    rm = mm.regrid_matrices("ice", np.full(900, 1000.), scale=True, correctA=True)
    AvI, IvA = rm.matrix("AvI"), rm.matrix("IvA")
    back = IvA.apply(AvI.apply(np.ones((1, AvI.ncol_d)), force_conservation=False), force_conservation=False)
    seen = np.isfinite(back)
    assert seen.sum() > 50 and np.max(np.abs(back[seen] - 1.0)) <= 1e-12


def test_bad_arguments_are_einval_and_leave_null():
    spec = llc.small_spec(6, 1)
    sp = _capi.StereParams()
    assert lib().ibh_parse_sproj(b"+proj=stere +lat_0=90 +nadgrids=@null", C.byref(sp)) == _capi.IBH_EINVAL
    assert b"'nadgrids'" in lib().ibh_last_error()
    with pytest.raises(_capi.IcebinHipError, match="nadgrids") as ei:
        gg.regridder_from_specs(spec, llc.all_cells(spec), *ice_grid(), "+proj=stere +lat_0=90 +nadgrids=@null", [0., 1.])
    assert ei.value.code == _capi.IBH_EINVAL
    good = gg._stere_params(llc.SPROJ["searise_north"])
    for realised, n in (([5, 3], 1), ([3, 5], 0), ([3, 3], 1), ([spec.nA + 7], 1)):
        r = np.asarray(realised, np.int64)
        d = _capi.LonLatCellsDesc(nlonb=7, nlatb=5, lonb=ptr(spec.lonb).value, latb=ptr(spec.latb).value, indices=(C.c_int32 * 2)(1, 0),
                                  south_pole=1, north_pole=1, points_in_side=n, eq_rad=6371000., nrealised=len(r), realised=ptr(r).value,
                                  proj=C.pointer(good), keep_lonlat=0)
        h = C.c_void_p(12345)
        assert lib().ibh_lonlat_cells_create(C.byref(d), C.byref(h)) == _capi.IBH_EINVAL, (realised, n)
        assert h.value is None
    h = C.c_void_p(12345)
    d = _capi.LonLatRegridderDesc(cells=None, nx=2, ny=2)
    assert lib().ibh_regridder_create_lonlat(C.byref(d), None, C.byref(h)) == _capi.IBH_EINVAL and h.value is None
