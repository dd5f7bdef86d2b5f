"""CPU checks of the lon/lat path's float64 restatement (tests/lonlat_restatement.py) against the 50-digit golden file and
against exact clipping, and of the sproj parser.  The measured errors are the source of the GPU tests' tolerances
(tests/test_gpu_lonlat.py) and are written down in DESIGN.md 13."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lonlat_cases as llc          # noqa: E402
import lonlat_restatement as llr    # noqa: E402
from icebin_amd import _capi        # noqa: E402
from icebin_amd import gridgen as gg    # noqa: E402


def restatement_errors():
    """(worst coordinate error / a, worst area error / area) of the restatement against the golden file."""
    g = np.load(llc.GOLDEN)
    coord = area = 0.0
    for name, s in llc.SPROJ.items():
        p = gg.parse_sproj(s)
        x, y = llr.project(llr.stere_setup(p), g[name + "/lon"], g[name + "/lat"])
        coord = max(coord, np.max(np.abs(x - g[name + "/x"])) / p["a"], np.max(np.abs(y - g[name + "/y"])) / p["a"])
    for tag, spec, pname in (("north", llc.small_spec(points_in_side=2), "searise_north"), ("south", llc.south_spec(points_in_side=2), "searise_south")):
        c = llr.cells(spec, g["areas_%s/cells" % tag], llr.stere_setup(gg.parse_sproj(llc.SPROJ[pname])))
        for key, ref in (("native_area", g["areas_%s/native" % tag]), ("proj_area", g["areas_%s/proj" % tag])):
            area = max(area, np.max(np.abs(c[key] - ref) / np.abs(ref)))
    return float(coord), float(area)


def test_restatement_against_golden():
    coord, area = restatement_errors()
    print("restatement vs 50-digit golden: worst coordinate error / a = %.3e, worst area error / area = %.3e" % (coord, area))
    # double precision: a handful of roundings of unit-size quantities, amplified by nothing (|x|, |y| <= a few a)
    assert coord < 1e-14 and area < 1e-13


@pytest.mark.parametrize("name", sorted(llc.ANCHORS))
def test_snyder_anchor(name):
    """Snyder's worked examples (1987, pp. 313-316) to 0.05 m.  The polar one is a SOUTH-polar case and pins the sign of x there:
    for the south pole only the latitude changes sign on the way in (PJ_stere.c: phi and cos(lam)); negating the longitude
    difference as well would mirror x (+1540033.61 m for Snyder's -1540033.6 m)."""
    a = llc.ANCHORS[name]
    x, y = llr.stere_forward(llr.stere_setup(a["params"]), a["lon"], a["lat"])
    g = np.load(llc.GOLDEN)["anchor/" + name]
    print("anchor %s: restatement (%.4f, %.4f), 50 digits (%.4f, %.4f), Snyder (%.1f, %.1f)" % (name, x, y, g[0], g[1], a["x"], a["y"]))
    assert abs(x - g[0]) < 1e-6 and abs(y - g[1]) < 1e-6
    assert abs(x - a["x"]) <= 0.05 and abs(y - a["y"]) <= 0.05


# ---- the streamed clip against exact clipping ------------------------------------------------------------------------------
def exact_clip_area(px, py, x0, x1, y0, y1):
    """Sutherland-Hodgman in Fractions of the float inputs: the exact area of the polygon inside the rectangle."""
    F = Fraction
    poly = [(F(float(x)), F(float(y))) for x, y in zip(px, py)]
    for axis, bound, lower in ((0, F(float(x0)), True), (0, F(float(x1)), False), (1, F(float(y0)), True), (1, F(float(y1)), False)):
        out = []
        for k in range(len(poly)):
            a, b = poly[k], poly[(k + 1) % len(poly)]
            ina = a[axis] >= bound if lower else a[axis] <= bound
            inb = b[axis] >= bound if lower else b[axis] <= bound
            if ina:
                out.append(a)
            if ina != inb:
                t = (bound - a[axis]) / (b[axis] - a[axis])
                out.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])))
        poly = out
        if not poly:
            return F(0)
    s = F(0)
    for k in range(len(poly)):
        s += poly[k - 1][0] * poly[k][1] - poly[k][0] * poly[k - 1][1]
    return s / 2


def clip_pair(scale=1.0, shift=(0.0, 0.0)):
    """An 9 x 7 ice grid of 1 x 1.25 cells around the origin under rotated quadrilaterals, an octagon with a concave side and a
    24-gon; scaled and shifted on request (the shifted case: x 1000, shift (-6e5, -2e6) -- polar-stereographic metres)."""
    rng = np.random.default_rng(5)
    xe, ye = -4.5 + np.arange(10) * 1.0, -4.0 + np.arange(8) * 1.25
    polys = []
    for k in range(6):
        c, r, th = rng.uniform(-3, 3, 2), rng.uniform(0.8, 2.5), rng.uniform(0, 2 * np.pi)
        ang = th + np.array([0, .5, 1, 1.5]) * np.pi + rng.uniform(-.3, .3, 4)
        polys.append(np.stack([c[0] + r * np.cos(ang), c[1] + r * np.sin(ang)], 1))
    ang = np.linspace(0, 2 * np.pi, 8, endpoint=False)
    rad = np.array([2.2, 2.2, 0.9, 2.2, 2.2, 2.2, 2.2, 2.2])
    polys.append(np.stack([0.3 + rad * np.cos(ang), -0.2 + rad * np.sin(ang)], 1))
    ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
    polys.append(np.stack([-1.1 + 3.1 * np.cos(ang), 0.7 + 2.6 * np.sin(ang)], 1))
    xe, ye = xe * scale + shift[0], ye * scale + shift[1]
    polys = [p * scale + np.asarray(shift) for p in polys]
    return xe, ye, polys


def stream_clip_error(scale, shift):
    """Worst |streamed restatement - exact| / ice-cell area over every candidate pair of the grid pair."""
    xe, ye, polys = clip_pair(scale, shift)
    worst = Fraction(0)
    for p in polys:
        for ix in range(len(xe) - 1):
            for iy in range(len(ye) - 1):
                a = llr.clip_area(p[:, 0], p[:, 1], xe[ix], xe[ix + 1], ye[iy], ye[iy + 1])
                ex = exact_clip_area(p[:, 0], p[:, 1], xe[ix], xe[ix + 1], ye[iy], ye[iy + 1])
                cell = (Fraction(float(xe[ix + 1])) - Fraction(float(xe[ix]))) * (Fraction(float(ye[iy + 1])) - Fraction(float(ye[iy])))
                worst = max(worst, abs(Fraction(a) - ex) / cell)
    return float(worst)


# the bound the GPU test holds the streamed kernel to (tests/test_gpu_lonlat.py): each of <= ~30 shoelace terms and <= 8
# intersections rounds products of cell-sized numbers, <= 1 ulp of the cell's area each; the subtraction of the corner adds
# half an ulp of the COORDINATE, i.e. (distance from origin / cell size) * 2^-53 of the cell's size per vertex
def stream_clip_bound(origin_over_cell):
    return 64 * 2.0 ** -52 + 8 * origin_over_cell * 2.0 ** -53


# k_gg_clip, for comparisons with it: the same number of terms on ABSOLUTE coordinates, every product up to (distance from the
# origin)^2 -- relative to the cell's area, (origin / cell size)^2 ulps per term
def array_clip_bound(origin_over_cell):
    return 64 * 2.0 ** -52 * origin_over_cell ** 2


def test_stream_clip_against_exact():
    near = stream_clip_error(1.0, (0.0, 0.0))
    far = stream_clip_error(1000.0, (-6e5, -2e6))
    print("streamed clip vs exact, relative to the ice cell's area: near the origin %.3e, x1000 shifted (-6e5, -2e6) %.3e" % (near, far))
    assert near <= stream_clip_bound(5.0) and far <= stream_clip_bound(2.1e6 / 1000.0)


def test_parse_sproj_matches_the_library_and_names_unknown_keys():
    import ctypes as C
    from icebin_amd.build import build_library
    build_library()
    L = _capi.lib()
    for s in list(llc.SPROJ.values()) + ["+proj=stere +lat_0=90 +lat_ts=70 +lon_0=-45 +k=1 +x_0=0 +y_0=0 +datum=WGS84 +units=m +no_defs",
                                         "proj=stere lat_0=-90 lon_0=12.5 k_0=0.994 x_0=2000000 y_0=-3e5 a=6378137 b=6356752.3"]:
        sp = _capi.StereParams()
        assert L.ibh_parse_sproj(s.encode(), C.byref(sp)) == 0, L.ibh_last_error()
        p = gg.parse_sproj(s)
        for k in ("lat_0", "lon_0", "lat_ts", "k_0", "x_0", "y_0", "a", "b", "has_lat_ts"):
            assert getattr(sp, k) == p[k], (s, k, getattr(sp, k), p[k])
    assert gg.parse_sproj(llc.SPROJ["searise_north"])["a"] == 6378137.0
    for s, key in (("+proj=stere +lat_0=90 +towgs84=0,0,0", "towgs84"), ("+proj=laea +lat_0=90", "proj"), ("+proj=stere +ellps=GRS80", "ellps"),
                   ("+proj=stere +lat_0=abc", "lat_0"), ("+proj=stere +units=km", "units"), ("+lat_0=90", "proj")):
        sp = _capi.StereParams()
        assert L.ibh_parse_sproj(s.encode(), C.byref(sp)) == _capi.IBH_EINVAL
        assert "'%s'" % key in L.ibh_last_error().decode()
        with pytest.raises(_capi.IcebinHipError, match="'%s'" % key) as ei:
            gg.parse_sproj(s)
        assert ei.value.code == _capi.IBH_EINVAL


def test_spherical_clip_lonlat_and_cell_indices():
    for indices in ((1, 0), (0, 1)):
        spec = llc.small_spec(indices=indices)
        every = llc.all_cells(spec)
        assert len(set(every.tolist())) == 6 * 4 + 2 and every[0] == 0 and every[-1] == spec.nlat * 6 + 5 < spec.nA
        for idx in every:
            assert llr.decode(spec, int(idx)) is not None
        keep = gg.spherical_clip_lonlat(spec, -80., 60., -60., 70.)
        want = sorted(spec.cell_index(i, j) for j in (1, 2) for i in range(6) if spec.lonb[i] <= -60. and spec.lonb[i + 1] >= -80.)
        assert keep.tolist() == want and len(want) > 0
        assert gg.spherical_clip_lonlat(spec, -180., 85., 180., 90.).tolist() == sorted(
            [spec.cell_index(i, 3) for i in range(6)] + [spec.north_cap_index])
