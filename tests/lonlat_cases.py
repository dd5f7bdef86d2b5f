"""The cases the lon/lat tests share: the reference's projection strings, the small grid specs and the sample points of the
golden file (tests/golden/lonlat_reference.npz, written by tests/golden/make_lonlat_reference.py)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lonlat_reference.npz")

SPROJ = {
    "searise_north": "+proj=stere +lon_0=-39 +lat_0=90 +lat_ts=71.0 +ellps=WGS84",                              # searise_grid.cpp:113
    "searise_south": "+proj=stere +lon_0=0 +lat_0=-90 +lat_ts=71.0 +ellps=WGS84",                               # searise_grid.cpp:119
    "mar_oblique": "+proj=stere +lon_0=-40.0 +lat_0=70.5 +lat_ts=0.0 +k=1.0 +a=6371229 +b=6371129 +no_defs",    # mar_grid.cpp:116
    "sphere": "+proj=stere +lat_0=90 +lon_0=-45 +lat_ts=70 +R=6371000 +units=m",
}
# Snyder 1987's two worked ellipsoidal examples (pp. 313-316, quoted from memory): International and Clarke 1866 ellipsoids
ANCHORS = {
    "polar": dict(params=dict(lat_0=-90., lon_0=-100., lat_ts=-71., has_lat_ts=1, k_0=1., x_0=0., y_0=0., a=6378388.0,
                              b=6378388.0 * (1 - 1 / 297.0)), lon=150., lat=-75., x=-1540033.6, y=-560526.4),
    "oblique": dict(params=dict(lat_0=40., lon_0=-100., lat_ts=0., has_lat_ts=0, k_0=0.9999, x_0=0., y_0=0., a=6378206.4,
                                b=6378206.4 * (1 - 0.00676866) ** .5), lon=-90., lat=30., x=971630.8, y=-1063049.3),
}


def sample_points(name, p):
    """~200 (lon, lat) per projection: random ones in the projection's hemisphere, points within 1e-6 degree of the pole, on
    the central meridian, and with lon - lon_0 beyond +-180 degrees."""
    rng = np.random.default_rng(sorted(SPROJ).index(name) + 11)
    lat0, lon0 = p["lat_0"], p["lon_0"]
    n = 170
    if abs(lat0) == 90:
        s = 1. if lat0 > 0 else -1.
        lat = s * rng.uniform(30, 90, n)
        lon = rng.uniform(-180, 180, n)
        pole = [(lon0 + d, s * (90 - 1e-6)) for d in (0., 37., -120., 180.)] + [(lon0 + 10., s * (90 - 1e-9)), (lon0 - 77., s * 90.)]
    else:
        lat = np.clip(lat0 + rng.uniform(-40, 40, n), -89, 89)
        lon = lon0 + rng.uniform(-80, 80, n)
        pole = [(lon0 + d, 90 - 1e-6) for d in (0., 37., -120.)] + [(lon0, lat0), (lon0 + 1e-6, lat0 - 1e-6)]
    mer = [(lon0, la) for la in np.clip(lat0 + np.array([-35., -20., -5., 5., 20., 35.]), -89, 89)]
    if abs(lat0) == 90:
        mer = [(lon0, np.sign(lat0) * la) for la in (35., 50., 65., 71., 80., 89.)]
    far = [(lon0 + d, la) for d, la in zip((200., -200., 350., -350., 181., -181., 540., -359.),
                                           (np.sign(lat0) if abs(lat0) == 90 else 1.) * np.array([60., 62., 64., 66., 68., 70., 72., 74.]))]
    pts = np.array(list(zip(lon, lat)) + pole + mer + far)
    return np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1])


def small_spec(nlon=6, points_in_side=1, indices=(1, 0), south_pole=True, north_pole=True, eq_rad=6371000.):
    """nlon x 4 grid of 10-degree-ish cells over 48..88 N (nlon = 4: all the way round, 90-degree cells); the caps are flags
    of the spec.  south_spec mirrors it."""
    from icebin_amd.gridgen import GridSpec_LonLat
    lonb = -99. + np.arange(nlon + 1) * (360. / nlon if nlon == 4 else 10.5)
    latb = np.array([48., 58.5, 68., 79., 88.])
    return GridSpec_LonLat(lonb, latb, indices, south_pole, north_pole, points_in_side, eq_rad)


def south_spec(nlon=6, points_in_side=1, indices=(1, 0), south_pole=True, north_pole=True, eq_rad=6371000.):
    from icebin_amd.gridgen import GridSpec_LonLat
    lonb = -30. + np.arange(nlon + 1) * (360. / nlon if nlon == 4 else 10.5)
    latb = np.array([-88., -79., -68., -58.5, -48.])
    return GridSpec_LonLat(lonb, latb, indices, south_pole, north_pole, points_in_side, eq_rad)


def all_cells(spec):
    """Every cell of the spec, caps included, ascending."""
    out = [spec.cell_index(i, j) for j in range(len(spec.latb) - 1) for i in range(spec.nlon)]
    if spec.south_pole:
        out.append(spec.south_cap_index)
    if spec.north_pole:
        out.append(spec.north_cap_index)
    return np.asarray(sorted(out), np.int64)
