"""make_topoO (modele/topo_base.cpp:263-809 with callZ, :20-221): the base ocean-grid TOPO planes FOCEAN, FLAKE, FGRND, FGICE, ZATMO,
... from the four 1' planes FGICE1m / ZICETOP1m / ZSOLG1m / FOCEAN1m and the lake plane FLAKES, with every plane resident in HBM
(ibh_make_topoo_*).  The result feeds merge_topoO / make_topoA / update_topo as it is."""
import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _capi
from ._arrays import dptr, einval, named_planes, stream_arg, to_device
from ._capi import check, lib

MAX_TILE = 8192                 # IBH_MAKE_TOPOO_MAX_TILE: fine cells of a tile sorted in LDS; larger tiles take the long path
# the reference's order of out.add (:275-377), with the attributes it gives
ATTRS = OrderedDict([
    ("FOCEAN", OrderedDict(description="0 or 1, Bering Strait 1 cell wide", units="1", source="GISS 1Qx1")),
    ("FLAKE", OrderedDict(description="Lake Surface Fraction", units="0:1", sources="GISS 1Qx1")),
    ("FGRND", OrderedDict(description="Ground Surface Fraction", units="0:1", sources="GISS 1Qx1")),
    ("FGICE", OrderedDict(description="Glacial Ice Surface Fraction", units="0:1", sources="GISS 1Qx1")),
    ("FGICE_greenland", OrderedDict(description="Greenland Ice Surface Fraction", units="0:1", sources="GISS 1Qx1")),
    ("ZATMO", OrderedDict(description="Atmospheric Topography", units="m", sources="ETOPO2 1Qx1")),
    ("dZOCEN", OrderedDict(description="Ocean Thickness", units="m", sources="ETOPO2 1Qx1")),
    ("dZLAKE", OrderedDict(description="Lake Thickness", units="m", sources="ETOPO2 1Qx1")),
    ("dZGICE", OrderedDict(description="Glacial Ice Thickness", units="m", sources="Ekholm,Bamber")),
    ("ZSOLDG", OrderedDict(description="Solid Ground Topography", units="m", sources="ETOPO2 1Qx1")),
    ("ZICETOP", OrderedDict(description="Atmospheric Topography (Ice-Covered Regions Only)", units="m", sources="ETOPO2 1Qx1")),
    ("ZLAND_MIN", OrderedDict(description="Minimum land/ice topography in this cell (not computed)", units="m", sources="ETOPO2 1Qx1")),
    ("ZLAND_MAX", OrderedDict(description="Maximum land/ice topography in this cell (not computed)", units="m", sources="ETOPO2 1Qx1")),
    ("ZSGLO", OrderedDict(description="Lowest Solid Topography", units="m", sources="ETOPO2 1Qx1")),
    ("ZLAKE", OrderedDict(description="Lake Surface Topography", units="m", sources="ETOPO2 1Qx1")),
    ("ZGRND", OrderedDict(description="Topography Break between Ground and GIce", units="m", sources="ETOPO2 1Qx1")),
    ("ZSGHI", OrderedDict(description="Highest Solid Topography", units="m", sources="ETOPO2 1Qx1")),
    ("FOCEANF", OrderedDict(description="Fractional ocean ocver", units="1", sources="GISS 1Qx1")),
    ("FGICEF", OrderedDict(description="Glacial Ice Surface Fraction (Ocean NOT rounded)", units="0:1", sources="GISS 1Qx1")),
    ("ZATMOF", OrderedDict(description="Atmospheric Topography", units="m", sources="ETOPO2 1Qx1")),
])
PLANES = tuple(ATTRS)
# ibh_make_topoo_status: the two fatal conditions (count, first cell), then the reference's stderr warnings as counts
COUNTS = ("FGICE_low", "FGICE_high", "FLAKE_reduced", "FGRND_range", "dZOCEN_nonpositive", "FLAKE_one")


def _ij(cells, what):
    """A list of 1-based (i, j) as int32 [n, 2]."""
    a = np.asarray(list(cells), np.int64).reshape(-1, 2) if len(cells) else np.zeros((0, 2), np.int64)
    if a.size and (np.abs(a) >= 2 ** 31).any():
        raise einval("%s: an entry overflows int32" % what)
    return np.ascontiguousarray(a, np.int32)


def fatal_message(kind, hspecI, hspecO, J, I):
    """The reference's message (:85-89, :146-148) for ocean cell (I, J), 1-based."""
    IMAX = 1 if J in (1, hspecO.jm) else hspecO.im
    J11, J1M = (J - 1) * hspecI.jm // hspecO.jm + 1, J * hspecI.jm // hspecO.jm
    I11, I1M = (I - 1) * hspecI.im // hspecO.im + 1, (hspecI.im if IMAX == 1 else I * hspecI.im // hspecO.im)
    if kind == "ocean":
        return ("Ocean cell FOCEAN(%d,%d)=%g has no ocean area on 2-minute grid; I11,I1M,J11,J1M = %d,%d,%d,%d"
                % (I, J, 1., I11, I1M, J11, J1M))
    return "Continental cell (%d,%d) has no continental area on 2-minute grid. (%d-%d, %d-%d)" % (I, J, I11, I1M, J11, J1M)


class TopoO(_capi.Handle):
    """What make_topoO returns: the 20 planes under the reference's names (PLANES), torch.float64 CUDA tensors [jmO, imO], and
    .counts, the reference's stderr warnings as counts (COUNTS)."""
    _destroy = "ibh_make_topoo_destroy"

    def __init__(self, hspecI, hspecO, hspecS):
        self.hspecI, self.hspecO, self.hspecS = hspecI, hspecO, hspecS
        self.counts = None

    def topoo(self):
        """The planes as the dict merge_topoO / make_topoA / update_topo take (they stay in HBM)."""
        return OrderedDict((n, getattr(self, n)) for n in PLANES)

    def write(self, fname):
        """lon, lat and the planes over (jm, im) through ncio, with the reference's attributes (:275-377)."""
        from . import ncio
        O = self.hspecO
        ds = ncio.Dataset()
        dj, di = ds.add_dim("jm", O.jm), ds.add_dim("im", O.im)
        lon = -180. + (O.offi + np.arange(O.im, dtype=np.float64) + .5) * (360. / O.im)        # HntrSpec::lonc (GridSpec.cpp:196-210)
        half = (np.arange(O.jm // 2, dtype=np.float64) + .5) * (O.dlat / 60.)                  # HntrSpec::latc (:214-228)
        lat = np.sort(np.concatenate([half, -half]))
        ds.add_var("lon", np.float64, (di,), lon)
        ds.add_var("lat", np.float64, (dj,), lat)
        for n in PLANES:
            ds.add_var(n, np.float64, (dj, di), getattr(self, n).cpu().numpy(), ATTRS[n])
        ds.write(fname)
        return fname


def make_topoO(hspecI, hspecO, FGICE1m, ZICETOP1m, ZSOLG1m, FOCEAN1m, hspecS, FLAKES, set_to_land=(), set_to_ocean=(), resets=()):
    """_make_topoO(FGICE1m, ZICETOP1m, ZSOLG1m, FOCEAN1m, FLAKES) (topo_base.cpp:263-809) with the grids as arguments.  hspecI: the
    fine grid of the four int16 planes [jmI, imI] (the reference's g1mx1m), hspecO: the ocean grid of the outputs (g1qx1), hspecS:
    the grid of FLAKES, float64 [jmS, imS] (g10mx10m); hspecI must nest in hspecO, whose sizes must be even.  set_to_land /
    set_to_ocean: 1-based (i, j) cells of SET_TO (:416-494); resets: (elevation, [(i, j), ...]) groups (:231-248); the reference's
    own lists for g1qx1 are in tests/golden/make_topoo_g1qx1_cells.json.  The planes are all host numpy arrays (uploaded once in
    their own width) or all torch CUDA tensors (read in place, on torch's current stream); inputs are never written.  Returns a
    TopoO.  Raises ValueError with the reference's message for the first ocean cell without ocean area or continental cell
    without land; the semantics, line by line, are in include/icebin_hip.h."""
    planes, on_device = named_planes(
        (("FGICE1m", FGICE1m, "int16", hspecI.size), ("ZICETOP1m", ZICETOP1m, "int16", hspecI.size), ("ZSOLG1m", ZSOLG1m, "int16", hspecI.size),
         ("FOCEAN1m", FOCEAN1m, "int16", hspecI.size), ("FLAKES", FLAKES, "float64", hspecS.size)),
        "FGICE1m / ZICETOP1m / ZSOLG1m / FOCEAN1m / FLAKES: some planes are on the host and some on the device", null="first")
    land, ocean = _ij(set_to_land, "set_to_land"), _ij(set_to_ocean, "set_to_ocean")
    rij = _ij([ij for _, ijs in resets for ij in ijs], "resets")
    relev = np.ascontiguousarray([float(elev) for elev, ijs in resets for _ in ijs], np.float64)
    h = C.c_void_p()
    check(lib().ibh_make_topoo_create(C.byref(h), hspecI.im, hspecI.jm, hspecI.offi, hspecI.dlat, hspecO.im, hspecO.jm, hspecO.offi, hspecO.dlat,
                                      hspecS.im, hspecS.jm, hspecS.offi, hspecS.dlat, len(land), _capi.ptr(land), len(ocean), _capi.ptr(ocean),
                                      len(rij), _capi.ptr(rij), _capi.ptr(relev)))
    res = TopoO(hspecI, hspecO, hspecS)
    res._h = h
    import torch
    if not on_device:
        planes = [to_device(p) for p in planes]
    out = torch.empty((len(PLANES), hspecO.jm, hspecO.im), dtype=torch.float64, device=planes[0].device)
    s = stream_arg(out)
    check(lib().ibh_make_topoo_device(h, *[dptr(p) for p in planes], dptr(out), hspecO.size, s))
    st = np.zeros(10, np.int64)
    check(lib().ibh_make_topoo_status(h, s, _capi.ptr(st)))
    res._keep = planes
    first = [(int(st[k]), kind) for k, kind in ((1, "ocean"), (3, "continental")) if st[k] >= 0]
    if first:
        x, kind = min(first)
        raise ValueError(fatal_message(kind, hspecI, hspecO, x // hspecO.im + 1, x % hspecO.im + 1))
    res.counts = OrderedDict(zip(COUNTS, (int(v) for v in st[4:])))
    for k, n in enumerate(PLANES):
        setattr(res, n, out[k])
    return res
