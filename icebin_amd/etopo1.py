"""etopo1_ice (modele/etopo1_ice.cpp:45-247): the global ice extent FGICE1m and the planes FOCEAN1m / ZICETOP1m / ZSOLG1m on the fine
grid, from the ETOPO1 planes FOCEAN / ZICTOP / ZSOLID and the coarse ice fractions FGICE1, with every plane resident in HBM
(ibh_etopo1_ice_*).  The results feed global_ec.IceScan as they are."""
import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _capi
from ._arrays import dptr, is_cuda, named_planes, stream_arg, to_device
from ._capi import check, lib

MAX_TILE = 8192                 # IBH_ETOPO1_MAX_TILE: fine cells of one coarse cell
PLANES = ("FOCEAN1m", "FGICE1m", "ZICETOP1m", "ZSOLG1m")
PLANES_H = ("FOCEANh", "FGICEh", "ZICETOPh", "ZSOLGh")


class Etopo1Ice(_capi.Handle):
    """What etopo1_ice returns: .FOCEAN1m / .FGICE1m / .ZICETOP1m / .ZSOLG1m, torch.int16 CUDA tensors [jmI, imI], and
    .FOCEANh / .FGICEh / .ZICETOPh / .ZSOLGh, torch.float64 [jmH, imH] (None without hspecH)."""
    _destroy = "ibh_etopo1_ice_destroy"

    def __init__(self, hspecI, hspecC, hspecH, include_greenland):
        self.hspecI, self.hspecC, self.hspecH, self.include_greenland = hspecI, hspecC, hspecH, bool(include_greenland)
        for n in PLANES + PLANES_H:
            setattr(self, n, None)

    def ice_scan(self, hspecO):
        """global_ec.IceScan(hspecO, hspecI, FGICE1m, ZICETOP1m) on the resident planes (global_ec.cpp:762-816)."""
        from .global_ec import IceScan
        return IceScan(hspecO, self.hspecI, self.FGICE1m, self.ZICETOP1m)

    def make_topoO(self, hspecO, hspecS, FLAKES, set_to_land=(), set_to_ocean=(), resets=()):
        """topoo.make_topoO on the resident planes (topo_base.cpp:263-809): no 1' plane leaves the device.  FLAKES: a torch CUDA
        tensor, or a host array (uploaded)."""
        from .topoo import make_topoO
        if not is_cuda(FLAKES):
            FLAKES = to_device(np.ascontiguousarray(FLAKES, np.float64), self.FGICE1m.device)
        return make_topoO(self.hspecI, hspecO, self.FGICE1m, self.ZICETOP1m, self.ZSOLG1m, self.FOCEAN1m, hspecS, FLAKES, set_to_land,
                          set_to_ocean, resets)

    def write(self, ofname_root):
        """<root>1m.nc (:143-157, :229-243) and, with h planes, <root>h.nc (store_h, :27-28) through ncio, CDF-5: `short` /
        `double` variables under the reference's names over (jm1m, im1m) / (jmh, imh), with the units, description and source
        attributes the tool itself puts.  The input file's own attributes are not copied.  Returns the file names."""
        from . import ncio
        g = "" if self.include_greenland else ", Greenland removed"
        ds = ncio.Dataset()
        ds.attrs["source"] = "etopo1_ice.cpp" + g
        dims = (ds.add_dim("jm1m", self.hspecI.jm), ds.add_dim("im1m", self.hspecI.im))
        etopo1 = OrderedDict(units="m", source="ETOPO1" + g)
        attrs = {"ZICETOP1m": etopo1, "ZSOLG1m": etopo1, "FOCEAN1m": OrderedDict(units="1", source="ETOPO1" + g),
                 "FGICE1m": OrderedDict(description="Fractional ice cover (0 or 1)", units="1", source="etopo1_ice.cpp output" + g)}
        for n in ("ZICETOP1m", "ZSOLG1m", "FOCEAN1m", "FGICE1m"):       # the reference's order of writing
            ds.add_var(n, np.int16, dims, getattr(self, n).cpu().numpy(), attrs[n])
        names = [ofname_root + "1m.nc"]
        ds.write(names[0])
        if self.hspecH is not None:
            dh = ncio.Dataset()
            dims = (dh.add_dim("jmh", self.hspecH.jm), dh.add_dim("imh", self.hspecH.im))
            for n in ("ZICETOPh", "ZSOLGh", "FOCEANh", "FGICEh"):
                dh.add_var(n, np.float64, dims, getattr(self, n).cpu().numpy())
            names.append(ofname_root + "h.nc")
            dh.write(names[1])
        return names


def etopo1_ice(hspecI, hspecC, focean, zictop, zsolid, fgiceC, include_greenland=False, hspecH=None):
    """etopo1_ice(files, include_greenland, ofname_root) (etopo1_ice.cpp:45-247) from arrays.  hspecI: the fine grid (the
    reference's g1mx1m), hspecC: the grid of the ice fractions (g1x1), hspecH: the grid of the h planes (ghxh; None: none);
    hspecI must nest in hspecC and a coarse cell hold at most MAX_TILE fine cells.  focean / zictop / zsolid: int16 [jmI, imI]
    (FOCEAN: 0 land, 1 ocean, 2 Greenland), fgiceC: float64 [jmC, imC]; all host numpy arrays (uploaded once in their own
    width) or all torch CUDA tensors (read in place, on torch's current stream).  Inputs are never written.  Returns an
    Etopo1Ice; the semantics, line by line, are in include/icebin_hip.h."""
    planes, on_device = named_planes((("focean", focean, "int16", hspecI.size), ("zictop", zictop, "int16", hspecI.size),
                                      ("zsolid", zsolid, "int16", hspecI.size), ("fgiceC", fgiceC, "float64", hspecC.size)),
                                     "focean / zictop / zsolid / fgiceC: some planes are on the host and some on the device")
    H = hspecH
    h = C.c_void_p()
    check(lib().ibh_etopo1_ice_create(C.byref(h), hspecI.im, hspecI.jm, hspecI.offi, hspecI.dlat, hspecC.im, hspecC.jm,
                                      H.im if H else 0, H.jm if H else 0, H.offi if H else 0., H.dlat if H else 0.))
    res = Etopo1Ice(hspecI, hspecC, hspecH, include_greenland)
    res._h = h
    import torch
    if not on_device:
        planes = [to_device(p) for p in planes]
    dev = planes[0].device
    out = [torch.empty((hspecI.jm, hspecI.im), dtype=torch.int16, device=dev) for _ in PLANES]
    outh = torch.empty((4, H.size), dtype=torch.float64, device=dev) if H else None
    check(lib().ibh_etopo1_ice_device(h, *[dptr(p) for p in planes], int(bool(include_greenland)), *[dptr(o) for o in out], dptr(outh),
                                      H.size if H else 0, stream_arg(planes[0])))
    res._keep = planes          # the inputs are read on the stream: they live as long as the result
    for n, o in zip(PLANES, out):
        setattr(res, n, o)
    if H:
        for k, n in enumerate(PLANES_H):
            setattr(res, n, outh[k].view(H.jm, H.im))
    return res
