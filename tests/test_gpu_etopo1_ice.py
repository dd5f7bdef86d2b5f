"""etopo1_ice on the GPU (icebin_amd.etopo1) against the plain-loop restatement of modele/etopo1_ice.cpp:45-247
(tests/etopo1_ice_restatement.py): every int16 plane equal cell for cell, the h planes bitwise Hntr.regrid_device of the output
planes.  Nothing here takes a tolerance."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import etopo1_ice_restatement as er  # noqa: E402

PLANES = ("FOCEAN1m", "FGICE1m", "ZICETOP1m", "ZSOLG1m")


def spec(im, jm, offi=0.):
    from icebin_amd import HntrSpec
    return HntrSpec(im, jm, offi, 180. * 60. / jm)


# name -> (coarse, fine): mult 3, 4, 5; the real tile (60 x 60, the 3600-key sort); a band start (30 * 14 // 15 = 28) inside the north
# half with one-row tiles; mult_i != mult_j; jmI > imI (the column bound of the transposed check); a tile of exactly the limit
GRIDS = {"m3": ((8, 4), (24, 12)), "m4": ((8, 4), (32, 16)), "m5": ((8, 4), (40, 20)), "m60": ((4, 2), (240, 120)),
         "band": ((6, 30), (24, 30)), "m7x2": ((8, 4), (56, 8)), "tall": ((2, 8), (6, 24)), "limit": ((4, 2), (512, 128))}


def grids(name):
    c, f = GRIDS[name]
    return spec(*f), spec(*c)


def tile(a, I, Cg, j1, i1):
    mi, mj = I.im // Cg.im, I.jm // Cg.jm
    return a[j1 * mj:(j1 + 1) * mj, i1 * mi:(i1 + 1) * mi]


@functools.lru_cache(maxsize=None)
def make_planes(name):
    """focean in {0, 1, 2, 3} at random (a quarter each, so Greenland cells lie on both sides of i = jmI, on the diagonal, in
    transposed pairs in both orders, and with transposed targets in the south half), elevations with many ties and both int16
    extremes, thicknesses around the 50 m threshold and one that overflows int16, fractions in [0, 1.2) with a third of them 0.
    Then, over the north coarse cells in turn, as many of the special tiles as the grid has room for."""
    I, Cg = grids(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    fo = rng.integers(0, 4, (I.jm, I.im)).astype(np.int16)
    zt = (rng.integers(-3, 4, fo.shape) * 100).astype(np.int16)
    zt[rng.random(fo.shape) < 0.03] = -32768
    zt[rng.random(fo.shape) < 0.03] = 32767
    zs = np.clip(zt.astype(np.int64) - rng.integers(0, 100, fo.shape), -32768, 32767).astype(np.int16)
    over = rng.random(fo.shape) < 0.02              # 32767 - (-32768) = 65535 in int; an int16 difference would be -1
    zt[over], zs[over] = 32767, -32768
    jh = I.jm // 2                                  # Greenland on the diagonal and as a transposed pair, where the plane has room
    for j, i in ((jh, jh), (jh, jh + 1), (jh + 1, jh)):
        if j < I.jm and i < I.im:
            fo[j, i] = 2
    fC = np.where(rng.random((Cg.jm, Cg.im)) < 1 / 3, 0., rng.random((Cg.jm, Cg.im)) * 1.2)
    dI, dC = er.make_dxyp(I), er.make_dxyp(Cg)
    north = [(j1, i1) for j1 in range(Cg.jm // 2, Cg.jm) for i1 in range(Cg.im)]
    mj = I.jm // Cg.jm

    def first_cell_fraction(j1, i1, share):
        """all land, one highest cell in the tile's last row: the fraction that leaves `share` of that cell's area"""
        tile(fo, I, Cg, j1, i1)[:] = 0
        t = tile(zt, I, Cg, j1, i1)
        t[t == 32767] = 300
        t[-1, -1] = 32767
        return share * dI[(j1 + 1) * mj - 1] / dC[j1]

    specials = [("no land", lambda j1, i1: 0.5), ("one land cell", lambda j1, i1: 0.7), ("snow >= 1", lambda j1, i1: 1.5),
                ("snow 0", lambda j1, i1: 0.), ("snow -0.0", lambda j1, i1: -0.), ("snow NaN", lambda j1, i1: float("nan")),
                ("snow < 0", lambda j1, i1: -0.3), ("first cell by rounding", lambda j1, i1: first_cell_fraction(j1, i1, .75)),
                ("not even the first", lambda j1, i1: first_cell_fraction(j1, i1, .25)), ("exactly one cell", lambda j1, i1: first_cell_fraction(j1, i1, 1.))]
    # spread over the north cells so that some land in the polar-most row (the 78N band) where the grid has several rows
    order = north[::-1][::2] + north[::-1][1::2]
    for (what, frac), (j1, i1) in zip(specials, order):
        t = tile(fo, I, Cg, j1, i1)
        if what == "no land":
            t[t == 0] = 1
        elif what == "one land cell":
            t[t == 0] = 3
            t[t.shape[0] // 2, -1] = 0
        elif what.startswith("snow"):
            t[:] = 0
        fC[j1, i1] = frac(j1, i1)
    for a in (fo, zt, zs, fC):
        a.setflags(write=False)
    return fo, zt, zs, fC


@functools.lru_cache(maxsize=None)
def reference(name, incl):
    I, Cg = grids(name)
    out = er.etopo1_ice(I, Cg, *make_planes(name), incl)
    for a in out.values():
        a.setflags(write=False)
    return out


def assert_planes(res, ref, what):
    for n in PLANES:
        got = getattr(res, n)
        assert str(got.dtype) == "torch.int16" and got.is_cuda and tuple(got.shape) == ref[n].shape, (what, n)
        got = got.cpu().numpy()
        bad = np.argwhere(got != ref[n])
        assert len(bad) == 0, (what, n, len(bad), bad[:5].tolist(), got[tuple(bad[0])], ref[n][tuple(bad[0])])


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_bytes(a, b):
    """two torch tensors hold the same bytes (a NaN fraction equals itself)"""
    return np.array_equal(a.cpu().numpy().reshape(-1).view(np.uint8), b.cpu().numpy().reshape(-1).view(np.uint8))


@pytest.mark.parametrize("incl", [False, True], ids=["no_greenland", "greenland"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_host_planes_match_the_restatement(name, incl):
    from icebin_amd import etopo1
    I, Cg = grids(name)
    planes = make_planes(name)
    before = [p.copy() for p in planes]
    res = etopo1.etopo1_ice(I, Cg, *planes, include_greenland=incl)
    assert_planes(res, reference(name, incl), (name, incl))
    assert all(getattr(res, n) is None for n in etopo1.PLANES_H)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(planes, before))
    ref = reference(name, incl)
    assert ref["FGICE1m"].any() and (ref["FGICE1m"] == 0).any()


def test_the_planes_exercise_what_they_claim():
    # the special tiles did what their names say, in the restatement: so the comparison above covers those paths
    I, Cg = grids("m4")
    fo, zt, zs, fC = make_planes("m4")
    dI, dC = er.make_dxyp(I), er.make_dxyp(Cg)
    taken = {}
    for j1 in range(Cg.jm // 2, Cg.jm):
        for i1 in range(Cg.im):
            cells = er.tile_cells(fo, zt, j1, i1, 4, 4, False)
            taken[(j1, i1)] = (len(cells), len(er.fill(cells, [dI[c[1]] for c in cells], fC[j1, i1] * dC[j1])) if fC[j1, i1] != 0 else None)
    counts = list(taken.values())
    assert (0, 0) in counts and any(n == 1 for n, _ in counts)                      # no land; one land cell
    assert (16, 16) in counts and (16, None) in counts                              # snow >= 1: all, no break; snow == 0: skipped
    assert sum(1 for n, t in counts if n == 16 and t == 0) >= 3                     # NaN, negative, a quarter of the first cell
    assert sum(1 for n, t in counts if n == 16 and t == 1) >= 2                     # the first cell by rounding; exactly one cell
    assert len({dI[j] for j in range(12, 16)}) == 4                                 # a tile's rows differ in area
    assert I.jm * 14 // 15 > I.jm // 2 and I.jm * 14 // 15 < I.jm                   # the band starts inside the north half
    g = np.argwhere((fo == 2) & (np.arange(I.jm)[:, None] >= I.jm // 2))
    G = {tuple(x) for x in g.tolist()}
    assert any(i >= I.jm for _, i in G) and any(i < I.jm for _, i in G) and any(i == j for j, i in G)
    assert any((i, j) in G and i < j for j, i in G) and any((i, j) in G and i > j for j, i in G)
    assert any(i < I.jm // 2 for _, i in G)                                         # transposed targets in the south half
    tall = make_planes("tall")[0]
    assert any(j >= 6 for j, i in np.argwhere(tall == 2).tolist())                  # j >= imI: the reference would leave its array


@pytest.mark.parametrize("incl", [False, True], ids=["no_greenland", "greenland"])
@pytest.mark.parametrize("name", ["m3", "m60", "band", "tall"])
def test_device_planes_in_place_and_misaligned(name, incl):
    import torch
    from icebin_amd import etopo1
    I, Cg = grids(name)
    planes = make_planes(name)
    ref = reference(name, incl)
    dev = [torch.from_numpy(p.copy()).cuda() for p in planes]
    keep = [d.clone() for d in dev]
    res = etopo1.etopo1_ice(I, Cg, *dev, include_greenland=incl)
    assert_planes(res, ref, (name, incl, "device"))
    assert all(same_bytes(a, b) for a, b in zip(dev, keep))
    # odd element offsets: FOCEAN and ZICTOP 2 bytes past a 16-byte boundary (a head of 7 cells, ZICTOP aligned with it), ZSOLID 6
    # bytes past one (read cell by cell); the fresh outputs are then not aligned with the pieces either
    mis = []
    for p, off in zip(planes[:3], (1, 1, 3)):
        buf = torch.full((p.size + 8,), -7, dtype=torch.int16, device="cuda")
        buf[off:off + p.size] = torch.from_numpy(p.reshape(-1).copy())
        assert buf.data_ptr() % 16 == 0
        mis.append((buf, buf[off:off + p.size]))
    snap = [b.clone() for b, _ in mis]
    res2 = etopo1.etopo1_ice(I, Cg, *[v for _, v in mis], dev[3], include_greenland=incl)
    assert_planes(res2, ref, (name, incl, "misaligned"))
    assert all(same_bytes(b, s) for (b, _), s in zip(mis, snap)) and same_bytes(dev[3], keep[3])


@pytest.mark.parametrize("name,H,offi", [("m3", (12, 6), 0.), ("m4", (8, 4), 0.), ("m3", (12, 6), 1.5), ("m60", (24, 12), 0.)])
def test_h_planes_are_the_typed_regrid_bitwise(name, H, offi):
    import torch
    from icebin_amd import Hntr, etopo1
    (imI, jmI), Cg = GRIDS[name][1], grids(name)[1]
    I, Hs = spec(imI, jmI, offi), spec(*H)
    res = etopo1.etopo1_ice(I, Cg, *make_planes(name), include_greenland=True, hspecH=Hs)
    assert_planes(res, reference(name, True), (name, "with h planes"))
    hntr = Hntr(17.17, Hs, I)
    for n1m, nh in zip(etopo1.PLANES, etopo1.PLANES_H):
        got = getattr(res, nh)
        assert got.dtype == torch.float64 and tuple(got.shape) == (Hs.jm, Hs.im)
        want = hntr.regrid_device(1.0, getattr(res, n1m).reshape(1, -1), mean_polar=True)
        assert np.array_equal(bits(got.cpu().numpy().reshape(-1)), bits(want.cpu().numpy().reshape(-1))), nh
    assert float(res.FGICEh.max()) > 0


def test_ice_scan_on_the_resident_planes():
    from icebin_amd import etopo1, global_ec
    I, Cg = grids("m4")
    res = etopo1.etopo1_ice(I, Cg, *make_planes("m4"), include_greenland=False)
    scan = res.ice_scan(Cg)
    other = global_ec.IceScan(Cg, I, res.FGICE1m.cpu().numpy(), res.ZICETOP1m.cpu().numpy())
    assert scan.elevI_range == other.elevI_range
    assert np.array_equal(scan.nice.cpu().numpy(), other.nice.cpu().numpy()) and int(scan.nice.sum()) == int(res.FGICE1m.sum())
    assert np.array_equal(bits(scan.fgiceO.cpu().numpy()), bits(other.fgiceO.cpu().numpy()))


@pytest.mark.parametrize("incl", [False, True], ids=["no_greenland", "greenland"])
def test_write_reads_back_through_ncio(tmp_path, incl):
    from icebin_amd import etopo1, ncio
    I, Cg, Hs = *grids("m3"), spec(12, 6)
    res = etopo1.etopo1_ice(I, Cg, *make_planes("m3"), include_greenland=incl, hspecH=Hs)
    root = str(tmp_path / "etopo1_ice")
    assert res.write(root) == [root + "1m.nc", root + "h.nc"]
    assert open(root + "1m.nc", "rb").read(4) == b"CDF\x05" and open(root + "h.nc", "rb").read(4) == b"CDF\x05"
    g = "" if incl else ", Greenland removed"
    ds = ncio.Dataset.read(root + "1m.nc")
    assert dict(ds.dims) == {"jm1m": I.jm, "im1m": I.im} and ds.attrs["source"] == "etopo1_ice.cpp" + g
    assert list(ds.variables) == ["ZICETOP1m", "ZSOLG1m", "FOCEAN1m", "FGICE1m"]
    for n in PLANES:
        v = ds.variables[n]
        assert v.dims == ("jm1m", "im1m") and v.data.dtype == np.int16 and np.array_equal(v.data, getattr(res, n).cpu().numpy()), n
    assert dict(ds.variables["ZICETOP1m"].attrs) == {"units": "m", "source": "ETOPO1" + g} == dict(ds.variables["ZSOLG1m"].attrs)
    assert dict(ds.variables["FOCEAN1m"].attrs) == {"units": "1", "source": "ETOPO1" + g}
    assert dict(ds.variables["FGICE1m"].attrs) == {"description": "Fractional ice cover (0 or 1)", "units": "1",
                                                   "source": "etopo1_ice.cpp output" + g}
    dh = ncio.Dataset.read(root + "h.nc")
    assert dict(dh.dims) == {"jmh": Hs.jm, "imh": Hs.im} and list(dh.variables) == ["ZICETOPh", "ZSOLGh", "FOCEANh", "FGICEh"]
    for n in etopo1.PLANES_H:
        v = dh.variables[n]
        assert v.dims == ("jmh", "imh") and v.data.dtype == np.float64 and np.array_equal(bits(v.data), bits(getattr(res, n).cpu().numpy())), n


def test_the_host_entry_and_the_refusals_of_the_device_entry():
    import torch
    from icebin_amd import _capi, etopo1
    L = _capi.lib()
    I, Cg, Hs = *grids("m5"), spec(10, 4)
    fo, zt, zs, fC = [np.array(p) for p in make_planes("m5")]
    res = etopo1.etopo1_ice(I, Cg, fo, zt, zs, fC, include_greenland=False, hspecH=Hs)
    out = [np.full((I.jm, I.im), -9, np.int16) for _ in PLANES]
    outh = np.full((4, Hs.size + 3), -9.)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    _capi.check(L.ibh_etopo1_ice_host(res._h, p(fo), p(zt), p(zs), p(fC), 0, *[p(o) for o in out], p(outh), Hs.size + 3))
    for n, o in zip(PLANES, out):
        assert np.array_equal(o, reference("m5", False)[n]), n
    for k, n in enumerate(etopo1.PLANES_H):
        assert np.array_equal(bits(outh[k, :Hs.size]), bits(getattr(res, n).cpu().numpy().reshape(-1))), n
    assert (outh[:, Hs.size:] == -9.).all()         # the gaps between the h planes are left alone
    # the device entry: NULL planes, misalignment, outputs over inputs or over each other, h planes without room
    d = [torch.from_numpy(a).cuda() for a in (fo, zt, zs)] + [torch.from_numpy(fC).cuda()]
    o = [torch.empty((I.jm, I.im), dtype=torch.int16, device="cuda") for _ in PLANES]
    oh = torch.empty((4, Hs.size), dtype=torch.float64, device="cuda")
    good = [t.data_ptr() for t in d] + [t.data_ptr() for t in o] + [oh.data_ptr()]

    def call(ptrs, ldh=Hs.size, h=res._h):
        return L.ibh_etopo1_ice_device(h, *[C.c_void_p(x) for x in ptrs[:4]], 0, *[C.c_void_p(x) for x in ptrs[4:8]], C.c_void_p(ptrs[8]), ldh, None)

    def swap(k, v):
        return good[:k] + [v] + good[k + 1:]

    bad = [swap(k, None) for k in range(8)] + [swap(0, good[0] + 1), swap(3, good[3] + 4), swap(5, good[5] + 1), swap(8, good[8] + 4)]
    bad += [swap(4, good[0]), swap(5, good[1] + 2 * (I.size - 1)), swap(6, good[2]), swap(7, good[6]), swap(7, good[6] + 2), swap(5, good[4])]
    for ptrs in bad:
        assert call(ptrs) == _capi.IBH_EINVAL, ptrs
    assert call(good, ldh=Hs.size - 1) == _capi.IBH_EINVAL
    plain = etopo1.etopo1_ice(I, Cg, fo, zt, zs, fC)                # a handle made without hspecH has no h planes to give
    assert call(good, h=plain._h) == _capi.IBH_EINVAL
    torch.cuda.synchronize()
    assert call(good) == _capi.IBH_OK                               # and the same arguments, unbroken, are accepted
    torch.cuda.synchronize()
    for n, t in zip(PLANES, o):
        assert np.array_equal(t.cpu().numpy(), reference("m5", False)[n]), n


def test_a_tile_one_above_the_limit_is_refused():
    from icebin_amd import _capi, etopo1
    I, Cg = grids("limit")
    assert (I.im // Cg.im) * (I.jm // Cg.jm) == etopo1.MAX_TILE
    I2, C2 = spec(2731, 6), spec(1, 2)
    with pytest.raises(_capi.IcebinHipError, match=str(etopo1.MAX_TILE)):
        etopo1.etopo1_ice(I2, C2, np.zeros((6, 2731), np.int16), np.zeros((6, 2731), np.int16), np.zeros((6, 2731), np.int16), np.zeros((2, 1)))
