"""Times etopo1_ice at the production size (profiles/etopo1_ice_kernels.txt): the 1' planes (21600 x 10800, 233 M cells)
onto the 1 deg ice fractions (360 x 180), the h planes onto 1/2 deg (720 x 360), synthetic planes resident in HBM.

  etopo1_ice_times.py [reps]    per fraction field: the whole call (host clock around etopo1_ice plus a synchronize, and device
                                events, best of reps) with and without the h planes; the four typed regrids on their own; and the
                                plain-loop restatement on one core at a size it can finish (4320 x 2160 onto 72 x 36, mult 60)

Run it under rocprofv3 --kernel-trace --stats for the kernels on their own (k_et_planes, k_et_tiles, k_et_unice, hntr_regrid_kernel);
the launches come in the order of the cases below.  Bytes: k_et_planes reads 6 and writes 8 per fine cell, k_et_unice reads 2 per cell
of the north half, k_et_tiles reads 4 per cell of a tile whose fraction is not 0.  The yardstick is what this box gives a plain read
stream, 5.96 TB/s."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from icebin_amd import Hntr, HntrSpec, etopo1  # noqa: E402

READ_STREAM = 5.96e12
I, Cg, H = HntrSpec(21600, 10800, 0., 1.), HntrSpec(360, 180, 0., 60.), HntrSpec(720, 360, 0., 30.)


def planes(dev, all_land):
    """30 % land, 68 % ocean, a block of Greenland in the north; elevations in steps of 1 m (few ties) over [-400, 4000)"""
    g = torch.Generator(device=dev).manual_seed(5)
    u = torch.rand((I.jm, I.im), device=dev, generator=g)
    fo = (u >= 0.3).to(torch.int16)
    if all_land:
        fo.zero_()
    fo[I.jm * 5 // 6:I.jm * 47 // 48, I.im // 3:I.im * 4 // 9] = 2
    del u
    zt = torch.randint(-400, 4000, (I.jm, I.im), dtype=torch.int16, device=dev, generator=g)
    zs = zt - torch.randint(0, 100, (I.jm, I.im), dtype=torch.int16, device=dev, generator=g)
    return fo, zt, zs


def fractions(case, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    if case == "sparse":        # 3 % of the cells, fractions 0.1 - 0.5
        on = torch.rand((Cg.jm, Cg.im), device=dev, generator=g) < 0.03
        return torch.where(on, 0.1 + 0.4 * torch.rand((Cg.jm, Cg.im), device=dev, generator=g, dtype=torch.float64), 0.).to(torch.float64)
    return torch.ones((Cg.jm, Cg.im), dtype=torch.float64, device=dev)


def best(fn, reps):
    wall, evs = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        keep = fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        evs.append(e0.elapsed_time(e1))
        del keep
    return round(min(wall), 3), round(min(evs), 3)


def main(reps=3):
    dev = torch.device("cuda:0")
    for case, all_land in (("sparse", False), ("full", False), ("full_all_land", True)):
        fo, zt, zs = planes(dev, all_land)
        fC = fractions("sparse" if case == "sparse" else "full", dev)
        res = etopo1.etopo1_ice(I, Cg, fo, zt, zs, fC, False, H)        # warm-up: the allocations, the regridder's tables
        torch.cuda.synchronize()
        ice = int(res.FGICE1m.sum(dtype=torch.int64))
        hntr = Hntr(17.17, H, I)
        outs = [getattr(res, n).reshape(1, -1) for n in etopo1.PLANES]
        regrid = best(lambda: [hntr.regrid_device(1.0, o, mean_polar=True) for o in outs], reps)
        del res
        with_h = best(lambda: etopo1.etopo1_ice(I, Cg, fo, zt, zs, fC, False, H), reps)
        no_h = best(lambda: etopo1.etopo1_ice(I, Cg, fo, zt, zs, fC, False), reps)
        nI = I.size
        print(json.dumps(dict(case=case, north_cells_nonzero=int((fC[Cg.jm // 2:] != 0).sum()), ice_cells=ice, call_with_h_wall_ms=with_h[0],
                              call_with_h_event_ms=with_h[1], call_no_h_wall_ms=no_h[0], call_no_h_event_ms=no_h[1],
                              four_regrids_wall_ms=regrid[0], four_regrids_event_ms=regrid[1], planes_bytes=14 * nI,
                              planes_floor_ms=round(14 * nI / READ_STREAM * 1e3, 4))), flush=True)
        del fo, zt, zs, fC, outs
    # the restatement on one core
    import etopo1_ice_restatement as er
    I2, C2 = HntrSpec(4320, 2160, 0., 5.), HntrSpec(72, 36, 0., 300.)
    rng = np.random.default_rng(5)
    fo = (rng.random((I2.jm, I2.im)) >= 0.3).astype(np.int16)
    zt = rng.integers(-400, 4000, fo.shape).astype(np.int16)
    zs = (zt - rng.integers(0, 100, fo.shape)).astype(np.int16)
    fC = np.ones((C2.jm, C2.im))
    t0 = time.perf_counter()
    ref = er.etopo1_ice(I2, C2, fo, zt, zs, fC, False)
    t1 = time.perf_counter() - t0
    res = etopo1.etopo1_ice(I2, C2, fo, zt, zs, fC, False)
    same = all(np.array_equal(ref[n], getattr(res, n).cpu().numpy()) for n in etopo1.PLANES)
    print(json.dumps(dict(case="restatement 4320x2160 onto 72x36, every fraction 1.0", cells=I2.size, restatement_s=round(t1, 2),
                          us_per_cell=round(t1 / I2.size * 1e6, 2), equal_to_the_library=same)), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3)
