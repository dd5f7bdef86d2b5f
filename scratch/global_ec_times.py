"""Times global_ec's path from a 1-minute ice grid with a SYNTHETIC mask (global_ec; profiles/global_ec_1min_kernels.txt):
the exchange-grid count, ibh_regridder_create_hntr end to end (host and device mask), AvI / EvI / IvE / IvA (scale=false,
correctA) and I2vE onto 1/2 deg, for GCM grids of 1/2 deg and 2 x 2.5 deg.  The exchange grid's floor is the mask read plus
the emitted grid, 8*nI + 16*nX bytes, against 8 TB/s.  Run it under rocprofv3 --kernel-trace --stats for kernel times."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from icebin_amd import HntrSpec, SparseSet, global_ec  # noqa: E402

PEAK = 8e12
R = 6371000.
ICE = HntrSpec(21600, 10800, 0., 1.)
GCMS = [("halfdeg", HntrSpec(720, 360, 0., 30.)), ("2x2.5deg", HntrSpec(144, 90, 0., 120.))]
I2 = HntrSpec(720, 360, 0., 30.)


def synthetic_mask():
    """Ice poleward of 60 degrees, plus a 'Greenland' box (60-84 N, 70-20 W); elevations from a smooth function."""
    lat = -90. + (np.arange(ICE.jm) + 0.5) / 60.
    lon = -180. + (np.arange(ICE.im) + 0.5) / 60.
    LA, LO = np.meshgrid(lat, lon, indexing="ij")
    ice = (np.abs(LA) > 60.) | ((LA > 60.) & (LA < 84.) & (LO > -70.) & (LO < -20.))
    em = np.where(ice, 1500. + 1400. * np.sin(np.radians(LA)) * np.cos(np.radians(LO)), np.nan)
    return em.reshape(-1)


def best_ms(f, reps):
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts)


def main(reps=3):
    em = synthetic_mask()
    dem = torch.from_numpy(em).cuda()
    nice = int(np.count_nonzero(~np.isnan(em)))
    hc = global_ec.hcdefs(0., 3000., 200.)
    print(json.dumps(dict(ice="1min synthetic mask", nI=ICE.size, ice_cells=nice, nhc=len(hc))), flush=True)
    for gname, A in GCMS:
        nX = global_ec.exgrid_count(A, ICE, em, R)
        floor = (8 * ICE.size + 16 * nX) / PEAK * 1e3
        ms = best_ms(lambda: global_ec.exgrid_count(A, ICE, dem, R), reps)
        print(json.dumps(dict(gcm=gname, what="exgrid count (device mask)", nX=nX, ms=round(ms, 3))), flush=True)
        for mname, m in (("host", em), ("device", dem)):
            ms = best_ms(lambda: global_ec.gcm_from_hntr(A, ICE, m, hc, True, R), reps)
            print(json.dumps(dict(gcm=gname, what="create_hntr end to end (%s mask)" % mname, nX=nX, ms=round(ms, 3),
                                  floor_ms=round(floor, 3), share_of_8TBps=round(floor / ms, 3))), flush=True)
        gcm = global_ec.gcm_from_hntr(A, ICE, dem, hc, True, R)
        rm = gcm.regrid_matrices("globalI", dem, scale=False, correctA=True)
        for name in ("AvI", "EvI", "IvE", "IvA"):
            ms = best_ms(lambda: rm.matrix_d(name, scale=False, correctA=True), reps)
            w = rm.matrix_d(name, scale=False, correctA=True)
            print(json.dumps(dict(gcm=gname, what=name, nnz=w.nnz, built_fast=w.built_fast(), ms=round(ms, 3))), flush=True)
        IvE = rm.matrix_d("IvE", (SparseSet(), SparseSet()), scale=False, correctA=True)
        ms = best_ms(lambda: global_ec.make_I2vX(IvE, ICE, I2, em, SparseSet(I2.size), R), reps)
        w = global_ec.make_I2vX(IvE, ICE, I2, em, SparseSet(I2.size), R)
        print(json.dumps(dict(gcm=gname, what="I2vE onto 1/2 deg (host mask -> includeI)", nnz=w.nnz, ms=round(ms, 3))), flush=True)
        del gcm, rm, IvE, w


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3)
