"""Times make_topoO at the production size (profiles/make_topoo_kernels.txt): the 1' planes (21600 x 10800, 233 M cells)
onto the 1/4 x 1 degree ocean grid (288 x 180, tiles of 75 x 60), FLAKES on 10' (2160 x 1080), synthetic planes resident in HBM.

  make_topoo_times.py [reps] [--no-check]   the whole call (host clock around make_topoO, which creates the handle and reads the
                                            status back, and device events around ibh_make_topoo_device alone; best of reps), then --
                                            unless --no-check -- the plain-loop restatement of the same planes on one core, and
                                            "equal" or the first differing cell

Run it under rocprofv3 --kernel-trace --stats with --no-check for the kernels on their own (k_to_cells, k_to_gice, k_to_tiles<false>:
the interior tiles, k_to_tiles<true>: the two pole tiles of 1 296 000 cells, k_to_resets, k_to_blocks, hntr_regrid_kernel).  Bytes:
k_to_tiles reads 6 per fine cell (three int16 planes), the six regrids 2 or 4 per fine cell each, the ocean-grid passes 8 per plane
and cell of 51840.  The yardstick is what this box gives a plain read stream, 5.96 TB/s."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from icebin_amd import Hntr, HntrSpec, _capi, topoo  # noqa: E402

READ_STREAM = 5.96e12
I, O, S = HntrSpec(21600, 10800, 0., 1.), HntrSpec(288, 180, 0., 60.), HntrSpec(2160, 1080, 0., 10.)


def planes(dev):
    """Land by ocean cell: 40 % of the ocean cells are 90 % land, the others 10 %, so that both branches of callZ and every sort size
    occur; ice on a tenth of the cells; elevations in steps of 1 m over [-400, 4000); ZSOLG1m below ZICETOP1m on the western half."""
    g = torch.Generator(device=dev).manual_seed(5)
    mi, mj = I.im // O.im, I.jm // O.jm
    p = torch.where(torch.rand((O.jm, O.im), device=dev, generator=g) < .4, .9, .1).to(torch.float32)
    p = p.repeat_interleave(mj, 0).repeat_interleave(mi, 1)
    fo = (torch.rand((I.jm, I.im), device=dev, generator=g) >= p).to(torch.int16)
    del p
    fg = (torch.rand((I.jm, I.im), device=dev, generator=g) < .1).to(torch.int16)
    zt = torch.randint(-400, 4000, (I.jm, I.im), dtype=torch.int16, device=dev, generator=g)
    zs = zt.clone()
    zs[:, :I.im // 2] -= torch.randint(0, 100, (I.jm, I.im // 2), dtype=torch.int16, device=dev, generator=g)
    fl = torch.rand((S.jm, S.im), device=dev, generator=g, dtype=torch.float64) * .3
    return fg, zt, zs, fo, fl


def cells():
    d = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "make_topoo_g1qx1_cells.json")))
    return ([tuple(c) for c in d["set_to_land"]], [tuple(c) for c in d["set_to_ocean"]],
            [(r["elev"], [tuple(c) for c in r["cells"]]) for r in d["resets"]])


def main(reps=3, check=True):
    dev = torch.device("cuda:0")
    fg, zt, zs, fo, fl = planes(dev)
    land, ocean, resets = cells()
    # the hand-set cells are for the real Earth: on these planes a SET_TO cell may have no cell of its kind, which is fatal; keep the
    # ones that do
    mi, mj = I.im // O.im, I.jm // O.jm
    frac = fo.view(O.jm, mj, O.im, mi).to(torch.float32).mean((1, 3)).cpu().numpy()
    land = [c for c in land if frac[c[1] - 1, c[0] - 1] < 1]
    ocean = [c for c in ocean if frac[c[1] - 1, c[0] - 1] > 0]
    kw = dict(set_to_land=land, set_to_ocean=ocean, resets=resets)
    res = topoo.make_topoO(I, O, fg, zt, zs, fo, S, fl, **kw)       # warm-up: the allocations, the regridders' tables
    torch.cuda.synchronize()
    wall, evs = [], []
    out = torch.empty((len(topoo.PLANES), O.size), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = topoo.make_topoO(I, O, fg, zt, zs, fo, S, fl, **kw)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        del r
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _capi.check(_capi.lib().ibh_make_topoo_device(res._h, *[C.c_void_p(p.data_ptr()) for p in (fg, zt, zs, fo, fl)], C.c_void_p(out.data_ptr()),
                                                      O.size, C.c_void_p(st)))
        e1.record()
        torch.cuda.synchronize()
        evs.append(e0.elapsed_time(e1))
    nI = I.size
    print(json.dumps(dict(case="21600x10800 onto 288x180, FLAKES 2160x1080", ocean_cells=int(res.FOCEAN.sum()), of=O.size,
                          call_wall_ms=round(min(wall), 3), enqueue_event_ms=round(min(evs), 3), counts=dict(res.counts),
                          tiles_bytes=6 * nI, tiles_floor_ms=round(6 * nI / READ_STREAM * 1e3, 4))), flush=True)
    if not check:
        return
    import make_topoo_restatement as mr
    hI, hS = Hntr(17.17, O, I), Hntr(17.17, O, S)
    v = lambda t: t.reshape(1, -1)  # noqa: E731
    six = [hI.regrid_device(1., v(fo), mean_polar=True), hI.regrid_device(1., v(fg), mean_polar=True), hS.regrid_device(1., v(fl), mean_polar=True),
           hI.regrid_device(v(fo), v(zs), mean_polar=True), hI.regrid_device(v(fg), v(zt), mean_polar=True),
           hI.regrid_device(v(fg), v(zs), mean_polar=True)]
    six = [x.cpu().numpy().reshape(O.jm, O.im) for x in six]
    host = [t.cpu().numpy() for t in (fg, zt, zs, fo)]
    t0 = time.perf_counter()
    ref, counts, pow_cells = mr.make_topoO(I.im, I.jm, O.im, O.jm, *host, *six, **kw)
    t1 = time.perf_counter() - t0
    ld = mr.make_topoO(I.im, I.jm, O.im, O.jm, *host, *six, real=np.longdouble, only_dzgice=True, **kw)[0]["dZGICE"]
    verdict = "equal"
    for n in topoo.PLANES:
        got = getattr(res, n).cpu().numpy()
        differ = got.view(np.int64) != ref[n].view(np.int64)
        if n == "dZGICE":
            differ &= ~pow_cells
            rel = np.abs(got[pow_cells].astype(np.longdouble) - ld[pow_cells]) / np.abs(ld[pow_cells]) if pow_cells.any() else np.zeros(1)
            bound = (2 * 2.5752 + O.im + O.jm + 8) * 2. ** -53
            if float(rel.max()) > bound:
                verdict = "dZGICE through pow: relative error %.3g above the bound %.3g" % (float(rel.max()), bound)
                break
        if differ.any():
            j, i = np.argwhere(differ)[0]
            verdict = "%s differs first at (I, J) = (%d, %d): %r, the restatement has %r" % (n, i + 1, j + 1, got[j, i], ref[n][j, i])
            break
    if verdict == "equal" and counts != dict(res.counts):
        verdict = "the counts differ: %r, the restatement has %r" % (dict(res.counts), counts)
    print(json.dumps(dict(case="restatement of the same planes on one core", cells=nI, restatement_s=round(t1, 1), pow_cells=int(pow_cells.sum()),
                          against_the_library=verdict)), flush=True)


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if x != "--no-check"]
    main(int(a[0]) if a else 3, "--no-check" not in sys.argv)
