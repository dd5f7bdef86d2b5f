"""Times the four coupler matrices (EvI, AvI, IvE, XvE: IceCoupler.cpp:361-468) built through GCMRegridder.to_modele at g5
against the same four built on the ocean grid alone (profiles/modele_times.txt), for every ocean pattern of
tests/test_gpu_modele.py.  Wall time of matrix_d per matrix, best of `reps`, identity ice / exchange sets and a fresh dimE
per round as the coupler has them.  Run it under rocprofv3 --kernel-trace --stats for kernel times."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from icebin_amd import HntrSpec, SparseSet, from_synthetic, synthetic  # noqa: E402

JOBS = (("EvI", 0, "E", "I", True), ("AvI", 0, "A", "I", True), ("IvE", 1, "E", "I", False), ("XvE", 1, "E", "X", False))


def oceans(g, ice):
    O = HntrSpec(g["im"], g["jm"], 0., 120.)
    has = np.zeros(O.size, bool)
    has[ice] = True
    kids = next([(2 * ja + dj) * O.im + 2 * ia + di for dj in (0, 1) for di in (0, 1)]
                for ja in range(O.jm // 2) for ia in range(O.im // 2)
                if all(has[(2 * ja + dj) * O.im + 2 * ia + di] for dj in (0, 1) for di in (0, 1)))
    rng = np.random.default_rng(5)
    out = {}
    for name in ("zero", "om1", "om2", "om4", "frac", "op1"):
        fp, fm = np.zeros(O.size), np.zeros(O.size)
        if name.startswith("om"):
            fm[kids[:int(name[2])]] = fp[kids[:int(name[2])]] = 1.
        elif name == "frac":
            fp[ice] = rng.uniform(0.05, 0.95, len(ice))
        elif name == "op1":
            fp[ice[::3]] = 1.
        out[name] = (fp, fm)
    return O, out


def time_builds(rm, nI, nX, reps, modele):
    dimI, dimX = SparseSet.identity(nI), SparseSet.identity(nX)
    best = {}
    for _ in range(reps + 1):
        dimE = SparseSet()
        for name, kind, _, G, scale in JOBS:
            dG = dimI if G == "I" else dimX
            dims = (dimE if name != "AvI" else None, dG) if kind == 0 else (dG, dimE)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w = rm.matrix_d(name, dims, scale=scale) if modele else rm.matrix_d(name, dims, scale=scale, correctA=True)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            best[name] = (min(ms, best.get(name, (1e30, 0))[0]), w.nnz)
            del w
    return best


def main(reps=5, config="g5"):
    torch.zeros(1, device="cuda:0")
    g = synthetic.make_grids(config)
    em = synthetic.dome_elevmask(g)
    gcmO = from_synthetic(g)
    nI, nX = g["nI"], len(g["ex_area"])
    rmO = gcmO.regrid_matrices("greenland", em)
    ice = np.sort(rmO.matrix_d("AvI").dim(0))
    base = time_builds(rmO, nI, nX, reps, False)
    for name, (ms, nnz) in base.items():
        print(json.dumps(dict(config=config, grid="O", matrix=name, nnz=nnz, ms=round(ms, 3))), flush=True)
    O, pats = oceans(g, ice)
    for pname, (fp, fm) in pats.items():
        rm = gcmO.to_modele((fp, fm), hspecO=O, eq_rad=6371000.).regrid_matrices("greenland", em)
        t = time_builds(rm, nI, nX, reps, True)
        for name, (ms, nnz) in t.items():
            print(json.dumps(dict(config=config, grid="A", ocean=pname, matrix=name, nnz=nnz, ms=round(ms, 3),
                                  times_O=round(ms / base[name][0], 2))), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, sys.argv[2] if len(sys.argv) > 2 else "g5")
