"""Times GCMRegridder_ModelE.global_AvE (profiles/global_ave_times.txt): the g5 Greenland sheet merged with a
base (global) ice matrix that covers every cell of the 144 x 90 ocean grid with 3 elevation classes, no ocean.  Wall time per
call, best of `reps`, with its two halves (compute_EOpvAOp_merged, compute_AAmvEAm) and, as the yardstick from the same run,
EvI through to_modele (profiles/modele_times.txt).  Run it under rocprofv3 --kernel-trace --stats for the dispatch count."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from icebin_amd import HntrSpec, SparseSet, compute_AAmvEAm, compute_EOpvAOp_merged, from_synthetic, synthetic  # noqa: E402


def best_of(reps, f):
    best, out = 1e30, None
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, out


def main(reps=5, config="g5", only=None):
    torch.zeros(1, device="cuda:0")
    g = synthetic.make_grids(config)
    em = synthetic.dome_elevmask(g)
    gcmO = from_synthetic(g)
    O = HntrSpec(g["im"], g["jm"], 0., 120.)
    nO = O.size
    rng = np.random.default_rng(7)
    iO = np.tile(np.arange(nO, dtype=np.int64), 3)
    ihc = np.repeat(np.arange(3, dtype=np.int64), nO)
    base = (np.asarray([500., 1500., 2500.]), (iO + nO * ihc, iO, rng.uniform(1e9, 5e10, 3 * nO)), (3 * nO, nO))
    fp, fm = np.zeros(nO), np.zeros(nO)
    gcmA = gcmO.to_modele((fp, fm), hspecO=O, eq_rad=6371000., global_ec=base)
    rmO = gcmO.regrid_matrices("greenland", em, scale=False, correctA=False)
    ms, (w, offsetE) = best_of(reps, lambda: gcmA.global_AvE(None, [em], fp, fm, scale=True))
    print(json.dumps(dict(config=config, call="global_AvE", nnz=w.nnz, shape_d=[w.nrow_d, w.ncol_d], offsetE=offsetE, ms=round(ms, 3))), flush=True)
    if only == "global_AvE":        # (for a dispatch count: the difference of two profiled runs with different reps)
        return
    ms1, eo = best_of(reps, lambda: compute_EOpvAOp_merged([rmO], base))
    print(json.dumps(dict(config=config, call="compute_EOpvAOp_merged", nnz=eo.EOpvAOp.nnz, nhc=eo.nhc, ms=round(ms1, 3))), flush=True)
    ms2, _ = best_of(reps, lambda: compute_AAmvEAm(eo, O, 6371000., fp, fm, scale=True))
    print(json.dumps(dict(config=config, call="compute_AAmvEAm", ms=round(ms2, 3))), flush=True)
    rm = gcmA.regrid_matrices("greenland", em)
    dimI = SparseSet.identity(g["nI"])
    ms3, EvI = best_of(reps, lambda: rm.matrix_d("EvI", (SparseSet(), dimI), scale=True))
    print(json.dumps(dict(config=config, call="to_modele EvI", nnz=EvI.nnz, ms=round(ms3, 3), global_AvE_over_EvI=round(ms / ms3, 2))), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, sys.argv[2] if len(sys.argv) > 2 else "g5", sys.argv[3] if len(sys.argv) > 3 else None)
