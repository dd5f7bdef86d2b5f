"""Times GCMRegridder_ModelE.update_topo and writes profiles/topo_times.txt: the g5 Greenland sheet under the
144 x 90 ocean, every ocean cell ModelE ocean before the merge, a base (global) ice matrix with 3 elevation classes on every
cell.  Wall time per call, best of `reps`, planes and masks resident in HBM, split into merge_topoO, global_AvE and make_topoA;
and the kernel time (HIP events around the launches, best of `reps`) of the row-statistics pass over the sheet's OvI beside an
apply of the same matrix followed by a separate min / max pass."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from icebin_amd import HntrSpec, SparseSet, from_synthetic, make_topoA, merge_topoO, synthetic  # noqa: E402


def best_of(reps, f):
    best, out = 1e30, None
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, out


def kernel_ms(reps, f):
    best = 1e30
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def main(reps=5, config="g5", outdir=os.path.join(ROOT, "profiles")):
    torch.zeros(1, device="cuda:0")
    g = synthetic.make_grids(config)
    land = synthetic.dome_elevmask(g)
    ice = np.where(np.random.default_rng(4).random(len(land)) < 0.3, np.nan, land)
    gcmO = from_synthetic(g)
    O = HntrSpec(g["im"], g["jm"], 0., 120.)
    nO = O.size
    rng = np.random.default_rng(7)
    iO = np.tile(np.arange(nO, dtype=np.int64), 3)
    ihc = np.repeat(np.arange(3, dtype=np.int64), nO)
    base = (np.asarray([500., 1500., 2500.]), (iO + nO * ihc, iO, rng.uniform(1e9, 5e10, 3 * nO)), (3 * nO, nO))
    gcmA = gcmO.to_modele((np.ones(nO), np.ones(nO)), hspecO=O, eq_rad=6371000., global_ec=base)
    d_land, d_ice = torch.from_numpy(land).cuda(), torch.from_numpy(ice).cuda()

    def topoo():
        z, o = torch.zeros(nO, dtype=torch.float64, device="cuda"), torch.ones(nO, dtype=torch.float64, device="cuda")
        return dict(FOCEANF=o.clone(), FGICEF=z.clone(), ZATMOF=z.clone(), FOCEAN=o.clone(), FLAKE=z.clone(), FGRND=z.clone(), FGICE=z.clone(),
                    ZATMO=z.clone(), ZLAKE=z.clone(), ZICETOP=z.clone())

    lines = []

    def report(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def whole():
        try:
            return gcmA.update_topo(topoo(), [d_land], [d_ice])
        except RuntimeError as e:
            return str(e)
    ms, out = best_of(reps, whole)
    report(config=config, call="update_topo", ms=round(ms, 3), halted=isinstance(out, str) and out.count("ERROR: "))
    t = topoo()
    ms1, (mask, errors) = best_of(reps, lambda: merge_topoO(topoo(), gcmO, [d_land], [d_ice], O, 6371000.))
    mask, errors = merge_topoO(t, gcmO, [d_land], [d_ice], O, 6371000.)
    report(config=config, call="merge_topoO", ms=round(ms1, 3), merged_cells=int(mask.sum()), errors=len(errors))
    fp, fm = t["FOCEANF"].cpu().numpy().reshape(-1), t["FOCEAN"].cpu().numpy().reshape(-1)
    ms2, (w, offsetE) = best_of(reps, lambda: gcmA.global_AvE([d_land], [d_ice], fp, fm, scale=True))
    report(config=config, call="global_AvE", ms=round(ms2, 3), nnz=w.nnz)
    nhc = len(gcmA.hcdefs)
    ui = [gcmA.underice(k) for k in range(nhc)]
    ms3, (a, errors2) = best_of(reps, lambda: make_topoA(t, mask, O, gcmA.hspecA, (1, gcmA.hspecA.size), gcmA.hcdefs, ui, w))
    report(config=config, call="make_topoA", ms=round(ms3, 3), nhc=nhc, errors=len(errors2))
    # the row statistics of the land build's OvI (scale = 1, correctA = 0) against an apply and a separate pass
    rm = gcmO.regrid_matrices("greenland", d_land, scale=False, correctA=True)
    OvI = rm.matrix_d("AvI", (SparseSet(), SparseSet.identity(g["nI"])), scale=True, correctA=False)
    x = d_land.reshape(1, -1)
    OvI.prepare(1)
    k1 = kernel_ms(reps, lambda: OvI.row_stats_device(d_land))
    k2 = kernel_ms(reps, lambda: OvI.apply_device(x, fill=float("nan"), force_conservation=False))
    k3 = kernel_ms(reps, lambda: OvI.row_stats_device(d_land, want_sum=False))
    report(config=config, call="row statistics", rows=OvI.nrow_d, nnz=OvI.nnz, row_stats_us=round(k1 * 1e3, 1), apply_us=round(k2 * 1e3, 1),
           minmax_pass_us=round(k3 * 1e3, 1), apply_plus_pass_over_row_stats=round((k2 + k3) / k1, 2))
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, "topo_times.txt"), "w") as f:
        f.write("GCMRegridder_ModelE.update_topo at %s (the synthetic Greenland sheet under the ModelE 144 x 90 ocean grid, a base ice matrix with 3\n"
                "elevation classes on every cell), MI355X.  scratch/topo_times.py %d %s: wall time of one call, best of %d, planes and masks in HBM;\n"
                "then the three calls on their own, and the kernel time (HIP events) of the row-statistics pass over the land build's OvI beside\n"
                "an apply of the same matrix and a separate min / max pass.  There is no earlier number to compare with.\n\n" % (config, reps, config, reps))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, sys.argv[2] if len(sys.argv) > 2 else "g5", *sys.argv[3:4])
