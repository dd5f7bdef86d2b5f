"""Times Hntr.matrix_d builds and the applies of the scaled matrix from a 1-minute A grid (Hntr matrices;
profiles/hntr_matrix_*.txt): identity-dims builds onto 1/2 deg, 1 deg and 4 x 5 deg, the ModelE-shaped general-dims build
(1 deg ocean clipped to a pre-populated set, 2 x 2.5 deg A numbered ADD_DENSE, transposed), and the applies at 1 and 8
fields.  Build bytes: 12*nnz + 4*(nrow+1) + 8*(nrow+ncol).  Apply bytes: 12*nnz + 4*(nrow+1) + 8*nvar*(nrow+ncol).  Run it
under rocprofv3 --kernel-trace --stats for kernel times."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from icebin_amd import Hntr, HntrSpec, SparseSet  # noqa: E402

PEAK = 8e12
CASES = [("1min_to_halfdeg", (720, 360, 0., 30.)), ("1min_to_1deg", (360, 180, 0., 60.)), ("1min_to_4x5deg", (72, 45, 0., 240.))]


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


def main(reps=5):
    dev = torch.device("cuda:0")
    A = HntrSpec(21600, 10800, 0., 1.)
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.rand((8, A.size), dtype=torch.float64, device=dev, generator=g)
    for name, bdef in CASES:
        B = HntrSpec(*bdef)
        h = Hntr(17.17, B, A, -1e30)
        ms = best_ms(lambda: h.matrix_d("scaled"), reps)
        w = h.matrix_d("scaled")
        nbytes = 12 * w.nnz + 4 * (w.nrow_d + 1) + 8 * (w.nrow_d + w.ncol_d)
        print(json.dumps(dict(case=name, what="build", B="%dx%d" % (B.im, B.jm), nnz=w.nnz, ms=round(ms, 4),
                              share_of_8TBps=round(nbytes / PEAK / (ms * 1e-3), 3), floor_ms=round(nbytes / PEAK * 1e3, 4))), flush=True)
        for nvar in (1, 8):
            out = w.apply_device(X[:nvar], force_conservation=False)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                w.apply_device(X[:nvar], out=out, force_conservation=False)
            e1.record()
            torch.cuda.synchronize()
            ams = e0.elapsed_time(e1) / reps
            ab = 12 * w.nnz + 4 * (w.nrow_d + 1) + 8 * nvar * (w.nrow_d + w.ncol_d)
            print(json.dumps(dict(case=name, what="apply", nvar=nvar, kernel=w.last_kernel(), ms=round(ams, 4),
                                  share_of_8TBps=round(ab / PEAK / (ams * 1e-3), 3))), flush=True)
        del w, h
    # compute_AOmvAAm's shape: general dims
    B, A2 = HntrSpec(360, 180, 0., 60.), HntrSpec(144, 90, 0., 120.)
    ocean = np.nonzero(np.random.default_rng(3).random(B.size) < 0.7)[0]
    clip = np.zeros(B.size, bool)
    clip[ocean] = True
    h = Hntr(17.17, B, A2)
    ms = best_ms(lambda: h.matrix_d("overlap", 6371000., includeB=clip, dims=(SparseSet(B.size, ocean), SparseSet()),
                                    transforms=(2, 0), transpose=True), reps)
    print(json.dumps(dict(case="modele_AOmvAAm_1deg_2x2.5deg", what="build general dims", ms=round(ms, 4))), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
