"""Times Hntr.regrid_device from 1-minute fields (Hntr; profiles/hntr_*.txt): 1' -> 1 deg and 1' -> 1/2 deg at
1 and 8 fields with a shared weight, and 1' -> 4 x 5 deg (the chain-bound case).  Device events around `reps` launches
after a warm-up; the algorithmic bytes are 8*(nvar+1)*nA + 8*nvar*nB.  Run it under rocprofv3 --kernel-trace --stats
for kernel times."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from icebin_amd import Hntr, HntrSpec  # noqa: E402

PEAK = 8e12
CASES = [("1min_to_1deg", (360, 180, 0., 60.), 1), ("1min_to_1deg", (360, 180, 0., 60.), 8),
         ("1min_to_halfdeg", (720, 360, 0., 30.), 1), ("1min_to_halfdeg", (720, 360, 0., 30.), 8),
         ("1min_to_4x5deg", (72, 45, 0., 240.), 1)]


def main(reps=5):
    dev = torch.device("cuda:0")
    A = HntrSpec(21600, 10800, 0., 1.)
    g = torch.Generator(device=dev).manual_seed(1)
    W = torch.rand(A.size, dtype=torch.float64, device=dev, generator=g)
    X = torch.rand((8, A.size), dtype=torch.float64, device=dev, generator=g)
    for name, bdef, nvar in CASES:
        B = HntrSpec(*bdef)
        h = Hntr(17.17, B, A, -1e30)
        out = h.regrid_device(W, X[:nvar])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = reps if B.size >= 64800 else 2
        e0.record()
        for _ in range(n):
            h.regrid_device(W, X[:nvar], out=out)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / n
        nbytes = 8 * (nvar + 1) * A.size + 8 * nvar * B.size
        print(json.dumps(dict(case=name, B="%dx%d" % (B.im, B.jm), nvar=nvar, ms=round(ms, 4), GBps=round(nbytes / ms / 1e6, 1),
                              share_of_8TBps=round(nbytes / PEAK / (ms * 1e-3), 3), floor_ms=round(nbytes / PEAK * 1e3, 4))), flush=True)
        del h


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
