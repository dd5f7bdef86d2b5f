"""Wall time of the smoothed builds scratch/time_smooth.py makes, best of 5 after one warm-up build, in the format of
profiles/r06_sharded_smoothing.txt (dev tool).  argv[1]: the label of the library under test (ICEBIN_HIP_LIB), e.g. parent / new."""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import icebin_amd
from icebin_amd import _capi, synthetic as syn

if not hasattr(ctypes.CDLL(_capi.LIB_PATH), "ibh_weighted_smoothed_by"):       # a library from before the getter existed
    _capi._SIGS.pop("ibh_weighted_smoothed_by")
label = sys.argv[1] if len(sys.argv) > 1 else "run"
for cfg, sig in (("g20", (60e3, 60e3, 250.)), ("g5", (50e3, 50e3, 100.)), ("g5", (25e3, 25e3, 100.))):
    g = syn.make_grids(cfg)
    em = syn.dome_elevmask(g)
    rm = icebin_amd.from_synthetic(g).regrid_matrices("greenland", em, scale=True, correctA=True, sigma=sig)
    for name in ("IvA", "IvE"):
        w = rm.matrix(name)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            w = rm.matrix(name)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        print("%s %s %s sigma=%s nnz=%d best-of-5 %.3f ms (all: %s)" % (label, cfg, name, sig, w.nnz, min(ts), " ".join("%.3f" % t for t in ts)), flush=True)
