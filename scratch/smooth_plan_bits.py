"""The bits and the launches of the smoothed builds, for a comparison of two library builds (dev tool).  Prints, for IvA / IvE on the
synthetic 50 km / 20 km / 5 km grids under a set of sigmas and the five (smooth_direct, smooth_tile) settings, nnz and the SHA-256 of
rowptr, colind, the bits of val, wM and Mw: run it once per library (ICEBIN_HIP_LIB) and diff the outputs.  With a file name as
argv[1] a one-element torch cos_() separates the builds and the labels go to that file: run it under `rocprofv3 --kernel-trace` and
hand the two traces to scratch/compare_launches.py.  (5 km takes the two narrow sigmas only: the triplet pipeline of a wide one
does not fit a card.)"""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import icebin_amd
from icebin_amd import _capi, synthetic as syn

if not hasattr(ctypes.CDLL(_capi.LIB_PATH), "ibh_weighted_smoothed_by"):       # a library from before the getter existed
    _capi._SIGS.pop("ibh_weighted_smoothed_by")

SIGMAS = ((60e3, 60e3, 250.0), (120e3, 120e3, 400.0), (200e3, 200e3, 1500.0), (50e3, 50e3, 100.0), (25e3, 25e3, 100.0))
KNOBS = ((-1, -1), (0, 1), (1, 0), (0, 0), (1, 1))
label_file = sys.argv[1] if len(sys.argv) > 1 else None
labels = []
mark = torch.zeros(1, device="cuda")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


for cfg in ("g50", "g20", "g5"):
    g = syn.make_grids(cfg)
    em = syn.dome_elevmask(g)
    mm = icebin_amd.from_synthetic(g)
    for sigma in (SIGMAS[3:] if cfg == "g5" else SIGMAS):
        rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True, sigma=sigma)
        for name in ("IvA", "IvE"):
            for direct, tile in KNOBS:
                label = "%s %s sigma=(%g, %g, %g) smooth_direct=%d smooth_tile=%d" % ((cfg, name) + sigma + (direct, tile))
                icebin_amd.set_tuning("smooth_direct", direct)
                icebin_amd.set_tuning("smooth_tile", tile)
                if label_file:
                    torch.cuda.synchronize()
                    mark.cos_()
                    torch.cuda.synchronize()
                    labels.append(label)
                try:
                    w = rm.matrix(name)
                    torch.cuda.synchronize()
                    rowptr, colind, val = w.csr_dense()
                    print("%s: nnz=%d conservative=%d rowptr=%s colind=%s val=%s wM=%s Mw=%s" % (
                        label, w.nnz, w.conservative, sha(rowptr), sha(colind), sha(val), sha(w.wM), sha(w.Mw)), flush=True)
                except icebin_amd.IcebinHipError as e:
                    print("%s: error %d %s" % (label, e.code, e), flush=True)
                finally:
                    icebin_amd.set_tuning("smooth_direct", -1)
                    icebin_amd.set_tuning("smooth_tile", -1)
if label_file:
    torch.cuda.synchronize()
    mark.cos_()
    torch.cuda.synchronize()
    labels.append("end")
    with open(label_file, "w") as f:
        f.write("\n".join(labels) + "\n")
