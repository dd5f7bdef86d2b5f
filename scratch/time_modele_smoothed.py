"""Wall time of the smoothed IvE / IvA through to_modele against the work they are made of (dev tool; profiles/modele_smoothed_times.txt).
Grid g5, ocean HntrSpec(144, 90, 0, 120), sigma = (60 km, 45 km, 250 m), no ocean.  Per build: 3 warm-up builds, then the median of 15
with the smallest, the largest and the quartiles -- the spread is the interquartile range.

  argv[1] = parent: (a) with ICEBIN_HIP_LIB naming a library of the parent commit: the O-grid smoothed IvE / IvA (scale = False,
                    correctA = False) and the unsmoothed to_modele IvE / IvA (scale = True); the smoothed to_modele build contains both
                    kinds of work, so their sum is the yardstick
  argv[1] = new:    (a) again, on this library; (b) the smoothed to_modele IvE / IvA with modele_rowlocal = 0 (crop_cols + the
                    generic product); (c) with modele_rowlocal = 1 (the row-local composition)"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import icebin_amd
from icebin_amd import HntrSpec, _capi, synthetic as syn
from icebin_amd.linear import linear_Weighted

_probe = C.CDLL(_capi.LIB_PATH)
for _name in [n for n in _capi._SIGS if not hasattr(_probe, n)]:         # a library from before an entry existed
    _capi._SIGS.pop(_name)
mode = sys.argv[1] if len(sys.argv) > 1 else "new"
SIGMA = (60e3, 45e3, 250.)
WARM, REPS = 3, 15


def timed(label, build):
    for _ in range(WARM):
        w = build()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        w = build()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    print("%-44s nnz=%-8d median %8.3f ms  IQR %6.3f  (min %.3f q1 %.3f q3 %.3f max %.3f)" % (label, w.nnz, q[2], q[3] - q[1], q[0], q[1],
                                                                                            q[3], q[4]), flush=True)
    return q[2], q[3] - q[1]


def modele_plain(rm, name):
    """The sigma = 0 entry, which every library has."""
    h = C.c_void_p()
    _capi.check(_capi.lib().ibh_modele_matrices_matrix_d(rm._h, name.encode(), None, None, 1, C.byref(h)))
    return linear_Weighted(h, keep=(rm,))


g = syn.make_grids("g5")
em = syn.dome_elevmask(g)
gcm = icebin_amd.from_synthetic(g)
hspecO = HntrSpec(144, 90, 0., 120.)
rmO = gcm.regrid_matrices("greenland", em)
rm = gcm.to_modele(None, hspecO=hspecO, eq_rad=6371000.).regrid_matrices("greenland", em)
print("# %s library %s" % (mode, os.path.basename(_capi.LIB_PATH)), flush=True)
res = {}
for name in ("IvE", "IvA"):
    res["a_smooth", name] = timed("(a) %s O-grid %s smoothed" % (mode, name),
                                  lambda: rmO.matrix_d(name, scale=False, correctA=False, sigma=SIGMA))
    res["a_modele", name] = timed("(a) %s to_modele %s sigma=0" % (mode, name), lambda: modele_plain(rm, name))
    print("(a) %s %s: the sum of the two medians %.3f ms" % (mode, name, res["a_smooth", name][0] + res["a_modele", name][0]), flush=True)
if mode == "new":
    for key, knob, what in (("b", 0, "crop_cols + product"), ("c", 1, "row-local")):
        icebin_amd.set_tuning("modele_rowlocal", knob)
        for name in ("IvE", "IvA"):
            w = rm.matrix_d(name, scale=True, sigma=SIGMA)
            assert w.composed_by() == knob + 1
            res[key, name] = timed("(%s) to_modele %s smoothed, %s" % (key, name, what), lambda: rm.matrix_d(name, scale=True, sigma=SIGMA))
    icebin_amd.set_tuning("modele_rowlocal", -1)
    for name in ("IvE", "IvA"):
        a = res["a_smooth", name][0] + res["a_modele", name][0]
        (b, sb), (c, sc) = res["b", name], res["c", name]
        print("%s: (b) %.3f ms = %.2f x (a), (c) %.3f ms = %.2f x (a); (b) - (c) = %.3f ms against a spread of %.3f ms" % (
            name, b, b / a, c, c / a, b - c, max(sb, sc)), flush=True)
