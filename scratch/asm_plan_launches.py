"""The kernel launches of the sorted-grid builds, for a comparison of two library builds (dev tool): run it under
`rocprofv3 --kernel-trace` once per build (ICEBIN_HIP_LIB) and hand the two traces to scratch/compare_launches.py.
Builds, a few times each: the six matrices on the synthetic 20 km / 5 km / 1 km grids, the coupler's step (EvI / AvI / IvE / XvE on
identity dims and a shared dimE, one after the other and as one batched call), and the small cases of tests/assembly_limit_cases.py
under each of their knob sets.  A one-element torch cos_() separates the builds in the trace; the labels go to argv[1]."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import icebin_amd
from icebin_amd import synthetic as syn
import assembly_limit_cases as alc
from test_gpu_assembly_limits import KNOBS, identity_dims

labels = []
mark = torch.zeros(1, device="cuda")


def build(label, fn):
    torch.cuda.synchronize()
    mark.cos_()
    torch.cuda.synchronize()
    labels.append(label)
    w = fn()
    torch.cuda.synchronize()
    return w


for cfg in ("g20", "g5", "g1"):
    g = syn.make_grids(cfg)
    em = syn.dome_elevmask(g)
    mm = icebin_amd.from_synthetic(g)
    rm = mm.regrid_matrices("greenland", em, scale=True, correctA=True)
    nI, nX, nE = g["nI"], len(g["ex_area"]), g["nA"] * len(g["hcdefs"])
    for rep in range(3):
        for name in ("AvI", "IvA", "EvI", "IvE", "XvE", "EvA"):
            build("%s %s own dims #%d" % (cfg, name, rep), lambda: rm.matrix(name))
    for rep in range(3):
        rs = mm.regrid_matrices("greenland", em + 0.01 * rep, scale=True, correctA=False)
        dimI, dimE, dimX = icebin_amd.SparseSet.identity(nI), icebin_amd.SparseSet(nE), icebin_amd.SparseSet.identity(nX)
        build("%s step EvI (fresh dimE, identity dimI) #%d" % (cfg, rep), lambda: rs.matrix_d("EvI", (dimE, dimI), scale=False, correctA=False))
        build("%s step AvI (identity dimI) #%d" % (cfg, rep), lambda: rs.matrix_d("AvI", (None, dimI), scale=False, correctA=False))
        build("%s step IvE (identity dimI, shared dimE) #%d" % (cfg, rep), lambda: rs.matrix_d("IvE", (dimI, dimE), scale=True, correctA=False))
        build("%s step XvE (identity dimX, shared dimE) #%d" % (cfg, rep), lambda: rs.matrix_d("XvE", (dimX, dimE), scale=False, correctA=False))
        dimI, dimE, dimX = icebin_amd.SparseSet.identity(nI), icebin_amd.SparseSet(nE), icebin_amd.SparseSet.identity(nX)
        build("%s step batched (unordered) #%d" % (cfg, rep),
              lambda: rs.matrix_batch([("EvI", (dimE, dimI), False, False), ("AvI", (None, dimI), False, False),
                                       ("IvE", (dimI, dimE), True, False), ("XvE", (dimX, dimE), False, False)]))

for case in alc.CASES:
    if sum(case["grid"]["ranges"]) >= 1 << 20:
        continue
    g, em = alc.build_grid(case["grid"])
    mm = icebin_amd.from_synthetic(g)
    for knobs in case["knobs"]:
        for k in KNOBS:
            icebin_amd.set_tuning(k, -2 ** 31)
        for k, v in knobs.items():
            icebin_amd.set_tuning(k, v)
        rm = mm.regrid_matrices("greenland", em)
        for name, branches, dims in case["builds"]:
            for rep in range(2):
                build("limits:%s %s dims=%s knobs=%s #%d" % (case["name"], name, dims, sorted(knobs.items()), rep),
                      lambda: rm.matrix_d(name, identity_dims(name, g, True) if dims == "identity" else (None, None), scale=True, correctA=True))
    for k in KNOBS:
        icebin_amd.set_tuning(k, -2 ** 31)
build("end", lambda: None)
with open(sys.argv[1], "w") as f:
    f.write("\n".join(labels) + "\n")
print("%d builds" % (len(labels) - 1))
