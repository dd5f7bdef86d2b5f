"""Records which kernel every apply of a grid of calls launches: tests/golden/apply_choices.json.

Only the public Python API is used (linear_Weighted.from_csr, the regridder matrices of tests/apply_kernel_recipes.FAMILIES,
set_kernel, set_option, prepare, apply_device, apply_many_device, last_kernel, last_launch), so the script runs on any commit:
    python tests/golden/make_apply_choices.py <commit hash>      (on the GPU, at the commit whose choices are the record)
tests/test_gpu_apply_choices.py imports CASES and record() from here and replays the same calls.

A CASE is one matrix under one VARIANT: the default tunings, one per-handle option set alone, one set_kernel request, or (the
shapes around the realign threshold) result planes that start off the 64-byte lines.  For every (nvar, nbatch) of the case a fresh
handle is applied twice and, after prepare(nvar, nbatch), a third time; each apply records (last_kernel, last_launch).

The matrices: the E-row matrices of g20 and g5 (EvI), AvI, IvA, IvE and a smoothed IvE of g5; synthetic CSRs on either side of
every threshold of the choice a matrix of <= 2^21 entries reaches -- the mean row length (6, 64, 192, 768, 1024), the row count
(16384, 2^18, 2^19) and the entry count (2^20, 2^21: one column per entry, the shape of an AvI, so batched launches reach the
column sweep's work bound).  The shapes that are there for a size threshold alone are applied to <= 4 fields."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import apply_kernel_recipes as akr  # noqa: E402

NVARS = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 33, 47, 48, 63, 64, 96, 128)
NBATCH = (1, 3, 4, 7, 8, 33)
OPTIONS = (("rowgroup_form", 0), ("rowgroup_form", 1), ("rowone", 0), ("rowdual_auto", 0), ("sweep_auto", 0), ("rowblock_lpt", 1))
KERNELS = ("rowblock", "shortrow", "rowdual", "colsweep", "rowgroup")
REGRID = (("g20", "EvI", None), ("g5", "EvI", None), ("g5", "AvI", None), ("g5", "IvA", None), ("g5", "IvE", None),
          ("g5", "IvE", (30e3, 30e3, 100.)))
OUTPUT = os.path.join(HERE, "apply_choices.json")


def _cases():
    out = []
    options = [("default",)] + [("option", k, v) for k, v in OPTIONS]
    for fam, name, sigma in REGRID:
        mid = "%s_%s%s" % (fam, name, "_smoothed" if sigma else "")
        for var in options:
            out.append(dict(matrix=("regrid", fam, name, sigma), mid=mid, variant=var, nvars=NVARS, nbatch=NBATCH))
        for k in KERNELS:       # (a request for a family is independent of most of the grid: a coarser one)
            out.append(dict(matrix=("regrid", fam, name, sigma), mid=mid, variant=("kernel", k), nvars=(1, 4, 16, 32, 64, 128), nbatch=(1, 4, 33)))
    for mean, below in ((6, True), (64, True), (192, True), (768, False), (1024, False)):      # (>= 6, >= 64, >= 192; <= 768, <= 1024)
        for d in ((-1, 0) if below else (0, 1)):
            nnz = mean * 256 + d
            for var in options:
                out.append(dict(matrix=("csr", 256, nnz, 2048), mid="mean_%d" % nnz, variant=var, nvars=NVARS, nbatch=NBATCH))
    rows = [(n, per) for n in (16384, 16385) for per in (1, 3, 7)]
    rows += [(n, per) for n in ((1 << 18) - 1, 1 << 18, (1 << 19) - 1, 1 << 19) for per in (1, 3)]
    for n, per in rows:
        for var in options + [("misaligned",)]:
            out.append(dict(matrix=("csr", n, n * per, 4096), mid="rows_%d_x%d" % (n, per), variant=var, nvars=NVARS[:4], nbatch=NBATCH))
    for nnz in ((1 << 20) - 1, 1 << 20, (1 << 21) - 1, 1 << 21):
        for var in options:
            out.append(dict(matrix=("csr", nnz >> 9, nnz, 0), mid="entries_%d" % nnz, variant=var, nvars=NVARS[:4], nbatch=NBATCH))
    for c in out:
        c["id"] = c["mid"] + "-" + "_".join(str(x) for x in c["variant"])
    return out


CASES = _cases()
_cache = {}


def _csr(nrow, nnz, ncol):
    """nnz entries dealt evenly over nrow rows (the first nnz % nrow rows hold one more); a row's columns are consecutive.
    ncol == 0: one column per entry."""
    lens = np.full(nrow, nnz // nrow, np.int64)
    lens[:nnz % nrow] += 1
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    if ncol == 0:
        ncol, colind = nnz, np.arange(nnz)
    else:
        start = (np.arange(nrow) * 37) % (ncol - lens.max() + 1)
        colind = np.repeat(start, lens) + np.arange(nnz) - np.repeat(rowptr[:-1], lens)
    return (nrow, ncol), rowptr.astype(np.int32), colind.astype(np.int32), np.ones(nnz), np.ones(nrow), np.ones(ncol)


def _factory(matrix):
    """() -> a fresh handle of the case's matrix"""
    if matrix not in _cache:
        if matrix[0] == "csr":
            _cache.clear()          # (one synthetic matrix at a time: the cases come matrix by matrix)
            _cache[matrix] = _csr(*matrix[1:])
        else:
            import icebin_amd
            from icebin_amd import synthetic as syn
            _, fam, _, sigma = matrix
            cfg, kw, _ = akr.FAMILIES[fam]
            g = syn.make_grids(cfg, **kw)
            mm = icebin_amd.from_synthetic(g)
            kws = dict(sigma=sigma) if sigma else {}
            _cache[matrix] = (mm, mm.regrid_matrices("greenland", syn.dome_elevmask(g), scale=True, correctA=True, **kws))
    if matrix[0] == "csr":
        from icebin_amd.linear import linear_Weighted
        return lambda: linear_Weighted.from_csr(*_cache[matrix])
    return lambda: _cache[matrix][1].matrix(matrix[2])


def record(case):
    """[(nvar, nbatch, [(last_kernel, last_launch) of the first apply, the second, the one after prepare])] of one case"""
    import torch
    make = _factory(case["matrix"])
    var = case["variant"]
    w = make()
    nrow, ncol = w.nrow_d, w.ncol_d
    X = torch.zeros((max(case["nvars"]), ncol), dtype=torch.float64, device="cuda")
    ld = nrow + 5               # ("misaligned": an odd leading dimension at an odd offset)
    Y = torch.empty(3 + max(case["nbatch"]) * max(case["nvars"]) * ld, dtype=torch.float64, device="cuda") if var[0] == "misaligned" else None
    out = []
    for nvar in case["nvars"]:
        for nbatch in case["nbatch"]:
            w = make()
            if var[0] == "option":
                w.set_option(var[1], var[2])
            elif var[0] == "kernel":
                w.set_kernel(var[1])
            outs = None
            if Y is not None:
                outs = [Y[3 + q * nvar * ld:3 + (q + 1) * nvar * ld].view(nvar, ld)[:, :nrow] for q in range(nbatch)]
            seen = []
            for state in range(3):
                if state == 2:
                    w.prepare(nvar, nbatch)
                if nbatch == 1:
                    w.apply_device(X[:nvar], out=None if outs is None else outs[0])
                else:
                    w.apply_many_device([X[:nvar]] * nbatch, outs=outs)
                seen.append((w.last_kernel(), w.last_launch()))
            out.append((nvar, nbatch, seen))
    torch.cuda.synchronize()
    return out


def main():
    names, cases = [], {}
    for case in CASES:
        t0 = time.time()
        flat = []
        for _, _, seen in record(case):
            for s in seen:
                s = "%s|%s" % s
                if s not in names:
                    names.append(s)
                flat.append(names.index(s))
        cases[case["id"]] = flat
        print("%-40s %4d applies %6.2f s" % (case["id"], len(flat), time.time() - t0), flush=True)
    # names: "last_kernel|last_launch"; a case: indices into names, (nvar, nbatch) in the case's order, three states each
    with open(sys.argv[2] if len(sys.argv) > 2 else OUTPUT, "w") as f:
        json.dump(dict(commit=sys.argv[1], names=names, cases=cases), f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
