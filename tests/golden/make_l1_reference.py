"""Writes tests/golden/l1_reference.npz: the L1 cases of tests/l1_restatement.py with, per case, the exchange polygons, the
terms of the reference's own pylib/icebin/element_l1.py (loaded by path: it needs numpy and scipy only), its weightsA and
weightsI, the same terms in exact rational arithmetic from the same float inputs, and
    ref_err      max |reference - exact| / polygon area
    restate_err  max |restatement - exact| / element area    (the measure tests/test_l1_restatement.py bounds)
CPU only.  Usage: python tests/golden/make_l1_reference.py <path to the reference's pylib/icebin/element_l1.py>"""
import importlib.util
import os
import sys
import time
from types import SimpleNamespace as NS

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import l1_restatement as R  # noqa: E402


def reference_module(path):
    spec = importlib.util.spec_from_file_location("reference_element_l1", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def duck_grids(c, iA, iTri, vptr, qx, qy):
    """Objects with the attribute names compute_AvI reads (element_l1.py:118-143)."""
    verts = [NS(index=k, x=float(c["vx"][k]), y=float(c["vy"][k])) for k in range(len(c["vx"]))]
    gridI = NS(cells={t: NS(vertices=[verts[v] for v in el]) for t, el in enumerate(c["tri"])}, indexing=NS(base=[0]),
               vertices_nfull=len(verts))
    cellsX = {x: NS(i=int(iA[x]), j=int(iTri[x]), vertices=[NS(x=float(qx[k]), y=float(qy[k])) for k in range(vptr[x], vptr[x + 1])])
              for x in range(len(iA))}
    return NS(cells=cellsX), gridI


def main():
    ref = reference_module(sys.argv[1])
    out = {}
    for name, c in R.build_cases().items():
        t0 = time.time()
        iA, iTri, vptr, qx, qy = R.make_exgrid(c["vx"], c["vy"], c["tri"], R.polys_of(c), c["iA_poly"])
        exgrid, gridI = duck_grids(c, iA, iTri, vptr, qx, qy)
        M, wA, wI = ref.compute_AvI(exgrid, int(c["nA"]), gridI)
        ref_terms = np.asarray(M.data, np.float64).reshape(-1, 3)       # coo data in emission order: cell, then basis function
        exact, areas, elem = R.exact_terms(c["vx"], c["vy"], c["tri"], iTri, vptr, qx, qy)
        restated = R.cell_terms(c["vx"], c["vy"], c["tri"], iTri, vptr, qx, qy)
        ref_err = R.max_err_over(ref_terms, exact, areas)
        restate_err = R.max_err_over(restated, exact, elem)
        restate_err_poly = R.max_err_over(restated, exact, areas)
        # the exact terms as the nearest doubles, and a second double for what is left: tests rebuild the Fraction from the pair
        hi = np.array([[float(v) for v in s] for s in exact])
        from fractions import Fraction
        lo = np.array([[float(exact[x][k] - Fraction(hi[x][k])) for k in range(3)] for x in range(len(exact))])
        nnz = len(set(zip(M.row.tolist(), M.col.tolist())))
        for k, v in c.items():
            out[name + "/" + k] = v
        for k, v in dict(ex_iA=iA, ex_iTri=iTri, ex_vptr=vptr, ex_qx=qx, ex_qy=qy, ref_terms=ref_terms, ref_weightsA=np.asarray(wA, float),
                         ref_weightsI=np.asarray(wI, float), exact_hi=hi.reshape(-1, 3), exact_lo=lo.reshape(-1, 3),
                         poly_area=np.array([float(a) for a in areas]), elem_area=np.array([float(a) for a in elem]),
                         ref_err=np.float64(ref_err), restate_err=np.float64(restate_err), restate_err_poly=np.float64(restate_err_poly),
                         nnz=np.int64(nnz)).items():
            out[name + "/" + k] = v
        print("%-12s nX=%4d nnz=%4d ref_err=%.2e restate_err=%.2e (per polygon area %.2e)  %.1fs"
              % (name, len(iA), nnz, ref_err, restate_err, restate_err_poly, time.time() - t0))
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
