"""icebin.element_l1: the reference's entry point compute_AvI(exgrid, nA, gridI) (pylib/icebin/element_l1.py:96-148) over
the HIP library.  Grid objects are read through the reference's attribute names only:
    exgrid.cells[*].vertices[*].x/.y, .i (GCM cell), .j (element);  gridI.cells[*].vertices[*].index/.x/.y,
    gridI.indexing.base, gridI.vertices_nfull."""
import numpy as np
import scipy.sparse

from icebin_amd import l1


def _values(cells):
    return list(cells.values()) if hasattr(cells, "values") else list(cells)


def compute_AvI(exgrid, nA, gridI):
    """Returns (AvI, weightsA, weightsI): a scipy coo_matrix [nA, gridI.vertices_nfull] and its row and column sums.
        fA = (1/weightsA) AvI fI;   fI = (1/weightsI) IvA fA with IvA = transpose(AvI)."""
    base = int(gridI.indexing.base[0])
    nI = int(gridI.vertices_nfull)
    vx, vy = np.zeros(nI), np.zeros(nI)
    elements = _values(gridI.cells)
    keys = list(gridI.cells.keys()) if hasattr(gridI.cells, "keys") else list(range(len(elements)))
    ordinal = {k: n for n, k in enumerate(keys)}
    tri = np.zeros((len(elements), 3), np.int32)
    for n, cell in enumerate(elements):
        if len(cell.vertices) != 3:
            raise ValueError("element %r has %d vertices" % (keys[n], len(cell.vertices)))
        for k, v in enumerate(cell.vertices):
            tri[n, k] = v.index - base
            vx[tri[n, k]], vy[tri[n, k]] = v.x, v.y
    mesh = l1.Mesh(vx, vy, tri)
    cellsX = _values(exgrid.cells)
    ex = l1.exchange_grid_from_polygons([c.i - base for c in cellsX], [ordinal[c.j] for c in cellsX],
                                        polys=[[(v.x, v.y) for v in c.vertices] for c in cellsX])
    w = l1.compute_AvI(ex, nA, mesh)
    row, col, val = w.coo_dense()
    return scipy.sparse.coo_matrix((val, (row, col)), shape=(nA, nI)), w.wM, w.Mw
