"""linear_Weighted: the Python face of ibmisc::linear::Weighted (sphinx/source/matrix_formats.rst:121-195),
and SparseSet (spsparse::SparseSet<long,int>), both thin handles over the C-ABI."""
import ctypes as C

import numpy as np

from . import _capi
from ._arrays import dptr, leading_dim, padded_planes, plane_stride, stream_arg, to_device
from ._capi import check, lib, ptr


class SparseSet(_capi.Handle):
    """spsparse::SparseSet<long,int>: dense ids handed out first-seen (eigen_types.hpp:24)."""
    _destroy = "ibh_sparse_set_destroy"

    def __init__(self, sparse_extent=-1, to_sparse=None, _handle=None):
        h = C.c_void_p()
        if _handle is not None:
            h = _handle
        elif to_sparse is None:
            check(lib().ibh_sparse_set_create(int(sparse_extent), C.byref(h)))
        else:
            a = np.ascontiguousarray(to_sparse, np.int64)
            check(lib().ibh_sparse_set_from_array(int(sparse_extent), ptr(a), len(a), C.byref(h)))
        self._h = h

    @classmethod
    def identity(cls, n):
        """ibmisc id_sparse_set(n) (modele/merge_topo.cpp:48, IceCoupler.cpp:366)."""
        h = C.c_void_p()
        check(lib().ibh_sparse_set_create_identity(int(n), C.byref(h)))
        return cls(_handle=h)

    def sparse_extent(self):
        v = C.c_int64()
        check(lib().ibh_sparse_set_sparse_extent(self._h, C.byref(v)))
        return v.value

    def dense_extent(self):
        v = C.c_int32()
        check(lib().ibh_sparse_set_dense_extent(self._h, C.byref(v)))
        return v.value

    def to_sparse(self):
        out = np.empty(self.dense_extent(), np.int64)
        check(lib().ibh_sparse_set_to_sparse(self._h, ptr(out)))
        return out

    def add_dense(self, sparse):
        """Existing dense id of `sparse`, or the next one (first-seen order)."""
        d = C.c_int32()
        check(lib().ibh_sparse_set_add_dense(self._h, int(sparse), C.byref(d)))
        return d.value

    def to_dense(self, sparse):
        d = C.c_int32()
        check(lib().ibh_sparse_set_to_dense(self._h, int(sparse), C.byref(d)))
        if d.value < 0:
            raise KeyError(sparse)
        return d.value

    def in_sparse(self, sparse):
        d = C.c_int32()
        check(lib().ibh_sparse_set_to_dense(self._h, int(sparse), C.byref(d)))
        return d.value >= 0

    def add_dense_multivec(self, mv, stream=None):
        """add_dense of every index of a VectorMultivec in entry order, on the device (IceCoupler.cpp:294-300)."""
        check(lib().ibh_sparse_set_add_dense_multivec(self._h, mv._h, C.c_void_p(stream)))


class linear_Weighted(_capi.Handle):
    """A regrid matrix M plus its two weight vectors, resident in HBM.

    Mirrors ibmisc.linear_Weighted (matrix_formats.rst:139-195): apply_M, apply_weight, apply_wM,
    apply_Mw, to_coo, get_weights, shape; plus the C++ members of linear::Weighted_Eigen the IceBin
    callers touch (dims, wM, Mw, conservative, scaled, apply()).
    """
    _destroy = "ibh_weighted_destroy"

    def __init__(self, handle, keep=()):
        self._h = handle
        self._keep = keep          # objects that must outlive the handle (shared dims, regridder)
        nrow, ncol, nnz = C.c_int32(), C.c_int32(), C.c_int64()
        check(lib().ibh_weighted_shape(handle, C.byref(nrow), C.byref(ncol), C.byref(nnz)))
        self.nrow_d, self.ncol_d, self.nnz = nrow.value, ncol.value, nnz.value
        cons, sc = C.c_int(), C.c_int()
        check(lib().ibh_weighted_flags(handle, C.byref(cons), C.byref(sc)))
        self.conservative, self.scaled = bool(cons.value), bool(sc.value)
        self._dims = [None, None]
        self._sparse_extents = [None, None]

    # ---- loaders -------------------------------------------------------------------------
    @classmethod
    def from_coo(cls, shape, row, col, val, wM, Mw, conservative=True, scaled=True):
        """Dense-indexed triplets -> Weighted (to_eigen_M, eigen_types.cpp:9-34 / nc_read_weighted)."""
        row = np.ascontiguousarray(row, np.int32)
        col = np.ascontiguousarray(col, np.int32)
        val = np.ascontiguousarray(val, np.float64)
        wM = np.ascontiguousarray(wM, np.float64)
        Mw = np.ascontiguousarray(Mw, np.float64)
        assert len(row) == len(col) == len(val) and len(wM) == shape[0] and len(Mw) == shape[1]
        h = C.c_void_p()
        check(lib().ibh_weighted_from_coo(shape[0], shape[1], len(val), ptr(row), ptr(col), ptr(val), ptr(wM), ptr(Mw),
                                         int(conservative), int(scaled), C.byref(h)))
        return cls(h)

    @classmethod
    def from_csr(cls, shape, rowptr, colind, val, wM, Mw, conservative=True, scaled=True):
        rowptr = np.ascontiguousarray(rowptr, np.int32)
        colind = np.ascontiguousarray(colind, np.int32)
        val = np.ascontiguousarray(val, np.float64)
        wM = np.ascontiguousarray(wM, np.float64)
        Mw = np.ascontiguousarray(Mw, np.float64)
        assert len(rowptr) == shape[0] + 1 and len(wM) == shape[0] and len(Mw) == shape[1]
        h = C.c_void_p()
        check(lib().ibh_weighted_from_csr(shape[0], shape[1], ptr(rowptr), ptr(colind), ptr(val), ptr(wM), ptr(Mw),
                                         int(conservative), int(scaled), C.byref(h)))
        return cls(h)

    # ---- members -------------------------------------------------------------------------
    def dim(self, k):
        """dims[k]: dense -> sparse index table of this matrix (int64[dense_extent])."""
        if self._dims[k] is None:
            n = self.nrow_d if k == 0 else self.ncol_d
            out = np.empty(n, np.int64)
            check(lib().ibh_weighted_dim_to_sparse(self._h, k, ptr(out)))
            ext = C.c_int64()
            check(lib().ibh_weighted_dim(self._h, k, C.byref(ext), None))
            self._dims[k], self._sparse_extents[k] = out, ext.value
        return self._dims[k]

    def sparse_extent(self, k):
        self.dim(k)
        return self._sparse_extents[k]

    @property
    def shape(self):
        """Sparse shape of the matrix."""
        return (self.sparse_extent(0), self.sparse_extent(1))

    @property
    def wM(self):
        out = np.empty(self.nrow_d, np.float64)
        check(lib().ibh_weighted_get_wM(self._h, ptr(out)))
        return out

    @property
    def Mw(self):
        out = np.empty(self.ncol_d, np.float64)
        check(lib().ibh_weighted_get_Mw(self._h, ptr(out)))
        return out

    def get_weights(self, dim):
        """Weight vector in the sparse space (0 = B/output, 1 = A/input); zero where unset."""
        out = np.zeros(self.sparse_extent(dim), np.float64)
        out[self.dim(dim)] = self.wM if dim == 0 else self.Mw
        return out

    def coo_dense(self):
        """(row_d, col_d, val) in row-major order, dense index spaces."""
        row = np.empty(self.nnz, np.int32)
        col = np.empty(self.nnz, np.int32)
        val = np.empty(self.nnz, np.float64)
        check(lib().ibh_weighted_get_coo(self._h, ptr(row), ptr(col), ptr(val)))
        return row, col, val

    def csr_dense(self):
        rowptr = np.empty(self.nrow_d + 1, np.int32)
        col = np.empty(self.nnz, np.int32)
        val = np.empty(self.nnz, np.float64)
        check(lib().ibh_weighted_get_csr(self._h, ptr(rowptr), ptr(col), ptr(val)))
        return rowptr, col, val

    def to_coo(self):
        """scipy.sparse.coo_matrix in the ORIGINAL sparse index spaces (matrix_formats.rst:188-192)."""
        import scipy.sparse
        row, col, val = self.coo_dense()
        return scipy.sparse.coo_matrix((val, (self.dim(0)[row], self.dim(1)[col])), shape=self.shape)

    # ---- on-disk "Eigen format" (matrix_formats.rst:9-63) -----------------------------------
    def ncio(self, ds, vname, dim_names):
        """Weighted_Eigen::ncio(ncio, vname, {dimB, dimA}) into an icebin_amd.ncio.Dataset (write side;
        modele/global_ec.cpp:571-629, IceCoupler.cpp:473-488)."""
        from . import ncio
        row, col, val = self.coo_dense()
        ncio.put_weighted(ds, vname, dim_names, (self.dim(0), self.dim(1)), (self.sparse_extent(0), self.sparse_extent(1)),
                          row, col, val, self.wM, self.Mw, self.conservative, self.scaled)

    @classmethod
    def nc_read(cls, ds, vname):
        """ibmisc.nc_read_weighted(nc, vname) (matrix_formats.rst:139-147): the matrix, its weights and its
        dims from an Eigen-format file (a path or an icebin_amd.ncio.Dataset)."""
        from . import ncio
        if isinstance(ds, (str, bytes)) or hasattr(ds, "__fspath__"):
            ds = ncio.Dataset.read(ds)
        d = ncio.get_weighted(ds, vname)
        w = cls.from_coo((len(d["dims"][0]), len(d["dims"][1])), d["row"], d["col"], d["val"], d["wM"], d["Mw"],
                         d["conservative"], d["scaled"])
        w._dims = [np.asarray(d["dims"][0], np.int64), np.asarray(d["dims"][1], np.int64)]
        w._sparse_extents = list(d["sparse_extents"])
        return w

    # ---- products ------------------------------------------------------------------------
    def apply(self, A_b, fill=np.nan, force_conservation=True):
        """Weighted_Eigen::apply(A_b, fill, force_conservation, tmp) in DENSE index spaces
        (modele/merge_topo.cpp:65, modele/icebin22m.cpp:153).  A_b: [ncol_d] or [nvar, ncol_d]."""
        A = np.ascontiguousarray(np.atleast_2d(A_b), np.float64)
        if A.shape[1] != self.ncol_d:
            raise ValueError("apply: input has %d columns, matrix has %d dense columns" % (A.shape[1], self.ncol_d))
        B = np.empty((A.shape[0], self.nrow_d), np.float64)
        check(lib().ibh_weighted_apply_host(self._h, ptr(A), A.shape[0], A.shape[1], ptr(B), B.shape[1], float(fill),
                                           int(force_conservation)))
        return B if np.ndim(A_b) == 2 else B[0]

    def apply_device(self, dA, out=None, fill=float("nan"), force_conservation=True, stream=None):
        """Same on fields already resident in HBM: dA is a torch.float64 CUDA tensor [nvar, ncol_d]
        (row stride >= ncol_d); only enqueues work on `stream` (default: torch's current stream)."""
        import torch
        nvar, lda = _fields(torch, (dA,), self.ncol_d)
        out, ldb = _result(torch, out, nvar, self.nrow_d, dA.device)
        check(lib().ibh_weighted_apply_device(self._h, dA.data_ptr(), nvar, lda, out.data_ptr(), ldb, float(fill), int(force_conservation),
                                             stream_arg(dA, stream)))
        return out

    def apply_many_device(self, dAs, outs=None, fill=float("nan"), force_conservation=True, stream=None):
        """Several field batches through one launch (ibh_weighted_apply_many_device): dAs is a list of
        torch.float64 CUDA tensors [nvar, ncol_d] of equal shape and row stride; returns the list of
        results.  Bitwise the results of separate apply_device calls."""
        import torch
        nb = len(dAs)
        if nb == 0:
            return []
        nvar, lda = _fields(torch, dAs, self.ncol_d)
        if outs is None:
            outs = [padded_planes(nvar, self.nrow_d, dAs[0].device) for _ in range(nb)]
        ldb = _fields(torch, outs, self.nrow_d, "out", nvar)[1]
        xp = (C.c_void_p * nb)(*[a.data_ptr() for a in dAs])
        yp = (C.c_void_p * nb)(*[o.data_ptr() for o in outs])
        check(lib().ibh_weighted_apply_many_device(self._h, nb, xp, nvar, lda, yp, ldb, float(fill), int(force_conservation),
                                                  stream_arg(dAs[0], stream)))
        return outs

    def row_stats_device(self, dx, want_sum=True, want_min=True, want_max=True, stream=None):
        """(sum, min, max) per dense row over the STORED entries, in one pass over the CSR (ibh_weighted_row_stats_device):
        sum[r] = sum of val * x[col], min / max of x[col] starting from DBL_MAX / DBL_MIN (the smallest positive normal number,
        as merge_topoO's zland_max does).  dx: a contiguous torch.float64 CUDA tensor [ncol_d], which may hold NaN in columns
        no entry names.  An output not wanted is None.  Only enqueues work on `stream` (default: torch's current stream)."""
        import torch
        assert dx.is_cuda and dx.dtype == torch.float64 and dx.is_contiguous() and dx.numel() == self.ncol_d
        outs = [torch.empty(self.nrow_d, dtype=torch.float64, device=dx.device) if want else None for want in (want_sum, want_min, want_max)]
        check(lib().ibh_weighted_row_stats_device(self._h, dptr(dx), *[dptr(o) for o in outs], stream_arg(dx, stream)))
        return tuple(outs)

    def reserve(self, nvar):
        """Size the handle's per-apply scratch for up to nvar variables (needed before capturing
        applies into a hipGraph: growing scratch allocates)."""
        check(lib().ibh_weighted_reserve(self._h, int(nvar)))

    def prepare(self, nvar, nbatch=1):
        """Make applies of up to nvar variables, up to nbatch batches per launch, pure enqueues: builds the
        column-sweep / band structure those applies would otherwise build lazily on their second call and
        sizes all scratch (ibh_weighted_prepare).  Call once per matrix before capturing applies into a
        hipGraph or when the latency of the first applies matters."""
        check(lib().ibh_weighted_prepare(self._h, int(nvar), int(nbatch)))

    def pair_prepare(self, second, nvar=16):
        """Prepare the fused pair  B1 = self * A,  B2 = second * B1  (ibh_weighted_pair_prepare): EvI followed by AvE.
        Raises IcebinHipError (IBH_ENOTIMPL) when the two matrices do not pair; then make two applies."""
        check(lib().ibh_weighted_pair_prepare(self._h, second._h, int(nvar)))
        self._pair = second          # (keeps the second handle alive as long as the pairing)

    def apply_pair_device(self, second, dA, out1=None, out2=None, fill=float("nan"), stream=None):
        """One launch for both products (ibh_weighted_apply_pair_device); returns (B1, B2).  B1 is bitwise apply_device's
        result, B2 = second.apply_device(B1, force_conservation=False) to 1e-12."""
        import torch
        nvar, lda = _fields(torch, (dA,), self.ncol_d)
        out1, ld1 = _result(torch, out1, nvar, self.nrow_d, dA.device)
        out2, ld2 = _result(torch, out2, nvar, second.nrow_d, dA.device)
        check(lib().ibh_weighted_apply_pair_device(self._h, second._h, dA.data_ptr(), nvar, lda, out1.data_ptr(), ld1, out2.data_ptr(), ld2, float(fill),
                                                  stream_arg(dA, stream)))
        return out1, out2

    def apply_chain_device(self, second, third, dA, out1=None, out2=None, out3=None, fill=float("nan"), stream=None):
        """B1 = self * A, B2 = second * B1 (the fused pair: pair_prepare(second) first), B3 = third * B2, as two stream-ordered
        launches (ibh_weighted_apply_chain_device); returns (B1, B2, B3), bitwise the pair apply followed by third.apply_device."""
        import torch
        nvar, lda = _fields(torch, (dA,), self.ncol_d)
        out1, ld1 = _result(torch, out1, nvar, self.nrow_d, dA.device)
        out2, ld2 = _result(torch, out2, nvar, second.nrow_d, dA.device)
        out3, ld3 = _result(torch, out3, nvar, third.nrow_d, dA.device)
        check(lib().ibh_weighted_apply_chain_device(self._h, second._h, third._h, dA.data_ptr(), nvar, lda, out1.data_ptr(), ld1,
                                                   out2.data_ptr(), ld2, out3.data_ptr(), ld3, float(fill), stream_arg(dA, stream)))
        return out1, out2, out3

    def apply_transformed_device(self, dV, T, b, out=None, fill=float("nan"), stream=None):
        """The coupler's fused product  M * (V*T + b)  on HBM-resident fields (IceCoupler.cpp:203-252,
        :445): dV torch.float64 CUDA [nvar_in, ncol_d]; T [nvar_in, nvar_out] (the sparse variable
        transform as a dense array, exact zeros are structural), b [nvar_out]; returns [nvar_out, nrow_d]."""
        import torch
        T = np.ascontiguousarray(T, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        nin, ldv = _fields(torch, (dV,), self.ncol_d, "V")
        assert nin == T.shape[0] and b.shape == (T.shape[1],)
        nout = T.shape[1]
        if out is None:         # (a caller's array is taken as it comes, as ever)
            out = padded_planes(nout, self.nrow_d, dV.device)
        check(lib().ibh_weighted_apply_transformed_device(
            self._h, dV.data_ptr(), nin, ldv, ptr(T), ptr(b), nout, out.data_ptr(), plane_stride(out, self.nrow_d, "out"), float(fill),
            stream_arg(dV, stream)))
        return out

    def apply_transformed(self, V_b, T, b, fill=np.nan):
        """Host-array form of apply_transformed_device (dense index spaces)."""
        import torch
        dV = to_device(np.ascontiguousarray(np.atleast_2d(V_b), np.float64))
        out = self.apply_transformed_device(dV, T, b, fill=fill)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def apply_M(self, A_s, fill=np.nan, force_conservation=True):
        """Applies the regrid matrix to A_s (vectors in the ORIGINAL sparse space of the input grid):
        a 1-D vector or a 2-D array of row vectors; un-set output cells get `fill`
        (matrix_formats.rst:156-165)."""
        A = np.asarray(A_s, np.float64)
        one = A.ndim == 1
        A2 = A.reshape(1, -1) if one else A.reshape(A.shape[0], -1)
        if A2.shape[1] != self.sparse_extent(1):
            raise ValueError("apply_M: input has %d cells, the input grid has %d" % (A2.shape[1], self.sparse_extent(1)))
        B_d = self.apply(np.ascontiguousarray(A2[:, self.dim(1)]), fill, force_conservation)
        B_s = np.full((A2.shape[0], self.sparse_extent(0)), fill, np.float64)
        B_s[:, self.dim(0)] = B_d
        return B_s[0] if one else B_s

    def apply_weight(self, dim, A_s):
        """Dot product of a weight vector with A_s (dim 0: wM / output grid, 1: Mw / input grid)."""
        A = np.asarray(A_s, np.float64)
        one = A.ndim == 1
        A2 = A.reshape(1, -1) if one else A.reshape(A.shape[0], -1)
        if A2.shape[1] != self.sparse_extent(dim):
            raise ValueError("apply_weight: input has %d cells, expected %d" % (A2.shape[1], self.sparse_extent(dim)))
        A_d = np.ascontiguousarray(A2[:, self.dim(dim)])
        out = np.empty(A_d.shape[0], np.float64)
        check(lib().ibh_weighted_apply_weight_host(self._h, dim, ptr(A_d), A_d.shape[0], A_d.shape[1], ptr(out)))
        return out[0] if one else out

    def apply_wM(self, A_s):
        return self.apply_weight(0, A_s)

    def apply_Mw(self, A_s):
        return self.apply_weight(1, A_s)

    # ---- tuning / introspection ----------------------------------------------------------
    def set_kernel(self, name):
        check(lib().ibh_weighted_set_kernel(self._h, name.encode()))

    def set_option(self, key, value):
        """ibh_weighted_set_option: a launch option of THIS matrix (the apply-side ibh_set_tuning keys), read before the
        process-wide map; value None removes it."""
        check(lib().ibh_weighted_set_option(self._h, key.encode(), -2 ** 31 if value is None else int(value)))

    def built_fast(self):
        """True when the plan-based fast assembly path built this matrix (sorted exchange grids)."""
        v = C.c_int()
        check(lib().ibh_weighted_built_fast(self._h, C.byref(v)))
        return bool(v.value)

    def built_streamed(self):
        """True when the streamed variant of the plan-based assembly (streamasm.inl: large sorted grids) built this matrix."""
        v = C.c_int()
        check(lib().ibh_weighted_built_fast(self._h, C.byref(v)))
        return v.value in (2, 3)

    def built_sharded(self):
        """True when the ranks of a communicator shared the assembly of this matrix (ibh_regrid_matrices_matrix_d_sharded)."""
        v = C.c_int()
        check(lib().ibh_weighted_built_fast(self._h, C.byref(v)))
        return v.value == 3

    def smoothed_by(self):
        """The device form that smoothed this matrix (sigma != 0): 0 none, 1 the triplet pipeline, 2 the direct form, 3 the spatial
        tiles (ibh_weighted_smoothed_by)."""
        v = C.c_int()
        check(lib().ibh_weighted_smoothed_by(self._h, C.byref(v)))
        return v.value

    def composed_by(self):
        """How a to_modele matrix was composed: 0 not composed, 1 the generic sparse product, 2 the row-local form
        (ibh_weighted_composed_by)."""
        v = C.c_int()
        check(lib().ibh_weighted_composed_by(self._h, C.byref(v)))
        return v.value

    def last_kernel(self):
        buf = C.create_string_buffer(32)
        check(lib().ibh_weighted_last_kernel(self._h, buf, 32))
        return buf.value.decode()

    def last_launch(self):
        """The kernel instantiation of the last apply as rocprofv3 names it ("" before the first apply)."""
        buf = C.create_string_buffer(64)
        check(lib().ibh_weighted_last_launch(self._h, buf, 64))
        return buf.value.decode()


def _fields(torch, ts, n, what="A", nvar=None):
    """(nvar, ld) of the field batches ts of a device apply: torch.float64 CUDA tensors [nvar, n] with unit inner stride and one
    leading dimension (nvar None: that of the first).  The loop is here, not at the caller: one call per apply."""
    if nvar is None:
        nvar = ts[0].shape[0]
    ld = None
    for t in ts:
        assert t.is_cuda and t.dtype == torch.float64 and t.shape == (nvar, n) and t.stride(1) == 1
        if ld is None:
            s0 = t.stride(0)
            ld = leading_dim(nvar, s0, n, what)
        else:
            assert t.stride(0) == s0 or leading_dim(nvar, t.stride(0), n, what) == ld
    return nvar, ld


def _result(torch, out, nvar, n, device):
    """(out, ldb) of a device apply's result [nvar, n]: the caller's array, checked as the fields are, or padded planes on `device`."""
    if out is None:
        out = padded_planes(nvar, n, device)
    return out, _fields(torch, (out,), n, "out", nvar)[1]


def coo_multiply(M, xx, fill=np.nan, ignore_nan=False):
    """icebin.coo_multiply(M, x, fill=nan, ignore_nan=False) (coo_matvec, pylib/icebin_cython.cpp:158-192;
    tests/test_conserv/test_conserv.py:139): yy = M xx for a scipy.sparse COO matrix in the original
    (sparse) index spaces; rows with no (surviving) entry hold `fill`."""
    M = M.tocoo()
    xx = np.ascontiguousarray(xx, np.float64).reshape(-1)
    if xx.shape[0] != M.shape[1]:
        raise ValueError("coo_multiply: xx has %d elements, M has %d columns" % (xx.shape[0], M.shape[1]))
    yy = np.full(M.shape[0], fill, np.float64)
    row, col = np.ascontiguousarray(M.row, np.int32), np.ascontiguousarray(M.col, np.int32)
    data = np.ascontiguousarray(M.data, np.float64)
    check(lib().ibh_coo_matvec(ptr(yy), ptr(xx), int(bool(ignore_nan)), M.shape[0], M.shape[1], len(data), ptr(row), ptr(col),
                              ptr(data)))
    return yy


def compute_E1vE0c(XuE1s, XuE0s, nE):
    """e1ve0::compute_E1vE0c (slib/icebin/e1ve0.cpp:55-106): lists of XvE matrices (unscaled, one per ice sheet) for
    the new (E1) and the previous (E0) elevation mask -> the correction matrix as a linear_Weighted over the
    sparse E space; .to_coo() gives the reference's (iE1, iE0, value) tuples, sorted and consolidated."""
    n = len(XuE1s)
    assert n == len(XuE0s) and n >= 1
    a1 = (C.c_void_p * n)(*[w._h.value for w in XuE1s])
    a0 = (C.c_void_p * n)(*[w._h.value for w in XuE0s])
    h = C.c_void_p()
    check(lib().ibh_e1ve0_compute(n, a1, a0, int(nE), C.byref(h)))
    return linear_Weighted(h)


def nc_read_weighted(nc, vname):
    """ibmisc.nc_read_weighted (matrix_formats.rst:139-147)."""
    return linear_Weighted.nc_read(nc, vname)


def set_tuning(key, value):
    check(lib().ibh_set_tuning(key.encode(), int(value)))
