// icebin_hip.hpp -- host-side C++ mirror of IceBin's regrid-matrix interface over the C-ABI.
//
// Same class names, method names, argument order and defaults as the reference, so a caller of
//   GCMRegridder_Standard::regrid_matrices()  (slib/icebin/GCMRegridder.hpp:290-293, 369-372)
//   RegridMatrices_Dynamic::matrix_d()/matrix() (slib/icebin/RegridMatrices_Dynamic.hpp:51-59)
//   linear::Weighted_Eigen::apply()           (call sites modele/merge_topo.cpp:65, icebin22m.cpp:153)
//   modele::Hntr::regrid()                    (slib/icebin/modele/hntr.hpp:63-135; topo.cpp's lat-lon regrids)
//   modele::Hntr::overlap() / scaled_regrid_matrix() (hntr.hpp:205-338; GCMRegridder_ModelE.cpp, topo.cpp, global_ec.cpp)
// can switch to this header and link libicebin_hip.so instead of ibmisc/spsparse/Eigen.
// Differences, all forced by the absent third-party types:
//   - blitz::Array<double,N>  -> icebin::ArrayView<double> (pointer + extents, row-major, borrowed)
//     for inputs and std::vector<double> for results;
//   - Eigen matrix `M`        -> device CSR owned by the handle; host copies via M_coo();
//   - errors: (*icebin_error)(-1, ...) -> icebin::Exception (an std::runtime_error), like
//     everytrace::Exception (slib/icebin/error.hpp:28).
// Header-only; C++14.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/icebin_hip.h"
#include "ncio.hpp"

namespace icebin {

struct Exception : std::runtime_error {
    int code;
    Exception(int c, std::string const &msg) : std::runtime_error(msg), code(c) {}
};
inline void check(int rc) {
    if (rc != IBH_OK) throw Exception(rc, ibh_last_error());
}

/** Borrowed row-major view: stands in for blitz::Array<T,1> / <T,2> arguments. */
template <class T>
struct ArrayView {
    T *data;
    long extent0, extent1;     // extent1 == 1 for rank-1 views
    int rank;
    ArrayView() : data(nullptr), extent0(0), extent1(1), rank(1) {}
    ArrayView(T *p, long n) : data(p), extent0(n), extent1(1), rank(1) {}
    ArrayView(T *p, long n0, long n1) : data(p), extent0(n0), extent1(n1), rank(2) {}
    ArrayView(std::vector<typename std::remove_const<T>::type> const &v)
        : data(const_cast<T *>(v.data())), extent0((long)v.size()), extent1(1), rank(1) {}
    long size() const { return extent0 * extent1; }
};

// ---- eigen_types.hpp:16-24 -------------------------------------------------------------------
typedef long sparse_index_type;
typedef int dense_index_type;
typedef double val_type;

/** spsparse::SparseSet<long,int> (eigen_types.hpp:24). */
class SparseSetT {
    ibh_sparse_set *h_;
    SparseSetT(ibh_sparse_set *h) : h_(h) {}
public:
    SparseSetT() : h_(nullptr) { check(ibh_sparse_set_create(-1, &h_)); }
    explicit SparseSetT(long sparse_extent) : h_(nullptr) { check(ibh_sparse_set_create(sparse_extent, &h_)); }
    SparseSetT(SparseSetT const &) = delete;
    SparseSetT &operator=(SparseSetT const &) = delete;
    SparseSetT(SparseSetT &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    ~SparseSetT() { if (h_) ibh_sparse_set_destroy(h_); }
    /** ibmisc id_sparse_set<SparseSetT>(n) (modele/merge_topo.cpp:48, IceCoupler.cpp:366) */
    static SparseSetT identity(long n) { ibh_sparse_set *h; check(ibh_sparse_set_create_identity(n, &h)); return SparseSetT(h); }
    long sparse_extent() const { int64_t v; check(ibh_sparse_set_sparse_extent(h_, &v)); return (long)v; }
    int dense_extent() const { int32_t v; check(ibh_sparse_set_dense_extent(h_, &v)); return v; }
    /** The whole dense -> sparse table.  Cached on the host: a set only ever grows (add_dense, or a matrix
        build appending on the device), so the cache is refreshed when the dense extent has changed and
        to_sparse(id) is O(1) in the loop shape of IceCoupler.cpp:449-457. */
    std::vector<long> const &to_sparse_all() const {
        const int n = dense_extent();
        if ((int)cache_.size() != n) {
            std::vector<int64_t> t((size_t)n);
            check(ibh_sparse_set_to_sparse(h_, t.data()));
            cache_.assign(t.begin(), t.end());
        }
        return cache_;
    }
    long to_sparse(int id) const { return to_sparse_all().at((size_t)id); }
    /** spsparse::SparseSet::{add_dense, to_dense, in_sparse} (AbbrGrid.cpp:108, IceCoupler.cpp:298) */
    int add_dense(long sparse) { int32_t d; check(ibh_sparse_set_add_dense(h_, sparse, &d)); return d; }
    bool in_sparse(long sparse) const { int32_t d; check(ibh_sparse_set_to_dense(h_, sparse, &d)); return d >= 0; }
    int to_dense(long sparse) const {
        int32_t d; check(ibh_sparse_set_to_dense(h_, sparse, &d));
        if (d < 0) throw Exception(IBH_ENOKEY, "SparseSet: sparse index " + std::to_string(sparse) + " is not in the set");
        return d;
    }
    ibh_sparse_set *handle() const { return h_; }
    /** SparseSet::ncio (matrix_formats.rst:23-27): `int64 <vname>(<vname>.dense_extent)` with attribute `sparse_extent`.
        Reading replaces the contents of this set (it must not be in use by a matrix). */
    void ncio(NcIO &ncio, std::string const &vname) {
        if (ncio.reading()) {
            nc::Var const &v = ncio.file.var(vname);
            std::vector<int64_t> t = v.data.as<int64_t>();
            ibh_sparse_set *h = nullptr;
            check(ibh_sparse_set_from_array(v.att("sparse_extent").at<int64_t>(0), t.data(), (int32_t)t.size(), &h));
            if (h_) ibh_sparse_set_destroy(h_);
            h_ = h; cache_.clear();
        } else {
            if (ncio.file.has_var(vname)) return;            // dims shared by several matrices are written once (IceCoupler.cpp:479-487)
            std::vector<long> const &t = to_sparse_all();
            std::vector<int64_t> t64(t.begin(), t.end());
            const std::string d = ncio.file.add_dim(vname + ".dense_extent", (int64_t)t64.size());
            const int64_t ext = sparse_extent();
            ncio.file.add_var(vname, {d}, nc::Array::of(t64), {{"sparse_extent", nc::Array::of(&ext, 1)}});
            ncio.touch();
        }
    }
private:
    mutable std::vector<long> cache_;
};

// ---- RegridMatrices.hpp:17-37 ----------------------------------------------------------------
struct RegridParams {
    bool scale;
    bool correctA;
    std::array<double, 3> sigma;
    bool smooth() const { return sigma[0] != 0; }
    RegridParams() : scale(true), correctA(false), sigma({0., 0., 0.}) {}
    RegridParams(bool _scale, bool _correctA, std::array<double, 3> const &_sigma)
        : scale(_scale), correctA(_correctA), sigma(_sigma) {}
};

/** The ranks of a field-sharded regrid, one process per GPU (ibh_comm; RCCL over xGMI underneath).  Rank 0 calls
    Communicator::unique_id() and ships the 128 bytes to the others with whatever the host program has (ModelE: MPI_Bcast);
    then every rank constructs Communicator(world, rank, id) on its own device.  world == 1 needs neither id nor RCCL. */
class Communicator {
    ibh_comm *h_ = nullptr;
public:
    static std::array<char, IBH_UNIQUE_ID_BYTES> unique_id() {
        std::array<char, IBH_UNIQUE_ID_BYTES> id;
        check(ibh_comm_unique_id(id.data()));
        return id;
    }
    Communicator() { check(ibh_comm_create(1, 0, nullptr, &h_)); }
    Communicator(int world, int rank, std::array<char, IBH_UNIQUE_ID_BYTES> const &id) { check(ibh_comm_create(world, rank, id.data(), &h_)); }
    Communicator(int world, int rank, ibh_exchange_fn fn, void *user) { check(ibh_comm_create_custom(world, rank, fn, user, &h_)); }
    Communicator(Communicator const &) = delete;
    Communicator &operator=(Communicator const &) = delete;
    ~Communicator() { if (h_) ibh_comm_destroy(h_); }
    int world() const { int w; check(ibh_comm_info(h_, &w, nullptr)); return w; }
    int rank() const { int r; check(ibh_comm_info(h_, nullptr, &r)); return r; }
    /** make `stream` wait for the exchanges enqueued so far: the gathered results are complete behind it */
    void wait(void *stream) const { check(ibh_comm_wait(h_, stream)); }
    /** run the exchanges on the caller's stream (which outlives this object and is never destroyed by it) */
    void set_stream(void *stream) { check(ibh_comm_set_stream(h_, stream)); }
    /** "planes_padded": the gap between nrow_d and ldb of the result planes is padding the caller owns */
    void set_option(const char *key, int value) { check(ibh_comm_set_option(h_, key, value)); }
    ibh_comm *handle() const { return h_; }
};

namespace linear {
/** ibmisc::linear::Weighted / Weighted_Eigen: M plus wM, Mw, dims, conservative, scaled. */
class Weighted {
    ibh_weighted *h_;
    mutable std::vector<double> wM_, Mw_;
    mutable bool have_wM_ = false, have_Mw_ = false;
    bool file_dims_ = false;                       // loaded by ncio(): the dims are those of the file (the handle's are identities)
    std::array<std::vector<long>, 2> file_dim_;
    std::array<long, 2> file_extent_ = {{0, 0}};
public:
    bool conservative = true, scaled = true;
    /** an empty matrix, to be filled by ncio() from a file */
    Weighted() : h_(nullptr) {}
    explicit Weighted(ibh_weighted *h) : h_(h) {
        int c, s;
        check(ibh_weighted_flags(h, &c, &s));
        conservative = c != 0; scaled = s != 0;
    }
    Weighted(Weighted const &) = delete;
    Weighted &operator=(Weighted const &) = delete;
    virtual ~Weighted() { if (h_) ibh_weighted_destroy(h_); }
    ibh_weighted *handle() const { return h_; }

    /** Dense shape {nrow_d, ncol_d} and number of stored entries. */
    std::array<int, 2> shape_d() const { int32_t r, c; check(ibh_weighted_shape(h_, &r, &c, nullptr)); return {{r, c}}; }
    long nnz() const { int64_t n; check(ibh_weighted_shape(h_, nullptr, nullptr, &n)); return (long)n; }
    /** Sparse shape (dims[k]->sparse_extent()). */
    std::array<long, 2> shape() const {
        if (file_dims_) return {{file_extent_[0], file_extent_[1]}};
        int64_t a, b;
        check(ibh_weighted_dim(h_, 0, &a, nullptr)); check(ibh_weighted_dim(h_, 1, &b, nullptr));
        return {{(long)a, (long)b}};
    }
    /** dims[k]->to_sparse(j) for all j */
    std::vector<long> dim_to_sparse(int k) const {
        if (file_dims_) return file_dim_[(size_t)k];
        std::vector<int64_t> t((size_t)shape_d()[(size_t)k]);
        check(ibh_weighted_dim_to_sparse(h_, k, t.data()));
        return std::vector<long>(t.begin(), t.end());
    }
    /** Weighted_Eigen::ncio(ncio, vname, {dimB, dimA}) (modele/global_ec.cpp:571-605, IceCoupler.cpp:473-488): the "Eigen
        format" of sphinx/source/matrix_formats.rst:9-63 -- the dims under their own names (written once when several matrices
        share them), `<v>.info` {type "EIGEN", conservative, scaled, dim_names}, `<v>.M.info` {shape, conservative},
        `<v>.M.indices(nnz, rank)`, `<v>.M.values`, `<v>.Mw`, `<v>.wM`.  With a reading NcIO the matrix is LOADED from the file
        (to_eigen_M, eigen_types.cpp:9-34: ibh_weighted_from_coo) and keeps the file's dims. */
    void ncio(NcIO &ncio, std::string const &vname, std::array<std::string, 2> const &dim_names = {{"", ""}}) {
        if (ncio.reading()) {
            nc::File const &f = ncio.file;
            nc::Var const &info = f.var(vname + ".info");
            if (nc::find(info.attrs, "type") && info.att("type").str() != "EIGEN")
                throw Exception(IBH_ENOTIMPL, vname + ": matrix type '" + info.att("type").str() + "' is not the Eigen format");
            std::vector<std::string> names = nc::split_names(info.att("dim_names").str());
            if (names.size() != 2) throw Exception(IBH_EINVAL, vname + ".info:dim_names must name two dims");
            for (int k = 0; k < 2; ++k) {
                std::string n = names[(size_t)k];
                if (n.compare(0, vname.size() + 1, vname + ".") == 0) n = n.substr(vname.size() + 1);
                nc::Var const &d = f.var(n);
                std::vector<int64_t> t = d.data.as<int64_t>();
                file_dim_[(size_t)k].assign(t.begin(), t.end());
                file_extent_[(size_t)k] = (long)d.att("sparse_extent").at<int64_t>(0);
            }
            std::vector<int32_t> ind = f.var(vname + ".M.indices").data.as<int32_t>();
            std::vector<double> val = f.var(vname + ".M.values").data.as<double>();
            std::vector<double> wMv = f.var(vname + ".wM").data.as<double>(), Mwv = f.var(vname + ".Mw").data.as<double>();
            std::vector<int32_t> row(val.size()), col(val.size());
            for (size_t e = 0; e < val.size(); ++e) { row[e] = ind[2 * e]; col[e] = ind[2 * e + 1]; }
            const int cons = nc::find(info.attrs, "conservative") ? info.att("conservative").at<int>(0) : 1;
            const int sc = nc::find(info.attrs, "scaled") ? info.att("scaled").at<int>(0) : 1;
            ibh_weighted *h = nullptr;
            check(ibh_weighted_from_coo((int32_t)wMv.size(), (int32_t)Mwv.size(), (int64_t)val.size(), row.data(), col.data(), val.data(),
                                        wMv.data(), Mwv.data(), cons, sc, &h));
            if (h_) ibh_weighted_destroy(h_);
            h_ = h; conservative = cons != 0; scaled = sc != 0; file_dims_ = true; have_wM_ = have_Mw_ = false;
            return;
        }
        if (dim_names[0].empty() || dim_names[1].empty()) throw Exception(IBH_EINVAL, "Weighted::ncio: writing needs the two dim names");
        nc::File &f = ncio.file;
        std::array<std::string, 2> dnames;
        for (int k = 0; k < 2; ++k) {
            std::vector<long> t = dim_to_sparse(k);
            std::vector<int64_t> t64(t.begin(), t.end());
            dnames[(size_t)k] = f.add_dim(dim_names[(size_t)k] + ".dense_extent", (int64_t)t64.size());
            if (!f.has_var(dim_names[(size_t)k])) {
                const int64_t ext = shape()[(size_t)k];
                f.add_var(dim_names[(size_t)k], {dnames[(size_t)k]}, nc::Array::of(t64), {{"sparse_extent", nc::Array::of(&ext, 1)}});
            }
        }
        std::vector<int> row, col; std::vector<double> val;
        M_coo(row, col, val);
        const int32_t zero32 = 0, cons = conservative ? 1 : 0, sc = scaled ? 1 : 0;
        const int64_t zero64 = 0;
        f.add_var(vname + ".info", {}, nc::Array::of(&zero32, 1),
                  {{"type", nc::Array::str("EIGEN")}, {"conservative", nc::Array::of(&cons, 1)}, {"scaled", nc::Array::of(&sc, 1)},
                   {"dim_names", nc::Array::str(vname + "." + dim_names[0] + "," + vname + "." + dim_names[1])}});
        const int64_t shp[2] = {(int64_t)shape_d()[0], (int64_t)shape_d()[1]};
        f.add_var(vname + ".M.info", {}, nc::Array::of(&zero64, 1),
                  {{"shape", nc::Array::of(shp, 2)}, {"conservative", nc::Array::str(conservative ? "t" : "f")}});
        const std::string dn = f.add_dim(vname + ".M.nnz", (int64_t)val.size()), dr = f.add_dim(vname + ".M.rank", 2);
        std::vector<int32_t> ind(2 * val.size());
        for (size_t e = 0; e < val.size(); ++e) { ind[2 * e] = row[e]; ind[2 * e + 1] = col[e]; }
        f.add_var(vname + ".M.indices", {dn, dr}, nc::Array::of(ind));
        f.add_var(vname + ".M.values", {dn}, nc::Array::of(val));
        f.add_var(vname + ".Mw", {dnames[1]}, nc::Array::of(Mw()));
        f.add_var(vname + ".wM", {dnames[0]}, nc::Array::of(wM()));
        ncio.touch();
    }
    /** wM / Mw: host mirrors, downloaded once (the matrix is immutable after its build); wM(jj) as at
        IceCoupler.cpp:456. */
    std::vector<double> const &wM() const {
        if (!have_wM_) { wM_.resize((size_t)shape_d()[0]); check(ibh_weighted_get_wM(h_, wM_.data())); have_wM_ = true; }
        return wM_;
    }
    std::vector<double> const &Mw() const {
        if (!have_Mw_) { Mw_.resize((size_t)shape_d()[1]); check(ibh_weighted_get_Mw(h_, Mw_.data())); have_Mw_ = true; }
        return Mw_;
    }
    double wM(int jj) const { return wM().at((size_t)jj); }
    double Mw(int jj) const { return Mw().at((size_t)jj); }
    /** ->M as row-major COO in dense index space */
    void M_coo(std::vector<int> &row, std::vector<int> &col, std::vector<double> &val) const {
        size_t n = (size_t)nnz();
        row.resize(n); col.resize(n); val.resize(n);
        check(ibh_weighted_get_coo(h_, row.data(), col.data(), val.data()));
    }
    /** The `M` member callers poke (IceCoupler.cpp:408 iterates its entries, :445 multiplies with it): the
        matrix lives in HBM; this view gives its shape and, on demand, a host copy of the triplets. */
    struct MatrixView {
        Weighted const *w;
        int rows() const { return w->shape_d()[0]; }
        int cols() const { return w->shape_d()[1]; }
        long nonZeros() const { return w->nnz(); }
        struct Triplet { int row, col; double value; };
        std::vector<Triplet> triplets() const {
            std::vector<int> r, c; std::vector<double> v;
            w->M_coo(r, c, v);
            std::vector<Triplet> t(v.size());
            for (size_t k = 0; k < v.size(); ++k) t[k] = Triplet{r[k], c[k], v[k]};
            return t;
        }
    };
    MatrixView M{this};
    /** `tmp`: objects that must live as long as the matrix (RegridMatrices_Dynamic::matrix hands the dims it
        allocated to M->tmp, RegridMatrices_Dynamic.cpp:429-436). */
    std::vector<std::shared_ptr<void>> tmp;

    /** apply(A_b, fill, force_conservation, tmp): A_b is (nvar, ncol_d) or a rank-1 vector of
        ncol_d values; returns (nvar, nrow_d) row-major.  The reference's TmpAlloc argument owned
        the result; here the returned vector does. */
    std::vector<double> apply(ArrayView<const double> const &A_b, double fill = std::nan(""),
                              bool force_conservation = true) const {
        auto sh = shape_d();
        long nvar = A_b.rank == 1 ? 1 : A_b.extent0;
        long ncol = A_b.rank == 1 ? A_b.extent0 : A_b.extent1;
        if (ncol != sh[1]) throw Exception(IBH_EINVAL, "apply: input has " + std::to_string(ncol) +
                                                        " columns, matrix has " + std::to_string(sh[1]));
        std::vector<double> B((size_t)(nvar * sh[0]));
        check(ibh_weighted_apply_host(h_, A_b.data, (int32_t)nvar, ncol, B.data(), sh[0], fill, force_conservation ? 1 : 0));
        return B;
    }
    /** The coupler's fused product B = M * (A*T + b) (IceCoupler.cpp:203-252, :445) on HBM-resident
        fields: T is the (sparse) variable transform as a dense row-major nvar_in x nvar_out host array
        (exact zeros are structural), b the offsets. */
    void apply_transformed_device(const double *dA_b, int nvar_in, long lda, std::vector<double> const &T,
                                  std::vector<double> const &b, double *dB_b, long ldb, double fill, void *stream) const {
        check(ibh_weighted_apply_transformed_device(h_, dA_b, nvar_in, lda, T.data(), b.data(), (int32_t)b.size(),
                                                    dB_b, ldb, fill, stream));
    }
    /** Several field batches through one launch (ibh_weighted_apply_many_device): dA_b[q] -> dB_b[q], all nvar x lda / ldb. */
    void apply_many_device(std::vector<const double *> const &dA_b, int nvar, long lda, std::vector<double *> const &dB_b,
                           long ldb, double fill, bool force_conservation, void *stream) const {
        if (dA_b.size() != dB_b.size()) throw Exception(IBH_EINVAL, "apply_many_device: batch lists differ in length");
        check(ibh_weighted_apply_many_device(h_, (int32_t)dA_b.size(), dA_b.data(), nvar, lda, dB_b.data(), ldb, fill,
                                             force_conservation ? 1 : 0, stream));
    }
    /** The legacy COO product with its fill / ignore-NaN contract (coo_matvec, pylib/icebin_cython.cpp:158-192) on device arrays. */
    void matvec_device(const double *dxx, int nvar, long ldx, double *dyy, long ldy, bool ignore_nan, void *stream) const {
        check(ibh_weighted_matvec_device(h_, dxx, nvar, ldx, dyy, ldy, ignore_nan ? 1 : 0, stream));
    }
    /** Build now whatever apply structure (column sweep / bands) applies of up to nvar variables, nbatch batches per
        launch, would build lazily on their second call, and size all per-apply scratch: afterwards the device applies
        only enqueue work (ibh_weighted_prepare).  Once per matrix, e.g. right after matrix_d() in a coupler that
        applies the matrix more than once per step, and before capturing applies into a hipGraph. */
    void prepare(int nvar, int nbatch = 1) const { check(ibh_weighted_prepare(h_, nvar, nbatch)); }
    /** A launch option of THIS matrix (ibh_weighted_set_option): read before the process-wide ibh_set_tuning map. */
    void set_option(std::string const &key, int value) { check(ibh_weighted_set_option(h_, key.c_str(), value)); }
    /** Fused pair B1 = (*this) * A, B2 = second * B1 in one launch (EvI then AvE; ibh_weighted_pair_prepare /
        ibh_weighted_apply_pair_device).  pair_prepare throws Exception(IBH_ENOTIMPL) when the matrices do not pair: make the two
        apply() calls of the reference then. */
    void pair_prepare(Weighted const &second, int nvar = 16) const { check(ibh_weighted_pair_prepare(h_, second.h_, nvar)); }
    void apply_pair_device(Weighted const &second, const double *dA_b, int nvar, long lda, double *dB1_b, long ldb1, double *dB2_b,
                           long ldb2, double fill, void *stream) const {
        check(ibh_weighted_apply_pair_device(h_, second.h_, dA_b, nvar, lda, dB1_b, ldb1, dB2_b, ldb2, fill, stream));
    }
    /** the chain of BASELINE config 3 (EvI, AvE, IvA): the fused pair, then `third` on its result, the third product's launch
        overlapped with the pair kernel (ibh_weighted_apply_chain_device); bitwise the pair apply followed by third.apply_device */
    void apply_chain_device(Weighted const &second, Weighted const &third, const double *dA_b, int nvar, long lda, double *dB1_b, long ldb1,
                            double *dB2_b, long ldb2, double *dB3_b, long ldb3, double fill = std::nan(""), void *stream = nullptr) const {
        check(ibh_weighted_apply_chain_device(h_, second.h_, third.h_, dA_b, nvar, lda, dB1_b, ldb1, dB2_b, ldb2, dB3_b, ldb3, fill, stream));
    }
    /** apply() of world x nvar_local fields sharded by field over the ranks of `comm`: this rank's dA_local (nvar_local x lda)
        -> dB_all (world*nvar_local x ldb, the same on every rank once comm.wait(stream) has been honoured).  The SpMM runs on
        `stream`, the peer-to-peer exchange on the communicator's own stream, block_fields fields at a time (0: by size). */
    void apply_sharded_device(Communicator const &comm, const double *dA_local, int nvar_local, long lda, double *dB_all, long ldb,
                              double fill, void *stream, int block_fields = 0) const {
        check(ibh_weighted_apply_sharded_device(h_, comm.handle(), dA_local, nvar_local, lda, dB_all, ldb, fill, block_fields, stream));
    }
    /** the same with apply_device's force_conservation: each rank corrects its own fields before they travel
        (ibh_weighted_apply_sharded_conserve_device; a conservative matrix ignores the flag) */
    void apply_sharded_device(Communicator const &comm, const double *dA_local, int nvar_local, long lda, double *dB_all, long ldb,
                              double fill, bool force_conservation, void *stream, int block_fields = 0) const {
        check(ibh_weighted_apply_sharded_conserve_device(h_, comm.handle(), dA_local, nvar_local, lda, dB_all, ldb, fill,
                                                         force_conservation ? 1 : 0, block_fields, stream));
    }
    /** several field batches: ONE SpMM launch, ONE grouped exchange (ibh_weighted_apply_many_sharded_device) */
    void apply_many_sharded_device(Communicator const &comm, std::vector<const double *> const &dA_local, int nvar_local, long lda,
                                   std::vector<double *> const &dB_all, long ldb, double fill, void *stream) const {
        if (dA_local.size() != dB_all.size()) throw Exception(IBH_EINVAL, "apply_many_sharded_device: batch lists differ in length");
        check(ibh_weighted_apply_many_sharded_device(h_, comm.handle(), (int32_t)dA_local.size(), dA_local.data(), nvar_local, lda,
                                                     dB_all.data(), ldb, fill, stream));
    }
    /** ... with force_conservation (ibh_weighted_apply_many_sharded_conserve_device) */
    void apply_many_sharded_device(Communicator const &comm, std::vector<const double *> const &dA_local, int nvar_local, long lda,
                                   std::vector<double *> const &dB_all, long ldb, double fill, bool force_conservation, void *stream) const {
        if (dA_local.size() != dB_all.size()) throw Exception(IBH_EINVAL, "apply_many_sharded_device: batch lists differ in length");
        check(ibh_weighted_apply_many_sharded_conserve_device(h_, comm.handle(), (int32_t)dA_local.size(), dA_local.data(), nvar_local,
                                                              lda, dB_all.data(), ldb, fill, force_conservation ? 1 : 0, stream));
    }
    /** Device-resident variant: dA_b (nvar x lda) and dB_b (nvar x ldb) are HBM pointers; enqueues on stream. */
    void apply_device(const double *dA_b, int nvar, long lda, double *dB_b, long ldb, double fill,
                      bool force_conservation, void *stream) const {
        check(ibh_weighted_apply_device(h_, dA_b, nvar, lda, dB_b, ldb, fill, force_conservation ? 1 : 0, stream));
    }
};
typedef Weighted Weighted_Eigen;      // the concrete type callers name (RegridMatrices_Dynamic.hpp:27)
}   // namespace linear

// ---- multivec.hpp:16-71 ----------------------------------------------------------------------
/** icebin::VectorMultivec, resident in HBM (ibh_multivec).  index / weights / vals are read back on demand; the members
    with the reference's names take host arrays like its blitz arrays, the *_device ones take HBM pointers and a stream. */
class VectorMultivec {
    ibh_multivec *h_;
    explicit VectorMultivec(ibh_multivec *h) : h_(h) {}
    friend VectorMultivec concatenate(std::vector<VectorMultivec const *> const &vecs);
public:
    explicit VectorMultivec(int _nvar) : h_(nullptr) { check(ibh_multivec_create(_nvar, &h_)); }
    VectorMultivec(VectorMultivec const &) = delete;
    VectorMultivec &operator=(VectorMultivec const &) = delete;
    VectorMultivec(VectorMultivec &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    ~VectorMultivec() { if (h_) ibh_multivec_destroy(h_); }
    ibh_multivec *handle() const { return h_; }

    int nvar() const { int32_t v; check(ibh_multivec_size(h_, nullptr, &v)); return v; }
    size_t size() const { int64_t n; check(ibh_multivec_size(h_, &n, nullptr)); return (size_t)n; }
    void clear() { check(ibh_multivec_clear(h_)); }
    void reserve(size_t n) { check(ibh_multivec_reserve(h_, (int64_t)n)); }

    /** add(ix, val, weight) (multivec.cpp:8-13); the array form adds n entries with one copy. */
    void add(long ix, double const *val, double weight) { int64_t i = ix; check(ibh_multivec_add_host(h_, 1, &i, &weight, val)); }
    void add(long ix, std::vector<double> const &val, double weight) { add(ix, val.data(), weight); }
    void add(size_t n, int64_t const *ix, double const *weight, double const *val) { check(ibh_multivec_add_host(h_, (int64_t)n, ix, weight, val)); }

    std::vector<long> index() const {
        std::vector<int64_t> t(size());
        check(ibh_multivec_get(h_, t.data(), nullptr, nullptr));
        return std::vector<long>(t.begin(), t.end());
    }
    std::vector<double> weights() const { std::vector<double> t(size()); check(ibh_multivec_get(h_, nullptr, t.data(), nullptr)); return t; }
    std::vector<double> vals() const { std::vector<double> t(size() * (size_t)nvar()); check(ibh_multivec_get(h_, nullptr, nullptr, t.data())); return t; }
    /** val(varix, ix) (multivec.hpp:55-56); reads the values back: for a loop, take vals() once. */
    double val(int varix, long ix) const { return vals().at((size_t)ix * (size_t)nvar() + (size_t)varix); }

    /** "Sparsify while appending" (IceCoupler.cpp:447-458) from the field-major product of M: host array / HBM pointer. */
    void append_weighted(linear::Weighted const &M, double const *B_b, int nvar_, long ldb) {
        check(ibh_multivec_append_weighted_host(h_, M.handle(), B_b, nvar_, ldb));
    }
    void append_weighted_device(linear::Weighted const &M, double const *dB_b, int nvar_, long ldb, void *stream) {
        check(ibh_multivec_append_weighted_device(h_, M.handle(), dB_b, nvar_, ldb, stream));
    }
    void append(VectorMultivec const &other) { check(ibh_multivec_append(h_, other.h_)); }
    /** update_topo's packing (modele/GCMCoupler_ModelE.cpp:1099-1164; ibh_multivec_append_planes_host): for ihc < nclass (outer)
        and every cell c ascending with mask[c] != 0 || (mask0 && mask0[c] != 0) one entry (c * index_stride_cell + ihc *
        index_stride_class, planes[k][ihc * plane_class_stride + c] for every k, weight 1.0).  planes: nvar() host arrays; types:
        0 double / 1 int16 per plane, empty: all double.  Returns the kept cells.  The _device form takes device planes and masks. */
    long append_planes(std::vector<const void *> const &planes, std::vector<int32_t> const &types, long ncell, int nclass,
                       long plane_class_stride, const int16_t *mask, const int16_t *mask0, long index_stride_cell, long index_stride_class) {
        int64_t nkept = 0;
        check(ibh_multivec_append_planes_host(h_, planes.data(), plane_types(planes, types), (int32_t)planes.size(), ncell, nclass,
                                              plane_class_stride, mask, mask0, index_stride_cell, index_stride_class, &nkept));
        return (long)nkept;
    }
    long append_planes_device(std::vector<const void *> const &d_planes, std::vector<int32_t> const &types, long ncell, int nclass,
                              long plane_class_stride, const int16_t *d_mask, const int16_t *d_mask0, long index_stride_cell,
                              long index_stride_class, void *stream) {
        int64_t nkept = 0;
        check(ibh_multivec_append_planes_device(h_, d_planes.data(), plane_types(d_planes, types), (int32_t)d_planes.size(), ncell, nclass,
                                                plane_class_stride, d_mask, d_mask0, index_stride_cell, index_stride_class, &nkept, stream));
        return (long)nkept;
    }
    /** couple()'s unit conversion (modele/GCMCoupler_ModelE.cpp:1216-1228) over every entry: val = val * mm[ivar] + bb[ivar], a
        product then an add.  Enqueued on `stream`. */
    void affine(std::vector<double> const &mm, std::vector<double> const &bb, void *stream = nullptr) {
        if ((int)mm.size() != nvar() || (int)bb.size() != nvar())
            throw Exception(IBH_EINVAL, "affine: " + std::to_string(mm.size()) + " mm and " + std::to_string(bb.size()) + " bb for nvar=" +
                                            std::to_string(nvar()));
        check(ibh_multivec_affine_device(h_, mm.data(), bb.data(), stream));
    }
private:
    static const int32_t *plane_types(std::vector<const void *> const &planes, std::vector<int32_t> const &types) {
        if (types.empty()) return nullptr;
        if (types.size() != planes.size())
            throw Exception(IBH_EINVAL, "append_planes: " + std::to_string(types.size()) + " types for " + std::to_string(planes.size()) + " planes");
        return types.data();
    }
public:

    /** to_dense_scale(scaleE) (multivec.cpp:35-50): scaleE's length is nE. */
    void to_dense_scale(std::vector<double> &scaleE) const { check(ibh_multivec_to_dense_scale_host(h_, (int64_t)scaleE.size(), scaleE.data())); }
    void to_dense_scale_device(long nE, double *d_scale, void *stream) const { check(ibh_multivec_to_dense_scale(h_, nE, d_scale, stream)); }
    /** to_dense (multivec.cpp:55-81), all variables at once: [nvar x nE] field-major; and the reference's one-variable form,
        which computes them all and keeps one. */
    std::vector<double> to_dense(std::vector<double> const &scaleE, double fill) const {
        std::vector<double> out((size_t)nvar() * scaleE.size());
        check(ibh_multivec_to_dense_host(h_, scaleE.data(), fill, out.data(), (int64_t)scaleE.size(), (int64_t)scaleE.size()));
        return out;
    }
    void to_dense(int ivar, std::vector<double> const &scaleE, double fill, std::vector<double> &denseE) const {
        if (denseE.size() != scaleE.size()) throw Exception(IBH_EINVAL, "to_dense: denseE and scaleE differ in length");
        if (ivar < 0 || ivar >= nvar()) throw Exception(IBH_EINVAL, "to_dense: no variable " + std::to_string(ivar));
        std::vector<double> all = to_dense(scaleE, fill);
        std::copy(all.begin() + (long)ivar * (long)scaleE.size(), all.begin() + ((long)ivar + 1) * (long)scaleE.size(), denseE.begin());
    }
    void to_dense_device(double const *d_scale, double fill, double *d_out, long ld, long nE, void *stream) const {
        check(ibh_multivec_to_dense(h_, d_scale, fill, d_out, ld, nE, stream));
    }
    /** The in-place merge into the GCM's arrays (modele/GCMCoupler_ModelE.cpp:864-892), HBM pointers. */
    void update_dense(double const *d_scale, double *d_out, long ld, long nE, void *stream) const {
        check(ibh_multivec_update_dense(h_, d_scale, d_out, ld, nE, stream));
    }
    /** dimE0->add_dense of every index in entry order (IceCoupler.cpp:294-300), then the densified array (:306-314), HBM pointer. */
    void add_dense_to(SparseSetT &dim, void *stream = nullptr) const { check(ibh_sparse_set_add_dense_multivec(dim.handle(), h_, stream)); }
    void densify(SparseSetT const &dim, double *d_out, long ld, void *stream) const {
        check(ibh_multivec_densify_device(h_, dim.handle(), d_out, ld, stream));
    }
};
/** concatenate (multivec.cpp:15-33). */
inline VectorMultivec concatenate(std::vector<VectorMultivec const *> const &vecs) {
    std::vector<ibh_multivec const *> hs;
    for (VectorMultivec const *v : vecs) hs.push_back(v->handle());
    ibh_multivec *h = nullptr;
    check(ibh_multivec_concatenate((int32_t)hs.size(), hs.data(), &h));
    return VectorMultivec(h);
}

// ---- AbbrGrid.hpp:40-89 ----------------------------------------------------------------------
class ExchangeGrid {
public:
    std::vector<int> indices;       // Length*2: (ixA, ixI)
    std::vector<double> overlaps;
    void reserve(size_t n) { indices.reserve(n * 2); overlaps.reserve(n); }
    void add(std::array<int, 2> const &index, double _area) {
        indices.push_back(index[0]); indices.push_back(index[1]); overlaps.push_back(_area);
    }
    int dense_extent() const { return (int)overlaps.size(); }
    long sparse_extent() const { return (long)overlaps.size(); }
    long to_sparse(int id) const { return id; }
    int ijk(int id, int index) const { return indices[(size_t)id * 2 + (size_t)index]; }
    double native_area(int id) const { return overlaps[(size_t)id]; }
};

/** The parts of AbbrGrid (AbbrGrid.hpp:93-109) the regrid path reads. */
struct AbbrGrid {
    long sparse_extent = 0;             // dim.sparse_extent()
    std::vector<long> dim_to_sparse;    // dim: dense -> sparse
    std::vector<double> native_area;    // dense indexing
    std::string name, sproj;
};

struct InterpStyle { enum { Z_INTERP = 0, ELEV_CLASS_INTERP = 1 }; };    // IceRegridder.hpp:36-39

class GCMRegridder_Standard;
class RegridMatrices_Dynamic;

/** IceRegridder / IceRegridder_L0 (IceRegridder.hpp:46-133): one ice sheet. */
class IceRegridder {
    friend class GCMRegridder_Standard;
    ibh_regridder *h_ = nullptr;
    std::string _name;
    long _nI = 0, _nX = 0;
    // host copies of what ncio() writes (IceRegridder::ncio, IceRegridder.cpp:75-90); drop_host_copy() releases them
    ExchangeGrid aexgrid_;
    std::vector<double> gridA_proj_area_, gridI_centroid_xy_;
public:
    int interp_style = InterpStyle::Z_INTERP;
    void drop_host_copy() { aexgrid_ = ExchangeGrid(); gridA_proj_area_.clear(); gridI_centroid_xy_.clear(); gridA_proj_area_.shrink_to_fit(); }
    ~IceRegridder() { if (h_) ibh_regridder_destroy(h_); }
    std::string const &name() const { return _name; }
    size_t nI() const { return (size_t)_nI; }
    size_t nX() const { return (size_t)_nX; }
    ibh_regridder *handle() const { return h_; }
};

// ---- RegridMatrices.hpp:39-62 ----------------------------------------------------------------
class RegridMatrices {
    RegridParams _params;
public:
    RegridMatrices(RegridParams const &params) : _params(params) {}
    virtual ~RegridMatrices() {}
    RegridParams const &params() const { return _params; }
    virtual std::unique_ptr<linear::Weighted> matrix(std::string const &spec_name) const = 0;
};

// ---- RegridMatrices_Dynamic.hpp:20-59 --------------------------------------------------------
class RegridMatrices_Dynamic : public RegridMatrices {
    ibh_regrid_matrices *h_;
public:
    IceRegridder const *ice_regridder;
    RegridMatrices_Dynamic(IceRegridder const *_ice_regridder, ibh_regrid_matrices *h, RegridParams const &params)
        : RegridMatrices(params), h_(h), ice_regridder(_ice_regridder) {}
    ~RegridMatrices_Dynamic() { if (h_) ibh_regrid_matrices_destroy(h_); }
    ibh_regrid_matrices *handle() const { return h_; }

    /** matrix_d(spec_name, dims, params): ignores this->params() (RegridMatrices_Dynamic.hpp:51-54).
        dims may be pre-populated and are appended to; they must outlive the result. */
    std::unique_ptr<linear::Weighted_Eigen> matrix_d(std::string const &spec_name,
                                                     std::array<SparseSetT *, 2> dims,
                                                     RegridParams const &params) const {
        ibh_weighted *w = nullptr;
        check(ibh_regrid_matrices_matrix_d(h_, spec_name.c_str(), dims[0] ? dims[0]->handle() : nullptr,
                                           dims[1] ? dims[1]->handle() : nullptr, params.scale, params.correctA,
                                           params.sigma.data(), &w));
        return std::unique_ptr<linear::Weighted_Eigen>(new linear::Weighted_Eigen(w));
    }
    /** matrix_d with the ASSEMBLY shared by the ranks of `comm` (ibh_regrid_matrices_matrix_d_sharded): collective -- every rank
        makes the same call -- and every rank receives the whole matrix, bitwise what matrix_d builds, smoothed by params.sigma
        (IvA / IvE; ibh_regrid_matrices_matrix_d_sharded_sigma: the smoothing's spatial-tile form is shared too). */
    std::unique_ptr<linear::Weighted_Eigen> matrix_d_sharded(Communicator const &comm, std::string const &spec_name,
                                                             std::array<SparseSetT *, 2> dims, RegridParams const &params) const {
        ibh_weighted *w = nullptr;
        check(ibh_regrid_matrices_matrix_d_sharded_sigma(h_, comm.handle(), spec_name.c_str(), dims[0] ? dims[0]->handle() : nullptr,
                                                         dims[1] ? dims[1]->handle() : nullptr, params.scale, params.correctA,
                                                         params.sigma.data(), &w));
        return std::unique_ptr<linear::Weighted_Eigen>(new linear::Weighted_Eigen(w));
    }
    /** The matrices of one coupling step in one call (IceCoupler.cpp:361-468 builds EvI, AvI, IvE, XvE every step): the
        results of matrix_d(specs[k], dims[k], params[k]) in order; independent builds run concurrently in the library. */
    std::vector<std::unique_ptr<linear::Weighted_Eigen>> matrix_batch(std::vector<std::string> const &specs,
                                                                       std::vector<std::array<SparseSetT *, 2>> const &dims,
                                                                       std::vector<RegridParams> const &params) const {
        const size_t n = specs.size();
        if (dims.size() != n || params.size() != n) throw Exception(IBH_EINVAL, "matrix_batch: argument lists differ in length");
        std::vector<const char *> names(n);
        std::vector<ibh_sparse_set *> d0(n), d1(n);
        std::vector<int32_t> sc(n), ca(n);
        const double *sigma = nullptr;
        for (size_t k = 0; k < n; ++k) {
            names[k] = specs[k].c_str();
            d0[k] = dims[k][0] ? dims[k][0]->handle() : nullptr;
            d1[k] = dims[k][1] ? dims[k][1]->handle() : nullptr;
            sc[k] = params[k].scale; ca[k] = params[k].correctA;
            if (params[k].smooth()) sigma = params[k].sigma.data();      // one sigma per batch
        }
        std::vector<ibh_weighted *> w(n, nullptr);
        check(ibh_regrid_matrices_matrix_batch(h_, (int32_t)n, names.data(), d0.data(), d1.data(), sc.data(), ca.data(), sigma, w.data()));
        std::vector<std::unique_ptr<linear::Weighted_Eigen>> out;
        for (size_t k = 0; k < n; ++k) out.emplace_back(new linear::Weighted_Eigen(w[k]));
        return out;
    }
    /** Produces its own dims (RegridMatrices_Dynamic.cpp:425-437). */
    std::unique_ptr<linear::Weighted> matrix(std::string const &spec_name) const override {
        ibh_weighted *w = nullptr;
        check(ibh_regrid_matrices_matrix(h_, spec_name.c_str(), &w));
        return std::unique_ptr<linear::Weighted>(new linear::Weighted(w));
    }
};

// ---- GCMRegridder.hpp:207-399 ----------------------------------------------------------------
class GCMRegridder_Standard {
    AbbrGrid agridA_;
    std::vector<double> _hcdefs;
    long hc_stride_A_ = 1, hc_stride_HC_ = 0;
    std::vector<std::unique_ptr<IceRegridder>> sheets_;
    std::map<std::string, size_t> sheets_index_;
public:
    bool correctA = false;
    AbbrGrid const *agridA = nullptr;

    /** init(agridA, hcdefs, indexingHC, correctA) (GCMRegridder.cpp:65-86).  indexingHC is given by its
        two strides: iE = iA*stride_A + ihc*stride_HC; the Cython-built default is {1, nA}
        (icebin_cython.cpp:69). */
    void init(AbbrGrid &&_agridA, std::vector<double> &&hcdefs, std::array<long, 2> indexingHC_strides, bool _correctA) {
        agridA_ = std::move(_agridA);
        agridA = &agridA_;
        _hcdefs = std::move(hcdefs);
        hc_stride_A_ = indexingHC_strides[0]; hc_stride_HC_ = indexingHC_strides[1];
        correctA = _correctA;
    }
    void init(AbbrGrid &&_agridA, std::vector<double> &&hcdefs, bool _correctA) {
        long nA_ = _agridA.sparse_extent;
        init(std::move(_agridA), std::move(hcdefs), {{1, nA_}}, _correctA);
    }
    std::vector<double> const &hcdefs() const { return _hcdefs; }
    unsigned int nhc() const { return (unsigned int)_hcdefs.size(); }
    unsigned long nA() const { return (unsigned long)agridA_.sparse_extent; }
    unsigned long nE() const { return nA() * nhc(); }                      // GCMRegridder.hpp:273
    size_t nI(int sheet_index) const { return sheets_.at((size_t)sheet_index)->nI(); }

    /** add_sheet(name, regridder) + IceRegridder::init (GCMRegridder.hpp:353-367, IceRegridder.cpp:93-119):
        the ice grid is given by its size, the exchange grid by value; gridA_proj_area (dense, like
        agridA.native_area) may be empty = no projection (IceRegridder.cpp:106-108). */
    size_t add_sheet(std::string const &name, long nI, ExchangeGrid const &aexgrid,
                     std::vector<double> const &gridA_proj_area = {}, int interp_style = InterpStyle::Z_INTERP,
                     std::vector<double> const &gridI_centroid_xy = {} /* [2*nI], only for sigma != 0 */) {
        std::unique_ptr<IceRegridder> sheet(new IceRegridder);
        std::vector<int64_t> a2s(agridA_.dim_to_sparse.begin(), agridA_.dim_to_sparse.end());
        std::vector<double> const &proj = gridA_proj_area.empty() ? agridA_.native_area : gridA_proj_area;
        ibh_regridder_desc d{};
        d.nX = (int64_t)aexgrid.overlaps.size();
        d.ex_indices = aexgrid.indices.data(); d.ex_area = aexgrid.overlaps.data();
        d.nI = nI; d.nA = agridA_.sparse_extent; d.nA_dense = (int32_t)a2s.size();
        d.A_to_sparse = a2s.data(); d.A_native_area = agridA_.native_area.data(); d.A_proj_area = proj.data();
        d.nhc = (int32_t)_hcdefs.size(); d.hcdefs = _hcdefs.data();
        d.hc_stride_A = hc_stride_A_; d.hc_stride_HC = hc_stride_HC_; d.interp_style = interp_style;
        d.I_centroid_xy = gridI_centroid_xy.empty() ? nullptr : gridI_centroid_xy.data();
        check(ibh_regridder_create(&d, &sheet->h_));
        sheet->_name = name; sheet->_nI = nI; sheet->_nX = (long)d.nX; sheet->interp_style = interp_style;
        sheet->aexgrid_ = aexgrid; sheet->gridA_proj_area_ = proj; sheet->gridI_centroid_xy_ = gridI_centroid_xy;
        size_t ix = sheets_.size();
        sheets_index_[name] = ix;
        sheets_.push_back(std::move(sheet));
        return ix;
    }
    /** add_sheet for a regridder already built on the device (ibh_regridder_create_hntr; modele/global_ec.cpp:418-427): takes
        ownership of `built`; the host copies ncio() writes are read back from it. */
    size_t add_sheet(std::string const &name, ibh_regridder *built, int interp_style) {
        std::unique_ptr<IceRegridder> sheet(new IceRegridder);
        sheet->h_ = built;
        int64_t nI = 0, nX = 0;
        check(ibh_regridder_sizes(built, nullptr, nullptr, &nI, &nX, nullptr));
        sheet->_name = name; sheet->_nI = (long)nI; sheet->_nX = (long)nX; sheet->interp_style = interp_style;
        sheet->aexgrid_.indices.resize(2 * (size_t)nX); sheet->aexgrid_.overlaps.resize((size_t)nX);
        check(ibh_regridder_exgrid(built, &nX, sheet->aexgrid_.indices.data(), sheet->aexgrid_.overlaps.data()));
        int32_t nAd = 0;
        check(ibh_regridder_agridA(built, &nAd, nullptr, nullptr, nullptr));
        sheet->gridA_proj_area_.resize((size_t)nAd);
        check(ibh_regridder_agridA(built, &nAd, nullptr, nullptr, sheet->gridA_proj_area_.data()));
        size_t ix = sheets_.size();
        sheets_index_[name] = ix;
        sheets_.push_back(std::move(sheet));
        return ix;
    }
    /** GCMRegridder_Standard::ncio(ncio, vname) (GCMRegridder.cpp:104-150, AbbrGrid.cpp:23-29,167-194, IceRegridder.cpp:75-90): the
        IceBin input file -- `<v>.info` {correctA, sheets}, `<v>.agridA.*`, `<v>.indexingHC`, `<v>.hcdefs(<v>.nhc)`, and per sheet
        `<v>.<sheet>.info` {name, interp_style}, `.gridA_proj_area`, `.agridI.*`, `.aexgrid.indices / .overlaps`.  Reading builds
        this (empty) regridder from the file, sheets included (their arrays go to HBM); grid specs / polygons are not part of
        the regrid path and are neither written nor read. */
    void ncio(NcIO &ncio, std::string const &vname = "m") {
        static const std::map<std::string, int> interp = {{"Z_INTERP", 0}, {"ELEV_CLASS_INTERP", 1}};
        if (ncio.reading()) {
            nc::File const &f = ncio.file;
            nc::Var const &info = f.var(vname + ".info");
            AbbrGrid a;
            nc::Var const &adim = f.var(vname + ".agridA.dim");
            a.sparse_extent = (long)adim.att("sparse_extent").at<int64_t>(0);
            a.dim_to_sparse = adim.data.as<long>();
            a.native_area = f.var(vname + ".agridA.native_area").data.as<double>();
            a.name = "gridA";
            // indexingHC: dimension ids by descending stride (GCMRegridder.cpp:43): a file may carry either layout
            nc::Var const &ix = f.var(vname + ".indexingHC");
            std::vector<long> extent = ix.att("extent").as<long>(), order = ix.att("indices").as<long>();
            std::array<long, 2> strides = {{0, 0}};
            strides[(size_t)order[1]] = 1;
            strides[(size_t)order[0]] = extent[(size_t)order[1]];
            init(std::move(a), f.var(vname + ".hcdefs").data.as<double>(), strides, info.att("correctA").at<int>(0) != 0);
            for (std::string const &name : nc::split_names(info.att("sheets").str())) {
                const std::string v = vname + "." + name;
                nc::Var const &sinfo = f.var(v + ".info");
                const std::string style = sinfo.att("interp_style").type == nc::CHAR ? sinfo.att("interp_style").str() : std::string();
                const int istyle = style.empty() ? sinfo.att("interp_style").at<int>(0) : interp.at(style);
                nc::Var const &idim = f.var(v + ".agridI.dim");
                const long nI = (long)idim.att("sparse_extent").at<int64_t>(0);
                std::vector<long> i2s = idim.data.as<long>();
                std::vector<double> cen_d = f.var(v + ".agridI.centroid_xy").data.as<double>(), cen;
                bool any = false;
                for (double c : cen_d) any = any || c != 0.0;
                if (any) {                              // dense -> sparse ice index
                    cen.assign((size_t)(2 * nI), 0.0);
                    for (size_t k = 0; k < i2s.size(); ++k) { cen[2 * (size_t)i2s[k]] = cen_d[2 * k]; cen[2 * (size_t)i2s[k] + 1] = cen_d[2 * k + 1]; }
                }
                ExchangeGrid ex;
                ex.indices = f.var(v + ".aexgrid.indices").data.as<int>();
                ex.overlaps = f.var(v + ".aexgrid.overlaps").data.as<double>();
                add_sheet(name, nI, ex, f.var(v + ".gridA_proj_area").data.as<double>(), istyle, cen);
            }
            return;
        }
        nc::File &f = ncio.file;
        const int32_t zero = 0, ca = correctA ? 1 : 0;
        std::vector<std::string> names;
        for (auto const &sh : sheets_) names.push_back(sh->name());
        f.add_var(vname + ".info", {}, nc::Array::of(&zero, 1), {{"correctA", nc::Array::of(&ca, 1)}, {"sheets", nc::Array::str(nc::join_names(names))}});
        auto put_abbr = [&](std::string const &v, std::vector<long> const &to_sparse, long extent, std::vector<double> const &native,
                            std::vector<double> const &centroid, std::string const &gname) {
            f.add_var(v + ".info", {}, nc::Array::of(&zero, 1), {{"coordinates", nc::Array::str("XY")}, {"parameterization", nc::Array::str("L0")},
                                                               {"name", nc::Array::str(gname)}, {"sproj", nc::Array::str("")}});
            std::vector<int64_t> t64(to_sparse.begin(), to_sparse.end());
            const std::string d = f.add_dim(v + ".dim.dense_extent", (int64_t)t64.size());
            const int64_t ext = extent;
            f.add_var(v + ".dim", {d}, nc::Array::of(t64), {{"sparse_extent", nc::Array::of(&ext, 1)}});
            const std::string three = f.add_dim("three", 3), two = f.add_dim("two", 2);
            f.add_var(v + ".ijk", {d, three}, nc::Array::of(std::vector<int32_t>(3 * t64.size(), 0)));
            f.add_var(v + ".native_area", {d}, nc::Array::of(native));
            f.add_var(v + ".centroid_xy", {d, two}, nc::Array::of(centroid.empty() ? std::vector<double>(2 * t64.size(), 0.0) : centroid));
        };
        put_abbr(vname + ".agridA", agridA_.dim_to_sparse, agridA_.sparse_extent, agridA_.native_area, {}, "gridA");
        const int64_t base[2] = {0, 0}, extent[2] = {(int64_t)nA(), (int64_t)nhc()};
        const int32_t order[2] = {hc_stride_HC_ >= hc_stride_A_ ? 1 : 0, hc_stride_HC_ >= hc_stride_A_ ? 0 : 1};
        f.add_var(vname + ".indexingHC", {}, nc::Array::of(&zero, 1),
                  {{"base", nc::Array::of(base, 2)}, {"extent", nc::Array::of(extent, 2)}, {"indices", nc::Array::of(order, 2)}});
        f.add_var(vname + ".hcdefs", {f.add_dim(vname + ".nhc", (int64_t)_hcdefs.size())}, nc::Array::of(_hcdefs));
        f.add_dim("agridA.ndata", (int64_t)agridA_.dim_to_sparse.size());
        for (auto const &sh : sheets_) {
            if (sh->aexgrid_.overlaps.empty() && sh->nX() != 0) throw Exception(IBH_EINVAL, "sheet '" + sh->name() + "': host copy was dropped, cannot be written");
            const std::string v = vname + "." + sh->name();
            f.add_var(v + ".info", {}, nc::Array::of(&zero, 1), {{"name", nc::Array::str(sh->name())},
                      {"interp_style", nc::Array::str(sh->interp_style == InterpStyle::ELEV_CLASS_INTERP ? "ELEV_CLASS_INTERP" : "Z_INTERP")}});
            f.add_var(v + ".gridA_proj_area", {"agridA.ndata"}, nc::Array::of(sh->gridA_proj_area_));
            std::vector<long> iota((size_t)sh->nI());
            for (size_t k = 0; k < iota.size(); ++k) iota[k] = (long)k;
            put_abbr(v + ".agridI", iota, (long)sh->nI(), std::vector<double>(sh->nI(), 0.0), sh->gridI_centroid_xy_, "gridI");
            f.add_var(v + ".aexgrid.indices", {f.add_dim(v + ".aexgrid.nindices", (int64_t)sh->aexgrid_.indices.size())}, nc::Array::of(sh->aexgrid_.indices));
            f.add_var(v + ".aexgrid.overlaps", {f.add_dim(v + ".aexgrid.noverlaps", (int64_t)sh->aexgrid_.overlaps.size())}, nc::Array::of(sh->aexgrid_.overlaps));
        }
        ncio.touch();
    }
    /** ice_regridders().index.at(name) */
    size_t sheet_index(std::string const &name) const {
        auto it = sheets_index_.find(name);
        if (it == sheets_index_.end()) throw Exception(IBH_ENOKEY, "no ice sheet named '" + name + "'");
        return it->second;
    }
    IceRegridder const *ice_regridder(size_t ix) const { return sheets_.at(ix).get(); }
    /** ice_regridders().index.size() and the strides of indexingHC: iE = iA*stride_A + ihc*stride_HC */
    size_t nsheets() const { return sheets_.size(); }
    std::array<long, 2> indexingHC_strides() const { return {{hc_stride_A_, hc_stride_HC_}}; }

    /** regrid_matrices(sheet_index, elevmaskI, params = RegridParams()) (GCMRegridder.hpp:290-293;
        RegridMatrices_Dynamic.cpp:334-402).  elevmaskI is copied. */
    std::unique_ptr<RegridMatrices_Dynamic> regrid_matrices(int sheet_index, ArrayView<const double> const &elevmaskI,
                                                            RegridParams const &params = RegridParams()) const {
        IceRegridder const *regridder = sheets_.at((size_t)sheet_index).get();
        ibh_regrid_matrices *rm = nullptr;
        check(ibh_regrid_matrices_create(regridder->h_, elevmaskI.data, elevmaskI.size(), params.scale, params.correctA,
                                         params.sigma.data(), &rm));
        return std::unique_ptr<RegridMatrices_Dynamic>(new RegridMatrices_Dynamic(regridder, rm, params));
    }
    /** Same with the elevation mask already in device memory (no counterpart in the reference, whose
        ice models live on the host): copied device-to-device on `stream`. */
    std::unique_ptr<RegridMatrices_Dynamic> regrid_matrices_device(int sheet_index, const double *d_elevmaskI, long n,
                                                                   RegridParams const &params = RegridParams(),
                                                                   void *stream = nullptr) const {
        IceRegridder const *regridder = sheets_.at((size_t)sheet_index).get();
        ibh_regrid_matrices *rm = nullptr;
        check(ibh_regrid_matrices_create_device(regridder->h_, d_elevmaskI, n, params.scale, params.correctA,
                                                params.sigma.data(), stream, &rm));
        return std::unique_ptr<RegridMatrices_Dynamic>(new RegridMatrices_Dynamic(regridder, rm, params));
    }
    /** GCMRegridder::wA (GCMRegridder.hpp:305-315, icebin_cython.cpp:103-117) */
    std::vector<double> wA(std::string const &ice_sheet_name, bool native, double fill = 0.) const {
        std::vector<double> out((size_t)nA());
        check(ibh_regridder_wA(sheets_.at(sheet_index(ice_sheet_name))->h_, native, fill, out.data()));
        return out;
    }
};

// ---- e1ve0.hpp / e1ve0.cpp:55-106 ----------------------------------------------------------------
namespace e1ve0 {
/** compute_E1vE0c(XuE1s, XuE0s, nE, areaX): the correction matrix between last step's and this step's elevation grids,
    one XuE matrix per ice sheet; returned over the sparse E space (rows iE1, columns iE0), where the reference returns
    the same tuples as a spsparse::TupleList (areaX is unused there too). */
inline std::unique_ptr<linear::Weighted_Eigen> compute_E1vE0c(std::vector<linear::Weighted_Eigen const *> const &XuE1s,
                                                               std::vector<linear::Weighted_Eigen const *> const &XuE0s,
                                                               unsigned long nE) {
    if (XuE1s.size() != XuE0s.size() || XuE1s.empty()) throw Exception(IBH_EINVAL, "compute_E1vE0c: need one XuE1 and one XuE0 per ice sheet");
    std::vector<const ibh_weighted *> a, b;
    for (auto *w : XuE1s) a.push_back(w->handle());
    for (auto *w : XuE0s) b.push_back(w->handle());
    ibh_weighted *out = nullptr;
    check(ibh_e1ve0_compute((int32_t)a.size(), a.data(), b.data(), (int64_t)nE, &out));
    return std::unique_ptr<linear::Weighted_Eigen>(new linear::Weighted_Eigen(out));
}
}   // namespace e1ve0

// ---- gridgen/GridGen_Exchange.cpp:175-284 ----------------------------------------------------------
/** make_exchange_grid for a rectilinear XY ice grid under projected GCM-cell polygons (ibh_exgrid_generate): simple and
 *  counter-clockwise; a call with a non-convex polygon, or one of more than 16 vertices, runs the streamed clip. */
inline ExchangeGrid make_exchange_grid(std::vector<double> const &xedges, std::vector<double> const &yedges, bool x_fastest,
                                       std::vector<int> const &polyptr, std::vector<double> const &vx, std::vector<double> const &vy,
                                       std::vector<long> const &iA) {
    std::vector<int64_t> ia(iA.begin(), iA.end());
    ibh_exgrid_desc d{};
    d.nx = (int32_t)xedges.size() - 1; d.ny = (int32_t)yedges.size() - 1; d.xedges = xedges.data(); d.yedges = yedges.data();
    d.x_fastest = x_fastest; d.npoly = (int32_t)ia.size(); d.polyptr = polyptr.data(); d.vx = vx.data(); d.vy = vy.data(); d.iA = ia.data();
    ibh_exgrid *h = nullptr;
    check(ibh_exgrid_generate(&d, &h));
    ExchangeGrid ex;
    int64_t n = 0;
    int rc = ibh_exgrid_size(h, &n);
    if (rc == IBH_OK) { ex.indices.resize((size_t)(2 * n)); ex.overlaps.resize((size_t)n); rc = ibh_exgrid_get(h, ex.indices.data(), ex.overlaps.data()); }
    ibh_exgrid_destroy(h);
    check(rc);
    return ex;
}

// ---- from grid specs: GridSpec.hpp:180-247, gridgen/GridGen_LonLat.cpp:109-232 ----------------------------------------------
/** GridSpec_LonLat (GridSpec.hpp:180-247): boundaries in degrees, indices by decreasing stride ({1,0}: index = j*nlon + i). */
struct GridSpec_LonLat {
    std::vector<double> lonb, latb;
    std::vector<int> indices{1, 0};
    bool south_pole = false, north_pole = false;
    int points_in_side = 1;
    double eq_rad = 6371000.;
    int nlon() const { return (int)lonb.size() - 1; }
    int nlat() const { return (int)latb.size() - 1 + (south_pole ? 1 : 0) + (north_pole ? 1 : 0); }
};
/** The `sproj` string of an XY grid spec, parsed (ibh_parse_sproj): proj=stere only; an unknown key throws, named. */
inline ibh_stere_params parse_sproj(std::string const &sproj) {
    ibh_stere_params p{};
    check(ibh_parse_sproj(sproj.c_str(), &p));
    return p;
}
/** The realised cells of a lon/lat spec in HBM, projected (ibh_lonlat_cells): make_grid for the cells `realised` lists
    (strictly ascending sparse indices), with native and projected areas. */
class LonLatCells {
    ibh_lonlat_cells *h_ = nullptr;
public:
    LonLatCells(GridSpec_LonLat const &spec, std::vector<long> const &realised, std::string const &sproj) {
        ibh_stere_params p = parse_sproj(sproj);
        std::vector<int64_t> r(realised.begin(), realised.end());
        ibh_lonlat_cells_desc d{};
        d.nlonb = (int32_t)spec.lonb.size(); d.nlatb = (int32_t)spec.latb.size(); d.lonb = spec.lonb.data(); d.latb = spec.latb.data();
        if (spec.indices.size() != 2) throw std::runtime_error("GridSpec_LonLat: indices must have two entries");
        d.indices[0] = spec.indices[0]; d.indices[1] = spec.indices[1];
        d.south_pole = spec.south_pole; d.north_pole = spec.north_pole; d.points_in_side = spec.points_in_side; d.eq_rad = spec.eq_rad;
        d.nrealised = (int64_t)r.size(); d.realised = r.data(); d.proj = &p;
        check(ibh_lonlat_cells_create(&d, &h_));
    }
    ~LonLatCells() { ibh_lonlat_cells_destroy(h_); }
    LonLatCells(LonLatCells const &) = delete;
    LonLatCells &operator=(LonLatCells const &) = delete;
    ibh_lonlat_cells *handle() const { return h_; }
    long ncell() const { int32_t n = 0; check(ibh_lonlat_cells_size(h_, &n, nullptr, nullptr)); return n; }
    long nA() const { int64_t n = 0; check(ibh_lonlat_cells_size(h_, nullptr, nullptr, &n)); return (long)n; }
};
/** make_exchange_grid under those cells (ibh_exgrid_generate_lonlat): any number of vertices per cell. */
inline ExchangeGrid make_exchange_grid_lonlat(LonLatCells const &cells, std::vector<double> const &xedges, std::vector<double> const &yedges,
                                              bool x_fastest) {
    ibh_exgrid *h = nullptr;
    check(ibh_exgrid_generate_lonlat(cells.handle(), (int32_t)xedges.size() - 1, (int32_t)yedges.size() - 1, xedges.data(), yedges.data(),
                                     x_fastest, &h));
    ExchangeGrid ex;
    int64_t n = 0;
    int rc = ibh_exgrid_size(h, &n);
    if (rc == IBH_OK) { ex.indices.resize((size_t)(2 * n)); ex.overlaps.resize((size_t)n); rc = ibh_exgrid_get(h, ex.indices.data(), ex.overlaps.data()); }
    ibh_exgrid_destroy(h);
    check(rc);
    return ex;
}
/** From grid specs to a GCMRegridder_Standard with one sheet, built on the device (ibh_regridder_create_lonlat); indexingHC
    {1, nA} (HC slowest). */
inline std::unique_ptr<GCMRegridder_Standard> regridder_from_specs(GridSpec_LonLat const &spec, std::vector<long> const &realised,
                                                                   std::vector<double> const &xedges, std::vector<double> const &yedges,
                                                                   bool x_fastest, std::string const &sproj, std::vector<double> hcdefs,
                                                                   bool correctA = true, int interp_style = InterpStyle::Z_INTERP,
                                                                   std::string const &sheet_name = "ice") {
    LonLatCells cells(spec, realised, sproj);
    const long nA = cells.nA();
    ibh_lonlat_regridder_desc d{};
    d.cells = cells.handle();
    d.nx = (int32_t)xedges.size() - 1; d.ny = (int32_t)yedges.size() - 1; d.xedges = xedges.data(); d.yedges = yedges.data();
    d.x_fastest = x_fastest; d.nhc = (int32_t)hcdefs.size(); d.hcdefs = hcdefs.data();
    d.hc_stride_A = 1; d.hc_stride_HC = nA; d.interp_style = interp_style;
    ibh_regridder *rg = nullptr;
    check(ibh_regridder_create_lonlat(&d, nullptr, &rg));
    std::unique_ptr<ibh_regridder, int (*)(ibh_regridder *)> owned(rg, ibh_regridder_destroy);     // until the sheet owns it
    AbbrGrid a;
    int32_t nAd = 0;
    check(ibh_regridder_agridA(rg, &nAd, nullptr, nullptr, nullptr));
    std::vector<int64_t> a2s((size_t)nAd);
    a.native_area.resize((size_t)nAd);
    check(ibh_regridder_agridA(rg, &nAd, a2s.data(), a.native_area.data(), nullptr));
    a.sparse_extent = nA;
    a.dim_to_sparse.assign(a2s.begin(), a2s.end());
    a.name = "A";
    std::unique_ptr<GCMRegridder_Standard> gcm(new GCMRegridder_Standard);
    gcm->init(std::move(a), std::move(hcdefs), {{1, nA}}, correctA);
    gcm->add_sheet(sheet_name, owned.release(), interp_style);
    return gcm;
}

// ---- modele/hntr.hpp:63-135, GridSpec.hpp:143-160 ----------------------------------------------------
namespace modele {
/** HntrSpec(im, jm, offi, dlat) (GridSpec.hpp:143-160): offi = cells from the date line to the western edge of cell 1,
    dlat = minutes of latitude of a non-polar cell; fields are i-fastest, IJ = IA + im*(JA-1). */
struct HntrSpec {
    int im, jm;
    double offi, dlat;
    HntrSpec() : im(-1), jm(-1), offi(0), dlat(0) {}
    HntrSpec(int _im, int _jm, double _offi, double _dlat) : im(_im), jm(_jm), offi(_offi), dlat(_dlat) {}
    int size() const { return im * jm; }
};
/** make_dxyp(spec) (hntr.cpp:33-52): areas of the grid's rows on a unit sphere, 0-based storage [jm] (ibh_hntr_dxyp, host only). */
inline std::vector<double> make_dxyp(HntrSpec const &spec) {
    std::vector<double> d((size_t)(spec.jm > 0 ? spec.jm : 0));
    check(ibh_hntr_dxyp(spec.im, spec.jm, d.data()));
    return d;
}
/** The part of HntrGrid (hntr.hpp:17-54) a caller of Hntr reads: hntr.Agrid.spec, hntr.Bgrid.spec, and dxyp(j) with the
    reference's 1-based (Fortran) indexing, j = 1..jm. */
struct HntrGrid {
    HntrSpec spec;
    std::vector<double> dxyp_;
    HntrGrid() {}
    explicit HntrGrid(HntrSpec const &s) : spec(s), dxyp_(make_dxyp(s)) {}
    double dxyp(int j) const { return dxyp_.at((size_t)(j - 1)); }
};

/** DimClip (hntr.hpp:186-197): includes a B cell iff the set holds it. */
struct DimClip {
    SparseSetT const *dim;
    explicit DimClip(SparseSetT const *_dim) : dim(_dim) {}
    bool operator()(int ix) const { return dim->in_sparse(ix); }
};
/** The default includeB of the matrix forms: every B cell. */
struct IncludeAll {
    bool operator()(int) const { return true; }
};
/** spsparse's DenseTransform, per index of MakeDenseEigenT. */
enum class DenseTransform { ADD_DENSE = IBH_ADD_DENSE, TO_DENSE = IBH_TO_DENSE, TO_DENSE_IGNORE_MISSING = IBH_TO_DENSE_IGNORE_MISSING };
/** Which accumulator of Hntr::matrix: OverlapMatAccum (overlap) or ScaledRegridMatAccum (scaled_regrid_matrix). */
enum class HntrMatrix { OVERLAP = IBH_HNTR_OVERLAP, SCALED = IBH_HNTR_SCALED };

/** The element types of the typed regrid and their IBH_HNTR_* codes; any other type has no code and does not compile. */
template <class T> struct HntrElem;
template <> struct HntrElem<double> { static constexpr int code = IBH_HNTR_F64; };
template <> struct HntrElem<float> { static constexpr int code = IBH_HNTR_F32; };
template <> struct HntrElem<int16_t> { static constexpr int code = IBH_HNTR_I16; };
/** A constant weight in place of WTA: the reference's const_array(shape, c), a stride-0 array that holds one number. */
struct ConstWeight {
    double c;
};

/** Hntr (hntr.hpp:63-135): the partition is computed and uploaded to the current HIP device by the constructor; regrid
    runs on that device.  Owns a device handle: movable, not copyable. */
class Hntr {
    ibh_hntr *h_;
    /** The reference's dimension check (hntr.hpp:361-369). */
    void check_dims(long nW, long nA, long nB) const {
        if (nW != Agrid.spec.size() || nA != Agrid.spec.size() || nB != Bgrid.spec.size())
            throw Exception(IBH_EINVAL, "Error in dimensions: (" + std::to_string(nW) + ", " + std::to_string(nA) + ", " +
                                        std::to_string(nB) + ") vs. (" + std::to_string(Agrid.spec.size()) + ", " +
                                        std::to_string(Bgrid.spec.size()) + ")");
    }
public:
    HntrGrid const Agrid;
    HntrGrid const Bgrid;
    double DATMIS;

    /** Hntr(yp17, Bgrid, Agrid, DATMIS) (hntr.cpp:63-79); yp17 is ignored, as in the reference. */
    Hntr(double /*yp17*/, HntrSpec const &_B, HntrSpec const &_A, double _DATMIS = 0.0)
        : h_(nullptr), Agrid(_A), Bgrid(_B), DATMIS(_DATMIS) {
        check(ibh_hntr_create(&h_, _A.im, _A.jm, _A.offi, _A.dlat, _B.im, _B.jm, _B.offi, _B.dlat, _DATMIS));
    }
    Hntr(Hntr const &) = delete;
    Hntr &operator=(Hntr const &) = delete;
    Hntr(Hntr &&o) noexcept : h_(o.h_), Agrid(o.Agrid), Bgrid(o.Bgrid), DATMIS(o.DATMIS) { o.h_ = nullptr; }
    ~Hntr() { if (h_) ibh_hntr_destroy(h_); }

    /** regrid(WTA, A, B, mean_polar, wtm, wtb) (hntr.hpp:204-211, :341-435) on host arrays of one field; the reference's
        dimension check (:361-369) included. */
    void regrid(ArrayView<const double> const &WTA, ArrayView<const double> const &A, ArrayView<double> const &B,
                bool mean_polar = false, double wtm = 1.0, double wtb = 0.0) const {
        check_dims(WTA.size(), A.size(), B.size());
        check(ibh_hntr_regrid_host(h_, WTA.data, 0, A.data, 1, Agrid.spec.size(), B.data, Bgrid.spec.size(), mean_polar ? 1 : 0, wtm, wtb));
    }
    /** regrid(WTA, A, mean_polar) (hntr.hpp:214-218): allocates and returns B. */
    std::vector<double> regrid(ArrayView<const double> const &WTA, ArrayView<const double> const &A, bool mean_polar = false) const {
        std::vector<double> B((size_t)Bgrid.spec.size());
        regrid(WTA, A, ArrayView<double>(B.data(), (long)B.size()), mean_polar);
        return B;
    }
    /** regrid<WeightT, SrcT>(WTA, A, B, mean_polar, wtm, wtb): the reference's template (hntr.hpp:385-391) with DestT = double,
        for WeightT and SrcT in double, float, int16_t (e.g. regrid<double, int16_t, double> from the 1' ETOPO1 planes,
        etopo1_ice.cpp:22-26).  The planes are copied to the device in their own width; bitwise the double overload on the
        widened arrays.  Any other element type does not compile. */
    template <class WeightT, class SrcT>
    void regrid(ArrayView<const WeightT> const &WTA, ArrayView<const SrcT> const &A, ArrayView<double> const &B,
                bool mean_polar = false, double wtm = 1.0, double wtb = 0.0) const {
        check_dims(WTA.size(), A.size(), B.size());
        check(ibh_hntr_regrid_typed_host(h_, WTA.data, HntrElem<WeightT>::code, 0, 0.0, A.data, HntrElem<SrcT>::code, 1, Agrid.spec.size(),
                                         B.data, Bgrid.spec.size(), mean_polar ? 1 : 0, wtm, wtb));
    }
    /** The same under a constant weight, the reference's const_array(shape, c) as WTA: regrid(ConstWeight{1.0}, A, B, ...). */
    template <class SrcT>
    void regrid(ConstWeight const &WTA, ArrayView<const SrcT> const &A, ArrayView<double> const &B, bool mean_polar = false,
                double wtm = 1.0, double wtb = 0.0) const {
        check_dims(Agrid.spec.size(), A.size(), B.size());
        check(ibh_hntr_regrid_typed_host(h_, nullptr, IBH_HNTR_F64, 0, WTA.c, A.data, HntrElem<SrcT>::code, 1, Agrid.spec.size(), B.data,
                                         Bgrid.spec.size(), mean_polar ? 1 : 0, wtm, wtb));
    }
    /** Device overloads with typed pointers: as the double one below; wta_ld and lda count elements of the plane's own type.
        A pure enqueue on `stream` (ibh_hntr_regrid_typed_device). */
    template <class WeightT, class SrcT>
    void regrid(const WeightT *dWTA, long wta_ld, const SrcT *dA, int nvar, long lda, double *dB, long ldb, bool mean_polar = false,
                double wtm = 1.0, double wtb = 0.0, void *stream = nullptr) const {
        check(ibh_hntr_regrid_typed_device(h_, dWTA, HntrElem<WeightT>::code, wta_ld, 0.0, dA, HntrElem<SrcT>::code, nvar, lda, dB, ldb,
                                           mean_polar ? 1 : 0, wtm, wtb, stream));
    }
    template <class SrcT>
    void regrid(ConstWeight const &WTA, const SrcT *dA, int nvar, long lda, double *dB, long ldb, bool mean_polar = false,
                double wtm = 1.0, double wtb = 0.0, void *stream = nullptr) const {
        check(ibh_hntr_regrid_typed_device(h_, nullptr, IBH_HNTR_F64, 0, WTA.c, dA, HntrElem<SrcT>::code, nvar, lda, dB, ldb,
                                           mean_polar ? 1 : 0, wtm, wtb, stream));
    }
    /** Device overload: nvar fields resident in HBM, B[k*ldb + IJB] from A[k*lda + IJA]; the weight is one plane for all
        fields (wta_ld = 0) or one per field.  A pure enqueue on `stream` (ibh_hntr_regrid_device). */
    void regrid(const double *dWTA, long wta_ld, const double *dA, int nvar, long lda, double *dB, long ldb,
                bool mean_polar = false, double wtm = 1.0, double wtb = 0.0, void *stream = nullptr) const {
        check(ibh_hntr_regrid_device(h_, dWTA, wta_ld, dA, nvar, lda, dB, ldb, mean_polar ? 1 : 0, wtm, wtb, stream));
    }
    ibh_hntr *handle() const { return h_; }

    /** overlap(accum, eq_rad, includeB) (hntr.hpp:284-291): accum.add({iB, iA}, FG * (1/WEIGHT) * (R2*dxyp(JB))) for every
        term, in the reference's stream order, 0-based sparse indices.  includeB(IJB-1) is evaluated on the host for every B
        cell first; the entries are computed on the device (ibh_hntr_triplets). */
    template <class AccumT, class IncludeT = IncludeAll>
    void overlap(AccumT &&accum, double eq_rad, IncludeT includeB = IncludeAll()) const {
        feed(accum, HntrMatrix::OVERLAP, eq_rad, includeB);
    }
    /** scaled_regrid_matrix(accum, includeB) (hntr.hpp:327-336): the same with FG * (1/WEIGHT). */
    template <class AccumT, class IncludeT = IncludeAll>
    void scaled_regrid_matrix(AccumT &&accum, IncludeT includeB = IncludeAll()) const {
        feed(accum, HntrMatrix::SCALED, 1.0, includeB);
    }
    /** MakeDenseEigenT(overlap | scaled_regrid_matrix, transforms, dims, transpose) (GCMRegridder_ModelE.cpp:92-121) as a
        Weighted in HBM (ibh_hntr_matrix_d): dims = {dimB, dimA}, IN/OUT, nullptr for a fresh identity set owned by the result;
        transforms per generator index (B, then A); transpose 'T' swaps only the output.  wM / Mw are the row / column sums. */
    template <class IncludeT = IncludeAll>
    std::unique_ptr<linear::Weighted> matrix_d(HntrMatrix kind, double eq_rad, std::array<SparseSetT *, 2> const &dims = {{nullptr, nullptr}},
                                               std::array<DenseTransform, 2> const &transforms = {{DenseTransform::ADD_DENSE, DenseTransform::ADD_DENSE}},
                                               char transpose = '.', IncludeT includeB = IncludeAll()) const {
        std::vector<uint8_t> mask;
        const uint8_t *m = include_mask(includeB, mask);
        ibh_weighted *w = nullptr;
        check(ibh_hntr_matrix_d(h_, (int)kind, eq_rad, m, dims[0] ? dims[0]->handle() : nullptr, (int)transforms[0],
                                dims[1] ? dims[1]->handle() : nullptr, (int)transforms[1], transpose == 'T' ? 1 : 0, &w));
        return std::unique_ptr<linear::Weighted>(new linear::Weighted(w));
    }

private:
    const uint8_t *include_mask(IncludeAll const &, std::vector<uint8_t> &) const { return nullptr; }
    template <class IncludeT>
    const uint8_t *include_mask(IncludeT const &includeB, std::vector<uint8_t> &mask) const {
        mask.resize((size_t)Bgrid.spec.size());
        for (int i = 0; i < Bgrid.spec.size(); ++i) mask[(size_t)i] = includeB(i) ? 1 : 0;
        return mask.data();
    }
    template <class AccumT, class IncludeT>
    void feed(AccumT &accum, HntrMatrix kind, double eq_rad, IncludeT const &includeB) const {
        std::vector<uint8_t> mask;
        const uint8_t *m = include_mask(includeB, mask);
        int64_t n = 0;
        check(ibh_hntr_triplets(h_, (int)kind, eq_rad, m, &n, nullptr, nullptr, nullptr));
        std::vector<int32_t> iB((size_t)n), iA((size_t)n);
        std::vector<double> val((size_t)n);
        if (n) check(ibh_hntr_triplets(h_, (int)kind, eq_rad, m, &n, iB.data(), iA.data(), val.data()));
        for (size_t k = 0; k < (size_t)n; ++k) accum.add({iB[k], iA[k]}, val[k]);
    }
};

/** hcdefs of global_ec (modele/global_ec.cpp:403-407): elev = lo, lo+skip, ... while elev <= hi, accumulated by addition. */
inline std::vector<double> make_hcdefs(double ec_lo, double ec_hi, double ec_skip) {
    std::vector<double> hcdefs;
    for (double elev = ec_lo; elev <= ec_hi; elev += ec_skip) hcdefs.push_back(elev);
    return hcdefs;
}

/** new_gcmA_standard (modele/global_ec.cpp:384-432): Hntr(17.17, hspecA, hspecI).overlap(ExchAccum(...), eq_rad) under the
    ice mask, built on the device (ibh_regridder_create_hntr) into a GCMRegridder_Standard with one sheet "globalI";
    indexingHC {1, nA} (HC slowest).  dimA / dimI, if given (empty), receive _dimA and _dimI. */
inline std::unique_ptr<GCMRegridder_Standard> new_gcmA_standard(HntrSpec const &hspecA, HntrSpec const &hspecI,
                                                                ArrayView<const double> const &elevmaskI, std::vector<double> hcdefs,
                                                                bool correctA, double eq_rad, int interp_style = InterpStyle::Z_INTERP,
                                                                SparseSetT *dimA = nullptr, SparseSetT *dimI = nullptr) {
    Hntr hntr(17.17, hspecA, hspecI);
    ibh_hntr_regridder_desc d{};
    d.hntr = hntr.handle(); d.eq_rad = eq_rad;
    d.elevmaskI = elevmaskI.data; d.nmask = elevmaskI.size();
    d.nhc = (int32_t)hcdefs.size(); d.hcdefs = hcdefs.data();
    d.hc_stride_A = 1; d.hc_stride_HC = hspecA.size();
    d.interp_style = interp_style;
    ibh_regridder *rg = nullptr;
    check(ibh_regridder_create_hntr(&d, dimA ? dimA->handle() : nullptr, dimI ? dimI->handle() : nullptr, &rg));
    std::unique_ptr<ibh_regridder, int (*)(ibh_regridder *)> owned(rg, ibh_regridder_destroy);     // until the sheet owns it
    AbbrGrid a;
    int32_t nAd = 0;
    check(ibh_regridder_agridA(rg, &nAd, nullptr, nullptr, nullptr));
    std::vector<int64_t> a2s((size_t)nAd);
    a.native_area.resize((size_t)nAd);
    check(ibh_regridder_agridA(rg, &nAd, a2s.data(), a.native_area.data(), nullptr));
    a.sparse_extent = hspecA.size();
    a.dim_to_sparse.assign(a2s.begin(), a2s.end());
    a.name = "A";
    std::unique_ptr<GCMRegridder_Standard> gcmA(new GCMRegridder_Standard);
    gcmA->init(std::move(a), std::move(hcdefs), {{1, (long)hspecA.size()}}, correctA);
    gcmA->add_sheet("globalI", owned.release(), interp_style);
    return gcmA;
}

/** make_I2vX (modele/global_ec.cpp:345-376): IvX (IvE or IvA) onto the plottable grid hspecI2, through
    Hntr(17.17, hspecI, hspecI2).overlap(eq_rad, ElevMaskClip(elevmaskI)) (ibh_weighted_make_I2vX).  dims {dimI2, dimX}; dimI2
    must outlive the result. */
inline std::unique_ptr<linear::Weighted_Eigen> make_I2vX(linear::Weighted_Eigen const &IvX, HntrSpec const &hspecI,
                                                         HntrSpec const &hspecI2, ArrayView<const double> const &elevmaskI,
                                                         SparseSetT &dimI2, double eq_rad) {
    Hntr hntr_IvI2(17.17, hspecI, hspecI2);
    std::vector<uint8_t> incl((size_t)elevmaskI.size());
    for (size_t i = 0; i < incl.size(); ++i) incl[i] = std::isnan(elevmaskI.data[i]) ? 0 : 1;
    ibh_weighted *w = nullptr;
    check(ibh_weighted_make_I2vX(IvX.handle(), hntr_IvI2.handle(), eq_rad, incl.data(), (int64_t)incl.size(), dimI2.handle(), &w));
    return std::unique_ptr<linear::Weighted_Eigen>(new linear::Weighted_Eigen(w));
}

/** check_negative (modele/global_ec.cpp:440-463): prints every negative weight and matrix entry, then throws if there was one. */
inline void check_negative(linear::Weighted_Eigen const &mat, std::string const &name) {
    bool neg = false;
    std::array<std::vector<double> const *, 2> const weights{{&mat.wM(), &mat.Mw()}};
    for (int j = 0; j < 2; ++j) {
        auto const &wt = *weights[(size_t)j];
        for (size_t i = 0; i < wt.size(); ++i)
            if (wt[i] < 0) { printf("wt[%d](%d) = %g\n", j, (int)i, wt[i]); neg = true; }
    }
    for (auto const &t : mat.M.triplets())
        if (t.value < 0) { printf("%s(%d,%d)=%g\n", name.c_str(), t.row, t.col, t.value); neg = true; }
    if (neg) throw Exception(IBH_EINVAL, "Negative values found in matrix or weights for " + name);
}

// ---- global_ec in chunks: main() of modele/global_ec.cpp (:752-893) and combine_global_ec.cpp's combine_chunks (:94-262) ----
namespace global_ec {

/** {chunkno, jO0, iO0, jO1, iO1} (global_ec.cpp:892): the ocean cells [jO0 * imO + iO0, jO1 * imO + iO1) in row-major order. */
typedef std::array<int, 5> Chunk;
struct ChunkPlan {
    std::vector<Chunk> chunks;
    std::vector<long> nice;         // the count the reference prints (:891): the chunk's ice plus the cell that ended it
};

/** The global ice of main() (:762-816) on the device (ibh_global_ec_scan_create): the int16 planes FGICE1m / ZICETOP1m
    [jmI, imI] on the host (uploaded once in their own width) or, with on_device, in HBM (read on `stream`; they outlive the
    scan).  hspecI must nest in hspecO. */
class IceScan {
    ibh_global_ec_scan *h_ = nullptr;
public:
    HntrSpec const hspecO, hspecI;
    IceScan(HntrSpec const &_hspecO, HntrSpec const &_hspecI, ArrayView<const int16_t> const &fgiceI, ArrayView<const int16_t> const &elevI,
            bool on_device = false, void *stream = nullptr)
        : hspecO(_hspecO), hspecI(_hspecI) {
        if (fgiceI.size() != elevI.size()) throw Exception(IBH_EINVAL, "fgiceI / elevI: the planes differ in size");
        check(ibh_global_ec_scan_create(hspecO.im, hspecO.jm, hspecO.offi, hspecO.dlat, hspecI.im, hspecI.jm, hspecI.offi, hspecI.dlat,
                                        fgiceI.data, elevI.data, fgiceI.size(), IBH_HNTR_I16, on_device ? 1 : 0, stream, &h_));
    }
    IceScan(IceScan const &) = delete;
    IceScan &operator=(IceScan const &) = delete;
    ~IceScan() { if (h_) ibh_global_ec_scan_destroy(h_); }
    ibh_global_ec_scan *handle() const { return h_; }
    int mult_i() const { return hspecI.im / hspecO.im; }
    int mult_j() const { return hspecI.jm / hspecO.jm; }
    /** Hntr(17.17, hspecO, hspecI).regrid(const 1.0, fgiceI) (:778-780), [jmO * imO] */
    std::vector<double> fgiceO() const {
        std::vector<double> f((size_t)hspecO.size());
        check(ibh_global_ec_scan_get(h_, nullptr, nullptr, nullptr, f.data(), nullptr));
        return f;
    }
    /** the cells with fgiceI != 0 of every ocean cell's tile, [jmO * imO] */
    std::vector<int> nice() const {
        std::vector<int32_t> n((size_t)hspecO.size());
        check(ibh_global_ec_scan_get(h_, nullptr, nullptr, nullptr, nullptr, n.data()));
        return std::vector<int>(n.begin(), n.end());
    }
    /** the two arrays where they are, in HBM */
    const double *fgiceO_device() const { const double *p; check(ibh_global_ec_scan_get(h_, &p, nullptr, nullptr, nullptr, nullptr)); return p; }
    const int32_t *nice_device() const { const int32_t *p; check(ibh_global_ec_scan_get(h_, nullptr, &p, nullptr, nullptr, nullptr)); return p; }
    /** elevI_range (:805-813) */
    std::array<int16_t, 2> elevI_range() const {
        std::array<int16_t, 2> r;
        check(ibh_global_ec_scan_get(h_, nullptr, nullptr, r.data(), nullptr, nullptr));
        return r;
    }
    /** args.ec_range (:815-816): the same for every chunk */
    std::array<double, 2> ec_range(double ec_skip) const {
        std::array<double, 2> out;
        check(ibh_global_ec_ec_range(elevI_range().data(), ec_skip, out.data()));
        return out;
    }
};

/** The chunk plan (:863-893; ibh_global_ec_chunk_plan): chunk_size must exceed mult_i * mult_j. */
inline ChunkPlan chunk_plan(IceScan const &scan, long chunk_size = 12000000) {
    int32_t n = 0;
    check(ibh_global_ec_chunk_plan(scan.handle(), chunk_size, 0, nullptr, nullptr, &n));
    std::vector<int32_t> ch(5 * (size_t)n);
    std::vector<int64_t> nice((size_t)n);
    check(ibh_global_ec_chunk_plan(scan.handle(), chunk_size, n, ch.data(), nice.data(), &n));
    ChunkPlan plan;
    for (size_t c = 0; c < (size_t)n; ++c) plan.chunks.push_back({{ch[5 * c], ch[5 * c + 1], ch[5 * c + 2], ch[5 * c + 3], ch[5 * c + 4]}});
    plan.nice.assign(nice.begin(), nice.end());
    return plan;
}

/** A chunk's elevmaskI (:818-855) into a device array of hspecI.size() doubles, one launch on `stream`. */
inline void chunk_mask(IceScan const &scan, Chunk const &chunk, double *d_elevmaskI, void *stream = nullptr) {
    check(ibh_global_ec_chunk_mask(scan.handle(), chunk[1], chunk[2], chunk[3], chunk[4], d_elevmaskI, scan.hspecI.size(), stream));
}
/** The same, brought to the host (for new_gcmA_standard's host mask). */
inline std::vector<double> chunk_mask(IceScan const &scan, Chunk const &chunk) {
    std::vector<double> em((size_t)scan.hspecI.size());
    check(ibh_global_ec_chunk_mask_host(scan.handle(), chunk[1], chunk[2], chunk[3], chunk[4], em.data(), (int64_t)em.size()));
    return em;
}

/** What combine_chunks gives: the combined matrix over the first-seen numbering of the chunks' sets, with the chunks' weights
    summed in chunk order, and the triplet stream it was summed from, in sparse indices (the reference's contract and
    EOpvAOpBase's form). */
struct CombinedChunks {
    std::unique_ptr<linear::Weighted_Eigen> M;
    std::vector<int64_t> iB, iA;
    std::vector<double> val;
};
/** combine_chunks (combine_global_ec.cpp:94-262) for one matrix: the chunks' UNSCALED matrices in chunk order, read where they
    are, in HBM (ibh_global_ec_combine_chunks). */
inline CombinedChunks combine_chunks(std::vector<linear::Weighted const *> const &mats, bool scale = false) {
    std::vector<const ibh_weighted *> hs;
    size_t nnz = 0;
    for (linear::Weighted const *m : mats) {
        if (!m) throw Exception(IBH_EINVAL, "mats: null chunk matrix");
        hs.push_back(m->handle());
        nnz += (size_t)m->nnz();
    }
    CombinedChunks out;
    out.iB.resize(nnz); out.iA.resize(nnz); out.val.resize(nnz);
    ibh_weighted *w = nullptr;
    check(ibh_global_ec_combine_chunks((int32_t)hs.size(), hs.data(), nullptr, nullptr, scale ? 1 : 0, out.iB.data(), out.iA.data(),
                                       out.val.data(), &w));
    out.M.reset(new linear::Weighted_Eigen(w));
    return out;
}

}   // namespace global_ec

// ---- modele/etopo1_ice.cpp:45-247 --------------------------------------------------------------------
/** The grids of one etopo1_ice (ibh_etopo1_ice_create): the row areas of hspecI and hspecC and, with hspecH, the regridder of
    store_h (:22), on the current HIP device.  hspecI must nest in hspecC, a coarse cell holding at most IBH_ETOPO1_MAX_TILE
    fine cells.  Owns a device handle: not copyable. */
class Etopo1IceGrids {
    ibh_etopo1_ice *h_ = nullptr;
public:
    HntrSpec const hspecI, hspecC, hspecH;      // hspecH.im == 0: no h planes
    Etopo1IceGrids(HntrSpec const &_hspecI, HntrSpec const &_hspecC, HntrSpec const *_hspecH = nullptr)
        : hspecI(_hspecI), hspecC(_hspecC), hspecH(_hspecH ? *_hspecH : HntrSpec(0, 0, 0., 0.)) {
        check(ibh_etopo1_ice_create(&h_, hspecI.im, hspecI.jm, hspecI.offi, hspecI.dlat, hspecC.im, hspecC.jm, hspecH.im, hspecH.jm,
                                    hspecH.offi, hspecH.dlat));
    }
    Etopo1IceGrids(Etopo1IceGrids const &) = delete;
    Etopo1IceGrids &operator=(Etopo1IceGrids const &) = delete;
    ~Etopo1IceGrids() { if (h_) ibh_etopo1_ice_destroy(h_); }
    ibh_etopo1_ice *handle() const { return h_; }
    bool has_h() const { return hspecH.im != 0; }
    /** The planes where they are, in HBM: a pure enqueue on `stream` (ibh_etopo1_ice_device).  d_planes_h: the four h planes
        FOCEANh, FGICEh, ZICETOPh, ZSOLGh, ldh doubles apart, or nullptr. */
    void run_device(const int16_t *d_focean, const int16_t *d_zictop, const int16_t *d_zsolid, const double *d_fgiceC, bool include_greenland,
                    int16_t *d_FOCEAN1m, int16_t *d_FGICE1m, int16_t *d_ZICETOP1m, int16_t *d_ZSOLG1m, double *d_planes_h = nullptr, long ldh = 0,
                    void *stream = nullptr) const {
        check(ibh_etopo1_ice_device(h_, d_focean, d_zictop, d_zsolid, d_fgiceC, include_greenland ? 1 : 0, d_FOCEAN1m, d_FGICE1m, d_ZICETOP1m,
                                    d_ZSOLG1m, d_planes_h, ldh, stream));
    }
};

/** What etopo1_ice writes to <root>1m.nc and <root>h.nc, as arrays: the int16 planes [jmI * imI] and the double h planes
    [jmH * imH] (empty without hspecH). */
struct Etopo1Ice {
    std::vector<int16_t> FOCEAN1m, FGICE1m, ZICETOP1m, ZSOLG1m;
    std::vector<double> FOCEANh, FGICEh, ZICETOPh, ZSOLGh;
};

/** etopo1_ice(files, include_greenland, ofname_root) (etopo1_ice.cpp:45-247) from host arrays instead of files
    (ibh_etopo1_ice_host): focean / zictop / zsolid are the file's FOCEAN / ZICTOP / ZSOLID [jmI * imI], fgiceC its FGICE1
    [jmC * imC]; every plane crosses PCIe once in its own width.  hspecH: the grid of the h planes, nullptr for none. */
inline Etopo1Ice etopo1_ice(HntrSpec const &hspecI, HntrSpec const &hspecC, ArrayView<const int16_t> const &focean,
                            ArrayView<const int16_t> const &zictop, ArrayView<const int16_t> const &zsolid, ArrayView<const double> const &fgiceC,
                            bool include_greenland = false, HntrSpec const *hspecH = nullptr) {
    if (focean.size() != hspecI.size() || zictop.size() != hspecI.size() || zsolid.size() != hspecI.size())
        throw Exception(IBH_EINVAL, "focean / zictop / zsolid: a plane does not hold the " + std::to_string(hspecI.size()) + " cells of hspecI");
    if (fgiceC.size() != hspecC.size())
        throw Exception(IBH_EINVAL, "fgiceC: the plane does not hold the " + std::to_string(hspecC.size()) + " cells of hspecC");
    Etopo1IceGrids grids(hspecI, hspecC, hspecH);
    Etopo1Ice out;
    const size_t nI = (size_t)hspecI.size(), nH = hspecH ? (size_t)hspecH->size() : 0;
    out.FOCEAN1m.resize(nI); out.FGICE1m.resize(nI); out.ZICETOP1m.resize(nI); out.ZSOLG1m.resize(nI);
    std::vector<double> planes_h(4 * nH);
    check(ibh_etopo1_ice_host(grids.handle(), focean.data, zictop.data, zsolid.data, fgiceC.data, include_greenland ? 1 : 0, out.FOCEAN1m.data(),
                              out.FGICE1m.data(), out.ZICETOP1m.data(), out.ZSOLG1m.data(), nH ? planes_h.data() : nullptr, (int64_t)nH));
    if (nH) {
        out.FOCEANh.assign(planes_h.begin(), planes_h.begin() + (long)nH);
        out.FGICEh.assign(planes_h.begin() + (long)nH, planes_h.begin() + 2 * (long)nH);
        out.ZICETOPh.assign(planes_h.begin() + 2 * (long)nH, planes_h.begin() + 3 * (long)nH);
        out.ZSOLGh.assign(planes_h.begin() + 3 * (long)nH, planes_h.end());
    }
    return out;
}

// ---- modele/topo_base.cpp:20-221, :263-809 -----------------------------------------------------------
/** The hand-set cells of _make_topoO, 1-based (i, j) on the ocean grid: SET_TO = TO_LAND (:416-446) and TO_OCEAN (:449-494, set
    after the land cells), and the resets (:231-248) with their elevations.  Empty by default; the reference's own lists for g1qx1
    are the settings fixture tests/golden/make_topoo_g1qx1_cells.json. */
struct TopoOCells {
    std::vector<std::pair<int, int>> set_to_land, set_to_ocean;
    struct Reset { int i, j; double elev; };
    std::vector<Reset> resets;
};

/** What ibh_make_topoo_status reports: the reference's stderr warnings as counts. */
struct TopoOCounts {
    long FGICE_low = 0, FGICE_high = 0, FLAKE_reduced = 0, FGRND_range = 0, dZOCEN_nonpositive = 0, FLAKE_one = 0;
};

/** The grids, tables and scratch of one make_topoO (ibh_make_topoo_create) on the current HIP device: hspecI (the reference's
    g1mx1m) must nest in hspecO (g1qx1), whose sizes must be even; hspecS (g10mx10m) is the grid of FLAKES.  Owns a device
    handle: not copyable. */
class MakeTopoOGrids {
    ibh_make_topoo *h_ = nullptr;
public:
    HntrSpec const hspecI, hspecO, hspecS;
    MakeTopoOGrids(HntrSpec const &_hspecI, HntrSpec const &_hspecO, HntrSpec const &_hspecS, TopoOCells const &cells = TopoOCells())
        : hspecI(_hspecI), hspecO(_hspecO), hspecS(_hspecS) {
        std::vector<int32_t> land, ocean, rij;
        std::vector<double> relev;
        for (auto const &c : cells.set_to_land) { land.push_back(c.first); land.push_back(c.second); }
        for (auto const &c : cells.set_to_ocean) { ocean.push_back(c.first); ocean.push_back(c.second); }
        for (auto const &r : cells.resets) { rij.push_back(r.i); rij.push_back(r.j); relev.push_back(r.elev); }
        check(ibh_make_topoo_create(&h_, hspecI.im, hspecI.jm, hspecI.offi, hspecI.dlat, hspecO.im, hspecO.jm, hspecO.offi, hspecO.dlat, hspecS.im,
                                    hspecS.jm, hspecS.offi, hspecS.dlat, (int32_t)cells.set_to_land.size(), land.data(),
                                    (int32_t)cells.set_to_ocean.size(), ocean.data(), (int32_t)cells.resets.size(), rij.data(), relev.data()));
    }
    MakeTopoOGrids(MakeTopoOGrids const &) = delete;
    MakeTopoOGrids &operator=(MakeTopoOGrids const &) = delete;
    ~MakeTopoOGrids() { if (h_) ibh_make_topoo_destroy(h_); }
    ibh_make_topoo *handle() const { return h_; }
    /** The planes where they are, in HBM: a pure enqueue on `stream` (ibh_make_topoo_device); plane k of the
        IBH_MAKE_TOPOO_NPLANE outputs goes to d_planes + k * ld. */
    void run_device(const int16_t *d_FGICE1m, const int16_t *d_ZICETOP1m, const int16_t *d_ZSOLG1m, const int16_t *d_FOCEAN1m,
                    const double *d_FLAKES, double *d_planes, long ld, void *stream = nullptr) const {
        check(ibh_make_topoo_device(h_, d_FGICE1m, d_ZICETOP1m, d_ZSOLG1m, d_FOCEAN1m, d_FLAKES, d_planes, ld, stream));
    }
    /** Waits for `stream`; throws as make_topoO does for the first fatal cell, else returns the warning counts. */
    TopoOCounts status(void *stream = nullptr) const {
        int64_t s[IBH_MAKE_TOPOO_NSTATUS];
        check(ibh_make_topoo_status(h_, stream, s));
        return counts(s);
    }
    /** the status words as counts, or the reference's error (:85-89, :146-148) for the first cell in its order */
    TopoOCounts counts(const int64_t *s) const {
        const int64_t first = s[1] >= 0 && (s[3] < 0 || s[1] < s[3]) ? s[1] : s[3];
        if (first >= 0) {
            const bool ocean = first == s[1];
            const int J = (int)(first / hspecO.im) + 1, I = (int)(first % hspecO.im) + 1;
            const bool pole = J == 1 || J == hspecO.jm;
            const int J11 = (J - 1) * hspecI.jm / hspecO.jm + 1, J1M = J * hspecI.jm / hspecO.jm;
            const int I11 = (I - 1) * hspecI.im / hspecO.im + 1, I1M = pole ? hspecI.im : I * hspecI.im / hspecO.im;
            char buf[256];
            if (ocean)
                std::snprintf(buf, sizeof buf, "Ocean cell FOCEAN(%d,%d)=%g has no ocean area on 2-minute grid; I11,I1M,J11,J1M = %d,%d,%d,%d", I, J,
                              1., I11, I1M, J11, J1M);
            else
                std::snprintf(buf, sizeof buf, "Continental cell (%d,%d) has no continental area on 2-minute grid. (%d-%d, %d-%d)", I, J, I11, I1M,
                              J11, J1M);
            throw Exception(IBH_EINVAL, buf);
        }
        TopoOCounts c;
        c.FGICE_low = (long)s[4]; c.FGICE_high = (long)s[5]; c.FLAKE_reduced = (long)s[6]; c.FGRND_range = (long)s[7];
        c.dZOCEN_nonpositive = (long)s[8]; c.FLAKE_one = (long)s[9];
        return c;
    }
};

/** What _make_topoO returns (its ArrayBundle, :274-380), as arrays [jmO * imO] under the reference's names in its order. */
struct BaseTopoO {
    static const char *const *names() {
        static const char *const n[IBH_MAKE_TOPOO_NPLANE] = {"FOCEAN", "FLAKE", "FGRND", "FGICE", "FGICE_greenland", "ZATMO", "dZOCEN", "dZLAKE",
                                                             "dZGICE", "ZSOLDG", "ZICETOP", "ZLAND_MIN", "ZLAND_MAX", "ZSGLO", "ZLAKE", "ZGRND",
                                                             "ZSGHI", "FOCEANF", "FGICEF", "ZATMOF"};
        return n;
    }
    std::vector<std::vector<double>> planes;    // [IBH_MAKE_TOPOO_NPLANE][jmO * imO]
    TopoOCounts counts;
    std::vector<double> const &at(std::string const &name) const {
        for (int k = 0; k < IBH_MAKE_TOPOO_NPLANE; ++k)
            if (name == names()[k]) return planes[(size_t)k];
        throw Exception(IBH_EINVAL, "BaseTopoO: no plane named " + name);
    }
};

/** _make_topoO(FGICE1m, ZICETOP1m, ZSOLG1m, FOCEAN1m, FLAKES) (topo_base.cpp:263-809) from host arrays, with the grids as
    arguments (ibh_make_topoo_host): every plane crosses PCIe once in its own width.  Throws the reference's error for the first
    ocean cell without ocean area (:85) or continental cell without land (:146). */
inline BaseTopoO make_topoO(HntrSpec const &hspecI, HntrSpec const &hspecO, ArrayView<const int16_t> const &FGICE1m,
                        ArrayView<const int16_t> const &ZICETOP1m, ArrayView<const int16_t> const &ZSOLG1m,
                        ArrayView<const int16_t> const &FOCEAN1m, HntrSpec const &hspecS, ArrayView<const double> const &FLAKES,
                        TopoOCells const &cells = TopoOCells()) {
    if (FGICE1m.size() != hspecI.size() || ZICETOP1m.size() != hspecI.size() || ZSOLG1m.size() != hspecI.size() || FOCEAN1m.size() != hspecI.size())
        throw Exception(IBH_EINVAL, "FGICE1m / ZICETOP1m / ZSOLG1m / FOCEAN1m: a plane does not hold the " + std::to_string(hspecI.size()) +
                                        " cells of hspecI");
    if (FLAKES.size() != hspecS.size())
        throw Exception(IBH_EINVAL, "FLAKES: the plane does not hold the " + std::to_string(hspecS.size()) + " cells of hspecS");
    MakeTopoOGrids grids(hspecI, hspecO, hspecS, cells);
    const size_t nO = (size_t)hspecO.size();
    std::vector<double> flat((size_t)IBH_MAKE_TOPOO_NPLANE * nO);
    int64_t s[IBH_MAKE_TOPOO_NSTATUS];
    check(ibh_make_topoo_host(grids.handle(), FGICE1m.data, ZICETOP1m.data, ZSOLG1m.data, FOCEAN1m.data, FLAKES.data, flat.data(), (int64_t)nO, s));
    BaseTopoO out;
    out.counts = grids.counts(s);
    for (int k = 0; k < IBH_MAKE_TOPOO_NPLANE; ++k) out.planes.emplace_back(flat.begin() + (long)((size_t)k * nO), flat.begin() + (long)((size_t)(k + 1) * nO));
    return out;
}

// ---- modele/GCMRegridder_ModelE.hpp ------------------------------------------------------------------
/** make_hntrA (modele/hntr.cpp:232-241): the atmosphere grid is exactly twice as coarse as the ocean grid. */
inline HntrSpec make_hntrA(HntrSpec const &hntrO) {
    if ((hntrO.im % 2 != 0) || (hntrO.jm % 2 != 0))
        throw Exception(IBH_EINVAL, "Ocean grid must have even number of gridcells for im and jm (vs. " + std::to_string(hntrO.im) + " " +
                                        std::to_string(hntrO.jm) + ")");
    return HntrSpec(hntrO.im / 2, hntrO.jm / 2, hntrO.offi * 0.5, hntrO.dlat * 2.);
}

/** What GCMRegridder_ModelE::regrid_matrices returns (GCMRegridder_ModelE.cpp:487-571): AvI EvI AvX EvX IvA IvE XvA XvE, the
    aliases EAmvIp AAmvIp IpvEAm IpvAAm and the test matrices AOmvAAm / AAmvAOm, on the atmosphere grid.  Holds the O-grid
    matrices it is composed from (the reference's rm->tmp.take(rmO)). */
class RegridMatrices_ModelE : public RegridMatrices {
    ibh_modele_matrices *h_;
    std::unique_ptr<RegridMatrices_Dynamic> rmO_;
public:
    RegridMatrices_ModelE(ibh_modele_matrices *h, std::unique_ptr<RegridMatrices_Dynamic> &&rmO, RegridParams const &params)
        : RegridMatrices(params), h_(h), rmO_(std::move(rmO)) {}
    ~RegridMatrices_ModelE() { if (h_) ibh_modele_matrices_destroy(h_); }
    RegridMatrices_ModelE(RegridMatrices_ModelE const &) = delete;
    RegridMatrices_ModelE &operator=(RegridMatrices_ModelE const &) = delete;

    /** matrix_d(spec_name, dims, params): params.correctA is ignored, as compute_XAmvGp / compute_GpvXAm ignore it; params.sigma
        smooths IvA / IvE (the coupler's IvE, IceCoupler.cpp:461-463), is ignored by AvI EvI AvX EvX and refused for XvA / XvE
        (ibh_modele_matrices_matrix_d_sigma); dims may be pre-populated, are appended to and must outlive the result. */
    std::unique_ptr<linear::Weighted_Eigen> matrix_d(std::string const &spec_name, std::array<SparseSetT *, 2> dims,
                                                     RegridParams const &params) const {
        ibh_weighted *w = nullptr;
        check(ibh_modele_matrices_matrix_d_sigma(h_, spec_name.c_str(), dims[0] ? dims[0]->handle() : nullptr,
                                                 dims[1] ? dims[1]->handle() : nullptr, params.scale, params.sigma.data(), &w));
        return std::unique_ptr<linear::Weighted_Eigen>(new linear::Weighted_Eigen(w));
    }
    std::unique_ptr<linear::Weighted> matrix(std::string const &spec_name) const override {
        return matrix_d(spec_name, {{nullptr, nullptr}}, params());
    }
};

// ---- modele/merge_topo.hpp, modele/topo.hpp: the library functions behind global_AvE ---------------
enum { UI_UNUSED = 0, UI_LOCALICE = 1, UI_GLOBALICE = 2, UI_VGHOST = 3, UI_HGHOST = 4, UI_SEALAND = 5 };     // modele/grids.hpp:44-49

/** The base (global) ice EOpvAOp of the global_ecO file, UNSCALED, as COO arrays in sparse indices over `shape` (the order of
    the arrays is the order the merge reads them in), its elevation classes and the strides of its indexingHC. */
struct EOpvAOpBase {
    std::vector<double> hcdefs;
    std::vector<int64_t> iE, iO;
    std::vector<double> val;
    std::array<long, 2> shape = {{0, 0}};
    std::array<long, 2> indexingHC_strides = {{1, 0}};      // {1, 0}: {1, nO}
    bool empty() const { return hcdefs.empty() && val.empty(); }
};

/** EOpvAOpResult (modele/merge_topo.hpp): the merged EOpvAOp over {dimEOp, dimAOp} (unscaled; its Mw is wAOp), the first row
    key of the base ice, the elevation classes it stacks and indexingHC as strides plus extents. */
struct EOpvAOpResult {
    std::unique_ptr<SparseSetT> dimEOp;
    std::unique_ptr<linear::Weighted_Eigen> EOpvAOp;
    long offsetE = 0;
    std::vector<double> hcdefs;
    std::vector<int16_t> underice_hc;
    std::array<long, 2> indexingHC_strides = {{1, 0}};
    std::array<long, 2> indexingHC_extents = {{0, 0}};       // {nO, nhc}
};

/** compute_EOpvAOp_merged and, with squash_ecs, squash_ECs (modele/merge_topo.cpp:375-527; ibh_modele_merge_EOpvAOp).  gcmO: the
    ice sheets on the ocean grid; emIs: one elevmask per sheet, in sheet order (:405-411 builds each sheet's EvA from them).
    dimAOp is appended to and must outlive the result.  The reference's `errors` vector is never filled there and is not
    mirrored; squash_ECs is reached through the flag. */
inline EOpvAOpResult compute_EOpvAOp_merged(SparseSetT &dimAOp, EOpvAOpBase const &base, GCMRegridder_Standard const *gcmO,
                                            std::vector<ArrayView<const double>> const &emIs, bool use_global_ice, bool use_local_ice,
                                            bool squash_ecs) {
    if (emIs.size() != gcmO->nsheets())
        throw Exception(IBH_EINVAL, "compute_EOpvAOp_merged: " + std::to_string(emIs.size()) + " ice masks for " +
                                        std::to_string(gcmO->nsheets()) + " sheets");
    const long nO = (long)gcmO->nA();
    std::vector<std::unique_ptr<RegridMatrices_Dynamic>> rmOs;
    std::vector<const ibh_regrid_matrices *> hs;
    for (size_t k = 0; k < emIs.size(); ++k) {
        rmOs.push_back(gcmO->regrid_matrices((int)k, emIs[k], RegridParams(false, false, {{0., 0., 0.}})));
        hs.push_back(rmOs.back()->handle());
    }
    EOpvAOpResult ret;
    ret.dimEOp.reset(new SparseSetT);
    ret.hcdefs.resize(gcmO->nhc() + base.hcdefs.size());
    ret.underice_hc.resize(ret.hcdefs.size());
    const std::array<long, 2> sO = gcmO->indexingHC_strides();
    const long sAb = base.indexingHC_strides[1] ? base.indexingHC_strides[0] : sO[0];
    const long sHCb = base.indexingHC_strides[1] ? base.indexingHC_strides[1] : sO[1];
    ibh_weighted *w = nullptr;
    int64_t offsetE = 0, sA = 0, sHC = 0;
    int32_t nhc = 0;
    check(ibh_modele_merge_EOpvAOp(hs.data(), (int)hs.size(), nO, base.shape[0], base.shape[1], (int64_t)base.val.size(), base.iE.data(),
                                   base.iO.data(), base.val.data(), base.hcdefs.data(), (int32_t)base.hcdefs.size(), sAb, sHCb,
                                   use_global_ice, use_local_ice, squash_ecs, dimAOp.handle(), ret.dimEOp->handle(), &w, &offsetE, &nhc,
                                   ret.hcdefs.data(), ret.underice_hc.data(), &sA, &sHC));
    ret.EOpvAOp.reset(new linear::Weighted_Eigen(w));
    ret.offsetE = (long)offsetE;
    ret.hcdefs.resize((size_t)nhc); ret.underice_hc.resize((size_t)nhc);
    ret.indexingHC_strides = {{(long)sA, (long)sHC}};
    ret.indexingHC_extents = {{nO, (long)nhc}};
    return ret;
}

/** _compute_AAmvEAm_EIGEN (modele/topo.cpp:242-347; ibh_modele_AAmvEAm): AAmvEAm of a given EOpvAOp over {dimEOp, dimAOp} on the
    atmosphere grid make_hntrA(hntrO).  indexingHCO / indexingHCA: {stride_A, stride_HC}; nhc: the class extent of both.  dims =
    {dimAAm, dimEAm} may be pre-populated, are appended to and must outlive the result (nullptr: owned by the result). */
inline std::unique_ptr<linear::Weighted_Eigen> _compute_AAmvEAm_EIGEN(std::array<SparseSetT *, 2> dims, bool scale, double eq_rad,
                                                                      HntrSpec const &hntrO, std::array<long, 2> indexingHCO,
                                                                      std::array<long, 2> indexingHCA, int nhc,
                                                                      ArrayView<const double> const &foceanAOp,
                                                                      ArrayView<const double> const &foceanAOm,
                                                                      linear::Weighted_Eigen const &EOpvAOp, SparseSetT const &dimEOp,
                                                                      SparseSetT const &dimAOp) {
    if (foceanAOp.size() != foceanAOm.size()) throw Exception(IBH_EINVAL, "foceanAOp and foceanAOm differ in length");
    ibh_weighted *w = nullptr;
    check(ibh_modele_AAmvEAm(EOpvAOp.handle(), dimEOp.handle(), dimAOp.handle(), hntrO.im, hntrO.jm, hntrO.offi, hntrO.dlat, eq_rad, nhc,
                             indexingHCO[0], indexingHCO[1], indexingHCA[0], indexingHCA[1], foceanAOp.data, foceanAOm.data,
                             foceanAOp.size(), scale, dims[0] ? dims[0]->handle() : nullptr, dims[1] ? dims[1]->handle() : nullptr, &w));
    return std::unique_ptr<linear::Weighted_Eigen>(new linear::Weighted_Eigen(w));
}
/** _compute_AAmvEAm (topo.cpp:349-374): the same with sets of its own; M_coo / dim_to_sparse / wM / Mw of the result give the
    reference's to_tuple form.  nhc and the indexings are what make_topoa.cpp:131-135 passes: every merged class, in the order
    of the merged indexingHC on both grids. */
inline std::unique_ptr<linear::Weighted_Eigen> _compute_AAmvEAm(bool scale, double eq_rad, HntrSpec const &hntrO,
                                                                ArrayView<const double> const &foceanAOp,
                                                                ArrayView<const double> const &foceanAOm, EOpvAOpResult const &eo,
                                                                SparseSetT const &dimAOp) {
    const int nhc = (int)eo.hcdefs.size();
    const long nA = (long)hntrO.size() / 4;
    const bool hc_slowest = eo.indexingHC_strides[1] >= eo.indexingHC_strides[0];
    const std::array<long, 2> sA = hc_slowest ? std::array<long, 2>{{1, nA}} : std::array<long, 2>{{(long)nhc, 1}};
    return _compute_AAmvEAm_EIGEN({{nullptr, nullptr}}, scale, eq_rad, hntrO, eo.indexingHC_strides, sA, nhc, foceanAOp, foceanAOm, *eo.EOpvAOp,
                                  *eo.dimEOp, dimAOp);
}


// ---- modele/merge_topo.hpp, modele/topo.hpp: update_topo's field handling ------------------------------------
namespace topo_detail {
inline std::string cell(long c, int im) { return "(" + std::to_string(c % im + 1) + ", " + std::to_string(c / im + 1) + "): "; }
inline std::string g(double v) { char b[64]; snprintf(b, sizeof b, "%g", v); return b; }
/** sanity_check_land_fractions' strings (modele/topo.cpp:873-888) of the cells whose flag has `bit` set, j then i */
inline void land_fraction_errors(std::vector<uint32_t> const &flags, uint32_t bit, const double *focean, const double *flake,
                                 const double *fgrnd, const double *fgice, int im, std::vector<std::string> &errors) {
    for (size_t c = 0; c < flags.size(); ++c) {
        if (!(flags[c] & bit)) continue;
        const double all_frac = focean[c] + fgrnd[c] + flake[c] + fgice[c];
        errors.push_back(cell((long)c, im) + "FOCEAN(" + g(focean[c]) + ") + FGRND(" + g(fgrnd[c]) + ") + FLAKE(" + g(flake[c]) + ") + FGICE(" +
                         g(fgice[c]) + ")  = " + g(all_frac));
    }
}
}   // namespace topo_detail

/** merge_topoO (modele/merge_topo.cpp:84-360; ibh_modele_merge_topoO) with the reference's argument order; the planes are plain
    row-major arrays [jmO * imO] (iO = j * imO + i) where the reference has blitz arrays.  The nine leading planes are merged
    into in place; zland_minO2, zland_maxO2 and mergemaskOm2 are written.  hspecO names the ocean grid (the reference reads it from
    gcmO's grid spec).  paramsA is accepted and, as in the reference, only its sigma (which must be zero) matters: the builds
    use (scale, correctA) = (true, false) and (false, true).  eq_rad is accepted and unused.  errors receives the sanity
    checks' strings, check by check, then j, then i. */
inline void merge_topoO(double *foceanOp2, double *fgiceOp2, double *zatmoOp2, double *foceanOm2, double *flakeOm2, double *fgrndOm2,
                        double *fgiceOm2, double *zatmoOm2, double *zicetopO2, double *zland_minO2, double *zland_maxO2, int16_t *mergemaskOm2,
                        GCMRegridder_Standard const *gcmO, HntrSpec const &hspecO, RegridParams const &paramsA,
                        std::vector<ArrayView<const double>> const &emI_lands, std::vector<ArrayView<const double>> const &emI_ices,
                        double const eq_rad, std::vector<std::string> &errors) {
    if (emI_lands.size() != gcmO->nsheets() || emI_ices.size() != gcmO->nsheets())
        throw Exception(IBH_EINVAL, "merge_topoO: " + std::to_string(emI_lands.size()) + " land masks and " + std::to_string(emI_ices.size()) +
                                        " ice masks for " + std::to_string(gcmO->nsheets()) + " sheets");
    std::vector<std::unique_ptr<RegridMatrices_Dynamic>> keep;
    std::vector<const ibh_regrid_matrices *> lands, ices;
    const RegridParams params(false, true, paramsA.sigma);
    for (size_t k = 0; k < emI_ices.size(); ++k) {
        keep.push_back(gcmO->regrid_matrices((int)k, emI_lands[k], params));
        lands.push_back(keep.back()->handle());
        keep.push_back(gcmO->regrid_matrices((int)k, emI_ices[k], params));
        ices.push_back(keep.back()->handle());
    }
    double *planes[11] = {foceanOp2, fgiceOp2, zatmoOp2, foceanOm2, flakeOm2, fgrndOm2, fgiceOm2, zatmoOm2, zicetopO2, zland_minO2, zland_maxO2};
    static const char *const labels[9] = {"foceanOp2", "fgiceOp2", "zatmoOp2", "foceanOm2", "flakeOm2", "fgrndOm2", "fgiceOm2", "zatmoOm2",
                                          "zicetopO2"};
    std::vector<uint32_t> flags((size_t)hspecO.size());
    int64_t nerr = 0;
    check(ibh_modele_merge_topoO(lands.data(), (int32_t)lands.size(), ices.data(), (int32_t)ices.size(), hspecO.im, hspecO.jm, eq_rad, planes,
                                 mergemaskOm2, flags.data(), &nerr));
    if (!nerr) return;
    for (int bit = 0; bit < 18; ++bit)
        for (size_t c = 0; c < flags.size(); ++c)
            if (flags[c] >> bit & 1u)
                errors.push_back(topo_detail::cell((long)c, hspecO.im) + labels[bit % 9] + (bit < 9 ? "-0" : "") + " is NaN");
    topo_detail::land_fraction_errors(flags, 1u << 18, foceanOm2, flakeOm2, fgrndOm2, fgiceOm2, hspecO.im, errors);
}

/** make_topoA (modele/topo.cpp:581-855; ibh_modele_make_topoA) with the reference's argument order; planes are plain row-major
    arrays ([jm * im]; fhc3, elevE3, underice3: [(nhc + 1) * jmA * imA]); indexingHCA: {stride_A, stride_HC}; AAmvEAm is read in
    SPARSE indices through its two sets.  Returns the strings of sanity_check_land_fractions, then sanity_check_fhc. */
inline std::vector<std::string> make_topoA(const double *foceanOm2, const double *flakeOm2, const double *fgrndOm2, const double *fgiceOm2,
                                           const double *zatmoOm2, const double *zlakeOm2, const double *zicetopOm2, const double *zland_minOm2,
                                           const double *zland_maxOm2, const int16_t *mergemaskOm2, HntrSpec const &hspecO,
                                           HntrSpec const &hspecA, std::array<long, 2> indexingHCA, std::vector<double> const &hcdefs,
                                           std::vector<int16_t> const &underice_hc, linear::Weighted_Eigen const &AAmvEAm, double *foceanA2,
                                           double *flakeA2, double *fgrndA2, double *fgiceA2, double *zatmoA2, double *zlakeA2, double *zicetopA2,
                                           double *zland_minA2, double *zland_maxA2, int16_t *mergemaskA2, double *fhc3, double *elevE3,
                                           int16_t *underice3) {
    if (hcdefs.size() != underice_hc.size()) throw Exception(IBH_EINVAL, "make_topoA: hcdefs and underice_hc differ in length");
    const double *O[9] = {foceanOm2, flakeOm2, fgrndOm2, fgiceOm2, zatmoOm2, zlakeOm2, zicetopOm2, zland_minOm2, zland_maxOm2};
    double *A[9] = {foceanA2, flakeA2, fgrndA2, fgiceA2, zatmoA2, zlakeA2, zicetopA2, zland_minA2, zland_maxA2};
    const size_t nA = (size_t)hspecA.size(), nhc = hcdefs.size();
    std::vector<uint32_t> flags(nA);
    int64_t nerr = 0;
    check(ibh_modele_make_topoA(O, mergemaskOm2, hspecO.im, hspecO.jm, hspecO.offi, hspecO.dlat, hspecA.im, hspecA.jm, hspecA.offi, hspecA.dlat,
                                indexingHCA[0], indexingHCA[1], hcdefs.data(), underice_hc.data(), (int32_t)nhc, AAmvEAm.handle(), A, mergemaskA2,
                                fhc3, elevE3, underice3, flags.data(), &nerr));
    std::vector<std::string> errors;
    if (!nerr) return errors;
    topo_detail::land_fraction_errors(flags, 1u, foceanA2, flakeA2, fgrndA2, fgiceA2, hspecA.im, errors);
    for (size_t c = 0; c < nA; ++c) {
        if (!(flags[c] & 2u)) continue;
        double all_fhc = 0;
        for (size_t ihc = 0; ihc <= nhc; ++ihc) all_fhc += fhc3[ihc * nA + c];
        all_fhc += 1.0;
        errors.push_back(topo_detail::cell((long)c, hspecA.im) + "sum(FHC) = " + topo_detail::g(all_fhc - 1.0));
    }
    return errors;
}

/** What update_topo hands back: the TOPOA planes [jmA * imA] under TopoABundles' names, the elevation-class arrays
    [(nhc + 1) * jmA * imA], wEAm_base (the entries of AAmvEAm's Mw whose sparse index is >= offsetE) and offsetE. */
struct TopoA {
    std::vector<double> focean, flake, fgrnd, fgice, zatmo, hlake, zicetop, zland_min, zland_max, fhc, elevE;
    std::vector<int16_t> mergemask, underice;
    std::vector<std::pair<long, double>> wEAm_base;
    long offsetE = 0;
};
/** The TOPOO planes update_topo merges into, under topoo_bundle's names (modele/topo.cpp:384-474), each [jmO * imO]. */
struct TopoO {
    std::vector<double> FOCEANF, FGICEF, ZATMOF, FOCEAN, FLAKE, FGRND, FGICE, ZATMO, ZLAKE, ZICETOP, ZLAND_MIN, ZLAND_MAX;
    std::vector<int16_t> mergemask;
};
/** The planes of make_topoO that update_topo starts from. */
inline TopoO topoo(BaseTopoO const &b) {
    TopoO t;
    t.FOCEANF = b.at("FOCEANF"); t.FGICEF = b.at("FGICEF"); t.ZATMOF = b.at("ZATMOF"); t.FOCEAN = b.at("FOCEAN"); t.FLAKE = b.at("FLAKE");
    t.FGRND = b.at("FGRND"); t.FGICE = b.at("FGICE"); t.ZATMO = b.at("ZATMO"); t.ZLAKE = b.at("ZLAKE"); t.ZICETOP = b.at("ZICETOP");
    t.ZLAND_MIN = b.at("ZLAND_MIN"); t.ZLAND_MAX = b.at("ZLAND_MAX");
    return t;
}

/** The end of GCMCoupler_ModelE::update_topo (modele/GCMCoupler_ModelE.cpp:1090-1167) and couple()'s unit conversion
    (:1216-1228): the TOPOA planes packed into gcm_ivalss_s[ATOPO] and [ETOPO] on the device, from one pass over the masks
    (ibh_multivec_append_planes_many_host).  varsA: the ATOPO contract's variables, names of TopoABundles' 2-D planes; varsE: the
    ETOPO contract's, out of fhc elevE underice_d (the int16 plane, converted while it is packed); an unknown name throws
    IBH_ENOKEY, as the reference's .at(name) throws (:1114, :1147).  index_strides_E: indexingE as {stride of the cell j * im + i,
    stride of the class}.  mm / bb: the contract's scale and offset per variable (one empty: ones / zeros; both empty: no
    conversion).  The object owns mergemaskA0, the previous step's mask (:1017, :1167). */
class TopoPacker {
    std::vector<std::string> varsA_, varsE_;
    std::array<long, 2> stridesE_;
    std::vector<double> mmA_, bbA_, mmE_, bbE_;
    std::vector<int16_t> mergemaskA0_;
    bool have0_ = false;

    static void units(std::vector<double> &mm, std::vector<double> &bb, size_t nvar) {
        if (mm.empty() && bb.empty()) return;
        if (mm.empty()) mm.assign(nvar, 1.);
        if (bb.empty()) bb.assign(nvar, 0.);
        if (mm.size() != nvar || bb.size() != nvar)
            throw Exception(IBH_EINVAL, "TopoPacker: " + std::to_string(mm.size()) + " mm and " + std::to_string(bb.size()) + " bb for " +
                                            std::to_string(nvar) + " variables");
    }
    static const void *planeA(TopoA const &a, std::string const &name) {
        const char *names[9] = {"focean", "flake", "fgrnd", "fgice", "zatmo", "hlake", "zicetop", "zland_min", "zland_max"};
        std::vector<double> const *planes[9] = {&a.focean, &a.flake, &a.fgrnd, &a.fgice, &a.zatmo, &a.hlake, &a.zicetop, &a.zland_min, &a.zland_max};
        for (int k = 0; k < 9; ++k)
            if (name == names[k]) return planes[k]->data();
        throw Exception(IBH_ENOKEY, "TopoPacker: no TOPOA plane named '" + name + "'");
    }
    static const void *planeE(TopoA const &a, std::string const &name, int32_t &type) {
        type = name == "underice_d";
        if (name == "fhc") return a.fhc.data();
        if (name == "elevE") return a.elevE.data();
        if (name == "underice_d") return a.underice.data();
        throw Exception(IBH_ENOKEY, "TopoPacker: no TOPOE array named '" + name + "'");
    }
public:
    TopoPacker(std::vector<std::string> varsA, std::vector<std::string> varsE, std::array<long, 2> index_strides_E, std::vector<double> mmA = {},
               std::vector<double> bbA = {}, std::vector<double> mmE = {}, std::vector<double> bbE = {})
        : varsA_(std::move(varsA)), varsE_(std::move(varsE)), stridesE_(index_strides_E), mmA_(std::move(mmA)), bbA_(std::move(bbA)),
          mmE_(std::move(mmE)), bbE_(std::move(bbE)) {
        TopoA none;
        int32_t type;
        for (std::string const &n : varsA_) planeA(none, n);
        for (std::string const &n : varsE_) planeE(none, n, type);
        units(mmA_, bbA_, varsA_.size());
        units(mmE_, bbE_, varsE_.size());
    }
    std::vector<int16_t> const &mergemaskA0() const { return mergemaskA0_; }

    /** a: update_topo's / make_topoA's planes; nhc: the classes to pack (a.fhc, a.elevE and a.underice carry nhc + 1: the
        sea-land class is not packed, as in the reference).  run_ice = false (initialisation): the previous mask is this step's
        (:1017); afterwards this step's mask is kept (:1167).  The entries go behind those outA / outE hold; the conversion runs
        over ALL entries of each vector, as :1216-1228 does. */
    void pack(TopoA const &a, int nhc, bool run_ice, VectorMultivec &outA, VectorMultivec &outE) {
        const long ncell = (long)a.mergemask.size();
        if (run_ice && !have0_) throw Exception(IBH_EINVAL, "TopoPacker::pack: run_ice without a mask of an earlier step");
        if (run_ice && (long)mergemaskA0_.size() != ncell)
            throw Exception(IBH_EINVAL, "TopoPacker::pack: the previous mask has " + std::to_string(mergemaskA0_.size()) + " cells, this one " +
                                            std::to_string(ncell));
        std::vector<const void *> pA, pE;
        std::vector<int32_t> tE(varsE_.size(), 0);
        for (std::string const &n : varsA_) pA.push_back(planeA(a, n));
        for (size_t k = 0; k < varsE_.size(); ++k) pE.push_back(planeE(a, varsE_[k], tE[k]));
        const ibh_plane_pack packs[2] = {{outA.handle(), pA.data(), nullptr, (int32_t)pA.size(), 1, ncell, 1, ncell},
                                         {outE.handle(), pE.data(), tE.data(), (int32_t)pE.size(), nhc, ncell, stridesE_[0], stridesE_[1]}};
        check(ibh_multivec_append_planes_many_host(packs, 2, ncell, a.mergemask.data(), run_ice ? mergemaskA0_.data() : a.mergemask.data(),
                                                   nullptr));
        mergemaskA0_ = a.mergemask;
        have0_ = true;
        if (!mmA_.empty()) outA.affine(mmA_, bbA_);
        if (!mmE_.empty()) outE.affine(mmE_, bbE_);
    }
};

/** GCMRegridder_ModelE (GCMRegridder_ModelE.hpp:102-200): gcmO regrids between (AOp, EOp, Ip) on ModelE's ocean grid; this
    class hands out the matrices between (AAm, EAm, Ip).  The reference reads the ocean HntrSpec and the earth's radius from
    gcmO's grid spec; here the caller names them.  The base ice of the global_ecO file comes in memory (EOpvAOpBase); the file
    name must be empty (the zlib / NetCDF-4 containers are out of scope). */
class GCMRegridder_ModelE {
    HntrSpec hspecO_;
    double eq_rad_;
    EOpvAOpBase base_;
public:
    std::shared_ptr<GCMRegridder_Standard> const gcmO;

    /** The form with the base ice in memory (the global_ecO file's EOpvAOp_base and hcdefs, :458-480): what global_AvE merges in. */
    GCMRegridder_ModelE(EOpvAOpBase base, std::shared_ptr<GCMRegridder_Standard> const &_gcmO, HntrSpec const &hspecO, double eq_rad)
        : GCMRegridder_ModelE("", _gcmO, hspecO, eq_rad) { base_ = std::move(base); }

    GCMRegridder_ModelE(std::string const &_global_ecO, std::shared_ptr<GCMRegridder_Standard> const &_gcmO, HntrSpec const &hspecO,
                        double eq_rad)
        : hspecO_(hspecO), eq_rad_(eq_rad), gcmO(_gcmO) {
        if (!_global_ecO.empty()) throw Exception(IBH_ENOTIMPL, "GCMRegridder_ModelE: the global_ecO file is not supported");
        make_hntrA(hspecO);
        if ((unsigned long)hspecO.size() != gcmO->nA())
            throw Exception(IBH_EINVAL, "GCMRegridder_ModelE: hspecO has " + std::to_string(hspecO.size()) + " cells, gcmO " +
                                            std::to_string(gcmO->nA()));
    }
    unsigned int nhc() const { return gcmO->nhc(); }
    unsigned long nA() const { return gcmO->nA() / 4; }
    unsigned long nE() const { return gcmO->nE() / 4; }
    HntrSpec const &hspecO() const { return hspecO_; }
    HntrSpec hspecA() const { return make_hntrA(hspecO_); }
    double eq_rad() const { return eq_rad_; }
    /** hcdefs() (GCMRegridder_ModelE.cpp:468-471): the local classes, then the base ice's; underice(ihc) (.hpp:157) */
    std::vector<double> hcdefs() const {
        std::vector<double> h(gcmO->hcdefs());
        h.insert(h.end(), base_.hcdefs.begin(), base_.hcdefs.end());
        return h;
    }
    int underice(int ihc) const { return ihc < (int)gcmO->nhc() ? UI_LOCALICE : UI_GLOBALICE; }

    /** global_AvE (GCMRegridder_ModelE.cpp:579-628), composed the way the offline tools compose the library functions
        (make_merged_topoo.cpp:232-238, make_topoa.cpp:131-135,191-196): the merge with the BASE hcdefs, then
        _compute_AAmvEAm over every merged class.  emI_lands is accepted and, as in the reference, not used. */
    std::unique_ptr<linear::Weighted_Eigen> global_AvE(std::vector<ArrayView<const double>> const &emI_lands,
                                                       std::vector<ArrayView<const double>> const &emI_ices,
                                                       ArrayView<const double> const &foceanAOp, ArrayView<const double> const &foceanAOm,
                                                       bool scale, long &offsetE) const {
        (void)emI_lands;
        SparseSetT dimAOp;
        EOpvAOpResult eo = compute_EOpvAOp_merged(dimAOp, base_, gcmO.get(), emI_ices, !base_.empty(), true, false);
        offsetE = eo.offsetE;
        return _compute_AAmvEAm(scale, eq_rad_, hspecO_, foceanAOp, foceanAOm, eo, dimAOp);
    }


    /** GCMCoupler_ModelE::update_topo's body (modele/GCMCoupler_ModelE.cpp:1026-1082): merge_topoO with RegridParams(false, true,
        0), global_AvE(scale = true), wEAm_base, make_topoA.  topoo holds the merged planes afterwards.  Throws with the
        sanity-check strings when a check fails.  Reading the TOPOO file stays with the caller; the packing into VectorMultivecs
        (:1099-1167) is the overload below. */
    TopoA update_topo(TopoO &topoo, std::vector<ArrayView<const double>> const &emI_lands,
                      std::vector<ArrayView<const double>> const &emI_ices) const {
        const size_t nO = (size_t)hspecO_.size();
        for (std::vector<double> *p : {&topoo.FOCEANF, &topoo.FGICEF, &topoo.ZATMOF, &topoo.FOCEAN, &topoo.FLAKE, &topoo.FGRND, &topoo.FGICE,
                                       &topoo.ZATMO, &topoo.ZLAKE, &topoo.ZICETOP})
            if (p->size() != nO) throw Exception(IBH_EINVAL, "update_topo: a TOPOO plane has " + std::to_string(p->size()) + " cells, the ocean grid " +
                                                                 std::to_string(nO));
        topoo.ZLAND_MIN.resize(nO); topoo.ZLAND_MAX.resize(nO); topoo.mergemask.resize(nO);
        auto halt = [](std::vector<std::string> const &errors) {
            if (errors.empty()) return;
            std::string msg = "Errors in TOPO merging or regridding; halting!";
            for (std::string const &e : errors) msg += "\nERROR: " + e;
            throw Exception(IBH_EINVAL, msg);
        };
        std::vector<std::string> errors;
        merge_topoO(topoo.FOCEANF.data(), topoo.FGICEF.data(), topoo.ZATMOF.data(), topoo.FOCEAN.data(), topoo.FLAKE.data(), topoo.FGRND.data(),
                    topoo.FGICE.data(), topoo.ZATMO.data(), topoo.ZICETOP.data(), topoo.ZLAND_MIN.data(), topoo.ZLAND_MAX.data(),
                    topoo.mergemask.data(), gcmO.get(), hspecO_, RegridParams(false, true, {{0., 0., 0.}}), emI_lands, emI_ices, eq_rad_, errors);
        halt(errors);
        TopoA a;
        auto AAmvEAm = global_AvE(emI_lands, emI_ices, ArrayView<const double>(topoo.FOCEANF), ArrayView<const double>(topoo.FOCEAN), true,
                                  a.offsetE);
        std::vector<long> iE = AAmvEAm->dim_to_sparse(1);
        std::vector<double> const &Mw = AAmvEAm->Mw();
        for (size_t d = 0; d < iE.size(); ++d)
            if (iE[d] >= a.offsetE) a.wEAm_base.push_back(std::make_pair(iE[d], Mw[d]));
        const std::vector<double> hc = hcdefs();
        std::vector<int16_t> ui;
        for (int ihc = 0; ihc < (int)hc.size(); ++ihc) ui.push_back((int16_t)underice(ihc));
        const HntrSpec A = hspecA();
        const size_t nA = (size_t)A.size(), n3 = nA * (hc.size() + 1);
        const std::array<long, 2> sO = gcmO->indexingHC_strides();
        const std::array<long, 2> sA = sO[1] >= sO[0] ? std::array<long, 2>{{1, (long)nA}} : std::array<long, 2>{{(long)hc.size(), 1}};
        for (std::vector<double> *p : {&a.focean, &a.flake, &a.fgrnd, &a.fgice, &a.zatmo, &a.hlake, &a.zicetop, &a.zland_min, &a.zland_max})
            p->resize(nA);
        a.mergemask.resize(nA); a.fhc.resize(n3); a.elevE.resize(n3); a.underice.resize(n3);
        halt(make_topoA(topoo.FOCEAN.data(), topoo.FLAKE.data(), topoo.FGRND.data(), topoo.FGICE.data(), topoo.ZATMO.data(), topoo.ZLAKE.data(),
                        topoo.ZICETOP.data(), topoo.ZLAND_MIN.data(), topoo.ZLAND_MAX.data(), topoo.mergemask.data(), hspecO_, A, sA, hc, ui,
                        *AAmvEAm, a.focean.data(), a.flake.data(), a.fgrnd.data(), a.fgice.data(), a.zatmo.data(), a.hlake.data(),
                        a.zicetop.data(), a.zland_min.data(), a.zland_max.data(), a.mergemask.data(), a.fhc.data(), a.elevE.data(),
                        a.underice.data()));
        return a;
    }

    /** update_topo to its end (:1026-1167) with couple()'s unit conversion (:1216-1228): the planes as above, then packed by
        `packer` (which holds mergemaskA0 from step to step) behind the entries of gcm_ivalsA / gcm_ivalsE, every class of hcdefs(). */
    TopoA update_topo(TopoO &topoo, std::vector<ArrayView<const double>> const &emI_lands,
                      std::vector<ArrayView<const double>> const &emI_ices, bool run_ice, TopoPacker &packer, VectorMultivec &gcm_ivalsA,
                      VectorMultivec &gcm_ivalsE) const {
        TopoA a = update_topo(topoo, emI_lands, emI_ices);
        packer.pack(a, (int)hcdefs().size(), run_ice, gcm_ivalsA, gcm_ivalsE);
        return a;
    }

    /** make_agridA (GCMRegridder_ModelE.cpp:57-78): the realised atmosphere cells, first-seen in Hntr's stream order. */
    std::vector<long> agridA_dim(int sheet_index) const {
        std::vector<int64_t> a((size_t)nA());
        int32_t n = 0;
        check(ibh_modele_agridA(gcmO->ice_regridder(sheet_index)->handle(), hspecO_.im, hspecO_.jm, hspecO_.offi, hspecO_.dlat, &n, a.data()));
        return std::vector<long>(a.begin(), a.begin() + n);
    }

    /** regrid_matrices(sheet_index, foceanAOp, foceanAOm, elevmaskI, params) (GCMRegridder_ModelE.hpp:180-186): the arrays are
        copied.  The O-grid matrices are made with a zero sigma; params.sigma stays with the result, whose matrix(name) passes it
        per call (RegridMatrices_Dynamic.cpp:425-437). */
    std::unique_ptr<RegridMatrices_ModelE> regrid_matrices(int sheet_index, ArrayView<const double> const &foceanAOp,
                                                           ArrayView<const double> const &foceanAOm,
                                                           ArrayView<const double> const &elevmaskI,
                                                           RegridParams const &params = RegridParams()) const {
        if (foceanAOp.size() != foceanAOm.size()) throw Exception(IBH_EINVAL, "foceanAOp and foceanAOm differ in length");
        auto rmO = gcmO->regrid_matrices(sheet_index, elevmaskI, RegridParams(params.scale, params.correctA, {{0., 0., 0.}}));
        ibh_modele_matrices *h = nullptr;
        check(ibh_modele_matrices_create(rmO->handle(), hspecO_.im, hspecO_.jm, hspecO_.offi, hspecO_.dlat, eq_rad_, foceanAOp.data,
                                         foceanAOm.data, foceanAOp.size(), &h));
        return std::unique_ptr<RegridMatrices_ModelE>(new RegridMatrices_ModelE(h, std::move(rmO), params));
    }
};

/** GCMRegridder_WrapE (GCMRegridder_ModelE.hpp:206-251): a GCMRegridder_ModelE with the two ocean fractions it is used with
    (sparse O indexing; zero until set), so that regrid_matrices has GCMRegridder's signature. */
class GCMRegridder_WrapE {
public:
    std::unique_ptr<GCMRegridder_ModelE> gcmA;
    std::vector<double> foceanOp, foceanOm;

    explicit GCMRegridder_WrapE(std::unique_ptr<GCMRegridder_ModelE> &&_gcmA)
        : gcmA(std::move(_gcmA)), foceanOp(gcmA->gcmO->nA(), 0.), foceanOm(gcmA->gcmO->nA(), 0.) {}
    GCMRegridder_WrapE(std::unique_ptr<GCMRegridder_ModelE> &&_gcmA, std::vector<double> _foceanOp, std::vector<double> _foceanOm)
        : gcmA(std::move(_gcmA)), foceanOp(std::move(_foceanOp)), foceanOm(std::move(_foceanOm)) {}
    unsigned int nhc() const { return gcmA->nhc(); }
    unsigned long nA() const { return gcmA->nA(); }
    unsigned long nE() const { return gcmA->nE(); }
    std::unique_ptr<RegridMatrices_ModelE> regrid_matrices(int sheet_index, ArrayView<const double> const &elevmaskI,
                                                           RegridParams const &params = RegridParams()) const {
        return gcmA->regrid_matrices(sheet_index, ArrayView<const double>(foceanOp), ArrayView<const double>(foceanOm), elevmaskI, params);
    }
};
}   // namespace modele

// ---- pylib/icebin_cython.hpp:70-87 -----------------------------------------------------------
namespace cython {
/** new_regrid_matrices(gcm, sheet_name, elevmaskI, scale, correctA, sigma_x, sigma_y, sigma_z, conserve):
    like the reference (icebin_cython.cpp:215-236) looks the sheet up by name, checks the shape {nI}
    and ignores `conserve`.  The PyObject* becomes a plain (pointer, length). */
inline RegridMatrices *new_regrid_matrices(GCMRegridder_Standard const *gcm, std::string const &sheet_name,
                                           const double *elevmaskI, long elevmaskI_len, bool scale, bool correctA,
                                           double sigma_x, double sigma_y, double sigma_z, bool /*conserve*/) {
    auto sheet_index = gcm->sheet_index(sheet_name);
    return gcm->regrid_matrices((int)sheet_index, ArrayView<const double>(elevmaskI, elevmaskI_len),
                                RegridParams(scale, correctA, {{sigma_x, sigma_y, sigma_z}})).release();
}
/** RegridMatrices_matrix(cself, spec_name) (icebin_cython.cpp:195-198) */
inline linear::Weighted *RegridMatrices_matrix(RegridMatrices *cself, std::string const &spec_name) {
    return cself->matrix(spec_name).release();
}
/** new_GCMRegridder_WrapE(global_ecO, gcmO) (icebin_cython.cpp, used by GCMRegridder.to_modele, _icebin.pyx:128-147): gcmO is
    BORROWED -- the Python object that owns it is kept alive by the wrapper's Python object. */
inline modele::GCMRegridder_WrapE *new_GCMRegridder_WrapE(GCMRegridder_Standard *gcmO, modele::HntrSpec const &hspecO, double eq_rad) {
    std::shared_ptr<GCMRegridder_Standard> borrowed(gcmO, [](GCMRegridder_Standard *) {});
    return new modele::GCMRegridder_WrapE(
        std::unique_ptr<modele::GCMRegridder_ModelE>(new modele::GCMRegridder_ModelE("", borrowed, hspecO, eq_rad)));
}
inline void GCMRegridder_WrapE_set_focean(modele::GCMRegridder_WrapE *cself, const double *foceanAOp, const double *foceanAOm, long n) {
    cself->foceanOp.assign(foceanAOp, foceanAOp + n);
    cself->foceanOm.assign(foceanAOm, foceanAOm + n);
}
inline RegridMatrices *new_regrid_matrices_modele(modele::GCMRegridder_WrapE const *gcm, std::string const &sheet_name,
                                                  const double *elevmaskI, long elevmaskI_len, bool scale, bool correctA,
                                                  double sigma_x, double sigma_y, double sigma_z, bool /*conserve*/) {
    auto sheet_index = gcm->gcmA->gcmO->sheet_index(sheet_name);
    return gcm->regrid_matrices((int)sheet_index, ArrayView<const double>(elevmaskI, elevmaskI_len),
                                RegridParams(scale, correctA, {{sigma_x, sigma_y, sigma_z}})).release();
}
}   // namespace cython

}   // namespace icebin
