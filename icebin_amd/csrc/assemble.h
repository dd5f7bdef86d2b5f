// assemble.h -- entry points of the assembly path (assemble.hip).
#pragma once
#include <memory>

#include "common.h"
#include "prims.h"

namespace ibh {
// The forms one triplets -> CSR build took (build_csr_from_contributions), as ibh_selftest_triplets reports them; introspection only
enum { ORDER_IN_ORDER = 0, ORDER_PIECES = 1, ORDER_RADIX = 2 };     // the contributions were in order / pieces sorted in LDS / radix
enum { SRB_NOT_TRIED = 0, SRB_TAKEN = 1, SRB_DECLINED = 2 };        // per-row slots (a row over SRB_MAX declines, then the sort)
enum { OPT_NOT_TRIED = 0, OPT_HELD = 1, OPT_FAILED = 2 };           // the optimistic row-only sort and its check
enum { SEG_NONE = 0, SEG_THREAD = 1, SEG_WAVE = 2 };                // seg_sums: no launch / a thread / a wave per segment
enum { PTR_NONE = 0, PTR_SEARCH = 1, PTR_HEADS_FILL = 2 };          // rowptr_from_rows: every row searches / heads + fill
struct CsrBuildTrace { int order = ORDER_IN_ORDER, short_rows = SRB_NOT_TRIED, optimistic = OPT_NOT_TRIED, seg_form = SEG_NONE,
                       rowptr_form = PTR_NONE; };
// RegridMatrices_Dynamic::matrix_d (RegridMatrices_Dynamic.cpp:412-423) on device.
// comm: the sharded build (streamasm.inl) -- every rank of the communicator makes this call with the same arguments and gets the
// whole matrix; the ranks share the work when the build is one the streamed path serves, and build redundantly otherwise
bool assemble_matrix(const ibh_regrid_matrices *rm, const char *spec_name, ibh_sparse_set *dim0, ibh_sparse_set *dim1,
                     int scale, int correctA, const double sigma[3], ibh_weighted **out, bool fast_only = false, ibh_comm *comm = nullptr);
// the per-ice-cell class bytes of an elevmask (ibh_regrid_matrices::em_cls), made on `stream` when the streamed build will serve this grid
// (returns false otherwise); d_src != nullptr: read the elevations there and fill rm->elevmaskI (allocated) in the same pass
bool elevmask_classes(const ibh_regrid_matrices *rm, hipStream_t stream, const double *d_src = nullptr);
// n builds with the results of n matrix_d calls in order; independent ones run concurrently (assemble.hip assemble_batch)
void assemble_batch(const ibh_regrid_matrices *rm, int n, const char *const *specs, ibh_sparse_set *const *dim0,
                    ibh_sparse_set *const *dim1, const int32_t *scale, const int32_t *correctA, const double sigma[3],
                    ibh_weighted **out);
// Eigen setFromTriplets (to_eigen_M, eigen_types.cpp:9-34) on device: fills w's CSR from host COO.
void weighted_from_coo_device(ibh_weighted *w, int nrow, int ncol, int64_t n, const int32_t *row, const int32_t *col,
                              const double *val);
// setFromTriplets from DEVICE triplets (dense ids, input order) plus wM / Mw = sum(M, dim, '+'), enqueued on st (assemble.hip)
void weighted_from_device_triplets(ibh_weighted *w, int nrow, int ncol, int64_t n, const int32_t *drow, const int32_t *dcol,
                                   const double *dval, hipStream_t st);
// the same without the weights: only w's CSR (csrops.hip: the products and re-numbered copies)
void csr_from_device_triplets(ibh_weighted *w, int nrow, int ncol, int64_t n, const int32_t *drow, const int32_t *dcol,
                              const double *dval, hipStream_t st);
// compute_E1vE0c (e1ve0.cpp:55-106) on device; `out` comes with identity dims over nE.
void e1ve0_compute(int nsheets, const ibh_weighted *const *XuE1s, const ibh_weighted *const *XuE0s, int64_t nE, ibh_weighted *out);
// make_I2vX's products (global_ec.cpp:345-376): IvI2 = I2vI by columns (rows dense I); fills out's CSR, wM, Mw and flags
void i2vx_compute(const ibh_weighted *IvI2, const ibh_weighted *IvX, ibh_weighted *out);
// make_exchange_grid (gridgen/GridGen_Exchange.cpp:175-284) for a rectilinear XY ice grid (gridgen.hip)
void exgrid_generate(const ibh_exgrid_desc *d, ibh_exgrid *out);
// the same from polygons already in HBM (d_*: device arrays, ascending iA; edges on the host), through the streamed clip
void exgrid_generate_polys(int nx, int ny, const double *xedges, const double *yedges, int x_fastest, int npoly, const int32_t *d_polyptr,
                           const double *d_vx, const double *d_vy, const int64_t *d_iA, ibh_exgrid *out, hipStream_t st);
}  // namespace ibh
