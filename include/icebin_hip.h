/*
 * icebin_hip.h -- C-ABI of libicebin_hip.so, the MI355X (gfx950) implementation
 * of IceBin's conservative-regridding hot path.
 *
 * This is the drop-in boundary: plain C, opaque handles, plain
 * pointers and sizes, int status codes.  Every entry point replaces one piece
 * of the reference's C++ interface, cited as file:line under /root/reference.
 * The reference-side binding a maintainer would add is shown in INTEGRATION.md;
 * icebin_amd/host/ (C++) and the icebin_amd Python package (ctypes) are two users of it.
 *
 * Conventions
 *   - All functions return IBH_OK (0) or a negative IBH_E* code; the message is
 *     available from ibh_last_error() (thread-local).  This replaces
 *     (*icebin_error)(-1, fmt, ...) (slib/icebin/error.hpp:28-32): the host
 *     wrappers re-throw it as a C++ exception / Python RuntimeError.
 *   - Host arrays are borrowed for the duration of the call only.
 *   - "_d" = dense (renumbered) index, "_s" = sparse (native) index
 *     (sphinx/source/sparse_matrices.rst).  Dense ids are int32, sparse ids
 *     int64, values double (slib/icebin/eigen_types.hpp:16-18).
 *   - Fields ("variables") are stored field-major: A_b[k*lda + j], the
 *     blitz::Array<double,2>(nvar, n) layout of modele/icebin22m.cpp:142.
 *   - Single-threaded per handle; the stream argument is a hipStream_t passed
 *     as void* (NULL = the default stream).  The library uses the current HIP
 *     device of the calling thread; handles are bound to the device they were
 *     created on.
 *   - There is no CPU fallback: without a HIP device every compute entry
 *     point fails with IBH_ENODEVICE.
 */
#ifndef ICEBIN_HIP_H
#define ICEBIN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBH_OK          0
#define IBH_EINVAL     -1   /* bad argument / inconsistent sizes                       */
#define IBH_ENODEVICE  -2   /* no usable HIP device                                    */
#define IBH_EHIP       -3   /* a HIP runtime call failed                               */
#define IBH_ERANGE     -4   /* elevation above the last height class                   */
                            /*   (IceRegridder_L0.cpp:84-85)                           */
#define IBH_ENOTIMPL   -5   /* feature outside the hot-path scope                      */
#define IBH_ENOKEY     -6   /* unknown matrix name (regrids.at(), RegridMatrices_Dynamic.cpp:419) */

const char *ibh_last_error(void);
/* Library / device info.  ibh_device_count does not initialise the GPU context. */
int ibh_version(void);
int ibh_device_count(int *count);
int ibh_set_device(int device);

/* ------------------------------------------------------------------------- */
/* SparseSet: spsparse::SparseSet<long,int> (eigen_types.hpp:24; used as the
 * `dims` of every matrix, RegridMatrices_Dynamic.hpp:51-54).  Host-side value
 * type: dense -> sparse table in first-seen order.  Passed IN/OUT to matrix_d:
 * a pre-populated set is appended to, never reset (IceCoupler.cpp:366-371). */
typedef struct ibh_sparse_set ibh_sparse_set;
int ibh_sparse_set_create(int64_t sparse_extent, ibh_sparse_set **out);
int ibh_sparse_set_create_identity(int64_t n, ibh_sparse_set **out);          /* ibmisc id_sparse_set, modele/merge_topo.cpp:48 */
int ibh_sparse_set_from_array(int64_t sparse_extent, const int64_t *to_sparse, int32_t n, ibh_sparse_set **out);
int ibh_sparse_set_destroy(ibh_sparse_set *s);
int ibh_sparse_set_sparse_extent(const ibh_sparse_set *s, int64_t *out);
int ibh_sparse_set_dense_extent(const ibh_sparse_set *s, int32_t *out);
int ibh_sparse_set_to_sparse(const ibh_sparse_set *s, int64_t *out /* [dense_extent] */);
/* SparseSet::to_dense (-1 when the key is absent: in_sparse() == false) and add_dense (existing id or the
 * next one, first-seen order: AbbrGrid.cpp:108, IceCoupler.cpp:298), host side. */
int ibh_sparse_set_to_dense(const ibh_sparse_set *s, int64_t sparse, int32_t *dense);
int ibh_sparse_set_add_dense(ibh_sparse_set *s, int64_t sparse, int32_t *dense);

/* ------------------------------------------------------------------------- */
/* Exchange-grid generation: make_exchange_grid (slib/icebin/gridgen/GridGen_Exchange.cpp:175-284) for a
 * rectilinear ice grid in the projected plane (gridgen/searise_grid.cpp) under GCM-cell polygons
 * whose vertices the caller has projected to that plane (OGrid, GridGen_Exchange.cpp:120-166; simple, counter-
 * clockwise, 3 or more vertices, ascending iA).  A call whose polygons are all convex and of up to 16 vertices runs
 * the array clip; one polygon with more vertices or not convex (the host tests every polygon: turns of one sign,
 * edge directions winding once) sends the call to the streamed clip, which takes concave polygons.
 * ibh_set_tuning("gridgen_stream_clip", 0 | 1) forces one; forcing the array clip on a call it cannot take is
 * IBH_EINVAL naming the vertex count or the first polygon that is not convex.  Every non-empty overlap becomes one exchange cell
 * (iA, iI, area) with area = Cell::proj_area of the overlap polygon (Grid.cpp:42-70); cells come out
 * sorted by (iA, iI) like ExchangeGrid's constructor leaves them (AbbrGrid.cpp:10-21).  The result
 * stays in HBM; ibh_exgrid_get copies it out (the layout ibh_regridder_desc takes). */
typedef struct ibh_exgrid_desc {
    int32_t        nx, ny;          /* ice cells along x and y                                   */
    const double  *xedges, *yedges; /* [nx+1], [ny+1] cell edges, ascending                      */
    int32_t        x_fastest;       /* iI = iy*nx + ix when non-zero, else ix*ny + iy            */
    int32_t        npoly;           /* realised GCM cells                                        */
    const int32_t *polyptr;         /* [npoly+1] vertex ranges                                   */
    const double  *vx, *vy;         /* projected vertices                                        */
    const int64_t *iA;              /* [npoly] sparse atmosphere index, ascending                */
} ibh_exgrid_desc;
typedef struct ibh_exgrid ibh_exgrid;
int ibh_exgrid_generate(const ibh_exgrid_desc *desc, ibh_exgrid **out);
int ibh_exgrid_size(const ibh_exgrid *ex, int64_t *nX);
int ibh_exgrid_get(const ibh_exgrid *ex, int32_t *indices /* [2*nX] */, double *overlaps /* [nX] */);
int ibh_exgrid_destroy(ibh_exgrid *ex);

/* ------------------------------------------------------------------------- */
/* L1 ice grids: a triangle mesh carrying piecewise-linear fields (GridParameterization::L1; the reference serves them in
 * Python only, pylib/icebin/element_l1.py).  The mesh handle holds the vertices and the elements (three vertex ids each,
 * counter-clockwise) in HBM.  Creation checks on the device that every id lies in [0, nvert) and that every element has a
 * strictly positive signed area; otherwise IBH_EINVAL, and the message names the first offending element (the reference's
 * np.linalg.solve raises on a degenerate element, element_l1.py:27-51). */
typedef struct ibh_l1_mesh ibh_l1_mesh;
int ibh_l1_mesh_create(int32_t nvert, const double *vx, const double *vy, int32_t ntri, const int32_t *tri /* [3*ntri] */,
                       ibh_l1_mesh **out);
int ibh_l1_mesh_destroy(ibh_l1_mesh *mesh);
/* The exchange grid of a mesh: one cell per (GCM cell, element) overlap of positive area, holding (iA, iTri), the area and
 * the overlap polygon (counter-clockwise, 3..19 vertices, mesh coordinates), sorted by (iA, iTri).  Generated here
 * (make_exchange_grid, slib/icebin/gridgen/GridGen_Exchange.cpp:175-284, for triangles: polygons as in ibh_exgrid_desc --
 * convex, counter-clockwise, projected, 3..16 vertices, ascending iA.  The clip intersects half-planes, so more vertices,
 * a clockwise polygon, a reflex vertex or edges that wind more than once are IBH_EINVAL naming polygon and vertex; a turn
 * counts as reflex only beyond what rounding of the stored coordinates can do, 16 eps M (|e_k|_1 + |e_k+1|_1) with M the
 * polygon's largest |coordinate|, so sides with computed collinear points pass) or taken from the
 * caller as the reference's exgrid.cells carry it (element_l1.py:96-148 reads cellX.vertices, .i, .j): any order, sorted
 * here by (iA, iTri), ties in input order.  The area is Cell::proj_area (Grid.cpp:42-70) of the stored polygon, summed
 * with the polygon's vertex 0 as the origin.  Two calls on the same input give the same bytes. */
typedef struct ibh_l1_exgrid ibh_l1_exgrid;
int ibh_l1_exgrid_generate(const ibh_l1_mesh *mesh, int32_t npoly, const int32_t *polyptr /* [npoly+1] */, const double *px,
                           const double *py, const int64_t *iA /* [npoly] */, ibh_l1_exgrid **out);
int ibh_l1_exgrid_from_polygons(int64_t nX, const int32_t *iA, const int32_t *iTri, const int32_t *vptr /* [nX+1] */,
                                const double *qx, const double *qy, ibh_l1_exgrid **out);
int ibh_l1_exgrid_size(const ibh_l1_exgrid *ex, int64_t *nX, int64_t *nq /* polygon vertices in all; may be NULL */);
/* any of the arrays may be NULL */
int ibh_l1_exgrid_get(const ibh_l1_exgrid *ex, int32_t *indices /* [2*nX] */, double *areas /* [nX] */,
                      int32_t *vptr /* [nX+1] */, double *qx /* [nq] */, double *qy /* [nq] */);
int ibh_l1_exgrid_destroy(ibh_l1_exgrid *ex);
/* compute_AvI (element_l1.py:96-148): per exchange cell the integrals of the element's three basis functions over the
 * cell's polygon (integrate_subelement, element_l1.py:27-93, evaluated in the element's own frame), as three triplets
 * (iA, tri[3*iTri+k], value_k), summed per (row, column) in stream order -- ascending exchange cell, then k, the first
 * term assigned.  which = "AvI": rows over nA, columns over the mesh's vertices; "IvA": the transpose, same values.
 * Identity dims, wM = row sums over ascending column, Mw = column sums over ascending row, conservative; scale != 0:
 * M = diag(1/wM) M with wM and Mw unchanged (fA = (1/weightsA) AvI fI, element_l1.py:100-102).  There is no ice mask.
 * The terms variant copies out the 3*nX triplets themselves, before any summing. */
typedef struct ibh_weighted ibh_weighted;      /* declared with the Weighted entries below */
int ibh_l1_terms(const ibh_l1_exgrid *ex, const ibh_l1_mesh *mesh, int64_t nA, const char *which, int32_t *row, int32_t *col,
                 double *val);
int ibh_l1_matrix(const ibh_l1_exgrid *ex, const ibh_l1_mesh *mesh, int64_t nA, const char *which, int scale,
                  ibh_weighted **out);

/* ------------------------------------------------------------------------- */
/* Hntr: icebin::modele::Hntr (slib/icebin/modele/hntr.hpp:63-135, hntr.cpp:63-168), GISS's HNTR4 conservative
 * regridder between two lat-lon grids.  A grid is HntrSpec(im, jm, offi, dlat) (GridSpec.hpp:143-160): offi = cells
 * from the date line to the western edge of cell 1, dlat = minutes of latitude of a non-polar cell; fields are
 * stored i-fastest, flat index IJ = IA + im*(JA-1) (numpy shape (jm, im)).
 * ibh_hntr_create replaces Hntr(yp17, Bspec, Aspec, DATMIS) (hntr.cpp:63-79): the partition (partition_east_west,
 * partition_north_south, hntr.cpp:84-168) is computed on the host with libm sin and uploaded once.  Specs need
 * im, jm >= 1, dlat > 0, finite offi; a partition with an index outside [1, 2*imA] x [1, jmA] (the reference never
 * checks; column windows count modulo whole turns of imA, as the reference's IA = 1 + (IAREV-1) % imA does) is
 * IBH_EINVAL.  Allocates on the device: without one, IBH_ENODEVICE. */
typedef struct ibh_hntr ibh_hntr;
int ibh_hntr_create(ibh_hntr **out, int32_t imA, int32_t jmA, double offiA, double dlatA, int32_t imB, int32_t jmB,
                    double offiB, double dlatB, double datmis);
int ibh_hntr_destroy(ibh_hntr *h);
/* Hntr::regrid(WTA, A, B, mean_polar, wtm, wtb) (hntr.hpp:204-244, RegridAccum and Hntr::regrid :341-435) on nvar
 * fields at once: B[k*ldb + IJB] for k < nvar from A[k*lda + IJA] with the weight wtm*WTA + wtb, where WTA is one
 * plane shared by every field (wta_ld = 0) or one plane per field (WTA[k*wta_ld + IJA]).  Cells whose covered weight
 * is 0 get DATMIS; mean_polar replaces rows 1 and jmB by their mean (refused with jmB = 1, where the reference loops
 * forever).  Bitwise the reference's loop order for every nvar; the gaps between planes are left untouched.
 * _device: device pointers, a pure enqueue on `stream`.  _host: host arrays (copies over PCIe, synchronous). */
int ibh_hntr_regrid_device(const ibh_hntr *h, const double *dWTA, int64_t wta_ld, const double *dA, int32_t nvar, int64_t lda,
                           double *dB, int64_t ldb, int mean_polar, double wtm, double wtb, void *stream);
int ibh_hntr_regrid_host(const ibh_hntr *h, const double *WTA, int64_t wta_ld, const double *A, int32_t nvar, int64_t lda,
                         double *B, int64_t ldb, int mean_polar, double wtm, double wtb);
/* The same with typed planes and a constant weight, the instantiations of the reference's template
 * regrid<WeightT, SrcT, DestT> (hntr.hpp:385-391) that its callers use: regrid<double, int16_t, double> from the 1' ETOPO1
 * planes (etopo1_ice.cpp:22-26, topo_base.cpp:390-399, :646-663) and const_array(shape, c) as the weight.  Element codes;
 * 0 and 1 are the plane_type codes of ibh_multivec_append_planes_*: */
#define IBH_HNTR_F64 0      /* double */
#define IBH_HNTR_I16 1      /* int16_t */
#define IBH_HNTR_F32 2      /* float */
/* WTA holds elements of wta_type and A of a_type (all fields of a call share one type); wta_ld and lda count elements of the
 * plane's own type, so a plane base is aligned to its element only.  WTA == NULL selects the constant weight wta_const, a
 * plane that holds one number: wta_type and wta_ld are then ignored and no weight plane is read.  Every element becomes a
 * double (exactly) before it enters the chain wta = wtm*WTA + wtb; wt = FG*wta; WEIGHT += wt; VALUE += wt*A, so the result is
 * bitwise that of ibh_hntr_regrid_* on the widened planes, or on a plane filled with wta_const.  B stays double.  The checks of
 * ibh_hntr_regrid_* hold; a type code other than the three above is IBH_EINVAL and the message names it.
 * _device: a pure enqueue on `stream`.  _host: copies every plane over PCIe in its own width (never widened on the host),
 * synchronous. */
int ibh_hntr_regrid_typed_device(const ibh_hntr *h, const void *dWTA, int wta_type, int64_t wta_ld, double wta_const, const void *dA,
                                 int a_type, int32_t nvar, int64_t lda, double *dB, int64_t ldb, int mean_polar, double wtm, double wtb,
                                 void *stream);
int ibh_hntr_regrid_typed_host(const ibh_hntr *h, const void *WTA, int wta_type, int64_t wta_ld, double wta_const, const void *A,
                               int a_type, int32_t nvar, int64_t lda, double *B, int64_t ldb, int mean_polar, double wtm, double wtb);
/* What a regrid of nvar fields would launch, without launching anything: NV = fields per group (1 with per-field weights,
 * wta_ld != 0), L = chain lanes per wave, K = columns per chunk, lds_bytes = dynamic LDS of a workgroup.  wta_is_const != 0:
 * the constant weight (wta_type and wta_ld ignored).  nvar >= 1. */
int ibh_hntr_regrid_shape(const ibh_hntr *h, int32_t nvar, int wta_is_const, int wta_type, int64_t wta_ld, int a_type, int32_t *NV,
                          int32_t *L, int32_t *K, int64_t *lds_bytes);
/* The partition alone, host only (no device needed): SINA[jmA+1], SINB[jmB+1]; IMIN, IMAX, FMIN, FMAX [imB]
 * (IMAX(imB) already += imA, as hntr.cpp:116 leaves it); JMIN, JMAX, GMIN, GMAX [jmB].  Indices are the reference's,
 * 1-based; entry i of a per-column or per-row array belongs to IB or JB = i+1. */
int ibh_hntr_partition(int32_t imA, int32_t jmA, double offiA, double dlatA, int32_t imB, int32_t jmB, double offiB,
                       double dlatB, double *SINA, double *SINB, int32_t *IMIN, int32_t *IMAX, double *FMIN, double *FMAX,
                       int32_t *JMIN, int32_t *JMAX, double *GMIN, double *GMAX);

/* Hntr's matrix forms (hntr.hpp:205-338: Hntr::matrix with OverlapMatAccum / ScaledRegridMatAccum; hntr.cpp:33-52
 * make_dxyp).  The included B cells are visited in stream order: JB, then IB, ascending; inside a cell JA from JMIN(JB) to
 * JMAX(JB), then IAREV from IMIN(IB) to IMAX(IB), IA = 1 + (IAREV-1) % imA, term FG = F*G.  Every term becomes the entry
 * (IJB-1, IJA-1) with value FG * (1/WEIGHT) * (R2*dxyp(JB)) (IBH_HNTR_OVERLAP, R2 = eq_rad^2) or FG * (1/WEIGHT)
 * (IBH_HNTR_SCALED), WEIGHT = the cell's FG summed in stream order.  includeB: host byte mask [imB*jmB] (NULL: every cell),
 * what the reference's includeB functor or DimClip answers. */
#define IBH_HNTR_OVERLAP 0
#define IBH_HNTR_SCALED  1
/* make_dxyp (hntr.cpp:33-52): dxyp[j-1] = dLON*(sin(dLAT*(j-jm/2)) - sin(dLAT*(j-jm/2-1))), dLON = 2pi/im, dLAT = pi/jm,
 * jm/2 in integer division; offi and dlat play no part.  Host only, no device needed. */
int ibh_hntr_dxyp(int32_t im, int32_t jm, double *dxyp /* [jm] */);
/* The entries in stream order, for an arbitrary host accumulator (accum.add({iB, iA}, val)): iB, iA 0-based sparse.  With
 * iB, iA and val all NULL only *n is set (host only); otherwise the three arrays hold *n entries.  More than INT32_MAX
 * entries: IBH_EINVAL, with *n set, also when only asking for *n. */
int ibh_hntr_triplets(const ibh_hntr *h, int kind, double eq_rad, const uint8_t *includeB, int64_t *n, int32_t *iB,
                      int32_t *iA, double *val);
/* Transforms of MakeDenseEigenT (spsparse): ADD_DENSE numbers keys first-seen in stream order, TO_DENSE fails with
 * IBH_EINVAL on a key the set lacks, TO_DENSE_IGNORE_MISSING drops the entry.  An entry's indices are transformed in
 * order, B then A, and the entry stops at the first index dropped: when TO_DENSE_IGNORE_MISSING drops its B index, its A
 * index is neither numbered nor looked up. */
#define IBH_ADD_DENSE               0
#define IBH_TO_DENSE                1
#define IBH_TO_DENSE_IGNORE_MISSING 2
typedef struct ibh_weighted ibh_weighted;      /* declared with the Weighted entries below */
/* MakeDenseEigenT(overlap | scaled_regrid_matrix, {tB, tA}, {dimB, dimA}, transpose ? 'T' : '.') as a Weighted in HBM
 * (GCMRegridder_ModelE.cpp:92-121): transforms are given per generator index (B first, then A) whatever transpose is;
 * transpose only swaps the output (rows A, columns B).  Duplicate entries (a window wider than imA visits one A column twice)
 * are summed in stream order; columns ascend inside a row.  wM / Mw are the row / column sums, visited column-major
 * (sum(M, dim, '+')); conservative = 1, scaled = 0 for the overlap and 1 for the scaled matrix.
 * dimB / dimA are IN/OUT as in ibh_regrid_matrices_matrix_d and must outlive the result; NULL gives a fresh identity set over
 * the whole grid, owned by the result.  A set whose sparse extent is -1 takes the grid's size; any other extent is IBH_EINVAL,
 * as are a bad kind or transform and the same set on both sides.  More than INT32_MAX entries is IBH_EINVAL before anything
 * is allocated.  On any error *out is NULL and both sets are as they were: new keys are adopted only once the matrix is built.
 * With NULL or full identity dims and no transpose the CSR is built in place, without a sort; other dims go through a
 * first-seen numbering on the device and setFromTriplets. */
int ibh_hntr_matrix_d(const ibh_hntr *h, int kind, double eq_rad, const uint8_t *includeB, ibh_sparse_set *dimB, int tB,
                      ibh_sparse_set *dimA, int tA, int transpose, ibh_weighted **out);

/* ------------------------------------------------------------------------- */
/* Regridder: the state of GCMRegridder_Standard (GCMRegridder.hpp:207-302) and
 * one IceRegridder_L0 (IceRegridder.hpp:46-133) that the path reads, uploaded
 * to HBM once.  Replaces GCMRegridder_Standard::init + add_sheet
 * (GCMRegridder.cpp:65-86, GCMRegridder.hpp:353-367) and IceRegridder::init
 * (IceRegridder.cpp:93-119) for the data they keep. */
typedef struct ibh_regridder_desc {
    /* ExchangeGrid (AbbrGrid.hpp:40-89) */
    int64_t        nX;
    const int32_t *ex_indices;    /* [2*nX] interleaved (iA_s, iI_s), AbbrGrid.hpp:42 */
    const double  *ex_area;       /* [nX] overlaps, AbbrGrid.hpp:43                  */
    int64_t        nI;            /* ice-grid sparse extent (IceRegridder::nI)       */
    /* agridA (AbbrGrid.hpp:93-109) and IceRegridder::gridA_proj_area */
    int64_t        nA;            /* atmosphere sparse extent (GCMRegridder::nA)     */
    int32_t        nA_dense;
    const int64_t *A_to_sparse;   /* [nA_dense] agridA->dim                          */
    const double  *A_native_area; /* [nA_dense]                                      */
    const double  *A_proj_area;   /* [nA_dense] (== native when sproj=="", IceRegridder.cpp:106-108) */
    /* elevation classes */
    int32_t        nhc;
    const double  *hcdefs;        /* [nhc] ascending (GCMRegridder.hpp:253-256)      */
    int64_t        hc_stride_A;   /* indexingHC.tuple_to_index: iE = iA*stride_A + ihc*stride_HC */
    int64_t        hc_stride_HC;  /*   (icebin_cython.cpp:69 -> 1 and nA)            */
    int32_t        interp_style;  /* 0 Z_INTERP, 1 ELEV_CLASS_INTERP (IceRegridder.hpp:36-39) */
    /* agridI.centroid_xy (AbbrGrid.hpp:108-109) by SPARSE ice index, [2*nI] (x, y); only the smoother
     * (sigma != 0, smoother.cpp:69-99) reads it; may be NULL */
    const double  *I_centroid_xy;
} ibh_regridder_desc;

typedef struct ibh_regridder ibh_regridder;
int ibh_regridder_create(const ibh_regridder_desc *desc, ibh_regridder **out);
int ibh_regridder_destroy(ibh_regridder *rg);
int ibh_regridder_sizes(const ibh_regridder *rg, int64_t *nA, int64_t *nE, int64_t *nI, int64_t *nX, int32_t *nhc);
/* GCMRegridder::wA (GCMRegridder.hpp:305-315, icebin_cython.cpp:103-117):
 * out[nA] = fill, then out[A_to_sparse[id]] = native or projected area. */
int ibh_regridder_wA(const ibh_regridder *rg, int native, double fill, double *out /* [nA] */);

/* global_ec: a regridder built in place from Hntr's overlap under an ice mask (modele/global_ec.cpp:296-322 ExchAccum,
 * :384-432 new_gcmA_standard; gridgen/GridGen_LonLat.cpp:234-275 make_abbr_grid; GridSpec.cpp:80-122 make_grid_spec;
 * IceRegridder.cpp:93-119).  The Hntr handle has A = the ice grid and B = the GCM grid.  Every stream-order entry
 * (iB, iA, v) of its IBH_HNTR_OVERLAP form (WEIGHT summed over every term of the B cell) whose ice cell has a non-NaN
 * elevmaskI becomes the exchange cell (iA_gcm = iB, iI = iA, area = v), appended in stream order: sorted by GCM cell, and a
 * window wider than imA gives two cells for one ice column (ExchangeGrid::add appends).  agridA holds the GCM cells with at
 * least one exchange cell, ascending (ADD_DENSE in stream order); its native area restates make_abbr_grid from
 * make_grid_spec(hspecA, pole_caps = false) with the reference's degree quirk:
 *   native[id] = ((sin(latb[j+1]) - sin(latb[j])) * (lonb[i+1] - lonb[i])) * ((D2R * eq_rad) * eq_rad),
 * latb and lonb in DEGREES passed to sin, D2R = M_PI/180.  Projected area = native (no projection, IceRegridder.cpp:106-108),
 * so the correctA ratio is exactly 1, also where the quirk area is negative.  The GCM grid needs an even jm (the grid
 * spec of an odd jm has jm-1 rows); an odd im, which make_grid_spec refuses, is accepted. */
typedef struct ibh_hntr_regridder_desc {
    const ibh_hntr *hntr;          /* A = ice (hspecI), B = GCM (hspecA)                          */
    double          eq_rad;
    const double   *elevmaskI;     /* [nmask] = [imA*jmA]; NaN = no ice                           */
    int64_t         nmask;
    int32_t         mask_on_device;/* elevmaskI is a device pointer (read on `stream`)            */
    void           *stream;
    int32_t         nhc;
    const double   *hcdefs;        /* [nhc] ascending                                             */
    int64_t         hc_stride_A, hc_stride_HC;     /* as in ibh_regridder_desc; global_ec: 1, nA   */
    int32_t         interp_style;  /* 0 Z_INTERP, 1 ELEV_CLASS_INTERP                             */
} ibh_hntr_regridder_desc;
/* The number of exchange cells the mask keeps, in 64 bits, counted on the device; allocates nothing but a word. */
int ibh_hntr_exgrid_count(const ibh_hntr_regridder_desc *desc, int64_t *nX);
/* Count, scan and fill on the device; the regridder is what ibh_regridder_create builds from the same arrays (no
 * centroids).  INT32_MAX exchange cells or more (ibh_regridder_create's limit), nE = nA*nhc >= 2^31 or a mask of the wrong length is IBH_EINVAL before
 * anything is allocated.  dimA_out / dimI_out (may be NULL) must be empty sets; they receive the GCM cells of agridA
 * (ascending) and the ice cells in first-seen stream order (_dimA, _dimI of new_gcmA_standard).  On error *out is NULL and
 * both sets are as they were. */
int ibh_regridder_create_hntr(const ibh_hntr_regridder_desc *desc, ibh_sparse_set *dimA_out, ibh_sparse_set *dimI_out,
                              ibh_regridder **out);
/* Copy-outs of a regridder's state: the exchange grid (indices [2*nX] interleaved (iA, iI), overlaps [nX]; with both
 * NULL only *nX is set) and agridA ([nA_dense] each; *nA_dense is always set, and each non-NULL array is filled). */
int ibh_regridder_exgrid(const ibh_regridder *rg, int64_t *nX, int32_t *indices, double *overlaps);
int ibh_regridder_agridA(const ibh_regridder *rg, int32_t *nA_dense, int64_t *to_sparse, double *native_area, double *proj_area);

/* ------------------------------------------------------------------------- */
/* From grid specs: the realised cells of a GridSpec_LonLat (gridgen/GridGen_LonLat.cpp:109-232), projected to the ice
 * grid's plane with proj.4's `stere` (the only projection the reference's grid generators name), their native areas
 * (graticule_area_exact / polar_graticule_area_exact, :79-102) and projected areas (Cell::proj_area, Grid.cpp:42-71), all
 * computed on the device and kept in HBM; then the exchange grid and the regridder from them without a host copy.
 *
 * ibh_parse_sproj: "+proj=stere +lat_0=.. +lon_0=.. [+lat_ts=..] [+k=.. | +k_0=..] [+x_0=..] [+y_0=..] [+ellps=WGS84 |
 * +datum=WGS84 | +a=.. +b=.. | +R=..] [+units=m] [+no_defs]" (the leading '+' is optional).  Any other key or value is
 * IBH_EINVAL and the message names the key.  WGS84: a = 6378137, 1/f = 298.257223563; no ellipsoid given: WGS84. */
typedef struct ibh_stere_params {
    double  lat_0, lon_0;           /* degrees                                                   */
    double  lat_ts;                 /* degrees; read only when has_lat_ts                        */
    double  k_0, x_0, y_0;          /* scale factor; false easting / northing, metres            */
    double  a, b;                   /* semi-axes, metres; a == b: a sphere                       */
    int32_t has_lat_ts;
} ibh_stere_params;
int ibh_parse_sproj(const char *sproj, ibh_stere_params *out);
/* (lon, lat) in degrees -> (x, y) in metres for n points, host arrays, evaluated on the device with the function the cell
 * kernels use. */
int ibh_lonlat_project(const ibh_stere_params *proj, int64_t n, const double *lon, const double *lat, double *x, double *y);

typedef struct ibh_lonlat_cells_desc {
    int32_t        nlonb, nlatb;    /* entries of lonb (= nlon + 1) and of latb                  */
    const double  *lonb, *latb;     /* cell boundaries, degrees, ascending                       */
    int32_t        indices[2];      /* {0,1}: index = i*nlat + j; {1,0}: index = j*nlon + i      */
    int32_t        south_pole, north_pole;       /* the grid has that cap                        */
    int32_t        points_in_side;  /* >= 1: points per side of a cell (and per lonb interval of a cap) */
    double         eq_rad;          /* radius for the native areas, metres                       */
    int64_t        nrealised;
    const int64_t *realised;        /* [nrealised] sparse indices of the cells to realise, strictly ascending */
    const ibh_stere_params *proj;
    int32_t        keep_lonlat;     /* also keep the unprojected vertices (tests)                */
} ibh_lonlat_cells_desc;
/* nlat = nlatb - 1 + south_pole + north_pole; an ordinary cell (ilon, ilat) has i = ilon, j = ilat + south_pole; the south
 * cap has index 0 and the north cap nlat*nlon + nlon - 1 (pole.j = nlat(), :180-182: one row past the last), so the sparse
 * extent nA is nlon*nlat without a north cap and nlon*(nlat + 1) with one.  A realised index that is no cell of the spec, an
 * unsorted list, points_in_side < 1 or non-ascending boundaries is IBH_EINVAL; on error *out is NULL. */
typedef struct ibh_lonlat_cells ibh_lonlat_cells;
int ibh_lonlat_cells_create(const ibh_lonlat_cells_desc *desc, ibh_lonlat_cells **out);
int ibh_lonlat_cells_size(const ibh_lonlat_cells *cells, int32_t *ncell, int64_t *nvert, int64_t *nA);
/* Copy-out (tests): every non-NULL array is filled.  iA, native_area, proj_area [ncell]; polyptr [ncell+1]; vx, vy [nvert];
 * lon, lat [nvert] only for a handle created with keep_lonlat. */
int ibh_lonlat_cells_get(const ibh_lonlat_cells *cells, int64_t *iA, int32_t *polyptr, double *vx, double *vy, double *native_area,
                         double *proj_area, double *lon, double *lat);
int ibh_lonlat_cells_destroy(ibh_lonlat_cells *cells);
/* ibh_exgrid_generate under these cells: the polygons are read where they lie, through the streamed clip (no vertex limit). */
int ibh_exgrid_generate_lonlat(const ibh_lonlat_cells *cells, int32_t nx, int32_t ny, const double *xedges, const double *yedges,
                               int32_t x_fastest, ibh_exgrid **out);
/* The regridder of that exchange grid, what ibh_regridder_create builds from the copied-out arrays: agridA = the realised
 * cells (ascending) with their native areas, A_proj_area their projected areas, nA as above, nI = nx*ny, I_centroid_xy the
 * cell centres (.5 * (e[k] + e[k+1])).  dimA_out (may be NULL) must be an empty set and receives the realised cells.  On error
 * *out is NULL and dimA_out is as it was. */
typedef struct ibh_lonlat_regridder_desc {
    const ibh_lonlat_cells *cells;
    int32_t        nx, ny;
    const double  *xedges, *yedges; /* [nx+1], [ny+1] ice-cell edges, ascending                  */
    int32_t        x_fastest;
    int32_t        nhc;
    const double  *hcdefs;          /* [nhc] ascending                                           */
    int64_t        hc_stride_A, hc_stride_HC;    /* as in ibh_regridder_desc                     */
    int32_t        interp_style;    /* 0 Z_INTERP, 1 ELEV_CLASS_INTERP                           */
} ibh_lonlat_regridder_desc;
int ibh_regridder_create_lonlat(const ibh_lonlat_regridder_desc *desc, ibh_sparse_set *dimA_out, ibh_regridder **out);

/* ------------------------------------------------------------------------- */
/* Weighted: ibmisc::linear::Weighted_Eigen {dims, M, wM, Mw, conservative,
 * scaled} (RegridMatrices_Dynamic.cpp:63-65,100,115,123,421).  M lives in HBM
 * as CSR (int32 rowptr/colind, f64 values, columns ascending inside a row). */
typedef struct ibh_weighted ibh_weighted;

/* RegridMatrices: GCMRegridder_Standard::regrid_matrices
 * (RegridMatrices_Dynamic.cpp:334-402; Cython shim new_regrid_matrices,
 * icebin_cython.cpp:215-236).  Copies elevmaskI (length must equal nI) to HBM.  For a grid of 2^20
 * exchange cells and more the call also derives one byte per ice cell from its elevation (masked /
 * beyond the last elevation class / first class and class count): every matrix built from this
 * object reads that byte where only the mask or the class pattern matters (36 M ice cells: 0.22 ms
 * for copy + bytes against 0.13 ms for the copy alone; smaller grids make the bytes when a build
 * first asks).  Results are unaffected. */
typedef struct ibh_regrid_matrices ibh_regrid_matrices;
int ibh_regrid_matrices_create(const ibh_regridder *rg, const double *elevmaskI, int64_t n,
                               int scale, int correctA, const double sigma[3],
                               ibh_regrid_matrices **out);
/* Same with the elevation mask already in HBM (an ice model that runs on the GPU: the host form
 * moves 8*nI bytes over PCIe per coupling step, 4 ms at 1 km).  Copied device-to-device on `stream`,
 * which is synchronised before returning. */
int ibh_regrid_matrices_create_device(const ibh_regridder *rg, const double *d_elevmaskI, int64_t n,
                                      int scale, int correctA, const double sigma[3], void *stream,
                                      ibh_regrid_matrices **out);
int ibh_regrid_matrices_destroy(ibh_regrid_matrices *rm);

/* RegridMatrices_Dynamic::matrix_d(spec, dims, params) (:412-423).
 * spec in {AvI IvA AvX XvA EvI IvE EvX XvE EvA AvE}.  dim0/dim1 are IN/OUT;
 * they must outlive the result unless passed as NULL, in which case fresh
 * sets owned by the result are used (== RegridMatrices_Dynamic::matrix, :425-437). */
int ibh_regrid_matrices_matrix_d(const ibh_regrid_matrices *rm, const char *spec,
                                 ibh_sparse_set *dim0, ibh_sparse_set *dim1,
                                 int scale, int correctA, const double sigma[3],
                                 ibh_weighted **out);
/* The matrices of one coupling step in ONE call (IceCoupler.cpp:361-468 builds EvI, AvI, IvE, XvE per step with a
 * shared dimE and identity dimI / dimX): the results -- matrices and dims -- are those of n ibh_regrid_matrices_matrix_d
 * calls in the order given (sigma[3], or NULL for no smoothing, applies to all); builds that cannot influence each
 * other run concurrently on the library's worker threads and their own streams, a build that reads a set an earlier
 * one numbers waits for it.  On error nothing is returned (out[] all NULL) and the first failing job's status is. */
int ibh_regrid_matrices_matrix_batch(const ibh_regrid_matrices *rm, int32_t n, const char *const *specs,
                                     ibh_sparse_set *const *dim0, ibh_sparse_set *const *dim1,
                                     const int32_t *scale, const int32_t *correctA, const double sigma[3],
                                     ibh_weighted **out /* [n] */);
/* RegridMatrices::matrix(spec) (RegridMatrices.hpp:60-61): own dims, params of rm. */
int ibh_regrid_matrices_matrix(const ibh_regrid_matrices *rm, const char *spec, ibh_weighted **out);

/* Load a Weighted from dense-indexed triplets: to_eigen_M (eigen_types.cpp:9-34)
 * / ibmisc.nc_read_weighted (matrix_formats.rst:139-147).  Duplicates are
 * summed in input order (Eigen setFromTriplets).  dims are identity. */
int ibh_weighted_from_coo(int32_t nrow, int32_t ncol, int64_t nnz,
                          const int32_t *row, const int32_t *col, const double *val,
                          const double *wM /* [nrow] */, const double *Mw /* [ncol] */,
                          int conservative, int scaled, ibh_weighted **out);
/* Same from host CSR arrays (columns need not be sorted; no duplicate merging). */
int ibh_weighted_from_csr(int32_t nrow, int32_t ncol, const int32_t *rowptr,
                          const int32_t *colind, const double *val,
                          const double *wM, const double *Mw,
                          int conservative, int scaled, ibh_weighted **out);
int ibh_weighted_destroy(ibh_weighted *w);

/* compute_E1vE0c (slib/icebin/e1ve0.cpp:55-106): the matrix that carries fields on last step's elevation
 * grid (E0) to this step's (E1), E1vE0c = diag(1/sum_sheets Mw(XuE1)) * sum_sheets[E1uX * (XvE0 - XvE1)].
 * XuE1s / XuE0s: one unscaled XvE matrix per ice sheet for the new and the old elevation mask
 * (IceCoupler.cpp:464-468 builds them; dims[0] over the exchange grid, dims[1] over E).  The result is a
 * Weighted over the SPARSE E space (identity dims of extent nE, rows iE1, columns iE0, entries sorted
 * by (iE1, iE0), duplicates summed; wM = Mw = 1): the reference returns the same tuples as a TupleList. */
int ibh_e1ve0_compute(int32_t nsheets, const ibh_weighted *const *XuE1s, const ibh_weighted *const *XuE0s,
                      int64_t nE, ibh_weighted **out);

/* make_I2vX (modele/global_ec.cpp:345-376): IvX (IvE or IvA, dims {dimI, dimX}) mapped onto a coarser lat-lon grid I2.
 * hIvI2 is Hntr(hspecI as B, hspecI2 as A); includeI the host byte mask [nI] (!isnan(elevmaskI); NULL: every cell).
 *   I2vI = MakeDenseEigenT(overlap(eq_rad, includeI), {TO_DENSE_IGNORE_MISSING, ADD_DENSE}, {dimI, dimI2}, 'T')
 *   M    = (I2vI * diag(1/IvX.wM)) * IvX.M        left factor rounded once per element; every output entry sums its terms
 *                                                 over the dense I index ascending, the first assigned (Eigen's
 *                                                 conservative sparse product)
 *   wM   = (I2vI * diag(sum(I2vI, 1, '-'))) * IvX.wM   column sums of I2vI (rows ascending, from 0), inverted; the product
 *                                                 sums over I ascending from 0
 *   Mw   = IvX.Mw; conservative from IvX, scaled = 0; dims {dimI2, IvX's dims[1]}.
 * dimI2 (IN/OUT, must outlive the result; NULL: a fresh set owned by the result) is numbered first-seen; IvX's dims[1] is
 * shared when IvX does not own it, else copied.  A grid or mask that does not match IvX's ice dim is IBH_EINVAL; on any
 * error *out is NULL and dimI2 is as it was. */
int ibh_weighted_make_I2vX(const ibh_weighted *IvX, const ibh_hntr *hIvI2, double eq_rad, const uint8_t *includeI, int64_t nincl,
                           ibh_sparse_set *dimI2, ibh_weighted **out);

/* ------------------------------------------------------------------------- */
/* global_ec in chunks: main() of modele/global_ec.cpp below "Check that I grid fits neatly into O grid" (:752-893) and
 * combine_chunks of modele/combine_global_ec.cpp (:94-262).  The ocean grid O and the ice grid I nest: imI % imO == 0 and
 * jmI % jmO == 0, else IBH_EINVAL "Hntr grid (%dx%d) must be an even multiple of (%dx%d)" (:752-760); mult_i = imI / imO,
 * mult_j = jmI / jmO, O cell k = jO * imO + iO owns the ice cells jI in [jO * mult_j, (jO + 1) * mult_j), iI in
 * [iO * mult_i, (iO + 1) * mult_i).  Every entry validates its arguments before it touches a device. */
typedef struct ibh_global_ec_scan ibh_global_ec_scan;
/* The ice scan (:762-813).  fgiceI / elevI: the int16 planes FGICE1m / ZICETOP1m [jmI, imI] (plane_type must be
 * IBH_HNTR_I16, nplane = imI * jmI), on the host (on_device = 0: uploaded once in their own width and kept by the scan) or
 * on the device (on_device = 1: read on `stream`, and they outlive the scan).  Left on the device:
 *   fgiceO[nO]  = Hntr(17.17, hspecO, hspecI).regrid(const 1.0, fgiceI) (:778-780), bitwise ibh_hntr_regrid_typed_device
 *   nice[nO]    = the number of cells with fgiceI != 0 in the O cell's tile (the count of :881-884)
 *   elevI_range = {min, max} of elevI over the cells with fgiceI != 0, from {10000, -10000} (:805-813)
 * nice and the range come from one pass over both planes with integer atomics, so they are exact.  Waits for the device. */
int ibh_global_ec_scan_create(int32_t imO, int32_t jmO, double offiO, double dlatO, int32_t imI, int32_t jmI, double offiI, double dlatI,
                              const void *fgiceI, const void *elevI, int64_t nplane, int plane_type, int on_device, void *stream,
                              ibh_global_ec_scan **out);
/* Frees what the scan holds of :763-803: the regridded fgiceO, the counts, and the copies of host planes (never the caller's). */
int ibh_global_ec_scan_destroy(ibh_global_ec_scan *s);
/* What the scan holds of :762-816; every output may be NULL.  d_fgiceO / d_nice: the device arrays fgiceO (:778-780) and the tile
 * counts (:881-884), valid as long as the scan; elevI_range[2] (:805-813); fgiceO / nice: host copies [nO]. */
int ibh_global_ec_scan_get(const ibh_global_ec_scan *s, const double **d_fgiceO, const int32_t **d_nice, int16_t *elevI_range, double *fgiceO,
                           int32_t *nice);
/* fgiceO (:778-780) and the tile counts (:881-884) copied device to device into the caller's arrays [nO] (either may be NULL), on
 * `stream`; only enqueues. */
int ibh_global_ec_scan_copy_device(const ibh_global_ec_scan *s, double *d_fgiceO, int32_t *d_nice, void *stream);
/* ec_range = {ec_skip * floor(min / ec_skip), ec_skip * ceil(max / ec_skip)} in double (:815-816).  Host only. */
int ibh_global_ec_ec_range(const int16_t *elevI_range, double ec_skip, double *ec_range /* [2] */);
/* The chunk plan (:863-893) over c[k] = fgiceO[k] != 0 ? nice[k] : 0, k row-major.  Chunk n starts where chunk n - 1 ended and
 * ends, exclusive, at the first k >= start whose running sum of c from start, that cell included, is >= chunk_size (the cell
 * itself goes to the next chunk -- goto endscan2 does not advance iO -- while its ice is in this chunk's reported nice), or at
 * nO.  chunks[5 * n] = {chunkno, jO0, iO0, jO1, iO1}, the last bound (jmO, 0); nice[n] the reported count; *nchunks the number
 * of chunks there are, of which the first min(cap, *nchunks) are written (chunks / nice may be NULL).  No ice: one chunk with
 * nice = 0.  chunk_size must exceed mult_i * mult_j, else IBH_EINVAL: a full O cell would reach a smaller chunk_size on its
 * own, the chunk would end where it starts, and the reference loops forever.  The masking and the scan run on the device and
 * the nO + 1 sums are read back once per scan; the walk is host code. */
int ibh_global_ec_chunk_plan(ibh_global_ec_scan *s, int64_t chunk_size, int32_t cap, int32_t *chunks, int64_t *nice, int32_t *nchunks);
/* The walk of :863-893 over host counts c[nO] (each in [0, mult_i * mult_j]; c[k] stands for the count of :881-884 where
 * fgiceO(jO, iO) != 0, :878, and is 0 elsewhere), with the same rules and outputs.  Host only, no device needed. */
int ibh_global_ec_chunk_plan_counts(int32_t imO, int32_t jmO, int32_t mult_i, int32_t mult_j, const int32_t *counts, int64_t chunk_size,
                                    int32_t cap, int32_t *chunks, int64_t *nice, int32_t *nchunks);
/* A chunk's mask (:818-855) into the device array d_elevmaskI [nI]: (double)elevI where the cell's O cell k lies in
 * [jO0 * imO + iO0, jO1 * imO + iO1), fgiceO[k] != 0 and fgiceI != 0, else NaN.  One launch on `stream`; only enqueues. */
int ibh_global_ec_chunk_mask(const ibh_global_ec_scan *s, int32_t jO0, int32_t iO0, int32_t jO1, int32_t iO1, double *d_elevmaskI,
                             int64_t nmask, void *stream);
/* elevmaskI of :818-855 for the same chunk into the HOST array elevmaskI [nI] (a device array of the call's own, one download).
 * Waits for the device. */
int ibh_global_ec_chunk_mask_host(const ibh_global_ec_scan *s, int32_t jO0, int32_t iO0, int32_t jO1, int32_t iO1, double *elevmaskI,
                                  int64_t nmask);
/* combine_chunks (combine_global_ec.cpp:94-262) for one matrix BvA: mats[c] is chunk c's UNSCALED matrix (a scaled one is
 * IBH_EINVAL) with its weights wM_c / Mw_c; its sets dimB_c / dimA_c are the first nrow / ncol entries of the handle's own
 * dims, or -- with dims_host -- the host arrays dims_host[2 * c], dims_host[2 * c + 1] over the sparse extents
 * extents[2 * c], extents[2 * c + 1] (matrices read back from files); such an array that names a sparse index twice is
 * IBH_EINVAL, as a set cannot.  Chunks whose sparse extents disagree are IBH_EINVAL.
 *   dimB_out = the first-seen numbering of the stream dimB_c[i], c ascending then i < len(wM_c) ascending; dimA_out alike
 *   wM_out[d] = the sum from 0.0, in chunk order, of the wM_c[i] that name d (:197-200); Mw_out alike (:247-249)
 *   sM_s      = 1 / the same sum (:152-174)
 *   stream    = (dimB_c[row], dimA_c[col], scale ? v * sM_s[dimB_c[row]] : v), chunks in order, a chunk's entries in stored
 *               row-major order (:217-227); written to the host arrays stream_iB / stream_iA / stream_val [sum of nnz_c]
 *               (all three or none), the reference's contract and the base of ibh_modele_merge_EOpvAOp
 *   *out      = setFromTriplets of that stream over {dimB_out, dimA_out} (duplicates across chunks summed in stream order),
 *               with wM_out / Mw_out as its weights, scaled = scale, conservative = the AND of the chunks' flags; it owns
 *               its two sets.
 * The iE % 12960 locality check (:229-245) is tied to one grid and is not made.  Waits for the device. */
int ibh_global_ec_combine_chunks(int32_t nchunks, const ibh_weighted *const *mats, const int64_t *const *dims_host, const int64_t *extents,
                                 int scale, int64_t *stream_iB, int64_t *stream_iA, double *stream_val, ibh_weighted **out);

/* ------------------------------------------------------------------------- */
/* etopo1_ice: etopo1_ice(files, include_greenland, ofname_root) of modele/etopo1_ice.cpp (:45-247) from arrays instead of
 * files.  The fine grid I (the reference's g1mx1m) and the coarse grid C of the ice fractions (g1x1) nest: imI % imC == 0 and
 * jmI % jmC == 0, mult_i = imI / imC, mult_j = jmI / jmC, coarse cell (j1, i1) owns the fine rows [j1 * mult_j, (j1 + 1) * mult_j)
 * and columns [i1 * mult_i, (i1 + 1) * mult_i).  Planes are int16 [jmI, imI], i fastest.  In the reference's order, with C int
 * arithmetic:
 *   FGICE1m = 0 (:51-52); rows j >= (jmI * 14) / 15: FOCEAN == 0 -> 1 (:84-93); rows j < jmI / 2: FOCEAN == 0 and
 *   ZICTOP - ZSOLID >= 50 -> 1 (:109-117); rows j >= jmI / 2, FOCEAN == 2 (Greenland): with include_greenland
 *   ZICTOP - ZSOLID >= 50 -> 1, without it ZICETOP1m = ZSOLG1m = -300 (:121-140); elsewhere ZICETOP1m / ZSOLG1m are the inputs.
 *   For j1 in [jmC / 2, jmC) and every i1 with fgiceC[j1, i1] != 0 (:166-209): the tile's cells with FOCEAN == 0 (the Greenland
 *   clause of :179, `(include_greenland && focean) == 2`, is never true), ascending by (-ZICTOP, j, i) with the negation taken
 *   in int (the reference's tuple narrows it to int16, undefined at -32768); remain = fgiceC * dxypC[j1]; along the sorted
 *   cells, area = dxypI[j]: area <= remain -> remain -= area, FGICE1m = 1; else FGICE1m = 1 if remain >= area * .5, and stop.
 *   The subtractions are one fp64 chain in that order.  NaN, negative and > 1 fractions take what these comparisons give.
 *   Rows j >= jmI / 2, FOCEAN == 2 (:212-224): FOCEAN1m = include_greenland ? 0 : 1 (elsewhere the input), and the
 *   TRANSPOSED cell (i, j) loses its ice (FGICE1m = 0) where the ocean mask the loop is rewriting reads 1 there: the new value
 *   where FOCEAN[i, j] == 2, i >= jmI / 2 and i <= j (the loop has been there), the input elsewhere.  Where i >= jmI or
 *   j >= imI the reference indexes outside its array; nothing is read or written there.
 *   The h planes (store_h, :17-29): Hntr(17.17, hspecH, hspecI), constant weight 1.0, mean_polar, bitwise
 *   ibh_hntr_regrid_typed_device of each output plane.
 * A tile holds at most IBH_ETOPO1_MAX_TILE fine cells (its sort keys live in LDS), else IBH_EINVAL. */
#define IBH_ETOPO1_MAX_TILE 8192
typedef struct ibh_etopo1_ice ibh_etopo1_ice;
/* The grids of one etopo1_ice (:22, :166-167): the row areas make_dxyp(hspecI) / make_dxyp(hspecC) and, with imH != 0, the
 * regridder of store_h (:22) are made once and uploaded.  imH == jmH == 0: no h planes.  Shapes, nesting and the tile limit are
 * checked before a device is looked for; the messages name both shapes.  Waits for the device. */
int ibh_etopo1_ice_create(ibh_etopo1_ice **out, int32_t imI, int32_t jmI, double offiI, double dlatI, int32_t imC, int32_t jmC, int32_t imH,
                          int32_t jmH, double offiH, double dlatH);
/* Frees the tables of :22 and :166-167 (never a caller's plane). */
int ibh_etopo1_ice_destroy(ibh_etopo1_ice *h);
/* etopo1_ice (:45-247) on planes in HBM: inputs FOCEAN / ZICTOP / ZSOLID int16 [jmI * imI] and FGICE1 double [jmC * imC], never
 * written; outputs four int16 planes [jmI * imI] and, with d_planes_h != NULL, the four h planes FOCEANh, FGICEh, ZICETOPh,
 * ZSOLGh as doubles at d_planes_h + k * ldh (ldh >= imH * jmH).  A NULL plane, a misaligned one, an output that overlaps an
 * input or another output, or h planes from a handle made without hspecH are IBH_EINVAL before a device is touched.  A pure
 * enqueue on `stream`. */
int ibh_etopo1_ice_device(const ibh_etopo1_ice *h, const int16_t *d_focean, const int16_t *d_zictop, const int16_t *d_zsolid, const double *d_fgiceC,
                          int include_greenland, int16_t *d_FOCEAN1m, int16_t *d_FGICE1m, int16_t *d_ZICETOP1m, int16_t *d_ZSOLG1m, double *d_planes_h,
                          int64_t ldh, void *stream);
/* etopo1_ice (:45-247) on host arrays of the same shapes: every plane crosses PCIe once in its own width.  Waits for the device. */
int ibh_etopo1_ice_host(const ibh_etopo1_ice *h, const int16_t *focean, const int16_t *zictop, const int16_t *zsolid, const double *fgiceC,
                        int include_greenland, int16_t *FOCEAN1m, int16_t *FGICE1m, int16_t *ZICETOP1m, int16_t *ZSOLG1m, double *planes_h,
                        int64_t ldh);

/* ------------------------------------------------------------------------- */
/* make_topoO: _make_topoO of modele/topo_base.cpp (:263-809) with its callZ (:20-221), from arrays and with the grids as
 * arguments in place of g1mx1m / g1qx1 / g10mx10m.  The fine grid I of the four int16 planes nests in the ocean grid O of the
 * outputs (imI % imO == 0, jmI % jmO == 0; ocean cell (J, I) owns the fine rows [(J-1) * mult_j, J * mult_j) and columns
 * [(I-1) * mult_i, I * mult_i)); imO and jmO are even (the 2 x 2 block pass, :774-795); the grid S of FLAKES need not nest.
 * The outputs are IBH_MAKE_TOPOO_NPLANE double planes [jmO * imO], i fastest, in the reference's order of out.add (:275-377):
 *   FOCEAN FLAKE FGRND FGICE FGICE_greenland ZATMO dZOCEN dZLAKE dZGICE ZSOLDG ZICETOP ZLAND_MIN ZLAND_MAX ZSGLO ZLAKE ZGRND
 *   ZSGHI FOCEANF FGICEF ZATMOF
 * Steps, in the reference's order, every band bound in C int (and double where written), all arithmetic fp64 without contraction:
 *   the six regrids (:392, :399, :575, :646, :661, :663), mean_polar, bitwise ibh_hntr_regrid_typed_device of the same planes;
 *   the south-pole row (:498-502) and the rounding under SET_TO (:506-531); FLAKE's bands and wedge (:578-586), apportioning and
 *   std::round to 1/256 (:589-600), the clamp for J > JM/6 (:608-623); FGRND with its 1e-14 snap (:633-641); dZOCEN (:646-655);
 *   dZGICE (:671-711): the sums over I in order per row, SUMDFR / SUMDF over J in order, CONSTK, the fill -- the cells filled
 *   through pow (:708) carry the device pow's error, every other cell is bitwise; ZSOLDG = -dZOCEN, ZICETOP = 0 (:723-724);
 *   callZ (:61-220) for every ocean cell, one tile of imI x mult_j fine cells on rows 1 and JM (IMAX = 1), replicated along the row
 *   for the eight planes of :211-218: the sums of :92-108 / :124-142 are sequential chains in traversal order (J1m outer, I1m
 *   inner) with area = make_dxyp(hspecI)[J1m - 1]; the continental cells are sorted ascending by (ZICETOP1m, traversal position)
 *   -- std::sort on the depth alone (:117-118, :144) leaves ties in any order, this is one of them -- and the walks of :159-205 are
 *   sequential chains in that order; the resets (:747-758) in list order; the 2 x 2 lake -> ground pass (:774-795).
 * Planes the reference never writes are 0: ZLAND_MIN, ZLAND_MAX, FGICE_greenland, and ZATMOF at I >= 2 of rows 1 and JM.
 * The debug outputs (int.nc, the printf tables) are not made.  The two fatal conditions -- an ocean cell without an ocean fine
 * cell (:85), a continental cell without land (:146) -- and the stderr warnings are counted on the device (ibh_make_topoo_status);
 * after a fatal condition the planes' contents are unspecified.
 * A tile of at most IBH_MAKE_TOPOO_MAX_TILE fine cells is sorted in LDS; larger tiles (at 1' on 1/4 x 1 degree: the two pole
 * tiles) take a path with scratch in global memory sized at create, with the same order and the same chains. */
#define IBH_MAKE_TOPOO_MAX_TILE 8192
#define IBH_MAKE_TOPOO_NPLANE 20
#define IBH_MAKE_TOPOO_NSTATUS 10
typedef struct ibh_make_topoo ibh_make_topoo;
/* The grids and the hand-set cells of one make_topoO: make_dxyp(hspecI) and make_dxyp(hspecO) (:98, :672), Hntr(17.17, hspecO,
 * hspecI) (:391) and Hntr(17.17, hspecO, hspecS) (:574), SET_TO (:403-494: land_ij then ocean_ij, a later entry wins) and the
 * resets (:231-248), each list as 1-based (i, j) pairs [2 * n] (reset_elev[n]: the elevations), and the long path's scratch.
 * IBH_EINVAL before a device is looked for: a size <= 0, grids that do not nest, odd imO or jmO, 2^31 or more fine cells, a list
 * entry outside [1, imO] x [1, jmO]; the messages name the shapes.  Waits for the device. */
int ibh_make_topoo_create(ibh_make_topoo **out, int32_t imI, int32_t jmI, double offiI, double dlatI, int32_t imO, int32_t jmO, double offiO,
                          double dlatO, int32_t imS, int32_t jmS, double offiS, double dlatS, int32_t nland, const int32_t *land_ij, int32_t nocean,
                          const int32_t *ocean_ij, int32_t nreset, const int32_t *reset_ij, const double *reset_elev);
/* Frees the tables and the scratch (never a caller's plane). */
int ibh_make_topoo_destroy(ibh_make_topoo *h);
/* _make_topoO (:263-809) on planes in HBM: four int16 planes [jmI * imI] and FLAKES double [jmS * imS], never written; plane k
 * of the outputs at d_planes + k * ld (ld >= imO * jmO; the gaps are left untouched).  A NULL or misaligned plane, a short ld or
 * outputs that overlap an input are IBH_EINVAL before a device is touched.  A pure enqueue on `stream`; the handle's work planes,
 * scratch and status serve one call at a time. */
int ibh_make_topoo_device(ibh_make_topoo *h, const int16_t *d_FGICE1m, const int16_t *d_ZICETOP1m, const int16_t *d_ZSOLG1m,
                          const int16_t *d_FOCEAN1m, const double *d_FLAKES, double *d_planes, int64_t ld, void *stream);
/* What the last call on `stream` found, after waiting for it; status[IBH_MAKE_TOPOO_NSTATUS]:
 *   [0] ocean cells without an ocean fine cell (:85), [1] the first of them, (J-1) * imO + (I-1), -1: none;
 *   [2] continental cells without land (:146), [3] the first of them, -1: none;
 *   the warnings, as counts: [4] FGICE < 0 (:610), [5] FGICE > 1 (:614), [6] FLAKE reduced (:618), [7] FGRND outside [0, 1]
 *   (:637), [8] dZOCEN <= 0 on an ocean cell (:652), [9] FLAKE == 1 (:763). */
int ibh_make_topoo_status(const ibh_make_topoo *h, void *stream, int64_t *status);
/* _make_topoO (:263-809) on host arrays of the same shapes: every plane crosses PCIe once in its own width.  status (may be
 * NULL) as above.  Waits for the device. */
int ibh_make_topoo_host(ibh_make_topoo *h, const int16_t *FGICE1m, const int16_t *ZICETOP1m, const int16_t *ZSOLG1m, const int16_t *FOCEAN1m,
                        const double *FLAKES, double *planes, int64_t ld, int64_t *status);
/* out[k] = pow(x[k], .3) as the kernels of make_topoO evaluate it (:690, :708), for measuring its error.  A pure enqueue. */
int ibh_selftest_pow03(const double *d_x, int64_t n, double *d_out, void *stream);

/* ------------------------------------------------------------------------- */
/* ModelE's regridder: GCMRegridder_ModelE::regrid_matrices (slib/icebin/modele/GCMRegridder_ModelE.cpp:487-571).  rmO holds
 * the matrices on ModelE's OCEAN grid O = HntrSpec(imO, jmO, offiO, dlatO); the atmosphere grid A is make_hntrA(O) =
 * HntrSpec(imO/2, jmO/2, offiO/2, 2*dlatO) (modele/hntr.cpp:232-241).  foceanAOp / foceanAOm [nO], sparse O indexing: the
 * ocean fraction the ice model sees (may be fractional) and the one ModelE sees (0 or 1); both are copied.  rmO must outlive
 * the result.  IBH_EINVAL before anything is allocated: odd imO or jmO, imO*jmO != nA of the regridder, nO != nA, an
 * indexingHC that is neither (stride_A, stride_HC) = (1, nO) nor (nhc, 1) -- the A grid keeps the order with nA_A =
 * (imO/2)*(jmO/2) in place of nO (:451-456).  A non-zero sigma in rmO: IBH_ENOTIMPL. */
typedef struct ibh_modele_matrices ibh_modele_matrices;
int ibh_modele_matrices_create(const ibh_regrid_matrices *rmO, int32_t imO, int32_t jmO, double offiO, double dlatO, double eq_rad,
                               const double *foceanAOp, const double *foceanAOm, int64_t nO, ibh_modele_matrices **out);
/* matrix_d of that object.  spec in {AvI EvI AvX EvX} (compute_XAmvGp, :318-368; aliases AAmvIp EAmvIp), {IvA IvE XvA XvE}
 * (compute_GpvXAm, :379-433; aliases IpvAAm IpvEAm), both through ComputeXAmvGp_Helper (:168-280), or the test matrices
 * AOmvAAm / AAmvAOm (:92-121, Hntr's clipped overlap: see ibh_hntr_matrix_d; for both, dim0 is dimAOm, which also clips,
 * and dim1 dimAAm, as the reference passes them; conservative = 1); any other name: IBH_ENOKEY.  The sets are
 * numbered as the reference numbers them: the ice / exchange set by the first O-grid build (Av{G}, scale = false, correctA =
 * true), the atmosphere set by the Hntr stream (raw_EOvEA's for E), whichever side they stand on.  conservative = 0, scaled =
 * scale; XAmvGp: wM = wXAm, Mw = XOpvIp.Mw; GpvXAm: wM = XOpvIp.Mw, Mw = wXAm.  Every product sums its terms over the dense
 * inner index ascending, the first assigned, each operand rounded before the product.
 * dim0 / dim1 are IN/OUT as in ibh_regrid_matrices_matrix_d and must outlive the result; NULL: a fresh set owned by the
 * result.  A set with sparse extent -1 takes nA_A, nE_A = nA_A*nhc, nI or nX; any other extent is IBH_EINVAL.  A cell of the
 * O-grid build whose foceanAOm is neither 0 nor 1 is IBH_EINVAL and the message names the cell (topo.cpp:70-71); an Hntr
 * overlap below 1e-8 in magnitude is IBH_EINVAL (topo.cpp:138-139).  On any error *out is NULL and both sets are as they were. */
int ibh_modele_matrices_matrix_d(const ibh_modele_matrices *mm, const char *spec, ibh_sparse_set *dim0, ibh_sparse_set *dim1,
                                 int scale, ibh_weighted **out);
/* matrix_d with RegridParams(scale, correctA, sigma): the coupler's smoothed IvE (IceCoupler.cpp:461-463).  sigma == NULL or
 * sigma[0] == 0 is exactly ibh_modele_matrices_matrix_d, which is this entry with a zero sigma.  As in the reference, where of
 * the builders behind matrix_d only compute_IvAE reads sigma (RegridMatrices_Dynamic.cpp:237-248) and compute_GpvXAm hands the
 * caller's params to one O-grid build (:404-409): for IvA IvE IpvAAm IpvEAm sigma goes to the build of IpvXOp (scale = false,
 * correctA = false) and to nothing else -- wM = XOpvIp.Mw and Mw = wXAm are those of sigma = 0, conservative stays 0; AvI EvI AvX
 * EvX AOmvAAm AAmvAOm ignore it; XvA / XvE with a non-zero sigma are IBH_ENOTIMPL, the O-grid's own refusal (the smoother needs
 * ice-grid centroids).  The smoother's checks come through unchanged: three positive sigmas and the ice grid's centroids, else
 * IBH_EINVAL.  dim0 / dim1 as above, pre-populated sets and the identity dimI included; on any error both are as they were.
 * The composition crop_mvp(IpvXOp) * diag * XOmvXAm of a smoothed build is row-local (every row of XOmvXAm holds at most one
 * entry; ibh_set_tuning "modele_rowlocal": 1 whenever it can serve, also for sigma = 0; 0 never; -1 the default, smoothed builds
 * only).  It declines a row of more than 128 kept entries to the generic product; the bits are the same either way.
 * ibh_weighted_smoothed_by of the result reports the form that smoothed IpvXOp, ibh_weighted_composed_by the composition. */
int ibh_modele_matrices_matrix_d_sigma(const ibh_modele_matrices *mm, const char *spec, ibh_sparse_set *dim0, ibh_sparse_set *dim1,
                                       int scale, const double sigma[3], ibh_weighted **out);
int ibh_modele_matrices_destroy(ibh_modele_matrices *mm);
/* make_agridA (:57-78): the cells of A under the realised cells of rgO's grid, first-seen in Hntr's stream order.
 * *nA_dense is always set; to_sparse (may be NULL) receives that many indices (at most (imO/2)*(jmO/2)). */
int ibh_modele_agridA(const ibh_regridder *rgO, int32_t imO, int32_t jmO, double offiO, double dlatO, int32_t *nA_dense,
                      int64_t *to_sparse);
/* GCMRegridder_ModelE::global_AvE (modele/GCMRegridder_ModelE.cpp:579-628) in its library functions, composed the way the
 * offline tools compose them (make_merged_topoo.cpp:232-238, make_topoa.cpp:131-135,186-196); DESIGN.md 16.
 *
 * ibh_modele_merge_EOpvAOp: compute_EOpvAOp_merged and, with squash_ecs, squash_ECs (modele/merge_topo.cpp:375-527).  rmOs:
 * one regrid_matrices per ice sheet, in sheet order, all on the ocean grid of nO cells with the same nhc and indexingHC
 * (their mask is that sheet's emI_ice; their scale / correctA are ignored: EvA is built with scale = false, correctA =
 * false, sigma = 0 and fresh sets, :401-411).  One triplet stream in SPARSE indices: with use_local_ice every sheet's EvA
 * visited by columns, rows ascending inside (:417-423); with use_global_ice the base matrix (base_iE + offsetE, base_iO,
 * base_val) in the order of the arrays ([INFERRED]: the reference reads a ZArray generator, :441-446), offsetE = nO *
 * nhc_local (:434; nhc_local = the sheets' nhc, 0 without sheets), else 0.  The stream numbers {dimEOp, dimAOp} first-seen
 * ({ADD_DENSE, ADD_DENSE}) and is summed as setFromTriplets sums it (duplicates in stream order, the first assigned).  The
 * result's wM / Mw are sum(M, dim, '+'): Mw is the wAOp that ibh_modele_AAmvEAm reads.  conservative = scaled = 0.
 *   base_*            the base (global) ice EOpvAOp, UNSCALED, as host COO arrays in sparse indices over the shape (base_nE,
 *                     base_nO), with the nhc_base elevations hcdefs_base and the strides of indexingHC_base; read only with
 *                     use_global_ice, except the strides, which always give the order of the result's indexingHC
 *   dimAOp            IN/OUT (NULL: owned by the result), appended to; dimEOp: OUT, a fresh set (NULL: owned by the result)
 *   sparse extents    dimEOp offsetE + base_nE, dimAOp base_nO (:454-455); without global ice nO * nhc_local and nO (the
 *                     reference leaves 0 there); after squash_ecs dimEOp has extent(dimAOp) * nhc_out (:520-521)
 *   hcdefs_out, underice_out   [nhc_local + nhc_base] at most; *nhc_out entries are written: the local classes (UI_LOCALICE =
 *                     1) then the base ones (UI_GLOBALICE = 2) (:426-449); after squash_ecs the sorted distinct elevations,
 *                     all UI_GLOBALICE (:481-490), and a row key (iO, ihc0) of the merge has become (iO, to_new[ihc0]),
 *                     computed in 64 bits (the reference uses int)
 *   stride_*_out      indexingHC_base with its class extent replaced by *nhc_out (:364-372): (1, stride_HC) class-slowest, else
 *                     (*nhc_out, 1)
 * IBH_EINVAL, naming the offender: a sheet whose grid disagrees with nO or whose nhc / strides differ from sheet 0's, base_nO
 * != nO, a base index outside its shape, a dimEOp that is not empty, sets whose extents disagree.  On any error *EOpvAOp is
 * NULL and both sets are as they were. */
int ibh_modele_merge_EOpvAOp(const ibh_regrid_matrices *const *rmOs, int nsheets, int64_t nO, int64_t base_nE, int64_t base_nO,
                             int64_t base_nnz, const int64_t *base_iE, const int64_t *base_iO, const double *base_val,
                             const double *hcdefs_base, int32_t nhc_base, int64_t base_stride_A, int64_t base_stride_HC, int use_global_ice,
                             int use_local_ice, int squash_ecs, ibh_sparse_set *dimAOp, ibh_sparse_set *dimEOp, ibh_weighted **EOpvAOp,
                             int64_t *offsetE, int32_t *nhc_out, double *hcdefs_out, int16_t *underice_out, int64_t *stride_A_out,
                             int64_t *stride_HC_out);
/* _compute_AAmvEAm_EIGEN (modele/topo.cpp:242-347): the atmosphere-grid matrix AAmvEAm of a GIVEN EOpvAOp (unscaled, dense over
 * {dimEOp, dimAOp}, its Mw = wAOp = sum(EOpvAOp, 1, '+')) on the ocean grid O = HntrSpec(imO, jmO, offiO, dlatO) under A =
 * make_hntrA(O).  nhc and the strides of indexingHCO (sA_O, sHC_O) and indexingHCA (sA_A, sHC_A) are explicit: raw_EOvEA
 * (topo.cpp:147-161) looks for the classes [0, nhc) only.  With the canonical order of DESIGN.md 16:
 *   M = diag(scale ? sAAmvAOm : wAAm .* sAAmvAOm) * AAmvAOm * diag(EOmvAOms) * AOmvEOm * diag(EAmvEOms) * EOmvEAm
 *   wM = wAAm, Mw = wEAm, conservative = 0, scaled = scale
 * dimAAm / dimEAm: IN/OUT (NULL: owned by the result), sparse extents nA_A and nA_A * nhc (-1 is taken as that).  IBH_EINVAL:
 * odd imO or jmO, imO * jmO != nO, a cell of dimAOp outside [0, nO) or with foceanAOm neither 0 nor 1 (topo.cpp:70-71, names the
 * cell), an Hntr overlap below 1e-8 (topo.cpp:138-139).  On any error *out is NULL and both sets are as they were. */
int ibh_modele_AAmvEAm(const ibh_weighted *EOpvAOp, const ibh_sparse_set *dimEOp, const ibh_sparse_set *dimAOp, int32_t imO, int32_t jmO,
                       double offiO, double dlatO, double eq_rad, int32_t nhc, int64_t sA_O, int64_t sHC_O, int64_t sA_A, int64_t sHC_A,
                       const double *foceanAOp, const double *foceanAOm, int64_t nO, int scale, ibh_sparse_set *dimAAm,
                       ibh_sparse_set *dimEAm, ibh_weighted **out);
/* GCMCoupler_ModelE::update_topo's field handling (modele/GCMCoupler_ModelE.cpp:972-1098): merge_topoO and make_topoA; DESIGN.md 17.
 *
 * ibh_weighted_row_stats_device: the statistics merge_topoO reads an OvI through, in ONE pass over the CSR.  Per dense row r:
 * sum[r] = the sum of val * x[col], min[r] / max[r] = the smallest / largest x[col], over the STORED entries of the row alone
 * (x may hold NaN in columns no entry names).  min starts at DBL_MAX and max at DBL_MIN, the smallest positive normal number,
 * as the reference's zland_min / zland_max do (merge_topo.cpp:181-182): a row without entries gives (0, DBL_MAX, DBL_MIN) and a
 * row whose x are all below DBL_MIN keeps DBL_MIN.  Any of d_sum / d_min / d_max may be NULL.  d_x [ncol_d], outputs
 * [nrow_d], all device pointers.  The order of a row's sum depends on the row's length and the matrix's shape alone
 * (repeatable; 1e-12 of the sequential sum).  A pure enqueue on `stream`. */
int ibh_weighted_row_stats_device(const ibh_weighted *w, const double *d_x, double *d_sum, double *d_min, double *d_max, void *stream);
/* merge_topoO (modele/merge_topo.cpp:84-360).  emI_lands / emI_ices: one regrid_matrices per ice sheet for the land mask and
 * one for the ice mask (their elevmaskI is emI_lands[k] / emI_ices[k]; their scale / correctA are ignored), in sheet order, both
 * of sheet k made from the same ice regridder, every sheet on one ocean grid of imO x jmO cells.  planes: eleven arrays
 * [jmO*imO], iO = j*imO + i, in this order: the in/out planes foceanOp fgiceOp zatmoOp foceanOm flakeOm fgrndOm fgiceOm zatmoOm
 * zicetopO, then the out-only zland_minO zland_maxO; mergemaskOm (int16) is out-only.  Per sheet the four AvI (scale = 1,
 * correctA = 0 and scale = 0, correctA = 1 for either mask, fresh dimO, identity dimI) are built by ibh_regrid_matrices_matrix_batch's
 * builder and accumulated in sheet order; then the per-cell update, the single-cell-ocean pass (one parallel pass from a
 * snapshot of foceanOm: equal to the reference's sequential loop), the sanity checks and the NaN of the unset
 * zland_*.  zland_maxO keeps DBL_MIN on a merged cell whose land lies entirely below that (the reference's quirk).
 * flags [nO]: one word per cell; bit k < 9: plane k was NaN on entry ("<name>2-0"), bit 9 + k: plane k is NaN on return,
 * bit 18: the land fractions do not sum to 1 within 1e-13.  *nerrors = the number of set bits.  The call succeeds when checks
 * fail, as the reference's does.  eq_rad is accepted and unused.  IBH_EINVAL naming the offender, before anything is touched:
 * mask counts that differ, imO * jmO != nA of a sheet, a sheet on another ocean grid, a non-zero sigma.
 * _device: device pointers (planes: a host array of device pointers), enqueued on `stream`, which is synchronised before
 * returning; the other form copies host arrays. */
int ibh_modele_merge_topoO_device(const ibh_regrid_matrices *const *emI_lands, int32_t nlands, const ibh_regrid_matrices *const *emI_ices,
                                  int32_t nices, int32_t imO, int32_t jmO, double eq_rad, double *const *d_planes /* [11] */,
                                  int16_t *d_mergemaskOm, uint32_t *d_flags, int64_t *nerrors, void *stream);
int ibh_modele_merge_topoO(const ibh_regrid_matrices *const *emI_lands, int32_t nlands, const ibh_regrid_matrices *const *emI_ices, int32_t nices,
                           int32_t imO, int32_t jmO, double eq_rad, double *const *planes /* [11] */, int16_t *mergemaskOm, uint32_t *flags,
                           int64_t *nerrors);
/* make_topoA (modele/topo.cpp:581-855).  planesO: the nine ocean planes foceanOm flakeOm fgrndOm fgiceOm zatmoOm zlakeOm zicetopOm
 * zland_minOm zland_maxOm [jmO*imO] and mergemaskOm (int16); the two HntrSpecs; (hc_stride_A, hc_stride_HC): the strides of
 * indexingHCA; hcdefs / underice_hc [nhc] (host); AAmvEAm: read in SPARSE indices through its two sets.  planesA: the nine
 * atmosphere planes in TopoABundles' order (focean flake fgrnd fgice zatmo hlake zicetop zland_min zland_max) [jmA*imA],
 * mergemaskA (int16), fhc3 / elevE3 (double) and underice3 (int16) [nhc + 1, jmA, imA].  flags [nA]: bit 0: the land fractions
 * do not sum to 1 within 1e-13, bit 1: sum(FHC) is neither 0 nor 1 within 1e-13; *nerrors = the number of set bits.
 * IBH_EINVAL naming the entry: an entry of AAmvEAm whose iE splits into another A cell ("Matrix is non-local"), an ihc outside
 * [0, nhc), an iA outside [0, nA); the outputs are then undefined (_device) or untouched (host form).  One host wait. */
int ibh_modele_make_topoA_device(const double *const *d_planesO /* [9] */, const int16_t *d_mergemaskOm, int32_t imO, int32_t jmO,
                                 double offiO, double dlatO, int32_t imA, int32_t jmA, double offiA, double dlatA, int64_t hc_stride_A,
                                 int64_t hc_stride_HC, const double *hcdefs, const int16_t *underice_hc, int32_t nhc,
                                 const ibh_weighted *AAmvEAm, double *const *d_planesA /* [9] */, int16_t *d_mergemaskA, double *d_fhc3,
                                 double *d_elevE3, int16_t *d_underice3, uint32_t *d_flags, int64_t *nerrors, void *stream);
int ibh_modele_make_topoA(const double *const *planesO /* [9] */, const int16_t *mergemaskOm, int32_t imO, int32_t jmO, double offiO,
                          double dlatO, int32_t imA, int32_t jmA, double offiA, double dlatA, int64_t hc_stride_A, int64_t hc_stride_HC,
                          const double *hcdefs, const int16_t *underice_hc, int32_t nhc, const ibh_weighted *AAmvEAm,
                          double *const *planesA /* [9] */, int16_t *mergemaskA, double *fhc3, double *elevE3, int16_t *underice3,
                          uint32_t *flags, int64_t *nerrors);
/* Diagnostic: the sparse product the ModelE matrices are composed with, alone.  C = L * R for two matrices in HBM (columns
 * ascending inside a row, L's columns = R's rows): C(r, c) sums L(r, k) * R(k, c) over k ascending, the first term assigned;
 * an entry exists wherever a term does.  Identity dims, wM = Mw = 0, flags of L.  Used by tests/test_gpu_modele.py. */
int ibh_selftest_csr_product(const ibh_weighted *L, const ibh_weighted *R, ibh_weighted **out);
/* Diagnostic: the composition of the I-row ModelE matrices alone, crop_cols(L) * R, by one named form: 1 crop_cols + the product
 * above, 2 the row-local kernel.  Host arrays: map[nmap = L's columns] into [-1, R's rows), one-to-one (-1: the entry is dropped);
 * rs[L's rows] and cs[R's rows], either may be NULL.  Per entry (i, p, v) of L with k = map[p] >= 0 and a non-empty row k of R:
 * the term ((rs ? rs[i] * v : v) [* cs[k]]) * R(k, c) for each entry c of that row, every product rounded; C(i, c) sums its
 * terms in ascending k, the first assigned.  Form 2 serves an R whose rows hold at most one entry and rows of at most 128 kept
 * entries; otherwise it leaves the build to form 1, and ibh_weighted_composed_by of *out tells which form built it.  Identity dims,
 * wM = Mw = 0, flags of L.  Every argument is checked before a device is touched.  Used by tests/test_gpu_compose_cols.py. */
int ibh_selftest_compose_cols(const ibh_weighted *L, const int32_t *map, int64_t nmap, const double *rs, const double *cs,
                              const ibh_weighted *R, int form, ibh_weighted **out);
/* Diagnostic: the shared triplets -> CSR build (Eigen setFromTriplets: duplicates summed in input order, the first term
 * assigned) on n host triplets with dense ids, and the plain weights as a matrix build takes them.  mode 0: local disorder
 * is expected, as ibh_weighted_from_coo; mode 1: it is not (the ice-row builds: per-row slots, the optimistic row-only sort).
 * *out: identity dims, wM = sum(M, 0, '+') (columns ascending, from 0), Mw = sum(M, 1, '+') (rows ascending, from 0) through
 * per-column slots when nnz <= 4 * ncol, else through the stable sort by column.  info_out[IBH_TRIPLETS_INFO]: the forms that ran,
 *   [0] order: 0 in order, 1 pieces sorted in LDS, 2 radix sort       [1] per-row slots: 0 not tried, 1 taken, 2 declined
 *   [2] optimistic row-only sort: 0 not tried, 1 held, 2 failed        [3] sums of the values: 0 none, 1 thread, 2 wave per entry
 *   [4] row pointer: 0 none, 1 every row searches, 2 heads + fill      [5] wM: as [3], per row
 *   [6] Mw: 0 no entries, 1 slots, 2 sort                              [7] slots: columns of more than 64 entries
 *   [8], [9] sort: as [3] per column, as [4] for the column pointer.
 * Every argument is checked before a device is touched.  Used by tests/test_gpu_csr_build.py. */
#define IBH_TRIPLETS_INFO 10
int ibh_selftest_triplets(int32_t nrow, int32_t ncol, int64_t n, const int32_t *row, const int32_t *col, const double *val, int mode,
                          ibh_weighted **out, int32_t *info_out);
/* Diagnostic: one piece of the CSR algebra alone (csrops.h).  Host arrays: idx[nidx], a[na], b[nb]; an unused one is NULL with
 * length 0.  The matrix ops take `in` and return *mat_out (identity dims, wM = Mw = 0, flags of `in`):
 *   TRANSPOSE;  CROP_ROWS idx = src[nout] (-1: an empty row), a = rs[nrow] or none;  CROP_COLS idx = map[ncol] into [0, nout)
 *   (-1: dropped; one-to-one), a = rs[nrow] or none, b = cs[nout] or none;  SCALE_ROWS a[nrow] * v;  SCALE_COLS v * a[ncol];
 *   SCALE_ROWS_RECIP v * (1 / a[nrow]), rows without entries skipped.
 * The vector ops take in = NULL and fill vec_out (double[nout]): RECIP 1 / a;  MUL a * b;  GATHER a[idx[k]].  EXPAND_ROWS takes
 * `in` and fills vec_out (int32[nnz]) with the row of every entry.  Every argument is checked before a device is touched. */
enum { IBH_CSROP_TRANSPOSE = 0, IBH_CSROP_CROP_ROWS, IBH_CSROP_CROP_COLS, IBH_CSROP_SCALE_ROWS, IBH_CSROP_SCALE_COLS,
       IBH_CSROP_SCALE_ROWS_RECIP, IBH_CSROP_RECIP, IBH_CSROP_MUL, IBH_CSROP_GATHER, IBH_CSROP_EXPAND_ROWS };
int ibh_selftest_csr_op(int op, const ibh_weighted *in, const int32_t *idx, int64_t nidx, const double *a, int64_t na, const double *b,
                        int64_t nb, int64_t nout, ibh_weighted **mat_out, void *vec_out);

/* Public members of Weighted_Eigen, read back to host. */
int ibh_weighted_shape(const ibh_weighted *w, int32_t *nrow_d, int32_t *ncol_d, int64_t *nnz);
int ibh_weighted_flags(const ibh_weighted *w, int *conservative, int *scaled);
int ibh_weighted_dim(const ibh_weighted *w, int k, int64_t *sparse_extent, int32_t *dense_extent);
int ibh_weighted_dim_to_sparse(const ibh_weighted *w, int k, int64_t *out /* [dense_extent] */);
int ibh_weighted_get_wM(const ibh_weighted *w, double *out /* [nrow_d] */);
int ibh_weighted_get_Mw(const ibh_weighted *w, double *out /* [ncol_d] */);
/* ->M in row-major COO order (row asc, col asc); any of row/col/val may be NULL. */
int ibh_weighted_get_coo(const ibh_weighted *w, int32_t *row, int32_t *col, double *val);
int ibh_weighted_get_csr(const ibh_weighted *w, int32_t *rowptr, int32_t *colind, double *val);

/* Weighted_Eigen::apply(A_b, fill, force_conservation, tmp)
 * (call sites modele/merge_topo.cpp:65, modele/icebin22m.cpp:153; inline Eigen
 * products IceCoupler.cpp:237,445).  B_b[k, :] = M * A_b[k, :] for k < nvar in
 * dense index spaces; rows with wM == 0 receive `fill`; when the matrix is
 * not conservative and force_conservation != 0 each variable is rescaled by
 * (Mw . A) / (wM . B).  _host takes host pointers (copies over PCIe);
 * _device takes device pointers and only enqueues work on `stream`: no allocation, copy or
 * synchronisation once the handle has been prepared (ibh_weighted_prepare).  On a handle that was
 * NOT prepared an apply may (a) grow scratch (allocates; an error inside a stream capture) and (b) on
 * the SECOND apply of a large elevation-class matrix build the column-sweep / band structure the faster
 * kernels read (allocates, synchronises `stream` a few times; skipped inside a capture; a build that
 * fails leaves the matrix on its row-by-row kernel, the apply still succeeds) --
 * ibh_set_tuning("lazy_structures", 0) switches (b) off for the process.  lda/ldb:
 * distance in doubles between consecutive variables (>= dense extents); any value
 * works, ldb a multiple of 64 (512-byte planes) is fastest for the I-row matrices.
 * The handle keeps small per-apply scratch buffers: use one stream at a time per handle. */
int ibh_weighted_apply_host(const ibh_weighted *w, const double *A_b, int32_t nvar, int64_t lda,
                            double *B_b, int64_t ldb, double fill, int force_conservation);
int ibh_weighted_apply_device(const ibh_weighted *w, const double *dA_b, int32_t nvar, int64_t lda,
                              double *dB_b, int64_t ldb, double fill, int force_conservation,
                              void *stream);
/* Several field batches through ONE launch: for q < nbatch, dB_b[q] = M * dA_b[q], every batch
 * [nvar x ncol_d] -> [nvar x nrow_d] with the same nvar / lda / ldb -- what a caller that applies one
 * matrix to several groups of variables in a row does (Weighted_Eigen::apply call sites
 * modele/merge_topo.cpp:65, modele/icebin22m.cpp:153; the coupler's per-sheet products IceCoupler.cpp:237,445).
 * dA_b / dB_b are HOST arrays of nbatch DEVICE pointers, read during the call (they travel in the
 * kernel arguments: no device-side table, nothing left pending on them).  Results are bitwise those of
 * nbatch separate ibh_weighted_apply_device calls.  A 64-field 5 km apply is a latency-sized problem
 * (launch + dependent loads are a third of its 11 us); batched, that cost is paid once per launch.
 * More than IBH_MAX_BATCH batches are split into several launches. */
#define IBH_MAX_BATCH 32
int ibh_weighted_apply_many_device(const ibh_weighted *w, int32_t nbatch, const double *const *dA_b, int32_t nvar,
                                   int64_t lda, double *const *dB_b, int64_t ldb, double fill,
                                   int force_conservation, void *stream);
/* Make applies of up to nvar variables, up to nbatch field batches per ibh_weighted_apply_many_device
 * call, pure enqueues: builds NOW (synchronously, on the default stream) whatever structure those applies
 * would otherwise build lazily (column sweep / bands: see above) and sizes every per-apply scratch buffer
 * (transposed inputs of the I-row kernels, partial sums of the sweep / band kernels for the batch depth,
 * conservation factors, transform scratch).  Call it once after a matrix is built and before capturing
 * applies into a hipGraph, or whenever the latency of the first applies matters.  Eager and captured
 * applies of a prepared handle run the same kernels and are bitwise equal.
 * ibh_weighted_reserve(w, nvar) only sizes scratch for single applies (nbatch = 1) and builds nothing. */
int ibh_weighted_prepare(const ibh_weighted *w, int32_t nvar, int32_t nbatch);

/* Fused pair: B1 = first * A and B2 = second * B1 in ONE launch -- the step "ice -> elevation classes -> atmosphere" of a
 * coupler (E = EvI * I, A = AvE * E; the reference makes two Weighted_Eigen::apply calls, ibmisc linear/eigen.cpp, one per
 * matrix: RegridMatrices_Dynamic.cpp:354-390 hands out the two matrices).  Possible when every row of `second` reads rows of one
 * row group of `first` only, which AvE after EvI does by construction (a GCM cell's value combines that cell's own elevation
 * classes); the rows need not be numbered alike (the pairing goes through the sparse indices of the shared dimension).
 * ibh_weighted_pair_prepare builds `first`'s row groups if it has none, works the pairing out on the host (synchronises) and
 * returns IBH_ENOTIMPL when the two matrices do not pair -- the caller then makes two applies.  ibh_weighted_apply_pair_device is
 * a pure enqueue (graph-capturable); B1 is bitwise what ibh_weighted_apply_device(first) writes, B2 is the second matrix's
 * result with the same fill / wM == 0 rule, summed in a fixed order (1e-12 of the separate apply, bitwise when `second` lists
 * its columns in the order of `first`'s rows).  Conservative matrices only (no smoothing). */
int ibh_weighted_pair_prepare(const ibh_weighted *first, const ibh_weighted *second, int32_t nvar);
int ibh_weighted_apply_pair_device(const ibh_weighted *first, const ibh_weighted *second, const double *dA_b, int32_t nvar, int64_t lda,
                                   double *dB1_b, int64_t ldb1, double *dB2_b, int64_t ldb2, double fill, void *stream);
/* The chain of BASELINE config 3, ice -> elevation classes -> atmosphere -> ice, in one call: B1 = first * A and B2 = second * B1
 * as the fused pair above (ibh_weighted_pair_prepare(first, second) first), B3 = third * B2 (IvA; the reference: three
 * Weighted_Eigen::apply calls, IceCoupler.cpp:203-252 builds its inputs the same way).  Two stream-ordered launches; B1, B2, B3 are
 * bitwise what the pair apply followed by ibh_weighted_apply_device(third) writes; a pure enqueue (graph-capturable). */
int ibh_weighted_apply_chain_device(const ibh_weighted *first, const ibh_weighted *second, const ibh_weighted *third, const double *dA_b,
                                    int32_t nvar, int64_t lda, double *dB1_b, int64_t ldb1, double *dB2_b, int64_t ldb2, double *dB3_b,
                                    int64_t ldb3, double fill, void *stream);
int ibh_weighted_reserve(const ibh_weighted *w, int32_t nvar);
/* The coupler's fused product B = M * (A*T + b) (IceCoupler.cpp:203-252 construct_ice_ivalsI and
 * :445 gcm_ivalsX = M * (ice_ovalsI*T + b)): dA_b [nvar_in x ncol_d] field-major device pointer,
 * T [nvar_in x nvar_out] row-major HOST array holding the sparse variable transform (exact zeros are
 * structural and skipped, as Eigen's dense*sparse product does), b [nvar_out] host, dB_b
 * [nvar_out x nrow_d] device.  The small dense transform is applied on the SMALL side of M (inputs
 * when ncol_d <= nrow_d, outputs otherwise), so no transformed copy of the large field array is
 * ever written.  Uses scratch owned by the handle: calls on one handle must be stream-ordered.
 * T and b are consumed during the call (kernel arguments) when nvar_in*nvar_out + nvar_out <= 384;
 * larger transforms are staged through a device copy and synchronise the stream. */
int ibh_weighted_apply_transformed_device(const ibh_weighted *w, const double *dA_b, int32_t nvar_in, int64_t lda,
                                          const double *T, const double *b, int32_t nvar_out,
                                          double *dB_b, int64_t ldb, double fill, void *stream);
/* The legacy COO product behind icebin.coo_multiply(M, x, fill, ignore_nan) (coo_matvec,
 * pylib/icebin_cython.cpp:158-192; used by tests/test_conserv/test_conserv.py:139-205 and
 * pylib/icebin/ibplotter.py:88): yy[row] = sum of data*xx[col] over the row's entries, skipping entries
 * whose input is NaN when ignore_nan != 0; a row with no surviving entry is NOT written (yy keeps what
 * the caller preset, i.e. `fill`).  No wM test, no conservation correction.
 * _device: on the CSR of a Weighted, field-major device arrays, only enqueues work on `stream`.
 * ibh_coo_matvec: the reference's signature (host arrays, arbitrary triplet order, duplicates add up). */
int ibh_weighted_matvec_device(const ibh_weighted *w, const double *dxx, int32_t nvar, int64_t ldx,
                               double *dyy, int64_t ldy, int ignore_nan, void *stream);
int ibh_coo_matvec(double *yy /* [nrow] in/out */, const double *xx /* [ncol] */, int ignore_nan,
                   int64_t nrow, int64_t ncol, int64_t nnz, const int32_t *row, const int32_t *col,
                   const double *data);
/* linear_Weighted.apply_weight(dim, A) (matrix_formats.rst:167-186):
 * out[k] = sum_j w[j] * A_b[k*lda + j], w = wM (dim 0) or Mw (dim 1); host pointers. */
int ibh_weighted_apply_weight_host(const ibh_weighted *w, int dim, const double *A_b,
                                   int32_t nvar, int64_t lda, double *out /* [nvar] */);

/* ------------------------------------------------------------------------- */
/* Field-sharded applies across the GPUs of one node (BASELINE.json north_star).  One process per GPU:
 * rank r owns the fields [r*nvar_local, (r+1)*nvar_local) of a regrid of world*nvar_local fields (contiguous in the
 * field-major arrays), every rank holds the same matrix (built redundantly: a build is cheaper than broadcasting it),
 * the SpMM needs no communication and the results are reassembled on EVERY rank.  The reference has no counterpart:
 * it gathers everything to MPI rank 0 and regrids there (modele/GCMCoupler_ModelE.cpp:764-792).
 *   ibh_comm_unique_id   rank 0 obtains an id (ncclGetUniqueId) and ships it to the other ranks by whatever the host
 *                        program has (MPI_Bcast in ModelE: GCMCoupler_ModelE.cpp; a file; torch.distributed);
 *   ibh_comm_create      every rank: the communicator on its CURRENT device (ncclCommInitRank; id may be NULL for
 *                        world == 1, which needs no RCCL).  RCCL is loaded at run time (dlopen; ICEBIN_RCCL_LIB
 *                        overrides the search): without it only world == 1 and custom transports work;
 *   ibh_comm_create_custom  the same choreography over a transport the caller supplies (tests; other fabrics):
 *                        fn(user, d_base, count, stride, world, rank, stream) must deliver every rank's `count` doubles at
 *                        d_base + rank*stride to d_base + rank*stride on every peer, ordered on `stream`; 0 = success. */
#define IBH_UNIQUE_ID_BYTES 128
typedef struct ibh_comm ibh_comm;
typedef int (*ibh_exchange_fn)(void *user, double *d_base, int64_t count, int64_t stride, int world, int rank, void *stream);
int ibh_comm_unique_id(char id[IBH_UNIQUE_ID_BYTES]);
int ibh_comm_create(int world, int rank, const char id[IBH_UNIQUE_ID_BYTES], ibh_comm **out);
int ibh_comm_create_custom(int world, int rank, ibh_exchange_fn fn, void *user, ibh_comm **out);
/* A custom transport that also carries pieces of UNEQUAL size (the sharded assembly, ibh_regrid_matrices_matrix_d_sharded):
 * fn(user, d_base, offsets[world + 1] (bytes), world, rank, stream) must deliver every rank q's bytes
 * [offsets[q], offsets[q+1]) of d_base to the same place on every peer, ordered on `stream`; 0 = success. */
typedef int (*ibh_gatherv_fn)(void *user, void *d_base, const int64_t *offsets, int world, int rank, void *stream);
int ibh_comm_set_custom_gatherv(ibh_comm *c, ibh_gatherv_fn fn);
/* The exchange stream.  By default the communicator creates its own (non-blocking) stream and DESTROYS it in ibh_comm_destroy:
 * the `stream` a custom transport's callbacks receive for the field exchanges is that stream, and it is invalid once
 * ibh_comm_destroy has returned -- a transport whose allocator keeps per-stream state (torch's pinned-host cache records the
 * streams a block was used on) must drop that state before it destroys the communicator, or hand in a stream of its own:
 * ibh_comm_set_stream makes the communicator enqueue its exchanges on the CALLER's stream, which the caller keeps alive until
 * after ibh_comm_destroy and destroys itself (the library synchronises it in ibh_comm_destroy, never destroys it).  Call it
 * before the first apply; a stream that also carries the SpMMs serialises exchange and compute.  (The callbacks of the sharded
 * ASSEMBLY, ibh_gatherv_fn and the 32-byte ibh_exchange_fn call of ibh_regrid_matrices_matrix_d_sharded, always receive the
 * caller's build stream.) */
int ibh_comm_set_stream(ibh_comm *c, void *stream);
/* Options of one communicator.  "planes_padded" (default 0): 1 = the caller owns the gap [nrow_d, ldb) of every result plane of
 * the sharded applies on this communicator as padding (planes rounded up to whole 512-byte lines, as the library's own wrappers
 * allocate them): the planes of a field block then travel as ONE piece and the padding of the peers' planes is overwritten.
 * With 0 nothing outside [0, nrow_d) of a plane is touched on any rank: planes travel one by one unless ldb == nrow_d.
 * Unknown key: IBH_ENOKEY. */
int ibh_comm_set_option(ibh_comm *c, const char *key, int value);
int ibh_comm_destroy(ibh_comm *c);
int ibh_comm_info(const ibh_comm *c, int *world, int *rank);
/* Weighted::apply of world*nvar_local fields, sharded by field: dB_all [world*nvar_local x ldb] (device, the same
 * shape on every rank) receives rank r's results in rows [r*nvar_local, (r+1)*nvar_local).  The local SpMM is enqueued on
 * `stream` and writes straight into this rank's rows; the exchange -- direct peer-to-peer sends (xGMI is a full mesh:
 * seven concurrent transfers use all links) -- runs on a stream the communicator owns, `block_fields` fields at a time
 * (0: chosen by size -- one exchange for KB-sized results, blocks of >= 8 fields and ~128 MB for the GB-sized results of
 * the I-row matrices) so that it overlaps the SpMM of the following block and of the following apply.  dB_all is complete once
 * ibh_comm_wait(c, s) has made stream s wait for the exchanges enqueued so far.  Same results as ibh_weighted_apply_device
 * on each rank's fields (bitwise), without the conservation correction: a smoothed (non-conservative) matrix needs
 * ibh_weighted_apply_sharded_conserve_device.
 * ldb > nrow_d: a true leading dimension (a column view of a larger array) unless the communicator says otherwise -- every plane
 * travels by itself and nothing outside [0, nrow_d) of a plane is touched on any rank; ibh_comm_set_option(c, "planes_padded", 1)
 * declares the gap padding owned by the caller, the planes of a block then travel as one piece (fewer, larger transfers).
 * Streams: any stream may issue applies and waits on one communicator; an apply whose results overlap an exchange still in
 * flight is ordered behind it whichever stream enqueued that exchange (the last 8 exchanges are tracked individually, older
 * unfinished ones through the range hull of their successor). */
int ibh_weighted_apply_sharded_device(const ibh_weighted *w, ibh_comm *c, const double *dA_local, int32_t nvar_local,
                                      int64_t lda, double *dB_all, int64_t ldb, double fill, int32_t block_fields,
                                      void *stream);
/* The same for nbatch independent field batches (ibh_weighted_apply_many_device: ONE SpMM launch) whose results travel in
 * ONE grouped exchange -- for KB-sized results (A- and E-row matrices: a [64, 122] AvI result is 62 KB) an exchange per
 * apply is latency-bound, a group of 32 is not.  dA_local / dB_all: host arrays of nbatch device pointers. */
int ibh_weighted_apply_many_sharded_device(const ibh_weighted *w, ibh_comm *c, int32_t nbatch, const double *const *dA_local,
                                           int32_t nvar_local, int64_t lda, double *const *dB_all, int64_t ldb, double fill,
                                           void *stream);
/* The two sharded applies with force_conservation (ibh_weighted_apply_device's): every rank holds whole fields, so the factor
 * (Mw . A_k) / (wM . B_k) of field k is local -- each field block is corrected on its rank before it travels, no collective.
 * Bitwise ibh_weighted_apply_device(force_conservation) on each rank's fields; a conservative matrix ignores the flag, and
 * force_conservation = 0 is the call above. */
int ibh_weighted_apply_sharded_conserve_device(const ibh_weighted *w, ibh_comm *c, const double *dA_local, int32_t nvar_local,
                                               int64_t lda, double *dB_all, int64_t ldb, double fill, int force_conservation,
                                               int32_t block_fields, void *stream);
int ibh_weighted_apply_many_sharded_conserve_device(const ibh_weighted *w, ibh_comm *c, int32_t nbatch, const double *const *dA_local,
                                                    int32_t nvar_local, int64_t lda, double *const *dB_all, int64_t ldb, double fill,
                                                    int force_conservation, void *stream);
int ibh_comm_wait(ibh_comm *c, void *stream);
/* RegridMatrices_Dynamic::matrix_d with the ASSEMBLY shared by the ranks of a communicator (BASELINE.json config 5: "overlap
 * COO->CSR assembly + apply, 8 x MI355X"; the reference rebuilds its matrices every coupling step, IceCoupler.cpp:361-468, on one
 * core).  Collective: every rank calls it with the same arguments on the same regridder / elevation mask and receives the WHOLE
 * matrix -- bitwise the result of ibh_regrid_matrices_matrix_d.  The exchange grid is sorted by atmosphere cell
 * (AbbrGrid.cpp:10-21), so rank k runs the streamed passes over a contiguous block of ranges holding ~1/world of the exchange
 * cells; three exchanges on the caller's thread stream (counters; the first-seen flags and class ranks the ranks look up in each
 * other's blocks, ~1 byte per exchange cell; the pieces of the CSR / weights / dims tables) complete it.  Served this way: the
 * eight A/E/I/X matrices on sets numbered by the build (dims NULL or empty) AND on the sets the reference's coupler passes
 * (IceCoupler.cpp:366-377, 462-467) -- an identity dimI / dimX on the ice / exchange side (A/E-row matrices: Mw travels as
 * {position, value} pairs; X rows: a block of cells is a block of rows; I rows: the row lengths are merged before the row pointer
 * is scanned, the rows travel in first-seen order and are copied to their places), a pre-populated dimE as the column set (looked
 * up in the table every rank has; the column sums travel as pairs) --, sorted grids, at most 8 ranks; anything else (EvA / AvE, a
 * pre-populated row set, unsorted grids) is built redundantly on every rank (same result).  ibh_weighted_built_fast reports 3 for a shared build.  A custom transport needs
 * ibh_comm_set_custom_gatherv.  No smoothing: ibh_regrid_matrices_matrix_d_sharded_sigma. */
int ibh_regrid_matrices_matrix_d_sharded(const ibh_regrid_matrices *rm, ibh_comm *c, const char *spec, ibh_sparse_set *dim0,
                                         ibh_sparse_set *dim1, int scale, int correctA, ibh_weighted **out);
/* The same with RegridParams' sigma (IvA / IvE smoothed, as the coupler's IvE, IceCoupler.cpp:461-463): bitwise
 * ibh_regrid_matrices_matrix_d(..., sigma) on every rank, conservative = 0.  The unsmoothed matrix comes from the shared build
 * above; the smoothing's spatial-tile form (grids of more than ibh_set_tuning "smooth_direct_max_rows" rows) is shared too --
 * rank k smooths the rows of a contiguous range of spatial bins balanced by work, the rows travel through the gatherv --, its
 * direct form and the triplet pipeline run on every rank.  ibh_weighted_built_fast: 3 when the smoothing was shared, 1 when it
 * ran on every rank.  sigma NULL or zero: ibh_regrid_matrices_matrix_d_sharded.  Refusals as matrix_d: smoothing of an X-row
 * matrix IBH_ENOTIMPL; a sigma component <= 0 or no ice-grid centroids IBH_EINVAL. */
int ibh_regrid_matrices_matrix_d_sharded_sigma(const ibh_regrid_matrices *rm, ibh_comm *c, const char *spec, ibh_sparse_set *dim0,
                                               ibh_sparse_set *dim1, int scale, int correctA, const double sigma[3], ibh_weighted **out);

/* Device pointers of the CSR and weights, for callers that keep fields resident
 * (IceCoupler.cpp:408,445,456 read ->M and ->wM directly). */
typedef struct ibh_weighted_device_view {
    int32_t nrow, ncol; int64_t nnz;
    const int32_t *rowptr, *colind; const double *val, *wM, *Mw;
} ibh_weighted_device_view;
int ibh_weighted_device_view_get(const ibh_weighted *w, ibh_weighted_device_view *out);

/* ------------------------------------------------------------------------- */
/* VectorMultivec: icebin::VectorMultivec (slib/icebin/multivec.hpp:16-69), the parallel sparse vectors the coupler
 * exchanges with the GCM, resident in HBM.  Layout as the reference's (multivec.hpp:25-31, :55-56): index int64[n],
 * weights double[n], vals double[n * nvar] with vals[ix * nvar + ivar].  Fewer than 2^31 entries.  Capacity grows
 * geometrically; after ibh_multivec_reserve(mv, n) appends up to n entries in all allocate nothing.
 *
 * Order of arithmetic: every sum over entries naming the same cell runs in ENTRY order, one product then one add, no
 * contraction, no floating-point atomics: each result is the reference loop's, bit for bit.  The merge calls
 * (to_dense_scale, to_dense, update_dense) share a grouping of the entries by index that the handle keeps until the
 * vector changes.
 *
 * Errors: an index < 0 or >= nE is IBH_EINVAL and the message names the entry (icebin_error, multivec.cpp:43,67).  The
 * check is one status word read back, so ibh_multivec_to_dense_scale / _to_dense / _update_dense SYNCHRONISE THE STREAM
 * ONCE when they group the entries (the first of them after a change; later ones only enqueue), and
 * ibh_multivec_densify_device / ibh_sparse_set_add_dense_multivec synchronise it like a matrix build.  On error the
 * output's contents are unspecified and the handle is unchanged. */
typedef struct ibh_multivec ibh_multivec;
/* VectorMultivec(nvar) (multivec.hpp:36); nvar < 1 is IBH_EINVAL.  size() (:39).  clear: n = 0, the capacity is kept. */
int ibh_multivec_create(int32_t nvar, ibh_multivec **out);
int ibh_multivec_destroy(ibh_multivec *mv);
int ibh_multivec_size(const ibh_multivec *mv, int64_t *n, int32_t *nvar);       /* either may be NULL */
int ibh_multivec_clear(ibh_multivec *mv);
int ibh_multivec_reserve(ibh_multivec *mv, int64_t n);
/* add() (multivec.cpp:8-13) for n entries at once, from host arrays: index[n], weights[n], vals[n * nvar]. */
int ibh_multivec_add_host(ibh_multivec *mv, int64_t n, const int64_t *index, const double *weights, const double *vals);
/* The public members index, weights, vals (multivec.hpp:25-29) copied to the host (any may be NULL), or as device
 * pointers, valid until the next call that appends. */
int ibh_multivec_get(const ibh_multivec *mv, int64_t *index, double *weights, double *vals);
typedef struct ibh_multivec_device_view {
    int64_t n; int32_t nvar;
    const int64_t *index; const double *weights, *vals;
} ibh_multivec_device_view;
int ibh_multivec_device_view_get(const ibh_multivec *mv, ibh_multivec_device_view *out);
/* "Sparsify while appending to the global VectorMultivec" (IceCoupler.cpp:447-458): one entry per dense row jj of w,
 * rows ascending: index = w's dims[0] to_sparse(jj), weight = wM(jj), values = dB_b[ivar * ldb + jj], the field-major
 * result of an apply of w (the transpose the reference's comment speaks of).  EVERY row is appended, as there; the
 * reference's gcm_ivalsX is a plain Eigen product, which a caller gets by passing fill = 0 to the apply.
 * nvar != the vector's is IBH_EINVAL.  A pure enqueue on `stream` when the capacity suffices. */
int ibh_multivec_append_weighted_device(ibh_multivec *mv, const ibh_weighted *w, const double *dB_b, int32_t nvar, int64_t ldb,
                                        void *stream);
/* update_topo's packing of the TOPO planes (modele/GCMCoupler_ModelE.cpp:1099-1164).  Appends, for ihc = 0..nclass-1 (outer)
 * and every cell c = 0..ncell-1 ascending with d_mask[c] != 0 || (d_mask0 && d_mask0[c] != 0) -- :1122, :1156; d_mask0 is the
 * previous step's mask (:1017, :1167), NULL: none -- one entry:
 *   index = c * index_stride_cell + ihc * index_stride_class (indexingA / indexingE's tuple_to_index), weight = 1.0,
 *   vals[k] = plane k at [ihc * plane_class_stride + c]   (type 0: double, copied bit for bit; type 1: int16, converted: the
 *             underice_d of :1090-1097 without the double plane)
 * d_planes: HOST array of nvar device pointers; plane_type: [nvar] on the host, NULL = all double.  *nkept = the kept cells
 * (may be NULL).  The nclass * nkept entries go behind the existing ones; no floating-point arithmetic but the conversion.
 * ONE host wait on `stream` (the count, which sizes the buffers).  ncell == 0 or nclass == 0 appends nothing.
 * IBH_EINVAL, naming the offender and before the vector is touched: a null handle, mask or plane (where one would be read),
 * nvar != the vector's, a plane type other than 0 or 1, ncell < 0, nclass < 0, a negative class stride, 2^31 cells or more, a
 * total of 2^31 entries or more.
 * The _many form packs several vectors from ONE pass over the masks (the A and the E vector of an update_topo share the list
 * of kept cells); a vector may be named by one pack only. */
typedef struct ibh_plane_pack {
    ibh_multivec *mv;
    const void *const *planes;      /* HOST array of nvar plane pointers: device planes for _device, host planes for _host */
    const int32_t *plane_type;      /* [nvar] on the host, NULL: all double */
    int32_t nvar, nclass;
    int64_t plane_class_stride, index_stride_cell, index_stride_class;
} ibh_plane_pack;
int ibh_multivec_append_planes_device(ibh_multivec *mv, const void *const *d_planes, const int32_t *plane_type, int32_t nvar, int64_t ncell,
                                      int32_t nclass, int64_t plane_class_stride, const int16_t *d_mask, const int16_t *d_mask0,
                                      int64_t index_stride_cell, int64_t index_stride_class, int64_t *nkept, void *stream);
int ibh_multivec_append_planes_many_device(const ibh_plane_pack *packs, int32_t npack, int64_t ncell, const int16_t *d_mask,
                                           const int16_t *d_mask0, int64_t *nkept, void *stream);
/* The same from host arrays (plane k holds (nclass - 1) * plane_class_stride + ncell elements): copied in, the device call
 * runs on the default stream. */
int ibh_multivec_append_planes_host(ibh_multivec *mv, const void *const *planes, const int32_t *plane_type, int32_t nvar, int64_t ncell,
                                    int32_t nclass, int64_t plane_class_stride, const int16_t *mask, const int16_t *mask0,
                                    int64_t index_stride_cell, int64_t index_stride_class, int64_t *nkept);
int ibh_multivec_append_planes_many_host(const ibh_plane_pack *packs, int32_t npack, int64_t ncell, const int16_t *mask, const int16_t *mask0,
                                         int64_t *nkept);
/* couple()'s unit conversion (modele/GCMCoupler_ModelE.cpp:1216-1228) over ALL entries: vals[ix * nvar + k] = vals[ix * nvar + k]
 * * mm[k] + bb[k], one product then one add, no contraction.  mm, bb: [nvar] on the host, read during the call.  A pure enqueue;
 * no index changes, so the grouping of the merge calls stays valid. */
int ibh_multivec_affine_device(ibh_multivec *mv, const double *mm, const double *bb, void *stream);
/* concatenate() (multivec.cpp:15-33): the entries of `other` behind mv's / of mvs[0..k) in order into a new vector.
 * k == 0 or differing nvar is IBH_EINVAL (:19-20, :29-30).  Device copies on the default stream. */
int ibh_multivec_append(ibh_multivec *mv, const ibh_multivec *other);
int ibh_multivec_concatenate(int32_t k, const ibh_multivec *const *mvs, ibh_multivec **out);
/* to_dense_scale() (multivec.cpp:35-50): d_scale[nE] (device) = 0, += weights in entry order, then 1/x of EVERY
 * element: a cell no entry names holds +inf. */
int ibh_multivec_to_dense_scale(const ibh_multivec *mv, int64_t nE, double *d_scale, void *stream);
/* to_dense() (multivec.cpp:55-81) for all variables at once: d_out[ivar * ld + iE] (device).  The reference's rule is kept
 * as it is: a cell starts untouched (NaN); per entry p = val * scale[iE]; a NaN running value BECOMES p, else p is added;
 * a cell that ends NaN gets `fill`.  So a NaN term is forgotten once another follows it, and a trailing one (or a zero
 * weight sum, 0 * inf) becomes `fill`. */
int ibh_multivec_to_dense(const ibh_multivec *mv, const double *d_scale, double fill, double *d_out, int64_t ld, int64_t nE,
                          void *stream);
/* The in-place update of the GCM's arrays (modele/GCMCoupler_ModelE.cpp:864-892): the cells the entries name are set to
 * 0.0, then += val * scale[iE] in entry order; all other cells keep their contents.  The (j,i) / (ihc,j,i) index
 * arithmetic and the clearing of a whole elevation-class column (:918) are ModelE's and stay with the caller. */
int ibh_multivec_update_dense(const ibh_multivec *mv, const double *d_scale, double *d_out, int64_t ld, int64_t nE, void *stream);
/* dimE0->add_dense(index[i]) for every entry in order (IceCoupler.cpp:294-300), on the device: a pre-populated set is
 * appended to, first-seen.  An index < 0 or beyond the set's sparse extent is IBH_EINVAL and leaves the set as it was. */
int ibh_sparse_set_add_dense_multivec(ibh_sparse_set *set, const ibh_multivec *mv, void *stream);
/* Densify onto a set (IceCoupler.cpp:306-314): d_out[nvar x dense_extent] (device, row stride ld) = 0, then
 * d_out[ivar * ld + to_dense(index[i])] += val(ivar, i) in entry order; the weights are not used.  An index the set
 * lacks is IBH_EINVAL (to_dense raises there, :310). */
int ibh_multivec_densify_device(const ibh_multivec *mv, const ibh_sparse_set *set, double *d_out, int64_t ld, void *stream);
/* Host-array forms of three of the calls above, for a caller that holds no device arrays (the blitz arrays of
 * multivec.cpp:35-81 and the Eigen product of IceCoupler.cpp:445-458 live on the host): the arrays are copied to the
 * device, the device call runs on the default stream, the result is copied back.  Same bits, same refusals. */
int ibh_multivec_append_weighted_host(ibh_multivec *mv, const ibh_weighted *w, const double *B_b, int32_t nvar, int64_t ldb);
int ibh_multivec_to_dense_scale_host(const ibh_multivec *mv, int64_t nE, double *scale /* [nE] */);
int ibh_multivec_to_dense_host(const ibh_multivec *mv, const double *scale, double fill, double *out /* [nvar x ld] */, int64_t ld,
                               int64_t nE);

/* Tuning / introspection (not part of the reference interface). */
int ibh_weighted_set_kernel(ibh_weighted *w, const char *name_or_auto);   /* "auto", "rowblock", "shortrow", "rowdual", "colsweep", "rowgroup" */
int ibh_weighted_last_kernel(const ibh_weighted *w, char *buf, int buflen);
/* The kernel INSTANTIATION the last apply launched, spelled as rocprofv3 prints it ("spmm_rowblock_kernel<1, 1, 14, 8, false>",
 * "spmm_rowone_kernel<8, 14>", "spmm_shortrow_kernel<true, 8, false, true>", the band kernel "spmm_rowblock_kernel<2, 1, 4, 4, true>",
 * "spmm_sweep_kernel<true, false, 0>"; "" before the first apply): bench.py checks it against the kernel a committed PMC profile
 * was taken on before quoting that profile's traffic. */
int ibh_weighted_last_launch(const ibh_weighted *w, char *buf, int buflen);
/* A launch option of THIS matrix (the apply-side keys of ibh_set_tuning: rowblock_*, rowone*, rowgroup_*, shortrow_*, sweep_*,
 * rowdual_*, lazy_structures): read before the process-wide map by every apply / prepare of this handle, so host threads that
 * tune different matrices do not interfere.  value INT32_MIN removes the option.  Like every call on a handle: not concurrently
 * with an apply of the same handle. */
int ibh_weighted_set_option(ibh_weighted *w, const char *key, int value);
/* 1 when the matrix was assembled by the plan-based fast path for sorted exchange grids (fastasm.inl), 3 when the ranks of a
 * communicator shared the streamed build (ibh_regrid_matrices_matrix_d_sharded), 2 when its streamed
 * variant did (streamasm.inl: grids of 2^20 exchange cells and more; ibh_set_tuning("assemble_stream", 0 | 1) overrides),
 * 0 when the general pipeline built it (ibh_set_tuning("assemble_fast", 0) forces the latter).  Results are bit-identical. */
int ibh_weighted_built_fast(const ibh_weighted *w, int *out);
/* Which device form smoothed the matrix (sigma != 0, IvA / IvE): 0 not smoothed, 1 the triplet pipeline, 2 the direct form (one wave
 * per row), 3 the spatial tiles.  The forms are tried in the order tiles, direct, triplets as ibh_set_tuning "smooth_tile",
 * "smooth_direct" (1 always, 0 never, -1 by size: "smooth_direct_max_rows") admit them; a form whose tables overflow leaves the build
 * to the next one.  Same structure from every form, entries to rounding.  Introspection only. */
int ibh_weighted_smoothed_by(const ibh_weighted *w, int *out);
/* How a matrix of ibh_modele_matrices_matrix_d[_sigma] was composed: 0 not composed (any other matrix, AOmvAAm / AAmvAOm), 1 the
 * generic sparse product, 2 the row-local form (IvA IvE XvA XvE of a smoothed build, or under ibh_set_tuning("modele_rowlocal", 1)).
 * Same bits from both.  Introspection only. */
int ibh_weighted_composed_by(const ibh_weighted *w, int *out);
/* PROCESS-WIDE launch-heuristic overrides for measurements and tests -- experiments only; a product caller that needs a knob sets it
 * on the handle (ibh_weighted_set_option).  (README.md lists the keys: assemble_fast, assemble_fast_eva,
 * assemble_range_shape, assemble_stream_count, assemble_static_count, modele_rowlocal, rowgroup_*, rowone*, rowblock_*, shortrow_*, sweep_*,
 * lazy_structures ...).  No key changes a result beyond the documented tolerance of the kernel it selects; the assembly keys
 * change no bit.  value INT32_MIN: back to the built-in default. */
int ibh_set_tuning(const char *key, int value);
/* DIAGNOSTIC measurement hooks (bench.py only; not for product code: ibh_set_launch_events is thread-local
 * one-shot state that changes which launch API the calling thread's next apply uses): HIP events owned by
 * the library, and a one-shot request to attach a pair of them to the NEXT SpMM launch of the calling thread (hipExtLaunchKernel: start = the
 * kernel begins, stop = it ends -- the kernel's own duration, as rocprofv3's kernel trace reports it,
 * without the host's submission latency in front).  ibh_event_elapsed_ms waits for `stop`. */
int ibh_event_create(void **out);
int ibh_event_destroy(void *ev);
int ibh_event_elapsed_ms(void *start, void *stop, float *ms);
int ibh_set_launch_events(void *start, void *stop);
/* Diagnostic: run the assembly's ordering primitive (order analysis + independent-piece LDS sort,
 * falling back to the device-wide radix sort) on host keys with payload 0..n-1 and return the
 * resulting permutation, which must equal a stable sort by key.  key = (hi field << 32) | lo field,
 * fields below 2^hi_bits / 2^lo_bits.  *path_out: 0 already ordered, 1 pieces sorted in LDS,
 * 2 device-wide radix sort.  Used by tests/test_gpu_parity.py. */
int ibh_selftest_sort(const uint64_t *keys, int64_t n, int lo_bits, int hi_bits, uint32_t *perm_out, int *path_out);
/* Diagnostics of the assembly's integer primitives (prims.hip), one primitive per call on the calling thread's
 * per-thread stream; host buffers in and out.  Used by tests/test_gpu_prims.py.
 * ibh_selftest_scan: kind 0 = u32, 1 = u8 (in: n bytes), 2 = three-channel scan of packed words (out: 3n values,
 * channel by channel; total_out: 3 values).  out[i] = sum of in[0..i) mod 2^32; *total_out = the sum of all n.
 * flags: IBH_SCAN_IN_PLACE (u32 only: input and output are one device buffer), IBH_SCAN_FRESH_STATE (free the
 * thread's scan status buffer first), IBH_SCAN_NEAR_WRAP (move the status epoch to 2^30 - 2 first, so that the
 * call after this one takes the 30-bit rollover). */
#define IBH_SCAN_IN_PLACE     1
#define IBH_SCAN_FRESH_STATE  2
#define IBH_SCAN_NEAR_WRAP    4
int ibh_selftest_scan(int kind, const void *in, int64_t n, uint32_t *out, uint32_t *total_out, int flags);
/* The device-wide stable radix sort by `nfields` (shift, nbits) pairs, least significant field first, with
 * payload 0..n-1: the permuted keys (all 64 bits) and the payload. */
int ibh_selftest_radix_sort(const uint64_t *keys, int64_t n, const int32_t *fields, int nfields, uint64_t *keys_out,
                            uint32_t *perm_out);
/* As ibh_selftest_sort, and also the analysis: info_out = {flags, nchunks, maxlen, nsmall, nmid, nbig}.  try_pieces = 0:
 * the flags-only analysis followed by the radix sort it plans (the low field is skipped when it never decreases). */
int ibh_selftest_order(const uint64_t *keys, int64_t n, int lo_bits, int hi_bits, int try_pieces, uint32_t *perm_out,
                       uint32_t *info_out, int *path_out);
/* Diagnostic of the first-seen numbering of a key stream (sparseset.hip), as the Hntr matrices, global_ec and the global AvE
 * use it; host buffers in and out.  Used by tests/test_gpu_numbering.py.  The key of stream position p is keys[p * stride],
 * key_bytes 4 (int32) or 8 (int64); act (may be NULL): one byte per position, 0 = the numbering does not see it.  The old
 * set over [0, extent): n_old = -1 no set (the identity over the whole extent, which nothing can grow), else n_old entries,
 * the identity prefix (identity = 1) or to_sparse[n_old].  transform: IBH_ADD_DENSE, IBH_TO_DENSE or
 * IBH_TO_DENSE_IGNORE_MISSING.  check_range = 1: keys outside [0, extent) are skipped on the device and reported;
 * 0: such a key is IBH_EINVAL.  dense_out[n]: the dense id of every position, -1 where it is not seen, missing or out of
 * range; table_out (a set is given: room for n_old + min(n, extent) entries): the set's dense -> sparse table afterwards,
 * n_old + *n_new_out entries; *status_out: the IBH_NUMBER_KEYS_* bits (with OUT_OF_RANGE nothing is added, as a build
 * fails there). */
#define IBH_NUMBER_KEYS_OUT_OF_RANGE  1u    /* check_range: a key outside [0, extent) */
#define IBH_NUMBER_KEYS_MISSING       2u    /* IBH_TO_DENSE: a key the set lacks */
int ibh_selftest_number_keys(const void *keys, int key_bytes, int stride, int64_t n, const uint8_t *act, int64_t extent,
                             const int64_t *to_sparse, int32_t n_old, int identity, int transform, int check_range,
                             int32_t *dense_out, int64_t *table_out, int32_t *n_new_out, uint32_t *status_out);
/* Return the build workspaces of ALL host threads (the caller's and the library's worker threads') and
 * all cached device blocks to the driver (the library keeps freed device memory for reuse: a coupler
 * rebuilds the same matrices every step).  Call it while no build is in flight. */
int ibh_release_cached_memory(void);

#ifdef __cplusplus
}
#endif
#endif
