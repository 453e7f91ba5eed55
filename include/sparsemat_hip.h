/*
 * sparsemat_hip.h -- C ABI of libsparsemat_hip.so: the MI355X (gfx950) drop-in for the
 * CSR SpMV / BLAS-1 / CG hot path of the Rust crate lostinc0de/sparsemat.
 *
 * The host (Rust, C++ or Python) OWNS the CRS arrays; this library copies them to HBM
 * (or borrows device arrays the host already placed there) and runs hand-written HIP
 * kernels.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 * There is NO CPU fallback: without a HIP device every compute entry point fails with
 * SMH_ERR_NO_DEVICE.
 *
 * Conventions
 *   - every function returns an int status (SMH_OK == 0); a message for the calling
 *     thread's last failure is available from smh_last_error().  Nothing ever
 *     unwinds/throws across the ABI: the Rust shim turns a non-zero status into the
 *     reference's panic text.
 *   - host arrays are borrowed for the duration of the call only.
 *   - value type T is f32 or f64 (smh_dtype); index type I is u32 (the reference's
 *     SparseMatCRS<T,u32>; other index widths stay on the reference's CPU path).
 *   - `*_dev` entry points take DEVICE pointers and a hipStream_t (as void*; NULL is the
 *     HIP null stream, as everywhere in HIP) and are asynchronous; the others run on the
 *     handle's private stream and synchronise before returning.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the
 * reference repository root).
 */
#ifndef SPARSEMAT_HIP_H
#define SPARSEMAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  3 (round 4): smh_crs_tiled_layout is back to its version-2 form of SIX out pointers (round 3 had appended a
 * seventh without a version bump: a caller built against the older header would have had the library write through a garbage
 * pointer) and the product count has its own entry point, smh_crs_tiled_products; REMOVED since version 2:
 * smh_crs_set_stream_windows and smh_crs_stream_windows (K1s's column windows are chosen by the inspector alone; the K1s-w kernel
 * they steered left the library); ADDED: smh_crs_tiled_products, smh_crs_prepare_stats,
 * smh_comm_ranks_seen, smh_rccl_version, smh_par_set_threads,
 * smh_crs_stream_value_dict, smh_crs_set_stream_value_dict; ADDED later without a version change (additions only):
 * smh_update_plan_create, smh_update_plan_create_dev, smh_update_plan_execute, smh_update_plan_execute_dev,
 * smh_update_plan_stats, smh_update_plan_destroy; smh_crs_permute, smh_crs_permute_dev, smh_crs_permute_symmetric,
 * smh_crs_permute_symmetric_dev, smh_vec_permute, smh_vec_permute_dev, smh_crs_bandwidth, smh_crs_span_fraction, smh_crs_rcm,
 * smh_crs_rcm_dev; smh_crs_trisolve_levels, smh_crs_trisolve, smh_crs_trisolve_vec, smh_crs_sgs_apply_vec, smh_pcg_sgs_solve,
 * smh_pcg_sgs_solve_vec; smh_crs_color, smh_crs_color_dev; smh_crs_ilu0, smh_crs_ilu0_refactor, smh_crs_ilu_apply_vec,
 * smh_pcg_ilu_solve, smh_pcg_ilu_solve_vec; smh_gmres_solve, smh_gmres_solve_vec; smh_gmres_precond_solve,
 * smh_gmres_precond_solve_vec; smh_bicgstab_precond_solve, smh_bicgstab_precond_solve_vec; smh_crs_fsai, smh_crs_fsai_apply_vec,
 * smh_pcg_fsai_solve, smh_pcg_fsai_solve_vec; smh_crs_fsai_ns, smh_crs_fsai_ns_apply_vec, smh_gmres_fsai_solve, smh_gmres_fsai_solve_vec,
 * smh_bicgstab_fsai_solve, smh_bicgstab_fsai_solve_vec; smh_crs_cast, smh_vec_cast, smh_refine_solve, smh_refine_solve_vec; smh_eigsh, smh_eigsh_vec, smh_eigsh_last_timing.  A caller checks smh_abi_version() == SMH_ABI_VERSION once at load time (rust/src/lib.rs does). */
#define SMH_ABI_VERSION 3

/* ---- status codes ------------------------------------------------------------------ */
enum {
    SMH_OK = 0,
    SMH_ERR_DIM_MISMATCH = 1,  /* "Dimension mismatch" densevec.rs:53,62; "Matrix and vector size mismatch" linearsolver.rs:35 */
    SMH_ERR_NOT_SQUARE = 2,    /* "Matrix is not symmetric" linearsolver.rs:31 */
    SMH_ERR_INDEX_RANGE = 3,   /* a column index >= x.dim(): the implicit slice panic of densevec.rs:41 */
    SMH_ERR_INVALID = 4,       /* malformed CRS arrays / bad argument / misaligned device pointer */
    SMH_ERR_HIP = 5,           /* a HIP runtime call failed (message carries hipGetErrorString) */
    SMH_ERR_OOM = 6,           /* hipMalloc failed */
    SMH_ERR_NO_DEVICE = 7,     /* no HIP device: there is no CPU fallback */
    SMH_ERR_CAPACITY = 8,      /* nnz >= u32::MAX: "Maximum number of {} entries reached" sparsemat_crs.rs:82-84 */
    SMH_ERR_COMM = 9           /* an RCCL call failed (message carries ncclGetErrorString) */
};

typedef enum { SMH_F32 = 0, SMH_F64 = 1 } smh_dtype;

/* SpMV kernel families (DESIGN.md "Kernels") */
typedef enum {
    SMH_SPMV_AUTO = 0,   /* pick from the row-length statistics taken at create time        */
    SMH_SPMV_VECTOR = 1, /* K1: (sub-)wavefront per row, 16-B coalesced chunks, shfl reduce  */
    SMH_SPMV_MERGE = 2,  /* K2: merge-path tiles, LDS-staged products, deterministic fix-up  */
    SMH_SPMV_SEQ = 3,    /* one lane per row, storage order, mul then add: bit-exact vs the */
                         /* reference loop sparsematrix.rs:146-158 (checker, not fast)      */
    SMH_SPMV_STREAM = 4, /* K1s: short rows; dense entry stream, rounded products in LDS,   */
                         /* one thread folds a row in storage order: fast AND bit-exact     */
                         /* (stencil-like matrices stream 16-bit column codes, built once)  */
    SMH_SPMV_COLBLOCK = 5, /* K2c: columns without locality and x larger than an L2: the     */
                         /* device copy is split into blocks of 2^19 columns, y += A_b x    */
    SMH_SPMV_COLFUSED = 6, /* K2f: the same blocking in ONE sweep over y: a wave keeps the   */
                         /* sums of its rows in registers while all waves walk the column   */
                         /* blocks together (AUTO's choice when the rows are of similar     */
                         /* length; runs K2c when a (row, block) pair exceeds 255 entries)  */
    SMH_SPMV_COLSPLIT = 7, /* K2s: skewed rows without column locality (BASELINE C3): the rows */
                         /* of >= 64 entries as a compacted matrix through K2c, the rest     */
                         /* through K2f, y assembled from both (K2c when not worth it)      */
    SMH_SPMV_TILED = 8   /* K2t: columns without locality, two streaming passes over a 2-D   */
                         /* tiled copy: products against slices of x held in LDS, then one  */
                         /* wavefront per block of rows folds them (no gather leaves a CU)  */
} smh_spmv_variant;

/* sparse triangular solves: which triangle of the stored matrix, and whether its diagonal is the stored one or an implied 1 */
typedef enum { SMH_TRI_LOWER = 0, SMH_TRI_UPPER = 1 } smh_tri_uplo;
typedef enum { SMH_DIAG_NON_UNIT = 0, SMH_DIAG_UNIT = 1 } smh_tri_diag;

typedef struct smh_crs smh_crs; /* device-resident SparseMatCRS<T,u32>  (sparsemat_crs.rs:9-17) */
typedef struct smh_vec smh_vec; /* device-resident DenseVec<T>          (densevec.rs:5-7)      */
typedef struct smh_mvec smh_mvec; /* k device-resident DenseVec<T>s of one dimension, interleaved */

/* ---- library / device --------------------------------------------------------------- */
int smh_abi_version(void);
const char *smh_last_error(void);            /* thread-local, never NULL */
const char *smh_status_string(int status);   /* the reference's panic text for a status */
int smh_device_count(int *count_out);        /* 0 devices is SMH_OK with *count_out == 0 */
int smh_set_device(int device);              /* device used by handles created afterwards (per thread) */
int smh_device_synchronize(void);

/* ---- SparseMatCRS<T,u32> --------------------------------------------------------------
 * smh_crs_create: replaces building a SparseMatCRS (fields sparsemat_crs.rs:9-17; the
 * only bulk constructor, from_sparsemat_index :24-50, is pub(crate)): copies
 * offset_rows[n_rows+1], columns[nnz], values[nnz] to HBM.  Columns of a row are taken in
 * storage order, unsorted and with duplicates allowed, exactly as iter_row (:102-110)
 * yields them.  Monotone offsets, offset_rows[0]==0 and offset_rows[n_rows]==nnz are always
 * checked (on the device); validate != 0 additionally requires columns < n_cols.          */
int smh_crs_create(smh_dtype dtype, size_t n_rows, size_t n_cols, size_t nnz,
                   const uint32_t *offset_rows, const uint32_t *columns, const void *values,
                   int validate, smh_crs **out);
/* Same, over arrays that already live in device memory (borrowed, not copied, must outlive
 * the handle; columns/values 16-byte aligned).  device = ordinal owning the pointers.
 * Values written in place afterwards are announced with smh_crs_update_values(m, NULL): the K1r ring's
 * value records (smh_crs_ring_values) are derived from the values too, like the K2c copies. */
int smh_crs_create_dev(smh_dtype dtype, size_t n_rows, size_t n_cols, size_t nnz,
                       const uint32_t *offset_rows_dev, const uint32_t *columns_dev,
                       const void *values_dev, int validate, smh_crs **out);
/* ---- assembly on the device ----------------------------------------
 * smh_crs_assemble: replaces a stream of n_ops calls `mat.add_to(rows[k], cols[k], values[k])`
 * (ops == NULL or ops[k] == 0; sparsematrix.rs:231-233) / `mat.set(...)` (ops[k] == 1; :226-228)
 * on a SparseMatIndexList (get_mut sparsemat_indexlist.rs:158-164, push :45-53 over
 * indexlist.rs:62-83) followed by `to_crs()` (sparsemat_indexlist.rs:61-63 ->
 * sparsemat_crs.rs:24-50), with the identical result: n_rows = largest row + 1, n_cols =
 * largest column + 1, one entry per distinct (row, column) in order of first appearance
 * inside its row, value = left fold of the entry's operations in stream order from zero.
 * Bit-exact, including the values.  n_ops == 0 gives the empty matrix (no rows);
 * n_ops >= u32::MAX is SMH_ERR_CAPACITY (indexlist.rs:69).  The _dev form takes device arrays. */
int smh_crs_assemble(smh_dtype dtype, size_t n_ops, const uint32_t *rows, const uint32_t *cols,
                     const void *values, const uint8_t *ops, smh_crs **out);
int smh_crs_assemble_dev(smh_dtype dtype, size_t n_ops, const uint32_t *rows_dev,
                         const uint32_t *cols_dev, const void *values_dev, const uint8_t *ops_dev,
                         smh_crs **out);
/* smh_crs_replay: the same stream applied to a SparseMatCRS itself -- get_mut sparsemat_crs.rs:143-149
 * over find_index :54-67 / push :71-92 -- which is the container SparseMatrix::transpose and ::prod
 * fill through `set` (sparsematrix.rs:174-210).  Same entries and values as smh_crs_assemble, but
 * a row stores them in REVERSE order of first appearance (push inserts at the row's start, :85-87),
 * and the container's first-push quirk is honoured (:75-81: the first push leaves n_rows == 0):
 * if the second operation's row is smaller than the first one's, the first entry is orphaned
 * (Vec::resize truncates offset_rows) -- no row reaches it, so it is not part of the result
 * arrays although the reference's n_non_zero_entries() still counts it and n_cols covers it; if
 * the second operation names the same (row, column), the first keeps an entry of its own at the
 * end of the row; a single operation gives a matrix without rows.  Bit-exact. */
int smh_crs_replay(smh_dtype dtype, size_t n_ops, const uint32_t *rows, const uint32_t *cols,
                   const void *values, const uint8_t *ops, smh_crs **out);
int smh_crs_replay_dev(smh_dtype dtype, size_t n_ops, const uint32_t *rows_dev,
                       const uint32_t *cols_dev, const void *values_dev, const uint8_t *ops_dev,
                       smh_crs **out);
/* SparseMatrix::transpose (sparsematrix.rs:174-184) of a SparseMatCRS: `ret.set(j, i, val)` for
 * every entry in row-major storage order, replayed as above (so row j of the result lists the
 * source rows in DESCENDING order of visit, duplicates of (i, j) keep the last value, and the
 * quirk drops the very first entry when the second stored entry has a smaller column). */
int smh_crs_transpose(const smh_crs *a, smh_crs **out);
/* Diagnostics: how this thread's last smh_crs_transpose was carried out -- 0 the general route (stable device-wide sort
 * by target row through the replay machinery), 1 two bucketed passes (csrc/transpose_bucket.hip: matrices with local
 * structure -- bands, stencils, block orderings -- without repeated entries; the same result bit for bit, about twice
 * as fast).  SMH_TRANSPOSE_BUCKETED=0 (environment) keeps every call on the general route. */
int smh_last_transpose_route(void);
/* ColumnIter::assemble_column_info (sparsemat_crs.rs:180-191) as flat arrays: rows[k] = row of
 * entry k (the reference's `rows` vector), and its per-column IndexList (entry indices in storage
 * order, indexlist.rs:62-83) as col_ptr[n_cols + 1] / entries[nnz]: iter_col(j) (:193-204, next
 * :211-219) yields (rows[e], values[e]) for e in entries[col_ptr[j] .. col_ptr[j+1]).  A column
 * index >= n_cols is SMH_ERR_INDEX_RANGE.  The _dev form writes device arrays. */
int smh_crs_column_info(const smh_crs *m, uint32_t *rows, uint32_t *col_ptr, uint32_t *entries);
int smh_crs_column_info_dev(const smh_crs *m, uint32_t *rows_dev, uint32_t *col_ptr_dev,
                            uint32_t *entries_dev);
/* SparseMatrix::prod (sparsematrix.rs:186-210), self = a, rhs = b, both SparseMatCRS: the matrix the
 * reference's loops leave in a fresh SparseMatCRS -- entry (i, j) = the sum over rhs' column j in
 * storage order of val(i, row) * val_rhs with the same order of additions (bit-exact), sums that
 * compare == 0 dropped (:203), rows in descending column order (ascending `set` calls into a CRS),
 * n_rows / n_cols = largest kept row / column + 1; one kept sum leaves a matrix without rows (the
 * first-push quirk).  The reference's Err("Dimension mismatch") (:188-190: a.n_rows != b.n_cols or
 * a.n_cols != b.n_rows) is SMH_ERR_DIM_MISMATCH.  No column tables are needed on rhs. */
int smh_crs_prod(const smh_crs *a, const smh_crs *b, smh_crs **out);
/* ---- reordering (EXTENSION: the reference has no permutation and no ordering; csrc/permute.hip, csrc/reorder.hip) -----------------
 * A permutation is n uint32_t with perm[new] = old (scipy's convention: A[perm][:, perm]).  Every array argument carries its
 * length: a length that is not the dimension it permutes is SMH_ERR_DIM_MISMATCH.  An entry >= n, or a value that occurs twice,
 * is SMH_ERR_INVALID, the message naming the first offending position.  Validation runs on the device before anything is
 * allocated for a result; on any error the operands are untouched and *out stays NULL.  The _dev forms take DEVICE arrays on the
 * handle's device and, like smh_crs_apply_dev, wait for all work on the device before they read them; every form has finished
 * when it returns.
 * smh_crs_permute: out[i][j] = a[row_perm[i]][col_perm[j]] -- row i of the result is row row_perm[i] of a with the same entries in
 * the same storage order, every column c relabelled to col_perm^-1[c], values copied bit for bit.  Unsorted and duplicate columns
 * stay as they are: the storage-order sums of smh_crs_spmv(SEQ / STREAM) are kept.  Either permutation may be NULL (identity, its
 * length ignored); rectangular matrices are allowed (row_perm: n_rows entries, col_perm: n_cols).  With a column permutation a
 * stored column >= n_cols is SMH_ERR_INDEX_RANGE.  The result is a new library-owned handle with a's smh_crs_set_* settings and
 * its own create-time statistics.  A handle holding an orphan (smh_crs_orphans) is SMH_ERR_INVALID.
 * smh_crs_permute_symmetric: P A P^T, i.e. smh_crs_permute(a, perm, perm); a not square is SMH_ERR_NOT_SQUARE. */
int smh_crs_permute(const smh_crs *a, const uint32_t *row_perm, size_t n_row_perm, const uint32_t *col_perm, size_t n_col_perm, smh_crs **out);
int smh_crs_permute_dev(const smh_crs *a, const uint32_t *row_perm_dev, size_t n_row_perm, const uint32_t *col_perm_dev, size_t n_col_perm,
                        smh_crs **out);
int smh_crs_permute_symmetric(const smh_crs *a, const uint32_t *perm, size_t n_perm, smh_crs **out);
int smh_crs_permute_symmetric_dev(const smh_crs *a, const uint32_t *perm_dev, size_t n_perm, smh_crs **out);
/* max i - j (*lower_out) and max j - i (*upper_out) over the stored entries, 0 for a matrix without entries: one pass, integer
 * max.  Either out may be NULL. */
int smh_crs_bandwidth(const smh_crs *m, uint32_t *lower_out, uint32_t *upper_out);
/* mean column span of a 64-row tile / n_cols: the locality statistic AUTO tests (taken on first use; also smh_crs_colblock's
 * span_fraction_out, without building that copy) */
int smh_crs_span_fraction(smh_crs *m, double *out);
/* The reverse Cuthill-McKee ordering of a square pattern: perm_out[n_rows] with perm_out[new] = old, ready for
 * smh_crs_permute_symmetric.  Not square: SMH_ERR_NOT_SQUARE; a stored column >= n_cols: SMH_ERR_INDEX_RANGE; 2^31 stored entries
 * or more: SMH_ERR_CAPACITY.  Definition (the result equals it exactly; values are never read):
 *   graph     vertices 0..n-1; u ~ v iff u != v and an entry (u, v) or (v, u) is stored -- stored zeros count, duplicates once;
 *             deg(v) = number of distinct neighbours;
 *   roots     while unvisited vertices remain, the root is the unvisited vertex with the smallest (deg, index): all isolated
 *             vertices come first, in index order;
 *   levels    from the root level by level: the next level is the set of unvisited neighbours of the current one; each new vertex
 *             v has the key (position in the order of its earliest-placed parent, deg(v), v) and the level is appended in
 *             ascending key order (Cuthill-McKee, ties broken by index);
 *   result    that order reversed.
 * *n_components_out counts roots, *n_levels_out levels over all components, root levels included (either may be NULL).
 * Cost: one round of a few kernels and one small read-back per level plus one per component -- a chain of n vertices takes n
 * rounds. */
int smh_crs_rcm(const smh_crs *m, uint32_t *perm_out, size_t *n_components_out, size_t *n_levels_out);
int smh_crs_rcm_dev(const smh_crs *m, uint32_t *perm_out_dev, size_t *n_components_out, size_t *n_levels_out);
/* A multicolour ordering of a square pattern (csrc/color.hip), for the level-scheduled triangular solves below: colors_out[n_rows] by
 * ORIGINAL row and perm_out[n_rows] with perm_out[new] = old, ready for smh_crs_permute_symmetric; either array may be NULL, and so
 * may either count.  Statuses as smh_crs_rcm's, in its order: not square SMH_ERR_NOT_SQUARE; a stored column >= n_cols
 * SMH_ERR_INDEX_RANGE; 2^31 stored entries or more SMH_ERR_CAPACITY.  n_rows == 0: SMH_OK, 0 colours, 0 rounds.  The _dev form takes the
 * two arrays on the handle's device, with the conventions of smh_crs_rcm_dev.  Definition (the result equals it exactly; values are
 * never read):
 *   graph     smh_crs_rcm's: vertices 0..n-1; u ~ v iff u != v and an entry (u, v) or (v, u) is stored -- stored zeros count,
 *             duplicates once; deg(v) = number of distinct neighbours;
 *   hash      h(v) = mix(v XOR seed) on 32 bits, mix the bijection x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b;
 *             x ^= x >> 16, all mod 2^32 (mix(1) = 0x688990c0);
 *   priority  the 64-bit key deg(v) << 32 | h(v): all keys are distinct; the largest degree comes first, the hash breaks ties;
 *   colour    visiting the vertices in DESCENDING key order, each takes the smallest colour >= 0 that no neighbour of higher key
 *             holds (sequential greedy in priority order: *n_colors_out <= max deg + 1);
 *   rounds    round(v) = 0 when no neighbour has a higher key, else 1 + max round(w) over the neighbours w of higher key;
 *             *n_rounds_out = 1 + max round -- the Jones-Plassmann schedule of the same colouring, which is what the device executes;
 *   result    perm_out = the vertices sorted by (colour, index): every colour a contiguous block, the original order kept inside it.
 * For a structurally symmetric pattern a row of colour c has a neighbour of every colour below c, so after
 * smh_crs_permute_symmetric(perm) the LOWER schedule's level_of_row IS the colour of that row and it has n_colors levels, UPPER at
 * most as many; for any other pattern both have at most n_colors.  Greedy with hashed ties does not find the 2 colours of a red-black
 * ordering (a grid takes 4 .. 6).  Cost: one kernel per round, one small read-back per batch of 4 .. 64 rounds, one radix sort. */
int smh_crs_color(const smh_crs *m, uint32_t seed, uint32_t *colors_out, uint32_t *perm_out, size_t *n_colors_out, size_t *n_rounds_out);
int smh_crs_color_dev(const smh_crs *m, uint32_t seed, uint32_t *colors_out_dev, uint32_t *perm_out_dev, size_t *n_colors_out, size_t *n_rounds_out);
/* #[derive(Clone)] (sparsemat_crs.rs:8): a new handle with copies of the dims, arrays, orphans and the smh_crs_set_* settings;
 * derived forms (codes, plans, column-blocked copies) are rebuilt lazily.  The copy is library-owned even when `a` borrows. */
int smh_crs_clone(const smh_crs *a, smh_crs **out);
/* SparseMatrix::add / sub (sparsematrix.rs:123-143): `*a.get_mut(i, j) += val` (-= val) for every entry of b, row by row in
 * storage order -- get_mut = find_index (the FIRST match in the row, sparsemat_crs.rs:54-67) or else push (inserts at the START
 * of the row, :71-92).  Bit for bit the reference's result:
 *   - n_rows = max(a.n_rows, 1 + last row of b holding an entry); empty trailing rows of b do not grow a;
 *   - n_cols = max(a.n_cols, 1 + largest column that created a NEW entry); matched columns and b.n_cols do not grow it;
 *   - row i = the new columns in REVERSE order of first appearance in b's row i, then a's row i unchanged in order;
 *   - a b entry whose column exists in a's row folds into the first occurrence (later repeats in a are left alone); a new
 *     entry folds from zero; folds run in b's storage order, one rounding per operation (acc + v; acc - v for sub);
 *   - exact zeros stay stored (unlike prod); a's orphan stays (smh_crs_orphans of the result == of a), b's is not visited.
 * a without rows and without an orphan (SparseMatCRS::new()): the result is smh_crs_replay of b's entries as add_to
 * operations (values negated for sub), first-push quirk and its orphan included, with n_cols at least a.n_cols (push only
 * raises it, :72-74).  a without rows but WITH an orphan: SMH_ERR_INVALID, a untouched -- the reference's hidden
 * offset_rows length decides whether the orphan comes back, and the handle does not keep it.  Entries plus orphans of the
 * result reaching u32::MAX: SMH_ERR_CAPACITY ("Maximum number of 4294967295 entries reached", :82-84), decided before
 * anything is allocated or written.  Different dtypes or devices: SMH_ERR_INVALID (a compile-time error in the reference).
 * No dimension check (the reference has none).  b may be a itself (a += a behaves as if b had been cloned first), and b's
 * private stream is synchronised before b is read.
 * smh_crs_add / smh_crs_sub: *out = a.clone() + b / a.clone() - b (Add / Sub, sparsematrix.rs:397-419); a is not changed.
 * smh_crs_add_assign / smh_crs_sub_assign: a += b / a -= b (AddAssign / SubAssign :372-388, i.e. a.add(&b)).  Every form
 * derived from a (merge tiles, K1s codes and value dictionary, K1r plan, K2c / K2f / K2s / K2t copies, statistics) is dropped
 * and rebuilt on next use.  Borrowed arrays (smh_crs_create_dev): if every b entry lands on an existing entry of a, the
 * values are updated in place in the lent value array (as smh_crs_scale does) and the handle keeps borrowing; otherwise the
 * handle moves to library-owned arrays and the lent arrays are not written at all. */
int smh_crs_add(const smh_crs *a, const smh_crs *b, smh_crs **out);
int smh_crs_sub(const smh_crs *a, const smh_crs *b, smh_crs **out);
int smh_crs_add_assign(smh_crs *a, const smh_crs *b);
int smh_crs_sub_assign(smh_crs *a, const smh_crs *b);
/* Diagnostics: how this thread's last add / sub was carried out (csrc/matadd.hip) -- 0 the general route (rows of a and b
 * merged and sorted stably by column; any row length; also a without rows, through the replay), 1 short rows (one thread per
 * row, rows of at most 64 entries), 2 structure unchanged (every b entry lands on an existing entry: values only; also an
 * empty b), 3 same pattern (b entry k lands on a entry k: element-wise).  Same bits on every route.  SMH_ADD_FAST=0
 * (environment) keeps every call on the general route. */
int smh_last_add_route(void);
/* SparseMatrix::get (sparsemat_crs.rs:136-142 via find_index :54-67): *value_out = the FIRST entry of row i whose column is
 * j, or zero (+0) when there is none or i >= n_rows (an orphan is never reached).  value_out holds one value of the handle's
 * dtype.  smh_crs_get_many: the same for n queries (rows[k], cols[k]) -> values_out[k], host arrays; _dev: device arrays on
 * the handle's device (SMH_ERR_INVALID otherwise).  The _dev forms wait for all work on the device before they read the
 * arrays and have written the results when they return, as smh_crs_assemble_dev does.  NULL arrays with n > 0:
 * SMH_ERR_INVALID. */
int smh_crs_get(const smh_crs *m, size_t i, size_t j, void *value_out);
int smh_crs_get_many(const smh_crs *m, size_t n, const uint32_t *rows, const uint32_t *cols, void *values_out);
int smh_crs_get_many_dev(const smh_crs *m, size_t n, const uint32_t *rows_dev, const uint32_t *cols_dev, void *values_out_dev);
/* A stream of set / add_to calls on an existing handle, in stream order (sparsematrix.rs:224-233): m.add_to(rows[k], cols[k],
 * values[k]) when ops is NULL or ops[k] == 0, m.set(...) when ops[k] != 0 -- get_mut = find_index (the FIRST match in the
 * row) or else push (inserts at the START of the row, sparsemat_crs.rs:71-92).  Bit for bit the reference's result; for a
 * handle with rows:
 *   - n_rows = max(m.n_rows, 1 + largest row of any operation) (an operation on a row >= m.n_rows always creates an entry);
 *   - n_cols = max(m.n_cols, 1 + largest column that created a NEW entry);
 *   - row i = its new columns in REVERSE order of first appearance among the stream's operations on row i, then m's row i
 *     unchanged;
 *   - an operation whose (row, column) exists in m's row goes to the first occurrence (later repeats in m are left alone);
 *   - every target is the left fold of its operations in stream order, from m's value or from +0 for a new entry: add_to is
 *     acc + v (one rounding), set is v.  So add_to(-0.0) on a new entry gives +0, set(-0.0) gives -0;
 *   - m's orphan stays (smh_crs_orphans unchanged).
 * A handle without rows and without an orphan (SparseMatCRS::new()): the result is smh_crs_replay of the stream, first-push
 * quirk included, with n_cols at least m.n_cols.  A handle without rows but with one orphan -- the state the first push
 * leaves, made by a one-operation replay / transpose / add-to-empty and smh_crs_eye(1), which keep that operation on the
 * handle (smh_crs_clone copies it, smh_crs_scale scales its value as it scales stored values) -- continues the same way: the replay of (that operation ++ the stream).  Such a handle
 * without the operation: SMH_ERR_INVALID, m untouched.  Entries plus orphans reaching u32::MAX: SMH_ERR_CAPACITY, decided
 * before anything is allocated or written; n_ops == 0 leaves m untouched.  NULL arrays with n_ops > 0: SMH_ERR_INVALID.
 * Derived forms: when every operation lands on an existing entry, the values are folded in place (a borrowed value array,
 * smh_crs_create_dev, is written where it is and stays borrowed); every form derived from the structure stays and the
 * value-derived ones are refreshed as smh_crs_update_values(m, NULL) does.  Otherwise the handle is rebuilt on
 * library-owned arrays as smh_crs_add_assign rebuilds it (derived forms rebuilt on next use, smh_crs_set_* settings kept,
 * lent arrays not written).  Every target's operations are folded by one GPU thread in stream order, so a stream piling very
 * many operations onto one entry is folded serially.  _dev: device arrays (ops may be NULL) under smh_crs_get_many_dev's rules.  Not under a stream
 * capture. */
int smh_crs_apply(smh_crs *m, size_t n_ops, const uint32_t *rows, const uint32_t *cols, const void *values, const uint8_t *ops);
int smh_crs_apply_dev(smh_crs *m, size_t n_ops, const uint32_t *rows_dev, const uint32_t *cols_dev, const void *values_dev,
                      const uint8_t *ops_dev);
/* Diagnostics: how this thread's last smh_crs_apply[_dev] was carried out (csrc/matupdate.hip) -- 0 the general route (the
 * operations split into those with a target and those creating entries, both sorted; the handle is rebuilt), 1 values only
 * (every operation lands on an existing entry: sorted by target and folded in place; also n_ops == 0), 2 replay (a handle
 * without rows).  Same bits on every route.  SMH_APPLY_FAST=0 (environment) sends every handle with rows to the general
 * route. */
int smh_last_apply_route(void);
/* A reusable update plan: re-assembly on a FIXED pattern (csrc/matplan.hip).  smh_crs_apply on a stream whose operations all
 * land on existing entries looks every target up, sorts the stream by target and folds -- and only the fold depends on the
 * values.  A plan keeps the targets and the sorted order of one (rows, cols, ops) stream; executing it with n_ops new values
 * is one gather-and-fold pass.
 * Create: ops as for smh_crs_apply (NULL or ops[k] == 0: add_to, else set); _dev: device arrays under smh_crs_apply_dev's
 * rules.  EVERY operation must land on an existing entry of m (the first match in its row, as find_index picks it);
 * otherwise SMH_ERR_INVALID, the message giving the number of operations without one, m untouched, *out NULL.  To plan a
 * stream that first has to create entries: call smh_crs_apply once -- its general route creates them -- and make the plan
 * on the resulting handle.  A handle without rows: SMH_ERR_INVALID.  n_ops == 0: a valid plan whose execute does nothing.
 * n_ops >= u32::MAX: SMH_ERR_CAPACITY.  NULL arrays with n_ops > 0: SMH_ERR_INVALID.
 * Execute: `values` holds n_ops values of the handle's dtype in stream order (host array: uploaded through a staging buffer
 * the plan keeps; _dev: under smh_crs_apply_dev's rules); both forms have finished when they return.  With from_zero == 0, m
 * is afterwards what smh_crs_apply(m, n_ops, rows, cols, values, ops) leaves, bit for bit: every target the left fold of its
 * operations in stream order from the stored value (add_to: acc + v, one rounding; set: v).  With from_zero != 0 the fold
 * of every TARGETED entry starts from +0 instead -- the stream `set(r, c, +0)` for every distinct (row, column), then the
 * stream itself: "zero, then assemble" without a second pass; entries the stream never targets are not touched.  Operations
 * in front of their target's last `set` cannot reach the result and are dropped when the plan is made (n_live_ops counts the
 * rest).  Execute allocates nothing on the device and sorts nothing.  The handle is treated as apply's values-only route
 * treats it (smh_crs_update_values(m, NULL): structure-derived forms stay, value-derived ones are refreshed or dropped); a
 * borrowed value array is written in place and stays borrowed.  Not under a stream capture.
 * Binding: a plan belongs to one handle in one structure.  Executing it on another handle (a clone included), or after the
 * handle's offsets, columns or storage order changed (smh_crs_sort_rows; an apply / add_assign / sub_assign that rebuilt the
 * handle), is SMH_ERR_INVALID and writes nothing; smh_crs_scale, smh_crs_update_values, values-only apply / add_assign and
 * other plans' executes leave it valid.  m may be destroyed first: the plan can then only be destroyed.  A plan and its
 * handle follow the threading rule of a handle.
 * Stats (any out may be NULL): operations of the stream, distinct targets, kept operations, most operations on one target
 * (dropped ones included), the number of kept operations above which a run is folded by a workgroup of its own instead of
 * one thread, and the bytes of device memory the plan holds. */
typedef struct smh_update_plan smh_update_plan;
int smh_update_plan_create(const smh_crs *m, size_t n_ops, const uint32_t *rows, const uint32_t *cols, const uint8_t *ops,
                           smh_update_plan **out);
int smh_update_plan_create_dev(const smh_crs *m, size_t n_ops, const uint32_t *rows_dev, const uint32_t *cols_dev,
                               const uint8_t *ops_dev, smh_update_plan **out);
int smh_update_plan_execute(smh_update_plan *p, smh_crs *m, const void *values, int from_zero);
int smh_update_plan_execute_dev(smh_update_plan *p, smh_crs *m, const void *values_dev, int from_zero);
int smh_update_plan_stats(const smh_update_plan *p, size_t *n_ops, size_t *n_targets, size_t *n_live_ops, size_t *longest_run,
                          size_t *long_run_threshold, size_t *device_bytes);
int smh_update_plan_destroy(smh_update_plan *p);
/* SparseMatrix::eye (sparsematrix.rs:91-98) on a SparseMatCRS, i.e. set(i, i, 1) for i < dim: dim 0 the empty matrix; dim 1
 * no rows, one orphan, n_cols 1 (the first-push quirk; the operation is kept as for a one-operation replay); dim >= 2 the
 * identity (built directly, without a sort). */
int smh_crs_eye(smh_dtype dtype, size_t dim, smh_crs **out);
/* is_symmetric (sparsematrix.rs:212-222: get(j, i) != val for some stored entry -> false; get takes
 * the first match in storage order) and is_sorted (:251-271): *out = 1 / 0. */
int smh_crs_is_symmetric(const smh_crs *m, int *out);
int smh_crs_is_sorted(const smh_crs *m, int *out);
/* Sortable::sort_row (sparsemat_crs.rs:163-172) for every row: ascending columns, stable
 * (duplicates of a column keep their storage order).  Sorts the handle's arrays in place. */
int smh_crs_sort_rows(smh_crs *m);
int smh_crs_destroy(smh_crs *m);
/* host mutated values: re-upload.  values_host == NULL: the device values (borrowed arrays of
 * smh_crs_create_dev) were changed in place -- derived copies (K2c) are rebuilt on next use.
 * The K1r ring's value records (smh_crs_ring_values) are derived from the values too: they are dropped here, and the next
 * product tests the new values and builds them again or streams the value array. */
int smh_crs_update_values(smh_crs *m, const void *values_host);
int smh_crs_download(const smh_crs *m, uint32_t *offset_rows, uint32_t *columns, void *values);
/* n_rows :124-126, n_cols :128-130, n_non_zero_entries :132-134 */
size_t smh_crs_n_rows(const smh_crs *m);
size_t smh_crs_n_cols(const smh_crs *m);
size_t smh_crs_nnz(const smh_crs *m);
/* entries the reference's SparseMatCRS would still hold in columns / values although no row reaches them (the first-push
 * quirk of smh_crs_replay / smh_crs_transpose / smh_crs_prod, see smh_crs_replay): 0 or 1.  The reference's
 * n_non_zero_entries() (= columns.len(), sparsemat_crs.rs:132-134) and density() count them: they equal
 * smh_crs_nnz() + smh_crs_orphans(); the arrays of this handle hold smh_crs_nnz() entries. */
size_t smh_crs_orphans(const smh_crs *m);
int smh_crs_dtype(const smh_crs *m);
int smh_crs_max_row_len(const smh_crs *m, uint32_t *out);
/* smallest / largest column index stored (0/0 for a matrix without entries): the part of x a
 * row block references -- what SparseMatPar exchanges between ranks */
int smh_crs_col_range(const smh_crs *m, uint32_t *min_out, uint32_t *max_out);
/* SparseMatrix::scale (sparsemat_crs.rs:153-157): values *= a */
int smh_crs_scale(smh_crs *m, double a);
/* variant AUTO resolves to; lanes_out = lanes per row of the VECTOR kernel */
int smh_crs_resolved_variant(const smh_crs *m, int *variant_out, int *lanes_out);
/* override the VECTOR kernel's lanes-per-row (1,2,4,...,64; 0 = automatic) */
int smh_crs_set_vector_lanes(smh_crs *m, int lanes);
/* K1s XS, the STREAM kernel for coded single-pass tiles with the tile's column intervals of x staged in LDS by 16-byte loads
 * issued before the tile's own: mode -1 = automatic (x beyond the L2s; 2048 entries of x per tile, 4096 on f32),
 * 0 = never, 1 = whenever every tile's intervals fit a stage.  smh_crs_stream_layout reports what a STREAM launch of this
 * matrix uses: 16-bit column codes, byte row lengths, the two-chunk body (no tile above 2045 entries) and the 16-byte chunks
 * of x per thread staged (0 none, 2 or 4); a launch still falls back to gathers from memory when x is not 16-byte aligned
 * (the staged pieces are aligned 16-byte blocks of x: the last one may be read up to 12 bytes past x_len, inside the block --
 * and page -- that holds x's last entry; those values are never used).  Same bits as K1s in every form. */
int smh_crs_set_stream_xs(smh_crs *m, int mode);
int smh_crs_stream_layout(smh_crs *m, int *coded_out, int *byte_lengths_out, int *small_tiles_out, int *xs_chunks_out);
/* K1s XD-V, the value dictionary of the CSR-stream kernel (spmv_stream_xd.hip): when the matrix holds at most 32 distinct values (bit
 * patterns; 16 with the 4096-entry stage of x) -- every constant-coefficient stencil, unweighted graph Laplacians, adjacency matrices --
 * and the kernel runs with stage offsets (K1s XD), the spare bits of the 16-bit codes name each entry's value in a dictionary and the
 * value array is not read by the product: 2 bytes per entry instead of 6 (f32) / 10 (f64).  Same products, same order of additions:
 * still bit for bit SparseMatrix::mvp (sparsematrix.rs:146-158).  Built by smh_crs_prepare / the first product; smh_crs_update_values
 * makes the library look again, smh_crs_scale scales the dictionary.  *n_values_out: entries of the dictionary in use, 0 = the form is
 * not active; values_out (optional): room for 32 values.  smh_crs_set_stream_value_dict: -1 automatic, 0 never (SMH_STREAM_VDICT=0). */
int smh_crs_stream_value_dict(smh_crs *m, int *n_values_out, void *values_out);
int smh_crs_set_stream_value_dict(smh_crs *m, int mode);
/* K1s XD: the XS kernel with its per-entry address arithmetic moved into the build -- the 16-bit code array holds the byte offset
 * of x[col] inside the tile's LDS stage instead of (interval, offset), the products are staged unskewed, 16 bytes per store.  Same
 * bits again.  The unskewed stage collides on rows of even length, hence mode -1 = automatic (when x is staged and most rows have
 * an odd length: stencils with a diagonal), 0 = never, 1 = whenever x is staged.  A launch whose x cannot be staged (alignment,
 * length) streams the u32 columns instead.  smh_crs_stream_direct: does a STREAM launch of this matrix run in that form? */
int smh_crs_set_stream_direct(smh_crs *m, int mode);
int smh_crs_stream_direct(smh_crs *m, int *direct_out);
/* 16-B chunks per lane and pass of the pipelined VECTOR body (1..3; 0 = automatic): a lane group
 * covers 4*lanes*chunks entry slots of its row per pass */
int smh_crs_set_vector_chunks(smh_crs *m, int chunks);
/* K1r, the pipelined VECTOR kernel with an LDS-resident sliding window of x: mode -1 =
 * automatic (always; rows whose column span exceeds the ring gather from L2),
 * 0 = plain K1, 1 = same as -1.  The ring holds 16384 columns (64 KiB of f32 with two 512-thread
 * blocks per CU, 128 KiB of f64 with one 1024-thread block per CU).  When at least a quarter of
 * the rows run in ring phases the handle also keeps a u16 array with the low halves of the
 * columns (2 bytes per entry, built on first use): ring phases only need `column mod 16384` and
 * stream that array instead of the u32 columns (same arithmetic, bitwise identical results). */
int smh_crs_set_ring(smh_crs *m, int mode);
/* the K1r phase plan (integer structure, invariants checked in tests): phase_ptr_out needs
 * n_blocks+1 entries, phases_out 11 u32 per phase {row_begin,row_end,load_lo,load_hi,use_ring,
 * lo1,lo2,lo3,hi1,hi2,hi3} (load ranges of band 0 and, in banded plans, of bands 1..3);
 * call first with NULL arrays to get the sizes.                                           */
/* columns the ring of this matrix's plan holds: 16384, or 32768 for f32 matrices whose rows need the
 * wider window (128 KiB of LDS, one 1024-thread block per CU) */
int smh_crs_ring_entries(smh_crs *m, uint32_t *out);
/* what the ring phases of the VECTOR family stream for their columns under the current settings (builds the plan and the
 * form on first use): 0 = the 32-bit columns (also when the ring kernel is not in use), 1 = 16-bit columns, 2 = the compact
 * form, 12 bits per column (f32 on the single-window ring of 16384 columns; SMH_RING_COL12 = auto / 0 / 1).  The form changes
 * speed only, never a result. */
int smh_crs_ring_column_form(smh_crs *m, int *form_out);
/* what those phases stream for their VALUES under the current settings (builds the plan and the forms on first use):
 * *form_out = 0: the value array itself; 1: 24-bit fixed-point values, four of them with the chunk's four low column bytes in one
 * 16-byte record (4.5 instead of 5.5 bytes per entry; *exponent_out = E, every value being k * 2^E with -2^23 <= k < 2^23);
 * -1: the matrix was tested and refused (some value is no such multiple, or is NaN, +-Inf, -0.0 or subnormal), it streams the value
 * array.  The form is taken only together with the compact column form (form 2 above), for a matrix ALL of whose streamed values
 * decode to their own bits -- checked value by value when the records are written -- so it changes speed only, never a result.
 * SMH_RING_VAL24 = auto / 0 / 1: 0 = never; 1 = same as auto (it cannot force a matrix that does not qualify).  exponent_out may
 * be NULL; it receives 0 unless *form_out is 1. */
int smh_crs_ring_values(smh_crs *m, int *form_out, int *exponent_out);
/* 1: one sliding window (slot = column mod ring size).  4: banded ring for rows that reference a few narrow
 * column intervals far apart (stencils): band k holds the k-th interval of the tiles, slot = k * S +
 * column mod S, S = ring size / 4.  intervals_out (optional, banded plans only): 8 u32 per 64-row tile,
 * {lo0,hi0,..,lo3,hi3} sorted and disjoint; all zero = tile without entries, [1,0) = not describable. */
int smh_crs_ring_bands(smh_crs *m, uint32_t *bands_out, uint32_t *intervals_out);
int smh_crs_ring_plan(smh_crs *m, uint32_t *n_blocks_out, size_t *n_phases_out,
                      double *ring_fraction_out, int *active_out, uint32_t *phase_ptr_out,
                      uint32_t *phases_out);
/* which phases of that plan are REGULAR (read-only; built with the plan): len_out[p], n_phases values, = L when phase p
 * gathers from the ring (use_ring == 1), L > 0 and offsets[r] == offsets[row_begin] + (r - row_begin) * L for every r in
 * [row_begin, row_end]; else 0.  Where every phase of the plan gathers from the ring, some phase is regular and the ring phases
 * stream 16-bit or 12-bit columns, the ring kernel computes the row offsets of the regular phases instead of streaming them
 * (SMH_RING_REGULAR = auto / 0: 0 = every phase loads its offsets).  The table changes speed only, never a result. */
int smh_crs_ring_regular(smh_crs *m, uint32_t *len_out);
/* which form of the ring kernel a plain product (no inner_prod) of the VECTOR family would launch NOW, under the current settings
 * and knobs (builds the plan and the forms on first use, like a product; the handle is not const for that reason):
 * *form_out = 0: the kernel with the three bodies (ring gathers, two kinds of global gathers); 1: the kernel with the regular and the
 * loading ring body (smh_crs_ring_regular); 2: the all-regular form -- f32 on the single-window ring of 16384 columns, EVERY phase
 * that holds rows regular: the regular body alone, in workgroups of 768 threads (24 wavefronts per CU instead of 16;
 * SMH_RING_ALLREG = auto / 0: 0 = form 1 instead); -1: the ring kernel is not in use (then the other two are 0).
 * *threads_out = the workgroup size, *resident_per_cu_out = how many such workgroups a compute unit holds at once, as
 * hipOccupancyMaxActiveBlocksPerMultiprocessor answers for that instantiation with its dynamic LDS (0: a matrix without entries
 * launches none).  inner_prod always runs form 0 or 1: the order of its sum goes with the wavefronts of a workgroup.  The form
 * changes speed only, never a result. */
int smh_crs_ring_launch_form(smh_crs *m, int *form_out, int *threads_out, int *resident_per_cu_out);

/* K2c, the column-blocked copy (built on first use; integer structure, checked bit-exact in tests):
 * block b holds the entries with column >> shift == b, as a CSR over all rows whose offsets
 * offsets_out[b*(n_rows+1) + r] are absolute positions into columns_out / values_out [nnz]; inside a
 * (row, block) pair the entries keep their storage order.  Call with NULL arrays for the sizes.
 * span_fraction_out (may be NULL): mean column span of a 64-row tile / n_cols, the locality
 * statistic AUTO uses (COLBLOCK when it exceeds 0.25 and x holds at least 4 MiB).  More than 128
 * blocks (n_cols > 2^26 at the default width) is SMH_ERR_INVALID.                              */
int smh_crs_set_colblock_shift(smh_crs *m, uint32_t shift); /* block = 2^shift columns; 0 = automatic (19) */
int smh_crs_colblock(smh_crs *m, uint32_t *shift_out, size_t *n_blocks_out, int *rows_per_thread_out,
                     double *span_fraction_out, uint32_t *offsets_out, uint32_t *columns_out,
                     void *values_out);

/* K2f, the fused column-blocked copy (built on first use; integer structure, checked bit-exact in tests): rows are
 * grouped into tiles -- tile t = rows [tile_rows[t], tile_rows[t+1]) = 64 lanes x h consecutive rows each, h <=
 * rows_per_lane chosen greedily in row order so that a tile holds at most 1.25x the entries of a mean full-height tile
 * (h = 1 when even 64 rows exceed that) -- and columns into blocks of 2^shift; the entries are sorted by (tile, block,
 * row, storage order).  segments_out[t * n_blocks + b] = position of the first entry of (tile t, block b)
 * (n_tiles * n_blocks + 1 values), counts_out[((t * n_blocks + b) * 64 + lane) * rows_per_lane + j] = entries of row
 * tile_rows[t] + lane * h + j in block b (one byte each; zero for j >= h), columns_out / values_out [nnz] the permuted
 * entries.  Call with NULL arrays for the sizes.  *fits_out == 0: a (row, block) pair holds more than 255 entries,
 * there is no such copy (SMH_SPMV_COLFUSED then runs K2c).  Block width: smh_crs_set_colblock_shift, default 2^18
 * columns; more than 255 blocks is SMH_ERR_INVALID. */
int smh_crs_colfused(smh_crs *m, int *fits_out, uint32_t *shift_out, size_t *n_blocks_out, uint32_t *rows_per_lane_out,
                     size_t *n_tiles_out, uint32_t *tile_rows_out, uint32_t *segments_out, uint8_t *counts_out,
                     uint32_t *columns_out, void *values_out);

/* K2t, the 2-D tiled copy (built on first use of SMH_SPMV_TILED; spmv_tiled.hip): the entries by column slice of
 * *slice_columns_out (16384) columns, within a slice by (row, storage order), cut into chunks of at most 64 E entries (E = 4 for
 * f32, 2 for f64: 16 bytes of values per lane) that start at row boundaries where one lies within 16 entries of the nominal
 * start; every chunk owns 64 E slots of the copy (*copy_entries_out slots in total, the unused ones zero).  Pass 1 multiplies a
 * chunk against the slice of x held in LDS and folds the entries of one row into one product sum, so a (row, slice) pair
 * yields one product (more only where a chunk boundary cuts it): *n_products_out product slots (each chunk's share padded to
 * 16 bytes).  The rows are cut into *n_row_blocks_out blocks of consecutive rows holding the same number of products -- about
 * 174 (f32) / 60 (f64) per (slice, row block) tile -- and at most *rows_per_block_out rows (the largest block); pass 2: one
 * wavefront per row block adds its tiles' products to wave-private row sums, slice by slice.  The sum of a row is therefore
 * taken per slice (slices ascending; inside a slice the fold order documented at the top of spmv_tiled.hip): within the parity
 * bound, bitwise reproducible, not bit-identical to the reference's storage-order fold.  A row's result can be -0.0 where the
 * reference (which starts every row from +0.0, sparsematrix.rs:149) returns +0.0 -- only when every product of the row is -0.0;
 * equal in value.  Memory: the copy (sizeof(T) + 2 bytes per slot), the products of the last launch (sizeof(T) + 2 bytes per
 * product slot) and a table of (n_row_blocks + 1) x n_slices u32 (beyond 4 GiB: SMH_ERR_INVALID).  Any out pointer may be NULL. */
int smh_crs_tiled_layout(smh_crs *m, uint32_t *n_slices_out, uint32_t *slice_columns_out, uint32_t *rows_per_block_out,
                         uint32_t *n_row_blocks_out, size_t *copy_entries_out);
/* ... and the number of product slots pass 1 writes / pass 2 reads (its own entry point: see the ABI history above). */
int smh_crs_tiled_products(smh_crs *m, size_t *n_products_out);

/* The arrays of that plan, for inspection (tests restate the build and the passes' summation order from them): `which` =
 * 0 first chunk of each slice (u32, n_slices + 1) | 1 per chunk {first product slot, entries} (2 x u32) | 2 the copy's 16-bit
 * codes (bit 15: same row as the entry before; bits 0-13: column within the slice) | 3 the copy's values | 4 per product slot:
 * its row relative to its row block, or rows_per_block for padding (u16) | 5 first row of each row block (u32, n_row_blocks + 1)
 * | 6 tile table: (n_row_blocks + 1) x n_slices first product slots (u32) | 7 the products of the last launch.  out == NULL: only
 * *bytes_out is set. */
int smh_crs_tiled_array(smh_crs *m, int which, void *out, size_t capacity_bytes, size_t *bytes_out);

/* K2s, the row-length split (built on first use): *split_out == 1 when the handle keeps its rows of >= *min_long_out
 * entries as a compacted sub-matrix (row i of it = row long_rows_out[i], n_long of them; global columns) and all rows
 * with those emptied as a second one -- both are ordinary handles owned by `m` (inspect, do not destroy) -- and 0 when
 * that is not worth it (long rows more than a quarter of the rows, or holding less than a quarter of the entries). */
int smh_crs_colsplit(smh_crs *m, int *split_out, uint32_t *min_long_out, size_t *n_long_out, uint32_t *long_rows_out,
                     smh_crs **long_out, smh_crs **short_out);

/* SparseMatrix::mvp (sparsematrix.rs:146-158) == `A * v` (Mul, sparsematrix.rs:435-443):
 * y[0..n_rows) = A.x.  x_len is x.dim(); a column index >= x_len is SMH_ERR_INDEX_RANGE
 * (the reference panics in densevec.rs:41).  y has exactly n_rows entries (ret.set grows
 * it one row at a time, vector.rs:40-42 / densevec.rs:44-49); empty rows give 0.        */
int smh_crs_spmv(smh_crs *m, const void *x_host, size_t x_len, void *y_host, int variant);
/* Builds now what the first product with `variant` would build lazily (K1r phase plan, merge-path
 * table, K2c blocked copy: device allocations and a synchronisation): call it before capturing
 * smh_crs_spmv_dev into a hipGraph of your own.  Never needed for correctness otherwise.      */
int smh_crs_prepare(smh_crs *m, int variant);
/* What the inspectors cost -- the reference has no set-up step at all (iter_row, sparsemat_crs.rs:102-110, is a slice zip), so an
 * honest comparison carries it.  Runs smh_crs_prepare(m, variant) (a no-op when already built) and reports, accumulated over the
 * handle's life: *prepare_ms_out = host wall time of the create-time inspection (statistics passes, K1r inspector) plus every
 * build smh_crs_prepare performed, device-synchronised; *derived_bytes_out = the device memory those builds left allocated
 * beside the CRS arrays (16-bit column arrays, code / phase tables, K2t's copy, product buffer and tile table ...; blocks below
 * 1 MiB are not counted).  A plan built lazily by a first product that was NOT preceded by smh_crs_prepare is not in the figures. */
int smh_crs_prepare_stats(smh_crs *m, int variant, double *prepare_ms_out, size_t *derived_bytes_out);
int smh_crs_spmv_dev(smh_crs *m, const void *x_dev, size_t x_len, void *y_dev, int variant,
                     void *stream);
/* SparseMatrix::inner_prod (sparsematrix.rs:161-171): lhs^T A rhs = sum over all entries of
 * lhs[i] * a_ij * rhs[j].  An lhs that ends at or before the last row holding entries, or a column
 * index >= rhs_len, is SMH_ERR_INDEX_RANGE (the reference panics in densevec.rs:41; rows without
 * entries never index lhs, so trailing empty rows may lie beyond lhs_len, as in the reference).
 * Computed as dot(lhs, A rhs): the dot rides the SpMV's epilogue where the kernel has one, then a
 * two-stage deterministic reduction (tolerance-level parity, like dot).  Rows without entries are
 * no terms of that dot either: NaN or Inf in lhs there does not reach the result. */
int smh_crs_inner_prod(smh_crs *m, const void *lhs_host, size_t lhs_len, const void *rhs_host,
                       size_t rhs_len, int variant, double *out);
/* merge-path tile table (integer structure, checked bit-exact in tests): tile t starts at
 * (row_out[t], nnz_out[t]); arrays need smh_crs_merge_tiles()+1 entries.                 */
size_t smh_crs_merge_tiles(const smh_crs *m);
size_t smh_crs_merge_tile_items(const smh_crs *m);
int smh_crs_merge_table(smh_crs *m, uint32_t *row_out, uint32_t *nnz_out);

/* ---- DenseVec<T> ------------------------------------------------------------------------
 * Vector::with_capacity/from_vec (densevec.rs:24-34), dim (:36-38), iter (:20-22)      */
int smh_vec_create(smh_dtype dtype, size_t n, smh_vec **out);                  /* zeros */
int smh_vec_from_host(smh_dtype dtype, size_t n, const void *host, smh_vec **out);
int smh_vec_wrap_dev(smh_dtype dtype, size_t n, void *dev_ptr, smh_vec **out); /* borrowed */
int smh_vec_destroy(smh_vec *v);
int smh_vec_upload(smh_vec *v, const void *host);
int smh_vec_download(const smh_vec *v, void *host);
size_t smh_vec_dim(const smh_vec *v);
int smh_vec_dtype(const smh_vec *v);
void *smh_vec_data(const smh_vec *v); /* device pointer */
int smh_vec_copy(smh_vec *dst, const smh_vec *src);                            /* clone() */
/* EXTENSION (see smh_crs_permute for permutations and their statuses): inverse == 0 gathers, dst[i] = src[perm[i]]; inverse != 0
 * scatters, dst[perm[i]] = src[i] -- so x.permute(p) undoes with permute(p, inverse).  dst and src: different vectors of equal
 * dimension (SMH_ERR_DIM_MISMATCH) and dtype (SMH_ERR_INVALID); perm has that many entries. */
int smh_vec_permute(smh_vec *dst, const smh_vec *src, const uint32_t *perm, size_t n_perm, int inverse);
int smh_vec_permute_dev(smh_vec *dst, const smh_vec *src, const uint32_t *perm_dev, size_t n_perm, int inverse);
/* Vector::add / sub / scale (densevec.rs:51-58, :60-67, :69-73; += -= *= sugar :76-96):
 * x += y, x -= y over the first y.dim() entries; SMH_ERR_DIM_MISMATCH iff x.dim() < y.dim().
 * ALIASING (handles made by smh_vec_wrap_dev can share storage; add, sub, axpy, xpby and the two element-wise smh_blas_*_dev
 * below alike): over the y.dim() entries an operation touches, the operand that is written and the one that is read are the SAME
 * storage (same device pointer: x.add(x) doubles x) or DISJOINT.  Byte ranges that overlap in part are refused with
 * SMH_ERR_INVALID ("... x and y overlap in part") before anything is launched, both buffers untouched: every thread writes its own
 * x[i] after reading y[i] and would read what another thread writes.  Entries of x behind y.dim() are neither read nor written
 * and do not count.  The operations that only read -- smh_vec_dot, smh_vec_norm_squared, smh_vec_norm, smh_blas_dot_dev -- take
 * any overlap. */
int smh_vec_add(smh_vec *x, const smh_vec *y);
int smh_vec_sub(smh_vec *x, const smh_vec *y);
int smh_vec_scale(smh_vec *x, double a);
/* y += round(a*x)  -- `*x += p.clone() * alpha` linearsolver.rs:47 (densevec.rs:121-130, :76-81) */
int smh_vec_axpy(smh_vec *y, double a, const smh_vec *x);
/* p = round(b*p) + r -- `p.scale(beta); p.add(&r)` linearsolver.rs:58-59 */
int smh_vec_xpby(smh_vec *p, double b, const smh_vec *r);
/* Vector::inner_prod (vector.rs:50-53; `v * w` densevec.rs:133-140), norm_squared (:56-58):
 * deterministic two-stage tree reduction in T, result widened to double (T::into::<f64>) */
int smh_vec_dot(const smh_vec *x, const smh_vec *y, double *out);
int smh_vec_norm_squared(const smh_vec *x, double *out);
int smh_vec_norm(const smh_vec *x, double *out); /* vector.rs:61-63 */
/* The same kernels on raw device pointers with DEVICE-resident scalars, asynchronous on `stream`:
 * the building blocks of the row-partitioned CG, whose scalars are all-reduced on the device.
 * dot: *result_dev = x.y (type T; scratch_dev needs smh_blas_dot_scratch_bytes()).
 * axpy: y += round(*a_dev * x) (linearsolver.rs:47,49).  xpby: p = round(*b_dev * p) + r (:58-59).
 * SMH_ERR_INVALID: a dtype that is not SMH_F32 / SMH_F64, a NULL pointer (x, y only when n > 0), and for axpy / xpby two buffers
 * whose n entries overlap in part (the aliasing rule above: the same pointer or disjoint). */
int smh_blas_dot_dev(smh_dtype dtype, const void *x_dev, const void *y_dev, size_t n, void *result_dev,
                     void *scratch_dev, void *stream);
size_t smh_blas_dot_scratch_bytes(void);
int smh_blas_axpy_dev(smh_dtype dtype, void *y_dev, const void *a_dev, const void *x_dev, size_t n, void *stream);
int smh_blas_xpby_dev(smh_dtype dtype, void *p_dev, const void *b_dev, const void *r_dev, size_t n, void *stream);
/* SparseMatrix::mvp on device vectors; y is resized semantics-free: y.dim() must be n_rows */
int smh_crs_spmv_vec(smh_crs *m, const smh_vec *x, smh_vec *y, int variant);
/* SparseMatrix::inner_prod on device vectors (sparsematrix.rs:161-171) */
int smh_crs_inner_prod_vec(smh_crs *m, const smh_vec *lhs, const smh_vec *rhs, int variant, double *out);

/* ---- k DenseVec<T>s of one dimension, held against one matrix ---------------------------------
 * The reference has no such type: its SparseMatrix::mvp (sparsematrix.rs:146-158) is generic over the vector and is
 * simply called once per right-hand side.  smh_mvec holds k vectors of dimension n (each what a DenseVec is,
 * densevec.rs:5-7) INTERLEAVED on the device: element i of vector c at data[i * ld + c], ld = k rounded up to a
 * multiple of 4; the padding columns are zero and stay zero.  `host` is always k vectors of n entries, one after the
 * other (k DenseVecs' iter(), densevec.rs:20-22, collected back to back); both transpositions run on the device.
 * k == 0, a bad dtype or n * ld * sizeof(T) overflowing is SMH_ERR_INVALID, reported before the device is asked for. */
int smh_mvec_create(smh_dtype dtype, size_t n, size_t k, smh_mvec **out);      /* zeros (Vector::with_capacity, densevec.rs:24-29, k times) */
int smh_mvec_from_host(smh_dtype dtype, size_t n, size_t k, const void *host, smh_mvec **out); /* from_vec (:31-34), k times */
int smh_mvec_upload(smh_mvec *mv, const void *host);
int smh_mvec_download(const smh_mvec *mv, void *host);
int smh_mvec_destroy(smh_mvec *mv);
size_t smh_mvec_dim(const smh_mvec *mv);   /* n: every vector's dim() (densevec.rs:36-38) */
size_t smh_mvec_count(const smh_mvec *mv); /* k */
size_t smh_mvec_ld(const smh_mvec *mv);    /* 4 * ceil(k / 4) */
int smh_mvec_dtype(const smh_mvec *mv);
void *smh_mvec_data(const smh_mvec *mv);   /* device pointer: n * ld elements, 16-byte aligned */
/* Column c <-> a DenseVec (clone(), densevec.rs:9 derive, of one vector): SMH_ERR_DIM_MISMATCH when v.dim() != n,
 * SMH_ERR_INVALID for c >= k or a dtype mismatch. */
int smh_mvec_set_column(smh_mvec *mv, size_t c, const smh_vec *v);
int smh_mvec_get_column(const smh_mvec *mv, size_t c, smh_vec *v);
/* The per-column BLAS-1 of k DenseVecs: every element-wise operation rounds once; the padding columns stay +0 whatever the
 * data (scale keeps them by selection: an infinite or NaN factor does not reach them).  `a` and `out` are host arrays of k
 * entries; scale multiplies column c by T(a[c]).  dot and norm_squared sum column c in a fixed tree whose order depends on
 * n alone -- not on k, on c or on the other columns -- and return T widened to f64.
 * Statuses, all decided on the host before any launch: SMH_ERR_DIM_MISMATCH when dim() or count() differ, SMH_ERR_INVALID for
 * a dtype mismatch or a NULL factor / output array. */
int smh_mvec_copy(smh_mvec *dst, const smh_mvec *src);
int smh_mvec_add(smh_mvec *x, const smh_mvec *y);                             /* x_c += y_c  (densevec.rs:51-58, k times) */
int smh_mvec_sub(smh_mvec *x, const smh_mvec *y);                             /* x_c -= y_c  (:60-67) */
int smh_mvec_scale(smh_mvec *x, const double *a);                             /* x_c *= T(a[c])  (:69-73) */
int smh_mvec_dot(const smh_mvec *x, const smh_mvec *y, double *out);          /* vector.rs:50-53 per column */
int smh_mvec_norm_squared(const smh_mvec *x, double *out);                    /* :56-58 */

/* SparseMatrix::mvp (sparsematrix.rs:146-158) for k right-hand sides in ONE sweep over the matrix (kernel K1m): for every
 * c < k, column c of y is bit for bit what smh_crs_spmv(m, x_c, ..., SMH_SPMV_SEQ) returns -- each product rounded, then added
 * in storage order from T(0), no FMA contraction; empty rows give +0 -- for any matrix the handle can hold and every k >= 1.
 * Padding columns of y are written as +0 whatever the data.  The kernel reads the handle's column and value arrays directly
 * (no derived form): smh_crs_update_values, smh_crs_scale and values written in place into borrowed arrays
 * (smh_crs_create_dev) take effect with the next product and need no refresh.
 * Statuses, all decided on the host before any launch: SMH_ERR_INVALID (k == 0, a dtype that is not the matrix's, x and y the
 * same storage, a device pointer that is not 16-byte aligned, ld < k or not a multiple of 4, n * ld * sizeof(T) overflowing);
 * SMH_ERR_INDEX_RANGE (a column index >= x.dim(): the reference panics in densevec.rs:41); SMH_ERR_DIM_MISMATCH (y.dim() !=
 * n_rows or y.count() != x.count()).
 * _dev: asynchronous on `stream`, raw interleaved device pointers (x: x_len * ld elements, y: n_rows * ld), no allocation and
 * no synchronisation.  _host: x_host is k x x_len and y_host k x n_rows in the host format above. */
int smh_crs_spmv_many(smh_crs *m, const smh_mvec *x, smh_mvec *y);
int smh_crs_spmv_many_dev(smh_crs *m, const void *x_dev, size_t x_len, void *y_dev, size_t k, size_t ld, void *stream);
int smh_crs_spmv_many_host(smh_crs *m, const void *x_host, size_t x_len, size_t k, void *y_host);

/* ---- ConjugateGradient::solve (linearsolver.rs:27-61) -----------------------------------
 * Device-resident: SpMV + fused updates + reductions, scalars (alpha, beta, r.r) stay in
 * HBM; the stop rule `sqrt(f64(r.r)) < tol`, tested before the beta update (:52-54), is
 * evaluated on the device every iteration and polled by the host every `check_every`
 * iterations (kernels of later iterations are no-ops once it fired, so x is exactly the x
 * of the iteration that converged).  tol/iter_max: the private fields :12-15 (Default
 * 1e-12 / 10000, :17-24).  Status: SMH_ERR_NOT_SQUARE (:30-32), SMH_ERR_DIM_MISMATCH
 * (:33-36).  iters_out = loop bodies entered (a body that breaks counts), rr_out = last
 * r.norm_squared() as f64.                                                               */
int smh_cg_solve(smh_crs *m, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len,
                 double tol, size_t iter_max, int variant, size_t *iters_out, double *rr_out);
int smh_cg_solve_vec(smh_crs *m, const smh_vec *b, smh_vec *x, double tol, size_t iter_max,
                     int variant, size_t check_every, size_t *iters_out, double *rr_out);
/* ... on k right-hand sides at once (kernel K5m): for every c < k, column c of x is ConjugateGradient::solve(A, b_c, x_c) --
 * its own alpha, beta, stop test and iteration count -- while all columns share one sweep over the matrix per body
 * (smh_crs_spmv_many) and fused multi-vector updates.  A column that has stopped (converged, or iter_max bodies entered) keeps
 * the bits of its stopping body; the solve ends when no column is active; no value of one column reaches another (b_c = 0
 * runs its 0 / 0 recurrence to iter_max like the reference and leaves its neighbours alone).  x: in x0, out the solution.
 * iters_out[c] = bodies column c entered, rr_out[c] = its last r.r as f64 (k entries each).  check_every: bodies per poll
 * (0: default).  Statuses, all decided on the host before any launch: SMH_ERR_NOT_SQUARE, SMH_ERR_DIM_MISMATCH (b.dim() or
 * x.dim() != n_rows, or the counts differ), SMH_ERR_INVALID (a dtype that is not the matrix's, b and x the same storage, NULL
 * output arrays); those of smh_crs_spmv_many pass through.  _host: b_host and x_host_inout are k x n in the host format. */
int smh_cg_solve_many(smh_crs *m, const smh_mvec *b, smh_mvec *x, double tol, size_t iter_max, size_t check_every,
                      size_t *iters_out, double *rr_out);
int smh_cg_solve_many_host(smh_crs *m, const void *b_host, size_t n, size_t k, void *x_host_inout, double tol,
                           size_t iter_max, size_t *iters_out, double *rr_out);

/* Diagnostics, per thread: how many batches this thread's last single-matrix device-resident solve (smh_cg_solve and every
 * solver below but the k-column CG) replayed from its captured hipGraph.  0: nothing was captured -- iter_max <= check_every, a
 * capture that did not come about, or another host thread was using the library (Threading): the bodies were
 * launched one by one, the same bits. */
int smh_last_solve_replays(void);

/* Jacobi-preconditioned CG -- an EXTENSION (the reference has no
 * preconditioner): the recurrence of ConjugateGradient::solve with z = r / diag(A), diag_i =
 * get(i, i) (first match in storage order); same guards, statuses, stop rule (on r.r, tested
 * before the beta update) and outputs as smh_cg_solve.  A zero or absent diagonal entry is
 * SMH_ERR_INVALID.  Host vectors; x is updated in place. */
int smh_pcg_jacobi_solve(smh_crs *m, const void *b_host, size_t b_len, void *x_host_inout,
                         size_t x_len, double tol, size_t iter_max, int variant, size_t *iters_out,
                         double *rr_out);

/* ---- sparse triangular solves and symmetric Gauss-Seidel -- EXTENSIONS (the reference has neither) ----------------------------
 * The triangle of a square handle: for uplo = SMH_TRI_LOWER the stored entries (i, c) with c < i, for SMH_TRI_UPPER those with
 * c > i, and the diagonal; entries of the other triangle are ignored.  The solve is level-scheduled: the dependency of row i is
 * every stored column c in the triangle's strict part (stored zeros count, duplicates once); level(i) = 0 without one, else
 * 1 + max level(c).  The schedule is a derived form of the handle, built on the device on first use, one per uplo: the rows of
 * each level, and for every row the position of its diagonal entry -- the FIRST stored (i, i) in storage order, the rule of
 * smh_crs_get and the Jacobi preconditioner.  It holds positions only: smh_crs_update_values, smh_crs_scale and a values-only
 * smh_crs_apply leave it valid; smh_crs_sort_rows and whatever replaces the handle's arrays drop it.
 * A level of more than R rows is one kernel launch; a run of consecutive levels of at most R rows each is ONE launch of one
 * workgroup that walks them (a bidiagonal chain of n rows: one launch).  No kernel waits for another workgroup.
 * smh_crs_trisolve_levels: the level count, the level of every row (n_rows entries, or NULL), the kernel launches one solve
 * enqueues, and R.  Any out pointer may be NULL.
 * smh_crs_trisolve: x = T^-1 b; diag = SMH_DIAG_UNIT takes the diagonal as 1 and needs none stored.  Every operation is rounded
 * once and nothing is fused; for row i (LOWER; UPPER: c > i):
 *     s = b[i];  for k = off[i] .. off[i+1]-1 in storage order:  c = col[k];  if c < i:  s = s - val[k] * x[c]
 *     x[i] = NON_UNIT ? s / val[diagpos[i]] : s
 * so duplicate off-diagonal entries are each subtracted and further stored (i, i) after the first are ignored.  A zero diagonal
 * VALUE is not an error: the solve gives IEEE's +-Inf or NaN.  _vec: x may be b (in place).
 * Statuses, all decided before any launch: SMH_ERR_NOT_SQUARE; SMH_ERR_DIM_MISMATCH; SMH_ERR_INDEX_RANGE (a stored column >=
 * n); SMH_ERR_INVALID (a NULL pointer, a vector dtype that is not the matrix's, b and x overlapping in part, a bad uplo or diag,
 * a handle that holds an orphaned entry, or -- NON_UNIT -- a row without a stored diagonal entry: the message names the first). */
int smh_crs_trisolve_levels(smh_crs *m, int uplo, size_t *n_levels_out, uint32_t *level_of_row_out, size_t *n_launches_out,
                            size_t *small_level_rows_out);
int smh_crs_trisolve(smh_crs *m, int uplo, int diag, const void *b_host, size_t b_len, void *x_host, size_t x_len);
int smh_crs_trisolve_vec(smh_crs *m, int uplo, int diag, const smh_vec *b, smh_vec *x);
/* The symmetric Gauss-Seidel preconditioner M = (D + L) D^-1 (D + U) of a square handle (D, L, U: its diagonal as above and its
 * strict triangles).  smh_crs_sgs_apply_vec: z = M^-1 r as  w = trisolve(LOWER, NON_UNIT, r);  u_i = w_i * d_i;  z =
 * trisolve(UPPER, NON_UNIT, u), each operation rounded once; z may be r.  Statuses as smh_crs_trisolve_vec's.
 * smh_pcg_sgs_solve: the recurrence of smh_pcg_jacobi_solve with that z; same guards, statuses, stop rule (on r.r, before
 * beta) and outputs; device-resident like smh_cg_solve (bodies enqueued past the stop change nothing; check_every: bodies per
 * poll, 0 = default, 8; a batch of many kernel launches is replayed in smaller batches or launched plainly, which changes no
 * bit):
 *     r = b - A x;  z = M^-1 r;  rr = r.r;  rz = r.z;  p = z
 *     body:  ap = A p;  alpha = rz / p.ap;  r = r - ap*alpha;  rr = r.r;  x = x + p*alpha;  sqrt(f64(rr)) < tol: stop
 *            z = M^-1 r;  rz' = r.z;  beta = rz' / rz;  rz = rz';  p = p*beta + z
 * A zero or absent diagonal entry is SMH_ERR_INVALID (the message names the row); a stored column >= n SMH_ERR_INDEX_RANGE;
 * _vec: additionally SMH_ERR_INVALID for a NULL vector, a dtype that is not the matrix's, b and x the same storage. */
int smh_crs_sgs_apply_vec(smh_crs *m, const smh_vec *r, smh_vec *z);
int smh_pcg_sgs_solve(smh_crs *m, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len,
                      double tol, size_t iter_max, int variant, size_t *iters_out, double *rr_out);
int smh_pcg_sgs_solve_vec(smh_crs *m, const smh_vec *b, smh_vec *x, double tol, size_t iter_max,
                          int variant, size_t check_every, size_t *iters_out, double *rr_out);

/* The incomplete LU factorization without fill, ILU(0) -- an EXTENSION.  smh_crs_ilu0: *f_out is a new library-owned handle with
 * a's offsets, columns, storage order and smh_crs_set_* settings; its values are the unit-lower factor L on the stored (i, c)
 * with c < i and U on those with c >= i.  It is an ordinary handle (download, mvp, trisolve; the caller destroys it).  With w
 * a's values and diagpos[k] the position of the stored (k, k), every operation rounded once and nothing fused:
 *     for i = 0 .. n-1:
 *       for kk = off[i] .. off[i+1]-1 in storage order, k = col[kk], while k < i:
 *           w[kk] = w[kk] / w[diagpos[k]]
 *           for jj = diagpos[k]+1 .. off[k+1]-1  (j = col[jj] > k):
 *               if row i stores column j at position t:  w[t] = w[t] - w[kk] * w[jj]
 * Rows are factored level by level of the LOWER schedule of the pattern (smh_crs_trisolve_levels: the same levels and launches).
 * Statuses, checked before anything is written: SMH_ERR_NOT_SQUARE; SMH_ERR_INVALID for a handle that holds an orphan;
 * SMH_ERR_INDEX_RANGE for a stored column >= n; SMH_ERR_INVALID for a row whose columns are not strictly ascending (unsorted, or
 * a duplicate: smh_crs_sort_rows sorts, duplicates are not folded) and for a row without a stored (i, i), the message naming
 * the first such row; SMH_ERR_INVALID for a NULL a or f_out.  A zero pivot is not an error: the values are IEEE's +-Inf or NaN, as
 * in the triangular solve.  *zero_pivot_out (may be NULL): the smallest row i whose final U(i, i) compares equal to 0, SIZE_MAX
 * without one.
 * smh_crs_ilu0_refactor: new values on the same pattern (time stepping, Newton): a's values are copied into f and factored with
 * f's schedule; the result is bit for bit that of smh_crs_ilu0(a).  SMH_ERR_DIM_MISMATCH when n differs; SMH_ERR_INVALID when the
 * dtype, the device, the number of entries, the offsets or the columns differ (compared on the device) or f is a; a's statuses
 * as above.  A refused call leaves f untouched.
 * smh_crs_ilu_apply_vec: z = U^-1 L^-1 r as  w = trisolve(f, LOWER, UNIT, r);  z = trisolve(f, UPPER, NON_UNIT, w); z may be r.
 * Statuses as smh_crs_trisolve_vec's.
 * smh_pcg_ilu_solve: the recurrence of smh_pcg_sgs_solve with that z: the product (and its p.Ap) is a's, the solves are f's; same
 * guards, stop rule, check_every and outputs.  A zero or absent diagonal entry of f is SMH_ERR_INVALID (the message names the
 * row); a and f differing in n SMH_ERR_DIM_MISMATCH, in dtype or device SMH_ERR_INVALID, decided before any launch.  What f's
 * values are is the caller's business: nothing ties f to a beyond these. */
int smh_crs_ilu0(const smh_crs *a, smh_crs **f_out, size_t *zero_pivot_out);
int smh_crs_ilu0_refactor(smh_crs *f, const smh_crs *a, size_t *zero_pivot_out);
int smh_crs_ilu_apply_vec(smh_crs *f, const smh_vec *r, smh_vec *z);
int smh_pcg_ilu_solve(smh_crs *a, smh_crs *f, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len,
                      double tol, size_t iter_max, int variant, size_t *iters_out, double *rr_out);
int smh_pcg_ilu_solve_vec(smh_crs *a, smh_crs *f, const smh_vec *b, smh_vec *x, double tol, size_t iter_max,
                          int variant, size_t check_every, size_t *iters_out, double *rr_out);

/* The factorized sparse approximate inverse (FSAI, Kolotilina and Yeremin) -- an EXTENSION: a preconditioner applied by two
 * products, where SGS and ILU(0) take two triangular solves.  smh_crs_fsai: *g_out is a new library-owned handle of a's dtype, lower
 * triangular, whose pattern is exactly the stored (i, c) of a with c <= i, columns ascending; *gt_out is its transpose as
 * smh_crs_transpose(g) stores it (n = 1: a copy of g, where the one-operation transposition would leave an orphan).  For an SPD a, G^T G approximates a^-1 and diag(G a G^T) = 1.  Both are ordinary handles (mvp,
 * get_many, clone, download; the caller destroys them).  Every operation is rounded once and nothing is fused; sqrt is IEEE's.
 * For row i let J = (j_0 < ... < j_(m-1) = i) be its stored columns <= i and B the dense lower triangle B[p][q], q <= p: the stored
 * entry (j_p, j_q) of row j_p, or 0 where none is stored.  Only entries on or below a's diagonal are ever read: the result is the
 * FSAI of the symmetric matrix that a's lower triangle defines.
 *     for k = 0 .. m-2:                                          (elimination, no pivoting)
 *         for p = k+1 .. m-1:  l_p = B[p][k] / B[k][k]
 *         for p = k+1 .. m-1, q = k+1 .. p:  B[p][q] = B[p][q] - l_p * B[q][k]      (B[q][k]: the value before its division)
 *         for p = k+1 .. m-1:  B[p][k] = l_p
 *     y_(m-1) = 1;  for p = m-2 .. 0:  s = 0;  for q = p+1 .. m-1 ascending:  s = s + B[q][p] * y_q;   y_p = -s
 *     g = 1 / sqrt(B[m-1][m-1]);  G[i, j_p] = y_p * g
 * The rows are independent: one sweep of lane groups, the triangle in the LDS (a long row: a workgroup, the triangle in global
 * scratch; the same bits).  A LIMIT: a row with m > 128 is refused.
 * Statuses, checked on the device before anything is written, in smh_crs_ilu0's order: SMH_ERR_NOT_SQUARE; SMH_ERR_INVALID for a
 * handle that holds an orphan; SMH_ERR_INDEX_RANGE for a stored column >= n; SMH_ERR_INVALID for a row whose columns are not
 * strictly ascending and for a row without a stored (i, i), the message naming the first such row; then SMH_ERR_INVALID for a row
 * with m > 128, the message naming the first; SMH_ERR_INVALID for a NULL a, g_out or gt_out.  A matrix that is not SPD is not an
 * error: *not_spd_out (may be NULL) is the smallest row whose last pivot B[m-1][m-1] is not > 0 (a NaN is not), SIZE_MAX without
 * one, and such a row holds the IEEE values of the operations above.
 * smh_crs_fsai_apply_vec: w = G r, z = G^T w by the handles' own products (SMH_SPMV_AUTO) on g's stream; z may be r.  Statuses
 * as smh_crs_ilu_apply_vec's, with g in f's place (no diagonal is asked for: nothing divides); in addition g and gt differing in n
 * SMH_ERR_DIM_MISMATCH, in dtype or device SMH_ERR_INVALID, gt not square SMH_ERR_NOT_SQUARE.
 * smh_pcg_fsai_solve: the recurrence of smh_pcg_sgs_solve with that z: the product (by `variant`) and its p.Ap are a's, the
 * two products of an application go through AUTO; same guards, stop rule, check_every and outputs.  Statuses as
 * smh_pcg_ilu_solve's, decided before any launch, with g and then gt in f's place; the factors' values are the caller's business
 * (no probe of a diagonal). */
int smh_crs_fsai(const smh_crs *a, smh_crs **g_out, smh_crs **gt_out, size_t *not_spd_out);
int smh_crs_fsai_apply_vec(smh_crs *g, smh_crs *gt, const smh_vec *r, smh_vec *z);
int smh_pcg_fsai_solve(smh_crs *a, smh_crs *g, smh_crs *gt, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len,
                       double tol, size_t iter_max, int variant, size_t *iters_out, double *rr_out);
int smh_pcg_fsai_solve_vec(smh_crs *a, smh_crs *g, smh_crs *gt, const smh_vec *b, smh_vec *x, double tol, size_t iter_max,
                           int variant, size_t check_every, size_t *iters_out, double *rr_out);

/* The non-symmetric FSAI -- an EXTENSION: two factors, M^-1 = G_U G_L ~ a^-1, for matrices that are not symmetric.  *gl_out and *gu_out
 * are new library-owned handles of a's dtype, ordinary ones as smh_crs_fsai's are.  Every operation is rounded once and nothing is fused.
 * The row solve R(C, i) on a CRS matrix C with ascending rows: J = (j_0 < ... < j_(m-1) = i) the stored columns <= i of row i, B the
 * dense m x m matrix B[p][q] = the stored entry (j_p, j_q) of C, or 0 where none is stored -- the full square, both triangles:
 *     for k = 0 .. m-2:                                          (elimination, no pivoting)
 *         for p = k+1 .. m-1:  l_p = B[p][k] / B[k][k]
 *         for p = k+1 .. m-1, q = k+1 .. m-1:  B[p][q] = B[p][q] - l_p * B[k][q]
 *         for p = k+1 .. m-1:  B[p][k] = l_p
 *     y_(m-1) = 1;  for p = m-2 .. 0:  s = 0;  for q = p+1 .. m-1 ascending:  s = s + B[q][p] * y_q;   y_p = -s
 *     d = B[m-1][m-1]                                            (d * the last row of B^-1 = y)
 * G_L: row i, on J, is y of R(a, i): lower triangular with a stored unit diagonal, G_L ~ L^-1 of a = L D U.  G_U: let H hold in row i,
 * on the stored columns <= i of row i of a^T, y / d of R(a^T, i) -- one division per entry; a^T with its rows ascending --; G_U is the
 * transposition of H as smh_crs_transpose stores it (n = 1: a copy): upper triangular on the stored (i, c) of a with c >= i.  For a
 * dense pattern G_U G_L = a^-1.  The rows are independent: one sweep of lane groups per factor, the square in the LDS (a group of
 * 1, 2, 4, .. 64 lanes holds m <= 4, 5, 8, 11, 16, 22, 32; a longer row: a workgroup, the square in global scratch; the same bits).
 * Statuses: smh_crs_fsai's in its order; then SMH_ERR_INVALID for a row with more than 128 stored entries on or below the diagonal,
 * then for a column with more than 128 on or above it, the message naming the first ("row", "column"); nothing is made on refusal.
 * *singular_out (may be NULL) is the smallest i for which d of either row solve is zero or not finite, SIZE_MAX without one: a
 * result, not an error, and such rows hold the IEEE values of the operations above.
 * smh_crs_fsai_ns_apply_vec: smh_crs_fsai_apply_vec under this pair's name: w = G_L r, z = G_U w through SMH_SPMV_AUTO; z may be r. */
int smh_crs_fsai_ns(const smh_crs *a, smh_crs **gl_out, smh_crs **gu_out, size_t *singular_out);
int smh_crs_fsai_ns_apply_vec(smh_crs *gl, smh_crs *gu, const smh_vec *r, smh_vec *z);

/* BiCGSTAB (van der Vorst, unpreconditioned) for non-symmetric systems -- an EXTENSION (the reference's only solver is
 * the conjugate gradient).  Device-resident like smh_cg_solve: scalars in HBM, the stop decided on the device in every
 * body and polled every `check_every` bodies (0: default, 8), bodies enqueued past the stop are no-ops, so x and all
 * outputs are those of the stopping body.  One rounding per operation; the comparisons with zero are exact:
 *   r = b - A x;  r^ = r;  p = r;  rho = r^.r;  rr = r.r          (no stop test before the first body)
 *   body:  v = A p;  rv = r^.v;                  rv == 0: breakdown 2, stop (x untouched by this body)
 *          alpha = rho / rv;  s = r - v*alpha;  ss = s.s
 *                                                sqrt(f64(ss)) < tol: x += p*alpha; rr = ss; converged (half-step stop)
 *          t = A s;  ts = t.s;  tt = t.t;        tt == 0: x += p*alpha; rr = ss; breakdown 3, stop
 *          omega = ts / tt;  x = (x + p*alpha) + s*omega;  r = s - t*omega;  rr = r.r;  rho' = r^.r
 *                                                sqrt(f64(rr)) < tol: converged
 *                                                rho' == 0 or omega == 0: breakdown 1, stop (x keeps this body's update)
 *          beta = (rho'/rho) * (alpha/omega);  rho = rho';  p = r + (p - v*omega)*beta
 * A breakdown is not an error: the call returns SMH_OK and *breakdown_out holds 0 (none), 1, 2 or 3.  iters_out = bodies
 * entered, rr_out = the last r.r (s.s after a half-step stop or breakdown 3) as f64; the output pointers may be NULL.
 * Statuses, decided on the host before any launch: SMH_ERR_NOT_SQUARE, SMH_ERR_DIM_MISMATCH, SMH_ERR_INVALID (a NULL
 * handle or vector, a vector dtype that is not the matrix's, b and x the same storage).  x: in x0, out the solution. */
int smh_bicgstab_solve(smh_crs *m, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len,
                       double tol, size_t iter_max, int variant,
                       size_t *iters_out, double *rr_out, int *breakdown_out);
int smh_bicgstab_solve_vec(smh_crs *m, const smh_vec *b, smh_vec *x, double tol, size_t iter_max,
                           int variant, size_t check_every,
                           size_t *iters_out, double *rr_out, int *breakdown_out);

/* Restarted GMRES(m) (Saad & Schultz, unpreconditioned) for non-symmetric systems -- an EXTENSION, the robust companion of
 * smh_bicgstab_solve: it cannot break down before the Krylov space is exhausted and does not stagnate where BiCGSTAB's omega
 * goes to zero (a spectrum near the imaginary axis); a body is ONE product and sweeps over a basis of up to m + 1 vectors of n
 * kept on the device (so its memory is (m + 5) n values).  Device-resident like smh_bicgstab_solve: the stop is decided on the
 * device in every body and polled every `check_every` bodies (0: default, 8), bodies enqueued past the stop are no-ops.
 * `restart` is m, 1 <= m <= 128; 0 stands for 30.  One rounding per operation, sqrt correctly rounded, comparisons with zero exact:
 *   set-up:  r = b - A x;  rr = r.r;  beta = sqrt(rr);  beta == 0: stop, no body entered, breakdown 2
 *            v_0 = r / beta;  g = (beta);  j = 0;  cycles = 1
 *   body:    w = A v_j;  h1_c = v_c.w (c <= j);  w -= v_c h1_c (c ascending);  h2_c = v_c.w;  w -= v_c h2_c;  h = h1 + h2
 *            hn = sqrt(w.w);  the stored rotations on h;  d = sqrt(h_j h_j + hn hn);  c_j = h_j / d;  s_j = hn / d
 *            R[0..j, j] = (h_0 .. h_{j-1}, c_j h_j + s_j hn);  g_{j+1} = (-s_j) g_j;  g_j = c_j g_j;  j += 1
 *            v_j = w / hn (w itself when hn == 0)
 *            the cycle ends when hn == 0 (breakdown 1: the Krylov space is exhausted, x is updated from it), |f64(g_j)| < tol
 *            (converged), iters == iter_max, or -- none of these, which stop the solve -- j == m (restart)
 *   cycle end:  R y = g[0..j) by back substitution;  x += v_0 y_0 + .. + v_{j-1} y_{j-1} (ascending, term by term)
 *            r = v_0 z_0 + .. + v_j z_j with z the transposed rotations applied to g_j e_j: NO product; rr = r.r
 *            on a restart:  beta = sqrt(rr);  beta == 0: stop, breakdown 2;  else v_0 = r / beta, g = (beta), j = 0, cycles += 1
 * (the orders in full: csrc/gmres.hip and tests/gmres_model.py).  d is not scaled against overflow; a singular matrix gives
 * IEEE values, not an error; non-finite data run to iter_max.  A breakdown is not an error: the call returns SMH_OK and
 * *breakdown_out holds 0, 1 or 2.  iters_out = bodies entered, rr_out = the last rebuilt r.r (the initial residual's before the
 * first cycle end) as f64, cycles_out = the number of times a v_0 was formed; the output pointers may be NULL.
 * Statuses, decided on the host before any launch: smh_bicgstab_solve's, then SMH_ERR_INVALID for restart > 128.
 * x: in x0, out the solution. */
int smh_gmres_solve(smh_crs *m, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len,
                    double tol, size_t iter_max, size_t restart, int variant,
                    size_t *iters_out, double *rr_out, size_t *cycles_out, int *breakdown_out);
int smh_gmres_solve_vec(smh_crs *m, const smh_vec *b, smh_vec *x, double tol, size_t iter_max, size_t restart,
                        int variant, size_t check_every,
                        size_t *iters_out, double *rr_out, size_t *cycles_out, int *breakdown_out);

/* Thick-restart Lanczos (Wu & Simon) with full reorthogonalisation -- an EXTENSION (the reference has no eigensolver): the k
 * algebraically largest (SMH_EIGSH_LARGEST) or smallest (SMH_EIGSH_SMALLEST) eigenpairs of a SYMMETRIC matrix.  Symmetry is the
 * caller's promise, as it is for smh_cg_solve: nothing checks it.  A multiple eigenvalue is found once (single-vector Lanczos).
 * ncv = m, the columns of the basis: clipped to n, then k + 2 <= m <= 128 (0: the default, min(n, max(2 k + 1, 20))); whenever
 * k + 2 > n, m = n and the first cycle is the whole space.  One rounding per operation, nothing contracted; the recurrence in full,
 * with its orders: csrc/eigsh.hip and tests/eigsh_model.py.  In short: v_0 = start / |start|; a body at column j is w = A v_j,
 * classical Gram-Schmidt twice against v_0 .. v_j (smh_gmres_solve's sweeps), alpha_j, beta_j = |w|, v_{j+1} = w / beta_j; a cycle of
 * m - l bodies ends with ONE host round trip: the projected (arrowhead + tridiagonal) matrix is diagonalised in f64 by cyclic
 * Jacobi, est_i = |beta_{m-1} Y[m-1, i]|, pair i is converged when est_i <= tol * max|theta|, n_conv is the converged prefix of the
 * wanted order; unless n_conv == k, restarts == restart_max or m == n the basis is rotated on the device to the l = k + (m - k) / 2
 * wanted Ritz vectors and the cycle continues at column l.  tol is used as given (0 converges only on an exact zero estimate).
 * *breakdown_out: 0 none; 1 beta_j == 0, the Krylov space is exhausted: the min(k, j + 1) pairs that exist are returned exact (the
 * values and estimates past them NaN, the vectors past them zero); 2 the start vector's norm is zero or not finite; 3 a non-finite
 * alpha / beta (non-finite data).  2 and 3 return nothing: evals_out, est_out and the vectors are not written, *n_conv_out = 0.
 * A breakdown is not an error: the call returns SMH_OK.  *n_conv_out < k with SMH_OK and breakdown 0 is an exhausted restart_max:
 * the k best pairs are returned with their estimates.  evals_out / est_out: k values, in the wanted order; products_out: bodies
 * entered; the vectors are not renormalised.  The output pointers may be NULL, the vectors too.
 * evecs_host_out: k x n values (vector i at [i * n]); evecs: an smh_mvec of k columns.  Memory: (2 m + 4) n values.
 * Statuses, decided on the host before any launch (a refused call writes nothing): a NULL handle or a NULL start of n > 0, a dtype
 * that is not the matrix's, k == 0, k > n, ncv outside [k + 2, 128] after clipping, `which` out of range, evecs of another column
 * count: SMH_ERR_INVALID; not square: SMH_ERR_NOT_SQUARE; start_len or a handle's dimension != n: SMH_ERR_DIM_MISMATCH. */
#define SMH_EIGSH_LARGEST 0
#define SMH_EIGSH_SMALLEST 1
int smh_eigsh(smh_crs *m, const void *start_host, size_t start_len, size_t k, size_t ncv, int which, double tol,
              size_t restart_max, int variant, double *evals_out, void *evecs_host_out, double *est_out,
              size_t *n_conv_out, size_t *restarts_out, size_t *products_out, int *breakdown_out);
int smh_eigsh_vec(smh_crs *m, const smh_vec *start, smh_mvec *evecs, size_t k, size_t ncv, int which, double tol,
                  size_t restart_max, int variant, double *evals_out, double *est_out,
                  size_t *n_conv_out, size_t *restarts_out, size_t *products_out, int *breakdown_out);
/* A measuring aid: of this thread's last smh_eigsh*, the host step's wall time summed over its cycle ends and their number; and, only
 * when the environment variable SMH_EIGSH_TIMING is set (the solve then waits for every rotation, which moves no bit), the wall
 * time of the rotations, Yt's upload included, and their number (0 otherwise).  The pointers may be NULL. */
int smh_eigsh_last_timing(double *host_step_ms_out, size_t *cycles_out, double *rotation_ms_out, size_t *rotations_out);

/* Right-preconditioned GMRES(m) -- an EXTENSION: A M^-1 u = b, x = M^-1 u, inside the solver above, so the residual it minimises is
 * the true one, b - A x, and the stop rule, rr, cycles and both breakdown codes keep their meaning.  Everything not named here is
 * smh_gmres_solve's contract, word for word.  One rounding per operation, nothing contracted:
 *   set-up:     unchanged (r = b - A x; M is not applied to the residual)
 *   body:       u = M^-1 v_j;  w = A u;  both Gram-Schmidt passes, the step and v_{j+1} = w / hn unchanged
 *   cycle end:  y unchanged;  t = (..(v_0 y_0 + v_1 y_1) .. + v_{j-1} y_{j-1})   (starts from the product, as r does)
 *               q = M^-1 t;  x = x + q                       (one application per cycle, one add per element)
 *               r, rr, the restart: unchanged (rebuilt from the basis; no product)
 * precond = SMH_PRECOND_JACOBI: M^-1 v is v_i / d_i, a division, d_i the first stored (i, i) (as smh_pcg_jacobi_solve forms z);
 * SMH_PRECOND_SGS: smh_crs_sgs_apply_vec's operations on a itself; SMH_PRECOND_ILU: smh_crs_ilu_apply_vec's on the factor handle
 * f (smh_crs_ilu0; what its values are is the caller's business).  SMH_PRECOND_NONE forwards to smh_gmres_solve*: its bits.
 * f is the ILU factor and NULL for every other kind: a non-NULL f with another kind, a NULL f with SMH_PRECOND_ILU and any other
 * value of precond are SMH_ERR_INVALID.  Memory: (m + 6) n values with Jacobi, (m + 7) n with SGS and ILU.  A batch of many kernel
 * launches (two applications per body) is replayed in smaller batches or launched plainly, which changes no bit.
 * rr is the RECURRENCE residual's r.r: with an ill-conditioned M (triangular solves that amplify rounding) it parts from
 * |b - A x|^2, which the caller then forms itself.
 * Statuses, decided before any launch of the solve: smh_gmres_solve's; ILU: smh_pcg_ilu_solve's about f (n: SMH_ERR_DIM_MISMATCH;
 * dtype, device, an orphaned entry, a zero or absent diagonal entry, the message naming the row: SMH_ERR_INVALID; a stored column
 * >= n: SMH_ERR_INDEX_RANGE); SGS: smh_pcg_sgs_solve's about a; Jacobi: smh_pcg_jacobi_solve's about the diagonal. */
#define SMH_PRECOND_NONE 0
#define SMH_PRECOND_JACOBI 1
#define SMH_PRECOND_SGS 2
#define SMH_PRECOND_ILU 3
int smh_gmres_precond_solve(smh_crs *a, int precond, smh_crs *f, const void *b_host, size_t b_len, void *x_host_inout,
                            size_t x_len, double tol, size_t iter_max, size_t restart, int variant,
                            size_t *iters_out, double *rr_out, size_t *cycles_out, int *breakdown_out);
int smh_gmres_precond_solve_vec(smh_crs *a, int precond, smh_crs *f, const smh_vec *b, smh_vec *x, double tol,
                                size_t iter_max, size_t restart, int variant, size_t check_every,
                                size_t *iters_out, double *rr_out, size_t *cycles_out, int *breakdown_out);

/* Right-preconditioned BiCGSTAB -- an EXTENSION: A M^-1 u = b, x = M^-1 u, inside smh_bicgstab_solve's recurrence, so the residual it
 * carries is the true one, b - A x, and the stop rule, rr, iters and the three breakdown codes keep their meaning.  Everything not
 * named here is smh_bicgstab_solve's contract, word for word.  One rounding per operation, nothing contracted:
 *   set-up:  unchanged (r = b - A x; r^ = r; p = r; rho = r^.r; rr = r.r; M is not applied to the residual)
 *   body:    p^ = M^-1 p;  v = A p^;  rv = r^.v;                 rv == 0: breakdown 2 (x untouched)
 *            alpha = rho / rv;  s = r - v*alpha;  ss = s.s
 *                                                             sqrt(f64(ss)) < tol: x += p^*alpha; rr = ss; converged
 *            s^ = M^-1 s;  t = A s^;  ts = t.s;  tt = t.t;       tt == 0: x += p^*alpha; rr = ss; breakdown 3
 *            omega = ts / tt;  x = (x + p^*alpha) + s^*omega;  r = s - t*omega;  rr = r.r;  rho' = r^.r
 *            the stop test, breakdown 1, beta and p = r + (p - v*omega)*beta: unchanged
 * precond and f are smh_gmres_precond_solve's: SMH_PRECOND_JACOBI divides by the first stored (i, i); SMH_PRECOND_SGS applies
 * smh_crs_sgs_apply_vec's operations on a itself; SMH_PRECOND_ILU smh_crs_ilu_apply_vec's on the factor handle f;
 * SMH_PRECOND_NONE forwards to smh_bicgstab_solve*: its bits.  f is the ILU factor and NULL for every other kind: a non-NULL f
 * with another kind, a NULL f with SMH_PRECOND_ILU and any other value of precond are SMH_ERR_INVALID, decided first.  Memory:
 * ten vectors of n against seven.  A batch of many kernel launches (two applications per body) is replayed in smaller batches or
 * launched plainly, which changes no bit.  rr is the RECURRENCE residual's r.r, as it is in smh_bicgstab_solve.
 * Statuses, decided before any launch of the solve: smh_bicgstab_solve's; then what smh_gmres_precond_solve decides about the
 * preconditioner, with its codes and messages (ILU: f's n, dtype, device, an orphaned entry, a zero or absent diagonal entry, a
 * stored column >= n; SGS: the same about a; Jacobi: a zero or absent diagonal entry of a). */
int smh_bicgstab_precond_solve(smh_crs *a, int precond, smh_crs *f, const void *b_host, size_t b_len, void *x_host_inout,
                               size_t x_len, double tol, size_t iter_max, int variant,
                               size_t *iters_out, double *rr_out, int *breakdown_out);
int smh_bicgstab_precond_solve_vec(smh_crs *a, int precond, smh_crs *f, const smh_vec *b, smh_vec *x, double tol,
                                   size_t iter_max, int variant, size_t check_every,
                                   size_t *iters_out, double *rr_out, int *breakdown_out);

/* GMRES(m) and BiCGSTAB right-preconditioned by a pair of product handles -- an EXTENSION: M^-1 v = gt (g v), two products, where
 * SGS and ILU(0) take two level-scheduled triangular solves: no schedule, no levels, the same cost in every ordering.  The pair is
 * (G_L, G_U) of smh_crs_fsai_ns, or (G, G^T) of smh_crs_fsai for a symmetric a; what its values are is the caller's business (no
 * diagonal is probed: nothing divides by a factor's value).  The arguments are those of smh_gmres_precond_solve* and
 * smh_bicgstab_precond_solve* with the pair in place of `precond, f`; the recurrences are theirs, operation for operation: one
 * application per GMRES body (u = M^-1 v_j) and one per cycle end (q = M^-1 t), two per BiCGSTAB body (p^ = M^-1 p, s^ = M^-1 s).
 * WHICH PRODUCT FORMS WHAT.  The applications inside a body go through the handles' own kernels (SMH_SPMV_AUTO), ungated like the
 * body's own product: in bodies enqueued past the stop they form the same vector from unchanged input again.  GMRES's cycle end forms
 * q by two storage-order products, w' = g t and q = gt w', each one lane per row with the product rounded, then added
 * (SMH_SPMV_SEQ's operations and bits), behind the device word that says a cycle end is due: they return at once in every body that
 * ends no cycle, where two more AUTO products would have run, and cost, each time.  Every sweep that writes x, r or the basis is
 * gated as before.  `variant` is a's product's.  Memory: (m + 7) n values for GMRES and ten vectors of n for BiCGSTAB, as with SGS and
 * ILU(0); the cycle end needs no vector more.  A captured batch stays under the node budget of the triangular kinds.
 * Statuses, decided before any launch, x left untouched: SMH_ERR_INVALID for a NULL g or gt; then smh_pcg_fsai_solve's about a, g
 * and gt (not square; the pair's n: SMH_ERR_DIM_MISMATCH; dtype, device: SMH_ERR_INVALID), the vectors' as smh_gmres_solve* and
 * smh_bicgstab_solve*, GMRES's restart; an orphaned entry in g or gt SMH_ERR_INVALID; a stored column >= n SMH_ERR_INDEX_RANGE. */
int smh_gmres_fsai_solve(smh_crs *a, smh_crs *g, smh_crs *gt, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len,
                         double tol, size_t iter_max, size_t restart, int variant,
                         size_t *iters_out, double *rr_out, size_t *cycles_out, int *breakdown_out);
int smh_gmres_fsai_solve_vec(smh_crs *a, smh_crs *g, smh_crs *gt, const smh_vec *b, smh_vec *x, double tol, size_t iter_max,
                             size_t restart, int variant, size_t check_every,
                             size_t *iters_out, double *rr_out, size_t *cycles_out, int *breakdown_out);
int smh_bicgstab_fsai_solve(smh_crs *a, smh_crs *g, smh_crs *gt, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len,
                            double tol, size_t iter_max, int variant, size_t *iters_out, double *rr_out, int *breakdown_out);
int smh_bicgstab_fsai_solve_vec(smh_crs *a, smh_crs *g, smh_crs *gt, const smh_vec *b, smh_vec *x, double tol, size_t iter_max,
                                int variant, size_t check_every, size_t *iters_out, double *rr_out, int *breakdown_out);

/* ---- mixed precision -- EXTENSIONS (the reference has one precision; csrc/refine.hip) ----
 * smh_crs_cast: *out is a new library-owned handle with a's dims, offsets, columns, orphan and smh_crs_set_* settings, as
 * smh_crs_clone copies them, and a's values converted on the device to `dtype`: f64 -> f32 rounds to nearest even and finite values
 * beyond f32's range become +-Inf; f32 -> f64 is exact; NaN stays NaN, a zero keeps its sign, results that are f32 subnormals are
 * kept.  dtype == a's: smh_crs_clone's result.  overflow_out (optional): the finite values that became infinite.  Derived forms are
 * rebuilt lazily on the new handle.  Not under a stream capture.  SMH_ERR_INVALID for a NULL a or out, or an unknown dtype.
 * smh_vec_cast: dst[i] = convert(src[i]) by the same rule.  SMH_ERR_INVALID for a NULL handle, SMH_ERR_DIM_MISMATCH when the dims
 * differ; with equal dtypes it is smh_vec_copy(dst, src); with different dtypes, vectors that share storage are SMH_ERR_INVALID. */
int smh_crs_cast(const smh_crs *a, smh_dtype dtype, smh_crs **out, size_t *overflow_out);
int smh_vec_cast(const smh_vec *src, smh_vec *dst);

/* Mixed-precision iterative refinement: an f64-accurate x of A x = b with the bodies run by the f32 solvers.  a is the f64 handle, b
 * and x are f64; a_lo is an f32 handle of a's dimension on a's device -- normally smh_crs_cast(a, SMH_F32); what its values are is the
 * caller's business, as with factor handles --, f_lo and f2_lo are f32 factors OF a_lo.  Each operation is rounded once, nothing is
 * contracted:
 *   set-up:  r = b - A x        (A x: a's product through `variant`; one subtraction per element)
 *            rr = r.r           (f64: products rounded, then the fused solvers' tree on their grid; tests/refine_model.py)
 *            outer = 0;  inner_iters = 0
 *   loop:    rr == 0 or sqrt(rr) < tol:  code 0 (converged), stop
 *            outer == outer_max:         code 1, stop
 *            e = floor(ilogb(rr) / 2)    (on the host, from the polled rr; |r 2^-e|^2 is in [1, 4); a non-finite rr takes e = 0)
 *            r_lo[i] = (float)(r[i] * 2^-e)          (the product is exact: one rounding, the conversion)
 *            d_lo = 0;  the inner solver on a_lo d_lo = r_lo with tolerance inner_tol, inner_iter_max, restart, variant_lo, check_every
 *            inner_iters += its bodies;  outer += 1
 *            x_prev = x;  x[i] = x[i] + (double)d_lo[i] * 2^e    (the product is exact: one rounding, the addition)
 *            r = b - A x;  rr' = r.r
 *            not (rr' < rr):  x = x_prev;  code 2 (stalled; covers NaN), stop with the old rr
 *            rr = rr'
 * The inner solvers' stop rule is absolute, sqrt(rr) < tol: on the normalised residual inner_tol is a relative reduction between
 * inner_tol / 2 and inner_tol, and r_lo . r_lo stays away from f32 underflow.  An inner breakdown is not an error: its d_lo is used
 * and the outer test decides.  One 8-byte poll per outer step is the only host round trip of the outer loop.  Not under a stream
 * capture.  0 stands for the default in outer_max (20), inner_tol (1e-4), inner_iter_max (10000) and restart (30).
 * The inner solve goes through the existing entry points, bit for bit:
 *   inner \ precond   NONE                 JACOBI    SGS                    ILU (f_lo)             FSAI (f_lo, f2_lo)
 *   SMH_INNER_CG      smh_cg_solve_vec     refused   smh_pcg_sgs_solve_vec  smh_pcg_ilu_solve_vec  smh_pcg_fsai_solve_vec
 *   _BICGSTAB         smh_bicgstab_precond_solve_vec (NONE forwards) ............................  smh_bicgstab_fsai_solve_vec
 *   _GMRES            smh_gmres_precond_solve_vec ...............................................  smh_gmres_fsai_solve_vec
 * SMH_PRECOND_FSAI is a kind of these two entry points only: f_lo = G or G_L, f2_lo = G^T or G_U.  CG with SMH_PRECOND_JACOBI is
 * SMH_ERR_INVALID: the Jacobi-preconditioned CG has no device-vector form.
 * Outputs (optional): outer steps, the inner solves' bodies in total, the last accepted r.r, the code.
 * Statuses, decided before any launch, x left untouched, in this order: SMH_ERR_INVALID for a NULL a, a_lo, b or x; a not f64 or
 * a_lo not f32; a vector that is not f64; b and x in one storage; an unknown inner or precond (and CG with Jacobi); a factor given
 * where the kind takes none or missing where it takes one; then a_lo's dims (SMH_ERR_DIM_MISMATCH) or device (SMH_ERR_INVALID)
 * differing from a's; SMH_ERR_NOT_SQUARE; the vectors' dims (SMH_ERR_DIM_MISMATCH); restart > 128 (SMH_ERR_INVALID).  Whatever the
 * inner entry point refuses about a_lo and the factors comes back from the first outer step with its own code and message, x still
 * untouched.  Memory: three f64 and two f32 vectors of n beside the inner solver's own.
 * smh_refine_solve: the same on host arrays of b_len / x_len f64 values (x: in x0, out the result; a NULL array of a non-zero length
 * and b_host == x_host_inout are SMH_ERR_INVALID). */
#define SMH_INNER_CG 0
#define SMH_INNER_BICGSTAB 1
#define SMH_INNER_GMRES 2
#define SMH_PRECOND_FSAI 4 /* smh_refine_solve* only */
int smh_refine_solve_vec(smh_crs *a, smh_crs *a_lo, int inner, int precond, smh_crs *f_lo, smh_crs *f2_lo, const smh_vec *b,
                         smh_vec *x, double tol, size_t outer_max, double inner_tol, size_t inner_iter_max, size_t restart,
                         int variant, int variant_lo, size_t check_every,
                         size_t *outer_out, size_t *inner_iters_out, double *rr_out, int *code_out);
int smh_refine_solve(smh_crs *a, smh_crs *a_lo, int inner, int precond, smh_crs *f_lo, smh_crs *f2_lo, const void *b_host,
                     size_t b_len, void *x_host_inout, size_t x_len, double tol, size_t outer_max, double inner_tol,
                     size_t inner_iter_max, size_t restart, int variant, int variant_lo, size_t check_every,
                     size_t *outer_out, size_t *inner_iters_out, double *rr_out, int *code_out);

/* ---- SparseMatPar<SparseMatCRS<T,u32>> (sparsemat_par.rs:12-35, 86-140) over the GPUs of one node ----
 * The reference keeps n_blocks sub-matrices of R = n_rows / n_blocks rows (with_sub_matrices :20-28;
 * integer division :21); block b = global rows [b R, (b+1) R) with local row ids and GLOBAL column
 * ids; its (commented-out) mvp_par :37-68 multiplies every block against the shared rhs and places
 * the results at b * R -- a row partition plus an all-gather.  Here block b lives on a GPU, the local
 * product is the library's SpMV, and the exchange runs INSIDE the library, device to device over
 * xGMI: an in-place RCCL all-gather of the y slices (ncclAllGather at recvbuff + b R; a ragged last
 * block adds one ncclBroadcast of its tail), or -- when the blocks' column intervals say that less
 * than half of the vector is referenced -- grouped ncclSend / ncclRecv of exactly the referenced
 * entries ("window"; a banded matrix moves a halo).  Two ways to own the blocks:
 *   one process, all blocks   smh_par_create (splits host arrays) / smh_par_adopt (blocks already on
 *                             their devices): ncclCommInitAll over the blocks' devices when they are
 *                             distinct (backend RCCL), or -- backend PEER, also the only choice when
 *                             blocks share a device -- one pull kernel per block that reads the peers'
 *                             slices directly (peer access; hipMemcpyPeerAsync where there is none).
 *   one process per GPU       smh_comm_unique_id on one rank, smh_comm_create (ncclCommInitRank) on
 *                             all, smh_par_create_rank around each rank's own block: rank = block id.
 * The last block takes the remainder rows -- the reference clamps the block id to n_blocks (:32), one
 * past the last block, and panics there.  R == 0 is SMH_ERR_INVALID (the reference divides by zero in
 * :32).  Vectors of the partitioned path are smh_par_vec: one full-length device buffer per local
 * block; block b OWNS entries [b R, (b+1) R), the rest of a buffer is valid as far as the last
 * upload / exchange made it so.  All smh_par_*_dev / _vec calls are asynchronous on the blocks'
 * private streams (ordered among themselves); smh_par_synchronize waits for them.              */
typedef struct smh_par smh_par;
typedef struct smh_par_vec smh_par_vec;
typedef struct smh_comm smh_comm; /* one rank of an RCCL communicator (one process per GPU) */

enum { SMH_EXCHANGE_NONE = 0, SMH_EXCHANGE_ALLGATHER = 1, SMH_EXCHANGE_WINDOW = 2, SMH_EXCHANGE_AUTO = 3 };
enum { SMH_PAR_BACKEND_AUTO = 0, SMH_PAR_BACKEND_PEER = 1, SMH_PAR_BACKEND_RCCL = 2 };
#define SMH_COMM_ID_BYTES 128

/* ncclGetUniqueId -> id_out[SMH_COMM_ID_BYTES]: call on ONE rank, hand the bytes to the others by any
 * host-side means (a file, a socket, the launcher's store), then every rank calls smh_comm_create
 * (ncclCommInitRank) with its rank on its device (smh_set_device first).  Collective. */
int smh_comm_unique_id(void *id_out);
int smh_comm_create(const void *id, int n_ranks, int rank, smh_comm **out);
int smh_comm_destroy(smh_comm *c);
int smh_comm_size(const smh_comm *c);
int smh_comm_rank(const smh_comm *c);
/* What RCCL itself reports (a first run on a node answers "did the library see N ranks, and which RCCL" by itself):
 * *count_out = ncclCommCount of the rank's communicator, *device_out = ncclCommCuDevice (either may be NULL);
 * *version_out = ncclGetVersion (e.g. 22203; needs no communicator). */
int smh_comm_ranks_seen(const smh_comm *c, int *count_out, int *device_out);
int smh_rccl_version(int *version_out);
/* helpers for a host without a collective library of its own (bench, tests): a barrier across the
 * ranks (device work of this rank's device drained first), and max over ranks of one double */
int smh_comm_barrier(smh_comm *c);
int smh_comm_max_f64(smh_comm *c, double *value_inout);

int smh_par_create(smh_dtype dtype, size_t n_blocks, const int *device_ids, size_t n_rows,
                   size_t n_cols, const uint32_t *offset_rows, const uint32_t *columns,
                   const void *values, int validate, smh_par **out);
/* WHERE the rows are cut ("nnz-balanced split points ... as an option for skewed matrices").  SMH_SPLIT_ROWS: the
 * reference's arithmetic -- R = n_rows / n_blocks rows per block (sparsemat_par.rs:21), the remainder to the last one.
 * SMH_SPLIT_NNZ: block k starts at the first row whose entries begin at or beyond k nnz / n_blocks (every block keeps at least one
 * row): equal work per GPU for skewed matrices.  The partition is then a table of n_blocks + 1 row boundaries (smh_par_split);
 * smh_par_get_block_and_row_id searches it, the window plan and the interior rows follow it, and the all-gather exchange -- whose
 * in-place ncclAllGather needs equal counts -- becomes one grouped launch of n_blocks ncclBroadcast, each slice from its owner.
 * smh_par_adopt_split / smh_par_create_rank_split take blocks cut elsewhere: split_rows = the n_blocks + 1 boundaries (NULL: the
 * reference's partition); row_begin = this rank's first row ((size_t)-1: the reference's partition; all ranks or none). */
enum { SMH_SPLIT_ROWS = 0, SMH_SPLIT_NNZ = 1 };
int smh_par_create_split(smh_dtype dtype, size_t n_blocks, const int *device_ids, size_t n_rows,
                         size_t n_cols, const uint32_t *offset_rows, const uint32_t *columns,
                         const void *values, int validate, int split_mode, smh_par **out);
int smh_par_adopt_split(size_t n_blocks, smh_crs *const *blocks, size_t n_rows, const size_t *split_rows, smh_par **out);
int smh_par_create_rank_split(smh_comm *comm, size_t n_rows, smh_crs *block, size_t row_begin, smh_par **out);
/* rows_out[k] .. rows_out[k + 1]: the rows of block k (n_blocks + 1 values, whichever way the partition was cut) */
int smh_par_split(const smh_par *p, size_t *rows_out);
/* blocks that already live on their devices (device-born inputs): blocks[b] = rows [b R, (b+1) R) of
 * an n_rows-row matrix, all with the same n_cols and dtype.  Borrowed: they must outlive the handle. */
int smh_par_adopt(size_t n_blocks, smh_crs *const *blocks, size_t n_rows, smh_par **out);
/* one process per GPU: this rank's block (borrowed) of an n_rows-row matrix; n_blocks = comm size,
 * block id = comm rank.  Collective (the ranks exchange their column intervals). */
int smh_par_create_rank(smh_comm *comm, size_t n_rows, smh_crs *block, smh_par **out);
int smh_par_destroy(smh_par *p);
size_t smh_par_n_blocks(const smh_par *p);
size_t smh_par_n_local_blocks(const smh_par *p);  /* n_blocks, or 1 with one process per GPU */
size_t smh_par_n_rows(const smh_par *p);
size_t smh_par_n_cols(const smh_par *p);          /* :109-115 */
size_t smh_par_nnz(const smh_par *p);             /* n_non_zero_entries :117-123 (local blocks) */
size_t smh_par_rows_per_block(const smh_par *p);  /* n_rows_sub_matrix :13 */
/* local block i: its device matrix (owned by the par handle unless adopted), global row range, device */
int smh_par_block(const smh_par *p, size_t block, smh_crs **crs_out, size_t *row_begin,
                  size_t *row_end, int *device);
/* the private stream local block i's work is enqueued on (to bracket it with events of the caller's) */
int smh_par_block_stream(const smh_par *p, size_t block, void **stream_out);
/* get_block_and_row_id (:31-35), clamped to the last block */
int smh_par_get_block_and_row_id(const smh_par *p, size_t row, size_t *block_out, size_t *row_out);
int smh_par_scale(smh_par *p, double a);          /* :135-139 */
/* exchange backend of a one-process handle (AUTO: RCCL when every block has a device of its own, else
 * PEER); SMH_PAR_BACKEND=peer|rccl in the environment overrides AUTO.  RCCL with blocks sharing a
 * device is SMH_ERR_INVALID; a per-rank handle is always RCCL. */
int smh_par_set_backend(smh_par *p, int backend);
int smh_par_backend(const smh_par *p);
/* The exchange beside the product (on by default; SMH_PAR_OVERLAP=0 in the environment switches it off).  The blocks of the
 * reference's design are independent (sparsemat_par.rs:54-64: every block multiplies on its own, results at b R), so the order
 * in which a block's rows are multiplied is free of semantics.  When the exchange of a call is a WINDOW and the block's kernel
 * can be launched by runs of rows (K1s: 256-row tiles, K1r: the plan's row ranges -- same kernels, same arithmetic per row, so
 * results are bit-identical either way), smh_par_spmv_dev multiplies the rows other blocks reference on a second stream per
 * block, the exchange behind them, and the block's INTERIOR rows on its main stream meanwhile; smh_par_cg_solve_vec starts the
 * exchange of p on the second stream and behind it the rows that wait for it, and multiplies the interior rows (which reference no
 * other block's entries) on the main stream meanwhile.  (Ring matrices: the few boundary rows go through the plain lane-group
 * kernel, whose results are the ring kernel's bit for bit.)  smh_par_interior:
 * the rows [*row_begin, *row_end) (local) of local block i that its kernel for `variant` treats as interior (equal: none -- the
 * call is then not split for that block). */
int smh_par_set_overlap(smh_par *p, int on);
/* One-process handles with several local blocks: every block's runtime calls (kernel launches, event records and waits) are issued
 * by a host thread of its own -- block 0's by the caller -- instead of one thread issuing them block after block (the reference's
 * intended design is independent blocks, sparsemat_par.rs:54-64).  mode: -1 automatic (off unless SMH_PAR_THREADS=1: with the blocks
 * on ONE device, the only set-up measured so far, the runtime serialises its callers and nothing is gained), 0 one issuing thread,
 * 1 a thread per block.  Streams, events, kernels and their order per block do not depend on it: results are
 * bit for bit the same.  Synchronises the handle's streams. */
int smh_par_set_threads(smh_par *p, int mode);
int smh_par_interior(const smh_par *p, size_t local_block, int variant, size_t *row_begin, size_t *row_end);
/* what SMH_EXCHANGE_AUTO resolves to for this matrix (WINDOW when the matrix is square and no block
 * receives half of the vector or more, else ALLGATHER; NONE for one block) and the largest number of
 * entries any block receives in a window exchange */
int smh_par_exchange_mode(const smh_par *p, int mode, int *resolved_out, size_t *max_recv_out);
/* The plan arithmetic on its own (pure host code, no device): block `block` of n_blocks over n_rows
 * rows, needs[q] != 0 iff block q has entries, referencing columns [lo[q], hi[q]] (inclusive).
 * recv_begin/end[q] = the range of q's slice this block receives in a window exchange, send_begin/
 * end[q] = the range of its own slice it sends to q (empty: begin == end == 0).  auto_mode_out /
 * max_recv_out as smh_par_exchange_mode (for a square matrix). */
int smh_par_plan(size_t n_blocks, size_t n_rows, const uint8_t *needs, const uint32_t *lo,
                 const uint32_t *hi, size_t block, size_t *recv_begin, size_t *recv_end,
                 size_t *send_begin, size_t *send_end, int *auto_mode_out, size_t *max_recv_out);
/* ... for a partition given by its n_blocks + 1 row boundaries (NULL: as smh_par_plan) */
int smh_par_plan_split(size_t n_blocks, size_t n_rows, const size_t *split_rows, const uint8_t *needs, const uint32_t *lo,
                       const uint32_t *hi, size_t block, size_t *recv_begin, size_t *recv_end,
                       size_t *send_begin, size_t *send_end, int *auto_mode_out, size_t *max_recv_out);

/* distributed DenseVec: n entries in one device buffer per local block.  upload replicates a host
 * vector into every local buffer; download collects the OWNED slices (n == n_rows) of the local
 * blocks at their global offsets (with one process per GPU: this rank's rows only);
 * download_block copies local block i's whole buffer; ptr gives its device pointer. */
int smh_par_vec_create(smh_par *p, size_t n, smh_par_vec **out);
int smh_par_vec_destroy(smh_par_vec *v);
size_t smh_par_vec_dim(const smh_par_vec *v);
int smh_par_vec_upload(smh_par_vec *v, const void *host);
int smh_par_vec_download(const smh_par_vec *v, void *host);
int smh_par_vec_download_block(const smh_par_vec *v, size_t local_block, void *host);
int smh_par_vec_ptr(const smh_par_vec *v, size_t local_block, void **dev_ptr_out);
/* the intended mvp_par (:37-68), device resident: every local block writes y[b R ..) = A_b x into ITS
 * slice of y (x must be valid on the columns the block references), then ONE exchange of y
 * (SMH_EXCHANGE_*): afterwards y is valid everywhere (ALLGATHER) or on every block's own slice plus the
 * columns it references (WINDOW) -- ready to be the next x.  x != y.  Asynchronous. */
int smh_par_spmv_dev(smh_par *p, const smh_par_vec *x, smh_par_vec *y, int variant, int exchange);
/* the exchange on its own: v (n == n_rows) holds every block's owned slice */
int smh_par_exchange(smh_par *p, smh_par_vec *v, int mode);
int smh_par_synchronize(smh_par *p);
/* y = A x on host vectors (the trait-default mvp through iter_row :86-89): blocks run concurrently,
 * each uploading only x[min column .. max column] of its rows.  One-process handles only. */
int smh_par_spmv(smh_par *p, const void *x_host, size_t x_len, void *y_host, int variant);
/* ConjugateGradient::solve (linearsolver.rs:27-61) with x, r, p, Ap distributed by rows: per iteration
 * ONE window exchange of p, the local SpMV, and two cross-block folds (p.Ap, r.r) of device-resident
 * scalars -- each block reduces its rows to one value, the values meet (peer-visible slots / a
 * 1-element ncclAllGather) and every block folds the same n_blocks values in the same fixed order, so
 * all blocks take the same alpha, beta and stop decision without the host; the host polls the stop
 * flag every check_every iterations (0: default) like smh_cg_solve.  _vec: b and x hold the owned
 * slices (x in/out).  The host-vector form takes full-length vectors (with one process per GPU only
 * this rank's rows of b are read and of x written).  Same statuses and outputs as smh_cg_solve. */
int smh_par_cg_solve_vec(smh_par *p, const smh_par_vec *b, smh_par_vec *x, double tol, size_t iter_max,
                         int variant, size_t check_every, size_t *iters_out, double *rr_out);
int smh_par_cg_solve(smh_par *p, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len,
                     double tol, size_t iter_max, int variant, size_t *iters_out, double *rr_out);

/* ---- synthetic workloads (bench / test support, DESIGN.md "Synthetic inputs") ------------
 * Counter-based generators writing straight into device memory so 10M..80M-row inputs never
 * cross PCIe.  pattern: 0 banded-stratified (ascending), 1 uniform (draw order),
 * 2 contiguous band (k consecutive columns around the diagonal), 3 window (k <= 64 distinct
 * columns drawn without replacement from [row - 4096, row + 4096], ascending).              */
int smh_synth_x(smh_dtype dtype, uint64_t seed, size_t begin, size_t n, void *x_dev, void *stream);
int smh_synth_fixed(smh_dtype dtype, uint64_t seed, int pattern, size_t n, uint32_t k,
                    size_t row_begin, size_t row_end, uint32_t *offset_rows_dev,
                    uint32_t *columns_dev, void *values_dev, void *stream);
int smh_synth_powerlaw_cdf(uint32_t kmax, double alpha, uint32_t *cdf_host);
int smh_synth_powerlaw_lengths(uint64_t seed, size_t row_begin, size_t row_end, uint32_t kmax,
                               const uint32_t *cdf_host, uint32_t *lengths_host);
int smh_synth_fill(smh_dtype dtype, uint64_t seed, size_t n_cols, size_t row_begin, size_t row_end,
                   const uint32_t *offset_rows_dev, uint32_t *columns_dev, void *values_dev,
                   void *stream);
/* 7-point Laplacian on an nx*ny*nz grid (natural ordering, diag 6, off-diag -1), rows
 * [row_begin,row_end), offsets rebased.  offsets need rows+1, columns/values nnz entries
 * (call with NULL arrays to get nnz_out only).                                            */
int smh_synth_laplace3d(smh_dtype dtype, size_t nx, size_t ny, size_t nz, size_t row_begin,
                        size_t row_end, uint32_t *offset_rows_dev, uint32_t *columns_dev,
                        void *values_dev, size_t *nnz_out, void *stream);

/* ---- device memory kept by the library ---------------------------------------------------
 * Everything the library allocates on a device (matrix arrays, plans, scratch of assembly /
 * transpose / prod, vectors, smh_dev_alloc) goes through a caching layer (csrc/pool.hip): freed
 * blocks of 1 MiB and more stay with the library, at most SMH_POOL_MAX_BYTES per device (environment,
 * default 16 GiB, 0 = off), because a fresh hipMalloc of a few GB takes 1.2-1.4 s every few calls
 * on this platform.  smh_pool_trim returns everything kept to the HIP runtime (call it before
 * another library in the process needs the memory); smh_pool_stats reports kept and in-use bytes
 * of pooled blocks.  Not part of the reference's interface (its Vec allocations have no such cost). */
int smh_pool_trim(void);
int smh_pool_stats(size_t *kept_bytes_out, size_t *live_bytes_out);

/* ---- raw device memory helpers for hosts without a HIP binding (the Rust shim) ---------- */
int smh_dev_alloc(size_t bytes, void **out);
int smh_dev_free(void *p);
int smh_dev_upload(void *dst_dev, const void *src_host, size_t bytes);
int smh_dev_download(void *dst_host, const void *src_dev, size_t bytes);
int smh_dev_memset(void *dst_dev, int value, size_t bytes, void *stream); /* asynchronous */
/* streams and timing events (hipStream_t / hipEvent_t as void*): what bench.py brackets every launch with */
int smh_stream_create(void **stream_out);
int smh_stream_destroy(void *stream);
int smh_stream_synchronize(void *stream);
int smh_event_create(void **event_out);
int smh_event_destroy(void *event);
int smh_event_record(void *event, void *stream);
int smh_event_elapsed_ms(void *start, void *stop, float *ms_out); /* waits for `stop` */

#ifdef __cplusplus
}
#endif
#endif /* SPARSEMAT_HIP_H */
