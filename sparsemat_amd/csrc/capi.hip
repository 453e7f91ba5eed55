// capi.hip -- extern "C" boundary of libsparsemat_hip.so (see include/sparsemat_hip.h).
//
// Host-side logic only: argument checks with the reference's panic conditions, HBM residency of
// the CRS arrays, handle creation.  What a handle derives is built in crs_forms.hip; which kernel a product runs and its
// launches are spmv_dispatch.hip's.  No CPU compute path exists here: every entry point that computes needs a HIP device.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "crs_forms.hpp"
#include "solver_host.hpp"

namespace smh {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

void clear_error() { g_err[0] = 0; }

int fail(int status, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return status;
}

int hip_fail(hipError_t e, const char *what, const char *file, int line) {
    int status = (e == hipErrorOutOfMemory) ? SMH_ERR_OOM : (e == hipErrorNoDevice ? SMH_ERR_NO_DEVICE : SMH_ERR_HIP);
    snprintf(g_err, sizeof g_err, "HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    (void)hipGetLastError();  // clear sticky state
    return status;
}

int require_device() {
    note_thread();
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(SMH_ERR_NO_DEVICE, "no HIP device visible: libsparsemat_hip has no CPU fallback");
    }
    return SMH_OK;
}

// host threads using the library, and captures in progress (internal.hpp: "host threads and graph capture").  Both counters
// are sequentially consistent: of a thread that enters a capture and a thread that is counted at the same moment at least one
// sees the other -- the first backs off, or the second waits.
__thread bool t_thread_counted = false;
__thread int t_solve_replays = 0;
static std::atomic<int> g_threads{0}, g_capturing{0};

void count_thread() {
    struct Counted {
        Counted() { g_threads.fetch_add(1); }
        ~Counted() { g_threads.fetch_sub(1); }
    };
    static thread_local Counted counted;  // (leaves the count when the thread ends)
    (void)counted;
    t_thread_counted = true;
    while (g_capturing.load() > 0) std::this_thread::yield();
}

bool capture_enter() {
    note_thread();
    g_capturing.fetch_add(1);
    if (g_threads.load() > 1) {
        g_capturing.fetch_sub(1);
        return false;
    }
    return true;
}

void capture_leave() { g_capturing.fetch_sub(1); }

}  // namespace smh

extern "C" int smh_last_solve_replays(void) { return smh::t_solve_replays; }

namespace smh {

uint64_t next_crs_id() {
    static std::atomic<uint64_t> next{1};
    return next.fetch_add(1, std::memory_order_relaxed);
}

int current_device() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); d = 0; }
    return d;
}

// defined in the kernel files
int cg_solve(smh_crs *m, const smh_vec *b, smh_vec *x, double tol, size_t iter_max, int variant, size_t check_every, size_t *iters_out,
             double *rr_out);  // cg.hip: the solve behind smh_cg_solve_vec
int synth_x(int dtype, uint64_t seed, size_t begin, size_t n, void *x, hipStream_t s);
int synth_fixed(int dtype, uint64_t seed, int pattern, size_t n, uint32_t k, size_t row_begin, size_t row_end,
                uint32_t *off, uint32_t *col, void *val, hipStream_t s);
int synth_fill(int dtype, uint64_t seed, size_t n_cols, size_t row_begin, size_t row_end, const uint32_t *off,
               uint32_t *col, void *val, hipStream_t s);
size_t synth_laplace3d_nnz(size_t nx, size_t ny, size_t nz, size_t row_begin, size_t row_end);
int synth_laplace3d(int dtype, size_t nx, size_t ny, size_t nz, size_t row_begin, size_t row_end, uint32_t *off,
                    uint32_t *col, void *val, hipStream_t s);
void synth_powerlaw_cdf(uint32_t kmax, double alpha, uint32_t *cdf);
void synth_powerlaw_lengths(uint64_t seed, size_t row_begin, size_t row_end, uint32_t kmax, const uint32_t *cdf,
                            uint32_t *lengths);

static bool valid_dtype(int dt) { return dt == SMH_F32 || dt == SMH_F64; }

static int finish_create_inner(smh_crs *m, int validate) {
    SMH_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    if (m->n_rows > 0) {
        CrsStats h_st;
        {
            Scratch scr;
            CrsStats *d_st = nullptr;
            SMH_TRY(scr.alloc(&d_st, 1));
            SMH_TRY(read_back(d_st, &h_st, 1, m->stream, [&](CrsStats *d) { return launch_crs_stats(m->d_off, m->d_col, m->n_rows, m->nnz, d, m->stream); }));
            // (reuse the first word of the scratch for the K1s tile statistics: 256-row and 512-row tiles)
            if (!(h_st.bad & 1u)) {
                uint32_t *d_word = &d_st->max_row_len;
                SMH_TRY(read_back(d_word, &m->max_tile_entries, 1, m->stream,
                                  [&](uint32_t *d) { return launch_stream_max_tile(m->d_off, m->n_rows, kStreamRows, d, m->stream); }));
                SMH_TRY(read_back(d_word, &m->max_tile512_entries, 1, m->stream,
                                  [&](uint32_t *d) { return launch_stream_max_tile(m->d_off, m->n_rows, 2 * kStreamRows, d, m->stream); }));
            }
        }
        m->max_row_len = h_st.max_row_len;
        m->max_col = h_st.max_col;
        m->min_col = m->nnz ? ~h_st.min_col_inv : 0u;
        m->have_stats = true;
        // a malformed row structure would send the kernels out of bounds: always refused
        if (h_st.bad & 1u) return fail(SMH_ERR_INVALID, "offset_rows is not monotone non-decreasing");
        if (h_st.bad & 2u) return fail(SMH_ERR_INVALID, "offset_rows[0] != 0");
        if (h_st.bad & 4u) return fail(SMH_ERR_INVALID, "offset_rows[n_rows] != nnz");
        if (validate && m->nnz > 0 && (size_t)h_st.max_col >= m->n_cols)
            return fail(SMH_ERR_INDEX_RANGE, "column index %u >= n_cols %zu", h_st.max_col, m->n_cols);
        // x larger than the L2s: take the locality statistic AUTO needs (one pass over columns[]; it is the K1r
        // inspector, so its plan is ready too)
        // ... and rows long enough for the lane-group kernels: AUTO wants to know whether their columns fit the ring
        const bool lane_group_rows = m->n_rows && m->nnz > 8 * m->n_rows;  // (mean row > 8)
        if (m->n_cols * dtype_size(m->dtype) >= kColblockMinXBytes || lane_group_rows)
            SMH_TRY(ensure_ring_plan(m, lane_group_rows));
    }
    return SMH_OK;
}
static int finish_create(smh_crs *m, int validate) {
    // (what the create-time inspection costs: the statistics passes and, for matrices AUTO needs it for, the K1r inspector)
    const auto t0 = std::chrono::steady_clock::now();
    const long long b0 = pool_thread_net_bytes();
    const int rc = finish_create_inner(m, validate);
    m->create_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    m->create_bytes = pool_thread_net_bytes() - b0;
    return rc;
}

// Every handle is made here: a fresh handle on the current device over device arrays, with the create-time inspection done
// (finish_create).  like (optional): the settings it takes, else the defaults.  Owned arrays go with the handle, also on failure;
// borrowed ones are never freed by it.
static int wrap_arrays(int dtype, const smh_crs *like, size_t n_rows, size_t n_cols, size_t nnz, uint32_t *off, uint32_t *col, void *val,
                       bool owns, int validate, smh_crs **out) {
    smh_crs *m = new (std::nothrow) smh_crs();
    if (!m) {
        if (owns) { (void)hipFree(off); (void)hipFree(col); (void)hipFree(val); }
        return fail(SMH_ERR_OOM, "host allocation failed");
    }
    m->dtype = dtype; m->device = current_device(); m->owns = owns;
    m->n_rows = n_rows; m->n_cols = n_cols; m->nnz = nnz;
    m->d_off = off; m->d_col = col; m->d_val = val;
    if (like) m->knobs = like->knobs;
    const int rc = finish_create(m, validate);
    if (rc != SMH_OK) return keep_error(rc, [&] { (void)smh_crs_destroy(m); });
    *out = m;
    return SMH_OK;
}
// ... the handle takes the arrays of `arrays`
int wrap_arrays(int dtype, const smh_crs *like, size_t n_rows, size_t n_cols, size_t nnz, CrsArrays &arrays, int validate, smh_crs **out) {
    uint32_t *off = nullptr, *col = nullptr;
    void *val = nullptr;
    arrays.release(&off, &col, &val);
    return wrap_arrays(dtype, like, n_rows, n_cols, nnz, off, col, val, true, validate, out);
}

static int check_create_args(int dtype, size_t n_rows, size_t nnz, const void *off, const void *col, const void *val,
                             smh_crs **out) {
    if (!out) return fail(SMH_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid_dtype(dtype)) return fail(SMH_ERR_INVALID, "dtype must be SMH_F32 or SMH_F64");
    // Index = u32: UNSET = u32::MAX is reserved, entry count must stay below it (sparsemat_crs.rs:82-84)
    if (nnz >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "Maximum number of %u entries reached", 0xFFFFFFFFu);
    if (n_rows >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "n_rows does not fit the u32 index type");
    if (n_rows > 0 && !off) return fail(SMH_ERR_INVALID, "offset_rows is NULL");
    if (nnz > 0 && (!col || !val)) return fail(SMH_ERR_INVALID, "columns/values is NULL");
    return SMH_OK;
}

static int vec_check_pair(const smh_vec *x, const smh_vec *y) {
    if (!x || !y) return fail(SMH_ERR_INVALID, "NULL vector handle");
    if (x->dtype != y->dtype) return fail(SMH_ERR_INVALID, "vector dtype mismatch");
    return SMH_OK;
}

// The element-wise kernels (k_ew, blas1.hip) read y[i] and write x[i] in the same thread and know nothing about any other thread's
// entries: over the n entries they touch, x and y are the same array or disjoint.  Two ranges that overlap IN PART would make thread i
// read what thread i +- k writes -- a result that depends on scheduling -- so they are refused before anything is launched.
static int ew_check_overlap(const void *x, const void *y, size_t n, int dtype, const char *what) {
    const size_t bytes = n * dtype_size(dtype);
    const char *px = (const char *)x, *py = (const char *)y;
    if (px != py && px < py + bytes && py < px + bytes) return fail(SMH_ERR_INVALID, "%s: x and y overlap in part", what);
    return SMH_OK;
}

// scratch for reductions of the vector API: per thread, per device
struct ReduceBuffer { void *d = nullptr; int device = -1; };
static thread_local ReduceBuffer g_red;
static int reduce_scratch(void **out) {
    const int dev = current_device();
    if (!g_red.d || g_red.device != dev) {
        // (a scratch left on another device is intentionally leaked: handles are device-bound)
        SMH_HIP(hipMalloc(&g_red.d, (kReducePartials + 8) * sizeof(double)));
        g_red.device = dev;
    }
    *out = g_red.d;
    return SMH_OK;
}

}  // namespace smh

using namespace smh;

extern "C" {

int smh_abi_version(void) { return SMH_ABI_VERSION; }

const char *smh_last_error(void) { return g_err; }

const char *smh_status_string(int status) {
    switch (status) {
        case SMH_OK: return "ok";
        case SMH_ERR_DIM_MISMATCH: return "Dimension mismatch";
        case SMH_ERR_NOT_SQUARE: return "Matrix is not symmetric";
        case SMH_ERR_INDEX_RANGE: return "index out of bounds";
        case SMH_ERR_INVALID: return "invalid argument";
        case SMH_ERR_HIP: return "HIP runtime error";
        case SMH_ERR_OOM: return "out of device memory";
        case SMH_ERR_NO_DEVICE: return "no HIP device (no CPU fallback)";
        case SMH_ERR_CAPACITY: return "Maximum number of entries reached";
        case SMH_ERR_COMM: return "RCCL error";
        default: return "unknown status";
    }
}

int smh_device_count(int *count_out) {
    if (!count_out) return fail(SMH_ERR_INVALID, "count_out is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); n = 0; }
    *count_out = n;
    return SMH_OK;
}

int smh_set_device(int device) {
    SMH_TRY(require_device());
    SMH_HIP(hipSetDevice(device));
    return SMH_OK;
}

int smh_device_synchronize(void) {
    SMH_TRY(require_device());
    SMH_HIP(hipDeviceSynchronize());
    return SMH_OK;
}

// ---- SparseMatCRS ------------------------------------------------------------------------------------
int smh_crs_create(smh_dtype dtype, size_t n_rows, size_t n_cols, size_t nnz, const uint32_t *offset_rows,
                   const uint32_t *columns, const void *values, int validate, smh_crs **out) {
    SMH_TRY(check_create_args(dtype, n_rows, nnz, offset_rows, columns, values, out));
    SMH_TRY(require_device());
    const size_t vs = dtype_size(dtype);
    CrsArrays arrays;
    SMH_TRY(arrays.alloc(n_rows, nnz, vs));
    if (n_rows > 0) SMH_HIP(hipMemcpy(arrays.off, offset_rows, (n_rows + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    else SMH_HIP(hipMemset(arrays.off, 0, sizeof(uint32_t)));
    if (nnz > 0) {
        SMH_HIP(hipMemcpy(arrays.col, columns, nnz * sizeof(uint32_t), hipMemcpyHostToDevice));
        SMH_HIP(hipMemcpy(arrays.val, values, nnz * vs, hipMemcpyHostToDevice));
    }
    return wrap_arrays(dtype, nullptr, n_rows, n_cols, nnz, arrays, validate, out);
}

int smh_crs_create_dev(smh_dtype dtype, size_t n_rows, size_t n_cols, size_t nnz, const uint32_t *offset_rows_dev,
                       const uint32_t *columns_dev, const void *values_dev, int validate, smh_crs **out) {
    SMH_TRY(check_create_args(dtype, n_rows, nnz, offset_rows_dev, columns_dev, values_dev, out));
    SMH_TRY(require_device());
    if (((uintptr_t)columns_dev & 15u) || ((uintptr_t)values_dev & 15u))
        return fail(SMH_ERR_INVALID, "columns/values device pointers must be 16-byte aligned");
    return wrap_arrays(dtype, nullptr, n_rows, n_cols, nnz, const_cast<uint32_t *>(offset_rows_dev), const_cast<uint32_t *>(columns_dev),
                       const_cast<void *>(values_dev), false, validate, out);
}

// a device copy of a host array (none of a null one), freed with `scr`
static int upload(Scratch &scr, const void *host, size_t bytes, const void **dev) {
    *dev = nullptr;
    if (!host) return SMH_OK;
    char *d = nullptr;
    SMH_TRY(scr.alloc(&d, bytes));
    if (bytes) SMH_HIP(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
    *dev = d;
    return SMH_OK;
}

// add_to / set stream -> CRS (assemble.hip).  `on_device`: the arrays are device pointers.
// into_crs: the stream is replayed on a SparseMatCRS instead of a SparseMatIndexList + to_crs(): rows come out in reverse order
// of first appearance (push prepends, sparsemat_crs.rs:85-87) and the container's first-push quirk applies (:75-81: the first push
// leaves n_rows == 0, so the second operation never finds an entry):
//   * second row <  first row: Vec::resize truncates offset_rows and the first entry is orphaned -- it stays in columns / values
//     (and in n_cols) but no row reaches it; the result is the replay of operations 1.. alone.  Orphans are not materialised here;
//   * second (row, column) == first: the first operation keeps an entry of its own, the oldest of its row (= last in storage);
//   * a single operation: no rows at all (n_rows stays 0), one orphan.
static int assemble_common(smh_dtype dtype, size_t n_ops, const uint32_t *rows, const uint32_t *cols, const void *values,
                           const uint8_t *ops, bool on_device, bool into_crs, smh_crs **out, bool transposing = false) {
    // transposing: every operation is `set` (ops unused) and repeats of a (row, column) pair are neighbours in the row's list
    if (!out) return fail(SMH_ERR_INVALID, "NULL out pointer");
    if (dtype != SMH_F32 && dtype != SMH_F64) return fail(SMH_ERR_INVALID, "unknown dtype %d", (int)dtype);
    if (n_ops && (!rows || !cols || !values)) return fail(SMH_ERR_INVALID, "NULL operation array");
    if (n_ops >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "Maximum number of %u entries reached", 0xFFFFFFFFu);
    SMH_TRY(require_device());
    const size_t vs = dtype_size(dtype);
    // the first two operations decide the SparseMatCRS quirk
    size_t skip = 0, min_cols = 0, orphans = 0;
    bool twin = false;
    uint32_t r01[2] = {0, 0}, c01[2] = {0, 0};
    double v0 = 0.0;  // (holds an f32 or an f64 bit pattern)
    uint8_t op0 = 0;
    auto fold_v0 = [&]() {  // push(i, j, zero) then `=` or `+=` (sparsematrix.rs:226-233)
        if (op0) return;
        if (dtype == SMH_F64) { double v; memcpy(&v, &v0, 8); v = 0.0 + v; memcpy(&v0, &v, 8); }
        else { float v; memcpy(&v, &v0, 4); v = 0.0f + v; memcpy(&v0, &v, 4); }
    };
    if (into_crs && n_ops) {
        const size_t k = n_ops < 2 ? n_ops : 2;
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost;
        SMH_HIP(hipMemcpy(r01, rows, k * sizeof(uint32_t), kind));
        SMH_HIP(hipMemcpy(c01, cols, k * sizeof(uint32_t), kind));
        SMH_HIP(hipMemcpy(&v0, values, vs, kind));
        if (transposing) op0 = 1;
        else if (ops) SMH_HIP(hipMemcpy(&op0, ops, 1, kind));
        if (n_ops == 1) { fold_v0(); orphans = 1; }
        else if (r01[1] < r01[0]) { skip = 1; min_cols = (size_t)c01[0] + 1; orphans = 1; }
        else if (r01[1] == r01[0] && c01[1] == c01[0]) { skip = 1; twin = true; }
    }
    Scratch in;  // device copies of host operation arrays
    CrsArrays arrays;
    size_t n_rows = 0, n_cols = 0, nnz = 0;
    const bool single = into_crs && n_ops == 1;
    if (n_ops == 0 || single) {  // SparseMatCRS::new() (sparsemat_crs.rs:47-49): no rows at all
        SMH_TRY(arrays.alloc(0, 0, vs));
        SMH_HIP(hipMemset(arrays.off, 0, sizeof(uint32_t)));
        n_cols = single ? (size_t)c01[0] + 1 : 0;
    } else {
        const void *d_rows = rows, *d_cols = cols, *d_vals = values, *d_ops = ops;
        if (!on_device) {
            SMH_TRY(upload(in, rows, n_ops * sizeof(uint32_t), &d_rows));
            SMH_TRY(upload(in, cols, n_ops * sizeof(uint32_t), &d_cols));
            SMH_TRY(upload(in, values, n_ops * vs, &d_vals));
            SMH_TRY(upload(in, ops, n_ops, &d_ops));
        }
        SMH_TRY(assemble_triplets(dtype, n_ops - skip, (const uint32_t *)d_rows + skip, (const uint32_t *)d_cols + skip, (const char *)d_vals + skip * vs,
                                  d_ops ? (const uint8_t *)d_ops + skip : nullptr, into_crs, transposing, transposing, &n_rows, &n_cols, &nnz,
                                  &arrays.off, &arrays.col, &arrays.val, nullptr));
        if (min_cols > n_cols) n_cols = min_cols;
        if (twin) {  // the first operation's own entry
            fold_v0();
            SMH_TRY(append_to_row(dtype, arrays.off, &arrays.col, &arrays.val, n_rows, &nnz, r01[0], c01[0], &v0, nullptr));
        }
    }
    SMH_TRY(wrap_arrays(dtype, nullptr, n_rows, n_cols, nnz, arrays, 0, out));
    (*out)->orphans = orphans;
    if (single) {  // push(i, j, zero) then `=` or `+=`: kept on the handle so that smh_crs_apply can continue the replay; nothing else reads it
        (*out)->has_first_op = true;
        (*out)->first_row = r01[0];
        (*out)->first_col = c01[0];
        memcpy(&(*out)->first_val_bits, &v0, 8);
    }
    return SMH_OK;
}

int smh_crs_assemble(smh_dtype dtype, size_t n_ops, const uint32_t *rows, const uint32_t *cols, const void *values,
                     const uint8_t *ops, smh_crs **out) {
    return assemble_common(dtype, n_ops, rows, cols, values, ops, false, false, out);
}

int smh_crs_assemble_dev(smh_dtype dtype, size_t n_ops, const uint32_t *rows_dev, const uint32_t *cols_dev,
                         const void *values_dev, const uint8_t *ops_dev, smh_crs **out) {
    return assemble_common(dtype, n_ops, rows_dev, cols_dev, values_dev, ops_dev, true, false, out);
}

int smh_crs_replay(smh_dtype dtype, size_t n_ops, const uint32_t *rows, const uint32_t *cols, const void *values,
                   const uint8_t *ops, smh_crs **out) {
    return assemble_common(dtype, n_ops, rows, cols, values, ops, false, true, out);
}

int smh_crs_replay_dev(smh_dtype dtype, size_t n_ops, const uint32_t *rows_dev, const uint32_t *cols_dev,
                       const void *values_dev, const uint8_t *ops_dev, smh_crs **out) {
    return assemble_common(dtype, n_ops, rows_dev, cols_dev, values_dev, ops_dev, true, true, out);
}

static thread_local int g_transpose_route = 0;
int smh_last_transpose_route(void) { return g_transpose_route; }

// SparseMatrix::transpose (sparsematrix.rs:174-184) for Self = SparseMatCRS: `ret.set(j, i, val)` for every entry in row-major
// storage order into a fresh SparseMatCRS -- the replay above with rows = the columns array (borrowed), columns = the row of
// every entry, all operations `set`.
int smh_crs_transpose(const smh_crs *a, smh_crs **out) {
    if (!a || !out) return fail(SMH_ERR_INVALID, "NULL argument");
    SMH_HIP(hipStreamSynchronize(a->stream));
    if (a->nnz == 0) return assemble_common((smh_dtype)a->dtype, 0, nullptr, nullptr, nullptr, nullptr, true, true, out);
    g_transpose_route = 0;
    // matrices with local structure: two bucketed passes instead of the device-wide sort (transpose_bucket.hip).  The container's first-push quirks (second target row below the first: the first entry is
    // orphaned; a single operation) and repeated (row, column) pairs stay with the general route.
    const bool bucketed_allowed = !(getenv("SMH_TRANSPOSE_BUCKETED") && atoi(getenv("SMH_TRANSPOSE_BUCKETED")) == 0);
    if (bucketed_allowed && a->nnz >= 2 && a->have_stats) {
        uint32_t c01[2] = {0, 0};
        SMH_HIP(hipMemcpy(c01, a->d_col, sizeof c01, hipMemcpyDeviceToHost));
        if (c01[1] >= c01[0]) {
            CrsArrays t;
            size_t t_rows = 0, t_cols = 0;
            bool done = false;
            SMH_TRY(transpose_bucketed(a->dtype, a->d_off, a->d_col, a->d_val, a->n_rows, a->nnz, a->max_col, &t.off, &t.col, &t.val, &t_rows, &t_cols, &done,
                                       nullptr));
            if (done) {
                SMH_TRY(wrap_arrays(a->dtype, nullptr, t_rows, t_cols, a->nnz, t, 0, out));
                g_transpose_route = 1;
                return SMH_OK;
            }
        }
    }
    Scratch scr;
    uint32_t *d_rowof = nullptr;
    SMH_TRY(scr.alloc(&d_rowof, a->nnz));
    SMH_TRY(expand_rows(a->d_off, a->n_rows, d_rowof, nullptr));
    SMH_HIP(hipStreamSynchronize(nullptr));
    return assemble_common((smh_dtype)a->dtype, a->nnz, a->d_col, d_rowof, a->d_val, nullptr, true, true, out, true);
}

static int column_info_common(const smh_crs *m, uint32_t *rows, uint32_t *col_ptr, uint32_t *entries, bool on_device) {
    if (!m || !rows || !col_ptr || !entries) return fail(SMH_ERR_INVALID, "NULL argument");
    if (m->nnz && (size_t)m->max_col >= m->n_cols)
        return fail(SMH_ERR_INDEX_RANGE, "column %u out of range for %zu columns", m->max_col, m->n_cols);
    SMH_HIP(hipStreamSynchronize(m->stream));
    if (on_device) return column_info(m->d_off, m->d_col, m->n_rows, m->n_cols, m->nnz, m->max_col, rows, col_ptr, entries, m->stream);
    Scratch scr;
    uint32_t *d[3] = {nullptr, nullptr, nullptr};
    SMH_TRY(scr.alloc(&d[0], m->nnz));
    SMH_TRY(scr.alloc(&d[1], m->n_cols + 1));
    SMH_TRY(scr.alloc(&d[2], m->nnz));
    SMH_TRY(column_info(m->d_off, m->d_col, m->n_rows, m->n_cols, m->nnz, m->max_col, d[0], d[1], d[2], m->stream));
    if (m->nnz) SMH_HIP(hipMemcpy(rows, d[0], m->nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
    SMH_HIP(hipMemcpy(col_ptr, d[1], (m->n_cols + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (m->nnz) SMH_HIP(hipMemcpy(entries, d[2], m->nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SMH_OK;
}

int smh_crs_column_info(const smh_crs *m, uint32_t *rows, uint32_t *col_ptr, uint32_t *entries) {
    return column_info_common(m, rows, col_ptr, entries, false);
}

int smh_crs_column_info_dev(const smh_crs *m, uint32_t *rows_dev, uint32_t *col_ptr_dev, uint32_t *entries_dev) {
    return column_info_common(m, rows_dev, col_ptr_dev, entries_dev, true);
}

// SparseMatrix::prod (sparsematrix.rs:186-210) for SparseMatCRS operands; Err("Dimension mismatch") of :188-190 as a status
int smh_crs_prod(const smh_crs *a, const smh_crs *b, smh_crs **out) {
    if (!a || !b || !out) return fail(SMH_ERR_INVALID, "NULL argument");
    if (a->dtype != b->dtype) return fail(SMH_ERR_INVALID, "operands differ in value type");
    if (a->n_rows != b->n_cols || a->n_cols != b->n_rows) return fail(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
    if (a->nnz && (size_t)a->max_col >= a->n_cols)
        return fail(SMH_ERR_INDEX_RANGE, "column %u out of range for %zu columns", a->max_col, a->n_cols);
    SMH_HIP(hipStreamSynchronize(a->stream));
    SMH_HIP(hipStreamSynchronize(b->stream));
    CrsArrays arrays;
    size_t n_rows = 0, n_cols = 0, nnz = 0;
    SMH_TRY(prod_crs(a->dtype, a->d_off, a->d_col, a->d_val, a->n_rows, a->nnz, a->max_col, b->d_off, b->d_col, b->d_val, b->n_rows, &n_rows, &n_cols,
                     &nnz, &arrays.off, &arrays.col, &arrays.val, nullptr));
    return wrap_arrays(a->dtype, nullptr, n_rows, n_cols, nnz, arrays, 0, out);
}

// ---- reordering (EXTENSION; permute.hip, reorder.hip): a permutation is n u32 with perm[new] = old ---------------------------
static int check_dev_array(const void *p, int device, const char *what);
// One permutation argument of an entry point: checked for its length, brought to the device when it is a host array, validated
// there (`inv` = its inverse afterwards).  perm == NULL: the identity, nothing to do (*d_perm stays null).
static int take_permutation(Scratch &scr, const uint32_t *perm, size_t len, size_t n, bool on_device, int device, const char *what,
                            const uint32_t **d_perm, uint32_t **inv) {
    *d_perm = nullptr;
    *inv = nullptr;
    if (!perm) return SMH_OK;
    if (len != n) return fail(SMH_ERR_DIM_MISMATCH, "%s has %zu entries, %zu expected", what, len, n);
    if (n == 0) return SMH_OK;
    if (on_device) {
        SMH_TRY(check_dev_array(perm, device, what));
        *d_perm = perm;
    } else {
        const void *d = nullptr;
        SMH_TRY(upload(scr, perm, n * sizeof(uint32_t), &d));
        *d_perm = (const uint32_t *)d;
    }
    SMH_TRY(scr.alloc(inv, n));
    return validate_permutation(*d_perm, n, *inv, what, nullptr);
}

static int permute_common(const smh_crs *a, const uint32_t *row_perm, size_t n_row_perm, const uint32_t *col_perm, size_t n_col_perm, bool on_device,
                          smh_crs **out) {
    if (!out) return fail(SMH_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!a) return fail(SMH_ERR_INVALID, "NULL handle");
    if (a->orphans) return fail(SMH_ERR_INVALID, "a handle holding an orphaned entry cannot be permuted");
    if (col_perm) SMH_TRY(columns_within_n_cols(a, "permute"));
    if (on_device) SMH_HIP(hipDeviceSynchronize());  // the caller's writes to the arrays come first
    SMH_HIP(hipStreamSynchronize(a->stream));
    Scratch scr;
    const uint32_t *d_rp = nullptr, *d_cp = nullptr;
    uint32_t *row_inv = nullptr, *col_inv = nullptr;
    SMH_TRY(take_permutation(scr, row_perm, n_row_perm, a->n_rows, on_device, a->device, "row_perm", &d_rp, &row_inv));
    SMH_TRY(take_permutation(scr, col_perm, n_col_perm, a->n_cols, on_device, a->device, "col_perm", &d_cp, &col_inv));
    CrsArrays arrays;
    SMH_TRY(permute_crs(a->dtype, a->d_off, a->d_col, a->d_val, a->n_rows, a->nnz, d_rp, col_inv, &arrays, nullptr));
    return wrap_arrays(a->dtype, a, a->n_rows, a->n_cols, a->nnz, arrays, 0, out);
}

int smh_crs_permute(const smh_crs *a, const uint32_t *row_perm, size_t n_row_perm, const uint32_t *col_perm, size_t n_col_perm, smh_crs **out) {
    return permute_common(a, row_perm, n_row_perm, col_perm, n_col_perm, false, out);
}
int smh_crs_permute_dev(const smh_crs *a, const uint32_t *row_perm_dev, size_t n_row_perm, const uint32_t *col_perm_dev, size_t n_col_perm,
                        smh_crs **out) {
    return permute_common(a, row_perm_dev, n_row_perm, col_perm_dev, n_col_perm, true, out);
}

static int permute_symmetric_common(const smh_crs *a, const uint32_t *perm, size_t n_perm, bool on_device, smh_crs **out) {
    if (!out) return fail(SMH_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!a || !perm) return fail(SMH_ERR_INVALID, "NULL argument");
    if (a->n_rows != a->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");
    if (a->orphans) return fail(SMH_ERR_INVALID, "a handle holding an orphaned entry cannot be permuted");
    SMH_TRY(columns_within_n_cols(a, "permute_symmetric"));
    if (on_device) SMH_HIP(hipDeviceSynchronize());
    SMH_HIP(hipStreamSynchronize(a->stream));
    Scratch scr;
    const uint32_t *d_p = nullptr;
    uint32_t *inv = nullptr;
    SMH_TRY(take_permutation(scr, perm, n_perm, a->n_rows, on_device, a->device, "perm", &d_p, &inv));  // (validated once, one inverse)
    CrsArrays arrays;
    SMH_TRY(permute_crs(a->dtype, a->d_off, a->d_col, a->d_val, a->n_rows, a->nnz, d_p, inv, &arrays, nullptr));
    return wrap_arrays(a->dtype, a, a->n_rows, a->n_cols, a->nnz, arrays, 0, out);
}

int smh_crs_permute_symmetric(const smh_crs *a, const uint32_t *perm, size_t n_perm, smh_crs **out) {
    return permute_symmetric_common(a, perm, n_perm, false, out);
}
int smh_crs_permute_symmetric_dev(const smh_crs *a, const uint32_t *perm_dev, size_t n_perm, smh_crs **out) {
    return permute_symmetric_common(a, perm_dev, n_perm, true, out);
}

static int vec_permute_common(smh_vec *dst, const smh_vec *src, const uint32_t *perm, size_t n_perm, int inverse, bool on_device) {
    SMH_TRY(vec_check_pair(dst, src));
    if (!perm && n_perm) return fail(SMH_ERR_INVALID, "perm is NULL");
    if (dst->n != src->n) return fail(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
    if (dst == src || (dst->d && dst->d == src->d)) return fail(SMH_ERR_INVALID, "a vector cannot be permuted into itself");
    if (n_perm != src->n) return fail(SMH_ERR_DIM_MISMATCH, "perm has %zu entries, %zu expected", n_perm, src->n);
    if (src->n == 0) return SMH_OK;
    SMH_HIP(hipDeviceSynchronize());  // vectors work on the null stream; the caller's writes to a device array come first
    Scratch scr;
    const uint32_t *d_p = nullptr;
    uint32_t *inv = nullptr;
    SMH_TRY(take_permutation(scr, perm, n_perm, src->n, on_device, src->device, "perm", &d_p, &inv));
    SMH_TRY(launch_vec_permute(src->dtype, dst->d, src->d, d_p, src->n, inverse != 0, nullptr));
    SMH_HIP(hipStreamSynchronize(nullptr));
    return SMH_OK;
}

int smh_vec_permute(smh_vec *dst, const smh_vec *src, const uint32_t *perm, size_t n_perm, int inverse) {
    return vec_permute_common(dst, src, perm, n_perm, inverse, false);
}
int smh_vec_permute_dev(smh_vec *dst, const smh_vec *src, const uint32_t *perm_dev, size_t n_perm, int inverse) {
    return vec_permute_common(dst, src, perm_dev, n_perm, inverse, true);
}

int smh_crs_bandwidth(const smh_crs *m, uint32_t *lower_out, uint32_t *upper_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    uint32_t h[2] = {0, 0};
    if (m->n_rows && m->nnz) {
        SMH_HIP(hipStreamSynchronize(m->stream));
        Scratch scr;
        uint32_t *d = nullptr;
        SMH_TRY(scr.alloc(&d, 2));
        SMH_TRY(read_back(d, h, 2, m->stream, [&](uint32_t *q) { return launch_bandwidth(m->d_off, m->d_col, m->n_rows, q, m->stream); }));
    }
    if (lower_out) *lower_out = h[0];
    if (upper_out) *upper_out = h[1];
    return SMH_OK;
}

int smh_crs_span_fraction(smh_crs *m, double *out) {
    if (!m || !out) return fail(SMH_ERR_INVALID, "NULL argument");
    SMH_TRY(ensure_ring_plan(m, false));  // the locality statistic is taken with the K1r inspector
    *out = m->span_fraction;
    return SMH_OK;
}

static int rcm_common(const smh_crs *m, uint32_t *perm_out, size_t *n_components_out, size_t *n_levels_out, bool on_device) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (m->n_rows != m->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");
    if (m->n_rows && !perm_out) return fail(SMH_ERR_INVALID, "perm_out is NULL");
    SMH_TRY(columns_within_n_cols(m, "rcm"));
    if (on_device) {
        SMH_TRY(check_dev_array(perm_out, m->device, "perm_out"));
        SMH_HIP(hipDeviceSynchronize());
    }
    SMH_HIP(hipStreamSynchronize(m->stream));
    Scratch scr;
    uint32_t *d_perm = perm_out;
    if (!on_device) SMH_TRY(scr.alloc(&d_perm, m->n_rows));
    size_t comps = 0, levels = 0;
    SMH_TRY(rcm_order(m->d_off, m->d_col, m->n_rows, m->nnz, d_perm, &comps, &levels, m->stream));
    if (!on_device && m->n_rows) SMH_HIP(hipMemcpy(perm_out, d_perm, m->n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (n_components_out) *n_components_out = comps;
    if (n_levels_out) *n_levels_out = levels;
    return SMH_OK;
}

int smh_crs_rcm(const smh_crs *m, uint32_t *perm_out, size_t *n_components_out, size_t *n_levels_out) {
    return rcm_common(m, perm_out, n_components_out, n_levels_out, false);
}
int smh_crs_rcm_dev(const smh_crs *m, uint32_t *perm_out_dev, size_t *n_components_out, size_t *n_levels_out) {
    return rcm_common(m, perm_out_dev, n_components_out, n_levels_out, true);
}

static int color_common(const smh_crs *m, uint32_t seed, uint32_t *colors_out, uint32_t *perm_out, size_t *n_colors_out, size_t *n_rounds_out,
                        bool on_device) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (m->n_rows != m->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");
    SMH_TRY(columns_within_n_cols(m, "color"));
    const size_t n = m->n_rows;
    if (on_device) {
        if (colors_out) SMH_TRY(check_dev_array(colors_out, m->device, "colors_out"));
        if (perm_out) SMH_TRY(check_dev_array(perm_out, m->device, "perm_out"));
        SMH_HIP(hipDeviceSynchronize());
    }
    SMH_HIP(hipStreamSynchronize(m->stream));
    Scratch scr;
    uint32_t *d_colors = colors_out, *d_perm = perm_out;
    if (!on_device) {
        if (colors_out) SMH_TRY(scr.alloc(&d_colors, n));
        if (perm_out) SMH_TRY(scr.alloc(&d_perm, n));
    }
    size_t colors = 0, rounds = 0;
    SMH_TRY(color_order(m->d_off, m->d_col, n, m->nnz, seed, d_colors, d_perm, &colors, &rounds, m->stream));
    if (!on_device && n) {
        if (colors_out) SMH_HIP(hipMemcpy(colors_out, d_colors, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (perm_out) SMH_HIP(hipMemcpy(perm_out, d_perm, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (n_colors_out) *n_colors_out = colors;
    if (n_rounds_out) *n_rounds_out = rounds;
    return SMH_OK;
}

int smh_crs_color(const smh_crs *m, uint32_t seed, uint32_t *colors_out, uint32_t *perm_out, size_t *n_colors_out, size_t *n_rounds_out) {
    return color_common(m, seed, colors_out, perm_out, n_colors_out, n_rounds_out, false);
}
int smh_crs_color_dev(const smh_crs *m, uint32_t seed, uint32_t *colors_out_dev, uint32_t *perm_out_dev, size_t *n_colors_out, size_t *n_rounds_out) {
    return color_common(m, seed, colors_out_dev, perm_out_dev, n_colors_out, n_rounds_out, true);
}

// ---- #[derive(Clone)] (sparsemat_crs.rs:8) and SparseMatrix::add / sub (sparsematrix.rs:123-143, matadd.hip) ------------------
static thread_local int g_add_route = 2;
int smh_last_add_route(void) { return g_add_route; }

// in place: `a` takes the fresh handle's state, and every form derived from the old one (merge tiles, K1s codes and value
// dictionary, K1r plan, K2c / K2f / K2s / K2t copies, statistics) goes with the old state.  keep_arrays: the fresh handle
// works on the old handle's arrays (values updated where they are), so the old state must not free them.
// The swap takes whole structs: `a` stays the handle it was (its id), in a new structure epoch unless only the values changed.
static void replace_state(smh_crs *a, smh_crs *fresh, bool keep_arrays) {
    std::swap(*a, *fresh);
    a->id = fresh->id;
    a->epoch = fresh->epoch + (keep_arrays ? 0 : 1);
    if (keep_arrays) fresh->owns = false;
    (void)smh_crs_destroy(fresh);
}

int smh_crs_clone(const smh_crs *a, smh_crs **out) {
    if (!a || !out) return fail(SMH_ERR_INVALID, "NULL argument");
    *out = nullptr;
    SMH_HIP(hipStreamSynchronize(a->stream));
    const size_t vs = dtype_size(a->dtype);
    CrsArrays arrays;
    SMH_TRY(arrays.alloc(a->n_rows, a->nnz, vs));
    SMH_HIP(hipMemcpy(arrays.off, a->d_off, (a->n_rows + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    if (a->nnz) {
        SMH_HIP(hipMemcpy(arrays.col, a->d_col, a->nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice));
        SMH_HIP(hipMemcpy(arrays.val, a->d_val, a->nnz * vs, hipMemcpyDeviceToDevice));
    }
    SMH_TRY(wrap_arrays(a->dtype, a, a->n_rows, a->n_cols, a->nnz, arrays, 0, out));
    (*out)->orphans = a->orphans;
    (*out)->has_first_op = a->has_first_op;
    (*out)->first_row = a->first_row;
    (*out)->first_col = a->first_col;
    (*out)->first_val_bits = a->first_val_bits;
    return SMH_OK;
}

// a_mut != NULL: a += b in place (a_mut == a); else *out = a.clone() + b
static int add_common(smh_crs *a_mut, const smh_crs *a, const smh_crs *b, bool subtract, smh_crs **out) {
    if (!a || !b || (!a_mut && !out)) return fail(SMH_ERR_INVALID, "NULL argument");
    if (out) *out = nullptr;
    if (a->dtype != b->dtype) return fail(SMH_ERR_INVALID, "operands differ in value type");
    if (a->device != b->device) return fail(SMH_ERR_INVALID, "operands live on different devices");
    if (a->n_rows == 0 && a->orphans)
        return fail(SMH_ERR_INVALID, "add / sub: the left operand has no rows but an orphaned entry -- the reference's hidden offset_rows "
                                     "length decides whether it comes back to life, and the handle does not keep it");
    SMH_HIP(hipStreamSynchronize(b->stream));  // b's reads come after whatever b's stream still has to do
    SMH_HIP(hipStreamSynchronize(a->stream));
    g_add_route = 2;
    if (b->nnz == 0) {  // nothing visited: a unchanged (b's orphan is not reached by any row)
        if (a_mut) return SMH_OK;
        return smh_crs_clone(a, out);
    }
    smh_crs *fresh = nullptr;
    if (a->n_rows == 0) {
        // SparseMatCRS::new() (no offset_rows): the replay of b's entries as add_to operations, first-push quirk included
        g_add_route = 0;
        const size_t vs = dtype_size(a->dtype);
        Scratch scr;
        uint32_t *rows = nullptr;
        char *neg = nullptr;
        SMH_TRY(scr.alloc(&rows, b->nnz));
        SMH_TRY(expand_rows(b->d_off, b->n_rows, rows, nullptr));
        if (subtract) {  // 0 - v == 0 + (-v) in IEEE 754, signed zeros included
            SMH_TRY(scr.alloc(&neg, (b->nnz + 4) * vs));
            SMH_HIP(hipMemcpy(neg, b->d_val, b->nnz * vs, hipMemcpyDeviceToDevice));
            SMH_TRY(launch_scale_values(a->dtype, neg, b->nnz, -1.0, nullptr));
        }
        SMH_HIP(hipStreamSynchronize(nullptr));
        SMH_TRY(assemble_common((smh_dtype)a->dtype, b->nnz, rows, b->d_col, subtract ? (const void *)neg : b->d_val, nullptr, true, true, &fresh));
        if (fresh->n_cols < a->n_cols) fresh->n_cols = a->n_cols;  // push only raises n_cols (sparsemat_crs.rs:72-74)
        fresh->knobs = a->knobs;
        if (a_mut) replace_state(a_mut, fresh, false);
        else *out = fresh;
        return SMH_OK;
    }
    AddOperand oa, ob;
    oa.off = a->d_off; oa.col = a->d_col; oa.val = a->d_val;
    oa.n_rows = a->n_rows; oa.n_cols = a->n_cols; oa.nnz = a->nnz; oa.orphans = a->orphans;
    oa.max_row_len = a->max_row_len; oa.max_col = a->max_col;
    ob.off = b->d_off; ob.col = b->d_col; ob.val = b->d_val;
    ob.n_rows = b->n_rows; ob.n_cols = b->n_cols; ob.nnz = b->nnz; ob.orphans = b->orphans;
    ob.max_row_len = b->max_row_len; ob.max_col = b->max_col;
    const bool force_general = getenv("SMH_ADD_FAST") && atoi(getenv("SMH_ADD_FAST")) == 0;
    AddResult r;
    SMH_TRY(add_crs(a->dtype, subtract, oa, ob, a_mut != nullptr, a == b, force_general, &r, a->stream));
    g_add_route = r.route;
    if (r.values_only) {  // (borrowed by the fresh handle until it has been built: a failure must not free a's arrays)
        SMH_TRY(wrap_arrays(a->dtype, a, a->n_rows, a->n_cols, a->nnz, a->d_off, a->d_col, a->d_val, false, 0, &fresh));
        fresh->owns = a->owns;
    } else
        SMH_TRY(wrap_arrays(a->dtype, a, r.n_rows, r.n_cols, r.nnz, r.arrays, 0, &fresh));
    fresh->orphans = a->orphans;
    if (a_mut) replace_state(a_mut, fresh, r.values_only);
    else *out = fresh;
    return SMH_OK;
}

int smh_crs_add(const smh_crs *a, const smh_crs *b, smh_crs **out) { return add_common(nullptr, a, b, false, out); }
int smh_crs_sub(const smh_crs *a, const smh_crs *b, smh_crs **out) { return add_common(nullptr, a, b, true, out); }
int smh_crs_add_assign(smh_crs *a, const smh_crs *b) { return add_common(a, a, b, false, nullptr); }
int smh_crs_sub_assign(smh_crs *a, const smh_crs *b) { return add_common(a, a, b, true, nullptr); }

// ---- SparseMatrix::get / set / add_to / eye (sparsematrix.rs:91-98, 224-233; sparsemat_crs.rs:54-92, 136-150; matupdate.hip) ------
static thread_local int g_apply_route = 1;
int smh_last_apply_route(void) { return g_apply_route; }

// a device array of the caller must live on the handle's device (where the runtime can tell)
static int check_dev_array(const void *p, int device, const char *what) {
    if (!p) return SMH_OK;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return SMH_OK; }
    if (a.type == hipMemoryTypeDevice && a.device != device)
        return fail(SMH_ERR_INVALID, "%s lives on device %d, the handle on device %d", what, a.device, device);
    return SMH_OK;
}

static UpdMatrix upd_view(const smh_crs *m) {
    UpdMatrix u;
    u.off = m->d_off; u.col = m->d_col; u.val = m->d_val;
    u.n_rows = m->n_rows; u.n_cols = m->n_cols; u.nnz = m->nnz; u.orphans = m->orphans;
    u.max_row_len = m->max_row_len;
    return u;
}

static int get_many_common(const smh_crs *m, size_t n, const uint32_t *rows, const uint32_t *cols, void *values_out, bool on_device) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (n && (!rows || !cols || !values_out)) return fail(SMH_ERR_INVALID, "NULL query array");
    if (n == 0) return SMH_OK;
    const size_t vs = dtype_size(m->dtype);
    if (on_device) {
        SMH_TRY(check_dev_array(rows, m->device, "rows"));
        SMH_TRY(check_dev_array(cols, m->device, "cols"));
        SMH_TRY(check_dev_array(values_out, m->device, "values_out"));
        SMH_HIP(hipDeviceSynchronize());  // the caller's writes to the arrays come first
    }
    SMH_HIP(hipStreamSynchronize(m->stream));
    if (m->n_rows == 0) {  // find_index needs i < n_rows (sparsemat_crs.rs:54-67): every answer is zero
        if (on_device) SMH_HIP(hipMemset(values_out, 0, n * vs));
        else memset(values_out, 0, n * vs);
        return SMH_OK;
    }
    Scratch st;  // device copies of host query arrays
    const void *d_rows = rows, *d_cols = cols;
    void *d_out = values_out;
    if (!on_device) {
        SMH_TRY(upload(st, rows, n * sizeof(uint32_t), &d_rows));
        SMH_TRY(upload(st, cols, n * sizeof(uint32_t), &d_cols));
        char *out_dev = nullptr;
        SMH_TRY(st.alloc(&out_dev, n * vs));
        d_out = out_dev;
    }
    SMH_TRY(crs_get_many(m->dtype, upd_view(m), n, (const uint32_t *)d_rows, (const uint32_t *)d_cols, d_out, m->stream));
    if (!on_device) SMH_HIP(hipMemcpy(values_out, d_out, n * vs, hipMemcpyDeviceToHost));
    return SMH_OK;
}

int smh_crs_get(const smh_crs *m, size_t i, size_t j, void *value_out) {
    if (!m || !value_out) return fail(SMH_ERR_INVALID, "NULL argument");
    if (i >= m->n_rows || j > 0xFFFFFFFFull) {  // no row i, or a column no entry can have
        memset(value_out, 0, dtype_size(m->dtype));
        return SMH_OK;
    }
    const uint32_t r = (uint32_t)i, c = (uint32_t)j;
    return get_many_common(m, 1, &r, &c, value_out, false);
}
int smh_crs_get_many(const smh_crs *m, size_t n, const uint32_t *rows, const uint32_t *cols, void *values_out) {
    return get_many_common(m, n, rows, cols, values_out, false);
}
int smh_crs_get_many_dev(const smh_crs *m, size_t n, const uint32_t *rows_dev, const uint32_t *cols_dev, void *values_out_dev) {
    return get_many_common(m, n, rows_dev, cols_dev, values_out_dev, true);
}

static int apply_common(smh_crs *m, size_t n, const uint32_t *rows, const uint32_t *cols, const void *values, const uint8_t *ops, bool on_device) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (n && (!rows || !cols || !values)) return fail(SMH_ERR_INVALID, "NULL operation array");
    if (n >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "Maximum number of %u entries reached", 0xFFFFFFFFu);
    if (n == 0) {  // nothing applied: m untouched
        g_apply_route = 1;
        return SMH_OK;
    }
    if (m->n_rows == 0 && m->orphans && !m->has_first_op)
        return fail(SMH_ERR_INVALID, "apply: the handle has no rows but an orphaned entry whose operation it does not know");
    const size_t vs = dtype_size(m->dtype);
    if (on_device) {
        SMH_TRY(check_dev_array(rows, m->device, "rows"));
        SMH_TRY(check_dev_array(cols, m->device, "cols"));
        SMH_TRY(check_dev_array(values, m->device, "values"));
        SMH_TRY(check_dev_array(ops, m->device, "ops"));
        SMH_HIP(hipDeviceSynchronize());  // the caller's writes to the arrays come first
    }
    SMH_HIP(hipStreamSynchronize(m->stream));
    Scratch st;  // device copies of host operation arrays
    const void *d_rows = rows, *d_cols = cols, *d_vals = values, *d_ops = ops;
    if (!on_device) {
        SMH_TRY(upload(st, rows, n * sizeof(uint32_t), &d_rows));
        SMH_TRY(upload(st, cols, n * sizeof(uint32_t), &d_cols));
        SMH_TRY(upload(st, values, n * vs, &d_vals));
        SMH_TRY(upload(st, ops, n, &d_ops));
    }
    smh_crs *fresh = nullptr;
    if (m->n_rows == 0) {
        // SparseMatCRS::new(), or the state its first push leaves (sparsemat_crs.rs:75-76): the replay of (that push ++ the stream)
        g_apply_route = 2;
        if (!m->has_first_op) {
            SMH_TRY(assemble_common((smh_dtype)m->dtype, n, (const uint32_t *)d_rows, (const uint32_t *)d_cols, d_vals, (const uint8_t *)d_ops, true,
                                    true, &fresh));
        } else {
            Scratch cat;  // that push's operation ++ the stream
            uint32_t *c_rows = nullptr, *c_cols = nullptr;
            char *c_vals = nullptr;
            uint8_t *c_ops = nullptr;
            SMH_TRY(cat.alloc(&c_rows, n + 1));
            SMH_TRY(cat.alloc(&c_cols, n + 1));
            SMH_TRY(cat.alloc(&c_vals, (n + 1) * vs));
            SMH_TRY(cat.alloc(&c_ops, n + 1));
            const uint8_t set = 1;  // the recorded value is already folded: `set` it
            SMH_HIP(hipMemcpy(c_rows, &m->first_row, sizeof(uint32_t), hipMemcpyHostToDevice));
            SMH_HIP(hipMemcpy(c_cols, &m->first_col, sizeof(uint32_t), hipMemcpyHostToDevice));
            SMH_HIP(hipMemcpy(c_vals, &m->first_val_bits, vs, hipMemcpyHostToDevice));
            SMH_HIP(hipMemcpy(c_ops, &set, 1, hipMemcpyHostToDevice));
            SMH_HIP(hipMemcpy(c_rows + 1, d_rows, n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
            SMH_HIP(hipMemcpy(c_cols + 1, d_cols, n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
            SMH_HIP(hipMemcpy(c_vals + vs, d_vals, n * vs, hipMemcpyDeviceToDevice));
            if (d_ops) SMH_HIP(hipMemcpy(c_ops + 1, d_ops, n, hipMemcpyDeviceToDevice));
            else SMH_HIP(hipMemset(c_ops + 1, 0, n));
            SMH_TRY(assemble_common((smh_dtype)m->dtype, n + 1, c_rows, c_cols, c_vals, c_ops, true, true, &fresh));
        }
        if (fresh->n_cols < m->n_cols) fresh->n_cols = m->n_cols;  // push only raises n_cols (sparsemat_crs.rs:72-74)
        fresh->knobs = m->knobs;
        replace_state(m, fresh, false);
        return SMH_OK;
    }
    const bool force_general = getenv("SMH_APPLY_FAST") && atoi(getenv("SMH_APPLY_FAST")) == 0;
    UpdResult r;
    SMH_TRY(crs_apply(m->dtype, upd_view(m), n, (const uint32_t *)d_rows, (const uint32_t *)d_cols, d_vals, (const uint8_t *)d_ops, force_general, &r,
                      m->stream));
    g_apply_route = r.route;
    if (r.values_only)  // structure unchanged: every form derived from it stays, the value-derived ones are refreshed
        return smh_crs_update_values(m, nullptr);
    SMH_TRY(wrap_arrays(m->dtype, m, r.n_rows, r.n_cols, r.nnz, r.arrays, 0, &fresh));
    fresh->orphans = m->orphans;
    replace_state(m, fresh, false);
    return SMH_OK;
}

int smh_crs_apply(smh_crs *m, size_t n_ops, const uint32_t *rows, const uint32_t *cols, const void *values, const uint8_t *ops) {
    return apply_common(m, n_ops, rows, cols, values, ops, false);
}
int smh_crs_apply_dev(smh_crs *m, size_t n_ops, const uint32_t *rows_dev, const uint32_t *cols_dev, const void *values_dev, const uint8_t *ops_dev) {
    return apply_common(m, n_ops, rows_dev, cols_dev, values_dev, ops_dev, true);
}

// ---- a reusable update plan: re-assembly on a fixed pattern as one gather-and-fold pass (matplan.hip) ---------------------------
}  // extern "C"
struct smh_update_plan {
    uint64_t crs_id = 0, epoch = 0;  // the handle and the structure it was made for
    UpdPlan plan;
    StageBuf stage;  // the host form's upload of the values (lazy, reused)
};
extern "C" {

static int plan_create_common(const smh_crs *m, size_t n, const uint32_t *rows, const uint32_t *cols, const uint8_t *ops, bool on_device,
                              smh_update_plan **out) {
    if (!out) return fail(SMH_ERR_INVALID, "NULL out pointer");
    *out = nullptr;
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (n && (!rows || !cols)) return fail(SMH_ERR_INVALID, "NULL operation array");
    if (n >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "Maximum number of %u entries reached", 0xFFFFFFFFu);
    if (m->n_rows == 0) return fail(SMH_ERR_INVALID, "update plan: the handle has no rows, so no operation has an entry to land on");
    smh_update_plan *p = new (std::nothrow) smh_update_plan();
    if (!p) return fail(SMH_ERR_OOM, "host allocation failed");
    p->crs_id = m->id; p->epoch = m->epoch;
    const int rc = [&]() -> int {
        if (n == 0) return SMH_OK;  // a valid plan whose execute does nothing
        if (on_device) {
            SMH_TRY(check_dev_array(rows, m->device, "rows"));
            SMH_TRY(check_dev_array(cols, m->device, "cols"));
            SMH_TRY(check_dev_array(ops, m->device, "ops"));
            SMH_HIP(hipDeviceSynchronize());  // the caller's writes to the arrays come first
        }
        SMH_HIP(hipStreamSynchronize(m->stream));
        Scratch st;  // device copies of host operation arrays; the sorted operations
        const void *d_rows = rows, *d_cols = cols, *d_ops = ops;
        if (!on_device) {
            SMH_TRY(upload(st, rows, n * sizeof(uint32_t), &d_rows));
            SMH_TRY(upload(st, cols, n * sizeof(uint32_t), &d_cols));
            SMH_TRY(upload(st, ops, n, &d_ops));
        }
        uint32_t *key = nullptr, *src = nullptr;
        uint64_t n_absent = 0;
        SMH_TRY(st.alloc(&key, n));
        SMH_TRY(st.alloc(&src, n));
        SMH_TRY(crs_plan_targets(upd_view(m), n, (const uint32_t *)d_rows, (const uint32_t *)d_cols, key, src, &n_absent, m->stream));
        if (n_absent)
            return fail(SMH_ERR_INVALID, "update plan: %llu of %llu operations have no entry to land on (smh_crs_apply creates entries; plan afterwards)",
                        (unsigned long long)n_absent, (unsigned long long)n);
        return plan_build(n, key, src, (const uint8_t *)d_ops, &p->plan, m->stream);
    }();
    if (rc != SMH_OK) return keep_error(rc, [&] { delete p; });
    *out = p;
    return SMH_OK;
}

int smh_update_plan_create(const smh_crs *m, size_t n_ops, const uint32_t *rows, const uint32_t *cols, const uint8_t *ops, smh_update_plan **out) {
    return plan_create_common(m, n_ops, rows, cols, ops, false, out);
}
int smh_update_plan_create_dev(const smh_crs *m, size_t n_ops, const uint32_t *rows_dev, const uint32_t *cols_dev, const uint8_t *ops_dev,
                               smh_update_plan **out) {
    return plan_create_common(m, n_ops, rows_dev, cols_dev, ops_dev, true, out);
}

static int plan_execute_common(smh_update_plan *p, smh_crs *m, const void *values, int from_zero, bool on_device) {
    if (!p || !m) return fail(SMH_ERR_INVALID, "NULL argument");
    if (p->crs_id != m->id) return fail(SMH_ERR_INVALID, "update plan: made for another handle");
    if (p->epoch != m->epoch) return fail(SMH_ERR_INVALID, "update plan: the handle's structure changed since the plan was made");
    const size_t n = p->plan.n_ops;
    if (n && !values) return fail(SMH_ERR_INVALID, "NULL value array");
    if (n == 0) return SMH_OK;
    const void *d_vals = values;
    if (on_device) {
        SMH_TRY(check_dev_array(values, m->device, "values"));
        SMH_HIP(hipDeviceSynchronize());  // the caller's writes to the array come first
    } else {
        const size_t bytes = n * dtype_size(m->dtype);
        SMH_TRY(p->stage.ensure_cap(bytes));
        SMH_HIP(hipMemcpy(p->stage.d.get(), values, bytes, hipMemcpyHostToDevice));
        d_vals = p->stage.d.get();
    }
    SMH_HIP(hipStreamSynchronize(m->stream));
    SMH_TRY(plan_execute(m->dtype, p->plan, d_vals, m->d_val, from_zero != 0, m->stream));
    SMH_HIP(hipStreamSynchronize(m->stream));
    return smh_crs_update_values(m, nullptr);  // as apply's values-only route: structure-derived forms stay, value-derived ones follow
}

int smh_update_plan_execute(smh_update_plan *p, smh_crs *m, const void *values, int from_zero) {
    return plan_execute_common(p, m, values, from_zero, false);
}
int smh_update_plan_execute_dev(smh_update_plan *p, smh_crs *m, const void *values_dev, int from_zero) {
    return plan_execute_common(p, m, values_dev, from_zero, true);
}

int smh_update_plan_stats(const smh_update_plan *p, size_t *n_ops, size_t *n_targets, size_t *n_live_ops, size_t *longest_run,
                          size_t *long_run_threshold, size_t *device_bytes) {
    if (!p) return fail(SMH_ERR_INVALID, "NULL plan");
    if (n_ops) *n_ops = p->plan.n_ops;
    if (n_targets) *n_targets = p->plan.n_targets;
    if (n_live_ops) *n_live_ops = p->plan.n_live;
    if (longest_run) *longest_run = p->plan.longest_run;
    if (long_run_threshold) *long_run_threshold = kPlanLongRun;
    if (device_bytes) *device_bytes = p->plan.device_bytes;
    return SMH_OK;
}

int smh_update_plan_destroy(smh_update_plan *p) {
    delete p;
    return SMH_OK;
}

int smh_crs_eye(smh_dtype dtype, size_t dim, smh_crs **out) {
    if (!out) return fail(SMH_ERR_INVALID, "NULL out pointer");
    *out = nullptr;
    if (!valid_dtype(dtype)) return fail(SMH_ERR_INVALID, "dtype must be SMH_F32 or SMH_F64");
    if (dim >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "Maximum number of %u entries reached", 0xFFFFFFFFu);
    SMH_TRY(require_device());
    if (dim <= 1) {  // no rows (dim 0); the first push alone: no rows, one orphan, n_cols 1 (dim 1)
        const uint32_t zero = 0;
        const uint8_t set = 1;
        const double one64 = 1.0;
        const float one32 = 1.0f;
        return assemble_common(dtype, dim, &zero, &zero, dtype == SMH_F64 ? (const void *)&one64 : (const void *)&one32, &set, false, true, out);
    }
    CrsArrays arrays;
    SMH_TRY(arrays.alloc(dim, dim, dtype_size(dtype)));
    SMH_TRY(build_eye(dtype, dim, arrays.off, arrays.col, arrays.val, nullptr));
    return wrap_arrays(dtype, nullptr, dim, dim, dim, arrays, 0, out);
}

int smh_crs_is_symmetric(const smh_crs *m, int *out) {
    if (!m || !out) return fail(SMH_ERR_INVALID, "NULL argument");
    return crs_is_symmetric(m->dtype, m->d_off, m->d_col, m->d_val, m->n_rows, out, m->stream);
}

int smh_crs_is_sorted(const smh_crs *m, int *out) {
    if (!m || !out) return fail(SMH_ERR_INVALID, "NULL argument");
    return crs_is_sorted(m->d_off, m->d_col, m->n_rows, out, m->stream);
}

int smh_crs_sort_rows(smh_crs *m) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(sort_rows(m->dtype, m->d_off, m->d_col, m->d_val, m->n_rows, m->nnz, m->max_col, m->stream));
    invalidate(m, Changed::Order);
    ++m->epoch;  // storage order changed: an update plan's targets are stale
    return SMH_OK;
}

int smh_crs_destroy(smh_crs *m) {
    if (!m) return SMH_OK;
    if (m->stream) { (void)hipStreamSynchronize(m->stream); (void)hipStreamDestroy(m->stream); }
    if (m->owns) { (void)hipFree(m->d_off); (void)hipFree(m->d_col); (void)hipFree(m->d_val); }
    (void)hipGetLastError();
    delete m;
    return SMH_OK;
}

int smh_crs_update_values(smh_crs *m, const void *values_host) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL argument");
    if (m->nnz && values_host) SMH_HIP(hipMemcpy(m->d_val, values_host, m->nnz * dtype_size(m->dtype), hipMemcpyHostToDevice));
    invalidate(m, Changed::Values);
    // the value dictionary of K1s XD-V described the OLD values: look again now (one pass over the values: nothing beside the copy above)
    // and take the indices out of the codes, or put the new ones in
    if (m->codes.state != Form::NotTried && m->codes.direct) {
        StreamCfg c;
        SMH_TRY(stream_cfg(m, &c, true));
    }
    return SMH_OK;
}

int smh_crs_download(const smh_crs *m, uint32_t *offset_rows, uint32_t *columns, void *values) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_HIP(hipStreamSynchronize(m->stream));
    if (offset_rows) SMH_HIP(hipMemcpy(offset_rows, m->d_off, (m->n_rows + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (columns && m->nnz) SMH_HIP(hipMemcpy(columns, m->d_col, m->nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (values && m->nnz) SMH_HIP(hipMemcpy(values, m->d_val, m->nnz * dtype_size(m->dtype), hipMemcpyDeviceToHost));
    return SMH_OK;
}

size_t smh_crs_n_rows(const smh_crs *m) { return m ? m->n_rows : 0; }
size_t smh_crs_n_cols(const smh_crs *m) { return m ? m->n_cols : 0; }
size_t smh_crs_nnz(const smh_crs *m) { return m ? m->nnz : 0; }
size_t smh_crs_orphans(const smh_crs *m) { return m ? m->orphans : 0; }
int smh_crs_dtype(const smh_crs *m) { return m ? m->dtype : -1; }

int smh_crs_max_row_len(const smh_crs *m, uint32_t *out) {
    if (!m || !out) return fail(SMH_ERR_INVALID, "NULL argument");
    *out = m->max_row_len;
    return SMH_OK;
}

int smh_crs_col_range(const smh_crs *m, uint32_t *min_out, uint32_t *max_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (min_out) *min_out = m->min_col;
    if (max_out) *max_out = m->max_col;
    return SMH_OK;
}

int smh_crs_scale(smh_crs *m, double a) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(launch_scale_values(m->dtype, m->d_val, m->nnz, a, m->stream));
    if (m->has_first_op) {
        // the reference scales every stored value (sparsemat_crs.rs:153-157), the orphaned first push included, and smh_crs_apply
        // brings that value back: scale the kept copy by the same kernel, so that it rounds exactly as a stored value does
        Scratch scr;
        char *d = nullptr;
        SMH_TRY(scr.alloc(&d, 16));
        SMH_HIP(hipMemcpyAsync(d, &m->first_val_bits, 8, hipMemcpyHostToDevice, m->stream));
        SMH_TRY(launch_scale_values(m->dtype, d, 1, a, m->stream));
        SMH_HIP(hipMemcpyAsync(&m->first_val_bits, d, 8, hipMemcpyDeviceToHost, m->stream));
        SMH_HIP(hipStreamSynchronize(m->stream));
    }
    // (K1s XD-V: every entry is its dictionary value times a, rounded as the entry itself is: the indices in the codes stay right)
    if (m->dict.state == Form::Ready) SMH_TRY(launch_scale_values(m->dtype, m->dict.values.get(), 32, a, m->stream));
    ring_values_changed(m);  // (K1r's chunk records hold the old values: the next product tests the scaled ones)
    if (m->cb.state == Form::Ready) SMH_TRY(launch_scale_values(m->dtype, m->cb.val.get(), m->nnz, a, m->stream));
    if (m->cf.state == Form::Ready) SMH_TRY(launch_scale_values(m->dtype, m->cf.val.get(), m->nnz, a, m->stream));
    if (m->tiled.state == Form::Ready) SMH_TRY(launch_scale_values(m->dtype, m->tiled.val.get(), (size_t)m->tiled.tot, a, m->stream));
    if (m->split.state == Form::Ready) {
        SMH_TRY(smh_crs_scale(m->split.long_part, a));
        SMH_TRY(smh_crs_scale(m->split.short_part, a));
    }
    SMH_HIP(hipStreamSynchronize(m->stream));
    return SMH_OK;
}

int smh_crs_tiled_layout(smh_crs *m, uint32_t *n_slices_out, uint32_t *slice_columns_out, uint32_t *rows_per_block_out, uint32_t *n_row_blocks_out,
                         size_t *copy_entries_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(tiled_build(m));
    if (n_slices_out) *n_slices_out = m->tiled.n_cb;
    if (slice_columns_out) *slice_columns_out = tiled_slice_columns(m->dtype);
    if (rows_per_block_out) *rows_per_block_out = m->tiled.R;
    if (n_row_blocks_out) *n_row_blocks_out = m->tiled.n_rb;
    if (copy_entries_out) *copy_entries_out = (size_t)m->tiled.tot;
    return SMH_OK;
}

int smh_crs_tiled_products(smh_crs *m, size_t *n_products_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(tiled_build(m));
    if (n_products_out) *n_products_out = (size_t)m->tiled.n_prod;
    return SMH_OK;
}

int smh_crs_tiled_array(smh_crs *m, int which, void *out, size_t capacity_bytes, size_t *bytes_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(tiled_build(m));
    return tiled_array(m, which, out, capacity_bytes, bytes_out);
}

int smh_crs_set_colblock_shift(smh_crs *m, uint32_t shift) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (shift > 31) return fail(SMH_ERR_INVALID, "column block shift must be 0 (automatic) or 1..31");
    if (shift != m->knobs.cb_forced_shift) invalidate(m, Changed::BlockWidth);
    m->knobs.cb_forced_shift = shift;
    return SMH_OK;
}

int smh_crs_colblock(smh_crs *m, uint32_t *shift_out, size_t *n_blocks_out, int *rows_per_thread_out,
                     double *span_fraction_out, uint32_t *offsets_out, uint32_t *columns_out, void *values_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(ensure_ring_plan(m, false));  // the locality statistic
    SMH_TRY(ensure_colblock(m));
    if (shift_out) *shift_out = m->cb.shift;
    if (n_blocks_out) *n_blocks_out = m->cb.blocks;
    if (rows_per_thread_out) *rows_per_thread_out = m->cb.rpt;
    if (span_fraction_out) *span_fraction_out = m->span_fraction;
    if (offsets_out)
        SMH_HIP(hipMemcpy(offsets_out, m->cb.off.get(), m->cb.blocks * (m->n_rows + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (columns_out && m->nnz) SMH_HIP(hipMemcpy(columns_out, m->cb.col.get(), m->nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (values_out && m->nnz) SMH_HIP(hipMemcpy(values_out, m->cb.val.get(), m->nnz * dtype_size(m->dtype), hipMemcpyDeviceToHost));
    return SMH_OK;
}

int smh_crs_colfused(smh_crs *m, int *fits_out, uint32_t *shift_out, size_t *n_blocks_out, uint32_t *rows_per_lane_out,
                     size_t *n_tiles_out, uint32_t *tile_rows_out, uint32_t *segments_out, uint8_t *counts_out, uint32_t *columns_out,
                     void *values_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(ensure_colfused(m));
    const size_t tile_rows = (size_t)64 * m->cf.rt, n_tiles = (m->cf.state == Form::Ready) ? m->cf.tiles : 0;
    if (fits_out) *fits_out = (m->cf.state == Form::Ready) ? 1 : 0;
    if (shift_out) *shift_out = m->cf.shift;
    if (n_blocks_out) *n_blocks_out = m->cf.blocks;
    if (rows_per_lane_out) *rows_per_lane_out = m->cf.rt;
    if (n_tiles_out) *n_tiles_out = n_tiles;
    if (m->cf.state != Form::Ready) return SMH_OK;
    SMH_HIP(hipStreamSynchronize(m->stream));
    if (tile_rows_out) SMH_HIP(hipMemcpy(tile_rows_out, m->cf.tile_row.get(), (n_tiles + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (segments_out) SMH_HIP(hipMemcpy(segments_out, m->cf.seg.get(), (n_tiles * m->cf.blocks + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (counts_out && n_tiles) SMH_HIP(hipMemcpy(counts_out, m->cf.cnt.get(), n_tiles * m->cf.blocks * tile_rows, hipMemcpyDeviceToHost));
    if (columns_out && m->nnz) SMH_HIP(hipMemcpy(columns_out, m->cf.col.get(), m->nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (values_out && m->nnz) SMH_HIP(hipMemcpy(values_out, m->cf.val.get(), m->nnz * dtype_size(m->dtype), hipMemcpyDeviceToHost));
    return SMH_OK;
}

int smh_crs_colsplit(smh_crs *m, int *split_out, uint32_t *min_long_out, size_t *n_long_out, uint32_t *long_rows_out, smh_crs **long_out,
                     smh_crs **short_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(ensure_split(m));
    const bool split = m->split.state == Form::Ready;
    if (split_out) *split_out = split ? 1 : 0;
    if (min_long_out) *min_long_out = kSplitMinLong;
    if (n_long_out) *n_long_out = split ? m->split.n_long : 0;
    if (long_out) *long_out = split ? m->split.long_part : nullptr;
    if (short_out) *short_out = split ? m->split.short_part : nullptr;
    if (long_rows_out && split && m->split.n_long)
        SMH_HIP(hipMemcpy(long_rows_out, m->split.rows.get(), m->split.n_long * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SMH_OK;
}

int smh_crs_resolved_variant(const smh_crs *m, int *variant_out, int *lanes_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (variant_out) *variant_out = resolve_variant(m, SMH_SPMV_AUTO);
    if (lanes_out) *lanes_out = auto_lanes(m);
    return SMH_OK;
}

int smh_crs_set_stream_xs(smh_crs *m, int mode) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (mode < -1 || mode > 1) return fail(SMH_ERR_INVALID, "mode must be -1 (automatic), 0 (never) or 1 (whenever the tiles allow)");
    m->knobs.use_stream_xs = mode;
    return recode_stream(m);
}

int smh_crs_set_stream_direct(smh_crs *m, int mode) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (mode < -1 || mode > 1) return fail(SMH_ERR_INVALID, "mode must be -1 (automatic), 0 (never) or 1 (whenever x is staged)");
    m->knobs.use_stream_direct = mode;
    return recode_stream(m);
}

int smh_crs_stream_direct(smh_crs *m, int *direct_out) {
    if (!m || !direct_out) return fail(SMH_ERR_INVALID, "NULL argument");
    StreamCfg c;
    SMH_TRY(stream_cfg(m, &c));
    *direct_out = c.direct && c.xs != 0;
    return SMH_OK;
}

int smh_crs_stream_value_dict(smh_crs *m, int *n_values_out, void *values_out) {
    if (!m || !n_values_out) return fail(SMH_ERR_INVALID, "NULL argument");
    StreamCfg c;
    SMH_TRY(stream_cfg(m, &c));
    *n_values_out = c.dict ? (int)m->dict.n : 0;
    if (c.dict && values_out) {
        SMH_HIP(hipMemcpyAsync(values_out, m->dict.values.get(), (size_t)m->dict.n * dtype_size(m->dtype), hipMemcpyDeviceToHost, m->stream));
        SMH_HIP(hipStreamSynchronize(m->stream));
    }
    return SMH_OK;
}

int smh_crs_set_stream_value_dict(smh_crs *m, int mode) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (mode < -1 || mode > 0) return fail(SMH_ERR_INVALID, "mode must be -1 (automatic: whenever the values allow) or 0 (never)");
    m->knobs.use_stream_vdict = mode;
    return recode_stream(m);
}

int smh_crs_stream_layout(smh_crs *m, int *coded_out, int *byte_lengths_out, int *small_tiles_out, int *xs_chunks_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    StreamCfg c;
    SMH_TRY(stream_cfg(m, &c));
    if (coded_out) *coded_out = c.code && c.cwin;
    if (byte_lengths_out) *byte_lengths_out = c.len8 && c.tbase;
    if (small_tiles_out) *small_tiles_out = c.small;
    if (xs_chunks_out) *xs_chunks_out = c.xs;
    return SMH_OK;
}

int smh_crs_set_vector_chunks(smh_crs *m, int chunks) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (chunks < 0 || chunks > 3) return fail(SMH_ERR_INVALID, "chunks per lane must be 0 (automatic), 1, 2 or 3");
    m->knobs.forced_chunks = chunks;
    return SMH_OK;
}

int smh_crs_set_ring(smh_crs *m, int mode) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (mode < -1 || mode > 1) return fail(SMH_ERR_INVALID, "ring mode must be -1 (auto), 0 (plain K1) or 1 (K1r)");
    m->knobs.use_ring = mode;
    return SMH_OK;
}

int smh_crs_ring_plan(smh_crs *m, uint32_t *n_blocks_out, size_t *n_phases_out, double *ring_fraction_out,
                      int *active_out, uint32_t *phase_ptr_out, uint32_t *phases_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(ensure_ring_plan(m));
    bool ring = false;
    SMH_TRY(vector_uses_ring(m, &ring));
    if (n_blocks_out) *n_blocks_out = m->ring.blocks;
    if (n_phases_out) *n_phases_out = m->ring.n_phases;
    if (ring_fraction_out) *ring_fraction_out = m->ring.fraction;
    if (active_out) *active_out = ring ? 1 : 0;
    if (phase_ptr_out)
        SMH_HIP(hipMemcpy(phase_ptr_out, m->ring.phase_ptr.get(), (m->ring.blocks + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (phases_out && m->ring.n_phases)
        SMH_HIP(hipMemcpy(phases_out, m->ring.phases.get(), m->ring.n_phases * sizeof(RingPhase), hipMemcpyDeviceToHost));
    return SMH_OK;
}

int smh_crs_ring_regular(smh_crs *m, uint32_t *len_out) {
    if (!m || !len_out) return fail(SMH_ERR_INVALID, "NULL argument");
    SMH_TRY(ensure_ring_plan(m));
    if (m->ring.n_phases)
        SMH_HIP(hipMemcpy(len_out, m->ring.reg_len.get(), m->ring.n_phases * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SMH_OK;
}

int smh_crs_ring_column_form(smh_crs *m, int *form_out) {
    if (!m || !form_out) return fail(SMH_ERR_INVALID, "NULL argument");
    bool ring = false;
    SMH_TRY(vector_uses_ring(m, &ring));
    *form_out = !ring ? 0 : (m->ring.lo8.get() || m->ring.rec16.get()) ? 2 : m->ring.col16.get() ? 1 : 0;
    return SMH_OK;
}

int smh_crs_ring_values(smh_crs *m, int *form_out, int *exponent_out) {
    if (!m || !form_out) return fail(SMH_ERR_INVALID, "NULL argument");
    bool ring = false;
    SMH_TRY(vector_uses_ring(m, &ring));
    const bool rec = ring && m->ring.rec16.get();
    *form_out = rec ? 1 : (ring && m->ring.v24 == Form::Refused) ? -1 : 0;
    if (exponent_out) *exponent_out = rec ? m->ring.v24_exp : 0;
    return SMH_OK;
}

int smh_crs_ring_entries(smh_crs *m, uint32_t *out) {
    if (!m || !out) return fail(SMH_ERR_INVALID, "NULL argument");
    SMH_TRY(ensure_ring_plan(m));
    *out = m->ring.entries;
    return SMH_OK;
}

int smh_crs_ring_bands(smh_crs *m, uint32_t *bands_out, uint32_t *intervals_out) {
    if (!m || !bands_out) return fail(SMH_ERR_INVALID, "NULL argument");
    SMH_TRY(ensure_ring_plan(m));
    *bands_out = m->ring.bands;
    if (intervals_out && m->ring.bands == 4 && m->ring.win.get())
        SMH_HIP(hipMemcpy(intervals_out, m->ring.win.get(), ((m->n_rows + 63) / 64) * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SMH_OK;
}

int smh_crs_set_vector_lanes(smh_crs *m, int lanes) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (lanes != 0 && (lanes < 1 || lanes > 64 || (lanes & (lanes - 1))))
        return fail(SMH_ERR_INVALID, "lanes per row must be 0 or a power of two in 1..64");
    m->knobs.forced_lanes = lanes;
    return SMH_OK;
}

int smh_crs_prepare(smh_crs *m, int variant) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    // what the inspectors cost (smh_crs_prepare_stats): wall time of the build, device-synchronised at both ends, and the
    // device memory it leaves allocated (pooled blocks: everything of 1 MiB and more; scratch freed inside the build nets out)
    const auto t0 = std::chrono::steady_clock::now();
    const long long b0 = pool_thread_net_bytes();
    // (AUTO's plan refused by its lazy build: resolved again, as often as the first product would)
    int rc = prepare_forms(m, variant);
    if (rc == SMH_OK && m->stream) {
        const hipError_t e = hipStreamSynchronize(m->stream);
        if (e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
    }
    m->prepare_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    m->prepare_bytes += pool_thread_net_bytes() - b0;
    return rc;
}

int smh_crs_prepare_stats(smh_crs *m, int variant, double *prepare_ms_out, size_t *derived_bytes_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(smh_crs_prepare(m, variant));
    if (prepare_ms_out) *prepare_ms_out = m->create_ms + m->prepare_ms;
    if (derived_bytes_out) *derived_bytes_out = (size_t)(m->prepare_bytes + m->create_bytes > 0 ? m->prepare_bytes + m->create_bytes : 0);
    return SMH_OK;
}

int smh_crs_spmv_dev(smh_crs *m, const void *x_dev, size_t x_len, void *y_dev, int variant, void *stream) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (m->n_rows && (!y_dev || (m->nnz && !x_dev))) return fail(SMH_ERR_INVALID, "NULL device vector");
    return spmv_enqueue(m, x_dev, x_len, y_dev, variant, (hipStream_t)stream);
}

int smh_crs_spmv(smh_crs *m, const void *x_host, size_t x_len, void *y_host, int variant) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (m->n_rows == 0) return SMH_OK;
    if (!y_host || (x_len && !x_host)) return fail(SMH_ERR_INVALID, "NULL host vector");
    const size_t vs = dtype_size(m->dtype);
    SMH_TRY(m->stage_x.ensure_cap(x_len * vs));
    SMH_TRY(m->stage_y.ensure_cap(m->n_rows * vs));
    if (x_len) SMH_HIP(hipMemcpyAsync(m->stage_x.d.get(), x_host, x_len * vs, hipMemcpyHostToDevice, m->stream));
    SMH_TRY(spmv_enqueue(m, m->stage_x.d.get(), x_len, m->stage_y.d.get(), variant, m->stream));
    SMH_HIP(hipMemcpyAsync(y_host, m->stage_y.d.get(), m->n_rows * vs, hipMemcpyDeviceToHost, m->stream));
    SMH_HIP(hipStreamSynchronize(m->stream));
    return SMH_OK;
}

size_t smh_crs_merge_tiles(const smh_crs *m) {
    if (!m) return 0;
    return (size_t)(((uint64_t)m->n_rows + m->nnz + kMergeTile - 1) / kMergeTile);
}

size_t smh_crs_merge_tile_items(const smh_crs *) { return kMergeTile; }

int smh_crs_merge_table(smh_crs *m, uint32_t *row_out, uint32_t *nnz_out) {
    if (!m || !row_out || !nnz_out) return fail(SMH_ERR_INVALID, "NULL argument");
    SMH_TRY(ensure_merge_ws(m));
    if (m->merge.n_tiles == 0) { row_out[0] = 0; nnz_out[0] = 0; return SMH_OK; }
    SMH_HIP(hipMemcpy(row_out, m->merge.tile_row.get(), (m->merge.n_tiles + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    SMH_HIP(hipMemcpy(nnz_out, m->merge.tile_nz.get(), (m->merge.n_tiles + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SMH_OK;
}

// ---- DenseVec ----------------------------------------------------------------------------------------
int smh_vec_create(smh_dtype dtype, size_t n, smh_vec **out) {
    if (!out) return fail(SMH_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid_dtype(dtype)) return fail(SMH_ERR_INVALID, "dtype must be SMH_F32 or SMH_F64");
    SMH_TRY(require_device());
    smh_vec *v = new (std::nothrow) smh_vec();
    if (!v) return fail(SMH_ERR_OOM, "host allocation failed");
    v->dtype = dtype; v->n = n; v->owns = true; v->device = current_device();
    const size_t bytes = (n ? n : 1) * dtype_size(dtype);
    hipError_t e = hipMalloc(&v->d, bytes);
    if (e == hipSuccess) e = hipMemset(v->d, 0, bytes);
    if (e != hipSuccess) { delete v; return hip_fail(e, "smh_vec_create", __FILE__, __LINE__); }
    *out = v;
    return SMH_OK;
}

int smh_vec_from_host(smh_dtype dtype, size_t n, const void *host, smh_vec **out) {
    SMH_TRY(smh_vec_create(dtype, n, out));
    if (n) {
        int rc = smh_vec_upload(*out, host);
        if (rc != SMH_OK) { smh_vec_destroy(*out); *out = nullptr; return rc; }
    }
    return SMH_OK;
}

int smh_vec_wrap_dev(smh_dtype dtype, size_t n, void *dev_ptr, smh_vec **out) {
    if (!out) return fail(SMH_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid_dtype(dtype)) return fail(SMH_ERR_INVALID, "dtype must be SMH_F32 or SMH_F64");
    if (n && !dev_ptr) return fail(SMH_ERR_INVALID, "dev_ptr is NULL");
    SMH_TRY(require_device());
    smh_vec *v = new (std::nothrow) smh_vec();
    if (!v) return fail(SMH_ERR_OOM, "host allocation failed");
    v->dtype = dtype; v->n = n; v->d = dev_ptr; v->owns = false; v->device = current_device();
    *out = v;
    return SMH_OK;
}

int smh_vec_destroy(smh_vec *v) {
    if (!v) return SMH_OK;
    if (v->owns) { (void)hipFree(v->d); (void)hipGetLastError(); }
    delete v;
    return SMH_OK;
}

int smh_vec_upload(smh_vec *v, const void *host) {
    if (!v || (v->n && !host)) return fail(SMH_ERR_INVALID, "NULL argument");
    if (v->n) SMH_HIP(hipMemcpy(v->d, host, v->n * dtype_size(v->dtype), hipMemcpyHostToDevice));
    return SMH_OK;
}

int smh_vec_download(const smh_vec *v, void *host) {
    if (!v || (v->n && !host)) return fail(SMH_ERR_INVALID, "NULL argument");
    if (v->n) SMH_HIP(hipMemcpy(host, v->d, v->n * dtype_size(v->dtype), hipMemcpyDeviceToHost));
    return SMH_OK;
}

size_t smh_vec_dim(const smh_vec *v) { return v ? v->n : 0; }
int smh_vec_dtype(const smh_vec *v) { return v ? v->dtype : -1; }
void *smh_vec_data(const smh_vec *v) { return v ? v->d : nullptr; }

int smh_vec_copy(smh_vec *dst, const smh_vec *src) {
    SMH_TRY(vec_check_pair(dst, src));
    if (dst->n != src->n) return fail(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
    if (src->n) SMH_HIP(hipMemcpy(dst->d, src->d, src->n * dtype_size(src->dtype), hipMemcpyDeviceToDevice));
    return SMH_OK;
}

static int vec_ew(Ew op, smh_vec *x, const smh_vec *y, double a, const char *what) {
    SMH_TRY(vec_check_pair(x, y));
    // densevec.rs:52-54 / :61-63: panic iff self.dim() < rhs.dim(); zip() covers rhs.dim() entries
    if (x->n < y->n) return fail(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
    SMH_TRY(ew_check_overlap(x->d, y->d, y->n, x->dtype, what));  // (the same storage, x.add(x), is legal: every thread its own entry)
    SMH_TRY(launch_ew(x->dtype, op, x->d, y->d, y->n, a, nullptr, nullptr));
    SMH_HIP(hipStreamSynchronize(nullptr));
    return SMH_OK;
}

int smh_vec_add(smh_vec *x, const smh_vec *y) { return vec_ew(Ew::Add, x, y, 0.0, "smh_vec_add"); }
int smh_vec_sub(smh_vec *x, const smh_vec *y) { return vec_ew(Ew::Sub, x, y, 0.0, "smh_vec_sub"); }
int smh_vec_axpy(smh_vec *y, double a, const smh_vec *x) { return vec_ew(Ew::Axpy, y, x, a, "smh_vec_axpy"); }
int smh_vec_xpby(smh_vec *p, double b, const smh_vec *r) { return vec_ew(Ew::Xpby, p, r, b, "smh_vec_xpby"); }

int smh_vec_scale(smh_vec *x, double a) {
    if (!x) return fail(SMH_ERR_INVALID, "NULL vector handle");
    SMH_TRY(launch_ew(x->dtype, Ew::Scale, x->d, nullptr, x->n, a, nullptr, nullptr));
    SMH_HIP(hipStreamSynchronize(nullptr));
    return SMH_OK;
}

int smh_vec_dot(const smh_vec *x, const smh_vec *y, double *out) {
    SMH_TRY(vec_check_pair(x, y));
    if (!out) return fail(SMH_ERR_INVALID, "out is NULL");
    const size_t n = x->n < y->n ? x->n : y->n;  // zip truncates (vector.rs:52)
    void *scratch = nullptr;
    SMH_TRY(reduce_scratch(&scratch));
    char *res = (char *)scratch + kReducePartials * sizeof(double);
    SMH_TRY(launch_dot(x->dtype, x->d, y->d, n, scratch, res, nullptr));
    if (x->dtype == SMH_F64) {
        double h = 0;
        SMH_HIP(hipMemcpy(&h, res, sizeof h, hipMemcpyDeviceToHost));
        *out = h;
    } else {
        float h = 0;
        SMH_HIP(hipMemcpy(&h, res, sizeof h, hipMemcpyDeviceToHost));
        *out = (double)h;
    }
    return SMH_OK;
}

// lhs^T (A rhs) on device vectors, by one of three routes (spmv_inner_prod, spmv_dispatch.hip):
//   K1r   the ring kernel's DOT form: the lane that would store a row's sum adds fma(lhs[row], sum, .) to its own accumulator, a
//         workgroup folds lanes and waves, one partial per workgroup and one for an unpadded array's last <= 3 entries, launch_fold2
//   K1s   the CSR-stream kernels' dot epilogue with y == NULL: round(lhs[row] * sum) per thread, one partial per tile, launch_fold2
//   else  y = A rhs by the matrix's own kernel into the handle's y staging, then launch_dot(lhs, y) over the rows that hold entries
// sparsematrix.rs:161-171 sums lhs_i * a_ij * rhs_j over all entries in storage order; each route regroups that sum in a fixed
// order of its own, so against the reference parity is tolerance-level, like dot -- and against the CPU model of its order
// (tests/inner_prod_model.py) each route is bit for bit (tests/test_inner_prod_bits_gpu.py).  A row without entries is no term in
// any of them, as in the reference, whatever lhs holds there.
static int inner_prod_dev(smh_crs *m, const void *d_lhs, size_t lhs_len, const void *d_rhs, size_t rhs_len, int variant,
                          double *out) {
    if (!out) return fail(SMH_ERR_INVALID, "out is NULL");
    *out = 0.0;
    if (m->n_rows == 0 || m->nnz == 0) return SMH_OK;
    const size_t vs = dtype_size(m->dtype);
    // lhs.get(i) is evaluated inside the entry loop (sparsematrix.rs:165-168): only rows that hold entries index lhs, so a
    // short lhs is an error only if it ends before the last non-empty row (densevec.rs:41 panics there).  The kernels read
    // lhs for every row, so a short-but-legal lhs is continued with zeros in a scratch copy.
    Scratch scr;
    if (lhs_len < m->n_rows) {
        size_t lo = 0, hi = m->n_rows;  // smallest i with offset_rows[i] == nnz; rows i.. are empty
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            uint32_t off = 0;
            SMH_HIP(hipMemcpyAsync(&off, m->d_off + mid, sizeof off, hipMemcpyDeviceToHost, m->stream));
            SMH_HIP(hipStreamSynchronize(m->stream));
            if ((size_t)off >= m->nnz) hi = mid; else lo = mid + 1;
        }
        if (lhs_len < lo)  // row lo - 1 is the last one with entries
            return fail(SMH_ERR_INDEX_RANGE, "index out of bounds: the len is %zu but the index is %zu", lhs_len, lo - 1);
        char *padded = nullptr;
        SMH_TRY(scr.alloc(&padded, m->n_rows * vs));
        SMH_HIP(hipMemsetAsync(padded, 0, m->n_rows * vs, m->stream));
        if (lhs_len) SMH_HIP(hipMemcpyAsync(padded, d_lhs, lhs_len * vs, hipMemcpyDeviceToDevice, m->stream));
        d_lhs = padded;
    }
    void *scratch = nullptr;
    SMH_TRY(reduce_scratch(&scratch));
    char *res = (char *)scratch + kReducePartials * sizeof(double);
    SMH_TRY(spmv_inner_prod(m, d_lhs, d_rhs, rhs_len, variant, scratch, res));
    double h64 = 0;
    float h32 = 0;
    if (m->dtype == SMH_F64) SMH_HIP(hipMemcpyAsync(&h64, res, sizeof h64, hipMemcpyDeviceToHost, m->stream));
    else SMH_HIP(hipMemcpyAsync(&h32, res, sizeof h32, hipMemcpyDeviceToHost, m->stream));
    SMH_HIP(hipStreamSynchronize(m->stream));
    *out = m->dtype == SMH_F64 ? h64 : (double)h32;
    return SMH_OK;
}

int smh_crs_inner_prod_vec(smh_crs *m, const smh_vec *lhs, const smh_vec *rhs, int variant, double *out) {
    if (!m || !lhs || !rhs) return fail(SMH_ERR_INVALID, "NULL handle");
    if (lhs->dtype != m->dtype || rhs->dtype != m->dtype) return fail(SMH_ERR_INVALID, "value types differ");
    SMH_HIP(hipDeviceSynchronize());  // vectors may have pending work on other streams
    return inner_prod_dev(m, lhs->d, lhs->n, rhs->d, rhs->n, variant, out);
}

int smh_crs_inner_prod(smh_crs *m, const void *lhs_host, size_t lhs_len, const void *rhs_host, size_t rhs_len, int variant,
                       double *out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if ((lhs_len && !lhs_host) || (rhs_len && !rhs_host)) return fail(SMH_ERR_INVALID, "NULL host vector");
    const size_t vs = dtype_size(m->dtype);
    // rhs goes to the x staging; lhs to a scratch allocation of its own
    SMH_TRY(m->stage_x.ensure_cap(rhs_len * vs));
    Scratch scr;
    char *d_lhs = nullptr;
    SMH_TRY(scr.alloc(&d_lhs, (lhs_len ? lhs_len : 1) * vs));
    if (rhs_len) SMH_HIP(hipMemcpyAsync(m->stage_x.d.get(), rhs_host, rhs_len * vs, hipMemcpyHostToDevice, m->stream));
    if (lhs_len) SMH_HIP(hipMemcpyAsync(d_lhs, lhs_host, lhs_len * vs, hipMemcpyHostToDevice, m->stream));
    return inner_prod_dev(m, d_lhs, lhs_len, m->stage_x.d.get(), rhs_len, variant, out);
}

int smh_vec_norm_squared(const smh_vec *x, double *out) { return smh_vec_dot(x, x, out); }

int smh_vec_norm(const smh_vec *x, double *out) {
    SMH_TRY(smh_vec_norm_squared(x, out));
    *out = std::sqrt(*out);  // f64::sqrt(self.norm_squared().into())  vector.rs:61-63
    return SMH_OK;
}

// ---- BLAS-1 on raw device pointers with DEVICE-resident scalars (asynchronous) ------------------------
// Building blocks of a solver whose scalars never visit the host (the multi-GPU CG all-reduces them on
// the device between these calls).
int smh_blas_dot_dev(smh_dtype dtype, const void *x_dev, const void *y_dev, size_t n, void *result_dev,
                     void *scratch_dev, void *stream) {
    if (!valid_dtype(dtype)) return fail(SMH_ERR_INVALID, "dtype must be SMH_F32 or SMH_F64");
    if (!result_dev || !scratch_dev || (n && (!x_dev || !y_dev))) return fail(SMH_ERR_INVALID, "NULL device pointer");
    return launch_dot(dtype, x_dev, y_dev, n, scratch_dev, result_dev, (hipStream_t)stream);
}

size_t smh_blas_dot_scratch_bytes(void) { return (size_t)(kReducePartials + 8) * sizeof(double); }

int smh_blas_axpy_dev(smh_dtype dtype, void *y_dev, const void *a_dev, const void *x_dev, size_t n, void *stream) {
    if (!valid_dtype(dtype)) return fail(SMH_ERR_INVALID, "dtype must be SMH_F32 or SMH_F64");
    if (!a_dev || (n && (!x_dev || !y_dev))) return fail(SMH_ERR_INVALID, "NULL device pointer");
    SMH_TRY(ew_check_overlap(y_dev, x_dev, n, dtype, "smh_blas_axpy_dev"));
    return launch_ew(dtype, Ew::Axpy, y_dev, x_dev, n, 0.0, a_dev, (hipStream_t)stream);
}

int smh_blas_xpby_dev(smh_dtype dtype, void *p_dev, const void *b_dev, const void *r_dev, size_t n, void *stream) {
    if (!valid_dtype(dtype)) return fail(SMH_ERR_INVALID, "dtype must be SMH_F32 or SMH_F64");
    if (!b_dev || (n && (!p_dev || !r_dev))) return fail(SMH_ERR_INVALID, "NULL device pointer");
    SMH_TRY(ew_check_overlap(p_dev, r_dev, n, dtype, "smh_blas_xpby_dev"));
    return launch_ew(dtype, Ew::Xpby, p_dev, r_dev, n, 0.0, b_dev, (hipStream_t)stream);
}

int smh_crs_spmv_vec(smh_crs *m, const smh_vec *x, smh_vec *y, int variant) {
    if (!m || !x || !y) return fail(SMH_ERR_INVALID, "NULL handle");
    if (x->dtype != m->dtype || y->dtype != m->dtype) return fail(SMH_ERR_INVALID, "dtype mismatch");
    if (y->n != m->n_rows) return fail(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
    SMH_TRY(spmv_enqueue(m, x->d, x->n, y->d, variant, m->stream));
    SMH_HIP(hipStreamSynchronize(m->stream));
    return SMH_OK;
}

// ---- ConjugateGradient ---------------------------------------------------------------------------------
// The statuses are decided by check_solve_vec / check_solve_host (solver_host.hpp), before any launch.  check_every = 0 stands for
// 4 bodies per poll here (8 in the preconditioned solvers and BiCGSTAB).
constexpr size_t kCgCheckEvery = 4;

int smh_cg_solve_vec(smh_crs *m, const smh_vec *b, smh_vec *x, double tol, size_t iter_max, int variant,
                     size_t check_every, size_t *iters_out, double *rr_out) {
    SMH_TRY(check_solve_vec(m, b, x, "dtype mismatch", /*refuse_aliased*/ false, &check_every, kCgCheckEvery));
    return cg_solve(m, b, x, tol, iter_max, variant, check_every, iters_out, rr_out);
}

int smh_cg_solve(smh_crs *m, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len, double tol,
                 size_t iter_max, int variant, size_t *iters_out, double *rr_out) {
    SMH_TRY(check_solve_host(m, b_host, b_len, x_host_inout, x_len, /*null_vectors*/ false, /*refuse_aliased*/ false));
    smh_vec *b = nullptr, *x = nullptr;
    int rc = smh_vec_from_host((smh_dtype)m->dtype, b_len, b_host, &b);
    if (rc == SMH_OK) rc = smh_vec_from_host((smh_dtype)m->dtype, x_len, x_host_inout, &x);
    if (rc == SMH_OK) rc = smh_cg_solve_vec(m, b, x, tol, iter_max, variant, 0, iters_out, rr_out);
    if (rc == SMH_OK) rc = smh_vec_download(x, x_host_inout);
    smh_vec_destroy(b);
    smh_vec_destroy(x);
    return rc;
}

// ... on k right-hand sides at once (K5m, cg_many.hip)
int smh_cg_solve_many(smh_crs *m, const smh_mvec *b, smh_mvec *x, double tol, size_t iter_max, size_t check_every, size_t *iters_out,
                      double *rr_out) {
    if (!m || !b || !x) return fail(SMH_ERR_INVALID, "NULL handle");
    if (!iters_out || !rr_out) return fail(SMH_ERR_INVALID, "NULL output array");
    SMH_TRY(check_solve_vec(m, b, x, "multi-vector dtype differs from the matrix's", /*refuse_aliased*/ true, &check_every, kCgCheckEvery));
    return cg_solve_many(m, b, x, tol, iter_max, check_every, iters_out, rr_out);
}

int smh_cg_solve_many_host(smh_crs *m, const void *b_host, size_t n, size_t k, void *x_host_inout, double tol, size_t iter_max,
                           size_t *iters_out, double *rr_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (!iters_out || !rr_out) return fail(SMH_ERR_INVALID, "NULL output array");
    SMH_TRY(check_solve_host(m, b_host, n, x_host_inout, n, /*null_vectors*/ true, /*refuse_aliased*/ false));
    smh_mvec *b = nullptr, *x = nullptr;
    int rc = smh_mvec_from_host((smh_dtype)m->dtype, n, k, b_host, &b);
    if (rc == SMH_OK) rc = smh_mvec_from_host((smh_dtype)m->dtype, n, k, x_host_inout, &x);
    if (rc == SMH_OK) rc = smh_cg_solve_many(m, b, x, tol, iter_max, 0, iters_out, rr_out);
    if (rc == SMH_OK && n) rc = smh_mvec_download(x, x_host_inout);
    smh_mvec_destroy(b);
    smh_mvec_destroy(x);
    return rc;
}

// ---- synthetic workloads ---------------------------------------------------------------------------------
int smh_synth_x(smh_dtype dtype, uint64_t seed, size_t begin, size_t n, void *x_dev, void *stream) {
    SMH_TRY(require_device());
    return synth_x(dtype, seed, begin, n, x_dev, (hipStream_t)stream);
}

int smh_synth_fixed(smh_dtype dtype, uint64_t seed, int pattern, size_t n, uint32_t k, size_t row_begin,
                    size_t row_end, uint32_t *offset_rows_dev, uint32_t *columns_dev, void *values_dev, void *stream) {
    SMH_TRY(require_device());
    if (k == 0 || n < k || row_end < row_begin || row_end > n) return fail(SMH_ERR_INVALID, "bad generator arguments");
    if ((uint64_t)(row_end - row_begin) * k >= 0xFFFFFFFFull)
        return fail(SMH_ERR_CAPACITY, "Maximum number of %u entries reached", 0xFFFFFFFFu);  // sparsemat_crs.rs:82-84
    return synth_fixed(dtype, seed, pattern, n, k, row_begin, row_end, offset_rows_dev, columns_dev, values_dev,
                       (hipStream_t)stream);
}

int smh_synth_powerlaw_cdf(uint32_t kmax, double alpha, uint32_t *cdf_host) {
    if (!cdf_host || kmax == 0) return fail(SMH_ERR_INVALID, "bad arguments");
    synth_powerlaw_cdf(kmax, alpha, cdf_host);
    return SMH_OK;
}

int smh_synth_powerlaw_lengths(uint64_t seed, size_t row_begin, size_t row_end, uint32_t kmax, const uint32_t *cdf_host,
                               uint32_t *lengths_host) {
    if (!cdf_host || !lengths_host || kmax == 0) return fail(SMH_ERR_INVALID, "bad arguments");
    synth_powerlaw_lengths(seed, row_begin, row_end, kmax, cdf_host, lengths_host);
    return SMH_OK;
}

int smh_synth_fill(smh_dtype dtype, uint64_t seed, size_t n_cols, size_t row_begin, size_t row_end,
                   const uint32_t *offset_rows_dev, uint32_t *columns_dev, void *values_dev, void *stream) {
    SMH_TRY(require_device());
    if (n_cols == 0) return fail(SMH_ERR_INVALID, "n_cols == 0");
    return synth_fill(dtype, seed, n_cols, row_begin, row_end, offset_rows_dev, columns_dev, values_dev,
                      (hipStream_t)stream);
}

int smh_synth_laplace3d(smh_dtype dtype, size_t nx, size_t ny, size_t nz, size_t row_begin, size_t row_end,
                        uint32_t *offset_rows_dev, uint32_t *columns_dev, void *values_dev, size_t *nnz_out,
                        void *stream) {
    if (row_end < row_begin || row_end > nx * ny * nz) return fail(SMH_ERR_INVALID, "bad row range");
    const size_t nnz = synth_laplace3d_nnz(nx, ny, nz, row_begin, row_end);
    if (nnz_out) *nnz_out = nnz;
    if (!offset_rows_dev && !columns_dev && !values_dev) return SMH_OK;  // size query only (no device needed)
    if (nnz >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "block nnz exceeds u32");
    SMH_TRY(require_device());
    return synth_laplace3d(dtype, nx, ny, nz, row_begin, row_end, offset_rows_dev, columns_dev, values_dev,
                           (hipStream_t)stream);
}

// ---- raw device memory helpers -----------------------------------------------------------------------------
int smh_dev_alloc(size_t bytes, void **out) {
    if (!out) return fail(SMH_ERR_INVALID, "out is NULL");
    SMH_TRY(require_device());
    SMH_HIP(hipMalloc(out, bytes ? bytes : 1));
    return SMH_OK;
}
int smh_dev_free(void *p) {
    if (p) SMH_HIP(hipFree(p));
    return SMH_OK;
}
int smh_dev_upload(void *dst_dev, const void *src_host, size_t bytes) {
    if (bytes) SMH_HIP(hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice));
    return SMH_OK;
}
int smh_dev_download(void *dst_host, const void *src_dev, size_t bytes) {
    if (bytes) SMH_HIP(hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
    return SMH_OK;
}
int smh_dev_memset(void *dst_dev, int value, size_t bytes, void *stream) {
    if (bytes) SMH_HIP(hipMemsetAsync(dst_dev, value, bytes, (hipStream_t)stream));
    return SMH_OK;
}

// ---- streams and timing events for hosts without a HIP binding (bench.py: HIP events around every launch) ----
int smh_stream_create(void **stream_out) {
    if (!stream_out) return fail(SMH_ERR_INVALID, "stream_out is NULL");
    SMH_TRY(require_device());
    hipStream_t s = nullptr;
    SMH_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream_out = s;
    return SMH_OK;
}
int smh_stream_destroy(void *stream) {
    if (stream) SMH_HIP(hipStreamDestroy((hipStream_t)stream));
    return SMH_OK;
}
int smh_stream_synchronize(void *stream) {
    SMH_HIP(hipStreamSynchronize((hipStream_t)stream));
    return SMH_OK;
}
int smh_event_create(void **event_out) {
    if (!event_out) return fail(SMH_ERR_INVALID, "event_out is NULL");
    SMH_TRY(require_device());
    hipEvent_t e = nullptr;
    SMH_HIP(hipEventCreate(&e));
    *event_out = e;
    return SMH_OK;
}
int smh_event_destroy(void *event) {
    if (event) SMH_HIP(hipEventDestroy((hipEvent_t)event));
    return SMH_OK;
}
int smh_event_record(void *event, void *stream) {
    SMH_HIP(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
    return SMH_OK;
}
int smh_event_elapsed_ms(void *start, void *stop, float *ms_out) {
    if (!ms_out) return fail(SMH_ERR_INVALID, "ms_out is NULL");
    SMH_HIP(hipEventSynchronize((hipEvent_t)stop));
    SMH_HIP(hipEventElapsedTime(ms_out, (hipEvent_t)start, (hipEvent_t)stop));
    return SMH_OK;
}

}  // extern "C"
