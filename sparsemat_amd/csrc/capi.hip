// capi.hip -- the core of the extern "C" boundary of libsparsemat_hip.so (see include/sparsemat_hip.h): what belongs to no feature.
//
// The error channel, the thread and capture counting, the life cycle of a CRS handle (create, the create-time inspection, destroy,
// download, update_values, scale, sort_rows and the size getters) and of a DenseVec, raw device memory, streams and events.  Every
// other entry point lives with its feature's device code ("where an entry point lives").  What a handle derives is built
// in crs_forms.hip; which kernel a product runs and its launches are spmv_dispatch.hip's.  No CPU compute path exists: every entry
// point that computes needs a HIP device.
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstring>
#include <new>
#include <thread>

#include "crs_forms.hpp"

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
int wrap_arrays(int dtype, const smh_crs *like, size_t n_rows, size_t n_cols, size_t nnz, uint32_t *off, uint32_t *col, void *val,
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

int vec_check_pair(const smh_vec *x, const smh_vec *y) {
    if (!x || !y) return fail(SMH_ERR_INVALID, "NULL vector handle");
    if (x->dtype != y->dtype) return fail(SMH_ERR_INVALID, "vector dtype mismatch");
    return SMH_OK;
}

// in place: `a` takes the fresh handle's state, and every form derived from the old one (merge tiles, K1s codes and value
// dictionary, K1r plan, K2c / K2f / K2s / K2t copies, statistics) goes with the old state.  keep_arrays: the fresh handle
// works on the old handle's arrays (values updated where they are), so the old state must not free them.
// The swap takes whole structs: `a` stays the handle it was (its id), in a new structure epoch unless only the values changed.
void replace_state(smh_crs *a, smh_crs *fresh, bool keep_arrays) {
    std::swap(*a, *fresh);
    a->id = fresh->id;
    a->epoch = fresh->epoch + (keep_arrays ? 0 : 1);
    if (keep_arrays) fresh->owns = false;
    (void)smh_crs_destroy(fresh);
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

// ---- DenseVec: the life cycle (the arithmetic is blas1.hip's, the permutation permute.hip's) -------------
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
