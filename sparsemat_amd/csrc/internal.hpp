// internal.hpp -- shared declarations of libsparsemat_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sparsemat_hip.h"

namespace smh {

// ---- error plumbing: never throw across the C ABI --------------------------------------
void set_error(const char *fmt, ...);
int fail(int status, const char *fmt, ...);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

// ---- host threads and graph capture -------------------------------------------------------------------------------------
// The solvers capture a batch of bodies in hipStreamCaptureModeThreadLocal on the handle's non-blocking stream.  On ROCm 7.2 that
// does not keep other host threads out of the way: while ANY thread captures, a synchronous call on the legacy stream (hipMemcpy,
// hipMemset) or hipDeviceSynchronize from another thread is refused (hipErrorStreamCaptureImplicit / Unsupported) and invalidates
// the capture.  So a batch is captured only while one host thread is using the library: every thread is counted before its first
// call into the runtime that could disturb a capture -- in SMH_HIP, in require_device(), in the hipMalloc / hipFree of this library
// (the macros at the end of this file: a pooled free synchronises the device) and in smh_pool_trim -- and waits there, once, for a
// capture in progress to end (a capture only records launches on the host).  A thread that has ended is counted no longer, and with
// more than one thread counted capture_enter() says no: the bodies are then launched one by one, which gives the same bits
// (solve_in_batches).  The count is coarse: a thread that made one call stays counted until it ends, and from then on no solve of
// the process replays a graph; smh_last_solve_replays() tells a caller which of the two its last solve did.
extern __thread bool t_thread_counted;
extern __thread int t_solve_replays;  // graph launches of this thread's last solve_in_batches (smh_last_solve_replays)
void count_thread();      // capi.hip
inline void note_thread() { if (!t_thread_counted) count_thread(); }
bool capture_enter();     // true: the calling thread may capture now; then capture_leave() once the capture has ended
void capture_leave();

#define SMH_HIP(call)                                                     \
    do {                                                                  \
        ::smh::note_thread();                                             \
        hipError_t e__ = (call);                                          \
        if (e__ != hipSuccess) return ::smh::hip_fail(e__, #call, __FILE__, __LINE__); \
    } while (0)

#define SMH_TRY(expr)                 \
    do {                              \
        int rc__ = (expr);            \
        if (rc__ != SMH_OK) return rc__; \
    } while (0)

int require_device();  // SMH_ERR_NO_DEVICE when no HIP device is visible
int current_device();

// cleanup() (destroying a handle, a par or a comm, a teardown) without losing the error text that goes with status rc; returns rc
template <typename F> int keep_error(int rc, F &&cleanup) {
    char keep[512];
    strncpy(keep, smh_last_error(), sizeof keep);
    keep[sizeof keep - 1] = 0;
    cleanup();
    set_error("%s", keep);
    return rc;
}

inline size_t dtype_size(int dt) { return dt == SMH_F64 ? 8 : 4; }

// ---- device memory goes through the caching layer of pool.hip (see there for why) ---------------------------------------
hipError_t pool_malloc(void **out, size_t bytes);
hipError_t pool_free(void *p);
long long pool_thread_net_bytes();  // pooled bytes this thread has allocated minus freed so far (differences measure a build)

// Device scratch of a host-side driver: any number of allocations, freed when the owner goes out of scope.  (The owners call the
// pool directly, as the hipMalloc / hipFree macros at the end of this file do: pool.hip sees the same definitions.)
class Scratch {
  public:
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { for (void *q : p_) (void)pool_free(q); }
    // (count ? count : 1) elements of U
    template <typename U> int alloc(U **out, size_t count) {
        SMH_HIP(pool_malloc((void **)out, (count ? count : 1) * sizeof(U)));
        return adopt(*out);
    }
    int adopt(void *q) {  // frees q with the rest
        try {
            p_.push_back(q);
        } catch (...) {
            (void)pool_free(q);
            return fail(SMH_ERR_OOM, "host allocation failed");
        }
        return SMH_OK;
    }
    void free_now(const void *q) {  // early free
        if (!q) return;
        for (void *&x : p_)
            if (x == q) { (void)pool_free(x); x = nullptr; }
    }
    template <typename U> U *release(U *q) {  // hands q over to the caller
        for (void *&x : p_)
            if (x == q) x = nullptr;
        return q;
    }

  private:
    std::vector<void *> p_;
};

// The arrays of a new CRS matrix, padded like smh_crs_create's: off [n_rows + 1], col / val [nnz + 4].  Freed when the owner goes
// out of scope unless they were handed over (release; a handle takes them in capi.hip's wrap_arrays).
struct CrsArrays {
    uint32_t *off = nullptr, *col = nullptr;
    void *val = nullptr;
    CrsArrays() = default;
    CrsArrays(const CrsArrays &) = delete;
    CrsArrays &operator=(const CrsArrays &) = delete;
    CrsArrays(CrsArrays &&o) noexcept { o.release(&off, &col, &val); }
    CrsArrays &operator=(CrsArrays &&o) noexcept {
        if (this != &o) {
            free_all();
            o.release(&off, &col, &val);
        }
        return *this;
    }
    ~CrsArrays() { free_all(); }
    int alloc_off(size_t n_rows) {
        SMH_HIP(pool_malloc((void **)&off, (n_rows + 1) * sizeof(uint32_t)));
        return SMH_OK;
    }
    int alloc_entries(size_t nnz, size_t value_bytes) {
        SMH_HIP(pool_malloc((void **)&col, (nnz + 4) * sizeof(uint32_t)));
        SMH_HIP(pool_malloc(&val, (nnz + 4) * value_bytes));
        return SMH_OK;
    }
    int alloc(size_t n_rows, size_t nnz, size_t value_bytes) {
        SMH_TRY(alloc_off(n_rows));
        return alloc_entries(nnz, value_bytes);
    }
    int zero_padding(size_t nnz, size_t value_bytes, hipStream_t s) {  // the 4 entries past nnz
        SMH_HIP(hipMemsetAsync(col + nnz, 0, 4 * sizeof(uint32_t), s));
        SMH_HIP(hipMemsetAsync((char *)val + nnz * value_bytes, 0, 4 * value_bytes, s));
        return SMH_OK;
    }
    template <typename V> void release(uint32_t **off_out, uint32_t **col_out, V **val_out) {  // hands the arrays over to the caller
        *off_out = off; *col_out = col; *val_out = (V *)val;
        off = col = nullptr;
        val = nullptr;
    }

  private:
    void free_all() {
        (void)pool_free(off); (void)pool_free(col); (void)pool_free(val);
        off = col = nullptr;
        val = nullptr;
    }
};

// One device array of T (char: sized in bytes), freed when the owner goes out of scope or takes another; null after a move.
template <typename T> class DevArray {
  public:
    DevArray() = default;
    DevArray(const DevArray &) = delete;
    DevArray &operator=(const DevArray &) = delete;
    DevArray(DevArray &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevArray &operator=(DevArray &&o) noexcept {
        if (this != &o) {
            reset(o.p_);
            o.p_ = nullptr;
        }
        return *this;
    }
    ~DevArray() { reset(); }
    int alloc(size_t count) {  // exactly count elements
        reset();
        SMH_HIP(pool_malloc((void **)&p_, count * sizeof(T)));
        return SMH_OK;
    }
    T *get() const { return p_; }
    void reset(T *q = nullptr) {  // frees the array; q (optional, a pool allocation) is owned from here on
        (void)pool_free(p_);
        p_ = q;
    }

  private:
    T *p_ = nullptr;
};

// A stream (non-blocking), an event (untimed) and pinned host memory: empty until create / alloc succeeds, released when the owner goes out of
// scope or is assigned another (whose owner takes, and releases when it goes, what this one held).  Nothing synchronises a stream before it goes.
struct Stream {
    Stream() = default;
    Stream(Stream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream &operator=(Stream &&o) noexcept { std::swap(s_, o.s_); return *this; }
    ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
    int create() {
        *this = Stream();
        SMH_HIP(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
        return SMH_OK;
    }
    hipStream_t get() const { return s_; }

  private:
    hipStream_t s_ = nullptr;
};
struct Event {
    Event() = default;
    Event(Event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event &operator=(Event &&o) noexcept { std::swap(e_, o.e_); return *this; }
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    int create() {
        *this = Event();
        SMH_HIP(hipEventCreateWithFlags(&e_, hipEventDisableTiming));
        return SMH_OK;
    }
    hipEvent_t get() const { return e_; }

  private:
    hipEvent_t e_ = nullptr;
};
struct PinnedBuf {
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { std::swap(p_, o.p_); return *this; }
    ~PinnedBuf() { if (p_) (void)hipHostFree(p_); }
    int alloc(size_t bytes, unsigned flags) {  // flags: hipHostMalloc's
        *this = PinnedBuf();
        SMH_HIP(hipHostMalloc(&p_, bytes, flags));
        return SMH_OK;
    }
    void *get() const { return p_; }

  private:
    void *p_ = nullptr;
};
// A captured graph and its executable form: empty until end_capture / instantiate succeeds (a failure leaves the owner empty and is
// the caller's to handle: the solvers fall back to plain launches).  Nothing waits for a launched graph before its executable goes.
struct Graph {
    Graph() = default;
    Graph(Graph &&o) noexcept : g_(o.g_) { o.g_ = nullptr; }
    Graph &operator=(Graph &&o) noexcept { std::swap(g_, o.g_); return *this; }
    ~Graph() { if (g_) (void)hipGraphDestroy(g_); }
    hipError_t end_capture(hipStream_t s) {  // ends the capture that hipStreamBeginCapture began on s
        *this = Graph();
        hipGraph_t g = nullptr;
        const hipError_t rc = hipStreamEndCapture(s, &g);
        if (rc == hipSuccess) g_ = g;
        return rc;
    }
    hipGraph_t get() const { return g_; }

  private:
    hipGraph_t g_ = nullptr;
};
struct GraphExec {
    GraphExec() = default;
    GraphExec(GraphExec &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    GraphExec &operator=(GraphExec &&o) noexcept { std::swap(e_, o.e_); return *this; }
    ~GraphExec() { if (e_) (void)hipGraphExecDestroy(e_); }
    hipError_t instantiate(hipGraph_t g) {
        *this = GraphExec();
        hipGraphExec_t e = nullptr;
        const hipError_t rc = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
        if (rc == hipSuccess) e_ = e;
        return rc;
    }
    hipGraphExec_t get() const { return e_; }

  private:
    hipGraphExec_t e_ = nullptr;
};

// rocPRIM's two-phase calls: `call` names `tmp` and `bytes`; it is run once to size the temporary storage (bytes ? bytes : 16),
// then on it; stream s is synchronised before the storage is freed
#define SMH_ROCPRIM(s, call)                                           \
    do {                                                               \
        size_t bytes = 0;                                              \
        void *tmp = nullptr;                                           \
        SMH_HIP(call);                                                 \
        SMH_HIP(::smh::pool_malloc(&tmp, bytes ? bytes : 16));         \
        const hipError_t e1 = (call);                                  \
        const hipError_t e2 = hipStreamSynchronize(s);                 \
        (void)::smh::pool_free(tmp);                                   \
        SMH_HIP(e1);                                                   \
        SMH_HIP(e2);                                                   \
    } while (0)

constexpr int kWave = 64;           // gfx950 wavefront
constexpr int kBlock = 256;         // 4 waves: one per SIMD
// The sum of a value over the wavefront by DPP (row_shr 1, 2, 4, 8, row_bcast 15, 31: an inclusive scan; lane 63 ends with the total)
// -- six vector instructions in a fixed order, where the __shfl_down butterfly is a chain of six ds_bpermute round trips through
// the LDS at the very end of a workgroup's life.  Lanes without a source add +0.
template <int CTRL, int ROWS> __device__ __forceinline__ float wave_dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROWS, 0xF, false));
}
template <int CTRL, int ROWS> __device__ __forceinline__ double wave_dpp_add(double v) {
    const long long b = __double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, ROWS, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)((unsigned long long)b >> 32), CTRL, ROWS, 0xF, false);
    return v + __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
template <typename T> __device__ __forceinline__ T wave_sum_to_lane63(T v) {
    v = wave_dpp_add<0x111, 0xF>(v);
    v = wave_dpp_add<0x112, 0xF>(v);
    v = wave_dpp_add<0x114, 0xF>(v);
    v = wave_dpp_add<0x118, 0xF>(v);
    v = wave_dpp_add<0x142, 0xA>(v);
    v = wave_dpp_add<0x143, 0xC>(v);
    return v;
}
// the largest value over the wavefront, in every lane
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = (uint32_t)__shfl_xor((int)v, o, kWave);
        v = w > v ? w : v;
    }
    return v;
}
// blocks of kBlock threads for n items of a grid-stride launch: at least one, at most cap (kBuildGrid: the cap of most build steps)
constexpr uint64_t kBuildGrid = 16384;
inline unsigned grid_for(uint64_t n, uint64_t cap) {
    const uint64_t b = (n + kBlock - 1) / kBlock;
    return (unsigned)(b == 0 ? 1 : b > cap ? cap : b);
}
inline unsigned bits_for(uint64_t v) {  // bits needed to hold v (radix sort key width)
    unsigned b = 1;
    while (b < 64 && (v >> b)) ++b;
    return b;
}
constexpr int kMergeItemsPerThread = 8;
constexpr int kMergeTile = kBlock * kMergeItemsPerThread;  // merge items (rows + nnz) per tile
constexpr int kReducePartials = 1024;  // blocks of a stage-1 reduction
constexpr int kRingEntries = 16384;    // K1r: columns of x the LDS ring holds (64 KiB f32 / 128 KiB f64)
constexpr int kRingEntriesWide = 32768;  // ... f32 only, for rows that need it: 128 KiB, one 1024-thread block per CU
constexpr int kStreamRows = kBlock;    // K1s: rows per tile (one thread folds one row)
constexpr int kStreamCap = 4096;       // K1s: entries of a tile staged in LDS
constexpr int kStreamCapSmall = 2045;  // K1s: ... when no tile holds more (two 16-byte chunks per thread from an aligned start)
constexpr int kStreamCodeWidth = 16384;  // K1s 16-bit column codes: columns per interval (14 bits) x 4 intervals
constexpr int kManyCap = 2048;         // K1m: entries of a pass, per plane of the LDS product stage (KT = 8 on f64: half of it)

// ---- launchers (defined in the .hip files) ---------------------------------------------
// in-place exclusive scan of n u32 on the device; *total_out (optional) = their sum (spmv_colblock.hip)
int device_exclusive_scan_u32(uint32_t *data, uint64_t n, hipStream_t s, uint64_t *total_out);
// K1 / SEQ
int launch_spmv_vector(int dtype, int lanes, const uint32_t *off, const uint32_t *col, const void *val,
                       const void *x, void *y, size_t n_rows, size_t nnz, hipStream_t s);
int launch_spmv_seq(int dtype, const uint32_t *off, const uint32_t *col, const void *val, const void *x,
                    void *y, size_t n_rows, hipStream_t s);
// K2
int launch_merge_table(const uint32_t *off, size_t n_rows, size_t nnz, size_t n_tiles, uint32_t *tile_row,
                       uint32_t *tile_nz, hipStream_t s);
int launch_spmv_merge(int dtype, const uint32_t *off, const uint32_t *col, const void *val, const void *x,
                      void *y, size_t n_rows, size_t nnz, size_t n_tiles, const uint32_t *tile_row,
                      const uint32_t *tile_nz, uint32_t *carry_row, void *carry_val, hipStream_t s);
// K1s (CSR-stream for short rows)
int launch_spmv_stream(int dtype, const uint32_t *off, const uint32_t *col, const void *val, const void *x, void *y,
                       size_t n_rows, size_t nnz, bool padded, int rows_per_thread,
                       bool single_pass /* no tile holds more than kStreamCap entries */,
                       void *dot_partials /* optional: x.y per tile, stream_tiles() entries */,
                       const uint16_t *code, const uint32_t *cwin /* optional: 16-bit column codes + their interval table */,
                       const uint8_t *len8, const uint32_t *tbase /* optional (with codes): byte row lengths + tile starts */,
                       const void *dot_lhs /* with dot_partials: the vector dotted with y (NULL: x); y may then be NULL */,
                       hipStream_t s, bool small_tiles = false /* no tile holds more than kStreamCapSmall entries */,
                       int xs = 0 /* ... and the tiles' column intervals fit an LDS stage of x of xs * 1024 entries (2 or 4; stream_xs_* checked by the caller) */,
                       uint64_t tile_begin = 0, uint64_t tile_end = ~uint64_t(0) /* the matrix's tiles [begin, end) only (default: all) */);
int launch_stream_xs_stats(const uint32_t *win, size_t n_tiles, uint32_t *d_out2, hipStream_t s);
int launch_stream_len8(const uint32_t *off, size_t n_rows, uint8_t *len8, uint32_t *tbase, hipStream_t s);
size_t stream_tiles(size_t n_rows, int rows_per_thread);
int launch_stream_windows(const uint32_t *off, const uint32_t *col, size_t n_rows, uint32_t *win,
                          uint32_t *d_count, hipStream_t s);
int launch_stream_codes(const uint32_t *off, const uint32_t *col, const uint32_t *win, size_t n_rows, uint16_t *code,
                        hipStream_t s);
// K1m (spmv_many.hip): Y = A X on interleaved multi-vectors (element i of vector c at [i * ld + c]; ld a multiple of 4, 16-byte aligned
// pointers, x != y: checked by the caller, mvec.hip); ceil(ld / KT) sweeps, columns at and beyond k are stored as +0
int launch_spmv_many(int dtype, const uint32_t *off, const uint32_t *col, const void *val, const void *x, void *y, size_t n_rows, size_t nnz,
                     bool padded, size_t k, size_t ld, hipStream_t s);
// K1s XD (spmv_stream_xd.hip): the code array as byte offsets into the tile's LDS stage of x, an unskewed product stage
int launch_spmv_stream_xd(int dtype, const void *val, const void *x, void *y, size_t n_rows, void *dot_partials, const uint16_t *scode,
                          const uint32_t *cwin, const uint8_t *len8, const uint32_t *tbase, const void *dot_lhs, hipStream_t s, int xs,
                          uint64_t tile_begin = 0, uint64_t tile_end = ~uint64_t(0), const void *dict = nullptr /* K1s XD-V: value dictionary */,
                          bool dict_high = false /* ... its indices sit in the codes' high spare bits alone */);
bool stream_value_dict_high(int dtype, uint32_t n, int xs);
// K1s XD-V (spmv_stream_xd.hip): the dictionary of val's distinct bit patterns (32 entries of the value type on the device; *count_out
// = 0 when there are more), the codes' spare bits filled with the entries' dictionary indices, and how many indices those bits can name
int stream_value_dict(int dtype, const void *val, size_t nnz, void *dict_out, uint32_t *count_out, hipStream_t s);
int launch_stream_value_codes(int dtype, const void *val, size_t nnz, const void *dict, uint32_t n, int xs, uint16_t *code, hipStream_t s);
uint32_t stream_value_dict_capacity(int xs);
int launch_stream_stage_codes(const uint32_t *off, const uint32_t *col, const uint32_t *win, size_t n_rows, uint32_t elem_bytes,
                              uint16_t *code, hipStream_t s);
int launch_stream_odd_rows(const uint8_t *len8, size_t n_padded, unsigned long long *d_out, hipStream_t s);
int launch_stream_max_tile(const uint32_t *off, size_t n_rows, size_t tile_rows, uint32_t *d_out, hipStream_t s);
// K2c (column-blocked CSR; each block runs the K1s kernel)
int launch_spmv_stream_block(int dtype, const uint32_t *off, const uint32_t *col, const void *val, const void *x, void *y,
                             size_t n_rows, size_t nnz_total, int rows_per_thread, bool single_pass, bool accumulate,
                             hipStream_t s);
int build_colblock(int dtype, const uint32_t *off, const uint32_t *col, const void *val, size_t n_rows, size_t nnz,
                   uint32_t shift, size_t n_blocks, uint32_t **off2_out, uint32_t **col2_out, void **val2_out,
                   hipStream_t s);
// K2f (column-blocked, one sweep over y; spmv_colfused.hip)
int build_colfused(int dtype, const uint32_t *off, const uint32_t *col, const void *val, size_t n_rows, size_t nnz, uint32_t shift,
                   size_t n_blocks, uint32_t rt, size_t *n_tiles_out, uint32_t **tile_row_out, uint32_t **seg_out, uint8_t **cnt_out,
                   uint32_t **col2_out, void **val2_out, bool *fits_out, hipStream_t s);
int launch_spmv_colfused(int dtype, uint32_t rt, const uint32_t *tile_row, size_t n_tiles, const uint32_t *seg, const uint8_t *cnt,
                         const uint32_t *col, const void *val, const void *x, void *y, size_t n_rows, size_t nnz, uint32_t n_blocks,
                         int device, hipStream_t s);
// K2s (a skewed matrix as a long-row and a short-row column-blocked matrix; spmv_colsplit.hip)
int build_colsplit(int dtype, const uint32_t *off, const uint32_t *col, const void *val, size_t n_rows, size_t nnz, uint32_t min_long,
                   size_t *n_long_out, size_t *nnz_long_out, uint32_t **long_rows_out, uint32_t **off_l_out, uint32_t **col_l_out, void **val_l_out,
                   uint32_t **off_s_out, uint32_t **col_s_out, void **val_s_out, hipStream_t s);
int launch_split_scatter(int dtype, const uint32_t *long_rows, const void *y_long, size_t n_long, void *y, hipStream_t s);
// on-device assembly (assemble.hip): add_to/set stream -> CRS; sort_row for all rows.  Device pointers.
int assemble_triplets(int dtype, size_t n, const uint32_t *rows, const uint32_t *cols, const void *vals, const uint8_t *ops,
                      bool reverse_rows, bool all_set, bool repeats_adjacent, size_t *n_rows_out, size_t *n_cols_out, size_t *nnz_out,
                      uint32_t **off_out, uint32_t **col_out, void **val_out, hipStream_t s);
int expand_rows(const uint32_t *off, size_t n_rows, uint32_t *rows_out, hipStream_t s);
// transpose_bucket.hip: the column lists of ColumnIter by the same two bucketed passes (col_ptr [n_cols + 1], entries [nnz]: device arrays)
int column_lists_bucketed(const uint32_t *off, const uint32_t *col, size_t n_rows, size_t n_cols, size_t nnz, uint32_t max_col, uint32_t *col_ptr,
                          uint32_t *entries, bool *done, hipStream_t s);
// transpose_bucket.hip: transposition by two bucketed passes; *done == false: not applicable, nothing produced
int transpose_bucketed(int dtype, const uint32_t *off, const uint32_t *col, const void *val, size_t n_rows, size_t nnz, uint32_t max_col,
                       uint32_t **off_out, uint32_t **col_out, void **val_out, size_t *n_rows_out, size_t *n_cols_out, bool *done, hipStream_t s);
int append_to_row(int dtype, uint32_t *off, uint32_t **col, void **val, size_t n_rows, size_t *nnz, size_t row, uint32_t column,
                  const void *value_host, hipStream_t s);
int column_info(const uint32_t *off, const uint32_t *col, size_t n_rows, size_t n_cols, size_t nnz, uint32_t max_col, uint32_t *rows,
                uint32_t *col_ptr, uint32_t *entries, hipStream_t s);
int sort_rows(int dtype, const uint32_t *off, uint32_t *col, void *val, size_t n_rows, size_t nnz, uint32_t max_col,
              hipStream_t s);
// structure predicates and SparseMatrix::prod (matops.hip).  Device pointers.
int crs_is_sorted(const uint32_t *off, const uint32_t *col, size_t n_rows, int *out, hipStream_t s);
int crs_is_symmetric(int dtype, const uint32_t *off, const uint32_t *col, const void *val, size_t n_rows, int *out, hipStream_t s);
int prod_crs(int dtype, const uint32_t *a_off, const uint32_t *a_col, const void *a_val, size_t a_rows, size_t a_nnz, uint32_t a_max_col,
             const uint32_t *b_off, const uint32_t *b_col, const void *b_val, size_t b_rows, size_t *n_rows_out, size_t *n_cols_out,
             size_t *nnz_out, uint32_t **off_out, uint32_t **col_out, void **val_out, hipStream_t s);
// SparseMatrix::add / sub (matadd.hip).  Device pointers; operands with at least one row (a) / one entry (b).
struct AddOperand {
    const uint32_t *off = nullptr, *col = nullptr;
    const void *val = nullptr;
    size_t n_rows = 0, n_cols = 0, nnz = 0, orphans = 0;
    uint32_t max_row_len = 0, max_col = 0;
};
struct AddResult {
    size_t n_rows = 0, n_cols = 0, nnz = 0;
    CrsArrays arrays;          // the new arrays; all null when values_only
    int route = 0;             // smh_last_add_route
    bool values_only = false;  // in_place and no new entry: a's values were updated where they are
};
int add_crs(int dtype, bool subtract, const AddOperand &a, const AddOperand &b, bool in_place, bool alias, bool force_general, AddResult *res,
            hipStream_t s);
// SparseMatrix::get / set / add_to in batches (matupdate.hip).  Device pointers; m with at least one row.
struct UpdMatrix {
    const uint32_t *off = nullptr, *col = nullptr;
    void *val = nullptr;  // written in place by the values-only route
    size_t n_rows = 0, n_cols = 0, nnz = 0, orphans = 0;
    uint32_t max_row_len = 0;
};
struct UpdResult {
    size_t n_rows = 0, n_cols = 0, nnz = 0;
    CrsArrays arrays;          // the new arrays; all null when values_only
    int route = 0;             // smh_last_apply_route
    bool values_only = false;  // no new entry: m's values were updated where they are
};
int crs_get_many(int dtype, const UpdMatrix &m, size_t n, const uint32_t *rows, const uint32_t *cols, void *values_out, hipStream_t s);
int crs_apply(int dtype, const UpdMatrix &m, size_t n, const uint32_t *rows, const uint32_t *cols, const void *vals, const uint8_t *ops,
              bool force_general, UpdResult *res, hipStream_t s);
int build_eye(int dtype, size_t dim, uint32_t *off, uint32_t *col, void *val, hipStream_t s);
// Reordering (permute.hip, reorder.hip; a permutation is n u32 with perm[new] = old).  Device pointers.
// validate: `first` [n] is the caller's scratch and afterwards the inverse of perm; SMH_ERR_INVALID names the first offending position
int validate_permutation(const uint32_t *perm, size_t n, uint32_t *first, const char *what, hipStream_t s);
// out[i][j] = a[row_perm[i]][col_perm[j]] given col_inv = col_perm^-1 (either may be null: identity); storage order and values kept
int permute_crs(int dtype, const uint32_t *a_off, const uint32_t *a_col, const void *a_val, size_t n_rows, size_t nnz, const uint32_t *row_perm,
                const uint32_t *col_inv, CrsArrays *out, hipStream_t s);
int launch_vec_permute(int dtype, void *dst, const void *src, const uint32_t *perm, size_t n, bool inverse, hipStream_t s);
int launch_bandwidth(const uint32_t *off, const uint32_t *col, size_t n_rows, uint32_t *d_out2, hipStream_t s);  // {max i - j, max j - i}
// the reverse Cuthill-McKee ordering of a square pattern whose columns are all below n (perm_out: n entries)
int rcm_order(const uint32_t *off, const uint32_t *col, size_t n, size_t nnz, uint32_t *perm_out, size_t *n_components, size_t *n_levels, hipStream_t s);
// the graph both orderings work on (reorder.hip): u ~ v iff u != v and (u, v) or (v, u) is stored, as adj_off [n + 1] / adj_col with
// ascending neighbour lists, owned by scr; n > 0; 2^31 stored entries or more are SMH_ERR_CAPACITY
int symmetrised_pattern(const uint32_t *off, const uint32_t *col, size_t n, size_t nnz, Scratch &scr, uint32_t **adj_off_out, uint32_t **adj_col_out,
                        hipStream_t s);
// the multicolour ordering of the same pattern (color.hip): colors_out [n] by original row and perm_out [n], either may be null
int color_order(const uint32_t *off, const uint32_t *col, size_t n, size_t nnz, uint32_t seed, uint32_t *colors_out, uint32_t *perm_out, size_t *n_colors,
                size_t *n_rounds, hipStream_t s);
// A reusable update plan (matplan.hip): the sorted order and the targets of one (rows, cols, ops) stream on one structure.  Runs
// are numbered class by class: the short ones [0, n_short), then the long ones (more than kPlanLongRun kept operations).
constexpr uint32_t kPlanLongRun = 64;  // longest run one thread of the short-run kernel folds
struct UpdPlan {
    size_t n_ops = 0, n_targets = 0, n_live = 0, longest_run = 0, n_short = 0, device_bytes = 0;
    DevArray<uint32_t> pos;      // stream positions of the kept operations, grouped by run, in stream order inside a run (padded to 16 bytes)
    DevArray<uint32_t> off;      // n_targets + 1: where each run starts in pos
    DevArray<uint32_t> tgt;      // n_targets: the entry of m each run folds into
    DevArray<uint32_t> setbits;  // one bit per run: its first kept operation is a `set` (the stored value is not read)
};
// matupdate.hip: key_out[q] = target of the q-th operation in (target, stream order), src_out[q] = its stream position (n entries
// each); *n_absent_out = operations without a target in m (then nothing else is produced)
int crs_plan_targets(const UpdMatrix &m, size_t n, const uint32_t *rows, const uint32_t *cols, uint32_t *key_out, uint32_t *src_out,
                     uint64_t *n_absent_out, hipStream_t s);
int plan_build(size_t n, const uint32_t *key, const uint32_t *src, const uint8_t *ops, UpdPlan *plan, hipStream_t s);
// one gather-and-fold pass over the plan: m_val[tgt] = fold of values[pos] from m_val[tgt] (from_zero: from +0); enqueued on s
int plan_execute(int dtype, const UpdPlan &plan, const void *values, void *m_val, bool from_zero, hipStream_t s);
// K1r (LDS x-ring): inspector, host plan, kernel
struct RingPhase {
    uint32_t row_begin, row_end;  // rows of this phase (row_begin is a multiple of 64)
    uint32_t load_lo, load_hi;    // columns of x to add to the LDS ring before the phase (may be empty); band 0
    uint32_t use_ring;            // 0: the phase's column span exceeds the ring -> global gathers
    uint32_t band_lo[3], band_hi[3];  // banded ring (4 bands of a quarter of the ring each): loads of bands 1..3
};
constexpr int kRingPhaseWords = 11;
int launch_tile_span(const uint32_t *off, const uint32_t *col, size_t n_rows, size_t n_tiles, uint32_t *cmin,
                     uint32_t *cmax, hipStream_t s);
// col16 (optional): the low halves of the columns, padded with zeros to a multiple of 4 entries plus one chunk; ring
// phases then stream 2 instead of 4 bytes per column
// c12 (optional, instead of col16; f32 on the single-window ring of kRingEntries columns): the compact form of ring_col12.hpp,
// 1.5 bytes per column -- lo8: one byte per entry, hdr: one u16 per 4-entry chunk (both padded like col16), escapes: 2 u32 per
// chunk the code cannot hold
// rec16 (optional, instead of lo8; matrices whose values all fit the 24-bit code of ring_val24.hpp): one 16-byte record per chunk --
// the four values as 24-bit integers and, in its fourth dword, the chunk's dword of lo8 -- with scale = 2^E; hdr and escapes as
// before.  The ring phases then read neither lo8 nor the value array.
struct RingCol12 {
    const uint8_t *lo8 = nullptr;
    const uint16_t *hdr = nullptr;
    const uint32_t *escapes = nullptr;
    const uint32_t *rec16 = nullptr;
    float scale = 0.0f;
};
int launch_spmv_ring2(int dtype, int lanes, int chunks, const uint32_t *off, const uint32_t *col, const uint16_t *col16, const RingCol12 &c12,
                      const void *val, const void *x, void *y, size_t n_rows, size_t nnz, bool padded, unsigned n_blocks,
                      const uint32_t *phase_ptr, const RingPhase *phases, unsigned ring_entries, unsigned bands,
                      hipStream_t s, void *dot_partials = nullptr /* DOT form: y = lhs (read only), n_blocks + 1 partials of lhs . (A x) */,
                      unsigned block_begin = 0, unsigned block_end = ~0u /* the plan's row ranges [begin, end) only (default: all; not with the DOT form) */,
                      const uint32_t *reg_len = nullptr /* RingPlan::reg_len: regular phases compute their row offsets (NULL: every phase loads them) */,
                      int *resident_out = nullptr, int *threads_out = nullptr /* both: a query, nothing is enqueued -- the workgroups of the kernel
                      this call would launch that a CU holds at once (hipOccupancyMaxActiveBlocksPerMultiprocessor; 0: none) and their size */);
// K1r's all-regular form (spmv_ring2_allreg.hip): f32, the single-window ring of kRingEntries columns, no DOT, for a plan whose phases
// are all regular (RingPlan::reg_all) -- the REG body alone in workgroups of kRingAllregThreads threads, y bit for bit that of the
// REGK form.  The column form is the one c12 / col16 hold (records, compact form, 16-bit columns); the other arguments and the
// query are launch_spmv_ring2's.  ring2_allreg_has: (lanes, chunks) has the form (it is built where it needs no scratch within 80 VGPRs).
constexpr int kRingAllregThreads = 768;
bool ring2_allreg_has(int lanes, int chunks);
int launch_spmv_ring2_allreg(int lanes, int chunks, const uint32_t *off, const uint32_t *col, const uint16_t *col16, const RingCol12 &c12,
                             const float *val, const float *x, float *y, size_t n_rows, size_t nnz, bool padded, unsigned n_blocks,
                             const uint32_t *phase_ptr, const RingPhase *phases, hipStream_t s, unsigned block_begin, unsigned block_end,
                             const uint32_t *reg_len, int *resident_out = nullptr, int *threads_out = nullptr);
// the <= 3 entries of an unpadded array's last partial chunk, added to their rows behind a K1r launch that covers the last rows
int launch_ring2_tail(int dtype, const uint32_t *off, const uint32_t *col, const void *val, const void *x, void *y, size_t n_rows,
                      uint64_t k_begin, size_t nnz, hipStream_t s);
// reg_len[p] = L when phase p gathers from the ring (use_ring == 1), L > 0 and off[r] == off[row_begin] + (r - row_begin) * L for
// every r in [row_begin, row_end]; else 0.  One read of the offsets.
int launch_ring_regular(const uint32_t *off, const RingPhase *phases, size_t n_phases, uint32_t *reg_len, hipStream_t s);
// banded ring (4 bands): per-tile column intervals (the K1s inspector over 64-row tiles) and the 16-bit ring slots
int launch_tile_intervals(const uint32_t *off, const uint32_t *col, size_t n_rows, size_t tile_rows, size_t max_width,
                          uint32_t *win, uint32_t *d_count, hipStream_t s);
int launch_ring_band_codes(const uint32_t *off, const uint32_t *col, const uint32_t *win, size_t n_rows, uint32_t S,
                           uint16_t *code, hipStream_t s);
int launch_narrow_columns(const uint32_t *col, size_t nnz, uint16_t *col16, size_t n_out, hipStream_t s);
// the compact form's build.  count: jobs (2 u32 per phase) = the chunks each ring phase streams, counts[0] = how many those are,
// counts[1] = how many of them the code cannot hold.  encode: lo8 / hdr (n_chunks_out chunks, all written) and the side table
// (room for counts[1] entries of the count pass; counts[1] is reused as its allocator)
int launch_col12_count(const uint32_t *off, const uint32_t *col, size_t nnz, const RingPhase *phases, size_t n_phases, uint32_t *jobs,
                       unsigned long long *counts, hipStream_t s);
int launch_col12_encode(const uint32_t *col, size_t nnz, const uint32_t *jobs, size_t n_phases, size_t n_chunks_out, uint8_t *lo8,
                        uint16_t *hdr, uint32_t *escapes, unsigned long long *counts, hipStream_t s);
// the chunk records' build (f32).  count: jobs as above (counts: 2 words of scratch for it), stats[0] = 1024 + the largest E every
// non-zero value of the jobs' chunks is a multiple of 2^E for (~0u: there is none), stats[1] != 0: some value the code never holds.
// encode: rec16 (n_chunks_out records of 16 bytes, all written; the fourth dword from lo8), *misses = values of the jobs' chunks
// that do not decode to their own bits
int launch_val24_count(const uint32_t *off, const float *val, size_t nnz, const RingPhase *phases, size_t n_phases, uint32_t *jobs,
                       unsigned long long *counts, uint32_t *stats, hipStream_t s);
int launch_val24_encode(const float *val, size_t nnz, const uint32_t *jobs, size_t n_phases, size_t n_chunks_out, const uint8_t *lo8, int exponent,
                        uint32_t *rec16, unsigned long long *misses, hipStream_t s);
// structure statistics / validation
struct CrsStats {
    uint32_t max_row_len;
    uint32_t max_col;
    uint32_t min_col_inv;  // ~(smallest column)
    uint32_t bad;  // bit0: offsets not monotone, bit1: off[0]!=0, bit2: off[n]!=nnz
};
int launch_crs_stats(const uint32_t *off, const uint32_t *col, size_t n_rows, size_t nnz, CrsStats *d_stats,
                     hipStream_t s);
// K2t (spmv_tiled.hip)
void tiled_geometry(size_t n_rows, size_t n_cols, size_t nnz, int dtype, uint32_t *n_cb, uint32_t *rows_per_block, uint32_t *n_rb);
int tiled_build(::smh_crs *m);   // lazy; leaves m->tiled Ready or Refused
uint32_t tiled_slice_columns(int dtype);
int columns_within_n_cols(const ::smh_crs *m, const char *what);  // crs_forms.hip: SMH_ERR_INDEX_RANGE when max_col >= n_cols
int tiled_array(::smh_crs *m, int which, void *out, size_t capacity_bytes, size_t *bytes_out);
int launch_spmv_tiled(::smh_crs *m, const void *x, size_t x_len, void *y, hipStream_t s);
size_t spmv_fused_dot_partials(::smh_crs *m, size_t x_len, int variant, bool any_lhs = false);
// y = A x on stream s with the handle's kernel (spmv_dispatch.hip).  dot_partials (optional): when spmv_fused_dot_partials() > 0 the
// kernel also leaves that many partial sums of x.y there (K1s epilogue; square matrices) -- CG's / PCG's p.Ap for free
int spmv_enqueue(::smh_crs *m, const void *x, size_t x_len, void *y, int variant, hipStream_t s, void *dot_partials = nullptr,
                 const void *dot_lhs = nullptr);
// products of a run of rows (spmv_dispatch.hip; used by par_step.hip and par_cg.hip to multiply a block's boundary rows before / after its interior ones)
int spmv_rows_granularity(::smh_crs *m, int variant, size_t *gran_out);
int spmv_enqueue_rows(::smh_crs *m, const void *x, size_t x_len, void *y, int variant, hipStream_t s, size_t row0, size_t row1,
                      void *dot_partials = nullptr, const void *dot_lhs = nullptr);
// ... of a SHORT run (a block's boundary rows), any row0 / row1: ring matrices through the plain lane-group kernel (same bits)
int spmv_enqueue_rows_short(::smh_crs *m, const void *x, size_t x_len, void *y, int variant, hipStream_t s, size_t row0, size_t row1);
// BLAS-1 (a_dev: scalar read from device memory when non-null, else `a`)
enum class Ew { Add, Sub, Scale, Axpy, Xpby, RSubInto };
int launch_ew(int dtype, Ew op, void *x, const void *y, size_t n, double a, const void *a_dev, hipStream_t s);
// rows_off (n + 1 CRS row offsets): element i is a term only where rows_off[i + 1] != rows_off[i] (SparseMatrix::inner_prod)
int launch_dot(int dtype, const void *x, const void *y, size_t n, void *partials, void *result_dev,
               hipStream_t s, const uint32_t *rows_off = nullptr);
int launch_fold2(int dtype, const void *in, size_t count, void *partials, void *result_dev, hipStream_t s);  // *result = sum(in)
int launch_scale_values(int dtype, void *v, size_t n, double a, hipStream_t s);
// Sparse triangular solves (trisolve.hip).  ensure_tri_schedule: the lazy level schedule m->tri[uplo] of a square handle whose
// columns are all below n.  trisolve_enqueue: x = T^-1 b on s by that schedule (built before; device pointers, x may be b); scale_rhs:
// the right-hand side is b[i] * val[diagpos[i]], rounded once; active (optional): a device flag, 0 = every launch returns at once
int ensure_tri_schedule(::smh_crs *m, int uplo);
int tri_lanes(const ::smh_crs *m);  // lanes of the group a row gets, in the solves and in ilu.hip
int trisolve_enqueue(::smh_crs *m, int uplo, int diag, bool scale_rhs, const void *b, void *x, const uint32_t *active, hipStream_t s);
// what smh_crs_ilu0 and smh_crs_fsai require of a pattern (ilu.hip): square, no orphan, columns below n, rows strictly ascending, every
// (i, i) stored -- checked on the device in that order, nothing written; what: whose refusal it is
int ilu_check(const ::smh_crs *a, const char *what);

// ---- the device-resident solvers (cg.hip, pcg.hip, par_cg.hip) ----------------------------------------------------------------------
// The scalar block of a solve: it lives in device memory, the kernels of cg.hip advance it, the host copies it back once per batch.
// (pcg.hip's PcgScalars has the same layout -- asserted there -- with r.z in the place of rr_prev.)
template <typename T>
struct CgScalars {
    T rr, rr_prev, pap, alpha, beta;
    uint32_t converged;
    uint32_t active;
    uint32_t entered;  // the current loop body was entered: its x update is due (set with alpha)
    uint32_t pad_;
    uint64_t iters;
    uint64_t iter_max;
    double tol;
};
// what cg_read_scalars relies on when the host polls another solver's leading block S<T> through it: CgScalars' size, and rr,
// converged and iters at CgScalars' offsets
template <template <typename> class S, typename T> constexpr bool scalars_like_cg_t() {
    return sizeof(S<T>) == sizeof(CgScalars<T>) && offsetof(S<T>, rr) == offsetof(CgScalars<T>, rr) &&
           offsetof(S<T>, converged) == offsetof(CgScalars<T>, converged) && offsetof(S<T>, iters) == offsetof(CgScalars<T>, iters);
}
template <template <typename> class S> constexpr bool scalars_like_cg() { return scalars_like_cg_t<S, float>() && scalars_like_cg_t<S, double>(); }
size_t cg_scalars_bytes(int dtype);  // cg.hip
// host view of a copy of the scalar block after a poll (cg.hip)
void cg_read_scalars(int dtype, const void *host_copy, int *converged, uint64_t *iters, double *rr);

// The loop of a single-matrix solve on stream s: up to iter_max bodies, body() enqueues one.  "active" drops on the device at the
// stop (cg.hip), and bodies enqueued past it are no-ops there, so the host enqueues check_every bodies at a time and polls the
// scalar block (d_sc, through the pinned h_sc) once per batch.  With more than one batch to go the batch is captured ONCE into a
// hipGraph and replayed, always whole: for small systems the loop is launch-bound.  If the capture does not come about the bodies
// are launched one by one.  *converged, *iters, *rr: the block as the last poll saw it.
// capture = false: never captured (a body of very many launches: SGS-PCG on a matrix of many levels).
template <typename Body>
int solve_in_batches(int dtype, hipStream_t s, size_t iter_max, size_t check_every, Body &&body, const void *d_sc, void *h_sc, int *converged,
                     size_t *iters, double *rr, bool capture = true) {
    Graph graph;
    GraphExec exec;
    t_solve_replays = 0;
    const bool may_capture = capture && iter_max > check_every && capture_enter();  // (no: another host thread is using the library)
    if (may_capture && hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        int crc = SMH_OK;
        for (size_t i = 0; i < check_every && crc == SMH_OK; ++i) crc = body();
        const hipError_t ce = graph.end_capture(s);  // (also after a body that failed: the stream must leave capture mode)
        if (crc != SMH_OK || ce != hipSuccess || !graph.get() || exec.instantiate(graph.get()) != hipSuccess)
            (void)hipGetLastError();  // exec is empty: plain stream launches instead
    } else {
        (void)hipGetLastError();
    }
    if (may_capture) capture_leave();
    auto poll = [&]() -> int {
        SMH_HIP(hipMemcpyAsync(h_sc, d_sc, cg_scalars_bytes(dtype), hipMemcpyDeviceToHost, s));
        SMH_HIP(hipStreamSynchronize(s));
        uint64_t it64 = 0;
        cg_read_scalars(dtype, h_sc, converged, &it64, rr);
        *iters = (size_t)it64;
        return SMH_OK;
    };
    auto run = [&]() -> int {
        size_t launched = 0;
        while (launched < iter_max) {
            size_t batch = iter_max - launched < check_every ? iter_max - launched : check_every;
            if (exec.get()) {
                SMH_HIP(hipGraphLaunch(exec.get(), s));
                ++t_solve_replays;
                batch = check_every;
            } else {
                for (size_t i = 0; i < batch; ++i) SMH_TRY(body());
            }
            launched += batch;
            SMH_TRY(poll());
            if (*converged) break;
        }
        if (iter_max == 0) SMH_TRY(poll());
        return SMH_OK;
    };
    const int rc = run();
    if (rc != SMH_OK) (void)hipStreamSynchronize(s);  // a replayed batch may still run: it ends before its graph goes
    return rc;
}

// ---- what a CRS handle derives lazily from its own arrays (built by crs_forms.hip's ensure_* and spmv_tiled.hip's tiled_build) ----
// Each form is filled in a local instance and move-assigned into the handle when it is complete; a default-constructed one is
// "not built", and assigning that drops the form (the members free themselves).
enum class Form {
    NotTried,
    Ready,
    Refused,  // the build was attempted and the form does not apply to this matrix: AUTO takes its next choice, nothing is tried again
};
struct MergeTable {  // K2
    Form state = Form::NotTried;
    size_t n_tiles = 0;
    DevArray<uint32_t> tile_row, tile_nz, carry_row;
    DevArray<char> carry_val;
};
struct RingPlan {  // K1r
    Form state = Form::NotTried;
    bool bands_tried = false;             // the plan was built with the banded attempt allowed
    unsigned blocks = 0;
    double fraction = 0.0;                // share of rows whose gathers are served from the LDS ring
    unsigned entries = kRingEntries;      // ring size the plan was built for
    unsigned bands = 1;                   // 1: one sliding window; 4: banded ring (needs col16 = ring slots)
    size_t n_phases = 0;
    DevArray<uint32_t> phase_ptr;
    DevArray<RingPhase> phases;
    DevArray<uint32_t> reg_len;           // one per phase: the row length of a ring phase whose rows are all equally long, else 0 (launch_ring_regular)
    bool reg_applies = false;             // every phase gathers from the ring and some are regular: launches pass reg_len (k_spmv_ring2's REGK form)
    bool reg_all = false;                 // ... and every phase that holds rows is regular: f32 launches without DOT take the all-regular form
    DevArray<uint32_t> win;              // banded plan: the tiles' column intervals (8 u32 per 64-row tile)
    DevArray<uint16_t> col16;             // 16-bit column array for the ring phases (built from the plan on first use; null: not used)
    // the compact column form (ring_col12.hpp), which the ring phases then stream instead of col16.  c12: NotTried until the counting pass has run; Ready: at most one
    // chunk in 1024 escapes, AUTO takes the form; Refused: AUTO keeps col16.  The arrays exist while the form is in use.
    Form c12 = Form::NotTried;
    uint64_t c12_chunks = 0, c12_escapes = 0;  // chunks the ring phases stream; those of them the code cannot hold
    DevArray<uint8_t> lo8;
    DevArray<uint16_t> hdr;
    DevArray<uint32_t> escapes;
    // the chunk records of the 24-bit value code (ring_val24.hpp), built INSTEAD of lo8 where the compact form is in use, the plan
    // takes the REGK kernel and every value the ring phases stream decodes to its own bits (hdr and escapes are shared).  v24:
    // NotTried until the values have been tested (and again after they changed); Ready: they fit, with exponent v24_exp; Refused.
    Form v24 = Form::NotTried;
    int v24_exp = 0;
    DevArray<uint32_t> rec16;             // 4 u32 per chunk; exists while the form is in use (then lo8 does not)
};
struct StreamCodes {  // K1s 16-bit column codes (Ready only when every tile has a description; Refused holds nothing)
    Form state = Form::NotTried;
    DevArray<uint32_t> cwin;              // 8 u32 per 256-row tile
    DevArray<uint16_t> code;              // one u16 per entry
    DevArray<uint8_t> len8;               // with max_row_len <= 255: one byte per row (its length) ...
    DevArray<uint32_t> tbase;             // ... and one u32 per 256-row tile (its first entry)
    uint32_t xs_chunks = 0xFFFFFFFFu, xs_end = 0;  // K1s XS: most x chunks a tile needs; largest x index + 1 they touch
    uint64_t odd_rows = 0;                // rows of odd length (taken with the byte lengths)
    bool direct = false;                  // code holds stage byte offsets (K1s XD) instead of column codes
    // K1s XD-V: ... and, in their spare bits, indices into a dictionary of the matrix's distinct values (the value array is then not read)
    bool vdict = false;                   // the codes carry the indices now (built for a stage of vdict_xs * 1024 entries)
    int vdict_xs = 0;
};
struct StreamDict {  // K1s XD-V value dictionary: follows the values, where the codes follow the structure
    Form state = Form::NotTried;          // NotTried: not looked at (or the values changed); Refused: too many distinct values
    uint32_t n = 0;
    DevArray<char> values;                // 32 values (kept across a look: a product in flight may still read it)
};
struct ColBlock {  // K2c column-blocked copy
    Form state = Form::NotTried;
    uint32_t shift = 0;                   // block width = 2^shift columns
    size_t blocks = 0;
    int rpt = 1;                          // rows per thread of the K1s launches (tile = 256*rpt rows)
    bool single_pass = false;             // no tile of any block exceeds the LDS stage
    DevArray<uint32_t> off, col;
    DevArray<char> val;
};
struct ColFused {  // K2f fused column-blocked copy (Refused: the byte table cannot describe the matrix; the geometry stays readable)
    Form state = Form::NotTried;
    uint32_t shift = 0, rt = 0;
    size_t blocks = 0, tiles = 0;
    DevArray<uint32_t> seg, col, tile_row;
    DevArray<uint8_t> cnt;
    DevArray<char> val;
};
struct RowSplit {  // K2s row-length split: two sub-handles (owned) + the rows of the long one (Refused: not worth building)
    Form state = Form::NotTried;
    ::smh_crs *long_part = nullptr, *short_part = nullptr;
    DevArray<uint32_t> rows;
    DevArray<char> y;
    size_t n_long = 0;
    hipStream_t side = nullptr;           // the LONG part runs beside the SHORT one (fork / join by events)
    hipEvent_t fork = nullptr, join = nullptr;
    RowSplit() = default;
    RowSplit(RowSplit &&o) noexcept { swap(o); }
    RowSplit &operator=(RowSplit &&o) noexcept {
        RowSplit old(std::move(*this));  // (dropped at the end of this scope)
        swap(o);
        return *this;
    }
    ~RowSplit();  // crs_forms.hip; the sub-handles go through smh_crs_destroy (capi.hip), like every handle
    void swap(RowSplit &o) noexcept {
        std::swap(state, o.state); std::swap(long_part, o.long_part); std::swap(short_part, o.short_part);
        std::swap(rows, o.rows); std::swap(y, o.y); std::swap(n_long, o.n_long);
        std::swap(side, o.side); std::swap(fork, o.fork); std::swap(join, o.join);
    }
};
struct Tiled {  // K2t 2-D tiled copy (spmv_tiled.hip): entries by column slice, within a slice by row (Refused: its build failed)
    Form state = Form::NotTried;
    uint32_t n_cb = 0, n_rb = 0, R = 0;   // column slices, row blocks, rows of the largest block
    uint64_t tot = 0;                     // entries of the copy (slices padded to 8)
    DevArray<char> val, prod;             // values in copy order; the products of the last launch
    DevArray<uint16_t> code, row;         // column within the slice; row within the row block
    DevArray<uint32_t> tstart;            // (n_rb + 1) x n_cb tile starts, relative to the slice
    DevArray<uint32_t> rbstart;           // first row of each row block (n_rb + 1); blocks hold equal entry counts
    DevArray<uint32_t> cptr;              // (round 3's form) first chunk of each slice (n_cb + 1)
    DevArray<char> chunk;                 // per chunk {where its product sums go, entries}
    uint32_t n_chunks = 0, max_slice_chunks = 0;
    bool dups = false;                    // a chunk boundary cuts a (row, slice) pair somewhere: pass 2 checks for equal neighbours
    uint64_t n_prod = 0;                  // product slots (one per (row, slice, chunk), chunk shares padded to 16 bytes)
};
struct TriSchedule {  // level schedule of a triangular solve (trisolve.hip), one per uplo: positions only, no values
    Form state = Form::NotTried;
    size_t n_levels = 0;
    uint64_t first_no_diag = ~0ull;       // the first row without a stored (i, i); ~0: every row has one
    DevArray<uint32_t> rows;              // the rows level by level, ascending inside a level (n)
    DevArray<uint32_t> level_ptr;         // where each level starts in rows (n_levels + 1)
    DevArray<uint32_t> level;             // level of each row (n)
    DevArray<uint32_t> diagpos;           // first k with col[k] == i (n; ~0u: none)
    // one kernel launch: a level of more than kTriSmallRows rows on a grid, or a run of consecutive levels of at most that many
    // rows each walked by one workgroup (kTriSmallBlock threads) with a barrier between levels
    struct Launch { uint32_t level_begin, level_end, row_begin, row_end; bool small; };
    std::vector<Launch> launches;
};
// R: one pass of the multi-level kernel's workgroup (kTriSmallBlock threads) at the 8 lanes per row of a stencil.  Measured on the
// natural 1024^2 five-point grid (2047 levels of 1 .. 1024 rows): with R = 1024 the whole solve was one workgroup on one CU, 19 ms
// -- 9 us per level, several passes of dependent gathers each -- where a launch per level costs about 6 us
constexpr uint32_t kTriSmallRows = 128;
constexpr uint32_t kTriSmallBlock = 1024;
struct StageBuf {  // a staging vector of the host-pointer API (lazy, reused)
    DevArray<char> d;
    size_t cap = 0;
    int ensure_cap(size_t bytes) {
        if (cap >= bytes && d.get()) return SMH_OK;
        cap = 0;
        const size_t want = bytes < 256 ? 256 : bytes;
        SMH_TRY(d.alloc(want));
        cap = want;
        return SMH_OK;
    }
};
// the smh_crs_set_* settings a clone (and a handle updated in place) carries
struct Knobs {
    int forced_lanes = 0;
    int forced_chunks = 0;
    int stream_rows_per_thread = 0;       // 0 automatic (2 when every 512-row tile fits), 1 force one
    uint32_t cb_forced_shift = 0;         // 0 automatic (2 MiB of x per block)
    int use_ring = -1;                    // -1 automatic, 0 never, 1 always (when lanes <= 8), 2 always with the first K1r body
    int use_stream_xs = -1;               // K1s XS: -1 automatic (x beyond the L2s; the 4096-entry stage on f32 only), 0 never, 1 whenever the tiles allow
    int use_stream_direct = -1;           // K1s XD: -1 automatic (most rows of odd length), 0 never, 1 whenever x is staged
    int use_stream_vdict = -1;            // -1 automatic (whenever the values allow), 0 never
    int use_col16 = -1;                   // -1 automatic (when at least a quarter of the rows are ring rows), 0 never, 1 always
    int use_col12 = -1;                   // the compact form instead: -1 automatic (where it applies, few chunks escape and use_col16 is automatic too), 0 never, 1 wherever it applies
    int use_val24 = -1;                   // the chunk records with 24-bit values, where the compact form is in use: -1 / 1 when the values fit, 0 never
};

}  // namespace smh

// ---- handles ------------------------------------------------------------------------------
namespace smh {
uint64_t next_crs_id();  // capi.hip: a process-unique id for every handle ever made
}
struct smh_crs {
    // what an update plan is bound to: this handle (id) in this structure (epoch: advanced whenever offsets, columns or storage
    // order change -- replace_state, sort_rows; not by scale / update_values / a values-only apply or += / a plan execute)
    uint64_t id = smh::next_crs_id();
    uint64_t epoch = 0;
    int dtype = SMH_F32;
    int device = 0;
    size_t n_rows = 0, n_cols = 0, nnz = 0;
    size_t orphans = 0;  // entries the reference's container still holds but no row reaches (first-push quirk of a replay): 0 or 1
    // the single operation of a handle without rows but with its orphan (the one-operation replay, smh_crs_eye(1)): row, column
    // and folded value (f32 / f64 bits), so that smh_crs_apply can continue the replay as the reference does
    bool has_first_op = false;
    uint32_t first_row = 0, first_col = 0;
    uint64_t first_val_bits = 0;
    uint32_t *d_off = nullptr;
    uint32_t *d_col = nullptr;
    void *d_val = nullptr;
    bool owns = true;
    bool no_split = false;  // this handle IS a part of a K2s split: never split again (not a setting: a clone does not take it)
    hipStream_t stream = nullptr;
    // statistics
    uint32_t max_row_len = 0;
    uint32_t max_col = 0;
    uint32_t min_col = 0;
    uint32_t max_tile_entries = 0;  // most entries in any 256-row tile (K1s eligibility)
    uint32_t max_tile512_entries = 0;  // ... in any 512-row tile (K1s with two rows per thread)
    bool have_stats = false;
    double span_fraction = 0.0;  // mean column span of a 64-row tile / n_cols (1: no locality at all); taken with the first K1r plan
    smh::Knobs knobs;
    // the derived forms (all lazy)
    smh::MergeTable merge;
    smh::RingPlan ring;
    smh::StreamCodes codes;
    smh::StreamDict dict;
    smh::ColBlock cb;
    smh::ColFused cf;
    smh::RowSplit split;
    smh::Tiled tiled;
    smh::TriSchedule tri[2];  // [SMH_TRI_LOWER], [SMH_TRI_UPPER]
    smh::StageBuf stage_x, stage_y;
    // what the inspectors cost (smh_crs_prepare_stats): wall ms / pooled device bytes left allocated, create-time and prepare-time
    double create_ms = 0.0, prepare_ms = 0.0;
    long long create_bytes = 0, prepare_bytes = 0;
};

struct smh_vec {
    int dtype = SMH_F32;
    int device = 0;
    size_t n = 0;
    void *d = nullptr;
    bool owns = true;
};

// k vectors of dimension n, interleaved: element i of vector c at d[i * ld + c]; ld = k rounded up to a multiple of 4, the padding
// columns are zero and stay zero (mvec.hip).  The storage frees itself with the handle.
struct smh_mvec {
    int dtype = SMH_F32;
    int device = 0;
    size_t n = 0, k = 0, ld = 0;
    smh::DevArray<char> d;
};

namespace smh {
// K5m (cg_many.hip): ConjugateGradient::solve on the k columns of b and x at once; the argument checks are the entry point's
// (smh_cg_solve_many, in the same file).  iters_out / rr_out: k entries each.  (The per-column BLAS-1 of smh_mvec and the column tree: mvec_tree.hpp.)
int cg_solve_many(::smh_crs *m, const ::smh_mvec *b, ::smh_mvec *x, double tol, size_t iter_max, size_t check_every, size_t *iters_out,
                  double *rr_out);
}  // namespace smh

// ---- every .hip file of the library but pool.hip allocates device memory through the pool (declared at the top) ----------
#ifndef SMH_POOL_IMPL
#define hipMalloc(p, n) (::smh::note_thread(), ::smh::pool_malloc((void **)(p), (n)))
#define hipFree(p) (::smh::note_thread(), ::smh::pool_free((void *)(p)))
#endif
