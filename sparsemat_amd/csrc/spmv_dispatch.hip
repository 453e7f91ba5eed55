// spmv_dispatch.hip -- which kernel a product runs (AUTO's rules, with the measurements behind every threshold), which derived forms
// that kernel runs on, and its launches.  Host-side logic only; the forms themselves are built in crs_forms.hip.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "crs_forms.hpp"

namespace smh {

// ---- variant selection ---------------------------------------------------------------------------
static double mean_row(const smh_crs *m) { return m->n_rows ? (double)m->nnz / (double)m->n_rows : 0.0; }

// lanes sized to the mean row alone (the skew test of AUTO)
static int mean_lanes(const smh_crs *m) {
    const double mean = mean_row(m);
    // one pass of a lane group covers 4*lanes entry slots: size the group to the mean row; short rows
    // start anywhere inside their first 16-B chunk, so they get 3 slots of slack (measured on the 7-point
    // Laplacian: 4 lanes 2.87 ms, 2 lanes 3.68 ms, 1 lane x 3 chunks 3.11 ms)
    const double need = mean < 16.0 ? mean + 3.0 : mean;
    int lanes = 1;
    while (lanes < 64 && 4.0 * lanes < need) lanes <<= 1;
    return lanes;
}

int auto_lanes(const smh_crs *m) {
    if (m->knobs.forced_lanes) return m->knobs.forced_lanes;
    const double mean = mean_row(m);
    int lanes = mean_lanes(m);
    // Long rows in the pipelined body (contiguous-band matrices, 320 M entries, same box): rows of 128 / 256 entries
    // run in 0.313 / 0.301 ms with 16 lanes (2 / 4 passes of 64 slots) against 0.359 / 0.348 ms with one pass of 32 / 64
    // lanes; rows of 100 entries prefer one pass of 32 lanes (0.398 vs 0.500 ms).
    if (m->knobs.use_ring != 0) {
        if (mean >= 128.0) lanes = 16;
        else if (lanes > 32) lanes = 32;
        // ... and when their columns do not fit the ring (global gathers, one cache line each) 8 lanes lose least
        // (banded +-32768, rows of 256: 1.28-1.33 ms with 4-8 lanes, 1.51 ms with 16, 1.62-1.80 ms with 64)
        if (mean > 32.0 && m->ring.state == Form::Ready && m->ring.fraction < 0.5) lanes = 8;
    }
    return lanes;
}

// 16-B chunks each lane loads per pass (pipelined K1r body only): 4*lanes*chunks entry slots per row and pass
static int auto_chunks(const smh_crs *m) {
    const int lanes = auto_lanes(m);
    if (m->knobs.forced_chunks) {
        if (lanes == 1) return m->knobs.forced_chunks;
        if (lanes == 2) return m->knobs.forced_chunks > 2 ? 2 : m->knobs.forced_chunks;
        return 1;
    }
    return 1;
}

// K2c geometry: column blocks of 2 MiB of x
// 2^19 columns: 2 MiB of f32 x.  f64 takes the same width (4 MiB of x, a whole L2): measured on C3, 20 blocks of
// 2^19 run in 3.64 ms, 39 blocks of 2^18 in 5.08 ms -- the per-block sweeps of offsets and y (12 B + 8 B per row)
// outweigh the better hit rate (profiles/r01_colblock_sweep.log)
uint32_t cb_shift_for(const smh_crs *m) { return m->knobs.cb_forced_shift ? m->knobs.cb_forced_shift : 19u; }
// K2f geometry: blocks of 2^18 columns (1 MiB of f32 x, 2 MiB of f64 x): its waves walk the blocks without a barrier and
// spread over a few of them, so the L2 has to hold more than one (measured on C2-uniform, f32: 2^18 2.05 ms, 2^19 2.40 ms);
// a forced width applies to both blocked variants
uint32_t cf_shift_for(const smh_crs *m) { return m->knobs.cb_forced_shift ? m->knobs.cb_forced_shift : 18u; }
// the blocks of 2^shift columns that n_cols columns make (at least one)
size_t blocks_for(size_t n_cols, uint32_t shift) {
    const uint64_t w = 1ull << shift;
    const uint64_t b = ((uint64_t)n_cols + w - 1) / w;
    return (size_t)(b ? b : 1);
}
// x too large for the L2s AND rows whose columns span a large part of it (statistic taken at create time for
// matrices with more than 8 MiB of x): gathers would miss L1 and L2 -> column-blocked execution
// (tools/experiment_gather.py, 4M rows x 32 uniform columns, f32: K1 / K2c at x = 4 MiB 0.80 / 0.68 ms, 8 MiB
// 1.25 / 0.66 ms, 16 MiB 1.76 / 0.71 ms, 64 MiB 2.35 / 1.44 ms)
const size_t kColblockMinXBytes = 4u << 20;
static bool wants_colblock(const smh_crs *m) {
    const size_t b = blocks_for(m->n_cols, cb_shift_for(m));
    return m->n_cols * dtype_size(m->dtype) >= kColblockMinXBytes && m->span_fraction > 0.25 && b >= 2 && b <= 128;
}

// K2t is an option: not switched off, its copy was not refused, >= min_tile entries per (slice, row block) tile, a tile table of <= 1 GiB
static bool tiled_fits(const smh_crs *m, double min_tile = 32.0) {
    static const bool tiled_off = getenv("SMH_TILED") && atoi(getenv("SMH_TILED")) == 0;  // tuning knob
    if (tiled_off || m->tiled.state == Form::Refused) return false;
    uint32_t n_cb = 0, R = 0, n_rb = 0;
    tiled_geometry(m->n_rows, m->n_cols, m->nnz, m->dtype, &n_cb, &R, &n_rb);
    const double tile = (double)m->nnz / (double)n_cb / (double)n_rb;
    return tile >= min_tile && (double)(n_rb + 1) * (double)n_cb * 4.0 <= (double)(1u << 30);
}

int resolve_variant(const smh_crs *m, int variant) {
    if (variant != SMH_SPMV_AUTO) return variant;
    if (wants_colblock(m)) {
        // one sweep over y (K2f) unless its byte table cannot describe the matrix / it was switched off
        static const bool fused_off = getenv("SMH_COLBLOCK_FUSED") && atoi(getenv("SMH_COLBLOCK_FUSED")) == 0;  // tuning knob
        if (fused_off || m->cf.state == Form::Refused || blocks_for(m->n_cols, cf_shift_for(m)) > 255) return SMH_SPMV_COLBLOCK;
        // K2f's waves keep their tiles for the whole sweep: that only works while they stay together, i.e. for rows of
        // similar length.  Skewed rows (BASELINE C3, power law 1..2048) let them drift over all column blocks at once
        // -- 5.2-5.6 ms against K2c's 3.25 ms, and a lock step costs more than it recovers (profiles/r02_k2f_sweep.log) --
        // so those stay with the per-block launches, whose tiles the dispatcher hands out dynamically.
        // (measured on parts of C3, profiles/r02_c3_split_probe.log: rows of up to 63 / 127 entries, mean 5.5 / 7.9, still run
        // best through K2f -- 0.82 / 1.15 ms against K2c's 0.97 / 1.26; up to 255 entries K2c wins, 1.61 against 1.79)
        const double mean = mean_row(m);
        const double similar = 2.0 * mean + 8.0 > 128.0 ? 2.0 * mean + 8.0 : 128.0;
        if ((double)m->max_row_len <= similar) {
            // the two streaming passes of K2t, whose gathers stay in LDS: ahead of K2f on every shape measured (1-10 M rows x 8-64
            // entries, profiles/r02_tiled_crossover.log) -- f32 (16 B per entry against CSR's 8) by 31-66 % (C2-uniform 1.14 ms against
            // 1.90), f64 (28 B against 12) by 13-66 % (10 M columns, rows of 8 / 16 / 32 / 64: 0.71 / 1.06 / 1.99 / 3.63 ms against 1.00 /
            // 1.63 / 3.13 / 6.36; 4 M x 16: 0.44 against 0.50).  Needs >= 32 entries per tile (>= 12 measured on f64 with 39 blocks)
            const size_t blocks = blocks_for(m->n_cols, cf_shift_for(m));
            const bool pays = m->dtype == SMH_F32 ? tiled_fits(m)
                              : m->no_split       ? false  // (the parts of a K2s split stay as measured)
                                                  : tiled_fits(m, blocks >= 24 ? 12.0 : 32.0);
            if (pays) return SMH_SPMV_TILED;
            return SMH_SPMV_COLFUSED;
        }
        // skewed rows: K2t folds the entries a long row has in one slice inside its first pass and cuts its row blocks by product
        // counts, so long rows cost it nothing special.  Round 3's form is ahead on both value types: C3 (f64) 1.6 ms against K2s's 2.76
        // and K2c's 3.25; a 3M-row f32 power law (184 slices) 0.23 ms against K2c's 0.62 (tests/test_auto_choice_gpu.py)
        if (!m->no_split && tiled_fits(m, m->dtype == SMH_F64 && blocks_for(m->n_cols, cf_shift_for(m)) >= 24 ? 12.0 : 32.0)) return SMH_SPMV_TILED;  // (the parts of a K2s split stay as measured)
        // ... and a matrix with a minority of long rows is taken apart by row length (K2s)
        static const bool split_off = getenv("SMH_COLBLOCK_SPLIT") && atoi(getenv("SMH_COLBLOCK_SPLIT")) == 0;  // tuning knob
        // ... when K2c's sweeps (per column block and row: one offset, y read and written) weigh as much as the entries
        // themselves: C3 (f64, 10M rows, 20 blocks) 4.0 GB of sweeps for 3.8 GB of entries -> 2.78 against 3.26 ms; a 3M-row
        // f32 power law (6 blocks) 0.22 GB for 0.76 GB -> K2c stays ahead, 0.61 against 0.75 ms
        const double vs = (double)dtype_size(m->dtype);
        const double sweeps = (double)blocks_for(m->n_cols, cb_shift_for(m)) * (double)m->n_rows * (4.0 + 2.0 * vs), entries = (double)m->nnz * (4.0 + vs);
        if (!split_off && !m->no_split && m->split.state != Form::Refused && sweeps >= 0.6 * entries) return SMH_SPMV_COLSPLIT;
        return SMH_SPMV_COLBLOCK;
    }
    const int lanes = mean_lanes(m);
    // short rows (stencils, FEM): the dense CSR-stream kernel (a tile denser than its LDS stage takes several passes)
    const double mean = mean_row(m);
    // ... except rows of 9-12 entries whose columns fit the LDS ring (plan taken at create time): there the ring kernel
    // with 4 lanes wins (banded, 320 M entries, rows of 12: 0.445 vs 0.637 ms; rows of 8: 0.572 vs 0.586 ms, a tie)
    const bool short_ring_rows = mean > 8.0 && m->ring.state == Form::Ready && m->ring.fraction >= 0.5 && m->knobs.use_ring != 0;
    if (mean <= 12.0 && m->max_row_len <= 64 && !short_ring_rows) return SMH_SPMV_STREAM;
    // skew test: the longest row needs >= 8 passes of a group sized for the mean row
    if ((uint64_t)m->max_row_len >= 8ull * 4ull * (uint64_t)lanes && m->max_row_len > 64) return SMH_SPMV_MERGE;
    // long rows whose columns do not fit the LDS ring (plan taken at create time): every kernel is then bound by one
    // cache line per gather; the dense stream kernel loses least up to ~128 entries per row (banded +-8192..32768,
    // 320 M entries: rows of 64 / 128: K1s 0.91 / 1.18 ms, lane-group kernels 1.24-1.42 / 1.34-1.69 ms)
    if (mean > 32.0 && mean <= 128.0 && m->ring.state == Form::Ready && m->ring.fraction < 0.5) return SMH_SPMV_STREAM;
    return SMH_SPMV_VECTOR;
}

// K2c's launches: one K1s sweep per column block, the later ones accumulating into y
static int launch_colblock(const smh_crs *m, const void *x, void *y, hipStream_t s) {
    for (size_t b = 0; b < m->cb.blocks; ++b)
        SMH_TRY(launch_spmv_stream_block(m->dtype, m->cb.off.get() + b * (m->n_rows + 1), m->cb.col.get(), m->cb.val.get(), x, y,
                                         m->n_rows, m->nnz, m->cb.rpt, m->cb.single_pass, b > 0, s));
    return SMH_OK;
}

// one K1s launch over the tiles [t0, t1) with the configuration `c`
static int stream_launch(smh_crs *m, const StreamCfg &c, const void *x, size_t x_len, void *y, hipStream_t s, void *dot_partials,
                         const void *dot_lhs, uint64_t t0, uint64_t t1) {
    // the staged chunks are groups of 4 entries of x fetched with 16-byte loads (f32: one load, f64: two, entries [g, g+2) and
    // [g+2, g+4)); with x itself 16-byte aligned a load that holds at least one valid entry may reach past x_len but never past the
    // 16-byte block (hence page, hence allocation granule) its valid entry lies in.  f32: the last chunk holds a valid entry when
    // x_len rounded up to 4 reaches stream_xs_end; f64: its SECOND load starts at stream_xs_end - 2 and must hold a valid entry
    // too (x_len >= stream_xs_end - 1), else the gathers stay global
    const bool xs_ok = ((m->dtype == SMH_F64 ? x_len + 1 : ((x_len + 3) & ~(size_t)3)) >= (size_t)m->codes.xs_end) &&
                       (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
    if (c.direct) {
        if (xs_ok && c.xs)
            return launch_spmv_stream_xd(m->dtype, m->d_val, x, y, m->n_rows, dot_partials, c.code, c.cwin, c.len8, c.tbase, dot_lhs, s,
                                         c.xs, t0, t1, c.dict, c.dict_high);
        // stage offsets mean nothing without the stage: this call streams the u32 columns (same arithmetic, same order)
        return launch_spmv_stream(m->dtype, m->d_off, m->d_col, m->d_val, x, y, m->n_rows, m->nnz, m->owns, c.rpt, c.single_pass,
                                  dot_partials, nullptr, nullptr, nullptr, nullptr, dot_lhs, s, false, 0, t0, t1);
    }
    return launch_spmv_stream(m->dtype, m->d_off, m->d_col, m->d_val, x, y, m->n_rows, m->nnz, m->owns, c.rpt, c.single_pass,
                              dot_partials, c.code, c.cwin, c.len8, c.tbase, dot_lhs, s, c.small, xs_ok ? c.xs : 0, t0, t1);
}

// one K1r launch over the plan's row ranges [b0, b1) (dot_partials: the DOT form, whole plan only -- see launch_spmv_ring2)
// resident_out, threads_out (both or neither) / form_out: a query instead of the launch -- launch_spmv_ring2's, and which form of the
// kernel the launch would take: 0 = the three bodies, 1 = REGK, 2 = the all-regular form (smh_crs_ring_launch_form)
static int launch_ring(smh_crs *m, const void *x, void *y, hipStream_t s, void *dot_partials = nullptr, unsigned b0 = 0, unsigned b1 = ~0u,
                       int *resident_out = nullptr, int *threads_out = nullptr, int *form_out = nullptr) {
    // regular phases compute their row offsets from the plan's table, where it applies (RingPlan::reg_applies) and the ring phases
    // stream a narrow column form; SMH_RING_REGULAR=0 (tuning knob, read per launch like SMH_RING_COL12): no table, every phase
    // loads its offsets
    const char *reg_env = getenv("SMH_RING_REGULAR");
    const bool reg_off = reg_env && strcmp(reg_env, "auto") != 0 && atoi(reg_env) == 0;
    const uint32_t *reg_len = m->ring.reg_applies && !reg_off && (m->ring.lo8.get() || m->ring.rec16.get() || m->ring.col16.get()) ? m->ring.reg_len.get() : nullptr;
    // the chunk records (vector_uses_ring keeps them only for a plan and a setting that pass reg_len) with 2^E, an exact power of two
    const RingCol12 c12{m->ring.lo8.get(), m->ring.hdr.get(), m->ring.escapes.get(), m->ring.rec16.get(),
                        m->ring.rec16.get() ? ldexpf(1.0f, m->ring.v24_exp) : 0.0f};
    // owned arrays are padded to a multiple of 4 entries; borrowed ones may end inside a 16-B chunk
    const bool padded = m->owns || m->nnz % 4 == 0;
    const int lanes = auto_lanes(m), chunks = auto_chunks(m);
    // a plan whose phases are ALL regular (RingPlan::reg_all), f32 on the single-window ring of kRingEntries columns, no DOT (the
    // order of inner_prod's sum goes with the 8 waves of a 512-thread workgroup): the all-regular form, 24 wavefronts per CU instead
    // of 16, same y.  SMH_RING_ALLREG=0 (tuning knob, read per launch): the REGK kernel as before.
    const char *all_env = getenv("SMH_RING_ALLREG");
    const bool all_off = all_env && strcmp(all_env, "auto") != 0 && atoi(all_env) == 0;
    const bool allreg = reg_len && m->ring.reg_all && !dot_partials && m->dtype == SMH_F32 && m->ring.entries == (unsigned)kRingEntries &&
                        m->ring.bands == 1 && !all_off && ring2_allreg_has(lanes, chunks);
    if (form_out) *form_out = allreg ? 2 : reg_len ? 1 : 0;
    if (allreg)
        return launch_spmv_ring2_allreg(lanes, chunks, m->d_off, m->d_col, m->ring.col16.get(), c12, (const float *)m->d_val, (const float *)x,
                                        (float *)y, m->n_rows, m->nnz, padded, m->ring.blocks, m->ring.phase_ptr.get(), m->ring.phases.get(), s,
                                        b0, b1, reg_len, resident_out, threads_out);
    return launch_spmv_ring2(m->dtype, lanes, chunks, m->d_off, m->d_col, m->ring.col16.get(), c12, m->d_val, x, y, m->n_rows, m->nnz,
                             padded, m->ring.blocks, m->ring.phase_ptr.get(), m->ring.phases.get(), m->ring.entries,
                             m->ring.bands, s, dot_partials, b0, b1, reg_len, resident_out, threads_out);
}

// Can y = A x also leave the partial sums of x.y (CG's p.Ap) in its epilogue?  Only the K1s kernel does;
// returns the number of partials it would write (0: not fused -- run a separate dot).
// any_lhs: the dot is taken with a vector of its own (n_rows entries; SparseMatrix::inner_prod) instead of x itself, so
// the matrix need not be square
size_t spmv_fused_dot_partials(smh_crs *m, size_t x_len, int variant, bool any_lhs) {
    if (const char *e = getenv("SMH_CG_FUSED_DOT")) {  // tuning knob: 0 = always the separate dot
        if (atoi(e) == 0) return 0;
    }
    if (resolve_variant(m, variant) != SMH_SPMV_STREAM) return 0;
    if (!any_lhs && (m->n_rows != m->n_cols || x_len < m->n_rows)) return 0;
    StreamCfg c;
    if (stream_cfg(m, &c) != SMH_OK) return 0;
    return stream_tiles(m->n_rows, c.rpt);
}

// every product gathers x[column]: an x that the largest column (a create-time statistic) does not index is refused
static int x_covers_columns(const smh_crs *m, size_t x_len) {
    if (m->nnz > 0 && (size_t)m->max_col >= x_len)
        return fail(SMH_ERR_INDEX_RANGE, "index out of bounds: the len is %zu but the index is %u", x_len, m->max_col);
    return SMH_OK;
}

// ---- which derived forms a variant runs on ---------------------------------------------------------------------------------------
// what one call has resolved: the variant, and what its builders report to the launch
struct Resolved {
    int v = SMH_SPMV_AUTO;
    bool ring = false;  // VECTOR: runs as K1r
    StreamCfg stream;   // STREAM
};

// The forms that variant r->v runs on, built on first use: the one table behind the product and smh_crs_prepare.  eager (prepare):
// the K1s code array is also brought into the form the current settings ask for (a launch path only reads it: see stream_cfg), and
// a Ready split prepares its two parts.
static int build_forms(smh_crs *m, Resolved *r, bool eager) {
    switch (r->v) {
        case SMH_SPMV_VECTOR: return vector_uses_ring(m, &r->ring);  // builds the K1r phase plan when the ring is used
        case SMH_SPMV_SEQ: return SMH_OK;
        case SMH_SPMV_STREAM: return stream_cfg(m, &r->stream, eager);  // code tables
        case SMH_SPMV_COLSPLIT:
            SMH_TRY(ensure_split(m));
            if (m->split.state != Form::Ready) return ensure_colblock(m);  // not worth splitting: the per-block launches
            if (eager) {
                SMH_TRY(smh_crs_prepare(m->split.short_part, SMH_SPMV_AUTO));
                return smh_crs_prepare(m->split.long_part, SMH_SPMV_AUTO);
            }
            return SMH_OK;
        case SMH_SPMV_COLFUSED:
            SMH_TRY(ensure_colfused(m));
            // (not Ready: a (row, block) pair with more than 255 entries -- the per-block launches)
            return (m->cf.state == Form::Ready) ? SMH_OK : ensure_colblock(m);
        case SMH_SPMV_COLBLOCK: return ensure_colblock(m);
        case SMH_SPMV_TILED: return tiled_build(m);
        case SMH_SPMV_MERGE: return ensure_merge_ws(m);
        default: return fail(SMH_ERR_INVALID, "unknown SpMV variant %d", r->v);
    }
}

// Resolve, then build.  AUTO chose a plan and its lazy build failed (scratch out of memory, ...; K2t needs ~5 x 4 B x nnz of scratch,
// a copy of the entries and a product buffer): a failed ensure_split or tiled_build leaves its form Refused, AUTO's rules read
// that as "does not apply" and resolve differently -- K2c / K2f / K1 can still serve -- so the error is forgotten and the next
// choice is built, within this call.  Every other builder assigns its form only when it is complete: its failure changes no
// resolution and is returned.  A wrong column index (SMH_ERR_INDEX_RANGE) is the caller's to hear of.  Each round turns one form
// Refused, so the loop ends.
static int resolve_and_build(smh_crs *m, int variant, bool eager, Resolved *r) {
    for (;;) {
        r->v = resolve_variant(m, variant);
        const int rc = build_forms(m, r, eager);
        if (rc == SMH_OK || variant != SMH_SPMV_AUTO || rc == SMH_ERR_INDEX_RANGE || resolve_variant(m, variant) == r->v) return rc;
        clear_error();
    }
}

int prepare_forms(smh_crs *m, int variant) {
    Resolved r;
    return resolve_and_build(m, variant, true, &r);
}

// enqueue y = A x on stream s (device pointers); dot_partials (optional, K1s only): see above
int spmv_enqueue(smh_crs *m, const void *x, size_t x_len, void *y, int variant, hipStream_t s, void *dot_partials, const void *dot_lhs) {
    SMH_TRY(x_covers_columns(m, x_len));
    Resolved r;
    SMH_TRY(resolve_and_build(m, variant, false, &r));
    switch (r.v) {
        case SMH_SPMV_VECTOR:
            if (r.ring) return launch_ring(m, x, y, s);
            return launch_spmv_vector(m->dtype, auto_lanes(m), m->d_off, m->d_col, m->d_val, x, y, m->n_rows, m->nnz, s);
        case SMH_SPMV_SEQ:
            return launch_spmv_seq(m->dtype, m->d_off, m->d_col, m->d_val, x, y, m->n_rows, s);
        case SMH_SPMV_STREAM:
            return stream_launch(m, r.stream, x, x_len, y, s, dot_partials, dot_lhs, 0, ~uint64_t(0));
        case SMH_SPMV_COLSPLIT:
            if (m->split.state == Form::Ready) {
                // The two parts lean on different resources (LONG: the L2 gather path; SHORT: HBM streams and latency), which
                // suggests running LONG on a stream of its own beside SHORT (fork and join by events).  Measured on C3, one box:
                // 2.90 ms overlapped against 2.79 ms back to back -- K2f sizes its rounds to the whole chip and the blocks of
                // x of the two parts evict each other -- so it is a knob, off by default (SMH_COLSPLIT_OVERLAP=1)
                static const bool overlap = getenv("SMH_COLSPLIT_OVERLAP") && atoi(getenv("SMH_COLSPLIT_OVERLAP")) != 0;
                hipStream_t sl = overlap ? m->split.side : s;
                if (overlap) {
                    SMH_HIP(hipEventRecord(m->split.fork, s));
                    SMH_HIP(hipStreamWaitEvent(sl, m->split.fork, 0));
                }
                SMH_TRY(spmv_enqueue(m->split.long_part, x, x_len, m->split.y.get(), SMH_SPMV_AUTO, sl));  // the long rows, compacted
                if (overlap) SMH_HIP(hipEventRecord(m->split.join, sl));
                SMH_TRY(spmv_enqueue(m->split.short_part, x, x_len, y, SMH_SPMV_AUTO, s));             // every row (0 for the long ones)
                if (overlap) SMH_HIP(hipStreamWaitEvent(s, m->split.join, 0));
                return launch_split_scatter(m->dtype, m->split.rows.get(), m->split.y.get(), m->split.n_long, y, s);
            }
            return launch_colblock(m, x, y, s);
        case SMH_SPMV_COLFUSED:
            if (m->cf.state == Form::Ready)
                return launch_spmv_colfused(m->dtype, m->cf.rt, m->cf.tile_row.get(), m->cf.tiles, m->cf.seg.get(), m->cf.cnt.get(), m->cf.col.get(), m->cf.val.get(),
                                            x, y, m->n_rows, m->nnz, (uint32_t)m->cf.blocks, m->device, s);
            [[fallthrough]];
        case SMH_SPMV_COLBLOCK:
            return launch_colblock(m, x, y, s);
        case SMH_SPMV_TILED:
            return launch_spmv_tiled(m, x, x_len, y, s);
        case SMH_SPMV_MERGE:
            return launch_spmv_merge(m->dtype, m->d_off, m->d_col, m->d_val, x, y, m->n_rows, m->nnz, m->merge.n_tiles,
                                     m->merge.tile_row.get(), m->merge.tile_nz.get(), m->merge.carry_row.get(), m->merge.carry_val.get(), s);
        default:
            return fail(SMH_ERR_INVALID, "unknown SpMV variant %d", variant);
    }
}

// ---- products of a run of rows (par_step.hip, par_cg.hip: a block's boundary rows before / after its interior ones) --------------------------
// The kernels whose launches decompose by rows WITHOUT changing any row's arithmetic: K1s (256-row tiles; bit-exact anyway) and
// K1r (the plan's row ranges; a row's lanes, chunks and order do not depend on which workgroup takes it).  *gran_out = the row
// granularity a run must respect (0: this handle's kernel for `variant` cannot be launched by parts).
// ... with what the launch of a run needs besides (*r)
static int resolve_rows(smh_crs *m, int variant, Resolved *r, size_t *gran_out) {
    *gran_out = 0;
    if (m->n_rows == 0) return SMH_OK;
    r->v = resolve_variant(m, variant);
    if (r->v == SMH_SPMV_STREAM) {
        SMH_TRY(stream_cfg(m, &r->stream));
        *gran_out = (size_t)kStreamRows * (size_t)r->stream.rpt;
    } else if (r->v == SMH_SPMV_VECTOR) {
        SMH_TRY(vector_uses_ring(m, &r->ring));
        if (r->ring && m->ring.blocks) {
            const size_t n_tiles = (m->n_rows + 63) / 64;
            *gran_out = ((n_tiles + m->ring.blocks - 1) / m->ring.blocks) * 64;  // build_ring_plan: tiles per row range
        }
    }
    return SMH_OK;
}
int spmv_rows_granularity(smh_crs *m, int variant, size_t *gran_out) {
    Resolved r;
    return resolve_rows(m, variant, &r, gran_out);
}

// y[row0, row1) = (A x)[row0, row1): row0 a multiple of the granularity, row1 too or == n_rows.  Same kernels, same arithmetic as
// the whole product.  dot_partials: as spmv_enqueue (K1s only; the tiles of the run write their partials, the others are left alone)
int spmv_enqueue_rows(smh_crs *m, const void *x, size_t x_len, void *y, int variant, hipStream_t s, size_t row0, size_t row1,
                      void *dot_partials, const void *dot_lhs) {
    SMH_TRY(x_covers_columns(m, x_len));
    if (row1 > m->n_rows) row1 = m->n_rows;
    if (row0 >= row1) return SMH_OK;
    Resolved r;
    size_t gran = 0;
    SMH_TRY(resolve_rows(m, variant, &r, &gran));
    if (gran == 0 || row0 % gran || (row1 % gran && row1 != m->n_rows))
        return fail(SMH_ERR_INVALID, "rows [%zu, %zu) cannot be launched on their own (granularity %zu)", row0, row1, gran);
    if (r.v == SMH_SPMV_STREAM)
        return stream_launch(m, r.stream, x, x_len, y, s, dot_partials, dot_lhs, row0 / gran, (row1 + gran - 1) / gran);
    if (dot_partials) return fail(SMH_ERR_INVALID, "a product by parts with the dot epilogue needs the CSR-stream kernel");
    return launch_ring(m, x, y, s, nullptr, (unsigned)(row0 / gran), (unsigned)((row1 + gran - 1) / gran));
}

// The same for a SHORT run of rows (a partition block's boundary rows: a few thousand), any row0 / row1.  One ring workgroup walks its
// ~6500 rows in ~100 us whatever else the chip does -- the ring kernel gets its rate from 512 of them at once -- so two boundary
// launches were 200 us of a rank's 340 us step (profiles/r04_par_boundary_rows_k1.log).  The plain lane-group kernel K1 (same lanes,
// same chunk grid and lane layout, same order of FMAs; x through L1 / L2 instead of the LDS ring) gives the ring kernel's bits in
// both value types (tests/test_ring_gpu.py::test_k1_is_k1r_bit_for_bit, and every overlap-on / overlap-off comparison of the
// partition tests), and a short run is a hundred small workgroups: microseconds.  Everything else goes the way of spmv_enqueue_rows.
int spmv_enqueue_rows_short(smh_crs *m, const void *x, size_t x_len, void *y, int variant, hipStream_t s, size_t row0, size_t row1) {
    static const bool off = getenv("SMH_PAR_BOUNDARY_K1") && atoi(getenv("SMH_PAR_BOUNDARY_K1")) == 0;  // tuning knob
    if (row1 > m->n_rows) row1 = m->n_rows;
    if (row0 >= row1) return SMH_OK;
    if (!off && resolve_variant(m, variant) == SMH_SPMV_VECTOR && auto_lanes(m) >= 4 && row1 - row0 <= (size_t)1 << 20) {
        bool ring = false;
        SMH_TRY(vector_uses_ring(m, &ring));
        if (ring) {
            SMH_TRY(x_covers_columns(m, x_len));
            return launch_spmv_vector(m->dtype, auto_lanes(m), m->d_off + row0, m->d_col, m->d_val, x, (char *)y + row0 * dtype_size(m->dtype), row1 - row0,
                                      m->nnz, s);
        }
    }
    return spmv_enqueue_rows(m, x, x_len, y, variant, s, row0, row1, nullptr, nullptr);
}

// ---- lhs^T (A rhs) (smh_crs_inner_prod*) -------------------------------------------------------------------------------------------
// The product by the matrix's own kernel on the handle's stream, folded with lhs (n_rows entries) into *res: inside the kernel where
// it has a dot form, else y = A rhs into the handle's y staging and the two-stage dot.  scratch: kReducePartials partials.
// In all three routes a row without entries is no term of the sum (the reference reads lhs[i] inside the entry loop), whatever lhs
// holds there; the summation order of each route is a CPU model's bit for bit (tests/inner_prod_model.py).
int spmv_inner_prod(smh_crs *m, const void *d_lhs, const void *d_rhs, size_t rhs_len, int variant, void *scratch, void *res) {
    const size_t vs = dtype_size(m->dtype);
    const size_t n_dot = spmv_fused_dot_partials(m, rhs_len, variant, true);
    bool ring = false;
    if (!n_dot && resolve_variant(m, variant) == SMH_SPMV_VECTOR) SMH_TRY(vector_uses_ring(m, &ring));
    if (ring) {
        // K1r: the lanes that would store a row's sum multiply it by lhs[row] instead and the blocks leave partial sums
        SMH_TRY(x_covers_columns(m, rhs_len));
        SMH_TRY(m->stage_y.ensure_cap(((size_t)m->ring.blocks + 1) * vs));
        SMH_TRY(launch_ring(m, d_rhs, const_cast<void *>(d_lhs), m->stream, m->stage_y.d.get()));
        SMH_TRY(launch_fold2(m->dtype, m->stage_y.d.get(), (size_t)m->ring.blocks + 1, scratch, res, m->stream));
    } else if (n_dot) {
        // K1s: lhs_i * (A rhs)_i summed per tile in the SpMV's epilogue -- no y vector, no second pass; the tile partials
        // are folded by the two small reduction kernels
        SMH_TRY(m->stage_y.ensure_cap(n_dot * vs));  // (the staging buffer holds the partials here)
        SMH_TRY(spmv_enqueue(m, d_rhs, rhs_len, nullptr, variant, m->stream, m->stage_y.d.get(), d_lhs));
        SMH_TRY(launch_fold2(m->dtype, m->stage_y.d.get(), n_dot, scratch, res, m->stream));
    } else {
        SMH_TRY(m->stage_y.ensure_cap(m->n_rows * vs));
        SMH_TRY(spmv_enqueue(m, d_rhs, rhs_len, m->stage_y.d.get(), variant, m->stream));
        SMH_TRY(launch_dot(m->dtype, d_lhs, m->stage_y.d.get(), m->n_rows, scratch, res, m->stream, m->d_off));  // (rows with entries only)
    }
    return SMH_OK;
}

// ---- the entry points: prepare, the products, inner_prod --------------------------------------------------------------------------
// lhs^T (A rhs) on device vectors, by one of three routes (spmv_inner_prod above):
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

}  // namespace smh

using namespace smh;

extern "C" {

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

int smh_crs_ring_launch_form(smh_crs *m, int *form_out, int *threads_out, int *resident_per_cu_out) {
    if (!m || !form_out || !threads_out || !resident_per_cu_out) return fail(SMH_ERR_INVALID, "NULL argument");
    *form_out = -1;
    *threads_out = *resident_per_cu_out = 0;
    bool ring = false;
    SMH_TRY(vector_uses_ring(m, &ring));  // (builds the forms a product would)
    if (!ring) return SMH_OK;
    return launch_ring(m, nullptr, nullptr, nullptr, nullptr, 0, ~0u, resident_per_cu_out, threads_out, form_out);
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

int smh_crs_spmv_vec(smh_crs *m, const smh_vec *x, smh_vec *y, int variant) {
    if (!m || !x || !y) return fail(SMH_ERR_INVALID, "NULL handle");
    if (x->dtype != m->dtype || y->dtype != m->dtype) return fail(SMH_ERR_INVALID, "dtype mismatch");
    if (y->n != m->n_rows) return fail(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
    SMH_TRY(spmv_enqueue(m, x->d, x->n, y->d, variant, m->stream));
    SMH_HIP(hipStreamSynchronize(m->stream));
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

}  // extern "C"
