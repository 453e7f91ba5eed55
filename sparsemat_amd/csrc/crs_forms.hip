// crs_forms.hip -- what a CRS handle derives lazily from its own arrays (the forms of internal.hpp) and when it goes: the ensure_*
// builders, the K1s configuration, invalidate.  Host-side logic only.  (K2t's builder is tiled_build, spmv_tiled.hip.)
#include <cstdlib>
#include <cstring>
#include <vector>

#include "crs_forms.hpp"
#include "ring_val24.hpp"

namespace smh {

// defined in the kernel files
void build_ring_plan(size_t n_rows, size_t ring_entries, const uint32_t *cmin, const uint32_t *cmax, size_t n_blocks,
                     uint32_t noring_mode, std::vector<uint32_t> &phase_ptr, std::vector<RingPhase> &phases,
                     double *ring_row_fraction);
void build_ring_plan_banded(size_t n_rows, size_t ring_entries, const uint32_t *win, size_t n_blocks, uint32_t noring_mode,
                            std::vector<uint32_t> &phase_ptr, std::vector<RingPhase> &phases, double *ring_row_fraction);

int ensure_merge_ws(smh_crs *m) {
    if (m->merge.state == Form::Ready) return SMH_OK;
    MergeTable t;
    const uint64_t items = (uint64_t)m->n_rows + (uint64_t)m->nnz;
    t.n_tiles = (size_t)((items + kMergeTile - 1) / kMergeTile);
    if (t.n_tiles) {
        SMH_TRY(t.tile_row.alloc(t.n_tiles + 1));
        SMH_TRY(t.tile_nz.alloc(t.n_tiles + 1));
        SMH_TRY(t.carry_row.alloc(t.n_tiles));
        SMH_TRY(t.carry_val.alloc(t.n_tiles * dtype_size(m->dtype)));
        SMH_TRY(launch_merge_table(m->d_off, m->n_rows, m->nnz, t.n_tiles, t.tile_row.get(), t.tile_nz.get(), m->stream));
        SMH_HIP(hipStreamSynchronize(m->stream));
    }
    t.state = Form::Ready;
    m->merge = std::move(t);
    return SMH_OK;
}

// K1r: inspector pass + host plan, once per matrix
// with_bands = false: the single-window plans only (what AUTO needs at create time from a matrix with rows too short
// for the lane-group kernels anyway); the banded attempt -- an inspector pass, a table readback, a host pass over the
// tiles: ~50 ms at 134 M rows -- then waits until the VECTOR family is actually used.
int ensure_ring_plan(smh_crs *m, bool with_bands) {
    if (m->ring.state == Form::Ready && (!with_bands || m->ring.bands_tried)) return SMH_OK;
    m->ring = RingPlan();  // planned without the banded attempt: plan again, completely (the old plan goes first: no higher peak)
    RingPlan p;
    p.bands_tried = with_bands;
    const size_t n_tiles = (m->n_rows + 63) / 64;
    int cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, m->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    // Two 512-thread blocks (64 KiB of LDS each) are resident per CU; the row range is cut into 3x as many
    // blocks so that the hardware dispatcher evens out the tail (round 1, on C2: 2/CU 0.4245 ms, 8/CU 0.404 ms, 24/CU 0.402 ms;
    // round 3, the final kernel: 4 / 6 / 8 / 12 / 16 per CU 0.360 / 0.357 / 0.361 / 0.364 / 0.371 ms, and 0.350-0.353 against
    // 0.356-0.359 ms for 6 against 8 on banded and window matrices, f64 level -- profiles/r03_k1r_blocks_per_cu.log)
    unsigned per_cu = 6;
    if (const char *e = getenv("SMH_RING_BLOCKS_PER_CU")) {  // tuning knob
        const int v = atoi(e);
        if (v >= 1 && v <= 64) per_cu = (unsigned)v;
    }
    unsigned blocks = per_cu * (unsigned)cus;
    blocks = (blocks + 7u) & ~7u;
    std::vector<uint32_t> cmin(n_tiles), cmax(n_tiles);
    if (n_tiles) {
        Scratch scr;
        uint32_t *d_min = nullptr, *d_max = nullptr;
        SMH_TRY(scr.alloc(&d_min, n_tiles));
        SMH_TRY(scr.alloc(&d_max, n_tiles));
        SMH_TRY(read_back(d_min, cmin.data(), n_tiles, m->stream, [&](uint32_t *) -> int {
            SMH_TRY(launch_tile_span(m->d_off, m->d_col, m->n_rows, n_tiles, d_min, d_max, m->stream));
            SMH_HIP(hipMemcpyAsync(cmax.data(), d_max, n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
            return SMH_OK;
        }));
    }
    double span_fraction = 0.0;
    {  // locality statistic for AUTO: mean column span of a 64-row tile relative to n_cols
        double acc = 0.0;
        size_t used = 0;
        for (size_t t = 0; t < n_tiles; ++t)
            if (cmin[t] <= cmax[t]) { acc += (double)(cmax[t] - cmin[t]) + 1.0; ++used; }
        span_fraction = used && m->n_cols ? acc / (double)used / (double)m->n_cols : 0.0;
    }
    std::vector<uint32_t> phase_ptr;
    std::vector<RingPhase> phases;
    // Phases without a ring gather through L1/L2.  Bypassing L1 (nontemporal gathers, mode 2) was measured
    // SLOWER on both kinds of such matrices (uniform columns 6.29 vs 5.48 ms, 512^3 Laplacian 3.77 vs 2.68 ms),
    // so it stays a tuning knob.  The uniform case is bound by the per-CU L1 miss path (rocprofv3: TA busy 78 %,
    // 71 % of wave cycles stalled on VMEM issue, ~59 G gathers/s) -- only column blocking would change that.
    uint32_t noring_mode = 0;
    if (const char *e = getenv("SMH_GATHER_NT")) noring_mode = atoi(e) ? 2u : 0u;
    build_ring_plan(m->n_rows, kRingEntries, cmin.data(), cmax.data(), blocks, noring_mode, phase_ptr, phases,
                    &p.fraction);
    p.entries = kRingEntries;
    // f32 rows that do not fit 16384 columns but fit 32768: the wide ring (128 KiB of LDS, one 1024-thread block per CU
    // like f64, so half as many blocks).  Rows of 64 entries in a +-8192 band: 0.90 ms (K1s) -> see DESIGN.md.
    const char *wide_env = getenv("SMH_RING_WIDE");  // tuning knob: 0 = never
    if (m->dtype == SMH_F32 && p.fraction < 0.5 && !(wide_env && atoi(wide_env) == 0)) {
        std::vector<uint32_t> phase_ptr_w;
        std::vector<RingPhase> phases_w;
        double frac_w = 0.0;
        const unsigned blocks_w = ((blocks / 2) + 7u) & ~7u;
        build_ring_plan(m->n_rows, kRingEntriesWide, cmin.data(), cmax.data(), blocks_w, noring_mode, phase_ptr_w, phases_w, &frac_w);
        if (frac_w >= 0.5) {
            phase_ptr.swap(phase_ptr_w);
            phases.swap(phases_w);
            p.fraction = frac_w;
            p.entries = kRingEntriesWide;
            blocks = blocks_w;
        }
    }
    // Still mostly outside the ring: rows that reference a few narrow column intervals far apart (stencils on
    // structured grids) get the BANDED ring -- four bands of a quarter of the ring, one per interval of the tile.
    const char *band_env = getenv("SMH_RING_BANDS");  // tuning knob: 0 = never
    if (with_bands && p.fraction < 0.5 && n_tiles && m->nnz && !(band_env && atoi(band_env) == 0)) {
        const unsigned sizes[2] = {(unsigned)kRingEntries, (unsigned)kRingEntriesWide};
        const int n_sizes = m->dtype == SMH_F32 && !(wide_env && atoi(wide_env) == 0) ? 2 : 1;
        std::vector<uint32_t> h_win(n_tiles * 8);
        Scratch scr;
        uint32_t *d_count = nullptr;
        SMH_TRY(p.win.alloc(n_tiles * 8));
        SMH_TRY(scr.alloc(&d_count, 1));
        for (int si = 0; si < n_sizes && p.bands == 1; ++si) {
            const unsigned ring = sizes[si];
            SMH_TRY(read_back(p.win.get(), h_win.data(), n_tiles * 8, m->stream, [&](uint32_t *d_win) {
                return launch_tile_intervals(m->d_off, m->d_col, m->n_rows, 64, ring / 4, d_win, d_count, m->stream);
            }));
            std::vector<uint32_t> phase_ptr_b;
            std::vector<RingPhase> phases_b;
            double frac_b = 0.0;
            const unsigned blocks_b = ring == (unsigned)kRingEntries || m->dtype == SMH_F64 ? blocks : ((blocks / 2) + 7u) & ~7u;
            build_ring_plan_banded(m->n_rows, ring, h_win.data(), blocks_b, noring_mode, phase_ptr_b, phases_b, &frac_b);
            if (frac_b >= 0.5 && frac_b > p.fraction) {
                phase_ptr.swap(phase_ptr_b);
                phases.swap(phases_b);
                p.fraction = frac_b;
                p.entries = ring;
                p.bands = 4;
                blocks = blocks_b;
            }
        }
        if (p.bands != 4) p.win.reset();  // (kept with a banded plan: the 16-bit ring slots are built from it on first use)
    }
    SMH_TRY(p.phase_ptr.alloc(phase_ptr.size()));
    SMH_TRY(p.phases.alloc(phases.size() + 1));
    SMH_HIP(hipMemcpy(p.phase_ptr.get(), phase_ptr.data(), phase_ptr.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!phases.empty())
        SMH_HIP(hipMemcpy(p.phases.get(), phases.data(), phases.size() * sizeof(RingPhase), hipMemcpyHostToDevice));
    // which ring phases of the plan that was taken (16384 slots, 32768 slots or banded) have rows of one length: those compute their
    // row offsets instead of streaming them (k_spmv_ring2's REG body).  One read of the offsets, here, so that no launch path builds it.
    // The kernel that reads the table has the two ring bodies only (see there), so it applies to plans without global-gather phases.
    SMH_TRY(p.reg_len.alloc(phases.size() + 1));
    if (!phases.empty()) {
        std::vector<uint32_t> h_reg(phases.size());
        SMH_TRY(read_back(p.reg_len.get(), h_reg.data(), phases.size(), m->stream, [&](uint32_t *d_reg) {
            return launch_ring_regular(m->d_off, p.phases.get(), phases.size(), d_reg, m->stream);
        }));
        // all_regular: a phase without rows (reg_len 0: k_ring_regular has no row to take L from) does not count against it -- the
        // regular body returns for it before it reads anything (phase_rows: `base >= re`), as it does in the REGK kernel's other body
        bool ring_only = true, any_regular = false, all_regular = true;
        for (size_t i = 0; i < phases.size(); ++i) {
            ring_only = ring_only && phases[i].use_ring == 1u;
            any_regular = any_regular || h_reg[i] != 0u;
            all_regular = all_regular && (h_reg[i] != 0u || phases[i].row_end == phases[i].row_begin);
        }
        p.reg_applies = ring_only && any_regular;
        p.reg_all = p.reg_applies && all_regular;
    }
    p.blocks = blocks;
    p.n_phases = phases.size();
    p.state = Form::Ready;
    m->ring = std::move(p);
    m->span_fraction = span_fraction;
    return SMH_OK;
}

// The column-blocked / tiled builders size their tables from n_cols and index them with col >> shift (col / slice): a handle
// created without validation (smh_crs_create_dev's default) may hold columns >= n_cols, which would walk past those tables.
// Every such build starts here (max_col is a create-time statistic: no per-call cost).
int columns_within_n_cols(const smh_crs *m, const char *what) {
    if (m->nnz && (size_t)m->max_col >= m->n_cols)
        return fail(SMH_ERR_INDEX_RANGE, "%s: column index %u >= n_cols %zu", what, m->max_col, m->n_cols);
    return SMH_OK;
}

// K2c: build the column-blocked copy, once per matrix
int ensure_colblock(smh_crs *m) {
    if (m->cb.state == Form::Ready) return SMH_OK;
    SMH_TRY(columns_within_n_cols(m, "column-blocked variant"));
    const size_t blocks = blocks_for(m->n_cols, cb_shift_for(m));
    if (blocks == 0 || blocks > 128)
        return fail(SMH_ERR_INVALID, "column-blocked variant: %zu column blocks (supported: 1..128)", blocks);
    if ((uint64_t)blocks * (m->n_rows + 1) >= (1ull << 34)) return fail(SMH_ERR_OOM, "column-blocked offsets too large");
    ColBlock c;
    c.shift = cb_shift_for(m);
    uint32_t *off2 = nullptr, *col2 = nullptr;
    void *val2 = nullptr;
    SMH_TRY(build_colblock(m->dtype, m->d_off, m->d_col, m->d_val, m->n_rows, m->nnz, c.shift, blocks, &off2, &col2, &val2, m->stream));
    c.off.reset(off2);
    c.col.reset(col2);
    c.val.reset((char *)val2);
    c.blocks = blocks;
    // tile height of the K1s launches: the tallest of 2048/1024/512/256 rows whose busiest tile fits the LDS stage
    Scratch scr;
    uint32_t *d_max = nullptr;
    SMH_TRY(scr.alloc(&d_max, 1));
    int rpt = 8;
    uint32_t worst = 0;
    for (; rpt >= 1; rpt >>= 1) {
        worst = 0;
        for (size_t b = 0; b < blocks; ++b) {
            uint32_t h = 0;
            SMH_TRY(read_back(d_max, &h, 1, m->stream, [&](uint32_t *d) {
                return launch_stream_max_tile(c.off.get() + b * (m->n_rows + 1), m->n_rows, (size_t)kStreamRows * rpt, d, m->stream);
            }));
            worst = h > worst ? h : worst;
        }
        if (worst <= (uint32_t)kStreamCap || rpt == 1) break;
    }
    c.rpt = rpt < 1 ? 1 : rpt;
    c.single_pass = worst <= (uint32_t)kStreamCap;  // else 256-row tiles, several passes where needed
    c.state = Form::Ready;
    m->cb = std::move(c);
    return SMH_OK;
}

// K2f: build the fused column-blocked copy, once per matrix (Refused afterwards: not describable -> K2c)
int ensure_colfused(smh_crs *m) {
    if (m->cf.state != Form::NotTried) return SMH_OK;
    SMH_TRY(columns_within_n_cols(m, "fused column-blocked variant"));
    const size_t blocks = blocks_for(m->n_cols, cf_shift_for(m));
    if (blocks > 255) return fail(SMH_ERR_INVALID, "fused column-blocked variant: %zu column blocks (supported: 1..255)", blocks);
    uint32_t rt = 16;
    if (const char *e = getenv("SMH_COLFUSED_RT")) {  // tuning knob: rows per lane, 8 or 16
        if (atoi(e) == 8) rt = 8;
    }
    ColFused c;
    bool fits = false;
    uint32_t *tile_row = nullptr, *seg = nullptr, *col2 = nullptr;
    uint8_t *cnt = nullptr;
    void *val2 = nullptr;
    SMH_TRY(build_colfused(m->dtype, m->d_off, m->d_col, m->d_val, m->n_rows, m->nnz, cf_shift_for(m), blocks, rt, &c.tiles,
                           &tile_row, &seg, &cnt, &col2, &val2, &fits, m->stream));
    c.tile_row.reset(tile_row);
    c.seg.reset(seg);
    c.cnt.reset(cnt);
    c.col.reset(col2);
    c.val.reset((char *)val2);
    c.shift = cf_shift_for(m);
    c.blocks = blocks;
    c.rt = rt;
    c.state = fits ? Form::Ready : Form::Refused;
    m->cf = std::move(c);
    return SMH_OK;
}

// K2s: the row-length split, once per matrix (Refused afterwards: not worth it / not possible -> K2c)
const uint32_t kSplitMinLong = 64;  // rows of this many entries and more form the LONG part
int ensure_split(smh_crs *m) {
    if (m->split.state != Form::NotTried) return SMH_OK;
    SMH_TRY(columns_within_n_cols(m, "row-length split"));
    m->split.state = Form::Refused;  // until the build below is complete: a split that failed or does not pay is not tried again
    if (m->no_split || m->n_rows == 0 || m->nnz == 0) return SMH_OK;
    RowSplit sp;
    size_t nnz_long = 0;
    uint32_t *rows = nullptr;
    CrsArrays long_part, short_part;
    SMH_TRY(build_colsplit(m->dtype, m->d_off, m->d_col, m->d_val, m->n_rows, m->nnz, kSplitMinLong, &sp.n_long, &nnz_long, &rows, &long_part.off,
                           &long_part.col, &long_part.val, &short_part.off, &short_part.col, &short_part.val, m->stream));
    sp.rows.reset(rows);
    // worth it when the long rows are a minority that holds a good part of the entries
    const bool worth = sp.n_long > 0 && sp.n_long * 4 <= m->n_rows && nnz_long * 4 >= m->nnz;
    if (!worth) return SMH_OK;
    auto part = [&](size_t n_rows, size_t nnz, CrsArrays &arrays, uint32_t shift, smh_crs **out) -> int {
        SMH_TRY(wrap_arrays(m->dtype, nullptr, n_rows, m->n_cols, nnz, arrays, 0, out));
        (*out)->no_split = true;
        (*out)->knobs.cb_forced_shift = shift;
        return SMH_OK;
    };
    // LONG: K2c with 2^18-column blocks (1.93 against 2.03 ms with 2^19 on C3's long part); SHORT: its own AUTO with 2^19
    SMH_TRY(part(sp.n_long, nnz_long, long_part, 18u, &sp.long_part));
    SMH_TRY(part(m->n_rows, m->nnz - nnz_long, short_part, 19u, &sp.short_part));
    SMH_TRY(sp.y.alloc(sp.n_long * dtype_size(m->dtype)));
    SMH_HIP(hipStreamCreateWithFlags(&sp.side, hipStreamNonBlocking));
    SMH_HIP(hipEventCreateWithFlags(&sp.fork, hipEventDisableTiming));
    SMH_HIP(hipEventCreateWithFlags(&sp.join, hipEventDisableTiming));
    sp.state = Form::Ready;
    m->split = std::move(sp);
    return SMH_OK;
}
// (the sub-handles go through smh_crs_destroy, like every handle)
RowSplit::~RowSplit() {
    (void)smh_crs_destroy(long_part);
    (void)smh_crs_destroy(short_part);
    rows.reset();
    y.reset();
    if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
    if (fork) (void)hipEventDestroy(fork);
    if (join) (void)hipEventDestroy(join);
}

// K1s: 16-bit column codes, once per matrix.  Kept only when EVERY tile has a description (stencils, bands): the kernel
// variant then has no per-tile branch; any other matrix streams its u32 columns as before and nothing stays allocated.
static int ensure_stream_codes(smh_crs *m) {
    if (m->codes.state != Form::NotTried) return SMH_OK;
    StreamCodes c;
    c.state = Form::Refused;  // (nothing to describe, or some tile without a description)
    const size_t n_tiles = (m->n_rows + kStreamRows - 1) / kStreamRows;
    if (n_tiles && m->nnz) {
        uint32_t h_count = 0;
        SMH_TRY(c.cwin.alloc(n_tiles * 8));
        SMH_TRY(read_back(&h_count, 1, m->stream, [&](uint32_t *d_count) {
            return launch_stream_windows(m->d_off, m->d_col, m->n_rows, c.cwin.get(), d_count, m->stream);
        }));
        if ((size_t)h_count == n_tiles) c.state = Form::Ready;
        else c.cwin.reset();  // some tile's columns need more than 4 intervals of 16384
    }
    if (c.state == Form::Ready) {
        const size_t n_out = ((m->nnz + 3) & ~size_t(3)) + 4;
        SMH_TRY(c.code.alloc(n_out));
        SMH_HIP(hipMemsetAsync(c.code.get(), 0, n_out * sizeof(uint16_t), m->stream));
        SMH_TRY(launch_stream_codes(m->d_off, m->d_col, c.cwin.get(), m->n_rows, c.code.get(), m->stream));
        // ... and with rows of at most 255 entries the row boundaries shrink from a u32 offset to a byte per row
        if (m->max_row_len <= 255u) {
            SMH_TRY(c.len8.alloc(n_tiles * kStreamRows));
            SMH_TRY(c.tbase.alloc(n_tiles + 1));
            SMH_TRY(launch_stream_len8(m->d_off, m->n_rows, c.len8.get(), c.tbase.get(), m->stream));
            // how much of x a tile's intervals span (decides whether the body that stages x in LDS applies)
            uint32_t h_xs[2] = {0xFFFFFFFFu, 0};
            SMH_TRY(read_back(h_xs, 2, m->stream, [&](uint32_t *d_xs) { return launch_stream_xs_stats(c.cwin.get(), n_tiles, d_xs, m->stream); }));
            c.xs_chunks = h_xs[0];
            c.xs_end = h_xs[1];
            // ... and how many rows have an odd length (decides whether the unskewed product stage of K1s XD applies)
            unsigned long long h_odd = 0;
            SMH_TRY(read_back(&h_odd, 1, m->stream, [&](unsigned long long *d_odd) {
                return launch_stream_odd_rows(c.len8.get(), n_tiles * kStreamRows, d_odd, m->stream);
            }));
            c.odd_rows = (uint64_t)h_odd;
        }
        SMH_HIP(hipStreamSynchronize(m->stream));
    }
    m->codes = std::move(c);
    return SMH_OK;
}

// K1r's compact column form: the counting pass (once per matrix and storage order) and, when the form is taken (*use: forced,
// or few enough escapes), its arrays
static void drop_ring_col12(smh_crs *m) {
    m->ring.lo8.reset();
    m->ring.hdr.reset();
    m->ring.escapes.reset();
    m->ring.rec16.reset();  // (the records hold the low column bytes: they go with the form, what is known about the values stays)
}
// (the low bytes live in lo8 or, with the 24-bit value code, in the chunk records: either one counts as "built")
static int ensure_ring_col12(smh_crs *m, bool forced, bool *use) {
    RingPlan &r = m->ring;
    *use = forced || r.c12 == Form::Ready;
    if (r.c12 != Form::NotTried && (!*use || r.lo8.get() || r.rec16.get())) return SMH_OK;
    r.rec16.reset();
    Scratch scr;
    uint32_t *jobs = nullptr;
    unsigned long long *d_counts = nullptr, h_counts[2] = {0, 0};
    SMH_TRY(scr.alloc(&jobs, 2 * r.n_phases));
    SMH_TRY(scr.alloc(&d_counts, 2));
    SMH_TRY(read_back(d_counts, h_counts, 2, m->stream, [&](unsigned long long *d) {
        return launch_col12_count(m->d_off, m->d_col, m->nnz, r.phases.get(), r.n_phases, jobs, d, m->stream);
    }));
    r.c12_chunks = h_counts[0];
    r.c12_escapes = h_counts[1];
    r.c12 = r.c12_escapes * 1024ull <= r.c12_chunks ? Form::Ready : Form::Refused;
    *use = forced || r.c12 == Form::Ready;
    if (!*use) return SMH_OK;
    const size_t n_chunks_out = ((m->nnz + 3) >> 2) + 1;  // (one chunk beyond the padded end, like col16)
    DevArray<uint8_t> lo8;
    DevArray<uint16_t> hdr;
    DevArray<uint32_t> escapes;
    SMH_TRY(lo8.alloc(n_chunks_out * 4));
    SMH_TRY(hdr.alloc(n_chunks_out));
    SMH_TRY(escapes.alloc(2 * (size_t)(r.c12_escapes ? r.c12_escapes : 1)));
    SMH_TRY(launch_col12_encode(m->d_col, m->nnz, jobs, r.n_phases, n_chunks_out, lo8.get(), hdr.get(), escapes.get(), d_counts, m->stream));
    SMH_HIP(hipStreamSynchronize(m->stream));
    r.lo8 = std::move(lo8);
    r.hdr = std::move(hdr);
    r.escapes = std::move(escapes);
    return SMH_OK;
}

// K1r's chunk records with 24-bit values (ring_val24.hpp), for a handle whose compact column form is built: the counting pass gives
// the exponent (or refuses: a value the code never holds, an exponent outside its bound), the encoder writes the records from the
// values and lo8 and counts the values that do not come back bit for bit -- the form is taken (*use, and lo8 goes) only when there is
// none.  Tested once per set of values (smh_crs_update_values / smh_crs_scale / a new storage order reset v24 to NotTried).
void ring_values_changed(smh_crs *m) {
    m->ring.rec16.reset();  // (the compact column form then has no low bytes: ensure_ring_col12 builds it again on the next use)
    m->ring.v24 = Form::NotTried;
    m->ring.v24_exp = 0;
}
static int ensure_ring_val24(smh_crs *m, bool *use) {
    RingPlan &r = m->ring;
    *use = r.v24 != Form::Refused;
    if (!*use || r.rec16.get()) return SMH_OK;
    r.v24 = Form::Refused;  // until the records are complete
    r.v24_exp = 0;
    *use = false;
    Scratch scr;
    uint32_t *jobs = nullptr;
    unsigned long long *d_counts = nullptr, h_misses = 0;
    uint32_t h_stats[2] = {0, 0};
    SMH_TRY(scr.alloc(&jobs, 2 * r.n_phases));
    SMH_TRY(scr.alloc(&d_counts, 2));
    const float *val = (const float *)m->d_val;
    SMH_TRY(read_back(h_stats, 2, m->stream, [&](uint32_t *d_stats) {
        return launch_val24_count(m->d_off, val, m->nnz, r.phases.get(), r.n_phases, jobs, d_counts, d_stats, m->stream);
    }));
    const int E = h_stats[0] == ~0u ? 0 : (int)h_stats[0] - 1024;  // (no non-zero value: any exponent does)
    if (h_stats[1] != 0u || !val24::exponent_ok(E)) return SMH_OK;
    const size_t n_chunks_out = ((m->nnz + 3) >> 2) + 1;  // (as lo8)
    DevArray<uint32_t> rec16;
    SMH_TRY(rec16.alloc(n_chunks_out * 4));
    SMH_TRY(read_back(d_counts, &h_misses, 1, m->stream, [&](unsigned long long *d) {
        return launch_val24_encode(val, m->nnz, jobs, r.n_phases, n_chunks_out, r.lo8.get(), E, rec16.get(), d, m->stream);
    }));
    if (h_misses != 0) return SMH_OK;  // (a value of more than 24 bits: the records go, lo8 stays)
    r.rec16 = std::move(rec16);
    r.lo8.reset();
    r.v24 = Form::Ready;
    r.v24_exp = E;
    *use = true;
    return SMH_OK;
}

// does the VECTOR family run as K1r (LDS x-ring) for this matrix?
int vector_uses_ring(smh_crs *m, bool *out) {
    *out = false;
    if (m->knobs.use_ring == 0 || m->n_rows == 0) return SMH_OK;
    SMH_TRY(ensure_ring_plan(m));
    // the pipelined body also wins without the ring (its global-gather phases), so it is the default
    // whenever its lane widths apply; mode 0 keeps the plain K1 kernel selectable
    *out = true;
    // 16-bit columns for the ring phases: a ring slot is `column mod 16384`, so the low half of a column is all a
    // ring phase reads -- 6 instead of 8 bytes per f32 entry from HBM.  One extra 2-byte-per-entry array, built once.
    int want = m->knobs.use_col16;
    if (const char *e = getenv("SMH_RING_COL16")) want = atoi(e) ? 1 : 0;  // tuning knob
    // ... or, f32 on the single-window ring of 16384 columns, the compact form of ring_col12.hpp: 5.5 bytes per entry.  Chosen
    // by itself when col16 would be, nobody has asked for or against col16, and a counting pass (once per matrix) finds at most
    // one chunk in 1024 that the code cannot hold; SMH_RING_COL12=1 takes it wherever it applies, however many chunks escape.
    int want12 = m->knobs.use_col12;
    if (const char *e = getenv("SMH_RING_COL12")) want12 = strcmp(e, "auto") == 0 ? -1 : (atoi(e) ? 1 : 0);  // tuning knob
    const bool can12 = m->dtype == SMH_F32 && m->ring.bands == 1 && m->ring.entries == (unsigned)kRingEntries && m->nnz > 0;
    bool use12 = can12 && (want12 == 1 || (want12 < 0 && want < 0 && m->ring.fraction >= 0.25));
    // ... and with it, where the values are 24-bit fixed-point numbers (ring_val24.hpp), 16-byte chunk records instead of the low
    // bytes AND the value array: 4.5 bytes per entry.  Exactly where the compact form is taken and the plan runs the REGK kernel (the
    // only one with a record body); SMH_RING_VAL24=0 never, 1 = automatic: a matrix that does not qualify cannot be forced.
    int want24 = m->knobs.use_val24;
    if (const char *e = getenv("SMH_RING_VAL24")) want24 = strcmp(e, "auto") == 0 ? -1 : (atoi(e) ? 1 : 0);  // tuning knob
    const char *reg_env = getenv("SMH_RING_REGULAR");  // (as launch_ring reads it)
    const bool reg_off = reg_env && strcmp(reg_env, "auto") != 0 && atoi(reg_env) == 0;
    bool use24 = use12 && want24 != 0 && m->ring.reg_applies && !reg_off;
    if (!use24) m->ring.rec16.reset();  // (switched off: the low bytes come back below, lazily, as with the col12 / col16 switch)
    if (use12) SMH_TRY(ensure_ring_col12(m, want12 == 1, &use12));
    if (!use12) drop_ring_col12(m);
    if (use12 && use24) SMH_TRY(ensure_ring_val24(m, &use24));
    // (the banded plan cannot do without: its gathers take the ring slot from that array)
    // col16 is built by the same rule as before also when the compact form is in use, although the kernel then does not read it:
    // tests/test_bench_contract_gpu.py pins `derived_bytes` to at least 2 bytes per entry.  Dropping it here (`!use12 &&`: 2 bytes
    // per entry of device memory and a 0.5 ms pass less on the headline) has to go together with that assertion.
    const bool use16 = m->ring.bands == 4 || want == 1 || (want < 0 && m->ring.fraction >= 0.25);
    if (use16 && !m->ring.col16.get() && m->nnz) {
        const size_t n_out = ((m->nnz + 3) & ~size_t(3)) + 4;
        DevArray<uint16_t> col16;
        SMH_TRY(col16.alloc(n_out));
        if (m->ring.bands == 4) {
            SMH_HIP(hipMemsetAsync(col16.get(), 0, n_out * sizeof(uint16_t), m->stream));
            SMH_TRY(launch_ring_band_codes(m->d_off, m->d_col, m->ring.win.get(), m->n_rows, m->ring.entries / 4, col16.get(), m->stream));
        } else {
            SMH_TRY(launch_narrow_columns(m->d_col, m->nnz, col16.get(), n_out, m->stream));
        }
        SMH_HIP(hipStreamSynchronize(m->stream));
        m->ring.col16 = std::move(col16);
    } else if (!use16) {
        m->ring.col16.reset();
    }
    return SMH_OK;
}

// Which derived forms go when the matrix changes under them (each is rebuilt on its next use); dropping = a default-constructed form.
void invalidate(smh_crs *m, Changed what) {
    // the column-blocked / split / tiled copies hold the values, keep storage order inside a (row, block) pair, and are cut by the block width
    m->cb = ColBlock();
    m->cf = ColFused();
    m->split = RowSplit();
    m->tiled = Tiled();
    if (what == Changed::Values) m->dict.state = Form::NotTried;  // (the dictionary array stays: a product in flight may still read it)
    // K1r's chunk records are made of the values (and, like lo8, of the order inside the rows): the next product tests them again.
    // hdr and the escapes stay: the columns did not change.
    if (what == Changed::Values || what == Changed::Order) ring_values_changed(m);
    if (what == Changed::Order) {
        // the K1s codes and the 16-bit column array follow the storage order too; the ring plan's phases and windows stay: they
        // depend on each tile's column set, not on order
        m->codes = StreamCodes();
        m->ring.col16.reset();
        drop_ring_col12(m);
        m->ring.c12 = Form::NotTried;  // (which chunks escape depends on the order inside the rows)
        // the level schedules hold entry positions (the levels themselves would stay: they depend on each row's column set)
        m->tri[0] = TriSchedule();
        m->tri[1] = TriSchedule();
    }
}

// K1s configuration of this handle
static int stream_rpt(const smh_crs *m) {
    // rows per thread: 512-row tiles measured no better than 256-row tiles (1.86 vs 1.80 ms on the 512^3
    // Laplacian), so one row per thread unless asked (SMH_STREAM_RPT=2, tuning knob)
    int want = m->knobs.stream_rows_per_thread;
    if (const char *e = getenv("SMH_STREAM_RPT")) want = atoi(e);
    return want == 2 && m->max_tile512_entries <= (uint32_t)kStreamCap ? 2 : 1;
}

// K1s configuration the STREAM variant runs with for this handle (StreamCfg; builds the code tables on first use)
// recode = false (every launch path): the configuration is READ from the handle -- the code array keeps the meaning it has.
// recode = true (the first build, smh_crs_prepare, the setters): the code array is rewritten in place when the choice between
// column codes and K1s XD's stage offsets has changed -- behind a device synchronisation, because a product enqueued on any
// stream may still read it; never under a stream capture (the callers say so in the header), and a graph captured before the
// change must be captured again.
int stream_cfg(smh_crs *m, StreamCfg *c, bool recode) {
    *c = StreamCfg();
    // a 512-row tiling is only chosen when every such tile fits the LDS stage; the 256-row tiling takes
    // tiles of any density (loop-free body when the create-time statistic says that none overflows)
    c->rpt = stream_rpt(m);
    c->single_pass = m->have_stats && (c->rpt == 2 || m->max_tile_entries <= (uint32_t)kStreamCap);
    // 16-bit column codes when every tile's columns fall into <= 4 intervals of <= 16384 (stencils, bands)
    const char *c16_env = getenv("SMH_STREAM_C16");  // tuning knob: 0 = always the u32 columns
    // (single-pass tiles only: on dense multi-pass tiles -- banded C2 through K1s -- the decode costs more than
    // the bytes save, 0.83 vs 0.80 ms)
    if (!(c16_env && atoi(c16_env) == 0) && c->rpt == 1 && c->single_pass) {
        const bool first = m->codes.state == Form::NotTried;
        SMH_TRY(ensure_stream_codes(m));
        if (first) recode = true;  // (the build itself: allocations and synchronisations anyway)
        c->code = m->codes.code.get();
        c->cwin = m->codes.code.get() ? m->codes.cwin.get() : nullptr;
        static const bool l8_off = getenv("SMH_STREAM_L8") && atoi(getenv("SMH_STREAM_L8")) == 0;  // tuning knob
        if (c->cwin && !l8_off) { c->len8 = m->codes.len8.get(); c->tbase = m->codes.tbase.get(); }
        static const bool small_off = getenv("SMH_STREAM_SMALL") && atoi(getenv("SMH_STREAM_SMALL")) == 0;  // tuning knob
        c->small = !small_off && m->have_stats && m->max_tile_entries <= (uint32_t)kStreamCapSmall;
        static const bool xs_off = getenv("SMH_STREAM_XS") && atoi(getenv("SMH_STREAM_XS")) == 0;  // tuning knob
        // worth it from ~1 MB of x on (tools/dev/xs_threshold.py, profiles/r03_xs_threshold.log: 64^3 ... 320^3 cubes and 1000^2 / 2000^2
        // grids, -11 .. -20 % with the 2048-entry stage, -18 .. -40 % as K1s XD, both dtypes; below that the launch dominates).  The
        // 4096-entry stage pays on f32 only (grid planes 1024 wide, x of 17-34 MB: -7 .. -9 %; f64, LDS-limited to three blocks per
        // CU: +3 .. +10 %).  (Round 2 had 8 MB / 32 MB here: its inspector described a tile whose columns span < 16384 as ONE interval,
        // so a 64^3 .. 100^3 cube staged its whole span or nothing.)
        const bool forced = m->knobs.use_stream_xs == 1;
        const size_t x_bytes = m->n_cols * dtype_size(m->dtype);
        const bool on2 = forced || x_bytes >= ((size_t)1 << 20), on4 = forced || (x_bytes >= ((size_t)8 << 20) && m->dtype == SMH_F32);
        c->xs = (xs_off || m->knobs.use_stream_xs == 0 || !c->small || !c->len8) ? 0
                : (m->codes.xs_chunks <= 2u * kBlock && on2) ? 2
                : (m->codes.xs_chunks <= 4u * kBlock && on4) ? 4 : 0;
        // K1s XD: the code array as stage offsets.  The unskewed product stage it goes with collides on rows of even length, so
        // automatic = most rows odd (stencils with a diagonal)
        static const bool xd_off = getenv("SMH_STREAM_XD") && atoi(getenv("SMH_STREAM_XD")) == 0;  // tuning knob
        const bool want_direct = c->code && c->xs != 0 && !xd_off && m->knobs.use_stream_direct != 0 &&
                                 (m->knobs.use_stream_direct == 1 || 2 * m->codes.odd_rows >= (uint64_t)m->n_rows);
        // K1s XD-V: the matrix's distinct values in a dictionary, their indices in the codes' spare bits (spmv_stream_xd.hip) -- when
        // the values allow it (at most 32 bit patterns; 16 with the 4096-entry stage).  Looked at once per matrix, and again after
        // smh_crs_update_values.
        static const bool vd_off = getenv("SMH_STREAM_VDICT") && atoi(getenv("SMH_STREAM_VDICT")) == 0;  // tuning knob
        bool want_vdict = want_direct && !vd_off && m->knobs.use_stream_vdict != 0 && m->dict.state != Form::Refused;
        bool dict_rebuilt = false;  // (the indices in the codes belong to the dictionary they were made with)
        if (recode && want_vdict && m->dict.state == Form::NotTried) {
            if (!m->dict.values.get()) SMH_TRY(m->dict.values.alloc(32 * dtype_size(m->dtype)));
            SMH_HIP(hipDeviceSynchronize());  // (a product in flight may still read the dictionary)
            uint32_t n_vals = 0;
            SMH_TRY(stream_value_dict(m->dtype, m->d_val, m->nnz, m->dict.values.get(), &n_vals, m->stream));
            m->dict.n = n_vals;
            m->dict.state = n_vals ? Form::Ready : Form::Refused;
            dict_rebuilt = true;
        }
        want_vdict = want_vdict && m->dict.state == Form::Ready && m->dict.n <= stream_value_dict_capacity(c->xs);
        const bool form_ok = want_direct == m->codes.direct && want_vdict == m->codes.vdict && (!want_vdict || m->codes.vdict_xs == c->xs) &&
                             !(dict_rebuilt && (want_vdict || m->codes.vdict));
        if (recode && c->code && !form_ok) {
            SMH_HIP(hipDeviceSynchronize());  // (a product enqueued on any stream may still read the array)
            if (want_direct)
                SMH_TRY(launch_stream_stage_codes(m->d_off, m->d_col, m->codes.cwin.get(), m->n_rows, (uint32_t)dtype_size(m->dtype), m->codes.code.get(), m->stream));
            else
                SMH_TRY(launch_stream_codes(m->d_off, m->d_col, m->codes.cwin.get(), m->n_rows, m->codes.code.get(), m->stream));
            if (want_vdict)
                SMH_TRY(launch_stream_value_codes(m->dtype, m->d_val, m->nnz, m->dict.values.get(), m->dict.n, c->xs, m->codes.code.get(), m->stream));
            SMH_HIP(hipStreamSynchronize(m->stream));
            m->codes.direct = want_direct;
            m->codes.vdict = want_vdict;
            m->codes.vdict_xs = want_vdict ? c->xs : 0;
        }
        // (stage offsets without a stage -- xs == 0 after a setter that was not followed by a prepare cannot happen: the setters
        // recode; an x too short / misaligned for the stage is handled per call in stream_launch)
        c->direct = c->code && m->codes.direct;
        c->dict = c->direct && m->codes.vdict ? m->dict.values.get() : nullptr;
        c->dict_high = c->dict && stream_value_dict_high(m->dtype, m->dict.n, m->codes.vdict_xs);
    }
    return SMH_OK;
}

// a setting that decides the code array's meaning has changed: the array (if it was built) is rewritten now, not inside a later launch
int recode_stream(smh_crs *m) {
    if (m->codes.state == Form::NotTried) return SMH_OK;
    StreamCfg c;
    return stream_cfg(m, &c, true);
}

}  // namespace smh

using namespace smh;

extern "C" {

// ---- the entry points: the knobs of the derived forms and what they let a caller see ---------------------------------------------
int smh_crs_span_fraction(smh_crs *m, double *out) {
    if (!m || !out) return fail(SMH_ERR_INVALID, "NULL argument");
    SMH_TRY(ensure_ring_plan(m, false));  // the locality statistic is taken with the K1r inspector
    *out = m->span_fraction;
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

}  // extern "C"
