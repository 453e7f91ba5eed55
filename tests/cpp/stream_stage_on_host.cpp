// stream_stage_on_host.cpp -- the K1s family's stage layout and code bits (sparsemat_amd/csrc/stream_stage.hpp: what the kernels' fills,
// the code builder and the eligibility statistic all call) on the host, built with -fsanitize=address,undefined by
// tests/test_stream_stage_host.py.  For hand-written and random interval tables (1 to 4 sorted, disjoint intervals, unaligned starts,
// a zero-width unused tail, totals up to exactly 2048 and 4096 stage entries):
//   1. an exact-size stage is filled through the chunk map from an exact-size x -- x has layout.end() entries, so a chunk that would
//      leave x, or the stage, is an error of the sanitizer's -- and every column of every interval is found at its entry index;
//   2. the byte code of every entry survives the offset mask, f32 and f64, stages of 2048 and 4096 entries;
//   3. every dictionary index below the capacity round-trips through both index forms beside every offset;
//   4. the XCD tile map is a partition of the launch's tiles into 8 contiguous runs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "stream_stage.hpp"

using namespace smh::stage;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++failures <= 20) printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
        }                                                                  \
    } while (0)

struct Table {
    uint32_t w[8];
};

// what the layout is, said without it: the used intervals back to back, each from its 4-aligned start in whole chunks
static void one_table(const Table &t, uint32_t cap_entries) {
    const Layout lay = layout(t.w);
    uint32_t chunks = 0, end = 0;
    for (int q = 0; q < 4; ++q) {
        const uint32_t a = t.w[2 * q], e = t.w[2 * q + 1];
        if (e > a) {
            const uint32_t al = a - a % 4, n = (e - al + 3) / 4;
            chunks += n;
            end = std::max(end, al + 4 * n);
        }
    }
    CHECK(lay.chunks() == chunks && lay.end() == end && 4 * chunks <= cap_entries);
    if (lay.chunks() != chunks || lay.end() != end) return;
    // the kernels' fill: stage chunk j <- chunk x_chunk(j) of x (exact-size arrays)
    std::vector<uint32_t> x(lay.end()), stage(4 * (size_t)lay.chunks());
    for (size_t i = 0; i < x.size(); ++i) x[i] = 0x9E3779B9u * (uint32_t)(i + 1);  // (distinct values)
    for (uint32_t j = 0; j < lay.chunks(); ++j) {
        const uint64_t g = 4ull * lay.x_chunk(j);
        for (int e = 0; e < 4; ++e) stage[4 * (size_t)j + e] = x[g + e];
    }
    // the code builder's map: every column of every interval
    const uint32_t first[4] = {lay.first_entry0(), lay.first_entry1(), lay.first_entry2(), lay.first_entry3()};
    for (int q = 0; q < 4; ++q) {
        const uint32_t a = t.w[2 * q], e = t.w[2 * q + 1];
        for (uint32_t c = a; c < e; ++c) {
            const uint32_t i = lay.entry(c);
            CHECK(i < stage.size());
            if (i >= stage.size()) return;
            CHECK(stage[i] == x[c]);
            CHECK(i == first[q] + (c - a));  // (the XS body: the interval's first entry + the column code's offset)
            for (int xs = 2; xs <= 4; xs += 2)
                for (uint32_t elem = 4; elem <= 8; elem += 4) {
                    if (i >= (uint32_t)xs * 1024u) continue;
                    const uint32_t code = i * elem;
                    CHECK(code < 65536u && code_ofs(code, elem, xs) == code);
                }
        }
    }
}

static void hand_written() {
    const Table tables[] = {
        {{0, 1, 0, 0, 0, 0, 0, 0}},                              // a single interval starting at 0, one column
        {{0, 2048, 0, 0, 0, 0, 0, 0}},                           // ... the whole 2048-entry stage
        {{0, 4096, 0, 0, 0, 0, 0, 0}},                           // ... the whole 4096-entry stage
        {{1, 2, 0, 0, 0, 0, 0, 0}},                              // starts = 1, 2, 3 mod 4
        {{2, 9, 0, 0, 0, 0, 0, 0}},
        {{3, 4, 0, 0, 0, 0, 0, 0}},
        {{3, 5, 0, 0, 0, 0, 0, 0}},                              // ... across a chunk boundary
        {{1, 6, 102, 111, 203, 204, 1027, 1041}},                // ... all three residues at once
        {{5, 8, 8, 12, 13, 16, 16, 17}},                         // intervals that touch after alignment (shared chunks are staged twice)
        {{4, 7, 7, 8, 0, 0, 0, 0}},                              // ... inside one chunk
        {{1001, 1257, 2001, 2257, 3001, 3257, 0, 0}},            // three planes of a stencil, the fourth interval unused
        {{7, 7, 0, 0, 0, 0, 0, 0}},                              // zero-width entries alone
        {{0, 0, 0, 0, 0, 0, 0, 0}},                              // an empty tile
        {{1, 0, 0, 0, 0, 0, 0, 0}},                              // a tile the inspector could not describe: [1, 0), nothing staged
        {{1, 2045, 0, 0, 0, 0, 0, 0}},                           // exactly 2048 entries from an unaligned start
        {{3, 1024, 5001, 6022, 9002, 10024, 20003, 21024}},      // exactly 4096: 256 + 256 + 256 + 256 chunks, all starts unaligned
    };
    for (const Table &t : tables) one_table(t, 4096);
    const Layout none = layout(tables[12].w);
    CHECK(none.chunks() == 0 && none.end() == 0);
    const Layout bad = layout(tables[13].w);
    CHECK(bad.chunks() == 0 && bad.end() == 0);
}

static void random_tables(size_t count) {
    std::mt19937_64 rng(20241021);
    size_t exact[2] = {0, 0};
    for (size_t it = 0; it < count; ++it) {
        const uint32_t cap = (rng() & 1) ? 2048u : 4096u;
        const int used = 1 + (int)(rng() % 4);
        // chunk budgets: sometimes the whole stage exactly
        const bool full = rng() % 4 == 0;
        uint32_t left = cap / 4;
        uint32_t n[4] = {0, 0, 0, 0};
        for (int q = 0; q < used; ++q) {
            const uint32_t rest = (uint32_t)(used - 1 - q);  // at least one chunk for each interval still to come
            n[q] = (q == used - 1 && full) ? left : 1u + (uint32_t)(rng() % (left - rest));
            left -= n[q];
        }
        Table t{};
        uint32_t pos = (uint32_t)(rng() % 50000);  // first column this interval may take
        bool share = false;                         // ... in the chunk the interval before ends in (staged twice then)
        uint32_t total = 0;
        for (int q = 0; q < used; ++q) {
            const uint32_t al = share ? pos & ~3u : (pos + 3u) & ~3u;
            const uint32_t least = share ? pos & 3u : 0u;
            const uint32_t lead = least + (uint32_t)(rng() % (4u - least));     // start = lead mod 4
            const uint32_t last_fill = 1u + (uint32_t)(rng() % 4);              // entries used of the last chunk
            uint32_t a = al + lead, e = al + 4u * (n[q] - 1u) + last_fill;
            if (e <= a) e = a + 1u;                                             // (one chunk: keep a column)
            t.w[2 * q] = a;
            t.w[2 * q + 1] = e;
            total += n[q];
            share = rng() % 3 == 0;
            pos = share ? e : e + (uint32_t)(rng() % 30000);
        }
        for (int q = used; q < 4; ++q) {  // the unused tail: zero width, any start (the inspector writes zeros)
            const uint32_t z = rng() % 2 ? 0u : (uint32_t)(rng() % 100000);
            t.w[2 * q] = t.w[2 * q + 1] = z;
        }
        if (4 * total == cap) ++exact[cap == 4096u];
        one_table(t, cap);
    }
    CHECK(exact[0] > count / 50 && exact[1] > count / 50);  // both stages are filled to the last entry often enough
    printf("random tables: %zu (%zu / %zu fill the 2048- / 4096-entry stage exactly)\n", count, exact[0], exact[1]);
}

static void code_bits() {
    for (int xs = 2; xs <= 4; xs += 2)
        for (uint32_t elem = 4; elem <= 8; elem += 4) {
            const uint32_t low = code_low_bits(elem), shift = code_high_shift(elem, xs), entries = (uint32_t)xs * 1024u;
            CHECK((1u << low) == elem && (entries * elem) == (1u << shift) && shift <= 16u);
            CHECK(code_values(xs) == (xs == 4 ? 16u : 32u) && code_values(xs) == (1u << (low + 16u - shift)));
            CHECK(code_values_high(elem, xs) == (1u << (16u - shift)) && code_values_high(elem, xs) <= code_values(xs));
            for (uint32_t i = 0; i < entries; ++i) {
                const uint32_t ofs = i * elem;
                for (uint32_t v = 0; v < code_values(xs); ++v) {
                    const uint32_t c = code_pack(ofs, v, low, shift);  // the index in the low and the high bits
                    CHECK(c < 65536u && code_ofs(c, elem, xs) == ofs && code_value(c, elem, xs) == v);
                }
                for (uint32_t v = 0; v < code_values_high(elem, xs); ++v) {
                    const uint32_t c = code_pack(ofs, v, 0u, shift);  // ... in the high bits alone
                    CHECK(c < 65536u && code_ofs(c, elem, xs) == ofs && code_value_high(c, elem, xs) == v);
                    CHECK(c == code_pack(ofs, v << low, low, shift));  // (the same code the general form gives for index v << low)
                }
            }
        }
}

static void tile_map() {
    const uint64_t counts[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 63, 64, 65, 508, 704, 3907, 524288, (1ull << 33) + 5};
    for (uint64_t n : counts) {
        uint64_t next = 0, least = ~0ull, most = 0;
        for (uint64_t g = 0; g < 8; ++g) {
            const XcdRun r = xcd_run(n, g);
            CHECK(r.first == next);
            next = r.first + r.count;
            least = std::min(least, r.count);
            most = std::max(most, r.count);
        }
        CHECK(next == n && most - least <= 1);
    }
}

int main() {
    hand_written();
    random_tables(6000);
    code_bits();
    tile_map();
    printf("stream_stage_on_host: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
