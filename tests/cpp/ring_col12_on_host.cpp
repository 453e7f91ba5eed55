// ring_col12_on_host.cpp -- K1r's compact column form (sparsemat_amd/csrc/ring_col12.hpp: the functions the encoder kernel and
// the ring kernel call) on the host, built with -fsanitize=address,undefined by tests/test_ring_col12_host.py:
//   1. the rank is a bijection of the 969 triples onto [0, 969), the table inverts it, and every triple round-trips for
//      several first strata, the mod-64 wrap included;
//   2. 10^6 random chunks (sorted columns in a window, unsorted ones, spans the code cannot hold) go through a stream
//      encoder / decoder shaped like the kernels' (exact-size arrays): every chunk comes back as its true slots, every chunk
//      the code cannot hold is flagged and comes back through the side table, and "cannot hold" is checked against a search
//      over all headers for a sample of them;
//   3. padding chunks -- and any header bits at all -- decode to slots inside the ring.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "ring_col12.hpp"

using namespace smh::col12;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++failures <= 20) printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
        }                                                                  \
    } while (0)

static constexpr Table kTable = make_table();

static bool same(const uint32_t (&a)[4], const uint32_t (&b)[4]) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]; }

// is there any header whose decoding (with these low bytes) gives the slots?  (the definition, by search)
static bool some_header_decodes_to(const uint32_t (&slot)[4]) {
    const uint32_t lo = (slot[0] & 255u) | (slot[1] & 255u) << 8 | (slot[2] & 255u) << 16 | (slot[3] & 255u) << 24;
    for (uint32_t t = 0; t < kTriples; ++t) {
        uint32_t got[4];
        decode_chunk((slot[0] >> 8) << 10 | t, lo, kTable.e, got);
        if (same(got, slot)) return true;
    }
    return false;
}

static void all_triples() {
    std::vector<int> seen(kTriples, 0);
    size_t n = 0;
    const uint32_t firsts[] = {0, 1, 17, 31, 46, 47, 48, 55, 62, 63};
    const uint32_t lows[][4] = {{0, 0, 0, 0}, {255, 255, 255, 255}, {1, 2, 3, 4}, {200, 7, 255, 0}};
    for (uint32_t d3 = 0; d3 <= kMaxGap; ++d3)
        for (uint32_t d2 = 0; d2 <= d3; ++d2)
            for (uint32_t d1 = 0; d1 <= d2; ++d1) {
                const uint32_t t = triple_rank(d1, d2, d3);
                CHECK(t < kTriples);
                if (t >= kTriples) continue;
                ++seen[t];
                ++n;
                CHECK(kTable.e[t] == pack_triple(d1, d2, d3));
                for (uint32_t h0 : firsts)
                    for (const auto &lo : lows) {
                        const uint32_t slot[4] = {h0 << 8 | lo[0], ((h0 + d1) & 63u) << 8 | lo[1], ((h0 + d2) & 63u) << 8 | lo[2],
                                                  ((h0 + d3) & 63u) << 8 | lo[3]};
                        uint16_t hdr = 0xFFFF;
                        uint32_t l = 0, got[4];
                        CHECK(encode_chunk(slot, &hdr, &l));
                        CHECK(!is_escape(hdr) && (hdr >> 10) == h0 && (hdr & 1023u) == t);
                        decode_chunk(hdr, l, kTable.e, got);
                        CHECK(same(got, slot));
                    }
            }
    CHECK(n == kTriples);
    for (uint32_t t = 0; t < kTriples; ++t) CHECK(seen[t] == 1);
    for (uint32_t t = kTriples; t < kTableEntries; ++t) CHECK(kTable.e[t] == 0);
    // one stratum too far, a step backwards: not encodable
    {
        uint16_t hdr;
        uint32_t l;
        const uint32_t far[4] = {5u << 8, 5u << 8, 6u << 8, (5u + kMaxGap + 1u) << 8}, back[4] = {9u << 8, 11u << 8, 10u << 8, 12u << 8},
                       wrap_back[4] = {1u << 8 | 3u, 0u << 8 | 3u, 1u << 8, 2u << 8};
        CHECK(!encode_chunk(far, &hdr, &l) && !encode_chunk(back, &hdr, &l) && !encode_chunk(wrap_back, &hdr, &l));
    }
}

static void random_chunks(size_t n_chunks) {
    std::mt19937_64 rng(20240611);
    std::vector<uint32_t> truth(4 * n_chunks);
    for (size_t c = 0; c < n_chunks; ++c) {
        uint32_t col[4];
        const unsigned kind = (unsigned)(rng() % 8);
        if (kind < 5) {  // a sorted row piece inside a window: spans from a few columns to the whole 8193-wide window
            const uint32_t base = (uint32_t)(rng() % 4000000000ull), span = 1u + (uint32_t)(rng() % (kind < 2 ? 1200u : kind < 4 ? 4500u : 8193u));
            for (auto &v : col) v = base + (uint32_t)(rng() % span);
            for (int i = 0; i < 4; ++i)
                for (int k = i + 1; k < 4; ++k)
                    if (col[k] < col[i]) { const uint32_t v = col[i]; col[i] = col[k]; col[k] = v; }
        } else if (kind == 5) {  // the end of one row and the start of the next
            const uint32_t base = (uint32_t)(rng() % 4000000000ull);
            col[0] = base + 7000u + (uint32_t)(rng() % 1000u);
            col[1] = col[0] + (uint32_t)(rng() % 200u);
            col[2] = base + (uint32_t)(rng() % 1000u);
            col[3] = col[2] + (uint32_t)(rng() % 300u);
        } else {  // anything
            for (auto &v : col) v = (uint32_t)rng();
        }
        for (int q = 0; q < 4; ++q) truth[4 * c + q] = col[q] & (kSlots - 1u);
    }
    // the encoder as the kernel runs it: exact-size arrays, escaped chunks numbered as they come
    std::vector<uint32_t> lo(n_chunks);
    std::vector<uint16_t> hdr(n_chunks);
    size_t n_escapes = 0;
    for (size_t c = 0; c < n_chunks; ++c) {
        const uint32_t slot[4] = {truth[4 * c], truth[4 * c + 1], truth[4 * c + 2], truth[4 * c + 3]};
        uint16_t h;
        uint32_t l;
        n_escapes += encode_chunk(slot, &h, &l) ? 0 : 1;
    }
    std::vector<uint32_t> escapes(2 * n_escapes);
    size_t next = 0, searched = 0;
    for (size_t c = 0; c < n_chunks; ++c) {
        const uint32_t slot[4] = {truth[4 * c], truth[4 * c + 1], truth[4 * c + 2], truth[4 * c + 3]};
        uint16_t h = 0;
        uint32_t l = 0;
        const bool ok = encode_chunk(slot, &h, &l);
        if (!ok) {
            if (searched < 3000) { ++searched; CHECK(!some_header_decodes_to(slot)); }
            uint32_t pair[2];
            pack_escape(slot, pair);
            l = (uint32_t)next++;
            escapes[2 * l] = pair[0];
            escapes[2 * l + 1] = pair[1];
            h = (uint16_t)kEscape;
        } else if (c % 97 == 0) {
            CHECK(some_header_decodes_to(slot));
        }
        lo[c] = l;
        hdr[c] = h;
    }
    CHECK(next == n_escapes);
    // the decoder as the ring kernel runs it
    size_t escaped = 0;
    for (size_t c = 0; c < n_chunks; ++c) {
        uint32_t slot[4];
        decode_chunk(hdr[c], lo[c], kTable.e, slot);
        for (uint32_t v : slot) CHECK(v < kSlots);  // (also of an escaped chunk, before its true slots replace these)
        if (is_escape(hdr[c])) {
            ++escaped;
            CHECK(lo[c] < n_escapes);
            unpack_escape(escapes[2 * lo[c]], escapes[2 * lo[c] + 1], slot);
        }
        const uint32_t want[4] = {truth[4 * c], truth[4 * c + 1], truth[4 * c + 2], truth[4 * c + 3]};
        CHECK(same(slot, want));
    }
    CHECK(escaped == n_escapes);
    CHECK(n_escapes > n_chunks / 8 && n_escapes < n_chunks - n_chunks / 8);  // both kinds are well represented
    printf("random chunks: %zu, escaped %zu (%zu of them checked by search)\n", n_chunks, n_escapes, searched);
}

static void padding_and_arbitrary_bits() {
    uint32_t slot[4];
    decode_chunk(0, 0, kTable.e, slot);  // a padding chunk
    for (uint32_t v : slot) CHECK(v == 0);
    CHECK(!is_escape(0));
    std::mt19937 rng(7);
    for (uint32_t hdr = 0; hdr < 65536; ++hdr) {
        const uint32_t los[3] = {0u, 0xFFFFFFFFu, (uint32_t)rng()};
        for (uint32_t l : los) {
            decode_chunk(hdr, l, kTable.e, slot);
            for (uint32_t v : slot) CHECK(v < kSlots);
        }
    }
    unpack_escape(0xFFFFFFFFu, 0xFFFFFFFFu, slot);
    for (uint32_t v : slot) CHECK(v < kSlots);
}

int main() {
    all_triples();
    random_chunks(1000000);
    padding_and_arbitrary_bits();
    printf("ring_col12_on_host: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
