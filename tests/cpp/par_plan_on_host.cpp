// The partition's arithmetic (sparsemat_amd/csrc/par_plan.hpp, unchanged) as a host program under ASan + UBSan, against brute force.
// Every array is allocated at its exact size, so a read or write one past the end is a sanitizer report.
#include "par_plan.hpp"

#include <cstdio>
#include <memory>
#include <random>
#include <vector>

using namespace smh::plan;

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++failures <= 20) {                        \
                printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); \
                printf(__VA_ARGS__);                       \
                printf("\n");                              \
            }                                              \
        }                                                  \
    } while (0)

template <class T> std::unique_ptr<T[]> exact(const std::vector<T> &v) {  // a heap copy of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

static std::mt19937 rng(12345);
static size_t rnd(size_t lo, size_t hi) { return lo + rng() % (hi - lo + 1); }  // [lo, hi]

// one partition with one set of column intervals, against sets of columns
static void check_plan(size_t nb, size_t n, const std::vector<size_t> *split_v) {
    std::vector<uint8_t> needs_v(nb);
    std::vector<uint32_t> lo_v(nb), hi_v(nb);
    for (size_t q = 0; q < nb; ++q) {
        needs_v[q] = rnd(0, 4) != 0;
        lo_v[q] = (uint32_t)rnd(0, n - 1);
        hi_v[q] = (uint32_t)rnd(lo_v[q], n - 1);
    }
    auto needs = exact(needs_v);
    auto lo = exact(lo_v), hi = exact(hi_v);
    std::unique_ptr<size_t[]> split = split_v ? exact(*split_v) : nullptr;
    const Part pt{nb, n, split.get(), needs.get(), lo.get(), hi.get()};

    // block_rows tiles [0, n) in order; the lookup inverts it for every row
    std::vector<size_t> owner(n, nb);
    size_t at = 0;
    for (size_t k = 0; k < nb; ++k) {
        size_t r0, r1;
        block_rows(pt, k, &r0, &r1);
        CHECK(r0 == at && r1 >= r0 && r1 <= n, "block %zu of %zu, %zu rows: [%zu, %zu) after %zu", k, nb, n, r0, r1, at);
        if (!split_v) CHECK(r0 == k * (n / nb) && (k + 1 == nb ? r1 == n : r1 == (k + 1) * (n / nb)), "reference rows of block %zu", k);
        for (size_t r = r0; r < r1; ++r) owner[r] = k;
        at = r1;
    }
    CHECK(at == n, "the blocks end at %zu of %zu", at, n);
    for (size_t r = 0; r < n; ++r) {
        size_t k = nb, loc = n, r0, r1;
        block_of_row(pt, r, &k, &loc);
        CHECK(k == owner[r], "row %zu: block %zu, owner %zu (%zu blocks, %zu rows, %s)", r, k, owner[r], nb, n, split_v ? "split" : "reference");
        if (k < nb) {
            block_rows(pt, k, &r0, &r1);
            CHECK(loc == r - r0, "row %zu: local %zu", r, loc);
        }
    }
    // every column a block references outside its own rows lies in exactly one recv_range; none covers the receiver's rows;
    // a range out of src is a run of src's rows; what q receives from src is what src sends to q (the plan entry point's two calls)
    size_t worst = 0;
    for (size_t q = 0; q < nb; ++q) {
        std::vector<int> covered(n, 0);
        size_t got = 0;
        for (size_t src = 0; src < nb; ++src) {
            size_t a = 99, e = 99;
            recv_range(pt, q, src, &a, &e);
            CHECK(a <= e && e <= n, "recv_range(%zu, %zu) = [%zu, %zu)", q, src, a, e);
            if (a == e) CHECK(a == 0, "an empty range is [0, 0)");
            for (size_t c = a; c < e; ++c) {
                ++covered[c];
                CHECK(owner[c] == src && src != q, "column %zu in recv_range(%zu, %zu) is owned by %zu", c, q, src, owner[c]);
            }
            got += e - a;
            size_t sa, se;  // src's send list, as smh_par_plan_split fills it for block src
            recv_range(pt, q, src, &sa, &se);
            std::vector<size_t> brute;
            for (size_t c = 0; c < n; ++c)
                if (needs_v[q] && c >= lo_v[q] && c <= hi_v[q] && owner[c] == src && src != q) brute.push_back(c);
            CHECK(se - sa == brute.size() && (brute.empty() || (sa == brute.front() && se == brute.back() + 1)), "send %zu -> %zu: [%zu, %zu), %zu columns by hand", src, q,
                  sa, se, brute.size());
        }
        for (size_t c = 0; c < n; ++c) {
            const bool referenced = needs_v[q] && c >= lo_v[q] && c <= hi_v[q], own = owner[c] == q;
            CHECK(covered[c] == (referenced && !own ? 1 : 0), "block %zu, column %zu: in %d ranges (referenced %d, own %d)", q, c, covered[c], referenced, own);
        }
        worst = got > worst ? got : worst;
    }
    int mode = -1;
    size_t max_recv = 999;
    plan_summary(pt, &mode, &max_recv);
    CHECK(max_recv == worst, "plan_summary: %zu, by hand %zu", max_recv, worst);
    CHECK(mode == (nb <= 1 ? SMH_EXCHANGE_NONE : worst * 2 < n ? SMH_EXCHANGE_WINDOW : SMH_EXCHANGE_ALLGATHER), "automatic mode %d", mode);
    plan_summary(pt, nullptr, nullptr);

    if (split_v) {
        size_t k = 99;
        CHECK(check_split(nb, n, split.get(), &k) == SplitFault::None, "a good split table is refused");
    }
}

static void check_split_tables() {
    size_t k = 99;
    {
        auto s = exact(std::vector<size_t>{1, 4, 9});
        CHECK(check_split(2, 9, s.get(), &k) == SplitFault::Ends, "a table that does not start at 0");
    }
    {
        auto s = exact(std::vector<size_t>{0, 4, 8});
        CHECK(check_split(2, 9, s.get(), &k) == SplitFault::Ends, "a table that does not end at n_rows");
    }
    {
        auto s = exact(std::vector<size_t>{0, 6, 4, 9});
        CHECK(check_split(3, 9, s.get(), &k) == SplitFault::Descends && k == 1, "a block that ends before it begins (block %zu)", k);
    }
    {
        auto s = exact(std::vector<size_t>{0, 0, 9, 9});
        CHECK(check_split(3, 9, s.get(), &k) == SplitFault::None, "empty blocks are allowed");
    }
}

// split_by_nnz against its definition by linear scan
static void check_nnz_split(size_t nb, const std::vector<uint32_t> &off_v) {
    const size_t n = off_v.size() - 1;
    auto off = exact(off_v);
    std::vector<size_t> split;
    split_by_nnz(nb, n, off.get(), split);
    CHECK(split.size() == nb + 1 && split[0] == 0 && split[nb] == n, "ends of the nnz split");
    const uint64_t nnz = (uint64_t)off_v[n] - off_v[0];
    size_t prev = 0;
    for (size_t k = 1; k < nb; ++k) {
        const uint64_t want = off_v[0] + nnz * k / nb;
        size_t r = 0;
        while (r < n && off_v[r] < want) ++r;  // the first row whose entries begin at or beyond k nnz / n_blocks
        if (r < prev + 1) r = prev + 1;        // ... but every block keeps a row
        if (r > n - (nb - k)) r = n - (nb - k);
        CHECK(split[k] == r, "nnz split %zu of %zu blocks, %zu rows: %zu, by hand %zu", k, nb, n, split[k], r);
        prev = split[k];
    }
    for (size_t k = 0; k < nb; ++k) CHECK(split[k + 1] > split[k], "block %zu of the nnz split has no row", k);
}

static void check_tile_runs() {
    for (size_t nt = 0; nt <= 10; ++nt)
        for (unsigned bits = 0; bits < (1u << nt); ++bits) {
            std::vector<uint8_t> d_v(nt);
            for (size_t t = 0; t < nt; ++t) d_v[t] = (bits >> t) & 1;
            auto d = exact(d_v);
            size_t t0 = 99, t1 = 99, b0 = 0, b1 = 0;
            longest_clean_run(d.get(), nt, &t0, &t1);
            for (size_t a = 0; a <= nt; ++a)
                for (size_t e = a; e <= nt; ++e) {
                    bool clean = true;
                    for (size_t t = a; t < e; ++t) clean = clean && !d_v[t];
                    if (clean && e - a > b1 - b0) { b0 = a; b1 = e; }  // (a ascending: the first of equally long runs)
                }
            CHECK(t1 - t0 == b1 - b0 && (b1 == b0 || t0 == b0), "%zu tiles, pattern %#x: [%zu, %zu), by hand [%zu, %zu)", nt, bits, t0, t1, b0, b1);
            CHECK(t0 <= t1 && t1 <= nt, "run [%zu, %zu) of %zu tiles", t0, t1, nt);
        }
}

static void check_rounding() {
    for (size_t n_loc = 1; n_loc <= 24; ++n_loc)
        for (size_t in0 = 0; in0 <= n_loc; ++in0)
            for (size_t in1 = 0; in1 <= n_loc; ++in1)
                for (size_t gran = 0; gran <= 9; ++gran) {
                    size_t a = 99, e = 99;
                    round_interior(in0, in1, n_loc, gran, &a, &e);
                    if (a == e) { CHECK(a == 0, "an empty interior is [0, 0)"); }
                    else {
                        CHECK(in0 <= a && a < e && e <= in1, "[%zu, %zu) leaves [%zu, %zu) (n_loc %zu, gran %zu)", a, e, in0, in1, n_loc, gran);
                        CHECK(gran && a % gran == 0 && (e % gran == 0 || e == n_loc), "[%zu, %zu) is no run of %zu rows (n_loc %zu)", a, e, gran, n_loc);
                        CHECK(!(a == 0 && e == n_loc), "the whole block [%zu, %zu) is no interior", a, e);
                    }
                    // by hand: the largest such run inside [in0, in1)
                    size_t ba = 0, be = 0;
                    if (gran && in1 > in0)
                        for (size_t x = in0; x < in1; ++x) {
                            if (x % gran) continue;
                            for (size_t y = in1; y > x; --y)
                                if (y % gran == 0 || y == n_loc) {
                                    if (y - x > be - ba) { ba = x; be = y; }
                                    break;
                                }
                        }
                    if (ba == 0 && be == n_loc) ba = be = 0;
                    CHECK(a == ba && e == be, "in [%zu, %zu) of %zu by %zu: [%zu, %zu), by hand [%zu, %zu)", in0, in1, n_loc, gran, a, e, ba, be);
                }
}

// the tiles other blocks reference, with blocks of several tiles
static void check_referenced_tiles() {
    for (int trial = 0; trial < 200; ++trial) {
        const size_t nb = rnd(2, 4), n = rnd(nb * 300, nb * 900);
        std::vector<uint8_t> needs_v(nb);
        std::vector<uint32_t> lo_v(nb), hi_v(nb);
        for (size_t q = 0; q < nb; ++q) {
            needs_v[q] = rnd(0, 5) != 0;
            lo_v[q] = (uint32_t)rnd(0, n - 1);
            hi_v[q] = (uint32_t)rnd(lo_v[q], n - 1 < lo_v[q] + 700 ? n - 1 : lo_v[q] + 700);
        }
        auto needs = exact(needs_v);
        auto lo = exact(lo_v), hi = exact(hi_v);
        const Part pt{nb, n, nullptr, needs.get(), lo.get(), hi.get()};
        for (size_t me = 0; me < nb; ++me) {
            size_t r0, r1;
            block_rows(pt, me, &r0, &r1);
            const size_t nt = (r1 - r0 + kTileRows - 1) / kTileRows;
            std::unique_ptr<uint8_t[]> dirty(new uint8_t[nt]());
            mark_referenced_tiles(pt, me, r0, dirty.get());
            for (size_t t = 0; t < nt; ++t) {
                bool want = false;
                for (size_t r = r0 + t * kTileRows; r < r1 && r < r0 + (t + 1) * kTileRows; ++r)
                    for (size_t q = 0; q < nb; ++q) want = want || (q != me && needs_v[q] && r >= lo_v[q] && r <= hi_v[q]);
                CHECK((dirty[t] != 0) == want, "block %zu tile %zu: %d, by hand %d", me, t, dirty[t], want);
            }
        }
    }
}

int main() {
    for (size_t nb = 1; nb <= 6; ++nb)
        for (size_t n = nb; n <= 40; ++n) {
            for (int trial = 0; trial < 6; ++trial) check_plan(nb, n, nullptr);
            for (int trial = 0; trial < 8; ++trial) {  // split tables: sorted random cuts, so some blocks are empty
                std::vector<size_t> split(nb + 1, 0);
                split[nb] = n;
                for (size_t k = 1; k < nb; ++k) split[k] = trial == 0 ? 0 : trial == 1 ? n : rnd(0, n);
                for (size_t i = 1; i < nb; ++i)
                    for (size_t j = i + 1; j < nb; ++j)
                        if (split[j] < split[i]) std::swap(split[i], split[j]);
                check_plan(nb, n, &split);
            }
            // row offsets: random row lengths, all rows empty, one heavy row, a first offset that is not 0
            for (int kind = 0; kind < 6; ++kind) {
                std::vector<uint32_t> off(n + 1, kind == 5 ? 7u : 0u);
                const size_t heavy = rnd(0, n - 1);
                for (size_t r = 0; r < n; ++r) {
                    uint32_t len = 0;
                    if (kind == 0 || kind == 5) len = (uint32_t)rnd(0, 9);
                    if (kind == 2) len = r == heavy ? 1000u : 0u;
                    if (kind == 3) len = r == heavy ? 1000u : (uint32_t)rnd(0, 2);
                    if (kind == 4) len = (uint32_t)(r * r % 7);
                    off[r + 1] = off[r] + len;  // (kind 1: every row empty)
                }
                check_nnz_split(nb, off);
            }
        }
    check_split_tables();
    check_tile_runs();
    check_rounding();
    check_referenced_tiles();
    printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
