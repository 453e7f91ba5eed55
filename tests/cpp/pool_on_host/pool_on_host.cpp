// csrc/pool.hip, unchanged (the test copies it here as pool.inc), on the stand-in runtime of internal.hpp, from eight threads on
// two "devices" under ThreadSanitizer.  Every thread allocates and frees blocks below and above the layer's 1 MiB floor, writes a
// pattern of its own into each block and finds it again before the free, trims now and then, and moves to the other device now
// and then (so that pool_free meets blocks of a device that is not current).  The budget per device is below what the freed
// blocks of many sizes add up to, so the refuse-trim-retry path of pool_malloc is taken.  A request that stays refused after the
// trim (the other threads' live blocks fill the device) is no failure: the thread goes on without that block, and main asserts
// that some retry did succeed.
//   usage: pool_on_host [steps [budget_MiB]]
#include "pool.inc"

#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

namespace {

constexpr int kThreads = 8, kHeld = 4;
constexpr size_t kMiB = 1ull << 20;

struct Held { unsigned char *p = nullptr; size_t bytes = 0; unsigned tag = 0; };

struct Result { long long failures = 0, pooled = 0, small = 0, unserved_pooled = 0, unserved_small = 0, net = -1; char first[200] = ""; };

uint64_t next(uint64_t &s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 33; }

// the pattern: the first and the last 64 bytes and one byte per 64 KiB
template <typename F> void each_probe(size_t bytes, F f) {
    for (size_t i = 0; i < 64 && i < bytes; ++i) f(i);
    for (size_t i = 65536; i + 64 < bytes; i += 65536) f(i);
    for (size_t i = bytes > 64 ? bytes - 64 : 0; i < bytes; ++i) f(i);
}
unsigned char pat(unsigned tag, size_t i) { return (unsigned char)(tag * 131u + i * 7u + (i >> 12)); }

void fail(Result &r, const char *what, int t, int step, size_t bytes) {
    if (!r.failures++) snprintf(r.first, sizeof r.first, "thread %d step %d: %s (%zu bytes)", t, step, what, bytes);
}

void release(Result &r, Held &h, int t, int step) {
    if (!h.p) return;
    bool ok = true;
    each_probe(h.bytes, [&](size_t i) { ok &= h.p[i] == pat(h.tag, i); });
    if (!ok) fail(r, "the pattern of a block was overwritten while this thread held it", t, step, h.bytes);
    if (smh::pool_free(h.p) != hipSuccess) fail(r, "pool_free refused", t, step, h.bytes);
    h = Held{};
}

void worker(int t, int steps, Result &r) {
    (void)hipSetDevice(t % stub::kDevices);
    uint64_t s = 0x9E3779B97F4A7C15ull * (t + 1);
    Held held[kHeld];
    for (int step = 0; step < steps; ++step) {
        Held &h = held[next(s) % kHeld];
        release(r, h, t, step);
        const uint64_t kind = next(s) % 8;
        // 0 .. 2: below the floor; 3: at the floor and one byte under it; the rest 1 .. 8 MiB, not multiples of the 2 MiB granule
        size_t bytes = kind < 3 ? 1 + next(s) % (kMiB - 1) : kind == 3 ? kMiB - (next(s) & 1) : kMiB + next(s) % (7 * kMiB);
        void *p = nullptr;
        const hipError_t e = smh::pool_malloc(&p, bytes);
        if (e == hipErrorOutOfMemory) { ++(bytes >= kMiB ? r.unserved_pooled : r.unserved_small); continue; }
        if (e != hipSuccess || !p) { fail(r, "pool_malloc failed with another status than out of memory", t, step, bytes); continue; }
        (bytes >= kMiB ? r.pooled : r.small)++;
        h = Held{(unsigned char *)p, bytes, (unsigned)(t * 1000003 + step)};
        each_probe(bytes, [&](size_t i) { h.p[i] = pat(h.tag, i); });
        if (next(s) % 197 == 0) (void)smh_pool_trim();
        if (next(s) % 61 == 0) { int d = 0; (void)hipGetDevice(&d); (void)hipSetDevice(1 - d); }
        if (next(s) % 97 == 0) {  // (both are sums of blocks rounded up to the 2 MiB granule)
            size_t kept = 0, live = 0;
            (void)smh_pool_stats(&kept, &live);
            if (kept % (2 * kMiB) || live % (2 * kMiB)) fail(r, "smh_pool_stats reports a size that is no sum of pooled blocks", t, step, kept + live);
        }
    }
    for (Held &h : held) release(r, h, t, steps);
    r.net = smh::pool_thread_net_bytes();
}

}  // namespace

int main(int argc, char **argv) {
    const int steps = argc > 1 ? atoi(argv[1]) : 2000;
    const size_t budget_mib = argc > 2 ? (size_t)atoll(argv[2]) : 96;
    stub::rt().budget = budget_mib * kMiB;
    std::vector<Result> res(kThreads);
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; ++t) th.emplace_back(worker, t, steps, std::ref(res[t]));
    for (auto &x : th) x.join();
    long long failures = 0, pooled = 0, small = 0, unserved_pooled = 0, unserved_small = 0;
    for (int t = 0; t < kThreads; ++t) {
        failures += res[t].failures;
        pooled += res[t].pooled;
        small += res[t].small;
        unserved_pooled += res[t].unserved_pooled;
        unserved_small += res[t].unserved_small;
        if (res[t].failures) printf("FAIL %s (%lld in this thread)\n", res[t].first, res[t].failures);
        if (res[t].net != 0) { printf("FAIL thread %d: pool_thread_net_bytes() = %lld after it freed all it allocated\n", t, res[t].net); ++failures; }
    }
    size_t kept = 0, live = 0;
    (void)smh_pool_stats(&kept, &live);
    if (live != 0) { printf("FAIL live bytes %zu at the end\n", live); ++failures; }
    if (kept == 0) { printf("FAIL nothing kept at the end: the layer was off\n"); ++failures; }
    (void)smh_pool_trim();
    (void)smh_pool_stats(&kept, &live);
    if (kept != 0 || live != 0) { printf("FAIL kept %zu live %zu after the last trim\n", kept, live); ++failures; }
    stub::Runtime &R = stub::rt();
    if (!R.out.empty() || R.used[0] || R.used[1]) { printf("FAIL %zu blocks (%zu + %zu bytes) still with the runtime\n", R.out.size(), R.used[0], R.used[1]); ++failures; }
    if (R.double_frees) { printf("FAIL %zu frees of a pointer the runtime does not hold\n", R.double_frees); ++failures; }
    const long long refused = stub::n_refused.load(), syncs = stub::n_sync.load();
    // a pooled request that stayed unserved was refused twice, before the trim and after it; a small one, which the layer passes
    // on, once: what is left of the refusals was followed by a retry that succeeded
    const long long retried_ok = refused - 2 * unserved_pooled - unserved_small;
    if (retried_ok < 1) { printf("FAIL %lld refusals, %lld + %lld requests unserved: no retry after a trim succeeded\n", refused, unserved_pooled, unserved_small); ++failures; }
    if (syncs != pooled) { printf("FAIL %lld device synchronisations for %lld frees of pooled blocks\n", syncs, pooled); ++failures; }
    if (small == 0 || pooled == 0) { printf("FAIL allocations: %lld small, %lld pooled\n", small, pooled); ++failures; }
    printf("threads %d steps %d budget %zu MiB per device: %lld small, %lld pooled, %lld refused (%lld retried with success, %lld requests unserved), %lld syncs, %lld last-error reads\n",
           kThreads, steps, budget_mib, small, pooled, refused, retried_ok, unserved_pooled + unserved_small, syncs, stub::n_last_error.load());
    printf("ok (%lld failures)\n", failures);
    return failures ? 1 : 0;
}
