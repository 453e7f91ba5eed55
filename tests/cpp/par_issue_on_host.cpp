// The issuing threads (sparsemat_amd/csrc/par_issue.hpp, unchanged) as a host program: under ThreadSanitizer, and under ASan + UBSan.
#include "par_issue.hpp"

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <vector>

using smh::IssuePool;

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

static thread_local char last_error[64] = "";  // the library's thread-local error text, in small
static const char *message_hook() { return last_error; }
static int fail_with(int rc, const char *text) {
    strncpy(last_error, text, sizeof last_error - 1);
    return rc;
}

struct Started {
    std::atomic<int> hooks{0};
    int throw_at = 0;  // the start hook of worker throw_at throws (0: none)
};
static void start_hook(void *ctx, size_t k) {
    Started *s = static_cast<Started *>(ctx);
    s->hooks.fetch_add(1);
    if ((int)k == s->throw_at) throw std::runtime_error("no thread for you");
}

static void set_hooks(IssuePool &pool, Started *st) {
    pool.hooks.start = start_hook;
    pool.hooks.message = message_hook;
    pool.hooks.ctx = st;
    pool.hooks.thrown = 77;
}

static void wait_until_asleep(const IssuePool &pool) {  // (no fixed pause: the pool says when every worker has gone to sleep)
    while (pool.n_sleeping() < pool.n_threads()) std::this_thread::yield();
}

// phases back to back, a gap in which the workers fall asleep, more phases; failures and exceptions on the way
static void run_phases(size_t n, bool threads) {
    Started st;
    IssuePool pool;
    set_hooks(pool, &st);
    std::vector<int> count(n, 0);
    std::vector<std::thread::id> who(n);
    int phase = 0;
    auto fn = [&](size_t k) -> int {
        if (phase == 0) who[k] = std::this_thread::get_id();
        else if (who[k] != std::this_thread::get_id()) return fail_with(5, "block moved to another thread");
        ++count[k];
        return 0;
    };
    auto all_ran = [&](const char *when) {
        for (size_t k = 0; k < n; ++k) CHECK(count[k] == phase, "%s: n %zu, block %zu ran %d times in %d phases", when, n, k, count[k], phase);
    };
    for (; phase < 400;) {
        const int rc = pool.run(n, fn, threads);
        ++phase;
        CHECK(rc == 0, "phase %d: status %d", phase, rc);
    }
    all_ran("back to back");
    CHECK(pool.n_threads() == (threads ? n - 1 : 0), "%zu threads for %zu blocks", pool.n_threads(), n);
    CHECK(st.hooks.load() == (int)pool.n_threads(), "%d start hooks", st.hooks.load());
    CHECK(who[0] == std::this_thread::get_id(), "block 0 is the caller's");
    for (size_t k = 1; k < n; ++k) {
        CHECK(threads ? who[k] != who[0] : who[k] == who[0], "block %zu on the wrong side", k);
        for (size_t j = 1; j < k && threads; ++j) CHECK(who[k] != who[j], "blocks %zu and %zu share a thread", j, k);
    }
    wait_until_asleep(pool);
    for (int i = 0; i < 300; ++i) {
        CHECK(pool.run(n, fn, threads) == 0, "a phase after the gap");
        ++phase;
    }
    all_ran("after the gap");

    // a failing block: its status and ITS text come back, whichever thread it ran on; the phase after it runs as ever
    for (size_t bad = 0; bad < n; ++bad) {
        std::vector<int> ran(n, 0);
        const int rc = pool.run(n, [&](size_t k) -> int {
            ++ran[k];
            if (k != bad) return 0;
            char text[32];
            snprintf(text, sizeof text, "block %zu says no", k);
            return fail_with(40 + (int)k, text);
        }, threads);
        char want[32];
        snprintf(want, sizeof want, "block %zu says no", bad);
        CHECK(rc == 40 + (int)bad, "failing block %zu: status %d", bad, rc);
        const char *text = pool.message() ? pool.message() : last_error;  // (NULL: this thread's own text holds it)
        CHECK(!strcmp(text, want), "failing block %zu: text '%s'", bad, text);
        CHECK((pool.message() != nullptr) == (threads && bad > 0), "who holds the text of block %zu", bad);
        for (size_t k = 0; k < n; ++k) CHECK(ran[k] == (threads || k <= bad ? 1 : 0), "failing block %zu: block %zu ran %d times", bad, k, ran[k]);
        CHECK(pool.run(n, fn, threads) == 0, "the phase after a failure");
        ++phase;
        all_ran("after a failure");
        CHECK(pool.message() == nullptr, "a clean phase holds no text");
    }
    // a throwing block: a status and a text, nothing terminates, nothing leaves run()
    for (size_t bad = 0; bad < n; ++bad) {
        const int rc = pool.run(n, [&](size_t k) -> int {
            if (k == bad) throw std::runtime_error("thrown in a phase");
            return 0;
        }, threads);
        CHECK(rc == 77 && pool.message() && strstr(pool.message(), "thrown in a phase"), "throwing block %zu: status %d, text '%s'", bad, rc,
              pool.message() ? pool.message() : "(null)");
        const int rc2 = pool.run(n, [&](size_t k) -> int {
            if (k == bad) throw 3;
            return 0;
        }, threads);
        CHECK(rc2 == 77 && pool.message(), "block %zu throwing an int: status %d", bad, rc2);
        CHECK(pool.run(n, fn, threads) == 0, "the phase after an exception");
        ++phase;
        all_ran("after an exception");
    }
    // threads off and on again: the workers are joined and started anew
    pool.stop();
    CHECK(pool.n_threads() == 0, "stop() leaves %zu threads", pool.n_threads());
    phase = 0;
    std::fill(count.begin(), count.end(), 0);
    for (; phase < 50;) {
        CHECK(pool.run(n, fn, threads) == 0, "a phase after a restart");
        ++phase;
    }
    all_ran("after a restart");
}

// the m-th worker cannot be started: everything on the caller, now and later, nothing left behind, nobody waited for
static void run_failed_start(size_t n, int m) {
    Started st;
    st.throw_at = m;
    IssuePool pool;
    set_hooks(pool, &st);
    std::vector<int> count(n, 0);
    const std::thread::id me = std::this_thread::get_id();
    bool elsewhere = false;
    auto fn = [&](size_t k) -> int {
        ++count[k];
        elsewhere = elsewhere || std::this_thread::get_id() != me;
        return 0;
    };
    for (int phase = 1; phase <= 30; ++phase) {
        CHECK(pool.run(n, fn, true) == 0, "n %zu, worker %d refused: phase %d", n, m, phase);
        CHECK(pool.n_threads() == 0, "n %zu, worker %d refused: %zu threads kept", n, m, pool.n_threads());
        for (size_t k = 0; k < n; ++k) CHECK(count[k] == phase, "n %zu, worker %d refused: block %zu ran %d times in %d phases", n, m, k, count[k], phase);
    }
    CHECK(!elsewhere, "work left the caller");
    CHECK(st.hooks.load() <= (int)n - 1, "the threads were started once (%d hooks)", st.hooks.load());
}

static void run_destruction(size_t n) {
    auto nothing = [](size_t) { return 0; };
    {
        IssuePool pool;  // destroyed while its workers sleep
        CHECK(pool.run(n, nothing, true) == 0, "a phase");
        wait_until_asleep(pool);
    }
    {
        IssuePool pool;  // ... and while they spin
        for (int i = 0; i < 20; ++i) CHECK(pool.run(n, nothing, true) == 0, "a phase");
    }
    {
        IssuePool pool;  // ... and before any phase
    }
}

int main() {
    for (size_t n : {(size_t)1, (size_t)2, (size_t)8}) {
        run_phases(n, true);
        run_phases(n, false);
        for (int m = 1; m < (int)n; ++m) run_failed_start(n, m);
        run_destruction(n);
    }
    {
        IssuePool pool;  // nothing to do is no failure
        CHECK(pool.run(0, [](size_t) { return 1; }, true) == 0, "n = 0");
    }
    printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
