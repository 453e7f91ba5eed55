// par_issue.hpp -- the ISSUING HOST THREADS of a partitioned handle, one per local block.  Host only (the device a worker binds to
// is the business of a start hook), so the class compiles and is tested as a program of its own (tests/test_par_issue_on_host.py).
//
// The solver and the product step are sequences of PHASES -- "every block does X on its streams" -- separated by the points where one
// block's stream must wait for an event another block has recorded (the record has to be issued, on the host, before the wait is).
// Round 3 issued every phase from the caller's thread: ~30 runtime calls per block and CG iteration, 0.84-0.92 ms per iteration with
// 8 blocks on one device against 0.27 ms of kernels.  With the threads on, block k's calls are issued by thread k (block 0's by the
// caller), all at once, and the phases meet at a host barrier; the streams, events, kernels and their order per block are unchanged,
// so every result is bit for bit the same.  (An earlier attempt to get rid of the calls -- ONE hipGraph captured across all blocks'
// streams -- died inside the runtime during capture from 4 blocks on; this needs nothing of the graph machinery.)
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <exception>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

namespace smh {

class IssuePool {
public:
    struct Hooks {
        void (*start)(void *ctx, size_t k) = nullptr;  // on worker k before its first phase; a throw counts as a thread that did not start
        const char *(*message)() = nullptr;            // the calling thread's error text, read after an fn that failed
        void *ctx = nullptr;
        int thrown = -1;                               // the status an exception out of fn becomes
    };
    Hooks hooks;

    IssuePool() = default;
    IssuePool(const IssuePool &) = delete;
    IssuePool &operator=(const IssuePool &) = delete;
    ~IssuePool() { stop(); }

    // fn(k) for every k in [0, n): with `threads`, concurrently -- worker k runs fn(k), the caller fn(0) -- returning when all have
    // returned (a HOST barrier: what fn issued is on the streams, not necessarily executed); else one after the other on the caller,
    // up to the first failure.  Returns the first failure's status (the caller's before the workers', those by k); its text is
    // message() unless that is NULL, which says the calling thread's own error text already holds it.  Nothing is thrown: an
    // exception out of fn is a failure with status hooks.thrown.  Threads that cannot be had are not an error: what was started is
    // torn down, and this and every later call run on the caller.
    template <class F> int run(size_t n, F &&fn, bool threads) {
        fn_ = [](void *c, size_t k) -> int { return (*static_cast<typename std::remove_reference<F>::type *>(c))(k); };
        ctx_ = const_cast<void *>(static_cast<const void *>(&fn));
        held_ = nullptr;
        if (threads && n > 1 && !fallback_ && th_.size() != n - 1) start(n - 1);
        if (!threads || n <= 1 || fallback_) {
            for (size_t k = 0; k < n; ++k) {
                const int rc = call(k, msg0_, false);
                if (rc != 0) return hold(rc, msg0_);
            }
            return 0;
        }
        pending_.store((uint32_t)th_.size(), std::memory_order_release);
        {
            // (the generation changes under the lock a sleeper checks it under: no wake-up is lost)
            std::lock_guard<std::mutex> lk(mu_);
            gen_.fetch_add(1, std::memory_order_acq_rel);
        }
        if (sleepers_.load(std::memory_order_acquire)) cv_.notify_all();
        const int rc0 = call(0, msg0_, false);  // block 0 is the caller's
        while (pending_.load(std::memory_order_acquire)) __builtin_ia32_pause();
        if (rc0 != 0) return hold(rc0, msg0_);
        for (size_t k = 1; k < n; ++k)
            if (rc_[k] != 0) return hold(rc_[k], msg_[k]);
        return 0;
    }
    const char *message() const { return held_; }
    size_t n_threads() const { return th_.size(); }
    size_t n_sleeping() const { return sleepers_.load(std::memory_order_acquire); }  // (idle workers stop spinning after a few ms)

    // joins the workers (sleeping or spinning); the next threaded run starts new ones
    void stop() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_.store(true, std::memory_order_release);
        }
        cv_.notify_all();
        for (std::thread &t : th_) t.join();
        th_.clear();
        stop_.store(false, std::memory_order_release);
    }

private:
    std::vector<std::thread> th_;         // worker k is th_[k - 1]
    std::mutex mu_;
    std::condition_variable cv_;
    std::atomic<uint64_t> gen_{0};        // phases handed out so far
    std::atomic<uint32_t> pending_{0};    // workers still inside the current phase
    std::atomic<uint32_t> sleepers_{0};   // workers blocked on cv_ (a phase start wakes them)
    std::atomic<uint32_t> reported_{0};   // workers that have run their start hook
    std::atomic<bool> stop_{false}, start_failed_{false};
    bool fallback_ = false;               // threads could not be had: everything on the caller from now on
    int (*fn_)(void *, size_t) = nullptr;
    void *ctx_ = nullptr;
    std::vector<int> rc_;
    std::vector<std::string> msg_;        // (the error text is thread-local: a worker hands its own to the caller)
    std::string msg0_;
    const char *held_ = nullptr;

    int hold(int rc, const std::string &msg) {
        held_ = msg.empty() ? nullptr : msg.c_str();
        return rc;
    }

    // fn(k) with nothing thrown; msg: the failure's text when it has to travel (a worker's, an exception's), else empty
    int call(size_t k, std::string &msg, bool on_worker) noexcept {
        msg.clear();
        try {
            const int rc = fn_(ctx_, k);
            if (rc != 0 && on_worker && hooks.message) msg = hooks.message();
            return rc;
        } catch (const std::exception &e) {
            try { msg = std::string("exception while issuing a block's calls: ") + e.what(); } catch (...) { msg.clear(); }
        } catch (...) {
            try { msg = "exception while issuing a block's calls"; } catch (...) { msg.clear(); }
        }
        return hooks.thrown;
    }

    void start(size_t n_workers) noexcept {
        stop();
        reported_.store(0, std::memory_order_release);
        start_failed_.store(false, std::memory_order_release);
        try {
            rc_.assign(n_workers + 1, 0);
            msg_.assign(n_workers + 1, std::string());
            th_.reserve(n_workers);
            for (size_t k = 1; k <= n_workers; ++k) th_.emplace_back(&IssuePool::worker, this, k);
        } catch (...) {
            start_failed_.store(true, std::memory_order_release);
        }
        // (every worker that exists reports before the first phase: it has read the generation it starts from by then)
        while (reported_.load(std::memory_order_acquire) < th_.size()) std::this_thread::yield();
        if (start_failed_.load(std::memory_order_acquire)) {
            stop();
            fallback_ = true;
        }
    }

    void worker(size_t k) noexcept {
        try {
            if (hooks.start) hooks.start(hooks.ctx, k);
        } catch (...) {
            start_failed_.store(true, std::memory_order_release);
        }
        uint64_t seen = gen_.load(std::memory_order_acquire);
        reported_.fetch_add(1, std::memory_order_acq_rel);
        for (;;) {
            // wait for the next phase: spin while the solver is running (phases follow each other within microseconds), sleep otherwise
            unsigned spins = 0;
            while (gen_.load(std::memory_order_acquire) == seen && !stop_.load(std::memory_order_acquire)) {
                if (++spins < 200000u) {
                    __builtin_ia32_pause();
                } else {
                    std::unique_lock<std::mutex> lk(mu_);
                    sleepers_.fetch_add(1, std::memory_order_acq_rel);
                    cv_.wait(lk, [&] { return gen_.load(std::memory_order_acquire) != seen || stop_.load(std::memory_order_acquire); });
                    sleepers_.fetch_sub(1, std::memory_order_acq_rel);
                    spins = 0;
                }
            }
            if (stop_.load(std::memory_order_acquire)) return;
            seen = gen_.load(std::memory_order_acquire);
            rc_[k] = call(k, msg_[k], true);
            pending_.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
};

}  // namespace smh
