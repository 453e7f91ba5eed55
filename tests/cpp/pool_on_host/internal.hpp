// Stand-in for csrc/internal.hpp that lets tests/cpp/pool_on_host/pool_on_host.cpp compile csrc/pool.hip, unchanged, for the host:
// the runtime is malloc with a byte budget per "device" (a request beyond it is refused, as a full HBM refuses it), the current
// device is one integer per thread, and hipDeviceSynchronize / hipGetLastError only count.  Everything the stub keeps is behind
// its own mutex or atomic, so that whatever ThreadSanitizer reports is pool.hip's.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <unordered_map>

#define SMH_OK 0

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorMemoryAllocation = 2, hipErrorInvalidDevice = 101 };

namespace stub {
constexpr int kDevices = 2;
struct Block { size_t bytes; int device; };
struct Runtime {
    std::mutex mu;
    std::unordered_map<void *, Block> out;   // what hipMalloc has handed out and hipFree has not taken back
    size_t used[kDevices] = {};
    size_t budget = ~size_t(0);              // per device
    size_t double_frees = 0;
};
inline Runtime &rt() { static Runtime r; return r; }
inline std::atomic<long long> n_refused{0}, n_sync{0}, n_last_error{0};
inline thread_local int t_device = 0;
}  // namespace stub

inline hipError_t hipGetDevice(int *d) { *d = stub::t_device; return hipSuccess; }
inline hipError_t hipSetDevice(int d) {
    if (d < 0 || d >= stub::kDevices) return hipErrorInvalidDevice;
    stub::t_device = d;
    return hipSuccess;
}
inline hipError_t hipDeviceSynchronize() { ++stub::n_sync; return hipSuccess; }
inline hipError_t hipGetLastError() { ++stub::n_last_error; return hipSuccess; }
inline hipError_t hipMalloc(void **out, size_t bytes) {
    stub::Runtime &R = stub::rt();
    const int d = stub::t_device;
    std::lock_guard<std::mutex> g(R.mu);
    if (R.used[d] + bytes > R.budget) { ++stub::n_refused; return hipErrorOutOfMemory; }
    void *p = malloc(bytes ? bytes : 1);
    if (!p) return hipErrorOutOfMemory;
    R.used[d] += bytes;
    R.out.emplace(p, stub::Block{bytes, d});
    *out = p;
    return hipSuccess;
}
inline hipError_t hipFree(void *p) {
    if (!p) return hipSuccess;
    stub::Runtime &R = stub::rt();
    std::lock_guard<std::mutex> g(R.mu);
    auto it = R.out.find(p);
    if (it == R.out.end()) { ++R.double_frees; return hipErrorInvalidValue; }
    R.used[it->second.device] -= it->second.bytes;
    R.out.erase(it);
    free(p);
    return hipSuccess;
}

namespace smh {
inline void note_thread() {}   // (the library counts its host threads here: nothing to count without a runtime)
hipError_t pool_malloc(void **out, size_t bytes);
hipError_t pool_free(void *p);
long long pool_thread_net_bytes();
}  // namespace smh
extern "C" {
int smh_pool_trim(void);
int smh_pool_stats(size_t *kept_bytes_out, size_t *live_bytes_out);
}
