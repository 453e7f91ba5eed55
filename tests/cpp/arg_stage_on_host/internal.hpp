// Stand-in for csrc/internal.hpp that lets tests/cpp/arg_stage_on_host/arg_stage_on_host.cpp compile csrc/arg_stage.hpp, unchanged,
// for the host: device memory is malloc (the k-th allocation from now on can be refused, as a full HBM refuses it), hipMemcpy is
// memcpy, hipDeviceSynchronize only counts, and hipPointerGetAttributes answers what the test scripted.  Everything is counted, so
// that the test can say what a call did and what it did not do.  Scratch has the interface of the library's (alloc, freed with
// its owner); the status codes are the library's own (include/sparsemat_hip.h).
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sparsemat_hip.h"

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
enum hipMemoryType { hipMemoryTypeUnregistered = 0, hipMemoryTypeHost = 1, hipMemoryTypeDevice = 2 };
struct hipPointerAttribute_t { hipMemoryType type; int device; };

namespace stub {
inline long long n_alloc = 0, n_free = 0, n_live = 0, n_sync = 0, n_h2d = 0, n_d2h = 0, n_attr = 0, n_last_error = 0;
inline long long refuse_alloc = -1;  // the allocation with this number (counted from the last reset) is refused; -1: none
inline int attr_device = -1;         // what hipPointerGetAttributes says: device memory of this device; -1: it does not know the pointer
inline char error[512] = "";
inline void reset() {
    n_alloc = n_free = n_sync = n_h2d = n_d2h = n_attr = n_last_error = 0;
    refuse_alloc = -1;
    attr_device = -1;
    error[0] = 0;
}
}  // namespace stub

inline hipError_t hipDeviceSynchronize() { ++stub::n_sync; return hipSuccess; }
inline hipError_t hipGetLastError() { ++stub::n_last_error; return hipSuccess; }
inline hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    if (kind == hipMemcpyHostToDevice) ++stub::n_h2d;
    if (kind == hipMemcpyDeviceToHost) ++stub::n_d2h;
    memcpy(dst, src, bytes);
    return hipSuccess;
}
inline hipError_t hipPointerGetAttributes(hipPointerAttribute_t *a, const void *) {
    ++stub::n_attr;
    if (stub::attr_device < 0) return hipErrorInvalidValue;
    a->type = hipMemoryTypeDevice;
    a->device = stub::attr_device;
    return hipSuccess;
}

namespace smh {

inline void note_thread() {}
inline int fail(int status, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(stub::error, sizeof stub::error, fmt, ap);
    va_end(ap);
    return status;
}
inline int hip_fail(hipError_t e, const char *what, const char *, int) {
    return fail(e == hipErrorOutOfMemory ? SMH_ERR_OOM : SMH_ERR_HIP, "HIP error %d in %s", (int)e, what);
}

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

inline hipError_t pool_malloc(void **out, size_t bytes) {
    if (stub::n_alloc++ == stub::refuse_alloc) return hipErrorOutOfMemory;
    *out = malloc(bytes);  // (exactly the bytes asked for: AddressSanitizer sees a copy that runs past them)
    if (!*out) return hipErrorOutOfMemory;
    ++stub::n_live;
    return hipSuccess;
}
inline hipError_t pool_free(void *p) {
    if (!p) return hipSuccess;
    ++stub::n_free;
    --stub::n_live;
    free(p);
    return hipSuccess;
}

class Scratch {
  public:
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { for (void *q : p_) (void)pool_free(q); }
    template <typename U> int alloc(U **out, size_t count) {
        SMH_HIP(pool_malloc((void **)out, (count ? count : 1) * sizeof(U)));
        p_.push_back(*out);
        return SMH_OK;
    }

  private:
    std::vector<void *> p_;
};

}  // namespace smh
