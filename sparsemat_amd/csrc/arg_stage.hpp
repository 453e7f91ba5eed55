// arg_stage.hpp -- the arrays of an entry point that exists as a host form and a _dev form ("a host array, or the caller's device
// array"), staged one way.  A host/_dev pair is one `*_common(..., bool on_device)`; it takes every array through an ArgStage:
//   in / out               the device pointer to work on: the caller's own (checked to live on the handle's device), or scratch
//                          that holds a copy of the host input / is copied back to the host output by finish().  NULL stays NULL.
//   callers_writes_first   the device-wide synchronisation that lets the caller's pending writes to its device arrays land
//                          (nothing in the host form: a host array is read when it is uploaded)
//   finish                 the host outputs go back, each once; an output of zero bytes is not copied
// Known differences, kept (each site says so where it opts out):
//   * assemble / replay and column_info check no device array and do no device-wide synchronisation in their _dev forms
//     (kUnchecked, no callers_writes_first): the arrays are read on the null stream, behind whatever the caller queued there.
//   * assemble / replay read the first two operations straight from the caller's arrays, before anything is staged.
//   * the permutations (permute, permute_symmetric) synchronise first and check afterwards, inside take_permutation (permute.hip).
//   * vec_permute synchronises device-wide in BOTH forms (vectors work on the null stream), by a call of its own.
//   * get_many answers zeros for a handle without rows after the checks and the synchronisations, without staging the queries.
//   * update_plan_execute stages host values in the plan's own reusable StageBuf (repeated executes do not allocate): it takes
//     only the check and the synchronisation from here.
#pragma once
#include "internal.hpp"

namespace smh {

// a device array of the caller must live on the handle's device (where the runtime can tell)
inline int check_dev_array(const void *p, int device, const char *what) {
    if (!p) return SMH_OK;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return SMH_OK; }
    if (a.type == hipMemoryTypeDevice && a.device != device)
        return fail(SMH_ERR_INVALID, "%s lives on device %d, the handle on device %d", what, a.device, device);
    return SMH_OK;
}

class ArgStage {
  public:
    static constexpr int kUnchecked = -1;  // in place of the handle's device: this pair checks no device array
    ArgStage(bool on_device, int device) : on_device_(on_device), device_(device) {}
    Scratch &scratch() { return scr_; }  // further device scratch of the call, freed with the staged copies

    int check(const void *p, const char *what) const {
        return on_device_ && device_ != kUnchecked ? check_dev_array(p, device_, what) : SMH_OK;
    }
    int in(const void *p, size_t bytes, const char *what, const void **dev) {
        void *d = nullptr;
        *dev = nullptr;
        SMH_TRY(take(const_cast<void *>(p), bytes, what, &d));
        if (d != p && bytes) SMH_HIP(hipMemcpy(d, p, bytes, hipMemcpyHostToDevice));
        *dev = d;
        return SMH_OK;
    }
    int out(void *p, size_t bytes, const char *what, void **dev) {
        if (!on_device_ && p && n_back_ == kMaxOut) return fail(SMH_ERR_INVALID, "ArgStage: more than %d host outputs", kMaxOut);
        SMH_TRY(take(p, bytes, what, dev));
        if (*dev != p) back_[n_back_++] = {p, *dev, bytes};
        return SMH_OK;
    }
    int callers_writes_first() const {
        if (on_device_) SMH_HIP(hipDeviceSynchronize());
        return SMH_OK;
    }
    int finish() {
        const int n = n_back_;
        n_back_ = 0;
        for (int i = 0; i < n; ++i)
            if (back_[i].bytes) SMH_HIP(hipMemcpy(back_[i].host, back_[i].dev, back_[i].bytes, hipMemcpyDeviceToHost));
        return SMH_OK;
    }

  private:
    int take(void *p, size_t bytes, const char *what, void **dev) {  // the caller's pointer, checked; or scratch in a host array's place
        *dev = p;
        if (on_device_ || !p) return check(p, what);
        char *q = nullptr;
        *dev = nullptr;
        SMH_TRY(scr_.alloc(&q, bytes));
        *dev = q;
        return SMH_OK;
    }
    static constexpr int kMaxOut = 3;  // (column_info has the most)
    struct Back { void *host, *dev; size_t bytes; };
    const bool on_device_;
    const int device_;
    Scratch scr_;
    Back back_[kMaxOut];
    int n_back_ = 0;
};

}  // namespace smh
