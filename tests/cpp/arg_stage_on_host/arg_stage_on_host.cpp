// csrc/arg_stage.hpp, unchanged (the test copies it here), on the stand-in runtime of internal.hpp, under AddressSanitizer and
// UBSan: what the host form and the _dev form of an entry point get from ArgStage, what each call does and does not do, and that
// a refused allocation at any argument leaves nothing behind.
#include "arg_stage.hpp"

#include <cstdio>

using smh::ArgStage;

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            printf("FAILED line %d: %s\n", __LINE__, #cond);               \
        }                                                                  \
    } while (0)

struct Buffers {
    uint32_t rows[5] = {7, 0, 0xFFFFFFFFu, 3, 3};
    double vals[3] = {1.5, -0.0, 1e300};
    uint8_t none = 9;           // a non-null argument of zero bytes
    uint32_t out_a[4];
    float out_b[2];
    uint8_t out_none = 0x5A;    // a non-null output of zero bytes
    Buffers() { memset(out_a, 0xEE, sizeof out_a); memset(out_b, 0xEE, sizeof out_b); }
    bool outputs_untouched() const {
        const unsigned char *a = (const unsigned char *)out_a, *b = (const unsigned char *)out_b;
        for (size_t i = 0; i < sizeof out_a; ++i) if (a[i] != 0xEE) return false;
        for (size_t i = 0; i < sizeof out_b; ++i) if (b[i] != 0xEE) return false;
        return out_none == 0x5A;
    }
};

struct Staged { const void *rows = nullptr, *vals = nullptr, *null_in = nullptr, *none = nullptr; void *a = nullptr, *b = nullptr, *null_out = nullptr, *out_none = nullptr; };

// the staging of one entry point, as a *_common writes it: inputs, outputs, "the caller's writes come first"
int stage_all(ArgStage &st, Buffers &h, Staged &d, bool sync = true) {
    SMH_TRY(st.in(h.rows, sizeof h.rows, "rows", &d.rows));
    SMH_TRY(st.in(h.vals, sizeof h.vals, "vals", &d.vals));
    SMH_TRY(st.in(nullptr, 64, "ops", &d.null_in));
    SMH_TRY(st.in(&h.none, 0, "none", &d.none));
    SMH_TRY(st.out(h.out_a, sizeof h.out_a, "out_a", &d.a));
    SMH_TRY(st.out(nullptr, 64, "perm_out", &d.null_out));
    SMH_TRY(st.out(h.out_b, sizeof h.out_b, "out_b", &d.b));
    SMH_TRY(st.out(&h.out_none, 0, "out_none", &d.out_none));
    if (sync) SMH_TRY(st.callers_writes_first());
    return SMH_OK;
}
constexpr int kAllocs = 6;  // of stage_all in the host form: every non-null argument, the two of zero bytes included

void host_form() {
    stub::reset();
    Buffers h;
    {
        ArgStage st(false, 0);
        Staged d;
        CHECK(stage_all(st, h, d) == SMH_OK);
        // inputs: device copies, byte for byte; NULL stays NULL; nothing is asked about a host pointer; no device-wide sync
        CHECK(d.rows && d.rows != h.rows && !memcmp(d.rows, h.rows, sizeof h.rows));
        CHECK(d.vals && d.vals != h.vals && !memcmp(d.vals, h.vals, sizeof h.vals));
        CHECK(d.null_in == nullptr && d.null_out == nullptr);
        CHECK(d.none && d.none != &h.none && d.out_none && d.out_none != &h.out_none);
        CHECK(stub::n_h2d == 2 && stub::n_d2h == 0);  // (the zero-byte input is not copied)
        CHECK(stub::n_alloc == kAllocs && stub::n_attr == 0 && stub::n_sync == 0);
        // outputs: scratch; the host arrays are written by finish() alone, each once
        CHECK(d.a && d.a != h.out_a && d.b && d.b != h.out_b);
        const uint32_t a[4] = {4, 3, 2, 1};
        const float b[2] = {0.5f, -2.0f};
        memcpy(d.a, a, sizeof a);
        memcpy(d.b, b, sizeof b);
        CHECK(h.outputs_untouched());
        CHECK(st.finish() == SMH_OK);
        CHECK(!memcmp(h.out_a, a, sizeof a) && !memcmp(h.out_b, b, sizeof b) && h.out_none == 0x5A);
        CHECK(stub::n_d2h == 2);  // (the zero-byte output is not copied)
        memset(h.out_a, 0xEE, sizeof h.out_a);
        CHECK(st.finish() == SMH_OK);
        CHECK(stub::n_d2h == 2 && ((unsigned char *)h.out_a)[0] == 0xEE);
        CHECK(stub::n_sync == 0 && stub::n_live == kAllocs);
    }
    CHECK(stub::n_live == 0 && stub::n_free == kAllocs);
}

void device_form() {
    Buffers h;  // (stands for the caller's device arrays)
    // the caller's pointers as given; no allocation, no copy; one device-wide sync when asked
    for (int device : {0, ArgStage::kUnchecked}) {
        for (bool sync : {true, false}) {
            stub::reset();
            stub::attr_device = 0;
            ArgStage st(true, device);
            Staged d;
            CHECK(stage_all(st, h, d, sync) == SMH_OK);
            CHECK(d.rows == h.rows && d.vals == h.vals && d.null_in == nullptr && d.none == &h.none);
            CHECK(d.a == h.out_a && d.b == h.out_b && d.null_out == nullptr && d.out_none == &h.out_none);
            CHECK(st.finish() == SMH_OK);
            CHECK(stub::n_alloc == 0 && stub::n_h2d == 0 && stub::n_d2h == 0 && h.outputs_untouched());
            CHECK(stub::n_sync == (sync ? 1 : 0));
            CHECK(stub::n_attr == (device == ArgStage::kUnchecked ? 0 : 6));  // every non-null pointer is asked about, or none
        }
    }
    // a pointer on another device: refused at its argument, before any sync
    stub::reset();
    stub::attr_device = 1;
    {
        ArgStage st(true, 0);
        Staged d;
        CHECK(stage_all(st, h, d) == SMH_ERR_INVALID);
        CHECK(!strcmp(stub::error, "rows lives on device 1, the handle on device 0"));
        CHECK(stub::n_attr == 1 && stub::n_sync == 0 && stub::n_alloc == 0);
        void *p = nullptr;
        CHECK(st.out(h.out_a, sizeof h.out_a, "perm_out", &p) == SMH_ERR_INVALID);
        CHECK(!strcmp(stub::error, "perm_out lives on device 1, the handle on device 0"));
        CHECK(st.check(h.vals, "values") == SMH_ERR_INVALID && st.check(nullptr, "values") == SMH_OK);
        CHECK(stub::n_sync == 0);
    }
    // ... not by a pair that checks no device array, and not where the runtime does not know the pointer
    {
        ArgStage st(true, ArgStage::kUnchecked);
        Staged d;
        CHECK(stage_all(st, h, d) == SMH_OK && stub::n_sync == 1);
    }
    stub::reset();
    {
        ArgStage st(true, 0);
        Staged d;
        CHECK(stage_all(st, h, d) == SMH_OK && stub::n_attr == 6 && stub::n_last_error == 6);
    }
    // the host form asks nothing, whatever the runtime would say
    stub::reset();
    stub::attr_device = 1;
    {
        ArgStage st(false, 0);
        const void *p = nullptr;
        CHECK(st.in(h.rows, sizeof h.rows, "rows", &p) == SMH_OK && st.check(h.rows, "rows") == SMH_OK && stub::n_attr == 0);
    }
    CHECK(stub::n_live == 0);
}

void refused_allocation() {
    for (int k = 0; k < kAllocs; ++k) {
        stub::reset();
        stub::refuse_alloc = k;
        Buffers h;
        {
            ArgStage st(false, 0);
            Staged d;
            CHECK(stage_all(st, h, d) == SMH_ERR_OOM);  // (the entry point returns here: finish() is never reached)
            CHECK(stub::n_alloc == k + 1 && stub::n_live == k);
            CHECK(stub::n_sync == 0 && stub::n_d2h == 0 && h.outputs_untouched());
            if (k == 0) CHECK(d.rows == nullptr);
        }
        CHECK(stub::n_live == 0);
    }
    // more host outputs than any pair has: refused, nothing written past the table
    stub::reset();
    Buffers h;
    {
        ArgStage st(false, 0);
        void *p = nullptr;
        for (int i = 0; i < 3; ++i) CHECK(st.out(h.out_a, sizeof h.out_a, "out_a", &p) == SMH_OK);
        CHECK(st.out(h.out_b, sizeof h.out_b, "out_b", &p) == SMH_ERR_INVALID && stub::n_alloc == 3);
    }
    CHECK(stub::n_live == 0);
}

}  // namespace

int main() {
    host_form();
    device_form();
    refused_allocation();
    CHECK(stub::n_live == 0);
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ok (0 failures)\n");
    return 0;
}
