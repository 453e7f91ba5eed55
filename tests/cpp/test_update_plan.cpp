// The reference's SparseMatCRS test matrix (lostinc0de/sparsemat src/lib.rs:114-154) built by add_to, then re-assembled through
// UpdatePlan of the C++ mirror (include/sparsemat.hpp): from zero it reproduces the assembled values and the product, without
// from_zero it equals apply, and a moved-from plan is inert.  Built and run by tests/test_cpp_update_plan_gpu.py.
#include <cstdio>
#include <utility>
#include <vector>

#include "sparsemat.hpp"

using namespace sparsemat;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static std::vector<float> values_of(const SparseMatCRS<float> &m) {
    std::vector<uint32_t> off, col;
    std::vector<float> val;
    m.raw_parts(off, col, val);
    return val;
}

int main() {
    const std::vector<uint32_t> rows{0, 2, 1, 3, 3}, cols{1, 2, 2, 2, 3};
    const std::vector<float> vals{4.2f, 2.12f, 4.12f, 1.12f, 5.12f};
    auto sp = SparseMatCRS<float>::new_empty();
    for (size_t k = 0; k < vals.size(); ++k) sp.add_to(rows[k], cols[k], vals[k]);
    const std::vector<float> assembled{4.2f, 4.12f, 2.12f, 5.12f, 1.12f};
    CHECK(values_of(sp) == assembled);

    auto plan = sp.update_plan(rows, cols);
    CHECK(plan.n_ops() == 5 && plan.n_targets() == 5 && plan.n_live_ops() == 5);
    sp *= 3.0f;  // whatever is stored: from_zero does not read it
    plan.execute(vals, true);
    CHECK(values_of(sp) == assembled);
    auto x = DenseVec<float>::from_vec({2.0f, 4.8f, 1.2f, 3.4f});
    CHECK((sp * x).get(0) == 20.16f);  // assert_eq!(mvp.get(0), 20.16)

    // without from_zero: apply
    const std::vector<float> more{0.5f, -1.0f, 0.25f, 2.0f, -0.75f};
    auto ref = sp.clone();
    ref.apply(rows, cols, more);
    plan.execute(more);
    CHECK(values_of(sp) == values_of(ref));

    // a stream with repeats and a set: everything in front of the set is dropped
    const std::vector<uint32_t> r2{3, 0, 3}, c2{2, 1, 2};
    auto plan2 = sp.update_plan(r2, c2, {0, 0, 1});
    CHECK(plan2.n_targets() == 2 && plan2.n_live_ops() == 2);
    ref.apply(r2, c2, {1.0f, 0.5f, 7.0f}, {0, 0, 1});
    plan2.execute({1.0f, 0.5f, 7.0f});
    CHECK(values_of(sp) == values_of(ref) && sp.get(3, 2) == 7.0f);

    // a moved-from plan is inert; the plan it was moved into works
    UpdatePlan<float> moved = std::move(plan);
    CHECK(plan.handle() == nullptr);
    const auto before = values_of(sp);
    plan.execute(vals, true);
    CHECK(values_of(sp) == before);
    moved.execute(vals, true);
    CHECK(values_of(sp) == assembled);

    // bound to its matrix: a clone refuses the plan and keeps its values
    int status = 0;
    auto other = sp.clone();
    other.scale(2.0f);
    const auto other_before = values_of(other);
    status = smh_update_plan_execute(moved.handle(), other.handle(), vals.data(), 1);
    CHECK(status == SMH_ERR_INVALID && values_of(other) == other_before);
    // ... and to its structure: stale once the rows were sorted
    status = 0;
    try {
        UpdatePlan<float> p3 = other.update_plan(rows, cols);
        other.sort_rows();
        p3.execute(vals);
    } catch (const Panic &p) {
        status = p.status;
    }
    CHECK(status == SMH_ERR_INVALID);
    status = 0;
    try {
        sp.update_plan({0}, {0});  // (0, 0) is not an entry
    } catch (const Panic &p) {
        status = p.status;
    }
    CHECK(status == SMH_ERR_INVALID);
    std::printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
