// sparsemat.hpp -- C++ host-side mirror of the reference crate's interface for the hot path, header-only
// over the C ABI of libsparsemat_hip.so (include/sparsemat_hip.h).
//
// The reference is a Rust crate; this image has no Rust toolchain, so the tested host side above the C
// ABI is this C++ mirror (same names, argument meaning and failure behaviour as the reference) plus the
// Python mirror used by the tests/bench (sparsemat_amd/).  The Rust shim a maintainer would add is in
// rust/ and INTEGRATION.md.
//
//   sparsemat::DenseVec<T>            <- densevec.rs:5-140, vector.rs:5-64
//   sparsemat::SparseMatCRS<T>        <- sparsemat_crs.rs (Index = u32), SparseMatrix::mvp sparsematrix.rs:146-158
//   sparsemat::ConjugateGradient      <- linearsolver.rs:6-61
//   sparsemat::Panic                  <- the reference's panic!() texts (linearsolver.rs:31,35; densevec.rs:53,62)
//
// T is float or double.  Everything computes on the device; there is no CPU fallback.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "sparsemat_hip.h"

namespace sparsemat {

struct Panic : std::runtime_error {
    int status;
    Panic(int st, const std::string &msg) : std::runtime_error(msg), status(st) {}
};

namespace detail {
inline void check(int status) {
    if (status != SMH_OK) {
        std::string msg = smh_last_error();
        if (msg.empty()) msg = smh_status_string(status);
        throw Panic(status, msg);
    }
}
template <typename T> struct dtype_of;
template <> struct dtype_of<float> { static constexpr smh_dtype value = SMH_F32; };
template <> struct dtype_of<double> { static constexpr smh_dtype value = SMH_F64; };
}  // namespace detail

template <typename T>
class DenseVec {
  public:
    using Value = T;
    DenseVec() { detail::check(smh_vec_create(detail::dtype_of<T>::value, 0, &h_)); }
    explicit DenseVec(size_t n) { detail::check(smh_vec_create(detail::dtype_of<T>::value, n, &h_)); }
    // Vector::from_vec (densevec.rs:30-34)
    static DenseVec from_vec(const std::vector<T> &v) {
        DenseVec r(nullptr);
        detail::check(smh_vec_from_host(detail::dtype_of<T>::value, v.size(), v.data(), &r.h_));
        return r;
    }
    DenseVec(const DenseVec &o) : DenseVec(o.dim()) { detail::check(smh_vec_copy(h_, o.h_)); }  // Clone
    DenseVec(DenseVec &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DenseVec &operator=(DenseVec o) { std::swap(h_, o.h_); return *this; }
    ~DenseVec() { smh_vec_destroy(h_); }

    size_t dim() const { return smh_vec_dim(h_); }  // densevec.rs:36-38
    std::vector<T> to_vec() const {                 // iter().collect()
        std::vector<T> v(dim());
        detail::check(smh_vec_download(h_, v.data()));
        return v;
    }
    T get(size_t i) const {                         // densevec.rs:40-42 (bounds checked)
        if (i >= dim()) throw Panic(SMH_ERR_INDEX_RANGE, "index out of bounds");
        return to_vec()[i];
    }
    void add(const DenseVec &rhs) { detail::check(smh_vec_add(h_, rhs.h_)); }   // :51-58
    void sub(const DenseVec &rhs) { detail::check(smh_vec_sub(h_, rhs.h_)); }   // :60-67
    void scale(T a) { detail::check(smh_vec_scale(h_, (double)a)); }            // :69-73
    T inner_prod(const DenseVec &rhs) const {                                   // vector.rs:50-53
        double out = 0;
        detail::check(smh_vec_dot(h_, rhs.h_, &out));
        return (T)out;
    }
    T norm_squared() const {                                                    // vector.rs:56-58
        double out = 0;
        detail::check(smh_vec_norm_squared(h_, &out));
        return (T)out;
    }
    double norm() const { return std::sqrt((double)norm_squared()); }           // vector.rs:61-63
    // an extension (see SparseMatCRS::permute): out[i] = (*this)[perm[i]], or with `inverse` out[perm[i]] = (*this)[i]
    DenseVec permute(const std::vector<uint32_t> &perm, bool inverse = false) const {
        static const uint32_t none = 0;
        DenseVec r(dim());
        detail::check(smh_vec_permute(r.h_, h_, perm.empty() ? &none : perm.data(), perm.size(), inverse ? 1 : 0));
        return r;
    }
    // operator sugar (densevec.rs:76-140)
    DenseVec &operator+=(const DenseVec &r) { add(r); return *this; }
    DenseVec &operator-=(const DenseVec &r) { sub(r); return *this; }
    DenseVec &operator*=(T a) { scale(a); return *this; }
    friend DenseVec operator+(DenseVec l, const DenseVec &r) { l += r; return l; }
    friend DenseVec operator-(DenseVec l, const DenseVec &r) { l -= r; return l; }
    friend DenseVec operator*(DenseVec l, T a) { l *= a; return l; }
    friend T operator*(const DenseVec &l, const DenseVec &r) { return l.inner_prod(r); }

    // an extension (smh_vec_cast): a new vector of U, converted on the device -- f64 -> f32 to nearest even, f32 -> f64 exactly
    template <typename U> DenseVec<U> cast() const {
        DenseVec<U> r(dim());
        detail::check(smh_vec_cast(h_, r.handle()));
        return r;
    }

    smh_vec *handle() const { return h_; }

  private:
    explicit DenseVec(std::nullptr_t) : h_(nullptr) {}
    smh_vec *h_ = nullptr;
};

// k DenseVecs of one dimension held against one matrix (smh_mvec): interleaved on the device, k vectors of n entries on the host.
// The reference has no such type -- its mvp (sparsematrix.rs:146-158) is generic over the vector and called once per right-hand
// side; SparseMatCRS::mvp_many gives the same k results, bit for bit, from one sweep over the matrix.  Move-only.
template <typename T>
class MultiVec {
  public:
    using Value = T;
    MultiVec(size_t n, size_t k) { detail::check(smh_mvec_create(detail::dtype_of<T>::value, n, k, &h_)); }  // zeros
    explicit MultiVec(const std::vector<std::vector<T>> &vecs) {
        const size_t n = vecs.empty() ? 0 : vecs[0].size();
        std::vector<T> flat;
        flat.reserve(n * vecs.size());
        for (const auto &v : vecs) {
            if (v.size() != n) throw Panic(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
            flat.insert(flat.end(), v.begin(), v.end());
        }
        detail::check(smh_mvec_from_host(detail::dtype_of<T>::value, n, vecs.size(), flat.data(), &h_));
    }
    MultiVec(MultiVec &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    MultiVec &operator=(MultiVec &&o) noexcept { std::swap(h_, o.h_); return *this; }
    MultiVec(const MultiVec &) = delete;
    ~MultiVec() { smh_mvec_destroy(h_); }

    size_t dim() const { return smh_mvec_dim(h_); }      // every vector's dim() (densevec.rs:36-38)
    size_t count() const { return smh_mvec_count(h_); }  // k
    std::vector<std::vector<T>> to_vecs() const {
        const size_t n = dim(), k = count();
        std::vector<T> flat(n * k);
        detail::check(smh_mvec_download(h_, flat.data()));
        std::vector<std::vector<T>> out(k);
        for (size_t c = 0; c < k; ++c) out[c].assign(flat.begin() + c * n, flat.begin() + (c + 1) * n);
        return out;
    }
    DenseVec<T> column(size_t c) const {
        DenseVec<T> v(dim());
        detail::check(smh_mvec_get_column(h_, c, v.handle()));
        return v;
    }
    void set_column(size_t c, const DenseVec<T> &v) { detail::check(smh_mvec_set_column(h_, c, v.handle())); }

    // the per-column BLAS-1 (densevec.rs:51-73, vector.rs:50-58, k times): in place, one rounding per operation; dot and
    // norm_squared give one f64 per column, each summed in a fixed order that depends on dim() alone
    MultiVec copy() const {  // clone() (densevec.rs:9 derive)
        MultiVec ret(dim(), count());
        detail::check(smh_mvec_copy(ret.h_, h_));
        return ret;
    }
    void add(const MultiVec &o) { detail::check(smh_mvec_add(h_, o.h_)); }
    void sub(const MultiVec &o) { detail::check(smh_mvec_sub(h_, o.h_)); }
    void scale(const std::vector<double> &factors) {  // column c times T(factors[c])
        if (factors.size() != count()) throw Panic(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
        detail::check(smh_mvec_scale(h_, factors.data()));
    }
    std::vector<double> dot(const MultiVec &o) const {
        std::vector<double> out(count());
        detail::check(smh_mvec_dot(h_, o.h_, out.data()));
        return out;
    }
    std::vector<double> norm_squared() const {
        std::vector<double> out(count());
        detail::check(smh_mvec_norm_squared(h_, out.data()));
        return out;
    }

    smh_mvec *handle() const { return h_; }

  private:
    smh_mvec *h_ = nullptr;
};

template <typename T> class SparseMatCRS;

// A reusable update plan (smh_update_plan): the targets and the sorted order of one (rows, cols, ops) stream on one SparseMatCRS,
// made by SparseMatCRS::update_plan.  execute(values) leaves what apply(rows, cols, values, ops) leaves, bit for bit, in one
// gather-and-fold pass; from_zero folds every targeted entry from +0 ("zero, then assemble").  Move-only; a moved-from plan is
// inert (execute does nothing).  The matrix must outlive every execute, not the plan.
template <typename T>
class UpdatePlan {
  public:
    UpdatePlan(UpdatePlan &&o) noexcept : p_(o.p_), m_(o.m_), n_(o.n_) { o.p_ = nullptr; o.m_ = nullptr; o.n_ = 0; }
    UpdatePlan &operator=(UpdatePlan &&o) noexcept { std::swap(p_, o.p_); std::swap(m_, o.m_); std::swap(n_, o.n_); return *this; }
    UpdatePlan(const UpdatePlan &) = delete;
    ~UpdatePlan() { smh_update_plan_destroy(p_); }

    void execute(const std::vector<T> &values, bool from_zero = false) {
        if (!p_) return;
        if (values.size() != n_) throw Panic(SMH_ERR_INVALID, "values and the plan's stream differ in length");
        detail::check(smh_update_plan_execute(p_, m_, values.data(), from_zero ? 1 : 0));
    }
    size_t n_ops() const { return n_; }
    size_t n_targets() const { return stat(1); }
    size_t n_live_ops() const { return stat(2); }
    smh_update_plan *handle() const { return p_; }

  private:
    friend class SparseMatCRS<T>;
    UpdatePlan() = default;
    size_t stat(int which) const {
        size_t v[3] = {0, 0, 0};
        if (p_) detail::check(smh_update_plan_stats(p_, &v[0], &v[1], &v[2], nullptr, nullptr, nullptr));
        return v[which];
    }
    smh_update_plan *p_ = nullptr;
    smh_crs *m_ = nullptr;
    size_t n_ = 0;
};

template <typename T>
class SparseMatCRS {
  public:
    using Value = T;
    using Index = uint32_t;
    // The reference has no public raw-array constructor (from_sparsemat_index is pub(crate),
    // sparsemat_crs.rs:24-50): this is the documented addition.  Arrays are borrowed for the call.
    static SparseMatCRS from_raw_parts(size_t n_rows, size_t n_cols, const std::vector<uint32_t> &offset_rows,
                                       const std::vector<uint32_t> &columns, const std::vector<T> &values) {
        if (n_rows && offset_rows.size() != n_rows + 1) throw Panic(SMH_ERR_INVALID, "offset_rows must have n_rows+1 entries");
        if (columns.size() != values.size()) throw Panic(SMH_ERR_INVALID, "columns and values differ in length");
        SparseMatCRS m;
        detail::check(smh_crs_create(detail::dtype_of<T>::value, n_rows, n_cols, values.size(), offset_rows.data(),
                                     columns.data(), values.data(), 1, &m.h_));
        return m;
    }
    SparseMatCRS(SparseMatCRS &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    SparseMatCRS &operator=(SparseMatCRS &&o) noexcept { std::swap(h_, o.h_); return *this; }
    SparseMatCRS(const SparseMatCRS &) = delete;
    ~SparseMatCRS() { smh_crs_destroy(h_); }

    size_t n_rows() const { return smh_crs_n_rows(h_); }              // sparsemat_crs.rs:124-126
    size_t n_cols() const { return smh_crs_n_cols(h_); }              // :128-130
    size_t n_non_zero_entries() const { return smh_crs_nnz(h_); }     // :132-134
    bool empty() const { return n_rows() == 0; }                      // sparsematrix.rs:119-121
    double density() const {                                           // sparsematrix.rs:237-241
        return (double)n_non_zero_entries() / (double)(n_rows() * n_cols());
    }
    double sparsity() const { return 1.0 - density(); }                // sparsematrix.rs:244-246
    void scale(T a) { detail::check(smh_crs_scale(h_, (double)a)); }  // sparsemat_crs.rs:153-157

    // SparseMatrix::mvp (sparsematrix.rs:146-158): returns a NEW vector with dim == n_rows
    DenseVec<T> mvp(const DenseVec<T> &rhs, int variant = SMH_SPMV_AUTO) const {
        DenseVec<T> ret(n_rows());
        detail::check(smh_crs_spmv_vec(h_, rhs.handle(), ret.handle(), variant));
        return ret;
    }
    std::vector<T> mvp(const std::vector<T> &rhs, int variant = SMH_SPMV_AUTO) const {
        std::vector<T> y(n_rows());
        detail::check(smh_crs_spmv(h_, rhs.data(), rhs.size(), y.data(), variant));
        return y;
    }
    // mvp for every vector of rhs in one sweep over the matrix (smh_crs_spmv_many): column c is bit for bit mvp(rhs.column(c), SMH_SPMV_SEQ)
    MultiVec<T> mvp_many(const MultiVec<T> &rhs) const {
        MultiVec<T> ret(n_rows(), rhs.count());
        detail::check(smh_crs_spmv_many(h_, rhs.handle(), ret.handle()));
        return ret;
    }
    // SparseMatrix::inner_prod (sparsematrix.rs:161-171): lhs^T A rhs
    T inner_prod(const DenseVec<T> &lhs, const DenseVec<T> &rhs) const {
        double out = 0.0;
        detail::check(smh_crs_inner_prod_vec(h_, lhs.handle(), rhs.handle(), SMH_SPMV_AUTO, &out));
        return (T)out;
    }
    // `A * v` (sparsemat_ops! Mul<DenseVec>, sparsematrix.rs:435-443)
    friend DenseVec<T> operator*(const SparseMatCRS &a, const DenseVec<T> &v) { return a.mvp(v); }

    // Sortable::sort_row (sparsemat_crs.rs:163-172) for every row: ascending columns, stable
    void sort_rows() { detail::check(smh_crs_sort_rows(h_)); }
    // SparseMatrix::transpose (sparsematrix.rs:174-184): `ret.set(j, i, val)` over the entries in storage order, into a
    // fresh SparseMatCRS -- same arrays as the reference's container ends up with (rows reversed, first-push quirk)
    SparseMatCRS transpose() const {
        SparseMatCRS t;
        detail::check(smh_crs_transpose(h_, &t.h_));
        return t;
    }
    // SparseMatrix::prod (sparsematrix.rs:186-210): self * rhs as the reference's loops build it (same order of
    // additions, zero sums dropped, rows in descending column order); Err("Dimension mismatch") becomes a Panic
    SparseMatCRS prod(const SparseMatCRS &rhs) const {
        SparseMatCRS c;
        detail::check(smh_crs_prod(h_, rhs.h_, &c.h_));
        return c;
    }
    // Reordering (an extension: the reference has none; sparsemat_hip.h "reordering").  A permutation is n u32 with
    // perm[new] = old.  permute: out[i][j] = (*this)[row_perm[i]][col_perm[j]], rows keep their entries in storage order, values
    // bit for bit; an EMPTY vector is the identity.  permute_symmetric: P A P^T.
    SparseMatCRS permute(const std::vector<uint32_t> &row_perm, const std::vector<uint32_t> &col_perm) const {
        SparseMatCRS r;
        detail::check(smh_crs_permute(h_, row_perm.empty() ? nullptr : row_perm.data(), row_perm.size(), col_perm.empty() ? nullptr : col_perm.data(),
                                      col_perm.size(), &r.h_));
        return r;
    }
    SparseMatCRS permute_symmetric(const std::vector<uint32_t> &perm) const {
        static const uint32_t none = 0;
        SparseMatCRS r;
        detail::check(smh_crs_permute_symmetric(h_, perm.empty() ? &none : perm.data(), perm.size(), &r.h_));
        return r;
    }
    // the reverse Cuthill-McKee ordering of the symmetrised pattern (computed on the device; one round of kernels per level)
    struct RcmStats { size_t n_components = 0, n_levels = 0; };
    std::vector<uint32_t> rcm(RcmStats *stats = nullptr) const {
        std::vector<uint32_t> perm(n_rows() ? n_rows() : 1);
        RcmStats st;
        detail::check(smh_crs_rcm(h_, perm.data(), &st.n_components, &st.n_levels));
        perm.resize(n_rows());
        if (stats) *stats = st;
        return perm;
    }
    // a multicolour ordering of the symmetrised pattern (smh_crs_color; computed on the device): the rows sorted by (colour, index),
    // ready for permute_symmetric, after which a triangular solve has at most n_colors levels.  colors: by ORIGINAL row
    struct ColorStats {
        size_t n_colors = 0, n_rounds = 0;
        std::vector<uint32_t> colors;
    };
    std::vector<uint32_t> color(uint32_t seed = 0, ColorStats *stats = nullptr) const {
        std::vector<uint32_t> perm(n_rows() ? n_rows() : 1);
        ColorStats st;
        st.colors.resize(perm.size());
        detail::check(smh_crs_color(h_, seed, st.colors.data(), perm.data(), &st.n_colors, &st.n_rounds));
        perm.resize(n_rows());
        st.colors.resize(n_rows());
        if (stats) *stats = std::move(st);
        return perm;
    }
    // Sparse triangular solves and symmetric Gauss-Seidel (extensions: the reference has neither; sparsemat_hip.h).  The triangle
    // uplo (SMH_TRI_LOWER / SMH_TRI_UPPER) of this square matrix with the first stored (i, i) of a row as its diagonal entry, or an
    // implied 1 (unit_diagonal); level-scheduled on the device, every operation rounded once, a row's subtractions in storage order.
    struct TriLevels {
        size_t n_levels = 0, n_launches = 0, small_level_rows = 0;
        std::vector<uint32_t> level_of_row;
    };
    TriLevels trisolve_levels(int uplo = SMH_TRI_LOWER) const {
        TriLevels t;
        t.level_of_row.resize(n_rows() ? n_rows() : 1);
        detail::check(smh_crs_trisolve_levels(h_, uplo, &t.n_levels, t.level_of_row.data(), &t.n_launches, &t.small_level_rows));
        t.level_of_row.resize(n_rows());
        return t;
    }
    std::vector<T> trisolve(const std::vector<T> &b, int uplo = SMH_TRI_LOWER, bool unit_diagonal = false) const {
        std::vector<T> x(b.size());
        detail::check(smh_crs_trisolve(h_, uplo, unit_diagonal ? SMH_DIAG_UNIT : SMH_DIAG_NON_UNIT, b.data(), b.size(), x.data(), x.size()));
        return x;
    }
    // x may be b: in place
    void trisolve(const DenseVec<T> &b, DenseVec<T> &x, int uplo = SMH_TRI_LOWER, bool unit_diagonal = false) const {
        detail::check(smh_crs_trisolve_vec(h_, uplo, unit_diagonal ? SMH_DIAG_UNIT : SMH_DIAG_NON_UNIT, b.handle(), x.handle()));
    }
    // z = M^-1 r, M = (D + L) D^-1 (D + U); z may be r
    void sgs_apply(const DenseVec<T> &r, DenseVec<T> &z) const { detail::check(smh_crs_sgs_apply_vec(h_, r.handle(), z.handle())); }
    // ILU(0), the incomplete LU factorization without fill (an extension; smh_crs_ilu0): a new matrix on this one's pattern holding
    // the unit-lower L below the diagonal and U on and above it, factored on the device level by level.  Rows strictly ascending
    // (sort_rows), every diagonal stored.  zero_pivot (optional): the first row whose U(i, i) == 0, no_zero_pivot without one -- not
    // an error, the values are IEEE's.
    static constexpr size_t no_zero_pivot = (size_t)-1;
    SparseMatCRS ilu0(size_t *zero_pivot = nullptr) const {
        SparseMatCRS f;
        detail::check(smh_crs_ilu0(h_, &f.h_, zero_pivot));
        return f;
    }
    // this factor again from the values of a, which has the pattern the factor was made on: the bits of a.ilu0(); returns zero_pivot
    size_t ilu0_refactor(const SparseMatCRS &a) {
        size_t zero_pivot = no_zero_pivot;
        detail::check(smh_crs_ilu0_refactor(h_, a.h_, &zero_pivot));
        return zero_pivot;
    }
    // z = U^-1 L^-1 r with this matrix an ilu0 factor; z may be r
    void ilu_apply(const DenseVec<T> &r, DenseVec<T> &z) const { detail::check(smh_crs_ilu_apply_vec(h_, r.handle(), z.handle())); }
    // FSAI, the factorized sparse approximate inverse (an extension; smh_crs_fsai): {g, gt}, g lower triangular on the stored (i, c)
    // of this matrix with c <= i, G^T G ~ A^-1 and diag(G A G^T) = 1 for an SPD matrix, gt its transpose -- two ordinary matrices,
    // built in one data-parallel sweep on the device.  Rows strictly ascending (sort_rows), every diagonal stored, at most 128
    // entries of a row on or below it; only those are read.  not_spd (optional): the first row whose last pivot is not > 0,
    // no_zero_pivot without one -- not an error, the values are IEEE's.
    std::pair<SparseMatCRS, SparseMatCRS> fsai(size_t *not_spd = nullptr) const {
        SparseMatCRS g, gt;
        detail::check(smh_crs_fsai(h_, &g.h_, &gt.h_, not_spd));
        return {std::move(g), std::move(gt)};
    }
    // z = G^T (G r) with this matrix the g and gt the transpose of fsai(): two products; z may be r
    void fsai_apply(const SparseMatCRS &gt, const DenseVec<T> &r, DenseVec<T> &z) const {
        detail::check(smh_crs_fsai_apply_vec(h_, gt.h_, r.handle(), z.handle()));
    }
    // The non-symmetric FSAI (an extension; smh_crs_fsai_ns): {gl, gu} with G_U G_L ~ A^-1, gl lower triangular with a unit diagonal
    // on the stored (i, c) with c <= i, gu upper triangular on the stored (i, c) with c >= i -- two ordinary matrices; on a dense
    // pattern G_U G_L = A^-1.  Rows strictly ascending (sort_rows), every diagonal stored, at most 128 entries of a row on or below
    // and of a column on or above it.  singular (optional): the first row whose last pivot, in either factor's row solve, is zero or
    // not finite, no_zero_pivot without one -- not an error, the values are IEEE's.
    std::pair<SparseMatCRS, SparseMatCRS> fsai_ns(size_t *singular = nullptr) const {
        SparseMatCRS gl, gu;
        detail::check(smh_crs_fsai_ns(h_, &gl.h_, &gu.h_, singular));
        return {std::move(gl), std::move(gu)};
    }
    // z = G_U (G_L r) with this matrix the gl and gu the other factor of fsai_ns(): two products; z may be r
    void fsai_ns_apply(const SparseMatCRS &gu, const DenseVec<T> &r, DenseVec<T> &z) const {
        detail::check(smh_crs_fsai_ns_apply_vec(h_, gu.h_, r.handle(), z.handle()));
    }
    // {max i - j, max j - i} over the stored entries
    std::pair<uint32_t, uint32_t> bandwidth() const {
        uint32_t lo = 0, hi = 0;
        detail::check(smh_crs_bandwidth(h_, &lo, &hi));
        return {lo, hi};
    }
    // #[derive(Clone)] (sparsemat_crs.rs:8): an independent library-owned copy (the copy constructor stays deleted: copies
    // of device matrices are explicit)
    SparseMatCRS clone() const {
        SparseMatCRS c;
        detail::check(smh_crs_clone(h_, &c.h_));
        return c;
    }
    // an extension (smh_crs_cast): a new matrix of U with this one's dims, pattern, orphan and kernel settings, the values converted
    // on the device -- f64 -> f32 to nearest even, f32 -> f64 exactly; U == T is clone().  overflow (optional): the finite values
    // that became infinite
    template <typename U> SparseMatCRS<U> cast(size_t *overflow = nullptr) const {
        SparseMatCRS<U> c;
        detail::check(smh_crs_cast(h_, detail::dtype_of<U>::value, &c.h_, overflow));
        return c;
    }
    // SparseMatrix::add / sub (sparsematrix.rs:123-143), in place: `*get_mut(i, j) += val` (-=) for every entry of rhs in
    // storage order -- new columns pushed to the start of their row, folds into the first occurrence, bit for bit.  rhs may
    // be *this.  The operators of sparsemat_ops! (:370-433): +=, -=, *= T, and +, -, * T on a clone.
    void add(const SparseMatCRS &rhs) { detail::check(smh_crs_add_assign(h_, rhs.h_)); }
    void sub(const SparseMatCRS &rhs) { detail::check(smh_crs_sub_assign(h_, rhs.h_)); }
    SparseMatCRS &operator+=(const SparseMatCRS &rhs) { add(rhs); return *this; }
    SparseMatCRS &operator-=(const SparseMatCRS &rhs) { sub(rhs); return *this; }
    SparseMatCRS &operator*=(T a) { scale(a); return *this; }
    friend SparseMatCRS operator+(const SparseMatCRS &a, const SparseMatCRS &b) {
        SparseMatCRS c;
        detail::check(smh_crs_add(a.h_, b.h_, &c.h_));
        return c;
    }
    friend SparseMatCRS operator-(const SparseMatCRS &a, const SparseMatCRS &b) {
        SparseMatCRS c;
        detail::check(smh_crs_sub(a.h_, b.h_, &c.h_));
        return c;
    }
    friend SparseMatCRS operator*(const SparseMatCRS &a, T s) {
        SparseMatCRS c = a.clone();
        c.scale(s);
        return c;
    }
    size_t orphans() const { return smh_crs_orphans(h_); }  // see smh_crs_orphans
    // SparseMatrix::get (sparsemat_crs.rs:136-142 via find_index :54-67): the first match in the row, zero when absent
    // (smh_crs_get: one query on the device; get_many for batches).
    T get(size_t i, size_t j) const {
        T out = T(0);
        detail::check(smh_crs_get(h_, i, j, &out));
        return out;
    }
    std::vector<T> get_many(const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols) const {
        if (rows.size() != cols.size()) throw Panic(SMH_ERR_INVALID, "rows and cols differ in length");
        std::vector<T> out(rows.size(), T(0));
        detail::check(smh_crs_get_many(h_, rows.size(), rows.data(), cols.data(), out.data()));
        return out;
    }
    // SparseMatrix::set / add_to (sparsematrix.rs:226-233) on this container: one device call each -- correct, but batch a
    // stream into apply() (smh_crs_apply: ops[k] != 0 is set, an empty ops vector means all add_to)
    void set(size_t i, size_t j, T val) { apply({index(i)}, {index(j)}, {val}, {1}); }
    void add_to(size_t i, size_t j, T val) { apply({index(i)}, {index(j)}, {val}, {}); }
    void apply(const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols, const std::vector<T> &vals,
               const std::vector<uint8_t> &ops = {}) {
        if (rows.size() != vals.size() || cols.size() != vals.size() || (!ops.empty() && ops.size() != vals.size()))
            throw Panic(SMH_ERR_INVALID, "rows, cols, values and ops differ in length");
        detail::check(smh_crs_apply(h_, vals.size(), rows.data(), cols.data(), vals.data(), ops.empty() ? nullptr : ops.data()));
    }
    // a reusable plan for re-assembling this matrix from the stream (rows, cols, ops) with new values: every operation must
    // land on an existing entry (apply the stream once to create them, then plan); stale once the structure changes
    UpdatePlan<T> update_plan(const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols, const std::vector<uint8_t> &ops = {}) {
        if (rows.size() != cols.size() || (!ops.empty() && ops.size() != rows.size()))
            throw Panic(SMH_ERR_INVALID, "rows, cols and ops differ in length");
        UpdatePlan<T> p;
        detail::check(smh_update_plan_create(h_, rows.size(), rows.data(), cols.data(), ops.empty() ? nullptr : ops.data(), &p.p_));
        p.m_ = h_;
        p.n_ = rows.size();
        return p;
    }
    // SparseMatCRS::new() (sparsemat_crs.rs:47-49) and SparseMatrix::eye (sparsematrix.rs:91-98)
    static SparseMatCRS new_empty() {
        SparseMatCRS m;
        detail::check(smh_crs_replay(detail::dtype_of<T>::value, 0, nullptr, nullptr, nullptr, nullptr, &m.h_));
        return m;
    }
    static SparseMatCRS eye(size_t dim) {
        SparseMatCRS m;
        detail::check(smh_crs_eye(detail::dtype_of<T>::value, dim, &m.h_));
        return m;
    }
    bool is_symmetric() const {  // sparsematrix.rs:212-222
        int out = 0;
        detail::check(smh_crs_is_symmetric(h_, &out));
        return out != 0;
    }
    bool is_sorted() const {  // sparsematrix.rs:263-271
        int out = 0;
        detail::check(smh_crs_is_sorted(h_, &out));
        return out != 0;
    }
    // ColumnIter::assemble_column_info (sparsemat_crs.rs:180-191) as arrays: rows[k] = row of entry k; iter_col(j)
    // (:193-204) walks entries[col_ptr[j] .. col_ptr[j+1]) and yields (rows[e], values[e])
    void column_info(std::vector<uint32_t> &rows, std::vector<uint32_t> &col_ptr, std::vector<uint32_t> &entries) const {
        rows.assign(n_non_zero_entries() ? n_non_zero_entries() : 1, 0u);
        entries.assign(rows.size(), 0u);
        col_ptr.assign(n_cols() + 1, 0u);
        detail::check(smh_crs_column_info(h_, rows.data(), col_ptr.data(), entries.data()));
        rows.resize(n_non_zero_entries());
        entries.resize(n_non_zero_entries());
    }
    // the CRS arrays as stored (offset_rows, columns, values)
    void raw_parts(std::vector<uint32_t> &offset_rows, std::vector<uint32_t> &columns, std::vector<T> &values) const {
        offset_rows.assign(n_rows() + 1, 0u);
        columns.assign(n_non_zero_entries(), 0u);
        values.assign(n_non_zero_entries(), T(0));
        detail::check(smh_crs_download(h_, offset_rows.data(), columns.data(), values.data()));
    }

    smh_crs *handle() const { return h_; }

  private:
    template <typename U> friend class SparseMatIndexList;
    template <typename U> friend class SparseMatCRS;  // (cast<U>() fills the other type's handle)
    SparseMatCRS() = default;
    // a row or column index of Index = u32: larger ones are refused, never truncated
    static uint32_t index(size_t i) {
        if (i > 0xFFFFFFFFull) throw Panic(SMH_ERR_INVALID, "index does not fit the u32 index type");
        return (uint32_t)i;
    }
    smh_crs *h_ = nullptr;
};

// Assembly with the call surface of the reference's SparseMatIndexList (sparsemat_indexlist.rs): `add_to` /
// `set` (sparsematrix.rs:231-233 / :226-228) are RECORDED (O(1) each, no list walk) and `to_crs()` (:61-63 ->
// sparsemat_crs.rs:24-50) builds the identical CRS on the device with smh_crs_assemble: rows in order of first
// appearance, duplicates folded in call order, bit for bit.
template <typename T>
class SparseMatIndexList {
  public:
    void add_to(size_t i, size_t j, T val) { record(i, j, val, 0); }
    void set(size_t i, size_t j, T val) { record(i, j, val, 1); }
    // SparseMatrix::get (sparsemat_indexlist.rs:148-155): value of (i, j), zero when absent.  Folds the
    // recorded calls (O(calls)): meant for spot checks, as in the reference's tests.
    T get(size_t i, size_t j) const {
        T acc = T(0);
        for (size_t k = 0; k < vals_.size(); ++k)
            if (rows_[k] == i && cols_[k] == j) acc = ops_[k] ? vals_[k] : T(acc + vals_[k]);
        return acc;
    }
    size_t n_rows() const { return n_rows_; }  // indexlist.rs:58-60
    size_t n_cols() const { return n_cols_; }  // sparsemat_indexlist.rs:46-48
    SparseMatCRS<T> to_crs() const {
        SparseMatCRS<T> m;
        detail::check(smh_crs_assemble(detail::dtype_of<T>::value, vals_.size(), rows_.data(), cols_.data(), vals_.data(),
                                       ops_.data(), &m.h_));
        return m;
    }
    // The same calls made on a SparseMatCRS directly (get_mut sparsemat_crs.rs:143-149 -> push :71-92 inserts at the
    // START of the row, first-push quirk included): the matrix src/lib.rs:114-154 builds.  smh_crs_replay.
    SparseMatCRS<T> as_direct_crs() const {
        SparseMatCRS<T> m;
        detail::check(smh_crs_replay(detail::dtype_of<T>::value, vals_.size(), rows_.data(), cols_.data(), vals_.data(),
                                     ops_.data(), &m.h_));
        return m;
    }

  private:
    void record(size_t i, size_t j, T val, uint8_t op) {
        if (i >= 0xFFFFFFFFull || j >= 0xFFFFFFFFull) throw Panic(SMH_ERR_CAPACITY, "index exceeds u32");
        rows_.push_back((uint32_t)i); cols_.push_back((uint32_t)j); vals_.push_back(val); ops_.push_back(op);
        if (i + 1 > n_rows_) n_rows_ = i + 1;
        if (j + 1 > n_cols_) n_cols_ = j + 1;
    }
    std::vector<uint32_t> rows_, cols_;
    std::vector<T> vals_;
    std::vector<uint8_t> ops_;
    size_t n_rows_ = 0, n_cols_ = 0;
};

// SparseMatPar<SparseMatCRS<T,u32>> (sparsemat_par.rs:12-35, 86-140) driven by one process: block b = rows
// [b R, (b+1) R), R = n_rows / n_blocks (the last block takes the remainder), on device devices[b] (empty: block b on
// device b mod device count).  Filled from a global CRS; host vectors in, host vectors out.
template <typename T>
class SparseMatPar {
  public:
    static SparseMatPar with_sub_matrices(size_t n_blocks, size_t n_rows, size_t n_cols, const std::vector<uint32_t> &offset_rows,
                                          const std::vector<uint32_t> &columns, const std::vector<T> &values,
                                          const std::vector<int> &devices = {}) {
        if (offset_rows.size() != n_rows + 1) throw Panic(SMH_ERR_INVALID, "offset_rows must have n_rows+1 entries");
        if (columns.size() != values.size()) throw Panic(SMH_ERR_INVALID, "columns and values differ in length");
        if (!devices.empty() && devices.size() != n_blocks) throw Panic(SMH_ERR_INVALID, "one device per block");
        SparseMatPar m;
        detail::check(smh_par_create(detail::dtype_of<T>::value, n_blocks, devices.empty() ? nullptr : devices.data(), n_rows, n_cols,
                                     offset_rows.data(), columns.data(), values.data(), 1, &m.h_));
        return m;
    }
    SparseMatPar(SparseMatPar &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    SparseMatPar &operator=(SparseMatPar &&o) noexcept { std::swap(h_, o.h_); return *this; }
    SparseMatPar(const SparseMatPar &) = delete;
    ~SparseMatPar() { smh_par_destroy(h_); }

    size_t n_rows() const { return smh_par_n_rows(h_); }
    size_t n_cols() const { return smh_par_n_cols(h_); }                       // sparsemat_par.rs:109-115
    size_t n_non_zero_entries() const { return smh_par_nnz(h_); }              // :117-123
    size_t n_blocks() const { return smh_par_n_blocks(h_); }
    void scale(T a) { detail::check(smh_par_scale(h_, (double)a)); }           // :135-139
    std::pair<size_t, size_t> get_block_and_row_id(size_t row) const {         // :31-35, clamped to the last block
        size_t b = 0, r = 0;
        detail::check(smh_par_get_block_and_row_id(h_, row, &b, &r));
        return {b, r};
    }
    std::vector<T> mvp(const std::vector<T> &rhs, int variant = SMH_SPMV_AUTO) const {
        std::vector<T> y(n_rows());
        detail::check(smh_par_spmv(h_, rhs.data(), rhs.size(), y.data(), variant));
        return y;
    }
    smh_par *handle() const { return h_; }

    // A DenseVec distributed over the blocks: one full-length device buffer per block, block b owns [b R, (b+1) R).
    class ParVec {
      public:
        ParVec(const SparseMatPar &m, size_t n) { detail::check(smh_par_vec_create(m.h_, n, &v_)); }
        ParVec(const SparseMatPar &m, const std::vector<T> &host) : ParVec(m, host.size()) {
            detail::check(smh_par_vec_upload(v_, host.data()));
        }
        ParVec(ParVec &&o) noexcept : v_(o.v_) { o.v_ = nullptr; }
        ParVec(const ParVec &) = delete;
        ~ParVec() { smh_par_vec_destroy(v_); }
        size_t dim() const { return smh_par_vec_dim(v_); }
        std::vector<T> to_vec() const {  // the owned slices of all blocks = the whole vector
            std::vector<T> out(dim());
            detail::check(smh_par_vec_download(v_, out.data()));
            return out;
        }
        smh_par_vec *handle() const { return v_; }

      private:
        smh_par_vec *v_ = nullptr;
    };
    // The reference's intended mvp_par (sparsemat_par.rs:37-68), device resident: every block multiplies against the
    // shared x, its results go to offset b * R of y, then ONE exchange inside the library (RCCL all-gather, or only the
    // entries each block references) makes y usable as the next x.  Asynchronous: synchronize() waits.
    void mvp_par(const ParVec &x, ParVec &y, int variant = SMH_SPMV_AUTO, int exchange = SMH_EXCHANGE_AUTO) const {
        detail::check(smh_par_spmv_dev(h_, x.handle(), y.handle(), variant, exchange));
    }
    void synchronize() const { detail::check(smh_par_synchronize(h_)); }

  private:
    SparseMatPar() = default;
    smh_par *h_ = nullptr;
};

// linearsolver.rs:12-61.  The reference keeps tol / iter_max private with only Default (1e-12, 10000);
// the two-argument constructor is the documented addition.
class ConjugateGradient {
  public:
    ConjugateGradient() = default;
    ConjugateGradient(double tol, size_t iter_max) : tol_(tol), iter_max_(iter_max) {}
    // LinearSolver::solve(&self, mat, b, x): x is updated in place; panics become sparsemat::Panic with
    // the reference's text ("Matrix is not symmetric", "Matrix and vector size mismatch").
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const DenseVec<T> &b, DenseVec<T> &x) {
        detail::check(smh_cg_solve_vec(mat.handle(), b.handle(), x.handle(), tol_, iter_max_, SMH_SPMV_AUTO, 0,
                                       &iterations_, &r_norm_squared_));
    }
    // Jacobi-preconditioned variant -- an extension, not in the reference: z = r / diag(A); host vectors
    template <typename T>
    void solve_jacobi(const SparseMatCRS<T> &mat, const std::vector<T> &b, std::vector<T> &x) {
        detail::check(smh_pcg_jacobi_solve(mat.handle(), b.data(), b.size(), x.data(), x.size(), tol_, iter_max_, SMH_SPMV_AUTO,
                                           &iterations_, &r_norm_squared_));
    }
    // the same solve on a row-partitioned matrix (M = SparseMatPar): host vectors, x updated in place
    template <typename T>
    void solve(const SparseMatPar<T> &mat, const std::vector<T> &b, std::vector<T> &x) {
        detail::check(smh_par_cg_solve(mat.handle(), b.data(), b.size(), x.data(), x.size(), tol_, iter_max_, SMH_SPMV_AUTO,
                                       &iterations_, &r_norm_squared_));
    }
    // solve on the k columns of b and x at once (smh_cg_solve_many): column c is solve(mat, b_c, x_c) with its own alpha, beta,
    // stop test and iteration count; all columns share one sweep over the matrix per body.  Same panics as solve.
    template <typename T>
    void solve_many(const SparseMatCRS<T> &mat, const MultiVec<T> &b, MultiVec<T> &x) {
        std::vector<size_t> iters(b.count());
        std::vector<double> rr(b.count());
        detail::check(smh_cg_solve_many(mat.handle(), b.handle(), x.handle(), tol_, iter_max_, 0, iters.data(), rr.data()));
        iterations_many_ = std::move(iters);
        r_norm_squared_many_ = std::move(rr);
    }
    size_t iterations() const { return iterations_; }
    double r_norm_squared() const { return r_norm_squared_; }
    // ... of the last solve_many, per column
    const std::vector<size_t> &iterations_many() const { return iterations_many_; }
    const std::vector<double> &r_norm_squared_many() const { return r_norm_squared_many_; }

  private:
    double tol_ = 1e-12;
    size_t iter_max_ = 10000;
    size_t iterations_ = 0;
    double r_norm_squared_ = 0.0;
    std::vector<size_t> iterations_many_;
    std::vector<double> r_norm_squared_many_;
};

// CG preconditioned by symmetric Gauss-Seidel -- an extension, not in the reference (smh_pcg_sgs_solve*): the recurrence of
// ConjugateGradient::solve_jacobi with z = M^-1 r by two level-scheduled triangular solves; same panics and stop rule.
class SGSConjugateGradient {
  public:
    SGSConjugateGradient() = default;
    SGSConjugateGradient(double tol, size_t iter_max) : tol_(tol), iter_max_(iter_max) {}
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const DenseVec<T> &b, DenseVec<T> &x) {
        detail::check(smh_pcg_sgs_solve_vec(mat.handle(), b.handle(), x.handle(), tol_, iter_max_, SMH_SPMV_AUTO, 0, &iterations_,
                                            &r_norm_squared_));
    }
    // host vectors, x updated in place
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const std::vector<T> &b, std::vector<T> &x) {
        detail::check(smh_pcg_sgs_solve(mat.handle(), b.data(), b.size(), x.data(), x.size(), tol_, iter_max_, SMH_SPMV_AUTO, &iterations_,
                                        &r_norm_squared_));
    }
    size_t iterations() const { return iterations_; }
    double r_norm_squared() const { return r_norm_squared_; }

  private:
    double tol_ = 1e-12;
    size_t iter_max_ = 10000;
    size_t iterations_ = 0;
    double r_norm_squared_ = 0.0;
};

// CG preconditioned by ILU(0) -- an extension, not in the reference (smh_pcg_ilu_solve*): SGSConjugateGradient's recurrence with
// z = U^-1 L^-1 r by the two solves on `factor` (mat.ilu0()); the product is mat's.  Same panics and stop rule.
class ILUConjugateGradient {
  public:
    ILUConjugateGradient() = default;
    ILUConjugateGradient(double tol, size_t iter_max) : tol_(tol), iter_max_(iter_max) {}
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const SparseMatCRS<T> &factor, const DenseVec<T> &b, DenseVec<T> &x) {
        detail::check(smh_pcg_ilu_solve_vec(mat.handle(), factor.handle(), b.handle(), x.handle(), tol_, iter_max_, SMH_SPMV_AUTO, 0, &iterations_,
                                            &r_norm_squared_));
    }
    // host vectors, x updated in place
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const SparseMatCRS<T> &factor, const std::vector<T> &b, std::vector<T> &x) {
        detail::check(smh_pcg_ilu_solve(mat.handle(), factor.handle(), b.data(), b.size(), x.data(), x.size(), tol_, iter_max_, SMH_SPMV_AUTO,
                                        &iterations_, &r_norm_squared_));
    }
    // ... factoring mat first
    template <typename T, typename V>
    void solve(const SparseMatCRS<T> &mat, const V &b, V &x) {
        const SparseMatCRS<T> factor = mat.ilu0();
        solve(mat, factor, b, x);
    }
    size_t iterations() const { return iterations_; }
    double r_norm_squared() const { return r_norm_squared_; }

  private:
    double tol_ = 1e-12;
    size_t iter_max_ = 10000;
    size_t iterations_ = 0;
    double r_norm_squared_ = 0.0;
};

// CG preconditioned by the factorized sparse approximate inverse -- an extension, not in the reference (smh_pcg_fsai_solve*):
// SGSConjugateGradient's recurrence with z = G^T (G r) by two products on the pair mat.fsai() gives; the body's product is mat's.
// Same panics and stop rule.  The forms without a pair factor mat first and panic (SMH_ERR_INVALID) when it is not positive definite.
class FSAIConjugateGradient {
  public:
    FSAIConjugateGradient() = default;
    FSAIConjugateGradient(double tol, size_t iter_max) : tol_(tol), iter_max_(iter_max) {}
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const SparseMatCRS<T> &g, const SparseMatCRS<T> &gt, const DenseVec<T> &b, DenseVec<T> &x) {
        detail::check(smh_pcg_fsai_solve_vec(mat.handle(), g.handle(), gt.handle(), b.handle(), x.handle(), tol_, iter_max_, SMH_SPMV_AUTO, 0,
                                             &iterations_, &r_norm_squared_));
    }
    // host vectors, x updated in place
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const SparseMatCRS<T> &g, const SparseMatCRS<T> &gt, const std::vector<T> &b, std::vector<T> &x) {
        detail::check(smh_pcg_fsai_solve(mat.handle(), g.handle(), gt.handle(), b.data(), b.size(), x.data(), x.size(), tol_, iter_max_,
                                         SMH_SPMV_AUTO, &iterations_, &r_norm_squared_));
    }
    // ... factoring mat first
    template <typename T, typename V>
    void solve(const SparseMatCRS<T> &mat, const V &b, V &x) {
        size_t not_spd = SparseMatCRS<T>::no_zero_pivot;
        const auto f = mat.fsai(&not_spd);
        if (not_spd != SparseMatCRS<T>::no_zero_pivot)
            throw Panic(SMH_ERR_INVALID, "FSAI: the matrix is not positive definite (row " + std::to_string(not_spd) + ")");
        solve(mat, f.first, f.second, b, x);
    }
    size_t iterations() const { return iterations_; }
    double r_norm_squared() const { return r_norm_squared_; }

  private:
    double tol_ = 1e-12;
    size_t iter_max_ = 10000;
    size_t iterations_ = 0;
    double r_norm_squared_ = 0.0;
};

// BiCGSTAB for non-symmetric systems -- an extension, not in the reference (smh_bicgstab_solve*): device-resident like
// ConjugateGradient, same panics and stop rule.  breakdown(): 0 none, 1 rho' == 0 or omega == 0, 2 r^.v == 0, 3 t.t == 0
// (sparsemat_hip.h); a breakdown ends the solve without a panic.
// precond (smh_bicgstab_precond_solve*): SMH_PRECOND_NONE (the default: the calls above), _JACOBI, _SGS or _ILU -- right
// preconditioning, A M^-1 u = b, x = M^-1 u, as GMRES below.  SMH_PRECOND_ILU takes the factor (mat.ilu0()) or, in the overloads
// without one, factors mat first.
class BiCGStab {
  public:
    BiCGStab() = default;
    BiCGStab(double tol, size_t iter_max, int precond = SMH_PRECOND_NONE) : tol_(tol), iter_max_(iter_max), precond_(precond) {}
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const DenseVec<T> &b, DenseVec<T> &x) {
        if (precond_ == SMH_PRECOND_ILU) return solve(mat, mat.ilu0(), b, x);
        if (precond_ != SMH_PRECOND_NONE) return solve_precond(mat, nullptr, b, x);
        detail::check(smh_bicgstab_solve_vec(mat.handle(), b.handle(), x.handle(), tol_, iter_max_, SMH_SPMV_AUTO, 0, &iterations_,
                                             &r_norm_squared_, &breakdown_));
    }
    // host vectors, x updated in place
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const std::vector<T> &b, std::vector<T> &x) {
        if (precond_ == SMH_PRECOND_ILU) return solve(mat, mat.ilu0(), b, x);
        if (precond_ != SMH_PRECOND_NONE) return solve_precond(mat, nullptr, b, x);
        detail::check(smh_bicgstab_solve(mat.handle(), b.data(), b.size(), x.data(), x.size(), tol_, iter_max_, SMH_SPMV_AUTO,
                                         &iterations_, &r_norm_squared_, &breakdown_));
    }
    // ... with the ILU(0) factor of mat (a factor with another kind is the library's SMH_ERR_INVALID)
    template <typename T, typename V>
    void solve(const SparseMatCRS<T> &mat, const SparseMatCRS<T> &factor, const V &b, V &x) {
        solve_precond(mat, factor.handle(), b, x);
    }
    // ... right-preconditioned by a pair of product handles, M^-1 v = gt (g v) (smh_bicgstab_fsai_solve*): mat.fsai_ns()'s {gl, gu},
    // or mat.fsai()'s {g, gt} for a symmetric matrix; the kind given to the constructor is not looked at
    template <typename T>
    void solve_fsai(const SparseMatCRS<T> &mat, const SparseMatCRS<T> &g, const SparseMatCRS<T> &gt, const DenseVec<T> &b, DenseVec<T> &x) {
        detail::check(smh_bicgstab_fsai_solve_vec(mat.handle(), g.handle(), gt.handle(), b.handle(), x.handle(), tol_, iter_max_, SMH_SPMV_AUTO, 0,
                                                  &iterations_, &r_norm_squared_, &breakdown_));
    }
    template <typename T>
    void solve_fsai(const SparseMatCRS<T> &mat, const SparseMatCRS<T> &g, const SparseMatCRS<T> &gt, const std::vector<T> &b, std::vector<T> &x) {
        detail::check(smh_bicgstab_fsai_solve(mat.handle(), g.handle(), gt.handle(), b.data(), b.size(), x.data(), x.size(), tol_, iter_max_,
                                              SMH_SPMV_AUTO, &iterations_, &r_norm_squared_, &breakdown_));
    }
    // ... factoring mat through fsai_ns() first
    template <typename T, typename V>
    void solve_fsai(const SparseMatCRS<T> &mat, const V &b, V &x) {
        const auto f = mat.fsai_ns();
        solve_fsai(mat, f.first, f.second, b, x);
    }
    size_t iterations() const { return iterations_; }
    double r_norm_squared() const { return r_norm_squared_; }
    int breakdown() const { return breakdown_; }

  private:
    template <typename T>
    void solve_precond(const SparseMatCRS<T> &mat, smh_crs *factor, const DenseVec<T> &b, DenseVec<T> &x) {
        detail::check(smh_bicgstab_precond_solve_vec(mat.handle(), precond_, factor, b.handle(), x.handle(), tol_, iter_max_,
                                                     SMH_SPMV_AUTO, 0, &iterations_, &r_norm_squared_, &breakdown_));
    }
    template <typename T>
    void solve_precond(const SparseMatCRS<T> &mat, smh_crs *factor, const std::vector<T> &b, std::vector<T> &x) {
        detail::check(smh_bicgstab_precond_solve(mat.handle(), precond_, factor, b.data(), b.size(), x.data(), x.size(), tol_, iter_max_,
                                                 SMH_SPMV_AUTO, &iterations_, &r_norm_squared_, &breakdown_));
    }
    double tol_ = 1e-12;
    size_t iter_max_ = 10000;
    int precond_ = SMH_PRECOND_NONE;
    size_t iterations_ = 0;
    double r_norm_squared_ = 0.0;
    int breakdown_ = 0;
};

// Restarted GMRES(m) for non-symmetric systems -- an extension, not in the reference (smh_gmres_solve*): the robust companion of
// BiCGStab (no breakdown before the Krylov space is exhausted, no stagnation near the imaginary axis), device-resident like it, same
// panics.  restart: 1 .. 128 (0: the library's default, 30).  breakdown(): 0 none, 1 the Krylov space is exhausted (x is updated from
// it), 2 the residual at a cycle's start is exactly zero (sparsemat_hip.h); cycles(): how many times a v_0 was formed.
// precond (smh_gmres_precond_solve*): SMH_PRECOND_NONE (the default: the calls above), _JACOBI, _SGS or _ILU -- right preconditioning,
// A M^-1 u = b, x = M^-1 u; r_norm_squared() is then the recurrence residual's.  SMH_PRECOND_ILU takes the factor (mat.ilu0()) or,
// in the overloads without one, factors mat first.
class GMRES {
  public:
    GMRES() = default;
    GMRES(double tol, size_t iter_max, size_t restart = 30, int precond = SMH_PRECOND_NONE)
        : tol_(tol), iter_max_(iter_max), restart_(restart), precond_(precond) {}
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const DenseVec<T> &b, DenseVec<T> &x) {
        if (precond_ == SMH_PRECOND_ILU) return solve(mat, mat.ilu0(), b, x);
        if (precond_ != SMH_PRECOND_NONE) return solve_precond(mat, nullptr, b, x);
        detail::check(smh_gmres_solve_vec(mat.handle(), b.handle(), x.handle(), tol_, iter_max_, restart_, SMH_SPMV_AUTO, 0, &iterations_,
                                          &r_norm_squared_, &cycles_, &breakdown_));
    }
    // host vectors, x updated in place
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const std::vector<T> &b, std::vector<T> &x) {
        if (precond_ == SMH_PRECOND_ILU) return solve(mat, mat.ilu0(), b, x);
        if (precond_ != SMH_PRECOND_NONE) return solve_precond(mat, nullptr, b, x);
        detail::check(smh_gmres_solve(mat.handle(), b.data(), b.size(), x.data(), x.size(), tol_, iter_max_, restart_, SMH_SPMV_AUTO,
                                      &iterations_, &r_norm_squared_, &cycles_, &breakdown_));
    }
    // ... with the ILU(0) factor of mat (a factor with another kind is the library's SMH_ERR_INVALID)
    template <typename T, typename V>
    void solve(const SparseMatCRS<T> &mat, const SparseMatCRS<T> &factor, const V &b, V &x) {
        solve_precond(mat, factor.handle(), b, x);
    }
    // ... right-preconditioned by a pair of product handles, M^-1 v = gt (g v) (smh_gmres_fsai_solve*): mat.fsai_ns()'s {gl, gu}, or
    // mat.fsai()'s {g, gt} for a symmetric matrix; the kind given to the constructor is not looked at
    template <typename T>
    void solve_fsai(const SparseMatCRS<T> &mat, const SparseMatCRS<T> &g, const SparseMatCRS<T> &gt, const DenseVec<T> &b, DenseVec<T> &x) {
        detail::check(smh_gmres_fsai_solve_vec(mat.handle(), g.handle(), gt.handle(), b.handle(), x.handle(), tol_, iter_max_, restart_, SMH_SPMV_AUTO,
                                               0, &iterations_, &r_norm_squared_, &cycles_, &breakdown_));
    }
    template <typename T>
    void solve_fsai(const SparseMatCRS<T> &mat, const SparseMatCRS<T> &g, const SparseMatCRS<T> &gt, const std::vector<T> &b, std::vector<T> &x) {
        detail::check(smh_gmres_fsai_solve(mat.handle(), g.handle(), gt.handle(), b.data(), b.size(), x.data(), x.size(), tol_, iter_max_, restart_,
                                           SMH_SPMV_AUTO, &iterations_, &r_norm_squared_, &cycles_, &breakdown_));
    }
    // ... factoring mat through fsai_ns() first
    template <typename T, typename V>
    void solve_fsai(const SparseMatCRS<T> &mat, const V &b, V &x) {
        const auto f = mat.fsai_ns();
        solve_fsai(mat, f.first, f.second, b, x);
    }
    size_t iterations() const { return iterations_; }
    double r_norm_squared() const { return r_norm_squared_; }
    size_t cycles() const { return cycles_; }
    int breakdown() const { return breakdown_; }

  private:
    template <typename T>
    void solve_precond(const SparseMatCRS<T> &mat, smh_crs *factor, const DenseVec<T> &b, DenseVec<T> &x) {
        detail::check(smh_gmres_precond_solve_vec(mat.handle(), precond_, factor, b.handle(), x.handle(), tol_, iter_max_, restart_,
                                                  SMH_SPMV_AUTO, 0, &iterations_, &r_norm_squared_, &cycles_, &breakdown_));
    }
    template <typename T>
    void solve_precond(const SparseMatCRS<T> &mat, smh_crs *factor, const std::vector<T> &b, std::vector<T> &x) {
        detail::check(smh_gmres_precond_solve(mat.handle(), precond_, factor, b.data(), b.size(), x.data(), x.size(), tol_, iter_max_,
                                              restart_, SMH_SPMV_AUTO, &iterations_, &r_norm_squared_, &cycles_, &breakdown_));
    }
    double tol_ = 1e-12;
    size_t iter_max_ = 10000;
    size_t restart_ = 30;
    int precond_ = SMH_PRECOND_NONE;
    size_t iterations_ = 0;
    double r_norm_squared_ = 0.0;
    size_t cycles_ = 0;
    int breakdown_ = 0;
};

// Thick-restart Lanczos with full reorthogonalisation -- an extension, not in the reference (smh_eigsh*): the k algebraically largest
// (SMH_EIGSH_LARGEST) or smallest (SMH_EIGSH_SMALLEST) eigenpairs of a SYMMETRIC matrix.  Symmetry is the caller's promise, as it is
// for ConjugateGradient: nothing checks it; a multiple eigenvalue is found once.  ncv: the columns of the basis, k + 2 .. 128 after
// clipping to the dimension (0: min(n, max(2 k + 1, 20))); tol is used as given: pair i is converged when its estimate is at most
// tol * max|theta|; restart_max: the restarts allowed.  After solve: values() / estimates() (k each, wanted-first; empty after
// breakdown 2 or 3, which return nothing), n_conv() (< k: restart_max ran out, the k best pairs are returned all the same),
// restarts(), products(), breakdown() (0; 1 the Krylov space is exhausted; 2 a zero or non-finite start; 3 non-finite data).
// The vectors are not renormalised.
class Lanczos {
  public:
    Lanczos() = default;
    Lanczos(size_t k, int which = SMH_EIGSH_LARGEST, double tol = 1e-10, size_t ncv = 0, size_t restart_max = 1000)
        : k_(k), ncv_(ncv), which_(which), tol_(tol), restart_max_(restart_max) {}
    // device vectors: evecs holds k columns; the overload without it computes no vectors
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const DenseVec<T> &start, MultiVec<T> &evecs) { run_vec(mat, start, evecs.handle()); }
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const DenseVec<T> &start) { run_vec(mat, start, nullptr); }
    // host vectors: evecs becomes k vectors of n (left as it is after breakdown 2 or 3)
    template <typename T>
    void solve(const SparseMatCRS<T> &mat, const std::vector<T> &start, std::vector<std::vector<T>> &evecs) {
        std::vector<T> flat(k_ * start.size());
        begin();
        detail::check(smh_eigsh(mat.handle(), start.data(), start.size(), k_, ncv_, which_, tol_, restart_max_, SMH_SPMV_AUTO, values_.data(),
                                flat.data(), estimates_.data(), &n_conv_, &restarts_, &products_, &breakdown_));
        end();
        if (breakdown_ == 2 || breakdown_ == 3) return;
        evecs.assign(k_, std::vector<T>());
        for (size_t c = 0; c < k_; ++c) evecs[c].assign(flat.begin() + c * start.size(), flat.begin() + (c + 1) * start.size());
    }
    const std::vector<double> &values() const { return values_; }
    const std::vector<double> &estimates() const { return estimates_; }
    size_t n_conv() const { return n_conv_; }
    size_t restarts() const { return restarts_; }
    size_t products() const { return products_; }
    int breakdown() const { return breakdown_; }

  private:
    void begin() { values_.assign(k_ ? k_ : 1, 0.0); estimates_.assign(k_ ? k_ : 1, 0.0); }
    void end() {
        const bool nothing = breakdown_ == 2 || breakdown_ == 3;
        values_.resize(nothing ? 0 : k_);
        estimates_.resize(nothing ? 0 : k_);
    }
    template <typename T>
    void run_vec(const SparseMatCRS<T> &mat, const DenseVec<T> &start, smh_mvec *evecs) {
        begin();
        detail::check(smh_eigsh_vec(mat.handle(), start.handle(), evecs, k_, ncv_, which_, tol_, restart_max_, SMH_SPMV_AUTO, values_.data(),
                                    estimates_.data(), &n_conv_, &restarts_, &products_, &breakdown_));
        end();
    }
    size_t k_ = 6, ncv_ = 0;
    int which_ = SMH_EIGSH_LARGEST;
    double tol_ = 1e-10;
    size_t restart_max_ = 1000;
    std::vector<double> values_, estimates_;
    size_t n_conv_ = 0, restarts_ = 0, products_ = 0;
    int breakdown_ = 0;
};

// Mixed-precision iterative refinement -- an extension, not in the reference (smh_refine_solve*): an f64-accurate x of A x = b whose
// bodies run in f32.  Each outer step forms r = b - A x in f64, scales it by a power of two, converts it to f32, solves
// A_lo d = r_lo from d = 0 with the inner solver (SMH_INNER_CG, _BICGSTAB or _GMRES, preconditioned by SMH_PRECOND_NONE, _JACOBI -- not
// with CG --, _SGS, _ILU or _FSAI) to inner_tol, and adds d to x in f64.  code(): 0 sqrt(r.r) < tol, 1 outer_max steps taken, 2 a
// step did not lower r.r (it is undone).  The forms without mat_lo cast mat themselves; those without factors factor mat_lo through
// ilu0(), and through fsai() (CG) or fsai_ns().
class IterativeRefinement {
  public:
    IterativeRefinement() = default;
    IterativeRefinement(double tol, size_t outer_max = 20, int inner = SMH_INNER_CG, int precond = SMH_PRECOND_NONE, double inner_tol = 1e-4,
                        size_t inner_iter_max = 10000, size_t restart = 30)
        : tol_(tol), outer_max_(outer_max), inner_(inner), precond_(precond), inner_tol_(inner_tol), inner_iter_max_(inner_iter_max), restart_(restart) {}
    // with the f32 matrix and its f32 factors (nullptr where the kind takes none)
    void solve(const SparseMatCRS<double> &mat, const SparseMatCRS<float> &mat_lo, const SparseMatCRS<float> *f, const SparseMatCRS<float> *f2,
               const DenseVec<double> &b, DenseVec<double> &x) {
        detail::check(smh_refine_solve_vec(mat.handle(), mat_lo.handle(), inner_, precond_, f ? f->handle() : nullptr, f2 ? f2->handle() : nullptr, b.handle(),
                                           x.handle(), tol_, outer_max_, inner_tol_, inner_iter_max_, restart_, SMH_SPMV_AUTO, SMH_SPMV_AUTO, 0, &outer_iterations_,
                                           &iterations_, &r_norm_squared_, &code_));
    }
    // host vectors, x updated in place
    void solve(const SparseMatCRS<double> &mat, const SparseMatCRS<float> &mat_lo, const SparseMatCRS<float> *f, const SparseMatCRS<float> *f2,
               const std::vector<double> &b, std::vector<double> &x) {
        detail::check(smh_refine_solve(mat.handle(), mat_lo.handle(), inner_, precond_, f ? f->handle() : nullptr, f2 ? f2->handle() : nullptr, b.data(), b.size(),
                                       x.data(), x.size(), tol_, outer_max_, inner_tol_, inner_iter_max_, restart_, SMH_SPMV_AUTO, SMH_SPMV_AUTO, 0,
                                       &outer_iterations_, &iterations_, &r_norm_squared_, &code_));
    }
    // ... factoring mat_lo first
    template <typename V>
    void solve(const SparseMatCRS<double> &mat, const SparseMatCRS<float> &mat_lo, const V &b, V &x) {
        if (precond_ == SMH_PRECOND_ILU) {
            const SparseMatCRS<float> f = mat_lo.ilu0();
            return solve(mat, mat_lo, &f, nullptr, b, x);
        }
        if (precond_ == SMH_PRECOND_FSAI) {
            const auto f = inner_ == SMH_INNER_CG ? mat_lo.fsai() : mat_lo.fsai_ns();
            return solve(mat, mat_lo, &f.first, &f.second, b, x);
        }
        solve(mat, mat_lo, nullptr, nullptr, b, x);
    }
    // ... casting mat first
    template <typename V>
    void solve(const SparseMatCRS<double> &mat, const V &b, V &x) {
        const SparseMatCRS<float> mat_lo = mat.template cast<float>();
        solve(mat, mat_lo, b, x);
    }
    size_t outer_iterations() const { return outer_iterations_; }
    size_t iterations() const { return iterations_; }  // the inner solves' bodies in total
    double r_norm_squared() const { return r_norm_squared_; }
    int code() const { return code_; }

  private:
    double tol_ = 1e-12;
    size_t outer_max_ = 20;
    int inner_ = SMH_INNER_CG;
    int precond_ = SMH_PRECOND_NONE;
    double inner_tol_ = 1e-4;
    size_t inner_iter_max_ = 10000;
    size_t restart_ = 30;
    size_t outer_iterations_ = 0;
    size_t iterations_ = 0;
    double r_norm_squared_ = 0.0;
    int code_ = 0;
};

}  // namespace sparsemat
