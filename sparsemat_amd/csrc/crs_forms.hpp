// crs_forms.hpp -- what crosses between the host sides of the library's files: capi.hip (the core of the C boundary: errors, the life
// cycle of a handle), crs_forms.hip (what a CRS handle derives, and when it goes), spmv_dispatch.hip (which kernel a product runs,
// and its launches) and the entry points that live with their feature's device code.  What the kernel files and the solvers call
// is in internal.hpp.
#pragma once
#include "internal.hpp"

namespace smh {

// ---- capi.hip --------------------------------------------------------------------------------------------------------------------
void clear_error();  // (beside set_error) an error that a fallback has absorbed: its text goes
inline bool valid_dtype(int dt) { return dt == SMH_F32 || dt == SMH_F64; }
// a fresh handle over device arrays, made on the current device with the create-time inspection done.  The first form takes the
// arrays of `arrays` (ensure_split makes the two parts of a K2s split with it); the second owns or borrows the three it is given
int wrap_arrays(int dtype, const ::smh_crs *like, size_t n_rows, size_t n_cols, size_t nnz, CrsArrays &arrays, int validate, ::smh_crs **out);
int wrap_arrays(int dtype, const ::smh_crs *like, size_t n_rows, size_t n_cols, size_t nnz, uint32_t *off, uint32_t *col, void *val, bool owns,
                int validate, ::smh_crs **out);
void replace_state(::smh_crs *a, ::smh_crs *fresh, bool keep_arrays);  // `a` takes the state of `fresh`, which goes (add_assign, apply)
int vec_check_pair(const ::smh_vec *x, const ::smh_vec *y);            // two vector handles of one value type

// ---- the entry points' helpers that other features call ----------------------------------------------------------------------------
// assemble.hip: the add_to / set stream -> CRS behind smh_crs_assemble / replay [_dev]; transpose, add / sub and apply replay with it
int assemble_common(smh_dtype dtype, size_t n_ops, const uint32_t *rows, const uint32_t *cols, const void *values, const uint8_t *ops,
                    bool on_device, bool into_crs, ::smh_crs **out, bool transposing = false);
UpdMatrix upd_view(const ::smh_crs *m);  // matupdate.hip: the handle as get / apply / the update plan see it
int reduce_scratch(void **out);          // blas1.hip: the calling thread's scratch for reductions (dot, inner_prod) on the current device

// ---- defined here: the read-back the builders and the create-time inspection share ------------------------------------------------
// "Launch into a few device words, bring them to the host": launch(d) fills `count` elements at d (device scratch), which are
// copied to `host` behind a synchronisation of s.  The second form allocates the scratch itself.
template <typename U, typename F> int read_back(U *d, U *host, size_t count, hipStream_t s, F &&launch) {
    SMH_TRY(launch(d));
    SMH_HIP(hipMemcpyAsync(host, d, count * sizeof(U), hipMemcpyDeviceToHost, s));
    SMH_HIP(hipStreamSynchronize(s));
    return SMH_OK;
}
template <typename U, typename F> int read_back(U *host, size_t count, hipStream_t s, F &&launch) {
    Scratch scr;
    U *d = nullptr;
    SMH_TRY(scr.alloc(&d, count));
    return read_back(d, host, count, s, launch);
}

// ---- crs_forms.hip: the lazy builders (each a no-op once its form is there) and what drops the forms -------------------------------
extern const uint32_t kSplitMinLong;
int ensure_merge_ws(::smh_crs *m);
int ensure_ring_plan(::smh_crs *m, bool with_bands = true);
int ensure_colblock(::smh_crs *m);
int ensure_colfused(::smh_crs *m);
int ensure_split(::smh_crs *m);
int vector_uses_ring(::smh_crs *m, bool *out);
enum class Changed { Values, Order, BlockWidth };  // update_values / apply's values-only route; sort_rows; set_colblock_shift
void invalidate(::smh_crs *m, Changed what);
// the values changed where invalidate is not called (smh_crs_scale): K1r's chunk records go, the next product tests the new values
void ring_values_changed(::smh_crs *m);
// K1s configuration the STREAM variant runs with for this handle (builds the code tables on first use)
struct StreamCfg {
    int rpt = 1;
    bool single_pass = false;
    const uint16_t *code = nullptr;
    const uint32_t *cwin = nullptr;
    const uint8_t *len8 = nullptr;
    const uint32_t *tbase = nullptr;
    bool small = false; // no tile beyond kStreamCapSmall entries: the two-chunk body
    int xs = 0;         // ... and every tile's column intervals fit an LDS stage of x: 16-byte chunks per thread (2 or 4), 0 = no
    bool direct = false;  // `code` holds byte offsets into that stage, not column codes: only K1s XD (spmv_stream_xd.hip) reads it
    const void *dict = nullptr;  // ... with value-dictionary indices in their spare bits (K1s XD-V): the kernel does not read the values
    bool dict_high = false;      // ... in the high spare bits alone (few values)
};
int stream_cfg(::smh_crs *m, StreamCfg *c, bool recode = false);
int recode_stream(::smh_crs *m);

// ---- spmv_dispatch.hip -----------------------------------------------------------------------------------------------------------
extern const size_t kColblockMinXBytes;
uint32_t cb_shift_for(const ::smh_crs *m);
uint32_t cf_shift_for(const ::smh_crs *m);
size_t blocks_for(size_t n_cols, uint32_t shift);
int auto_lanes(const ::smh_crs *m);
int resolve_variant(const ::smh_crs *m, int variant);
// smh_crs_prepare: resolve, build every form the variant runs on, fall back as the first product would
int prepare_forms(::smh_crs *m, int variant);
// smh_crs_inner_prod*: lhs^T (A rhs) into *res (device) by the matrix's own kernel on the handle's stream; lhs has n_rows entries
int spmv_inner_prod(::smh_crs *m, const void *d_lhs, const void *d_rhs, size_t rhs_len, int variant, void *scratch, void *res);

}  // namespace smh
