//! Raw declarations of include/sparsemat_hip.h (ABI version 3) -- the subset the shim uses.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_double, c_int, c_void};

#[repr(C)] pub struct smh_crs { _private: [u8; 0] }
#[repr(C)] pub struct smh_vec { _private: [u8; 0] }
#[repr(C)] pub struct smh_mvec { _private: [u8; 0] }
#[repr(C)] pub struct smh_update_plan { _private: [u8; 0] }
#[repr(C)] pub struct smh_par { _private: [u8; 0] }
#[repr(C)] pub struct smh_par_vec { _private: [u8; 0] }
#[repr(C)] pub struct smh_comm { _private: [u8; 0] }

pub const SMH_OK: c_int = 0;
pub const SMH_ERR_DIM_MISMATCH: c_int = 1;
pub const SMH_F32: c_int = 0;
pub const SMH_F64: c_int = 1;
pub const SMH_SPMV_AUTO: c_int = 0;
pub const SMH_TRI_LOWER: c_int = 0;
pub const SMH_TRI_UPPER: c_int = 1;
pub const SMH_DIAG_NON_UNIT: c_int = 0;
pub const SMH_DIAG_UNIT: c_int = 1;
pub const SMH_PRECOND_NONE: c_int = 0;
pub const SMH_PRECOND_JACOBI: c_int = 1;
pub const SMH_PRECOND_SGS: c_int = 2;
pub const SMH_PRECOND_ILU: c_int = 3;
pub const SMH_PRECOND_FSAI: c_int = 4;  // smh_refine_solve* only
pub const SMH_INNER_CG: c_int = 0;
pub const SMH_INNER_BICGSTAB: c_int = 1;
pub const SMH_INNER_GMRES: c_int = 2;
pub const SMH_EXCHANGE_NONE: c_int = 0;
pub const SMH_EXCHANGE_ALLGATHER: c_int = 1;
pub const SMH_EXCHANGE_WINDOW: c_int = 2;
pub const SMH_EXCHANGE_AUTO: c_int = 3;
pub const SMH_COMM_ID_BYTES: usize = 128;
pub const SMH_SPLIT_ROWS: c_int = 0;  // the reference's partition: R = n_rows / n_blocks rows per block (sparsemat_par.rs:21)
pub const SMH_SPLIT_NNZ: c_int = 1;   // opt-in: blocks of equal entry counts

extern "C" {
    pub fn smh_abi_version() -> c_int;
    pub fn smh_last_error() -> *const c_char;
    pub fn smh_device_count(count_out: *mut c_int) -> c_int;
    pub fn smh_pool_trim() -> c_int;  // return the device memory the library keeps (csrc/pool.hip) to the HIP runtime
    pub fn smh_pool_stats(kept_bytes_out: *mut usize, live_bytes_out: *mut usize) -> c_int;
    pub fn smh_crs_create(dtype: c_int, n_rows: usize, n_cols: usize, nnz: usize,
                          offset_rows: *const u32, columns: *const u32, values: *const c_void,
                          validate: c_int, out: *mut *mut smh_crs) -> c_int;
    pub fn smh_crs_destroy(m: *mut smh_crs) -> c_int;
    pub fn smh_crs_update_values(m: *mut smh_crs, values_host: *const c_void) -> c_int;
    pub fn smh_crs_spmv(m: *mut smh_crs, x_host: *const c_void, x_len: usize, y_host: *mut c_void,
                        variant: c_int) -> c_int;
    pub fn smh_cg_solve(m: *mut smh_crs, b_host: *const c_void, b_len: usize, x_host_inout: *mut c_void,
                        x_len: usize, tol: c_double, iter_max: usize, variant: c_int,
                        iters_out: *mut usize, rr_out: *mut c_double) -> c_int;
    // extension (not in the reference): Jacobi-preconditioned CG, same contract as smh_cg_solve
    pub fn smh_pcg_jacobi_solve(m: *mut smh_crs, b_host: *const c_void, b_len: usize, x_host_inout: *mut c_void,
                                x_len: usize, tol: c_double, iter_max: usize, variant: c_int,
                                iters_out: *mut usize, rr_out: *mut c_double) -> c_int;
    // extension (not in the reference): BiCGSTAB for non-symmetric systems; breakdown_out: 0 none, 1 rho' == 0 or
    // omega == 0, 2 r^.v == 0, 3 t.t == 0 (a breakdown is a result: the status stays SMH_OK)
    pub fn smh_bicgstab_solve(m: *mut smh_crs, b_host: *const c_void, b_len: usize, x_host_inout: *mut c_void,
                              x_len: usize, tol: c_double, iter_max: usize, variant: c_int,
                              iters_out: *mut usize, rr_out: *mut c_double, breakdown_out: *mut c_int) -> c_int;
    pub fn smh_bicgstab_solve_vec(m: *mut smh_crs, b: *const smh_vec, x: *mut smh_vec, tol: c_double, iter_max: usize,
                                  variant: c_int, check_every: usize,
                                  iters_out: *mut usize, rr_out: *mut c_double, breakdown_out: *mut c_int) -> c_int;
    // extension (not in the reference): restarted GMRES(m) for non-symmetric systems; restart: 1 ..= 128 (0: 30); cycles_out: how many
    // times a v_0 was formed; breakdown_out: 0 none, 1 the Krylov space is exhausted, 2 a cycle's starting residual is exactly zero
    pub fn smh_gmres_solve(m: *mut smh_crs, b_host: *const c_void, b_len: usize, x_host_inout: *mut c_void,
                           x_len: usize, tol: c_double, iter_max: usize, restart: usize, variant: c_int,
                           iters_out: *mut usize, rr_out: *mut c_double, cycles_out: *mut usize, breakdown_out: *mut c_int) -> c_int;
    pub fn smh_gmres_solve_vec(m: *mut smh_crs, b: *const smh_vec, x: *mut smh_vec, tol: c_double, iter_max: usize, restart: usize,
                               variant: c_int, check_every: usize,
                               iters_out: *mut usize, rr_out: *mut c_double, cycles_out: *mut usize, breakdown_out: *mut c_int) -> c_int;
    // extension (not in the reference): thick-restart Lanczos, the k algebraically largest (which = 0) or smallest (1) eigenpairs of a
    // SYMMETRIC matrix (the caller's promise); ncv: 0 or k + 2 ..= 128 after clipping to n; evals_out / est_out: k values; evecs: k x n
    // host values or an smh_mvec of k columns, null for none; breakdown_out: 0 none, 1 the Krylov space is exhausted, 2 a zero or
    // non-finite start, 3 non-finite data (2 and 3 write no pairs)
    pub fn smh_eigsh(m: *mut smh_crs, start_host: *const c_void, start_len: usize, k: usize, ncv: usize, which: c_int, tol: c_double,
                     restart_max: usize, variant: c_int, evals_out: *mut c_double, evecs_host_out: *mut c_void, est_out: *mut c_double,
                     n_conv_out: *mut usize, restarts_out: *mut usize, products_out: *mut usize, breakdown_out: *mut c_int) -> c_int;
    pub fn smh_eigsh_last_timing(host_step_ms_out: *mut c_double, cycles_out: *mut usize, rotation_ms_out: *mut c_double, rotations_out: *mut usize) -> c_int;
    pub fn smh_eigsh_vec(m: *mut smh_crs, start: *const smh_vec, evecs: *mut smh_mvec, k: usize, ncv: usize, which: c_int, tol: c_double,
                         restart_max: usize, variant: c_int, evals_out: *mut c_double, est_out: *mut c_double,
                         n_conv_out: *mut usize, restarts_out: *mut usize, products_out: *mut usize, breakdown_out: *mut c_int) -> c_int;
    // extension: the same solver right-preconditioned (A M^-1 u = b, x = M^-1 u); precond: SMH_PRECOND_*; f: the ILU(0) factor's
    // handle with SMH_PRECOND_ILU, null otherwise
    pub fn smh_gmres_precond_solve(a: *mut smh_crs, precond: c_int, f: *mut smh_crs, b_host: *const c_void, b_len: usize,
                                   x_host_inout: *mut c_void, x_len: usize, tol: c_double, iter_max: usize, restart: usize, variant: c_int,
                                   iters_out: *mut usize, rr_out: *mut c_double, cycles_out: *mut usize, breakdown_out: *mut c_int) -> c_int;
    pub fn smh_gmres_precond_solve_vec(a: *mut smh_crs, precond: c_int, f: *mut smh_crs, b: *const smh_vec, x: *mut smh_vec,
                                       tol: c_double, iter_max: usize, restart: usize, variant: c_int, check_every: usize,
                                       iters_out: *mut usize, rr_out: *mut c_double, cycles_out: *mut usize, breakdown_out: *mut c_int) -> c_int;
    // extension: BiCGSTAB right-preconditioned the same way (precond and f as above)
    pub fn smh_bicgstab_precond_solve(a: *mut smh_crs, precond: c_int, f: *mut smh_crs, b_host: *const c_void, b_len: usize,
                                      x_host_inout: *mut c_void, x_len: usize, tol: c_double, iter_max: usize, variant: c_int,
                                      iters_out: *mut usize, rr_out: *mut c_double, breakdown_out: *mut c_int) -> c_int;
    pub fn smh_bicgstab_precond_solve_vec(a: *mut smh_crs, precond: c_int, f: *mut smh_crs, b: *const smh_vec, x: *mut smh_vec,
                                          tol: c_double, iter_max: usize, variant: c_int, check_every: usize,
                                          iters_out: *mut usize, rr_out: *mut c_double, breakdown_out: *mut c_int) -> c_int;
    // extensions (not in the reference): level-scheduled sparse triangular solves, the symmetric Gauss-Seidel preconditioner
    // M = (D + L) D^-1 (D + U) built on them, and its CG (same contract as smh_pcg_jacobi_solve)
    pub fn smh_crs_trisolve_levels(m: *mut smh_crs, uplo: c_int, n_levels_out: *mut usize, level_of_row_out: *mut u32,
                                   n_launches_out: *mut usize, small_level_rows_out: *mut usize) -> c_int;
    pub fn smh_crs_trisolve(m: *mut smh_crs, uplo: c_int, diag: c_int, b_host: *const c_void, b_len: usize, x_host: *mut c_void,
                            x_len: usize) -> c_int;
    pub fn smh_crs_trisolve_vec(m: *mut smh_crs, uplo: c_int, diag: c_int, b: *const smh_vec, x: *mut smh_vec) -> c_int;
    pub fn smh_crs_sgs_apply_vec(m: *mut smh_crs, r: *const smh_vec, z: *mut smh_vec) -> c_int;
    pub fn smh_pcg_sgs_solve(m: *mut smh_crs, b_host: *const c_void, b_len: usize, x_host_inout: *mut c_void,
                             x_len: usize, tol: c_double, iter_max: usize, variant: c_int,
                             iters_out: *mut usize, rr_out: *mut c_double) -> c_int;
    pub fn smh_pcg_sgs_solve_vec(m: *mut smh_crs, b: *const smh_vec, x: *mut smh_vec, tol: c_double, iter_max: usize,
                                 variant: c_int, check_every: usize, iters_out: *mut usize, rr_out: *mut c_double) -> c_int;
    pub fn smh_crs_ilu0(a: *const smh_crs, f_out: *mut *mut smh_crs, zero_pivot_out: *mut usize) -> c_int;
    pub fn smh_crs_ilu0_refactor(f: *mut smh_crs, a: *const smh_crs, zero_pivot_out: *mut usize) -> c_int;
    pub fn smh_crs_ilu_apply_vec(f: *mut smh_crs, r: *const smh_vec, z: *mut smh_vec) -> c_int;
    pub fn smh_pcg_ilu_solve(a: *mut smh_crs, f: *mut smh_crs, b_host: *const c_void, b_len: usize, x_host_inout: *mut c_void,
                             x_len: usize, tol: c_double, iter_max: usize, variant: c_int,
                             iters_out: *mut usize, rr_out: *mut c_double) -> c_int;
    pub fn smh_pcg_ilu_solve_vec(a: *mut smh_crs, f: *mut smh_crs, b: *const smh_vec, x: *mut smh_vec, tol: c_double, iter_max: usize,
                                 variant: c_int, check_every: usize, iters_out: *mut usize, rr_out: *mut c_double) -> c_int;
    // extension: the factorized sparse approximate inverse (g lower triangular on a's lower pattern, gt its transpose; *not_spd_out:
    // the first row whose last pivot is not > 0, usize::MAX without one), z = G^T (G r) by two products, and the CG it preconditions
    pub fn smh_crs_fsai(a: *const smh_crs, g_out: *mut *mut smh_crs, gt_out: *mut *mut smh_crs, not_spd_out: *mut usize) -> c_int;
    pub fn smh_crs_fsai_apply_vec(g: *mut smh_crs, gt: *mut smh_crs, r: *const smh_vec, z: *mut smh_vec) -> c_int;
    pub fn smh_pcg_fsai_solve(a: *mut smh_crs, g: *mut smh_crs, gt: *mut smh_crs, b_host: *const c_void, b_len: usize, x_host_inout: *mut c_void,
                              x_len: usize, tol: c_double, iter_max: usize, variant: c_int, iters_out: *mut usize, rr_out: *mut c_double) -> c_int;
    pub fn smh_pcg_fsai_solve_vec(a: *mut smh_crs, g: *mut smh_crs, gt: *mut smh_crs, b: *const smh_vec, x: *mut smh_vec, tol: c_double,
                                  iter_max: usize, variant: c_int, check_every: usize, iters_out: *mut usize, rr_out: *mut c_double) -> c_int;
    // extension: the non-symmetric FSAI, two factors G_U G_L ~ A^-1, and GMRES / BiCGSTAB right-preconditioned by a pair of product
    // handles (its (gl, gu), or smh_crs_fsai's (g, gt) for a symmetric matrix)
    pub fn smh_crs_fsai_ns(a: *const smh_crs, gl_out: *mut *mut smh_crs, gu_out: *mut *mut smh_crs, singular_out: *mut usize) -> c_int;
    pub fn smh_crs_fsai_ns_apply_vec(gl: *mut smh_crs, gu: *mut smh_crs, r: *const smh_vec, z: *mut smh_vec) -> c_int;
    pub fn smh_gmres_fsai_solve(a: *mut smh_crs, g: *mut smh_crs, gt: *mut smh_crs, b_host: *const c_void, b_len: usize, x_host_inout: *mut c_void,
                                x_len: usize, tol: c_double, iter_max: usize, restart: usize, variant: c_int, iters_out: *mut usize,
                                rr_out: *mut c_double, cycles_out: *mut usize, breakdown_out: *mut c_int) -> c_int;
    pub fn smh_gmres_fsai_solve_vec(a: *mut smh_crs, g: *mut smh_crs, gt: *mut smh_crs, b: *const smh_vec, x: *mut smh_vec, tol: c_double,
                                    iter_max: usize, restart: usize, variant: c_int, check_every: usize, iters_out: *mut usize,
                                    rr_out: *mut c_double, cycles_out: *mut usize, breakdown_out: *mut c_int) -> c_int;
    pub fn smh_bicgstab_fsai_solve(a: *mut smh_crs, g: *mut smh_crs, gt: *mut smh_crs, b_host: *const c_void, b_len: usize, x_host_inout: *mut c_void,
                                   x_len: usize, tol: c_double, iter_max: usize, variant: c_int, iters_out: *mut usize, rr_out: *mut c_double,
                                   breakdown_out: *mut c_int) -> c_int;
    pub fn smh_bicgstab_fsai_solve_vec(a: *mut smh_crs, g: *mut smh_crs, gt: *mut smh_crs, b: *const smh_vec, x: *mut smh_vec, tol: c_double,
                                       iter_max: usize, variant: c_int, check_every: usize, iters_out: *mut usize, rr_out: *mut c_double,
                                       breakdown_out: *mut c_int) -> c_int;
    // extension: mixed precision.  A copy of a handle / a vector in the other dtype (f64 -> f32 to nearest even, f32 -> f64 exact), and
    // iterative refinement: the residual and the update in f64, the correction by an f32 solver on a_lo (inner: SMH_INNER_*; precond:
    // SMH_PRECOND_*, SMH_PRECOND_FSAI with the pair f_lo, f2_lo); 0 stands for the default in outer_max, inner_tol, inner_iter_max, restart
    pub fn smh_crs_cast(a: *const smh_crs, dtype: c_int, out: *mut *mut smh_crs, overflow_out: *mut usize) -> c_int;
    pub fn smh_vec_cast(src: *const smh_vec, dst: *mut smh_vec) -> c_int;
    pub fn smh_refine_solve_vec(a: *mut smh_crs, a_lo: *mut smh_crs, inner: c_int, precond: c_int, f_lo: *mut smh_crs, f2_lo: *mut smh_crs,
                                b: *const smh_vec, x: *mut smh_vec, tol: c_double, outer_max: usize, inner_tol: c_double, inner_iter_max: usize,
                                restart: usize, variant: c_int, variant_lo: c_int, check_every: usize, outer_out: *mut usize,
                                inner_iters_out: *mut usize, rr_out: *mut c_double, code_out: *mut c_int) -> c_int;
    pub fn smh_refine_solve(a: *mut smh_crs, a_lo: *mut smh_crs, inner: c_int, precond: c_int, f_lo: *mut smh_crs, f2_lo: *mut smh_crs,
                            b_host: *const c_void, b_len: usize, x_host_inout: *mut c_void, x_len: usize, tol: c_double, outer_max: usize,
                            inner_tol: c_double, inner_iter_max: usize, restart: usize, variant: c_int, variant_lo: c_int, check_every: usize,
                            outer_out: *mut usize, inner_iters_out: *mut usize, rr_out: *mut c_double, code_out: *mut c_int) -> c_int;
    pub fn smh_crs_inner_prod(m: *mut smh_crs, lhs_host: *const c_void, lhs_len: usize, rhs_host: *const c_void,
                              rhs_len: usize, variant: c_int, out: *mut c_double) -> c_int;
    // add_to (ops[k] == 0 / ops null) or set (ops[k] == 1) stream -> the CRS `to_crs()` would return
    pub fn smh_crs_assemble(dtype: c_int, n_ops: usize, rows: *const u32, cols: *const u32, values: *const c_void,
                            ops: *const u8, out: *mut *mut smh_crs) -> c_int;
    // the same stream applied to a SparseMatCRS itself (push prepends, first-push quirk): what transpose / prod fill
    pub fn smh_crs_replay(dtype: c_int, n_ops: usize, rows: *const u32, cols: *const u32, values: *const c_void,
                          ops: *const u8, out: *mut *mut smh_crs) -> c_int;
    pub fn smh_crs_transpose(a: *const smh_crs, out: *mut *mut smh_crs) -> c_int;
    pub fn smh_crs_set_stream_xs(m: *mut smh_crs, mode: c_int) -> c_int;  // K1s with x staged in LDS: -1 auto, 0 never, 1 whenever the tiles allow
    pub fn smh_crs_set_stream_direct(m: *mut smh_crs, mode: c_int) -> c_int;  // K1s XD (stage offsets instead of column codes): -1 auto, 0 never, 1 whenever x is staged
    pub fn smh_crs_stream_direct(m: *mut smh_crs, direct_out: *mut c_int) -> c_int;
    pub fn smh_crs_stream_layout(m: *mut smh_crs, coded_out: *mut c_int, byte_lengths_out: *mut c_int, small_tiles_out: *mut c_int, xs_chunks_out: *mut c_int) -> c_int;
    pub fn smh_last_transpose_route() -> c_int;  // 0 general (device-wide sort), 1 two bucketed passes: diagnostics only
    pub fn smh_crs_orphans(m: *const smh_crs) -> usize;
    pub fn smh_crs_prod(a: *const smh_crs, b: *const smh_crs, out: *mut *mut smh_crs) -> c_int;
    // #[derive(Clone)] and SparseMatrix::add / sub (src/sparsematrix.rs:123-143) with the operators of sparsemat_ops! (:370-433)
    pub fn smh_crs_clone(a: *const smh_crs, out: *mut *mut smh_crs) -> c_int;
    // reordering (an extension; a permutation is n u32 with perm[new] = old)
    pub fn smh_crs_permute(a: *const smh_crs, row_perm: *const u32, n_row_perm: usize, col_perm: *const u32, n_col_perm: usize,
                           out: *mut *mut smh_crs) -> c_int;
    pub fn smh_crs_permute_dev(a: *const smh_crs, row_perm_dev: *const u32, n_row_perm: usize, col_perm_dev: *const u32,
                               n_col_perm: usize, out: *mut *mut smh_crs) -> c_int;
    pub fn smh_crs_permute_symmetric(a: *const smh_crs, perm: *const u32, n_perm: usize, out: *mut *mut smh_crs) -> c_int;
    pub fn smh_crs_permute_symmetric_dev(a: *const smh_crs, perm_dev: *const u32, n_perm: usize, out: *mut *mut smh_crs) -> c_int;
    pub fn smh_crs_bandwidth(m: *const smh_crs, lower_out: *mut u32, upper_out: *mut u32) -> c_int;
    pub fn smh_crs_span_fraction(m: *mut smh_crs, out: *mut f64) -> c_int;
    // K1r: per phase of the plan (smh_crs_ring_plan's n_phases), the row length of a ring phase whose rows are all equally long, else 0
    pub fn smh_crs_ring_regular(m: *mut smh_crs, len_out: *mut u32) -> c_int;
    // K1r: what the ring phases stream for their values -- 0 the value array, 1 24-bit fixed-point records (k * 2^exponent), -1 refused
    pub fn smh_crs_ring_values(m: *mut smh_crs, form_out: *mut c_int, exponent_out: *mut c_int) -> c_int;
    // K1r: the form of the ring kernel a plain product would launch now -- 0 three bodies, 1 regular + loading body, 2 the all-regular form
    // (768-thread workgroups), -1 no ring kernel --, its workgroup size and how many such workgroups a CU holds at once
    pub fn smh_crs_ring_launch_form(m: *mut smh_crs, form_out: *mut c_int, threads_out: *mut c_int, resident_per_cu_out: *mut c_int) -> c_int;
    pub fn smh_crs_rcm(m: *const smh_crs, perm_out: *mut u32, n_components_out: *mut usize, n_levels_out: *mut usize) -> c_int;
    pub fn smh_crs_rcm_dev(m: *const smh_crs, perm_out_dev: *mut u32, n_components_out: *mut usize, n_levels_out: *mut usize) -> c_int;
    pub fn smh_crs_color(m: *const smh_crs, seed: u32, colors_out: *mut u32, perm_out: *mut u32, n_colors_out: *mut usize, n_rounds_out: *mut usize) -> c_int;
    pub fn smh_crs_color_dev(m: *const smh_crs, seed: u32, colors_out_dev: *mut u32, perm_out_dev: *mut u32, n_colors_out: *mut usize, n_rounds_out: *mut usize) -> c_int;
    pub fn smh_vec_permute(dst: *mut smh_vec, src: *const smh_vec, perm: *const u32, n_perm: usize, inverse: c_int) -> c_int;
    pub fn smh_vec_permute_dev(dst: *mut smh_vec, src: *const smh_vec, perm_dev: *const u32, n_perm: usize, inverse: c_int) -> c_int;
    pub fn smh_crs_add(a: *const smh_crs, b: *const smh_crs, out: *mut *mut smh_crs) -> c_int;
    pub fn smh_crs_sub(a: *const smh_crs, b: *const smh_crs, out: *mut *mut smh_crs) -> c_int;
    pub fn smh_crs_add_assign(a: *mut smh_crs, b: *const smh_crs) -> c_int;
    pub fn smh_crs_sub_assign(a: *mut smh_crs, b: *const smh_crs) -> c_int;
    pub fn smh_last_add_route() -> c_int;  // 0 general, 1 short rows, 2 structure unchanged, 3 same pattern: diagnostics only
    // SparseMatrix::get / set / add_to / eye (src/sparsematrix.rs:91-98, 224-233; src/sparsemat_crs.rs:54-92, 136-150)
    pub fn smh_crs_get(m: *const smh_crs, i: usize, j: usize, value_out: *mut c_void) -> c_int;
    pub fn smh_crs_get_many(m: *const smh_crs, n: usize, rows: *const u32, cols: *const u32, values_out: *mut c_void) -> c_int;
    pub fn smh_crs_get_many_dev(m: *const smh_crs, n: usize, rows_dev: *const u32, cols_dev: *const u32,
                                values_out_dev: *mut c_void) -> c_int;
    pub fn smh_crs_apply(m: *mut smh_crs, n_ops: usize, rows: *const u32, cols: *const u32, values: *const c_void,
                         ops: *const u8) -> c_int;
    pub fn smh_crs_apply_dev(m: *mut smh_crs, n_ops: usize, rows_dev: *const u32, cols_dev: *const u32,
                             values_dev: *const c_void, ops_dev: *const u8) -> c_int;
    pub fn smh_last_apply_route() -> c_int;  // 0 general, 1 values only, 2 replay: diagnostics only
    pub fn smh_last_solve_replays() -> c_int;  // graph launches of this thread's last single-matrix solve (0: none captured): diagnostics only
    // a reusable update plan: re-assembly on a fixed pattern as one gather-and-fold pass (every operation must land on an
    // existing entry; bound to one handle in one structure; from_zero != 0 folds every targeted entry from +0)
    pub fn smh_update_plan_create(m: *const smh_crs, n_ops: usize, rows: *const u32, cols: *const u32, ops: *const u8,
                                  out: *mut *mut smh_update_plan) -> c_int;
    pub fn smh_update_plan_create_dev(m: *const smh_crs, n_ops: usize, rows_dev: *const u32, cols_dev: *const u32,
                                      ops_dev: *const u8, out: *mut *mut smh_update_plan) -> c_int;
    pub fn smh_update_plan_execute(p: *mut smh_update_plan, m: *mut smh_crs, values: *const c_void, from_zero: c_int) -> c_int;
    pub fn smh_update_plan_execute_dev(p: *mut smh_update_plan, m: *mut smh_crs, values_dev: *const c_void, from_zero: c_int) -> c_int;
    pub fn smh_update_plan_stats(p: *const smh_update_plan, n_ops: *mut usize, n_targets: *mut usize, n_live_ops: *mut usize,
                                 longest_run: *mut usize, long_run_threshold: *mut usize, device_bytes: *mut usize) -> c_int;
    pub fn smh_update_plan_destroy(p: *mut smh_update_plan) -> c_int;
    pub fn smh_crs_eye(dtype: c_int, dim: usize, out: *mut *mut smh_crs) -> c_int;
    pub fn smh_crs_is_symmetric(m: *const smh_crs, out: *mut c_int) -> c_int;
    pub fn smh_crs_is_sorted(m: *const smh_crs, out: *mut c_int) -> c_int;
    pub fn smh_crs_column_info(m: *const smh_crs, rows: *mut u32, col_ptr: *mut u32, entries: *mut u32) -> c_int;
    pub fn smh_crs_sort_rows(m: *mut smh_crs) -> c_int;
    // SparseMatPar<SparseMatCRS<T,u32>>, one process: block b on device device_ids[b] (null: b mod device count)
    pub fn smh_par_create(dtype: c_int, n_blocks: usize, device_ids: *const c_int, n_rows: usize, n_cols: usize,
                          offset_rows: *const u32, columns: *const u32, values: *const c_void, validate: c_int,
                          out: *mut *mut smh_par) -> c_int;
    // the same with the rows cut by entry count (SMH_SPLIT_NNZ): the partition becomes a table of n_blocks + 1 row boundaries
    pub fn smh_par_create_split(dtype: c_int, n_blocks: usize, device_ids: *const c_int, n_rows: usize, n_cols: usize,
                                offset_rows: *const u32, columns: *const u32, values: *const c_void, validate: c_int,
                                split_mode: c_int, out: *mut *mut smh_par) -> c_int;
    pub fn smh_par_split(p: *const smh_par, rows_out: *mut usize) -> c_int;
    // exchange overlapped with the product of the rows that reference no other block (default on; bit-identical either way)
    pub fn smh_par_set_overlap(p: *mut smh_par, on: c_int) -> c_int;
    pub fn smh_par_interior(p: *const smh_par, local_block: usize, variant: c_int, row_begin: *mut usize, row_end: *mut usize) -> c_int;
    pub fn smh_par_destroy(p: *mut smh_par) -> c_int;
    pub fn smh_par_spmv(p: *mut smh_par, x_host: *const c_void, x_len: usize, y_host: *mut c_void, variant: c_int) -> c_int;
    pub fn smh_par_cg_solve(p: *mut smh_par, b_host: *const c_void, b_len: usize, x_host_inout: *mut c_void, x_len: usize,
                            tol: c_double, iter_max: usize, variant: c_int, iters_out: *mut usize,
                            rr_out: *mut c_double) -> c_int;
    // device-resident form: distributed vectors (one full-length buffer per local block), y = A x + ONE exchange of y
    // inside the library (in-place ncclAllGather / grouped ncclSend+ncclRecv of the referenced window / peer reads)
    pub fn smh_par_vec_create(p: *mut smh_par, n: usize, out: *mut *mut smh_par_vec) -> c_int;
    pub fn smh_par_vec_destroy(v: *mut smh_par_vec) -> c_int;
    pub fn smh_par_vec_upload(v: *mut smh_par_vec, host: *const c_void) -> c_int;
    pub fn smh_par_vec_download(v: *const smh_par_vec, host: *mut c_void) -> c_int;
    pub fn smh_par_spmv_dev(p: *mut smh_par, x: *const smh_par_vec, y: *mut smh_par_vec, variant: c_int, exchange: c_int) -> c_int;
    pub fn smh_par_exchange(p: *mut smh_par, v: *mut smh_par_vec, mode: c_int) -> c_int;
    pub fn smh_par_synchronize(p: *mut smh_par) -> c_int;
    pub fn smh_par_cg_solve_vec(p: *mut smh_par, b: *const smh_par_vec, x: *mut smh_par_vec, tol: c_double, iter_max: usize,
                                variant: c_int, check_every: usize, iters_out: *mut usize, rr_out: *mut c_double) -> c_int;
    // one process per GPU: ncclGetUniqueId on one rank, ncclCommInitRank on all, the rank's own block
    pub fn smh_comm_unique_id(id_out: *mut c_void) -> c_int;
    pub fn smh_comm_create(id: *const c_void, n_ranks: c_int, rank: c_int, out: *mut *mut smh_comm) -> c_int;
    pub fn smh_comm_destroy(c: *mut smh_comm) -> c_int;
    pub fn smh_par_create_rank(comm: *mut smh_comm, n_rows: usize, block: *mut smh_crs, out: *mut *mut smh_par) -> c_int;
    // row_begin = this rank's first row (usize::MAX: the reference's partition; all ranks or none)
    pub fn smh_par_create_rank_split(comm: *mut smh_comm, n_rows: usize, block: *mut smh_crs, row_begin: usize, out: *mut *mut smh_par) -> c_int;
    pub fn smh_crs_n_rows(m: *const smh_crs) -> usize;
    pub fn smh_crs_n_cols(m: *const smh_crs) -> usize;
    pub fn smh_crs_dtype(m: *const smh_crs) -> c_int;
    pub fn smh_crs_nnz(m: *const smh_crs) -> usize;
    pub fn smh_crs_download(m: *const smh_crs, offset_rows: *mut u32, columns: *mut u32, values: *mut c_void) -> c_int;
}
