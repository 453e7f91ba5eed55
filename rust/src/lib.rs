//! Drop-in glue between lostinc0de/sparsemat and libsparsemat_hip.so (MI355X / gfx950).
//!
//! NOT COMPILED HERE (no Rust toolchain in the build image).  It shows exactly what a maintainer adds
//! to the crate: a device handle cached next to the CRS arrays, an override of the trait default
//! `SparseMatrix::mvp` (src/sparsematrix.rs:146-158) inside `impl SparseMatrix for SparseMatCRS`
//! (src/sparsemat_crs.rs:95-158), and a device-resident `ConjugateGradient::solve`
//! (src/linearsolver.rs:27-61).  Non-zero statuses are re-raised as the reference's panics.
pub mod ffi;

use std::ffi::CStr;
use std::os::raw::{c_int, c_void};

/// Value types the HIP path accelerates; everything else stays on the reference's CPU loop.
pub trait HipValue: Copy {
    const DTYPE: c_int;
}
impl HipValue for f32 { const DTYPE: c_int = ffi::SMH_F32; }
impl HipValue for f64 { const DTYPE: c_int = ffi::SMH_F64; }

fn check(status: c_int) {
    if status != ffi::SMH_OK {
        // same text as the reference's panic!() ("Matrix is not symmetric", "Dimension mismatch", ...)
        let msg = unsafe { CStr::from_ptr(ffi::smh_last_error()) }.to_string_lossy().into_owned();
        panic!("{}", msg);
    }
}

/// The header this shim was written against (include/sparsemat_hip.h: `#define SMH_ABI_VERSION 3`).  Checked once per process
/// before the first handle is made: a library of another ABI version must not be called through these declarations.
pub const SMH_ABI_VERSION: c_int = 3;

fn check_abi() {
    static ONCE: std::sync::Once = std::sync::Once::new();
    ONCE.call_once(|| {
        let got = unsafe { ffi::smh_abi_version() };
        assert_eq!(got, SMH_ABI_VERSION, "libsparsemat_hip.so has ABI version {}, this shim expects {}", got, SMH_ABI_VERSION);
    });
}

/// Device-resident copy of a `SparseMatCRS<T, u32>`; the Rust side keeps owning the Vecs.
pub struct DeviceCrs {
    handle: *mut ffi::smh_crs,
    n_rows: usize,
}

impl DeviceCrs {
    /// `offset_rows`, `columns`, `values` are the private fields of SparseMatCRS
    /// (src/sparsemat_crs.rs:12-14), borrowed for the duration of the call.
    pub fn new<T: HipValue>(n_rows: usize, n_cols: usize, offset_rows: &[u32], columns: &[u32], values: &[T]) -> Self {
        assert_eq!(offset_rows.len(), n_rows + 1);
        assert_eq!(columns.len(), values.len());
        check_abi();
        let mut handle = std::ptr::null_mut();
        check(unsafe {
            ffi::smh_crs_create(T::DTYPE, n_rows, n_cols, values.len(), offset_rows.as_ptr(), columns.as_ptr(),
                                values.as_ptr() as *const c_void, 1, &mut handle)
        });
        DeviceCrs { handle, n_rows }
    }

    /// `SparseMatrix::mvp` for `V = DenseVec<T>`: returns a new Vec with `n_rows` entries.
    pub fn mvp<T: HipValue + Default>(&self, x: &[T]) -> Vec<T> {
        let mut y = vec![T::default(); self.n_rows];
        check(unsafe {
            ffi::smh_crs_spmv(self.handle, x.as_ptr() as *const c_void, x.len(), y.as_mut_ptr() as *mut c_void,
                              ffi::SMH_SPMV_AUTO)
        });
        y
    }

    /// `ConjugateGradient::solve`: `x` is updated in place; returns (iterations, r.r).
    pub fn cg_solve<T: HipValue>(&self, b: &[T], x: &mut [T], tol: f64, iter_max: usize) -> (usize, f64) {
        let (mut iters, mut rr) = (0usize, 0f64);
        check(unsafe {
            ffi::smh_cg_solve(self.handle, b.as_ptr() as *const c_void, b.len(), x.as_mut_ptr() as *mut c_void,
                              x.len(), tol, iter_max, ffi::SMH_SPMV_AUTO, &mut iters, &mut rr)
        });
        (iters, rr)
    }
}

/// BiCGSTAB for non-symmetric systems -- an extension, not in the reference (`smh_bicgstab_solve`): device-resident like
/// `cg_solve`, same panics and stop rule.  Uncompiled like the rest of this shim.
pub struct BiCGStab {
    pub tol: f64,
    pub iter_max: usize,
}

impl Default for BiCGStab {
    fn default() -> Self {
        BiCGStab { tol: 1e-12, iter_max: 10_000 }
    }
}

impl BiCGStab {
    /// `x` is updated in place; returns (bodies entered, last r.r, breakdown code: 0 none, 1 rho' == 0 or omega == 0,
    /// 2 r^.v == 0, 3 t.t == 0).  A breakdown ends the solve without a panic.
    pub fn solve<T: HipValue>(&self, mat: &DeviceCrs, b: &[T], x: &mut [T]) -> (usize, f64, i32) {
        let (mut iters, mut rr, mut breakdown) = (0usize, 0f64, 0 as std::os::raw::c_int);
        check(unsafe {
            ffi::smh_bicgstab_solve(mat.handle, b.as_ptr() as *const c_void, b.len(), x.as_mut_ptr() as *mut c_void,
                                    x.len(), self.tol, self.iter_max, ffi::SMH_SPMV_AUTO, &mut iters, &mut rr, &mut breakdown)
        });
        (iters, rr, breakdown as i32)
    }

    /// `solve` right-preconditioned (`smh_bicgstab_precond_solve`): `precond` is one of `ffi::SMH_PRECOND_*`, `factor` the ILU(0)
    /// factor's handle with `SMH_PRECOND_ILU` and `None` otherwise.
    pub fn solve_preconditioned<T: HipValue>(&self, mat: &DeviceCrs, precond: std::os::raw::c_int, factor: Option<&DeviceCrs>, b: &[T],
                                             x: &mut [T]) -> (usize, f64, i32) {
        let (mut iters, mut rr, mut breakdown) = (0usize, 0f64, 0 as std::os::raw::c_int);
        let f = factor.map_or(std::ptr::null_mut(), |f| f.handle);
        check(unsafe {
            ffi::smh_bicgstab_precond_solve(mat.handle, precond, f, b.as_ptr() as *const c_void, b.len(), x.as_mut_ptr() as *mut c_void,
                                            x.len(), self.tol, self.iter_max, ffi::SMH_SPMV_AUTO, &mut iters, &mut rr, &mut breakdown)
        });
        (iters, rr, breakdown as i32)
    }
}

/// Restarted GMRES(m) for non-symmetric systems -- an extension, not in the reference (`smh_gmres_solve`): the robust companion of
/// `BiCGStab` (no breakdown before the Krylov space is exhausted, no stagnation near the imaginary axis).  Uncompiled like the rest
/// of this shim.
pub struct Gmres {
    pub tol: f64,
    pub iter_max: usize,
    /// 1 ..= 128 (0: the library's default, 30)
    pub restart: usize,
}

impl Default for Gmres {
    fn default() -> Self {
        Gmres { tol: 1e-12, iter_max: 10_000, restart: 30 }
    }
}

impl Gmres {
    /// `x` is updated in place; returns (bodies entered, the last rebuilt r.r, cycles begun, breakdown code: 0 none, 1 the Krylov
    /// space is exhausted, 2 a cycle's starting residual is exactly zero).  A breakdown ends the solve without a panic.
    pub fn solve<T: HipValue>(&self, mat: &DeviceCrs, b: &[T], x: &mut [T]) -> (usize, f64, usize, i32) {
        let (mut iters, mut rr, mut cycles, mut breakdown) = (0usize, 0f64, 0usize, 0 as std::os::raw::c_int);
        check(unsafe {
            ffi::smh_gmres_solve(mat.handle, b.as_ptr() as *const c_void, b.len(), x.as_mut_ptr() as *mut c_void, x.len(), self.tol,
                                 self.iter_max, self.restart, ffi::SMH_SPMV_AUTO, &mut iters, &mut rr, &mut cycles, &mut breakdown)
        });
        (iters, rr, cycles, breakdown as i32)
    }

    /// `solve` right-preconditioned (`smh_gmres_precond_solve`): `precond` is one of `ffi::SMH_PRECOND_*`, `factor` the ILU(0)
    /// factor's handle with `SMH_PRECOND_ILU` and `None` otherwise.  The r.r returned is the recurrence residual's.
    pub fn solve_preconditioned<T: HipValue>(&self, mat: &DeviceCrs, precond: std::os::raw::c_int, factor: Option<&DeviceCrs>, b: &[T],
                                             x: &mut [T]) -> (usize, f64, usize, i32) {
        let (mut iters, mut rr, mut cycles, mut breakdown) = (0usize, 0f64, 0usize, 0 as std::os::raw::c_int);
        let f = factor.map_or(std::ptr::null_mut(), |f| f.handle);
        check(unsafe {
            ffi::smh_gmres_precond_solve(mat.handle, precond, f, b.as_ptr() as *const c_void, b.len(), x.as_mut_ptr() as *mut c_void,
                                         x.len(), self.tol, self.iter_max, self.restart, ffi::SMH_SPMV_AUTO, &mut iters, &mut rr,
                                         &mut cycles, &mut breakdown)
        });
        (iters, rr, cycles, breakdown as i32)
    }
}

/// CG preconditioned by symmetric Gauss-Seidel -- an extension, not in the reference (`smh_pcg_sgs_solve`): the Jacobi
/// recurrence with z = M^-1 r by two level-scheduled triangular solves.  Uncompiled like the rest of this shim.
pub struct SgsConjugateGradient {
    pub tol: f64,
    pub iter_max: usize,
}

impl Default for SgsConjugateGradient {
    fn default() -> Self {
        SgsConjugateGradient { tol: 1e-12, iter_max: 10_000 }
    }
}

impl SgsConjugateGradient {
    /// `x` is updated in place; returns (bodies entered, last r.r).
    pub fn solve<T: HipValue>(&self, mat: &DeviceCrs, b: &[T], x: &mut [T]) -> (usize, f64) {
        let (mut iters, mut rr) = (0usize, 0f64);
        check(unsafe {
            ffi::smh_pcg_sgs_solve(mat.handle, b.as_ptr() as *const c_void, b.len(), x.as_mut_ptr() as *mut c_void,
                                   x.len(), self.tol, self.iter_max, ffi::SMH_SPMV_AUTO, &mut iters, &mut rr)
        });
        (iters, rr)
    }
}

impl DeviceCrs {
    /// `SparseMatrix::inner_prod` (src/sparsematrix.rs:161-171): lhs^T A rhs.
    pub fn inner_prod<T: HipValue>(&self, lhs: &[T], rhs: &[T]) -> f64 {
        let mut out = 0f64;
        check(unsafe {
            ffi::smh_crs_inner_prod(self.handle, lhs.as_ptr() as *const c_void, lhs.len(), rhs.as_ptr() as *const c_void,
                                    rhs.len(), ffi::SMH_SPMV_AUTO, &mut out)
        });
        out
    }

    /// x = T^-1 b with T the lower (`upper == false`) or upper triangle of this square matrix, the first stored (i, i) of a row
    /// as its diagonal entry (`unit_diagonal`: an implied 1) -- an extension; every operation rounded once, storage order.
    pub fn trisolve<T: HipValue>(&self, b: &[T], x: &mut [T], upper: bool, unit_diagonal: bool) {
        check(unsafe {
            ffi::smh_crs_trisolve(self.handle, if upper { ffi::SMH_TRI_UPPER } else { ffi::SMH_TRI_LOWER },
                                  if unit_diagonal { ffi::SMH_DIAG_UNIT } else { ffi::SMH_DIAG_NON_UNIT },
                                  b.as_ptr() as *const c_void, b.len(), x.as_mut_ptr() as *mut c_void, x.len())
        });
    }

    /// The level schedule of a triangle: (levels, level of every row, kernel launches per solve).
    pub fn trisolve_levels(&self, upper: bool) -> (usize, Vec<u32>, usize) {
        let mut level = vec![0u32; self.n_rows.max(1)];
        let (mut levels, mut launches, mut small) = (0usize, 0usize, 0usize);
        check(unsafe {
            ffi::smh_crs_trisolve_levels(self.handle, if upper { ffi::SMH_TRI_UPPER } else { ffi::SMH_TRI_LOWER }, &mut levels,
                                         level.as_mut_ptr(), &mut launches, &mut small)
        });
        level.truncate(self.n_rows);
        (levels, level, launches)
    }

    /// `SparseMatrix::transpose` (src/sparsematrix.rs:174-184) for `Self = SparseMatCRS`: the arrays the reference's
    /// `ret.set(j, i, val)` loop leaves in a fresh SparseMatCRS (rows reversed, first-push quirk), built on the device.
    pub fn transpose(&self) -> DeviceCrs {
        let mut handle = std::ptr::null_mut();
        check(unsafe { ffi::smh_crs_transpose(self.handle, &mut handle) });
        DeviceCrs { handle, n_rows: unsafe { ffi::smh_crs_n_rows(handle) } }
    }

    /// Reordering (an extension: the reference has none).  A permutation is n u32 with `perm[new] = old`.
    /// `out[i][j] = self[row_perm[i]][col_perm[j]]`: rows keep their entries in storage order, values bit for bit; `None` is
    /// the identity.  A malformed permutation panics with the library's message.
    pub fn permute(&self, row_perm: Option<&[u32]>, col_perm: Option<&[u32]>) -> DeviceCrs {
        let mut handle = std::ptr::null_mut();
        let (rp, rn) = row_perm.map_or((std::ptr::null(), 0), |p| (p.as_ptr(), p.len()));
        let (cp, cn) = col_perm.map_or((std::ptr::null(), 0), |p| (p.as_ptr(), p.len()));
        check(unsafe { ffi::smh_crs_permute(self.handle, rp, rn, cp, cn, &mut handle) });
        DeviceCrs { handle, n_rows: unsafe { ffi::smh_crs_n_rows(handle) } }
    }

    /// `P A P^T` of a square matrix.
    pub fn permute_symmetric(&self, perm: &[u32]) -> DeviceCrs {
        let mut handle = std::ptr::null_mut();
        check(unsafe { ffi::smh_crs_permute_symmetric(self.handle, perm.as_ptr(), perm.len(), &mut handle) });
        DeviceCrs { handle, n_rows: unsafe { ffi::smh_crs_n_rows(handle) } }
    }

    /// The reverse Cuthill-McKee ordering of the symmetrised pattern, computed on the device: (perm, components, levels).
    pub fn rcm(&self) -> (Vec<u32>, usize, usize) {
        let mut perm = vec![0u32; self.n_rows.max(1)];
        let (mut comps, mut levels) = (0usize, 0usize);
        check(unsafe { ffi::smh_crs_rcm(self.handle, perm.as_mut_ptr(), &mut comps, &mut levels) });
        perm.truncate(self.n_rows);
        (perm, comps, levels)
    }

    /// A multicolour ordering of the symmetrised pattern, computed on the device (`smh_crs_color`): (perm, the colour of every
    /// ORIGINAL row, colours, rounds).  `perm` lists the rows by (colour, index), ready for `permute_symmetric`.
    pub fn color(&self, seed: u32) -> (Vec<u32>, Vec<u32>, usize, usize) {
        let mut perm = vec![0u32; self.n_rows.max(1)];
        let mut colors = vec![0u32; self.n_rows.max(1)];
        let (mut n_colors, mut n_rounds) = (0usize, 0usize);
        check(unsafe { ffi::smh_crs_color(self.handle, seed, colors.as_mut_ptr(), perm.as_mut_ptr(), &mut n_colors, &mut n_rounds) });
        perm.truncate(self.n_rows);
        colors.truncate(self.n_rows);
        (perm, colors, n_colors, n_rounds)
    }

    /// (max i - j, max j - i) over the stored entries.
    pub fn bandwidth(&self) -> (u32, u32) {
        let (mut lo, mut hi) = (0u32, 0u32);
        check(unsafe { ffi::smh_crs_bandwidth(self.handle, &mut lo, &mut hi) });
        (lo, hi)
    }

    /// `SparseMatrix::prod` (src/sparsematrix.rs:186-210) with the reference's `Result`: `Err("Dimension mismatch")`
    /// when `self.n_rows() != rhs.n_cols() || self.n_cols() != rhs.n_rows()`; no column tables needed on `rhs`.
    pub fn prod(&self, rhs: &DeviceCrs) -> Result<DeviceCrs, String> {
        let mut handle = std::ptr::null_mut();
        let status = unsafe { ffi::smh_crs_prod(self.handle, rhs.handle, &mut handle) };
        if status == ffi::SMH_ERR_DIM_MISMATCH {
            return Err(unsafe { CStr::from_ptr(ffi::smh_last_error()) }.to_string_lossy().into_owned());
        }
        check(status);
        Ok(DeviceCrs { handle, n_rows: unsafe { ffi::smh_crs_n_rows(handle) } })
    }

    /// `is_symmetric` (src/sparsematrix.rs:212-222) / `is_sorted` (:263-271) on the device copy.
    pub fn is_symmetric(&self) -> bool {
        let mut out: c_int = 0;
        check(unsafe { ffi::smh_crs_is_symmetric(self.handle, &mut out) });
        out != 0
    }
    pub fn is_sorted(&self) -> bool {
        let mut out: c_int = 0;
        check(unsafe { ffi::smh_crs_is_sorted(self.handle, &mut out) });
        out != 0
    }

    /// `ColumnIter::assemble_column_info` (src/sparsemat_crs.rs:180-191) as arrays `(rows, col_ptr, entries)`:
    /// `iter_col(j)` yields `(rows[e], values[e])` for `e in entries[col_ptr[j]..col_ptr[j+1]]`.
    pub fn column_info(&self) -> (Vec<u32>, Vec<u32>, Vec<u32>) {
        let nnz = unsafe { ffi::smh_crs_nnz(self.handle) };
        let n_cols = unsafe { ffi::smh_crs_n_cols(self.handle) };
        let (mut rows, mut col_ptr, mut entries) = (vec![0u32; nnz.max(1)], vec![0u32; n_cols + 1], vec![0u32; nnz.max(1)]);
        check(unsafe { ffi::smh_crs_column_info(self.handle, rows.as_mut_ptr(), col_ptr.as_mut_ptr(), entries.as_mut_ptr()) });
        rows.truncate(nnz);
        entries.truncate(nnz);
        (rows, col_ptr, entries)
    }

    /// `sort_row(i)` for every row (src/sparsemat_crs.rs:163-172), on the device copy.
    pub fn sort_rows(&mut self) {
        check(unsafe { ffi::smh_crs_sort_rows(self.handle) });
    }

    /// The CRS arrays as stored on the device: (n_cols, offset_rows, columns, values) -- what
    /// `SparseMatCRS::from_raw_parts` takes back on the Rust side.
    pub fn raw_parts<T: HipValue + Default>(&self) -> (usize, Vec<u32>, Vec<u32>, Vec<T>) {
        let nnz = unsafe { ffi::smh_crs_nnz(self.handle) };
        let (mut off, mut col, mut val) = (vec![0u32; self.n_rows + 1], vec![0u32; nnz], vec![T::default(); nnz]);
        check(unsafe { ffi::smh_crs_download(self.handle, off.as_mut_ptr(), col.as_mut_ptr(), val.as_mut_ptr() as *mut c_void) });
        (unsafe { ffi::smh_crs_n_cols(self.handle) }, off, col, val)
    }
}

/// Write-only recorder with the call surface of `SparseMatIndexList` assembly (src/sparsematrix.rs:226-233):
/// `add_to` / `set` append in O(1) (no walk of the row's list, src/sparsemat_indexlist.rs:29-42), `to_crs`
/// (src/sparsemat_indexlist.rs:61-63) assembles on the device -- same CRS, bit for bit: rows in order of first
/// appearance, duplicates folded in call order.
pub struct TripletStream<T: HipValue> {
    rows: Vec<u32>,
    cols: Vec<u32>,
    vals: Vec<T>,
    ops: Vec<u8>,
}

impl<T: HipValue> TripletStream<T> {
    pub fn with_capacity(cap: usize) -> Self {
        TripletStream { rows: Vec::with_capacity(cap), cols: Vec::with_capacity(cap), vals: Vec::with_capacity(cap), ops: Vec::with_capacity(cap) }
    }
    pub fn add_to(&mut self, i: usize, j: usize, val: T) { self.push(i, j, val, 0) }
    pub fn set(&mut self, i: usize, j: usize, val: T) { self.push(i, j, val, 1) }
    fn push(&mut self, i: usize, j: usize, val: T, op: u8) {
        self.rows.push(i as u32); self.cols.push(j as u32); self.vals.push(val); self.ops.push(op);
    }
    pub fn to_crs(&self) -> DeviceCrs {
        let mut handle = std::ptr::null_mut();
        check(unsafe {
            ffi::smh_crs_assemble(T::DTYPE, self.vals.len(), self.rows.as_ptr(), self.cols.as_ptr(),
                                  self.vals.as_ptr() as *const c_void, self.ops.as_ptr(), &mut handle)
        });
        DeviceCrs { handle, n_rows: unsafe { ffi::smh_crs_n_rows(handle) } }
    }
}

/// `#[derive(Clone)]` (src/sparsemat_crs.rs:8): an independent device copy (dims, arrays, orphans, kernel settings).
impl Clone for DeviceCrs {
    fn clone(&self) -> Self {
        let mut handle = std::ptr::null_mut();
        check(unsafe { ffi::smh_crs_clone(self.handle, &mut handle) });
        DeviceCrs { handle, n_rows: self.n_rows }
    }
}

impl DeviceCrs {
    /// `SparseMatrix::add` (src/sparsematrix.rs:123-133): `*self.get_mut(i, j) += val` for every entry of `rhs` in storage
    /// order -- new columns pushed to the start of their row, folds into the first occurrence; bit for bit.
    pub fn add(&mut self, rhs: &DeviceCrs) {
        check(unsafe { ffi::smh_crs_add_assign(self.handle, rhs.handle) });
        self.n_rows = unsafe { ffi::smh_crs_n_rows(self.handle) };
    }
    /// `SparseMatrix::sub` (src/sparsematrix.rs:135-143).
    pub fn sub(&mut self, rhs: &DeviceCrs) {
        check(unsafe { ffi::smh_crs_sub_assign(self.handle, rhs.handle) });
        self.n_rows = unsafe { ffi::smh_crs_n_rows(self.handle) };
    }
}

/// A row or column index of `Index = u32`: larger ones are refused, never truncated.
fn index(i: usize) -> u32 {
    u32::try_from(i).expect("index does not fit the u32 index type")
}

impl DeviceCrs {
    /// `SparseMatrix::eye` (src/sparsematrix.rs:91-98) on a SparseMatCRS: `set(i, i, 1)` for i < dim (dim 1 keeps the
    /// container's first-push quirk: no rows, one orphan).
    pub fn eye<T: HipValue>(dim: usize) -> Self {
        check_abi();
        let mut handle = std::ptr::null_mut();
        check(unsafe { ffi::smh_crs_eye(T::DTYPE, dim, &mut handle) });
        DeviceCrs { handle, n_rows: unsafe { ffi::smh_crs_n_rows(handle) } }
    }
    /// The library reads and writes values of the handle's own type: `T` must be it.
    fn assert_dtype<T: HipValue>(&self) {
        assert_eq!(unsafe { ffi::smh_crs_dtype(self.handle) }, T::DTYPE, "value type differs from the matrix's");
    }
    /// `SparseMatrix::get` (src/sparsemat_crs.rs:136-142): the first entry of row i with column j, zero when absent.
    pub fn get<T: HipValue + Default>(&self, i: usize, j: usize) -> T {
        self.assert_dtype::<T>();
        let mut out = T::default();
        check(unsafe { ffi::smh_crs_get(self.handle, i, j, &mut out as *mut T as *mut c_void) });
        out
    }
    /// `get` for every (rows[k], cols[k]) at once.
    pub fn get_many<T: HipValue + Default>(&self, rows: &[u32], cols: &[u32]) -> Vec<T> {
        assert_eq!(rows.len(), cols.len());
        self.assert_dtype::<T>();
        let mut out = vec![T::default(); rows.len()];
        check(unsafe {
            ffi::smh_crs_get_many(self.handle, rows.len(), rows.as_ptr(), cols.as_ptr(), out.as_mut_ptr() as *mut c_void)
        });
        out
    }
    /// `add_to(rows[k], cols[k], values[k])` (`ops[k] != 0`: `set`) for every k in stream order, bit for bit; an empty
    /// `ops` means all `add_to`.  `T` must be the handle's value type.
    pub fn apply<T: HipValue>(&mut self, rows: &[u32], cols: &[u32], values: &[T], ops: &[u8]) {
        assert!(rows.len() == values.len() && cols.len() == values.len() && (ops.is_empty() || ops.len() == values.len()));
        self.assert_dtype::<T>();
        check(unsafe {
            ffi::smh_crs_apply(self.handle, values.len(), rows.as_ptr(), cols.as_ptr(), values.as_ptr() as *const c_void,
                               if ops.is_empty() { std::ptr::null() } else { ops.as_ptr() })
        });
        self.n_rows = unsafe { ffi::smh_crs_n_rows(self.handle) };
    }
    /// `SparseMatrix::set` (src/sparsematrix.rs:226-228): one device call -- batch a stream into `apply`.
    pub fn set<T: HipValue>(&mut self, i: usize, j: usize, val: T) { self.apply(&[index(i)], &[index(j)], &[val], &[1]); }
    /// `SparseMatrix::add_to` (src/sparsematrix.rs:231-233): one device call -- batch a stream into `apply`.
    pub fn add_to<T: HipValue>(&mut self, i: usize, j: usize, val: T) { self.apply(&[index(i)], &[index(j)], &[val], &[]); }
    /// `SparseMatrix::sparsity` (src/sparsematrix.rs:243-246).
    pub fn sparsity(&self) -> f64 {
        let (nnz, n_cols) = unsafe { (ffi::smh_crs_nnz(self.handle), ffi::smh_crs_n_cols(self.handle)) };
        1.0 - nnz as f64 / (self.n_rows * n_cols) as f64
    }
}

/// A reusable update plan (`smh_update_plan`): the targets and the sorted order of one (rows, cols, ops) stream on one
/// `DeviceCrs`.  `execute` leaves what `apply(rows, cols, values, ops)` leaves, bit for bit, in one gather-and-fold pass; it is
/// refused (panic with the library's message) on another matrix or after the matrix's structure changed.
pub struct DeviceUpdatePlan {
    handle: *mut ffi::smh_update_plan,
    n_ops: usize,
}

impl DeviceCrs {
    /// Every operation must land on an existing entry: `apply` the stream once to create them, then plan.  An empty `ops`
    /// means all `add_to`.
    pub fn update_plan(&self, rows: &[u32], cols: &[u32], ops: &[u8]) -> DeviceUpdatePlan {
        assert!(rows.len() == cols.len() && (ops.is_empty() || ops.len() == rows.len()));
        let mut handle = std::ptr::null_mut();
        check(unsafe {
            ffi::smh_update_plan_create(self.handle, rows.len(), rows.as_ptr(), cols.as_ptr(),
                                        if ops.is_empty() { std::ptr::null() } else { ops.as_ptr() }, &mut handle)
        });
        DeviceUpdatePlan { handle, n_ops: rows.len() }
    }
}

impl DeviceUpdatePlan {
    /// `from_zero`: every targeted entry is folded from +0 instead of its stored value ("zero, then assemble" in one pass).
    pub fn execute<T: HipValue>(&mut self, m: &mut DeviceCrs, values: &[T], from_zero: bool) {
        assert_eq!(values.len(), self.n_ops);
        m.assert_dtype::<T>();
        check(unsafe { ffi::smh_update_plan_execute(self.handle, m.handle, values.as_ptr() as *const c_void, from_zero as c_int) });
    }
    /// Operations the plan kept: those at or after their target's last `set`.
    pub fn n_live_ops(&self) -> usize {
        let mut n = 0usize;
        let null = std::ptr::null_mut();
        check(unsafe { ffi::smh_update_plan_stats(self.handle, null, null, &mut n, null, null, null) });
        n
    }
}

impl Drop for DeviceUpdatePlan {
    fn drop(&mut self) {
        unsafe { ffi::smh_update_plan_destroy(self.handle) };
    }
}

// the operators of sparsemat_ops! (src/sparsematrix.rs:370-419); `+` / `-` work on a clone of self inside the library
impl std::ops::AddAssign for DeviceCrs {
    fn add_assign(&mut self, rhs: Self) { self.add(&rhs); }
}
impl std::ops::SubAssign for DeviceCrs {
    fn sub_assign(&mut self, rhs: Self) { self.sub(&rhs); }
}
impl std::ops::Add for DeviceCrs {
    type Output = Self;
    fn add(self, rhs: Self) -> Self {
        let mut handle = std::ptr::null_mut();
        check(unsafe { ffi::smh_crs_add(self.handle, rhs.handle, &mut handle) });
        DeviceCrs { handle, n_rows: unsafe { ffi::smh_crs_n_rows(handle) } }
    }
}
impl std::ops::Sub for DeviceCrs {
    type Output = Self;
    fn sub(self, rhs: Self) -> Self {
        let mut handle = std::ptr::null_mut();
        check(unsafe { ffi::smh_crs_sub(self.handle, rhs.handle, &mut handle) });
        DeviceCrs { handle, n_rows: unsafe { ffi::smh_crs_n_rows(handle) } }
    }
}

impl Drop for DeviceCrs {
    fn drop(&mut self) {
        unsafe { ffi::smh_crs_destroy(self.handle) };
    }
}

/// `SparseMatPar<SparseMatCRS<T, u32>>` (src/sparsemat_par.rs:12-35) on several devices of this process: block `b`
/// = rows `[b R, (b+1) R)`, `R = n_rows / n_blocks` (src/sparsemat_par.rs:21), on device `devices[b]`.  Built from the
/// global CRS arrays the sub-matrices concatenate to (local row ids, global column ids, as the reference stores them).
pub struct DevicePar {
    handle: *mut ffi::smh_par,
    n_rows: usize,
}

impl DevicePar {
    pub fn new<T: HipValue>(n_blocks: usize, devices: Option<&[i32]>, n_rows: usize, n_cols: usize, offset_rows: &[u32],
                            columns: &[u32], values: &[T]) -> Self {
        assert_eq!(offset_rows.len(), n_rows + 1);
        if let Some(d) = devices { assert_eq!(d.len(), n_blocks); }
        let mut handle = std::ptr::null_mut();
        check(unsafe {
            ffi::smh_par_create(T::DTYPE, n_blocks, devices.map_or(std::ptr::null(), |d| d.as_ptr()), n_rows, n_cols,
                                offset_rows.as_ptr(), columns.as_ptr(), values.as_ptr() as *const c_void, 1, &mut handle)
        });
        DevicePar { handle, n_rows }
    }

    /// Not in the reference: the same matrix cut into blocks of equal ENTRY counts (for skewed matrices; block lookup, exchanges
    /// and the solver follow the table of row boundaries `split()` returns).
    pub fn new_nnz_balanced<T: HipValue>(n_blocks: usize, devices: Option<&[i32]>, n_rows: usize, n_cols: usize, offset_rows: &[u32],
                                         columns: &[u32], values: &[T]) -> Self {
        assert_eq!(offset_rows.len(), n_rows + 1);
        if let Some(d) = devices { assert_eq!(d.len(), n_blocks); }
        let mut handle = std::ptr::null_mut();
        check(unsafe {
            ffi::smh_par_create_split(T::DTYPE, n_blocks, devices.map_or(std::ptr::null(), |d| d.as_ptr()), n_rows, n_cols,
                                      offset_rows.as_ptr(), columns.as_ptr(), values.as_ptr() as *const c_void, 1,
                                      ffi::SMH_SPLIT_NNZ, &mut handle)
        });
        DevicePar { handle, n_rows }
    }

    /// `SparseMatrix::mvp` through `iter_row` (src/sparsemat_par.rs:86-89): all blocks run concurrently.
    pub fn mvp<T: HipValue + Default>(&self, x: &[T]) -> Vec<T> {
        let mut y = vec![T::default(); self.n_rows];
        check(unsafe {
            ffi::smh_par_spmv(self.handle, x.as_ptr() as *const c_void, x.len(), y.as_mut_ptr() as *mut c_void, ffi::SMH_SPMV_AUTO)
        });
        y
    }

    /// `ConjugateGradient::solve` with `M = SparseMatPar<..>`: halos of `p` travel device to device, the two dot products are
    /// folded across the blocks on the devices (host vectors in and out).
    pub fn cg_solve<T: HipValue>(&self, b: &[T], x: &mut [T], tol: f64, iter_max: usize) -> (usize, f64) {
        let (mut iters, mut rr) = (0usize, 0f64);
        check(unsafe {
            ffi::smh_par_cg_solve(self.handle, b.as_ptr() as *const c_void, b.len(), x.as_mut_ptr() as *mut c_void, x.len(),
                                  tol, iter_max, ffi::SMH_SPMV_AUTO, &mut iters, &mut rr)
        });
        (iters, rr)
    }
}

/// A `DenseVec` distributed over the blocks of a `DevicePar`: block `b` owns entries `[b R, (b+1) R)`; every block keeps a
/// full-length device buffer, valid as far as the last upload / exchange made it.
pub struct DeviceParVec<'a> {
    handle: *mut ffi::smh_par_vec,
    par: &'a DevicePar,
}

impl<'a> DeviceParVec<'a> {
    pub fn from_slice<T: HipValue>(par: &'a DevicePar, host: &[T]) -> Self {
        let mut handle = std::ptr::null_mut();
        check(unsafe { ffi::smh_par_vec_create(par.handle, host.len(), &mut handle) });
        check(unsafe { ffi::smh_par_vec_upload(handle, host.as_ptr() as *const c_void) });
        DeviceParVec { handle, par }
    }
    pub fn zeros(par: &'a DevicePar) -> Self {
        let mut handle = std::ptr::null_mut();
        check(unsafe { ffi::smh_par_vec_create(par.handle, par.n_rows, &mut handle) });
        DeviceParVec { handle, par }
    }
    pub fn to_vec<T: HipValue + Default>(&self) -> Vec<T> {
        let mut out = vec![T::default(); self.par.n_rows];
        check(unsafe { ffi::smh_par_vec_download(self.handle, out.as_mut_ptr() as *mut c_void) });
        out
    }
}

impl<'a> Drop for DeviceParVec<'a> {
    fn drop(&mut self) {
        unsafe { ffi::smh_par_vec_destroy(self.handle) };
    }
}

impl DevicePar {
    /// The reference's intended `mvp_par` (src/sparsemat_par.rs:37-68), device resident: every block multiplies against the
    /// shared `x`, writes its slice of `y` at `b * R`, then ONE exchange inside the library (RCCL all-gather, or only the
    /// entries each block references) makes `y` usable as the next `x`.  Asynchronous; `synchronize` waits.
    pub fn mvp_dev(&self, x: &DeviceParVec, y: &mut DeviceParVec) {
        check(unsafe { ffi::smh_par_spmv_dev(self.handle, x.handle, y.handle, ffi::SMH_SPMV_AUTO, ffi::SMH_EXCHANGE_AUTO) });
    }
    pub fn synchronize(&self) {
        check(unsafe { ffi::smh_par_synchronize(self.handle) });
    }
    /// `ConjugateGradient::solve` on distributed vectors: scalars stay on the devices, folded across blocks in a fixed order.
    pub fn cg_solve_dev(&self, b: &DeviceParVec, x: &mut DeviceParVec, tol: f64, iter_max: usize) -> (usize, f64) {
        let (mut iters, mut rr) = (0usize, 0f64);
        check(unsafe { ffi::smh_par_cg_solve_vec(self.handle, b.handle, x.handle, tol, iter_max, ffi::SMH_SPMV_AUTO, 0, &mut iters, &mut rr) });
        (iters, rr)
    }
}

impl Drop for DevicePar {
    fn drop(&mut self) {
        unsafe { ffi::smh_par_destroy(self.handle) };
    }
}
