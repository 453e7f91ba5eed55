"""The cases of tests/test_blas1_bits_gpu.py -- data, sizes, element offsets, scalars -- in one place, so that tests/test_blas1_model.py
can show WITHOUT a device that the same cases tell every wrong variant of tests/blas1_model.py apart.

A reduction case is two host arrays and the element offsets at which the device test places them behind a 16-byte aligned address
(off % (16 / sizeof T) != 0: that operand is unaligned and the pair takes the kernel's V = 1 path).  Around and behind every operand
the device buffers hold NaN (reductions) or SENTINEL (element-wise): nothing outside the entries an operation may touch is ever a
harmless number."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
DTYPES = (F32, F64)
K_BLOCK, EW_CAP = 256, 768   # kBlock; stream_grid's cap on the element-wise grids (blas1.hip)


def vec_len(dtype):
    return 16 // np.dtype(dtype).itemsize


def sentinel(dtype):
    """a finite number no operation of the tests produces, and one that every operation would change: x + s, x * s, s - x != x"""
    return np.dtype(dtype).type(-123.4567)


@functools.lru_cache(maxsize=16)
def data(n, dtype, seed):
    """n values uniform in (-1, 1), read-only: shared among the tests.  The last four are at least 0.75 in magnitude: a product of
    two of them is larger than the last bit of every sum in these tests, so a tail that went missing cannot hide in a rounding."""
    a = np.random.default_rng([seed, n]).uniform(-1, 1, n)
    a[-4:] = np.copysign(0.75 + 0.25 * np.abs(a[-4:]), a[-4:])
    a = a.astype(dtype)
    a.setflags(write=False)
    return a


def is_aligned(dtype, *offsets):
    return all(o % vec_len(dtype) == 0 for o in offsets)


# ---- reductions ------------------------------------------------------------------------------------------------------------------
# each boundary of launch_dot's tree: a vector and its tail, a wave, a workgroup, a thread's second vector (1024 / 1027 in f32), the
# second workgroup (reduce_blocks: n / 2048 rounded up), 257 partials (stage 2's threads take a second one), the cap of 1024
# workgroups, and beyond it (every thread strides again)
REDUCTION_SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027, 2047, 2048, 2049, 3075,
                   524_289, 2_097_151, 2_097_152, 2_097_153, 4_198_403)
ALIGN_SIZES = (257, 2049, 524_289)
# the seeds of the size and alignment sweeps.  Chosen: with them the aligned and the unaligned tree give different bits at all three
# ALIGN_SIZES in both types (by chance about one pair in four sums to the same number both ways); tests/test_blas1_model.py asserts it
SEED_X, SEED_Y = 103, 104
TRUNCATION = ((2049, 1027), (1027, 2049))   # (len(x), len(y))
SPECIAL_SIZES = (2049 + 3, 2049 + 6)        # 2052 = whole vectors in both types; 2055: a tail of 3 (f32) / 1 (f64)
ALL_MINUS_ZERO_BIG = 524_289                # every thread of both stages holds a term (what "from_first" needs to show)


def offset_pairs(dtype):
    """(off_x, off_y): x only, y only, both off a 16-byte boundary -- and both ON one again behind a whole vector"""
    offs = range(1, vec_len(dtype))
    pairs = [(o, 0) for o in offs] + [(0, o) for o in offs] + [(o, o) for o in offs] + [(1, vec_len(dtype) - 1), (vec_len(dtype), vec_len(dtype))]
    return list(dict.fromkeys(pairs))


class RedCase:
    def __init__(self, name, group, make, off_x=0, off_y=0, shared=False):
        self.name, self.group, self._make, self.off_x, self.off_y, self.shared = name, group, make, off_x, off_y, shared

    def arrays(self, dtype):
        """(x, y) in `dtype`; shared: both are windows of ONE device buffer, y starting off_y - off_x entries behind x"""
        x, y = self._make(dtype)
        return np.ascontiguousarray(x, dtype), np.ascontiguousarray(y, dtype)

    def aligned(self, dtype):
        return is_aligned(dtype, self.off_x, self.off_y)


def special_positions(n, dtype):
    """where a lone special element sits: in a vector of the body, in the n % V tail, in the last thread's share, in the second
    workgroup's first vector (n > 2048: two workgroups of 256 threads; thread t's first vector holds elements t V ... t V + V - 1)"""
    V = vec_len(dtype)
    pos = {"body": V + 1, "last-thread": 511 * V + V - 1, "second-workgroup": 256 * V}
    if n % V:
        pos["tail"] = n - 1
    return pos


def _lone(n, pos, xv, yv, also=None):
    def make(dtype):
        x, y = data(n, dtype, 31).copy(), np.abs(data(n, dtype, 32)) + dtype(0.25)
        x[pos], y[pos] = xv, yv
        if also is not None:
            x[also[0]], y[also[0]] = also[1], also[2]
        return x, y
    return make


def _minus_zeros(n):
    return lambda dtype: (np.zeros(n, dtype), -np.abs(data(n, dtype, 33)) - dtype(0.5))


def _subnormal_products(n):
    def make(dtype):
        tiny = np.finfo(dtype).tiny
        return (dtype(1.5) + data(n, dtype, 34) * dtype(0.5)) * tiny, data(n, dtype, 35) * dtype(2.0 ** -6)
    return make


def reduction_cases(dtype):
    """every reduction case of the device test, for one type"""
    out = []
    for n in REDUCTION_SIZES:
        out.append(RedCase("n%d" % n, "size", lambda dt, n=n: (data(n, dt, SEED_X), data(n, dt, SEED_Y))))
    for n in ALIGN_SIZES:
        for ox, oy in offset_pairs(dtype):
            out.append(RedCase("n%d-off%d,%d" % (n, ox, oy), "align", lambda dt, n=n: (data(n, dt, SEED_X), data(n, dt, SEED_Y)), ox, oy))
    for nx, ny in TRUNCATION:
        def make(dt, nx=nx, ny=ny):
            x, y = data(nx, dt, 19).copy(), data(ny, dt, 20).copy()
            (x if nx > ny else y)[min(nx, ny):] = np.nan   # the surplus must not reach the sum
            return x, y
        out.append(RedCase("trunc%d,%d" % (nx, ny), "trunc", make))
        out.append(RedCase("trunc%d,%d-off1,0" % (nx, ny), "trunc", make, 1, 0))
    n = 2049
    out.append(RedCase("window-shift1", "overlap", lambda dt: (data(n + 1, dt, 21)[:n], data(n + 1, dt, 21)[1:]), 0, 1, shared=True))
    out.append(RedCase("window-shiftV", "overlap", lambda dt: (data(n + 8, dt, 21)[:n], data(n + 8, dt, 21)[vec_len(dt):n + vec_len(dt)]),
                       0, vec_len(dtype), shared=True))
    inf = np.inf
    for n in SPECIAL_SIZES:
        for where, pos in special_positions(n, dtype).items():
            tag = "n%d-%s" % (n, where)
            out.append(RedCase("nan-" + tag, "special", _lone(n, pos, np.nan, 1.0)))
            out.append(RedCase("+inf-" + tag, "special", _lone(n, pos, inf, 1.0)))
            out.append(RedCase("-inf-" + tag, "special", _lone(n, pos, 2.0, -inf)))
            out.append(RedCase("inf-inf-" + tag, "special", _lone(n, pos, inf, 1.0, also=(1, -inf, 1.0))))
            out.append(RedCase("inf*0-" + tag, "special", _lone(n, pos, inf, -0.0)))
            out.append(RedCase("overflow-" + tag, "special", _lone(n, pos, np.finfo(dtype).max, 1.0, also=(1, np.finfo(dtype).max, 1.0))))
        out.append(RedCase("minus-zeros-n%d" % n, "special", _minus_zeros(n)))
        out.append(RedCase("subnormal-products-n%d" % n, "special", _subnormal_products(n)))
        out.append(RedCase("subnormal-products-n%d-off1,1" % n, "special", _subnormal_products(n), 1, 1))
    out.append(RedCase("minus-zeros-n%d" % ALL_MINUS_ZERO_BIG, "special", _minus_zeros(ALL_MINUS_ZERO_BIG)))
    assert len({c.name for c in out}) == len(out)
    return out


# ---- element-wise ----------------------------------------------------------------------------------------------------------------
SMALL_SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027, 2049)
EW_UNALIGNED_SIZES = (196_607, 196_609)     # 768 * 256 threads: the cap of the VEC = false grid, and one element beyond it
SHORT_RHS = (1027, 4101)                    # (len(y), len(x)): 1027 % V != 0 in both types
EW_SCALAR = 0.7310585786300049              # not representable in f32 (nor is 0.1): the ordinary scalar of the size sweeps
SCALARS = (0.1, 1.0 / 3.0, 1.0 + 2.0 ** -24 + 2.0 ** -50, -0.0, 0.0, 1e39, 1e-46, float("nan"))
SCALAR_SIZE = 1027


def ew_cap_sizes(dtype):
    """the vector path's grid is capped at 768 workgroups of 256 threads, a vector of V elements each: one element short of the
    last full grid, one beyond (a tail element, no second trip yet), and twice the grid and five (a second trip and a tail)"""
    full = EW_CAP * K_BLOCK * vec_len(dtype)
    return (full - 1, full + 1, 2 * full + 5)


class EwCase:
    def __init__(self, name, n_x, n_y, off_x=0, off_y=0):
        self.name, self.n_x, self.n_y, self.off_x, self.off_y = name, n_x, n_y, off_x, off_y

    def arrays(self, dtype):
        return data(self.n_x, dtype, 41), data(self.n_y, dtype, 42)


def ew_cases(dtype):
    out = [EwCase("n%d" % n, n, n) for n in SMALL_SIZES + ew_cap_sizes(dtype)]
    for n in EW_UNALIGNED_SIZES + (5, 257):
        out += [EwCase("n%d-off%d,%d" % (n, ox, oy), n, n, ox, oy) for ox, oy in offset_pairs(dtype)]
    ny, nx = SHORT_RHS
    out += [EwCase("short%d-into%d" % (ny, nx), nx, ny), EwCase("short%d-into%d-off1,0" % (ny, nx), nx, ny, 1, 0),
            EwCase("short%d-into%d-off0,1" % (ny, nx), nx, ny, 0, 1), EwCase("short3-into7", 7, 3), EwCase("short0-into5", 5, 0)]
    assert len({c.name for c in out}) == len(out)
    return out


# ---- special values, element-wise ------------------------------------------------------------------------------------------------
def special_pool(dtype):
    f = np.finfo(dtype)
    sub = f.smallest_subnormal
    vals = [0.0, -0.0, np.inf, -np.inf, np.nan, f.max, -f.max, f.tiny, -f.tiny, sub, -sub, f.tiny - sub, 3 * sub,
            1.0, -1.0, 0.5, 1.5, 1 + f.eps, f.tiny * 1.5, f.max / 2, 2.0 ** -(f.nmant // 2 + 2)]
    return np.array(vals, dtype)


def special_pairs(dtype):
    """(x, y): every element of the pool against every other, 441 entries -- not a multiple of either vector length"""
    p = special_pool(dtype)
    return np.repeat(p, len(p)), np.tile(p, len(p))


def special_scalars(dtype):
    """0.5 and tiny take products into the subnormals and to zero, 2 and max over the top; then the signed zeros, Inf, NaN"""
    f = np.finfo(dtype)
    return (0.5, float(f.tiny), 2.0, float(f.max), float(f.eps), -0.0, 0.0, float("inf"), float("nan"), 1.0)
