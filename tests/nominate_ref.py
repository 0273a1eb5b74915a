"""K3 nominations and the fp16 operand image: float64 references and DERIVED tolerances (plain NumPy, no GPU).  TEST INFRASTRUCTURE.

Two contracts are restated here, from their documentation and not from a kernel's instruction order:

* the NOMINATING distance of a (row, query) pair, max(1 - x.q / (|x||q|), 0) with the zero-vector rules of nomination_dist (gemm.h):
  a zero query is at distance 0 from a zero row and 1 from every other row, a zero row at 1 from every nonzero query.  The certificate
  needs |f32 nominating distance - this value| <= F32_ERR_* (common.h), the constants mirrored in F32_ERR below;
* the fp16 OPERAND IMAGE (the comment above pack_image_kernel, gemm_rowreg.hip): per 32-row tile 16 KiB; quad (K-step m, lane
  l = 32 h + j) sits at byte 16 (64 m + l) and holds the 8 fp16 values of tile row j, dims 16 m + 8 h .. + 7, each
  fp16(unit row x 2^10); rows at or past the row count are zero rows; bit r of the tile's zero mask <=> tile row r is a zero row.

Tolerance of an image value.  With y = x / |x| * 2^10 in float64 the kernel forms an f32 value first -- 256 squares summed
(relative gamma_256 on a sum of positive terms, halved by the square root), a correctly rounded reciprocal square root, one multiply
by the power of two and one by the component: every f32 component is within gamma_260 of y, RELATIVE, the same derivation as
UNIT_QUERY_COEF in tests/ivf_ref.py -- and rounds it to fp16 once, to nearest: a stored value s is admissible when
    |s - y| <= gamma_260 |y| + ulp16(|y|) / 2,
ulp16 being fp16's spacing at |y|, 2^(e - 10) for 2^e <= |y| < 2^(e + 1) and 2^-24 (gradual underflow) below 2^-14.
"""
import numpy as np

DIM = 256
TILE_ROWS = 32
TILE_BYTES = 16384
ROW_SCALE = 2.0 ** 10          # F16X2_ROW_SCALE (mfma_tile.h)
U32 = 2.0 ** -24               # unit roundoff of f32

# common.h F32_ERR_*: the certificate's bound on |nominating f32 distance - exact distance| per nominating arithmetic
F32_ERR = {"f32": 2e-5, "bf16x3": 7e-5, "f16x2": 5.2e-4, "f16x1": 1.0e-3}

# What the f32 -> fp16 conversion of the image does with results below fp16's smallest normal 2^-14, AS OBSERVED on gfx950 by
# tests/test_gpu_image_tile.py (which fails if the device stops agreeing with this line): False = gradual underflow, the value is
# rounded to a multiple of 2^-24 like any other; True = flushed to zero, and image_value_tolerance widens by exactly |y| there.
IMAGE_FLUSHES_F16_SUBNORMALS = False


def gamma(n, u=U32):
    return n * u / (1.0 - n * u)


# ---------------------------------------------------------------------------------------------- exact distances
def exact_distances(rows, queries):
    """float64 [n_rows][nq]: max(1 - cos, 0); zero query: 0 against a zero row, else 1; zero row against a nonzero query: 1."""
    x = np.asarray(rows, dtype=np.float64).reshape(-1, DIM)
    q = np.asarray(queries, dtype=np.float64).reshape(-1, DIM)
    nx, nq = np.linalg.norm(x, axis=1), np.linalg.norm(q, axis=1)
    zx, zq = ~x.any(axis=1), ~q.any(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = (x / np.where(zx, 1.0, nx)[:, None]) @ (q / np.where(zq, 1.0, nq)[:, None]).T
    d = np.maximum(1.0 - cos, 0.0)
    d[zx, :] = 1.0
    d[:, zq] = 1.0
    d[np.ix_(zx, zq)] = 0.0
    return d


# ---------------------------------------------------------------------------------------------- fp16
def ulp16(a):
    """fp16's spacing at |a| (float64 in, float64 out): 2^(e - 10) in the binade [2^e, 2^(e + 1)), 2^-24 below 2^-14."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    # (log2 of a value just below a power of two may round up to it: settle the binade by comparison)
    e = np.where(2.0 ** e > a, e - 1, e)
    e = np.where(2.0 ** (e + 1) <= a, e + 1, e)
    return 2.0 ** (np.maximum(np.where(a > 0, e, -14.0), -14.0) - 10.0)


def fp16_rne(y):
    """float64 -> the nearest fp16 value (ties to the even significand, gradual underflow, +-inf past 65520), as float64: the rule
    the tolerance above assumes, written from the format's definition -- tests/test_nominate_ref_cpu.py holds it against numpy.float16."""
    y = np.asarray(y, dtype=np.float64)
    u = ulp16(y)
    k = y / u                                   # exact: u is a power of two
    r = np.floor(k)
    frac = k - r
    r = r + ((frac > 0.5) | ((frac == 0.5) & (np.mod(r, 2.0) == 1.0)))
    s = r * u
    return np.where(np.abs(s) >= 65520.0, np.copysign(np.inf, s), s)


def image_value_tolerance(y, flush=None):
    """|stored - y| allowed for the float64 target y = x / |x| * 2^10 (module docstring)."""
    flush = IMAGE_FLUSHES_F16_SUBNORMALS if flush is None else flush
    a = np.abs(np.asarray(y, dtype=np.float64))
    tol = gamma(260) * a + 0.5 * ulp16(a)
    if flush:   # a result below the smallest normal may come out as zero: the whole value is the error
        tol = np.where(a * (1.0 + gamma(260)) < 2.0 ** -14, np.maximum(tol, a), tol)
    return tol


# ---------------------------------------------------------------------------------------------- the image layout
def tile_to_values(tile_bytes):
    """16 KiB of one tile -> float16 [32 tile rows][256 dims]"""
    q = np.frombuffer(bytes(tile_bytes), dtype="<f2")
    assert q.size == TILE_BYTES // 2
    return np.ascontiguousarray(q.reshape(16, 2, TILE_ROWS, 8).transpose(2, 0, 1, 3).reshape(TILE_ROWS, DIM))   # [m][h][j][8] -> [j][m][h][8]


def values_to_tile(values):
    """float16 [32][256] -> the tile's 16 KiB: quad (m, l = 32 h + j) at byte 16 (64 m + l), tile row j, dims 16 m + 8 h .. + 7"""
    v = np.asarray(values, dtype="<f2").reshape(TILE_ROWS, 16, 2, 8)
    return np.ascontiguousarray(v.transpose(1, 2, 0, 3)).tobytes()


def image_targets(rows, tile):
    """What tile `tile` of the image of `rows` (f32 [n][256], n = the row count) must hold: (y float64 [32][256], zero mask).  Rows at
    or past the row count and zero rows: y = 0 and their mask bit set."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, DIM)
    y = np.zeros((TILE_ROWS, DIM), dtype=np.float64)
    mask = 0
    for r in range(TILE_ROWS):
        i = tile * TILE_ROWS + r
        x = rows[i].astype(np.float64) if i < len(rows) else np.zeros(DIM)
        if not x.any():
            mask |= 1 << r
            continue
        # (scaled by the largest magnitude first: the squares of a row at 2^40 or 2^-40 stay far from float64's limits either way)
        s = np.abs(x).max()
        y[r] = (x / s) / np.linalg.norm(x / s) * ROW_SCALE
    return y, mask


def check_image_tile(tile_bytes, zero_mask, rows, tile, flush=None):
    """Every value, mask bit and zero quad of one tile against image_targets; returns a list of messages (empty = the tile is right)."""
    got = tile_to_values(tile_bytes).astype(np.float64)
    y, mask = image_targets(rows, tile)
    bad = []
    if zero_mask != mask:
        bad.append(f"tile {tile}: zero mask {zero_mask:#010x}, expected {mask:#010x}")
    words = np.frombuffer(bytes(tile_bytes), dtype="<u2").reshape(16, 2, TILE_ROWS, 8)   # [m][h][j][8]: -0.0 is not an all-zero word
    for r in range(TILE_ROWS):
        if (mask >> r) & 1 and words[:, :, r, :].any():
            bad.append(f"tile {tile} row {r}: a zero row whose quads are not all-zero words")
    err = np.abs(got - y)
    tol = image_value_tolerance(y, flush)
    over = np.argwhere(~(err <= tol))
    for r, d in over[:8]:
        bad.append(f"tile {tile} row {r} dim {d}: stored {got[r, d]!r}, target {y[r, d]!r}, |diff| {err[r, d]:.3e} > {tol[r, d]:.3e}")
    return bad


# ---------------------------------------------------------------------------------------------- constructed worst-case rows
def bf16_rne(x):
    """f32 -> bf16 (round to nearest even) -> f32, as v_cvt_pk_bf16_f32 does"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def worst_case_rows_f16x2(rng, n_rows):
    """Unit rows whose elements x 2^10 sit EXACTLY on fp16 rounding midpoints, in two binades so that the row has unit norm
    to within 2^-13: the kernel's normalisation then shifts every element off its midpoint in the SAME direction and all
    256 roundings go the same way.  With a query of matching signs the rounding errors add up instead of cancelling:
    |error| = sum |delta_i q_i| -- the situation F32_ERR_F16X2 = 2^-11 (+ accumulation) is the bound for."""
    rows = np.zeros((n_rows, 256), dtype=np.float64)
    for r in range(n_rows):
        i = int(rng.integers(0, 4))
        j = 3 * (2 * i + 1) + (0 if r % 2 else -1)          # (2j + 1) = 6 (2i + 1) -+ 1: the norm is off by ~2^-14 only
        a = 2.0 ** -3 * (1 + (2 * i + 1) * 2.0 ** -11)       # 48 elements just above 2^-3: midpoint of the fp16 grid after x 2^10
        b = 2.0 ** -4 * (1 - (2 * j + 1) * 2.0 ** -12)       # 64 elements just below 2^-4
        pos = rng.permutation(256)
        sign = rng.choice([-1.0, 1.0], size=256)
        rows[r, pos[:48]] = a * sign[pos[:48]]
        rows[r, pos[48:112]] = b * sign[pos[48:112]]
    return rows


def worst_case_rows_bf16x3(rng, n_rows):
    """Unit rows (to within f32 rounding: one free element absorbs the rest of the norm) whose elements carry the bit
    pattern that maximises what bf16 x 3 drops: x = hi + lo + r with lo ~ 2^-8 |x| (the residual just below half a bf16
    ulp, so hi rounds DOWN) and r = 0.75 * 2^-17 |x| of the same sign (lo rounds down too).  With q = x the dropped terms
    lo.lo + 2 r.x are all positive: error ~ 2^-15 |x||q| = 3.1e-5, the worst this scheme can do -- against a bound of 1.5e-4."""
    rows = np.zeros((n_rows, 256), dtype=np.float64)
    frac = 2.0 ** -8 - 2.0 ** -16 + 0.75 * 2.0 ** -17       # bits below the 7 fraction bits of hi
    for r in range(n_rows):
        while True:
            n = 62
            t = rng.integers(0, 3, size=n)                   # the top 7 fraction bits are free: they tune the norm
            mags = 2.0 ** -3 * (1 + t * 2.0 ** -7 + frac)
            rest = 1.0 - float((mags ** 2).sum())
            if 2.0 ** -8 < rest < 2.0 ** -5:
                break
        pos = rng.permutation(256)
        sign = rng.choice([-1.0, 1.0], size=256)
        rows[r, pos[:n]] = mags * sign[pos[:n]]
        rows[r, pos[n]] = np.sqrt(rest) * sign[pos[n]]       # the free element
    return rows
