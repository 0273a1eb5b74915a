"""K3's LEVEL STAGE restated in NumPy (no GPU).  TEST INFRASTRUCTURE for tests/test_level_plan_cpu.py and tests/test_gpu_level_stage.py.

The stage is what lies between "one level launch nominates" (tests/test_gpu_nominations.py) and "the select ranks"
(tests/test_gpu_select.py): which tiles a launch visits, the slot minima of the bootstrap launch, the first thresholds
(bootstrap_tau_kernel) and the per-level select (level_select_kernel).  Everything here is written from the COMMENTS of gemm.h and
gemm_topk.hip -- what a level is, what a slot holds, what a threshold has to be -- not from the kernels' instruction order.
"""
import math

import numpy as np

# gemm.h
CAND_CAP = 2048
LEVEL0_MAX_TILES = 32
LEVEL_RATIO_KP_LIMIT = 24
BOOTSTRAP_MAX_TILES = 8192
BOOTSTRAP_SLOTS = 1024
RR_WAVES = 8                       # waves per block of gemm_rowreg_kernel
RR_SLOTS = {False: 4, True: 8}     # query tiles resident in LDS: bf16 x 3 / f16 x 2, and f16 x 1
TAU_KEEP = 6                       # bootstrap_tau_kernel: values each of the 32 lanes of a query keeps
SKIPS = (0, 4, 16, 64)             # the ratios level_tile implements
KEY_PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
INF_BITS = 0x7F800000

ROWREG, LDSROW, LEVEL = 0, 1, 2    # kernel families, as the hooks' route words name them
BOOT, APPENDED = 0, 1              # kind of a planned launch (smt_debug_gemm_plan word 0)


# ---------------------------------------------------------------------------------------------- level tiles
def level_tile(i, stride, skip):
    """Level tile i (from 0) of a level (stride, skip): "the i-th positive integer that is not a multiple of the ratio, times
    stride" (gemm.h) -- i counted from 0 -- and plainly i x stride when nothing is skipped.  Works on ints and on integer arrays."""
    if not skip:
        return i * stride
    # among every `skip` consecutive integers skip - 1 are no multiples: i = (skip - 1) d + r names the (r + 1)-th of block d
    d, r = i // (skip - 1), i % (skip - 1)
    return (d * skip + r + 1) * stride


def launch_tiles(stride, skip, tile_begin, tile_end):
    """The tiles a launch visits: level tiles tile_begin .. tile_end - 1, as an int64 array."""
    return level_tile(np.arange(tile_begin, tile_end, dtype=np.int64), stride, skip)


def non_multiples_brute(ratio, count):
    """The first `count` positive integers that are no multiple of `ratio`, by trying them one after the other."""
    out, u = [], 0
    while len(out) < count:
        u += 1
        if u % ratio:
            out.append(u)
    return out


def count_non_multiples_upto(u, ratio):
    """How many positive integers <= u are no multiple of ratio."""
    return u - u // ratio


# ---------------------------------------------------------------------------------------------- the plan, as documented
def documented_boot_stride(plan_tiles, boot_fine):
    """The bootstrap stride the comments of gemm_topk.hip document: every tile up to 2048 tiles; then every 2nd / 4th / 8th / 16th up to
    4 Ki / 8 Ki / 32 Ki / 128 Ki tiles (gemm_boot_fine = 0: every 16th throughout); beyond that every 64th, times 16 while more than
    BOOTSTRAP_MAX_TILES tiles are left."""
    if plan_tiles <= 2048:
        return 1
    if plan_tiles <= 131072:
        if not boot_fine:
            return 16
        return 2 if plan_tiles <= 4096 else 4 if plan_tiles <= 8192 else 8 if plan_tiles <= 32768 else 16
    s = 64
    while -(-plan_tiles // s) > BOOTSTRAP_MAX_TILES:
        s *= 16
    return s


# ---------------------------------------------------------------------------------------------- bootstrap slot minima
def slot_minima(dist, n_tiles, stride, tile_rows=None):
    """dist [rows][nq]: per (row, query) the value to minimise (NaN = the row does not count).  Level tile i of the bootstrap launch is
    tile i x stride; slot s holds the minimum over the counted rows of the level tiles with i = s mod 1024, +inf where there is none.
    tile_rows: for a filtered call the row indices of each TABLE entry (a list of arrays); default: tile t = rows 32 t .. 32 t + 31.
    Returns [min(level tiles, 1024)][nq] in dist's dtype."""
    n_rows, nq = dist.shape
    level_tiles = -(-n_tiles // stride)
    slots = min(level_tiles, BOOTSTRAP_SLOTS)
    out = np.full((slots, nq), np.inf, dtype=dist.dtype)
    for i in range(level_tiles):
        t = i * stride
        rows = np.arange(32 * t, min(32 * t + 32, n_rows)) if tile_rows is None else tile_rows[t]
        if len(rows):
            with np.errstate(invalid="ignore"):
                out[i % BOOTSTRAP_SLOTS] = np.fmin(out[i % BOOTSTRAP_SLOTS], np.nanmin(dist[rows], axis=0))
    return out


def slot_has_tile(n_tiles, stride):
    level_tiles = -(-n_tiles // stride)
    return np.arange(min(level_tiles, BOOTSTRAP_SLOTS)) < level_tiles


# ---------------------------------------------------------------------------------------------- score_threshold
def _f32(x):
    return np.float32(x)


def fma32(a, b, c):
    """fl32(a x b + c) with ONE rounding, for float32 scalars.  a x b is exact in float64 (48 bits); the float64 sum is rounded once
    more, which can only matter when it lands exactly on a tie between two float32 values: the error term of the sum then says on
    which side the true value lies."""
    p = float(a) * float(b)
    cc = float(c)
    s = p + cc
    if math.isinf(s) or math.isnan(s):
        return _f32(s)
    bb = s - p
    err = (p - (s - bb)) + (cc - bb)          # TwoSum: p + cc = s + err exactly
    f = float(_f32(s))
    if err != 0.0 and s != f:
        other = float(np.nextafter(_f32(f), _f32(np.inf if s > f else -np.inf)))
        if s == (f + other) / 2.0:             # exactly between two neighbouring float32 values: the error term decides
            s = math.nextafter(s, math.inf if err > 0 else -math.inf)
    return _f32(s)


def score_threshold(tau, rq, fused=(True, True)):
    """gemm.h score_threshold in float32: the score a row needs for "distance <= tau".  The source writes
        t = ((1 - tau) - 1.2e-7 tau) / rq;  return t - |t| 2.4e-7
    and leaves to the compiler whether each product and the subtraction after it become ONE fused operation (hipcc contracts by
    default); fused = (first site, second site) says which do.  rq == 0 (zero query): tau itself."""
    tau, rq = _f32(tau), _f32(rq)
    if rq == 0.0:
        return tau
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        one_minus = _f32(1.0) - tau
        if fused[0] and np.isfinite(tau):
            num = fma32(-_f32(1.2e-7), tau, one_minus)
        else:
            num = one_minus - _f32(1.2e-7) * tau
        t = num / rq
        if fused[1] and np.isfinite(t):
            return fma32(-np.abs(t), _f32(2.4e-7), t)
        return t - np.abs(t) * _f32(2.4e-7)


def score_threshold_forms(tau, rq):
    """The bit patterns score_threshold may give: one per way of contracting its two multiply-subtract sites.  The source does not pin
    the contraction, so a build is right when it gives any of them (they differ in the last bit at most, rarely at all)."""
    return {int(np.float32(score_threshold(tau, rq, (a, b))).reshape(1).view(np.uint32)[0]) for a in (False, True) for b in (False, True)}


# ---------------------------------------------------------------------------------------------- bootstrap_tau_kernel
def kth_smallest_bits(values_u32, k):
    """The k-th smallest (from 1) of an array of non-negative f32 bit patterns (they order like the floats), or None when there are
    fewer than k."""
    v = np.sort(np.asarray(values_u32, dtype=np.uint32))
    return int(v[k - 1]) if k <= len(v) else None


def residue_subset(values_u32, keep=TAU_KEEP):
    """What bootstrap_tau_kernel ranks: slot s belongs to residue class s mod 32 (one lane), and each class keeps its `keep`
    smallest values."""
    v = np.asarray(values_u32, dtype=np.uint32)
    return np.concatenate([np.sort(v[l::32])[:keep] for l in range(32)])


def bootstrap_tau(slot_values_u32, kp):
    """The threshold bootstrap_tau_kernel publishes for one query, as bits: the kp-th smallest of the per-class keep-6 subsets of the
    slot values; +inf when there are fewer than kp slots, or fewer than kp finite values in the subset."""
    v = np.asarray(slot_values_u32, dtype=np.uint32)
    if kp > len(v):
        return INF_BITS
    t = kth_smallest_bits(residue_subset(v), kp)
    return INF_BITS if t is None or t >= INF_BITS else t


def exact_when(slot_values_u32, kp):
    """True when no residue class holds more than 6 of the kp smallest slot values (ties at the kp-th counted in): the subset then
    contains them all and the published threshold is the exact kp-th smallest."""
    v = np.asarray(slot_values_u32, dtype=np.uint32)
    if kp > len(v):
        return False
    kth = np.sort(v)[kp - 1]
    return all(int((v[l::32] <= kth).sum()) <= TAU_KEEP for l in range(32))


# ---------------------------------------------------------------------------------------------- level_select_kernel
def make_keys(dist_bits, rows):
    return (np.asarray(dist_bits, dtype=np.uint64) << np.uint64(32)) | np.asarray(rows, dtype=np.uint64)


def level_select(buf, count, kp, overflow_in=0, tau_in=INF_BITS):
    """One query of level_select_kernel.  buf: the query's CAND_CAP keys (uint64), count: its raw nomination count.  The first
    min(count, CAND_CAP) keys are the candidates (distinct, the kernel's precondition); whatever lies behind them is not read.
    Returns (buffer afterwards, count afterwards, tau bits, overflow flag): the head holds the kp smallest keys in order, KEY_PAD
    behind them up to kp when there are fewer; the rest of the buffer is unchanged.  tau = the distance bits of key kp - 1, +inf when
    there are fewer than kp keys -- and never above tau_in, the threshold in force (+inf at the head of a call): a threshold never
    rises."""
    buf = np.array(buf, dtype=np.uint64)
    n = min(int(count), CAND_CAP)
    keys = np.sort(buf[:n])
    assert len(np.unique(keys)) == n, "level_select: the keys of a query must be distinct"
    head = np.full(kp, KEY_PAD, dtype=np.uint64)
    head[:min(n, kp)] = keys[:kp]
    buf[:kp] = head
    tau = min(int(keys[kp - 1] >> np.uint64(32)) if n >= kp else INF_BITS, int(tau_in))
    return buf, min(n, kp), tau, 1 if (count > CAND_CAP or overflow_in) else 0
