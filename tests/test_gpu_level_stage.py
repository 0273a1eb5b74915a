"""GPU: K3's LEVEL STAGE -- what lies between "one level launch nominates" (test_gpu_nominations.py) and "the select ranks"
(test_gpu_select.py) -- on constructed inputs against NumPy (tests/level_ref.py):

  * level_tile() in all three kernel families: an arbitrary level launch (smt_debug_level_nominations) nominates, with +inf thresholds,
    exactly the rows of its tile set, once each;
  * the slot minima of the bootstrap launch (smt_debug_bootstrap_minima): bit for bit the minimum of the same family's all-pass
    nominating distances up to 2048 rows, within the family's F32_ERR_* of the float64 minimum beyond;
  * bootstrap_tau_kernel and level_select_kernel on buffers the test fills (smt_debug_bootstrap_tau, smt_debug_level_select);
  * the thresholds a real batched call publishes, read through the trace tap (smt_debug_gemm_trace): never below the k'-th nominating
    distance, never rising, the k' best at the end, an overflow always flagged.

Whole-call answers cannot show most of this: a threshold that is valid but loose, or a tile visited twice, only nominates too much, the
2048-slot buffers overflow, K2 re-answers and the answers stay right.  No tolerance here is new: every band is a F32_ERR_* of common.h
(tests/nominate_ref.F32_ERR), every other comparison is exact.  The plan itself is checked without a GPU (test_level_plan_cpu.py)."""
import functools

import numpy as np
import pytest

import semtools_amd as smt
from oracle import oracle as orc
from tests import level_ref as lref
from tests import nominate_ref as nref
from tests import synth
from tests.nomination_families import FAMILIES, LEVEL, ROWREG, ROWREG_FAMILIES, Family, restore, set_family

pytestmark = pytest.mark.gpu

INF32 = np.float32(np.inf)
F16X2_INV_SCALE = np.float32(1.0 / (1024.0 * 256.0))   # mfma_tile.h


@pytest.fixture(params=list(FAMILIES))
def fam(request, gpu_ctx):
    f = Family(request.param, gpu_ctx)
    set_family(gpu_ctx, f)
    yield f
    restore(gpu_ctx)


@pytest.fixture(params=ROWREG_FAMILIES)
def rfam(request, gpu_ctx):
    f = Family(request.param, gpu_ctx)
    set_family(gpu_ctx, f)
    yield f
    restore(gpu_ctx)


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]).copy()).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


@functools.lru_cache(maxsize=None)
def big_inputs():
    """65 600 i.i.d. unit rows (2050 tiles) with a handful of zero rows near the front, 64 queries of which query 1 is the zero query."""
    rows = synth.unit_rows(65600, seed=4242, dup_frac=0, zero_frac=0).copy()
    rows[[0, 15, 16, 31, 64, 79, 1040, 2040]] = 0.0
    qs = synth.unit_query(97, nq=64).copy()
    qs[1] = 0.0
    rows.setflags(write=False)
    qs.setflags(write=False)
    return rows, qs


def _level_len(stride, skip, n_tiles):
    """Level tiles of (stride, skip) that exist among n_tiles tiles, by counting."""
    n = 0
    while lref.level_tile(n, stride, skip) < n_tiles:
        n += 1
    return n


# ============================================================================================== 2. one arbitrary level on the device
# (stride, skip, tiles); the second group ends ON the corpus' ragged last tile where the first group's tile counts leave it unvisited
LEVELS = [(1, 4, 80), (1, 16, 68), (1, 64, 65), (4, 4, 300), (16, 0, 300), (1, 64, 64), (4, 4, 293), (16, 0, 289)]


@pytest.mark.parametrize("stride,skip,n_tiles", LEVELS, ids=[f"stride{s}-skip{k}-{n}tiles" for s, k, n in LEVELS])
def test_a_level_launch_nominates_exactly_the_rows_of_its_tile_set(fam, stride, skip, n_tiles):
    """+inf thresholds: hits == 1 on the rows of the launch's tiles (tests/level_ref), 0 everywhere else, counts = that many rows.
    The corpus' last tile is ragged, and in every level but (1, 64, 65), (4, 4, 300) and (16, 0, 300) the launch visits it.  The row-register kernel also starts in the middle of the level; the others must refuse that."""
    rows, qs = big_inputs()
    n = n_tiles * 32 - 13
    end = _level_len(stride, skip, n_tiles)
    assert 18 <= end <= 64, (end, n_tiles)                  # at most 2048 rows: the capacity of a candidate list
    visits_last = int(lref.level_tile(end - 1, stride, skip)) == n_tiles - 1
    assert visits_last == ((stride, skip, n_tiles) not in ((1, 64, 65), (4, 4, 300), (16, 0, 300)))
    c = fam.corpus(rows[:n])
    try:
        q = qs[:fam.nq_max]
        nq = len(q)
        for begin in (0, 17):
            if begin and fam.family != ROWREG:
                with pytest.raises(smt._lib.SmtError):
                    fam.run(c, q, level=(stride, skip, begin, end))
                continue
            if begin >= end:
                continue
            dist, hits, counts = fam.run(c, q, level=(stride, skip, begin, end))
            tiles = lref.launch_tiles(stride, skip, begin, end)
            want = np.zeros(n, dtype=bool)
            for t in tiles:
                want[32 * t:32 * t + 32] = True
            where = (fam.name, stride, skip, n_tiles, begin)
            assert np.array_equal(hits, np.repeat(want[:, None], nq, axis=1).astype(np.uint32)), (where, np.argwhere(hits != want[:, None])[:5].tolist())
            assert np.all(counts[:nq] == want.sum()) and np.all(counts[nq:] == 0), (where, counts.tolist(), int(want.sum()))
            assert np.isnan(dist[~want]).all() and not np.isnan(dist[want]).any(), where
        # a level whose last tile does not exist, and a skip level_tile does not implement
        for bad in ((stride, skip, 0, end + 1), (stride, 8, 0, 1), (1, 0, 0, 65)):
            with pytest.raises(smt._lib.SmtError):
                fam.run(c, q, level=bad)
    finally:
        c.close()


def test_a_level_launch_over_the_tables_of_a_filtered_call(fam):
    """Range-filtered: the level's tiles are ENTRIES of the tile table (row-register kernel; an entry = one aligned 32-row tile the
    ranges touch) resp. groups of 8 entries of the chunk table (LDS-row kernel; a chunk = up to 4 consecutive rows of one range)."""
    rows, qs = big_inputs()
    n = 3000
    q = qs[:fam.nq_max]
    nq = len(q)
    c = fam.corpus(rows[:n])
    try:
        if fam.family == LEVEL:          # the level kernel has no filtered form: the call must refuse
            with pytest.raises(smt._lib.SmtError):
                fam.run(c, q, ranges=[(3, 500)], level=(1, 4, 0, 3))
            return
        if fam.family == ROWREG:
            ranges, level = [(5, 1000), (1500, 1501), (1600, 3000)], (2, 4)
            inside = np.zeros(n, dtype=bool)
            for b, e in ranges:
                inside[b:e] = True
            entries = [np.flatnonzero(inside[32 * t:32 * t + 32]) + 32 * t for t in range((n + 31) // 32) if inside[32 * t:32 * t + 32].any()]
        else:
            ranges, level = [(3, 500), (600, 601), (700, 1000)], (1, 4)
            chunks = [np.arange(r0, min(r0 + 4, e)) for b, e in ranges for r0 in range(b, e, 4)]
            entries = [np.concatenate(chunks[i:i + 8]) for i in range(0, len(chunks), 8)]
        end = _level_len(level[0], level[1], len(entries))
        tiles = lref.launch_tiles(level[0], level[1], 0, end)
        want = np.zeros(n, dtype=bool)
        for t in tiles:
            want[entries[t]] = True
        assert 300 <= want.sum() <= 2048 and len(tiles) < len(entries)
        dist, hits, counts = fam.run(c, q, ranges=ranges, level=(level[0], level[1], 0, end))
        assert np.array_equal(hits, np.repeat(want[:, None], nq, axis=1).astype(np.uint32)), (fam.name, np.argwhere(hits != want[:, None])[:5].tolist())
        assert np.all(counts[:nq] == want.sum()) and np.all(counts[nq:] == 0), (fam.name, counts.tolist(), int(want.sum()))
    finally:
        c.close()


# ============================================================================================== 3. the bootstrap level's slot minima
def _assert_padding_columns(tile_min, nq, where):
    # the head launch presets every slot to +inf, the padding queries' columns included; nothing may lower them
    assert np.all(tile_min[:, nq:] == INF32), (where, "padding columns below the head's +inf", np.unique(tile_min[:, nq:]).tolist()[:8])


@pytest.mark.parametrize("n_tiles", [33, 64])
def test_bootstrap_slot_minima_are_the_minima_of_the_all_pass_nominations(rfam, n_tiles):
    """Up to 2048 rows the slot minima are BIT-EQUAL to the minimum, over the valid rows of the slot's tiles, of the family's all-pass
    nominating distances: the accumulators are the same and the distance is monotone in them.  Ragged last tile, zero rows, a zero
    query, 1 / 33 / 64 queries; then a filtered call over the tile table with tiles that hold a single wanted row."""
    rows, qs = big_inputs()
    n = n_tiles * 32 - 7
    c = rfam.corpus(rows[:n])
    try:
        allpass = rfam.run_all(c, qs)
        for nq in (1, 33, 64):
            tile_min, stride = rfam.bootstrap(c, qs[:nq])
            where = (rfam.name, n_tiles, nq)
            assert stride == 1 and tile_min.shape == (n_tiles, (nq + 31) // 32 * 32), (where, stride, tile_min.shape)
            want = lref.slot_minima(allpass[:, :nq], n_tiles, 1)
            a, b = tile_min[:, :nq].view(np.uint32), want.view(np.uint32)
            assert np.array_equal(a, b), (where, int((a != b).sum()), np.argwhere(a != b)[:5].tolist())
            _assert_padding_columns(tile_min, nq, where)
        if n_tiles == 64:
            ranges = [(0, 1), (40, 1100), (1130, 1131), (1200, n)]
            inside = np.zeros(n, dtype=bool)
            for b, e in ranges:
                inside[b:e] = True
            entries = [np.flatnonzero(inside[32 * t:32 * t + 32]) + 32 * t for t in range(n_tiles) if inside[32 * t:32 * t + 32].any()]
            assert len(entries) == 63 and len(entries[0]) == 1 and len(entries[35]) == 1
            nq = 33
            dist, hits, _ = rfam.run(c, qs[:nq], ranges=ranges)
            assert np.array_equal(hits > 0, np.repeat(inside[:, None], nq, axis=1))
            tile_min, stride = rfam.bootstrap(c, qs[:nq], ranges=ranges)
            want = lref.slot_minima(dist, len(entries), 1, tile_rows=entries)
            a, b = tile_min[:, :nq].view(np.uint32), want.view(np.uint32)
            assert stride == 1 and np.array_equal(a, b), (rfam.name, "filtered", int((a != b).sum()), np.argwhere(a != b)[:5].tolist())
            _assert_padding_columns(tile_min, nq, (rfam.name, "filtered"))
    finally:
        c.close()


@pytest.mark.parametrize("n_tiles,want_stride", [(1501, 1), (2050, 2)])
def test_bootstrap_slot_minima_lie_within_the_band_of_the_float64_minima(rfam, n_tiles, want_stride):
    """1501 tiles: slots 0 .. 476 hold two tiles; 2050 tiles: the stride is 2 and slot 0 holds level tiles 0 and 1024.  Every slot is
    within the family's F32_ERR_* of the float64 minimum over the rows that belong to it, and +inf exactly where no tile maps to it."""
    rows, qs = big_inputs()
    n = n_tiles * 32 - 5
    c = rfam.corpus(rows[:n])
    try:
        exact = nref.exact_distances(rows[:n], qs)
        for nq in (4, 64):
            tile_min, stride = rfam.bootstrap(c, qs[:nq])
            where = (rfam.name, n_tiles, nq)
            assert stride == want_stride and tile_min.shape[0] == 1024, (where, stride, tile_min.shape)
            want = lref.slot_minima(exact[:, :nq], n_tiles, stride)
            has = lref.slot_has_tile(n_tiles, stride)
            assert np.all(np.isinf(tile_min[~has, :nq])) and np.all(np.isfinite(tile_min[has, :nq])), where
            err = np.abs(tile_min[has, :nq].astype(np.float64) - want[has])
            print(f"BOOTMIN {rfam.name} {n_tiles} tiles {nq} queries: max |slot - float64 minimum| {err.max():.3e} of {rfam.bound:.1e}")
            assert err.max() <= rfam.bound, (where, float(err.max()))
            _assert_padding_columns(tile_min, nq, where)
    finally:
        c.close()


# ============================================================================================== 4a. bootstrap_tau_kernel
TAU_KINDS = ("random", "one-class", "all-equal", "zeros", "one-ulp", "denormal", "few-finite", "all-inf", "subset-inf")
RQS = np.array([0.0, 1.0, 0.7372914552688599, float(F16X2_INV_SCALE)], dtype=np.float32)


def _tau_values(kind, n_slots, kp, rng):
    """Slot values of one query as float32 (all >= 0)."""
    v = (0.5 + 0.5 * rng.random(n_slots)).astype(np.float32)
    if kind == "one-class":       # the kp smallest all in residue class 5 (as far as the class reaches)
        idx = np.arange(5, n_slots, 32)[:kp]
        v[idx] = (0.01 + 0.001 * np.arange(len(idx))).astype(np.float32)
    elif kind == "all-equal":     # the zero query against rows without a zero row
        v[:] = 1.0
    elif kind == "zeros":         # the kp smallest all 0.0
        v[rng.permutation(n_slots)[:kp]] = 0.0
    elif kind == "one-ulp":       # consecutive bit patterns
        v = (np.uint32(0x3F000000) + rng.permutation(n_slots).astype(np.uint32)).view(np.float32)
    elif kind == "denormal":
        v[rng.permutation(n_slots)[:max(1, n_slots // 2)]] = (1 + rng.permutation(n_slots)[:max(1, n_slots // 2)]).astype(np.uint32).view(np.float32)
    elif kind == "few-finite":    # fewer than kp finite values
        v[:] = np.inf
        v[rng.permutation(n_slots)[:min(n_slots, kp - 1)]] = 0.25
    elif kind == "all-inf":
        v[:] = np.inf
    elif kind == "subset-inf":    # at least kp finite values, but in so few residue classes that 6 of each are fewer than kp
        v[:] = np.inf
        for cls in range((kp - 1) // lref.TAU_KEEP):
            v[5 + cls::32] = (0.25 + 0.001 * np.arange(len(v[5 + cls::32]))).astype(np.float32)
    return v


@pytest.mark.parametrize("kp", [9, 34, 64])
@pytest.mark.parametrize("n_slots", [8, 33, 34, 63, 64, 1023, 1024])
def test_bootstrap_tau_on_constructed_slot_minima(gpu_ctx, kp, n_slots):
    """Per query the published tau is VALID (one of the slot values, at least kp of them at or below it), EXACT whenever no residue
    class mod 32 holds more than 6 of the kp smallest, and otherwise the kp-th smallest of the per-class 6-smallest subsets; +inf for
    kp > n_slots, fewer than kp finite values in the subset, all slots +inf.  qconst[2q] = score_threshold(tau, rq) bit for bit, the
    padding queries' words untouched."""
    import torch

    rng = np.random.default_rng(1000 * kp + n_slots)
    poison = np.float32(-7.5)
    for nq in (1, 2, 3, 31, 32, 33):
        nq_pad = (nq + 31) // 32 * 32
        for rot in (range(len(TAU_KINDS)) if nq <= 3 else (0,)):
            kinds = [TAU_KINDS[(q + rot) % len(TAU_KINDS)] for q in range(nq)]
            tm = np.full((n_slots, nq_pad), 0.125, dtype=np.float32)         # padding columns: small values nobody may publish
            for q in range(nq):
                tm[:, q] = _tau_values(kinds[q], n_slots, kp, rng)
            rq = np.zeros(nq_pad, dtype=np.float32)
            rq[:nq] = RQS[(np.arange(nq) + rot) % len(RQS)]
            qconst = np.stack([np.full(nq_pad, poison), rq], axis=1).astype(np.float32)
            d_tm, d_tau, d_qc = _dev(tm), _dev(np.full(nq_pad, poison, dtype=np.float32)), _dev(qconst)
            torch.cuda.synchronize()
            gpu_ctx.debug_bootstrap_tau(d_tm.data_ptr(), n_slots, nq, nq_pad, kp, d_tau.data_ptr(), d_qc.data_ptr())
            gpu_ctx.synchronize()
            tau, qc = _host(d_tau, np.float32), _host(d_qc, np.float32).reshape(nq_pad, 2)
            assert np.all(tau[nq:] == poison) and np.all(qc[nq:, 0] == poison), ("padding queries written", kp, n_slots, nq)
            assert np.array_equal(qc[:, 1].view(np.uint32), rq.view(np.uint32)), "1/|q| changed"
            for q in range(nq):
                where = (kinds[q], kp, n_slots, nq, q)
                bits = tm[:, q].view(np.uint32)
                got = int(tau[q:q + 1].view(np.uint32)[0])
                exact = lref.kth_smallest_bits(bits, kp)
                if kinds[q] == "subset-inf" and n_slots >= 1023:
                    assert int(np.isfinite(tm[:, q]).sum()) >= kp, (where, "the case needs kp finite slot values")
                if kp > n_slots or kinds[q] in ("few-finite", "all-inf", "subset-inf"):
                    assert got == lref.INF_BITS, where
                else:
                    assert got in set(bits.tolist()) and int((bits <= got).sum()) >= kp, (where, "not a valid threshold", hex(got))
                    assert got >= exact, where
                    if lref.exact_when(bits, kp):
                        assert got == exact, (where, hex(got), hex(exact))
                    if kinds[q] == "one-class" and kp > lref.TAU_KEEP and n_slots >= 32 * kp:
                        assert got > exact, (where, "the adversarial case is not adversarial")
                assert got == lref.bootstrap_tau(bits, kp), (where, hex(got), hex(lref.bootstrap_tau(bits, kp)))
                assert int(qc[q:q + 1, 0].view(np.uint32)[0]) in lref.score_threshold_forms(tau[q], rq[q]), (where, qc[q, 0], rq[q])


# ============================================================================================== 4b. level_select_kernel
def _select_case(n, kp, rng, flavour):
    """One query's buffer: min(n, CAP) distinct candidate keys, garbage behind them."""
    cap = lref.CAND_CAP
    m = min(n, cap)
    rows = rng.permutation(1 << 20)[:m].astype(np.uint64)
    if flavour == "ties":         # few distinct distances: the row decides
        dist = rng.integers(0x3F000000, 0x3F000004, m).astype(np.uint64)
    else:
        dist = rng.integers(0x3E000000, 0x3F800000, m).astype(np.uint64)
    if m >= 4 and flavour == "extremes":
        rows[:4] = [0, 0xFFFFFFFE, 0, 0xFFFFFFFE]
        dist[:4] = [0, 0, lref.INF_BITS, lref.INF_BITS]
    buf = rng.integers(0, 1 << 62, cap).astype(np.uint64)     # garbage, keys below every candidate among it
    buf[m:m + 3] = [0, 1, 2][:max(0, min(3, cap - m))]
    buf[:m] = lref.make_keys(dist, rows)[rng.permutation(m)]
    return buf


@pytest.mark.parametrize("kp", [9, 64])
@pytest.mark.parametrize("nq", [1, 64])
@pytest.mark.parametrize("with_qconst", [False, True])
def test_level_select_on_constructed_candidate_buffers(gpu_ctx, kp, nq, with_qconst):
    """The head holds the kp smallest of the first min(count, 2048) keys, counts = min(n, kp), tau = the distance bits of key kp - 1 or
    +inf when there are fewer (under the +inf a call starts with; under a finite threshold in force never above it), qconst follows
    only when given, overflow is set iff count > 2048 and stays set when it was.  Everything
    behind the head is left as it was."""
    import torch

    ns = [0, 1, kp - 1, kp, kp + 1, 2047, 2048, 2049, 1 << 31]
    rng = np.random.default_rng(77 * kp + nq + int(with_qconst))
    rounds = len(ns) if nq == 1 else 1
    for rnd in range(rounds):
        counts = np.array([ns[(q + rnd) % len(ns)] for q in range(nq)], dtype=np.uint32)
        flavours = [("plain", "ties", "extremes")[(q // len(ns) + rnd) % 3] for q in range(nq)]
        cand = np.stack([_select_case(int(counts[q]), kp, rng, flavours[q]) for q in range(nq)])
        overflow = np.array([(q + rnd) % 5 == 0 for q in range(nq)], dtype=np.uint32)      # some preset: sticky
        rq = RQS[(np.arange(nq) + rnd) % len(RQS)]
        qconst = np.stack([np.full(nq, -7.5, dtype=np.float32), rq], axis=1).astype(np.float32)
        d_c, d_n, d_o = _dev(cand), _dev(counts), _dev(overflow)
        # the threshold in force: +inf as at the head of a call, and for every third query a finite one inside the range of the keys'
        # distances, which the pass may lower and never raise
        tau_in = np.full(nq, lref.INF_BITS, dtype=np.uint32)
        tau_in[(np.arange(nq) + rnd) % 3 == 1] = 0x3F000002
        d_t, d_q = _dev(tau_in), _dev(qconst)
        torch.cuda.synchronize()
        gpu_ctx.debug_level_select(d_c.data_ptr(), d_n.data_ptr(), d_o.data_ptr(), d_t.data_ptr(), nq, kp,
                                   qconst_ptr=d_q.data_ptr() if with_qconst else None)
        gpu_ctx.synchronize()
        g_c, g_n, g_o = _host(d_c, np.uint64).reshape(nq, -1), _host(d_n, np.uint32), _host(d_o, np.uint32)
        g_t, g_q = _host(d_t, np.uint32), _host(d_q, np.float32).reshape(nq, 2)
        for q in range(nq):
            where = (kp, nq, with_qconst, rnd, q, int(counts[q]), flavours[q])
            buf, n_after, tau, ovf = lref.level_select(cand[q], int(counts[q]), kp, int(overflow[q]), int(tau_in[q]))
            assert np.array_equal(g_c[q], buf), (where, np.flatnonzero(g_c[q] != buf)[:5].tolist())
            assert g_n[q] == n_after and g_t[q] == tau and g_o[q] == ovf, (where, int(g_n[q]), hex(int(g_t[q])), int(g_o[q]))
            assert g_q[q, 1].view(np.uint32) == rq[q].view(np.uint32), where
            if with_qconst:
                forms = lref.score_threshold_forms(np.uint32(tau).view(np.float32), rq[q])
                assert int(g_q[q:q + 1, 0].view(np.uint32)[0]) in forms, (where, g_q[q, 0])
            else:
                assert g_q[q, 0] == np.float32(-7.5), where


# ============================================================================================== 5. the thresholds a real call publishes
SHAPES = {
    # name: (rows, tuning keys, family, query counts)
    "1056-rows": (1056, {}, "rowreg-f16x2-image", (1, 33)),
    "2048-rows": (2048, {}, "rowreg-f16x2-image", (1, 33)),
    "16416-rows-appended-levels": (16416, dict(gemm_bootstrap=0), "rowreg-f16x2-image", (1, 33)),
    "65600-rows-strided-bootstrap": (65600, {}, "rowreg-f16x2-image", (1, 33)),
    "65600-rows-split-level": (65600, dict(gemm_blocks=4), "rowreg-bf16x3", (160,)),
}
ROW_KINDS = ("iid", "ascending", "descending", "zero-rows")


@functools.lru_cache(maxsize=2)
def _trace_rows(n, kind):
    qs = synth.unit_query(4711, nq=160).copy()
    rows = synth.unit_rows(n, seed=99, dup_frac=0, zero_frac=0).copy()
    if kind in ("ascending", "descending"):
        order = np.argsort(rows.astype(np.float64) @ qs[0].astype(np.float64), kind="stable")
        rows = rows[order if kind == "ascending" else order[::-1]].copy()
    elif kind == "zero-rows":
        rows[np.random.default_rng(5).random(n) < 0.3] = 0.0
        qs[2] = 0.0
    return np.ascontiguousarray(rows), qs


@pytest.fixture
def own_ctx(gpu_ctx):
    """A context of its own for a test that changes tuning keys the library offers no way to read back: closed afterwards, so that
    nothing it set reaches a later test, whatever the defaults are."""
    ctx = smt.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("kind", ROW_KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_thresholds_a_real_batched_call_publishes(own_ctx, shape, kind):
    """Real calls through smt_search_topk_device with the trace buffer set.  T1 the selects traced are the selects the plan hook gives for
    the call; T2 every published tau >= D_kp, the kp-th smallest nominating distance over all rows (exact from the family's all-pass
    nominations up to 2048 rows, the float64 value minus F32_ERR_* beyond); T3 tau never rises; T4 without an overflow flag the last tau
    IS D_kp (within the band beyond 2048 rows) and the head of the buffer holds the kp smallest keys; T5 a count above 2048 in front of a
    select comes with the overflow flag and a verdict other than PROVED, never on the i.i.d. control, and the host form's answers
    equal the oracle's whatever overflowed."""
    import torch

    n, keys, fam_name, nqs = SHAPES[shape]
    f = Family(fam_name, own_ctx)
    rows, all_qs = _trace_rows(n, kind)
    set_family(own_ctx, f)
    for k, v in keys.items():
        own_ctx.set_tuning(k, v)
    own_ctx.set_tuning("image_use_min_rows", 1)          # one query over a corpus that has its image takes the batched route
    c = f.corpus(rows)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = keys.get("gemm_blocks", 0) or cus
    band = f.bound
    try:
        exact = allpass = None
        if n <= 2048:
            allpass = f.run_all(c, all_qs[:64])
        else:
            exact = nref.exact_distances(rows, all_qs[:max(nqs)])
        for nq in nqs:
            qs = all_qs[:nq]
            for k in (1, 56):
                kp = min(64, k + {"bf16x3": 8, "f16x2": 16, "f16x1": 24}[f.arith])
                plan = smt.Context.debug_gemm_plan((n + 31) // 32, nq, kp, family=0, f16x1=f.arith == "f16x1", blocks=blocks,
                                           gemm_bootstrap=keys.get("gemm_bootstrap", 1), gemm_boot_fine=1, gemm_split_last=2, gemm_qsplit=1)
                n_sel = sum(e["select"] for e in plan)
                words = n_sel * 2 * nq + nq + 2 * nq * kp
                d_trace = _dev(np.zeros(words + 64, dtype=np.uint32))
                qd = torch.from_numpy(qs).cuda()
                o_r = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
                o_d = torch.zeros((nq, k), dtype=torch.float64, device="cuda")
                st = torch.full((nq,), 7, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                own_ctx.debug_gemm_trace(d_trace.data_ptr(), words + 64)
                try:
                    c.search_topk_device(qd.data_ptr(), nq, k, 0, o_r.data_ptr(), o_d.data_ptr(), out_status_ptr=st.data_ptr())
                    own_ctx.synchronize()
                finally:
                    got_sel, got_words = own_ctx.debug_gemm_trace(None)
                where = (shape, kind, nq, k)
                # ---- T1
                assert (got_sel, got_words) == (n_sel, words), (where, "selects / words traced", got_sel, got_words, "planned", n_sel, words, plan)
                if shape.endswith("split-level"):
                    assert n_sel == 3 and plan[1]["tile_end"] == plan[2]["tile_begin"] == 512, plan
                t = _host(d_trace, np.uint32)
                per = t[:n_sel * 2 * nq].reshape(n_sel, 2, nq)
                counts, tau = per[:, 0, :], per[:, 1, :].view(np.float32)
                overflow = t[n_sel * 2 * nq:n_sel * 2 * nq + nq]
                head = t[n_sel * 2 * nq + nq:words].reshape(nq, kp, 2)      # little-endian keys: (row, distance bits)
                head_rows, head_dist = head[:, :, 0].astype(np.int64), head[:, :, 1].view(np.float32)
                status = st.cpu().numpy()
                for q in range(nq):
                    wq = where + (q,)
                    if allpass is not None:
                        order = np.lexsort((np.arange(n), allpass[:, q].view(np.uint32)))
                        d_kp = allpass[order[kp - 1], q]
                        floor = d_kp
                    else:
                        d_kp = np.sort(exact[:, q])[kp - 1]
                        floor = d_kp - band
                    # ---- T2, T3
                    assert np.all(tau[:, q] >= floor), (wq, "a threshold below the k'-th nominating distance", tau[:, q].tolist(), float(d_kp))
                    assert np.all(np.diff(tau[:, q]) <= 0), (wq, "tau rises", tau[:, q].tolist())
                    # ---- T5
                    over = bool(np.any(counts[:, q] > lref.CAND_CAP))
                    if over:
                        assert overflow[q] == 1 and status[q] != 0, (wq, "an overflowed buffer was not flagged", counts[:, q].tolist(), int(status[q]))
                    if kind == "iid":
                        assert not over and overflow[q] == 0, (wq, "the i.i.d. control overflows", counts[:, q].tolist())
                    # ---- T4
                    if overflow[q] == 0:
                        if allpass is not None:
                            assert tau[-1, q] == d_kp, (wq, float(tau[-1, q]), float(d_kp))
                            assert np.array_equal(head_rows[q], order[:kp]), (wq, head_rows[q].tolist(), order[:kp].tolist())
                            assert np.array_equal(head_dist[q].view(np.uint32), allpass[order[:kp], q].view(np.uint32)), wq
                        else:
                            assert abs(float(tau[-1, q]) - d_kp) <= band, (wq, float(tau[-1, q]), float(d_kp))
                            assert len(set(head_rows[q].tolist())) == kp and np.all(np.diff(head[q, :, 1].astype(np.int64)) >= 0), wq
                            assert np.all(np.abs(head_dist[q].astype(np.float64) - exact[head_rows[q], q]) <= band), wq
                            rest = np.ones(n, dtype=bool)
                            rest[head_rows[q]] = False
                            assert exact[rest, q].min() >= float(head_dist[q, -1]) - band, (wq, "a better row is missing from the head")
                # ---- the host form re-answers what overflowed: its answers are the oracle's
                res = c.search(qs, top_k=k)
                for q in (range(nq) if nq <= 33 else range(0, nq, 16)):
                    want = orc.search_documents(rows, [n], qs[q], 0, k, accurate=True)
                    assert res[q][0].tolist() == [r["match_line"] for r in want], (where, q)
    finally:
        own_ctx.debug_gemm_trace(None)
        c.close()
