"""The CONTENT of the fp16 operand image (pack_image_kernel, gemm_rowreg.hip), tile by tile, against the float64 reference of
tests/nominate_ref.py.  The searches over the image are re-scored in f64, so a wrong rounding, a misplaced quad or a missing zero bit
would only show when a near-tie makes the certificate lie; here every value, every mask bit and every zero quad is read back
(smt_debug_image_tile) and held against the contract: value = fp16(unit row x 2^10) within the derived tolerance, layout
quad (m, l = 32 h + j) at byte 16 (64 m + l), rows at or past the row count packed as zero rows whatever lies behind them."""
import numpy as np
import pytest

from tests import decoys
from tests import nominate_ref as ref
from tests import synth

pytestmark = pytest.mark.gpu

N = 200          # 6 full tiles and a last tile of 8 rows
ZERO_ROWS = (0, 15, 16, 31, 77, 199)
SPIKY, BIG, SMALL = 40, 41, 42


def _rows():
    rng = np.random.default_rng(31)
    rows = synth.unit_rows(N, seed=5, dup_frac=0, zero_frac=0).copy()
    rows[100:120] = (rng.standard_normal((20, 256)) * np.exp(3.0 * rng.standard_normal((20, 256)))).astype(np.float32)
    rows[list(ZERO_ROWS)] = 0.0
    # one dominant component; the others from 2^-12 down to 2^-40 of it, so that x 2^10 they cross fp16's subnormal range
    # (2^-14 .. 2^-24 <=> 2^-24 .. 2^-34 of the norm) with significands that do not sit on the subnormal grid
    spiky = np.zeros(256)
    spiky[0] = 1.0
    spiky[1:] = rng.choice([-1.0, 1.0], 255) * (1.0 + rng.random(255)) * 2.0 ** -np.linspace(12.0, 40.0, 255)
    rows[SPIKY] = spiky.astype(np.float32)
    rows[BIG] = (rows[BIG] / np.abs(rows[BIG]).max() * 0.9 * 2.0 ** 40).astype(np.float32)       # largest magnitude just inside 2^40
    rows[SMALL] = (rows[SMALL] / np.abs(rows[SMALL]).max() * 1.5 * 2.0 ** -40).astype(np.float32)  # ... and just inside 2^-40
    return np.ascontiguousarray(rows, dtype=np.float32)


ROWS = _rows()
ROWS.setflags(write=False)


def _check_all_tiles(c, rows):
    bad = []
    for t in range((len(rows) + 31) // 32):
        blob, zm = c.image_tile(t)
        bad += ref.check_image_tile(blob, zm, rows, t)
    assert not bad, bad[:10]


def test_every_tile_holds_fp16_of_the_unit_rows_times_2_to_the_10(gpu_ctx):
    """Every value of every tile within gamma_260 |y| + ulp16(|y|) / 2 of y = x / |x| x 2^10 (float64); exact mask bits; all-zero
    words for zero rows and for the rows past the end of the ragged last tile; rows at 2^40 and 2^-40 and a row whose small
    components fall into fp16's subnormal range.  What the conversion does there is OBSERVED and must match what
    tests/nominate_ref.py records (IMAGE_FLUSHES_F16_SUBNORMALS), which sets the tolerance and DESIGN.md 5's budget term."""
    import semtools_amd as smt

    c = smt.Corpus(gpu_ctx)
    c.append(ROWS)
    c.prepack(True)
    try:
        # the subnormal range first: targets between 2^-23 and 2^-15 round to a NONZERO fp16 subnormal under gradual underflow
        blob, zm = c.image_tile(SPIKY // 32)
        got = ref.tile_to_values(blob)[SPIKY % 32].astype(np.float64)
        y, _ = ref.image_targets(ROWS, SPIKY // 32)
        y = y[SPIKY % 32]
        sub = (np.abs(y) >= 2.0 ** -23) & (np.abs(y) < 2.0 ** -15)
        assert sub.sum() >= 40, sub.sum()
        flushed, kept = bool(np.all(got[sub] == 0.0)), bool(np.all(got[sub] != 0.0))
        print(f"IMAGESUB subnormal targets {int(sub.sum())}: stored nonzero {int((got[sub] != 0).sum())} -> "
              f"{'flushed to zero' if flushed else 'gradual underflow' if kept else 'MIXED'}")
        assert flushed != kept, "some subnormal results are flushed and some are kept"
        assert flushed == ref.IMAGE_FLUSHES_F16_SUBNORMALS, "tests/nominate_ref.py records the other behaviour: correct it and DESIGN.md 5"
        _check_all_tiles(c, ROWS)
        for r in ZERO_ROWS:
            assert (c.image_tile(r // 32)[1] >> (r % 32)) & 1
        assert c.image_tile(N // 32)[1] >> (N % 32) == (1 << (32 - N % 32)) - 1        # rows 200 .. 223: zero rows (199 is one too)
    finally:
        c.close()


def test_tile_bytes_do_not_change_when_rows_are_scaled_by_powers_of_two(gpu_ctx):
    """x / |x| is scale-free and a power of two changes no significand on the way: the image of 2^j x is the image of x, byte for byte."""
    import semtools_amd as smt

    base = ROWS[:96].copy()
    base[SPIKY] = ROWS[1]                                     # (ordinary rows only: 2^40 x the 2^40 row would leave the domain)
    base[BIG] = ROWS[2]
    base[SMALL] = ROWS[3]
    j = np.array([(-35, -7, -1, 0, 1, 5, 35)[i % 7] for i in range(96)])
    scaled = np.ldexp(base, j[:, None]).astype(np.float32)
    a, b = smt.Corpus(gpu_ctx), smt.Corpus(gpu_ctx)
    try:
        a.append(base)
        b.append(scaled)
        a.prepack(True)
        b.prepack(True)
        for t in range(3):
            assert a.image_tile(t) == b.image_tile(t), t
        _check_all_tiles(b, scaled)
    finally:
        a.close()
        b.close()


def test_the_tile_that_straddles_the_row_count_ignores_what_lies_behind_the_rows(gpu_ctx):
    """include/semtools_hip.h (smt_debug_image_tile): rows at or past the row count are packed as zero rows, whatever lies there.
    Two adopted corpora share their 45 rows and differ in the memory behind them -- finite decoy rows that would win every query
    (tests/decoys.py) -- and an owned corpus is truncated from 45 + 64 rows, image already built, into the middle of tile 1: the
    bytes and the mask of tile 1 are the same in all three, and they are the reference's."""
    import torch
    import semtools_amd as smt

    n = 45
    rows = np.ascontiguousarray(ROWS[32:32 + n])              # (rows 32 .. 76: the spiky row and the two scaled ones are among them)
    behind_a = decoys.finite_decoys(decoys.G)
    behind_b = decoys.finite_decoys(decoys.G, c=decoys.centre(seed=99), phase=2)
    assert not np.array_equal(behind_a, behind_b)
    bufs = [torch.from_numpy(np.concatenate([rows, behind])).cuda() for behind in (behind_a, behind_b)]
    torch.cuda.synchronize()
    adopted = [smt.Corpus(gpu_ctx, device_ptr=buf.data_ptr(), rows=n) for buf in bufs]
    owned = smt.Corpus(gpu_ctx)
    try:
        for c in adopted:
            c.prepack(True)
        owned.append(np.concatenate([rows, behind_a]))
        owned.prepack(True)
        assert owned.image_tile(1)[1] == 0                    # the decoys are rows of the corpus for now: tile 1 is full
        owned.truncate(n)
        tiles = [c.image_tile(1) for c in adopted + [owned]]
        assert tiles[0] == tiles[1] == tiles[2]
        assert tiles[0][1] == 0xFFFFFFFF & ~((1 << (n - 32)) - 1)
        for c in adopted + [owned]:
            _check_all_tiles(c, rows)
    finally:
        for c in adopted + [owned]:
            c.close()


def test_the_image_follows_write_rows_append_truncate_and_compact(gpu_ctx):
    """After every change of the rows the tiles it touched -- all tiles are read -- equal the reference of the NEW rows."""
    import semtools_amd as smt

    rng = np.random.default_rng(8)
    cur = ROWS.copy()
    c = smt.Corpus(gpu_ctx)
    c.append(cur)
    c.prepack(True)
    try:
        _check_all_tiles(c, cur)
        new = synth.unit_rows(5, seed=900, dup_frac=0, zero_frac=0)
        new[2] = 0.0
        c.write_rows(70, new)                                  # inside tile 2, a zero row appears, zero row 77 stays
        cur[70:75] = new
        _check_all_tiles(c, cur)
        c.write_rows(0, ROWS[1:2])                             # a zero row becomes a row: its mask bit must go
        cur[0] = ROWS[1]
        _check_all_tiles(c, cur)
        more = (rng.standard_normal((30, 256)) * 3.0).astype(np.float32)
        c.append(more)                                         # fills the ragged tile 6 and opens tile 7
        cur = np.concatenate([cur, more])
        _check_all_tiles(c, cur)
        c.truncate(100)                                        # into the middle of tile 3
        cur = cur[:100]
        _check_all_tiles(c, cur)
        c.append(more[:3])                                     # rows land where truncated rows were packed
        cur = np.concatenate([cur, more[:3]])
        _check_all_tiles(c, cur)
        c.compact([(0, 10), (50, 103)])                        # rows move down across tile borders
        cur = np.concatenate([cur[0:10], cur[50:103]])
        assert c.rows == len(cur) and np.array_equal(c.read_rows(0, len(cur)), cur)
        _check_all_tiles(c, cur)
    finally:
        c.close()
