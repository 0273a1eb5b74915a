"""The NumPy references of tests/nominate_ref.py, checked on the CPU: the image layout round-trips, the fp16 rule the image tolerance
rests on is numpy.float16's, the exact distance obeys the zero-vector rules, and the constructed worst-case rows are what their
docstrings claim (unit rows on rounding midpoints) -- so that a GPU test that fails against them points at the GPU."""
import numpy as np

from tests import nominate_ref as ref


def test_layout_round_trips_a_tile_and_puts_every_quad_where_the_contract_says():
    rng = np.random.default_rng(1)
    vals = rng.standard_normal((32, 256)).astype(np.float16)
    blob = ref.values_to_tile(vals)
    assert len(blob) == ref.TILE_BYTES
    assert np.array_equal(ref.tile_to_values(blob), vals)
    raw = np.frombuffer(blob, dtype="<f2")
    for m, h, j in [(0, 0, 0), (0, 1, 0), (3, 0, 17), (15, 1, 31), (8, 1, 5)]:
        off = 16 * (64 * m + 32 * h + j) // 2                     # quad (m, l = 32 h + j) at byte 16 (64 m + l)
        assert np.array_equal(raw[off:off + 8], vals[j, 16 * m + 8 * h:16 * m + 8 * h + 8]), (m, h, j)
    # a tile made of distinct bit patterns: the two maps are inverse permutations of the 8192 values
    ids = np.arange(8192, dtype=np.uint16).view(np.float16).reshape(32, 256)
    back = np.frombuffer(ref.values_to_tile(ids), dtype="<u2")
    assert sorted(back.tolist()) == list(range(8192))
    assert np.array_equal(ref.tile_to_values(back.tobytes()).view(np.uint16), ids.view(np.uint16))


def test_fp16_rule_is_numpy_float16():
    rng = np.random.default_rng(2)
    # a million values over every binade fp16 has, subnormals and the overflow edge included, both signs
    v = (rng.standard_normal(1_000_000) * 2.0 ** rng.integers(-27, 17, 1_000_000)).astype(np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        want = v.astype(np.float16).astype(np.float64)
    got = ref.fp16_rne(v)
    assert np.array_equal(got, want)
    fin = np.isfinite(want)
    assert np.all(np.abs(want[fin] - v[fin]) <= 0.5 * ref.ulp16(v[fin]))            # the tolerance's rounding term, gamma = 0
    # midpoints between neighbouring fp16 values, normal and subnormal: ties go to the even significand
    bits = rng.integers(0, 0x7BFF, 100_000).astype(np.uint16)
    lo = bits.view(np.float16).astype(np.float64)
    hi = (bits + 1).astype(np.uint16).view(np.float16).astype(np.float64)
    mid = 0.5 * (lo + hi)
    even = np.where(bits % 2 == 0, lo, hi)
    for sign in (1.0, -1.0):
        assert np.array_equal(ref.fp16_rne(sign * mid), sign * even)
        assert np.array_equal((sign * mid).astype(np.float16).astype(np.float64), sign * even)
    assert np.array_equal(hi - lo, ref.ulp16(lo))                                    # the spacing, subnormals included
    # at a midpoint both neighbours are admissible and nothing further away is
    tol = ref.image_value_tolerance(mid, flush=False)
    assert np.all(np.abs(lo - mid) <= tol) and np.all(np.abs(hi - mid) <= tol)
    assert np.all(np.abs(hi + (hi - lo) - mid) > tol)
    # the flushing variant widens by exactly the subnormal range
    y = np.array([2.0 ** -15, 2.0 ** -14 * (1 - 2.0 ** -10), 2.0 ** -14, 3.0])
    assert np.array_equal(ref.image_value_tolerance(y, flush=True) >= y, [True, True, False, False])


def test_exact_distance_and_image_targets_obey_the_zero_rules():
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((40, 256)).astype(np.float32)
    rows[[0, 15, 33]] = 0.0
    rows[5] *= np.float32(2.0 ** 40)
    rows[6] *= np.float32(2.0 ** -40)
    qs = rng.standard_normal((3, 256)).astype(np.float32)
    qs[1] = 0.0
    d = ref.exact_distances(rows, qs)
    assert d.shape == (40, 3) and np.all(d >= 0)
    assert np.all(d[[0, 15, 33], 1] == 0.0) and np.all(np.delete(d[:, 1], [0, 15, 33]) == 1.0)
    assert np.all(d[[0, 15, 33], 0] == 1.0) and np.all(d[[0, 15, 33], 2] == 1.0)
    cos = float(rows[7].astype(np.float64) @ qs[0].astype(np.float64)) / (np.linalg.norm(rows[7].astype(np.float64)) * np.linalg.norm(qs[0].astype(np.float64)))
    assert abs(d[7, 0] - (1.0 - cos)) < 1e-15
    y0, m0 = ref.image_targets(rows, 0)
    y1, m1 = ref.image_targets(rows, 1)
    assert m0 == (1 << 0) | (1 << 15) and m1 == (1 << 1) | (0xFFFFFFFF & ~0xFF)       # rows 40.. of tile 1 do not exist: zero rows
    assert np.allclose(np.linalg.norm(y0[[5, 6, 7]], axis=1), 1024.0, rtol=1e-14)      # scale-free, 2^40 and 2^-40 included
    assert not y1[8:].any()
    assert ref.check_image_tile(ref.values_to_tile(ref.fp16_rne(y0).astype(np.float16)), m0, rows, 0) == []
    wrong = ref.fp16_rne(y0).astype(np.float16)
    wrong[7, 100] = np.nextafter(wrong[7, 100], np.float16(np.inf))                     # one ulp off: caught
    assert len(ref.check_image_tile(ref.values_to_tile(wrong), m0, rows, 0)) == 1
    trunc = (np.trunc(y0 / ref.ulp16(y0)) * ref.ulp16(y0)).astype(np.float16)           # a truncating conversion: caught
    assert ref.check_image_tile(ref.values_to_tile(trunc), m0, rows, 0)


def test_worst_case_generators_produce_unit_rows_on_rounding_midpoints():
    rng = np.random.default_rng(4)
    r16 = ref.worst_case_rows_f16x2(rng, 64)
    assert np.array_equal(r16.astype(np.float32).astype(np.float64), r16)               # exact in f32: the device sees these very rows
    # unit to within 2^-13: normalising moves every element off its midpoint by that much, relative -- a small fraction of the
    # 2^-11 half-spacing, so all of a row's roundings go the same way and none reaches another grid point
    norms = np.linalg.norm(r16, axis=1)
    assert np.all(np.abs(norms - 1.0) <= 2.0 ** -13) and np.all(norms != 1.0)
    nz = r16 != 0
    assert np.all(nz.sum(axis=1) == 112)
    y = np.abs(r16[nz]) * ref.ROW_SCALE
    k = y / ref.ulp16(y)
    assert np.all(k - np.floor(k) == 0.5)                                                # every element x 2^10 is an fp16 midpoint
    rbf = ref.worst_case_rows_bf16x3(rng, 64)
    assert np.all(np.abs(np.linalg.norm(rbf.astype(np.float32).astype(np.float64), axis=1) - 1.0) <= 2.0 ** -22)   # unit as the device sees them
    frac = 2.0 ** -8 - 2.0 ** -16 + 0.75 * 2.0 ** -17
    constructed = 2.0 ** -3 * (1 + np.arange(3) * 2.0 ** -7 + frac)
    for row in rbf:
        a = np.abs(row[row != 0])
        assert a.size == 63
        built = a[np.isin(a, constructed)]                                               # all but the free element
        assert built.size == 62
        assert np.array_equal(built.astype(np.float32).astype(np.float64), built)        # exact in f32
        hi = ref.bf16_rne(built.astype(np.float32)).astype(np.float64)
        lo = ref.bf16_rne((built - hi).astype(np.float32)).astype(np.float64)
        r = built - hi - lo
        assert np.all(hi < built) and np.all(lo < built - hi)                            # both parts round DOWN
        assert np.all(r > 0.7 * 2.0 ** -17 * built)                                      # and what bf16 x 3 drops is ~ 0.75 x 2^-17 |x|
