"""CPU: the LEVEL PLAN of a batched (K3) call -- which tiles each launch of launch_gemm_topk visits -- as smt_debug_gemm_plan returns it:
the very list launch_gemm_topk walks (gemm_topk.hip gemm_level_plan), a pure host function, so nothing here needs a GPU.

Properties, not a second copy of the plan.  Answers cannot show most of what is checked here: a tile visited by two appended launches, a
level that is too large for its thresholds or a bootstrap slot fed by the wrong tile only NOMINATE too much -- the 2048-slot buffers
overflow, the select flags the query, K2 re-answers it exactly and the answers stay equal to the oracle's.

  P1  the appended launches' tile sets lie below plan_tiles, are pairwise disjoint, and their union is every tile exactly once: the
      precondition of level_select_kernel (distinct keys), and "every row is seen"
  P2  a bootstrap launch exists iff row-register kernel, more than LEVEL0_MAX_TILES tiles and gemm_bootstrap; its tiles are the multiples
      of its stride, at most BOOTSTRAP_MAX_TILES of them, slots = min(tiles, BOOTSTRAP_SLOTS); the stride is the documented one
  P3  without a bootstrap the first launch skips nothing and has at most LEVEL0_MAX_TILES tiles: it is appended WITHOUT a threshold,
      so all of its 32 x 32 rows must fit a candidate list
  P4  every skip is one level_tile implements; a select follows every launch, the first part of a split level included; the two parts of
      a split level adjoin; a level is split exactly under the conditions the comment in gemm_level_plan states
  P5  tests/level_ref.level_tile itself, against a brute-force list of non-multiples

What the properties catch was tried once on a scratch copy of gemm_topk.hip, one change at a time: the last level's skip 4 -> 16 (P1),
`parents` one too large (P1), the 4096-tile border of the bootstrap stride moved to 4095 (P2), the second part of a split level begun one
tile early (P4: the parts no longer adjoin).  Each made its property fail and no other change was needed to see it."""
import functools
import itertools

import numpy as np

import semtools_amd as smt
from tests import level_ref as ref

BORDERS = [1, 31, 32, 33, 34, 64, 513, 2048, 2049, 4096, 4097, 8192, 8193, 32768, 32769, 131072, 131073, 524288, 524289, 8388608, 8388609]
# a few dozen more, log-uniform up to 10^7 (seeded: the sweep is the same on every run)
RANDOM = sorted({int(v) for v in np.exp(np.random.default_rng(20240607).uniform(np.log(40.0), np.log(1e7), 36))})
PLAN_TILES = BORDERS + RANDOM
NQS = (1, 128, 129, 256, 257, 1000)
BLOCKS = (1, 4, 256)
KPS = (ref.LEVEL_RATIO_KP_LIMIT, ref.LEVEL_RATIO_KP_LIMIT + 1)

# the bootstrap stride on each side of every border, as DESIGN.md 4.3 and the comments of gemm_level_plan give it: {tiles: (fine, coarse)}
BOOT_STRIDE = {33: (1, 1), 2048: (1, 1), 2049: (2, 16), 4096: (2, 16), 4097: (4, 16), 8192: (4, 16), 8193: (8, 16), 32768: (8, 16),
               32769: (16, 16), 131072: (16, 16), 131073: (64, 64), 524288: (64, 64), 524289: (1024, 1024), 8388608: (1024, 1024),
               8388609: (16384, 16384)}


def _configs():
    for tiles in PLAN_TILES:
        for family, boot, fine, split, nq, blocks, kp in itertools.product((ref.ROWREG, ref.LDSROW, ref.LEVEL), (0, 1), (0, 1), (0, 1, 2), NQS,
                                                                           BLOCKS, KPS):
            for f16x1 in ((False, True) if family == ref.ROWREG else (False,)):
                yield dict(plan_tiles=tiles, nq=nq, kp=kp, family=family, f16x1=f16x1, blocks=blocks, gemm_bootstrap=boot, gemm_boot_fine=fine,
                           gemm_split_last=split, gemm_qsplit=1)


@functools.lru_cache(maxsize=None)
def _partition_errors(plan_tiles, levels):
    """levels: ((stride, skip, level tiles), ...) of the appended launches, the parts of a split level merged.  Every tile of the call
    must be visited by exactly one of them."""
    seen = np.zeros(plan_tiles, dtype=np.uint8)
    for stride, skip, end in levels:
        tiles = ref.launch_tiles(stride, skip, 0, end)
        if len(tiles) and (tiles[-1] >= plan_tiles or np.any(np.diff(tiles) <= 0)):
            return f"level {(stride, skip, end)} leaves the {plan_tiles} tiles or repeats one (last tile {int(tiles[-1])})"
        seen[tiles] += 1
    if not np.all(seen == 1):
        t = int(np.argmax(seen != 1))
        return f"tile {t} of {plan_tiles} is visited {int(seen[t])} times by {levels}"
    return None


def _check(cfg, plan, bad):
    tiles, nq, kp, blocks = cfg["plan_tiles"], cfg["nq"], cfg["kp"], cfg["blocks"]
    rowreg = cfg["family"] == ref.ROWREG
    nqt = (nq + 31) // 32
    appended = [e for e in plan if e["kind"] == ref.APPENDED]
    boots = [e for e in plan if e["kind"] == ref.BOOT]

    def fail(prop, why):
        bad[prop].append((why, cfg, plan))

    # ---- P4 first (P1 merges the parts of a split level and relies on their adjoining)
    levels, parts = [], []
    for e in appended:
        if e["skip"] not in ref.SKIPS:
            fail("P4", f"skip {e['skip']} is none level_tile implements")
        if e["select"] != 1:
            fail("P4", "an appended launch without a select pass behind it")
        if e["tile_begin"] > e["tile_end"]:
            fail("P4", "a launch that ends before it begins")
        if levels and (levels[-1][0], levels[-1][1]) == (e["stride"], e["skip"]):
            if e["tile_begin"] != levels[-1][2]:
                fail("P4", f"the second part of a split level begins at {e['tile_begin']}, the first ended at {levels[-1][2]}")
            if e["tile_begin"] == 0 or e["tile_begin"] == e["tile_end"]:
                fail("P4", "a split level with an empty part")
            if (e["qsplit"], e["blocks"]) != parts[-1][1:]:
                fail("P4", "the two parts of a level differ in shape")
            levels[-1] = (e["stride"], e["skip"], e["tile_end"])
            parts[-1] = (parts[-1][0] + 1,) + parts[-1][1:]
        else:
            if e["tile_begin"] != 0:
                fail("P4", f"a level that begins at level tile {e['tile_begin']}")
            levels.append((e["stride"], e["skip"], e["tile_end"]))
            parts.append((1, e["qsplit"], e["blocks"]))
        if e["tile_end"] > e["tile_begin"] and not (1 <= e["qsplit"] <= nqt and e["blocks"] >= 1 and e["blocks"] % e["qsplit"] == 0):
            fail("P4", "the shape of a launch: 1 <= qsplit <= query tiles, blocks a multiple of it")
    if any(p[0] > 2 for p in parts):
        fail("P4", "a level in more than two parts")
    # a level is split exactly when: row-register kernel, gemm_split_last set, it runs under thresholds, it is the last level -- or,
    # with gemm_split_last >= 2, the first level behind a bootstrap --, it admits ~16 k' rows per query or more (nothing skipped, or
    # ratio >= 16), the batch streams (more query tiles than stay resident in LDS), and it is long enough: 64 sweeps of the whole grid
    # (12 for the level behind the bootstrap).  Its first part is an eighth (a quarter) of it, rounded up to whole sweeps of the grid.
    sweep = blocks * ref.RR_WAVES
    for i, ((stride, skip, end), (n_parts, _, _)) in enumerate(zip(levels, parts)):
        first_after_boot = cfg["gemm_split_last"] >= 2 and bool(boots) and i == 0
        last = i == len(levels) - 1
        should = (rowreg and cfg["gemm_split_last"] != 0 and (i > 0 or bool(boots)) and (last or first_after_boot) and (skip == 0 or skip >= 16)
                  and nqt > ref.RR_SLOTS[cfg["f16x1"]] and end >= (12 if first_after_boot else 64) * sweep)
        if should != (n_parts == 2):
            fail("P4", f"level {i} {(stride, skip, end)} is in {n_parts} part(s), the stated conditions say {'two' if should else 'one'}")
        elif n_parts == 2:
            first_end = [e for e in appended if (e["stride"], e["skip"]) == (stride, skip)][0]["tile_end"]
            want = -(-(end // (4 if first_after_boot else 8)) // sweep) * sweep
            if first_end != want:
                fail("P4", f"the first part of level {i} ends at {first_end}, an eighth / a quarter in whole sweeps is {want}")

    # ---- P1
    err = _partition_errors(tiles, tuple(levels))
    if err:
        fail("P1", err)

    # ---- P2
    want_boot = rowreg and tiles > ref.LEVEL0_MAX_TILES and cfg["gemm_bootstrap"] != 0
    if len(boots) != (1 if want_boot else 0) or (boots and plan[0]["kind"] != ref.BOOT):
        fail("P2", f"{len(boots)} bootstrap launches, expected {int(want_boot)} at the head of the plan")
    for b in boots:
        n = -(-tiles // b["stride"])
        if (b["skip"], b["tile_begin"], b["tile_end"]) != (0, 0, n):
            fail("P2", f"the bootstrap's tiles are not the {n} multiples of its stride {b['stride']}")
        if n > ref.BOOTSTRAP_MAX_TILES:
            fail("P2", f"{n} bootstrap tiles")
        if b["slots"] != min(n, ref.BOOTSTRAP_SLOTS):
            fail("P2", f"{b['slots']} slots for {n} tiles")
        if b["stride"] != ref.documented_boot_stride(tiles, cfg["gemm_boot_fine"]):
            fail("P2", f"bootstrap stride {b['stride']}, documented {ref.documented_boot_stride(tiles, cfg['gemm_boot_fine'])}")
        if tiles in BOOT_STRIDE and b["stride"] != BOOT_STRIDE[tiles][0 if cfg["gemm_boot_fine"] else 1]:
            fail("P2", f"bootstrap stride {b['stride']} at the border {tiles}")
        if b["select"] != 1 or b["thresholds"]:
            fail("P2", "the bootstrap is followed by bootstrap_tau_kernel and runs under no threshold")
    # the first appended level behind a bootstrap visits every multiple of its stride, the bootstrap's own tiles among them
    if boots and appended and not (appended[0]["skip"] == 0 and boots[0]["stride"] % appended[0]["stride"] == 0):
        fail("P2", "the level behind the bootstrap does not cover the bootstrap's tiles")

    # ---- P3
    if not boots:
        e = appended[0]
        if e["skip"] != 0 or e["tile_begin"] != 0 or e["tile_end"] > ref.LEVEL0_MAX_TILES or e["thresholds"] or parts[0][0] != 1:
            fail("P3", "the first launch of a plan without bootstrap: nothing skipped, at most LEVEL0_MAX_TILES tiles, in one part")
    for i, e in enumerate(appended):
        if e["thresholds"] != (bool(boots) or e is not appended[0]):
            fail("P3", f"appended launch {i}: runs under thresholds = {e['thresholds']}")


@functools.lru_cache(maxsize=None)
def _sweep():
    bad = {p: [] for p in ("P1", "P2", "P3", "P4")}
    n = 0
    for cfg in _configs():
        _check(cfg, smt.Context.debug_gemm_plan(**cfg), bad)
        n += 1
    return n, bad


def _report(prop):
    n, bad = _sweep()
    assert n > 50000
    assert not bad[prop], f"{len(bad[prop])} of {n} plans; the first: {bad[prop][0]}"


def test_p1_every_tile_belongs_to_exactly_one_appended_launch():
    _report("P1")


def test_p2_the_bootstrap_launch_and_its_stride():
    assert set(BOOT_STRIDE) <= set(PLAN_TILES)
    _report("P2")


def test_p3_the_first_launch_without_a_threshold_fits_a_candidate_list():
    _report("P3")


def test_p4_skips_selects_and_split_levels():
    _report("P4")


def test_p4_the_sweep_reaches_split_levels_and_deep_plans():
    """The sweep is worth what it reaches: plans whose last level is split, plans whose first level behind the bootstrap is split,
    bootstrap strides above 64 with skip-16 middle levels, appended-levels plans of four and more levels."""
    seen = set()
    for cfg in _configs():
        if cfg["blocks"] != 4 or cfg["nq"] != 1000 or cfg["kp"] != KPS[0]:
            continue
        plan = smt.Context.debug_gemm_plan(**cfg)
        app = [e for e in plan if e["kind"] == ref.APPENDED]
        if plan[0]["kind"] == ref.BOOT:
            if len(app) >= 2 and (app[0]["stride"], app[0]["skip"]) == (app[1]["stride"], app[1]["skip"]):
                seen.add("first-after-boot split")
            if plan[0]["stride"] > 64 and any(e["skip"] == 16 for e in app):
                seen.add("deep bootstrap plan")
            if app[-1]["skip"] == 4:
                seen.add("ratio-4 last level")
        else:
            if len(app) >= 2 and app[-1]["tile_begin"] > 0:
                seen.add("last level split")
            if len({(e["stride"], e["skip"]) for e in app}) >= 4:
                seen.add("four appended levels")
    assert seen == {"first-after-boot split", "deep bootstrap plan", "ratio-4 last level", "last level split", "four appended levels"}, seen


def test_the_hook_refuses_what_it_cannot_plan():
    from semtools_amd import _lib as L
    import pytest

    for kw in (dict(plan_tiles=0), dict(nq=0), dict(kp=0), dict(kp=65), dict(family=3), dict(blocks=0)):
        with pytest.raises(L.SmtError):
            smt.Context.debug_gemm_plan(**{**dict(plan_tiles=100, nq=8, kp=18), **kw})


# ---------------------------------------------------------------------------------------------- P5: the reference's own level_tile
def test_p5_level_tile_of_the_reference_against_brute_force():
    rng = np.random.default_rng(7)
    for ratio in (4, 16, 64):
        brute = ref.non_multiples_brute(ratio, 5 * ratio + 40)
        for stride in (1, 4, 1024):
            got = [ref.level_tile(i, stride, ratio) for i in range(len(brute))]
            assert got == [u * stride for u in brute], (ratio, stride)
        assert np.array_equal(ref.launch_tiles(3, ratio, 2, 40), 3 * np.array(brute[2:40]))
        for i in (0, ratio - 2, ratio - 1):
            assert ref.level_tile(i, 1, ratio) == brute[i]
        # far out, where no list reaches: u is no multiple of the ratio, and exactly i + 1 non-multiples lie at or below it
        for i in [int(v) for v in rng.integers(0, 2 ** 33, 200)] + [2 ** 33, 2 ** 33 - 1]:
            u = ref.level_tile(i, 1, ratio)
            assert u % ratio != 0 and ref.count_non_multiples_upto(u, ratio) == i + 1, (ratio, i, u)
            assert ref.level_tile(i, 7, ratio) == 7 * u
    assert [ref.level_tile(i, 5, 0) for i in range(4)] == [0, 5, 10, 15]
