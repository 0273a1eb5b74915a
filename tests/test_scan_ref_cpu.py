"""tests/scan_ref.py held to account on the CPU: the reference that judges the scan stage's block lists (tests/test_gpu_scan_lists.py)
must itself be right, and must bite.

  * the deal restated from chunk_deal.h is a partition of the scanned rows, and the plan restates plan_scan's grid;
  * the reference lists of every case merge to the answer of oracle.search_documents(accurate=True);
  * every builder meets the conditions it asserts (the cap on unclear borders, the tie cases' exact keys);
  * every subtly wrong scan of scan_ref.WRONG_SCANS -- a Python model that returns lists -- fails its named case, while the right
    model passes every case."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import scan_ref as R
from tests import synth
from tests.threshold_ref import _ranges_layout


@functools.lru_cache(maxsize=None)
def case(name):
    rows = synth.unit_rows(4099, seed=8101, dup_frac=0.0, zero_frac=0.0)
    qs = synth.unit_query(8102, nq=8)
    if name == "ragged-4099":               # 1025 chunks, the last of 3 rows; two blocks of 8 waves
        return R.make_case(name, rows, qs[:3], 10, 2, 512, 4)
    if name == "tiny-7":                    # two chunks, 4 + 3 rows, one block each: lists shorter than k'
        return R.make_case(name, rows[:7], qs[:3], 1, 0, 64, 4)
    if name == "filtered-ragged":           # ranges of 1..9 rows: chunks short by 1, 2, 3 rows, a range ending on the last row
        return R.make_case(name, rows[:2003], qs[:2], 10, 2, 128, 4, ranges=_ranges_layout(2003))
    if name == "unroll2-two-passes":        # five queries at scan_unroll = 2: a pass of four at 8 rows per chunk, one at 2
        return R.make_case(name, rows[:1001], qs[:5], 10, 4, 128, 2)
    if name == "tie-zero-query":
        q = qs[:3].copy()
        q[1] = 0.0
        return R.make_case(name, rows, q, 10, 2, 512, 4, ties=True)
    if name == "tie-planted":
        deal = R.Deal(4099, 2, 8, 4)
        emb, q, near, zeros = R.planted_tie_corpus(deal, 18, seed=8103)
        c = R.make_case(name, emb, np.stack([q, 2 * q, 0.5 * q]), 10, 2, 512, 4, ties=True)
        c.near, c.zeros = near, zeros
        return c
    raise KeyError(name)


CASES = ("ragged-4099", "tiny-7", "filtered-ragged", "unroll2-two-passes", "tie-zero-query", "tie-planted")
NAMED = {"ragged-dropped": "tiny-7", "clamped-reread": "tiny-7", "next-block": "ragged-4099", "ties-rejected": "tie-zero-query",
         "kp-minus-1": "ragged-4099", "pad-wrong-slot": "tiny-7", "wave0-only": "ragged-4099", "off-1e-4": "ragged-4099",
         "guard-touched": "ragged-4099"}


@pytest.mark.parametrize("n,blocks,waves,U", [(1, 1, 1, 4), (7, 2, 1, 4), (33, 3, 2, 2), (1000, 4, 2, 8), (4099, 2, 8, 4), (4099, 256, 8, 4)])
def test_the_deal_is_a_partition_of_the_rows(n, blocks, waves, U):
    rows = R.block_rows(n, blocks, waves, U)
    assert len(rows) == blocks
    assert np.array_equal(np.sort(np.concatenate(rows)), np.arange(n))
    # the kernel's own formula: ticket t of block b is chunk ((t // waves) * blocks + b) * waves + t % waves
    for b in range(blocks):
        mine = []
        for t in range(-(-n // U) + waves):
            c = ((t // waves) * blocks + b) * waves + t % waves
            mine += list(range(c * U, min(c * U + U, n)))
        assert sorted(mine) == rows[b].tolist(), (b, n, blocks, waves, U)


def test_the_filtered_deal_follows_the_chunk_table():
    ranges = _ranges_layout(2003)
    rows = R.block_rows(2003, 2, 2, 4, ranges)
    inside = np.concatenate([np.arange(b, e) for b, e in ranges])
    assert np.array_equal(np.sort(np.concatenate(rows)), inside)
    deal = R.Deal(2003, 2, 2, 4, ranges)
    assert {1, 2, 3, 4} == set(deal.cnt.tolist())              # chunks short by 1, 2 and 3 rows
    assert deal.scanned[-1] == 2002                            # a range ending on the last row


def test_the_plan_restates_plan_scan():
    assert R.planned_blocks(4099, 0, 512, 4, 256) == 129       # 1025 chunks / 8 waves: no idle blocks
    assert R.planned_blocks(1, 0, 512, 4, 256) == 1
    assert R.planned_blocks(7, 0, 64, 4, 256) == 2
    assert R.planned_blocks(2048, 32, 64, 8, 256) == 32
    assert R.planned_blocks(10 ** 6, 0, 512, 4, 256) == 256 and R.planned_blocks(10 ** 6, 600, 512, 4, 256) == 512
    assert R.planned_blocks(2003, 0, 64, 2, 256, ranges=[(0, 9)]) == 3      # filtered: 4-row chunks whatever scan_unroll says
    assert R.passes(7) == [(0, 4, 4), (4, 3, 4)] and R.passes(5) == [(0, 4, 4), (4, 1, 1)] and R.passes(2) == [(0, 2, 2)]
    assert R.kernel_unroll(2, 4) == 8 and R.kernel_unroll(2, 1) == 2 and R.kernel_unroll(4, 2) == 4
    assert R.steal_on(4099, 2, 512, 4, 1) and not R.steal_on(4099, 129, 512, 4, 1) and not R.steal_on(4099, 2, 256, 4, 1)
    assert R.route_word(4, True, 512, 7) == 4 | 0x10 | 512 << 8 | 4 << 20 | 4 << 24
    assert R.kprime(56) == 64 and R.kprime(1) == 9 and R.kprime(24, 16) == 40


@pytest.mark.parametrize("name", CASES)
def test_the_right_model_passes_and_merges_to_the_oracles_answer(name):
    c = case(name)
    keys = R.model_scan(c.d64, c.deals, c.kp)
    rep = R.check_lists(keys, c.d64, c.deals, c.kp, where=name)
    assert (c.ties or rep.ok_cap()) and rep.max_err <= 2.0 ** -23, (rep.unclear, rep.lists, rep.max_err)
    scanned = c.deals[0].scanned
    for q in range(c.nq):
        if not c.qs[q].any():
            continue                                               # (the zero query has no cosine; its lists are pinned below)
        k = min(c.top_k, len(scanned))
        ref = orc.search_documents(c.rows[scanned], [len(scanned)], c.qs[q], n_lines=0, top_k=k, accurate=True)
        rows, dist = R.merged_topk(keys, c.d64, q, k)
        assert rows.tolist() == [int(scanned[r["match_line"]]) for r in ref], (name, q)
        assert np.allclose(dist, [r["distance"] for r in ref], rtol=0, atol=1e-12), (name, q)


def test_the_tie_cases_pin_every_key():
    c = case("tie-zero-query")
    keys = R.model_scan(c.d64, c.deals, c.kp)
    assert np.array_equal(keys[1], R.zero_query_lists(c.deals[1], c.kp))
    assert R.key_rows(keys[1, 1, :3]).tolist() == c.deals[1].rows[1][:3].tolist()
    c = case("tie-planted")
    assert c.d64[np.concatenate(c.near), 0].max() < 0.61 and (c.d64[np.concatenate(c.zeros)] == 1.0).all()
    others = np.setdiff1d(np.arange(c.n), np.concatenate(c.near + c.zeros))
    assert c.d64[others].min() > 1.05
    keys = R.model_scan(c.d64, c.deals, c.kp)
    want, last3 = R.planted_tie_rows(c.near, c.zeros)
    for q in range(c.nq):
        for b in range(c.blocks):
            assert set(R.key_rows(keys[q, b]).tolist()) == want[b]
            assert np.array_equal(keys[q, b, -3:], (R.ONE_BITS << np.uint64(32)) | last3[b].astype(np.uint64))


@pytest.mark.parametrize("wrong", R.WRONG_SCANS)
def test_every_wrong_scan_fails_its_named_case(wrong):
    assert len(R.WRONG_SCANS) >= 8
    c = case(NAMED[wrong])
    keys = R.model_scan(c.d64, c.deals, c.kp, wrong=wrong)
    with pytest.raises(AssertionError):
        R.check_lists(keys, c.d64, c.deals, c.kp, where=wrong)
    if wrong == "ties-rejected":                                   # ... and the planted ties catch it too
        c = case("tie-planted")
        with pytest.raises(AssertionError):
            R.check_lists(R.model_scan(c.d64, c.deals, c.kp, wrong=wrong), c.d64, c.deals, c.kp, where=wrong)


def test_the_union_check_of_a_stolen_deal():
    """STEAL: the rows of a block are dealt at run time, so the lists are judged together -- a right scan under ANOTHER deal passes,
    one that drops the best row of the corpus does not."""
    c = case("ragged-4099")
    other = R.deals_of(c.n, c.blocks, 512, 8, c.nq)                # the same rows dealt differently
    keys = R.model_scan(c.d64, other, c.kp)
    R.check_lists(keys, c.d64, c.deals, c.kp, steal=True)
    with pytest.raises(AssertionError):
        R.check_lists(keys, c.d64, c.deals, c.kp)                  # (as a static deal it is wrong)
    best = int(np.argmin(c.d64[:, 0]))
    hit = np.argwhere(R.key_rows(keys[0]) == best)[0]
    keys[0, hit[0], hit[1]:-1] = keys[0, hit[0], hit[1] + 1:]
    keys[0, hit[0], -1] = R.PAD
    with pytest.raises(AssertionError):
        R.check_lists(keys, c.d64, c.deals, c.kp, steal=True)
