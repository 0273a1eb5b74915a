"""scan_wide_kernel keeps ONE sorted list per query and block in LDS, shared by the block's waves behind a lock (csrc/shared_list.h),
instead of one list per wave and a merge behind the row loop.  The block's list is the k' smallest keys of the block's rows whichever
wave met them, so nothing the select reads may change: every series here is compared byte for byte (rows, f64 distances, status
words) with its scan_take = 0 run at the same settings, and the histogram of smt_debug_scan_groups_wide must account for every call.

The cases are chosen for the list, not for the row loop: row counts around one full list, lists that stay partly empty (k' = 9 of
five rows), a full list (k' = 32), every row inserting in all eight lists against nothing inserting after the first k', with one
wave (a lock nobody else wants), four and eight waves of ONE block fighting for each lock, ties at the threshold, and passes that
serve one to eight calls (the tail copies that many lists).  Setup, series runner and references: tests/test_gpu_scan_wide.py."""
import pytest

from tests.test_gpu_scan_pairing import _same
from tests.test_gpu_scan_wide import ADV_SEEDS, CALLS, N_STEEP, S, _accounted, _eight_per_group, _series, _want  # noqa: F401

pytestmark = pytest.mark.gpu

RAGGED = (1, 5, 31, 33, 1000, 65_537)   # one ragged chunk, two chunks, one row less and one more than a full list, one block, several


@pytest.fixture(scope="module")
def SH(S):
    """S with the corpora this file adds (S closes whatever is in S.corpora)."""
    import semtools_amd as smt

    for n in RAGGED:
        if n not in S.corpora:
            S.corpora[n] = smt.Corpus(S.ctx, device_ptr=S.x.data_ptr(), rows=n)
    S.xcalm = S.xsteep.flip(0).contiguous()                        # the mirror image: distances RISE with the row number
    S.torch.cuda.synchronize()
    S.corpora["calm"] = smt.Corpus(S.ctx, device_ptr=S.xcalm.data_ptr(), rows=N_STEEP)
    return S


def _grouped(s, key, names, ks, take=7, full=None, **kw):
    """The series at scan_take = `take` against its scan_take = 0 run; with `full`, repeated (up to six times, every run checked)
    until some pass has served full + 1 calls."""
    want = _want(s, key, names, CALLS, ks, **kw)
    seen = 0
    for _ in range(6):
        got, by_size, counts = _series(s, names, CALLS, ks, take, **kw)
        _same(got, want)
        _accounted(by_size, counts, CALLS, take=take)
        seen += by_size[full] if full is not None else counts[0]
        if seen:
            break
    assert seen > 0, (key, take)
    return want


@pytest.mark.parametrize("k", [1, 10, 24])                          # k' = 9, 18, 32: an empty tail, the headline, a full list
@pytest.mark.parametrize("rows", RAGGED)
def test_ragged_rows(SH, rows, k):
    _grouped(SH, ("uniform", rows, k), (rows,), (k,))


@pytest.mark.parametrize("k", [10, 24])
@pytest.mark.parametrize("threads", [64, 256, 512])                 # one wave: the lock is never contended; four; eight
@pytest.mark.parametrize("blocks", [1, 2])                          # 1: all the waves of one block fight for each lock
@pytest.mark.parametrize("name", ["steep", "calm"])
def test_contention(SH, name, blocks, threads, k):
    """steep: every row a wave reduces is the block's best so far, in all eight lists -- each of them takes its lock.  calm: the
    first k' rows fill the lists and nothing inserts after them.  The references are computed at the same grid."""
    SH.ctx.set_tuning("scan_blocks", blocks)
    SH.ctx.set_tuning("scan_threads", threads)
    try:
        want = _grouped(SH, ("contention", name, blocks, threads, k), (name,), (k,), full=7, qsel=_eight_per_group, queries=SH.qsteep)
    finally:
        SH.ctx.set_tuning("scan_blocks", 0)
        SH.ctx.set_tuning("scan_threads", 512)
    expect = list(range(N_STEEP - 1, N_STEEP - 1 - k, -1)) if name == "steep" else list(range(k))
    for i in range(CALLS):
        assert want[0][i, :k].tolist() == expect, i


def test_ties_at_the_threshold_and_the_zero_query(SH):
    def qsel(i):
        return (i // 3) % 8                                        # the zero query three times, then the duplicated row's three times ...
    want = _grouped(SH, ("dup",), ("dup",), (10,), qsel=qsel)
    assert want[0][6, :3].tolist() == [7, 107, 40_007]             # the three copies of a row, equal distances, in row order


@pytest.mark.parametrize("seed", ADV_SEEDS)
def test_near_ties_in_every_position_of_a_group(SH, seed):
    """40 near-ties around the 10th place (tests/test_gpu_nearties.py), the query in each of the eight places of a group in turn."""
    q_adv = SH.torch.from_numpy(SH.adv[seed][0]).to(SH.qs.device)
    name = ("adv", seed)
    alone = _want(SH, ("adv alone", seed), (name,), 8, (10,), queries=q_adv[None])
    more = 0
    for place in range(8):
        qs = SH.qs[8:16].clone()
        qs[place] = q_adv
        want = _want(SH, ("adv", seed, place), (name,), CALLS, (10,), qsel=_eight_per_group, queries=qs)
        got, by_size, counts = _series(SH, (name,), CALLS, (10,), 7, qsel=_eight_per_group, queries=qs)
        _same(got, want)
        _accounted(by_size, counts, CALLS)
        for i in range(CALLS):
            if _eight_per_group(i) == place:                       # ... and the query's answer is that of the query alone
                assert all(x[i].tobytes() == y[0].tobytes() for x, y in zip(got, alone)), (place, i)
        more += sum(by_size[4:])
    assert more > 0


@pytest.mark.parametrize("take", range(8))
def test_groups_of_one_to_eight(SH, take):
    """A pass that serves n calls writes n lists per block and leaves the others' alone."""
    if take == 0:
        want = _want(SH, ("uniform", 65_537, 10), (65_537,), CALLS, (10,))
        got, by_size, counts = _series(SH, (65_537,), CALLS, (10,), 0)
        _same(got, want)
        assert counts == (0, 0, 0) and by_size == (0,) * 8, (counts, by_size)
    else:
        _grouped(SH, ("uniform", 65_537, 10), (65_537,), (10,), take=take, full=take)
