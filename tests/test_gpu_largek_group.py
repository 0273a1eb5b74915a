"""GPU: the grouped collect of the large-k route (largek_collect_group_kernel, tuning key largek_group) and the sweep of range-filtered
batches (largek_sweep_filtered), DESIGN 4.5.  One pass for up to four queries must give the BYTES of a pass per query.  The device
form takes no ranges: those cases go through Corpus.search, which re-answers what the route could not prove, so every list must be
the oracle's, and the verdicts are read from the context's counter of non-PROVED lists."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import synth

pytestmark = pytest.mark.gpu

R4 = ((1, 6), (7, 8), (64, 1101), (2000, 4099))   # 3142 rows, chunks of 1 - 4 valid rows
R20 = ((3, 9000), (9002, 20001))
# (rows, ranges, top_k, queries, share of the lists that may be other than PROVED)
CASES = ([(1027, None, 1024, nq, 0.0) for nq in (2, 3, 4)] + [(4099, R4, 1024, nq, 0.0) for nq in (2, 4, 5, 7)] + [(4099, R4, 57, 258, 0.0)] +
         [(20001, None, k, nq, 0.05) for k in (57, 1024) for nq in (2, 3, 4)] + [(20001, R20, k, nq, 0.05) for k in (57, 1024) for nq in (2, 5, 7)])
_REF = {}


@pytest.fixture(scope="module")
def env():
    import torch
    import semtools_amd as smt

    ctx = smt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    ctx.set_tuning("largek_sweep_filtered", 0)
    held = {}
    for n in (1027, 4099, 20001):
        emb = synth.unit_rows(n, seed=n)
        x = torch.from_numpy(emb).to("cuda:0")
        held[n] = (emb, x, smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=n))
    yield ctx, held, synth.unit_query(77, nq=258)
    for _, _, c in held.values():
        c.close()
    ctx.close()


def _oracle(emb, ranges, q, i, k):
    key = (len(emb), ranges, i)
    if key not in _REF:
        sub = np.arange(len(emb)) if ranges is None else np.concatenate([np.arange(b, e) for b, e in ranges])
        res = orc.search_documents(emb[sub], [len(sub)], q, n_lines=0, top_k=1024, accurate=True)
        _REF[key] = (sub[[r["match_line"] for r in res]].astype(np.uint64), np.array([r["distance"] for r in res]))
    return _REF[key][0][:k], _REF[key][1][:k]


def _run(ctx, c, qs, k, ranges, group):
    """(rows [nq][k], f64 distances, status words or None, lists that were not PROVED) at largek_group = group."""
    import torch
    ctx.set_tuning("largek_group", group)
    ctx.uncertain_count(reset=True)
    if ranges is not None:
        res = c.search(qs, top_k=k, ranges=list(ranges))
        return np.stack([r for r, _ in res]), np.stack([d for _, d in res]), None, ctx.uncertain_count(reset=True)
    qd = torch.from_numpy(np.ascontiguousarray(qs)).to("cuda:0")
    rows = torch.empty((len(qs), k), dtype=torch.int64, device="cuda:0")
    dist = torch.empty((len(qs), k), dtype=torch.float64, device="cuda:0")
    st = torch.empty(len(qs), dtype=torch.int32, device="cuda:0")
    c.search_topk_device(qd.data_ptr(), len(qs), k, 0, rows.data_ptr(), dist.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    return rows.cpu().numpy().view(np.uint64), dist.cpu().numpy(), st.cpu().numpy(), ctx.uncertain_count(reset=True)


def _equals_oracle(emb, ranges, qs, k, rows, dist, st):
    for i in range(len(qs)):
        if st is None or st[i] == 0:
            orows, odist = _oracle(emb, ranges, qs[i], i, k)
            assert np.array_equal(rows[i], orows) and dist[i].tobytes() == odist.tobytes(), i


def _counters(ctx, fn):
    ctx.prof_enable(True)
    ctx.prof_reset()
    out = fn()
    r = {name: ctx.prof_read(name)[0] for name in ("largek_group", "largek_collect", "gemm_thr")}
    ctx.prof_enable(False)
    return r, out


@pytest.mark.parametrize("n,ranges,k,nq,slack", CASES)
def test_same_bytes_as_a_pass_per_query(env, n, ranges, k, nq, slack):
    ctx, held, qs = env
    emb, _, c = held[n]
    rows, dist, st, unproved = _run(ctx, c, qs[:nq], k, ranges, 4)
    rows1, dist1, st1, unproved1 = _run(ctx, c, qs[:nq], k, ranges, 1)
    assert rows.tobytes() == rows1.tobytes() and dist.tobytes() == dist1.tobytes() and unproved == unproved1
    assert st is None or st.tobytes() == st1.tobytes()
    assert unproved <= slack * nq, (unproved, nq)
    _equals_oracle(emb, ranges, qs[:nq], k, rows, dist, st)


@pytest.mark.parametrize("ranges,nq,group,want", [(None, 3, 4, 1), (R20, 7, 4, 1), (None, 1, 4, 0), (R20, 1, 4, 0), (None, 3, 1, 0), (R20, 7, 1, 0)])
def test_grouped_rounds_by_the_profile_counters(env, ranges, nq, group, want):
    ctx, held, qs = env
    r, _ = _counters(ctx, lambda: _run(ctx, held[20001][2], qs[:nq], 100, ranges, group))
    assert r["largek_group"] == want and r["largek_collect"] == 1 and r["gemm_thr"] == 0, r


@pytest.mark.parametrize("prepack", [False, True])
def test_filtered_batch_takes_the_sweep(env, prepack):
    ctx, held, qs = env
    emb, _, c = held[20001]
    ctx.set_tuning("largek_sweep_filtered", 9)
    try:
        if prepack:
            c.prepack(True)
        for k in (57, 1024):
            r, (rows, dist, st, unproved) = _counters(ctx, lambda: _run(ctx, c, qs[:13], k, R20, 4))
            assert r["gemm_thr"] == 1 and r["largek_collect"] == 0 and r["largek_group"] == 0, r
            assert unproved <= 0.05 * 13, unproved
            _equals_oracle(emb, R20, qs[:13], k, rows, dist, st)
    finally:
        ctx.set_tuning("largek_sweep_filtered", 0)
        if prepack:
            c.prepack(False)
