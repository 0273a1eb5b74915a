"""Every K2 instantiation the scan launcher can choose, against the CPU oracle.

The tuning keys scan_unroll (2, 4, 8) and scan_nontemporal (0, 1) select scan_topk_kernel instantiations that no other test
reaches: the suite runs at the defaults (4, 1).  Here every pair of them answers one to seven queries (passes of 1, 2, 3, 4, 4 + 1
and 4 + 3 queries) over corpora of 1, 5, 67 and 1031 rows, unfiltered and through a range filter, at top_k 3 and 56, on a grid of
two blocks of two waves: 1031 rows are 32 full rounds of the largest deal (2 blocks x 2 waves x 8 rows) plus a tail that is ragged
for 2, 4 and 8 rows per chunk; 1 and 5 rows leave whole waves without a chunk.  Rows must equal the oracle's and distances must be
the same bytes.  gemm_min_nq = 8 keeps five and seven queries on the scan kernels.

The one-query cases run at the context's async_select and at async_select = 0.  The default is 0 today, so the two are the same
run until it changes; the host form synchronises either way.  What reaches the one-query pipelines is the second test: the device
entry point with async_select = 1, over the two-stream pipeline and the flag pipeline (scan_overlap 1 and 0), where the launcher
picks the kernel in the same place.

Every instantiation computes the same answer, so neither test can tell WHICH one ran: they show that each one the launcher can
reach is right, and the counts of instantiations are pinned by tests/test_kernel_resources_groups.py."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import synth

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 67, 1031)
NQS = (1, 2, 3, 4, 5, 7)
TOP_KS = (3, 56)
RANGES = [(0, 1), (3, 10), (500, 1031)]
TUNING = {"gemm_min_nq": (8, 5), "scan_blocks": (2, 0), "scan_threads": (128, 512)}   # key: (here, default)


class _Setup:
    pass


@pytest.fixture(scope="module")
def S(gpu_ctx):
    import semtools_amd as smt

    s = _Setup()
    s.ctx = gpu_ctx
    s.qs = synth.unit_query(41, nq=max(NQS))
    s.emb = {n: synth.unit_rows(n, seed=200 + n) for n in ROWS}
    s.corpora = {}
    for n in ROWS:
        s.corpora[n] = smt.Corpus(gpu_ctx)
        s.corpora[n].append(s.emb[n])
    s.idx = np.concatenate([np.arange(b, e) for b, e in RANGES])
    # the oracle's answers, computed once: (rows or "filtered", query, top_k) -> (rows, distances)
    s.want = {}
    for key, emb, back in [(n, s.emb[n], None) for n in ROWS] + [("filtered", s.emb[1031][s.idx], s.idx)]:
        for qi in range(max(NQS)):
            for k in TOP_KS:
                res = orc.search_documents(emb, [len(emb)], s.qs[qi], n_lines=0, top_k=k, accurate=True)
                rows = np.array([r["match_line"] for r in res], dtype=np.int64)
                s.want[(key, qi, k)] = ((rows if back is None else back[rows]).tolist(), np.array([r["distance"] for r in res]))
    yield s
    for c in s.corpora.values():
        c.close()


def _check(s, key, got, k, what):
    for qi, (rows, dist) in enumerate(got):
        wrows, wdist = s.want[(key, qi, k)]
        assert rows.tolist() == wrows, (what, key, k, qi)
        assert np.array_equal(dist, wdist), (what, key, k, qi)


@pytest.mark.parametrize("nontemporal", [0, 1])
@pytest.mark.parametrize("unroll", [2, 4, 8])
def test_every_scan_instantiation_matches_the_oracle(S, unroll, nontemporal):
    ctx = S.ctx
    try:
        for key, (here, _) in TUNING.items():
            ctx.set_tuning(key, here)
        ctx.set_tuning("scan_unroll", unroll)
        ctx.set_tuning("scan_nontemporal", nontemporal)
        for nq in NQS:
            for async_select in ((None, 0) if nq == 1 else (None,)):   # (None: the context's default)
                if async_select is not None:
                    ctx.set_tuning("async_select", async_select)
                for k in TOP_KS:
                    for n in ROWS:
                        _check(S, n, S.corpora[n].search(S.qs[:nq], top_k=k), k, (unroll, nontemporal, nq, async_select))
                    got = S.corpora[1031].search(S.qs[:nq], top_k=k, ranges=RANGES)
                    _check(S, "filtered", got, k, (unroll, nontemporal, nq, async_select))
    finally:
        for key, (_, default) in TUNING.items():
            ctx.set_tuning(key, default)
        ctx.set_tuning("scan_unroll", 4)
        ctx.set_tuning("scan_nontemporal", 1)
        ctx.set_tuning("async_select", 0)


@pytest.mark.parametrize("nontemporal", [0, 1])
@pytest.mark.parametrize("unroll", [2, 4, 8])
def test_one_query_pipelines_run_the_same_instantiations(S, unroll, nontemporal):
    """The device entry point with async_select = 1: the two-stream pipeline (scan_overlap = 1) and the flag pipeline (0)."""
    import torch
    import semtools_amd as smt

    ctx = S.ctx
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(S.qs).to(dev)
    calls = 6
    try:
        for key, (here, _) in TUNING.items():
            ctx.set_tuning(key, here)
        ctx.set_tuning("scan_unroll", unroll)
        ctx.set_tuning("scan_nontemporal", nontemporal)
        ctx.set_tuning("async_select", 1)
        for overlap in (1, 0):
            ctx.set_tuning("scan_overlap", overlap)
            for n in (5, 1031):
                x = torch.from_numpy(S.emb[n]).to(dev)
                for k in (3, 56) if n == 1031 else (3,):          # (this entry point answers top_k <= rows)
                    rows = torch.full((calls, k), -7, dtype=torch.int64, device=dev)
                    dist = torch.full((calls, k), -7.0, dtype=torch.float64, device=dev)
                    torch.cuda.synchronize()
                    c = smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=n)
                    for i in range(calls):
                        c.search_topk_device(qd[i].data_ptr(), 1, k, 0, rows[i].data_ptr(), dist[i].data_ptr())
                    ctx.synchronize()
                    c.close()
                    got = [(rows[i].cpu().numpy(), dist[i].cpu().numpy()) for i in range(calls)]
                    _check(S, n, got, k, (unroll, nontemporal, overlap))
    finally:
        for key, (_, default) in TUNING.items():
            ctx.set_tuning(key, default)
        ctx.set_tuning("scan_unroll", 4)
        ctx.set_tuning("scan_nontemporal", 1)
        ctx.set_tuning("scan_overlap", 1)
        ctx.set_tuning("async_select", 0)
