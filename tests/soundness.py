"""The one assertion the large-k tests share (tests/test_gpu_largek_adversarial.py, tests/test_gpu_fuzz.py).

Device form: every status word is 0, 1 or 2 (no caller plants an invalid query; tests/test_gpu_largek.py covers status 3) and EVERY list marked PROVED (0) is the oracle's
answer -- same rows, f64 distances bit for bit, padding (2^64 - 1, +inf) behind min(k, n).  No case is skipped, nothing has a tolerance.
Host form: smt_search equals the oracle for every query whatever the device verdict was, byte-equal with largek_sampled = 0."""
import json
import os

import numpy as np

from oracle import oracle as orc

PAD_ROW = np.uint64(2**64 - 1)
VERDICTS = {}   # (family, k, route) -> [proved, uncertain, overflow, invalid]


def oracle_topk(emb, q, k):
    res = orc.search_documents(emb, [len(emb)], q, n_lines=0, top_k=k, accurate=True)
    return [r["match_line"] for r in res], np.array([r["distance"] for r in res], dtype=np.float64)


def device_topk(c, qs, k, with_status=True):
    """smt_search_topk_device[_ex] into outputs prefilled with a sentinel (an unwritten list is seen); returns
    (rows uint64 [nq, k], dist f64 [nq, k], status int32 [nq] or None, non-zero verdicts counted by the context)."""
    import torch

    qd = torch.from_numpy(np.ascontiguousarray(qs, dtype=np.float32).reshape(-1, 256)).to("cuda:0")
    nq = qd.shape[0]
    rows = torch.full((nq, k), -7, dtype=torch.int64, device="cuda:0")
    dist = torch.full((nq, k), -7.0, dtype=torch.float64, device="cuda:0")
    st = torch.full((nq,), 7, dtype=torch.int32, device="cuda:0") if with_status else None
    torch.cuda.synchronize()
    c.ctx.uncertain_count(reset=True)
    c.search_topk_device(qd.data_ptr(), nq, k, 0, rows.data_ptr(), dist.data_ptr(), st.data_ptr() if with_status else None)
    c.ctx.synchronize()
    torch.cuda.synchronize()
    counted = c.ctx.uncertain_count(reset=True)
    return rows.cpu().numpy().view(np.uint64), dist.cpu().numpy(), (st.cpu().numpy() if with_status else None), counted


def host_both(c, qs, **kw):
    """smt_search with and without the sampled route: byte-equal (the _both helper of tests/test_gpu_largek.py)."""
    ctx = c.ctx
    ctx.set_tuning("largek_sampled", 0)
    try:
        old = c.search(qs, **kw)
    finally:
        ctx.set_tuning("largek_sampled", 1)
    new = c.search(qs, **kw)
    assert len(old) == len(new)
    for (r0, d0), (r1, d1) in zip(old, new):
        assert r0.tolist() == r1.tolist() and d0.tobytes() == d1.tobytes()
    return new


def check_list(rows, dist, orows, odist, k, note):
    m = len(orows)
    assert m <= k
    assert rows[:m].tolist() == orows, note
    assert dist[:m].tobytes() == odist.tobytes(), note
    assert (rows[m:] == PAD_ROW).all() and np.isposinf(dist[m:]).all(), note


def assert_sound(c, emb, qs, k, *, route=None, host=True, ref=None, family=None, prepacked=False):
    """c: the Corpus holding `emb`.  route: None, "collect" or "sweep" -- confirmed by the profile counters.  ref: oracle answers
    (rows, dist) per query at some k' >= k, when the caller has them.  Returns the status words."""
    qs = np.ascontiguousarray(qs, dtype=np.float32).reshape(-1, 256)
    nq, n = len(qs), len(emb)
    ctx = c.ctx
    if ref is None:
        ref = [oracle_topk(emb, q, k) for q in qs]
    ref = [(r[:k], d[:k]) for r, d in ref]
    if route is not None:
        ctx.prof_enable(True)
        ctx.prof_reset()
    try:
        rows, dist, st, counted = device_topk(c, qs, k)
        if route is not None:
            n_thr, _ = ctx.prof_read("gemm_thr")
            n_collect, _ = ctx.prof_read("largek_collect")
            n_finish, _ = ctx.prof_read("largek_finish")
    finally:
        if route is not None:
            ctx.prof_enable(False)
    if route == "sweep":
        assert n_thr == 1 and n_collect == 0 and n_finish == 1, (n_thr, n_collect, n_finish)
    elif route == "collect":
        assert n_thr == 0 and n_collect == 1 and n_finish == 1, (n_thr, n_collect, n_finish)
    assert counted == int((st != 0).sum()), (counted, st)
    for i in range(nq):
        note = (family, k, nq, i, int(st[i]))
        assert st[i] in (0, 1, 2), note
        if st[i] == 0:
            check_list(rows[i], dist[i], ref[i][0], ref[i][1], k, note)
        else:   # an unproved list is still a written one
            assert not (rows[i].view(np.int64) == -7).any() and not (dist[i] == -7.0).any(), note
    # without a status pointer the lists are the same bytes (and the context counts the same verdicts)
    rows2, dist2, _, counted2 = device_topk(c, qs, k, with_status=False)
    same = st != 2   # which keys an overflowed buffer kept depends on the order of the atomics
    assert rows2[same].tobytes() == rows[same].tobytes() and dist2[same].tobytes() == dist[same].tobytes(), (family, k, nq)
    assert counted2 == counted, (family, k, nq)
    if host:
        got = host_both(c, qs, top_k=k)
        for i in range(nq):
            note = (family, k, nq, i, "host")
            assert got[i][0].tolist() == ref[i][0], note
            assert got[i][1].tobytes() == ref[i][1].tobytes(), note
    if family is not None:
        rt = route or "any"
        if prepacked:
            rt += "+image"
        v = VERDICTS.setdefault((family, k, rt), [0, 0, 0, 0])
        for s in st:
            v[int(s)] += 1
    return st


def dump_verdicts():
    """SMT_LARGEK_VERDICTS=<path>: the verdicts seen in this run, merged into that JSON file (profiles/largek_adversarial_verdicts.json)."""
    path = os.environ.get("SMT_LARGEK_VERDICTS")
    if not path or not VERDICTS:
        return
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f).get("verdicts", {})
    for (family, k, route), v in sorted(VERDICTS.items()):
        out[f"{family}|k={k}|{route}"] = dict(proved=v[0], uncertain=v[1], overflow=v[2], invalid=v[3])
    with open(path, "w") as f:
        json.dump(dict(note="status words of smt_search_topk_device_ex per family, k and route (tests/test_gpu_largek_adversarial.py)",
                       verdicts=out), f, indent=1, sort_keys=True)
        f.write("\n")
