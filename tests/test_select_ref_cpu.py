"""CPU: the NumPy select the GPU select test compares against (tests/select_ref.py) is right, its cases reach the branches of
final_select_kernel they were built for, and they discriminate.

  * select_ref.select == a brute-force rank count (a key is nominated when fewer than kp keys are smaller; an answer's slot is the
    number of passing rows in front of it by (distance, row)) on every case of up to 1024 keys per query;
  * by select_ref.model_survivors and the cases' shapes: every form of the rank code behind a real pruning bound, the few-keys
    shortcut, one list, both column_tau widths, both register forms with and without an overflow word, both rescoring forms, every
    shape of the column set, ties at tau inside and at the end of the tie group, columns that give no bound, too few keys, and every
    verdict -- the list this file's second test walks through;
  * a restatement of the kernel's algorithm, written below, equals the reference on every case, and with one of four faults built
    in -- a survivor cap of 256, ties at tau cut at the distance bits, a final order that forgets the row, a certificate with >= for
    > -- differs from it on at least one: a kernel with that fault would fail tests/test_gpu_select.py."""
import numpy as np
import pytest

from oracle import oracle_np
from tests import select_ref as sr

NAMES = sr.case_names()
PAD = sr.KEY_PAD
LOW = np.uint64(0xFFFFFFFF)


def _same(got, want):
    return all(np.array_equal(np.ascontiguousarray(g).view(np.uint64) if g.dtype == np.float64 else g,
                              np.ascontiguousarray(w).view(np.uint64) if w.dtype == np.float64 else w) for g, w in zip(got, want))


_DIST = {}


def _exact(name, q, row):
    """cosine_accurate of query q of the named case and a corpus row, computed once."""
    key = (name, q, int(row))
    if key not in _DIST:
        _DIST[key] = oracle_np.cosine_accurate(sr.case(name).queries[q], sr.corpus()[int(row)])
    return _DIST[key]


def _finish(c, q, nominated, n_keys, order_by_row=True, strict=True):
    """Nominated keys (in the order the kernel holds them) -> (rows, dist, count, status) of one query."""
    rows = (nominated & LOW).astype(np.int64)
    d = np.array([_exact(c.name, q, r) for r in rows], dtype=np.float64)
    slot = np.arange(len(rows))
    if c.ws_threshold is not None:
        keep = (1.0 - d) > np.float64(np.float32(c.ws_threshold))
        rows, d, slot = rows[keep], d[keep], slot[keep]
    valid = len(rows)
    # rank by counting pairs, as a kernel would
    before = (d[None, :] < d[:, None]) | ((d[None, :] == d[:, None]) & ((rows[None, :] < rows[:, None]) if order_by_row
                                                                         else (slot[None, :] < slot[:, None])))
    rank = before.sum(axis=1)
    out_r = np.full(c.k_out, PAD, dtype=np.uint64)
    out_d = np.full(c.k_out, np.inf)
    for e in np.nonzero(rank < c.k_out)[0]:
        assert out_r[rank[e]] == PAD, "two rows of one rank"
        out_r[rank[e]], out_d[rank[e]] = np.uint64(rows[e]) + np.uint64(c.row_base), d[e]
    ovf = c.overflow is not None and int(c.overflow[q]) != 0
    status = 0
    if not sr.magnitude_in_domain(c.queries[q]):
        status = 3
    elif c.f32_err > 0 and n_keys >= c.kp:
        floor_out = np.float64(np.array([int(nominated[c.kp - 1]) >> 32], dtype=np.uint32).view(np.float32)[0]) - c.f32_err
        if valid >= c.k_out:
            d_k = d[rank == c.k_out - 1][0]
            uncertain = not (floor_out > d_k if strict else floor_out >= d_k)
        else:
            uncertain = c.ws_threshold is None or (1.0 - floor_out) > np.float64(np.float32(c.ws_threshold))
        status = 2 if ovf else int(uncertain)
    elif ovf:
        status = 2
    return out_r, out_d, min(valid, c.k_out), status


def _brute(name):
    """The reference's contract by rank counts alone."""
    c = sr.case(name)
    out = [[], [], [], []]
    for q in range(c.nq):
        keys = c.lists[q].reshape(-1)
        keys = keys[keys != PAD]
        rank = (keys[None, :] < keys[:, None]).sum(axis=1)
        nominated = np.full(min(c.kp, len(keys)), PAD, dtype=np.uint64)
        nominated[rank[rank < c.kp]] = keys[rank < c.kp]
        for o, v in zip(out, _finish(c, q, nominated, len(keys))):
            o.append(v)
    return np.array(out[0]), np.array(out[1]), np.array(out[2], dtype=np.uint64), np.array(out[3], dtype=np.uint32)


@pytest.mark.parametrize("name", [n for n in NAMES if sr.spec(n)["L"] * sr.spec(n)["kp"] <= 1024])
def test_reference_equals_a_brute_force_rank_count(name):
    assert _same(sr.reference(name), _brute(name)), name


# ------------------------------------------------------------------------------------------------------------------- coverage
def _tau_ties(lists_q):
    """(entries of the deciding column at tau's distance bits, how many of them the column needs) -- for the column that gives
    tau; (0, 0) when no column gives a bound."""
    kp = lists_q.shape[1]
    tau = sr.model_tau(lists_q)
    for j in sr.columns(kp):
        c = -(-kp // j)
        col = lists_q[:, j - 1]
        col = np.sort(col[col != PAD])
        if len(col) >= c and col[c - 1] == tau:
            hi = col >> np.uint64(32)
            return int((hi == tau >> np.uint64(32)).sum()), c - int((hi < tau >> np.uint64(32)).sum())
    return 0, 0


def test_the_cases_reach_every_branch_by_the_model():
    seen = set()
    largest = {}
    for name in NAMES:
        c = sr.case(name)
        s = sr.spec(name)
        L, kp, k_out, M = c.L, c.kp, c.k_out, c.L * c.kp
        assert 1 <= k_out <= kp <= 72 and 1 <= L <= 512 and c.lists.shape == (c.nq, L, kp) and c.queries.shape == (c.nq, 256)
        for q in range(c.nq):
            lq = c.lists[q]
            real = lq[lq != PAD]
            assert len(np.unique(real & LOW)) == len(real) and ((real & LOW) < sr.N_ROWS).all(), name   # distinct rows of the corpus
            assert (lq[:, 1:] >= lq[:, :-1]).all(), name                                                 # ascending, padding last
            S = sr.model_survivors(lq)
            assert S is None or S <= sr.SURV_CAP, (name, S)
            if L == 1:
                seen.add("one_list")
                if len(real) < kp:
                    seen.add("one_list_padded")
                continue
            branch = "pairs" if S <= 96 else "T8" if S <= 128 else "T4" if S <= 256 else "T2" if S <= 512 else "T1"
            seen.add(("few" if M <= sr.FEW_KEYS else "bound", branch))
            if M > sr.FEW_KEYS:
                assert S <= 481, (name, S)                         # the proven worst case of the bound, at k' = 72
                largest[branch] = max(largest.get(branch, 0), S)
                seen.add("tau4" if L <= 256 else "tau8")
                ties, need = _tau_ties(lq)
                if ties > 1:
                    seen.add(("ties", "inside" if need < ties else "end", "tau4" if L <= 256 else "tau8"))
                entries = [(int((lq[:, j - 1] != PAD).sum()), -(-kp // j)) for j in sr.columns(kp)]
                if any(n < need_ for n, need_ in entries):
                    seen.add("no_bound_from_all" if all(n < need_ for n, need_ in entries) else "no_bound_from_some")
            if q == 0 and c.survivors:
                assert c.survivors[0] <= S <= c.survivors[1] and M > sr.FEW_KEYS, (name, S)
            if len(real) < kp:
                seen.add("fewer_than_kp")
            if len(real) < k_out:
                seen.add("fewer_than_k_out")
        seen.add(("kreg", 8 if M <= 8192 else 36, c.overflow is not None))
        seen.update([("M", M), ("kp", kp), ("nq", c.nq), ("L", L)])
        seen.add("staged_rows" if kp > 34 else "product_tables")
        if k_out == kp:
            seen.add("k_out_is_kp")
        if k_out == 1 and kp >= 64:
            seen.add("k_out_1_large_kp")
        if c.gaps:
            seen.add(("gaps", c.nq))
        rows, dist, counts, status = sr.reference(name)
        seen.update(("status", int(v), c.f32_err > 0) for v in status)
        if (dist[:, :-1] == dist[:, 1:])[np.isfinite(dist[:, 1:])].any():
            seen.add("equal_distances")
        if (dist == 0).any():
            seen.add("distance_0")
        if (counts < k_out).any():
            seen.add("short_answer")
        if s["content"] == "planted" and s["opts"]["plant"] == "contradict":
            nom = np.sort(c.lists[0].reshape(-1))[:kp]
            exact = np.array([_exact(name, 0, r) for r in (nom & LOW)])
            assert (np.diff(exact) < 0).all(), name                # key order is the exact order reversed
            seen.add("contradict")
    want = [("bound", "pairs"), ("bound", "T8"), ("bound", "T4"), ("bound", "T2"), ("few", "pairs"), ("few", "T4"), "one_list",
            "one_list_padded", "tau4", "tau8", ("ties", "inside", "tau4"), ("ties", "end", "tau4"), ("ties", "inside", "tau8"),
            "no_bound_from_all", "no_bound_from_some", "fewer_than_kp", "fewer_than_k_out", ("kreg", 8, False), ("kreg", 8, True),
            ("kreg", 36, False), ("kreg", 36, True), ("M", 512), ("M", 513), ("M", 8192), ("M", 8194), ("M", 36864), ("L", 256),
            ("L", 257), ("L", 512), "staged_rows", "product_tables", "k_out_is_kp", "k_out_1_large_kp", ("gaps", 3), ("gaps", 33),
            ("nq", 1), ("nq", 3), ("nq", 33), ("status", 0, True), ("status", 1, True), ("status", 2, True), ("status", 2, False),
            ("status", 3, True), ("status", 0, False), "equal_distances", "distance_0", "short_answer", "contradict"]
    want += [("kp", v) for v in (1, 2, 3, 34, 35, 64, 65, 72)]
    missing = [w for w in want if w not in seen]
    assert not missing, missing
    assert ("bound", "T1") not in seen and ("few", "T1") not in seen      # more than 512 survivors: out of reach (select.hip)
    assert largest["T2"] >= 410 and largest["T4"] >= 130 and largest["T8"] >= 97 and largest["pairs"] >= 90, largest


# ------------------------------------------------------------------------------------------- the kernel's algorithm, and faults
def _column_tau(col, c, cut_at_distance_bits):
    """The c-th smallest entry of a column the kernel's way: the distance bits first, then the row among the entries that share
    them.  None: fewer than c entries."""
    col = col[col != PAD]
    if len(col) < c:
        return None
    hi = col >> np.uint64(32)
    dstar = np.sort(hi)[c - 1]
    need = c - int((hi < dstar).sum())
    tied = np.sort(col[hi == dstar] & LOW)
    if cut_at_distance_bits:
        return dstar << np.uint64(32)
    return dstar << np.uint64(32) | (LOW if len(tied) == need else tied[need - 1])


def _kernel_way(name, fault=None):
    c = sr.case(name)
    out = [[], [], [], []]
    for q in range(c.nq):
        lq = c.lists[q]
        flat = lq.reshape(-1)
        n_keys = int((flat != PAD).sum())
        if c.L == 1:
            best = flat[flat != PAD]                      # the list is the nominated set, as it stands
        else:
            tau = PAD
            if c.L * c.kp > sr.FEW_KEYS:
                for j in sr.columns(c.kp):
                    t = _column_tau(lq[:, j - 1], -(-c.kp // j), fault == "ties_by_distance_bits")
                    tau = tau if t is None else min(tau, t)
            surv = flat[(flat != PAD) & (flat <= tau)][:256 if fault == "cap_256" else sr.SURV_CAP]
            rank = (surv[None, :] < surv[:, None]).sum(axis=1)
            best = np.full(c.kp, PAD, dtype=np.uint64)
            best[rank[rank < c.kp]] = surv[rank < c.kp]
            n_keys = c.kp if best[c.kp - 1] != PAD else int((best != PAD).sum())
            best = best[best != PAD]
        got = _finish(c, q, best, n_keys if c.L > 1 else len(best), order_by_row=fault != "order_by_distance_alone",
                      strict=fault != "certificate_ge")
        for o, v in zip(out, got):
            o.append(v)
    return np.array(out[0]), np.array(out[1]), np.array(out[2], dtype=np.uint64), np.array(out[3], dtype=np.uint32)


def test_the_kernels_algorithm_equals_the_reference_on_every_case():
    wrong = [n for n in NAMES if not _same(_kernel_way(n), sr.reference(n))]
    assert not wrong, wrong


@pytest.mark.parametrize("fault", ["cap_256", "ties_by_distance_bits", "order_by_distance_alone", "certificate_ge"])
def test_a_subtly_wrong_select_fails_some_case(fault):
    caught = [n for n in NAMES if not _same(_kernel_way(n, fault), sr.reference(n))]
    assert caught, "no case tells the select with the fault '%s' from the right one" % fault
    print(fault, "caught by", len(caught), "cases, e.g.", caught[:3])
