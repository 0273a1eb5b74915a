"""A NumPy reference of the select stage (csrc/select.hip final_select_kernel), a model of how many keys survive its pruning bound,
and the constructed block lists the select tests feed the kernel.  NumPy only: nothing here imports the library.  The reference is a
plain sort of all keys followed by oracle_np.cosine_accurate and a lexsort; it shares no code with the kernel's algorithm (column
bounds, compaction, counting ranks).  tests/test_select_ref_cpu.py holds it against a brute-force rank count, checks by the survivor
model that the cases reach every branch they were built for, and shows that they tell four subtly wrong selects from the right one.

A key is (f32 distance bits << 32) | row; a query's lists are [n_lists][kp] keys, every list ascending with KEY_PAD at its tail, the
real keys of a query naming distinct rows.  The keys' distance bits are whatever a case wants them to be: the select's answer depends
on them only through which kp keys are the smallest and through the certificate's floor."""
import zlib

import numpy as np

from oracle import oracle_np

KEY_PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
F32_ERR_SCAN, F32_ERR_F16X1 = 4e-6, 1.0e-3                  # csrc/common.h
DOMAIN_MIN, DOMAIN_MAX = np.float32(2.0 ** -40), np.float32(2.0 ** 40)   # csrc/common.h magnitude_in_domain; tests/test_gpu_domain.py
FEW_KEYS, SURV_CAP = 512, 1024                              # select.hip SEL_FEW_KEYS, SEL_SURV_CAP
N_ROWS, DIM = 40000, 256
ZERO_ROWS = (7, 20000, N_ROWS - 1)
DUP_FIRST, DUP_COUNT = 1000, 72                             # rows DUP_FIRST .. DUP_FIRST + 71 are one vector

_CORPUS = None


def corpus():
    """The [N_ROWS][256] f32 rows behind every case's keys: random rows, three zero rows, 72 copies of one row.  Read-only."""
    global _CORPUS
    if _CORPUS is None:
        c = np.random.default_rng(20261020).standard_normal((N_ROWS, DIM), dtype=np.float32)
        c[list(ZERO_ROWS)] = 0.0
        c[DUP_FIRST:DUP_FIRST + DUP_COUNT] = c[DUP_FIRST]
        c.setflags(write=False)
        _CORPUS = c
    return _CORPUS


# ------------------------------------------------------------------------------------------------------------------- the reference
def magnitude_in_domain(q):
    """The library answers for a query whose largest magnitude is 0 or lies in [2^-40, 2^40]; NaN and infinity lie outside."""
    m = np.max(np.abs(np.asarray(q, dtype=np.float32)))
    return bool(m == 0 or (m >= DOMAIN_MIN and m <= DOMAIN_MAX))   # (NaN compares false)


def select(rows_f32, queries, lists, k_out, ws_threshold=None, row_base=0, f32_err=0.0, overflow=None):
    """lists [nq][n_lists][kp] -> (rows uint64 [nq][k_out], dist float64 [nq][k_out], counts uint64 [nq], status uint32 [nq])."""
    lists = np.asarray(lists, dtype=np.uint64)
    nq, _, kp = lists.shape
    out_r = np.full((nq, k_out), KEY_PAD, dtype=np.uint64)
    out_d = np.full((nq, k_out), np.inf, dtype=np.float64)
    counts = np.zeros(nq, dtype=np.uint64)
    status = np.zeros(nq, dtype=np.uint32)
    thr = None if ws_threshold is None else np.float64(np.float32(ws_threshold))
    for q in range(nq):
        keys = lists[q].reshape(-1)
        keys = np.sort(keys[keys != KEY_PAD])
        nominated = keys[:kp]
        r = (nominated & np.uint64(0xFFFFFFFF)).astype(np.int64)
        d = np.array([oracle_np.cosine_accurate(queries[q], rows_f32[i]) for i in r], dtype=np.float64)
        if thr is not None:
            keep = (1.0 - d) > thr
            r, d = r[keep], d[keep]
        order = np.lexsort((r, d))
        r, d = r[order], d[order]
        valid = len(r)
        n = min(valid, k_out)
        out_r[q, :n] = r[:n].astype(np.uint64) + np.uint64(row_base)
        out_d[q, :n] = d[:n]
        counts[q] = n
        ovf = overflow is not None and int(overflow[q]) != 0
        if not magnitude_in_domain(queries[q]):
            status[q] = 3
        elif f32_err > 0 and len(keys) >= kp:
            floor_out = np.float64(np.array([int(nominated[kp - 1]) >> 32], dtype=np.uint32).view(np.float32)[0]) - np.float64(f32_err)
            if valid >= k_out:
                uncertain = not (floor_out > d[k_out - 1])
            else:
                uncertain = True if thr is None else bool((1.0 - floor_out) > thr)
            status[q] = 2 if ovf else (1 if uncertain else 0)
        elif ovf:
            status[q] = 2
    return out_r, out_d, counts, status


# ------------------------------------------------------------------------------------------------ a model of the survivor count
def columns(kp):
    """The columns (1-based) whose entries bound the kp-th smallest key: 1, 2, 4, .. below kp, and kp."""
    cols, j = [], 1
    while j < kp:
        cols.append(j)
        j *= 2
    return cols + [kp]


def model_tau(lists_q):
    """min over the columns j of the ceil(kp / j)-th smallest j-th entry; a column with fewer real entries gives no bound (KEY_PAD
    when no column gives one)."""
    lists_q = np.asarray(lists_q, dtype=np.uint64)
    kp = lists_q.shape[1]
    tau = KEY_PAD
    for j in columns(kp):
        c = -(-kp // j)
        col = lists_q[:, j - 1]
        col = np.sort(col[col != KEY_PAD])
        if len(col) >= c:
            tau = min(tau, col[c - 1])
    return tau


def model_survivors(lists_q):
    """How many keys of one query's lists [n_lists][kp] the kernel ranks: every real key up to 512 keys in all, the keys <= tau
    above that.  None for one list (nothing is ranked).  Only ever a witness that a case reaches a branch, never an answer."""
    lists_q = np.asarray(lists_q, dtype=np.uint64)
    L, kp = lists_q.shape
    if L == 1:
        return None
    real = lists_q[lists_q != KEY_PAD]
    if L * kp <= FEW_KEYS:
        return int(len(real))
    return int((real <= model_tau(lists_q)).sum())


# ------------------------------------------------------------------------------------------------------------------- case contents
def _key(d32, rows):
    d32 = np.ascontiguousarray(d32, dtype=np.float32)
    assert (d32 >= 0).all()                                    # (bit order is value order for these)
    return (d32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(rows, dtype=np.uint64)


def _d32(q, rows):
    """A plausible f32 distance of each row: the f64 cosine distance by a matrix product, rounded to f32, clamped at 0."""
    x = corpus()[rows].astype(np.float64)
    qd = np.asarray(q, dtype=np.float64)
    den = np.sqrt((x * x).sum(axis=1)) * np.sqrt((qd * qd).sum())
    d = np.where(den > 0, 1.0 - (x @ qd) / np.where(den > 0, den, 1.0), 1.0)
    return np.maximum(d, 0.0).astype(np.float32)


def _lay(L, kp, keys, owner):
    """[L][kp]: list l holds keys[owner == l] ascending, KEY_PAD behind them."""
    out = np.full((L, kp), KEY_PAD, dtype=np.uint64)
    for l in range(L):
        mine = np.sort(keys[owner == l])
        assert len(mine) <= kp
        out[l, :len(mine)] = mine
    return out


def _deal(rng, room, n):
    """The list each of n keys goes to, at random, list l taking room[l] at the most."""
    slots = np.repeat(np.arange(len(room)), room)
    assert n <= len(slots)
    return rng.permutation(slots)[:n]


def _rows(rng, n, avoid=()):
    pool = np.setdiff1d(np.arange(N_ROWS), np.asarray(list(avoid), dtype=np.int64)) if len(avoid) else N_ROWS
    return rng.choice(pool, size=n, replace=False)


def _uncorrelated(rng, L, kp, q, fill=1.0, **_):
    """Distinct random rows under their plausible distances, dealt at random: about kp + 2 survivors."""
    M = L * kp
    n = M if fill >= 1.0 else int(fill * M)
    rows = _rows(rng, n)
    return _lay(L, kp, _key(_d32(q, rows), rows), _deal(rng, np.full(L, kp), n))


def _best_placed(rng, L, kp, q, where="one_list", **_):
    """Every slot filled; the kp best keys all in one list, or one per list (round the lists where there are fewer than kp)."""
    M = L * kp
    rows = _rows(rng, M)
    keys = np.sort(_key(_d32(q, rows), rows))
    order = rng.permutation(L)
    first = np.full(kp, order[0]) if where == "one_list" else order[np.arange(kp) % L]
    room = np.full(L, kp) - np.bincount(first, minlength=L)
    return _lay(L, kp, keys, np.concatenate([first, _deal(rng, room, M - kp)]))


def staircase_heights(kp, max_lists):
    """m[b] = how many small keys list b of a staircase holds: for every column j of the bound one list fewer than would let that
    column cut below the small keys (ceil(kp / j') - 1 lists hold j keys or more, j' the largest bounding column <= j)."""
    cols = columns(kp)
    n = []
    for j in range(1, kp + 1):
        jp = max(c for c in cols if c <= j)
        n.append(min(-(-kp // jp) - 1, max_lists))
    return np.array([sum(1 for v in n if v > b) for b in range(max(n) if n else 0)], dtype=np.int64)


def _staircase(rng, L, kp, q, big=True, max_lists=None, **_):
    """The lists that defeat the pruning bound: as many small keys as the columns allow, big keys behind them (big=False: padding
    behind them, so that no column has enough entries to give a bound at all)."""
    m = staircase_heights(kp, min(L - 1 if big else L, kp if max_lists is None else max_lists))
    n_small = int(m.sum())
    n = L * kp if big else n_small
    rows = _rows(rng, n)
    keys = np.sort(_key(_d32(q, rows), rows))
    lists_of = rng.permutation(L)
    owner = np.repeat(lists_of[:len(m)], m)[rng.permutation(n_small)]
    if big:
        room = np.full(L, kp) - np.bincount(owner, minlength=L)
        owner = np.concatenate([owner, _deal(rng, room, n - n_small)])
    return _lay(L, kp, keys, owner)


def _col1_ties(rng, L, kp, q, below=0, tied=None, **_):
    """Column 1 decides tau, and its entries share tau's 32 distance bits: `below` lists start below that distance, `tied` lists at
    it (rows differ), the others above it; every later entry lies above.  kp - below of the tied keys are wanted: tied == kp - below
    puts tau at the end of the tie group, more puts it inside."""
    tied = L - below if tied is None else tied
    assert L >= kp and below + tied <= L and tied >= kp - below
    M = L * kp
    rows = rng.permutation(_rows(rng, M))
    d = (0.6 + 0.3 * rng.random(M)).astype(np.float32)
    owner = np.repeat(np.arange(L), kp)
    head = np.arange(L) * kp                                  # one key per list: its first entry
    d[head[:below]] = (0.25 + 0.2 * rng.random(below)).astype(np.float32)
    d[head[below:below + tied]] = np.float32(0.5)
    relabel = rng.permutation(L)
    return _lay(L, kp, _key(d, rows), relabel[owner])


def _few_values(rng, L, kp, q, **_):
    """Three distance values in all, dealt at random: ties inside every column."""
    M = L * kp
    rows = _rows(rng, M)
    d = np.array([0.25, 0.5, 0.75], dtype=np.float32)[rng.integers(0, 3, size=M)]
    return _lay(L, kp, _key(d, rows), _deal(rng, np.full(L, kp), M))


def _ragged(rng, L, kp, q, **_):
    """Lists of padding only, one list with a single key, one full list, the others of any length."""
    lens = rng.integers(0, kp + 1, size=L)
    roles = rng.permutation(L)
    lens[roles[0]] = 1
    lens[roles[1:1 + max(1, L // 3)]] = 0
    if L >= 3:
        lens[roles[-1]] = kp
    n = int(lens.sum())
    rows = _rows(rng, n)
    return _lay(L, kp, _key(_d32(q, rows), rows), np.repeat(np.arange(L), lens))


def _scarce(rng, L, kp, q, total=0, **_):
    """`total` real keys in all, spread over the lists."""
    rows = _rows(rng, total)
    return _lay(L, kp, _key(_d32(q, rows), rows), _deal(rng, np.full(L, kp), total))


def _planted(rng, L, kp, q, plant="duplicates", **_):
    """The nominated set is chosen by hand and given small distance bits in a chosen order; every other key lies above them.
      duplicates   copies of one corpus row, the higher row under the smaller key, then random rows: equal in f64, the row decides
      contradict   random rows, the exactly nearest under the largest key: the f32 order is the f64 order reversed
      zero_rows    the corpus's zero rows at random places among random ones"""
    M = L * kp
    if plant == "duplicates":
        first = np.sort(DUP_FIRST + rng.permutation(DUP_COUNT)[:max(1, min(kp, DUP_COUNT) * 2 // 3)])[::-1]
    elif plant == "zero_rows":
        first = np.array(ZERO_ROWS[:min(kp, 3)], dtype=np.int64)
    else:
        first = np.zeros(0, dtype=np.int64)
    rest = _rows(rng, M - len(first), avoid=list(range(DUP_FIRST, DUP_FIRST + DUP_COUNT)) + list(ZERO_ROWS))
    n_fill = kp - len(first)
    chosen, others = np.concatenate([first, rest[:n_fill]]).astype(np.int64), rest[n_fill:]
    if plant == "contradict":
        exact = np.array([oracle_np.cosine_accurate(q, corpus()[i]) for i in chosen])
        chosen = chosen[np.argsort(-exact, kind="stable")]
    elif plant == "zero_rows":
        chosen = rng.permutation(chosen)
    d_chosen = (0.01 * (np.arange(kp) + 1) / kp).astype(np.float32)      # chosen[i] under the i-th smallest key
    keys = np.concatenate([_key(d_chosen, chosen), _key(_d32(q, others) + np.float32(0.05), others)])
    return _lay(L, kp, keys, _deal(rng, np.full(L, kp), len(keys)))


GENERATORS = {"uncorrelated": _uncorrelated, "best_placed": _best_placed, "staircase": _staircase, "col1_ties": _col1_ties,
              "few_values": _few_values, "ragged": _ragged, "scarce": _scarce, "planted": _planted}


# --------------------------------------------------------------------------------------------------------------------- queries
def _query(rng, kind):
    """random: a random vector; row: a copy of the duplicated corpus row (distance 0 to 72 rows); zero; at_max: the largest
    magnitude is exactly 2^40, the last one inside the domain; above_max / below_min: one f32 step outside it."""
    q = rng.standard_normal(DIM).astype(np.float32)
    if kind == "row":
        return corpus()[DUP_FIRST].copy()
    if kind == "zero":
        return np.zeros(DIM, dtype=np.float32)
    if kind in ("at_max", "above_max", "below_min"):
        i = int(np.argmax(np.abs(q)))
        edge = DOMAIN_MIN if kind == "below_min" else DOMAIN_MAX
        q = (q * (edge / np.abs(q[i])) * np.float32(0.5)).astype(np.float32)     # every other magnitude well below the edge
        q[i] = {"at_max": DOMAIN_MAX, "above_max": np.nextafter(DOMAIN_MAX, np.float32(np.inf)),
                "below_min": np.nextafter(DOMAIN_MIN, np.float32(0))}[kind]
        assert int(np.argmax(np.abs(q))) == i
    return q


# ------------------------------------------------------------------------------------------------------------- the case table
def _c(name, L, kp, k_out, content="uncorrelated", nq=1, queries="random", **opts):
    return name, dict(L=L, kp=kp, k_out=k_out, content=content, nq=nq, queries=queries, opts=opts)


def _table():
    t = []
    # every shape at which a branch of the kernel changes, on uncorrelated lists (one list: with padding at its tail)
    for L, kp, k_out in [(1, 1, 1), (1, 9, 1), (1, 64, 56), (1, 72, 64)]:
        t.append(_c("one_list-%dx%d_to_%d" % (L, kp, k_out), L, kp, k_out, nq=3, fill=1.0))
        t.append(_c("one_list_short-%dx%d_to_%d" % (L, kp, k_out), L, kp, k_out, nq=3, fill=0.6, gaps=True))
    shapes = [(2, 9, 1), (16, 11, 3), (8, 64, 56), (7, 72, 64), (57, 9, 1),                    # few keys: M <= 512, and 513
              (128, 64, 56), (241, 34, 26), (256, 33, 25), (512, 72, 64),                      # 8 keys per thread: M 8192 | 8194 ..
              (256, 11, 3), (257, 11, 3), (512, 11, 3),                                        # column_tau<4> | <8>
              (40, 34, 26), (40, 35, 27),                                                      # product tables | staged rows
              (512, 1, 1), (300, 2, 1), (300, 2, 2), (200, 3, 2), (16, 64, 1), (9, 65, 65), (9, 72, 72), (12, 66, 1),
              (20, 68, 60), (64, 56, 56)]
    for L, kp, k_out in shapes:
        t.append(_c("uncorrelated-%dx%d_to_%d" % (L, kp, k_out), L, kp, k_out))
    for L, kp, k_out in [(16, 11, 3), (57, 9, 1), (241, 34, 26), (256, 33, 25), (512, 72, 64), (257, 11, 3), (40, 35, 27)]:
        t.append(_c("best_in_one_list-%dx%d_to_%d" % (L, kp, k_out), L, kp, k_out, "best_placed", where="one_list"))
        t.append(_c("best_one_per_list-%dx%d_to_%d" % (L, kp, k_out), L, kp, k_out, "best_placed", where="one_per_list"))
    # query counts, with strides whose gaps hold foreign words (lists) and sentinels (outputs), an overflow word per query
    for L, kp, k_out, nq in [(16, 11, 3, 3), (57, 9, 1, 33), (64, 18, 10, 33), (256, 33, 25, 3), (1, 64, 56, 33)]:
        t.append(_c("strided-%dx%d_to_%d_nq%d" % (L, kp, k_out, nq), L, kp, k_out, nq=nq, gaps=True, overflow="drawn",
                    fill=1.0 if L > 1 else 0.8))
    # staircases: the survivor counts that take each form of the rank code behind a real bound (M > 512)
    for L, kp, k_out, mx, want in [(40, 16, 8, None, (1, 96)), (40, 24, 16, None, (1, 96)), (48, 32, 24, 20, (97, 128)),
                                   (48, 32, 24, None, (129, 256)), (64, 56, 56, None, (257, 512)), (256, 72, 64, None, (257, 512)),
                                   (512, 72, 72, None, (257, 512)), (300, 64, 1, None, (257, 512))]:
        t.append(_c("staircase-%dx%d_to_%d%s" % (L, kp, k_out, "" if mx is None else "_cut%d" % mx), L, kp, k_out, "staircase",
                    big=True, max_lists=mx, survivors=want))
    for L, kp, k_out, want in [(40, 24, 16, (1, 96)), (80, 72, 64, (257, 512)), (300, 40, 30, (129, 256))]:
        t.append(_c("staircase_no_bound-%dx%d_to_%d" % (L, kp, k_out), L, kp, k_out, "staircase", big=False, survivors=want))
    # ties at tau: inside the tie group and at its end, with and without lists below it; ties in every column
    for L, kp, k_out, below, tied in [(60, 9, 4, 0, None), (60, 9, 4, 0, 9), (60, 9, 4, 3, 6), (60, 9, 4, 3, 30), (300, 24, 16, 5, 200),
                                      (24, 24, 24, 0, None), (512, 33, 25, 1, 511)]:
        t.append(_c("col1_ties-%dx%d_to_%d_below%d_tied%s" % (L, kp, k_out, below, "all" if tied is None else tied), L, kp, k_out,
                    "col1_ties", below=below, tied=tied))
    for L, kp, k_out in [(16, 11, 3), (57, 9, 1), (241, 34, 26), (512, 72, 64), (300, 2, 2)]:
        t.append(_c("few_values-%dx%d_to_%d" % (L, kp, k_out), L, kp, k_out, "few_values"))
    # ragged lists, too few keys
    for L, kp, k_out, nq in [(3, 9, 4, 3), (57, 9, 1, 3), (64, 18, 10, 3), (300, 35, 27, 1), (512, 72, 64, 1)]:
        t.append(_c("ragged-%dx%d_to_%d_nq%d" % (L, kp, k_out, nq), L, kp, k_out, "ragged", nq=nq))
    for L, kp, k_out, total in [(1, 9, 4, 0), (1, 9, 4, 3), (16, 11, 3, 0), (16, 11, 3, 2), (16, 11, 3, 10), (16, 11, 3, 11),
                                (64, 18, 10, 9), (64, 18, 10, 17), (64, 18, 10, 18), (300, 35, 27, 34)]:
        t.append(_c("scarce-%dx%d_to_%d_holds%d" % (L, kp, k_out, total), L, kp, k_out, "scarce", total=total, f32_err=F32_ERR_SCAN))
    # planted nominations
    for plant in ("duplicates", "contradict", "zero_rows"):
        for L, kp, k_out in [(1, 64, 56), (16, 11, 3), (64, 18, 10), (40, 35, 27), (256, 72, 64)]:
            t.append(_c("%s-%dx%d_to_%d" % (plant, L, kp, k_out), L, kp, k_out, "planted", plant=plant))
    for L, kp, k_out in [(1, 64, 56), (16, 11, 3), (64, 18, 10), (40, 35, 27), (256, 72, 64)]:
        t.append(_c("query_is_a_row-%dx%d_to_%d" % (L, kp, k_out), L, kp, k_out, "planted", plant="duplicates", queries="row"))
        t.append(_c("zero_query-%dx%d_to_%d" % (L, kp, k_out), L, kp, k_out, "planted", plant="zero_rows", queries="zero"))
    t.append(_c("zero_query_uncorrelated-57x9_to_4", 57, 9, 4, queries="zero"))
    # the workspace score threshold on ordinary lists (a zero query scores 0 against every row but the zero rows)
    for thr in (-0.05, 0.0, 0.02):
        t.append(_c("threshold_%g-64x18_to_10" % thr, 64, 18, 10, nq=3, ws_threshold=thr, f32_err=F32_ERR_F16X1))
    t.append(_c("threshold_0.5_row_query-40x35_to_27", 40, 35, 27, "planted", plant="duplicates", queries="row", ws_threshold=0.5,
                f32_err=F32_ERR_SCAN))
    # the domain: the last magnitude inside, one step outside at either end, between ordinary queries
    t.append(_c("domain-16x11_to_3", 16, 11, 3, nq=5, queries=["random", "at_max", "above_max", "below_min", "random"],
                f32_err=F32_ERR_SCAN, overflow="drawn"))
    t.append(_c("domain-256x33_to_25", 256, 33, 25, nq=3, queries=["above_max", "random", "at_max"], f32_err=F32_ERR_SCAN))
    # the certificate's border: floor_out on the k_out-th distance and one f64 step either side of it; the same through the workspace
    # threshold; the threshold's own border with fewer than k_out rows passing.  Each without an overflow word, with a zero one and
    # with a set one.
    for L, kp, k_out in [(1, 12, 4), (16, 12, 4), (64, 44, 36)]:
        for form in ("plain", "threshold", "too_few"):
            for step in (-1, 0, 1):
                for ovf in (None, "zero", "set"):
                    t.append(_c("certificate_%s_%s-%dx%d_to_%d_overflow_%s" % (form, {-1: "below", 0: "at", 1: "above"}[step], L, kp, k_out,
                                                                              ovf), L, kp, k_out, "certificate", form=form, step=step,
                                overflow=ovf))
    return t


_TABLE = dict(_table())
assert len(_TABLE) == len(_table())
ERRS = (F32_ERR_SCAN, F32_ERR_F16X1, 0.0)
ROW_BASES = (0, (1 << 40) + 12345, 0xFFFFFFFF)


def case_names():
    return list(_TABLE)


def spec(name):
    return _TABLE[name]


class Case:
    """What a case holds: name, L, kp, k_out, nq; queries f32 [nq][256]; lists uint64 [nq][L][kp]; ws_threshold (None = none);
    row_base; f32_err; overflow uint32 [nq] or None; gaps (lay the lists and the outputs out with strides and fill the gaps);
    survivors: the (low, high) range the model's count of query 0 must fall in, or None."""


_CASES = {}
CERT_D = np.float32(1.25)   # the kp-th key's distance in the certificate cases: D - t is exact for every t in [0.625, 2.5]


def _cert_err(target):
    """f32_err with float64(CERT_D) - f32_err == target, exactly."""
    err = np.float64(CERT_D) - np.float64(target)
    assert err > 0 and np.float64(CERT_D) - err == target
    return float(err)


def _certificate(rng, c, L, kp, k_out, form, step):
    """The nominated keys carry small distance bits and the kp-th of them CERT_D, the others lie above.  plain / threshold: f32_err
    puts floor_out on the k_out-th exact distance or one f64 step beside it (threshold: a threshold every row passes).  too_few: a
    zero query, which scores 1 against the zero rows and 0 against the others, under the threshold 0.25: the three zero rows pass,
    fewer than k_out, and f32_err puts 1 - floor_out on the threshold or one step beside it."""
    M = L * kp if L > 1 else kp
    zero = form == "too_few"
    q = _query(rng, "zero" if zero else "random")
    first = np.array(ZERO_ROWS, dtype=np.int64) if zero else np.zeros(0, dtype=np.int64)
    rest = _rows(rng, M - len(first), avoid=ZERO_ROWS)
    chosen = rng.permutation(np.concatenate([first, rest[:kp - len(first)]]))
    d_chosen = (0.01 * (np.arange(kp) + 1) / kp).astype(np.float32)
    d_chosen[-1] = CERT_D
    others = rest[kp - len(first):]
    keys = np.concatenate([_key(d_chosen, chosen), _key((1.3 + 0.5 * rng.random(len(others))).astype(np.float32), others)])
    c.queries = q[None, :]
    c.lists = _lay(L, kp, keys, _deal(rng, np.full(L, kp), len(keys)))[None]
    toward = {-1: -np.inf, 0: None, 1: np.inf}[step]
    if zero:
        c.ws_threshold = 0.25
        target = np.float64(0.75)      # 1 - 0.75 == 0.25 and both neighbours of 0.75 give exact differences too
    else:
        c.ws_threshold = -1.0 if form == "threshold" else None
        exact = np.sort([oracle_np.cosine_accurate(q, corpus()[i]) for i in chosen])
        target = np.float64(exact[k_out - 1])
        assert 0.625 < target < 1.25
    c.f32_err = _cert_err(target if toward is None else np.nextafter(target, toward))


def case(name):
    """The named case, built once from a seed that depends on the name alone.  Its arrays are read-only."""
    if name in _CASES:
        return _CASES[name]
    s = spec(name)
    L, kp, k_out, nq, opts = s["L"], s["kp"], s["k_out"], s["nq"], s["opts"]
    seed = zlib.crc32(name.encode())
    rng = np.random.default_rng(seed)
    c = Case()
    c.name, c.L, c.kp, c.k_out, c.nq = name, L, kp, k_out, nq
    c.gaps = bool(opts.get("gaps", False))
    c.survivors = opts.get("survivors")
    c.row_base = ROW_BASES[seed % 3]
    c.ws_threshold = opts.get("ws_threshold")
    c.f32_err = opts.get("f32_err", ERRS[(seed // 3) % 3])
    if s["content"] == "certificate":
        _certificate(rng, c, L, kp, k_out, opts["form"], opts["step"])
    else:
        kinds = s["queries"] if isinstance(s["queries"], list) else [s["queries"]] * nq
        c.queries = np.stack([_query(rng, k) for k in kinds])
        gen = GENERATORS[s["content"]]
        c.lists = np.stack([gen(rng, L, kp, c.queries[i], **opts) for i in range(nq)])
    ovf = opts.get("overflow")
    c.overflow = None if ovf is None else {"zero": np.zeros(nq, dtype=np.uint32), "set": np.full(nq, 7, dtype=np.uint32),
                                           "drawn": (rng.integers(0, 2, size=nq) * rng.integers(1, 1 << 32, size=nq)).astype(np.uint32)}[ovf]
    if ovf == "drawn" and nq >= 2:
        c.overflow[0], c.overflow[1] = 0, 0x80000000
    for a in (c.queries, c.lists) + (() if c.overflow is None else (c.overflow,)):
        a.setflags(write=False)
    _CASES[name] = c
    return c


_REFS = {}


def reference(name):
    """select() of the named case, computed once: (rows, dist, counts, status)."""
    if name not in _REFS:
        c = case(name)
        _REFS[name] = select(corpus(), c.queries, c.lists, c.k_out, c.ws_threshold, c.row_base, c.f32_err, c.overflow)
    return _REFS[name]
