"""Scripts for the queued one-query pipeline with OTHER entry points between the queued calls, a host model of what the library
should hold after every step, and the oracle's answer of every step that answers something.

A script is a list of steps:
    ("search", corpus, query_index, k)   a one-query search_topk_device with its own output rows, a status word and
                                          row_base = 1000 * step + 3
    ("op", name, args)                    any other entry point; `apply_op` says what it does to the rows a corpus holds
A `Script` also carries the rows its corpora start with.  Nothing here touches a GPU: tests/test_pipeline_life_cpu.py checks the
scripts and the model on the CPU, tests/test_gpu_pipeline_life.py performs them.

THE VISIBILITY RULE.  A stale answer must not be able to hide, so every change of a corpus' contents moves the winner of every
query searched afterwards.  A corpus holds at most ONE copy of each of the sixteen queries (one copy: no ties; its distance is +0.0
or an ulp of 1 above it), sixteen consecutive rows, the "planted block".  A change of contents overwrites copies with fresh random unit rows
and plants them elsewhere, or drops or adds the part that holds them.  `check_script` asserts, for every such step and every
query, that the expected rows of the query's next search differ from what the contents before the step would give, and that every
expected top-k is separated from place k + 1 widely enough for a PROVED answer:

    the select proves an answer when the k-th exact distance lies below tau - eps, tau the (k + guard band)-th nominated distance
    and eps = F32_ERR_SCAN = 4e-6 the bound on |nominated - exact| (common.h).  tau >= exact distance of place
    k + 8 - eps >= that of place k + 1 - eps, so d[k + 1] - d[k] > 2 eps is sufficient at every guard band.

EXPECTED ANSWERS are oracle.search_documents(..., accurate=True) on the model's rows at the step (as tests/test_gpu_scan_dispatch.py
has it).  For corpora above 4096 rows the oracle runs on a candidate subset with the row numbers mapped back, as that test does for
its filtered case: the candidates are all rows whose float32 cosine distance (numpy) lies within 1e-3 of the (k + 1)-th smallest,
a thousand times the error of that arithmetic, so they contain the exact top k + 1, and a row's distance and the order by
(distance, row) do not depend on the other rows.  The CPU test compares the shortcut with the oracle on all 65 537 rows."""
import numpy as np

from oracle import oracle as orc

DIM = 256
NQ = 16
KS = (1, 10, 24)
SIZES = (1000, 65_537)          # one block, several blocks (tests/test_gpu_scan_deep.py)
KTOP = max(KS) + 1              # what the model keeps per (contents, query): every k of KS and the place behind it
F32_ERR_SCAN = 4e-6
PROVED_GAP = 2 * F32_ERR_SCAN
SUBSET_ABOVE = 4096
SUBSET_MARGIN = 1e-3
GUARD = 2                       # words in front of and behind every output list that no launch may touch
MODE_WORKSPACE = 1


def unit_rows(rng, n):
    x = rng.standard_normal((n, DIM), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(x)


QUERIES = unit_rows(np.random.default_rng(9000), NQ)


def qsel(i):
    return (i // 2) % NQ        # steps i, i + 2, ... i + 30 carry sixteen different queries (tests/test_gpu_scan_deep.py)


def approx_distances(rows, qs):
    """float32 cosine distances [rows, queries] by numpy, -1 where a row has no direction (zero rows: always candidates)"""
    nrm = np.sqrt(np.einsum("ij,ij->i", rows, rows))
    with np.errstate(divide="ignore", invalid="ignore"):
        approx = 1.0 - (rows @ qs.T) / (nrm[:, None] * np.linalg.norm(qs, axis=1).astype(np.float32)[None, :])
    approx[~np.isfinite(approx)] = -1.0
    return approx


def oracle_topk(rows, q, k, eligible=None, max_distance=None, full=False, approx=None):
    """The oracle's accurate answer over `rows` (the rows `eligible` of them, a sorted index array): (row numbers int64, float64
    distances) of the top k by (distance, row); with max_distance, of ALL rows strictly below it (documents mode).
    approx: approx_distances(rows, q[None])[:, 0], where the caller has it already."""
    idx = np.arange(len(rows), dtype=np.int64) if eligible is None else np.asarray(eligible, dtype=np.int64)
    if len(idx) > SUBSET_ABOVE and not full:
        approx = approx_distances(rows[idx], q[None])[:, 0] if approx is None else approx[idx]
        kk = min(k + 1, len(idx))
        bar = np.partition(approx, kk - 1)[kk - 1] + SUBSET_MARGIN
        if max_distance is not None:
            bar = max(bar, max_distance + SUBSET_MARGIN)
        idx = idx[approx <= bar]
    sub = np.ascontiguousarray(rows[idx])
    res = orc.search_documents(sub, [len(sub)], q, n_lines=0, top_k=k, max_distance=max_distance, accurate=True)
    return (idx[np.array([r["match_line"] for r in res], dtype=np.int64)] if res else np.zeros(0, np.int64),
            np.array([r["distance"] for r in res], dtype=np.float64))


def kept_index(keep):
    return np.concatenate([np.arange(b, e, dtype=np.int64) for b, e in keep] + [np.zeros(0, np.int64)])


# ops that change what a corpus holds (a compact that keeps everything does not: `mutates`)
CONTENT_OPS = ("write_rows", "torch_write", "truncate", "append", "compact", "embed", "readopt")
# ops that leave every corpus' rows alone
NEUTRAL_OPS = ("prepack", "set_tuning", "uncertain_count", "prof", "merge_packed", "search_host", "search_device", "ivf_build",
               "ivf_search", "ivf_close", "group_search", "synchronize")


def mutates(model, name, args):
    if name == "compact":
        return len(kept_index(args[1])) != len(model[args[0]])
    return name in CONTENT_OPS or name in ("close", "create")


def apply_op(model, name, args, table=None):
    """What op `name` does to the rows the library holds: model maps corpus name -> float32 [n, 256] (None: closed)."""
    if name in ("write_rows", "torch_write"):
        c, first, rows = args
        assert first + len(rows) <= len(model[c])
        model[c][first:first + len(rows)] = rows
    elif name == "truncate":
        c, n = args
        assert n <= len(model[c])
        model[c] = model[c][:n].copy()
    elif name == "append":
        c, rows = args
        model[c] = np.concatenate([model[c], rows])
    elif name == "compact":
        c, keep = args
        model[c] = np.ascontiguousarray(model[c][kept_index(keep)])
    elif name == "embed":
        c, ids, offsets = args
        model[c] = np.concatenate([model[c], orc.embed_lines(table, ids, offsets, True, 2048)])
    elif name == "readopt":                                          # closed, and adopted again at the same address with other contents
        c, rows = args
        assert len(rows) == len(model[c])
        model[c] = rows.copy()
    elif name == "close":
        model[args[0]] = None
    elif name == "create":                                           # (corpus, kind, rows)
        model[args[0]] = args[2].copy()
    else:
        assert name in NEUTRAL_OPS, name


class Script:
    def __init__(self, name, corpora, steps, table=None):
        self.name = name
        self.corpora = corpora      # corpus name -> ("owned" | "adopted", rows the corpus starts with)
        self.steps = steps
        self.table = table          # the f32 model table of "embed" steps

    def searches(self):
        return [i for i, s in enumerate(self.steps) if s[0] == "search"]


class Expected:
    """The model's word on a script: answers[i] for step i -- a search: (rows + row_base, distances); an answering op: see
    `_op_answer`; None otherwise -- and the steps that changed contents."""

    def __init__(self):
        self.answers = []
        self.mutations = []
        self.snapshots = {}         # step of an "ivf_search" -> the rows its corpus held then


def row_base(i):
    return 1000 * i + 3


def _op_answer(model, name, args):
    if name == "search_host":
        c, qis, kw = args
        out = []
        for qi in qis:
            q = QUERIES[qi]
            elig = kept_index(kw["ranges"]) if kw.get("ranges") is not None else None
            if kw.get("mode", 0) == MODE_WORKSPACE:
                # rows with score > 1 - max_distance in float32, then always the top_k of them (tests/test_gpu_nearties.py)
                rows, dist = oracle_topk(model[c], q, 64, eligible=elig)
                bar = float(np.float32(1.0) - np.float32(kw["max_distance"]))
                keep = [(d, r) for d, r in zip(dist.tolist(), rows.tolist()) if (1.0 - d) > bar]
                assert len(keep) < 64                                # (the 64 nearest hold every row that passes)
                keep = keep[:kw["top_k"]]
                out.append((np.array([r for _, r in keep], dtype=np.int64), np.array([d for d, _ in keep])))
            else:
                out.append(oracle_topk(model[c], q, kw["top_k"], eligible=elig, max_distance=kw.get("max_distance")))
        return out
    if name == "search_device":
        c, qis, k = args
        return [oracle_topk(model[c], QUERIES[qi], k) for qi in qis]
    if name == "group_search":
        c, qi, k = args
        return oracle_topk(model[c], QUERIES[qi], k)
    return None


def expected(script, check=False):
    """Replays `script` on the model.  check: also asserts the visibility rule and the PROVED gap (`check_script`)."""
    model = {c: rows.copy() for c, (_, rows) in script.corpora.items()}
    ver = {c: 0 for c in model}
    cache = {}

    def top(c, qi):
        key = (c, ver[c], qi)
        if key not in cache:
            if (c, ver[c]) not in cache:                             # (one matrix product per contents)
                for old in [x for x in cache if len(x) == 2 and x[0] == c]:
                    del cache[old]
                cache[(c, ver[c])] = approx_distances(model[c], QUERIES)
            cache[key] = oracle_topk(model[c], QUERIES[qi], KTOP, approx=cache[(c, ver[c])][:, qi])
        return cache[key]

    exp = Expected()
    pending = {}                                                     # search step -> [(mutation step, rows before it)]
    steps = script.steps
    for i, st in enumerate(steps):
        if st[0] == "search":
            _, c, qi, k = st
            assert model[c] is not None and k <= min(len(model[c]), KTOP - 1), (script.name, i)
            rows, dist = top(c, qi)
            exp.answers.append((rows[:k] + row_base(i), dist[:k]))
            if check:
                if len(dist) > k:
                    assert dist[k] - dist[k - 1] > PROVED_GAP, \
                        "%s step %d: place %d and %d of query %d are %g apart" % (script.name, i, k, k + 1, qi, dist[k] - dist[k - 1])
                for m, before in pending.pop(i, []):
                    assert rows[:k].tolist() != before, \
                        "%s: step %d (%s) does not move the winner of query %d, searched next at step %d" % (script.name, m, steps[m][1], qi, i)
            continue
        _, name, args = st
        if mutates(model, name, args):
            c = args[0]
            exp.mutations.append(i)
            if check and model.get(c) is not None:
                seen = set()
                for j in range(i + 1, len(steps)):                   # the next search of every query on this corpus
                    if steps[j][0] == "search" and steps[j][1] == c and steps[j][2] not in seen:
                        seen.add(steps[j][2])
                        k = min(steps[j][3], len(model[c]))
                        pending.setdefault(j, []).append((i, top(c, steps[j][2])[0][:k].tolist()))
            apply_op(model, name, args, script.table)
            ver[c] = ver.get(c, 0) + 1
            exp.answers.append(None)
        else:
            apply_op(model, name, args, script.table)
            exp.answers.append(_op_answer(model, name, args))
            if name == "ivf_search":
                exp.snapshots[i] = model[args[0]].copy()
    exp.final = model
    return exp


def check_script(script):
    """Asserts the visibility rule and the PROVED gap for `script`; returns the model's expectations."""
    return expected(script, check=True)


# ------------------------------------------------------------------------------------------------------------- building scripts

class Builder:
    """Writes a script while it keeps the model, so that the arguments of a step fit the contents at that step."""

    def __init__(self, name, seed, corpora, table=None):
        """corpora: corpus name -> (kind, rows, where the planted block starts: a row, "end" or "random")"""
        self.rng = np.random.default_rng(seed)
        self.name = name
        self.steps = []
        self.table = table
        self.model, self.block, self.initial = {}, {}, {}
        self.n_search = 0
        self.n_planted = 0
        for c, (kind, n, at) in corpora.items():
            rows = unit_rows(self.rng, n)
            p = n - NQ if at == "end" else int(self.rng.integers(0, n - NQ + 1)) if at == "random" else at
            rows[p:p + NQ] = QUERIES
            self.block[c] = p
            self.model[c] = rows
            self.initial[c] = (kind, rows.copy())

    def script(self):
        return Script(self.name, self.initial, self.steps, self.table)

    def fresh(self, n):
        return unit_rows(self.rng, n)

    def search(self, c, qi, k):
        self.steps.append(("search", c, qi, k))
        self.n_search += 1

    def run(self, c, n, k, only=None):
        """n searches of corpus c at one k (a group ends where k changes): the queries in the order of `qsel`, or query `only`."""
        for _ in range(n):
            self.search(c, qsel(self.n_search) if only is None else only, k)

    def op(self, name, *args):
        apply_op(self.model, name, args, self.table)
        self.steps.append(("op", name, args))

    def rows(self, c):
        return len(self.model[c])

    def planted(self):
        """the sixteen queries in an order no block of this script had before: a block planted where one stood earlier still moves
        every winner"""
        self.n_planted += 1
        return np.roll(QUERIES, 1 + (self.n_planted - 1) % (NQ - 1), axis=0)

    def replant_rows(self, c):
        """(first row, 32 rows) that overwrite the planted block with fresh rows and plant it right behind itself, or None when
        there is no room behind it"""
        p, n = self.block[c], self.rows(c)
        if p + 2 * NQ > n:
            return None
        self.block[c] = p + NQ
        return p, np.concatenate([self.fresh(NQ), self.planted()])

    def replant(self, c, op="write_rows"):
        """One write over the block and the sixteen rows behind it; at the end of the corpus two writes: fresh rows over the
        block, the block at a row drawn at random."""
        p = self.block[c]
        w = self.replant_rows(c)
        if w is not None:
            self.op(op, c, w[0], w[1])
            return
        self.op(op, c, p, self.fresh(NQ))
        self.block[c] = int(self.rng.integers(0, p - NQ))
        self.op(op, c, self.block[c], self.planted())

    def tail_with_block(self, n, first=False):
        """n rows whose last (first) sixteen are the planted block"""
        return np.concatenate([self.planted(), self.fresh(n - NQ)] if first else [self.fresh(n - NQ), self.planted()])


def _k(j):
    return KS[j % len(KS)]


SEG = 10         # searches per segment: above the eight that the grouping condition asks for
COVER = 2 * NQ   # searches in which `qsel` names every query: behind a step whose effect the next one undoes

# The seed of every script's random rows.  Whether two places of a random top-k lie closer than PROVED_GAP is luck (about one in a
# hundred per query and contents at 65 537 rows): check_script says so, and such a seed is no use.
SEEDS = {"write_rows": 201, "write_last_chunk": 102, "truncate": 103, "compact": 104, "prepack": 105, "embed": 106,
         "other_searches": 201, "two_corpora": 108, "ivf": 109, "tuning_draining": 110, "tuning_plain": 111, "small_ops": 201,
         "group_path": 113, "random_life": 1000}


def write_rows_script(n):
    b = Builder("write_rows/%d" % n, SEEDS["write_rows"], {"a": ("owned", n, "random")})
    for j in range(6):
        b.run("a", SEG, _k(j))
        b.replant("a")
    b.run("a", SEG, 10)
    return b.script()


def write_last_chunk_script(n):
    """One row of the last chunk, ragged at 65 537 rows: the block sits at the end, row n - 1 is the copy of query 15."""
    b = Builder("write_last_chunk/%d" % n, SEEDS["write_last_chunk"], {"a": ("owned", n, "end")})
    b.run("a", SEG, 10)
    for j in range(3):
        b.op("write_rows", "a", n - 1, b.fresh(1))                   # query 15 loses its copy ...
        b.run("a", SEG, _k(j), only=NQ - 1)
        b.op("write_rows", "a", n - 1, QUERIES[NQ - 1:])             # ... and has it back
        b.run("a", SEG, _k(j + 1), only=NQ - 1)
    b.replant("a")
    b.run("a", COVER, 10)
    return b.script()


def truncate_script(n):
    """truncate, then searches; truncate + append back to the same row count within the capacity; an append that outgrows it."""
    b = Builder("truncate/%d" % n, SEEDS["truncate"], {"a": ("owned", n, "end")})
    b.run("a", SEG, 10)
    b.op("truncate", "a", n - NQ)                                    # the block goes
    b.run("a", SEG, 10)
    b.op("append", "a", b.planted())                                 # ... and is back: the same count, the same address
    b.run("a", SEG, 24)
    for j in range(2):
        b.op("truncate", "a", n - 40)
        b.op("append", "a", b.tail_with_block(40, first=j == 0))     # back to back: n rows again, the block at n - 40, then at n - 16
        b.run("a", SEG, _k(j))
    b.op("truncate", "a", n - NQ)
    grow = 2 * max(n, 1024)                                          # past twice the rows: corpus_reserve moves them and frees the old block
    b.op("append", "a", b.tail_with_block(grow))
    b.run("a", COVER, 10)
    b.op("truncate", "a", n - NQ)
    b.run("a", SEG, 1)
    return b.script()


def compact_script(n):
    """compact_bounce_rows = 64: dropping one row in front bounces every step; dropping 200 copies directly."""
    b = Builder("compact/%d" % n, SEEDS["compact"], {"a": ("owned", n, 300)})
    b.op("set_tuning", "compact_bounce_rows", 64)
    b.run("a", 14, 10)
    b.op("compact", "a", [(0, n)])                                   # keeps everything: no drain by design, answers unchanged
    b.run("a", 14, 10)
    b.op("compact", "a", [(0, 10), (11, n)])                         # bounced (delta 1): every row behind row 10 moves, the block to 299
    b.run("a", 14, 24)
    b.op("compact", "a", [(0, 99), (299, n - 1)])                    # direct (delta 200): the block moves to row 99
    b.run("a", 14, 1)
    b.op("compact", "a", [(0, 99), (99 + NQ, n - 201)])              # ... and goes (delta 16: bounced)
    b.block["a"] = None
    b.run("a", 14, 10)
    b.op("set_tuning", "compact_bounce_rows", 65536)
    return b.script()


def prepack_script(n):
    b = Builder("prepack/%d" % n, SEEDS["prepack"], {"a": ("owned", n, "random")})
    b.run("a", SEG, 10)
    b.op("prepack", "a", True)
    b.run("a", SEG, 10)
    b.replant("a")                                                   # (the image is packed again from the written tile on)
    b.run("a", SEG, 24)
    b.op("search_host", "a", list(range(9)), dict(top_k=10))         # nine queries: the batched kernels, which read the image
    b.run("a", SEG, 10)
    b.op("prepack", "a", False)
    b.run("a", SEG, 1)
    b.replant("a")
    b.run("a", SEG, 10)
    return b.script()


def embed_table():
    """A small f32 table: rows 0 .. 15 are the queries, the rest random"""
    return np.ascontiguousarray(np.concatenate([QUERIES, unit_rows(np.random.default_rng(9001), 48)]))


def embed_script(n):
    table = embed_table()
    b = Builder("embed/%d" % n, SEEDS["embed"], {"a": ("owned", n, "random")}, table=table)
    b.run("a", SEG, 10)
    for j in range(2):
        p = b.block["a"]
        b.op("write_rows", "a", p, b.fresh(NQ))                      # the copies go ...
        b.run("a", SEG, _k(j))
        # ... and come back as embedded lines: twenty lines of three tokens of the random part, then one line per query
        ids = np.concatenate([b.rng.integers(NQ, len(table), size=60), np.arange(NQ)]).astype(np.uint32)
        offsets = np.concatenate([np.arange(0, 60, 3), 60 + np.arange(NQ + 1)]).astype(np.uint64)
        b.op("embed", "a", ids, offsets)
        b.block["a"] = b.rows("a") - NQ
        b.run("a", COVER, _k(j + 1))
    return b.script()


def other_searches_script(n):
    """Another search kind on the same corpus between queued calls: the host form (top_k, max_distance, ranges, mode = 1), the
    device form with five queries, and k = 100 (the large-k route)."""
    b = Builder("other_searches/%d" % n, SEEDS["other_searches"], {"a": ("owned", n, 500)})
    d = oracle_topk(b.model["a"], QUERIES[3], 8)[1]
    b.run("a", SEG, 10)
    b.op("search_host", "a", [3], dict(top_k=10))
    b.run("a", SEG, 10)
    b.op("search_host", "a", [3], dict(top_k=10, max_distance=float((d[3] + d[4]) / 2)))   # four rows lie below it
    b.run("a", SEG, 24)
    b.op("search_host", "a", [3, 4], dict(top_k=10, ranges=[(0, 200), (480, 510), (700, n)]))   # (the block's first ten rows inside)
    b.run("a", SEG, 10)
    b.op("search_host", "a", [3], dict(top_k=8, max_distance=float((d[4] + d[5]) / 2), mode=MODE_WORKSPACE))   # five pass, top 8 of them
    b.run("a", SEG, 1)
    b.op("search_device", "a", [1, 2, 3, 4, 5], 10)
    b.run("a", SEG, 10)
    b.op("search_device", "a", [7], 100)
    b.run("a", SEG, 10)
    b.replant("a")
    b.run("a", SEG, 10)
    return b.script()


def two_corpora_script(n):
    """Queued calls on corpus a while corpus b of the same context is written, truncated, closed; an adopted corpus closed and
    adopted again at the same address with the same row count and other contents; an adopted corpus rewritten by a torch op on the
    context's stream behind a synchronise."""
    b = Builder("two_corpora/%d" % n, SEEDS["two_corpora"], {"a": ("adopted", n, "random"), "b": ("owned", 1000, "end")})
    b.run("a", SEG, 10)
    b.replant("b")
    b.run("a", SEG, 10)
    b.op("truncate", "b", 900)
    b.run("a", SEG, 24)
    b.op("close", "b")
    b.run("a", SEG, 10)
    other = b.fresh(n)
    p = int(b.rng.integers(0, n - 4 * NQ))
    other[p:p + NQ] = b.planted()
    b.block["a"] = p
    b.op("readopt", "a", other)
    b.run("a", 14, 10)
    b.op("synchronize")
    b.replant("a", op="torch_write")
    b.run("a", 14, 1)
    return b.script()


def ivf_script(n):
    b = Builder("ivf/%d" % n, SEEDS["ivf"], {"a": ("owned", n, "random")})
    b.run("a", 16, 10)
    b.op("ivf_build", "a")
    b.run("a", 16, 10)
    b.op("ivf_search", "a", [0, 5, 9], 10)
    b.run("a", 16, 24)
    b.op("ivf_close", "a")
    b.replant("a")
    b.run("a", 16, 10)
    return b.script()


DRAINING_KEYS = [("scan_deep", (0, 15)), ("select_group", (0, 1)), ("scan_pair_ring", (64, 4096)), ("scan_overlap", (0, 1)),
                 ("async_select", (0, 1)), ("merge_on_aux", (1, 0))]
# stored without a drain: the grid and the list size of the NEXT launch change while earlier list sets are still in flight
PLAIN_KEYS = [("scan_blocks", (2, 0)), ("scan_threads", (128, 512)), ("scan_unroll", (8, 4)), ("guard_band", (16, 8)),
              ("direct_delivery", (0, 1))]


def tuning_script(n, plain):
    """set_tuning in mid-series, every key away from its default and back: answers must not move."""
    b = Builder("tuning_%s/%d" % ("plain" if plain else "draining", n), SEEDS["tuning_plain" if plain else "tuning_draining"], {"a": ("owned", n, "random")})
    if not plain:
        b.run("a", SEG, 10)
        for key, (away, back) in DRAINING_KEYS:                      # every switch drains: the counters are read behind each
            b.op("set_tuning", key, away)
            b.run("a", 6, 10)
            b.op("set_tuning", key, back)
            b.run("a", 8, 10)
    else:
        # A plain key's switches sit between queued calls with nothing drained; every key has a stretch of its own, ended by a
        # synchronise, so that the grouping around ITS switches is counted apart from the others' (scan_unroll = 8 included, under
        # which nothing groups: the runs in front of and behind it must).
        b.run("a", 8, 10)
        for key, (away, back) in PLAIN_KEYS:
            b.op("set_tuning", key, away)
            b.run("a", 8, 10)
            if key == "direct_delivery":                             # (the key concerns the host form: one such search, not delivered)
                b.op("search_host", "a", [6], dict(top_k=10))
                b.run("a", 8, 10)
            b.op("set_tuning", key, back)
            b.run("a", 8, 10)
            b.op("synchronize")
    b.replant("a")
    b.run("a", 8 if plain else SEG, 24)
    return b.script()


def small_ops_script(n):
    """uncertain_count(reset=True), prof_enable with prof_every = 4 on and off, merge_topk_packed_device between calls."""
    b = Builder("small_ops/%d" % n, SEEDS["small_ops"], {"a": ("owned", n, "random")})
    b.run("a", SEG, 10)
    b.op("uncertain_count")
    b.run("a", SEG, 10)
    b.op("set_tuning", "prof_every", 4)
    b.op("prof", True)
    b.run("a", 12, 10)
    b.op("prof", False)
    b.op("set_tuning", "prof_every", 1)
    b.run("a", SEG, 24)
    b.op("merge_packed", 0)
    b.run("a", SEG, 10)
    b.op("set_tuning", "merge_on_aux", 1)
    b.op("merge_packed", 1)
    b.run("a", SEG, 10)
    b.op("set_tuning", "merge_on_aux", 0)
    b.replant("a")
    b.run("a", SEG, 1)
    return b.script()


def group_path_script(n):
    """Group.from_ctx(ctx) with a one-shard ShardedCorpus over the same tensor: its search_topk_device (flag pipeline) alternates
    with direct corpus calls (two-stream pipeline) in runs of four."""
    b = Builder("group_path/%d" % n, SEEDS["group_path"], {"a": ("adopted", n, "random")})
    for j in range(8):
        b.run("a", 4, 10)
        for t in range(4):
            b.op("group_search", "a", (4 * j + t) % NQ, 10)
    b.run("a", SEG, 10)
    b.op("synchronize")
    b.replant("a", op="torch_write")
    for j in range(2):
        b.run("a", 4, 10)
        for t in range(4):
            b.op("group_search", "a", (4 * j + t + 5) % NQ, 10)
    b.run("a", SEG, 10)
    return b.script()


def random_life_script(seed, n_steps=150):
    """150 steps, 70 % of them searches, the ops drawn from the scripted ones with the model applied.  A change of contents that
    takes two steps (the copies go, the copies come back elsewhere) has no search between them, so no search ever sees a corpus
    without copies twice; a tuning key set away from its default, or profiling switched on, is set back by the next op; an index is
    built, searched and closed in three steps on end, since it names rows by position.  Drawn from: every scripted op but a
    corpus closed for good (it would only shorten the life; close + adopt at the same address is drawn) and the host form's
    max_distance / ranges / mode variants (their thresholds are read off one fixed corpus in other_searches_script)."""
    table = embed_table()
    b = Builder("random_life/%d" % seed, SEEDS["random_life"] + seed,
                {"small": ("owned", SIZES[0], "random"), "big": ("owned", SIZES[1], "random"), "torch": ("adopted", 5000, "random")},
                table=table)
    names = list(b.model)
    kinds = ["write", "truncate_append", "grow", "compact", "prepack", "embed", "host", "device5", "large_k", "tuning", "keep_all",
             "uncertain", "torch_write", "ivf", "merge", "prof", "group", "readopt"]
    cur, restore = None, None
    while len(b.steps) < n_steps:
        if cur is None:
            cur = (names[int(b.rng.integers(0, len(names)))], KS[int(b.rng.integers(0, len(KS)))])
        # (ops of two or three steps would pull the share of searches below 70 %: the draw leans against the share so far)
        if b.rng.random() < (0.85 if b.n_search < 0.7 * len(b.steps) else 0.55):
            b.run(cur[0], 1, cur[1])
            continue
        if restore is not None:
            b.op(*restore)
            restore = None
            continue
        c = names[int(b.rng.integers(0, len(names)))]
        owned = b.initial[c][0] == "owned"
        kind = kinds[int(b.rng.integers(0, len(kinds)))]
        n, p = b.rows(c), b.block[c]
        if kind == "write" and owned:
            b.replant(c)
        elif kind == "torch_write" and not owned:
            b.op("synchronize")
            b.replant(c, op="torch_write")
        elif kind == "truncate_append" and owned:                    # the rows from the block on go and come back with the block last
            b.op("truncate", c, p)
            b.op("append", c, b.tail_with_block(n - p + NQ))
            b.block[c] = b.rows(c) - NQ
        elif kind == "grow" and owned and n < 70_000:
            b.op("write_rows", c, p, b.fresh(NQ))
            b.op("append", c, b.tail_with_block(n + 100))
            b.block[c] = b.rows(c) - NQ
        elif kind == "compact" and owned and n > 600:                # drops the block and 100 rows more; plants it again in front
            keep = [(0, p), (p + NQ, n - 100)] if p + NQ <= n - 100 else [(0, p - 100)]
            b.op("compact", c, [r for r in keep if r[0] < r[1]])
            b.block[c] = int(b.rng.integers(0, 200))
            b.op("write_rows", c, b.block[c], b.planted())
        elif kind == "keep_all" and owned:
            b.op("compact", c, [(0, n)])
        elif kind == "prepack":
            b.op("prepack", c, bool(b.rng.integers(0, 2)))
        elif kind == "embed" and owned:
            b.op("write_rows", c, p, b.fresh(NQ))
            order = np.roll(np.arange(NQ), int(b.rng.integers(0, NQ)))
            ids = np.concatenate([b.rng.integers(NQ, len(table), size=12), order]).astype(np.uint32)
            offsets = np.concatenate([np.arange(0, 12, 3), 12 + np.arange(NQ + 1)]).astype(np.uint64)
            b.op("embed", c, ids, offsets)
            b.block[c] = b.rows(c) - NQ
        elif kind == "host":
            b.op("search_host", c, [int(b.rng.integers(0, NQ))], dict(top_k=10))
        elif kind == "device5":
            b.op("search_device", c, [int(x) for x in b.rng.integers(0, NQ, size=5)], 10)
        elif kind == "large_k":
            b.op("search_device", c, [int(b.rng.integers(0, NQ))], 100)
        elif kind == "tuning":
            key, values = (PLAIN_KEYS + DRAINING_KEYS)[int(b.rng.integers(0, len(PLAIN_KEYS) + len(DRAINING_KEYS)))]
            b.op("set_tuning", key, values[0])
            restore = ("set_tuning", key, values[1])
            continue                                                 # (the searches go on where they were)
        elif kind == "prof":
            b.op("prof", True)
            restore = ("prof", False)
            continue
        elif kind == "ivf":
            b.op("ivf_build", c)
            b.op("ivf_search", c, [int(x) for x in b.rng.integers(0, NQ, size=3)], 10)
            b.op("ivf_close", c)
        elif kind == "merge":
            b.op("merge_packed", int(b.rng.integers(0, 8)))
        elif kind == "group" and not owned:
            b.op("group_search", c, int(b.rng.integers(0, NQ)), 10)
        elif kind == "readopt" and not owned:                        # closed and adopted again at its address: other rows, the block elsewhere
            other = b.fresh(n)
            b.block[c] = int(b.rng.integers(0, n - 4 * NQ))
            other[b.block[c]:b.block[c] + NQ] = b.planted()
            b.op("readopt", c, other)
        elif kind == "uncertain":
            b.op("uncertain_count")
        else:
            continue
        if b.rng.random() < 0.5:
            cur = None
    if restore is not None:
        b.op(*restore)
    b.run("small", SEG, 10)
    return b.script()


SCRIPTED = {
    "write_rows": write_rows_script,
    "write_last_chunk": write_last_chunk_script,
    "truncate": truncate_script,
    "compact": compact_script,
    "prepack": prepack_script,
    "embed": embed_script,
    "other_searches": other_searches_script,
    "two_corpora": two_corpora_script,
    "ivf": ivf_script,
    "tuning_draining": lambda n: tuning_script(n, 0),
    "tuning_plain": lambda n: tuning_script(n, 1),
    "small_ops": small_ops_script,
    "group_path": group_path_script,
}
RANDOM_SEEDS = (1, 2, 3)


def all_scripts():
    """(id, function that builds the script) of every script the GPU test performs"""
    out = [("%s-%d" % (name, n), (lambda f=f, n=n: f(n))) for name, f in SCRIPTED.items() for n in SIZES]
    return out + [("random_life-%d" % seed, (lambda seed=seed: random_life_script(seed))) for seed in RANDOM_SEEDS]
