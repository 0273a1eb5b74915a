"""GPU: final_select_kernel (csrc/select.hip) -- every top_k <= 56 answer leaves the library through it -- on constructed block lists,
against a NumPy select (tests/select_ref.py), bit for bit: rows and counts as uint64, distances by their 64-bit patterns, both status
outputs, the growth of the context's sticky counter, and the words between strided lists.  No tolerance anywhere.

The lists go through smt_debug_select_lists, which hands them to launch_select unchanged; the rows behind the keys are one host-built
corpus of 40 000 rows, uploaded once.  Nothing is scanned.  For one-query cases of several lists the survivor count the kernel
records (word 8 behind the tuning key select_debug_ptr) must equal select_ref.model_survivors: the witness that the case ran the
branch it was built for.  tests/test_select_ref_cpu.py shows, without a GPU, which branches those are and that the cases tell a subtly
wrong select from the right one.

Not here: the lists of a production scan.  No entry point hands them out (the scan's list buffer is internal to the call), so the tie
between this contract and what the scan writes stays with the end-to-end tests (test_gpu_scan.py, test_gpu_nearties.py)."""
import numpy as np
import pytest

from tests import select_ref as sr

pytestmark = pytest.mark.gpu

NAMES = sr.case_names()
POISON, GUARD = np.uint64(0xA5A5A5A5A5A5A5A5), np.uint64(0xC3C3C3C3C3C3C3C3)
POISON32, GUARD32 = np.uint32(0xA5A5A5A5), np.uint32(0xC3C3C3C3)
G = 64                       # guard words on either side of an output
LIST_GAP = np.array([0, 1, 3, 0x3F000000_00000005, 0x7F7FFFFF_00000009], dtype=np.uint64)   # foreign words between two queries' lists:
OUT_GAP = 3                                                                                 # keys below every real key among them


@pytest.fixture(scope="module")
def env():
    import torch  # noqa: F401  (first: the library binds to the HIP runtime torch loaded)
    import semtools_amd as smt

    ctx = smt.Context(0)
    corpus = smt.Corpus(ctx)
    corpus.append(sr.corpus())
    assert corpus.rows == sr.N_ROWS
    yield ctx, corpus
    corpus.close()
    ctx.close()


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    view = {8: np.int64, 4: np.int32}[a.dtype.itemsize]
    return torch.from_numpy(a.view(view).copy()).cuda()


class _Guarded:
    """n poisoned words on the device (8 bytes each, or 4) with G guard words in front of them and G behind."""

    def __init__(self, n, bytes_per_word=8):
        dt, self.poison, self.guard = (np.uint64, POISON, GUARD) if bytes_per_word == 8 else (np.uint32, POISON32, GUARD32)
        h = np.full(G + n + G, self.poison, dtype=dt)
        h[:G] = self.guard
        h[G + n:] = self.guard
        self.n, self.dt = n, dt
        self.t = _dev(h)
        self.ptr = self.t.data_ptr() + G * bytes_per_word

    def read(self):
        h = self.t.cpu().numpy().view(self.dt)
        assert (h[:G] == self.guard).all(), "words in front of the output were written"
        assert (h[G + self.n:] == self.guard).all(), "words behind the output were written"
        return h[G:G + self.n].copy()

    def untouched(self):
        return bool((self.read() == self.poison).all())


class _Launch:
    """One call of the hook for a case: inputs uploaded, outputs poisoned and guarded.  passed: arguments as the library is to hear
    them where they are not the case's (the buffers keep the case's sizes)."""

    def __init__(self, corpus, c, optional_outputs=True, **passed):
        import torch

        self.c, self.corpus, self.passed = c, corpus, passed
        M = c.L * c.kp
        self.list_stride = M + len(LIST_GAP) if c.gaps else 0
        self.out_stride = c.k_out + OUT_GAP if c.gaps else 0
        stride = self.list_stride or M
        flat = np.tile(np.concatenate([np.zeros(M, dtype=np.uint64), LIST_GAP])[:stride], c.nq)
        for q in range(c.nq):
            flat[q * stride:q * stride + M] = c.lists[q].reshape(-1)
        self.lists_host = flat
        self.lists, self.queries = _dev(flat), _dev(c.queries)
        self.overflow = None if c.overflow is None else _dev(c.overflow)
        ostride = self.out_stride or c.k_out
        self.rows, self.dist = _Guarded(c.nq * ostride), _Guarded(c.nq * ostride)
        self.counts = _Guarded(c.nq) if optional_outputs else None
        self.uncertain = _Guarded(c.nq) if optional_outputs else None
        self.status = _Guarded(c.nq, 4) if optional_outputs else None
        torch.cuda.synchronize()

    def outputs(self):
        return [o for o in (self.rows, self.dist, self.counts, self.uncertain, self.status) if o is not None]

    def call(self):
        c, p = self.c, self.passed
        ptr = lambda o: None if o is None else o.ptr
        args = dict(queries_ptr=self.queries.data_ptr(), nq=c.nq, lists_ptr=self.lists.data_ptr(), n_lists=c.L, kp=c.kp, k_out=c.k_out,
                    out_rows_ptr=self.rows.ptr, out_dist_ptr=self.dist.ptr, list_stride=self.list_stride, out_stride=self.out_stride,
                    ws_threshold=c.ws_threshold, row_base=c.row_base, f32_err=c.f32_err,
                    overflow_ptr=None if self.overflow is None else self.overflow.data_ptr(), out_counts_ptr=ptr(self.counts),
                    out_uncertain_ptr=ptr(self.uncertain), out_status_ptr=ptr(self.status))
        args.update(p)
        self.corpus.debug_select_lists(**args)

    def answer(self):
        """(rows [nq][k_out], dist [nq][k_out]) after checking that the words between the output lists still hold the poison."""
        c = self.c
        ostride = self.out_stride or c.k_out
        r, d = self.rows.read().reshape(c.nq, ostride), self.dist.read().reshape(c.nq, ostride)
        assert (r[:, c.k_out:] == POISON).all() and (d[:, c.k_out:] == POISON).all(), "words between two output lists were written"
        return r[:, :c.k_out], d[:, :c.k_out].copy().view(np.float64)


def _assert_answer(name, got_r, got_d, want_r, want_d):
    bad = np.argwhere((got_r != want_r) | (np.ascontiguousarray(got_d).view(np.uint64) != np.ascontiguousarray(want_d).view(np.uint64)))
    if len(bad):
        q, i = (int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d slots differ; first at query %d slot %d: got (%d, %r), expected (%d, %r)"
                             % (name, len(bad), got_r.size, q, i, got_r[q, i], got_d[q, i], want_r[q, i], want_d[q, i]))


@pytest.mark.parametrize("name", NAMES)
def test_select_equals_the_numpy_select(env, name):
    ctx, corpus = env
    c = sr.case(name)
    want_r, want_d, want_counts, want_status = sr.reference(name)
    witness = c.nq == 1 and c.L > 1
    dbg = _dev(np.zeros(16, dtype=np.uint64)) if witness else None
    run = _Launch(corpus, c)           # (ends with a device-wide synchronisation: the uploads are done)
    ctx.synchronize()
    ctx.uncertain_count(reset=True)
    try:
        if witness:
            ctx.set_tuning("select_debug_ptr", dbg.data_ptr())
        run.call()
        ctx.synchronize()
    finally:
        ctx.set_tuning("select_debug_ptr", 0)
    got_r, got_d = run.answer()
    _assert_answer(name, got_r, got_d, want_r, want_d)
    assert np.array_equal(run.counts.read(), want_counts), name
    assert np.array_equal(run.status.read(), want_status), (name, run.status.read(), want_status)
    assert np.array_equal(run.uncertain.read(), want_status.astype(np.uint64)), name
    assert ctx.uncertain_count(reset=True) == int((want_status != 0).sum()), name
    assert np.array_equal(run.lists.cpu().numpy().view(np.uint64), run.lists_host), "the select wrote into its lists"
    if witness:
        S = int(dbg.cpu().numpy().view(np.uint64)[8])
        print("survivors %s device %d model %d" % (name, S, sr.model_survivors(c.lists[0])))
        assert S == sr.model_survivors(c.lists[0]), name
        if c.survivors:
            assert c.survivors[0] <= S <= c.survivors[1], name


@pytest.mark.parametrize("name", ["strided-16x11_to_3_nq3", "strided-256x33_to_25_nq3", "one_list_short-1x64_to_56", "domain-16x11_to_3"])
def test_optional_outputs_may_be_null(env, name):
    """Without counts, uncertain and status words the answer is the same and the sticky counter still counts."""
    ctx, corpus = env
    c = sr.case(name)
    want_r, want_d, _, want_status = sr.reference(name)
    run = _Launch(corpus, c, optional_outputs=False)
    ctx.synchronize()
    ctx.uncertain_count(reset=True)
    run.call()
    ctx.synchronize()
    _assert_answer(name, *run.answer(), want_r, want_d)
    assert ctx.uncertain_count(reset=True) == int((want_status != 0).sum())


def test_the_sticky_counter_adds_up_over_calls(env):
    """Two calls without a reset in between: the counter holds the sum, and reading it with reset = 0 leaves it."""
    ctx, corpus = env
    names = ["domain-16x11_to_3", "strided-57x9_to_1_nq33"]
    ctx.synchronize()
    ctx.uncertain_count(reset=True)
    for n in names:
        _Launch(corpus, sr.case(n)).call()
    ctx.synchronize()
    want = sum(int((sr.reference(n)[3] != 0).sum()) for n in names)
    assert want >= 3
    assert ctx.uncertain_count(reset=False) == want and ctx.uncertain_count(reset=True) == want and ctx.uncertain_count() == 0


def test_no_query_is_ok_and_touches_nothing(env):
    ctx, corpus = env
    run = _Launch(corpus, sr.case("strided-16x11_to_3_nq3"), nq=0)
    run.call()
    ctx.synchronize()
    assert all(o.untouched() for o in run.outputs())


# --------------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("passed", [dict(n_lists=0), dict(n_lists=513), dict(kp=0), dict(kp=73), dict(k_out=0), dict(k_out=12),
                                    dict(kp=73, k_out=73), dict(queries_ptr=None), dict(lists_ptr=None), dict(out_rows_ptr=None),
                                    dict(out_dist_ptr=None), dict(list_stride=175), dict(out_stride=2)],
                         ids=lambda p: "-".join("%s_%s" % kv for kv in p.items()))
def test_refusals(env, passed):
    """A list count outside 1..512, k' outside 1..72, k_out outside 1..k' (launch_select's own refusals), a null pointer, a stride
    shorter than what it strides over: SMT_E_INVALID, nothing enqueued, the poisoned outputs as they were."""
    from semtools_amd import _lib as L

    ctx, corpus = env
    ctx.synchronize()
    ctx.uncertain_count(reset=True)
    run = _Launch(corpus, sr.case("uncorrelated-16x11_to_3"), **passed)     # (16 x 11 keys, k_out 3)
    with pytest.raises(L.SmtError) as e:
        run.call()
    ctx.synchronize()
    assert e.value.code == L.SMT_E_INVALID, e.value
    assert all(o.untouched() for o in run.outputs())
    assert ctx.uncertain_count(reset=True) == 0
