"""Object wrappers over the C ABI handles (context / model / corpus)."""
import collections
import ctypes as C
import math

import numpy as np

from . import _lib as L


CompactStats = collections.namedtuple("CompactStats", "calls rows_moved")


def _f32c(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _table(a):
    """An embedding table as the library takes it: a C-contiguous float32, float16 or int8 array, kept in its own dtype.
    Anything that is not a numpy array (a list of rows) becomes float32; an array of another dtype is an error."""
    if not isinstance(a, np.ndarray):
        return _f32c(a)
    L.table_dtype_code(a.dtype)
    return np.ascontiguousarray(a)


def _open(obj):
    """The wrapper still owns a native handle.  An object made ON another one (a sharded corpus on its group) points into it, and its
    destroy reads it: close() asks this of the owner first, because the cycle collector finalises a dropped set of objects in any
    order -- the frames of a failed test, group first -- and a destroy that follows its owner's would read freed memory.  What is
    skipped then went with the owner's contexts or stays allocated until the process ends; close dependents first to free it."""
    return getattr(obj, "_h", None) is not None and bool(obj._h)


class Context:
    """One GPU + one HIP stream (smt_ctx).

    stream=None: the library creates a private non-blocking stream.
    stream=<int>: raw hipStream_t to enqueue on (0 = the null stream), e.g.
    torch.cuda.current_stream().cuda_stream."""

    def __init__(self, device=0, stream=None, _borrowed=None):
        self._h = C.c_void_p()
        self._owned = _borrowed is None
        if _borrowed is not None:          # a context owned by a Group (smt_group_ctx)
            self._h = C.c_void_p(_borrowed)
        elif stream is None:
            L.check(L.lib().smt_ctx_create(int(device), C.byref(self._h)))
        else:
            L.check(L.lib().smt_ctx_create_on_stream(int(device), C.c_void_p(int(stream)), C.byref(self._h)))
        self.device = device

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            if getattr(self, "_owned", True):
                L.lib().smt_ctx_destroy(self._h)
            self._h = None

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        L.check(L.lib().smt_ctx_synchronize(self._h))

    def uncertain_count(self, reset=True):
        """Selects whose exactness certificate failed since the last reset (device entry points only count them)."""
        n = C.c_uint64()
        L.check(L.lib().smt_ctx_uncertain_count(self._h, C.byref(n), int(bool(reset))))
        return int(n.value)

    def deliveries(self):
        """Host-form searches whose answer the select kernel delivered into pinned host memory (smt_debug_deliveries)."""
        n = C.c_uint64(0)
        L.check(L.lib().smt_debug_deliveries(self._h, C.byref(n)))
        return int(n.value)

    def scan_pairs(self):
        """(paired, alone, absorbed): one-query scans of the scan_overlap pipeline that took the query of the call two steps later
        along, ran alone, or were absorbed by the call two steps earlier (smt_debug_scan_pairs).  Synchronises.  With scan_pair > 1 a
        scan takes up to three later calls along: paired counts the scans that took any, absorbed every scan that ended at once.
        Tuning keys: scan_pair (0..3 calls taken along; scan_take: the same limit, 0..7; scan_deep: the same limit, 0..15, the default 15; switching any of them drains the pipeline), scan_pair_ring (slots of the descriptor ring in
        use, 64..4096) and, for tests, scan_pair_wait_us (0..5000: the deciding block waits that long for the later call)."""
        v = [C.c_uint64(0) for _ in range(3)]
        L.check(L.lib().smt_debug_scan_pairs(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def scan_groups(self):
        """by_size: by_size[n - 1] = scans of the scan_overlap pipeline whose corpus pass served n calls, n = 1..4
        (smt_debug_scan_groups).  Synchronises."""
        v = (C.c_uint64 * 4)()
        L.check(L.lib().smt_debug_scan_groups(self._h, v))
        return tuple(int(x) for x in v)

    def scan_groups_wide(self):
        """by_size: the same for n = 1..8 (smt_debug_scan_groups_wide): with the tuning key scan_take above 3 (0..7; the
        limit scan_pair sets, with the range of the eight-call kernel) a pass serves up to eight calls.  Synchronises."""
        v = (C.c_uint64 * 8)()
        L.check(L.lib().smt_debug_scan_groups_wide(self._h, v))
        return tuple(int(x) for x in v)

    def scan_groups_deep(self):
        """by_size: launches of the sixteen-call kernel by calls served, n = 1..16 (smt_debug_scan_groups_deep): with the tuning key
        scan_deep above 7 (0..15, the default 15; the limit scan_pair and scan_take set, with the range of the sixteen-call kernel) a pass serves up
        to sixteen calls.  scan_groups_wide() counts these launches only where they ran alone.  Synchronises."""
        v = (C.c_uint64 * 16)()
        L.check(L.lib().smt_debug_scan_groups_deep(self._h, v))
        return tuple(int(x) for x in v)

    def debug_scan_ring(self, calls_back, n_keys):
        """Test hook (smt_debug_scan_ring): the first n_keys keys (uint64) of the list set of the one-query pipeline call made
        `calls_back` calls ago.  Synchronises; read it before any other scan reuses the scratch."""
        out = np.empty(int(n_keys), dtype=np.uint64)
        L.check(L.lib().smt_debug_scan_ring(self._h, int(calls_back), int(n_keys), L.np_ptr(out)))
        return out

    def select_groups(self):
        """by_size: select launches of the one-launch-per-pass route by calls served, n = 0..16 (smt_debug_select_groups; tuning key
        select_group, default 1): 0 counts the launches of absorbed calls, whose answer their leader's launch wrote.  Synchronises."""
        v = (C.c_uint64 * 17)()
        L.check(L.lib().smt_debug_select_groups(self._h, v))
        return tuple(int(x) for x in v)

    def ov_ready_records(self):
        """Pipeline calls that put a ready event on the caller's stream (smt_debug_ov_ready; tuning key ov_skip_ready, default 1: a
        call made while that stream is empty puts none)."""
        n = C.c_uint64(0)
        L.check(L.lib().smt_debug_ov_ready(self._h, C.byref(n)))
        return int(n.value)

    def host_timing(self):
        """(ns, calls): host nanoseconds of the pipeline calls since set_tuning("host_timing", 1) by kind -- stream queries, ready
        event, scan launch, select launch, aux-stream event, the whole call -- and the calls timed (smt_debug_host_timing)."""
        v, n = (C.c_uint64 * 8)(), C.c_uint64(0)
        L.check(L.lib().smt_debug_host_timing(self._h, v, C.byref(n)))
        return tuple(int(x) for x in v), int(n.value)

    def compact_stats(self, reset=False):
        """CompactStats(calls, rows_moved): the Corpus.compact calls that succeeded on this context and the rows they moved."""
        n, m = C.c_uint64(0), C.c_uint64(0)
        L.check(L.lib().smt_ctx_compact_stats(self._h, C.byref(n), C.byref(m), int(bool(reset))))
        return CompactStats(int(n.value), int(m.value))

    def aux_stream(self):
        """Raw hipStream_t of the context's second stream (async selects run there, or -- tuning key scan_overlap -- it
        waits for them); wrap it with torch.cuda.ExternalStream to chain torch / RCCL work behind an async select."""
        st = C.c_void_p()
        L.check(L.lib().smt_ctx_aux_stream(self._h, C.byref(st)))
        return int(st.value or 0)

    def set_tuning(self, key, value):
        L.check(L.lib().smt_set_tuning(self._h, key.encode(), int(value)))

    def prof_enable(self, on=True):
        L.check(L.lib().smt_prof_enable(self._h, int(bool(on))))

    def prof_reset(self):
        L.check(L.lib().smt_prof_reset(self._h))

    def prof_read(self, kernel):
        n, ms = C.c_uint64(), C.c_double()
        L.check(L.lib().smt_prof_read(self._h, kernel.encode(), C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def merge_topk_device(self, rows_ptr, dist_ptr, n_lists, nq, k_in, k_out, out_rows_ptr, out_dist_ptr):
        L.check(L.lib().smt_merge_topk_device(self._h, C.c_void_p(rows_ptr), C.c_void_p(dist_ptr), n_lists, nq,
                                              k_in, k_out, C.c_void_p(out_rows_ptr), C.c_void_p(out_dist_ptr)))


    def merge_topk_packed_device(self, packed_ptr, n_lists, nq, k_in, k_out, out_packed_ptr):
        L.check(L.lib().smt_merge_topk_packed_device(self._h, C.c_void_p(packed_ptr), n_lists, nq, k_in, k_out,
                                                     C.c_void_p(out_packed_ptr)))

    def debug_merge_sources(self, list_ptrs, nq, k_in, k_out, out_packed_ptr, n_lists=None):
        """Test hook (smt_debug_merge_sources): the in-place merge of the peer transport over packed [nq][2][k_in] lists, one device
        pointer each.  n_lists: the count passed on, where it is not len(list_ptrs)."""
        n = len(list_ptrs)
        lp = (C.c_void_p * max(n, 1))(*[C.c_void_p(int(p)) for p in list_ptrs])
        L.check(L.lib().smt_debug_merge_sources(self._h, lp, n if n_lists is None else int(n_lists), nq, k_in, k_out,
                                                C.c_void_p(out_packed_ptr)))

    def debug_merge_packed_strided(self, packed_ptr, list_stride_words, n_lists, nq, k_in, k_out, out_packed_ptr):
        """Test hook (smt_debug_merge_packed_strided): merge_topk_packed_device over lists list_stride_words apart (0 = dense)."""
        L.check(L.lib().smt_debug_merge_packed_strided(self._h, C.c_void_p(packed_ptr), int(list_stride_words), n_lists, nq, k_in, k_out,
                                                       C.c_void_p(out_packed_ptr)))

    def debug_combine_status(self, n, nq, out_status_ptr, word_ptrs=None, base_ptr=None, stride_words=0):
        """Test hook (smt_debug_combine_status): the worst of n sources' status words per query, the sources given by pointer
        (word_ptrs) or stride_words apart behind base_ptr -- exactly one of the two."""
        wp = None
        if word_ptrs is not None:
            wp = (C.c_void_p * max(len(word_ptrs), 1))(*[C.c_void_p(int(p)) for p in word_ptrs])
        L.check(L.lib().smt_debug_combine_status(self._h, wp, C.c_void_p(base_ptr) if base_ptr else None, int(stride_words), int(n), int(nq),
                                                 C.c_void_p(out_status_ptr)))

    @staticmethod
    def debug_gemm_plan(plan_tiles, nq, kp, family=0, f16x1=False, blocks=256, gemm_bootstrap=1, gemm_boot_fine=1, gemm_split_last=2,
                        gemm_qsplit=1):
        """Test hook (smt_debug_gemm_plan; host only: no GPU and no context, call it on the class): the launches of a batched call's level plan, in order -- a list of dicts
        with the keys kind (0 bootstrap, 1 appended), stride, skip, tile_begin, tile_end, qsplit, blocks, slots, select, thresholds,
        buffer_fits."""
        cap = 16
        out = np.zeros((cap, L.GEMM_PLAN_WORDS), dtype=np.uint64)
        n = C.c_uint32(0)
        L.check(L.lib().smt_debug_gemm_plan(int(plan_tiles), int(nq), int(kp), int(family), int(bool(f16x1)), int(blocks), int(gemm_bootstrap),
                                            int(gemm_boot_fine), int(gemm_split_last), int(gemm_qsplit), L.np_ptr(out), cap, C.byref(n)))
        keys = ("kind", "stride", "skip", "tile_begin", "tile_end", "qsplit", "blocks", "slots", "select")
        plan = []
        for w in out[:int(n.value)].tolist():
            e = dict(zip(keys, w))
            e["thresholds"], e["buffer_fits"] = bool(w[9] & 1), bool(w[9] & 2)
            plan.append(e)
        return plan

    def debug_bootstrap_tau(self, tile_min_ptr, n_slots, nq, nq_pad, kp, tau_ptr, qconst_ptr):
        """Test hook (smt_debug_bootstrap_tau): bootstrap_tau_kernel on device buffers, asynchronous on the context's stream."""
        L.check(L.lib().smt_debug_bootstrap_tau(self._h, C.c_void_p(int(tile_min_ptr)), int(n_slots), int(nq), int(nq_pad), int(kp),
                                                C.c_void_p(int(tau_ptr)), C.c_void_p(int(qconst_ptr))))

    def debug_level_select(self, cand_ptr, counts_ptr, overflow_ptr, tau_ptr, nq, kp, qconst_ptr=None):
        """Test hook (smt_debug_level_select): level_select_kernel in place on device buffers (distinct keys per query), asynchronous on
        the context's stream."""
        L.check(L.lib().smt_debug_level_select(self._h, C.c_void_p(int(cand_ptr)), C.c_void_p(int(counts_ptr)), C.c_void_p(int(overflow_ptr)),
                                               C.c_void_p(int(tau_ptr)), C.c_void_p(int(qconst_ptr)) if qconst_ptr else None, int(nq), int(kp)))

    def debug_gemm_trace(self, buf_ptr=None, cap_words=0):
        """Test hook (smt_debug_gemm_trace): sets (or, without a pointer, clears) the trace buffer of batched calls; returns
        (select passes, 32-bit words) recorded since it was last set."""
        n, w = C.c_uint32(0), C.c_uint64(0)
        L.check(L.lib().smt_debug_gemm_trace(self._h, C.c_void_p(int(buf_ptr)) if buf_ptr else None, int(cap_words), C.byref(n), C.byref(w)))
        return int(n.value), int(w.value)


class Model:
    """Device-resident model2vec table (smt_model)."""

    def __init__(self, ctx, table=None, normalize=True, device_ptr=None, V=None, dtype=np.float32, mapping=None, weights=None,
                 mapping_ptr=None, weights_ptr=None, n_tokens=None):
        """table: a float32, float16 or int8 array [V x 256], uploaded as it is (K1 widens narrow rows in registers).
        device_ptr / V / dtype: adopt a table of that dtype already in device memory.
        mapping / weights: the indexed form of a vocabulary-quantised model -- token id -> table row (integers) and one scalar per
        token (converted to float32 by value); either may be None (identity / 1).  A line pools weights[t] * table[mapping[t]].
        With device_ptr they are given as device pointers to uint32 / float32 arrays (mapping_ptr, weights_ptr, n_tokens)."""
        self.ctx = ctx
        self._h = C.c_void_p()
        if device_ptr is not None:
            if mapping is not None or weights is not None:
                raise ValueError("with device_ptr the token arrays are device pointers too: mapping_ptr / weights_ptr / n_tokens")
            indexed = mapping_ptr is not None or weights_ptr is not None
            L.check(L.lib().smt_model_create_from_device_indexed(
                ctx._h, C.c_void_p(device_ptr), L.table_dtype_code(dtype), int(V), L.DIM,
                C.c_void_p(mapping_ptr) if mapping_ptr is not None else None, C.c_void_p(weights_ptr) if weights_ptr is not None else None,
                int(n_tokens if n_tokens is not None else V) if indexed else 0, int(normalize), C.byref(self._h)))
            self.V = int(V)
        else:
            table = _table(table)
            assert table.ndim == 2
            mapping, weights, n_tok = L.token_arrays(mapping, weights, table.shape[0])
            L.check(L.lib().smt_model_create_indexed(ctx._h, L.np_ptr(table), L.table_dtype_code(table.dtype), table.shape[0],
                                                     table.shape[1], L.np_ptr(mapping), L.np_ptr(weights), n_tok, int(normalize),
                                                     C.byref(self._h)))
            self.V = table.shape[0]

    @classmethod
    def from_file(cls, ctx, path, byte_offset, V, normalize=True, dtype=np.float32, mapping=None, weights=None):
        """Stream a table [V x 256] of `dtype` that sits at `byte_offset` of a file into device memory as stored; mapping / weights
        (host arrays) as in the constructor."""
        mapping, weights, n_tok = L.token_arrays(mapping, weights, int(V))
        self = cls.__new__(cls)
        self.ctx = ctx
        self._h = C.c_void_p()
        L.check(L.lib().smt_model_create_from_file_indexed(ctx._h, str(path).encode(), int(byte_offset), L.table_dtype_code(dtype), int(V),
                                                           L.DIM, L.np_ptr(mapping), L.np_ptr(weights), n_tok, int(normalize),
                                                           C.byref(self._h)))
        self.V = int(V)
        return self

    def _token_info(self):
        n, hm, hw, nb = C.c_uint64(), C.c_int(), C.c_int(), C.c_uint64()
        L.check(L.lib().smt_model_token_info(self._h, C.byref(n), C.byref(hm), C.byref(hw), C.byref(nb)))
        return int(n.value), bool(hm.value), bool(hw.value), int(nb.value)

    @property
    def n_tokens(self):
        """token ids the model knows (a plain model: its rows)"""
        return self._token_info()[0]

    @property
    def has_mapping(self):
        return self._token_info()[1]

    @property
    def has_weights(self):
        return self._token_info()[2]

    @property
    def token_bytes(self):
        """bytes of the packed token array in device memory (8 per token; 0 for a plain model)"""
        return self._token_info()[3]

    def _info(self):
        dt, v, nbytes = C.c_int(), C.c_uint64(), C.c_uint64()
        L.check(L.lib().smt_model_info(self._h, C.byref(dt), C.byref(v), C.byref(nbytes)))
        return int(dt.value), int(v.value), int(nbytes.value)

    @property
    def table_dtype(self):
        """numpy dtype of the table in device memory"""
        return L.TABLE_NP[self._info()[0]]

    @property
    def table_bytes(self):
        return self._info()[2]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            # a handle that outlived its Context (an error path, garbage collection at interpreter exit) is dropped, not
            # destroyed: smt_model_destroy would read the freed context (the C ABI's rule is children first)
            if getattr(getattr(self, "ctx", None), "_h", None):
                L.lib().smt_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def embed(self, ids, offsets, max_tokens=2048, append_to=None, want_host=True):
        """encode_with_args' pool step for a CSR batch of token ids.  Returns
        ([n_lines x 256] f32 or None, first_row or None)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.size - 1, 0)
        out = np.empty((n, L.DIM), dtype=np.float32) if want_host else None
        first = C.c_uint64(0)
        L.check(L.lib().smt_embed(self._h, L.np_ptr(ids), L.np_ptr(offsets), n, int(max_tokens),
                                  L.np_ptr(out) if want_host else None,
                                  append_to._h if append_to is not None else None, C.byref(first)))
        return out, (int(first.value) if append_to is not None else None)

    def embed_device(self, ids_ptr, offsets_ptr, n_lines, max_tokens, out_ptr):
        L.check(L.lib().smt_embed_device(self._h, C.c_void_p(ids_ptr), C.c_void_p(offsets_ptr), int(n_lines),
                                         int(max_tokens), C.c_void_p(out_ptr)))


class _DeviceTokenizer:
    """What the device tokenizers share: the calls on the C functions smt_<_prefix>_*.  A line owns its looked-at bytes as id slots,
    and _extra_slot more."""

    _prefix = None
    _extra_slot = 0

    def _c(self, name):
        return getattr(L.lib(), "smt_%s_%s" % (self._prefix, name))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._c("destroy")(self._h)
            self._h = None

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def pack(lines):
        """(text bytes, uint64 line_begin, uint32 line_len) of lines packed back to back, no separator"""
        lines = [x.encode() if isinstance(x, str) else bytes(x) for x in lines]
        lens = np.array([len(x) for x in lines], dtype=np.uint32)
        begin = np.zeros(len(lines), dtype=np.uint64)
        if len(lines) > 1:
            begin[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        return b"".join(lines), begin, lens

    def tokenize(self, lines=None, text=None, line_begin=None, line_len=None, keep_bytes=0, max_tokens=0, drop_unk=True, ids_cap=None):
        """-> (ids uint32, offsets uint64 [n + 1], flags uint8 [n]) through smt_<family>_tokenize.  `lines` are packed back to
        back; or give text / line_begin / line_len.  ids_cap defaults to the looked-at bytes of all lines (Unigram: + one per line)."""
        if lines is not None:
            text, line_begin, line_len = self.pack(lines)
        line_begin = np.ascontiguousarray(line_begin, dtype=np.uint64)
        line_len = np.ascontiguousarray(line_len, dtype=np.uint32)
        n = len(line_len)
        if ids_cap is None:
            ids_cap = int(np.minimum(line_len, keep_bytes).sum() if keep_bytes else line_len.sum()) + n * self._extra_slot
        ids = np.zeros(max(int(ids_cap), 1), dtype=np.uint32)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        flags = np.zeros(max(n, 1), dtype=np.uint8)
        buf = C.create_string_buffer(bytes(text), max(len(text), 1))
        L.check(self._c("tokenize")(self._h, C.cast(buf, C.c_void_p), L.np_ptr(line_begin), L.np_ptr(line_len), n, int(keep_bytes),
                                    int(max_tokens), int(bool(drop_unk)), L.np_ptr(ids), int(ids_cap), L.np_ptr(offsets), L.np_ptr(flags)))
        return ids[:int(offsets[n])].copy(), offsets, flags[:n].copy()

    def scan_device(self, text_ptr, text_bytes, line_begin_ptr, line_len_ptr, n_lines, keep_bytes, max_tokens, drop_unk, counts_ptr, flags_ptr,
                    n_flagged_ptr):
        """pass 1 on raw device pointers (ints); enqueued on the context's stream"""
        vp = C.c_void_p
        L.check(self._c("scan_device")(self._h, vp(text_ptr), int(text_bytes), vp(line_begin_ptr), vp(line_len_ptr), int(n_lines),
                                       int(keep_bytes), int(max_tokens), int(bool(drop_unk)), vp(counts_ptr), vp(flags_ptr), vp(n_flagged_ptr)))

    def emit_device(self, n_lines, ids_out_ptr, ids_cap, offsets_out_ptr, patch_line_ptr=None, patch_off_ptr=None, patch_ids_ptr=None, n_patch=0,
                    n_patch_ids=0):
        """pass 2 on raw device pointers (ints); enqueued on the context's stream.  ids_cap >= min(text bytes, n_lines * keep_bytes)
        + n_patch_ids (Unigram: + n_lines)"""
        vp = C.c_void_p
        L.check(self._c("emit_device")(self._h, int(n_lines), vp(patch_line_ptr), vp(patch_off_ptr), vp(patch_ids_ptr), int(n_patch),
                                       int(n_patch_ids), vp(ids_out_ptr), int(ids_cap), vp(offsets_out_ptr)))


class WordPiece(_DeviceTokenizer):
    """The device tokenizer (smt_wordpiece): lines through BertNormalizer -> BertPreTokenizer -> WordPiece.  Pure-ASCII lines by
    default; with `codepoints` (or utf8=True beside host_tokenizer) the UTF-8 form, which covers the code points the caller states.

    WordPiece(ctx, vocab={piece: id}, unk_id=.., flags=L.WP_*, added=[..]) builds it from a vocabulary;
    WordPiece(ctx, host_tokenizer=<smt_host_tokenizer handle>) takes the device form of a loaded tokenizer.json
    (SmtError with code SMT_E_UNSUPPORTED when it has none); utf8=True takes its UTF-8 form (smt_host_tokenizer_to_device_utf8).
    codepoints: a list of (first, last, class L.WP_CP_*, output str or bytes, "" = itself) for the code points >= U+0080, sorted and
    disjoint (smt_wordpiece_create_utf8).  Calls smt_wordpiece_{tokenize,scan_device,emit_device,destroy}."""

    _prefix = "wordpiece"

    def __init__(self, ctx, vocab=None, unk_id=-1, prefix="##", max_input_chars_per_word=100,
                 flags=L.WP_NORMALIZER | L.WP_CLEAN_TEXT | L.WP_LOWERCASE, added=(), host_tokenizer=None, codepoints=None, utf8=False):
        self.ctx = ctx
        self._h = C.c_void_p()
        if host_tokenizer is not None:
            to_device = L.lib().smt_host_tokenizer_to_device_utf8 if utf8 else L.lib().smt_host_tokenizer_to_device
            L.check(to_device(host_tokenizer, ctx._h, C.byref(self._h)))
            return
        pieces = [(p.encode() if isinstance(p, str) else bytes(p), int(i)) for p, i in (vocab.items() if hasattr(vocab, "items") else vocab)]
        pool = b"".join(p for p, _ in pieces)
        off = np.zeros(len(pieces) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(p) for p, _ in pieces], dtype=np.uint64)
        ids = np.array([i for _, i in pieces], dtype=np.uint32)
        added_b = [a.encode() if isinstance(a, str) else bytes(a) for a in added]
        aoff = np.zeros(len(added_b) + 1, dtype=np.uint32)
        aoff[1:] = np.cumsum([len(a) for a in added_b], dtype=np.uint64)
        pre = prefix.encode() if isinstance(prefix, str) else bytes(prefix)
        prm = L.SmtWordpieceParams(pool, L.np_ptr(off), L.np_ptr(ids), len(pieces), pre, len(pre), int(unk_id),
                                   int(max_input_chars_per_word), int(flags), b"".join(added_b), L.np_ptr(aoff), len(added_b))
        if codepoints is None:
            L.check(L.lib().smt_wordpiece_create(ctx._h, C.byref(prm), C.byref(self._h)))
            return
        outs = [(o.encode() if isinstance(o, str) else bytes(o)) for _, _, _, o in codepoints]
        first = np.array([c[0] for c in codepoints], dtype=np.uint32)
        last = np.array([c[1] for c in codepoints], dtype=np.uint32)
        cls = np.array([c[2] for c in codepoints], dtype=np.uint8)
        ooff = np.zeros(len(outs) + 1, dtype=np.uint32)
        ooff[1:] = np.cumsum([len(o) for o in outs], dtype=np.uint64)
        cps = L.SmtWordpieceCodepoints(L.np_ptr(first), L.np_ptr(last), L.np_ptr(cls), b"".join(outs), L.np_ptr(ooff), len(outs))
        L.check(L.lib().smt_wordpiece_create_utf8(ctx._h, C.byref(prm), C.byref(cps), C.byref(self._h)))

    def info(self):
        """(bytes of the whole device table, bytes of its code-point part -- 0 for the ASCII form --, True for the UTF-8 form)"""
        table, cps, utf8 = C.c_uint64(), C.c_uint64(), C.c_int()
        L.check(L.lib().smt_wordpiece_info(self._h, C.byref(table), C.byref(cps), C.byref(utf8)))
        return int(table.value), int(cps.value), bool(utf8.value)


class Unigram(_DeviceTokenizer):
    """The device tokenizer (smt_unigram): lines through a per-character normalizer -> Metaspace -> Unigram.  Pure-ASCII lines by
    default; with `codepoints` (or utf8=True beside host_tokenizer) the UTF-8 form, which covers the code points the caller states.

    Unigram(ctx, vocab=[(piece, score), ..], unk_id=.., replacement="\u2581", prepend="always", byte_map=.., added=[..]) builds it
    from a vocabulary (the id of a piece is its index; unk_score defaults to the lowest score - 10; byte_map: 128 entries, the byte
    a byte becomes or 0xFF for dropped, default the identity); Unigram(ctx, host_tokenizer=<smt_host_tokenizer handle>) takes the
    device form of a loaded tokenizer.json (SmtError with code SMT_E_UNSUPPORTED when it has none); utf8=True takes its UTF-8 form
    (smt_host_tokenizer_to_device_unigram_utf8).  codepoints: a list of (first, last, class L.WP_CP_*, output str or bytes, "" =
    itself) for the code points >= U+0080, sorted and disjoint (smt_unigram_create_utf8; no class ALONE; the replacement's own code
    point is a SPACE).  Calls smt_unigram_{tokenize,scan_device,emit_device,destroy}; a line can hold one token more than looked-at
    bytes."""

    _prefix, _extra_slot = "unigram", 1

    def __init__(self, ctx, vocab=None, unk_id=-1, replacement="\u2581", prepend="always", byte_map=None, added=(), unk_score=None,
                 host_tokenizer=None, codepoints=None, utf8=False):
        self.ctx = ctx
        self._h = C.c_void_p()
        if host_tokenizer is not None:
            to_device = L.lib().smt_host_tokenizer_to_device_unigram_utf8 if utf8 else L.lib().smt_host_tokenizer_to_device_unigram
            L.check(to_device(host_tokenizer, ctx._h, C.byref(self._h)))
            return
        pieces = [(p.encode() if isinstance(p, str) else bytes(p), float(s)) for p, s in vocab]
        pool = b"".join(p for p, _ in pieces)
        off = np.zeros(len(pieces) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(p) for p, _ in pieces], dtype=np.uint64)
        ids = np.arange(len(pieces), dtype=np.uint32)
        scores = np.array([s for _, s in pieces], dtype=np.float64)
        if unk_score is None:
            unk_score = (float(scores.min()) if len(pieces) else 0.0) - 10.0
        added_b = [a.encode() if isinstance(a, str) else bytes(a) for a in added]
        aoff = np.zeros(len(added_b) + 1, dtype=np.uint32)
        aoff[1:] = np.cumsum([len(a) for a in added_b], dtype=np.uint64)
        rep = replacement.encode() if isinstance(replacement, str) else bytes(replacement)
        bmap = np.arange(128, dtype=np.uint8) if byte_map is None else np.ascontiguousarray(byte_map, dtype=np.uint8)
        if bmap.size != 128:
            raise ValueError("byte_map has 128 entries")
        prm = L.SmtUnigramParams(pool, L.np_ptr(off), L.np_ptr(ids), len(pieces), L.np_ptr(scores), float(unk_score), int(unk_id), rep,
                                 len(rep), int(L.UG_PREPEND.get(prepend, prepend)), L.np_ptr(bmap), b"".join(added_b), L.np_ptr(aoff),
                                 len(added_b))
        if codepoints is None and not utf8:
            L.check(L.lib().smt_unigram_create(ctx._h, C.byref(prm), C.byref(self._h)))
            return
        codepoints = list(codepoints or [])
        outs = [(o.encode() if isinstance(o, str) else bytes(o)) for _, _, _, o in codepoints]
        first = np.array([c[0] for c in codepoints], dtype=np.uint32)
        last = np.array([c[1] for c in codepoints], dtype=np.uint32)
        cls = np.array([c[2] for c in codepoints], dtype=np.uint8)
        ooff = np.zeros(len(outs) + 1, dtype=np.uint32)
        ooff[1:] = np.cumsum([len(o) for o in outs], dtype=np.uint64)
        cps = L.SmtWordpieceCodepoints(L.np_ptr(first), L.np_ptr(last), L.np_ptr(cls), b"".join(outs), L.np_ptr(ooff), len(outs))
        L.check(L.lib().smt_unigram_create_utf8(ctx._h, C.byref(prm), C.byref(cps), C.byref(self._h)))

    def info(self):
        """(bytes of the whole device table, bytes of its code-point part -- 0 for the ASCII form --, True for the UTF-8 form)"""
        table, cps, utf8 = C.c_uint64(), C.c_uint64(), C.c_int()
        L.check(L.lib().smt_unigram_info(self._h, C.byref(table), C.byref(cps), C.byref(utf8)))
        return int(table.value), int(cps.value), bool(utf8.value)

    def set_long_pieces(self, n):
        """0 (the default): a piece over L.UG_MAX_WORD raw bytes flags its line; L.UG_MAX_WORD < n <= L.UG_MAX_LONG: pieces up to n
        raw bytes are tokenized on the device too, from the next scan on (smt_unigram_set_long_pieces)"""
        L.check(L.lib().smt_unigram_set_long_pieces(self._h, int(n)))

    def set_space_rules(self, collapse_runs, drop_trailing):
        """the space rules of an XLM-R-style chain, from the next scan on (smt_unigram_set_space_rules): collapse_runs -- a space behind
        a space starts no piece; drop_trailing -- the replacement alone at a line's end emits nothing.  False, False: the default"""
        L.check(L.lib().smt_unigram_set_space_rules(self._h, int(bool(collapse_runs)), int(bool(drop_trailing))))

    def set_long_rules(self, on):
        """True: while a space rule is on and set_long_pieces set a limit, pieces over L.UG_MAX_WORD raw bytes are tokenized on the
        device too instead of flagging their lines, from the next scan on (smt_unigram_set_long_rules).  False: the default"""
        L.check(L.lib().smt_unigram_set_long_rules(self._h, int(bool(on))))

    def long_stats(self):
        """(long pieces the last scan's long-piece kernel tokenized, their raw bytes); waits for the stream (smt_unigram_long_stats)"""
        pieces, raw = C.c_uint64(), C.c_uint64()
        L.check(L.lib().smt_unigram_long_stats(self._h, C.byref(pieces), C.byref(raw)))
        return int(pieces.value), int(raw.value)


class Lower:
    """Lower-casing of packed UTF-8 lines on the device (smt_lower): line by line the bytes of the host layer's to_lowercase, lines
    with ill-formed UTF-8 flagged and copied unchanged.

    Lower(ctx) uses the library's own tables (Rust's str::to_lowercase).  Lower(ctx, tables=dict(runs=[(first, last, delta, stride)],
    multi=[(cp, [to, ..])] or [(cp, n, [to, ..])], cased=[(first, last)], ignorable=[(first, last)], final_sigma=bool)) states them:
    code points >= U+0080, every list sorted (smt_lower_tables_check).  Calls smt_lower_{create,device,lines,destroy}."""

    def __init__(self, ctx, tables=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        if tables is None:
            L.check(L.lib().smt_lower_create(ctx._h, None, C.byref(self._h)))
            return
        st, _keep = self.tables_struct(tables)
        L.check(L.lib().smt_lower_create(ctx._h, C.byref(st), C.byref(self._h)))

    @staticmethod
    def tables_struct(tables):
        """(SmtLowerTables, the arrays it points into) of a tables dict"""
        runs = list(tables.get("runs", ()))
        multi = [(m[0], len(m[1]), m[1]) if len(m) == 2 else tuple(m) for m in tables.get("multi", ())]
        cased = list(tables.get("cased", ()))
        ign = list(tables.get("ignorable", ()))
        to = np.zeros(max(len(multi), 1) * 3, dtype=np.uint32)
        for i, (_, _, t) in enumerate(multi):
            to[i * 3:i * 3 + min(len(t), 3)] = list(t)[:3]
        keep = [np.array([r[0] for r in runs], dtype=np.uint32), np.array([r[1] for r in runs], dtype=np.uint32),
                np.array([r[2] for r in runs], dtype=np.int32), np.array([r[3] for r in runs], dtype=np.uint32),
                np.array([m[0] for m in multi], dtype=np.uint32), np.array([m[1] for m in multi], dtype=np.uint32), to,
                np.array([r[0] for r in cased], dtype=np.uint32), np.array([r[1] for r in cased], dtype=np.uint32),
                np.array([r[0] for r in ign], dtype=np.uint32), np.array([r[1] for r in ign], dtype=np.uint32)]
        p = [L.np_ptr(a) for a in keep]
        st = L.SmtLowerTables(p[0], p[1], p[2], p[3], len(runs), p[4], p[5], p[6], len(multi), p[7], p[8], len(cased), p[9], p[10], len(ign),
                              1 if tables.get("final_sigma", False) else 0)
        return st, keep

    @staticmethod
    def check_tables(tables):
        """smt_lower_tables_check on a tables dict: SMT_OK or SMT_E_INVALID (smt_last_error says why); needs no device"""
        st, _keep = Lower.tables_struct(tables)
        return L.lib().smt_lower_tables_check(C.byref(st))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            L.lib().smt_lower_destroy(self._h)
            self._h = None

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass

    pack = staticmethod(_DeviceTokenizer.pack)

    def lower(self, lines=None, text=None, line_begin=None, line_len=None, out_cap=None):
        """-> (out text bytes, out_begin uint64 [n + 1], out_len uint32 [n], flags uint8 [n]) through smt_lower_lines.  `lines` are packed back
        to back; or give text / line_begin / line_len.  out_cap defaults to the bound, 1.5 x the text up to the last line's end."""
        if lines is not None:
            text, line_begin, line_len = self.pack(lines)
        line_begin = np.ascontiguousarray(line_begin, dtype=np.uint64)
        line_len = np.ascontiguousarray(line_len, dtype=np.uint32)
        n = len(line_len)
        text_bytes = int(line_begin[-1]) + int(line_len[-1]) if n else 0
        if out_cap is None:
            out_cap = text_bytes + text_bytes // 2
        out = np.zeros(max(int(out_cap), 1), dtype=np.uint8)
        out_begin = np.zeros(n + 1, dtype=np.uint64)
        out_len = np.zeros(max(n, 1), dtype=np.uint32)
        flags = np.zeros(max(n, 1), dtype=np.uint8)
        buf = C.create_string_buffer(bytes(text), max(len(text), 1))
        L.check(L.lib().smt_lower_lines(self._h, C.cast(buf, C.c_void_p), L.np_ptr(line_begin), L.np_ptr(line_len), n, L.np_ptr(out), int(out_cap),
                                  L.np_ptr(out_begin), L.np_ptr(out_len), L.np_ptr(flags)))
        return out[:int(out_begin[n])].tobytes(), out_begin, out_len[:n].copy(), flags[:n].copy()

    def lower_device(self, text_ptr, text_bytes, line_begin_ptr, line_len_ptr, n_lines, out_text_ptr, out_cap, out_begin_ptr, out_len_ptr,
                     flags_ptr, n_flagged_ptr):
        """smt_lower_device on raw device pointers (ints); enqueued on the context's stream"""
        vp = C.c_void_p
        L.check(L.lib().smt_lower_device(self._h, vp(text_ptr), int(text_bytes), vp(line_begin_ptr), vp(line_len_ptr), int(n_lines),
                                         vp(out_text_ptr), int(out_cap), vp(out_begin_ptr), vp(out_len_ptr), vp(flags_ptr), vp(n_flagged_ptr)))


class Corpus:
    """Row-major f32 [rows x 256] matrix resident in HBM (smt_corpus)."""

    def __init__(self, ctx, capacity_rows=0, device_ptr=None, rows=None, _handle=None, _borrowed=False):
        self.ctx = ctx
        self._h = C.c_void_p()
        self._borrowed = _borrowed     # a shard owned by a ShardedCorpus
        if _handle is not None:
            self._h = _handle
        elif device_ptr is not None:
            L.check(L.lib().smt_corpus_from_device(ctx._h, C.c_void_p(device_ptr), int(rows), L.DIM, C.byref(self._h)))
        else:
            L.check(L.lib().smt_corpus_create(ctx._h, L.DIM, int(capacity_rows), C.byref(self._h)))

    @classmethod
    def load(cls, ctx, path):
        h = C.c_void_p()
        L.check(L.lib().smt_corpus_load(ctx._h, str(path).encode(), C.byref(h)))
        return cls(ctx, _handle=h)

    def save(self, path):
        L.check(L.lib().smt_corpus_save(self._h, str(path).encode()))

    def append_to_file(self, path, rows_on_disk):
        L.check(L.lib().smt_corpus_append_to_file(self._h, str(path).encode(), int(rows_on_disk)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            if not getattr(self, "_borrowed", False) and getattr(getattr(self, "ctx", None), "_h", None):   # (see Model.close)
                L.lib().smt_corpus_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def rows(self):
        return int(L.lib().smt_corpus_rows(self._h))

    def __len__(self):
        return self.rows

    def append(self, rows):
        rows = _f32c(rows).reshape(-1, L.DIM)
        first = C.c_uint64(0)
        L.check(L.lib().smt_corpus_append_host(self._h, L.np_ptr(rows), rows.shape[0], C.byref(first)))
        return int(first.value)

    def write_rows(self, first_row, rows):
        rows = _f32c(rows).reshape(-1, L.DIM)
        L.check(L.lib().smt_corpus_write_rows(self._h, int(first_row), L.np_ptr(rows), rows.shape[0]))

    def read_rows(self, first_row, n_rows):
        out = np.empty((int(n_rows), L.DIM), dtype=np.float32)
        L.check(L.lib().smt_corpus_read_rows(self._h, int(first_row), int(n_rows), L.np_ptr(out)))
        return out

    def truncate(self, n_rows):
        L.check(L.lib().smt_corpus_truncate(self._h, int(n_rows)))

    def compact(self, ranges):
        """smt_corpus_compact: keep exactly the rows inside `ranges` ([(begin, end), ...] sorted, disjoint) and close the gaps in place,
        on the device.  Returns the rows that moved (the kept rows behind the first dropped one)."""
        rng, n = _ranges_arg(list(ranges))
        moved = C.c_uint64(0)
        L.check(L.lib().smt_corpus_compact(self._h, C.cast(rng, C.c_void_p), n, C.byref(moved)))
        return int(moved.value)

    def prepack(self, enable=True):
        """smt_corpus_prepack: build (or drop) the fp16 operand image the batched searches read -- half the bytes per row.  For a
        corpus adopted from device memory this is the only way to get one; call it again after changing rows."""
        L.check(L.lib().smt_corpus_prepack(self._h, 1 if enable else 0))

    @property
    def image_bytes(self):
        return int(L.lib().smt_corpus_image_bytes(self._h))

    def image_tile(self, tile):
        """Test hook (smt_debug_image_tile): (the 16 KiB of tile `tile` of the up-to-date operand image as bytes, its zero-row mask)."""
        buf = np.empty(16384, dtype=np.uint8)
        zm = C.c_uint32(0)
        L.check(L.lib().smt_debug_image_tile(self._h, int(tile), L.np_ptr(buf), C.byref(zm)))
        return buf.tobytes(), int(zm.value)

    def debug_batched_scores(self, queries, first_row=0, n_rows=None):
        """Test hook (smt_debug_batched_scores): the f32 distances the batched kernels nominate candidates with,
        float32 [n_rows, nq]."""
        q = _f32c(queries).reshape(-1, L.DIM)
        n_rows = self.rows - first_row if n_rows is None else int(n_rows)
        out = np.empty((n_rows, 32), dtype=np.float32)
        L.check(L.lib().smt_debug_batched_scores(self._h, L.np_ptr(q), q.shape[0], int(first_row), n_rows, L.np_ptr(out)))
        return out[:, :q.shape[0]].copy()

    def debug_nominations(self, queries, tau=None, buffered=False, ranges=None, top_k=10, level=None):
        """Test hook (smt_debug_nominations): what the PRODUCTION kernels of a batched top_k call over this corpus nominate in one
        level over all tiles, under the distance thresholds tau (one per query; None = +inf, admit everything).  Returns
        (dist float32 [rows, nq], NaN where the pair was not nominated; hits uint32 [rows, nq], the keys that named the pair;
        counts uint32 [ceil(nq / 32) * 32], raw per query, padding queries included; route, see the header).
        level = (stride, skip, tile_begin, tile_end): that level launch instead (smt_debug_level_nominations)."""
        q = _f32c(queries).reshape(-1, L.DIM)
        nq = q.shape[0]
        t = np.full(nq, np.inf, dtype=np.float32) if tau is None else np.ascontiguousarray(tau, dtype=np.float32).reshape(nq)
        rng, n_rng = _ranges_arg(ranges)
        rows = self.rows
        dist = np.empty((rows, nq), dtype=np.float32)
        hits = np.empty((rows, nq), dtype=np.uint32)
        counts = np.empty((nq + 31) // 32 * 32, dtype=np.uint32)
        route = C.c_uint32(0)
        rng_p = C.cast(rng, C.c_void_p) if rng is not None else None
        if level is None:
            L.check(L.lib().smt_debug_nominations(self._h, L.np_ptr(q), nq, int(top_k), rng_p, n_rng, L.np_ptr(t), int(bool(buffered)),
                                                  L.np_ptr(dist), L.np_ptr(hits), L.np_ptr(counts), C.byref(route)))
        else:
            stride, skip, tile_begin, tile_end = (int(v) for v in level)
            L.check(L.lib().smt_debug_level_nominations(self._h, L.np_ptr(q), nq, int(top_k), rng_p, n_rng, L.np_ptr(t), int(bool(buffered)),
                                                        stride, skip, tile_begin, tile_end, L.np_ptr(dist), L.np_ptr(hits),
                                                        L.np_ptr(counts), C.byref(route)))
        return dist, hits, counts, int(route.value)

    def debug_bootstrap_minima(self, queries, ranges=None, top_k=10):
        """Test hook (smt_debug_bootstrap_minima): the bootstrap launch of the batched top_k call over this corpus.  Returns
        (tile_min float32 [slots, ceil(nq / 32) * 32], the bootstrap stride, route)."""
        q = _f32c(queries).reshape(-1, L.DIM)
        nq = q.shape[0]
        nq_pad = (nq + 31) // 32 * 32
        rng, n_rng = _ranges_arg(ranges)
        out = np.empty((1024, nq_pad), dtype=np.float32)
        slots, stride, route = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
        L.check(L.lib().smt_debug_bootstrap_minima(self._h, L.np_ptr(q), nq, int(top_k), C.cast(rng, C.c_void_p) if rng is not None else None,
                                                   n_rng, L.np_ptr(out), C.byref(slots), C.byref(stride), C.byref(route)))
        return out[:int(slots.value)].copy(), int(stride.value), int(route.value)

    def debug_scan_lists(self, queries, top_k, ranges=None, cap_keys=None):
        """Test hook (smt_debug_scan_lists): the block lists the scan stage writes for a synchronous top_k call of 1..8 queries under
        the current tuning.  Returns (keys uint64 [nq + 1, blocks, k'], the last set the untouched guard; route, see the header).
        cap_keys: the capacity handed to the library (default: the largest a call can need)."""
        q = _f32c(queries).reshape(-1, L.DIM)
        nq = q.shape[0]
        rng, n_rng = _ranges_arg(ranges)
        cap = (nq + 1) * 512 * 64 if cap_keys is None else int(cap_keys)
        out = np.empty(max(cap, 1), dtype=np.uint64)
        blocks, kp, route = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        L.check(L.lib().smt_debug_scan_lists(self._h, L.np_ptr(q), nq, int(top_k), C.cast(rng, C.c_void_p) if rng is not None else None,
                                             n_rng, L.np_ptr(out), cap, C.byref(blocks), C.byref(kp), C.byref(route)))
        b, k = int(blocks.value), int(kp.value)
        return out[:(nq + 1) * b * k].reshape(nq + 1, b, k).copy(), int(route.value)

    def debug_select_lists(self, queries_ptr, nq, lists_ptr, n_lists, kp, k_out, out_rows_ptr, out_dist_ptr, list_stride=0, out_stride=0,
                           ws_threshold=None, row_base=0, f32_err=0.0, overflow_ptr=None, out_counts_ptr=None, out_uncertain_ptr=None,
                           out_status_ptr=None):
        """Test hook (smt_debug_select_lists): the select stage on constructed block lists [nq][n_lists][kp] of keys (device pointers,
        asynchronous on the context's stream).  ws_threshold: the score threshold, None = none.  Every row a key names must lie below
        self.rows."""
        opt = lambda p: C.c_void_p(int(p)) if p else None
        L.check(L.lib().smt_debug_select_lists(self._h, opt(queries_ptr), int(nq), opt(lists_ptr), int(list_stride), int(n_lists), int(kp),
                                               int(k_out), 0 if ws_threshold is None else 1, 0.0 if ws_threshold is None else float(ws_threshold),
                                               int(row_base), float(f32_err), opt(overflow_ptr), int(out_stride), opt(out_rows_ptr),
                                               opt(out_dist_ptr), opt(out_counts_ptr), opt(out_uncertain_ptr), opt(out_status_ptr)))

    def search(self, queries, top_k=3, max_distance=None, mode=L.MODE_DOCUMENTS, ranges=None, row_base=0,
               out_cap=None):
        """Returns a list (one per query) of (rows uint64[n], dist float64[n]).

        mode/threshold semantics: see include/semtools_hip.h (smt_search)."""
        q = _f32c(queries).reshape(-1, L.DIM)
        nq = q.shape[0]
        if out_cap is None:
            out_cap = max(int(top_k), 1)
            if max_distance is not None and mode == L.MODE_DOCUMENTS:
                out_cap = max(self.rows, 1)
        rng, n_rng = _ranges_arg(ranges)
        while True:
            out_rows = np.empty((nq, out_cap), dtype=np.uint64)
            out_dist = np.empty((nq, out_cap), dtype=np.float64)
            counts = np.zeros(nq, dtype=np.uint64)
            rc = L.lib().smt_search(self._h, L.np_ptr(q), nq, int(top_k),
                                    float("nan") if max_distance is None else float(max_distance), int(mode),
                                    C.cast(rng, C.c_void_p) if rng is not None else None, n_rng, int(row_base),
                                    L.np_ptr(out_rows), L.np_ptr(out_dist), L.np_ptr(counts), int(out_cap))
            if rc == L.SMT_E_TRUNCATED:
                out_cap = int(counts.max())
                continue
            L.check(rc)
            break
        return [(out_rows[i, :int(counts[i])].copy(), out_dist[i, :int(counts[i])].copy()) for i in range(nq)]

    def range_sets(self):
        """(kept, hits, builds) of the range lists this corpus keeps on the device (smt_debug_range_sets)."""
        v = [C.c_uint64() for _ in range(3)]
        L.check(L.lib().smt_debug_range_sets(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def search_topk_device(self, queries_ptr, nq, top_k, row_base, out_rows_ptr, out_dist_ptr, out_status_ptr=None):
        """out_status_ptr: device-addressable uint32[nq] receiving the per-query verdict (smt_search_topk_device_ex: 0 proved exact,
        1 certificate failed, 2 candidate buffer overflowed, 3 = SMT_STATUS_INVALID_QUERY: the query lies outside the domain), or None."""
        if out_status_ptr:
            L.check(L.lib().smt_search_topk_device_ex(self._h, C.c_void_p(queries_ptr), int(nq), int(top_k), int(row_base),
                                                      C.c_void_p(out_rows_ptr), C.c_void_p(out_dist_ptr), C.c_void_p(int(out_status_ptr))))
            return
        L.check(L.lib().smt_search_topk_device(self._h, C.c_void_p(queries_ptr), int(nq), int(top_k), int(row_base),
                                               C.c_void_p(out_rows_ptr), C.c_void_p(out_dist_ptr)))


class IvfPq:
    """IVF-PQ index over a resident Corpus (smt_ivfpq).  Approximate top-k membership, exact distances."""

    def __init__(self, corpus, nlist=4096, train_iters=10, train_sample=0, local_pca=False, _path=None):
        self.corpus = corpus
        self._h = C.c_void_p()
        if _path is not None:
            L.check(L.lib().smt_ivfpq_load(corpus._h, str(_path).encode(), C.byref(self._h)))
            return
        prm = L.SmtIvfPqParams(int(nlist), 32, 8, int(train_iters), int(train_sample), 0, 1 if local_pca else 0)
        L.check(L.lib().smt_ivfpq_build(corpus._h, C.byref(prm), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            L.lib().smt_ivfpq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def save(self, path):
        L.check(L.lib().smt_ivfpq_save(self._h, str(path).encode()))

    def append(self):
        """Take in the rows appended to the corpus since the build (no retraining).  Returns how many."""
        n = C.c_uint64()
        L.check(L.lib().smt_ivfpq_append(self._h, C.byref(n)))
        return int(n.value)

    def compact(self, ranges):
        """smt_ivfpq_compact: Corpus.compact(ranges) on the index's corpus, with the index carried along instead of rebuilt (dead
        entries dropped, kept ones renamed, quantisers untouched).  Returns (rows_moved, entries_dropped)."""
        rng, n = _ranges_arg(list(ranges))
        moved, dropped = C.c_uint64(0), C.c_uint64(0)
        L.check(L.lib().smt_ivfpq_compact(self._h, C.cast(rng, C.c_void_p), n, C.byref(moved), C.byref(dropped)))
        return int(moved.value), int(dropped.value)

    @classmethod
    def load(cls, corpus, path):
        """Restore an index saved beside `corpus` (fails unless the row count matches)."""
        return cls(corpus, _path=path)

    def info(self):
        n, nl, nb = C.c_uint64(), C.c_uint32(), C.c_uint64()
        ms = (C.c_double * 4)()
        L.check(L.lib().smt_ivfpq_info(self._h, C.byref(n), C.byref(nl), C.byref(nb), ms))
        return dict(rows=int(n.value), nlist=int(nl.value), index_bytes=int(nb.value),
                    build_ms=dict(coarse_kmeans=ms[0], assign_all=ms[1], pq_train=ms[2], sort_encode=ms[3]))

    def list_sizes(self):
        out = np.empty(self.info()["nlist"], dtype=np.uint64)
        L.check(L.lib().smt_ivfpq_list_sizes(self._h, L.np_ptr(out)))
        return out

    def search(self, queries, top_k=10, nprobe=32, rerank=0, row_base=0, ranges=None, wide=False):
        """ranges: search inside these corpus rows only (smt_ivfpq_search_ranges: [(begin, end)] sorted and disjoint, or a
        PackedRanges; an empty list is the unfiltered search); None calls smt_ivfpq_search.
        wide: through smt_ivfpq_search_wide, which takes top_k up to 1024 (top_k <= 56: the same bytes as without it); there an
        empty list of ranges is an empty filter, and the answer is empty."""
        q = _f32c(queries).reshape(-1, L.DIM)
        nq = q.shape[0]
        cap = max(int(top_k), 1)
        out_rows = np.empty((nq, cap), dtype=np.uint64)
        out_dist = np.empty((nq, cap), dtype=np.float64)
        counts = np.zeros(nq, dtype=np.uint64)
        if wide:
            rng, n_rng = _ranges_arg(ranges)
            L.check(L.lib().smt_ivfpq_search_wide(self._h, L.np_ptr(q), nq, int(top_k), int(nprobe), int(rerank),
                                                  C.cast(rng, C.c_void_p) if rng is not None else None, n_rng, int(row_base),
                                                  L.np_ptr(out_rows), L.np_ptr(out_dist), L.np_ptr(counts), cap))
        elif ranges is None:
            L.check(L.lib().smt_ivfpq_search(self._h, L.np_ptr(q), nq, int(top_k), int(nprobe), int(rerank), int(row_base),
                                             L.np_ptr(out_rows), L.np_ptr(out_dist), L.np_ptr(counts), cap))
        else:
            rng, n_rng = _ranges_arg(ranges)
            L.check(L.lib().smt_ivfpq_search_ranges(self._h, L.np_ptr(q), nq, int(top_k), int(nprobe), int(rerank),
                                                    C.cast(rng, C.c_void_p), n_rng, int(row_base),
                                                    L.np_ptr(out_rows), L.np_ptr(out_dist), L.np_ptr(counts), cap))
        return [(out_rows[i, :int(counts[i])].copy(), out_dist[i, :int(counts[i])].copy()) for i in range(nq)]

    def search_device(self, queries_ptr, nq, top_k, nprobe, rerank, row_base, out_rows_ptr, out_dist_ptr, ranges=None, wide=False):
        """Device-resident form (raw pointers; asynchronous on the context's stream).  ranges (host side, as in search): inside
        these rows only, through smt_ivfpq_search_ranges_device.  wide: smt_ivfpq_search_wide_device (top_k up to 1024)."""
        if wide:
            rng, n_rng = _ranges_arg(ranges)
            L.check(L.lib().smt_ivfpq_search_wide_device(self._h, C.c_void_p(queries_ptr), int(nq), int(top_k), int(nprobe), int(rerank),
                                                         C.cast(rng, C.c_void_p) if rng is not None else None, n_rng, int(row_base),
                                                         C.c_void_p(out_rows_ptr), C.c_void_p(out_dist_ptr)))
            return
        if ranges is None:
            L.check(L.lib().smt_ivfpq_search_device(self._h, C.c_void_p(queries_ptr), int(nq), int(top_k), int(nprobe), int(rerank),
                                                    int(row_base), C.c_void_p(out_rows_ptr), C.c_void_p(out_dist_ptr)))
            return
        rng, n_rng = _ranges_arg(ranges)
        L.check(L.lib().smt_ivfpq_search_ranges_device(self._h, C.c_void_p(queries_ptr), int(nq), int(top_k), int(nprobe), int(rerank),
                                                       C.cast(rng, C.c_void_p), n_rng, int(row_base),
                                                       C.c_void_p(out_rows_ptr), C.c_void_p(out_dist_ptr)))


class PackedRanges:
    """Row ranges marshalled once (a caller that searches the same document subset again and again: bench.py's workspace leg)."""

    def __init__(self, ranges):
        self.arr, self.n = _ranges_arg(list(ranges))


def _ranges_arg(ranges):
    if ranges is None:
        return None, 0
    if isinstance(ranges, PackedRanges):
        return ranges.arr, ranges.n
    n = len(ranges)
    rng = (L.SmtRange * max(n, 1))()
    for i, (b, e) in enumerate(ranges):
        rng[i].begin, rng[i].end = int(b), int(e)
    return rng, n


class Group:
    """A group of GPUs behind the C ABI (smt_group): one context + stream per device and one RCCL communicator.

    Group(devices=[0, 1, ...])                 single process drives every listed GPU (ncclCommInitAll)
    Group.from_rank(device, rank, n, id)       one rank per process; `id` = Group.unique_id() made on rank 0 and
                                               broadcast by the host (see semtools_amd.dist.group_from_torch)"""

    def __init__(self, devices=None, _handle=None):
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            if devices is None:
                n = L.lib().smt_device_count()
                L.check(min(n, 0))
                devices = range(n)
            devs = list(devices)
            arr = (C.c_int * len(devs))(*devs)
            L.check(L.lib().smt_group_create(arr, len(devs), C.byref(self._h)))
        self._ctx = {}

    @classmethod
    def logical(cls, device, n_shards):
        """n logical ranks on one device (peer reads or device copies instead of RCCL): the sharded path on a 1-GPU box."""
        h = C.c_void_p()
        L.check(L.lib().smt_group_create_logical(int(device), int(n_shards), C.byref(h)))
        return cls(_handle=h)

    @classmethod
    def from_ctx(cls, ctx):
        """A one-rank group around an existing Context: every sharded call forwards to its single-GPU counterpart."""
        h = C.c_void_p()
        L.check(L.lib().smt_group_from_ctx(ctx._h, C.byref(h)))
        g = cls(_handle=h)
        g._keep = ctx   # the context must outlive the group
        return g

    @classmethod
    def from_spec(cls, spec):
        """"0,1,2" / "all" / "<device>:<logical shards>" / "<device>" -- what the CLI reads from $SEMTOOLS_DEVICES."""
        h = C.c_void_p()
        L.check(L.lib().smt_host_group_from_spec(str(spec).encode(), C.byref(h)))
        return cls(_handle=h)

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * L.UNIQUE_ID_BYTES)()
        L.check(L.lib().smt_group_unique_id(buf))
        return bytes(buf)

    @classmethod
    def from_rank(cls, device, rank, n_ranks, unique_id):
        assert len(unique_id) == L.UNIQUE_ID_BYTES
        h = C.c_void_p()
        buf = (C.c_ubyte * L.UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        L.check(L.lib().smt_group_create_rank(int(device), int(rank), int(n_ranks), buf, C.byref(h)))
        return cls(_handle=h)

    def info(self):
        v = [C.c_int() for _ in range(5)]
        L.check(L.lib().smt_group_info(self._h, *[C.byref(x) for x in v]))
        return dict(n_ranks=v[0].value, n_local=v[1].value, first_rank=v[2].value, rccl_ranks=v[3].value,
                    rccl_version=v[4].value)

    def ctx(self, local_index=0):
        """The library-owned Context of local device i (tuning keys, profiling, Model(...) on that GPU)."""
        if local_index not in self._ctx:
            h = L.lib().smt_group_ctx(self._h, int(local_index))
            if not h:
                raise IndexError(local_index)
            self._ctx[local_index] = Context(_borrowed=h)
        return self._ctx[local_index]

    def synchronize(self):
        L.check(L.lib().smt_group_synchronize(self._h))

    @property
    def transport(self):
        """"peer" (k-lists read in place by the merging device: the default of one-process groups), "rccl" or "copy"."""
        t = L.lib().smt_group_transport(self._h)
        L.check(min(t, 0))
        return L.TRANSPORT_NAMES[t]

    def set_transport(self, name):
        code = {v: k for k, v in L.TRANSPORT_NAMES.items()}[name]
        L.check(L.lib().smt_group_set_transport(self._h, code))

    def barrier(self):
        L.check(L.lib().smt_group_barrier(self._h))

    def debug_fail_next(self, where, code):
        """Test hook (smt_debug_group_fail_next): the next local step of kind `where` on this process's ranks fails with `code`."""
        L.check(L.lib().smt_debug_group_fail_next(self._h, int(where), int(code)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            L.lib().smt_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardedModel:
    """The embedding table replicated on every GPU of a Group; embed() = Model.embed with the lines dealt over the ranks."""

    def __init__(self, group, table, normalize=True, mapping=None, weights=None):
        self.group = group
        self._h = C.c_void_p()
        table = _table(table).reshape(-1, L.DIM)
        self.V = table.shape[0]
        mapping, weights, n_tok = L.token_arrays(mapping, weights, self.V)
        L.check(L.lib().smt_sharded_model_create_indexed(group._h, L.np_ptr(table), L.table_dtype_code(table.dtype), self.V, L.DIM,
                                                         L.np_ptr(mapping), L.np_ptr(weights), n_tok, int(normalize), C.byref(self._h)))

    def _token_info(self):
        n, hm, hw, nb = C.c_uint64(), C.c_int(), C.c_int(), C.c_uint64()
        L.check(L.lib().smt_sharded_model_token_info(self._h, C.byref(n), C.byref(hm), C.byref(hw), C.byref(nb)))
        return int(n.value), bool(hm.value), bool(hw.value), int(nb.value)

    n_tokens = property(lambda self: self._token_info()[0])
    has_mapping = property(lambda self: self._token_info()[1])
    has_weights = property(lambda self: self._token_info()[2])
    token_bytes = property(lambda self: self._token_info()[3], doc="bytes of the token array, per replica")

    @property
    def table_bytes(self):
        """bytes of the table in device memory, per replica"""
        nbytes = C.c_uint64()
        L.check(L.lib().smt_sharded_model_info(self._h, None, None, C.byref(nbytes)))
        return int(nbytes.value)

    def close(self):
        if _open(self):
            if _open(self.group):
                L.lib().smt_sharded_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def embed(self, ids, offsets, max_tokens=2048, append_to=None, want_host=True):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        out = np.empty((n, L.DIM), dtype=np.float32) if want_host else None
        first = C.c_uint64(0)
        L.check(L.lib().smt_sharded_embed(self._h, L.np_ptr(ids) if len(ids) else None, L.np_ptr(offsets), n, int(max_tokens),
                                          L.np_ptr(out) if out is not None else None,
                                          append_to._h if append_to is not None else None, C.byref(first)))
        return out, int(first.value)


class ShardedCorpus:
    """Corpus row-sharded over a Group (smt_sharded_corpus): cut into ceil(N / n_ranks)-row ranges when made in one go,
    dealt over the ranks append by append when it grows.  Global row == insertion order either way.
    search() has Corpus.search's arguments and returns the same answer as the unsharded matrix would."""

    def __init__(self, group, rows=None, device_ptrs=None, shard_rows=None, path=None, layout=None, empty=False):
        self.group = group
        self._h = C.c_void_p()
        if empty:
            L.check(L.lib().smt_sharded_corpus_create(group._h, L.DIM, C.byref(self._h)))
        elif path is not None and layout is not None:
            pr = np.ascontiguousarray([p[0] for p in layout], dtype=np.uint64)
            rk = np.ascontiguousarray([p[1] for p in layout], dtype=np.uint32)
            L.check(L.lib().smt_sharded_corpus_load_layout(group._h, str(path).encode(), L.np_ptr(pr), L.np_ptr(rk), len(pr),
                                                           C.byref(self._h)))
        elif path is not None:
            L.check(L.lib().smt_sharded_corpus_load(group._h, str(path).encode(), C.byref(self._h)))
        elif device_ptrs is not None:
            n = len(device_ptrs)
            ptrs = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in device_ptrs])
            cnt = (C.c_uint64 * n)(*[int(r) for r in shard_rows])
            L.check(L.lib().smt_sharded_corpus_from_device(group._h, ptrs, cnt, L.DIM, C.byref(self._h)))
        else:
            rows = _f32c(rows).reshape(-1, L.DIM)
            L.check(L.lib().smt_sharded_corpus_from_host(group._h, L.np_ptr(rows), rows.shape[0], L.DIM, C.byref(self._h)))

    @classmethod
    def load(cls, group, path):
        return cls(group, path=path)

    def save(self, path):
        L.check(L.lib().smt_sharded_corpus_save(self._h, str(path).encode()))

    def append_to_file(self, path, rows_on_disk):
        L.check(L.lib().smt_sharded_corpus_append_to_file(self._h, str(path).encode(), int(rows_on_disk)))

    def layout(self):
        """[(rows, rank), ...] in global row order."""
        n = int(L.lib().smt_sharded_corpus_layout(self._h, None, None, 0))
        pr, rk = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)
        L.lib().smt_sharded_corpus_layout(self._h, L.np_ptr(pr), L.np_ptr(rk), n)
        return [(int(pr[i]), int(rk[i])) for i in range(n)]

    def read_rows(self, first_row, n_rows):
        out = np.empty((int(n_rows), L.DIM), dtype=np.float32)
        L.check(L.lib().smt_sharded_corpus_read_rows(self._h, int(first_row), int(n_rows), L.np_ptr(out)))
        return out

    def write_rows(self, first_row, rows):
        rows = _f32c(rows).reshape(-1, L.DIM)
        L.check(L.lib().smt_sharded_corpus_write_rows(self._h, int(first_row), L.np_ptr(rows), rows.shape[0]))

    def compact(self, ranges):
        """smt_sharded_corpus_compact: Corpus.compact with GLOBAL rows; every shard closes its own gaps.  Returns the rows moved."""
        rng, n = _ranges_arg(list(ranges))
        moved = C.c_uint64(0)
        L.check(L.lib().smt_sharded_corpus_compact(self._h, C.cast(rng, C.c_void_p), n, C.byref(moved)))
        return int(moved.value)

    def close(self):
        if _open(self):
            if _open(self.group):
                L.lib().smt_sharded_corpus_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def rows(self):
        return int(L.lib().smt_sharded_corpus_rows(self._h))

    def rank_rows(self):
        out = np.zeros(self.group.info()["n_ranks"], dtype=np.uint64)
        L.check(L.lib().smt_sharded_corpus_rank_rows(self._h, L.np_ptr(out)))
        return out

    def shard(self, local_index=0, want_base=True):
        """(Corpus view of local device i's shard, its first global row, its row count).  A corpus that grew by dealt
        appends has no single base per shard: pass want_base=False (the base comes back as None)."""
        h, base, n = C.c_void_p(), C.c_uint64(), C.c_uint64()
        L.check(L.lib().smt_sharded_corpus_shard(self._h, int(local_index), C.byref(h), C.byref(base) if want_base else None,
                                                 C.byref(n)))
        return Corpus(self.group.ctx(local_index), _handle=h, _borrowed=True), int(base.value) if want_base else None, int(n.value)

    def append(self, rows):
        rows = _f32c(rows).reshape(-1, L.DIM)
        first = C.c_uint64(0)
        L.check(L.lib().smt_sharded_corpus_append_host(self._h, L.np_ptr(rows), rows.shape[0], C.byref(first)))
        return int(first.value)

    def search(self, queries, top_k=3, max_distance=None, mode=L.MODE_DOCUMENTS, ranges=None, out_cap=None):
        q = _f32c(queries).reshape(-1, L.DIM)
        nq = q.shape[0]
        if out_cap is None:
            out_cap = max(int(top_k), 1)
            if max_distance is not None and mode == L.MODE_DOCUMENTS:
                # every row under the threshold: a first guess bounded by a TOTAL budget of 64 MB of result buffers (1000 queries x
                # 65 536 slots x 16 B was 1 GB of numpy arrays up front), grown on SMT_E_TRUNCATED to the true counts
                out_cap = max(int(top_k), min(self.rows, 1 << 16, (64 << 20) // (16 * max(nq, 1))), 1)
        rng, n_rng = _ranges_arg(ranges)
        while True:
            out_rows = np.empty((nq, out_cap), dtype=np.uint64)
            out_dist = np.empty((nq, out_cap), dtype=np.float64)
            counts = np.zeros(nq, dtype=np.uint64)
            rc = L.lib().smt_sharded_search(self._h, L.np_ptr(q), nq, int(top_k),
                                            float("nan") if max_distance is None else float(max_distance), int(mode),
                                            C.cast(rng, C.c_void_p) if rng is not None else None, n_rng,
                                            L.np_ptr(out_rows), L.np_ptr(out_dist), L.np_ptr(counts), int(out_cap))
            if rc == L.SMT_E_TRUNCATED:
                out_cap = int(counts.max())
                continue
            L.check(rc)
            break
        return [(out_rows[i, :int(counts[i])].copy(), out_dist[i, :int(counts[i])].copy()) for i in range(nq)]

    def search_topk_device(self, query_ptrs, nq, top_k, out_packed_ptrs, out_status_ptrs=None):
        """Device-resident form: one queries pointer and one output pointer (or 0/None) per LOCAL device.  out_status_ptrs: per local
        device a uint32[nq] buffer (or 0/None) for the per-query verdicts -- the worst status over the shards (_ex entry point)."""
        n = len(query_ptrs)
        qp = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in query_ptrs])
        op = (C.c_void_p * n)(*[C.c_void_p(int(p)) if p else C.c_void_p(None) for p in out_packed_ptrs])
        if out_status_ptrs is not None:
            sp = (C.c_void_p * n)(*[C.c_void_p(int(p)) if p else C.c_void_p(None) for p in out_status_ptrs])
            L.check(L.lib().smt_sharded_search_topk_device_ex(self._h, qp, int(nq), int(top_k), op, sp))
            return
        L.check(L.lib().smt_sharded_search_topk_device(self._h, qp, int(nq), int(top_k), op))


class ShardedIvfPq:
    """IVF index over a ShardedCorpus (smt_sharded_ivfpq): every rank indexes its rows; shared_centroids=True runs
    the coarse k-means data-parallel with an all-reduce of the centroid sums, so all ranks share one set of lists."""

    def __init__(self, sharded_corpus, nlist=4096, train_iters=10, local_pca=True, shared_centroids=True, _path=None):
        self.corpus = sharded_corpus
        self._h = C.c_void_p()
        if _path is not None:
            L.check(L.lib().smt_sharded_ivfpq_load(sharded_corpus._h, str(_path).encode(), C.byref(self._h)))
            return
        prm = L.SmtIvfPqParams(int(nlist), 32, 8, int(train_iters), 0, 0, 1 if local_pca else 0)
        L.check(L.lib().smt_sharded_ivfpq_build(sharded_corpus._h, C.byref(prm), int(bool(shared_centroids)), C.byref(self._h)))

    @classmethod
    def load(cls, sharded_corpus, path):
        return cls(sharded_corpus, _path=path)

    def save(self, path):
        L.check(L.lib().smt_sharded_ivfpq_save(self._h, str(path).encode()))

    def append(self):
        n = C.c_uint64(0)
        L.check(L.lib().smt_sharded_ivfpq_append(self._h, C.byref(n)))
        return int(n.value)

    def compact(self, ranges):
        """smt_sharded_ivfpq_compact: ShardedCorpus.compact(ranges) (GLOBAL rows) with every shard's index carried along.  Returns
        (rows_moved, entries_dropped), summed over the shards."""
        rng, n = _ranges_arg(list(ranges))
        moved, dropped = C.c_uint64(0), C.c_uint64(0)
        L.check(L.lib().smt_sharded_ivfpq_compact(self._h, C.cast(rng, C.c_void_p), n, C.byref(moved), C.byref(dropped)))
        return int(moved.value), int(dropped.value)

    def info(self):
        rows, nlist, nbytes = C.c_uint64(), C.c_uint32(), C.c_uint64()
        L.check(L.lib().smt_sharded_ivfpq_info(self._h, C.byref(rows), C.byref(nlist), C.byref(nbytes)))
        return dict(rows=int(rows.value), nlist=int(nlist.value), index_bytes=int(nbytes.value))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            L.lib().smt_sharded_ivfpq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shard_list_sizes(self, local_index, nlist):
        h = L.lib().smt_sharded_ivfpq_shard(self._h, int(local_index))
        out = np.empty(int(nlist), dtype=np.uint64)
        L.check(L.lib().smt_ivfpq_list_sizes(C.c_void_p(h), L.np_ptr(out)))
        return out

    def search(self, queries, top_k=10, nprobe=16, rerank=128, ranges=None, wide=False):
        """ranges: GLOBAL rows to search inside (smt_sharded_ivfpq_search_ranges); None calls smt_sharded_ivfpq_search.
        wide: smt_sharded_ivfpq_search_wide (top_k up to 1024 with n_ranks x top_k <= 8192; an empty list of ranges is an empty filter)."""
        q = _f32c(queries).reshape(-1, L.DIM)
        nq = q.shape[0]
        cap = max(int(top_k), 1)
        out_rows = np.empty((nq, cap), dtype=np.uint64)
        out_dist = np.empty((nq, cap), dtype=np.float64)
        counts = np.zeros(nq, dtype=np.uint64)
        if wide:
            rng, n_rng = _ranges_arg(ranges)
            L.check(L.lib().smt_sharded_ivfpq_search_wide(self._h, L.np_ptr(q), nq, int(top_k), int(nprobe), int(rerank),
                                                          C.cast(rng, C.c_void_p) if rng is not None else None, n_rng,
                                                          L.np_ptr(out_rows), L.np_ptr(out_dist), L.np_ptr(counts), cap))
        elif ranges is None:
            L.check(L.lib().smt_sharded_ivfpq_search(self._h, L.np_ptr(q), nq, int(top_k), int(nprobe), int(rerank),
                                                     L.np_ptr(out_rows), L.np_ptr(out_dist), L.np_ptr(counts), cap))
        else:
            rng, n_rng = _ranges_arg(ranges)
            L.check(L.lib().smt_sharded_ivfpq_search_ranges(self._h, L.np_ptr(q), nq, int(top_k), int(nprobe), int(rerank),
                                                            C.cast(rng, C.c_void_p), n_rng,
                                                            L.np_ptr(out_rows), L.np_ptr(out_dist), L.np_ptr(counts), cap))
        return [(out_rows[i, :int(counts[i])].copy(), out_dist[i, :int(counts[i])].copy()) for i in range(nq)]


def merge_topk(rows, dist, k_out):
    """Host merge of per-shard sorted top-k lists laid out [n_lists][nq][k_in]."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    n_lists, nq, k_in = rows.shape
    out_rows = np.empty((nq, k_out), dtype=np.uint64)
    out_dist = np.empty((nq, k_out), dtype=np.float64)
    counts = np.zeros(nq, dtype=np.uint64)
    L.check(L.lib().smt_merge_topk(L.np_ptr(rows), L.np_ptr(dist), n_lists, nq, k_in, int(k_out),
                                   L.np_ptr(out_rows), L.np_ptr(out_dist), L.np_ptr(counts)))
    return out_rows, out_dist, counts
