"""GPU parity: K1 over indexed model tables -- a table of n_rows rows shared by n_tokens tokens through `mapping`, with one scalar
`weights[t]` per token -- against plain pooling over the expanded f32 table

    E'[t] = fl32(weights[t] * widen(table[mapping[t]]))      (NumPy float32, one elementwise multiply)

The kernel rounds the product to f32 and then adds it, in token order, so the bar is bit-exactness (outputs compared as uint32
views) against two references: the oracle's embed_lines on E', and the GPU's own SMT_TABLE_F32 model built from E'."""
import ctypes as C
import json

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

NT = 300          # n_tokens
NR = 40           # n_rows
DTYPES = ["float32", "float16", "int8"]
ROW_BYTES = {"float32": 1024, "float16": 512, "int8": 256}
OOV = 2 ** 32 - 1
FORMS = ["both", "mapping", "weights", "identity", "permutation"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows_of(form):
    return NT if form in ("weights", "identity", "permutation") else NR


def _stored_table(dtype, n_rows):
    """Values of modest size (|x| <= 2 for the float types, the whole int8 range), so that with weights up to 2^20 every product
    and every sum over 2049 tokens stays finite."""
    rng = np.random.default_rng({"float32": 51, "float16": 53, "int8": 57}[dtype] + n_rows)
    if dtype == "int8":
        t = rng.integers(-128, 128, size=(n_rows, 256)).astype(np.int8)
        t[1] = np.where(np.arange(256) % 2 == 0, -128, 127).astype(np.int8)
    else:
        t = np.clip(rng.standard_normal((n_rows, 256)) * 0.5, -2, 2).astype(dtype)
        t[1] = np.where(np.arange(256) % 2 == 0, 1.5, -1.5).astype(dtype)
    t[2] = 0
    return np.ascontiguousarray(t)


def _mapping(form):
    """many-to-one: tokens 0..5 share row 0, tokens 290..299 the last row, tokens 6 and 7 both sit on row 1 (the cancelling pair)."""
    rng = np.random.default_rng(61)
    if form in ("both", "mapping"):
        m = rng.integers(0, NR, size=NT).astype(np.uint32)
        m[:6] = 0
        m[290:] = NR - 1
        m[6] = m[7] = 1
        return m
    if form == "identity":
        return np.arange(NT, dtype=np.uint32)
    if form == "permutation":
        return rng.permutation(NT).astype(np.uint32)
    return None


def _weights(form):
    """random in [0.25, 4], with hand-set entries: +0 and -0, a negative weight, 2^-130 (the product is an f32 subnormal), 2^20, and
    w / -w on tokens 6 / 7, which share a row in the many-to-one mapping."""
    if form not in ("both", "weights"):
        return None
    rng = np.random.default_rng(67)
    w = rng.uniform(0.25, 4.0, size=NT).astype(np.float32)
    w[8] = 0.0
    w[9] = -0.0
    w[10] = -1.75
    w[11] = np.float32(2.0 ** -130)
    w[12] = np.float32(2.0 ** 20)
    w[6] = 3.0
    w[7] = -3.0
    return w


_CASES = {}


def case(dtype, form):
    """(stored table, mapping or None, weights or None, E') -- built once, never written to."""
    key = (dtype, form)
    if key not in _CASES:
        table = _stored_table(dtype, _rows_of(form))
        m, w = _mapping(form), _weights(form)
        rows = table[m] if m is not None else table
        wide = rows.astype(np.float32)
        e = wide * w.astype(np.float32)[:, None] if w is not None else wide
        e = np.ascontiguousarray(e, dtype=np.float32)
        assert e.shape == (NT, 256) and np.isfinite(e).all()
        # every line sum stays finite: the longest line has 2049 tokens
        assert float(np.abs(e).max()) * 2049 < 3e38
        if w is not None and dtype != "int8":
            assert (np.abs(e[11][e[11] != 0]) < 2.0 ** -126).all()       # subnormal products
        for a in (table, e) + ((m,) if m is not None else ()) + ((w,) if w is not None else ()):
            a.setflags(write=False)
        _CASES[key] = (table, m, w, e)
    return _CASES[key]


def _csr(lines):
    offsets = np.zeros(len(lines) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in lines], out=offsets[1:])
    ids = np.concatenate([np.asarray(x, dtype=np.uint32) for x in lines] + [np.zeros(0, np.uint32)])
    return ids, offsets


def _border_lines():
    """17 lines on the kernel's borders: empty lines, 1 / 3 / 4 / 5 / 8 / 9 tokens (four tokens are in flight per step), a 2049-token
    line, ids equal to n_tokens, n_tokens + 1 and 2^32 - 1 inside a line, the hand-set weights, the pair that cancels to a zero
    row, a line of unknown ids only."""
    rng = np.random.default_rng(3)
    r = lambda n: rng.integers(0, NT, size=n).astype(np.uint32)
    lines = [r(0), r(1), r(3), r(4), r(5), r(8), r(9), r(0),
             r(2049),
             np.array([9, NT, 10, OOV, 11, NT + 1], np.uint32),
             np.arange(13, dtype=np.uint32),
             np.array([6, 7], np.uint32),
             np.array([NT, OOV, NT + 1], np.uint32),
             np.array([8, 9, 8, 2, 11], np.uint32),
             np.array([12, 10, 12], np.uint32),
             r(17), r(0)]
    assert len(lines) == 17
    return _csr(lines)


def _ragged_lines():
    """40 000 lines, more than one per lane group, so the runs are cut by work: lengths 0..32 with a dozen 2048-token lines."""
    rng = np.random.default_rng(29)
    n = 40_000
    lens = rng.integers(0, 33, size=n)
    lens[rng.choice(n, size=12, replace=False)] = 2048
    lens[500:540] = 0
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    ids = rng.integers(0, NT, size=int(offsets[-1])).astype(np.uint32)
    ids[rng.choice(ids.size, size=50, replace=False)] = NT
    ids[rng.choice(ids.size, size=50, replace=False)] = OOV
    return ids, offsets


_SETS = {}
_REFS = {}


def lines_of(name):
    if name not in _SETS:
        if name == "one":
            _SETS[name] = _csr([np.array([5, 17, 1, 299, 8], np.uint32)])
        elif name == "border":
            _SETS[name] = _border_lines()
        else:
            _SETS[name] = _ragged_lines()
        for a in _SETS[name]:
            a.setflags(write=False)
    return _SETS[name]


def reference(dtype, form, name, normalize, cap):
    """The oracle on E': computed once per case, shared, never written to."""
    key = (dtype, form, name, bool(normalize), cap)
    if key not in _REFS:
        ids, offsets = lines_of(name)
        ref = orc.embed_lines(case(dtype, form)[3], ids, offsets, normalize=bool(normalize), max_tokens=cap)
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


@pytest.fixture(scope="module", params=DTYPES)
def dtype(request):
    return request.param


@pytest.fixture(scope="module")
def models(dtype, gpu_ctx):
    """(form, normalize) -> indexed model, and form -> the GPU's own f32 model on E'"""
    import semtools_amd as smt

    made, wide = {}, {}

    def get(form, normalize=True):
        if (form, normalize) not in made:
            table, m, w, _ = case(dtype, form)
            made[(form, normalize)] = smt.Model(gpu_ctx, table, normalize=normalize, mapping=m, weights=w)
        return made[(form, normalize)]

    def get_wide(form, normalize=True):
        if (form, normalize) not in wide:
            wide[(form, normalize)] = smt.Model(gpu_ctx, case(dtype, form)[3], normalize=normalize)
        return wide[(form, normalize)]

    yield get, get_wide
    for m in list(made.values()) + list(wide.values()):
        m.close()


def test_token_info_and_model_info(dtype, models, gpu_ctx):
    from semtools_amd import _lib as L

    for form in FORMS:
        m = models[0](form)
        n_rows = _rows_of(form)
        assert m.n_tokens == NT and m.token_bytes == 8 * NT
        assert m.has_mapping == (form != "weights") and m.has_weights == (form in ("both", "weights"))
        assert m.table_dtype == np.dtype(dtype) and m.table_bytes == n_rows * ROW_BYTES[dtype]
        dt, v, nb = C.c_int(), C.c_uint64(), C.c_uint64()
        L.check(L.lib().smt_model_info(m._h, C.byref(dt), C.byref(v), C.byref(nb)))
        assert (dt.value, v.value, nb.value) == (L.table_dtype_code(dtype), n_rows, n_rows * ROW_BYTES[dtype])
    plain = models[1]("both")
    assert (plain.n_tokens, plain.has_mapping, plain.has_weights, plain.token_bytes) == (NT, False, False, 0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["one", "border"])
def test_border_lines_in_every_kernel_mode(dtype, models, gpu_ctx, name, form):
    """n_lines 1 and 17.  embed_batched bits: 1 = batched epilogue, 2 = ids prefetched (PF kernel), 4 = span limit 64 (the generic
    kernel takes the long runs behind the PF kernel), 8 = runs cut by line count.  max_tokens 2048, 16 and 0 on a 2049-token line."""
    ids, offsets = lines_of(name)
    lens = np.diff(offsets.astype(np.int64))
    try:
        for normalize in ((True, False) if form == "both" else (True,)):
            m, wide = models[0](form, normalize), models[1](form, normalize)
            for mode in (3, 2, 1, 0, 7, 6, 11):
                gpu_ctx.set_tuning("embed_batched", mode)
                for cap in (2048, 16, 0):
                    got, _ = m.embed(ids, offsets, max_tokens=cap)
                    same, _ = wide.embed(ids, offsets, max_tokens=cap)
                    ref = reference(dtype, form, name, normalize, cap)
                    print(dtype, form, name, normalize, "mode", mode, "cap", cap, "rows differing from the oracle",
                          int((_bits(got) != _bits(ref)).any(axis=1).sum()), "from the f32 model", int((_bits(got) != _bits(same)).any(axis=1).sum()))
                    assert np.array_equal(_bits(got), _bits(ref)), (dtype, form, name, normalize, mode, cap)
                    assert np.array_equal(_bits(got), _bits(same)), (dtype, form, name, normalize, mode, cap)
                    assert not got[lens == 0].any()
    finally:
        gpu_ctx.set_tuning("embed_batched", 3)


def test_hand_set_weights_do_what_they_should(dtype, models):
    """Not only equal to the reference: the cancelling pair gives a zero row, a line of unknown ids gives a zero row."""
    ids, offsets = lines_of("border")
    got, _ = models[0]("both", False).embed(ids, offsets, max_tokens=2048)
    assert not got[11].any() and not got[12].any()
    assert got[13].any() and got[14].any()


@pytest.mark.parametrize("form", ["both", "weights", "permutation"])
def test_runs_cut_by_work(dtype, models, gpu_ctx, form):
    """40 000 ragged lines: several lines per lane group, runs cut by work (default) and by line count, PF + generic kernel with the
    span limit at 64, the generic kernel alone with the per-line epilogue."""
    ids, offsets = lines_of("ragged")
    modes = ((3, True, 2048), (3, False, 16), (7, True, 2048), (11, True, 2048), (0, True, 16), (2, False, 2048)) if form == "both" else \
            ((3, True, 2048), (7, True, 16), (0, True, 2048))
    try:
        for mode, normalize, cap in modes:
            gpu_ctx.set_tuning("embed_batched", mode)
            got, _ = models[0](form, normalize).embed(ids, offsets, max_tokens=cap)
            same, _ = models[1](form, normalize).embed(ids, offsets, max_tokens=cap)
            ref = reference(dtype, form, "ragged", normalize, cap)
            print(dtype, form, "mode", mode, normalize, cap, "rows differing from the oracle", int((_bits(got) != _bits(ref)).any(axis=1).sum()),
                  "from the f32 model", int((_bits(got) != _bits(same)).any(axis=1).sum()))
            assert np.array_equal(_bits(got), _bits(same)), (dtype, form, mode, normalize, cap)
            assert np.array_equal(_bits(got), _bits(ref)), (dtype, form, mode, normalize, cap)
    finally:
        gpu_ctx.set_tuning("embed_batched", 3)


def test_the_three_creators_give_identical_rows(dtype, models, gpu_ctx, tmp_path):
    """create_indexed (the fixture), create_from_file_indexed with the table at an odd byte offset, create_from_device_indexed."""
    import torch
    import semtools_amd as smt

    table, m, w, _ = case(dtype, "both")
    ids, offsets = lines_of("border")
    want, _ = models[0]("both").embed(ids, offsets, max_tokens=2048)
    assert np.array_equal(_bits(want), _bits(reference(dtype, "both", "border", True, 2048)))
    path = tmp_path / "table.bin"
    with open(path, "wb") as f:
        f.write(b"\x5a" * 37)
        f.write(table.tobytes())
        f.write(b"\xa5" * 5)
    from_file = smt.Model.from_file(gpu_ctx, path, 37, NR, normalize=True, dtype=dtype, mapping=m, weights=w)
    dev = torch.from_numpy(np.array(table)).cuda()
    dmap = torch.from_numpy(m.astype(np.int32)).cuda()          # (the same 32 bits)
    dw = torch.from_numpy(np.array(w)).cuda()
    torch.cuda.synchronize()
    from_dev = smt.Model(gpu_ctx, device_ptr=dev.data_ptr(), V=NR, normalize=True, dtype=dtype, mapping_ptr=dmap.data_ptr(),
                         weights_ptr=dw.data_ptr(), n_tokens=NT)
    try:
        for mod in (from_file, from_dev):
            assert (mod.n_tokens, mod.has_mapping, mod.has_weights, mod.token_bytes) == (NT, True, True, 8 * NT)
            assert mod.table_bytes == NR * ROW_BYTES[dtype]
            got, _ = mod.embed(ids, offsets, max_tokens=2048)
            assert np.array_equal(_bits(got), _bits(want))
    finally:
        from_file.close()
        from_dev.close()


def test_refusals(gpu_ctx, tmp_path):
    """Every refusal is SMT_E_INVALID, names the offending token where there is one, and leaves the handle NULL."""
    import torch
    from semtools_amd import _lib as L

    lib = L.lib()
    table, m, w, _ = case("int8", "both")
    path = tmp_path / "t.bin"
    path.write_bytes(table.tobytes())
    dev = torch.from_numpy(np.concatenate([np.array(table).reshape(-1), np.zeros(64, np.int8)])).cuda()
    h = C.c_void_p()

    def host(mp, wp, n, dt=L.TABLE_I8, rows=NR):
        return lib.smt_model_create_indexed(gpu_ctx._h, L.np_ptr(table), dt, rows, 256, L.np_ptr(mp), L.np_ptr(wp), n, 1, C.byref(h))

    def file(mp, wp, n, dt=L.TABLE_I8):
        return lib.smt_model_create_from_file_indexed(gpu_ctx._h, str(path).encode(), 0, dt, NR, 256, L.np_ptr(mp), L.np_ptr(wp), n, 1, C.byref(h))

    def device(mp, wp, n, dt=L.TABLE_I8, off=0):
        keep = [torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda() if x is not None else None for x in (mp, wp)]
        torch.cuda.synchronize()
        return lib.smt_model_create_from_device_indexed(gpu_ctx._h, C.c_void_p(dev.data_ptr() + off), dt, NR, 256,
                                                        C.c_void_p(keep[0].data_ptr()) if keep[0] is not None else None,
                                                        C.c_void_p(keep[1].data_ptr()) if keep[1] is not None else None, n, 1, C.byref(h))

    m = np.array(m)
    w = np.array(w)
    bad_row = m.copy(); bad_row[123] = NR; bad_row[200] = NR + 5
    bad_inf = w.copy(); bad_inf[77] = np.inf
    bad_nan = w.copy(); bad_nan[78] = np.nan; bad_nan[250] = -np.inf
    for make in (host, file, device):
        for bad in (3, -1, 99):
            assert make(m, w, NT, dt=bad) == L.SMT_E_INVALID and b"dtype" in lib.smt_last_error() and not h
        assert make(m, w, 0) == L.SMT_E_INVALID and b"n_tokens" in lib.smt_last_error() and not h
        assert make(None, w, NT) == L.SMT_E_INVALID and b"n_rows" in lib.smt_last_error() and not h       # NT != NR without a mapping
        assert make(bad_row, w, NT) == L.SMT_E_INVALID and b"token 123" in lib.smt_last_error() and not h
        assert make(bad_row, None, NT) == L.SMT_E_INVALID and b"token 123" in lib.smt_last_error() and not h
        assert make(m, bad_inf, NT) == L.SMT_E_INVALID and b"token 77" in lib.smt_last_error() and not h
        assert make(m, bad_nan, NT) == L.SMT_E_INVALID and b"token 78" in lib.smt_last_error() and not h
    for off in (1, 4, 8):
        assert device(m, w, NT, off=off) == L.SMT_E_INVALID and b"aligned" in lib.smt_last_error() and not h
    group_h = C.c_void_p()
    import semtools_amd as smt
    group = smt.Group.logical(0, 2)
    try:
        rc = lib.smt_sharded_model_create_indexed(group._h, L.np_ptr(table), L.TABLE_I8, NR, 256, L.np_ptr(bad_row), L.np_ptr(w), NT, 1, C.byref(group_h))
        assert rc == L.SMT_E_INVALID and b"token 123" in lib.smt_last_error() and not group_h
    finally:
        group.close()


def test_append_from_an_indexed_model_then_search(dtype, models, gpu_ctx):
    import semtools_amd as smt

    ids, offsets = lines_of("border")
    ref = reference(dtype, "both", "border", True, 2048)
    c = smt.Corpus(gpu_ctx)
    try:
        _, first = models[0]("both").embed(ids, offsets, max_tokens=2048, append_to=c, want_host=False)
        assert first == 0 and c.rows == 17
        assert np.array_equal(_bits(c.read_rows(0, 17)), _bits(ref))
        q = ref[15]
        rows, dist = c.search(q, top_k=3)[0]
        res = orc.search_documents(np.asarray(ref), [17], q, 0, 3, accurate=True)
        assert rows.tolist() == [r["match_line"] for r in res] and rows[0] == 15
        assert np.allclose(dist, [r["distance"] for r in res], rtol=0, atol=1e-6)
    finally:
        c.close()


def test_a_logical_group_of_three_shards_gives_the_one_gpu_rows(dtype):
    import semtools_amd as smt

    table, m, w, _ = case(dtype, "both")
    group = smt.Group.logical(0, 3)
    try:
        sm = smt.ShardedModel(group, table, normalize=True, mapping=m, weights=w)
        assert (sm.n_tokens, sm.has_mapping, sm.has_weights, sm.token_bytes) == (NT, True, True, 8 * NT)
        assert sm.table_bytes == NR * ROW_BYTES[dtype]
        for name in ("border", "ragged"):
            ids, offsets = lines_of(name)
            got, _ = sm.embed(ids, offsets, max_tokens=2048)
            assert np.array_equal(_bits(got), _bits(reference(dtype, "both", name, True, 2048))), name
        sm.close()
    finally:
        group.close()


# ---------------------------------------------------------------- host layer: a three-tensor model directory

def _model_dir(tmp_path, table, m, w, wdtype):
    from safetensors.numpy import save_file

    d = tmp_path / "m"
    d.mkdir()
    tensors = {"embeddings": np.array(table)}
    if m is not None:
        tensors["mapping"] = m.astype(np.int64)
    if w is not None:
        tensors["weights"] = w.astype(wdtype)
    save_file(tensors, str(d / "model.safetensors"))
    n_vocab = NT if m is not None else table.shape[0]
    (d / "vocab.txt").write_text("".join(f"w{i}\n" for i in range(n_vocab - 1)) + "[UNK]\n")
    (d / "config.json").write_text(json.dumps({"normalize": True, "unk_token": "[UNK]"}))
    return d


def _host_reference(expanded, lines, n_vocab):
    ids, offsets = [], [0]
    for ln in lines:
        ids += [int(x[1:]) for x in ln.split() if x.startswith("w") and x[1:].isdigit() and int(x[1:]) < n_vocab - 1]
        offsets.append(len(ids))
    return orc.embed_lines(expanded, np.array(ids, np.uint32), np.array(offsets, np.uint64), True, 2048)


@pytest.mark.parametrize("where", ["one_gpu", "three_shards"])
@pytest.mark.parametrize("stored,wdtype", [("int8", "float64"), ("float16", "float16")])
def test_host_layer_serves_a_three_tensor_directory(gpu_ctx, tmp_path, where, stored, wdtype):
    """embeddings (I8 / F16) + mapping (int64) + weights (float64 / float16) + a vocabulary of n_tokens entries.  Six short lines go
    through the compact path (the whole table is not resident afterwards), 33 000 three-token lines through the full upload; both
    match the reference on E' bit for bit.  (float16 weights: the hand-set 2^-130 is not representable, the file's values are what
    the reference uses.)"""
    import semtools_amd as smt
    from semtools_amd import host

    table, m, w, _ = case(stored, "both")
    w_file = np.array(w)
    if wdtype == "float16":        # what binary16 can hold: 2^20 would be inf, 2^-130 zero
        w_file[12] = 2.0 ** 10
        w_file[11] = 2.0 ** -24
    w_file = w_file.astype(wdtype)
    w32 = w_file.astype(np.float32)
    assert np.isfinite(w32).all()
    expanded = np.ascontiguousarray(np.array(table)[m].astype(np.float32) * w32[:, None], dtype=np.float32)
    assert np.isfinite(expanded).all()
    d = _model_dir(tmp_path, table, m, w_file, wdtype)
    group = smt.Group.logical(0, 3) if where == "three_shards" else None
    mod = host.StaticModel(group if group is not None else gpu_ctx, model_dir=d)
    try:
        few = ["w0 w1 w2 w3 w4 w5 w6 w7", "w6 w7", "", "w8 w9 w10 nothing w298", "w12 w11 w12", "w17"]
        got = mod.encode_with_args(few, 2048)
        assert np.array_equal(_bits(got), _bits(_host_reference(expanded, few, NT)))
        assert not got[1].any()
        assert mod.table_info() == (np.dtype(stored), NR, NR * ROW_BYTES[stored], False)
        assert mod.token_info() == (NT, True, True, 8 * NT)
        rng = np.random.default_rng(8)
        toks = rng.integers(0, NT - 1, size=(33_000, 3))
        many = [f"w{a} w{b} w{c}" for a, b, c in toks]
        many[100] = ""
        got = mod.encode_with_args(many, 2048)
        assert np.array_equal(_bits(got), _bits(_host_reference(expanded, many, NT)))
        assert mod.table_info() == (np.dtype(stored), NR, NR * ROW_BYTES[stored], True)
        assert mod.token_info() == (NT, True, True, 8 * NT)
    finally:
        mod.close()
        if group is not None:
            group.close()


def test_a_plain_directory_still_loads_as_before(gpu_ctx, tmp_path):
    from semtools_amd import host

    table = case("float16", "weights")[0]       # 300 rows: six tokens are less than 1/16 of them, so the compact path serves the call
    assert table.shape[0] == NT
    d = _model_dir(tmp_path, table, None, None, None)
    mod = host.StaticModel(gpu_ctx, model_dir=d)
    try:
        few = ["w0 w1 w2 w3", "", "w38 w5"]
        got = mod.encode_with_args(few, 2048)
        assert np.array_equal(_bits(got), _bits(_host_reference(np.array(table).astype(np.float32), few, NT)))
        assert mod.table_info() == (np.dtype("float16"), NT, NT * 512, False)
        assert mod.token_info() == (NT, False, False, 0)
    finally:
        mod.close()
