"""GPU parity: K1 over model tables kept as stored -- IEEE half and int8 rows, widened in registers -- against the oracle's
pool_ids on the table widened with NumPy (astype(float32) is exact for both).  The kernel keeps the serial f32 chains of
the CPU code whatever the table's element type, so the bar is bit-exactness: outputs are compared as uint32 views."""
import ctypes as C
import json

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

V = 300
DTYPES = ["float16", "int8"]
ROW_BYTES = {"float16": 512, "int8": 256}
OOV = 2 ** 32 - 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _stored_table(dtype):
    rng = np.random.default_rng(41 if dtype == "float16" else 43)
    if dtype == "float16":
        t = (rng.standard_normal((V, 256)) * 0.1).astype(np.float16)
        sign = np.where(np.arange(256) % 2 == 0, 1.0, -1.0)
        t[0] = (sign * 0.0).astype(np.float16)                                   # +0 / -0
        t[1] = np.where(sign > 0, np.uint16(0x0001), np.uint16(0x8001)).astype(np.uint16).view(np.float16)   # smallest subnormal, both signs
        t[2] = np.full(256, 0x03FF, np.uint16).view(np.float16)                  # largest subnormal
        t[3] = np.float16(2.0 ** -14)                                            # smallest normal
        t[4] = np.float16(65504.0)
        t[5] = np.float16(-65504.0)
        t[6] = (sign * 1.5).astype(np.float16)                                   # alternating signs ...
        t[7] = (-sign * 1.5).astype(np.float16)                                  # ... and the row that cancels it to zero
        assert np.isfinite(t.astype(np.float32)).all()
    else:
        t = rng.integers(-128, 128, size=(V, 256)).astype(np.int8)
        t[0] = -128
        t[1] = 127
        t[2] = 0
        t[3] = np.where(np.arange(256) % 2 == 0, -128, 127).astype(np.int8)
    return np.ascontiguousarray(t)


def _csr(lines):
    offsets = np.zeros(len(lines) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in lines], out=offsets[1:])
    ids = np.concatenate([np.asarray(x, dtype=np.uint32) for x in lines] + [np.zeros(0, np.uint32)])
    return ids, offsets


def _border_lines():
    """17 lines on the kernel's borders: empty lines, 1 / 3 / 4 / 5 / 8 / 9 tokens (four tokens are in flight per step), a 2049-token
    line, ids equal to V and 2^32 - 1 inside a line, the hand-set rows, a line whose sum cancels to zero, a line of unknown ids only."""
    rng = np.random.default_rng(3)
    r = lambda n: rng.integers(0, V, size=n).astype(np.uint32)
    lines = [r(0), r(1), r(3), r(4), r(5), r(8), r(9), r(0),
             r(2049),
             np.array([9, V, 10, OOV, 11], np.uint32),
             np.arange(8, dtype=np.uint32),
             np.array([6, 7], np.uint32),
             np.array([V, OOV, V + 1], np.uint32),
             np.array([1, 1, 1, 2, 3], np.uint32),
             np.array([4, 5, 4], np.uint32),
             r(17), r(0)]
    assert len(lines) == 17
    return _csr(lines)


def _ragged_lines():
    """40 000 lines, more than one per lane group, so the runs are cut by work: lengths 0..32 with a few 2048-token lines."""
    rng = np.random.default_rng(29)
    n = 40_000
    lens = rng.integers(0, 33, size=n)
    lens[rng.choice(n, size=12, replace=False)] = 2048
    lens[500:540] = 0
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    ids = rng.integers(0, V, size=int(offsets[-1])).astype(np.uint32)
    ids[rng.choice(ids.size, size=50, replace=False)] = V          # unknown ids scattered about
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


def reference(dtype, name, normalize, cap):
    """The oracle on the widened table: computed once per case, shared, never written to."""
    key = (dtype, name, bool(normalize), cap)
    if key not in _REFS:
        ids, offsets = lines_of(name)
        ref = orc.embed_lines(_stored_table(dtype).astype(np.float32), ids, offsets, normalize=bool(normalize), max_tokens=cap)
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


@pytest.fixture(scope="module", params=DTYPES)
def typed(request, gpu_ctx):
    import semtools_amd as smt

    stored = _stored_table(request.param)
    models = {n: smt.Model(gpu_ctx, stored, normalize=n) for n in (True, False)}
    yield request.param, stored, models
    for m in models.values():
        m.close()


def test_model_info_reports_the_stored_type_and_size(typed):
    dtype, stored, models = typed
    m = models[True]
    assert m.table_dtype == np.dtype(dtype)
    assert m.table_bytes == V * ROW_BYTES[dtype]
    from semtools_amd import _lib as L

    dt, v, nb = C.c_int(), C.c_uint64(), C.c_uint64()
    L.check(L.lib().smt_model_info(m._h, C.byref(dt), C.byref(v), C.byref(nb)))
    assert (dt.value, v.value, nb.value) == ({"float16": L.TABLE_F16, "int8": L.TABLE_I8}[dtype], V, V * ROW_BYTES[dtype])


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("name", ["one", "border"])
def test_border_lines_in_every_kernel_mode(typed, gpu_ctx, name, normalize):
    """n_lines 1 and 17.  embed_batched bits: 1 = batched epilogue, 2 = ids prefetched (PF kernel), 4 = span limit 64 (the generic
    kernel takes the long runs behind the PF kernel), 8 = runs cut by line count.  max_tokens 2048, 16 and 0 on a 2049-token line."""
    dtype, _, models = typed
    ids, offsets = lines_of(name)
    try:
        for mode in (3, 2, 1, 0, 7, 6, 11):
            gpu_ctx.set_tuning("embed_batched", mode)
            for cap in (2048, 16, 0):
                got, _ = models[normalize].embed(ids, offsets, max_tokens=cap)
                ref = reference(dtype, name, normalize, cap)
                print(dtype, name, normalize, "mode", mode, "cap", cap, "rows differing", int((_bits(got) != _bits(ref)).any(axis=1).sum()))
                assert np.array_equal(_bits(got), _bits(ref)), (dtype, name, normalize, mode, cap)
                lens = np.diff(offsets.astype(np.int64))
                assert not got[lens == 0].any()
    finally:
        gpu_ctx.set_tuning("embed_batched", 3)


def test_runs_cut_by_work_and_typed_equals_widened(typed, gpu_ctx):
    """40 000 ragged lines: several lines per lane group, runs cut by work (default) and by line count, PF + generic kernel with the
    span limit at 64, the generic kernel alone with the per-line epilogue.  Besides the oracle, an f32 model built from the widened
    table must give the same bits (that holds whatever the oracle says)."""
    import semtools_amd as smt

    dtype, stored, models = typed
    ids, offsets = lines_of("ragged")
    wide = {n: smt.Model(gpu_ctx, stored.astype(np.float32), normalize=n) for n in (True, False)}
    try:
        for mode, normalize, cap in ((3, True, 2048), (3, True, 16), (3, False, 2048), (7, True, 2048), (7, False, 16), (11, True, 2048),
                                     (0, True, 16), (2, False, 2048), (1, True, 2048)):
            gpu_ctx.set_tuning("embed_batched", mode)
            got, _ = models[normalize].embed(ids, offsets, max_tokens=cap)
            same, _ = wide[normalize].embed(ids, offsets, max_tokens=cap)
            ref = reference(dtype, "ragged", normalize, cap)
            print(dtype, "mode", mode, normalize, cap, "rows differing from the oracle", int((_bits(got) != _bits(ref)).any(axis=1).sum()),
                  "from the widened model", int((_bits(got) != _bits(same)).any(axis=1).sum()))
            assert np.array_equal(_bits(got), _bits(same)), (dtype, mode, normalize, cap)
            assert np.array_equal(_bits(got), _bits(ref)), (dtype, mode, normalize, cap)
    finally:
        gpu_ctx.set_tuning("embed_batched", 3)
        for m in wide.values():
            m.close()


def test_bad_arguments_are_refused(gpu_ctx):
    import torch
    from semtools_amd import _lib as L

    lib = L.lib()
    stored = _stored_table("int8")
    h = C.c_void_p()
    for bad in (3, -1, 99):
        assert lib.smt_model_create_typed(gpu_ctx._h, L.np_ptr(stored), bad, V, 256, 1, C.byref(h)) == L.SMT_E_INVALID
        assert b"dtype" in lib.smt_last_error() and not h
        assert lib.smt_model_create_from_file_typed(gpu_ctx._h, b"/nonexistent", 0, bad, V, 256, 1, C.byref(h)) == L.SMT_E_INVALID
    dev = torch.zeros(V * 256 + 64, dtype=torch.int8, device="cuda")
    assert dev.data_ptr() % 16 == 0
    assert lib.smt_model_create_from_device_typed(gpu_ctx._h, C.c_void_p(dev.data_ptr()), 7, V, 256, 1, C.byref(h)) == L.SMT_E_INVALID
    for off in (1, 2, 4, 8):
        rc = lib.smt_model_create_from_device_typed(gpu_ctx._h, C.c_void_p(dev.data_ptr() + off), L.TABLE_I8, V, 256, 1, C.byref(h))
        assert rc == L.SMT_E_INVALID and b"aligned" in lib.smt_last_error() and not h


def test_the_three_creators_give_identical_rows(typed, gpu_ctx, tmp_path):
    """create_typed (the fixture), create_from_file_typed with the table at an odd byte offset of a file, create_from_device_typed."""
    import torch
    import semtools_amd as smt
    from semtools_amd import _lib as L

    dtype, stored, models = typed
    ids, offsets = lines_of("border")
    want, _ = models[True].embed(ids, offsets, max_tokens=2048)
    assert np.array_equal(_bits(want), _bits(reference(dtype, "border", True, 2048)))
    path = tmp_path / "table.bin"
    with open(path, "wb") as f:
        f.write(b"\x5a" * 37)
        f.write(stored.tobytes())
        f.write(b"\xa5" * 5)
    from_file = smt.Model.from_file(gpu_ctx, path, 37, V, normalize=True, dtype=dtype)
    dev = torch.from_numpy(stored).cuda()
    torch.cuda.synchronize()
    from_dev = smt.Model(gpu_ctx, device_ptr=dev.data_ptr(), V=V, normalize=True, dtype=dtype)
    try:
        for m in (from_file, from_dev):
            assert m.table_dtype == np.dtype(dtype) and m.table_bytes == V * ROW_BYTES[dtype]
            got, _ = m.embed(ids, offsets, max_tokens=2048)
            assert np.array_equal(_bits(got), _bits(want))
        with pytest.raises(L.SmtError):      # a file that ends inside the table is an I/O error, not a short table
            smt.Model.from_file(gpu_ctx, path, 37 + 64, V, normalize=True, dtype=dtype)
    finally:
        from_file.close()
        from_dev.close()


def test_append_from_a_typed_model_then_search(typed, gpu_ctx):
    import semtools_amd as smt

    dtype, _, models = typed
    ids, offsets = lines_of("border")
    ref = reference(dtype, "border", True, 2048)
    c = smt.Corpus(gpu_ctx)
    try:
        _, first = models[True].embed(ids, offsets, max_tokens=2048, append_to=c, want_host=False)
        assert first == 0 and c.rows == 17
        assert np.array_equal(_bits(c.read_rows(0, 17)), _bits(ref))
        q = ref[15]
        rows, dist = c.search(q, top_k=3)[0]
        res = orc.search_documents(np.asarray(ref), [17], q, 0, 3, accurate=True)
        assert rows.tolist() == [r["match_line"] for r in res] and rows[0] == 15
        assert np.allclose(dist, [r["distance"] for r in res], rtol=0, atol=1e-6)
    finally:
        c.close()


def test_a_logical_group_of_three_shards_gives_the_one_gpu_rows(typed):
    import semtools_amd as smt
    from semtools_amd import _lib as L

    dtype, stored, models = typed
    group = smt.Group.logical(0, 3)
    try:
        h = C.c_void_p()
        assert L.lib().smt_sharded_model_create_typed(group._h, L.np_ptr(stored), 5, V, 256, 1, C.byref(h)) == L.SMT_E_INVALID and not h
        sm = smt.ShardedModel(group, stored, normalize=True)
        assert sm.table_bytes == V * ROW_BYTES[dtype]
        for name in ("border", "ragged"):
            ids, offsets = lines_of(name)
            got, _ = sm.embed(ids, offsets, max_tokens=2048)
            assert np.array_equal(_bits(got), _bits(reference(dtype, name, True, 2048))), name
        sm.close()
    finally:
        group.close()


def _model_dir(tmp_path, stored):
    from safetensors.numpy import save_file

    d = tmp_path / "m"
    d.mkdir()
    save_file({"embeddings": stored}, str(d / "model.safetensors"))
    (d / "vocab.txt").write_text("".join(f"w{i}\n" for i in range(V - 1)) + "[UNK]\n")
    (d / "config.json").write_text(json.dumps({"normalize": True, "unk_token": "[UNK]"}))
    return d


def _host_reference(stored, lines):
    ids, offsets = [], [0]
    for ln in lines:
        ids += [int(w[1:]) for w in ln.split() if w.startswith("w") and w[1:].isdigit() and int(w[1:]) < V - 1]
        offsets.append(len(ids))
    return orc.embed_lines(stored.astype(np.float32), np.array(ids, np.uint32), np.array(offsets, np.uint64), True, 2048)


@pytest.mark.parametrize("where", ["one_gpu", "three_shards"])
def test_host_layer_keeps_f16_and_i8_directories_as_stored(typed, gpu_ctx, tmp_path, where):
    """A model directory with an F16 / I8 table: a handful of lines is served from a compact table of the rows they touch (read
    from the file in the stored type; the whole table is not resident afterwards), more than 32 768 lines upload the whole table
    -- as stored, so the model reports V x 512 / V x 256 bytes.  Both give the oracle's rows on the widened table."""
    import semtools_amd as smt
    from semtools_amd import host

    dtype, stored, _ = typed
    d = _model_dir(tmp_path, stored)
    group = smt.Group.logical(0, 3) if where == "three_shards" else None
    m = host.StaticModel(group if group is not None else gpu_ctx, model_dir=d)
    try:
        few = ["w0 w1 w2 w3 w4 w5 w6 w7", "w6 w7", "", "w1 w1 w2 nothing w298", "w4 w5 w4", "w17"]
        got = m.encode_with_args(few, 2048)
        assert np.array_equal(_bits(got), _bits(_host_reference(stored, few)))
        assert m.table_info() == (np.dtype(dtype), V, V * ROW_BYTES[dtype], False)
        rng = np.random.default_rng(8)
        n = 33_000
        toks = rng.integers(0, V - 1, size=(n, 3))
        many = [f"w{a} w{b} w{c}" for a, b, c in toks]
        many[100] = ""
        got = m.encode_with_args(many, 2048)
        assert np.array_equal(_bits(got), _bits(_host_reference(stored, many)))
        assert m.table_info() == (np.dtype(dtype), V, V * ROW_BYTES[dtype], True)
        assert m.table_bytes == V * ROW_BYTES[dtype]
    finally:
        m.close()
        if group is not None:
            group.close()
