"""GPU: the host layer with the device tokenizer route off and on for a Unigram tokenizer.json (include/semtools_host.h
smt_host_model_set_device_tokenizer): rows, search output, the workspace's files and its cached token ids must be the same bytes
either way; the route must really be taken when the table is resident (debug counter of device-tokenized lines), and must not be
for a lazy table or a group of several ranks.  The model directory holds a hand-written tokenizer.json (tests/unigram_ref.py) and a
small random table."""
import json

import numpy as np
import pytest

from tests import synth
from tests import unigram_ref as U

pytestmark = pytest.mark.gpu

NORM, PREPEND = "bert_clean", "always"
VOCAB = U.build_vocab()
MEDIAN = max(1, sorted(len(p.encode()) for p, _ in VOCAB)[len(VOCAB) // 2])   # model2vec's median token length, bytes


def _dir(root, seed):
    from safetensors.numpy import save_file

    root.mkdir()
    save_file({"embeddings": synth.table(len(VOCAB), seed=seed)}, str(root / "model.safetensors"))
    U.write_tokenizer(root / "tokenizer.json", norm=NORM, prepend=PREPEND)
    (root / "config.json").write_text(json.dumps({"normalize": True, "unk_token": "<unk>"}))
    return root


@pytest.fixture(scope="module")
def model_dirs(tmp_path_factory):
    base = tmp_path_factory.mktemp("ug_models")
    return _dir(base / "v1", 3), _dir(base / "v2", 77)


def _mixed_lines(n, seed):
    """mostly ASCII (words and draws from every ASCII byte, added tokens and unknown characters among them), every fifth line
    something the kernel flags or an empty line: Latin-1, CJK, an added token, a word over the length limit"""
    odd = ["café au lait, naïve façade the fox", "中文字符 the text 日本語のテキスト", "x<pad>y the <unk> fox", "", "the search fox é",
           "a" * 101 + " Ünïcödé", "   ", "the " + "ab" * 40 + " fox"]
    out = []
    for i, raw in enumerate(U.ascii_lines(seed, n)):
        out.append(odd[(i // 5) % len(odd)] if i % 5 == 4 else raw.decode().replace("\n", " ").replace("\r", " "))
    return out


def _covered(lines, max_length):
    ref = U.UnigramRef(U.tokenizer_json(norm=NORM, prepend=PREPEND))
    return sum(not ref.line(s.encode(), keep_bytes=max_length * MEDIAN)[1] for s in lines)


def _model(ctx, d, on):
    from semtools_amd import host

    return host.StaticModel(ctx, model_dir=d, device_tokenizer=on)


def test_rows_are_the_same_and_a_lazy_table_keeps_the_host_path(gpu_ctx, model_dirs, monkeypatch):
    monkeypatch.delenv("SEMTOOLS_EAGER_MODEL", raising=False)
    lines = _mixed_lines(2000, seed=41)
    off, on = _model(gpu_ctx, model_dirs[0], False), _model(gpu_ctx, model_dirs[0], True)
    try:
        assert not on.table_info()[3]                # nothing is resident yet: the call below decides from the ids what to upload
        want = off.encode_with_args(lines, 2048)
        got = on.encode_with_args(lines, 2048)
        assert np.array_equal(got, want) and np.abs(want).sum() > 0
        assert on.device_tokenized_lines() == 0      # a call that starts on a lazy table needs its ids on the host
    finally:
        off.close()
        on.close()


@pytest.mark.parametrize("max_length", [2048, 5])
def test_resident_table_takes_the_device_route(gpu_ctx, model_dirs, monkeypatch, max_length):
    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    lines = _mixed_lines(2000, seed=42)
    off, on = _model(gpu_ctx, model_dirs[0], False), _model(gpu_ctx, model_dirs[0], True)
    try:
        want = off.encode_with_args(lines, max_length)
        got = on.encode_with_args(lines, max_length)
        assert np.array_equal(got, want)
        assert off.device_tokenized_lines() == 0
        assert on.table_info()[3] and on.device_tokenized_lines() == _covered(lines, max_length) > 1000
    finally:
        off.close()
        on.close()


def test_search_and_workspace_bytes_do_not_depend_on_the_switch(gpu_ctx, model_dirs, tmp_path, monkeypatch, capfd):
    from semtools_amd import host

    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    monkeypatch.delenv("SEMTOOLS_WORKSPACE", raising=False)
    lines = _mixed_lines(700, seed=45)
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    a.write_text("\n".join(lines[:400]) + "\n")
    b.write_text("\n".join(lines[400:]) + "\n")
    files = [str(a), str(b)]
    query = "the search text fox"
    seen = {}
    for name, on in (("off", False), ("on", True)):
        home = tmp_path / name
        home.mkdir()
        monkeypatch.setenv("HOME", str(home))
        m, m2 = _model(gpu_ctx, model_dirs[0], on), _model(gpu_ctx, model_dirs[1], on)
        try:
            out = [host.search_content(m, query, "\n".join(lines), n_lines=1, top_k=5),
                   host.search_files(m, query, files, n_lines=0, top_k=4, ignore_case=True)]
            host.workspace_use(None, "ws")
            out.append(host.search_with_workspace(m, query, files, workspace_name="ws", n_lines=0, top_k=5))     # ingest: the TokenCsr sink
            root = home / ".semtools" / "workspaces" / "ws"
            out.append((root / "line_tokens.log").read_bytes())                                                 # the cached ids and lengths
            out.append((root / "line_embeddings.f32").read_bytes())
            out.append(host.workspace_reembed(m2, "ws"))                                                        # from the cached ids
            out.append((root / "line_embeddings.f32").read_bytes())
            out.append(host.search_with_workspace(m2, query, files, workspace_name="ws", n_lines=0, top_k=5))
            seen[name] = out, m.device_tokenized_lines()
        finally:
            m.close()
            m2.close()
    capfd.readouterr()
    assert seen["off"][1] == 0 and seen["on"][1] >= _covered(lines, 2048) > 400
    for x, y in zip(seen["off"][0], seen["on"][0]):
        assert x == y
    assert seen["on"][0][5].startswith("Re-embedded 700 lines of 2 documents")


def test_a_group_of_three_shards_keeps_the_host_path(gpu_ctx, model_dirs, monkeypatch):
    import semtools_amd as smt

    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    lines = _mixed_lines(2000, seed=46)
    one = _model(gpu_ctx, model_dirs[0], False)
    group = smt.Group.logical(0, 3)
    three = _model(group, model_dirs[0], True)
    try:
        assert np.array_equal(three.encode_with_args(lines, 2048), one.encode_with_args(lines, 2048))
        assert three.device_tokenized_lines() == 0
    finally:
        one.close()
        three.close()
        group.close()
