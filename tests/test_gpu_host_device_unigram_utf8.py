"""GPU: the host layer with the device tokenizer route off, on in its ASCII form (1) and on in its UTF-8 form (2,
smt_host_model_set_device_tokenizer) for a Unigram tokenizer.json: rows, search output, the workspace's files and its cached token
ids are the same bytes for all three; with 2 the lines tokenized on the device are exactly those tests/unigram_utf8_ref.py calls
covered, with 1 exactly those tests/unigram_ref.py does.  The model directory holds a hand-written tokenizer.json with the non-ASCII
vocabulary of tests/unigram_utf8_ref.py and a small random table."""
import json

import numpy as np
import pytest

from tests import synth
from tests import unigram_ref as U
from tests import unigram_utf8_ref as G

pytestmark = pytest.mark.gpu

NORM, PREPEND = "bert_clean", "always"
VOCAB = G.build_vocab()
MEDIAN = max(1, sorted(len(p.encode()) for p, _ in VOCAB)[len(VOCAB) // 2])   # model2vec's median token length, bytes


def _dir(root, seed):
    from safetensors.numpy import save_file

    root.mkdir()
    save_file({"embeddings": synth.table(len(VOCAB), seed=seed)}, str(root / "model.safetensors"))
    (root / "tokenizer.json").write_text(json.dumps(G.tokenizer_json(norm=NORM, prepend=PREPEND)))
    (root / "config.json").write_text(json.dumps({"normalize": True, "unk_token": "<unk>"}))
    return root


@pytest.fixture(scope="module")
def model_dirs(tmp_path_factory):
    base = tmp_path_factory.mktemp("ug8_models")
    return _dir(base / "v1", 5), _dir(base / "v2", 79)


def _lines(n, seed):
    """the mixed generator (a quarter pure ASCII), no line break inside a line; every 25th line something no form covers -- a
    Chinese character, a code point whose output keeps a combining class, an added token, a piece over the length limit -- or nothing"""
    odd = ["the 中文 fox", "the \u302e fox", "x<pad>y café", "", "the " + "м" * 40 + " fox"]
    out = []
    for i, raw in enumerate(G.utf8_lines(seed, n)):
        s = raw.decode().replace("\n", " ").replace("\r", " ")
        out.append(odd[(i // 25) % len(odd)] if i % 25 == 24 else s)
    return out


def _covered(lines, max_length, utf8):
    tj = G.tokenizer_json(norm=NORM, prepend=PREPEND)
    ref = G.UnigramUtf8Ref(tj, blocks=None) if utf8 else U.UnigramRef(tj)
    return sum(not ref.line(s.encode(), keep_bytes=max_length * MEDIAN)[1] for s in lines)


def _model(ctx, d, mode):
    from semtools_amd import host

    return host.StaticModel(ctx, model_dir=d, device_tokenizer=mode)


@pytest.mark.parametrize("max_length", [2048, 5])
def test_rows_are_equal_and_the_counts_are_the_references(gpu_ctx, model_dirs, monkeypatch, max_length):
    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    lines = _lines(3000, seed=51)
    models = {mode: _model(gpu_ctx, model_dirs[0], mode) for mode in (0, 1, 2)}
    try:
        rows = {mode: m.encode_with_args(lines, max_length) for mode, m in models.items()}
        assert np.array_equal(rows[1], rows[0]) and np.array_equal(rows[2], rows[0]) and np.abs(rows[0]).sum() > 0
        n0, n1, n2 = (models[mode].device_tokenized_lines() for mode in (0, 1, 2))
        want1, want2 = _covered(lines, max_length, False), _covered(lines, max_length, True)
        print("device-tokenized lines of 3000: off", n0, "ascii form", n1, "utf-8 form", n2)
        assert n0 == 0 and n1 == want1 and n2 == want2
        assert n2 > n1 and (max_length == 5 or (n1 < 1000 and n2 > 2400))
    finally:
        for m in models.values():
            m.close()


def test_switching_a_model_between_the_forms(gpu_ctx, model_dirs, monkeypatch):
    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    lines = ["the quick fox", "café the", "привет мир", "中文 again"]
    m = _model(gpu_ctx, model_dirs[0], 1)
    try:
        a = m.encode_with_args(lines, 512)
        assert m.device_tokenized_lines() == 1
        m.set_device_tokenizer(2)                  # the route is made anew for the other form (its counter starts again)
        b = m.encode_with_args(lines, 512)
        assert m.device_tokenized_lines() == 3 and np.array_equal(a, b)       # (the Chinese characters stay the host's)
    finally:
        m.close()


def test_the_environment_value_2(gpu_ctx, model_dirs, monkeypatch):
    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    monkeypatch.setenv("SEMTOOLS_DEVICE_TOKENIZER", "2")
    m = _model(gpu_ctx, model_dirs[0], None)
    try:
        m.encode_with_args(["the quick fox", "café again", "the \u302e fox"], 512)
        assert m.device_tokenized_lines() == 2
    finally:
        m.close()


def test_search_and_workspace_bytes_do_not_depend_on_the_setting(gpu_ctx, model_dirs, tmp_path, monkeypatch, capfd):
    from semtools_amd import host

    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    monkeypatch.delenv("SEMTOOLS_WORKSPACE", raising=False)
    lines = _lines(700, seed=55)
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    a.write_bytes(("\n".join(lines[:400]) + "\n").encode())
    b.write_bytes(("\n".join(lines[400:]) + "\n").encode())
    files = [str(a), str(b)]
    query = "the привет café fox"
    seen = {}
    for mode in (0, 1, 2):
        home = tmp_path / ("home%d" % mode)
        home.mkdir()
        monkeypatch.setenv("HOME", str(home))
        m, m2 = _model(gpu_ctx, model_dirs[0], mode), _model(gpu_ctx, model_dirs[1], mode)
        try:
            out = [host.search_content(m, query, "\n".join(lines), n_lines=1, top_k=5),
                   host.search_files(m, query, files, n_lines=0, top_k=4, ignore_case=True)]
            host.workspace_use(None, "ws")
            out.append(host.search_with_workspace(m, query, files, workspace_name="ws", n_lines=0, top_k=5))     # ingest
            root = home / ".semtools" / "workspaces" / "ws"
            out.append((root / "line_tokens.log").read_bytes())
            out.append((root / "line_embeddings.f32").read_bytes())
            out.append(host.workspace_reembed(m2, "ws"))                                                        # from the cached ids
            out.append((root / "line_embeddings.f32").read_bytes())
            out.append(host.search_with_workspace(m2, query, files, workspace_name="ws", n_lines=0, top_k=5))
            seen[mode] = out, m.device_tokenized_lines()
        finally:
            m.close()
            m2.close()
    capfd.readouterr()
    assert seen[0][1] == 0 and seen[2][1] > seen[1][1] > 0
    for mode in (1, 2):
        for x, y in zip(seen[0][0], seen[mode][0]):
            assert x == y, mode
    assert len(seen[0][0][3]) > 0 and len(seen[0][0][4]) > 0
