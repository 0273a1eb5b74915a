"""GPU: the host layer's device tokenizer route with the long-piece switch (smt_host_model_set_device_tokenizer_long,
SEMTOOLS_DEVICE_TOKENIZER_LONG) off and on for an XLM-R-style tokenizer.json -- a Precompiled normalizer over the character map of
tests/golden and the regex Replace in front of Metaspace, so the route's handle has its space rules on -- for device tokenizer 1 and
2, on a document that mixes the generator's lines with URL-like words of 65 .. 300 bytes and CJK lines written without spaces:
rows, search output, the workspace's files and its cached token ids are the same bytes as with the route off; the lines tokenized on
the device are exactly those the references call covered -- tests/precompiled_ref.py with the switch off,
tests/unigram_long_rules_ref.py with it on, where the URL and CJK lines are among them."""
import json
import random

import numpy as np
import pytest

from tests import precompiled_ref as P
from tests import synth
from tests import unigram_long_ref as LR
from tests import unigram_long_rules_ref as Q

pytestmark = pytest.mark.gpu

SHAPE = "A_ws"
VOCAB = Q.build_vocab()
MEDIAN = max(1, sorted(len(p.encode()) for p, _ in VOCAB)[len(VOCAB) // 2])   # model2vec's median token length, bytes
SETTINGS = [(0, False), (1, False), (1, True), (2, False), (2, True)]


def _dir(root, seed, shape=SHAPE):
    from safetensors.numpy import save_file

    root.mkdir()
    save_file({"embeddings": synth.table(len(VOCAB), seed=seed)}, str(root / "model.safetensors"))
    (root / "tokenizer.json").write_text(json.dumps(Q.tokenizer_json(shape)))
    (root / "config.json").write_text(json.dumps({"normalize": True, "unk_token": "<unk>"}))
    return root


@pytest.fixture(scope="module")
def model_dirs(tmp_path_factory):
    base = tmp_path_factory.mktemp("prel_models")
    return _dir(base / "v1", 5), _dir(base / "v2", 79), _dir(base / "b1", 5, "B")


def _lines(n, seed):
    """of every ten lines: seven of the generator of tests/precompiled_ref.py (mixed scripts, doubled spaces), two with a URL-like
    word of 65 .. 300 bytes behind a doubled space, one CJK line without spaces (30 .. 600 bytes, doubled spaces at either end);
    every 50th line something no form covers (an added token, a piece over 2048 bytes, a combining mark inside a long piece)"""
    rng = random.Random(seed)
    out = []
    for i, raw in enumerate(P.lines(seed, n)):
        s, k = raw.decode().replace("\n", " ").replace("\r", " "), i % 10
        if i % 50 == 49:
            s = ["x<pad>y " + "thefox" * 20, "the " + "abcd" * 600 + " fox", "the " + "abcd" * 20 + "é fox"][(i // 50) % 3]
        elif k in (3, 7):
            url = "https://example.org/" + "/".join(rng.choice(LR.KNOWN_WORDS) + rng.choice(["", "-12", "_a1b2"]) for _ in range(rng.randint(8, 40)))
            s = s[:40] + "  " + url[: rng.randint(65, 300)] + " " + s[40:70]
        elif k == 5:
            s = rng.choice(["", "  "]) + "".join(rng.choice(["中文", "中", "文", "中文中"]) for _ in range(rng.randint(8, 100))) + rng.choice(["", "  "])
        out.append(s)
    return out


def _covered(lines, max_length, utf8, long_pieces, shape=SHAPE):
    tj = Q.tokenizer_json(shape)
    ref = Q.LongRulesRef(tj, utf8=utf8) if long_pieces else P.PrecompiledRef(tj, utf8=utf8)
    return sum(not ref.line(s.encode(), keep_bytes=max_length * MEDIAN)[1] for s in lines)


def _model(ctx, d, mode, long_pieces):
    from semtools_amd import host

    m = host.StaticModel(ctx, model_dir=d, device_tokenizer=mode)
    if long_pieces is not None:
        m.set_device_tokenizer_long(long_pieces)
    return m


@pytest.mark.parametrize("shape", ["A_ws", "B"])
def test_rows_are_equal_and_the_counts_are_the_references(gpu_ctx, model_dirs, monkeypatch, shape):
    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    lines, max_length = _lines(1000, seed=61), 2048
    d = model_dirs[0] if shape == "A_ws" else model_dirs[2]
    models = {s: _model(gpu_ctx, d, *s) for s in SETTINGS}
    try:
        rows = {s: m.encode_with_args(lines, max_length) for s, m in models.items()}
        for s in SETTINGS[1:]:
            assert np.array_equal(rows[s], rows[SETTINGS[0]]), s
        assert np.abs(rows[SETTINGS[0]]).sum() > 0
        got = {s: models[s].device_tokenized_lines() for s in SETTINGS}
        want = {(mode, lp): _covered(lines, max_length, mode == 2, lp, shape) for mode, lp in SETTINGS[1:]}
        print("device-tokenized lines of", len(lines), shape, got)
        assert got[(0, False)] == 0
        for s in SETTINGS[1:]:
            assert got[s] == want[s], (s, got, want)
        # the lines with a URL-like word are the device's under both forms, the CJK lines under the UTF-8 form
        assert got[(1, True)] >= got[(1, False)] + 50 and got[(2, True)] >= got[(2, False)] + 250 and got[(2, True)] >= len(lines) * 0.88
    finally:
        for m in models.values():
            m.close()


def test_switching_and_the_environment(gpu_ctx, model_dirs, monkeypatch):
    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    lines = ["the quick  fox", "see  " + "thefox" * 20, "  " + "中文" * 30, "the ｆｕｌｌ text "]
    m = _model(gpu_ctx, model_dirs[0], 2, False)
    try:
        a = m.encode_with_args(lines, 512)
        assert m.device_tokenized_lines() == 2
        m.set_device_tokenizer_long(True)          # the route is made anew with the switch (its counter starts again)
        b = m.encode_with_args(lines, 512)
        assert m.device_tokenized_lines() == 4 and np.array_equal(a, b)
    finally:
        m.close()
    monkeypatch.setenv("SEMTOOLS_DEVICE_TOKENIZER", "1")
    monkeypatch.setenv("SEMTOOLS_DEVICE_TOKENIZER_LONG", "1")
    m = _model(gpu_ctx, model_dirs[0], None, None)
    try:
        c = m.encode_with_args(lines, 512)
        assert m.device_tokenized_lines() == 2 and np.array_equal(a, c)     # the ASCII form: the two non-ASCII lines stay the host's
    finally:
        m.close()


def test_search_and_workspace_bytes_do_not_depend_on_the_switch(gpu_ctx, model_dirs, tmp_path, monkeypatch, capfd):
    from semtools_amd import host

    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    monkeypatch.delenv("SEMTOOLS_WORKSPACE", raising=False)
    lines = _lines(500, seed=65)
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    a.write_bytes(("\n".join(lines[:300]) + "\n").encode())
    b.write_bytes(("\n".join(lines[300:]) + "\n").encode())
    files = [str(a), str(b)]
    query = "the  search 中文 ｆｕｌｌ fox "
    seen = {}
    for s in SETTINGS:
        home = tmp_path / ("home%d%d" % s)
        home.mkdir()
        monkeypatch.setenv("HOME", str(home))
        m, m2 = _model(gpu_ctx, model_dirs[0], *s), _model(gpu_ctx, model_dirs[1], *s)
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
            seen[s] = out, m.device_tokenized_lines()
        finally:
            m.close()
            m2.close()
    capfd.readouterr()
    assert seen[(0, False)][1] == 0 and seen[(1, True)][1] > seen[(1, False)][1] > 0 and seen[(2, True)][1] > seen[(2, False)][1] > 0
    for s in SETTINGS[1:]:
        for x, y in zip(seen[SETTINGS[0]][0], seen[s][0]):
            assert x == y, s
    assert len(seen[SETTINGS[0]][0][3]) > 0 and len(seen[SETTINGS[0]][0][4]) > 0
