"""GPU: the host layer with the device tokenizer route off, on in its ASCII form (1) and on in its UTF-8 form (2) for XLM-R-style
tokenizer.json files -- a Precompiled normalizer and the regex Replace in front of Metaspace, in the shape with a WhitespaceSplit (A)
and the shape with a Strip (B): rows, search output, the workspace's files and its cached token ids are the same bytes for all three
settings; the lines tokenized on the device are exactly those tests/precompiled_ref.py calls covered; a group of three shards keeps
the host path.  The model directory holds the vocabulary of tests/precompiled_ref.py and a small random table.  Reads the character
map of tests/golden and the library only."""
import json

import numpy as np
import pytest

from tests import precompiled_ref as P
from tests import synth

pytestmark = pytest.mark.gpu

SHAPES = ["A_ws", "B"]
VOCAB = P.build_vocab()
MEDIAN = max(1, sorted(len(p.encode()) for p, _ in VOCAB)[len(VOCAB) // 2])   # model2vec's median token length, bytes


def _dir(root, seed, shape):
    from safetensors.numpy import save_file

    root.mkdir()
    save_file({"embeddings": synth.table(len(VOCAB), seed=seed)}, str(root / "model.safetensors"))
    (root / "tokenizer.json").write_text(json.dumps(P.tokenizer_json(shape)))
    (root / "config.json").write_text(json.dumps({"normalize": True, "unk_token": "<unk>"}))
    return root


@pytest.fixture(scope="module")
def model_dirs(tmp_path_factory):
    base = tmp_path_factory.mktemp("pre_models")
    return {s: (_dir(base / (s + "_v1"), 5, s), _dir(base / (s + "_v2"), 79, s)) for s in SHAPES}


def _lines(n, seed):
    """the generator's lines, no line break inside a line; every 25th line something no form covers -- a combining mark, a character
    that outgrows its bytes, an added token, a run over the measure, a line of spaces -- or nothing"""
    odd = ["the café fox", "the ½ fox", "x<pad>y café", "", "the" + " " * 70 + "fox", "   "]
    out = []
    for i, raw in enumerate(P.lines(seed, n)):
        s = raw.decode().replace("\n", " ").replace("\r", " ")
        out.append(odd[(i // 25) % len(odd)] if i % 25 == 24 else s)
    return out


def _covered(lines, max_length, shape, utf8):
    ref = P.PrecompiledRef(P.tokenizer_json(shape), utf8=utf8)
    return sum(not ref.line(s.encode(), keep_bytes=max_length * MEDIAN)[1] for s in lines)


def _model(ctx, d, mode):
    from semtools_amd import host

    return host.StaticModel(ctx, model_dir=d, device_tokenizer=mode)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("max_length", [2048, 5])
def test_rows_are_equal_and_the_counts_are_the_references(gpu_ctx, model_dirs, monkeypatch, max_length, shape):
    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    lines = _lines(1200, seed=51)
    models = {mode: _model(gpu_ctx, model_dirs[shape][0], mode) for mode in (0, 1, 2)}
    try:
        rows = {mode: m.encode_with_args(lines, max_length) for mode, m in models.items()}
        assert np.array_equal(rows[1], rows[0]) and np.array_equal(rows[2], rows[0]) and np.abs(rows[0]).sum() > 0
        n0, n1, n2 = (models[mode].device_tokenized_lines() for mode in (0, 1, 2))
        want1, want2 = _covered(lines, max_length, shape, False), _covered(lines, max_length, shape, True)
        print("device-tokenized lines of 1200:", shape, "off", n0, "ascii form", n1, "utf-8 form", n2)
        assert n0 == 0 and n1 == want1 and n2 == want2
        assert n2 > n1 > 0 and (max_length == 5 or n2 > 1000)
    finally:
        for m in models.values():
            m.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_search_and_workspace_bytes_do_not_depend_on_the_setting(gpu_ctx, model_dirs, tmp_path, monkeypatch, capfd, shape):
    from semtools_amd import host

    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    monkeypatch.delenv("SEMTOOLS_WORKSPACE", raising=False)
    lines = _lines(500, seed=55)
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    a.write_bytes(("\n".join(lines[:300]) + "\n").encode())
    b.write_bytes(("\n".join(lines[300:]) + "\n").encode())
    files = [str(a), str(b)]
    query = "the  привет ｆｕｌｌ fox "
    seen = {}
    for mode in (0, 1, 2):
        home = tmp_path / ("home%d" % mode)
        home.mkdir()
        monkeypatch.setenv("HOME", str(home))
        m, m2 = _model(gpu_ctx, model_dirs[shape][0], mode), _model(gpu_ctx, model_dirs[shape][1], mode)
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


def test_a_group_of_three_shards_keeps_the_host_path(gpu_ctx, model_dirs, monkeypatch):
    import semtools_amd as smt

    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    lines = _lines(600, seed=46)
    one = _model(gpu_ctx, model_dirs["A_ws"][0], 0)
    group = smt.Group.logical(0, 3)
    three = _model(group, model_dirs["A_ws"][0], 2)
    try:
        assert np.array_equal(three.encode_with_args(lines, 2048), one.encode_with_args(lines, 2048))
        assert three.device_tokenized_lines() == 0
    finally:
        one.close()
        three.close()
        group.close()
