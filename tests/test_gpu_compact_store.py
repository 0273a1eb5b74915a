"""The workspace store's compaction (Store::compact_if_sparse) through the in-place device path: enough edits to cross the
4096-dead-rows trigger, then the persisted rows, the extent table and the search output are compared with the oracle and with a
workspace built fresh from the final files.  One GPU, and three logical shards (what SEMTOOLS_DEVICES=0:3 gives the CLI)."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import synth

pytestmark = pytest.mark.gpu

V = 20000


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    """A synthetic potion-style model on disk: model.safetensors (embeddings [V,256] f32), vocab.txt, config.json."""
    from safetensors.numpy import save_file

    d = tmp_path_factory.mktemp("model")
    table = synth.table(V, seed=2)
    save_file({"embeddings": table}, str(d / "model.safetensors"))
    (d / "vocab.txt").write_text("".join(f"w{i}\n" for i in range(V - 1)) + "[UNK]\n")
    (d / "config.json").write_text(json.dumps({"normalize": True, "unk_token": "[UNK]"}))
    return d, table


@pytest.fixture(scope="module", params=["one_gpu", "three_shards"])
def model(request, gpu_ctx, model_dir):
    import semtools_amd as smt
    from semtools_amd import host

    group = smt.Group.logical(0, 3) if request.param == "three_shards" else None
    m = host.StaticModel(group if group is not None else gpu_ctx, model_dir=model_dir[0])
    m.contexts = [group.ctx(i) for i in range(3)] if group is not None else [gpu_ctx]
    yield m
    m.close()
    if group is not None:
        group.close()


def tok(text):
    out = []
    for w in text.split():
        if w.startswith("w") and w[1:].isdigit() and int(w[1:]) < V - 1 and str(int(w[1:])) == w[1:]:
            out.append(int(w[1:]))
    return out


def oracle_embed(table, lines):
    ids, offsets = [], [0]
    for ln in lines:
        ids += tok(ln)
        offsets.append(len(ids))
    return orc.embed_lines(table, np.array(ids, np.uint32), np.array(offsets, np.uint64), True, 2048)


def write(path, lines, mtime):
    path.write_text("\n".join(lines) + "\n")
    os.utime(path, (mtime, mtime))


def stored(gpu_ctx, root):
    import semtools_amd as smt

    c = smt.Corpus.load(gpu_ctx, str(root / "line_embeddings.f32"))
    rows = c.read_rows(0, c.rows)
    c.close()
    ext = {e["path"]: (e["first_row"], e["n_rows"]) for e in json.loads((root / "line_rows.json").read_text())["extents"]}
    return rows, ext


def test_edits_past_the_trigger_compact_on_the_device(gpu_ctx, model, model_dir, tmp_path, monkeypatch, capfd):
    from semtools_amd import host

    monkeypatch.setenv("HOME", str(tmp_path))
    monkeypatch.delenv("SEMTOOLS_WORKSPACE", raising=False)
    table = model_dir[1]
    names = ("a", "b", "c", "d")
    lines = dict(a=synth.pseudo_prose(2500, vocab_size=V - 1, seed=3), b=synth.pseudo_prose(40, vocab_size=V - 1, seed=5),
                 c=synth.pseudo_prose(2500, vocab_size=V - 1, seed=4), d=synth.pseudo_prose(30, vocab_size=V - 1, seed=6))
    paths = {k: tmp_path / f"{k}.txt" for k in names}
    for k in names:
        write(paths[k], lines[k], 1_800_000_000)
    files = [str(paths[k]) for k in names]
    query = lines["b"][7]
    host.workspace_use(None, "cp")
    host.search_with_workspace(model, query, files, workspace_name="cp", n_lines=0, top_k=5)
    root = tmp_path / ".semtools" / "workspaces" / "cp"
    rows, ext = stored(gpu_ctx, root)
    assert len(rows) == 5070
    for ctx in model.contexts:
        ctx.compact_stats(reset=True)
    # both large files shrink: 5000 dead rows of 7570 -- past 4096 and past half of the matrix
    lines["a"] = lines["a"][100:1300]
    lines["c"] = lines["c"][:1299] + ["w1 w2 w3 w4"]
    write(paths["a"], lines["a"], 1_800_000_100)
    write(paths["c"], lines["c"], 1_800_000_100)
    out = host.search_with_workspace(model, query, files, workspace_name="cp", n_lines=0, top_k=5)
    assert "Updating workspace with 2500 lines" in capfd.readouterr().err
    for ctx in model.contexts:
        assert ctx.compact_stats().calls >= 1          # the in-place path ran on every shard's context
    assert sum(ctx.compact_stats().rows_moved for ctx in model.contexts) > 0
    rows, ext = stored(gpu_ctx, root)
    assert len(rows) == 40 + 30 + 1200 + 1300          # the live rows only
    # extents back to back from row 0; the surviving documents (b, d) come first, the re-embedded ones (a, c) behind them
    order = sorted(ext.items(), key=lambda kv: kv[1][0])
    at = 0
    for _, (f0, n) in order:
        assert f0 == at
        at += n
    assert at == len(rows) and {p for p, _ in order[:2]} == {str(paths["b"]), str(paths["d"])}
    assert {k: ext[str(paths[k])][1] for k in names} == dict(a=1200, b=40, c=1300, d=30)
    for k in names:
        f0, n = ext[str(paths[k])]
        assert np.array_equal(rows[f0:f0 + n].view(np.uint32), oracle_embed(table, lines[k]).view(np.uint32)), k
    # the same files in a workspace built fresh: the same search output
    host.workspace_use(None, "fresh")
    want = host.search_with_workspace(model, query, files, workspace_name="fresh", n_lines=0, top_k=5)
    assert out == want and out.startswith(f"{paths['b']}:7::8 (")
    host.workspace_use(None, "cp")
    assert host.search_with_workspace(model, query, files, workspace_name="cp", n_lines=0, top_k=5) == want   # (reloaded from disk)


def test_lopsided_compaction_goes_through_the_host(gpu_ctx, model_dir, tmp_path, monkeypatch, capfd):
    """When nearly every live row would sit on one shard, the store deals the rows again through the host (the 1.5 x policy of
    Store::compact_in_place) instead of compacting in place: same persisted rows either way."""
    import semtools_amd as smt
    from semtools_amd import host

    monkeypatch.setenv("HOME", str(tmp_path))
    monkeypatch.delenv("SEMTOOLS_WORKSPACE", raising=False)
    table = model_dir[1]
    group = smt.Group.logical(0, 3)
    model = host.StaticModel(group, model_dir=model_dir[0])
    model.contexts = [group.ctx(i) for i in range(3)]
    la, lb = synth.pseudo_prose(4500, vocab_size=V - 1, seed=8), synth.pseudo_prose(60, vocab_size=V - 1, seed=9)
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    write(a, la, 1_800_000_000)
    write(b, lb, 1_800_000_000)
    files = [str(a), str(b)]
    host.workspace_use(None, "lop")
    host.search_with_workspace(model, lb[3], files, workspace_name="lop", n_lines=0, top_k=3)
    for ctx in model.contexts:
        ctx.compact_stats(reset=True)
    la = la[:10]
    write(a, la, 1_800_000_100)
    out = host.search_with_workspace(model, lb[3], files, workspace_name="lop", n_lines=0, top_k=3)
    capfd.readouterr()
    assert all(ctx.compact_stats().calls == 0 for ctx in model.contexts)
    rows, ext = stored(gpu_ctx, tmp_path / ".semtools" / "workspaces" / "lop")
    assert len(rows) == 70 and ext[str(b)] == (0, 60) and ext[str(a)] == (60, 10)   # the survivor first, the re-embedded file behind it
    assert np.array_equal(rows.view(np.uint32), np.concatenate([oracle_embed(table, lb), oracle_embed(table, la)]).view(np.uint32))
    assert out.startswith(f"{b}:3::4 (")
    model.close()
    group.close()
