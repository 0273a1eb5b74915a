"""GPU: the workspace store carries its IVF index through Store::compact_in_place (smt_sharded_ivfpq_compact) instead of dropping it
and paying a rebuild at the next search.  One GPU and three logical shards.  The index files from before and after the compaction are
parsed: equal centroids prove that the index was carried (a rebuild on other rows gives other centroids), and the carried entries must
be tests/ivf_compact_ref.carry of the old file under the keep list read off line_rows.json."""
import json
import os

import numpy as np
import pytest

from tests import ivf_compact_ref as K
from tests import ivf_ref as R
from tests import synth
from tests.test_gpu_compact_store import stored, write
from tests.test_gpu_host import V, model, model_dir  # noqa: F401  (the fixtures of the host tests: one GPU / three shards)
from tests.test_gpu_ivf_compact_sharded import localize

pytestmark = pytest.mark.gpu

N_DOCS, DOC_LINES, NEW_LINES = 12, 1000, 150
UNTOUCHED = (1, 5, 9)                 # one document per shard's third of the rows: the in-place path stays balanced


def test_the_store_carries_its_index_through_a_compaction(gpu_ctx, model, tmp_path, monkeypatch, capfd):  # noqa: F811
    from semtools_amd import host

    monkeypatch.setenv("HOME", str(tmp_path))
    monkeypatch.delenv("SEMTOOLS_WORKSPACE", raising=False)
    monkeypatch.setenv("SEMTOOLS_INDEX_NPROBE", "512")
    paths = [tmp_path / f"doc{i:02d}.txt" for i in range(N_DOCS)]
    for i, p in enumerate(paths):
        write(p, synth.pseudo_prose(DOC_LINES, vocab_size=V - 1, seed=500 + i), 1_800_000_000)
    files = [str(p) for p in paths]
    query = synth.pseudo_prose(1, vocab_size=V - 1, seed=505)[0]
    host.workspace_use(None, "carry")
    root = tmp_path / ".semtools" / "workspaces" / "carry"
    cfg = json.loads((root / "config.json").read_text())
    cfg["oversample_factor"] = 64                       # rerank = min(512, 2 * top_k * oversample_factor) = 512 at top_k 5
    (root / "config.json").write_text(json.dumps(cfg))
    n = model.n_shards
    parts = [root / ("line_index.ivf" if n == 1 else f"line_index.ivf.r{r}of{n}") for r in range(n)]

    def search(min_rows):
        monkeypatch.setenv("SEMTOOLS_INDEX_MIN_ROWS", str(min_rows))
        return host.search_with_workspace(model, query, files, workspace_name="carry", n_lines=0, top_k=5)

    search(4000)                                        # 12 000 lines stored, the index built and saved
    assert all(p.exists() for p in parts)
    before = [R.read_index(p) for p in parts]
    rows_json = json.loads((root / "line_rows.json").read_text())
    gen_before = json.loads((root / "line_index.gen").read_text())["generation"]
    ext_before = {e["path"]: (e["first_row"], e["n_rows"]) for e in rows_json["extents"]}
    layout = [tuple(p) for p in rows_json["shards"]["pieces"]] if n > 1 else [(N_DOCS * DOC_LINES, 0)]
    assert sum(f["n_rows"] for f in before) == N_DOCS * DOC_LINES
    # nine documents shrink to 150 lines: 9 000 dead rows of 13 350 -- past 4 096 and past half
    for i, p in enumerate(paths):
        if i not in UNTOUCHED:
            write(p, synth.pseudo_prose(NEW_LINES, vocab_size=V - 1, seed=600 + i), 1_800_000_100)
    capfd.readouterr()
    got = search(4000)
    assert f"Updating workspace with {(N_DOCS - len(UNTOUCHED)) * NEW_LINES} lines" in capfd.readouterr().err
    live = len(UNTOUCHED) * DOC_LINES + (N_DOCS - len(UNTOUCHED)) * NEW_LINES
    rows, ext_after = stored(gpu_ctx, root)
    assert len(rows) == live                            # the compaction ran
    # the index files exist again, under the new generation
    assert all(p.exists() for p in parts) and not list(root.glob("line_index.ivf*.tmp"))
    gen_after = json.loads((root / "line_index.gen").read_text())
    assert gen_after["generation"] == json.loads((root / "line_rows.json").read_text())["generation"] > gen_before
    assert gen_after["n_ranks"] == n
    after = [R.read_index(p) for p in parts]
    for f in after:
        assert int(np.diff(f["offsets"].astype(np.int64)).max()) <= 512
    assert sum(f["n_rows"] for f in after) == live      # ... and the re-embedded rows were appended to it
    # carried, not rebuilt: the quantisers are the old ones, byte for byte
    for b, a in zip(before, after):
        for name in ("centroids", "cnorm_half", "codebooks", "basis", "lscale"):
            assert a[name].tobytes() == b[name].tobytes(), name
    # the keep list the store used: the extents, as they were, of the documents whose extent kept its length and came to the front
    survivors = sorted((ext_before[files[i]] for i in UNTOUCHED))
    keep = [(f0, f0 + cnt) for f0, cnt in survivors]
    at = 0
    for i in sorted(UNTOUCHED, key=lambda i: ext_before[files[i]][0]):
        assert ext_after[files[i]] == (at, DOC_LINES)
        at += DOC_LINES
    for r, (b, a) in enumerate(zip(before, after)):
        want = K.carry(b, localize(layout, keep, r))
        carried = a["ids"] < want["n_rows"]             # the rows appended since sit behind the carried ones on every shard
        assert want["n_rows"] > 0 and np.array_equal(a["ids"][carried], want["ids"])
        assert np.array_equal(a["codes"][carried], want["codes"])
        in_front = np.concatenate([[0], np.cumsum(carried)])
        assert np.array_equal(in_front[a["offsets"].astype(np.int64)], want["offsets"].astype(np.int64))
    # every list probed, lists of <= 512 rows, rerank 512: the index's answer is the exact one
    exact = search(1000000000)
    assert got == exact and got.count("::") == 5
    assert search(4000) == exact                        # (a fresh process loads the saved index)
