"""GPU: a workspace search over a path subset goes through the IVF index when the subset holds at least SEMTOOLS_INDEX_MIN_ROWS rows
(Store::search_line_embeddings -> smt_sharded_ivfpq_search_ranges), on one GPU and on three logical shards.  With every list probed,
lists of <= 512 rows and rerank 512 the index's answer IS the exact one."""
import json
import os

import numpy as np
import pytest

from tests import ivf_ref as R
from tests import synth
from tests.test_gpu_host import V, model, model_dir  # noqa: F401  (the fixtures of the host tests: one GPU / three shards)

pytestmark = pytest.mark.gpu


def test_a_large_path_subset_is_answered_by_the_index(model, tmp_path, monkeypatch):  # noqa: F811
    from semtools_amd import host

    monkeypatch.setenv("HOME", str(tmp_path))
    monkeypatch.delenv("SEMTOOLS_WORKSPACE", raising=False)
    files = []
    for i in range(6):
        f = tmp_path / f"big{i}.txt"
        f.write_text("\n".join(synth.pseudo_prose(1000, vocab_size=V - 1, seed=100 + i)) + "\n")
        files.append(str(f))
    query = synth.pseudo_prose(1, vocab_size=V - 1, seed=103)[0]
    host.workspace_use(None, "sub")
    root = tmp_path / ".semtools" / "workspaces" / "sub"
    cfg = json.loads((root / "config.json").read_text())
    cfg["oversample_factor"] = 64                       # rerank = min(512, 2 * top_k * oversample_factor) = 512 at top_k 5
    (root / "config.json").write_text(json.dumps(cfg))
    n = model.n_shards
    parts = [root / ("line_index.ivf" if n == 1 else f"line_index.ivf.r{r}of{n}") for r in range(n)]

    def search(paths, min_rows):
        monkeypatch.setenv("SEMTOOLS_INDEX_MIN_ROWS", str(min_rows))
        monkeypatch.setenv("SEMTOOLS_INDEX_NPROBE", "512")
        return host.search_with_workspace(model, query, paths, workspace_name="sub", n_lines=0, top_k=5)

    assert search(files, 1000000000).count("::") == 5  # stores the six files; policy off: exact scan, no index
    assert not any(p.exists() for p in parts)
    got = search(files[:2], 1500)                       # the first search with the policy on is a SUBSET search: 2000 rows >= 1500
    assert all(p.exists() for p in parts), "a subset of 2000 rows must build and use the index"
    for p in parts:
        assert max_list(p) <= 512
    exact = search(files[:2], 1000000000)
    assert got == exact and got.count("::") == 5        # (the formatted result text: five hits)
    assert "big2.txt" not in got and "big3.txt" not in got and "big4.txt" not in got and "big5.txt" not in got
    # one file: 1000 rows < 1500 -> the exact scan, the same answer either way
    stamp = [p.stat().st_mtime_ns for p in parts]
    assert search(files[:1], 1500) == search(files[:1], 1000000000)
    assert [p.stat().st_mtime_ns for p in parts] == stamp
    # a replaced file leaves dead rows behind; they lie outside every range of the subset
    (tmp_path / "big0.txt").write_text("\n".join(synth.pseudo_prose(900, vocab_size=V - 1, seed=100)) + "\n")
    os.utime(tmp_path / "big0.txt", (1_950_000_000, 1_950_000_000))
    got2 = search(files[:2], 1500)
    assert got2 == search(files[:2], 1000000000) and got2.count("::") == 5


def max_list(path):
    return int(np.diff(R.read_index(path)["offsets"].astype(np.int64)).max())
