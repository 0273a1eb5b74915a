"""GPU: ignore_case through the host layer with the device tokenizer route off, on with device lower-casing off, and on with it on
(smt_host_model_set_device_lower): the same rows, search text, workspace files and cached token ids for all three, and the rows of the
lines lowered up front by smt_host_to_lowercase.  Lines are lowered on the device only in the third configuration, and never for a
lazy table or a group of several ranks.  The model directories are those of the two host device-tokenizer test files: a WordPiece and
a Unigram tokenizer.json, at device tokenizer settings 1 and 2."""
import numpy as np
import pytest

from tests import lower_ref as R
from tests import test_gpu_host_device_tokenizer_utf8 as WP
from tests import test_gpu_host_device_unigram_utf8 as UG

pytestmark = pytest.mark.gpu

FAMILIES = {"wordpiece": (WP, "[PAD]", [p for p in WP.VOCAB if p.isascii() and p.isalpha()]),
            "unigram": (UG, "<pad>", [p for p, _ in UG.VOCAB if p.isascii() and p.isalpha()])}
ODD = ["\u00c9COLE \u00dcBER \u00c0 LA CAF\u00c9",                                  # Latin-1 capitals
       "\u039f\u0394\u03a5\u03a3\u03a3\u0395\u03a5\u03a3 \u039a\u0391\u0399 \u039b\u039f\u0393\u039f\u03a3",   # Greek, two final sigmas
       "\u0130stanbul \u0130STANBUL", "300 \u212a THE \u212b", "\u4e2d\u6587 THE FOX", None, ""]      # None: the added token


@pytest.fixture(scope="module", params=sorted(FAMILIES))
def family(request, tmp_path_factory):
    mod, added, words = FAMILIES[request.param]
    assert len(words) >= 5
    base = tmp_path_factory.mktemp("lower_" + request.param)
    return mod, added, words, (mod._dir(base / "v1", 5), mod._dir(base / "v2", 79))


def _lines(words, added, n, seed):
    """upper-case ASCII in most lines; every fifth line drawn from Latin-1 capitals, Greek with final sigmas, Istanbul with its dotted
    capital, a Kelvin sign, CJK, an added token, empty"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 5 == 4:
            odd = ODD[(i // 5) % len(ODD)]
            out.append("The " + added + " FOX" if odd is None else odd)
            continue
        ws = [words[int(k)] for k in rng.integers(len(words), size=int(rng.integers(1, 12)))]
        out.append(" ".join(w.upper() if rng.random() < 0.4 else w.capitalize() if rng.random() < 0.5 else w for w in ws))
    return out


CONFIGS = ("off", "host_lower", "device_lower")


def _model(ctx, d, config, setting):
    from semtools_amd import host

    if config == "off":
        return host.StaticModel(ctx, model_dir=d, device_tokenizer=0)
    return host.StaticModel(ctx, model_dir=d, device_tokenizer=setting, device_lower=config == "device_lower")


@pytest.mark.parametrize("setting", [1, 2])
@pytest.mark.parametrize("max_length", [2048, 5])
def test_rows_are_those_of_lines_lowered_up_front(gpu_ctx, family, monkeypatch, max_length, setting):
    """fails without the feature: host.StaticModel takes no device_lower and the library has no smt_host_encode_lowered"""
    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    mod, added, words, dirs = family
    lines = _lines(words, added, 3000, seed=61)
    assert sum(any(c.isupper() for c in s) for s in lines) > 2000
    models = {c: _model(gpu_ctx, dirs[0], c, setting) for c in CONFIGS}
    try:
        up_front = models["off"].encode_with_args([R.host_lower(s.encode()).decode() for s in lines], max_length)
        if mod is UG:       # (the WordPiece file's BertNormalizer lowers by itself; this Unigram file's normalizer does not)
            assert not np.array_equal(up_front, models["off"].encode_with_args(lines, max_length))   # lowering matters to these lines
        rows = {c: m.encode_with_args(lines, max_length, lower=True) for c, m in models.items()}
        for c in CONFIGS:
            assert np.array_equal(rows[c], up_front), c
        lowered = {c: m.device_lowered_lines() for c, m in models.items()}
        print("lines lowered on the device of 3000:", lowered, "tokenized there:", {c: m.device_tokenized_lines() for c, m in models.items()})
        assert lowered["off"] == 0 and lowered["host_lower"] == 0 and lowered["device_lower"] > 2000
        assert models["host_lower"].device_tokenized_lines() == models["device_lower"].device_tokenized_lines() > 0
    finally:
        for m in models.values():
            m.close()


@pytest.mark.parametrize("setting", [1, 2])
@pytest.mark.parametrize("max_length", [2048, 5])
def test_an_ill_formed_byte_behind_the_truncation_still_sends_the_line_to_the_host(gpu_ctx, family, monkeypatch, max_length, setting):
    """pass 1 looks at the first max_length x median bytes of a line only: a line whose ill-formed byte lies behind that cut is copied
    un-lowered by the device lower-casing, and must reach the host through the lower-casing's own flag -- its upper-case head is
    lowered there like everywhere else"""
    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    mod, added, words, dirs = family
    cut = max_length * mod.MEDIAN
    head = (" ".join(w.upper() for w in words) + " ").encode()
    long_head = head * (cut // len(head) + 2)                      # upper-case ASCII well past the cut
    assert len(long_head) > cut + len(head)
    bad = [long_head + b"\xff", long_head + b"tail \xc3", long_head + b"\xa9 Tail", long_head[:cut] + b"\xff",
           long_head[:cut + 1] + b"\xed\xa0\x80 X", long_head + b"\xc1\x81"]
    clean = [s.encode() for s in _lines(words, added, 60, seed=67)]
    lines = []
    for i, ln in enumerate(clean):
        lines.append(ln)
        if i % 10 == 5:
            lines.append(bad[(i // 10) % len(bad)])
    assert sum(not R.strictly_valid(ln) for ln in lines) == 6
    models = {c: _model(gpu_ctx, dirs[0], c, setting) for c in CONFIGS}
    try:
        up_front = models["off"].encode_with_args([R.host_lower(ln) for ln in lines], max_length)
        if mod is UG:       # (this Unigram file's normalizer does not lower: the head's rows depend on who lowered it)
            assert not np.array_equal(up_front, models["off"].encode_with_args(lines, max_length))
        for c, m in models.items():
            assert np.array_equal(m.encode_with_args(lines, max_length, lower=True), up_front), c
        assert models["device_lower"].device_lowered_lines() == len(lines) - 6
    finally:
        for m in models.values():
            m.close()


@pytest.mark.parametrize("setting", [1, 2])
def test_search_session_and_workspace_do_not_depend_on_where_lines_are_lowered(gpu_ctx, family, tmp_path, monkeypatch, capfd, setting):
    from semtools_amd import host

    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    monkeypatch.delenv("SEMTOOLS_WORKSPACE", raising=False)
    mod, added, words, dirs = family
    lines = [s.encode() for s in _lines(words, added, 3000, seed=65)]
    lines[7], lines[1500], lines[2999] = b"BAD \xff LINE The", b"CUT AT THE END \xc3", b"\xa9 LONE Fox"     # ill-formed: lowered by the host
    a, b = tmp_path / ("a%d.txt" % setting), tmp_path / ("b%d.txt" % setting)
    a.write_bytes(b"\n".join(lines[:1700]) + b"\n")
    b.write_bytes(b"\n".join(lines[1700:]) + b"\n")
    files = [str(a), str(b)]
    query = " ".join(words[:3]).upper()
    seen = {}
    for c in CONFIGS:
        home = tmp_path / ("home_%s_%d" % (c, setting))
        home.mkdir()
        monkeypatch.setenv("HOME", str(home))
        m, m2 = _model(gpu_ctx, dirs[0], c, setting), _model(gpu_ctx, dirs[1], c, setting)
        try:
            out = [host.search_files(m, query, files, n_lines=0, top_k=6, ignore_case=True),
                   host.search_content(m, query, b"\n".join(lines[:900]).decode(errors="replace"), n_lines=1, top_k=5, ignore_case=True)]
            s = host.Session(m, files, ignore_case=True)
            try:
                out.append((s.lines, s.search([query, words[3]], n_lines=0, top_k=5)))
            finally:
                s.close()
            host.workspace_use(None, "ws")
            out.append(host.search_with_workspace(m, query, files, workspace_name="ws", n_lines=0, top_k=5, ignore_case=True))     # ingest
            root = home / ".semtools" / "workspaces" / "ws"
            out.append((root / "line_tokens.log").read_bytes())          # the cached token ids
            out.append((root / "line_embeddings.f32").read_bytes())      # the rows
            out.append(host.workspace_reembed(m2, "ws"))
            out.append((root / "line_embeddings.f32").read_bytes())
            seen[c] = out, m.device_lowered_lines()
        finally:
            m.close()
            m2.close()
    capfd.readouterr()
    for c in ("host_lower", "device_lower"):
        for i, (x, y) in enumerate(zip(seen["off"][0], seen[c][0])):
            assert x == y, (c, i)
    assert len(seen["off"][0][4]) > 0 and len(seen["off"][0][5]) >= 3000 * 256 * 4
    # search_files, search_content (900 lines), the session and the workspace ingest each lower their lines
    assert seen["off"][1] == 0 and seen["host_lower"][1] == 0 and seen["device_lower"][1] > 2000


def test_a_lazy_table_and_a_group_of_three_shards_lower_on_the_host(gpu_ctx, family, monkeypatch):
    import semtools_amd as smt

    mod, added, words, dirs = family
    lines = _lines(words, added, 1500, seed=66)
    monkeypatch.delenv("SEMTOOLS_EAGER_MODEL", raising=False)
    off, lazy = _model(gpu_ctx, dirs[0], "off", 2), _model(gpu_ctx, dirs[0], "device_lower", 2)
    try:
        assert not lazy.table_info()[3]
        want = off.encode_with_args([R.host_lower(s.encode()).decode() for s in lines], 2048)
        assert np.array_equal(lazy.encode_with_args(lines, 2048, lower=True), want)
        assert lazy.device_lowered_lines() == 0 and lazy.device_tokenized_lines() == 0
    finally:
        off.close()
        lazy.close()
    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    group = smt.Group.logical(0, 3)
    three = _model(group, dirs[0], "device_lower", 2)
    try:
        assert np.array_equal(three.encode_with_args(lines, 2048, lower=True), want)
        assert three.device_lowered_lines() == 0
    finally:
        three.close()
        group.close()


def test_a_mostly_non_ascii_call_at_setting_1_gives_up_and_still_gives_the_same_rows(gpu_ctx, family, monkeypatch):
    """three batches of 16384: the ASCII form flags most lines of the first one, the route gives up, and the other two are lowered on
    the host inside their batch"""
    monkeypatch.setenv("SEMTOOLS_EAGER_MODEL", "1")
    mod, added, words, dirs = family
    base = ["ПРИВЕТ МИР " + words[i % len(words)].upper() for i in range(64)] + \
           ["İSTANBUL ΣΟΦΟΣ", words[0].upper() + " " + words[1].capitalize(), "300 K"]
    lines = [base[i % len(base)] for i in range(40000)]
    off, dev = _model(gpu_ctx, dirs[0], "off", 1), _model(gpu_ctx, dirs[0], "device_lower", 1)
    try:
        want = off.encode_with_args([R.host_lower(s.encode()).decode() for s in base], 2048)
        got = dev.encode_with_args(lines, 2048, lower=True)
        assert np.array_equal(got, want[np.arange(40000) % len(base)])
        assert dev.device_lowered_lines() == 16384            # the first batch only
    finally:
        off.close()
        dev.close()
