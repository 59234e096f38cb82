"""GPU parity at the kernels' structural edges: every corpus of tests/shape_corpora.py (words on the
register-strip, tile and chunk boundaries, exactly packed tiles, no word / one word / no pair / one
merge, the word-count kernel's slot, chunk and tile offsets) on every merge path and load shape,
against the reference's fixtures under tests/golden/shapes/ -- every .model byte, .vocab byte,
merge line and the merge count, and every call's documented return value."""
import os

import numpy as np
import pytest

import encode_ref
import shape_corpora as sc
from test_gpu_parity import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shape_corpus(tmp_path_factory):
    """name -> (fixture, corpus path): built once per module, md5-checked against the fixture."""
    import corpora
    root, made = tmp_path_factory.mktemp("shapes"), {}

    def get(name):
        if name not in made:
            case, path = sc.load_fixture(name), str(root / f"{name}.txt")
            sc.build(name, path)
            assert corpora.md5_file(path) == case["corpus"]["md5"], f"generator drift for {name}"
            made[name] = (case, path)
        return made[name]
    return get


def _trainer(case, layout="types", **opts):
    from shredword.trainer import BPETrainer
    cfg = case["config"]
    t = BPETrainer(vocab_size=cfg["vocab_size"], unk_id=cfg["unk_id"], character_coverage=cfg["character_coverage"],
                   min_pair_freq=cfg["min_pair_freq"])
    t.set_option("log", 0)
    t.set_option("layout", layout)
    for k, v in opts.items():
        t.set_option(k, v)
    return t


def _dry(case):
    """Training ended on an empty heap (not on the vocab target): merge_batch finds nothing more."""
    return case["merges"] < case["config"]["vocab_size"] - 256


def _finish(t, case, tmp_path, tag="g"):
    """train() -> merge_batch on the dry heap -> save; the four things _check compares."""
    from shredword.cbase import lib
    trace = str(tmp_path / f"{tag}.trace")
    t.set_option("trace", trace)
    merges = t.train()
    if _dry(case):
        assert lib.bpe_merge_batch(t.trainer, 5) == 0
    model, vocab = str(tmp_path / f"{tag}.model"), str(tmp_path / f"{tag}.vocab")
    t.save(model, vocab)
    return merges, open(model, "rb").read(), open(vocab, "rb").read(), open(trace).read()


def _train(case, corpus, tmp_path, layout="types", **opts):
    t = _trainer(case, layout, **opts)
    try:
        t.load_corpus(corpus)
        got = _finish(t, case, tmp_path)
        return got, t.stats()
    finally:
        t.destroy()


# path: (layout, options, environment)
PATHS = {
    "hybrid": ("types", {}, {}),
    "hybrid_verify": ("types", {"verify_argmax": 1}, {}),
    "index_depth1": ("types", {"hybrid": 0, "spec_depth": 1}, {}),
    "index_depth3": ("types", {"hybrid": 0, "spec_depth": 3}, {}),
    "index_finalize1024": ("types", {"hybrid": 0, "finalize": 1024}, {}),
    "resident": ("types", {"index": 0}, {}),
    "resident_hbm": ("types", {"index": 0}, {"SHREDWORD_RESIDENT_HBM": "1"}),
    "resident_depth3": ("types", {"index": 0}, {"SHREDWORD_SPEC_DEPTH": "3"}),
    "launch": ("types", {"resident": 0, "index": 0}, {}),
    "launch_no_speculation": ("types", {"resident": 0, "index": 0, "speculate": 0}, {}),
    "stream": ("stream", {}, {}),
}
# k_resident must really run here: every tile at most kWaveTok tokens.  (tile_edge holds words of 1024
# tokens and more, which plan_resident refuses for the whole table; tile_edge_short is its part of
# words up to 1023 tokens.)
RESIDENT_SHAPES = ["strip_edge", "tile_edge_short"] + sc.TILE_FILL


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", sc.TRAINER_SHAPES)
def test_shape_matches_reference(name, path, shape_corpus, tmp_path, monkeypatch):
    case, corpus = shape_corpus(name)
    layout, opts, env = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, st = _train(case, corpus, tmp_path, layout, **opts)
    _check(case, got)
    n = case["merges"]
    if path == "hybrid_verify":
        assert st["verify_failures"] == 0 and st["verify_checks"] == n
    if path.startswith("index_") and n > 0:
        assert st["index_merges"] >= n and st["index_on"] == 1 and st["resident_launches"] == 0
    if path == "index_depth3" and n > 200:
        assert st["index_undos"] > 0
    if path.startswith("launch"):
        assert st["resident_launches"] == 0
    if path == "launch_no_speculation":
        assert st["index_undos"] == 0
    if name in RESIDENT_SHAPES and (path.startswith("resident") or path.startswith("hybrid")):
        assert st["resident_launches"] > 0, st


@pytest.mark.parametrize("name", sc.TRAINER_SHAPES)
def test_shape_reset_and_retrain(name, shape_corpus, tmp_path):
    """shred_reset restores the loaded corpus: the second training on the same trainer writes the
    same bytes, merge numbering included."""
    case, corpus = shape_corpus(name)
    t = _trainer(case)
    try:
        t.load_corpus(corpus)
        first = _finish(t, case, tmp_path, "a")
        t.reset()
        second = _finish(t, case, tmp_path, "b")
    finally:
        t.destroy()
    _check(case, first)
    _check(case, second)


@pytest.mark.parametrize("layout", ["types", "stream"])
@pytest.mark.parametrize("name", ["tile_edge", "chunk_edge"])
def test_shape_rollback_restores_long_words(name, layout, shape_corpus):
    """The undo of a merge (k_unmerge) over words longer than a tile and longer than a chunk: the
    fixture's first merges, an a == a run and a pair across the seam, probed and rolled back on the
    freshly loaded corpus leave the device token stream as it was."""
    from shredword.cbase import lib
    case, corpus = shape_corpus(name)
    ops = encode_ref.model_merges(case["model_bytes"])
    t = _trainer(case, layout)
    try:
        t.load_corpus(corpus)
        lib.bpe_init(t.trainer)
        before = t.tokens()
        assert before.size > 50_000
        pairs = [tuple(int(x) for x in ops[0, :2]), (97, 97), (97, 98), (98, 97)]
        for pair in pairs:
            assert lib.shred_probe_rollback(t.trainer, *pair) == 0
            after = t.tokens()
            assert after.shape == before.shape and (after == before).all(), pair
    finally:
        t.destroy()


# ---- the on-device word count ----------------------------------------------------------------------
def _load_and_train(case, corpus, tmp_path, gpu_load, tag):
    t = _trainer(case, gpu_load=gpu_load)
    try:
        t.load_corpus(corpus)
        got = _finish(t, case, tmp_path, tag)
        return got, t.stats()
    finally:
        t.destroy()


def _table(st):
    return st["num_words"], st["num_symbols"], st["num_occurrences"]


@pytest.fixture(scope="module")
def load_edge_host(shape_corpus, tmp_path_factory):
    """The host count of load_edge, once: the table every device count must reproduce."""
    case, corpus = shape_corpus("load_edge")
    got, st = _load_and_train(case, corpus, tmp_path_factory.mktemp("le_host"), 0, "h")
    assert st["load_on_gpu"] == 0
    _check(case, got)
    words = sc.words_of(open(corpus, "rb").read())
    assert _table(st) == (len(set(words)), sum(len(w) for w in set(words)), len(words))
    return _table(st)


@pytest.mark.parametrize("wide", ["0", "1", "2"], ids=["narrow", "wide", "xwide"])
def test_load_edge_device_count(wide, shape_corpus, load_edge_host, tmp_path, monkeypatch):
    """k_word_count in its three workgroup shapes over words that start and end on both sides of
    every 64-byte chunk and 16384 / 32768 / 49152-byte tile boundary, share their first 16 bytes and
    cover whole chunks: the host's table, the reference's bytes."""
    monkeypatch.setenv("SHREDWORD_GPU_LOAD_MIN", "1")
    monkeypatch.setenv("SHREDWORD_LOAD_WIDE", wide)
    case, corpus = shape_corpus("load_edge")
    got, st = _load_and_train(case, corpus, tmp_path, 1, "d")
    assert st["load_on_gpu"] == 1
    assert _table(st) == load_edge_host
    _check(case, got)


@pytest.mark.parametrize("wide", ["0", "1", "2"], ids=["narrow", "wide", "xwide"])
def test_load_edge_host_count_ignores_the_shape(wide, shape_corpus, load_edge_host, tmp_path, monkeypatch):
    """gpu_load = 0 under the same environment stays on the host."""
    monkeypatch.setenv("SHREDWORD_GPU_LOAD_MIN", "1")
    monkeypatch.setenv("SHREDWORD_LOAD_WIDE", wide)
    case, corpus = shape_corpus("load_edge")
    got, st = _load_and_train(case, corpus, tmp_path, 0, "h")
    assert st["load_on_gpu"] == 0 and _table(st) == load_edge_host
    _check(case, got)


@pytest.mark.parametrize("env", [{"SHREDWORD_LOAD_SIM_SHARDS": "2"}, {"SHREDWORD_LOAD_SIM_SHARDS": "5"},
                                 {"SHREDWORD_LOAD_TABLE_SLOTS": "1024"},
                                 {"SHREDWORD_LOAD_READERS": "3", "SHREDWORD_LOAD_CHUNK_MB": "1"}],
                         ids=["shards2", "shards5", "table_grows", "streamed_file"])
def test_load_edge_device_count_variants(env, shape_corpus, load_edge_host, tmp_path, monkeypatch):
    """Byte ranges cut inside words (2 and 5 simulated shards), a device word table of 1024 slots
    that has to grow (872 distinct words > 3/4 of it), and the file streamed by 3 readers."""
    monkeypatch.setenv("SHREDWORD_GPU_LOAD_MIN", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case, corpus = shape_corpus("load_edge")
    size = os.path.getsize(corpus)
    data = open(corpus, "rb").read()
    for k in (2, 5):   # every cut of the 2 and 5 ranges falls inside a word or next to one
        cuts = [size * i // k for i in range(1, k)]
        assert any(data[c] not in sc.DELIMS and data[c - 1] not in sc.DELIMS for c in cuts)
    got, st = _load_and_train(case, corpus, tmp_path, 1, "v")
    assert st["load_on_gpu"] == 1
    assert _table(st) == load_edge_host
    if "SHREDWORD_LOAD_TABLE_SLOTS" in env:
        assert st["num_words"] > 768
    _check(case, got)


@pytest.mark.parametrize("wide", ["0", "2"], ids=["narrow", "xwide"])
@pytest.mark.parametrize("name", sc.DEGENERATE + ["tile_fill_0", "strip_edge"])
def test_degenerate_device_count(name, wide, shape_corpus, tmp_path, monkeypatch):
    """An empty file, delimiters only, one one-byte word ... through the device word count: the host
    count's table and the reference's bytes.  (A file of 0 bytes has nothing to count: it stays on
    the host by design, load_on_gpu = 0.)"""
    monkeypatch.setenv("SHREDWORD_GPU_LOAD_MIN", "1")
    monkeypatch.setenv("SHREDWORD_LOAD_WIDE", wide)
    case, corpus = shape_corpus(name)
    host, hst = _load_and_train(case, corpus, tmp_path, 0, "h")
    dev, dst = _load_and_train(case, corpus, tmp_path, 1, "d")
    assert hst["load_on_gpu"] == 0 and dst["load_on_gpu"] == (1 if case["corpus"]["size"] > 0 else 0)
    assert _table(hst) == _table(dst)
    words = sc.words_of(open(corpus, "rb").read())
    assert _table(dst) == (len(set(words)), sum(len(w) for w in set(words)), len(words))
    _check(case, host)
    _check(case, dev)


# ---- tiebreak=device and the encoder on the same corpora ---------------------------------------------
@pytest.mark.parametrize("name", ["strip_edge", "tile_fill_0", "one_merge", "one_run", "empty", "single_chars"])
def test_shape_tiebreak_device_matches_its_cpu_rule(name, shape_corpus, tmp_path):
    """test_gpu_tiebreak.py's checker on the shape corpora: the device's own selection against the
    CPU restatement of its rule (bpe_oracle --tiebreak-device 0), not against the fixtures."""
    import test_gpu_tiebreak as tb
    case, corpus = shape_corpus(name)
    n, model, vocab, trace, st = tb._train(case, corpus, tmp_path)
    om, ov, ot = tb._oracle_rule(case, corpus, tmp_path)
    assert trace == ot
    assert model == om
    assert vocab == ov
    assert st["sel_merges"] + st["sel_host_merges"] == n and (st["sel_merges"] == 0 or st["sel_launches"] >= 1)
    assert st["heap_size"] == 0  # the host heap took no part


@pytest.mark.parametrize("name", ["strip_edge", "load_edge"] + sc.DEGENERATE)
def test_shape_encoder_reproduces_the_vocab(name, shape_corpus, tmp_path):
    """BPEEncoder over the fixture's files (an empty .model included): the oracle encoder's ids, and
    id counts equal to the .vocab column."""
    from shredword.encoder import BPEEncoder
    case, corpus = shape_corpus(name)
    model, vocab = tmp_path / "f.model", tmp_path / "f.vocab"
    model.write_bytes(case["model_bytes"])
    vocab.write_bytes(case["vocab_bytes"])
    text = open(corpus, "rb").read()
    assert max((len(w) for w in sc.words_of(text)), default=0) <= 1024
    merges = encode_ref.model_merges(case["model_bytes"])
    toks = encode_ref.token_bytes(merges)
    freqs = encode_ref.vocab_freqs(case["vocab_bytes"], toks)
    unk = case["config"]["unk_id"]
    enc = BPEEncoder(str(model), str(vocab), unk_id=unk, device=0)
    try:
        ids = np.asarray(enc.encode(text))
    finally:
        enc.destroy()
    want = encode_ref.oracle_encode(merges, encode_ref.derived_byte_map(merges, freqs, unk), text)
    assert ids.shape == want.shape and (ids == want).all()
    assert (encode_ref.id_counts(ids, len(toks)) == freqs).all()
