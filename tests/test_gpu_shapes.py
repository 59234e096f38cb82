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
    # chained launches: the selected merge and up to 7 predicted successors in one k_merge, the
    # rejected tail undone by one k_unmerge (tests/test_chain_cpu.py: which shapes form chains)
    "launch_chain2": ("types", {"resident": 0, "index": 0, "chain": 2}, {}),
    "launch_chain8": ("types", {"resident": 0, "index": 0, "chain": 8}, {}),
    "stream_chain2": ("stream", {"chain": 2}, {}),
    "stream_chain8": ("stream", {"chain": 8}, {}),
    "launch_chain8_verify": ("types", {"resident": 0, "index": 0, "chain": 8, "verify_argmax": 1}, {}),
    # k_merge's grid cap: one completion counter up to 32 workgroups, tickets sharded by
    # blockIdx % 8 above (33: groups of 5, 4, 4, ...)
    "launch_groups1": ("types", {"resident": 0, "index": 0}, {"SHREDWORD_MERGE_GROUPS": "1"}),
    "launch_groups8": ("types", {"resident": 0, "index": 0}, {"SHREDWORD_MERGE_GROUPS": "8"}),
    "launch_groups32": ("types", {"resident": 0, "index": 0}, {"SHREDWORD_MERGE_GROUPS": "32"}),
    "launch_groups33": ("types", {"resident": 0, "index": 0}, {"SHREDWORD_MERGE_GROUPS": "33"}),
    "launch_groups40": ("types", {"resident": 0, "index": 0}, {"SHREDWORD_MERGE_GROUPS": "40"}),
    "launch_chain8_groups33": ("types", {"resident": 0, "index": 0, "chain": 8}, {"SHREDWORD_MERGE_GROUPS": "33"}),
}
CHAIN_PATHS = [p for p in PATHS if "chain" in p]
LOGGED_PATHS = [p for p in PATHS if "chain" in p or "groups" in p]
# k_resident must really run here: every tile at most kWaveTok tokens.  (tile_edge holds words of 1024
# tokens and more, which plan_resident refuses for the whole table; tile_edge_short is its part of
# words up to 1023 tokens.)
RESIDENT_SHAPES = ["strip_edge", "tile_edge_short"] + sc.TILE_FILL


# The shapes whose training forms chains (tests/test_chain_cpu.py proves it from the host logic alone):
# the degenerate ones end before a chain can (at most 7 merges; `remaining` cuts the chain to 1).
CHAIN_SHAPES = [n for n in sc.TRAINER_SHAPES if n not in sc.DEGENERATE]
_MERGE_LOGS = {}


def parse_merge_log(text):
    """SHREDWORD_MERGE_LOG -> (launches, undos).  `C seq X0 n_iter grid n occurrences records spilled
    wide` is a collected k_merge launch of n merges over n_iter candidate tiles (spilled: records that
    went through the global delta tables, wide: k_collect ran); `R seq X ntiles nundo` a k_unmerge of
    nundo merges from X over ntiles tiles."""
    launches, undos = [], []
    for line in text.splitlines():
        f = line.split()
        if f[0] == "C":
            launches.append(dict(zip(("seq", "X0", "n_iter", "grid", "n", "occ", "records", "spilled", "wide"),
                                     (int(v) for v in f[1:10]))))
        elif f[0] == "R":
            undos.append(dict(zip(("seq", "X", "ntiles", "nundo"), (int(v) for v in f[1:5]))))
    return launches, undos


def check_grids(launches, cap):
    """One filter window of 32 candidate tiles per workgroup and pass, up to the cap."""
    for c in launches:
        assert c["grid"] == min((c["n_iter"] + 31) // 32, cap), c


@pytest.fixture(scope="module")
def logged_run(shape_corpus, tmp_path_factory):
    """(name, path) -> (outputs, stats, launches, undos) of one training with the merge log on; run
    once per module, so the per-set assertions below share the per-case trainings."""
    def get(name, path):
        if (name, path) not in _MERGE_LOGS:
            case, corpus = shape_corpus(name)
            layout, opts, env = PATHS[path]
            tmp = tmp_path_factory.mktemp(f"{name}_{path}")
            env = dict(env, SHREDWORD_MERGE_LOG=str(tmp / "merge.log"))
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                got, st = _train(case, corpus, tmp, layout, **opts)
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            _MERGE_LOGS[(name, path)] = (got, st) + parse_merge_log(open(tmp / "merge.log").read())
        return _MERGE_LOGS[(name, path)]
    return get


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", sc.TRAINER_SHAPES)
def test_shape_matches_reference(name, path, shape_corpus, tmp_path, monkeypatch, logged_run):
    case, corpus = shape_corpus(name)
    layout, opts, env = PATHS[path]
    if path in LOGGED_PATHS:
        got, st, launches, undos = logged_run(name, path)
    else:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got, st = _train(case, corpus, tmp_path, layout, **opts)
    _check(case, got)
    n = case["merges"]
    if path in LOGGED_PATHS:
        cap = int(env.get("SHREDWORD_MERGE_GROUPS", 256))
        check_grids(launches, cap)
        assert sum(c["n"] for c in launches) - sum(u["nundo"] for u in undos) == n or st["num_tiles"] == 0
        assert st["index_merges"] == 0
        if path == "launch_groups1":
            assert all(c["grid"] == 1 for c in launches)
    if path in CHAIN_PATHS and name in CHAIN_SHAPES:
        k = opts["chain"]
        assert st["resident_launches"] == 0 and st["index_merges"] == 0
        if path != "launch_chain8_verify":  # (the argmax check undoes the tail before every select)
            assert st["spec_hits"] > 0 and st["spec_misses"] > 0
        assert max(c["n"] for c in launches) == k and any(c["n"] == k for c in launches)
        if k == 8:
            assert any(u["nundo"] >= 2 for u in undos)
        else:
            assert undos and all(u["nundo"] == 1 for u in undos)
    if path == "launch_chain8_verify":
        assert st["verify_failures"] == 0 and st["verify_checks"] == n
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


@pytest.mark.parametrize("path", CHAIN_PATHS)
def test_chain_paths_cover_both_candidate_modes(path, logged_run):
    """Over the shapes that chain, per path: launches that scanned the union of the chain's candidate
    tile lists (n_iter < tiles) and launches that scanned every tile, both with n > 1; and the
    records' way out is reported (spilled / wide: see parse_merge_log)."""
    listed = full = 0
    for name in CHAIN_SHAPES:
        _, st, launches, _ = logged_run(name, path)
        chains = [c for c in launches if c["n"] > 1]
        assert chains
        listed += sum(c["n_iter"] < st["num_tiles"] for c in chains)
        full += sum(c["n_iter"] == st["num_tiles"] for c in chains)
        assert all(c["n_iter"] <= st["num_tiles"] for c in launches)
    assert listed > 0 and full > 0


def test_grid_caps_bound_every_launch(logged_run):
    """SHREDWORD_MERGE_GROUPS on the shapes: at most 254 tiles here, so at most 8 workgroups (the
    single completion counter); under the cap 1 every launch is one workgroup, under 8 and above
    some launch has 8.  (Grids of 33 and more: test_gpu_parity.py::test_merge_grid_sizes_match_reference, on a
    table of 9,804 tiles.)"""
    for path in [p for p in LOGGED_PATHS if "groups" in p]:
        cap = int(PATHS[path][2]["SHREDWORD_MERGE_GROUPS"])
        grids = set()
        for name in ("tile_edge", "tile_fill32_p1"):
            grids |= {c["grid"] for c in logged_run(name, path)[2]}
        assert max(grids) == min(cap, 3), (path, grids)   # types: 90 and 33 tiles -> 3 and 2 windows
    grids = {c["grid"] for c in logged_run("tile_edge", "stream_chain8")[2]}
    assert max(grids) == 8, grids                         # stream: 254 tiles -> 8 windows


@pytest.mark.parametrize("layout", ["types", "stream"])
@pytest.mark.parametrize("name", ["tile_edge", "chunk_edge"])
def test_shape_chained_undo_restores_long_words(name, layout, shape_corpus, tmp_path, monkeypatch):
    """k_unmerge with several merges to undo over words longer than a tile and longer than a chunk:
    56 merges in bpe_merge_batch steps of 8 under chain = 8, the device token stream after every step
    equal to that of a trainer without speculation stepped alongside.  A rejected guess undoes the
    rest of its chain at once, in place, over the multi-chunk tiles; the merge log shows undos of
    >= 2 merges and launches of 8.  (Steps of one merge would not do: `remaining` = 1 cuts every
    chain to 1, tests/test_chain_cpu.py::test_stepped_training_chains_only_in_batches.)"""
    from shredword.cbase import lib
    case, corpus = shape_corpus(name)
    log = tmp_path / "merge.log"
    ref = _trainer(case, layout, resident=0, index=0, chain=1, speculate=0)
    t = _trainer(case, layout, resident=0, index=0, chain=8)
    try:
        ref.load_corpus(corpus)
        monkeypatch.setenv("SHREDWORD_MERGE_LOG", str(log))   # read when the device is created, at the load
        t.load_corpus(corpus)
        monkeypatch.delenv("SHREDWORD_MERGE_LOG")
        for x in (ref, t):
            lib.bpe_init(x.trainer)
        assert ref.tokens().size > 50_000
        for step in range(7):
            assert lib.bpe_merge_batch(ref.trainer, 8) == 8
            assert lib.bpe_merge_batch(t.trainer, 8) == 8
            want, got = ref.tokens(), t.tokens()
            assert got.shape == want.shape and (got == want).all(), f"streams differ after {8 * step + 8} merges"
        st = t.stats()
    finally:
        ref.destroy()
        t.destroy()
    assert st["spec_hits"] > 0 and st["spec_misses"] > 0 and st["resident_launches"] == 0 and st["index_merges"] == 0
    launches, undos = parse_merge_log(log.read_text())
    assert any(c["n"] == 8 for c in launches)
    assert any(u["nundo"] >= 2 and u["ntiles"] > 0 for u in undos)


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
