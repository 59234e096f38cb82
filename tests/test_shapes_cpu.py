"""CPU checks of the structural-edge corpora (tests/shape_corpora.py) and their reference fixtures
(tests/golden/shapes/): the oracle restatement and the product's host logic reproduce every fixture,
each corpus really sits on the edge it was built for (a word of every targeted length, a word that
crosses the boundary while training, exact tile packing, the load_edge offsets), and the constants
the recipes were written for are still the sources'."""
import os
import re
import subprocess

import numpy as np
import pytest

import encode_ref
import hostharness
import shape_corpora as sc
from conftest import PKG

CSRC = os.path.join(PKG, "csrc")


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
            assert case["config"] == sc.SHAPES[name]
            made[name] = (case, path)
        return made[name]
    return get


@pytest.fixture(scope="module")
def hh():
    return hostharness.load()


def test_every_shape_has_a_fixture():
    assert sorted(os.listdir(sc.SHAPES_GOLDEN)) == sorted(sc.SHAPES)
    for name, cfg in sc.SHAPES.items():
        assert 300 <= cfg["vocab_size"] <= 800 and cfg["min_pair_freq"] == 2
        assert len(sc.corpus_bytes(name)) < sc.MAX_BYTES
        assert sc.load_fixture(name)["merges"] <= 600


@pytest.mark.parametrize("name", list(sc.SHAPES))
def test_oracle_matches_shape_fixture(name, shape_corpus, oracle_bin, tmp_path):
    case, corpus = shape_corpus(name)
    cfg = case["config"]
    model, vocab, trace = (str(tmp_path / n) for n in ("o.model", "o.vocab", "o.trace"))
    subprocess.run([oracle_bin, corpus, str(cfg["vocab_size"]), str(cfg["unk_id"]), repr(cfg["character_coverage"]),
                    str(cfg["min_pair_freq"]), model, vocab, "--trace", trace], check=True, stderr=subprocess.DEVNULL)
    assert open(model, "rb").read() == case["model_bytes"]
    assert open(vocab, "rb").read() == case["vocab_bytes"]
    assert open(trace).read() == case["trace"]
    assert os.path.getsize(model) == 12 * case["merges"]


@pytest.mark.parametrize("layout", ["types", "stream"])
@pytest.mark.parametrize("name", list(sc.SHAPES))
def test_host_logic_matches_shape_fixture(name, layout, hh, shape_corpus, tmp_path):
    """The product's loader, tile packing, engine and selector over the CPU emulation of the kernels:
    zero tiles, an empty heap and one-word tables on the host side of the C ABI."""
    case, corpus = shape_corpus(name)
    h = hostharness.open_case(hh, corpus, case["config"], layout)
    try:
        trace = str(tmp_path / "t.txt")
        merges = hh.hh_train(h, trace.encode())
        if case["merges"] < case["config"]["vocab_size"] - 256:   # training ended on a dry heap
            assert hh.hh_merge_batch(h, 5) == 0
        model, vocab = str(tmp_path / "h.model"), str(tmp_path / "h.vocab")
        hh.hh_save(h, model.encode(), vocab.encode(), 1)
        got = (merges, open(trace).read(), open(model, "rb").read(), open(vocab, "rb").read())
    finally:
        hh.hh_close(h)
    assert got == (case["merges"], case["trace"], case["model_bytes"], case["vocab_bytes"])


# ---- the corpus hits its edge ----------------------------------------------------------------------
def _replay(case, data):
    """Every distinct word's token count after each merge: the fixture's merges applied left to
    right without overlap (str.replace's rule), one character per token id.  Returns
    {word: [len after 0, 1, ... merges]} and the final weighted token histogram."""
    cfg, merges = case["config"], encode_ref.model_merges(case["model_bytes"])
    kept = encode_ref.derived_byte_map(merges, encode_ref.vocab_freqs(case["vocab_bytes"],
                                                                      encode_ref.token_bytes(merges)), cfg["unk_id"])
    counts = {}
    for w in sc.words_of(data):
        counts[w] = counts.get(w, 0) + 1
    cur = {w: "".join(chr(int(kept[b])) for b in w) for w in counts}
    lens = {w: [len(s)] for w, s in cur.items()}
    for a, b, x in merges:
        pat, new = chr(int(a)) + chr(int(b)), chr(int(x))
        for w, s in cur.items():
            if pat in s:
                cur[w] = s = s.replace(pat, new)
            lens[w].append(len(s))
    hist = np.zeros(256 + len(merges), dtype=np.uint64)
    for w, s in cur.items():
        for ch in s:
            hist[ord(ch)] += counts[w]
    return lens, hist


def _crossings(lens, bound, pick=lambda w: True):
    """(word length, merge index, tokens before, tokens after) of every step from above `bound` to
    at or below it."""
    out = []
    for w, ls in lens.items():
        if pick(w):
            out += [(len(w), i, p, q) for i, (p, q) in enumerate(zip(ls, ls[1:])) if p > bound >= q]
    return sorted(out)


# bound = the largest token count on the near side, from the comparison in the code:
#   word_loop.hip   `if (L <= kStripTok)` (kStripTok: word_loop_dev.h) -> 25
#   tiles.cpp       `fill + need > kTileTokens`, need = len + 1        -> 1023 shares a tile
#   resident_loop   `len > kWaveTok` (a tile's length, header included) -> 1023
#   pair_count.hip  `for (cs = 0; cs < len; cs += kChunk)`, len = tile  -> 4095 is one chunk
EDGES = {"strip_edge": (sc.STRIP_LENGTHS, sc.K_STRIP_TOK),
         "tile_edge": (sc.TILE_LENGTHS, sc.K_TILE_TOKENS - 1),
         "chunk_edge": (sc.CHUNK_LENGTHS, sc.K_CHUNK - 1)}


@pytest.mark.parametrize("name", list(EDGES))
def test_trainer_shape_crosses_its_boundary(name, shape_corpus):
    case, corpus = shape_corpus(name)
    data = open(corpus, "rb").read()
    lengths, bound = EDGES[name]
    have = {}
    for w in set(sc.words_of(data)):
        have.setdefault(len(w), set()).add(w)
    for L in lengths:
        assert L in have, f"no word of {L} tokens"
        assert b"a" * L in have[L] or name == "chunk_edge", f"no run of {L}"
    if name == "chunk_edge":
        assert all(b"a" * L in have[L] for L in (4094, 4095, 4096, 4097, 4098, 8191, 8192))
        assert all((b"ab" * L)[:L] in have[L] for L in lengths if L % 2 == 0)
        assert all((b"b" + b"ab" * L)[:L] in have[L] for L in lengths if L % 2 == 1)
    else:
        assert all((b"ab" * L)[:L] in have[L] for L in lengths)
        assert all(len(have[L]) >= 3 for L in lengths)          # + the seeded random filling
    lens, hist = _replay(case, data)
    # the replay is the reference's training: the token histogram is the .vocab column
    toks = encode_ref.token_bytes(encode_ref.model_merges(case["model_bytes"]))
    assert (hist == encode_ref.vocab_freqs(case["vocab_bytes"], toks)).all()
    assert all(len(ls) == case["merges"] + 1 for ls in lens.values())
    cross = _crossings(lens, bound)
    runs = _crossings(lens, bound, lambda w: w == b"a" * len(w) and len(w) % 2 == 1)
    mixed = _crossings(lens, bound, lambda w: len(set(w)) > 2)
    print(f"{name}: {case['merges']} merges; {len(cross)} crossings of {bound} "
          f"(odd a-runs: {runs}; random fillings: {len(mixed)}); all: {cross}")
    assert cross, "no word crosses the boundary while training"
    assert runs, "no odd-length (a,a) run crosses the boundary"
    assert mixed, "no random filling crosses the boundary"
    if name != "strip_edge":   # the long words start on both sides and the doubled lengths come down across it
        assert any(L > 2 * bound - 6 for L, *_ in cross) and any(L <= bound + 3 for L, *_ in cross)


def test_tile_edge_short_fills_a_tile_exactly(hh, shape_corpus):
    """Its longest word is 1023 tokens: with the header a tile of exactly kWaveTok, the largest
    plan_resident accepts (`len > kWaveTok` refuses the table)."""
    case, corpus = shape_corpus("tile_edge_short")
    words = set(sc.words_of(open(corpus, "rb").read()))
    assert max(len(w) for w in words) == sc.K_TILE_TOKENS - 1
    for L in sc.TILE_SHORT_LENGTHS:
        assert {b"a" * L, (b"ab" * L)[:L]} <= words and sum(len(w) == L for w in words) == 3
    h = hostharness.open_case(hh, corpus, case["config"])
    try:   # each of the 9 long words owns a tile and cuts the shared tile around it in two
        full = -(-hh.hh_live_tokens(h) // sc.K_TILE_TOKENS)
        assert full + 9 <= hh.hh_num_tiles(h) + 9 and 9 < hh.hh_num_tiles(h) <= full + 2 * 9 + 2
    finally:
        hh.hh_close(h)


@pytest.mark.parametrize("name", sc.TILE_FILL)
def test_tile_fill_packs_as_intended(name, hh, shape_corpus):
    """128 words of 7 tokens (+ header) fill a 1024-token tile exactly: the table's last tile is one
    word short / full / holds the one word over (pack_tiles through the host harness)."""
    case, corpus = shape_corpus(name)
    n = sc.TILE_FILL_WORDS[name]
    words = set(sc.words_of(open(corpus, "rb").read()))
    assert len(words) == n and all(len(w) == 7 for w in words)
    per_tile = sc.K_TILE_TOKENS // 8
    assert per_tile * 8 == sc.K_TILE_TOKENS
    h = hostharness.open_case(hh, corpus, case["config"])
    try:
        assert hh.hh_num_words(h) == n
        assert hh.hh_live_tokens(h) == 8 * n
        assert hh.hh_num_tiles(h) == (n + per_tile - 1) // per_tile
    finally:
        hh.hh_close(h)
    tag = name.rsplit("_", 1)[1]
    assert n % per_tile == {"m1": per_tile - 1, "0": 0, "p1": 1}[tag]


def test_degenerate_corpora_are_what_they_say(shape_corpus):
    merges = {n: shape_corpus(n)[0]["merges"] for n in sc.DEGENERATE}
    assert merges == {"empty": 0, "delims_only": 0, "one_byte_word": 0, "single_chars": 0, "one_pair_once": 0,
                      "one_merge": 1, "one_run": merges["one_run"], "ab_literal": 0, "run_literal": 0}
    assert 0 < merges["one_run"] < 300 - 256                      # the heap runs dry before the target
    ops = encode_ref.model_merges(shape_corpus("one_run")[0]["model_bytes"])
    assert ops[0].tolist() == [97, 97, 256]                       # the corpus holds only the a == a pair
    assert all(t == b"a" * len(t) for t in encode_ref.token_bytes(ops)[256:])
    assert encode_ref.model_merges(shape_corpus("one_merge")[0]["model_bytes"]).tolist() == [[97, 98, 256]]
    assert shape_corpus("empty")[0]["corpus"]["size"] == 0


# ---- load_edge ---------------------------------------------------------------------------------
def test_load_edge_geometry(shape_corpus):
    case, corpus = shape_corpus("load_edge")
    d = open(corpus, "rb").read()
    assert len(d) == sc.LOAD_SIZE and len(d) % 49152 == 0
    assert d[-1] not in sc.DELIMS                                   # the last word has no delimiter
    dl = [c in sc.DELIMS for c in d]
    starts = {i for i in range(len(d)) if not dl[i] and (i == 0 or dl[i - 1])}
    ends = {i for i in range(len(d)) if not dl[i] and (i + 1 == len(d) or dl[i + 1])}   # a word's last byte
    seen = {}
    for B, kind in sc.LOAD_ANCHORS.items():
        if kind == "L1":
            assert B - 1 in starts and not dl[B]                    # starts at B - 1 and runs across B
        elif kind == "L2":
            assert B in starts
        elif kind == "L3":
            assert B - 1 in ends and dl[B] and B + 1 in starts
        elif kind == "L4":
            assert B in ends
        else:                                                      # mixed delimiters across B
            run = d[B - 20:B + 20]
            assert all(c in sc.DELIMS for c in run) and set(run) == set(sc.DELIMS)
        for size in (sc.K_CHUNK_BYTES,) + sc.LOAD_TILES:
            if B % size == 0:
                seen.setdefault(size, set()).add(kind)
    # a word cannot start at B - 1 and at B at once: every tile size meets every layout at some multiple
    for size in (sc.K_CHUNK_BYTES,) + sc.LOAD_TILES:
        assert seen[size] >= {"L1", "L2", "L3", "L4"}, (size, seen[size])
    assert all("Z" in seen[s] for s in (64, 16384, 32768))
    for B in (16384, 32768, 49152, 98304):                          # the issue's offsets carry an anchor
        assert B in sc.LOAD_ANCHORS
    for off, n in sc.LOAD_COVERS.items():                            # whole 64-byte chunks without a word start
        assert off in starts and off + n - 1 in ends and not any(dl[off:off + n])
        whole = [c for c in range(off // 64, (off + n) // 64 + 1) if off <= 64 * c and 64 * c + 64 <= off + n]
        assert whole and all(not (starts & set(range(64 * c + (64 * c == off), 64 * c + 64))) for c in whole)
    assert any(n >= 129 for n in sc.LOAD_COVERS.values())
    # the families: every length, several occurrences of every word over the whole file, shared
    # first 16 bytes with the difference at byte 17, at byte 18 or in the last byte
    fam = sc.load_family()
    assert {len(w) for w in fam} >= set(sc.LOAD_LENGTHS)
    where = {}
    for i, w in enumerate(sc.words_of(d)):
        where.setdefault(w, []).append(i)
    nwords = sum(len(v) for v in where.values())
    assert set(where) == set(fam)
    for w in fam:
        assert len(where[w]) >= 3, w
        assert where[w][0] < nwords // 2 < where[w][-1] or len(w) == 1, w
    by_prefix = {}
    for w in fam:
        if len(w) > 16:
            by_prefix.setdefault((w[:16], len(w)), []).append(w)
    diffs = set()
    for (_, L), ws in by_prefix.items():
        for u in ws:
            for v in ws:
                at = [i for i in range(L) if u[i] != v[i]]
                if len(at) == 1:
                    diffs.add((L, "last" if at[0] == L - 1 else at[0] + 1))
    for L in (40, 64, 65, 129, 200):
        assert {(L, 17), (L, 18), (L, "last")} <= diffs
    assert (17, "last") in diffs and (18, 17) in diffs and (18, "last") in diffs
    # the rare byte is cut at coverage 0.9 and lands on unk
    freqs = encode_ref.vocab_freqs(case["vocab_bytes"], encode_ref.token_bytes(encode_ref.model_merges(case["model_bytes"])))
    assert freqs[ord("z")] == 0 and freqs[case["config"]["unk_id"]] == d.count(b"z")


# ---- the constants the recipes were written for --------------------------------------------------------
def _const(path, name):
    src = open(os.path.join(CSRC, path)).read()
    m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=\s*[^,;]+,\s*)*" + name + r"\s*=\s*([^,;]+)[,;]", src)
    assert m, f"{name} not found in {path}"
    return m.group(1).strip()


def test_constants_guard():
    """Whoever retunes one of these: regenerate tests/golden/shapes (make_golden.py shapes) with
    shape_corpora.py's lengths moved to the new boundary."""
    assert int(_const("hip/word_loop_dev.h", "kStripV")) == sc.K_STRIP_V
    assert int(_const("hip/word_loop_dev.h", "kRunHdr")) == sc.K_RUN_HDR
    assert _const("hip/word_loop_dev.h", "kStrip") == "4 * kStripV"
    assert _const("hip/word_loop_dev.h", "kStripTok") == "kStrip - kRunHdr"
    assert int(_const("host/tiles.h", "kTileTokens")) == sc.K_TILE_TOKENS
    assert int(_const("hip/hip_common.h", "kThreads")) == sc.K_THREADS
    assert int(_const("hip/hip_common.h", "kPer")) == sc.K_PER
    assert _const("hip/hip_common.h", "kChunk") == "kThreads * kPer"
    assert _const("hip/hip_common.h", "kWaveTok") == "64 * kPer" and 64 * sc.K_PER == sc.K_TILE_TOKENS
    assert int(_const("hip/load_device.hip", "kSpell")) == sc.K_SPELL
    assert int(_const("hip/load_device.hip", "kChunkBytes")) == sc.K_CHUNK_BYTES
    assert tuple(int(_const("hip/load_device.hip", n)) for n in
                 ("kNarrowThreads", "kWideThreads", "kXWideThreads")) == sc.LOAD_THREADS
    assert sc.LOAD_TILES == (16384, 32768, 49152) and sc.K_STRIP_TOK == 25 and sc.K_CHUNK == 4096
