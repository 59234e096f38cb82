"""Deterministic corpora that sit on the trainer's and the word-count kernel's structural edges.

Every corpus here is valid input, small (< 256 KB, at most 600 merges) and built from a seeded
``random.Random``; the expected output is the reference's own (tests/golden/shapes/<name>/, written
by tests/golden/make_golden.py).  The constants below are the ones the recipes were written for;
tests/test_shapes_cpu.py reads them back from the sources, so whoever retunes a kernel is told to
regenerate the shapes.

===============  ======================================================  ==========================
shape            constant                                                what switches there
===============  ======================================================  ==========================
strip_edge       kStripTok = 4*kStripV - kRunHdr = 25 (word_loop_dev.h)  ``L <= kStripTok``: the word
                                                                         is merged in registers, a
                                                                         longer one by the chain walk
tile_edge        kTileTokens = kWaveTok = 1024, header included          ``fill + need > kTileTokens``
                 (tiles.h, tiles.cpp pack_tiles, resident_loop.hip)      / ``len > kWaveTok``: a word
                                                                         of <= 1023 tokens shares a
                                                                         tile (k_resident), a longer
                                                                         one owns its tile (k_merge)
chunk_edge       kChunk = kThreads*kPer = 4096 (hip_common.h,            ``cs += kChunk``: a tile of
                 pair_count.hip)                                         more than 4096 tokens
                                                                         (header + 4096) is walked
                                                                         chunk by chunk
tile_edge_short  the same, cut at 1023 tokens                            every tile <= kWaveTok: the
                                                                         table is k_resident's, with
                                                                         one-word tiles of 1022..1024
tile_fill*       kTileTokens / (1 + 7) = 128 words per tile              the last tile exactly full,
                                                                         one word short, one over
load_edge        kSpell = 16, kChunkBytes = 64, tiles of 64 x            an LDS slot keeps 16 bytes;
                 256 / 512 / 768 threads = 16384 / 32768 / 49152 bytes   a thread owns 64 bytes of
                 (load_device.hip)                                       word starts; a workgroup
                                                                         owns one tile
degenerate       --                                                      no word, one word, no pair,
                                                                         one merge, a dry heap
===============  ======================================================  ==========================

The coverage cut.  The reference keeps ``(size_t)(distinct_bytes * coverage)`` byte values
(bpe.cpp:160-175), so with fewer than 200 distinct bytes it always drops at least one: the rarest by
*distinct-word* count.  The trainer shapes therefore use the alphabet ``a``-``d`` plus one
sacrificial word ``z``: the cut takes ``z`` and leaves the alphabet whole.  The degenerate corpora
that must merge (``one_merge``, ``one_run``, ``one_pair_once``) carry the same ``z`` word;
``ab_literal`` and ``run_literal`` are the bare inputs, where the cut maps ``b`` (resp. every byte)
to unk and nothing merges.
"""
from __future__ import annotations

import gzip
import json
import os
import random

# The values this module was written for (tests/test_shapes_cpu.py::test_constants_guard).
K_STRIP_V, K_RUN_HDR = 7, 3
K_STRIP_TOK = 4 * K_STRIP_V - K_RUN_HDR          # 25
K_TILE_TOKENS = 1024                             # header included: a shared word has <= 1023 tokens
K_THREADS, K_PER = 256, 16
K_CHUNK = K_THREADS * K_PER                      # 4096, header included: one chunk holds <= 4095 tokens
K_SPELL, K_CHUNK_BYTES = 16, 64
LOAD_THREADS = (256, 512, 768)                   # narrow / wide / xwide (SHREDWORD_LOAD_WIDE 0 / 1 / 2)
LOAD_TILES = tuple(K_CHUNK_BYTES * t for t in LOAD_THREADS)   # 16384, 32768, 49152

DELIMS = b" \t\r\n"
MAX_BYTES = 256 * 1024

_CFG = ("vocab_size", "unk_id", "character_coverage", "min_pair_freq")


def _cfg(vocab, unk=0, cov=0.995, mpf=2):
    return dict(zip(_CFG, (vocab, unk, cov, mpf)))


SHAPES = {
    "strip_edge": _cfg(700),
    "tile_edge": _cfg(800),
    "tile_edge_short": _cfg(800),
    "chunk_edge": _cfg(500),
    "tile_fill_m1": _cfg(400), "tile_fill_0": _cfg(400), "tile_fill_p1": _cfg(400),
    "tile_fill32_m1": _cfg(600), "tile_fill32_0": _cfg(600), "tile_fill32_p1": _cfg(600),
    "load_edge": _cfg(600, unk=5, cov=0.9),
    # degenerate
    "empty": _cfg(300), "delims_only": _cfg(300), "one_byte_word": _cfg(300), "single_chars": _cfg(300),
    "one_pair_once": _cfg(300), "one_merge": _cfg(300), "one_run": _cfg(300),
    "ab_literal": _cfg(300), "run_literal": _cfg(300),
}
DEGENERATE = ["empty", "delims_only", "one_byte_word", "single_chars", "one_pair_once", "one_merge", "one_run",
              "ab_literal", "run_literal"]
TILE_FILL = [n for n in SHAPES if n.startswith("tile_fill")]
TRAINER_SHAPES = ["strip_edge", "tile_edge", "tile_edge_short", "chunk_edge"] + TILE_FILL + DEGENERATE

# word lengths (in tokens = bytes) every corpus must hold
STRIP_LENGTHS = list(range(23, 29)) + list(range(46, 57))
TILE_LENGTHS = list(range(1021, 1027)) + list(range(2044, 2053))
TILE_SHORT_LENGTHS = [1021, 1022, 1023]   # header + 1023 = a tile of exactly kWaveTok tokens
CHUNK_LENGTHS = list(range(4094, 4099)) + list(range(8190, 8195))
TILE_FILL_WORDS = {"tile_fill_m1": 127, "tile_fill_0": 128, "tile_fill_p1": 129,
                   "tile_fill32_m1": 32 * 128 - 1, "tile_fill32_0": 32 * 128, "tile_fill32_p1": 32 * 128 + 1}
LOAD_LENGTHS = [15, 16, 17, 18, 40, 64, 65, 129, 200]
LOAD_SIZE = 5 * 49152
SACRIFICE = b"z"   # the word the coverage cut takes (see the module docstring)


def _fill(kind: str, n: int, rnd: random.Random, alphabet: bytes = b"abcd") -> bytes:
    if kind == "run":
        return b"a" * n
    if kind == "abab":
        return (b"ab" * (n // 2 + 1))[:n]
    if kind == "baba":  # b + ab * N: the same pairs shifted by one
        return (b"b" + b"ab" * (n // 2 + 1))[:n]
    if kind == "rand":
        return bytes(rnd.choice(alphabet) for _ in range(n))
    raise ValueError(kind)


def _short_words(rnd: random.Random, n: int, lo: int = 3, hi: int = 9) -> list:
    seen, out = set(), []
    while len(out) < n:
        w = bytes(rnd.choice(b"abcd") for _ in range(rnd.randint(lo, hi)))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def _emit(rnd: random.Random, counted: list) -> bytes:
    """Every (word, count) occurrence, shuffled, eight words to a line."""
    occ = [w for w, c in counted for _ in range(c)]
    rnd.shuffle(occ)
    out = bytearray()
    for i, w in enumerate(occ):
        out += w + (b"\n" if i % 8 == 7 else b" ")
    out += SACRIFICE + b"\n"
    assert len(out) < MAX_BYTES, len(out)
    return bytes(out)


def _strip_edge() -> bytes:
    rnd = random.Random(2501)
    counted = []
    for L in STRIP_LENGTHS:
        for kind in ("run", "abab", "rand"):
            # 51 words over the 39 counts 2..40: a stride of 7 keeps neighbours apart
            counted.append((_fill(kind, L, rnd), 2 + (7 * len(counted)) % 39))
    counted += [(w, rnd.randint(1, 6)) for w in _short_words(rnd, 300)]
    return _emit(rnd, counted)


def _tile_edge(lengths=TILE_LENGTHS) -> bytes:
    """k_resident takes a table only if every tile is at most kWaveTok tokens long (plan_resident),
    so tile_edge -- words of 1024 tokens and more -- runs k_merge on every path, and
    tile_edge_short, the same recipe cut at 1023 tokens, runs k_resident with full one-word tiles."""
    rnd = random.Random(102401)
    reps = [2, 3, 2, 5, 2, 4, 3, 2]
    counted = []
    for L in lengths:
        for kind in ("run", "abab", "rand"):
            counted.append((_fill(kind, L, rnd), reps[len(counted) % len(reps)]))
    counted += [(w, 1 + (i % 3 == 0)) for i, w in enumerate(_short_words(rnd, 2000))]
    return _emit(rnd, counted)


def _chunk_edge() -> bytes:
    """4094..4098: the ab / b+ab family (ab*N has an even, b+ab*N an odd length), a*N and seeded
    random over a-c at every length.  8190..8194: the ab family at every length, a*N at 8191 and
    8192 (two 8k runs keep the corpus under 256 KB and the CPU replay quick)."""
    rnd = random.Random(409601)
    counted = []
    for L in CHUNK_LENGTHS:
        counted.append((_fill("abab" if L % 2 == 0 else "baba", L, rnd), 2))
        if L < 8000:
            counted.append((_fill("run", L, rnd), 3 if L == 4097 else 2))
            counted.append((_fill("rand", L, rnd, b"abc"), 3 if L == 4096 else 2))
        elif L in (8191, 8192):
            counted.append((_fill("run", L, rnd), 2))
    counted += [(w, rnd.randint(1, 4)) for w in _short_words(rnd, 300)]
    return _emit(rnd, counted)


def _tile_fill(nwords: int) -> bytes:
    rnd = random.Random(7128)
    words = _short_words(rnd, nwords, 7, 7)
    out = bytearray()
    for rep in range(2):
        for i, w in enumerate(words):
            out += w + (b"\n" if i % 8 == 7 else b" ")
    # no sacrificial word here: it would be a word of the table.  The cut takes the rarest of a-d
    # (mapped to unk 0, still a token), which leaves every word 7 tokens long.
    return bytes(out)


# ---- load_edge -----------------------------------------------------------------------------------
_P1 = b"abcdabcdabcdabcd"   # a 16-byte prefix (kSpell); load_family() draws 15 more


def load_family() -> list:
    """Distinct words sharing their first 16 bytes: per prefix and length, variants that differ only
    at byte 17, at byte 18 or in the last byte (as far as the length allows).  Over 768 words, so
    that a device word table of 1024 slots (3/4 full at 768) has to grow."""
    rnd = random.Random(1664)
    prefixes = [_P1]
    while len(prefixes) < 16:
        p = bytes(rnd.choice(b"abcd") for _ in range(16))
        if p not in prefixes:
            prefixes.append(p)
    words = []
    for pre in prefixes:
        for L in LOAD_LENGTHS:
            if L <= 16:
                words.append(pre[:L])
                continue
            body = bytearray(pre + bytes(rnd.choice(b"abcd") for _ in range(L - 16)))
            variants = {bytes(body)}
            for pos in (16, 17, L - 1):          # byte 17, byte 18, the last byte
                if pos < L:
                    for c in (b"abcd" if L < 129 else b"ab"):
                        v = bytearray(body)
                        v[pos] = c
                        variants.add(bytes(v))
            words += sorted(variants)
    # the rare byte, behind a shared prefix (coverage 0.9 of 5 distinct bytes keeps 4: z -> unk)
    words += [_P1 + b"z", _P1 + b"az" + b"b" * 30, b"z"]
    words = sorted(set(words))
    rnd.shuffle(words)
    assert len(words) > 768
    return words


# layouts at an offset B (L1..L4 use words of the family; Z is a mixed delimiter run across B)
#   L1: a word starts at B-1            L2: a word starts at B (a delimiter at B-1)
#   L3: a word ends at B-1 (its last byte), a delimiter at B, a word starts at B+1
#   L4: a word ends at B, a delimiter at B+1
# A word cannot start at B-1 and at B at once, so every B carries one layout and every tile size
# (and the 64-byte thread chunk) meets all of L1..L4 at some multiple of it.
LOAD_ANCHORS = {
    64: "L1", 128: "L2", 192: "L3", 256: "L4", 320: "Z",
    64 * 100: "L1", 64 * 101: "L2", 64 * 102: "L3", 64 * 103: "L4",
    16384: "L1", 32768: "Z", 49152: "L1", 65536: "L1", 81920: "L2", 98304: "L2", 114688: "L3",
    131072: "L3", 147456: "L3", 163840: "L4", 180224: "L4", 196608: "L4", 212992: "Z", 229376: "L2",
}
# words that cover whole 64-byte chunks with no word start inside: (offset, length)
LOAD_COVERS = {64 * 40: 64, 64 * 50 + 1: 200, 64 * 60 - 1: 129, 64 * 70: 65}


def _load_edge() -> bytes:
    rnd = random.Random(49152)
    fam = load_family()
    by_len = {}
    for w in fam:
        by_len.setdefault(len(w), []).append(w)
    longs = [w for w in fam if len(w) >= 17]
    buf = bytearray()
    nxt = [0]

    def word():
        w = fam[nxt[0] % len(fam)]
        nxt[0] += 1
        return w

    def pad_to(off, mixed=False):
        """Words, then a delimiter run that ends exactly at `off` (the byte before `off` is a delimiter)."""
        while len(buf) + 260 < off:
            buf.extend(word() + (b"\n" if rnd.random() < 0.15 else b" "))
        gap = off - len(buf)
        assert gap >= 1, (off, len(buf))
        buf.extend(bytes(rnd.choice(DELIMS) for _ in range(gap)) if mixed else b" " * gap)

    events = sorted([(b, ("anchor", k)) for b, k in LOAD_ANCHORS.items()] +
                    [(o, ("cover", n)) for o, n in LOAD_COVERS.items()])
    for B, (what, arg) in events:
        if what == "cover":
            pad_to(B)
            buf.extend(by_len[arg][B % len(by_len[arg])] + b" ")
            continue
        # (the 64 * k anchors stand 64 bytes apart: words of at most 18 bytes there)
        pool_w = pool_v = longs if B >= 16384 else by_len[17] + by_len[18]
        w, v = rnd.choice(pool_w), rnd.choice(pool_v)
        if arg == "L1":
            pad_to(B - 1)
            buf.extend(w + b" ")
        elif arg == "L2":
            pad_to(B, mixed=True)
            buf.extend(w + b"\n")
        elif arg == "L3":
            pad_to(B - len(w))
            buf.extend(w + b"\t" + v + b" ")
        elif arg == "L4":
            pad_to(B + 1 - len(w))
            buf.extend(w + b"\r\n")
        elif arg == "Z":
            pad_to(B - 20)
            buf.extend(bytes(DELIMS[i % 4] for i in range(40)))
            buf.extend(v + b" ")
    last = by_len[40][0]
    pad_to(LOAD_SIZE - len(last))
    buf.extend(last)                      # the last word has no trailing delimiter
    assert len(buf) == LOAD_SIZE and LOAD_SIZE % 49152 == 0 and LOAD_SIZE < MAX_BYTES
    return bytes(buf)


_DEGENERATE = {
    "empty": b"",
    "delims_only": DELIMS * 50,
    "one_byte_word": b"a\n",
    "single_chars": b"a b c " * 40 + b"\n",
    "one_pair_once": b"ab\n" + SACRIFICE + b"\n",
    "one_merge": b"ab ab\n" + SACRIFICE + b"\n",
    "one_run": b"a" * 37 + b" " + b"a" * 37 + b"\n" + SACRIFICE + b"\n",
    "ab_literal": b"ab ab\n",
    "run_literal": b"a" * 37 + b" " + b"a" * 37 + b"\n",
}


def corpus_bytes(name: str) -> bytes:
    if name in _DEGENERATE:
        return _DEGENERATE[name]
    if name in TILE_FILL_WORDS:
        return _tile_fill(TILE_FILL_WORDS[name])
    if name == "tile_edge_short":
        return _tile_edge(TILE_SHORT_LENGTHS)
    return {"strip_edge": _strip_edge, "tile_edge": _tile_edge, "chunk_edge": _chunk_edge,
            "load_edge": _load_edge}[name]()


def build(name: str, path: str) -> None:
    with open(path, "wb") as f:
        f.write(corpus_bytes(name))


def words_of(data: bytes) -> list:
    """The corpus's words as the reference splits them (strtok on " \\t\\r\\n"; no NUL bytes here)."""
    return data.replace(b"\t", b" ").replace(b"\r", b" ").replace(b"\n", b" ").split()


SHAPES_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shapes")


def load_fixture(name: str) -> dict:
    """tests/golden/shapes/<name>/ in conftest.load_case's form."""
    d = os.path.join(SHAPES_GOLDEN, name)
    with open(os.path.join(d, "case.json")) as f:
        case = json.load(f)
    with open(os.path.join(d, "model.bin"), "rb") as f:
        case["model_bytes"] = f.read()
    with open(os.path.join(d, "vocab.txt"), "rb") as f:
        case["vocab_bytes"] = f.read()
    with gzip.open(os.path.join(d, "trace.txt.gz"), "rt") as f:
        case["trace"] = f.read()
    return case
