"""Deterministic texts that sit on the structural edges of the encoder core
(csrc/hip/encode_device.hip: k_cache_insert / k_cache_encode / k_cache_words / k_encode_words, and the
word walk and LDS staging of csrc/hip/encode_words.h).

Every shape is ``(merges, byte_map, text, claims)``: the byte map comes from ``byte_map(packing)``, the
rest from ``SHAPES[name]``.  No offset is random: every feature sits at a computed byte position, and
the filler between features is short words of ``klmn`` joined by single delimiters, so the positions
are exact.  ``claims`` states what the shape is named for; tests/test_encode_shapes_cpu.py verifies
every claim against the text and the oracle, so a GPU test cannot pass by missing its edge.  The
constants below are the ones the shapes were written for; the CPU test reads them back from the
sources.

================  ==========================================  =====================================
family            constant                                    what switches there
================  ==========================================  =====================================
strip             kStrip = 32, kSpan = 32                     ``L <= kStrip``: the word merges on the
                                                              thread's LDS strip, a longer one in
                                                              global scratch; span offsets 0 and 31
inline_edges      kInlineBytes = 16, kInlineIds = 8           bytes and ids inline in the slot, or
                                                              in the arena: two stores, two compares
stage_hi_c0/_c1   kStageBytes = 4 + kChunk + kOverhang        TextView reads LDS inside [lo, hi) and
                  = 4356: windows [0, 4356), [4092, 8448)     global memory outside
tail_mod4         the window is cut to whole 4-byte words     the last n % 4 bytes are never staged
chunk_edges       kChunk = kThreads * kSpan = 4096            one workgroup per chunk; the look-back
                                                              over chunks with and without ids
max_word          kEncMaxWord = 1024                          1024 accepted, 1025 rejected
id16_edge         packed_ = 256 + max_rank < 0xFFFF           16-bit LDS packing; 0xFFFF = "no rank"
cache_grow*       SHREDWORD_ENCODE_CACHE_SLOTS                the table grows 4x on a full probe
                                                              window, then takes the direct path
arena             one int per byte of the text's chunks       all-distinct short words overflow it
                                                              (1 + L + ceil(L / 4) ints per word)
capacity, reuse   --                                          several chunks with ids in each
================  ==========================================  =====================================

Alphabet.  ``0x80..0xA0`` (33 distinct bytes): a chain of merges fuses any prefix of them into one
token.  ``ef``: one pair merge.  ``ghij``: a chain to one token.  ``x``, ``y``: no merge ever names
them.  ``klmn``: 60 trainer-like merges (the filler and the long words).  ``0xFF`` occurs in no text:
the forced-unpacked byte map sends it to -1, which switches the 16-bit packing off without changing
any expected id.
"""
from __future__ import annotations

import random
import re
from collections import namedtuple

import numpy as np

# The values this module was written for (tests/test_encode_shapes_cpu.py::test_constants_guard).
K_THREADS, K_SPAN = 128, 32
K_CHUNK = K_THREADS * K_SPAN                     # 4096
K_OVERHANG = 256
K_STAGE_BYTES = 4 + K_CHUNK + K_OVERHANG         # 4356
K_STRIP = 32
K_INLINE_BYTES, K_INLINE_IDS = 16, 8
K_MAX_WORD = 1024
K_CACHE_PROBES = 128

WORD = re.compile(rb"[^\t\r\n ]+")
DELIMS = b" \t\r\n"
MAX_BYTES = 64 * 1024
PACKINGS = ("packed", "unpacked")
UNUSED_BYTE = 0xFF

Shape = namedtuple("Shape", "name family merges text claims")


def byte_map(packing):
    """None (identity: the 16-bit packing is on when the merge list allows it), or the identity with
    one byte no text holds sent to -1, which forces the 32-bit strips."""
    if packing == "packed":
        return None
    assert packing == "unpacked"
    bm = np.arange(256, dtype=np.int32)
    bm[UNUSED_BYTE] = -1
    return bm


def stage_window(chunk, n):
    """[lo, hi) of the text the kernels stage in LDS for `chunk` (encode_words.h stage_chunk)."""
    cbase = chunk * K_CHUNK
    lo = cbase - 4 if cbase >= 4 else 0
    hi = min(lo + K_STAGE_BYTES, n)
    return lo, lo + 4 * ((hi - lo) // 4)


# ---- merges -------------------------------------------------------------------------------------

def _random_merges(rng, alphabet, M):
    """A trainer-like merge list over `alphabet`: operands drawn from ids that exist."""
    ids = list(alphabet)
    out = []
    seen = set()
    while len(out) < M:
        a, b = int(rng.choice(ids)), int(rng.choice(ids))
        if (a, b) in seen:
            continue
        seen.add((a, b))
        out.append([a, b, 256 + len(out)])
        ids.append(256 + len(out) - 1)
    return np.array(out, dtype=np.int32)


def _chain_merges(word: bytes):
    """Merges that fuse `word` (distinct bytes) into one token: (w0, w1), (256, w2), ..."""
    out, left = [], word[0]
    for i, c in enumerate(word[1:]):
        out.append([left, c, 256 + i])
        left = 256 + i
    return np.array(out, dtype=np.int32)


def _rebase(merges, base):
    """`merges` (numbered from 256) moved behind `base` earlier merges."""
    return np.where(merges >= 256, merges + base, merges).astype(np.int32)


CHAIN = bytes(range(0x80, 0x80 + 33))            # CHAIN[:k] -> one token, k = 2 .. 33
PAIR = b"ef"                                     # -> one token
QUAD = b"ghij"                                   # -> one token
NEVER = b"xy"                                    # never merge
ALPHA = b"klmn"


def _base_merges():
    parts, base = [], 0
    for m in (_chain_merges(CHAIN), _chain_merges(PAIR), _chain_merges(QUAD),
              _random_merges(np.random.default_rng(41), list(ALPHA), 60)):
        parts.append(_rebase(m, base))
        base += len(m)
    out = np.concatenate(parts).astype(np.int32)
    assert np.array_equal(out[:, 2], 256 + np.arange(len(out)))
    return out


MERGES = _base_merges()


def _never(L):
    return (NEVER * L)[:L]


# ---- texts --------------------------------------------------------------------------------------

def _word_no(i):
    """Short distinct words of klmn: the base-4 digits of i, 1 to 6 bytes."""
    out = bytearray()
    i += 1
    while i:
        out.append(ALPHA[i & 3])
        i >>= 2
    return bytes(out)


FILLER_WORDS = 61


def _filler(nbytes, start=0):
    """Exactly nbytes of short words and single delimiters, a word first and a delimiter last (one
    delimiter alone for nbytes == 1).  Neighbours differ, but the words repeat with period 61 (each
    `start` has its own 61): a text of all-distinct short words would overflow the word arena, which
    holds one int per text byte and spends 1 + L + ceil(L / 4) on a word of L bytes, and the call
    would rightly rerun on the direct path."""
    out = bytearray()
    i = start
    first = 64 * (start % 40)
    while len(out) < nbytes:
        rem = nbytes - len(out)
        if rem == 1:
            out += b" "
            break
        w = _word_no(first + i % FILLER_WORDS)
        if len(w) + 1 > rem or rem - (len(w) + 1) == 1:
            w = (w * 8)[:rem - 1]
        out += w
        out.append(b"   \n \t \r "[i % 9])
        i += 1
    assert len(out) == nbytes
    return bytes(out)


def _long_word(L, seed):
    r = random.Random(seed)
    return bytes(r.choice(ALPHA) for _ in range(L))


class _Text:
    """A text built left to right: words placed at exact offsets, filler between them."""

    def __init__(self):
        self.b = bytearray()
        self.placed = []   # (start, word)
        self._fill = 0

    def at(self, s, word):
        need = s - len(self.b)
        assert need >= 0, (s, len(self.b))
        if self.b and self.b[-1] not in DELIMS:
            assert need >= 1, (s, len(self.b))
            self.b += b" "
            need -= 1
        self.b += _filler(need, self._fill)
        self._fill += 101
        assert len(self.b) == s
        self.b += word
        self.placed.append((s, bytes(word)))
        return self

    def raw(self, data):
        self.b += data
        return self

    def fill_to(self, n):
        """Filler up to exactly n bytes (the text then ends in a delimiter)."""
        return self.at(n, b"")

    def done(self):
        self.placed = [(s, w) for s, w in self.placed if w]
        return bytes(self.b)


def _words_claim(t):
    return [(s, len(w)) for s, w in t.placed]


SHAPES = {}
FAMILIES = {}


def _add(name, family, text, claims, merges=None):
    assert name not in SHAPES
    SHAPES[name] = Shape(name, family, MERGES if merges is None else merges, text, claims)
    FAMILIES.setdefault(family, []).append(name)


def _build_strip():
    for L in (31, 32, 33):
        kinds = {"never": _never(L), "one": CHAIN[:L], "half": (PAIR * L)[:L]}
        t, pos = _Text(), 0
        for w in kinds.values():
            for off in (0, 31):
                s = pos + (off - pos) % K_SPAN         # the next span offset `off` behind a delimiter
                t.at(s, w)
                pos = s + L + 1
        # and once more behind the chunk seam, span offsets 0 and 31 of the second chunk
        t.at(K_CHUNK, kinds["one"]).at(K_CHUNK + 3 * K_SPAN + 31, kinds["never"])
        t.fill_to(K_CHUNK + 512)
        text = t.done()
        _add(f"strip_{L}", "strip", text,
             {"L": L, "words": _words_claim(t),
              "lm": {kinds["never"]: (L, L), kinds["one"]: (L, 1), kinds["half"]: (L, (L + 1) // 2)}})


def _build_inline():
    lm = {
        _never(8): (8, 8),
        _never(9): (9, 9),
        CHAIN[:16]: (16, 1),
        PAIR * 8: (16, 8),
        PAIR * 7 + NEVER: (16, 9),
        CHAIN[:17]: (17, 1),
        PAIR * 8 + b"x": (17, 9),
        QUAD * 8: (32, 8),
        # the partners of the pairs below
        CHAIN[:15] + b"x": (16, 2),
        CHAIN[:16] + b"x": (17, 2),
        PAIR * 7 + b"xx": (16, 9),
    }
    pairs = {
        "last_byte_16_inline": (CHAIN[:16], CHAIN[:15] + b"x"),
        "last_byte_16_arena": (PAIR * 7 + NEVER, PAIR * 7 + b"xx"),
        "last_byte_17": (CHAIN[:17], CHAIN[:16] + b"x"),
        "prefix": (CHAIN[:16], CHAIN[:17]),
    }
    block = b" ".join(lm) + b" "
    t = _Text()
    t.raw(block).raw(_filler(700)).raw(block)
    t.fill_to(K_CHUNK + 64)
    t.raw(block).raw(_filler(300, 7))
    text = t.done()
    _add("inline_edges", "inline_edges", text, {"lm": lm, "pairs": pairs})


def _build_stage():
    for chunk in (0, 1):
        cbase = chunk * K_CHUNK
        for start in (4095, 4064):
            for d in (-1, 0, 1):
                s = cbase + start
                # the window's end does not depend on n once the text reaches past it
                hi = stage_window(chunk, 1 << 20)[1]
                L = hi + d - s
                w = _long_word(L, 1000 * chunk + start + d)
                t = _Text()
                t.at(cbase + 64, w)      # the same word, fully inside the chunk's window
                t.at(s, w)
                t.fill_to(hi + 700)
                text = t.done()
                _add(f"stage_hi_c{chunk}_s{start}_e{'m1' if d < 0 else 'p' + str(d)}", f"stage_hi_c{chunk}", text,
                     {"chunk": chunk, "start": s, "end": s + L, "hi": hi, "d": d, "inside": cbase + 64,
                      "words": _words_claim(t)})


TAIL_N = (1, 2, 3, 5, 6, 7, 4095, 4096, 4097, 4098, 4099, 8191, 8193)


def _build_tail():
    for n in TAIL_N:
        tl = min(n, (n - 1) % 5 + 1)
        t = _Text()
        t.at(n - tl, (b"klmnk")[:tl])
        text = t.done()
        _add(f"tail_n{n}", "tail_mod4", text, {"n": n, "mod4": n % 4, "tail": tl, "words": _words_claim(t)})


def _build_chunk_edges():
    C = K_CHUNK
    t = _Text().at(C - 5, b"klmnk")                      # last byte 4095, delimiter at 4096
    t.raw(b" ").fill_to(C + 300)
    _add("chunk_word_ends_4095", "chunk_edges", t.done(), {"words": _words_claim(t), "delims": [C]})
    t = _Text().fill_to(C).at(C, b"klmnk").fill_to(C + 300)   # delimiter at 4095, word from 4096
    _add("chunk_word_starts_4096", "chunk_edges", t.done(), {"words": _words_claim(t), "delims": [C - 1]})
    t = _Text().at(C - 2, b"klmnk").fill_to(C + 300)     # bytes 4094 .. 4098
    _add("chunk_word_straddles", "chunk_edges", t.done(), {"words": _words_claim(t), "delims": [C - 3, C + 3]})
    t = _Text().at(C - 1, b"kl").fill_to(C + 300)        # bytes 4095, 4096
    _add("chunk_two_byte_word", "chunk_edges", t.done(), {"words": _words_claim(t), "delims": [C - 2, C + 1]})
    mid = (b" \t\r\n" * (C // 4))
    text = _filler(C) + mid + _filler(1500, 11)
    _add("chunk_middle_empty", "chunk_edges", text, {"empty_chunks": [1], "chunks": 3})
    _add("chunk_all_empty", "chunk_edges", mid * 3, {"empty_chunks": [0, 1, 2], "chunks": 3, "total": 0})
    _add("chunk_last_byte_only", "chunk_edges", b" " * (2 * C) + b"k", {"words": [(2 * C, 1)], "chunks": 3, "total": 1})


def _build_max_word():
    C = K_CHUNK
    for L in (K_MAX_WORD, K_MAX_WORD + 1):
        w = _long_word(L, L)
        for tag, s in (("s0", 0), ("s4064", C - K_SPAN), ("s4095", C - 1), ("end", None)):
            t = _Text()
            if s is None:
                t.at(5000, w)                            # ends at n, no delimiter behind it
            else:
                t.at(s, w).fill_to(s + L + 600)
            text = t.done()
            _add(f"max_word_{L}_{tag}", "max_word", text,
                 {"L": L, "words": _words_claim(t), "raises": L > K_MAX_WORD, "at_end": s is None})


def _build_id16():
    for M in (65279, 65280):
        merges = np.empty((M, 3), dtype=np.int32)
        merges[:, 0], merges[:, 1] = 97, 98              # repeated pair: only its first entry counts
        merges[:, 2] = 256 + np.arange(M)
        merges[-1, :2] = (256, 99)                       # rank M - 1 -> the top id
        text = b"abc ab abcabc ca cabc abca bca abcab c " * 40
        _add(f"id16_edge_{M}", "id16_edge", text,
             {"M": M, "top_id": 256 + M - 1, "packs": M == 65279, "fires": b"abc", "not_fires": b"ab"}, merges)


def _distinct_words(count, digits):
    """`count` distinct words: `digits` letters of a..p spelling i, then 0 .. 12 - digits - 1 more."""
    out = []
    for i in range(count):
        head = bytes(97 + ((i >> (4 * k)) & 15) for k in range(digits))
        out.append(head + (head * 4)[:i % (13 - digits)])
    return out


def _build_cache():
    w = _distinct_words(3000, 3)
    text = b" ".join(w) + b"\n" + b" ".join(reversed(w)) + b"\n"
    _add("cache_grow", "cache_grow", text, {"distinct": 3000, "each": 2, "slots": "1024", "lengths": (3, 12)})
    w = _distinct_words(6000, 4)
    text = b" ".join(w) + b"\n"
    _add("cache_grow_then_direct", "cache_grow_then_direct", text,
         {"distinct": 6000, "each": 1, "slots": "1024:4096", "max_slots": 4096})


def _build_arena():
    # 1024 distinct 3-byte words in one chunk: 5 ints each (header, ids, bytes) against 4 text bytes
    w = [bytes(97 + ((i >> (4 * k)) & 15) for k in range(3)) for i in range(1024)]
    _add("arena_short_words", "arena", b" ".join(w), {"distinct": 1024, "L": 3})


def _build_capacity_and_reuse():
    _add("capacity", "capacity", _filler(3 * K_CHUNK + 500, 23), {"chunks": 4})
    a, b = _filler(40 * 1024, 0), _filler(40 * 1024, 1777)
    _add("reuse_a", "reuse", a, {"other": "reuse_b"})
    _add("reuse_short", "reuse", b"kl mn", {"n": 5})
    _add("reuse_b", "reuse", b, {"other": "reuse_a"})


for _f in (_build_strip, _build_inline, _build_stage, _build_tail, _build_chunk_edges, _build_max_word,
           _build_id16, _build_cache, _build_arena, _build_capacity_and_reuse):
    _f()

# what tests/test_gpu_encode_shapes.py runs over shape x packing x path x entry
MATRIX_FAMILIES = ("strip", "inline_edges", "stage_hi_c0", "stage_hi_c1", "tail_mod4", "chunk_edges", "max_word",
                   "id16_edge")
MATRIX = [n for f in MATRIX_FAMILIES for n in FAMILIES[f]]

_EXPECTED = {}


def expected(name, packing="packed"):
    """The oracle's ids of a shape (read-only, computed once), or None where the oracle rejects the text."""
    from encode_ref import oracle_encode
    key = (name, packing)
    if key not in _EXPECTED:
        s = SHAPES[name]
        try:
            ids = oracle_encode(s.merges, byte_map(packing), s.text) if s.text else np.zeros(0, np.int32)
            ids.setflags(write=False)
        except ValueError:
            ids = None
        _EXPECTED[key] = ids
    return _EXPECTED[key]
