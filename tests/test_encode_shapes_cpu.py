"""CPU checks of the encoder's structural-edge shapes (tests/encode_shapes.py): every shape really has
the property it is named for, measured on the text itself and on the oracle encoder's ids, and the
constants the shapes were written for are still the sources'.  tests/test_gpu_encode_shapes.py runs
the shapes on the kernels; a shape that misses its claim is an error in the shape."""
import os
import re

import numpy as np
import pytest

import encode_shapes as es
from conftest import PKG
from encode_ref import oracle_encode

CSRC = os.path.join(PKG, "csrc")
C = es.K_CHUNK


def _const(rel, name):
    src = open(os.path.join(CSRC, rel)).read()
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([^;]+);", src)
    assert m, f"{name} not found in {rel}"
    return m.group(1).strip()


def test_constants_guard():
    """Whoever retunes one of these: move encode_shapes.py's offsets and lengths to the new boundary."""
    assert int(_const("hip/encode_words.h", "kThreads")) == es.K_THREADS
    assert int(_const("hip/encode_words.h", "kSpan")) == es.K_SPAN
    assert _const("hip/encode_words.h", "kChunk") == "kThreads * kSpan"
    assert int(_const("hip/encode_words.h", "kOverhang")) == es.K_OVERHANG
    assert _const("hip/encode_words.h", "kStageBytes") == "4 + kChunk + kOverhang"
    assert int(_const("hip/encode_device.hip", "kStrip")) == es.K_STRIP
    assert int(_const("hip/encode_device.hip", "kInlineBytes")) == es.K_INLINE_BYTES
    assert int(_const("hip/encode_device.hip", "kInlineIds")) == es.K_INLINE_IDS
    assert int(_const("hip/encode_device.hip", "kCacheProbes")) == es.K_CACHE_PROBES
    assert int(_const("host/encoder.h", "kEncMaxWord")) == es.K_MAX_WORD
    assert es.K_CHUNK == 4096 and es.K_STAGE_BYTES == 4356
    assert es.stage_window(0, 1 << 20) == (0, 4356) and es.stage_window(1, 1 << 20) == (4092, 8448)
    src = open(os.path.join(CSRC, "hip/encode_device.hip")).read()
    assert "packed_ = 256 + max_rank < 0xFFFFu;" in src


def _words(text):
    return [(m.start(), m.end() - m.start()) for m in es.WORD.finditer(text)]


def _lm(shape, word):
    """(L, m) of a word encoded alone."""
    return len(word), int(oracle_encode(shape.merges, None, word).size)


def test_shape_set():
    assert sorted(es.FAMILIES) == sorted(["strip", "inline_edges", "stage_hi_c0", "stage_hi_c1", "tail_mod4",
                                          "chunk_edges", "max_word", "id16_edge", "cache_grow",
                                          "cache_grow_then_direct", "arena", "capacity", "reuse"])
    assert len(es.MATRIX) == len(set(es.MATRIX)) == 46
    for name, s in es.SHAPES.items():
        assert len(s.text) < es.MAX_BYTES, name
        assert es.UNUSED_BYTE not in s.text, name
        assert np.array_equal(s.merges[:, 2], 256 + np.arange(len(s.merges))), name


@pytest.mark.parametrize("name", list(es.SHAPES))
def test_packings_share_their_ids(name):
    """The forced-unpacked byte map changes no expected id (and both reject what one rejects)."""
    a, b = es.expected(name, "packed"), es.expected(name, "unpacked")
    if es.SHAPES[name].claims.get("raises"):
        assert a is None and b is None
        return
    assert a is not None and a.dtype == np.int32 and np.array_equal(a, b)
    assert (es.byte_map("unpacked") < 0).sum() == 1 and es.byte_map("packed") is None


@pytest.mark.parametrize("name", [n for n in es.SHAPES if es.SHAPES[n].family not in
                                  ("cache_grow", "cache_grow_then_direct", "arena")])
def test_word_cache_holds_the_shape(name):
    """Nothing in these shapes may send the word cache to the direct path by design: the distinct words
    fit the arena (one int per byte of the text's chunks; header + ids + bytes per word) and are far
    fewer than one probe window, so a "direct path" line on the GPU is a kernel's doing."""
    s = es.SHAPES[name]
    distinct = {s.text[st:st + ln] for st, ln in _words(s.text)}
    arena = (len(s.text) + C - 1) // C * C
    assert sum(1 + len(w) + (len(w) + 3) // 4 for w in distinct) <= arena // 2, name
    assert len(distinct) <= 1024, name


@pytest.mark.parametrize("name", [n for n in es.SHAPES if "words" in es.SHAPES[n].claims])
def test_claimed_words_are_words_of_the_text(name):
    s = es.SHAPES[name]
    words = set(_words(s.text))
    assert s.claims["words"], name
    for sl in s.claims["words"]:
        assert tuple(sl) in words, (name, sl)
    for d in s.claims.get("delims", []):
        assert s.text[d] in es.DELIMS, (name, d)


@pytest.mark.parametrize("name", es.FAMILIES["strip"])
def test_strip(name):
    s = es.SHAPES[name]
    L = s.claims["L"]
    assert sorted(m for _, m in s.claims["lm"].values()) == sorted([1, (L + 1) // 2, L])
    for w, (wl, wm) in s.claims["lm"].items():
        assert _lm(s, w) == (wl, wm) == (L, wm)
        offs = {st % es.K_SPAN for st, ln in s.claims["words"] if s.text[st:st + ln] == w}
        assert {0, 31} <= offs, (name, w, offs)
    assert any(st >= C for st, _ in s.claims["words"])  # and behind the chunk seam
    assert (L > es.K_STRIP) == (name == "strip_33")


def test_inline_edges():
    s = es.SHAPES["inline_edges"]
    lm = s.claims["lm"]
    for want in ((8, 8), (9, 9), (16, 1), (16, 8), (16, 9), (17, 1), (17, 9), (32, 8)):
        assert want in lm.values()
    starts = {}
    for st, ln in _words(s.text):
        starts.setdefault(s.text[st:st + ln], []).append(st)
    for w, want in lm.items():
        assert _lm(s, w) == want, w
        assert len(starts[w]) >= 3 and len({st // C for st in starts[w]}) >= 2, w
    inline = lambda w: lm[w][0] <= es.K_INLINE_BYTES and lm[w][1] <= es.K_INLINE_IDS
    p = s.claims["pairs"]
    for key, L, both_inline in (("last_byte_16_inline", 16, True), ("last_byte_16_arena", 16, False),
                                ("last_byte_17", 17, False)):
        a, b = p[key]
        assert len(a) == len(b) == L and a[:-1] == b[:-1] and a[-1] != b[-1]
        assert inline(a) == inline(b) == both_inline
    a, b = p["prefix"]
    assert b.startswith(a) and len(a) == 16 and len(b) == 17 and inline(a) and not inline(b)


@pytest.mark.parametrize("name", es.FAMILIES["stage_hi_c0"] + es.FAMILIES["stage_hi_c1"])
def test_stage_window(name):
    s = es.SHAPES[name]
    c = s.claims
    lo, hi = es.stage_window(c["chunk"], len(s.text))
    assert hi == c["hi"] == (4356 if c["chunk"] == 0 else 8448) and len(s.text) > hi + 1
    cbase = c["chunk"] * C
    assert c["start"] - cbase in (4095, 4064) and c["end"] == hi + c["d"] and c["d"] in (-1, 0, 1)
    L = c["end"] - c["start"]
    assert 255 <= L <= 300 and L > es.K_STRIP
    assert (c["start"], L) in _words(s.text)
    w = s.text[c["start"]:c["end"]]
    # the same word once more, wholly inside the window, and nowhere else
    assert s.text[c["inside"]:c["inside"] + L] == w and lo <= c["inside"] and c["inside"] + L < hi
    assert (c["inside"], L) in _words(s.text) and s.text.count(w) == 2
    assert 1 < _lm(s, w)[1] < L


def test_stage_family_covers_every_end():
    for fam in ("stage_hi_c0", "stage_hi_c1"):
        got = {(es.SHAPES[n].claims["start"] % C, es.SHAPES[n].claims["d"]) for n in es.FAMILIES[fam]}
        assert got == {(st, d) for st in (4095, 4064) for d in (-1, 0, 1)}


def test_tail_mod4():
    assert tuple(es.SHAPES[n].claims["n"] for n in es.FAMILIES["tail_mod4"]) == es.TAIL_N == \
        (1, 2, 3, 5, 6, 7, 4095, 4096, 4097, 4098, 4099, 8191, 8193)
    tails = set()
    for name in es.FAMILIES["tail_mod4"]:
        s = es.SHAPES[name]
        n, tl = s.claims["n"], s.claims["tail"]
        assert len(s.text) == n and n % 4 == s.claims["mod4"] and 1 <= tl <= 5
        assert _words(s.text)[-1] == (n - tl, tl)  # reaches n, no trailing delimiter
        tails.add(tl)
        lo, hi = es.stage_window((n - 1) // C, n)
        assert n - hi == (n - lo) % 4  # the unstaged bytes
    assert tails == {1, 2, 3, 4, 5}
    assert {es.SHAPES[n].claims["mod4"] for n in es.FAMILIES["tail_mod4"]} == {0, 1, 2, 3}


def test_chunk_edges():
    S = es.SHAPES
    w = _words(S["chunk_word_ends_4095"].text)
    assert any(st + ln - 1 == C - 1 for st, ln in w) and S["chunk_word_ends_4095"].text[C] in es.DELIMS
    t = S["chunk_word_starts_4096"].text
    assert t[C - 1] in es.DELIMS and any(st == C for st, _ in _words(t))
    assert (C - 2, 5) in _words(S["chunk_word_straddles"].text)
    assert (C - 1, 2) in _words(S["chunk_two_byte_word"].text)
    for name in ("chunk_middle_empty", "chunk_all_empty", "chunk_last_byte_only"):
        s = S[name]
        assert (len(s.text) + C - 1) // C == s.claims["chunks"] == 3
        per_chunk = [sum(1 for st, _ in _words(s.text) if st // C == c) for c in range(3)]
        if "empty_chunks" in s.claims:
            assert [c for c in range(3) if per_chunk[c] == 0] == s.claims["empty_chunks"]
        if "total" in s.claims:
            assert es.expected(name).size == s.claims["total"]
    assert _words(S["chunk_last_byte_only"].text) == [(2 * C, 1)]
    assert es.expected("chunk_middle_empty").size > 0
    # no word of chunk 0 reaches into the empty middle chunk
    assert all(st + ln <= C for st, ln in _words(S["chunk_middle_empty"].text) if st < C)


def test_max_word():
    seen = set()
    for name in es.FAMILIES["max_word"]:
        s = es.SHAPES[name]
        L = s.claims["L"]
        (st, ln), = s.claims["words"]
        assert ln == L and (st, L) in _words(s.text)
        n = len(s.text)
        where = "end" if s.claims["at_end"] else st
        assert (st + L == n) == s.claims["at_end"]
        seen.add((L, where))
        if L == es.K_MAX_WORD:
            ids = es.expected(name)
            assert ids is not None and ids.size > 0 and 1 < _lm(s, s.text[st:st + L])[1] < L
        else:
            assert es.expected(name) is None  # the oracle rejects it too
            with pytest.raises(ValueError):
                oracle_encode(s.merges, None, s.text)
    assert seen == {(L, w) for L in (1024, 1025) for w in (0, 4064, 4095, "end")}


def test_id16_edge():
    for M, top, packs in ((65279, 0xFFFE, True), (65280, 0xFFFF, False)):
        s = es.SHAPES[f"id16_edge_{M}"]
        assert len(s.merges) == M and s.claims["top_id"] == top == 256 + M - 1 and s.claims["packs"] == packs
        assert (256 + (M - 1) < 0xFFFF) == packs  # the kernels' rule, on the largest rank
        assert s.merges[-1].tolist() == [256, 99, top]
        ids = es.expected(s.name)
        assert (ids == top).any() and (ids == 256).any()
        assert oracle_encode(s.merges, None, s.claims["fires"]).tolist() == [top]
        assert oracle_encode(s.merges, None, s.claims["not_fires"]).tolist() == [256]
        words = {s.text[st:st + ln] for st, ln in _words(s.text)}
        assert {s.claims["fires"], s.claims["not_fires"]} <= words


@pytest.mark.parametrize("name", ["cache_grow", "cache_grow_then_direct"])
def test_cache_shapes(name):
    s = es.SHAPES[name]
    words = [s.text[st:st + ln] for st, ln in _words(s.text)]
    distinct = set(words)
    assert len(distinct) == s.claims["distinct"] and len(words) == s.claims["each"] * len(distinct)
    start = int(s.claims["slots"].split(":")[0])
    assert len(distinct) > start  # more words than the starting table has slots: it must grow
    if "lengths" in s.claims:
        assert (min(map(len, distinct)), max(map(len, distinct))) == s.claims["lengths"]
    if "max_slots" in s.claims:
        assert len(distinct) > s.claims["max_slots"]  # and more than the ceiling: the direct path
    else:
        assert len(distinct) < 4 * start  # one growth step can hold them
    # the arena (one int per byte of the text's chunks) holds every word the table can: the only
    # flag is the full probe window (where the ceiling ends the call, the pass before it grows)
    need = sorted((1 + len(w) + (len(w) + 3) // 4 for w in distinct), reverse=True)
    arena = (len(s.text) + C - 1) // C * C
    assert sum(need[:start] if "max_slots" in s.claims else need) < arena


def test_arena_shape():
    s = es.SHAPES["arena_short_words"]
    distinct = {s.text[st:st + ln] for st, ln in _words(s.text)}
    assert len(distinct) == s.claims["distinct"] == len(_words(s.text)) and {len(w) for w in distinct} == {3}
    arena = (len(s.text) + C - 1) // C * C
    assert len(s.text) == 4095 and sum(1 + len(w) + (len(w) + 3) // 4 for w in distinct) > arena


def test_capacity_and_reuse_shapes():
    s = es.SHAPES["capacity"]
    nchunks = (len(s.text) + C - 1) // C
    assert nchunks == s.claims["chunks"] >= 3
    assert all(any(st // C == c for st, _ in _words(s.text)) for c in range(nchunks))
    a, b, short = es.SHAPES["reuse_a"], es.SHAPES["reuse_b"], es.SHAPES["reuse_short"]
    assert len(a.text) == len(b.text) == 40 * 1024 and a.text != b.text and len(short.text) == 5
    assert not np.array_equal(es.expected("reuse_a"), es.expected("reuse_b"))
