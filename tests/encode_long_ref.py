"""A Python reference encoder for words of any length (the oracle, oracle/encode_oracle.c, refuses
words above 1024 bytes).  It restates the definition of include/shredword_encode.h literally: words
are the maximal runs of bytes outside "\\t\\r\\n ", every byte becomes its byte-map id, and merge m
is applied to the word left to right without overlap, for m = 0, 1, ....  A merge whose operands
are both absent from the word is skipped (it cannot apply).  test_encode_long_ref_cpu.py pins it
against the oracle on words the oracle takes; the GPU tests of the long-word pass compare with it.
"""
import re

import numpy as np

WORD = re.compile(rb"[^\t\r\n ]+")


def apply_merge(toks, a, b, x):
    """One left-to-right pass without overlap: every (a, b) becomes x."""
    out, i, n = [], 0, len(toks)
    while i < n:
        if i + 1 < n and toks[i] == a and toks[i + 1] == b:
            out.append(x)
            i += 2
        else:
            out.append(toks[i])
            i += 1
    return out


def ref_encode_word(merges, byte_map, word: bytes) -> list:
    toks = [int(byte_map[c]) if byte_map is not None else c for c in word]
    present = set(toks)
    for a, b, x in merges:
        if a in present and b in present:
            new = apply_merge(toks, a, b, x)
            if len(new) != len(toks):
                toks = new
                present.add(x)
    return toks


def ref_encode(merges, byte_map, text: bytes) -> np.ndarray:
    """ids of every word of text, in text order."""
    m = [tuple(int(v) for v in row) for row in np.asarray(merges, dtype=np.int64).reshape(-1, 3)]
    seen, first = set(), []
    for a, b, x in m:  # a repeated pair never applies again: its first merge left none
        if (a, b) not in seen:
            seen.add((a, b))
            first.append((a, b, x))
    out = []
    for w in WORD.finditer(text):
        out.extend(ref_encode_word(first, byte_map, w.group()))
    return np.array(out, dtype=np.int32)


def ref_starts(merges, text: bytes, ids) -> np.ndarray:
    """Byte offset of every token: the ids' lengths (1 below 256 and for negative ids, else the sum of
    the merge's operands') tile the non-delimiter bytes of text in order."""
    lens = [1] * 256
    for a, b, _ in np.asarray(merges).reshape(-1, 3):
        lens.append(lens[a] + lens[b])
    starts, k, ids = [], 0, list(ids)
    for w in WORD.finditer(text):
        p = w.start()
        while p < w.end():
            assert k < len(ids), "fewer ids than the text's words need"
            starts.append(p)
            p += lens[ids[k]] if ids[k] >= 256 else 1
            k += 1
        assert p == w.end(), "a token spans a delimiter"
    assert k == len(ids), "more ids than the text's words need"
    return np.array(starts, dtype=np.int64)


def pairs(*ps):
    """Merges from byte-string pairs, each operand a byte or an earlier merge's token."""
    toks, out = {bytes([b]): b for b in range(256)}, []
    for a, b in ps:
        out.append([toks[a], toks[b], 256 + len(out)])
        toks[a + b] = 256 + len(out) - 1
    return np.array(out, dtype=np.int32).reshape(-1, 3)


# the hand-made tables of the long-word tests
AA = pairs((b"a", b"a"))
AA_AAAA = pairs((b"a", b"a"), (b"aa", b"aa"))
# local minima are not enough: abcd is Y d, not X Z (ranks 0, 1 and 5: three fillers between)
LOCAL_MIN = pairs((b"a", b"b"), (b"ab", b"c"), (b"x", b"y"), (b"y", b"x"), (b"x", b"x"), (b"c", b"d"))
LOCAL_MIN_2 = pairs((b"a", b"b"), (b"ab", b"c"), (b"c", b"d"))  # (c, d) at rank 2 as well
TABLES = {"aa": AA, "aa_aaaa": AA_AAAA, "local_min": LOCAL_MIN, "local_min_2": LOCAL_MIN_2}
