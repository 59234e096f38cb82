"""A Python reference for BPE-dropout: the definition of include/shredword_encode.h
(shred_encoder_set_dropout) restated literally.

Words are the maximal runs of bytes outside "\\t\\r\\n "; the tokens of a word start as the byte-map
ids of its bytes; a candidate is an adjacent token pair the merge list knows (its rank: the first
merge that lists the pair); the candidate whose right token begins at byte position pos is dropped iff
(u(seed, pos, rank) >> 32) < T; among the candidates not dropped, the one of lowest rank merges, the
leftmost on a tie, until none is left.  pos counts from pos_base, the position of text[0] in the text
passed to the call; for the document calls it is the offset in the copy that holds one inserted byte
behind every document, so document d is encoded with base doc_off[d] + d.

encode_word_naive is the definition word for word (every candidate looked up again in every round);
encode_word keeps the candidates' masked ranks between rounds, which gives the same ids because a
decision is a function of (seed, pos, rank) alone.  tests/test_encode_dropout_ref_cpu.py pins both.
"""
import re

import numpy as np

WORD = re.compile(rb"[^\t\r\n ]+")
M64 = (1 << 64) - 1
GOLDEN_RATIO = 0x9E3779B97F4A7C15
NONE = 1 << 62  # "no rank"
ID_LIMIT = 1 << 20  # ids outside [0, 2^20) never merge


def mix(x: int) -> int:
    """murmur3's fmix64."""
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def u(seed: int, pos: int, rank: int) -> int:
    return mix(mix((seed + GOLDEN_RATIO * (pos + 1)) & M64) ^ rank)


def threshold(p: float) -> int:
    return int(float(p) * 4294967296.0)


def dropped(seed: int, pos: int, rank: int, T: int) -> bool:
    return (u(seed, pos, rank) >> 32) < T


def rank_table(merges) -> dict:
    """(first, second) -> rank; the first entry of a repeated pair wins."""
    ranks = {}
    for a, b, x in np.asarray(merges, dtype=np.int64).reshape(-1, 3).tolist():
        if 0 <= a < ID_LIMIT and 0 <= b < ID_LIMIT:
            ranks.setdefault((a, b), x - 256)
    return ranks


def _candidate(ranks, toks, begins, j, seed, T):
    """The rank of the candidate (toks[j], toks[j + 1]), NONE when the table has none or it is dropped."""
    r = ranks.get((toks[j], toks[j + 1]))
    if r is None or dropped(seed, begins[j + 1], r, T):
        return NONE
    return r


def encode_word_naive(ranks, toks, begins, seed, T) -> list:
    toks, begins = list(toks), list(begins)
    while len(toks) > 1:
        cand = [_candidate(ranks, toks, begins, j, seed, T) for j in range(len(toks) - 1)]
        best = min(cand)
        if best == NONE:
            break
        p = cand.index(best)  # the leftmost of lowest rank
        toks[p:p + 2] = [256 + best]
        del begins[p + 1]
    return toks


def encode_word(ranks, toks, begins, seed, T) -> list:
    toks, begins = list(toks), list(begins)
    cand = [_candidate(ranks, toks, begins, j, seed, T) for j in range(len(toks) - 1)]
    while cand:
        best = min(cand)
        if best == NONE:
            break
        p = cand.index(best)
        toks[p:p + 2] = [256 + best]
        del begins[p + 1]
        del cand[p]
        if p > 0:
            cand[p - 1] = _candidate(ranks, toks, begins, p - 1, seed, T)
        if p < len(cand):
            cand[p] = _candidate(ranks, toks, begins, p, seed, T)
    return toks


def ref_dropout_encode(merges, byte_map, text: bytes, p: float, seed: int, pos_base: int = 0, word=encode_word,
                       ranks=None) -> np.ndarray:
    """ids of every word of text, in text order, under dropout (p, seed)."""
    ranks = rank_table(merges) if ranks is None else ranks
    T = threshold(p)
    out = []
    for w in WORD.finditer(text):
        toks = [int(byte_map[c]) if byte_map is not None else c for c in w.group()]
        out.extend(word(ranks, toks, range(pos_base + w.start(), pos_base + w.end()), seed, T))
    return np.array(out, dtype=np.int32)


def ref_dropout_docs(merges, byte_map, text: bytes, doc_off, p: float, seed: int):
    """(ids, row_off) of the documents text[doc_off[d]:doc_off[d + 1]], each encoded as if alone, with
    the positions of the copy: base doc_off[d] + d."""
    ranks = rank_table(merges)
    off = [int(v) for v in doc_off]
    ids, row = [], [0]
    for d in range(len(off) - 1):
        ids.append(ref_dropout_encode(merges, byte_map, text[off[d]:off[d + 1]], p, seed, off[d] + d, ranks=ranks))
        row.append(row[-1] + ids[-1].size)
    flat = np.concatenate(ids) if ids else np.zeros(0, np.int32)
    return flat.astype(np.int32), np.array(row, dtype=np.int64)
