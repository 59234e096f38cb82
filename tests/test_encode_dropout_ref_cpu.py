"""The BPE-dropout reference (tests/encode_dropout_ref.py) pinned without a GPU: the hash and the
threshold against the known answers of include/shredword_encode.h's definition, p = 0 against the
oracle, p = 1 against the bytes, the drop rate and the independence of the decisions, and the fast word
loop against the literal one."""
import math
import random

import numpy as np
import pytest

import corpora
from conftest import load_case
from encode_dropout_ref import (WORD, dropped, encode_word_naive, ref_dropout_docs, ref_dropout_encode, threshold, u)
from encode_long_ref import TABLES, pairs
from encode_ref import derived_byte_map, model_merges, oracle_encode, token_bytes, vocab_freqs

GOLDEN = "mixed2m_v4000"


def test_hash_known_answers():
    assert u(0, 0, 0) == 0x6393d51c06c618dc
    assert u(0, 1, 0) == 0x4b2e3986f3b849c8
    assert u(1, 1, 0) == 0x90c4337784c94d55
    assert u(12345, 4096, 7) == 0x8f0d35819974ac32
    assert u(2 ** 64 - 1, 2 ** 40 + 3, 65278) == 0x14bba98226fc98f0


def test_library_refuses_a_null_encoder():
    """The two C calls exist and check their handle (no GPU is needed for that)."""
    import ctypes
    from shredword.cbase import lib
    assert lib.shred_encoder_set_dropout(None, 0.5, 1) == -1
    p, seed = ctypes.c_double(), ctypes.c_uint64()
    assert lib.shred_encoder_dropout(None, ctypes.byref(p), ctypes.byref(seed)) == -1


def test_threshold_known_answers():
    assert threshold(0.1) == 429496729
    assert threshold(0.5) == 2147483648
    assert threshold(1.0) == 4294967296
    assert threshold(1e-10) == 0
    assert threshold(0.0) == 0


def _golden():
    case = load_case(GOLDEN)
    merges = model_merges(case["model_bytes"])
    freqs = vocab_freqs(case["vocab_bytes"], token_bytes(merges))
    return case, merges, derived_byte_map(merges, freqs, case["config"]["unk_id"])


def test_p0_is_the_oracle_on_the_small_corpus():
    _, merges, bm = _golden()
    text = ("\n".join(corpora.SMALL_TEXTS * 3) + "\n").encode()
    for m, b in ((merges, bm), (merges, None), (TABLES["local_min"], None)):
        assert np.array_equal(ref_dropout_encode(m, b, text, 0.0, 5), oracle_encode(m, b, text))
    # a threshold of 0 with p > 0 is p = 0 too
    assert np.array_equal(ref_dropout_encode(merges, bm, text, 1e-10, 5), oracle_encode(merges, bm, text))


def test_p0_is_the_oracle_on_a_golden_model(case_corpus):
    case, path = case_corpus(GOLDEN)
    _, merges, bm = _golden()
    text = open(path, "rb").read()[:96 * 1024]
    text = text[:text.rindex(b" ") + 1]
    assert np.array_equal(ref_dropout_encode(merges, bm, text, 0.0, 0, pos_base=77), oracle_encode(merges, bm, text))


def test_p1_leaves_every_byte():
    _, merges, bm = _golden()
    text = ("\n".join(corpora.SMALL_TEXTS) + "\t\r\n").encode()
    want = np.array([bm[c] for c in text if c not in b"\t\r\n "], dtype=np.int32)
    for seed in (0, 9):
        assert np.array_equal(ref_dropout_encode(merges, bm, text, 1.0, seed), want)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("seed", [0, 1, 2, 12345, 2 ** 63])
def test_drop_rate(p, seed):
    n = 20000
    ids = ref_dropout_encode(pairs((b"a", b"b")), None, b"ab " * n, p, seed)
    merged = int(np.count_nonzero(ids == 256))
    unmerged = n - merged
    assert ids.size == merged + 2 * unmerged
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"p {p} seed {seed}: unmerged share {unmerged / n:.5f}, {abs(unmerged / n - p) / sigma:.2f} sigma")
    assert abs(unmerged / n - p) <= 4 * sigma


def test_decisions_are_independent():
    n, T = 20000, threshold(0.5)
    bound = 4 * math.sqrt(0.25 / n)
    ranks = sum(dropped(7, pos, 0, T) == dropped(7, pos, 1, T) for pos in range(n)) / n
    seeds = sum(dropped(7, pos, 0, T) == dropped(8, pos, 0, T) for pos in range(n)) / n
    print(f"agreement: rank 0 / rank 1 {ranks:.4f}, seed 7 / seed 8 {seeds:.4f}")
    assert abs(ranks - 0.5) <= bound and abs(seeds - 0.5) <= bound


def test_fast_word_loop_is_the_literal_one():
    rnd = random.Random(4)
    _, merges, bm = _golden()
    words = [bytes(rnd.choice(b"abcdxy") for _ in range(rnd.randint(1, 40))) for _ in range(150)]
    hand = b" ".join(words) + b" banana bananabanana\n"
    real = ("\n".join(corpora.SMALL_TEXTS)).encode()
    for m, b, text in ((TABLES["local_min"], None, hand), (TABLES["aa_aaaa"], None, b"aaaaaaaaaaaaaaaaa aaaa a " * 9),
                       (pairs((b"a", b"n"), (b"an", b"a")), None, hand), (merges, bm, real)):
        for p, seed in ((0.1, 1), (0.5, 2), (0.9, 3)):
            fast = ref_dropout_encode(m, b, text, p, seed, pos_base=11)
            assert np.array_equal(fast, ref_dropout_encode(m, b, text, p, seed, pos_base=11, word=encode_word_naive))


def test_dropout_only_splits_and_depends_on_the_position():
    _, merges, _ = _golden()
    toks = token_bytes(merges)
    text = ("\n".join(corpora.SMALL_TEXTS)).encode()
    plain = ref_dropout_encode(merges, None, text, 0.0, 0)
    a = ref_dropout_encode(merges, None, text, 0.3, 1)
    b = ref_dropout_encode(merges, None, text, 0.3, 1, pos_base=1)
    assert a.size > plain.size and not np.array_equal(a, b)
    spell = lambda ids: b"".join(toks[i] for i in ids)
    assert spell(a) == spell(plain) == b"".join(WORD.findall(text))


def test_docs_form_uses_the_copy_positions():
    m = pairs((b"a", b"n"), (b"an", b"a"))
    docs = [b"banana banana", b"", b"banana\nbanana ", b"ban"]
    text = b"".join(docs)
    off = np.cumsum([0] + [len(d) for d in docs])
    ids, row = ref_dropout_docs(m, None, text, off, 0.5, 6)
    parts = [ref_dropout_encode(m, None, d, 0.5, 6, pos_base=int(off[i]) + i) for i, d in enumerate(docs)]
    assert np.array_equal(ids, np.concatenate(parts))
    assert row.tolist() == np.cumsum([0] + [x.size for x in parts]).tolist() and row[2] == row[1]
