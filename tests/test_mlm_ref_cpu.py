"""Pins tests/mlm_ref.py, the Python restatement of the masked-LM definitions of
include/shredword_encode.h (shred_mlm_*) that tests/test_gpu_mlm.py compares the GPU with, and the
library's exports; no GPU.

The statistical bounds are derived, not measured: the selected count of n independent draws at
probability p is binomial, standard deviation sqrt(n p (1 - p)), and 5 of them leave a chance below
1e-6 per check; the mask / random / keep split of the s selected tokens is binomial in s in the same
way.  A seed that falls outside them points at the hash, not at luck.
"""
import ctypes
import math

import numpy as np
import pytest

from mlm_ref import ACT, SEL, T, d, mlm_ref, word_begins

# token lengths of a vocabulary with the merges "ab" (256), "abab" (257) and one special of 5 bytes (258)
LENS = [1] * 256 + [2, 4, 5]
SPECIALS = (258, 259)
A, B = ord("a"), ord("b")
KW = dict(p=0.5, seed=7, p_mask=0.8, p_random=0.1, mask_id=1000, rand_vocab=258)


def test_constants_and_hash():
    assert SEL == 1 << 40 and ACT == SEL + 1
    assert T(0) == 0 and T(1) == 2 ** 32 and T(0.5) == 2 ** 31 and T(0.15) == int(0.15 * 4294967296.0)
    # d is dropout's u with the constant in the rank's place
    from encode_dropout_ref import u
    assert d(5, 9, SEL) == u(5, 9, SEL) and d(5, 9, SEL) != d(5, 9, ACT)


def test_begin_row_boundary_between_contiguous_tokens():
    """"abab" + "abab" as two rows with nothing between them: the starts are contiguous (0, 2, 4, 6) and
    only the row boundary begins the second word."""
    ids, starts = [256, 256, 256, 256], [0, 2, 4, 6]
    assert word_begins(ids, [0, 2, 4], starts, LENS) == [True, False, True, False]
    assert word_begins(ids, None, starts, LENS) == [True, False, False, False]
    assert word_begins(ids, [0, 4], starts, LENS) == [True, False, False, False]
    # empty rows put no begin anywhere but at the next row's first token
    assert word_begins(ids, [0, 0, 2, 2, 2, 4, 4], starts, LENS) == [True, False, True, False]
    # a gap in starts (a delimiter in the text) begins a word
    assert word_begins(ids, None, [0, 2, 5, 7], LENS) == [True, False, True, False]


def test_begin_special_next_to_a_word():
    """ab<|s|>ab: the special is a word of its own and the token after it begins one."""
    ids, starts = [256, 258, 256], [0, 2, 7]
    assert word_begins(ids, None, starts, LENS, SPECIALS) == [True, True, True]
    assert word_begins(ids, None, starts, LENS, (0, 0)) == [True, False, False]  # not registered: by bytes only


def test_begin_protected_id_inside_a_word():
    ids, starts = [A, B, ord("c"), A], [0, 1, 2, 3]
    assert word_begins(ids, None, starts, LENS) == [True, False, False, False]
    assert word_begins(ids, None, starts, LENS, protected={B}) == [True, True, True, False]
    out, labels, sel = mlm_ref(ids, None, p=1, seed=1, p_mask=1, p_random=0, mask_id=9, protect=[B], whole_word=True,
                               starts=starts, lens=LENS)
    assert out.tolist() == [9, B, 9, 9] and labels.tolist() == [A, -100, ord("c"), A] and sel == 3


def test_begin_negative_ids():
    """unk_id = -1 tokens cover one byte each."""
    ids, starts = [-1, -1, A, -1], [0, 1, 2, 4]
    assert word_begins(ids, None, starts, LENS) == [True, False, False, True]
    ids = [2 ** 31 - 1, A]  # an id past the table covers one byte too
    assert word_begins(ids, None, [0, 1], LENS) == [True, False]


def test_p_zero_and_one():
    ids = np.arange(300, 400, dtype=np.int32)
    out, labels, sel = mlm_ref(ids, None, **dict(KW, p=0))
    assert sel == 0 and np.array_equal(out, ids) and (labels == -100).all()
    out, labels, sel = mlm_ref(ids, None, **dict(KW, p=1))
    assert sel == ids.size and np.array_equal(labels, ids)
    out, labels, sel = mlm_ref(ids, None, **dict(KW, p=1, protect=[300, 399], ignore_id=-7))
    assert sel == ids.size - 2 and labels[0] == labels[-1] == -7 and out[0] == 300 and out[-1] == 399


def test_p_mask_one_and_random_one():
    ids = np.arange(300, 400, dtype=np.int32)
    out, labels, sel = mlm_ref(ids, None, **dict(KW, p_mask=1, p_random=0))
    assert sel > 0 and (out[labels != -100] == 1000).all() and np.array_equal(out[labels == -100], ids[labels == -100])
    out, labels, sel = mlm_ref(ids, None, **dict(KW, p_mask=0, p_random=1, rand_vocab=1))
    assert (out[labels != -100] == 0).all()
    out, labels, sel = mlm_ref(ids, None, **dict(KW, p_mask=0, p_random=1, rand_vocab=2 ** 31 - 1))
    assert (out[labels != -100] >= 0).all() and np.unique(out[labels != -100]).size > sel // 2
    out, labels, sel = mlm_ref(ids, None, **dict(KW, p_mask=0, p_random=0))
    assert np.array_equal(out, ids) and sel > 0


def test_bad_arguments_are_rejected():
    ids = [1, 2, 3]
    with pytest.raises(ValueError):
        mlm_ref(ids, None, **dict(KW, p_mask=0.75, p_random=0.5))  # T(p_mask) + T(p_random) > 2^32
    mlm_ref(ids, None, **dict(KW, p_mask=0.5, p_random=0.5))      # exactly 2^32 is allowed
    for bad in (dict(p=-0.1), dict(p=1.5), dict(p=float("nan")), dict(p_random=0.1, rand_vocab=0),
                dict(p_random=0.1, rand_vocab=2 ** 31), dict(protect=list(range(17))), dict(whole_word=True)):
        with pytest.raises(ValueError):
            mlm_ref(ids, None, **dict(KW, **bad))
    for row in ([0, 2], [1, 3], [0, 2, 1, 3], [0, -1, 3]):
        with pytest.raises(ValueError):
            mlm_ref(ids, row, **KW)


def _stream(n_rows=40, seed=3):
    """Rows of "ab" / "abab" / byte tokens with starts: words of one to three tokens."""
    rng = np.random.default_rng(seed)
    ids, starts, row, pos = [], [], [0], 0
    for _ in range(n_rows):
        for _ in range(int(rng.integers(0, 6))):
            for _ in range(int(rng.integers(1, 4))):
                t = int(rng.choice([A, 256, 257]))
                ids.append(t)
                starts.append(pos)
                pos += LENS[t]
            pos += 1  # the delimiter
        row.append(len(ids))
    return np.array(ids, np.int32), np.array(starts, np.int64), np.array(row, np.int64)


@pytest.mark.parametrize("whole", [False, True])
def test_index_base_shift_equals_slicing(whole):
    ids, starts, row = _stream()
    kw = dict(KW, whole_word=whole, starts=starts if whole else None, lens=LENS, index_base=1 << 33)
    out, labels, sel = mlm_ref(ids, row, **kw)
    done = 0
    for r in (0, 7, 20, len(row) - 1):
        a = int(row[r])
        kw_a = dict(kw, starts=starts[a:] if whole else None, index_base=(1 << 33) + a)
        o, l, s = mlm_ref(ids[a:], row[r:] - a, **kw_a)
        assert np.array_equal(o, out[a:]) and np.array_equal(l, labels[a:]) and s == int((labels[a:] != -100).sum())
        done += 1
    assert done == 4 and 0 < sel < ids.size
    if whole:  # the tokens of a word share one fate
        begin = word_begins(ids.tolist(), row, starts, LENS)
        for k in range(1, ids.size):
            if not begin[k]:
                assert (labels[k] == -100) == (labels[k - 1] == -100)


@pytest.mark.parametrize("seed", [0, 1, 0xDEADBEEFCAFEF00D])
def test_hash_stays_inside_its_binomial_bounds(seed):
    n, p, pm, pr = 65536, 0.15, 0.8, 0.1
    ids = np.full(n, 300, dtype=np.int32)
    out, labels, sel = mlm_ref(ids, None, p=p, seed=seed, p_mask=pm, p_random=pr, mask_id=-5, rand_vocab=256)
    assert abs(sel - n * p) <= 5 * math.sqrt(n * p * (1 - p))  # about 457
    picked = labels != -100
    assert int(picked.sum()) == sel
    masked = int((out[picked] == -5).sum())
    rand = int((out[picked] < 256).sum()) - masked  # random ids lie in [0, 256), the kept id is 300
    kept = int((out[picked] == 300).sum())
    assert masked + rand + kept == sel
    for got, q in ((masked, pm), (rand, pr), (kept, 1 - pm - pr)):
        assert abs(got - sel * q) <= 5 * math.sqrt(sel * q * (1 - q))


def test_library_exports_the_masking_calls():
    """Needs no GPU: a NULL encoder is refused before any device work."""
    from shredword.cbase import ShredMlmOpts, lib
    assert ctypes.sizeof(ShredMlmOpts) == 80
    opts = ShredMlmOpts(0, 0.15, 0, 0.8, 0.1, 3, -100, 256, None, 0, 1, 0)
    buf = np.zeros(4, dtype=np.int32)
    out, labels = np.full(4, 77, np.int32), np.full(4, 77, np.int32)
    assert lib.shred_mlm_rows(None, buf.ctypes.data, 4, None, 0, ctypes.byref(opts), None, out.ctypes.data,
                              labels.ctypes.data) == -1
    assert lib.shred_mlm_device(None, buf.ctypes.data, 4, None, 0, ctypes.byref(opts), None, out.ctypes.data,
                                labels.ctypes.data, None, None) == -1
    assert (out == 77).all() and (labels == 77).all()
