"""The yardstick of test_gpu_pair.py checked by itself, without a GPU: for every la, lb in 0 .. 12 and
every budget B in 0 .. 9, the rows that pair_ref.py's loops emit have the kept counts of the closed
forms in include/shredword_encode.h, on both truncation sides; the windows of window_second (every
stride 0 .. C - 1, with and without max_first) have the count of the header's formula, step C - stride,
cover all of b, and carry the same kept_a; and exactly the examples the header names cannot fit."""
import numpy as np
import pytest

import pair_ref

N = 13


def _closed(la, lb, B):
    """(ka, kb) of longest_first as the header states it."""
    s = min(la, lb)
    if la + lb <= B:
        return la, lb
    if 2 * s <= B:
        return (la, B - la) if la <= lb else (B - lb, lb)
    return B - B // 2, B // 2


def _one(a, b, B, truncation, side):
    rows = pair_ref.pair_kept(a, b, B, truncation, side)
    assert len(rows) == 1
    return rows[0]


def test_truncation_loops_match_the_closed_forms():
    for la in range(N):
        for lb in range(N):
            a, b = list(range(100, 100 + la)), list(range(200, 200 + lb))
            for B in list(range(10)) + [None]:
                lim = 10 ** 9 if B is None else B
                for side in ("right", "left"):
                    where = (la, lb, B, side)
                    ka, kb = _closed(la, lb, lim)
                    kept_a, sa, kept_b, sb = _one(a, b, B, "longest_first", side)
                    assert (len(kept_a), len(kept_b)) == (ka, kb), where
                    assert ka + kb == min(la + lb, lim) and ka <= la and kb <= lb
                    for kept, src, seg in ((kept_a, sa, a), (kept_b, sb, b)):
                        assert src == (0 if side == "right" else len(seg) - len(kept)), where
                        assert kept == seg[src:src + len(kept)], where
                    # only_first / only_second: the other segment whole, or the example cannot fit
                    for truncation, fixed, cut in (("only_first", b, a), ("only_second", a, b)):
                        if len(fixed) > lim:
                            with pytest.raises(pair_ref.CannotFit):
                                pair_ref.pair_kept(a, b, B, truncation, side)
                            continue
                        row = _one(a, b, B, truncation, side)
                        got_fixed, got_cut = (row[2:], row[:2]) if truncation == "only_first" else (row[:2], row[2:])
                        assert got_fixed == (fixed, 0), where
                        k = min(len(cut), lim - len(fixed))
                        src = 0 if side == "right" else len(cut) - k
                        assert got_cut == (cut[src:src + k], src), where


def test_window_second_matches_the_header():
    for la in range(N):
        for lb in range(N):
            a, b = list(range(100, 100 + la)), list(range(200, 200 + lb))
            for B in range(10):
                for max_first in (None, 1, 3):
                    ka = la if max_first is None else min(la, max_first)
                    C = B - ka
                    for side in ("right", "left"):
                        # strides 0 .. C - 1 fit; stride == C (and any C <= 0) cannot
                        for stride in range(max(C, 0) + 1):
                            where = (la, lb, B, max_first, side, stride)
                            if C < stride + 1:
                                with pytest.raises(pair_ref.CannotFit):
                                    pair_ref.pair_kept(a, b, B, "window_second", side, stride, max_first)
                                continue
                            step = C - stride
                            wins = pair_ref.pair_kept(a, b, B, "window_second", side, stride, max_first)
                            assert len(wins) == (1 if lb <= C else 1 + -(-(lb - C) // step)), where
                            sa = 0 if side == "right" else la - ka
                            covered = []
                            for j, (kept_a, src_a, kept_b, src_b) in enumerate(wins):
                                assert (kept_a, src_a) == (a[sa:sa + ka], sa), where
                                assert src_b == j * step and kept_b == b[src_b:src_b + C], where
                                if j + 1 < len(wins):
                                    assert len(kept_b) == C
                                else:
                                    assert src_b + len(kept_b) == lb
                                covered += kept_b if j == 0 else kept_b[stride:]
                            assert covered == b, where


def test_outputs_are_built_from_the_rows():
    ids_a = np.arange(10, 16, dtype=np.int32)   # rows of 2, 0, 4 ids
    ids_b = np.arange(50, 59, dtype=np.int32)   # rows of 0, 0, 9 ids
    ra, rb = np.array([0, 2, 2, 6]), np.array([0, 0, 0, 9])
    kw = dict(max_len=10, bos=-1, sep=(-2, -3), eos=-4, pad_id=9)   # B = 6
    batch, lengths, prow, slen, ssrc, roww, types, mask = pair_ref.pairs(ids_a, ra, ids_b, rb, **kw)
    assert batch.tolist() == [[-1, 10, 11, -2, -3, -4, 9, 9, 9, 9], [-1, -2, -3, -4, 9, 9, 9, 9, 9, 9],
                              [-1, 12, 13, 14, -2, -3, 50, 51, 52, -4]]
    assert types.tolist() == [[0, 0, 0, 0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0, 0, 0, 0],
                              [0, 0, 0, 0, 0, 0, 1, 1, 1, 1]]
    assert lengths.tolist() == [6, 4, 10] and mask.sum(axis=1).tolist() == [6, 4, 10]
    assert prow.tolist() == [0, 1, 2] and roww.tolist() == [0, 1, 2, 3]
    assert slen.tolist() == [[2, 0], [0, 0], [3, 3]] and ssrc.tolist() == [[0, 0], [2, 0], [2, 0]]
    left = pair_ref.pairs(ids_a, ra, ids_b, rb, truncate="left", pad="left", width=11, **kw)
    assert left[0][2].tolist() == [9, -1, 13, 14, 15, -2, -3, 56, 57, 58, -4]
    assert left[4].tolist() == [[0, 0], [2, 0], [3, 6]] and left[6][0].tolist() == [0] * 10 + [1]
    # window_second: C = 6 - 4 = 2 for the last example, step 1
    win = pair_ref.pairs(ids_a, ra, ids_b, rb, truncation="window_second", stride=1, **kw)
    assert win[5].tolist() == [0, 1, 2, 10] and win[2].tolist() == [0, 1] + [2] * 8
    assert win[0][9].tolist() == [-1, 12, 13, 14, 15, -2, -3, 57, 58, -4]
    assert win[3][0].tolist() == [2, 0] and win[4][9].tolist() == [2, 7]
    with pytest.raises(pair_ref.CannotFit):
        pair_ref.pairs(ids_a, ra, ids_b, rb, truncation="window_second", stride=2, **kw)
    with pytest.raises(pair_ref.CannotFit):
        pair_ref.pairs(ids_a, ra, ids_b, rb, truncation="only_first", **kw)
    none = pair_ref.pairs([], [0], [], [0], max_len=4)
    assert none[0].shape == (0, 0) and none[5].tolist() == [0] and none[3].shape == (0, 2)
    empty = pair_ref.pairs([], [0, 0], [], [0, 0])
    assert empty[0].shape == (1, 0) and empty[1].tolist() == [0] and empty[4].tolist() == [[0, 0]]
