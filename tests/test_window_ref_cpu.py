"""The yardstick of test_gpu_window.py checked by itself, without a GPU: for every row length up to
40, every C up to 8 and every stride below C, the windows that window_ref.py's loop makes have the
count of the formula in include/shredword_encode.h (w = 1 if len <= C, else 1 + ceil((len - C) /
step)), cover every id of the row in order, overlap by exactly `stride` ids, and only the last is
short."""
import numpy as np

import window_ref


def test_loop_matches_the_header_on_all_small_rows():
    for C in range(1, 9):
        for stride in range(C):
            step = C - stride
            for n in range(41):
                ids = list(range(100, 100 + n))
                wins = window_ref.row_windows(ids, C, stride)
                assert len(wins) == (1 if n <= C else 1 + -(-(n - C) // step)), (n, C, stride)
                assert wins[0][0] == 0
                covered = []
                for j, (start, kept) in enumerate(wins):
                    assert start == j * step and kept == ids[start:start + C]
                    if j + 1 < len(wins):
                        assert len(kept) == C                                    # only the last may be short
                        assert kept[step:] == wins[j + 1][1][:stride]            # exactly `stride` shared ids
                        assert wins[j + 1][0] - start == step
                    else:
                        assert len(kept) == min(C, n) if j == 0 else 1 <= len(kept) <= C
                        assert start + len(kept) == n                            # the last window ends the row
                    covered += kept if j == 0 else kept[stride:]                 # what the window adds
                assert covered == ids, (n, C, stride)


def test_outputs_are_built_from_the_windows():
    ids = np.arange(10, 27, dtype=np.int32)  # rows of 0, 7, 0, 10 ids
    row = np.array([0, 0, 7, 7, 17], dtype=np.int64)
    batch, lengths, wrow, wsrc, roww, mask = window_ref.windows(ids, row, max_len=6, stride=1, bos=-1, eos=-2, pad_id=9)
    # C = 4, step = 3: the row of 7 has windows at 0 and 3, the row of 10 at 0, 3 and 6
    assert roww.tolist() == [0, 1, 3, 4, 7] and wrow.tolist() == [0, 1, 1, 2, 3, 3, 3]
    assert wsrc.tolist() == [0, 0, 3, 7, 7, 10, 13] and lengths.tolist() == [2, 6, 6, 2, 6, 6, 6]
    assert batch.shape == (7, 6) and batch[0].tolist() == [-1, -2, 9, 9, 9, 9]
    assert batch[2].tolist() == [-1, 13, 14, 15, 16, -2] and batch[6].tolist() == [-1, 23, 24, 25, 26, -2]
    assert mask.sum(axis=1).tolist() == lengths.tolist() and mask[0].tolist() == [1, 1, 0, 0, 0, 0]
    left = window_ref.windows(ids, row, max_len=6, stride=1, bos=-1, eos=-2, pad_id=9, pad="left", width=7)
    assert left[0][0].tolist() == [9, 9, 9, 9, 9, -1, -2] and left[5][0].tolist() == [0, 0, 0, 0, 0, 1, 1]
    one = window_ref.windows(ids, None, max_len=17)
    assert one[0].shape == (1, 17) and one[4].tolist() == [0, 1]
    none = window_ref.windows([], [0], max_len=4)
    assert none[0].shape == (0, 0) and none[4].tolist() == [0]
