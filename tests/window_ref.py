"""The windows of shred_window_* (include/shredword_encode.h) by a plain Python loop: every window
of a row is made as a list by stepping a start index until a window reaches the row's end.  No
closed-form count and no prefix sums: the six outputs are built from the lists."""
import numpy as np


def row_windows(ids, C, stride):
    """The windows of one row (a list of ids): [(start in the row, the ids the window holds)]."""
    assert C >= 1 and 0 <= stride < C
    out, start = [], 0
    while True:
        out.append((start, ids[start:start + C]))
        if start + C >= len(ids):
            return out
        start += C - stride


def windows(ids, row=None, *, max_len, stride=0, bos=None, eos=None, pad_id=0, pad="right", width=None):
    """-> (batch, lengths, window_rows, window_src, row_windows, mask) as numpy arrays."""
    ids = [int(x) for x in ids]
    bounds = [(0, len(ids))] if row is None else [(int(a), int(b)) for a, b in zip(row[:-1], row[1:])]
    add = (bos is not None) + (eos is not None)
    emitted, win_row, win_src, row_win = [], [], [], [0]
    for r, (a, b) in enumerate(bounds):
        for start, kept in row_windows(ids[a:b], max_len - add, stride):
            emitted.append(([bos] if bos is not None else []) + kept + ([eos] if eos is not None else []))
            win_row.append(r)
            win_src.append(a + start)
        row_win.append(len(emitted))
    W = max([len(e) for e in emitted], default=0) if width is None else width
    batch, mask = [], []
    for e in emitted:
        fill = W - len(e)
        assert fill >= 0
        batch.append(e + [pad_id] * fill if pad == "right" else [pad_id] * fill + e)
        mask.append([1] * len(e) + [0] * fill if pad == "right" else [0] * fill + [1] * len(e))
    n = len(emitted)
    return (np.array(batch, dtype=np.int32).reshape(n, W), np.array([len(e) for e in emitted], dtype=np.int32),
            np.array(win_row, dtype=np.int32), np.array(win_src, dtype=np.int64), np.array(row_win, dtype=np.int64),
            np.array(mask, dtype=np.uint8).reshape(n, W))
