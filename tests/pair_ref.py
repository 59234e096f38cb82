"""The emitted rows of shred_pair_* (include/shredword_encode.h) by plain Python loops: longest_first
removes one id at a time, the windows of the second segment are made by stepping a start index until
one reaches the segment's end.  No closed forms and no prefix sums: the eight outputs are built from
lists."""
import numpy as np

STRATEGIES = ("longest_first", "only_first", "only_second", "window_second")


class CannotFit(Exception):
    """An example that the strategy cannot make fit (the -7 of the C ABI)."""


def _cut(seg, keep, side):
    """(the kept ids, the index in seg of the first of them)."""
    assert 0 <= keep <= len(seg)
    return (seg[:keep], 0) if side == "right" else (seg[len(seg) - keep:], len(seg) - keep)


def pair_kept(a, b, B, truncation, truncate="right", stride=0, max_first=None):
    """The emitted rows of one example as [(kept_a, index in a of its first id, kept_b, index in b)].
    B: the budget of kept ids per emitted row, None for no limit."""
    if truncation == "longest_first":
        ka, kb = len(a), len(b)
        while B is not None and ka + kb > B:
            if ka > kb:
                ka -= 1
            else:
                kb -= 1
        return [_cut(a, ka, truncate) + _cut(b, kb, truncate)]
    if truncation == "only_first":
        if B is not None and len(b) > B:
            raise CannotFit
        ka = len(a) if B is None else min(len(a), B - len(b))
        return [_cut(a, ka, truncate) + (list(b), 0)]
    if truncation == "only_second":
        if B is not None and len(a) > B:
            raise CannotFit
        kb = len(b) if B is None else min(len(b), B - len(a))
        return [(list(a), 0) + _cut(b, kb, truncate)]
    assert truncation == "window_second" and B is not None
    kept_a, src_a = _cut(a, len(a) if not max_first else min(len(a), max_first), truncate)
    C = B - len(kept_a)
    if C < stride + 1:
        raise CannotFit
    out, start = [], 0
    while True:
        out.append((kept_a, src_a, b[start:start + C], start))
        if start + C >= len(b):
            return out
        start += C - stride


def pairs(ids_a, row_a, ids_b, row_b, *, max_len=None, truncation="longest_first", stride=0, max_first=None, bos=None,
          sep=(), eos=None, truncate="right", pad_id=0, pad="right", width=None):
    """-> (batch, lengths, pair_rows, seg_len, seg_src, row_windows, types, mask) as numpy arrays."""
    ids_a, ids_b = [int(x) for x in ids_a], [int(x) for x in ids_b]
    assert len(row_a) == len(row_b)
    sep = list(sep)
    head, tail = ([bos] if bos is not None else []), ([eos] if eos is not None else [])
    add = len(head) + len(sep) + len(tail)
    B = None if not max_len else max_len - add
    assert B is None or B >= 0
    emitted, typ, win_row, seg_len, seg_src, row_win = [], [], [], [], [], [0]
    for r in range(len(row_a) - 1):
        a0, a1, b0, b1 = int(row_a[r]), int(row_a[r + 1]), int(row_b[r]), int(row_b[r + 1])
        for kept_a, sa, kept_b, sb in pair_kept(ids_a[a0:a1], ids_b[b0:b1], B, truncation, truncate, stride, max_first):
            emitted.append(head + kept_a + sep + kept_b + tail)
            typ.append([0] * (len(head) + len(kept_a) + len(sep)) + [1] * (len(kept_b) + len(tail)))
            win_row.append(r)
            seg_len.append([len(kept_a), len(kept_b)])
            seg_src.append([a0 + sa, b0 + sb])
        row_win.append(len(emitted))
    W = max([len(e) for e in emitted], default=0) if width is None else width
    batch, types, mask = [], [], []
    for e, t in zip(emitted, typ):
        fill = W - len(e)
        assert fill >= 0
        batch.append(e + [pad_id] * fill if pad == "right" else [pad_id] * fill + e)
        types.append(t + [0] * fill if pad == "right" else [0] * fill + t)
        mask.append([1] * len(e) + [0] * fill if pad == "right" else [0] * fill + [1] * len(e))
    n = len(emitted)
    return (np.array(batch, dtype=np.int32).reshape(n, W), np.array([len(e) for e in emitted], dtype=np.int32),
            np.array(win_row, dtype=np.int32), np.array(seg_len, dtype=np.int32).reshape(n, 2),
            np.array(seg_src, dtype=np.int64).reshape(n, 2), np.array(row_win, dtype=np.int64),
            np.array(types, dtype=np.uint8).reshape(n, W), np.array(mask, dtype=np.uint8).reshape(n, W))
