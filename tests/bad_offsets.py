"""Offset arrays that are bad at entry 256: the first entry of the second workgroup of a row pass (256
threads, one per entry), so the thread that finds a descent reads its neighbour, entry 255, across the
workgroup boundary.  The unit tests of every call that takes an offset array on the device add these to
their own small cases (a bad first or last entry, a descent, a negative entry, one above n)."""
import numpy as np


def _good(rows, n):
    row = np.minimum(np.arange(rows + 1, dtype=np.int64) * 2, n)
    row[-1] = n
    return row


def at_256(n):
    """Arrays over n >= 3 elements, good up to entry 255.  300 rows: entry 256 negative, above n (entry 257
    then descends from it too) or below entry 255.  256 rows, so entry 256 is the last entry and the only
    thread of its workgroup: it is n - 1, or it descends from entry 255 (which is then n)."""
    out = []
    for bad in (-1, n + 1, None):
        row = _good(300, n)
        row[256] = row[255] - 1 if bad is None else bad
        out.append(row.tolist())
    out.append(np.minimum(_good(256, n), n - 1).tolist())
    last = _good(256, n)
    last[255], last[256] = n, n - 1
    out.append(last.tolist())
    assert all(len(r) > 256 and r[255] >= 1 for r in out)
    return out
