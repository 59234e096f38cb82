"""A Python reference for the fill-in-the-middle calls: the definitions of include/shredword_encode.h
(shred_fim_*) restated literally, row by row.

    d(x, c), T(q)   those of the masked-LM section (mlm_ref)
    row r of length L, h = row_base + r:
      transformed  iff  L >= min_len and (d(h, FIM) >> 32) < T(fim_rate)
      x = ((d(h, CUT_A) >> 32) * (L + 1)) >> 32, y the same from CUT_B (uint64), a = min, b = max
      mode = 1 (SPM) iff (d(h, MODE) >> 32) < T(spm_rate), else 0 (PSM)
      PSM: pre prefix suf suffix mid middle      SPM: pre suf suffix mid prefix middle

tests/test_fim_ref_cpu.py pins this file; tests/test_gpu_fim.py compares the GPU with it.
"""
import numpy as np

from encode_dropout_ref import M64
from mlm_ref import T, check_rows, d

FIM = (1 << 40) + 4
CUT_A = (1 << 40) + 5
CUT_B = (1 << 40) + 6
MODE = (1 << 40) + 7


def check_args(fim_rate, spm_rate, min_len):
    """The -1 cases of the header, as ValueError."""
    for q in (fim_rate, spm_rate):
        if not 0.0 <= float(q) <= 1.0:  # NaN fails both comparisons
            raise ValueError("a rate outside [0, 1]")
    if int(min_len) < 0:
        raise ValueError("min_len < 0")


def decide(r: int, L: int, *, fim_rate, spm_rate, seed, min_len=0, row_base=0):
    """-> (a, b, mode) of row r of length L, or (-1, -1, -1) when it is not transformed."""
    h = (row_base + r) & M64
    if L < min_len or not (d(seed, h, FIM) >> 32) < T(fim_rate):
        return -1, -1, -1
    x = (((d(seed, h, CUT_A) >> 32) * (L + 1)) & M64) >> 32
    y = (((d(seed, h, CUT_B) >> 32) * (L + 1)) & M64) >> 32
    return min(x, y), max(x, y), 1 if (d(seed, h, MODE) >> 32) < T(spm_rate) else 0


def check_cuts(cuts, lens):
    """The -8 case."""
    c = np.asarray(cuts, dtype=np.int64).reshape(-1, 3)
    if c.shape[0] != len(lens):
        raise ValueError("cuts must hold 3 entries per row")
    for (a, b, m), L in zip(c.tolist(), lens):
        if (a, b, m) == (-1, -1, -1):
            continue
        if not (0 <= a <= b <= L and m in (0, 1)):
            raise ValueError("bad cuts")
    return c.tolist()


def fim_ref(ids, row_off=None, *, pre_id, suf_id, mid_id, fim_rate=0.5, spm_rate=0.5, seed=0, min_len=0, row_base=0,
            cuts=None):
    """-> (out_ids int32, out_row_off int64, out_src int64, out_seg uint8, row_info int64 [rows, 3])."""
    ids = [int(v) for v in np.asarray(ids).reshape(-1)]
    n = len(ids)
    check_args(fim_rate, spm_rate, min_len)
    row = check_rows(row_off, n) if row_off is not None else [0, n]
    R = len(row) - 1
    lens = [row[r + 1] - row[r] for r in range(R)]
    given = None if cuts is None else check_cuts(cuts, lens)
    out, src, seg, off, info = [], [], [], [0], []
    for r in range(R):
        s, L = row[r], lens[r]
        a, b, m = given[r] if given is not None else decide(r, L, fim_rate=fim_rate, spm_rate=spm_rate, seed=seed,
                                                            min_len=min_len, row_base=row_base)
        info.append((a, b, m))
        if m < 0:
            parts = [(0, range(s, s + L))]
        else:
            pre, mid, suf = (1, range(s, s + a)), (3, range(s + a, s + b)), (2, range(s + b, s + L))
            parts = [pre_id, pre, suf_id, suf, mid_id, mid] if m == 0 else [pre_id, suf_id, suf, mid_id, pre, mid]
        for p in parts:
            if isinstance(p, tuple):
                out += [ids[k] for k in p[1]]
                src += list(p[1])
                seg += [p[0]] * len(p[1])
            else:
                out.append(p)
                src.append(-1)
                seg.append(4)
        off.append(len(out))
    return (np.array(out, dtype=np.int32), np.array(off, dtype=np.int64), np.array(src, dtype=np.int64),
            np.array(seg, dtype=np.uint8), np.array(info, dtype=np.int64).reshape(R, 3))


def snap(text, s: int, B: int, p: int) -> int:
    """p moved back to the first byte of its UTF-8 character: at most 3 steps, never from 0 or from B."""
    steps = 0
    while p > 0 and p < B and (text[s + p] & 0xC0) == 0x80 and steps < 3:
        p -= 1
        steps += 1
    return p


def fim_cuts_ref(text, doc_off=None, *, fim_rate=0.5, spm_rate=0.5, seed=0, min_len=0, row_base=0):
    """-> (piece_off int64 [3 docs + 1], doc_mode int8 [docs]) of shred_fim_cuts_device."""
    text = bytes(text)
    n = len(text)
    check_args(fim_rate, spm_rate, min_len)
    off = check_rows(doc_off, n) if doc_off is not None else [0, n]
    piece, mode = [], []
    for k in range(len(off) - 1):
        s, e = off[k], off[k + 1]
        B = e - s
        a, b, m = decide(k, B, fim_rate=fim_rate, spm_rate=spm_rate, seed=seed, min_len=min_len, row_base=row_base)
        if m < 0:
            piece += [s, e, e]
        else:
            a = snap(text, s, B, a)
            b = max(snap(text, s, B, b), a)
            piece += [s, s + a, s + b]
        mode.append(m)
    return np.array(piece + [n], dtype=np.int64), np.array(mode, dtype=np.int8)


def fim_chars_ref(encode, text, doc_off=None, *, pre_id, suf_id, mid_id, **draw):
    """encode_fim(level="char"): fim_ref assembling the pieces of fim_cuts_ref, each encoded alone by
    encode(bytes) -> ids.  -> (fim_ref's tuple, the ids before the transform, their row_off, the cuts)."""
    text = bytes(text)
    piece, mode = fim_cuts_ref(text, doc_off, **draw)
    ids, row3 = [], [0]
    for k in range(piece.size - 1):
        ids += [int(v) for v in encode(text[piece[k]:piece[k + 1]])]
        row3.append(len(ids))
    row3 = np.array(row3, dtype=np.int64)
    cuts = [(-1, -1, -1) if m < 0 else (int(row3[3 * k + 1] - row3[3 * k]), int(row3[3 * k + 2] - row3[3 * k]), int(m))
            for k, m in enumerate(mode)]
    ids = np.array(ids, dtype=np.int32)
    return (fim_ref(ids, row3[0::3], pre_id=pre_id, suf_id=suf_id, mid_id=mid_id, cuts=cuts or np.zeros((0, 3))),
            ids, row3[0::3], cuts)
