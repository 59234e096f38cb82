"""A Python reference for the span-corruption calls: the definitions of include/shredword_encode.h
(shred_corrupt_*) restated literally, token by token.

    d(x, c)  = mix(mix(seed + G (x + 1)) ^ c)       as for masked-LM; START = 2^40 + 2, LEN = 2^40 + 3
    h        = index_base + k
    start(k) iff (d(h, START) >> 32) < T(p_start)
    L(k)     = 1 + #{ i in [1, len_n) : v >= C_i },  v = d(h, LEN) >> 32
    reach(k) = min(k + L(k), end of k's row)
    noise(j) iff j is not guarded and some start k has k <= j < reach(k)
    runs: maximal sequences of consecutive noise tokens of a row, ranked 0, 1, ..; those of rank >= Rmax
    = max(sentinel_n - (final_sentinel != 0), 0) are kept.
    input row:  the tokens, each corrupted run replaced by S_rank = sentinel_first + rank * sentinel_step
    target row: S_rank and the run, for every corrupted run; S_J at the end (final_sentinel, sentinel_n > 0)

It takes the len_cum list of the C ABI, so no float differs between the reference and the library.
tests/test_corrupt_ref_cpu.py pins this file; tests/test_gpu_corrupt.py compares the GPU with it.
"""
import numpy as np

from encode_dropout_ref import GOLDEN_RATIO, M64, mix  # noqa: F401  (the definitions' names)
from mlm_ref import MAX_PROTECT, T, check_rows, d

START = (1 << 40) + 2
LEN = (1 << 40) + 3
MAX_SPAN = 32
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def uniform_cum(lo: int, hi: int) -> list:
    """C_1 .. C_hi of a length uniform on lo .. hi: 0 below lo, then equal steps up to 2^32."""
    k = hi - lo + 1
    return [0 if i < lo else ((i - lo + 1) << 32) // k for i in range(1, hi + 1)]


def check_args(p_start, len_cum, sentinel_first, sentinel_step, sentinel_n, protect):
    """The -1 cases of the header, as ValueError."""
    if not 0.0 <= float(p_start) <= 1.0:  # NaN fails both comparisons
        raise ValueError("p_start outside [0, 1]")
    cum = [int(v) for v in len_cum]
    if not 1 <= len(cum) <= MAX_SPAN:
        raise ValueError("len_n outside [1, 32]")
    if any(a > b for a, b in zip(cum, cum[1:])) or cum[0] < 0 or cum[-1] != 1 << 32:
        raise ValueError("len_cum must not decrease and must end at 2^32")
    if sentinel_n < 0:
        raise ValueError("sentinel_n < 0")
    if sentinel_n > 0 and not INT32_MIN <= sentinel_first + (sentinel_n - 1) * sentinel_step <= INT32_MAX:
        raise ValueError("the last sentinel leaves int32")
    if len(protect) > MAX_PROTECT:
        raise ValueError("too many protected ids")


def noise_of(ids, row, *, p_start, len_cum, seed, index_base=0, protect=(), protect_specials=True, specials=(0, 0)):
    """noise[j] for every token, by the header's rule: every start marks its reach, guarded tokens are exempt."""
    n = len(ids)
    cum = [int(v) for v in len_cum]
    listed = set(int(v) for v in protect)
    lo, hi = specials
    guarded = lambda i: i in listed or (bool(protect_specials) and lo <= i < hi)
    t_start = T(p_start)
    covered = [False] * n
    for r in range(len(row) - 1):
        for k in range(row[r], row[r + 1]):
            h = (index_base + k) & M64
            if not (d(seed, h, START) >> 32) < t_start:
                continue
            v = d(seed, h, LEN) >> 32
            L = 1 + sum(1 for i in range(1, len(cum)) if v >= cum[i - 1])
            for j in range(k, min(k + L, row[r + 1])):
                covered[j] = True
    return [covered[j] and not guarded(int(ids[j])) for j in range(n)]


def corrupt_ref(ids, row_off=None, *, p_start, len_cum, seed=0, sentinel_first, sentinel_step=-1, sentinel_n=100,
                final_sentinel=True, protect=(), protect_specials=True, specials=(0, 0), index_base=0):
    """-> (in_ids int32, in_row_off int64, tgt_ids int32, tgt_row_off int64, in_src int64).  specials: the ids
    [lo, hi) of the registered specials."""
    ids = [int(v) for v in np.asarray(ids).reshape(-1)]
    n = len(ids)
    check_args(p_start, len_cum, sentinel_first, sentinel_step, sentinel_n, protect)
    row = check_rows(row_off, n) if row_off is not None else [0, n]
    noise = noise_of(ids, row, p_start=p_start, len_cum=len_cum, seed=seed, index_base=index_base, protect=protect,
                     protect_specials=protect_specials, specials=specials)
    fin = bool(final_sentinel)
    rmax = max(sentinel_n - int(fin), 0)
    S = lambda j: sentinel_first + j * sentinel_step
    in_ids, in_src, tgt_ids, in_row, tgt_row = [], [], [], [0], [0]
    for r in range(len(row) - 1):
        rank = -1  # of the run the walk is in, or of the last one it left
        prev = False
        for j in range(row[r], row[r + 1]):
            first = noise[j] and not prev
            prev = noise[j]
            if first:
                rank += 1
            if noise[j] and rank < rmax:
                if first:
                    in_ids.append(S(rank))
                    in_src.append(j)
                    tgt_ids.append(S(rank))
                tgt_ids.append(ids[j])
            else:
                in_ids.append(ids[j])
                in_src.append(j)
        if fin and sentinel_n > 0:
            tgt_ids.append(S(min(rank + 1, rmax)))
        in_row.append(len(in_ids))
        tgt_row.append(len(tgt_ids))
    return (np.array(in_ids, dtype=np.int32), np.array(in_row, dtype=np.int64), np.array(tgt_ids, dtype=np.int32),
            np.array(tgt_row, dtype=np.int64), np.array(in_src, dtype=np.int64))
