"""A Python reference for the masked-LM calls: the definitions of include/shredword_encode.h
(shred_mlm_*) restated literally, token by token.

    d(x, c) = mix(mix(seed + G (x + 1)) ^ c)      mix: fmix64, as for dropout
    T(q)    = int(q * 2^32)
    h(k)    = index_base + k                      per token
            = index_base + k'                     whole words: k' the last k' <= k at which a word begins
    selected(k)  iff  ids[k] is not protected and (d(h(k), SEL) >> 32) < T(p)
    a = d(index_base + k, ACT), v = a >> 32:  v < T(p_mask) -> mask_id;  v < T(p_mask) + T(p_random) ->
    ((a & 0xFFFFFFFF) * rand_vocab) >> 32;  else the id itself.

tests/test_mlm_ref_cpu.py pins this file; tests/test_gpu_mlm.py compares the GPU with it.
"""
import numpy as np

from encode_dropout_ref import GOLDEN_RATIO, M64, mix

SEL = 1 << 40
ACT = (1 << 40) + 1
MAX_PROTECT = 16
INT32_MAX = 2 ** 31 - 1


def d(seed: int, x: int, c: int) -> int:
    return mix(mix((seed + GOLDEN_RATIO * ((x + 1) & M64)) & M64) ^ c)


def T(q: float) -> int:
    return int(float(q) * 4294967296.0)


def token_len(lens, i: int) -> int:
    """Source bytes of id i: the table's, 1 for ids below 256, negative ids and ids past the table."""
    return int(lens[i]) if lens is not None and 256 <= i < len(lens) else 1


def check_args(p, p_mask, p_random, rand_vocab, protect, whole_word, starts):
    """The -1 cases of the header, as ValueError."""
    for q in (p, p_mask, p_random):
        if not 0.0 <= float(q) <= 1.0:  # NaN fails both comparisons
            raise ValueError("a probability outside [0, 1]")
    if T(p_mask) + T(p_random) > 2 ** 32:
        raise ValueError("T(p_mask) + T(p_random) > 2^32")
    if len(protect) > MAX_PROTECT:
        raise ValueError("too many protected ids")
    if float(p_random) > 0 and not 1 <= int(rand_vocab) <= INT32_MAX:
        raise ValueError("rand_vocab outside [1, INT32_MAX]")
    if whole_word and starts is None:
        raise ValueError("whole_word without starts")


def check_rows(row_off, n):
    """The -6 case."""
    row = [int(v) for v in row_off]
    if not row or row[0] != 0 or row[-1] != n or any(a > b for a, b in zip(row, row[1:])):
        raise ValueError("bad row_off")
    return row


def word_begins(ids, row_off, starts, lens, specials=(0, 0), protected=()) -> list:
    """begin[k] for every token: the header's rule, one token at a time.  specials: the ids [lo, hi) of
    the registered specials; protected: the ids that are units of their own (the protect list and, under
    protect_specials, nothing more than the specials, which begin words anyway)."""
    n = len(ids)
    firsts = {0}
    if row_off is not None:
        row = [int(v) for v in row_off]
        for r in range(len(row) - 1):
            if row[r] < row[r + 1]:
                firsts.add(row[r])
    lo, hi = specials
    is_special = lambda i: lo <= i < hi
    begin = []
    for k in range(n):
        if k == 0 or k in firsts:
            begin.append(True)
            continue
        cur, prev = int(ids[k]), int(ids[k - 1])
        if is_special(cur) or is_special(prev):
            begin.append(True)
        elif int(starts[k]) != int(starts[k - 1]) + token_len(lens, prev):
            begin.append(True)
        elif cur in protected or prev in protected:
            begin.append(True)
        else:
            begin.append(False)
    return begin


def mlm_ref(ids, row_off=None, *, p, seed, p_mask, p_random, mask_id, rand_vocab=0, protect=(), protect_specials=True,
            specials=(0, 0), whole_word=False, starts=None, lens=None, ignore_id=-100, index_base=0):
    """-> (out int32, labels int32, selected).  specials: the ids [lo, hi) of the registered specials."""
    ids = [int(v) for v in np.asarray(ids).reshape(-1)]
    n = len(ids)
    check_args(p, p_mask, p_random, rand_vocab, protect, whole_word, starts)
    if row_off is not None:
        check_rows(row_off, n)
    t_sel, t_mask, t_act = T(p), T(p_mask), T(p_mask) + T(p_random)
    listed = set(int(v) for v in protect)
    lo, hi = specials
    guarded = lambda i: i in listed or (protect_specials and lo <= i < hi)
    unit = list(range(n))
    if whole_word:
        begin = word_begins(ids, row_off, starts, lens, specials, listed)
        last = 0
        for k in range(n):
            if begin[k]:
                last = k
            unit[k] = last
    out, labels, selected = list(ids), [ignore_id] * n, 0
    for k in range(n):
        if guarded(ids[k]) or not (d(seed, (index_base + unit[k]) & M64, SEL) >> 32) < t_sel:
            continue
        selected += 1
        labels[k] = ids[k]
        a = d(seed, (index_base + k) & M64, ACT)
        v = a >> 32
        if v < t_mask:
            out[k] = mask_id
        elif v < t_act:
            out[k] = ((a & 0xFFFFFFFF) * int(rand_vocab)) >> 32
    return np.array(out, dtype=np.int32), np.array(labels, dtype=np.int32), selected
