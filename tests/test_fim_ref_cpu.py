"""Pins tests/fim_ref.py, the reference of the fill-in-the-middle calls: hand-written rows through
explicit cuts, the draw formulas against direct evaluation, the rates and min_len, row_base shifting,
UTF-8 snapping of the character-level cuts, and the permutation undone through out_src.
"""
import numpy as np
import pytest

from encode_dropout_ref import GOLDEN_RATIO, M64, mix
from fim_ref import CUT_A, CUT_B, FIM, MODE, check_args, decide, fim_chars_ref, fim_cuts_ref, fim_ref, snap

P, S, M = 901, 902, 903
SENT = dict(pre_id=P, suf_id=S, mid_id=M)
NO = (-1, -1, -1)


def run(ids, row=None, **kw):
    return [a.tolist() for a in fim_ref(np.array(ids, dtype=np.int32), row, **SENT, **kw)]


def test_constants():
    assert (FIM, CUT_A, CUT_B, MODE) == tuple((1 << 40) + k for k in (4, 5, 6, 7))


def test_hand_written_rows_in_both_modes():
    ids = [10, 11, 12, 13, 14]
    out, off, src, seg, info = run(ids, cuts=[(2, 3, 0)])
    assert out == [P, 10, 11, S, 13, 14, M, 12] and off == [0, 8]
    assert src == [-1, 0, 1, -1, 3, 4, -1, 2] and seg == [4, 1, 1, 4, 2, 2, 4, 3] and info == [[2, 3, 0]]
    out, off, src, seg, info = run(ids, cuts=[(2, 3, 1)])
    assert out == [P, S, 13, 14, M, 10, 11, 12] and off == [0, 8]
    assert src == [-1, -1, 3, 4, -1, 0, 1, 2] and seg == [4, 4, 2, 2, 4, 1, 1, 3] and info == [[2, 3, 1]]


def test_hand_written_edges():
    ids = [10, 11, 12]
    assert run(ids, cuts=[(0, 2, 0)])[0] == [P, S, 12, M, 10, 11]            # a = 0: no prefix
    assert run(ids, cuts=[(0, 2, 1)])[0] == [P, S, 12, M, 10, 11]
    assert run(ids, cuts=[(1, 1, 0)])[0] == [P, 10, S, 11, 12, M]            # a = b: no middle
    assert run(ids, cuts=[(1, 1, 1)])[0] == [P, S, 11, 12, M, 10]
    assert run(ids, cuts=[(1, 3, 0)])[0] == [P, 10, S, M, 11, 12]            # b = L: no suffix
    assert run(ids, cuts=[(1, 3, 1)])[0] == [P, S, M, 10, 11, 12]
    assert run(ids, cuts=[(0, 0, 0)])[0] == [P, S, 10, 11, 12, M]
    assert run(ids, cuts=[(3, 3, 0)])[0] == [P, 10, 11, 12, S, M]
    assert run(ids, cuts=[(0, 3, 1)])[3] == [4, 4, 4, 3, 3, 3]
    for m in (0, 1):                                                         # L = 0: the three sentinels
        out, off, src, seg, info = run([], cuts=[(0, 0, m)])
        assert out == [P, S, M] and off == [0, 3] and src == [-1] * 3 and seg == [4] * 3 and info == [[0, 0, m]]
    assert run([], cuts=[NO]) == [[], [0, 0], [], [], [list(NO)]]


def test_an_untransformed_row_between_two_transformed_ones():
    ids = [10, 11, 20, 21, 22, 30]
    out, off, src, seg, info = run(ids, [0, 2, 5, 5, 6], cuts=[(1, 1, 0), NO, (0, 0, 1), (0, 1, 0)])
    assert out == [P, 10, S, 11, M] + [20, 21, 22] + [P, S, M] + [P, S, M, 30]
    assert off == [0, 5, 8, 11, 15]
    assert src == [-1, 0, -1, 1, -1, 2, 3, 4, -1, -1, -1, -1, -1, -1, 5]
    assert seg == [4, 1, 4, 2, 4, 0, 0, 0, 4, 4, 4, 4, 4, 4, 3]
    assert info == [[1, 1, 0], list(NO), [0, 0, 1], [0, 1, 0]]


def test_bad_arguments():
    for bad in ([(2, 1, 0)], [(0, 4, 0)], [(0, 1, 2)], [(-1, -1, 0)], [(-1, 1, 0)], [(0, 1, -1)]):
        with pytest.raises(ValueError):
            run([1, 2, 3], cuts=bad)
    with pytest.raises(ValueError):
        run([1, 2, 3], [0, 2, 1, 3])
    for bad in (dict(fim_rate=float("nan")), dict(spm_rate=1.5), dict(fim_rate=-0.1), dict(min_len=-1)):
        with pytest.raises(ValueError):
            check_args(**dict(dict(fim_rate=0.5, spm_rate=0.5, min_len=0), **bad))


def hash_(seed, x, c):
    """d(x, c) written out once more, not imported."""
    return mix(mix((seed + GOLDEN_RATIO * (x + 1)) & M64) ^ c)


def test_draws_against_direct_evaluation():
    seen = set()
    for seed, base in ((0, 0), (7, 1 << 40), (2 ** 64 - 1, (1 << 63) + 5)):
        for r, L in enumerate([0, 1, 2, 7, 100, 5000, 1 << 20] * 6):
            h = (base + r) & M64
            on = (hash_(seed, h, (1 << 40) + 4) >> 32) < int(0.6 * 2 ** 32)
            x = ((hash_(seed, h, (1 << 40) + 5) >> 32) * (L + 1)) >> 32
            y = ((hash_(seed, h, (1 << 40) + 6) >> 32) * (L + 1)) >> 32
            m = 1 if (hash_(seed, h, (1 << 40) + 7) >> 32) < int(0.3 * 2 ** 32) else 0
            want = (min(x, y), max(x, y), m) if on else NO
            assert decide(r, L, fim_rate=0.6, spm_rate=0.3, seed=seed, row_base=base) == want
            assert want == NO or 0 <= want[0] <= want[1] <= L
            seen.add(want[2])
    assert seen == {-1, 0, 1}


def _random_rows(seed, rows=300, longest=9):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, longest + 1, size=rows)
    row = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rng.integers(0, 500, size=int(row[-1])).astype(np.int32), row


def test_rates_and_min_len():
    ids, row = _random_rows(1)
    R = row.size - 1
    out, off, src, seg, info = fim_ref(ids, row, **SENT, fim_rate=0.0, seed=3)
    assert np.array_equal(out, ids) and np.array_equal(off, row) and (info == -1).all() and (seg == 0).all()
    assert np.array_equal(src, np.arange(ids.size))
    out, off, src, seg, info = fim_ref(ids, row, **SENT, fim_rate=1.0, seed=3)
    assert out.size == ids.size + 3 * R and (info[:, 2] >= 0).all() and np.array_equal(np.diff(off), np.diff(row) + 3)
    assert set(info[:, 2].tolist()) == {0, 1}
    assert (fim_ref(ids, row, **SENT, fim_rate=1.0, spm_rate=0.0, seed=3)[4][:, 2] == 0).all()
    assert (fim_ref(ids, row, **SENT, fim_rate=1.0, spm_rate=1.0, seed=3)[4][:, 2] == 1).all()
    info = fim_ref(ids, row, **SENT, fim_rate=1.0, min_len=4, seed=3)[4]
    assert np.array_equal(info[:, 2] >= 0, np.diff(row) >= 4) and (np.diff(row) < 4).any()
    half = fim_ref(ids, row, **SENT, seed=3)[4][:, 2]
    assert 0.35 * R < (half >= 0).sum() < 0.65 * R


def test_row_base_shifts_the_rows():
    ids, row = _random_rows(2)
    kw = dict(SENT, seed=11, row_base=(1 << 63) + 77)
    whole = fim_ref(ids, row, **kw)
    for k in (1, 57, 299):
        cut = int(row[k])
        tail = fim_ref(ids[cut:], row[k:] - cut, **dict(kw, row_base=kw["row_base"] + k))
        assert np.array_equal(tail[0], whole[0][whole[1][k]:]) and np.array_equal(tail[4], whole[4][k:])
        assert np.array_equal(tail[2][tail[2] >= 0] + cut, whole[2][whole[1][k]:][tail[2] >= 0])
    assert not np.array_equal(whole[4], fim_ref(ids, row, **dict(kw, seed=12))[4])
    # a row alone is its own call: None as row_off is one row
    one = fim_ref(ids[:5], None, **kw)
    assert np.array_equal(one[0], fim_ref(ids[:5], [0, 5], **kw)[0]) and one[1].tolist()[0] == 0


def test_out_src_undoes_the_permutation():
    ids, row = _random_rows(3)
    out, off, src, seg, info = fim_ref(ids, row, **SENT, seed=5)
    keep = src >= 0
    assert np.array_equal(np.sort(src[keep]), np.arange(ids.size)) and np.array_equal(out[keep], ids[src[keep]])
    assert (seg[~keep] == 4).all() and (seg[keep] != 4).all()
    back = np.empty_like(ids)
    back[src[keep]] = out[keep]
    assert np.array_equal(back, ids)
    for r in range(row.size - 1):
        a, b, m = info[r]
        s = src[off[r]:off[r + 1]]
        g = seg[off[r]:off[r + 1]]
        if m < 0:
            assert (g == 0).all()
            continue
        assert (g == 1).sum() == a and (g == 3).sum() == b - a and (g == 2).sum() == row[r + 1] - row[r] - b
        assert g[-1] == (3 if b > a else 1 if m == 1 and a > 0 else 4) and g[0] == 4
        mid = s[g == 3]
        assert np.array_equal(mid, np.arange(row[r] + a, row[r] + b))


def test_snapping():
    two, three, four = "é".encode(), "€".encode(), "😀".encode()
    for ch in (two, three, four):
        t = b"a" + ch + b"b"
        B = len(t)
        for p in range(B + 1):
            want = 1 if 1 < p < 1 + len(ch) else p
            assert snap(t, 0, B, p) == want, (ch, p)
        assert snap(b"xx" + t, 2, B, 2) == 1                     # s is added to the index, not to the result
    run5 = b"a" + b"\x80" * 5 + b"b"
    assert [snap(run5, 0, 7, p) for p in range(8)] == [0, 0, 0, 0, 1, 2, 6, 7]   # at most 3 steps back
    only = b"\x80\x80"
    assert [snap(only, 0, 2, p) for p in range(3)] == [0, 0, 2]   # never from 0, never from B
    assert snap(two, 0, 2, 2) == 2 and snap(two + two, 0, 2, 2) == 2   # a == B is left alone


def test_character_cuts():
    docs = ["naïve café".encode(), b"", "€€€€".encode(), b"\x80\x80\x80", b"plain ascii text", "😀😀".encode()] * 20
    text = b"".join(docs)
    off = np.concatenate([[0], np.cumsum([len(x) for x in docs])])
    kw = dict(fim_rate=0.8, spm_rate=0.5, seed=9, row_base=3)
    piece, mode = fim_cuts_ref(text, off, **kw)
    assert piece.size == 3 * len(docs) + 1 and piece[-1] == len(text) and (np.diff(piece) >= 0).all()
    assert set(mode.tolist()) == {-1, 0, 1}
    moved = 0
    for k, doc in enumerate(docs):
        s, pa, pb = (int(v) for v in piece[3 * k:3 * k + 3])
        e = int(off[k + 1])
        assert s == off[k]
        a, b, m = decide(k, len(doc), **kw)
        assert m == mode[k]
        if m < 0:
            assert (pa, pb) == (e, e)
            continue
        assert s <= pa <= pb <= e and pa - s <= a and pb - s <= max(b, pa - s)
        moved += (pa - s != a) + (pb - s != b)
        if doc != b"\x80\x80\x80":
            for part in (doc[:pa - s], doc[pa - s:pb - s], doc[pb - s:]):
                part.decode("utf-8")                              # every piece is whole characters
    assert moved >= 5
    one = fim_cuts_ref(docs[0], None, **dict(kw, fim_rate=1.0))
    assert one[0].size == 4 and one[0][0] == 0 and one[0][-1] == len(docs[0])
    assert (fim_cuts_ref(text, off, **dict(kw, fim_rate=1.0, min_len=5))[1] >= 0).tolist() == [len(x) >= 5 for x in docs]


def test_character_level_rows_join_the_pieces():
    enc = lambda b: list(b)                                       # a byte-level tokenizer
    docs = [b"hello world", b"", b"abc"]
    text, off = b"".join(docs), [0, 11, 11, 14]
    (out, row, src, seg, info), ids, row_in, cuts = fim_chars_ref(enc, text, off, **SENT, fim_rate=1.0, seed=2)
    assert ids.tolist() == list(text) and row_in.tolist() == off
    piece, mode = fim_cuts_ref(text, off, fim_rate=1.0, seed=2)
    for k in range(3):
        a, b = int(piece[3 * k + 1] - piece[3 * k]), int(piece[3 * k + 2] - piece[3 * k])
        assert tuple(info[k]) == (a, b, mode[k]) == cuts[k]
    assert out.size == len(text) + 9 and np.array_equal(out[src >= 0], ids[src[src >= 0]])
