"""GPU tests of the repeat calls (include/shredword_encode.h, shred_repeat_*): every case runs through both ABIs, host
rows and device tensors, and every output equals, bit for bit, the numpy restatement of the header below."""
import ctypes

import numpy as np
import pytest

import bad_offsets

pytestmark = pytest.mark.gpu

T = 2048  # ids of a row per workgroup
SMALL, MID = 256, 4096  # gram counts around which rows of one tile, of two or three, and of more are taken
U = np.uint64
ALL = U(2 ** 64 - 1)
NGRAM, MULT = U((1 << 40) + 12), U((1 << 40) + 13)


def _mix(x):
    x = (x ^ (x >> U(33))) * U(0xff51afd7ed558ccd)
    x = (x ^ (x >> U(33))) * U(0xc4ceb9fe1a85ec53)
    return x ^ (x >> U(33))


def _d(seed, x, c):
    return _mix(_mix(U(seed) + U(0x9E3779B97F4A7C15) * (np.asarray(x, dtype=U) + U(1))) ^ c)


def repeat_ref(ids, row, w, seed=0):
    """The header's definition -> (grams, distinct, repeated, covered, top_count, top_pos, tok_first, tok_cov, rows)."""
    t = np.asarray(ids, dtype=np.int32).astype(np.uint32).astype(U)
    n = t.size
    row = np.array([0, n]) if row is None else np.asarray(row, dtype=np.int64)
    R, cnt = len(row) - 1, max(n - w + 1, 0)
    with np.errstate(over="ignore"):
        g, A, S = _d(seed, t, NGRAM), _d(seed, w, MULT) | U(1), np.zeros(cnt, dtype=U)
        for j in range(w):
            S = S * A + g[j:j + cnt]
        F = _mix(S)
    F[F == ALL] = ALL - U(1)
    of = np.searchsorted(row, np.arange(n), side="right") - 1
    k = np.flatnonzero(np.arange(cnt) + w <= row[of[:cnt] + 1])
    cut = np.searchsorted(of[k], np.arange(R + 1))
    out = np.zeros((6, R), dtype=np.int64)
    out[5] = -1
    tok_first, edge = np.full(n, -1, dtype=np.int64), np.zeros(n + 65, dtype=np.int64)
    for r in np.flatnonzero(np.diff(cut)):
        kr = k[cut[r]:cut[r + 1]]
        u, idx, inv, c = np.unique(F[kr], return_index=True, return_inverse=True, return_counts=True)
        c = c[inv.reshape(-1)]
        tok_first[kr] = kr[idx][inv.reshape(-1)]
        out[:, r] = kr.size, u.size, (c >= 2).sum(), 0, c.max(), kr[np.argmax(c)]
        np.add.at(edge, kr[c >= 2], 1)
        np.add.at(edge, kr[c >= 2] + w, -1)
    tok_cov = np.cumsum(edge)[:n] > 0
    out[3] = np.bincount(of[tok_cov], minlength=R)
    return (*out, tok_first, tok_cov, int((out[2] > 0).sum()))


@pytest.fixture(scope="module")
def enc():
    from shredword.encoder import BPEEncoder
    e = BPEEncoder.from_merges(np.array([[97, 98, 256]], dtype=np.int32))
    yield e
    e.destroy()


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _same(got, want, why):
    assert got[8] == want[8], why
    for i, (g, x) in enumerate(zip(got[:8], want[:8])):
        g = g if isinstance(g, np.ndarray) else g.cpu().numpy()
        assert g.dtype == x.dtype and g.shape == x.shape and np.array_equal(g, x), (why, i)


def _both(e, ids, row=None, w=5, seed=0):
    """The call on host rows and on device tensors, with and without token outputs, against the reference; -> it."""
    ids = np.asarray(ids, dtype=np.int32)
    row = None if row is None else np.asarray(row, dtype=np.int64)
    want = repeat_ref(ids, row, w, seed)
    for dev in (False, True):
        put = _dev if dev else (lambda a: a)
        call = e.repeat_device if dev else e.repeat_rows
        got = call(put(ids), put(row), ngram=w, seed=seed, token_outputs=True)
        assert not dev or got[9] >= 0
        _same(got, want, (dev, w, ids.size))
        few = call(put(ids), put(row), ngram=w, seed=seed)
        assert few[6] is None and few[7] is None
        _same(few[:6] + want[6:8] + few[8:9], want, (dev, w, "no token outputs"))
    return want


_ids = lambda n, seed, vocab=50000: np.random.default_rng(seed).integers(0, vocab, size=n).astype(np.int32)
_offsets = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _edge_stream(w):
    """Rows of every size with empty rows between, ids from a vocabulary of the row's size, a run of w + 2 ids planted
    twice in every row that holds it, and in the longest row a gram copied across the edge of its first tile."""
    gs = [0, 1, 2, SMALL - 1, SMALL, SMALL + 1, MID, MID + 1, MID + 2 * T + 1]
    lens, parts = [], []
    for i, g in enumerate(gs):
        L = g + w - 1
        a = _ids(L, 100 * w + i, max(L, 2))
        if L >= 2 * w + 4:
            a[L // 2:L // 2 + w + 2] = a[:w + 2]
        if g > MID + T:
            a[T - (w + 1) // 2:T - (w + 1) // 2 + w] = a[40:40 + w]
        lens += [L, 0]
        parts.append(a)
    return np.concatenate(parts), _offsets(lens), gs


@pytest.mark.parametrize("w", [1, 2, 13, 64])
def test_row_sizes_and_tile_edges(enc, w):
    ids, row, gs = _edge_stream(w)
    want = _both(enc, ids, row, w, seed=w)
    assert want[0][::2].tolist() == gs
    for r in (2 * 3, 2 * 6, 2 * 8):                      # a row of one tile, of three, of five
        assert 0 < want[2][r] < want[0][r], r
    assert want[7][int(row[16]) + T - 1] and (w == 1 or want[7][int(row[16]) + T])   # both sides of the tile's edge


@pytest.mark.parametrize("g", [SMALL, MID, MID + T + 5])
def test_one_key_all_keys_and_rows_that_are_never_compared(enc, g):
    """A row of one id value, and a row of all-distinct grams stored twice as adjacent rows."""
    w = 5
    L = g + w - 1
    ids = np.concatenate([[7, 7, 7], np.full(L, 9), np.arange(L), np.arange(L)]).astype(np.int32)
    want = _both(enc, ids, _offsets([3, L, L, L]), w)
    assert [x[1:].tolist() for x in want[:6]] == [[g] * 3, [1, g, g], [g, 0, 0], [L, 0, 0], [g, 1, 1], [3, 3 + L, 3 + 2 * L]]


@pytest.mark.parametrize("L", [200, 3000, 9000])
def test_ties_go_to_the_first_gram_and_tok_first_is_a_stream_index(enc, L):
    w, start = 4, 500
    ids = _ids(start + L, L)
    A, B = np.array([1, 2, 3, 4]) + 60000, np.array([4, 3, 2, 1]) + 60000   # outside the random vocabulary
    at_a, at_b = [start + 9, start + L // 2, start + L - 4], [start + 30, start + 80, start + L - 20]
    for at, gram in ((at_a, A), (at_b, B)):
        for s in at:
            ids[s:s + w] = gram
    want = _both(enc, ids, [0, start, start + L], w)
    assert want[4].tolist() == [1, 3] and want[5].tolist() == [0, at_a[0]]
    assert want[6][at_a].tolist() == [at_a[0]] * 3 and want[6][at_b].tolist() == [at_b[0]] * 3


@pytest.mark.parametrize("w", [2, 13, 64])
@pytest.mark.parametrize("n", [3000, 3 * T])
def test_coverage_is_the_union(enc, w, n):
    """Repeated grams 1, w - 1, w and w + 1 positions apart; their copies lie apart, further on in the row."""
    ids = np.arange(n, dtype=np.int32)
    starts = 100 + np.cumsum([0, 1, w - 1, w, w + 1])
    for i, s in enumerate(starts):
        ids[2000 + i * (w + 1):2000 + i * (w + 1) + w] = np.arange(s, s + w)
    want = _both(enc, ids, [0, 0, n], w)
    assert want[2].tolist() == [0, 10] and want[3][1] == len({j for s in starts for j in range(s, s + w)}) + 5 * w


def test_many_short_rows(enc):
    row = _offsets(np.random.default_rng(12).integers(0, 41, size=5000))
    want = _both(enc, _ids(row[-1], 2, 50), row, 3)
    assert 0 < want[8] < 5000 and 0 < (want[3] > want[2]).sum()


def test_host_pieces(enc, monkeypatch):
    """SHREDWORD_BATCH_PIECE below the longest row (1500 ids) and the row count (60): the unpieced call's bytes."""
    lens = np.random.default_rng(61).integers(0, 40, size=55)
    row = _offsets(np.r_[0, lens[:6], 0, 0, lens[6:20], 1500, lens[20:], 0])
    ids = _ids(row[-1], 61, 30)
    for r in (row, None):
        monkeypatch.delenv("SHREDWORD_BATCH_PIECE", raising=False)
        want = _both(enc, ids, r, 3, seed=77)
        assert want[8] > 0 and (r is None or want[5].max() > 1500)
        for piece in ("1", "7", "999"):
            monkeypatch.setenv("SHREDWORD_BATCH_PIECE", piece)
            _same(enc.repeat_rows(ids, r, ngram=3, seed=77, token_outputs=True), want, piece)


def _raw(e, dev, ids, row, w=3, skip=None, rows=None):
    """The C ABI on host arrays (dev false) or tensors, each buffer one element into its allocation and so only
    element-aligned -> (the return value, the eight outputs as the call left them: preset to 7, untouched by an
    error).  skip: the output passed as NULL."""
    import torch
    from shredword.cbase import lib
    row, lead = np.asarray(row, dtype=np.int64), lambda a: np.concatenate([a[:1], a])
    tail = [ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(ctypes.c_double())] if dev else []
    out = [np.full(ids.size + 400, 7, dt) for dt in [np.int64] * 7 + [np.uint8]]
    bufs = [(_dev(lead(a)) if dev else lead(a))[1:] for a in (ids, row, *out)]
    ptr = [t.data_ptr() if dev else t.ctypes.data for t in bufs]
    outs = [None if i == skip else p for i, p in enumerate(ptr[2:])]
    code = (lib.shred_repeat_device if dev else lib.shred_repeat_rows)(
        e.enc, ptr[0], len(ids), ptr[1], len(row) - 1 if rows is None else rows, w, 1, *outs, *tail)
    got = [t.cpu().numpy() if dev else t for t in bufs[2:]]
    assert code >= 0 or all((g == 7).all() for g in got), row
    return code, got


@pytest.mark.parametrize("dev", [False, True])
def test_element_aligned_views_and_errors_that_write_nothing(enc, dev):
    n = T + 77
    ids, good = _ids(n, 11, 40), _offsets([3, 0, T - 1, 75])
    want = repeat_ref(ids, good, 3, 1)
    code, got = _raw(enc, dev, ids, good)
    assert code == want[8] > 0
    for g, x, size in zip(got, want, [4] * 6 + [n, n]):
        assert np.array_equal(g[:size], x) and (g[size:] == 7).all()
    for bad in ([0, 50, 40, n], [1, 50, n], [0, 50, n - 1], [0, -1, n], [0, 50, n + 1, n], *bad_offsets.at_256(n)):
        assert _raw(enc, dev, ids, bad)[0] == -6, bad
    assert _raw(enc, dev, ids, good, w=0)[0] == -1 and _raw(enc, dev, ids, good, w=65)[0] == -1
    assert _raw(enc, dev, ids, good, rows=2 ** 62)[0] == -1
    for skip in range(6):
        assert _raw(enc, dev, ids, good, skip=skip)[0] == -1, skip
    put = _dev if dev else (lambda a: a)
    call = enc.repeat_device if dev else enc.repeat_rows
    for a, r in [(ids.astype(np.int64), good), (ids, good.astype(np.int32)), (ids.astype(np.float32), None), (ids, good[:0])]:
        with pytest.raises(ValueError):
            call(put(a), put(r))
    for kw in (dict(ngram=0), dict(ngram=65)):
        with pytest.raises(ValueError):
            call(put(ids), **kw)
    with pytest.raises(ValueError):
        call(put(ids), put(np.array([0, 700, 600, n])))


def test_ordered_behind_a_producer_on_the_callers_stream(enc):
    """The ids are produced by a copy still pending on a non-default stream when the call is made."""
    import torch
    src, row = _ids(5 * T, 71, 30), _offsets([T + 5, 0, 4 * T - 205, 200])
    want = repeat_ref(src, row, 3, 3)
    d_src, d_row, s = _dev(src), _dev(row), torch.cuda.Stream()
    ids, big = torch.zeros(src.size, dtype=torch.int32, device="cuda"), torch.ones(1 << 26, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(8):
            big = big * 1.0001 + 0.5   # keeps the stream busy
        ids.copy_(d_src)               # the producer, queued behind it
        got = enc.repeat_device(ids, d_row, ngram=3, seed=3, token_outputs=True, stream=s.cuda_stream)
    s.synchronize()
    assert want[8] >= 2
    _same(got, want, "stream")


def test_encode_repeats(enc):
    docs = [b"ab abab c ab ab", b"", b"abab ab c c c ab abab ab", b"c"]
    ids, row = enc.encode_batch(docs)[:2]
    got = enc.encode_repeats(docs, ngram=2, seed=4, token_outputs=True)
    assert np.array_equal(got[0], ids) and np.array_equal(got[1], row)
    want = enc.repeat_rows(ids, row, ngram=2, seed=4, token_outputs=True)
    _same(got[2:], want, "encode_repeats")
    assert want[8] == 2 and want[0].tolist() == [max(d - 1, 0) for d in np.diff(row)]
    assert enc.encode_repeats(b" ".join(docs), ngram=2)[8:10] == (None, None)
