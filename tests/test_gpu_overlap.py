"""GPU tests of the overlap calls (include/shredword_encode.h, shred_overlap_*): every case runs through both ABIs,
host rows and device tensors, and every output equals, bit for bit, the numpy restatement of the header below."""
import ctypes

import numpy as np
import pytest

import bad_offsets

pytestmark = pytest.mark.gpu

T = 2048  # shredword.encoder.OVERLAP_TILE, checked in test_tile_edges
U = np.uint64
ALL = U(2 ** 64 - 1)
NGRAM, MULT = U((1 << 40) + 12), U((1 << 40) + 13)


def _mix(x):
    x = (x ^ (x >> U(33))) * U(0xff51afd7ed558ccd)
    x = (x ^ (x >> U(33))) * U(0xc4ceb9fe1a85ec53)
    return x ^ (x >> U(33))


def _d(seed, x, c):
    return _mix(_mix(U(seed) + U(0x9E3779B97F4A7C15) * (np.asarray(x, dtype=U) + U(1))) ^ c)


def _grams(ids, row, w, seed):
    """-> (the positions whose gram exists, their fingerprints, the row of every token)."""
    t = np.asarray(ids, dtype=np.int32).astype(np.uint32).astype(U)
    row = np.array([0, t.size]) if row is None else np.asarray(row, dtype=np.int64)
    cnt = max(t.size - w + 1, 0)
    with np.errstate(over="ignore"):
        g, A, S = _d(seed, t, NGRAM), _d(seed, w, MULT) | U(1), np.zeros(cnt, dtype=U)
        for j in range(w):
            S = S * A + g[j:j + cnt]
        F = _mix(S)
    F[F == ALL] = ALL - U(1)
    of = np.searchsorted(row, np.arange(t.size), side="right") - 1
    k = np.flatnonzero(np.arange(cnt) + w <= row[of[:cnt] + 1])
    return k, F[k], of


def overlap_ref(ref, ids, row=None):
    """The header's definition -> (hits, covered, first, tok_ref, tok_cov, rows_hit); ref: (ids, row, w, seed) or None."""
    n = len(ids)
    R = 1 if row is None else len(row) - 1
    tok_ref, edge = np.full(n, -1, dtype=np.int64), np.zeros(n + 65, dtype=np.int64)
    w = ref[2] if ref else 1
    k, F, of = _grams(ids, row, w, ref[3] if ref else 0)
    if ref:
        pos, keys, _ = _grams(*ref)
        uniq, at = np.unique(keys, return_index=True)
        hit = np.isin(F, uniq)
        tok_ref[k[hit]] = pos[at[np.searchsorted(uniq, F[hit])]]
    at = np.flatnonzero(tok_ref >= 0)
    np.add.at(edge, at, 1)
    np.add.at(edge, at + w, -1)
    tok_cov = np.cumsum(edge)[:n] > 0
    first = np.full(R, -1, dtype=np.int64)
    first[of[at][::-1]] = at[::-1]
    hits = np.bincount(of[at], minlength=R).astype(np.int64)
    return hits, np.bincount(of[tok_cov], minlength=R).astype(np.int64), first, tok_ref, tok_cov, int((hits > 0).sum())


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
    assert got[5] == want[5], why
    for g, x in zip(got[:5], want[:5]):
        g = g if isinstance(g, np.ndarray) else g.cpu().numpy()
        assert g.dtype == x.dtype and g.shape == x.shape and np.array_equal(g, x), why


def _both(e, ref, ids, row=None, register=True):
    """The set ref = (ids, row, w, seed) registered (unless it is the one in place; None: no set) and the corpus call
    made, on host rows and on device tensors, both compared with the reference; -> the reference's."""
    ids = np.asarray(ids, dtype=np.int32)
    row = None if row is None else np.asarray(row, dtype=np.int64)
    if ref is not None:
        ref = (np.asarray(ref[0], dtype=np.int32), None if ref[1] is None else np.asarray(ref[1], dtype=np.int64), *ref[2:])
    want, w = overlap_ref(ref, ids, row), ref[2] if ref else 1
    for dev in (False, True):
        put = _dev if dev else (lambda a: a)
        if ref is not None and register:
            grams = e.set_overlap_refs(put(ref[0]), put(ref[1]), ngram=w, seed=ref[3])
            st = e.overlap_stats()
            assert grams == st["ref_grams"] == _grams(*ref)[0].size and st["distinct"] == np.unique(_grams(*ref)[1]).size
            assert st["table_bytes"] >= 24 * ref[0].size
        got = (e.overlap_device if dev else e.overlap_rows)(put(ids), put(row), token_outputs=True)
        assert not dev or got[6] >= 0
        _same(got, want, (dev, w, ids.size))
        few = (e.overlap_device if dev else e.overlap_rows)(put(ids), put(row))
        assert few[3] is None and few[4] is None
        _same(few[:3] + want[3:5] + few[5:6], want, (dev, w, "no token outputs"))
    return want


_ids = lambda n, seed, vocab=50000: np.random.default_rng(seed).integers(0, vocab, size=n).astype(np.int32)
_offsets = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _rows_of(ids, starts, w):
    """A reference set of the grams of ids at `starts`, one row each."""
    return np.concatenate([ids[s:s + w] for s in starts] + [ids[:0]]), _offsets([w] * len(starts)), w


@pytest.mark.parametrize("w", [1, 2, 13, 64])
def test_tile_edges(enc, w):
    """Grams that straddle a tile's edge, and coverage that reaches the next tile from the halo."""
    from shredword.encoder import OVERLAP_TILE
    assert T == OVERLAP_TILE
    for n in (T - 1, T, T + 1, T + w - 2, T + w - 1, 2 * T + 1):
        ids = _ids(n, n + w)
        starts = [s for s in (T - w, T - w + 1, T - 1, T, n - w) if s + w <= n]   # (n - w: the stream's last gram)
        want = _both(enc, (*_rows_of(ids, starts, w), w), ids)
        assert want[0][0] >= len(set(starts)) > 0


@pytest.mark.parametrize("w", [1, 2, 13, 64])
def test_row_edges(enc, w):
    """Rows around w among long ones, a row that ends at T, and grams across a row boundary on either side."""
    lens = [0, w - 1, w, w + 1, 0, 0, 700, w, 0, 0]
    lens += [T - sum(lens), 0, 3 * w, w - 1, 900, 0]
    row = _offsets(lens)
    ids = _ids(row[-1], w)
    inside, across = int(row[6]) + 5, int(row[7]) - 1           # in the row of 700; over its end
    ref_ids = np.concatenate([ids[inside:inside + w], ids[across:across + w], ids[row[14] + 9:row[14] + 9 + w], ids[T - w:T]])
    split = [w, w, w // 2, w - w // 2, w]                       # the third gram lies across two reference rows
    want = _both(enc, (ref_ids, _offsets(split), w, 5), ids, row)
    hit = set(np.flatnonzero(want[0]).tolist())                # (w == 1: ids, which may also occur elsewhere)
    assert hit == {6, 10} and want[0][[6, 10]].tolist() == [1, 1] if w > 1 else {6, 10, 14} <= hit


@pytest.mark.parametrize("w", [2, 13, 64])
def test_coverage_is_the_union(enc, w):
    ids = np.arange(3 * T, dtype=np.int32)
    starts = 100 + np.cumsum([0, 1, w - 1, w, w + 1])
    want = _both(enc, (*_rows_of(ids, starts, w), 1), ids, [0, 0, 3 * T])
    assert want[0].tolist() == [0, 5] and want[1][1] == len({j for s in starts for j in range(s, s + w)})
    same = np.full(3 * T, 9, dtype=np.int32)                    # one row takes counts from every tile
    want = _both(enc, (same[:w], None, w, 1), same, [0, 3 * T, 3 * T])
    assert want[0].tolist() == [3 * T - w + 1, 0] and want[1].tolist() == [3 * T, 0] and want[2].tolist() == [0, -1]


def test_tok_ref_is_the_smallest_position_and_first_the_first_hit(enc):
    gram, ids = np.arange(7, dtype=np.int32), _ids(3000, 8)
    ids[1000:1007] = ids[2000:2007] = ids[2990:2997] = gram
    ref = np.concatenate([[5, 5], gram, [6], gram, gram]).astype(np.int32)
    want = _both(enc, (ref, [0, 17, 24], 7, 2), ids, [0, 500, 1500, 1500, 3000])
    assert want[2].tolist() == [-1, 1000, -1, 2000] and want[3][[1000, 2000, 2990]].tolist() == [2, 2, 2]
    assert want[0].tolist() == [0, 1, 0, 2]


def test_many_short_rows(enc):
    rng = np.random.default_rng(12)
    row, ref_row = _offsets(rng.integers(0, 41, size=5000)), _offsets(rng.integers(0, 41, size=30))
    want = _both(enc, (_ids(ref_row[-1], 1, 50), ref_row, 3, 0), _ids(row[-1], 2, 50), row)
    assert 0 < want[5] < 5000 and 0 < (want[1] > want[0]).sum()


def test_reference_set_replaced_cleared_and_never_set():
    from shredword.encoder import BPEEncoder
    ids, row = _ids(T + 100, 4, 20), _offsets([T - 1, 0, 101])
    with BPEEncoder.from_merges(np.array([[97, 98, 256]], dtype=np.int32)) as e:
        assert _both(e, None, ids, row)[5] == 0 and e.overlap_stats()["table_bytes"] == 0     # never set
        assert _both(e, (ids[5:300], None, 2, 1), ids, row)[5] == 2
        assert _both(e, (ids[40:44], [0, 1, 4], 3, 9), ids, row)[0].sum() > 0                # the second set only
        for dev in (False, True):
            assert e.set_overlap_refs(_dev(ids[:0]) if dev else ids[:0]) == 0                # cleared
            assert _both(e, None, ids, row)[5] == 0 and e.overlap_stats() == dict(table_bytes=0, ref_grams=0, distinct=0)
            assert _both(e, (ids[:50], None, 2, 0), ids, row)[5] > 0


def test_host_pieces(enc, monkeypatch):
    """SHREDWORD_BATCH_PIECE below the longest row (1500 ids) and the row count (60): the unpieced call's bytes."""
    lens = np.random.default_rng(61).integers(0, 40, size=55)
    row = _offsets(np.r_[0, lens[:6], 0, 0, lens[6:20], 1500, lens[20:], 0])
    ids = _ids(row[-1], 61, 30)
    for r in (row, None):
        monkeypatch.delenv("SHREDWORD_BATCH_PIECE", raising=False)
        want = _both(enc, (_ids(400, 62, 30), [0, 100, 400], 3, 77), ids, r)
        assert want[5] > 0 and (r is None or want[2].max() > 1500)
        for piece in ("1", "7", "999"):
            monkeypatch.setenv("SHREDWORD_BATCH_PIECE", piece)
            _same(enc.overlap_rows(ids, r, token_outputs=True), want, piece)


def _raw(e, dev, ids, row, refs=None, hits=True, rows=None):
    """The C ABI on host arrays (dev false) or tensors, each buffer one element into its allocation and so only
    element-aligned.  refs = (ids, row, w): the reference call -> its return value.  Else the corpus call -> (the
    return value, the five outputs as the call left them: preset to 7, untouched by an error)."""
    import torch
    from shredword.cbase import lib
    row, lead = np.asarray(row, dtype=np.int64), lambda a: np.concatenate([a[:1], a])
    tail = [ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(ctypes.c_double())] if dev else []
    if refs is not None:
        bufs = [(_dev(lead(a)) if dev else lead(a))[1:] for a in (refs[0], np.asarray(refs[1], dtype=np.int64))]
        ptr = [t.data_ptr() if dev else t.ctypes.data for t in bufs]
        return (lib.shred_overlap_refs_device if dev else lib.shred_overlap_refs)(
            e.enc, ptr[0], len(refs[0]), ptr[1], len(refs[1]) - 1, refs[2], 1, *tail)
    out = [np.full(ids.size + 400, 7, dt) for dt in (np.int64, np.int64, np.int64, np.int64, np.uint8)]
    bufs = [(_dev(lead(a)) if dev else lead(a))[1:] for a in (ids, row, *out)]
    ptr = [t.data_ptr() if dev else t.ctypes.data for t in bufs]
    code = (lib.shred_overlap_device if dev else lib.shred_overlap_rows)(
        e.enc, ptr[0], len(ids), ptr[1], len(row) - 1 if rows is None else rows, ptr[2] if hits else None, *ptr[3:], *tail)
    got = [t.cpu().numpy() if dev else t for t in bufs[2:]]
    assert code >= 0 or all((g == 7).all() for g in got), row
    return code, got


@pytest.mark.parametrize("dev", [False, True])
def test_element_aligned_views_and_errors_that_write_nothing(enc, dev):
    n = T + 77
    ids, good = _ids(n, 11, 40), _offsets([3, 0, T - 1, 75])
    ref = (_ids(300, 12, 40), [0, 2, 150, 300], 3)
    assert _raw(enc, dev, ids, good, refs=ref) == _grams(*ref, 1)[0].size
    want = overlap_ref((*ref, 1), ids, good)

    def check():
        code, got = _raw(enc, dev, ids, good)
        assert code == want[5] > 0
        for g, x, size in zip(got, want, (4, 4, 4, n, n)):
            assert np.array_equal(g[:size], x) and (g[size:] == 7).all()
    check()
    for bad in ([0, 50, 40, n], [1, 50, n], [0, 50, n - 1], [0, -1, n], [0, 50, n + 1, n], *bad_offsets.at_256(n)):
        assert _raw(enc, dev, ids, bad)[0] == -6, bad
    assert _raw(enc, dev, ids, good, hits=False)[0] == -1 and _raw(enc, dev, ids, good, rows=2 ** 62)[0] == -1
    for w in (0, 65):                                          # refused, and the set stays
        assert _raw(enc, dev, ids, good, refs=(ref[0], ref[1], w)) == -1
    for bad in ([0, 200, 100, 300], [0, 299], *bad_offsets.at_256(300)):
        assert _raw(enc, dev, ids, good, refs=(ref[0], bad, 3)) == -6, bad
    check()
    put = _dev if dev else (lambda a: a)
    call = enc.overlap_device if dev else enc.overlap_rows
    for a, r in [(ids.astype(np.int64), good), (ids, good.astype(np.int32)), (ids.astype(np.float32), None), (ids, good[:0])]:
        with pytest.raises(ValueError):
            call(put(a), put(r))
        with pytest.raises(ValueError):
            enc.set_overlap_refs(put(a), put(r))
    for kw in (dict(ngram=0), dict(ngram=65)):
        with pytest.raises(ValueError):
            enc.set_overlap_refs(put(ids), **kw)
    with pytest.raises(ValueError):
        call(put(ids), put(np.array([0, 700, 600, n])))


def test_ordered_behind_a_producer_on_the_callers_stream(enc):
    """The ids are produced by a copy still pending on a non-default stream when the call is made."""
    import torch
    src, row = _ids(3 * T, 71, 30), _offsets([T + 5, 0, 2 * T - 5])
    ref = (_ids(200, 72, 30), None, 3, 3)
    want = overlap_ref(ref, src, row)
    enc.set_overlap_refs(ref[0], ngram=3, seed=3)
    d_src, d_row, s = _dev(src), _dev(row), torch.cuda.Stream()
    ids, big = torch.zeros(src.size, dtype=torch.int32, device="cuda"), torch.ones(1 << 26, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(8):
            big = big * 1.0001 + 0.5   # keeps the stream busy
        ids.copy_(d_src)               # the producer, queued behind it
        got = enc.overlap_device(ids, d_row, token_outputs=True, stream=s.cuda_stream)
    s.synchronize()
    assert want[5] > 0
    _same(got, want, "stream")


def test_encode_overlap(enc):
    docs = [b"ab abab c ab ab", b"", b"abab ab c c c ab abab ab", b"c"]
    ids, row = enc.encode_batch(docs)[:2]
    enc.set_overlap_refs(enc.encode(b"c c ab abab"), ngram=3, seed=4)
    got = enc.encode_overlap(docs, token_outputs=True)
    assert np.array_equal(got[0], ids) and np.array_equal(got[1], row)
    want = enc.overlap_rows(ids, row, token_outputs=True)
    _same(got[2:], want, "encode_overlap")
    assert want[0].tolist() == [2, 0, 5, 0] and enc.encode_overlap(b" ".join(docs))[5:7] == (None, None)
