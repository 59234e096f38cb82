"""GPU tests of the MinHash calls (include/shredword_encode.h, shred_minhash_*): every case runs through both ABIs,
host rows and device tensors, and every word of sig and of the keys equals the numpy restatement of the header below."""
import ctypes

import numpy as np
import pytest

import bad_offsets

pytestmark = pytest.mark.gpu

TILE = 2048  # shredword.encoder.MINHASH_TILE, checked in test_tile_edges
U = np.uint64
SHINGLE, PERM_A, PERM_B, BAND = (U((1 << 40) + k) for k in (8, 9, 10, 11))


def _mix(x):
    x = (x ^ (x >> U(33))) * U(0xff51afd7ed558ccd)
    x = (x ^ (x >> U(33))) * U(0xc4ceb9fe1a85ec53)
    return x ^ (x >> U(33))


def _d(seed, x, c):
    return _mix(_mix(U(seed) + U(0x9E3779B97F4A7C15) * (np.asarray(x, dtype=U) + U(1))) ^ c)


def minhash_ref(ids, row, K, w, seed=0, B=0):
    """The header's definition -> (sig uint32 [rows, K], keys uint64 [rows, B])."""
    ids = np.asarray(ids, dtype=np.int32).astype(np.uint32).astype(U)
    row = np.array([0, ids.size]) if row is None else np.asarray(row)
    R = row.size - 1
    with np.errstate(over="ignore"):
        a, b = _d(seed, np.arange(K), PERM_A) | U(1), _d(seed, np.arange(K), PERM_B)
        sig = np.full((R, K), 0xFFFFFFFF, dtype=np.uint32)
        for r in range(R):
            t = ids[row[r]:row[r + 1]]
            c = min(t.size, w)
            if c:
                cnt = t.size - c + 1
                h = np.full(cnt, _d(seed, c, SHINGLE))
                for j in range(c):
                    h = _mix(h ^ t[j:j + cnt])
                sig[r] = ((a[None, :] * (h >> U(32))[:, None] + b[None, :]) >> U(32)).min(axis=0)
        g = np.broadcast_to(_d(seed, np.arange(B), BAND), (R, B)) if B else np.zeros((R, 0), U)
        for k in range(K // B if B else 0):
            g = _mix(g ^ sig[:, k::K // B].astype(U))  # column j: sig[r, j K / B + k]
    return sig, g


@pytest.fixture(scope="module")
def enc():
    from shredword.encoder import BPEEncoder
    e = BPEEncoder.from_merges(np.array([[97, 98, 256]], dtype=np.int32))
    yield e
    e.destroy()


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _both(e, ids, row=None, K=128, w=5, seed=0, B=0):
    """The call on host rows and on device tensors, both compared with the reference; -> the reference's."""
    import torch
    ids = np.asarray(ids, dtype=np.int32)
    row = None if row is None else np.asarray(row, dtype=np.int64)
    want = minhash_ref(ids, row, K, w, seed, B)
    kw = dict(num_perm=K, shingle=w, seed=seed, bands=B)
    host = e.minhash_rows(ids, row, **kw)
    d_ids = _dev(ids)
    *dev, ms = e.minhash_device(d_ids, _dev(row), **kw)
    assert ms >= 0 and torch.equal(d_ids.cpu(), torch.from_numpy(ids)), "the input tensor is untouched"
    assert [t.dtype for t in dev] == [torch.int32, torch.int64][:len(dev)]
    dev = [t.cpu().numpy().view(dt) for t, dt in zip(dev, (np.uint32, np.uint64))]
    for name, got in (("host", host if B else (host,)), ("device", dev)):
        assert len(got) == (2 if B else 1)
        for g, x in zip(got, want):
            assert g.dtype == x.dtype and g.shape == x.shape and np.array_equal(g, x), (name, K, w, B)
    return want


_ids = lambda n, seed: np.random.default_rng(seed).integers(0, 50000, size=n).astype(np.int32)
_offsets = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
SHORT = _offsets([0, 0, 7, 1, 0, 12, 5, 4, 6, 0, 300, 3, 0])  # empty rows first, last and side by side
THREE = 2 * TILE + 3                                              # one row flushed by three tiles


@pytest.mark.parametrize("w", [1, 2, 5, 64])
def test_row_lengths_around_the_shingle(enc, w):
    row = _offsets([0, 0, 1, w - 1, w, w + 1, 0, w, 1, 0, 0, w + 1, w - 1, 0])
    _both(enc, _ids(row[-1], w), row, K=64, w=w, seed=w)
    for n in (0, 1, w - 1, w, w + 1):
        _both(enc, _ids(n, n), None, K=64, w=w, seed=9)
    _both(enc, [], [0], K=64, w=w, B=4)   # no rows: empty outputs from both calls


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, THREE])
def test_tile_edges(enc, n):
    from shredword.encoder import MINHASH_TILE
    assert TILE == MINHASH_TILE
    ids = _ids(n, n)
    _both(enc, ids, None, K=64, w=5)                       # one wave of permutations, four shares of the tile
    _both(enc, ids, [0, 0, n, n], K=128, w=64, B=16)       # shingles that straddle the edges
    if n == THREE:                                         # a row ends at an edge, the next begins there
        _both(enc, ids, [0, TILE - 3, TILE, TILE, 2 * TILE, n], K=128, w=5, B=1)
        _both(enc, ids, [0, TILE // 2 + 2, TILE, n], K=200, w=3)


def test_more_rows_in_a_tile_than_one_stage(enc):
    from shredword.encoder import BATCH_STAGE
    row = _offsets(np.random.default_rng(3).integers(1, 4, size=600))
    assert np.bincount(row[:-1] // TILE).max() > BATCH_STAGE
    _both(enc, _ids(row[-1], 3), row, K=64, w=2, B=4)


@pytest.mark.parametrize("K", [1, 7, 64, 128, 200, 512])
def test_permutation_counts(enc, K):
    _both(enc, _ids(SHORT[-1], K), SHORT, K=K, w=5, seed=K)
    _both(enc, _ids(THREE, K), None, K=K, w=5, seed=K)


@pytest.mark.parametrize("B", [1, 16, 128])
def test_bands(enc, B):
    sig, keys = _both(enc, _ids(SHORT[-1], B), SHORT, K=128, w=5, seed=2, B=B)
    empty = np.diff(SHORT) == 0
    assert (keys[empty] == keys[empty][0]).all() and (sig[empty] == 0xFFFFFFFF).all()


def test_id_values_and_equal_rows(enc):
    odd = np.array([-1, -2 ** 31, 2 ** 31 - 1, 0], dtype=np.int32)
    ids = np.concatenate([odd, _ids(TILE, 1), odd, [5]]).astype(np.int32)
    sig, keys = _both(enc, ids, [0, 4, TILE + 4, TILE + 8, TILE + 9], K=128, w=3, B=16)
    assert np.array_equal(sig[0], sig[2]) and np.array_equal(keys[0], keys[2]) and not np.array_equal(sig[0], sig[1])


def _raw(e, dev, ids, row, keys=True, K=128, w=5, B=0, rows=None):
    """The C ABI on host arrays (dev false) or tensors, each buffer one element into its allocation and so only
    element-aligned -> (the return value, sig, keys as the call left them: preset to 7, untouched by an error)."""
    import torch
    from shredword.cbase import ShredMinhashOpts, lib
    row, lead = np.asarray(row, dtype=np.int64), lambda a: np.concatenate([a[:1], a])
    out = (np.full(301 * 512, 7, np.uint32), np.full(301 * 512, 7, np.uint64))
    bufs = [(_dev(lead(a)) if dev else lead(a))[1:] for a in (ids, row, *out)]
    ptr = [t.data_ptr() if dev else t.ctypes.data for t in bufs]
    args = [e.enc, ptr[0], len(ids), ptr[1], len(row) - 1 if rows is None else rows,
            ctypes.byref(ShredMinhashOpts(1, K, w, B)), ptr[2], ptr[3] if keys else None]
    if dev:
        args += [ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(ctypes.c_double())]
    code = (lib.shred_minhash_device if dev else lib.shred_minhash_rows)(*args)
    sig, key = (t.cpu().numpy() if dev else t for t in bufs[2:])
    assert code >= 0 or ((sig == 7).all() and (key == 7).all()), (row, K, w, B)
    return code, sig, key


@pytest.mark.parametrize("dev", [False, True])
def test_element_aligned_views_and_errors_that_write_nothing(enc, dev):
    n = TILE + 77
    ids, good = _ids(n, 11), _offsets([3, 0, TILE - 1, 75])
    (code, sig, key), want = _raw(enc, dev, ids, good, B=16), minhash_ref(ids, good, 128, 5, 1, 16)
    assert code == 4 and (sig[4 * 128:] == 7).all() and (key[4 * 16:] == 7).all()
    assert np.array_equal(sig[:4 * 128], want[0].ravel()) and np.array_equal(key[:4 * 16], want[1].ravel())
    assert _raw(enc, dev, ids, good, keys=False)[0] == 4
    for bad in ([0, 50, 40, n], [1, 50, n], [0, 50, n - 1], [0, -1, n], [0, 50, n + 1, n], *bad_offsets.at_256(n)):
        assert _raw(enc, dev, ids, bad, B=16)[0] == -6, bad
    for kw in (dict(B=3), dict(B=129), dict(B=-1), dict(B=0), dict(K=0, B=0, keys=False), dict(K=513, B=0, keys=False),
               dict(w=0, B=16), dict(w=65, B=16), dict(B=16, keys=False), dict(B=16, rows=2 ** 62)):
        assert _raw(enc, dev, ids, good, **kw)[0] == -1, kw
    for row, kw in [(good, dict(num_perm=0)), (good, dict(num_perm=513)), (good, dict(shingle=0)), (good, dict(bands=3)),
                    (good, dict(shingle=65)), (good, dict(bands=200)), ([0, 5], {}), ([0, 700, 600, n], {})]:
        with pytest.raises(ValueError):
            enc.minhash_device(_dev(ids), _dev(np.array(row)), **kw) if dev else enc.minhash_rows(ids, row, **kw)


def test_ordered_behind_a_producer_on_the_callers_stream(enc):
    """The ids are produced by a kernel still pending on a non-default stream when the call is made."""
    import torch
    src, row = _ids(3 * TILE, 71), _offsets([TILE + 5, 0, 2 * TILE - 5])
    want = minhash_ref(src, row, 128, 5, 3, 16)
    d_src, d_row, s = _dev(src), _dev(row), torch.cuda.Stream()
    ids, big = torch.zeros(src.size, dtype=torch.int32, device="cuda"), torch.ones(1 << 26, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(8):
            big = big * 1.0001 + 0.5   # keeps the stream busy
        ids.copy_(d_src)               # the producer, queued behind it
        sig, keys, _ = enc.minhash_device(ids, d_row, seed=3, bands=16, stream=s.cuda_stream)
    s.synchronize()
    assert all(np.array_equal(t.cpu().numpy().view(x.dtype), x) for t, x in zip((sig, keys), want))


def test_encode_minhash(enc):
    docs = [b"ab abab c ab ab", b"", b"abab ab c c c ab abab ab"]
    ids, row, sig, keys = enc.encode_minhash(docs, num_perm=64, shingle=2, seed=4, bands=8)
    assert np.array_equal(ids, enc.encode_batch(docs)[0]) and row.size == 4 and row[1] == row[2]
    want = enc.minhash_rows(ids, row, num_perm=64, shingle=2, seed=4, bands=8)
    assert all(g.dtype == x.dtype and np.array_equal(g, x) for g, x in zip((sig, keys), want))
    assert len(enc.encode_minhash(b"".join(docs), num_perm=8)) == 3


def test_equal_columns_estimate_the_jaccard_similarity(enc):
    """Two rows of distinct ids, 2000 shared and 1000 private each: J = 2000 / 4000.  The share of equal
    columns is a mean of K = 512 draws of probability J: within four standard deviations, 4 sqrt(0.25 / 512).
    The seed is picked on the CPU: the first whose reference is inside half the bound."""
    ids = np.random.default_rng(6).permutation(100000)[:4000].astype(np.int32)
    both, row = np.concatenate([ids[:3000], ids[:2000], ids[3000:]]), [0, 3000, 6000]
    bound, share = 4 * (0.25 / 512) ** 0.5, lambda s: float((s[0] == s[1]).mean())
    seed = next(s for s in range(20) if abs(share(minhash_ref(both, row, 512, 1, s)[0]) - 0.5) < bound / 2)
    assert abs(share(_both(enc, both, row, K=512, w=1, seed=seed)[0]) - 0.5) <= bound


def test_host_pieces(enc, monkeypatch):
    """SHREDWORD_BATCH_PIECE below the longest row (1500 ids) and the row count (60): the unpieced call's bytes."""
    lens = np.random.default_rng(61).integers(0, 40, size=55)
    row = _offsets(np.r_[0, lens[:6], 0, 0, lens[6:20], 1500, lens[20:], 0])
    for r in (row, None):
        monkeypatch.delenv("SHREDWORD_BATCH_PIECE", raising=False)
        want = _both(enc, _ids(row[-1], 61), r, seed=77, B=16)
        for piece in ("1", "7", "999"):
            monkeypatch.setenv("SHREDWORD_BATCH_PIECE", piece)
            got = enc.minhash_rows(_ids(row[-1], 61), r, seed=77, bands=16)
            assert [g.tobytes() for g in got] == [x.tobytes() for x in want], piece
