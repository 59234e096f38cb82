"""GPU tests of the dedup calls (include/shredword_encode.h, shred_dedup_*): every case runs through both ABIs, host
rows and device tensors, and label, keep and the count equal the numpy restatement of the header below."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL = 2 ** 64 - 1


def dedup_ref(sig, keys, min_equal):
    """The header's definition -> (label int64, keep bool, components, candidates accepted, candidates rejected)."""
    R, B = keys.shape
    parent, rows, acc, rej = np.arange(R), np.arange(R), 0, 0

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for j in range(B if R else 0):
        inv = np.unique(keys[:, j], return_inverse=True)[1].reshape(-1)
        first = np.full(inv.max() + 1, R)
        np.minimum.at(first, inv, rows)
        rep = first[inv]
        cand = np.flatnonzero(rep != rows)
        ok = (sig[cand] == sig[rep[cand]]).sum(axis=1) >= min_equal if min_equal else np.ones(cand.size, bool)
        acc, rej = acc + int(ok.sum()), rej + int((~ok).sum())
        for r in cand[ok]:
            a, b = find(r), find(rep[r])
            parent[max(a, b)] = min(a, b)
    label = np.array([find(r) for r in range(R)], dtype=np.int64)
    return label, label == rows, int((label == rows).sum()), acc, rej


@pytest.fixture(scope="module")
def enc():
    from shredword.encoder import BPEEncoder
    e = BPEEncoder.from_merges(np.array([[97, 98, 256]], dtype=np.int32))
    yield e
    e.destroy()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _both(e, sig, keys, min_equal):
    """The call on host rows and on device tensors, both compared with the reference; -> the reference's."""
    import torch
    sig, keys = np.asarray(sig, dtype=np.uint32), np.asarray(keys, dtype=np.uint64)
    want = dedup_ref(sig, keys, min_equal)
    host = e.dedup_rows(sig, keys, min_equal=min_equal)
    d_sig, d_keys = _dev(sig.view(np.int32)), _dev(keys.view(np.int64))
    *dev, ms = e.dedup_device(d_sig, d_keys, min_equal=min_equal)
    assert ms >= 0 and np.array_equal(d_sig.cpu().numpy(), sig.view(np.int32)), "the input tensor is untouched"
    assert [t.dtype for t in dev[:2]] == [torch.int64, torch.bool]
    for name, got in (("host", host), ("device", [dev[0].cpu().numpy(), dev[1].cpu().numpy(), dev[2]])):
        assert got[0].dtype == np.int64 and got[1].dtype == np.bool_, name
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], \
            (name, sig.shape, keys.shape, min_equal)
    return want


def _random(R, B, K, span, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2, (R, K)).astype(np.uint32), rng.integers(0, max(int(span * R), 1), (R, B)).astype(np.uint64)


@pytest.mark.parametrize("B,K", [(1, 1), (1, 7), (4, 16), (16, 128), (128, 512)])
def test_sizes(enc, B, K):
    for R in (0, 1, 2, 63, 64, 65, 1000):
        sig, keys = _random(R, B, K, 2, seed=R)
        for m in (0, 1, K // 2 + 1, K):
            assert (_both(enc, sig, keys, m)[2] == 0) == (R == 0)


@pytest.mark.parametrize("R,B,K,m,span", [(1000, 4, 16, 9, 2), (5000, 16, 128, 68, 4), (65, 1, 7, 4, 0.3),
                                          (1000, 4, 16, 0, 8)])
def test_random_rows_link_some_and_not_all(enc, R, B, K, m, span):
    _, _, count, acc, rej = _both(enc, *_random(R, B, K, span), m)
    assert 1 < count < R and (m == 0 or (acc > 0 and rej > 0))


@pytest.mark.parametrize("K", [7, 200, 128, 512])
def test_threshold_edge(enc, K):
    """Rows 0, 1 agree in exactly m - 1 columns and rows 2, 3 in exactly m, spread over the row and its tail."""
    m, rng = K // 2 + 1, np.random.default_rng(K)
    sig, cols = np.arange(4 * K, dtype=np.uint32).reshape(4, K), rng.permutation(K)
    sig[1, cols[:m - 1]], sig[3, cols[:m]] = sig[0, cols[:m - 1]], sig[2, cols[:m]]
    assert (sig[0] == sig[1]).sum() == m - 1 and (sig[2] == sig[3]).sum() == m
    label = _both(enc, sig, np.array([[5], [5], [9], [9]]), m)[0]
    assert label.tolist() == [0, 1, 2, 2]


def test_one_bucket(enc):
    R, K = 5000, 16
    sig = np.arange(R * K, dtype=np.uint32).reshape(R, K)
    keys = np.full((R, 2), 12345, dtype=np.uint64)
    label, _, count, _, _ = _both(enc, sig, keys, 0)
    assert count == 1 and not label.any()
    assert _both(enc, sig, keys, K)[2] == R


@pytest.mark.parametrize("reverse", [False, True])
def test_a_path(enc, reverse):
    """Row i + 1 shares exactly one key with row i, in band i % B; reversed, the links arrive against the index order."""
    R, B = 5000, 4
    keys = np.random.default_rng(1).permutation(R * B).reshape(R, B).astype(np.uint64)
    for i in range(R - 1):
        keys[i + 1, i % B] = keys[i, i % B]
    label, _, count, _, _ = _both(enc, np.zeros((R, 4)), keys[::-1] if reverse else keys, 0)
    assert count == 1 and not label.any()


def test_key_values(enc):
    """0 and 2^64 - 1 as shared and as unshared keys; one value in two bands and equal low halves do not link."""
    X = 0x1234567800000042
    keys = np.array([[0, 11], [0, 12], [ALL, 13], [ALL, 14], [X, 0], [X + 2 ** 32, ALL], [21, 22], [ALL - 1, 21]],
                    dtype=np.uint64)
    for m in (0, 3):
        assert _both(enc, np.ones((8, 3)), keys, m)[0].tolist() == [0, 0, 2, 2, 4, 5, 6, 7]


@pytest.mark.parametrize("R", [1023, 1024, 1025])
def test_table_sizing_with_all_keys_distinct(enc, R):
    keys = np.random.default_rng(R).permutation(R * 3).reshape(R, 3).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    assert _both(enc, np.zeros((R, 4)), keys, 0)[2] == R


def test_band_groups(enc, monkeypatch):
    """SHREDWORD_DEDUP_GROUP bands at a time, and the two measurement switches, give the bytes of the unset call."""
    sig, keys = _random(1000, 4, 16, 2)
    monkeypatch.delenv("SHREDWORD_DEDUP_GROUP", raising=False)
    want = _both(enc, sig, keys, 9)
    for name, value in (("GROUP", "1"), ("GROUP", "3"), ("GROUP", "4"), ("ORDER", "band"), ("LANES", "wave")):
        monkeypatch.setenv("SHREDWORD_DEDUP_" + name, value)
        got = _both(enc, sig, keys, 9)
        assert [g.tobytes() for g in got[:2]] == [x.tobytes() for x in want[:2]] and got[2] == want[2], (name, value)


def _raw(e, dev, sig, keys, K=16, B=4, m=9, rows=None, no_sig=False, no_label=False):
    """The C ABI on host arrays (dev false) or tensors, each buffer one element into its allocation and so only
    element-aligned -> (the return value, label, keep as the call left them: preset to 7, untouched by an error)."""
    import torch
    from shredword.cbase import ShredDedupOpts, lib
    lead = lambda a: np.concatenate([a.ravel()[:1], a.ravel()])
    out = (np.full(1100, 7, np.int64), np.full(1100, 7, np.uint8))
    bufs = [(_dev(lead(a)) if dev else lead(a))[1:] for a in (sig, keys.view(np.int64), *out)]
    ptr = [t.data_ptr() if dev else t.ctypes.data for t in bufs]
    args = [e.enc, None if no_sig else ptr[0], ptr[1], len(keys) if rows is None else rows,
            ctypes.byref(ShredDedupOpts(K, B, m)), None if no_label else ptr[2], ptr[3]]
    if dev:
        args += [ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(ctypes.c_double())]
    code = (lib.shred_dedup_device if dev else lib.shred_dedup_rows)(*args)
    label, keep = (t.cpu().numpy() if dev else t for t in bufs[2:])
    assert code >= 0 or ((label == 7).all() and (keep == 7).all()), (K, B, m, rows)
    return code, label, keep


@pytest.mark.parametrize("dev", [False, True])
def test_element_aligned_views_and_errors_that_write_nothing(enc, dev):
    sig, keys = _random(1000, 4, 16, 2)
    want = dedup_ref(sig, keys, 9)
    code, label, keep = _raw(enc, dev, sig, keys)
    assert code == want[2] and np.array_equal(label[:1000], want[0]) and np.array_equal(keep[:1000], want[1])
    assert (label[1000:] == 7).all() and (keep[1000:] == 7).all()
    assert _raw(enc, dev, sig, keys, m=0, no_sig=True)[0] == dedup_ref(sig, keys, 0)[2]
    for kw in (dict(m=17), dict(m=-1), dict(B=0), dict(B=129), dict(K=0, m=0), dict(K=513), dict(no_sig=True),
               dict(no_label=True), dict(rows=2 ** 62)):
        assert _raw(enc, dev, sig, keys, **kw)[0] == -1, kw
    call = (lambda s, k, **kw: enc.dedup_device(_dev(s), _dev(k), **kw)) if dev else enc.dedup_rows  # unsigned dtypes
    for s, k, kw in [(sig[:999], keys, {}), (sig.ravel(), keys, {}), (sig, keys, dict(min_equal=17)),
                     (sig, keys, dict(threshold=1.5)), (sig.astype(np.float32), keys, {}), (sig, keys.astype(np.int32), {})]:
        with pytest.raises(ValueError):
            call(s, k, **kw)
    assert call(sig, keys, threshold=0.5)[2] == dedup_ref(sig, keys, 8)[2]


def test_ordered_behind_a_producer_on_the_callers_stream(enc):
    """sig and keys are produced by copies still pending on a non-default stream when the call is made."""
    import torch
    src = _random(1000, 4, 16, 2)
    want = dedup_ref(*src, 9)
    d_sig, d_keys, s = _dev(src[0].view(np.int32)), _dev(src[1].view(np.int64)), torch.cuda.Stream()
    sig, keys, big = torch.zeros_like(d_sig), torch.zeros_like(d_keys), torch.ones(1 << 26, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(8):
            big = big * 1.0001 + 0.5   # keeps the stream busy
        sig.copy_(d_sig)               # the producers, queued behind it
        keys.copy_(d_keys)
        label, keep, count, _ = enc.dedup_device(sig, keys, min_equal=9, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(label.cpu().numpy(), want[0]) and np.array_equal(keep.cpu().numpy(), want[1]) and count == want[2]


def test_encode_dedup(enc):
    """Rows 0 and 2 are identical, row 4 is a near-copy of them, rows 1 and 5 are empty."""
    doc = b"ab abab c ab ab abab c c ab abab ab c ab ab ab abab"
    docs = [doc, b"", doc, b"c c c c abab abab abab c c c", doc + b" c", b""]
    kw = dict(num_perm=64, shingle=2, seed=4, bands=8)
    ids, row, labels, keep = enc.encode_dedup(docs, threshold=0.5, **kw)
    assert np.array_equal(ids, enc.encode_batch(docs)[0]) and row.size == 7
    want = enc.dedup_rows(*enc.minhash_rows(ids, row, **kw), threshold=0.5)
    assert np.array_equal(labels, want[0]) and np.array_equal(keep, want[1]) and keep.dtype == np.bool_
    assert labels[0] == labels[2] == 0 and labels[1] == labels[5] == 1 and keep.sum() == want[2]
