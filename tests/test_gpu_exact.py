"""GPU tests of the exact-dedup calls (include/shredword_encode.h, shred_exact_*): every case runs through both ABIs, host
rows and device tensors, and every output equals, bit for bit, the numpy restatement of the header below."""
import ctypes

import numpy as np
import pytest

import bad_offsets

pytestmark = pytest.mark.gpu

T, S = 2304, 9  # ids per workgroup, ids per thread
U = np.uint64
ALL = U(2 ** 64 - 1)
NGRAM, MULT, ROW, GROUP = (U((1 << 40) + k) for k in (12, 13, 14, 15))


def _mix(x):
    x = (x ^ (x >> U(33))) * U(0xff51afd7ed558ccd)
    x = (x ^ (x >> U(33))) * U(0xc4ceb9fe1a85ec53)
    return x ^ (x >> U(33))


def _d(seed, x, c):
    return _mix(_mix(U(seed) + U(0x9E3779B97F4A7C15) * (np.asarray(x, dtype=U) + U(1))) ^ c)


def _print(x):
    x = _mix(x)
    return np.where(x == ALL, ALL - U(1), x)


class Ref:
    """The header's state and definition: a dict for the first occurrences."""

    def __init__(self, seed=0, min_len=1):
        self.seed, self.min_len, self.seen, self.groups_seen, self.tab = seed, min_len, 0, 0, {}

    def call(self, ids, row=None, grp=None, in_group=False):
        """-> (first, dup, print, g_dup_rows, g_dup_ids, g_in_rows, dups)"""
        t = np.asarray(ids, dtype=np.int32).astype(np.uint32).astype(U)
        row = np.array([0, t.size]) if row is None else np.asarray(row, dtype=np.int64)
        R, G = len(row) - 1, 0 if grp is None else len(grp) - 1
        of = np.zeros(R, dtype=np.int64) if grp is None else np.searchsorted(grp, np.arange(R), side="right") - 1
        first, dup, F = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=bool), np.zeros(R, dtype=U)
        gout = np.zeros((3, G), dtype=np.int64)
        with np.errstate(over="ignore"):
            g, A = _d(self.seed, t, NGRAM), _d(self.seed, 0, MULT) | U(1)
            for r in range(R):
                x = g[row[r]:row[r + 1]]
                pw = np.multiply.accumulate(np.r_[U(1), np.full(max(x.size - 1, 0), A)])[::-1][:x.size]
                F[r] = _print((pw * x).sum(dtype=U) ^ _d(self.seed, x.size, ROW))
                at = first[r] = self.seen + r
                if x.size < self.min_len:
                    continue
                first[r] = self.tab.setdefault(int(F[r]), at)
                dup[r] = first[r] < at
                if G:
                    gout[:2, of[r]] += dup[r], dup[r] * x.size
                if in_group:
                    gout[2, of[r]] += self.tab.setdefault(int(_print(F[r] ^ _d(self.seed, self.groups_seen + of[r], GROUP))), at) < at
        self.seen, self.groups_seen = self.seen + R, self.groups_seen + G
        g = [None] * 3 if grp is None else [gout[0], gout[1], gout[2] if in_group else None]
        return (first, dup, F, *g, int(dup.sum()))

    def stats(self, capacity):
        slots = 2
        while slots < 2 * capacity:
            slots *= 2
        return dict(table_bytes=16 * slots, capacity=capacity, distinct=len(self.tab), seen=self.seen, groups_seen=self.groups_seen)


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
    assert got[6] == want[6], why
    for i, (g, x) in enumerate(zip(got[:6], want[:6])):
        if x is None:
            assert g is None, (why, i)
            continue
        g = g if isinstance(g, np.ndarray) else g.cpu().numpy()
        g = g.view(U) if i == 2 else g
        assert g.dtype == x.dtype and g.shape == x.shape and np.array_equal(g, x), (why, i)


def _both(e, calls, seed=0, min_len=1, capacity=1 << 16):
    """A reset and the calls [(ids, row, grp, in_group), ..] through host rows and then through device tensors, each
    against a fresh reference -> the reference's results (of the second run, equal to the first's)."""
    for dev in (False, True):
        put = _dev if dev else (lambda a: a)
        e.exact_reset(capacity, seed=seed, min_len=min_len)
        ref, wants = Ref(seed, min_len), []
        for k, (ids, row, grp, in_group) in enumerate(calls):
            ids, arr = np.asarray(ids, dtype=np.int32), lambda a: None if a is None else np.asarray(a, dtype=np.int64)
            want = ref.call(ids, arr(row), arr(grp), in_group)
            got = (e.exact_device if dev else e.exact_rows)(put(ids), put(arr(row)), group_offsets=put(arr(grp)),
                                                           in_group=in_group, prints=True)
            assert not dev or got[7] >= 0
            _same(got, want, (dev, k))
            assert e.exact_stats() == ref.stats(capacity), (dev, k)
            wants.append(want)
    return wants


_ids = lambda n, seed, vocab=50000: (np.random.default_rng(seed).integers(0, vocab, size=n) - 1).astype(np.int32)
_offsets = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
_rows = lambda rows: (np.concatenate([np.asarray(r, dtype=np.int32) for r in rows] + [np.zeros(0, np.int32)]),
                      _offsets([len(r) for r in rows]))


@pytest.mark.parametrize("seed", [0, 2 ** 64 - 3])
def test_row_sizes_and_tile_edges_and_copies_at_other_offsets(enc, seed):
    """Rows of every size with empty rows between, then a row of 4 ids, then every row again: the copies lie 23270 ids
    further on, another offset mod the strip and mod the tile; the row of 5 T + 3 ids starts mid-tile and spans six."""
    lens = [0, 1, 2, S - 1, S, S + 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 5 * T + 3]
    rows = [x for i, L in enumerate(lens) for x in (_ids(L, 10 + i), [])]
    ids, row = _rows(rows + [_ids(4, 9)] + rows)
    shift = int(row[len(rows) + 1])
    assert shift % S and shift % T and int(row[26]) % T and int(row[26]) % S and (row[27] - 1) // T - row[26] // T >= 4
    want = _both(enc, [(ids, row, None, False)], seed=seed)[0]
    copies = np.r_[np.zeros(len(rows) + 1, bool), np.tile([True, False], len(lens))]
    copies[len(rows) + 1] = False  # the empty row
    assert np.array_equal(want[1], copies) and np.array_equal(want[0][copies], np.flatnonzero(copies) - len(rows) - 1)


@pytest.mark.parametrize("a, b", [([3, 0, -1, 8], [4, 0, -1, 8]), ([3, 0, -1, 8], [3, 0, -1, 9]), ([5, -1], [5, -1, 0]),
                                  ([0], [0, 0]), ([-1, 0, 7, 7], [7, -1, 7, 0])])
def test_near_misses_are_not_duplicates(enc, a, b):
    """Rows that differ in the first id, in the last, in length only (twice), and a permutation."""
    want = _both(enc, [(*_rows([a, b, a, b]), None, False)])[0]
    assert want[0].tolist() == [0, 1, 0, 1] and want[1].tolist() == [False, False, True, True]


@pytest.mark.parametrize("min_len", [0, 1, 3])
def test_min_len(enc, min_len):
    lens = [0, 1, 0, 1, 2, 2, 3, 3, 0]
    want = _both(enc, [(*_rows([[6] * L for L in lens]), None, False)], min_len=min_len)[0]
    assert want[1].tolist() == [L >= min_len and lens.index(L) < r for r, L in enumerate(lens)]
    assert all(want[0][r] == r for r, L in enumerate(lens) if L < min_len) and want[2][0] == want[2][2] != want[2][1]


def test_state_across_calls(enc):
    a, b = _rows([_ids(L, L) for L in (5, 0, T + 3, 1, 70)]), _rows([_ids(L, L) for L in (9, 70, 5, T + 3, 2)])
    one, two = _both(enc, [(*a, None, False), (*b, None, False)], seed=5)
    assert one[6] == 0 and two[0].tolist() == [5, 4, 0, 2, 9] and two[6] == 3
    assert enc.exact_stats()["seen"] == 10 and enc.exact_stats()["distinct"] == 6
    again = _both(enc, [(*b, None, False)], seed=6)[0]   # a reset forgets, a new seed changes the fingerprints
    assert again[6] == 0 and not (again[2] == two[2]).any()


def _lines(seed=0):
    """Lines as rows, documents as groups (two without rows): A repeats inside group 0; B comes back from an earlier
    group only; in group 3, C comes from group 2, D repeats inside, and A does both."""
    A, B, C, D = ([k, 0, -1, k] * (k + 1) for k in range(1, 5))
    return (*_rows([A, B, A, [], B, C, C, D, D, A, [], A]), [0, 4, 4, 6, 12, 12])


def test_groups(enc):
    ids, row, grp = _lines()
    one, two = _both(enc, [(ids, row, grp, True)] * 2)
    assert one[3].tolist() == [1, 0, 1, 4, 0] and one[5].tolist() == [1, 0, 0, 2, 0]   # in-group <= duplicates
    assert one[4].tolist() == [8, 0, 12, 16 + 20 + 2 * 8, 0]
    # the second call's groups have other global indices: every row is a duplicate, in its group only the repeats are
    assert two[3].tolist() == [3, 0, 2, 5, 0] and two[5].tolist() == one[5].tolist() and enc.exact_stats()["groups_seen"] == 10
    few = enc.exact_rows(ids, row, group_offsets=grp)
    assert few[2] is None and few[5] is None and few[3].tolist() == two[3].tolist()


def test_host_pieces(enc, monkeypatch):
    """SHREDWORD_BATCH_PIECE below the longest row (1500 ids) and the row count: the unpieced call's bytes, twice over
    (the second call starts from the first's seen and groups_seen)."""
    lens = np.random.default_rng(61).integers(0, 4, size=60)
    row = _offsets(np.r_[lens[:20], 1500, lens[20:], 1500, 0])
    ids, grp = _ids(row[-1], 61, 3), [0, 0, 7, 30, 30, 31, 63]
    ids[row[61]:row[62]] = ids[row[20]:row[21]]
    for r, g in ((row, grp), (row, None), (None, None)):
        monkeypatch.delenv("SHREDWORD_BATCH_PIECE", raising=False)
        calls = [(ids, r, g, g is not None)] * 2
        wants = _both(enc, calls, seed=77)
        assert r is None or (wants[0][1][61] and 0 < wants[0][6] < wants[1][6] == (np.diff(row) > 0).sum())
        for piece in ("1", "7", "999"):
            monkeypatch.setenv("SHREDWORD_BATCH_PIECE", piece)
            enc.exact_reset(1 << 16, seed=77)
            for want in wants:
                _same(enc.exact_rows(ids, r, group_offsets=g, in_group=g is not None, prints=True), want, piece)


def _raw(e, dev, ids, row, grp=None, skip=(), rows=None):
    """The C ABI on host arrays (dev false) or tensors, each buffer one element into its allocation and so only
    element-aligned -> (the return value, the six outputs as the call left them: preset to 7, untouched by an error).
    skip: the outputs passed as NULL (the group outputs are passed even without grp)."""
    import torch
    from shredword.cbase import lib
    row, lead = np.asarray(row, dtype=np.int64), lambda a: np.concatenate([a[:1], a])
    grp = None if grp is None else np.asarray(grp, dtype=np.int64)
    tail = [ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(ctypes.c_double())] if dev else []
    out = [np.full(400, 7, dt) for dt in (np.int64, np.uint8, np.uint64, np.int64, np.int64, np.int64)]
    bufs = [(_dev(lead(a)) if dev else lead(a))[1:] for a in (ids, row, np.zeros(1, np.int64) if grp is None else grp, *out)]
    ptr = [t.data_ptr() if dev else t.ctypes.data for t in bufs]
    outs = [None if i in skip else p for i, p in enumerate(ptr[3:])]
    before = e.exact_stats()
    code = (lib.shred_exact_device if dev else lib.shred_exact_rows)(
        e.enc, ptr[0], len(ids), ptr[1], len(row) - 1 if rows is None else rows, None if grp is None else ptr[2],
        0 if grp is None else len(grp) - 1, *outs, *tail)
    got = [t.cpu().numpy() if dev else t for t in bufs[3:]]
    assert code >= 0 or (all((g == 7).all() for g in got) and e.exact_stats() == before), row
    return code, got


@pytest.mark.parametrize("dev", [False, True])
def test_element_aligned_views_errors_and_capacity(dev):
    from shredword.encoder import BPEEncoder
    e = BPEEncoder.from_merges(np.array([[97, 98, 256]], dtype=np.int32))
    ids, row, grp = _lines()
    n, no_groups = ids.size, (3, 4, 5)
    assert _raw(e, dev, ids, row, skip=no_groups)[0] == -1      # before any reset
    e.exact_reset(5)                                            # 4 distinct lines, twice with the in-group keys
    assert _raw(e, dev, ids, row, grp)[0] == -1 and _raw(e, dev, ids, row, skip=no_groups)[0] == -1
    assert _raw(e, dev, ids[:row[5]], row[:6], skip=no_groups)[0] == 2
    e.exact_reset(20, seed=1)
    want = Ref(1).call(ids, row, np.asarray(grp), True)
    code, got = _raw(e, dev, ids, row, grp)
    assert code == want[6] == 6
    for g, x, size in zip(got, want, [12, 12, 12, 5, 5, 5]):
        assert np.array_equal(g[:size], x) and (g[size:] == 7).all()
    for bad in ([0, 50, 40, n], [1, 50, n], [0, 50, n - 1], [0, -1, n], [0, 50, n + 1, n], *bad_offsets.at_256(n)):
        assert _raw(e, dev, ids, bad, skip=no_groups)[0] == -6, bad
    for bad in ([0, 5, 4, 12], [1, 12], [0, 11], [0, -1, 12], [0, 13, 12]):
        assert _raw(e, dev, ids, row, bad)[0] == -6, bad
    wide = _offsets(np.r_[np.full(n, 1), np.zeros(300 - n, int)])   # 300 rows, so that grp_off has an entry 256
    for bad in bad_offsets.at_256(300):
        assert _raw(e, dev, ids, wide, bad)[0] == -6
    assert _raw(e, dev, ids, row, grp, skip=(0,))[0] == -1 and _raw(e, dev, ids, row, rows=2 ** 62, skip=no_groups)[0] == -1
    for k in no_groups:
        assert _raw(e, dev, ids, row, skip=set(no_groups) - {k})[0] == -1, k
    put = _dev if dev else (lambda a: a)
    call = e.exact_device if dev else e.exact_rows
    for a, r, g in [(ids.astype(np.int64), row, None), (ids, row.astype(np.int32), None), (ids, row[:0], None),
                    (ids, row, np.asarray(grp, dtype=np.int32)), (ids, [0, 70, 60, n], None), (ids, row, [0, 5, 4, 12])]:
        with pytest.raises(ValueError):
            call(put(a), put(np.asarray(r)), group_offsets=put(g if g is None else np.asarray(g)))
    with pytest.raises(ValueError):
        call(put(ids), put(row), in_group=True)
    e.exact_reset(0)
    assert e.exact_stats()["table_bytes"] == 0 and _raw(e, dev, ids, row, skip=no_groups)[0] == -1
    e.destroy()


def test_ordered_behind_a_producer_on_the_callers_stream(enc):
    """The ids are produced by a copy still pending on a non-default stream when the call is made."""
    import torch
    src, row = _ids(5 * T, 71, 30), _offsets([T + 5, 0, T + 5, 3 * T - 210, 200])
    src[T + 5:2 * T + 10] = src[:T + 5]
    enc.exact_reset(64, seed=3)
    want = Ref(3).call(src, row)
    d_src, d_row, s = _dev(src), _dev(row), torch.cuda.Stream()
    ids, big = torch.zeros(src.size, dtype=torch.int32, device="cuda"), torch.ones(1 << 26, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(8):
            big = big * 1.0001 + 0.5   # keeps the stream busy
        ids.copy_(d_src)               # the producer, queued behind it
        got = enc.exact_device(ids, d_row, prints=True, stream=s.cuda_stream)
    s.synchronize()
    assert want[6] == 1
    _same(got, want, "stream")


def test_encode_exact(enc):
    text = b"ab abab\nc ab\nab abab\n\nc ab\nab c c\n"
    lines = np.r_[0, np.flatnonzero(np.frombuffer(text, np.uint8) == 10) + 1]
    ids, row = enc.encode_docs(text, lines)[:2]
    enc.exact_reset(64, seed=4)
    want = enc.exact_rows(ids, row, group_offsets=[0, 3, 6], in_group=True, prints=True)
    enc.exact_reset(64, seed=4)
    got = enc.encode_exact(text, doc_offsets=lines, group_offsets=[0, 3, 6], in_group=True, prints=True)
    assert np.array_equal(got[0], ids) and np.array_equal(got[1], row)
    _same(got[2:], want, "encode_exact")
    assert want[1].tolist() == [False, False, True, False, True, False] and want[3].tolist() == [1, 1] and want[5].tolist() == [1, 0]
