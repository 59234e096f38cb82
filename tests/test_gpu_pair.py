"""GPU tests of the pair form of the batcher (include/shredword_encode.h: shred_pair_device /
shred_pair_rows; BPEEncoder.pair_rows / pair_device / encode_pairs).

The expected arrays come from pair_ref.py: plain Python loops (test_pair_ref_cpu.py checks them against
the header's closed forms).  Every case runs through both ABIs (host arrays in pieces, device tensors)
and all eight arrays are compared exactly.

Cases: segment lengths around the truncation thresholds of strategies 0 .. 2 for budgets 6 and 7, both
truncation sides, 0, 1, 2 and 4 added ids, and no max_len; window_second with examples of different
la in one call (so the window capacity differs inside a tile), down to C == stride + 1, lb around C
and C + step, an empty b, and max_first on both sides; the examples that cannot fit (-7) and the
argument errors on sentinel-filled buffers; output sizes on the tile boundary (BATCH_TILE - 1, + 0,
+ 1) with widths that are no multiple of a lane's 4 entries; one example whose windows fill more than
two tiles; more examples in a tile than one LDS round stages (BATCH_STAGE), with runs of examples that
are empty on both sides; width 0; pad="left", rows == 0; the sizing calls; outputs that are only
element-aligned; malformed offset arrays of either segment; host examples cut into pieces, under the
real piece budget and under small ones; encode_pairs end to end with the byte offsets of every kept
token.

Not tested: an e above INT32_MAX and a Wn * width that does not fit its type (checked by reading).
"""
import ctypes

import numpy as np
import pytest

import pair_ref

pytestmark = pytest.mark.gpu

SENT = -77  # fills outputs that a call must leave alone
NAMES = ("batch", "lengths", "pair_rows", "seg_len", "seg_src", "row_windows", "types", "mask")


def _tile():
    from shredword.encoder import BATCH_TILE
    return BATCH_TILE


def _stage():
    from shredword.encoder import BATCH_STAGE
    return BATCH_STAGE


@pytest.fixture(scope="module")
def enc():
    from shredword.encoder import BPEEncoder
    with BPEEncoder.from_merges([[97, 98, 256], [256, 99, 257]]) as e:
        yield e


def _rows_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def _example(rng, pairs):
    """[(la, lb)] -> (ids_a, row_a, ids_b, row_b) with random ids, those of b disjoint from those of a."""
    ra, rb = _rows_of([p[0] for p in pairs]), _rows_of([p[1] for p in pairs])
    return (rng.integers(0, 50_000, size=int(ra[-1])).astype(np.int32), ra,
            rng.integers(50_000, 100_000, size=int(rb[-1])).astype(np.int32), rb)


def _same(got, want, where):
    assert len(got) == len(want)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, where)


def _device(enc, ex, **kw):
    import torch
    return enc.pair_device(*[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in ex], mask=True, **kw)


def _check(enc, ex, **kw):
    """pair_rows and pair_device against the Python loops; returns the loops' arrays."""
    import torch
    want = pair_ref.pairs(*ex, **kw)
    _same(enc.pair_rows(*ex, mask=True, **kw), want, ("host", kw))
    dev = _device(enc, ex, **kw)
    assert len(dev) == 9 and dev[8] >= 0
    assert [t.dtype for t in dev[:8]] == [torch.int32] * 4 + [torch.int64] * 2 + [torch.uint8] * 2
    _same([t.cpu().numpy() for t in dev[:8]], want, ("device", kw))
    return want


# ---- the raw ABI --------------------------------------------------------------------------------

def _ptr(v):
    return None if v is None else ctypes.byref(ctypes.c_int32(v))


def _raw(enc, ex, width, out_size, emitted, *, max_len=0, strategy=0, trunc_side=0, max_a=0, stride=0, bos=None,
         sep=(), eos=None, cap=None, null_out=False):
    """Both ABIs on sentinel-filled buffers -> [(result, widest, out, types, mask, lengths, win_row, seg_len,
    seg_src, row_win)]."""
    import torch
    from shredword.cbase import lib
    ids_a, ra, ids_b, rb = [np.ascontiguousarray(x) for x in ex]
    ra, rb = ra.astype(np.int64), rb.astype(np.int64)
    R = ra.size - 1
    cap = out_size if cap is None else cap
    mid = (ctypes.c_int32 * 2)(*sep) if sep else None
    head = (_ptr(bos), mid, len(sep), _ptr(eos), max_len, trunc_side, strategy, max_a, stride, width, 0, 0)
    shapes = ((out_size, np.int32), (out_size, np.uint8), (out_size, np.uint8), (emitted, np.int32),
              (emitted, np.int32), (2 * emitted, np.int32), (2 * emitted, np.int64), (R + 1, np.int64))
    fill = lambda dt: 0xA5 if dt == np.uint8 else SENT
    res = []
    for device in (False, True):
        bufs = [np.full(max(k, 1), fill(dt), dtype=dt) for k, dt in shapes]
        widest = ctypes.c_size_t(12345)
        if device:
            bufs = [torch.from_numpy(b).cuda() for b in bufs]
            d = [torch.from_numpy(x).cuda() for x in (ids_a, ra, ids_b, rb)]
            p = [b.data_ptr() for b in bufs]
            r = lib.shred_pair_device(enc.enc, d[0].data_ptr(), ids_a.size, d[1].data_ptr(), d[2].data_ptr(), ids_b.size,
                                      d[3].data_ptr(), R, *head, None if null_out else p[0], cap, *p[1:],
                                      ctypes.byref(widest), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                                      None)
            bufs = [b.cpu().numpy() for b in bufs]
        else:
            p = [b.ctypes.data for b in bufs]
            r = lib.shred_pair_rows(enc.enc, ids_a.ctypes.data, ids_a.size, ra.ctypes.data, ids_b.ctypes.data,
                                    ids_b.size, rb.ctypes.data, R, *head, None if null_out else p[0], cap, *p[1:],
                                    ctypes.byref(widest))
        res.append((r, widest.value, *bufs))
    return res


def _untouched(*arrays):
    return all((a == (0xA5 if a.dtype == np.uint8 else SENT)).all() for a in arrays)


ADDED = {0: {}, 1: dict(bos=7), 2: dict(sep=(-8,), eos=2 ** 31 - 1), 4: dict(bos=-2 ** 31, sep=(5, 6), eos=9)}


# ---- 1. truncation thresholds -------------------------------------------------------------------

def test_truncation_thresholds(enc):
    rng = np.random.default_rng(1)
    for B in (6, 7):
        lens = sorted({0, 1, B // 2 - 1, B // 2, B // 2 + 1, B - 1, B, B + 1})
        for truncation in ("longest_first", "only_first", "only_second"):
            # a segment that is never cut and is longer than B cannot fit: test_cannot_fit
            pairs = [(la, lb) for la in lens for lb in lens
                     if not (truncation == "only_first" and lb > B) and not (truncation == "only_second" and la > B)]
            ex = _example(rng, pairs)
            for add, extra in ADDED.items():
                for truncate in ("right", "left"):
                    kw = dict(max_len=B + add, truncation=truncation, truncate=truncate, pad_id=-9, **extra)
                    want = _check(enc, ex, **kw)
                    assert want[0].shape == (len(pairs), B + add) and want[1].max() == B + add
            want = _check(enc, ex, truncation=truncation, bos=1, sep=(2, 3), eos=4)  # max_len=None: nothing is cut
            assert want[1].max() == 2 * (B + 1) + 4 - (truncation != "longest_first")
    with pytest.raises(TypeError):
        enc.pair_rows(ex[0], ex[1], ex[2])
    for bad in (dict(truncation="shortest_first"), dict(sep=(1, 2, 3)), dict(max_len=3, bos=1, sep=(1, 2), eos=1),
                dict(stride=1), dict(max_first=2), dict(pad="centre"), dict(truncate="middle"), dict(bos=2 ** 31),
                dict(truncation="window_second"), dict(truncation="window_second", max_len=2 ** 31)):
        with pytest.raises(ValueError):
            enc.pair_rows(*ex, **bad)
    with pytest.raises(ValueError):
        enc.pair_rows(ex[0], ex[1], ex[2], ex[3][:-1])  # another row count


# ---- 2. window_second ---------------------------------------------------------------------------

def test_window_second(enc):
    rng = np.random.default_rng(2)
    B = 8
    for stride in (0, 1, 3):
        pairs = []
        for la in sorted({0, 2, 4, B - stride - 1}):  # the last: C == stride + 1, the stride is C - 1
            C = B - la
            step = C - stride
            assert step >= 1
            pairs += [(la, lb) for lb in (0, 1, C - 1, C, C + 1, C + step - 1, C + step, C + step + 1,
                                          3 * C + 2 * step + 1)]
        order = rng.permutation(len(pairs))  # the capacities alternate inside a tile
        ex = _example(rng, [pairs[i] for i in order])
        for add, extra in ADDED.items():
            kw = dict(max_len=B + add, truncation="window_second", stride=stride, pad_id=-9, **extra)
            want = _check(enc, ex, **kw)
            assert want[0].shape[1] == B + add and want[5][-1] > len(pairs)
            _check(enc, ex, pad="left", width=B + add + 3, **kw)
    # max_first on both sides: la above it is cut, every C_r is at least B - 2
    ex = _example(rng, [(la, lb) for la in (0, 1, 2, 3, 9) for lb in (0, 5, 6, 7, 11, 12, 30)])
    for truncate in ("right", "left"):
        want = _check(enc, ex, max_len=11, truncation="window_second", stride=2, max_first=2, truncate=truncate,
                      bos=1, sep=(2,), eos=3)
        assert want[3][:, 0].max() == 2 and want[0].shape[1] == 11
    # the largest stride max_first allows, and one more (the host's argument check: -1)
    _check(enc, ex, max_len=8, truncation="window_second", stride=5, max_first=2)
    with pytest.raises(ValueError):
        enc.pair_rows(*ex, max_len=8, truncation="window_second", stride=6, max_first=2)
    for r, widest, *bufs in _raw(enc, ex, 8, 4096, 256, max_len=8, strategy=3, max_a=2, stride=6):
        assert r == -1 and widest == 12345 and _untouched(*bufs)


# ---- 3. examples that cannot fit, argument errors -----------------------------------------------

def test_cannot_fit(enc):
    import torch
    rng = np.random.default_rng(3)
    B = 6
    good = [(2, 3), (0, 0), (6, 0), (0, 6), (3, 3)]
    for kw, bad in ((dict(strategy=1), (1, B + 1)),                  # only_first: b alone is too long
                    (dict(strategy=2), (B + 1, 1)),                  # only_second: a alone is too long
                    (dict(strategy=3, stride=2), (B - 2, 9)),        # window_second: C_r == stride
                    (dict(strategy=3, stride=0), (B + 1, 0))):       # window_second: ka > B
        for at in (0, 2, len(good)):
            pairs = good[:at] + [bad] + good[at:]
            if kw["strategy"] == 3:
                pairs = [(min(la, 3), lb) if (la, lb) != bad else bad for la, lb in pairs]
            ex = _example(rng, pairs)
            for r, widest, *bufs in _raw(enc, ex, B + 2, 64 * (B + 2), 64, max_len=B + 2, bos=1, eos=2, **kw):
                assert r == -7 and widest == 12345 and _untouched(*bufs), (kw, at)
            name = pair_ref.STRATEGIES[kw["strategy"]]
            py = dict(max_len=B + 2, bos=1, eos=2, truncation=name, stride=kw.get("stride", 0))
            with pytest.raises(pair_ref.CannotFit):
                pair_ref.pairs(*ex, **py)
            with pytest.raises(ValueError, match="fit"):
                enc.pair_rows(*ex, **py)
            with pytest.raises(ValueError, match="fit"):
                enc.pair_device(*[torch.from_numpy(x).cuda() for x in ex], **py)
            # without the bad example the call works
            ok = _example(rng, [p for p in pairs if p != bad])
            _check(enc, ok, **py)


def test_argument_errors(enc):
    rng = np.random.default_rng(4)
    ex = _example(rng, [(4, 9), (0, 3), (2, 0)])
    for kw in (dict(strategy=4), dict(strategy=-1),                              # an unknown strategy
               dict(strategy=0, stride=1), dict(strategy=1, max_a=1), dict(strategy=2, stride=1, max_a=1),
               dict(strategy=3), dict(strategy=3, max_len=2 ** 31),               # window_second needs a max_len
               dict(strategy=0, max_len=3, bos=1, sep=(2, 3), eos=4),            # max_len < add
               dict(strategy=3, max_len=12, max_a=4, stride=8),                  # B - max_a < stride + 1
               dict(strategy=3, max_len=12, max_a=13),
               dict(strategy=0, trunc_side=2)):
        for r, widest, *bufs in _raw(enc, ex, 16, 16 * 16, 16, **kw):
            assert r == -1 and widest == 12345 and _untouched(*bufs), kw
    _check(enc, ex, max_len=12, truncation="window_second", max_first=4, stride=7)  # B - max_a == stride + 1


# ---- 4. tile and stage edges --------------------------------------------------------------------

def _window_pairs(rng, total, width):
    """(la, lb) whose windows under max_len = width, stride 0 and no added ids number exactly `total`."""
    pairs = []
    while total:
        la = int(rng.integers(0, width))
        C = width - la
        k = int(min(total, rng.integers(1, 6)))
        pairs.append((la, int(rng.integers(0, C + 1)) if k == 1 else C + (k - 1) * C - int(rng.integers(0, C))))
        total -= k
    return pairs


def test_tile_edges(enc):
    T = _tile()
    rng = np.random.default_rng(5)
    assert (T - 1) % 3 == 0 and T % 2 == 0 and (T + 1) % 5 == 0
    for width, Wn in ((3, (T - 1) // 3), (2, T // 2), (5, (T + 1) // 5),   # Wn * width == T - 1, T, T + 1
                      (1, T - 1), (1, T), (1, T + 1),
                      (3, 2 * T // 3 + 1), (7, 3 * T // 7 + 2)):             # rows straddle lanes and tiles
        ex = _example(rng, [(int(rng.integers(0, width + 2)), int(rng.integers(0, width + 2))) for _ in range(Wn)])
        for pad in ("right", "left"):
            want = _check(enc, ex, max_len=width, truncate="left", pad=pad, pad_id=-3, width=width)
            assert want[0].shape == (Wn, width)
        want = _check(enc, _example(rng, _window_pairs(rng, Wn, width)), max_len=width, truncation="window_second",
                      pad_id=-3, width=width)
        assert want[0].shape == (Wn, width)
    # the same with added ids: width 5 holds 3 ids of the pair
    ex = _example(rng, [(int(rng.integers(0, 4)), int(rng.integers(0, 4))) for _ in range((T + 1) // 5)])
    assert _check(enc, ex, max_len=5, bos=1, sep=(2,), width=5)[0].size == T + 1


def test_one_example_over_many_tiles(enc):
    T = _tile()
    rng = np.random.default_rng(6)
    # width 7 with one sep: B = 6, la = 2, C = 4, step 3: an example of 2 T / 7 + 40 windows fills more than
    # two tiles; short examples around it
    k = 2 * T // 7 + 40
    ex = _example(rng, [(3, 1), (0, 0), (2, 4 + (k - 1) * 3 - 1), (0, 0), (1, 9)])
    want = _check(enc, ex, max_len=7, truncation="window_second", stride=1, sep=(-6,), pad_id=-1)
    assert want[5].tolist() == [0, 1, 2, 2 + k, 3 + k, 5 + k] and k * 7 > 2 * T
    _check(enc, ex, max_len=9, truncation="window_second", stride=1, bos=5, sep=(-6,), eos=6, pad="left", width=11)
    # an emitted row wider than two tiles
    ex = _example(rng, [(10, 7), (2 * T, 3 * T), (T, 0)])
    want = _check(enc, ex, max_len=2 * T + 9, truncation="window_second", stride=100, max_first=T + 1)
    assert want[0].shape[1] == 2 * T + 9 and want[0].shape[0] > 3
    _check(enc, ex, max_len=2 * T + 9, truncate="left", eos=1)


def test_more_examples_in_a_tile_than_a_round_stages(enc):
    T, G = _tile(), _stage()
    rng = np.random.default_rng(7)
    # width 1: every emitted row is one entry; G + 5 examples of one id, then runs of examples that are empty on
    # both sides (one all-padding row each), an example of several windows in between, over three tiles
    pairs = [(0, 1)] * (G + 5) + [(0, 0)] * (G + 7) + [(0, 4)] + [(0, 0), (0, 1)] * 300 + [(0, 0)] * (2 * G + 9) + \
        [(0, 3)] + [(0, 1)] * T
    want = _check(enc, _example(rng, pairs), max_len=1, truncation="window_second", pad_id=-5)
    assert want[0].shape[1] == 1 and want[0].shape[0] == len(pairs) + 3 + 2 > 3 * T
    # the same shape under longest_first, ids on either side
    pairs = [(1, 0), (0, 1)] * (G // 2 + 3) + [(0, 0)] * (G + 7) + [(5, 5)] + [(0, 0)] * (G + 9) + [(1, 1)] * 9
    want = _check(enc, _example(rng, pairs), max_len=1, pad_id=-5)
    assert want[0].shape == (len(pairs), 1) and len(pairs) > 3 * G
    # width 2 with an eos: B == 1, an empty example is [eos, pad]
    pairs = [(0, 0)] * (G + 3) + [(2, 0)] + [(0, 0)] * (G + 3) + [(0, 1), (1, 0)] * 20 + [(5, 5)]
    ex = _example(rng, pairs)
    want = _check(enc, ex, max_len=2, eos=-4, pad_id=-5, width=2)
    assert want[0].shape[0] * 2 > T and want[0][0].tolist() == [-4, -5] and want[6][0].tolist() == [1, 0]
    _check(enc, ex, max_len=2, bos=-4, pad_id=-5, pad="left", width=3)
    # only empty examples and nothing added: width 0, and every example still has its row
    zero = np.zeros(G + 6, dtype=np.int64)
    none = np.zeros(0, np.int32)
    for kw in (dict(), dict(max_len=3, truncation="window_second", stride=2), dict(truncation="only_second")):
        want = _check(enc, (none, zero, none, zero), **kw)
        assert want[0].shape == (G + 5, 0) and want[2].tolist() == list(range(G + 5)) and not want[1].any()
    assert _check(enc, (none, zero, none, zero), width=2, pad_id=4)[0].tolist() == [[4, 4]] * (G + 5)


# ---- 5. output and argument forms ---------------------------------------------------------------

def test_rows_zero_and_no_mask(enc):
    none, zero = np.zeros(0, np.int32), np.zeros(1, np.int64)
    got = enc.pair_rows(none, zero, none, zero, max_len=4)
    assert got[0].shape == (0, 0) and got[3].shape == (0, 2) and got[5].tolist() == [0] and len(got) == 7
    _check(enc, (none, zero, none, zero), max_len=9, truncation="window_second", stride=1, bos=1, eos=2, width=6)
    rng = np.random.default_rng(8)
    ex = _example(rng, [(3, 4), (0, 2), (9, 9)])
    want = pair_ref.pairs(*ex, max_len=8, sep=(1,))
    _same(enc.pair_rows(*ex, max_len=8, sep=(1,)), want[:7], "no mask")
    _same(enc.pair_rows(*ex, max_len=8, sep=1, types=False), want[:6], "no types, a single sep id")
    _same(enc.pair_rows(*ex, max_len=8, sep=(1,), types=False, mask=True), want[:6] + want[7:], "mask only")
    with pytest.raises(ValueError, match="width"):
        enc.pair_rows(*ex, max_len=8, width=7)


def test_sizing_calls_write_nothing(enc):
    rng = np.random.default_rng(9)
    ex = _example(rng, [(0, 30), (3, 0), (2, 11), (0, 0), (4, 1)])
    kw = dict(max_len=10, stride=2, bos=1, sep=(3,), eos=2)  # B = 7
    want = pair_ref.pairs(*ex, truncation="window_second", **kw)
    Wn = want[0].shape[0]
    assert Wn == 6 + 1 + 3 + 1 + 1 and want[0].shape[1] == 10
    raw = dict(strategy=3, **kw)
    for args in (dict(width=10, null_out=True),            # out NULL
                 dict(width=9),                            # width too small
                 dict(width=10, cap=Wn * 10 - 1)):         # cap one short
        for r, widest, *bufs in _raw(enc, ex, out_size=Wn * 10, emitted=Wn, **args, **raw):
            assert r == Wn and widest == 10 and _untouched(*bufs), args
    for r, widest, out, types, mask, lengths, wrow, slen, ssrc, roww in _raw(enc, ex, 10, Wn * 10 + 9, Wn + 2, **raw):
        assert r == Wn and widest == 10
        for g, w in ((out, want[0]), (types, want[6]), (mask, want[7])):
            assert np.array_equal(g[:Wn * 10].reshape(Wn, 10), w) and _untouched(g[Wn * 10:])
        for g, w in ((lengths, want[1]), (wrow, want[2])):
            assert np.array_equal(g[:Wn], w) and _untouched(g[Wn:])
        for g, w in ((slen, want[3]), (ssrc, want[4])):
            assert np.array_equal(g[:2 * Wn].reshape(Wn, 2), w) and _untouched(g[2 * Wn:])
        assert np.array_equal(roww, want[5])
    # a width larger than needed
    for r, widest, out, *_ in _raw(enc, ex, 13, Wn * 13, Wn, **raw):
        assert r == Wn and widest == 10 and np.array_equal(out.reshape(Wn, 13), pair_ref.pairs(
            *ex, truncation="window_second", width=13, **kw)[0])


def test_device_views(enc):
    import torch
    from shredword.cbase import lib
    rng = np.random.default_rng(10)
    ex = _example(rng, [(int(rng.integers(0, 9)), int(rng.integers(0, 40))) for _ in range(300)])
    kw = dict(max_len=14, truncation="window_second", stride=3, max_first=5, bos=1, sep=(2, 3), pad_id=0, width=14)
    want = pair_ref.pairs(*ex, **kw)
    # inputs that are views of larger tensors
    d = [torch.cat([torch.zeros(3, dtype=t.dtype), t]).cuda()[3:] for t in map(torch.from_numpy, ex)]
    got = enc.pair_device(*d, mask=True, **kw)
    assert got[8] > 0
    _same([t.cpu().numpy() for t in got[:8]], want, "views")
    # outputs offset by one element: 4-byte but not 16-byte aligned (1 byte for types and mask), through the raw ABI
    Wn, W, R = want[0].shape[0], 14, 300
    big = torch.full((Wn * W + 1 + 8,), SENT, dtype=torch.int32, device="cuda")
    bt, bm = (torch.full((Wn * W + 1 + 8,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2))
    small = [torch.full((k * Wn + 2,), SENT, dtype=dt, device="cuda")
             for k, dt in ((1, torch.int32), (1, torch.int32), (2, torch.int32), (2, torch.int64))]
    roww = torch.full((R + 3,), SENT, dtype=torch.int64, device="cuda")
    assert big[1:].data_ptr() % 16 == 4 and bt[1:].data_ptr() % 4 == 1 and bm[1:].data_ptr() % 4 == 1
    bos, mid = ctypes.c_int32(1), (ctypes.c_int32 * 2)(2, 3)
    r = lib.shred_pair_device(enc.enc, d[0].data_ptr(), d[0].numel(), d[1].data_ptr(), d[2].data_ptr(), d[2].numel(),
                              d[3].data_ptr(), R, ctypes.byref(bos), mid, 2, None, 14, 0, 3, 5, 3, W, 0, 0,
                              big[1:].data_ptr(), Wn * W, bt[1:].data_ptr(), bm[1:].data_ptr(), small[0][1:].data_ptr(),
                              small[1][1:].data_ptr(), small[2][1:].data_ptr(), small[3][1:].data_ptr(),
                              roww[1:].data_ptr(), None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), None)
    assert r == Wn
    for t, w, s in ((big, want[0], SENT), (bt, want[6], 0xA5), (bm, want[7], 0xA5)):
        g = t.cpu().numpy()
        assert g[0] == s and np.array_equal(g[1:1 + Wn * W].reshape(Wn, W), w) and (g[1 + Wn * W:] == s).all()
    for t, w in zip(small, want[1:5]):
        t = t.cpu().numpy()
        assert t[0] == SENT and np.array_equal(t[1:1 + w.size], w.reshape(-1)) and t[1 + w.size] == SENT
    t = roww.cpu().numpy()
    assert t[0] == SENT and np.array_equal(t[1:R + 2], want[5]) and t[R + 2] == SENT
    # argument checks, as pad_device makes them
    for bad in ((d[0].cpu(), d[1], d[2], d[3]), (d[0], d[1], d[2], d[3].cpu()), (d[0].to(torch.int64), d[1], d[2], d[3]),
                (d[0], d[1], d[2], d[3].to(torch.int32)), (d[0], d[1][:0], d[2], d[3]), (d[0], d[1], d[2], d[3][:-1]),
                (d[0], None, d[2], d[3])):
        with pytest.raises(ValueError):
            enc.pair_device(*bad, max_len=10)


# ---- 6. malformed offset arrays -----------------------------------------------------------------

def test_malformed_row_offsets(enc):
    import torch
    rng = np.random.default_rng(11)
    n = 1000
    ids = rng.integers(0, 50_000, size=n).astype(np.int32)
    good = np.array([0, 400, 600, n], dtype=np.int64)
    for row in ([1, 500, 600, n],          # a first entry that is not 0
                [0, 500, 600, n - 1],      # a bad end point
                [0, 500, 600, n + 1],
                [0, 600, 599, n],          # a decreasing entry
                [0, -1, 5, n]):            # a negative entry
        row = np.array(row, dtype=np.int64)
        for ex in ((ids, row, ids, good), (ids, good, ids, row)):
            for strategy in (0, 3):
                for r, widest, *bufs in _raw(enc, ex, 64, 64 * 64, 64, max_len=64, strategy=strategy):
                    assert r == -6 and widest == 12345 and _untouched(*bufs), (row, strategy)
            with pytest.raises(ValueError, match="offsets"):
                enc.pair_rows(*ex, max_len=64)
            with pytest.raises(ValueError, match="offsets"):
                enc.pair_device(*[torch.from_numpy(x).cuda() for x in ex], max_len=64)
    _check(enc, (ids, good, ids, good), max_len=64, truncation="window_second", stride=8, max_first=16)  # still usable


# ---- 7. host pieces -----------------------------------------------------------------------------

def test_host_pieces_small(enc, monkeypatch):
    rng = np.random.default_rng(12)
    pairs = [(int(rng.integers(0, 30)), int(rng.integers(0, 200))) for _ in range(150)]
    pairs[40], pairs[41], pairs[90] = (0, 0), (25, 3000), (0, 0)   # one example longer than a piece of 999
    ex = _example(rng, pairs)
    monkeypatch.delenv("SHREDWORD_BATCH_PIECE", raising=False)
    for kw in (dict(max_len=40, truncation="window_second", stride=5, max_first=20, bos=1, sep=(2,), eos=3, pad="left",
                    pad_id=-1),
               dict(max_len=33, truncate="left", sep=(2, 2))):
        one = enc.pair_rows(*ex, mask=True, **kw)
        _same(one, pair_ref.pairs(*ex, **kw), "unpieced")
        for piece in ("1", "230", "999"):
            monkeypatch.setenv("SHREDWORD_BATCH_PIECE", piece)
            _same(enc.pair_rows(*ex, mask=True, **kw), one, piece)
        monkeypatch.delenv("SHREDWORD_BATCH_PIECE")


def test_host_pieces_under_the_real_budget(enc, monkeypatch):
    """Two examples of 2^23 + 1 ids each (a and b together): 2^24 + 2 ids, the fewest that the batch piece
    budget of 2^24 ids cuts into two pieces.  The rows are wide and cheap: only_first keeps 12 ids of a."""
    import torch
    monkeypatch.delenv("SHREDWORD_BATCH_PIECE", raising=False)
    half = (1 << 23) + 1
    la, lb = half - 4, 4
    assert 2 * (la + lb) == (1 << 24) + 2 and la + lb <= 1 << 24
    ids_a = np.arange(2 * la, dtype=np.int32)
    ids_b = -np.arange(1, 2 * lb + 1, dtype=np.int32)
    ex = (ids_a, _rows_of([la, la]), ids_b, _rows_of([lb, lb]))
    for kw in (dict(max_len=16, truncation="only_first"),
               dict(max_len=16, truncation="only_first", truncate="left", bos=5, sep=(6,), eos=7)):
        host = enc.pair_rows(*ex, mask=True, **kw)
        dev = enc.pair_device(*[torch.from_numpy(x).cuda() for x in ex], mask=True, **kw)
        _same(host, [t.cpu().numpy() for t in dev[:8]], kw)
    assert host[0].shape == (2, 16) and host[3].tolist() == [[9, 4], [9, 4]]
    assert host[0][1].tolist() == [5] + list(range(2 * la - 9, 2 * la)) + [6, -5, -6, -7, -8, 7]
    assert host[4].tolist() == [[la - 9, 0], [2 * la - 9, 4]]


# ---- 8. end to end ------------------------------------------------------------------------------

def test_encode_pairs_end_to_end(enc):
    qs = [b"abc ab", b"", b"c abcab", b"ab\nabc c", b"cab abc ab c"]
    ctx = [b"abcab cab abc ab ab c abc\nabc", b"ab abc", b"", b" \n ", b"abc abc abc abc ab ab ab c c c abcabc"]
    tok_len = enc.token_lengths
    BOS, SEP, EOS = 1000, 1001, 1002
    ids_a, ra = enc.encode_batch(qs)
    ids_b, rb = enc.encode_batch(ctx)
    assert np.diff(rb).max() > 10 and (np.diff(ra) == 0).sum() == 1
    for kw in (dict(max_len=9, truncation="window_second", stride=1, max_first=3),
               dict(max_len=8), dict(max_len=12, truncation="only_second", truncate="left")):
        kw.update(bos=BOS, sep=(SEP,), eos=EOS, pad_id=-1)
        got = enc.encode_pairs(qs, ctx, starts=True, mask=True, **kw)
        assert len(got) == 11 and got[8] >= 0
        arrays = [t.cpu().numpy() for t in got[:8]]
        _same(arrays, pair_ref.pairs(ids_a, ra, ids_b, rb, **kw), kw)
        assert len(enc.encode_pairs(qs, ctx, **kw)) == 8
        batch, lengths, prow, slen, ssrc, roww, types, mask = arrays
        starts = [t.cpu().numpy() for t in got[9:]]
        assert roww[-1] == batch.shape[0] >= len(qs) and roww.size == len(qs) + 1
        for w in range(batch.shape[0]):
            e, (ka, kb) = int(lengths[w]), slen[w]
            assert batch[w, 0] == BOS and batch[w, 1 + ka] == SEP and batch[w, e - 1] == EOS and e == 3 + ka + kb
            assert (batch[w, e:] == -1).all() and roww[prow[w]] <= w < roww[prow[w] + 1]
            for side, first, count, texts, ids, row in ((0, 1, ka, qs, ids_a, ra), (1, 2 + ka, kb, ctx, ids_b, rb)):
                text = b"".join(texts)
                for c in range(first, first + count):  # every kept token: its bytes are where starts says
                    k = int(ssrc[w, side]) + c - first
                    tok = int(batch[w, c])
                    assert tok == ids[k] and row[prow[w]] <= k < row[prow[w] + 1] and types[w, c] == side
                    assert text[starts[side][k]:starts[side][k] + tok_len[tok]] == enc.decode([tok])
    with pytest.raises(ValueError):
        enc.encode_pairs(qs, ctx[:-1])


# ---- 9. the identities the shared expansion rests on ---------------------------------------------

def _short_rows(rng):
    """BATCH_STAGE + 5 rows of 0 to 3 ids, with runs of empty rows."""
    lens = rng.integers(0, 4, size=_stage() + 5)
    lens[10:45] = 0
    lens[300:302] = 0
    return lens


def _offset(n, dt, fill):
    """A device buffer of n + 1 + 8 elements, to be written from element 1 on."""
    import torch
    return torch.full((n + 1 + 8,), fill, dtype=dt, device="cuda")


def _inside(buf, Wn, W, fill):
    """The [Wn, W] array written from element 1 of an _offset buffer; nothing else was touched."""
    g = buf.cpu().numpy()
    assert g[0] == fill and (g[1 + Wn * W:] == fill).all()
    return g[1:1 + Wn * W].reshape(Wn, W)


def test_window_is_a_pair_with_an_empty_first_row(enc):
    """window_device == pair_device(truncation="window_second") on examples whose first rows are empty."""
    import torch
    from shredword.cbase import lib
    rng = np.random.default_rng(21)
    lens = np.concatenate([_short_rows(rng), [3 * _tile() + 1]])
    row = _rows_of(lens)
    R, added, M, S, W = lens.size, 2, 9, 2, 11
    ids = torch.from_numpy(rng.integers(0, 50_000, size=int(row[-1])).astype(np.int32)).cuda()
    row = torch.from_numpy(row).cuda()
    ids_a, row_a = torch.empty(0, dtype=torch.int32, device="cuda"), torch.zeros(R + 1, dtype=torch.int64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bos, eos = ctypes.c_int32(1), ctypes.c_int32(2)
    for side, pad in enumerate(("right", "left")):
        kw = dict(max_len=M, stride=S, bos=1, eos=2, pad=pad, pad_id=-1, width=W, mask=True)
        win = [t.cpu().numpy() for t in enc.window_device(ids, row, **kw)[:6]]
        par = [t.cpu().numpy() for t in enc.pair_device(ids_a, row_a, ids, row, truncation="window_second", sep=(), **kw)[:8]]
        batch, lengths, wrow, wsrc, roww, mask = win
        Wn = batch.shape[0]
        assert Wn > R + 3 * _tile() // M and lengths.min() == added and lengths.max() == M
        for name, a, b in (("batch", batch, par[0]), ("lengths", lengths, par[1]), ("rows", wrow, par[2]),
                           ("row_windows", roww, par[5]), ("mask", mask, par[7])):
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, pad)
        assert np.array_equal(par[4][:, 1], wsrc) and (par[3][:, 0] == 0).all()
        assert np.array_equal(par[3][:, 1], lengths - added)
        types = mask.copy()
        types[np.arange(Wn), W - lengths if side else 0] = 0  # the bos column
        assert np.array_equal(par[6], types), pad
        # both into views offset by one element (the scalar stores), through the raw ABI
        wb, wm = _offset(Wn * W, torch.int32, SENT), _offset(Wn * W, torch.uint8, 0xA5)
        pb, pt, pm = _offset(Wn * W, torch.int32, SENT), _offset(Wn * W, torch.uint8, 0xA5), _offset(Wn * W, torch.uint8, 0xA5)
        assert wb[1:].data_ptr() % 16 == 4 and pb[1:].data_ptr() % 16 == 4
        assert all(t[1:].data_ptr() % 4 == 1 for t in (wm, pt, pm))
        r = lib.shred_window_device(enc.enc, ids.data_ptr(), ids.numel(), row.data_ptr(), R, ctypes.byref(bos),
                                    ctypes.byref(eos), M, S, W, -1, side, wb[1:].data_ptr(), Wn * W, None, wm[1:].data_ptr(),
                                    None, None, None, None, st, None)
        assert r == Wn
        r = lib.shred_pair_device(enc.enc, ids_a.data_ptr(), 0, row_a.data_ptr(), ids.data_ptr(), ids.numel(),
                                  row.data_ptr(), R, ctypes.byref(bos), None, 0, ctypes.byref(eos), M, 0, 3, 0, S, W, -1, side,
                                  pb[1:].data_ptr(), Wn * W, pt[1:].data_ptr(), pm[1:].data_ptr(), None, None, None, None,
                                  None, None, st, None)
        assert r == Wn
        assert np.array_equal(_inside(wb, Wn, W, SENT), batch) and np.array_equal(_inside(pb, Wn, W, SENT), batch)
        assert np.array_equal(_inside(wm, Wn, W, 0xA5), mask) and np.array_equal(_inside(pm, Wn, W, 0xA5), mask)
        assert np.array_equal(_inside(pt, Wn, W, 0xA5), types)


def test_pad_is_a_window_of_rows_that_fit(enc):
    """pad_device(max_len=M) == window_device(max_len=M, stride=0) on rows none longer than M - added."""
    import torch
    rng = np.random.default_rng(22)
    lens = _short_rows(rng)
    row = _rows_of(lens)
    ids = torch.from_numpy(rng.integers(0, 50_000, size=int(row[-1])).astype(np.int32)).cuda()
    row = torch.from_numpy(row).cuda()
    for pad in ("right", "left"):
        kw = dict(max_len=6, bos=1, eos=2, pad=pad, pad_id=-1, mask=True)
        assert lens.max() <= 6 - 2
        p = [t.cpu().numpy() for t in enc.pad_device(ids, row, **kw)[:3]]
        w = [t.cpu().numpy() for t in enc.window_device(ids, row, stride=0, **kw)[:6]]
        assert p[0].shape == (lens.size, 5)
        for name, a, b in (("batch", p[0], w[0]), ("lengths", p[1], w[1]), ("mask", p[2], w[5])):
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, pad)
        assert np.array_equal(w[2], np.arange(lens.size))
