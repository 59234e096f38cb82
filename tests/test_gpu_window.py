"""GPU tests of the windowing pass (include/shredword_encode.h: shred_window_device /
shred_window_rows; BPEEncoder.window_rows / window_device / encode_windows).

The expected arrays come from window_ref.py: a plain Python loop that steps a start index through
every row (test_window_ref_cpu.py checks that loop against the header's formula).  Every case runs
through both ABIs (host arrays in pieces, device tensors) and all six arrays are compared exactly.

Cases: the row lengths around C and C + step for strides 0, 1 and C - 1 and 0, 1 or 2 added ids,
down to max_len = add + 1; output sizes on the tile boundary (BATCH_TILE - 1, + 0, + 1) with widths
that are no multiple of a lane's 4 entries; one row whose windows fill more than two tiles; more
rows in a tile than one LDS round stages (BATCH_STAGE), with runs of empty rows; pad="left",
row_offsets=None and rows == 0; the sizing calls and the argument errors on sentinel-filled
buffers; malformed row offsets; host rows cut into pieces; device views and an output that is only
4-byte aligned; encode_windows end to end with the byte offsets of every kept token.

Not tested: a Wn * width that does not fit its type (checked by reading).
"""
import ctypes

import numpy as np
import pytest

import window_ref

pytestmark = pytest.mark.gpu

SENT = -77  # fills outputs that a call must leave alone
NAMES = ("batch", "lengths", "window_rows", "window_src", "row_windows", "mask")


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


def _ids(rng, n):
    return rng.integers(0, 50_000, size=n).astype(np.int32)


def _same(got, want, where):
    assert len(got) == len(want)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, where)


def _check(enc, ids, row=None, **kw):
    """window_rows and window_device against the Python loop; returns the loop's arrays."""
    import torch
    ids = np.asarray(ids, dtype=np.int32)
    row = None if row is None else np.asarray(row, dtype=np.int64)
    want = window_ref.windows(ids, row, **kw)
    _same(enc.window_rows(ids, row, mask=True, **kw), want, ("host", kw))
    d_ids = torch.from_numpy(ids).cuda()
    d_row = None if row is None else torch.from_numpy(row).cuda()
    dev = enc.window_device(d_ids, d_row, mask=True, **kw)
    assert len(dev) == 7 and dev[6] >= 0
    assert [t.dtype for t in dev[:6]] == [torch.int32, torch.int32, torch.int32, torch.int64, torch.int64, torch.uint8]
    _same([t.cpu().numpy() for t in dev[:6]], want, ("device", kw))
    _same(enc.window_rows(ids, row, **kw), want[:5], ("host, no mask", kw))
    return want


# ---- the raw ABI --------------------------------------------------------------------------------

def _ptr(v):
    return None if v is None else ctypes.byref(ctypes.c_int32(v))


def _raw(enc, ids, row, max_len, stride, width, out_size, windows, cap=None, null_out=False, bos=None, eos=None):
    """Both ABIs on sentinel-filled buffers -> [(result, widest, out, lengths, mask, win_row, win_src, row_win)]."""
    import torch
    from shredword.cbase import lib
    ids = np.asarray(ids, dtype=np.int32)
    row = None if row is None else np.asarray(row, dtype=np.int64)
    R = 1 if row is None else row.size - 1
    cap = out_size if cap is None else cap
    head = (_ptr(bos), _ptr(eos), max_len, stride, width, 0, 0)
    shapes = ((out_size, np.int32), (windows, np.int32), (out_size, np.uint8), (windows, np.int32),
              (windows, np.int64), (R + 1, np.int64))
    fill = lambda dt: 0xA5 if dt == np.uint8 else SENT
    res = []
    for device in (False, True):
        bufs = [np.full(max(k, 1), fill(dt), dtype=dt) for k, dt in shapes]
        widest = ctypes.c_size_t(12345)
        if device:
            bufs = [torch.from_numpy(b).cuda() for b in bufs]
            d_ids = torch.from_numpy(ids).cuda()
            d_row = None if row is None else torch.from_numpy(row).cuda()
            p = [b.data_ptr() for b in bufs]
            r = lib.shred_window_device(enc.enc, d_ids.data_ptr(), ids.size, None if row is None else d_row.data_ptr(),
                                        0 if row is None else R, *head, None if null_out else p[0], cap, p[1], p[2],
                                        p[3], p[4], p[5], ctypes.byref(widest),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), None)
            bufs = [b.cpu().numpy() for b in bufs]
        else:
            p = [b.ctypes.data for b in bufs]
            r = lib.shred_window_rows(enc.enc, ids.ctypes.data, ids.size, None if row is None else row.ctypes.data,
                                      0 if row is None else R, *head, None if null_out else p[0], cap, p[1], p[2],
                                      p[3], p[4], p[5], ctypes.byref(widest))
        res.append((r, widest.value, *bufs))
    return res


def _untouched(*arrays):
    return all((a == (0xA5 if a.dtype == np.uint8 else SENT)).all() for a in arrays)


# ---- 1. row lengths, strides, added ids ---------------------------------------------------------

def test_lengths_strides_and_added_ids(enc):
    rng = np.random.default_rng(1)
    for bos, eos in ((None, None), (7, None), (None, -8), (2 ** 31 - 1, -2 ** 31)):
        add = (bos is not None) + (eos is not None)
        for C in (1, 2, 5):  # C == 1: the smallest window, max_len = add + 1
            for stride in sorted({0, 1, C - 1} & set(range(C))):
                step = C - stride
                lens = [n for n in (0, 1, C - 1, C, C + 1, C + step - 1, C + step, C + step + 1, 3 * C + 2 * step + 1)
                        if n >= 0]
                row = _rows_of(lens)
                ids = _ids(rng, int(row[-1]))
                kw = dict(max_len=add + C, stride=stride, bos=bos, eos=eos, pad_id=-9)
                want = _check(enc, ids, row, **kw)
                assert want[0].shape[1] == add + C and want[1].max() == add + C
                _check(enc, ids, row, pad="left", width=add + C + 3, **kw)


# ---- 2. tile edges ------------------------------------------------------------------------------

def _lens_with_windows(rng, total, C, step):
    """Row lengths whose windows number exactly `total`: a row of k windows holds C + (k - 2) * step + 1 ..
    C + (k - 1) * step ids (k == 1: 0 .. C)."""
    lens = []
    while total:
        k = int(min(total, rng.integers(1, 6)))
        lens.append(int(rng.integers(0, C + 1)) if k == 1 else C + (k - 1) * step - int(rng.integers(0, step)))
        total -= k
    return lens


def test_tile_edges(enc):
    T = _tile()
    rng = np.random.default_rng(2)
    assert (T - 1) % 3 == 0 and (T + 1) % 5 == 0
    for width, Wn in ((3, (T - 1) // 3), (4, T // 4), (5, (T + 1) // 5),   # Wn * width == T - 1, T, T + 1
                      (1, T - 1), (1, T), (1, T + 1),
                      (3, 2 * T // 3 + 1), (7, 3 * T // 7 + 2)):             # windows straddle lanes and tiles
        for stride in sorted({0, 1, width - 1} & set(range(width))):
            lens = _lens_with_windows(rng, Wn, width, width - stride)
            row = _rows_of(lens)
            ids = _ids(rng, int(row[-1]))
            for pad in ("right", "left"):
                want = _check(enc, ids, row, max_len=width, stride=stride, pad=pad, pad_id=-3, width=width)
                assert want[0].shape == (Wn, width)
    # the same with a bos: width 5 holds 4 ids of the row
    lens = _lens_with_windows(rng, (T + 1) // 5, 4, 3)
    ids = _ids(rng, sum(lens))
    assert _check(enc, ids, _rows_of(lens), max_len=5, stride=1, bos=1)[0].size == T + 1


def test_one_row_over_many_tiles(enc):
    T = _tile()
    rng = np.random.default_rng(3)
    # width 7, step 4: a row of 2 T / 7 + 40 windows fills more than two tiles; short rows around it
    k = 2 * T // 7 + 40
    lens = [3, 0, 7 + (k - 1) * 4 - 2, 0, 9]
    ids = _ids(rng, sum(lens))
    want = _check(enc, ids, _rows_of(lens), max_len=7, stride=3, pad_id=-1)
    assert want[4].tolist() == [0, 1, 2, 2 + k, 3 + k, 5 + k] and k * 7 > 2 * T
    _check(enc, ids, _rows_of(lens), max_len=7, stride=3, bos=5, eos=6, pad="left", width=11)
    _check(enc, ids, None, max_len=6, stride=5)  # step 1: one window per id, all of one row
    # a window wider than two tiles
    ids = _ids(rng, 5 * T)
    want = _check(enc, ids, _rows_of([10, 5 * T - 10]), max_len=2 * T + 9, stride=100)
    assert want[0].shape == (4, 2 * T + 9)


def test_more_rows_in_a_tile_than_a_round_stages(enc):
    T, G = _tile(), _stage()
    rng = np.random.default_rng(4)
    # width 1: every window is one entry; G + 5 rows of one id, then runs of empty rows (one all-padding
    # window each), a row of several windows in between, over three tiles
    lens = [1] * (G + 5) + [0] * (G + 7) + [4] + [0, 1] * 300 + [0] * (2 * G + 9) + [3] + [1] * T
    ids = _ids(rng, sum(lens))
    want = _check(enc, ids, _rows_of(lens), max_len=1, pad_id=-5)
    assert want[0].shape[1] == 1 and want[0].shape[0] == len(lens) + 3 + 2 > 3 * T
    # width 2 with an eos: C == 1, an empty row is [eos, pad]
    lens = [0] * (G + 3) + [2] + [0] * (G + 3) + [1] * 40 + [5]
    ids = _ids(rng, sum(lens))
    want = _check(enc, ids, _rows_of(lens), max_len=2, eos=-4, pad_id=-5, width=2)
    assert want[0].shape[0] * 2 > T and want[0][0].tolist() == [-4, -5]
    _check(enc, ids, _rows_of(lens), max_len=2, bos=-4, pad_id=-5, pad="left", width=3)
    # only empty rows and nothing added: width 0, and every row still has its window
    row = np.zeros(G + 6, dtype=np.int64)
    want = _check(enc, np.zeros(0, np.int32), row, max_len=3, stride=2)
    assert want[0].shape == (G + 5, 0) and want[2].tolist() == list(range(G + 5)) and not want[1].any()
    assert _check(enc, np.zeros(0, np.int32), row, max_len=3, width=2, pad_id=4)[0].tolist() == [[4, 4]] * (G + 5)


# ---- 3. input forms -----------------------------------------------------------------------------

def test_input_forms(enc):
    rng = np.random.default_rng(5)
    none = np.zeros(0, np.int32)
    # rows == 0
    got = enc.window_rows(none, [0], max_len=4)
    assert got[0].shape == (0, 0) and [g.size for g in got[1:4]] == [0, 0, 0] and got[4].tolist() == [0]
    _check(enc, none, [0], max_len=4, stride=1, bos=1, eos=2, width=6)
    # row_offsets = None: one row
    ids = _ids(rng, 37)
    assert _check(enc, ids, max_len=10, stride=3)[4].tolist() == [0, 5]
    assert _check(enc, ids, max_len=40)[0].shape == (1, 37)
    assert _check(enc, ids, max_len=12, stride=2, bos=-5, eos=7, pad="left", width=13, pad_id=3)[0].shape == (5, 13)
    assert _check(enc, none, max_len=2)[0].shape == (1, 0)
    assert _check(enc, none, max_len=2, eos=3)[0].tolist() == [[3]]
    # empty rows between rows of ids
    _check(enc, ids, [0, 0, 0, 37, 37], max_len=8, stride=6, eos=0)
    with pytest.raises(TypeError):
        enc.window_rows(ids)  # max_len is required
    with pytest.raises(ValueError, match="width"):
        enc.window_rows(ids, max_len=10, width=9)
    with pytest.raises(ValueError):
        enc.window_rows(ids, max_len=10, pad="centre")
    with pytest.raises(ValueError):
        enc.window_rows(ids, [], max_len=10)


# ---- 4. sizing calls and argument errors --------------------------------------------------------

def test_sizing_calls_write_nothing(enc):
    rng = np.random.default_rng(6)
    lens = [0, 30, 3, 11, 0, 1]
    row = _rows_of(lens)
    ids = _ids(rng, sum(lens))
    want = window_ref.windows(ids, row, max_len=8, stride=2, bos=1, eos=2)  # C = 6, step = 4
    Wn = want[0].shape[0]
    assert Wn == 1 + 7 + 1 + 3 + 1 + 1 and want[0].shape[1] == 8
    kw = dict(bos=1, eos=2)
    for args in (dict(width=8, null_out=True),             # out NULL
                 dict(width=7),                            # width too small
                 dict(width=8, cap=Wn * 8 - 1)):           # cap one short
        for r, widest, *bufs in _raw(enc, ids, row, 8, 2, out_size=Wn * 8, windows=Wn, **args, **kw):
            assert r == Wn and widest == 8 and _untouched(*bufs), args
    for r, widest, out, lengths, mask, wrow, wsrc, roww in _raw(enc, ids, row, 8, 2, 8, Wn * 8 + 9, Wn + 2, **kw):
        assert r == Wn and widest == 8
        assert np.array_equal(out[:Wn * 8].reshape(Wn, 8), want[0]) and _untouched(out[Wn * 8:])
        assert np.array_equal(mask[:Wn * 8].reshape(Wn, 8), want[5]) and _untouched(mask[Wn * 8:])
        for g, w in ((lengths, want[1]), (wrow, want[2]), (wsrc, want[3])):
            assert np.array_equal(g[:Wn], w) and _untouched(g[Wn:])
        assert np.array_equal(roww, want[4])
    # a width larger than needed
    for r, widest, out, *_ in _raw(enc, ids, row, 8, 2, 11, Wn * 11, Wn, **kw):
        assert r == Wn and widest == 8 and np.array_equal(out.reshape(Wn, 11), window_ref.windows(
            ids, row, max_len=8, stride=2, bos=1, eos=2, width=11)[0])


def test_argument_errors(enc):
    rng = np.random.default_rng(7)
    row = _rows_of([4, 9, 0])
    ids = _ids(rng, 13)
    for max_len, stride, kw in ((4, 4, {}), (4, 5, {}),                       # stride >= C
                                (6, 4, dict(bos=1, eos=2)), (5, 4, dict(eos=2)),
                                (2, 0, dict(bos=1, eos=2)), (1, 0, dict(bos=1)),  # max_len <= add
                                (1, 0, dict(bos=1, eos=2)), (0, 0, dict(eos=1)),
                                (0, 0, {}),                                   # max_len == 0
                                (2 ** 31, 0, {}),                             # max_len past int32
                                (4, -1, {})):                                 # a negative stride
        with pytest.raises(ValueError):
            enc.window_rows(ids, row, max_len=max_len, stride=stride, **kw)
        with pytest.raises(ValueError):
            enc.encode_windows(b"ab abc", max_len=max_len, stride=stride, **kw)
        raw_stride = stride if stride >= 0 else 2 ** 64 - 1   # what a negative stride is to a size_t
        for r, widest, *bufs in _raw(enc, ids, row, max_len, raw_stride, 16, 16 * 16, 16, **kw):
            assert r == -1 and widest == 12345 and _untouched(*bufs), (max_len, stride, kw)
    for bad in (dict(bos=2 ** 31), dict(pad_id=-2 ** 31 - 1)):
        with pytest.raises(ValueError):
            enc.window_rows(ids, row, max_len=4, **bad)
    _check(enc, ids, row, max_len=4, stride=3)  # the largest stride that is allowed


# ---- 5. malformed row offsets -------------------------------------------------------------------

def test_malformed_row_offsets(enc):
    import torch
    rng = np.random.default_rng(8)
    n = 1000
    ids = _ids(rng, n)
    for row in ([1, 500, n],            # a first entry that is not 0
                [0, 500, n - 1],        # a last entry that is not n
                [0, 500, n + 1],
                [0, 600, 599, n],       # a decreasing pair
                [0, -1, n],             # a negative entry
                [-1, 500, n],
                [0, n + 5, n]):         # out of range
        for r, widest, *bufs in _raw(enc, ids, row, 64, 8, 64, 64 * 64, 64):
            assert r == -6 and widest == 12345 and _untouched(*bufs), row
        d_ids, d_row = torch.from_numpy(ids).cuda(), torch.tensor(row, dtype=torch.int64).cuda()
        with pytest.raises(ValueError, match="row_offsets"):
            enc.window_rows(ids, row, max_len=64, stride=8)
        with pytest.raises(ValueError, match="row_offsets"):
            enc.window_device(d_ids, d_row, max_len=64, stride=8)
    _check(enc, ids, [0, 500, n], max_len=64, stride=8)  # the encoder is still usable


# ---- 6. host pieces -----------------------------------------------------------------------------

def test_host_pieces(enc, monkeypatch):
    rng = np.random.default_rng(9)
    n = 40_000
    ends = set(int(x) for x in rng.choice(np.arange(1, n), size=n // 300, replace=False))
    ends = {e for e in ends if not 20_000 < e < 23_500}          # one row longer than a piece of 1001
    ends |= {999, 1001, 2000, 2002, 7000, 13013, 39000}          # rows that end exactly on piece cuts
    empties = [999, 2000, 2002, 13013, n]                        # empty rows on the cuts
    row = np.array([0] + sorted(list(ends) + empties + [n]), dtype=np.int64)
    lens = np.diff(row)
    assert lens.max() > 3000 and (lens == 0).sum() == 5 and lens.size > 100
    ids = _ids(rng, n)
    kw = dict(max_len=130, stride=32, bos=1, eos=2, pad="left", pad_id=-1)
    monkeypatch.delenv("SHREDWORD_BATCH_PIECE", raising=False)
    one = enc.window_rows(ids, row, mask=True, **kw)
    flat = enc.window_rows(ids, None, mask=True, **kw)
    _same(one, window_ref.windows(ids, row, **kw), "unpieced")
    _same(flat, window_ref.windows(ids, None, **kw), "unpieced, one row")
    for piece in ("1", "999", "1001"):
        monkeypatch.setenv("SHREDWORD_BATCH_PIECE", piece)
        _same(enc.window_rows(ids, row, mask=True, **kw), one, piece)
        _same(enc.window_rows(ids, None, mask=True, **kw), flat, piece)


# ---- 7. views -----------------------------------------------------------------------------------

def test_device_views(enc):
    import torch
    from shredword.cbase import lib
    rng = np.random.default_rng(10)
    text = b"".join(bytes(rng.choice([97, 98, 99], size=int(rng.integers(1, 9))).astype(np.uint8)) +
                    bytes([int(rng.choice([10, 32, 32, 32, 32, 32, 32]))]) for _ in range(3000)) + b"abc"
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    ids, _, line, _ = enc.encode_spans_device(d_text)  # views of larger tensors, as they are
    h_ids, h_line = ids.cpu().numpy(), line.cpu().numpy()
    assert np.diff(h_line).max() > 30
    want = window_ref.windows(h_ids, h_line, max_len=10, stride=3, eos=0)
    got = enc.window_device(ids, line, max_len=10, stride=3, eos=0, mask=True)
    assert got[6] > 0
    _same([t.cpu().numpy() for t in got[:6]], want, "views")
    # outputs offset by one element: 4-byte but not 16-byte aligned (1 byte for the mask), through the raw ABI
    Wn, W, R = want[0].shape[0], 10, h_line.size - 1
    big = torch.full((Wn * W + 1 + 8,), SENT, dtype=torch.int32, device="cuda")
    bm = torch.full((Wn * W + 1 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    small = [torch.full((Wn + 2,), SENT, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.int64)]
    roww = torch.full((R + 3,), SENT, dtype=torch.int64, device="cuda")
    assert big[1:].data_ptr() % 16 == 4 and bm[1:].data_ptr() % 4 == 1
    eos = ctypes.c_int32(0)
    r = lib.shred_window_device(enc.enc, ids.data_ptr(), ids.numel(), line.data_ptr(), R, None, ctypes.byref(eos), 10, 3,
                                W, 0, 0, big[1:].data_ptr(), Wn * W, small[0][1:].data_ptr(), bm[1:].data_ptr(),
                                small[1][1:].data_ptr(), small[2][1:].data_ptr(), roww[1:].data_ptr(), None,
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), None)
    assert r == Wn
    g, gm = big.cpu().numpy(), bm.cpu().numpy()
    assert g[0] == SENT and np.array_equal(g[1:1 + Wn * W].reshape(Wn, W), want[0]) and (g[1 + Wn * W:] == SENT).all()
    assert gm[0] == 0xA5 and np.array_equal(gm[1:1 + Wn * W].reshape(Wn, W), want[5]) and (gm[1 + Wn * W:] == 0xA5).all()
    for t, w in zip(small, want[1:4]):
        t = t.cpu().numpy()
        assert t[0] == SENT and np.array_equal(t[1:1 + Wn], w) and t[1 + Wn] == SENT
    t = roww.cpu().numpy()
    assert t[0] == SENT and np.array_equal(t[1:R + 2], want[4]) and t[R + 2] == SENT
    # argument checks, as pad_device makes them
    for bad in ((ids.cpu(), line), (ids, line.cpu()), (ids.to(torch.int64), line), (ids, line.to(torch.int32)),
                (ids, line[:0])):
        with pytest.raises(ValueError):
            enc.window_device(*bad, max_len=10)
    enc.device += 1  # the tensors are now on another device than the encoder
    try:
        with pytest.raises(ValueError, match="is on"):
            enc.window_device(ids, line, max_len=10)
    finally:
        enc.device -= 1


# ---- 8. end to end ------------------------------------------------------------------------------

def test_encode_windows_end_to_end(enc):
    rng = np.random.default_rng(11)
    docs = [b"", b"abc ab\nabcab c", b" \n ", b"cab"]
    docs += [b" ".join(bytes(rng.choice([97, 98, 99], size=int(rng.integers(1, 7))).astype(np.uint8))
                       for _ in range(int(k))) for k in (40, 3, 90)]
    from shredword.encoder import join_docs
    buf, off = join_docs(docs)
    text = buf.tobytes()
    ids, row, starts = enc.encode_docs(buf, off, starts=True)
    assert np.diff(row).max() > 60 and (np.diff(row) == 0).sum() == 2
    tok_len = enc.token_lengths
    BOS, EOS = 1000, 1001
    kw = dict(max_len=16, stride=5, bos=BOS, eos=EOS, pad_id=-1)
    got = enc.encode_windows(buf, doc_offsets=off, mask=True, **kw)
    _same(got, window_ref.windows(ids, row, **kw), "doc_offsets")
    _same(enc.encode_windows(docs, mask=True, **kw), got, "a list of documents")
    batch, lengths, wrow, wsrc, roww, mask = got
    assert roww[-1] == batch.shape[0] > len(docs) and roww.size == len(docs) + 1
    for w in range(batch.shape[0]):
        e = int(lengths[w])
        assert batch[w, 0] == BOS and batch[w, e - 1] == EOS and (batch[w, e:] == -1).all()
        assert roww[wrow[w]] <= w < roww[wrow[w] + 1]
        for c in range(1, e - 1):  # every kept token: its bytes are where starts says
            k = int(wsrc[w]) + c - 1
            tok = int(batch[w, c])
            assert tok == ids[k] and row[wrow[w]] <= k < row[wrow[w] + 1]
            assert text[starts[k]:starts[k] + tok_len[tok]] == enc.decode([tok])
    # rows that are lines
    lines_ids, line = enc.encode_lines(text)
    _same(enc.encode_windows(text, max_len=7, stride=2), window_ref.windows(lines_ids, line, max_len=7, stride=2)[:5],
          "lines")
