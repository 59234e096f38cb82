"""GPU tests of the batcher (include/shredword_encode.h: shred_pad_device / shred_pad_rows /
shred_pack_device / shred_pack_rows; BPEEncoder.pad_rows / pack_rows / pad_device / pack_device /
encode_padded / encode_packed).

The expected arrays come by another route than the kernels take: a plain Python loop over the rows
builds each emitted row as a list ([bos] + kept ids + [eos]), and the batch, the stream, the
positions, the segments and the row starts are made from those lists (list lengths, no prefix
sums).  Every case runs through both ABIs (host arrays in pieces, device tensors) and every returned
array is compared exactly.

Cases: degenerate inputs; every option; pad and pack sizes on the output-tile boundary (BATCH_TILE - 1,
+ 0, + 1) with rows that straddle a lane's 4 entries, rows longer than two tiles, more rows in a
tile than one LDS round stages (BATCH_STAGE), runs of rows that emit nothing; positions and segments;
malformed row offsets; host rows cut into pieces; device views and an output that is only 4-byte
aligned; a golden end to end.

Not tested: an e_r, rows * width or S * L that does not fit its type (checked by reading), and the
device footprint (see test_gpu_decode.py).
"""
import ctypes

import numpy as np
import pytest

from encode_ref import model_merges

pytestmark = pytest.mark.gpu

SENT = -77  # fills outputs that a call must leave alone


def _tile():
    from shredword.encoder import BATCH_TILE
    return BATCH_TILE


def _stage():
    from shredword.encoder import BATCH_STAGE
    return BATCH_STAGE


@pytest.fixture(scope="module")
def enc():
    from shredword.encoder import BPEEncoder
    with BPEEncoder.from_merges([[97, 98, 256], [256, 99, 257]]) as e:  # the batcher never reads the vocabulary
        yield e


# ---- the Python loop ----------------------------------------------------------------------------

def _emitted(ids, row, bos=None, eos=None, max_len=None, truncate="right"):
    """The emitted rows as lists."""
    ids = [int(x) for x in ids]
    bounds = [(0, len(ids))] if row is None else [(int(a), int(b)) for a, b in zip(row[:-1], row[1:])]
    add = (bos is not None) + (eos is not None)
    out = []
    for a, b in bounds:
        kept = ids[a:b]
        if max_len:
            k = max_len - add
            kept = kept[:k] if truncate == "right" else kept[max(len(kept) - k, 0):]
        out.append(([bos] if bos is not None else []) + kept + ([eos] if eos is not None else []))
    return out


def _want_pad(em, pad_id=0, pad="right", width=None):
    W = max([len(e) for e in em], default=0) if width is None else width
    batch, mask = [], []
    for e in em:
        fill = [pad_id] * (W - len(e))
        batch.append(e + fill if pad == "right" else fill + e)
        mask.append([1] * len(e) + [0] * len(fill) if pad == "right" else [0] * len(fill) + [1] * len(e))
    return (np.array(batch, dtype=np.int32).reshape(len(em), W), np.array([len(e) for e in em], dtype=np.int32),
            np.array(mask, dtype=np.uint8).reshape(len(em), W))


def _want_pack(em, seq_len, pad_id=0, drop_last=False):
    stream, pos, seg, start = [], [], [], [0]
    for r, e in enumerate(em):
        stream += e
        pos += list(range(len(e)))
        seg += [r] * len(e)
        start.append(len(stream))
    T = len(stream)
    S = T // seq_len if drop_last else -(-T // seq_len)
    tail = max(S * seq_len - T, 0)
    cut = lambda v, fill: np.array((v + [fill] * tail)[:S * seq_len], dtype=np.int32).reshape(S, seq_len)
    return cut(stream, pad_id), np.array(start, dtype=np.int64), cut(pos, 0), cut(seg, -1)


def _split(kw, names):
    return {k: v for k, v in kw.items() if k in names}


EMIT = ("bos", "eos", "max_len", "truncate")


def _check_pad(enc, ids, row=None, **kw):
    """pad_rows and pad_device against the Python loop; returns the batch."""
    import torch
    ids = np.asarray(ids, dtype=np.int32)
    row = None if row is None else np.asarray(row, dtype=np.int64)
    want = _want_pad(_emitted(ids, row, **_split(kw, EMIT)), **_split(kw, ("pad_id", "pad", "width")))
    got = enc.pad_rows(ids, row, mask=True, **kw)
    d_ids = torch.from_numpy(ids).cuda()
    d_row = None if row is None else torch.from_numpy(row).cuda()
    dev = enc.pad_device(d_ids, d_row, mask=True, **kw)
    assert len(got) == 3 and len(dev) == 4 and dev[3] >= 0
    assert [t.dtype for t in dev[:3]] == [torch.int32, torch.int32, torch.uint8]
    for name, w, g, d in zip(("batch", "lengths", "mask"), want, got, dev):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, "host", kw)
        d = d.cpu().numpy()
        assert d.shape == w.shape and np.array_equal(d, w), (name, "device", kw)
    two = enc.pad_rows(ids, row, **kw)  # without the mask
    assert len(two) == 2 and np.array_equal(two[0], want[0]) and np.array_equal(two[1], want[1])
    return got[0]


def _check_pack(enc, ids, row=None, **kw):
    """pack_rows and pack_device (with positions, segments, row_start) against the Python loop."""
    import torch
    ids = np.asarray(ids, dtype=np.int32)
    row = None if row is None else np.asarray(row, dtype=np.int64)
    want = _want_pack(_emitted(ids, row, **_split(kw, EMIT)), **_split(kw, ("seq_len", "pad_id", "drop_last")))
    got = enc.pack_rows(ids, row, positions=True, segments=True, **kw)
    d_ids = torch.from_numpy(ids).cuda()
    d_row = None if row is None else torch.from_numpy(row).cuda()
    dev = enc.pack_device(d_ids, d_row, positions=True, segments=True, **kw)
    assert len(got) == 4 and len(dev) == 5 and dev[4] >= 0
    assert [t.dtype for t in dev[:4]] == [torch.int32, torch.int64, torch.int32, torch.int32]
    for name, w, g, d in zip(("seqs", "row_start", "positions", "segments"), want, got, dev):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, "host", kw)
        d = d.cpu().numpy()
        assert d.shape == w.shape and np.array_equal(d, w), (name, "device", kw)
    two = enc.pack_rows(ids, row, **kw)  # without the optional arrays
    assert len(two) == 2 and np.array_equal(two[0], want[0]) and np.array_equal(two[1], want[1])
    seg_only = enc.pack_rows(ids, row, segments=True, **kw)
    assert len(seg_only) == 3 and np.array_equal(seg_only[2], want[3])
    return got


def _rows_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def _ids(rng, n):
    return rng.integers(0, 50_000, size=n).astype(np.int32)


# ---- the raw ABI --------------------------------------------------------------------------------

def _ptr(v):
    return None if v is None else ctypes.byref(ctypes.c_int32(v))


def _raw_pad(enc, ids, row, width, out_size, cap=None, bos=None, eos=None, max_len=0):
    """Both ABIs on sentinel-filled buffers -> [(result, out, lengths, mask)] as numpy."""
    import torch
    from shredword.cbase import lib
    ids = np.asarray(ids, dtype=np.int32)
    row = None if row is None else np.asarray(row, dtype=np.int64)
    R = 1 if row is None else row.size - 1
    cap = out_size if cap is None else cap
    opts = (_ptr(bos), _ptr(eos), max_len, 0, width, 0, 0)
    out = np.full(out_size, SENT, dtype=np.int32)
    lens = np.full(max(R, 1), SENT, dtype=np.int32)
    mask = np.full(out_size, 0xA5, dtype=np.uint8)
    r = lib.shred_pad_rows(enc.enc, ids.ctypes.data, ids.size, None if row is None else row.ctypes.data,
                           0 if row is None else R, *opts, out.ctypes.data, cap, lens.ctypes.data, mask.ctypes.data)
    res = [(r, out, lens, mask)]
    d_ids = torch.from_numpy(ids).cuda()
    d_row = None if row is None else torch.from_numpy(row).cuda()
    d_out = torch.full((out_size,), SENT, dtype=torch.int32, device="cuda")
    d_lens = torch.full((max(R, 1),), SENT, dtype=torch.int32, device="cuda")
    d_mask = torch.full((out_size,), 0xA5, dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = lib.shred_pad_device(enc.enc, d_ids.data_ptr(), ids.size, None if row is None else d_row.data_ptr(),
                             0 if row is None else R, *opts, d_out.data_ptr(), cap, d_lens.data_ptr(),
                             d_mask.data_ptr(), st, None)
    res.append((r, d_out.cpu().numpy(), d_lens.cpu().numpy(), d_mask.cpu().numpy()))
    return res


def _raw_pack(enc, ids, row, seq_len, out_size, cap=None, drop_last=0):
    """Both ABIs on sentinel-filled buffers -> [(result, out, pos, seg, row_start)] as numpy."""
    import torch
    from shredword.cbase import lib
    ids = np.asarray(ids, dtype=np.int32)
    row = None if row is None else np.asarray(row, dtype=np.int64)
    R = 1 if row is None else row.size - 1
    cap = out_size if cap is None else cap
    opts = (None, None, 0, 0, seq_len, 0, drop_last)
    bufs = [np.full(out_size, SENT, dtype=np.int32) for _ in range(3)] + [np.full(R + 1, SENT, dtype=np.int64)]
    r = lib.shred_pack_rows(enc.enc, ids.ctypes.data, ids.size, None if row is None else row.ctypes.data,
                            0 if row is None else R, *opts, bufs[0].ctypes.data, cap, bufs[1].ctypes.data,
                            bufs[2].ctypes.data, bufs[3].ctypes.data)
    res = [(r, *bufs)]
    d_ids = torch.from_numpy(ids).cuda()
    d_row = None if row is None else torch.from_numpy(row).cuda()
    d = [torch.full((out_size,), SENT, dtype=torch.int32, device="cuda") for _ in range(3)] + \
        [torch.full((R + 1,), SENT, dtype=torch.int64, device="cuda")]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = lib.shred_pack_device(enc.enc, d_ids.data_ptr(), ids.size, None if row is None else d_row.data_ptr(),
                              0 if row is None else R, *opts, d[0].data_ptr(), cap, d[1].data_ptr(), d[2].data_ptr(),
                              d[3].data_ptr(), st, None)
    res.append((r, *[t.cpu().numpy() for t in d]))
    return res


def _untouched(*arrays):
    return all((a == (0xA5 if a.dtype == np.uint8 else SENT)).all() for a in arrays)


# ---- 1. degenerate ------------------------------------------------------------------------------

def test_degenerate(enc):
    none = np.zeros(0, np.int32)
    rng = np.random.default_rng(1)
    # rows == 0
    batch, lengths = enc.pad_rows(none, [0])
    assert batch.shape == (0, 0) and lengths.shape == (0,)
    seqs, start = enc.pack_rows(none, [0], seq_len=8)
    assert seqs.shape == (0, 8) and start.tolist() == [0]
    _check_pad(enc, none, [0])
    _check_pad(enc, none, [0], bos=1, eos=2, width=3)
    _check_pack(enc, none, [0], seq_len=8)
    _check_pack(enc, none, [0], seq_len=8, bos=1, eos=2, drop_last=True)
    # row_offsets = None: one row
    ids = _ids(rng, 37)
    assert _check_pad(enc, ids).shape == (1, 37)
    assert _check_pad(enc, ids, bos=-5, eos=7, max_len=10, truncate="left", pad="left", width=12).shape == (1, 12)
    assert _check_pad(enc, none).shape == (1, 0)
    assert _check_pad(enc, none, eos=3).tolist() == [[3]]
    got = _check_pack(enc, ids, seq_len=10, eos=9)
    assert got[0].shape == (4, 10) and got[1].tolist() == [0, 38]
    assert _check_pack(enc, none, seq_len=4)[0].shape == (0, 4)
    # n == 0 with several empty rows; add == 0: pad returns width 0, pack S == 0
    for rows in (1, 5):
        row = [0] * (rows + 1)
        assert _check_pad(enc, none, row).shape == (rows, 0)
        assert _check_pad(enc, none, row, width=2, pad_id=-1).tolist() == [[-1, -1]] * rows
        got = _check_pack(enc, none, row, seq_len=3)
        assert got[0].shape == (0, 3) and got[1].tolist() == [0] * (rows + 1)
        # the same with bos and eos: every row is [bos, eos]
        assert _check_pad(enc, none, row, bos=11, eos=12).tolist() == [[11, 12]] * rows
        got = _check_pack(enc, none, row, seq_len=3, bos=11, eos=12)
        assert got[0].shape == (-(-2 * rows // 3), 3) and got[1].tolist() == list(range(0, 2 * rows + 1, 2))
        _check_pack(enc, none, row, seq_len=3, bos=11, eos=12, drop_last=True)
    # all rows empty between rows of ids
    _check_pad(enc, ids, [0, 0, 0, 37, 37])
    _check_pack(enc, ids, [0, 0, 0, 37, 37], seq_len=5)


# ---- 2. options ---------------------------------------------------------------------------------

def test_options(enc):
    rng = np.random.default_rng(2)
    lens = [0, 1, 2, 3, 7, 0, 30, 4, 1, 0]
    row = _rows_of(lens)
    ids = _ids(rng, int(row[-1]))
    big = 256 + enc.num_merges + 1000
    for bos, eos in ((None, None), (5, None), (None, 6), (5, 6), (-1, -2 ** 31), (big, 2 ** 31 - 1)):
        add = (bos is not None) + (eos is not None)
        # max_len == add keeps nothing (0 is "no limit"); add + 1 keeps one id; 64 is larger than every row
        for max_len in (None, add, add + 1, add + 3, 64):
            for truncate in ("right", "left"):
                kw = dict(bos=bos, eos=eos, max_len=max_len, truncate=truncate)
                for pad in ("right", "left"):
                    _check_pad(enc, ids, row, pad=pad, pad_id=-9, **kw)
                _check_pack(enc, ids, row, seq_len=7, pad_id=-9, **kw)
            if max_len:
                batch, lengths = enc.pad_rows(ids, row, bos=bos, eos=eos, max_len=max_len, width=max_len)
                assert batch.shape == (len(lens), max_len) and lengths.max() <= max_len
                if max_len == add:
                    assert (lengths == add).all()
    b = _check_pad(enc, ids, row, max_len=3, truncate="left", pad="left", pad_id=-1)
    assert b[6].tolist() == ids[row[7] - 3:row[7]].tolist() and b[1].tolist() == [-1, -1, int(ids[0])]
    for bad in (dict(truncate="middle"), dict(pad="center"), dict(bos=1, eos=2, max_len=1), dict(max_len=-1),
                dict(bos=2 ** 31), dict(pad_id=-2 ** 31 - 1), dict(width=-1)):
        with pytest.raises(ValueError):
            enc.pad_rows(ids, row, **bad)
    for bad in (dict(seq_len=0), dict(seq_len=-3), dict(seq_len=4, truncate="up"),
                dict(seq_len=4, bos=1, eos=1, max_len=1)):
        with pytest.raises(ValueError):
            enc.pack_rows(ids, row, **bad)
    with pytest.raises(TypeError):
        enc.pack_rows(ids, row)  # seq_len is required
    with pytest.raises(ValueError, match="width"):
        enc.pad_rows(ids, row, width=29)  # the longest row holds 30 ids
    from shredword.cbase import lib
    one = ctypes.c_int32(1)
    for r in (lib.shred_pad_rows(enc.enc, ids.ctypes.data, ids.size, row.ctypes.data, len(lens), ctypes.byref(one),
                                 ctypes.byref(one), 1, 0, 0, 0, 0, None, 0, None, None),          # max_len < add
              lib.shred_pad_rows(enc.enc, ids.ctypes.data, ids.size, row.ctypes.data, len(lens), None, None, 0, 2,
                                 0, 0, 0, None, 0, None, None),                                    # trunc_side
              lib.shred_pack_rows(enc.enc, ids.ctypes.data, ids.size, row.ctypes.data, len(lens), None, None, 0, 0,
                                  0, 0, 0, None, 0, None, None, None)):                            # seq_len == 0
        assert r == -1


# ---- 3. pad tile edges --------------------------------------------------------------------------

def _pad_case(enc, rng, rows, width, **kw):
    """rows x width with random row lengths in [0, width], at least one row full."""
    lens = rng.integers(0, width + 1, size=rows)
    lens[rng.integers(0, rows)] = width
    row = _rows_of(lens)
    ids = _ids(rng, int(row[-1]))
    for pad in ("right", "left"):
        assert _check_pad(enc, ids, row, pad=pad, pad_id=-3, **kw).shape == (rows, width)
    return ids, row


def test_pad_tile_edges(enc):
    T = _tile()
    rng = np.random.default_rng(3)
    assert (T - 1) % 3 == 0 and (T + 1) % 5 == 0
    for rows, width in ((T - 1, 1), (T, 1), (T + 1, 1),            # rows * width == T - 1, T, T + 1
                        ((T - 1) // 3, 3), ((T + 1) // 5, 5), (T // 4, 4),
                        (2 * T // 3 + 1, 3), (2 * T // 5 + 3, 5),  # a lane's 4 entries straddle rows, 3 tiles
                        (1, 2 * T + 7), (3, 2 * T + 7)):           # a row wider than two tiles
        _pad_case(enc, rng, rows, width)
    # width - 2 ids plus bos and eos, truncated from either side
    ids, row = _pad_case(enc, rng, 7, 150)
    for truncate in ("right", "left"):
        _check_pad(enc, ids, row, bos=1, eos=2, max_len=99, truncate=truncate, pad="left")
    # a width larger than needed, and the sizing call
    need = int(np.diff(row).max())
    assert enc.pad_rows(ids, row)[0].shape == (7, need)
    assert _check_pad(enc, ids, row, width=need + 1 + T)[:, need:].max() == 0
    # a too-small width on the raw ABI: the needed width comes back, nothing is written
    for r, out, lens, mask in _raw_pad(enc, ids, row, need - 1, 7 * need):
        assert r == need and _untouched(out, lens, mask)
    for r, out, lens, mask in _raw_pad(enc, ids, row, need, 7 * need, cap=7 * need - 1):  # cap one short
        assert r == need and _untouched(out, lens, mask)
    for r, out, lens, mask in _raw_pad(enc, ids, row, need, 7 * need + 9):
        want = _want_pad(_emitted(ids, row))
        assert r == need and np.array_equal(out[:7 * need].reshape(7, need), want[0]) and _untouched(out[7 * need:])
        assert np.array_equal(lens, want[1]) and np.array_equal(mask[:7 * need].reshape(7, need), want[2])
        assert _untouched(mask[7 * need:])


# ---- 4. pack tile edges -------------------------------------------------------------------------

def test_pack_tile_edges(enc):
    T, G = _tile(), _stage()
    rng = np.random.default_rng(4)
    for d in (-1, 0, 1):
        # T + d stream ids; for d >= 0 a row boundary exactly on the tile edge (300 + 0 + 424 + 300 == T)
        lens = [300, 0, 424, 299] if d < 0 else [300, 0, 424, 300, d]
        assert sum(lens) == T + d
        row = _rows_of(lens)
        ids = _ids(rng, T + d)
        for L in (1, 7, 128, T, T + d, T + d + 1, 4 * T):
            for drop in (False, True):
                _check_pack(enc, ids, row, seq_len=L, pad_id=-4, drop_last=drop)
        # with bos and eos the same ids give T + d + 2 * rows stream positions
        _check_pack(enc, ids, row, seq_len=64, bos=1, eos=2)
        # T + d positions once the 4 bos are counted
        lens = [299, 0, 423]
        lens.append(T + d - 4 - sum(lens))
        _check_pack(enc, ids[:sum(lens)], _rows_of(lens), seq_len=100, bos=3)
    # one row longer than two tiles, between short rows
    lens = [5, 2 * T + 9, 0, 3]
    ids = _ids(rng, sum(lens))
    _check_pack(enc, ids, _rows_of(lens), seq_len=T, eos=0)
    _check_pack(enc, ids, _rows_of(lens), seq_len=333, drop_last=True)
    _check_pack(enc, ids, None, seq_len=T + 1)
    # BATCH_STAGE + 5 rows of one id inside one tile: more than one LDS round
    assert G + 5 + 100 < T
    lens = [100] + [1] * (G + 5) + [50]
    ids = _ids(rng, sum(lens))
    _check_pack(enc, ids, _rows_of(lens), seq_len=64)
    ones = _ids(rng, 2 * T + 5)
    _check_pack(enc, ones, _rows_of([1] * (2 * T + 5)), seq_len=T)   # every tile: T rows, two rounds
    # BATCH_STAGE + 5 rows that emit nothing, then one row that does: the repeated-E search
    lens = [0] * (G + 5) + [40]
    ids = _ids(rng, 40)
    got = _check_pack(enc, ids, _rows_of(lens), seq_len=16)
    assert got[3][0, 0] == G + 5 and got[1][:G + 6].tolist() == [0] * (G + 6)
    # the same run in the middle of a tile and at its end: the rounds walk over it
    lens = [10] + [0] * (2 * G + 5) + [40] + [0] * (G + 5)
    ids = _ids(rng, 50)
    _check_pack(enc, ids, _rows_of(lens), seq_len=16)
    _check_pad(enc, ids, _rows_of(lens))
    # seq_len == 1; seq_len > T (one padded sequence, or none with drop_last); T % seq_len == 0
    lens = [3, 0, 4, 5]
    ids = _ids(rng, 12)
    row = _rows_of(lens)
    assert _check_pack(enc, ids, row, seq_len=1)[0].shape == (12, 1)
    assert _check_pack(enc, ids, row, seq_len=13, pad_id=-1)[0].shape == (1, 13)
    assert _check_pack(enc, ids, row, seq_len=13, drop_last=True)[0].shape == (0, 13)
    for L in (12, 6, 4):
        assert _check_pack(enc, ids, row, seq_len=L)[0].shape == (12 // L, L)
        assert _check_pack(enc, ids, row, seq_len=L, drop_last=True)[0].shape == (12 // L, L)
    # drop_last with row_start[rows] > S * seq_len: row_start is still written in full
    got = _check_pack(enc, ids, row, seq_len=5, drop_last=True)
    assert got[0].shape == (2, 5) and got[1].tolist() == [0, 3, 3, 7, 12]
    # capacity on the raw ABI: S comes back, nothing is written
    for r, out, pos, seg, start in _raw_pack(enc, ids, row, 5, 15, cap=14):
        assert r == 3 and _untouched(out, pos, seg, start)
    for r, out, pos, seg, start in _raw_pack(enc, ids, row, 5, 20):
        assert r == 3 and out[:12].tolist() == ids.tolist() and out[12:15].tolist() == [0] * 3
        assert _untouched(out[15:], pos[15:], seg[15:]) and start.tolist() == [0, 3, 3, 7, 12]


# ---- 5. pos and seg -----------------------------------------------------------------------------

def test_positions_and_segments(enc):
    rng = np.random.default_rng(5)
    lens = [4, 0, 9, 0, 0, 2]
    row = _rows_of(lens)
    ids = _ids(rng, 15)
    # truncation from the left and a bos: rows of [bos] + the last <= 4 ids
    seqs, start, pos, seg = _check_pack(enc, ids, row, seq_len=8, bos=-1, max_len=5, truncate="left", pad_id=-2)
    assert start.tolist() == [0, 5, 6, 11, 12, 13, 16]
    flat_pos, flat_seg, flat = pos.reshape(-1), seg.reshape(-1), seqs.reshape(-1)
    assert flat_pos[:16].tolist() == [0, 1, 2, 3, 4, 0, 0, 1, 2, 3, 4, 0, 0, 0, 1, 2]   # restarts at 0 on each row
    assert (flat[flat_pos == 0][:6] == -1).all()                                       # where the bos sits
    assert flat[6:11].tolist() == [-1] + ids[9:13].tolist()                            # the last 4 of row 2
    assert flat_seg[:16].tolist() == [0] * 5 + [1] + [2] * 5 + [3, 4] + [5] * 3
    # without the bos the empty rows emit nothing: seg skips 1, 3 and 4
    seqs, start, pos, seg = _check_pack(enc, ids, row, seq_len=8, max_len=4, truncate="left", pad_id=-2)
    assert seg.reshape(-1).tolist() == [0] * 4 + [2] * 4 + [5] * 2 + [-1] * 6
    assert pos.reshape(-1).tolist() == [0, 1, 2, 3] * 2 + [0, 1] + [0] * 6             # the pad tail is (0, -1)
    assert seqs.reshape(-1)[10:].tolist() == [-2] * 6 and start.tolist() == [0, 4, 4, 8, 8, 8, 10]


# ---- 6. malformed row offsets -------------------------------------------------------------------

def test_malformed_row_offsets(enc):
    import torch
    rng = np.random.default_rng(6)
    n = 1000
    ids = _ids(rng, n)
    cases = [[1, 500, n],            # a first entry that is not 0
             [0, 500, n - 1],        # a last entry that is not n
             [0, 500, n + 1],
             [0, 600, 599, n],       # a decreasing pair
             [0, -1, n],             # a negative entry
             [-1, 500, n],
             [0, n + 5, n]]
    for row in cases:
        R = len(row) - 1
        for r, out, lens, mask in _raw_pad(enc, ids, row, n, R * n):
            assert r == -6 and _untouched(out, lens, mask), row
        for r, out, pos, seg, start in _raw_pack(enc, ids, row, 16, n + 64):
            assert r == -6 and _untouched(out, pos, seg, start), row
        d_ids, d_row = torch.from_numpy(ids).cuda(), torch.tensor(row, dtype=torch.int64).cuda()
        with pytest.raises(ValueError, match="row_offsets"):
            enc.pad_rows(ids, row)
        with pytest.raises(ValueError, match="row_offsets"):
            enc.pack_rows(ids, row, seq_len=16)
        with pytest.raises(ValueError, match="row_offsets"):
            enc.pad_device(d_ids, d_row)
        with pytest.raises(ValueError, match="row_offsets"):
            enc.pack_device(d_ids, d_row, seq_len=16)
    with pytest.raises(ValueError):
        enc.pad_rows(ids, [])
    _check_pad(enc, ids, [0, 500, n])  # the encoder is still usable


# ---- 7. host pieces -----------------------------------------------------------------------------

def test_host_pieces(enc, monkeypatch):
    rng = np.random.default_rng(7)
    n = 40_000
    ends = set(int(x) for x in rng.choice(np.arange(1, n), size=n // 300, replace=False))
    ends = {e for e in ends if not 20_000 < e < 23_500}          # one row longer than a piece of 1001
    ends |= {999, 1001, 2000, 2002, 7000, 13013, 39000}          # rows that end exactly on piece cuts
    empties = [999, 2000, 2002, 13013, n]                        # empty rows on the cuts
    row = np.array([0] + sorted(list(ends) + empties + [n]), dtype=np.int64)
    lens = np.diff(row)
    assert lens.max() > 3000 and (lens == 0).sum() == 5 and lens.size > 100
    ids = _ids(rng, n)
    pad_kw = dict(bos=1, eos=2, max_len=700, truncate="left", pad="left", pad_id=-1)
    pack_kw = dict(seq_len=512, eos=2, pad_id=-1)
    monkeypatch.delenv("SHREDWORD_BATCH_PIECE", raising=False)
    pad_one = enc.pad_rows(ids, row, mask=True, **pad_kw)
    pack_one = enc.pack_rows(ids, row, positions=True, segments=True, **pack_kw)
    drop_one = enc.pack_rows(ids, row, positions=True, segments=True, drop_last=True, **pack_kw)
    flat_one = enc.pack_rows(ids, None, positions=True, segments=True, **pack_kw)
    want_pad = _want_pad(_emitted(ids, row, **_split(pad_kw, EMIT)), pad_id=-1, pad="left")
    want_pack = _want_pack(_emitted(ids, row, eos=2), 512, pad_id=-1)
    want_drop = _want_pack(_emitted(ids, row, eos=2), 512, pad_id=-1, drop_last=True)
    assert want_drop[1][-1] > want_drop[0].size
    for got, want in ((pad_one, want_pad), (pack_one, want_pack), (drop_one, want_drop)):
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want)
    for piece in ("1", "999", "1001"):
        monkeypatch.setenv("SHREDWORD_BATCH_PIECE", piece)
        for got, want in ((enc.pad_rows(ids, row, mask=True, **pad_kw), pad_one),
                          (enc.pack_rows(ids, row, positions=True, segments=True, **pack_kw), pack_one),
                          (enc.pack_rows(ids, row, positions=True, segments=True, drop_last=True, **pack_kw), drop_one),
                          (enc.pack_rows(ids, None, positions=True, segments=True, **pack_kw), flat_one)):
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w), piece


# ---- 8. views -----------------------------------------------------------------------------------

def test_device_views(enc):
    import torch
    from shredword.cbase import lib
    rng = np.random.default_rng(8)
    text = b"".join(bytes(rng.choice([97, 98, 99], size=int(rng.integers(1, 9))).astype(np.uint8)) +
                    bytes([int(rng.choice([10, 32, 32, 32]))]) for _ in range(2000)) + b"abc"
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    ids, _, line, _ = enc.encode_spans_device(d_text)  # views of larger tensors, as they are
    h_ids, h_line = ids.cpu().numpy(), line.cpu().numpy()
    em = _emitted(h_ids, h_line, eos=0)
    batch, lengths, mask, ms = enc.pad_device(ids, line, eos=0, mask=True)
    want = _want_pad(em)
    assert ms > 0 and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip((batch, lengths, mask), want))
    seqs, start, pos, seg, ms = enc.pack_device(ids, line, seq_len=256, eos=0, positions=True, segments=True)
    want = _want_pack(em, 256)
    assert ms > 0 and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip((seqs, start, pos, seg), want))
    # outputs offset by one element: 4-byte but not 16-byte aligned (1 byte for the mask), through the raw ABI
    R, W = h_line.size - 1, int(np.diff(h_line).max()) + 1
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    eos = ctypes.c_int32(0)
    big = torch.full((R * W + 1 + 8,), SENT, dtype=torch.int32, device="cuda")
    bl = torch.full((R + 1,), SENT, dtype=torch.int32, device="cuda")
    bm = torch.full((R * W + 1 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    assert big[1:].data_ptr() % 16 == 4 and bm[1:].data_ptr() % 4 == 1
    r = lib.shred_pad_device(enc.enc, ids.data_ptr(), ids.numel(), line.data_ptr(), R, None, ctypes.byref(eos), 0, 0,
                             W, 0, 0, big[1:].data_ptr(), R * W, bl[1:].data_ptr(), bm[1:].data_ptr(), st, None)
    want = _want_pad(em)
    got, gm = big.cpu().numpy(), bm.cpu().numpy()
    assert r == W and got[0] == SENT and np.array_equal(got[1:1 + R * W].reshape(R, W), want[0])
    assert (got[1 + R * W:] == SENT).all() and np.array_equal(bl.cpu().numpy()[1:], want[1])
    assert gm[0] == 0xA5 and np.array_equal(gm[1:1 + R * W].reshape(R, W), want[2]) and (gm[1 + R * W:] == 0xA5).all()
    want = _want_pack(em, 256)
    SL = want[0].size
    bufs = [torch.full((SL + 1 + 8,), SENT, dtype=torch.int32, device="cuda") for _ in range(3)]
    r = lib.shred_pack_device(enc.enc, ids.data_ptr(), ids.numel(), line.data_ptr(), R, None, ctypes.byref(eos), 0, 0,
                              256, 0, 0, bufs[0][1:].data_ptr(), SL, bufs[1][1:].data_ptr(), bufs[2][1:].data_ptr(),
                              None, st, None)
    assert r == SL // 256
    for t, w in zip(bufs, (want[0], want[2], want[3])):
        g = t.cpu().numpy()
        assert g[0] == SENT and np.array_equal(g[1:1 + SL], w.reshape(-1)) and (g[1 + SL:] == SENT).all()
    # argument checks, as decode_device makes them
    for bad in ((ids.cpu(), line), (ids, line.cpu()), (ids.to(torch.int64), line), (ids, line.to(torch.int32)),
                (ids, line[:0])):
        with pytest.raises(ValueError):
            enc.pad_device(*bad)
        with pytest.raises(ValueError):
            enc.pack_device(*bad, seq_len=8)
    enc.device += 1  # the tensors are now on another device than the encoder
    try:
        with pytest.raises(ValueError, match="is on"):
            enc.pad_device(ids, line)
        with pytest.raises(ValueError, match="is on"):
            enc.pack_device(ids, line, seq_len=8)
    finally:
        enc.device -= 1


# ---- 9. end to end ------------------------------------------------------------------------------

def test_golden_end_to_end(case_corpus, tmp_path):
    from shredword.encoder import BPEEncoder
    case, path = case_corpus("small_v300")
    text = open(path, "rb").read()[:4000]
    text = text[:text.rindex(b"\n") + 1] + b"last line without a newline"
    (tmp_path / "g.model").write_bytes(case["model_bytes"])
    (tmp_path / "g.vocab").write_bytes(case["vocab_bytes"])
    V = 256 + model_merges(case["model_bytes"]).shape[0]
    E = V  # an eos outside the vocabulary: the decoder can drop it again
    with BPEEncoder(str(tmp_path / "g.model"), str(tmp_path / "g.vocab"), unk_id=case["config"]["unk_id"]) as enc:
        ids, line = enc.encode_lines(text)
        assert line.size - 1 == text.count(b"\n") + 1 and ids.size > 500
        em = _emitted(ids, line, eos=E)
        got = enc.encode_padded(text, eos=E, mask=True)
        assert all(np.array_equal(g, w) for g, w in zip(got, _want_pad(em)))
        seqs, start = enc.encode_packed(text, seq_len=128, eos=E)
        want = _want_pack(em, 128)
        assert np.array_equal(seqs, want[0]) and np.array_equal(start, want[1])
        stream = seqs.reshape(-1)[:start[-1]]
        data, boff = enc.decode_rows(stream, start, sep=b"\n", unk=b"")  # row_start is a row_offsets of the stream
        lines = [data[boff[i]:boff[i + 1] - 1] for i in range(boff.size - 1)]
        assert lines == enc.decode_lines(ids, line)
        assert [stream[start[i]:start[i + 1] - 1].tolist() for i in range(line.size - 1)] == \
            [ids[line[i]:line[i + 1]].tolist() for i in range(line.size - 1)]
