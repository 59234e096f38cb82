"""GPU tests of the fill-in-the-middle calls (include/shredword_encode.h, shred_fim_*): every case runs
through both ABIs, device tensors and host rows, and is compared exactly (the stream, its offsets,
out_src, out_seg, row_info and the count) with tests/fim_ref.py, which tests/test_fim_ref_cpu.py pins.

The encoders come from from_merges with the merges "ab" and "abab" and specials, as in
test_gpu_corrupt.py.  The shapes are the smallest at which the kernels can go wrong: the edges of an
output tile of BATCH_TILE ids, sentinels on both sides of a tile edge, a row across three tiles, more
row beginnings in a tile than one BATCH_STAGE, views that are only element-aligned, caps that are exact
or one short, pieces smaller than a row, and character-level cuts inside multibyte characters.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import fim_ref

pytestmark = pytest.mark.gpu

A, B, C = ord("a"), ord("b"), ord("c")
MERGES = np.array([[A, B, 256], [256, 256, 257]], dtype=np.int32)  # "ab", "abab"
SPECIALS = [b"<|s|>", b"<PRE>", b"<SUF>", b"<MID>"]
SP, PRE, SUF, MID = 258, 259, 260, 261
SENT = dict(pre_id=PRE, suf_id=SUF, mid_id=MID)
NO = (-1, -1, -1)


@pytest.fixture(scope="module")
def enc():
    from shredword.encoder import BPEEncoder
    e = BPEEncoder.from_merges(MERGES, special_tokens=SPECIALS)
    assert [e.special_tokens[s] for s in SPECIALS] == [SP, PRE, SUF, MID]
    yield e
    e.destroy()


def _dev(a, dt=None):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype=dt or a.dtype)).cuda()


def _same(name, got, want):
    """(out_ids, out_row, out_src, out_seg, row_info) against the reference's."""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, k, g[:20], w[:20])


def _both(e, ids, row=None, cuts=None, **kw):
    """The call on host rows and on device tensors, both compared with the reference; -> the reference's."""
    import torch
    ids = np.asarray(ids, dtype=np.int32)
    row = None if row is None else np.asarray(row, dtype=np.int64)
    cuts = None if cuts is None else np.asarray(cuts, dtype=np.int64).reshape(-1, 3)
    kw = dict(SENT, **kw)
    want = fim_ref.fim_ref(ids, row, cuts=cuts, **kw)
    _same("host", e.fim_rows(ids, row, cuts=cuts, src=True, seg=True, info=True, **kw), want)
    d_ids = _dev(ids)
    *got, ms = e.fim_device(d_ids, _dev(row), cuts=_dev(cuts), src=True, seg=True, info=True, **kw)
    assert ms >= 0 and torch.equal(d_ids.cpu(), torch.from_numpy(ids)), "the input tensor is untouched"
    _same("device", [t.cpu().numpy() for t in got], want)
    assert len(e.fim_rows(ids, row, cuts=cuts, **kw)) == 2  # without the optional outputs
    return want


def _stream(n, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([A, B, C, 256, 257, SP, -1], dtype=np.int32), size=n,
                      p=[.2, .2, .2, .15, .15, .05, .05]).astype(np.int32)


def _rows(n, rows, seed):
    """rows + 1 offsets with runs of empty rows."""
    rng = np.random.default_rng(seed)
    at = np.sort(rng.integers(0, n + 1, size=max(rows - 1, 0)))
    return np.concatenate([[0], at, [n]]).astype(np.int64)


def _cuts(row, seed, p_no=0.3):
    """Valid random cuts, a share p_no of the rows not transformed."""
    rng = np.random.default_rng(seed)
    out = []
    for L in np.diff(row):
        a, b = sorted(int(v) for v in rng.integers(0, L + 1, size=2))
        out.append(NO if rng.random() < p_no else (a, b, int(rng.integers(2))))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


# ---- 1. output tile edges -------------------------------------------------------------------------------

def test_output_tile_edges(enc):
    from shredword.encoder import BATCH_TILE
    for T in (BATCH_TILE - 1, BATCH_TILE, BATCH_TILE + 1):
        n = T - 3
        want = _both(enc, _stream(n, T), None, fim_rate=1.0, seed=T)
        assert want[0].size == T
        n = T - 9                                             # five rows, three of them transformed
        row = np.array([0, 0, 200, 200, n - 7, n])
        cuts = np.array([(0, 0, 1), NO, (0, 0, 0), NO, (2, 5, T % 2)])
        want = _both(enc, _stream(n, T + 1), row, cuts)
        assert want[0].size == T
    for n in (0, 1, 3):
        for rate in (0.0, 1.0):
            _both(enc, _stream(n, n), None, fim_rate=rate, seed=n)
            _both(enc, _stream(n, n), [0, 0, n, n, n, n], fim_rate=rate, seed=n)


# ---- 2. each sentinel on both sides of a tile edge ------------------------------------------------------

def test_sentinels_at_a_tile_edge(enc):
    from shredword.encoder import BATCH_TILE
    L, a, b = 40, 10, 25
    for mode in (0, 1):
        at = (0, a + 1, a + 2 + L - b) if mode == 0 else (0, 1, 2 + L - b)
        for s in at:
            for target in (BATCH_TILE - 1, BATCH_TILE):      # the sentinel is the tile's last id, the next one's first
                lead = target - s
                n = lead + L + 9
                want = _both(enc, _stream(n, s + target), [0, lead, lead + L, n], [NO, (a, b, mode), (3, 3, 1 - mode)])
                assert want[3][target] == 4 and want[0][target] in (PRE, SUF, MID)


# ---- 3. one row across three tiles ----------------------------------------------------------------------

def test_a_row_across_three_tiles(enc):
    from shredword.encoder import BATCH_TILE
    L = 2 * BATCH_TILE + 5
    ids = _stream(L, 33)
    for mode in (0, 1):
        for a, b in ((300, BATCH_TILE + 700), (0, L), (BATCH_TILE, BATCH_TILE), (BATCH_TILE - 2, 2 * BATCH_TILE - 1)):
            want = _both(enc, ids, [0, 0, L, L], [(0, 0, mode), (a, b, mode), (0, 0, 1 - mode)])
            assert want[0].size == L + 9


# ---- 4. more row beginnings in a tile than one stage ------------------------------------------------------

def test_many_short_rows(enc):
    from shredword.encoder import BATCH_STAGE, BATCH_TILE
    for rows, seed in ((BATCH_STAGE + 88, 4), (2800, 5)):
        rng = np.random.default_rng(seed)
        row = np.concatenate([[0], np.cumsum(rng.integers(0, 3, size=rows))]).astype(np.int64)
        ids = _stream(int(row[-1]), seed)
        want = _both(enc, ids, row, _cuts(row, seed, p_no=0.9))
        begins = np.bincount(want[1][:-1] // BATCH_TILE)
        assert begins.max() > BATCH_STAGE
        if rows > 2000:
            assert want[0].size > 3 * BATCH_TILE
        _both(enc, ids, row, fim_rate=0.1, seed=seed)
    row = np.zeros(700, dtype=np.int64)                       # rows and no ids: sentinels only
    _both(enc, np.zeros(0, np.int32), row, fim_rate=1.0)
    _both(enc, np.zeros(0, np.int32), row, fim_rate=0.0)


# ---- 5. drawn decisions -----------------------------------------------------------------------------------

def test_drawn_decisions(enc):
    rng = np.random.default_rng(8)
    row = np.concatenate([[0], np.cumsum(rng.integers(0, 9, size=4000))]).astype(np.int64)
    ids = _stream(int(row[-1]), 8)
    info = fim_ref.fim_ref(ids, row, seed=21, **SENT)[4]
    assert (info[:, 2] == 0).any() and (info[:, 2] == 1).any() and (info[:, 2] == -1).any()
    assert ((info[:, 2] >= 0) & (info[:, 0] == info[:, 1])).any()
    _both(enc, ids, row, seed=21)
    big = (1 << 63) + 12345
    a = _both(enc, ids, row, seed=21, row_base=big)
    cut = int(row[1000])
    tail = _both(enc, ids[cut:], row[1000:] - cut, seed=21, row_base=big + 1000)
    assert np.array_equal(tail[0], a[0][a[1][1000]:])


# ---- 6. scalar options ------------------------------------------------------------------------------------

def test_scalar_options(enc):
    from shredword.encoder import BATCH_TILE
    n = BATCH_TILE + 9
    ids = _stream(n, 51)
    row = _rows(n, 40, 51)
    zero = _both(enc, ids, row, fim_rate=0.0, seed=4)
    assert np.array_equal(zero[0], ids) and np.array_equal(zero[1], row) and zero[0].size == n
    ml = int(np.median(np.diff(row)))
    one = _both(enc, ids, row, fim_rate=1.0, min_len=ml + 1, seed=4)
    assert np.array_equal(one[4][:, 2] >= 0, np.diff(row) > ml) and 0 < (one[4][:, 2] >= 0).sum() < 40
    assert (_both(enc, ids, row, fim_rate=1.0, spm_rate=0.0, seed=4)[4][:, 2] == 0).all()
    assert (_both(enc, ids, row, fim_rate=1.0, spm_rate=1.0, seed=4)[4][:, 2] == 1).all()
    _both(enc, ids, row, fim_rate=1.0, seed=4, pre_id=-5, suf_id=2 ** 31 - 1, mid_id=-2 ** 31)
    assert not np.array_equal(one[0], _both(enc, ids, row, fim_rate=1.0, min_len=ml + 1, seed=5)[0])


# ---- 7. the C ABI: errors, caps, views --------------------------------------------------------------------

def _opts(e, **kw):
    v = dict(SENT, fim_rate=0.5, spm_rate=0.5, seed=6, min_len=0, row_base=0)
    v.update(kw)
    return e._fim_opts(*[v[k] for k in ("pre_id", "suf_id", "mid_id", "fim_rate", "spm_rate", "seed", "min_len",
                                        "row_base")])


def _raw_device(e, opts, ids, row, cuts, out, cap, out_row, src, seg, info):
    import torch
    from shredword.cbase import lib
    ptr = lambda t: None if t is None else t.data_ptr()
    ms = ctypes.c_double()
    return lib.shred_fim_device(e.enc, ptr(ids), ids.numel(), ptr(row), 0 if row is None else row.numel() - 1,
                                ctypes.byref(opts), ptr(cuts), ptr(out), cap, ptr(out_row), ptr(src), ptr(seg),
                                ptr(info), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(ms))


def _raw_host(e, opts, ids, row, cuts, out, cap, out_row, src, seg, info):
    from shredword.cbase import lib
    ptr = lambda a: None if a is None else a.ctypes.data
    return lib.shred_fim_rows(e.enc, ptr(ids), ids.size, ptr(row), 0 if row is None else row.size - 1,
                              ctypes.byref(opts), ptr(cuts), ptr(out), cap, ptr(out_row), ptr(src), ptr(seg), ptr(info))


ABIS = (("host", _raw_host, lambda a: a, lambda a: a),
        ("device", _raw_device, lambda a: None if a is None else _dev(a), lambda t: t.cpu().numpy()))


def _filled(T, R):
    """out, out_row, src, seg, info with a guard element on both sides, pre-filled."""
    return [np.full(T + 2, -7, np.int32), np.full(R + 3, -7, np.int64), np.full(T + 2, -7, np.int64),
            np.full(T + 2, 249, np.uint8), np.full(3 * R + 2, -7, np.int64)]


def _untouched(bufs):
    return all((a == (249 if a.dtype == np.uint8 else -7)).all() for a in bufs)


def test_errors_write_nothing(enc):
    from shredword.cbase import ShredFimOpts
    n = 1200
    ids = _stream(n, 11)
    row = _rows(n, 6, 11)
    R = row.size - 1
    good = _opts(enc)
    ok_cuts = _cuts(row, 1)

    def both(opts, r=row, cuts=None, alias=False, no_row=False):
        res = []
        for name, raw, to, back in ABIS:
            b = [to(a) for a in _filled(n + 3 * R, r.size - 1)]
            d_ids = to(ids)
            code = raw(enc, opts, d_ids, to(r), to(cuts), d_ids if alias else b[0][1:], n + 3 * R,
                       None if no_row else b[1][1:], b[2][1:], b[3][1:], b[4][1:])
            if code < 0:
                assert _untouched([back(a) for a in b]), name
                assert np.array_equal(back(d_ids), ids)
            res.append(code)
        return tuple(res)

    assert both(good)[0] >= n and both(good, cuts=ok_cuts)[0] >= n
    for bad_row in ([0, 50, 40, n], [1, 50, n], [0, 50, n - 1], [0, -1, n], [0, 50, n + 1, n]):
        assert both(good, np.array(bad_row, dtype=np.int64)) == (-6, -6), bad_row
    L2 = int(row[3] - row[2])
    for bad in ((1, 0, 0) if L2 else (0, -1, 0), (0, L2 + 1, 0), (0, 0, 2), (-1, -1, 0), (0, -1, -1), (-1, 0, 1),
                (-2, -2, -2)):
        c = ok_cuts.copy()
        c[2] = bad
        assert both(good, cuts=c) == (-8, -8), bad

    def raw_opts(**kw):
        v = dict(row_base=0, seed=1, fim_rate=0.5, spm_rate=0.5, min_len=0, **SENT)
        v.update(kw)
        return ShredFimOpts(*[v[k] for k in ("row_base", "seed", "fim_rate", "spm_rate", "min_len", "pre_id", "suf_id",
                                             "mid_id")])

    assert both(raw_opts())[0] >= n
    for bad in (dict(fim_rate=float("nan")), dict(spm_rate=float("nan")), dict(fim_rate=-0.1), dict(spm_rate=1.5),
                dict(min_len=-1)):
        assert both(raw_opts(**bad)) == (-1, -1), bad
    assert both(good, alias=True) == (-1, -1)
    assert both(good, no_row=True) == (-1, -1)
    with pytest.raises(ValueError):
        enc.fim_rows(ids, np.array([0, 5], dtype=np.int64), **SENT)
    with pytest.raises(ValueError):
        enc.fim_rows(ids, row, cuts=np.array([(3, 2, 0)] * R), **SENT)
    for bad in (dict(fim_rate=2), dict(spm_rate=-1), dict(min_len=-1), dict(pre_id=2 ** 31), dict(cuts=[NO] * (R + 1))):
        with pytest.raises(ValueError):
            enc.fim_rows(ids, row, **dict(SENT, **bad))


def test_sizing(enc):
    """A cap one short, or no out_ids, leaves the outputs untouched and returns T_out; an exact cap writes
    nothing past it."""
    n = 1300
    ids = _stream(n, 9)
    row = _rows(n, 8, 9)
    R = row.size - 1
    want = fim_ref.fim_ref(ids, row, seed=6, **SENT)
    T = want[0].size
    assert n < T < n + 3 * R
    opts = _opts(enc)
    for short, null in ((0, False), (1, False), (0, True)):
        for name, raw, to, back in ABIS:
            b = [to(a) for a in _filled(T, R)]
            r = raw(enc, opts, to(ids), to(row), None, None if null else b[0][1:], T - short, b[1][1:], b[2][1:],
                    b[3][1:], b[4][1:])
            assert r == T, (name, short, null)
            got = [back(a) for a in b]
            if short or null:
                assert _untouched(got), (name, short, null)
            else:
                for k, w in enumerate(want):
                    w = w.reshape(-1)
                    fill = 249 if w.dtype == np.uint8 else -7
                    assert np.array_equal(got[k][1:1 + w.size], w) and got[k][0] == fill and got[k][-1] == fill, (name, k)


def test_views_that_are_only_element_aligned(enc):
    """Every buffer begins one element into its allocation; full tiles and a tail."""
    from shredword.encoder import BATCH_TILE
    n = 2 * BATCH_TILE + 7
    ids = _stream(n, 5)
    row = _rows(n, 6, 5)
    cuts = _cuts(row, 5)
    want = fim_ref.fim_ref(ids, row, cuts=cuts, **SENT)
    T, R = want[0].size, row.size - 1
    lead = lambda a: np.concatenate([np.full(1, -7, a.dtype), a.reshape(-1)])
    for name, raw, to, back in ABIS:
        t_ids, t_row, t_cuts = to(lead(ids)), to(lead(row)), to(lead(cuts))
        b = [to(a) for a in _filled(T, R)]
        r = raw(enc, _opts(enc), t_ids[1:], t_row[1:], t_cuts[1:], b[0][1:], T, b[1][1:], b[2][1:], b[3][1:], b[4][1:])
        assert r == T
        for t, w in zip(b, want):
            a, fill = back(t), 249 if w.dtype == np.uint8 else -7
            assert np.array_equal(a[1:-1], w.reshape(-1)) and a[0] == fill and a[-1] == fill, name


def test_ordered_behind_a_producer_on_the_callers_stream(enc):
    """The ids are produced by a kernel still pending on a non-default stream when the call is made."""
    import torch
    n = 1 << 20
    src = torch.from_numpy(_stream(n, 71)).cuda()
    row = torch.arange(0, n + 1, 64, dtype=torch.int64).cuda()
    kw = dict(SENT, seed=3, src=True, seg=True)
    want = [t.cpu() for t in enc.fim_device(src, row, **kw)[:4]]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ids = torch.zeros(n, dtype=torch.int32, device="cuda")
    big = torch.ones(1 << 26, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(8):
            big = big * 1.0001 + 0.5   # keeps the stream busy
        ids.copy_(src)                 # the producer, queued behind it
        got = enc.fim_device(ids, row, **kw)[:4]
    s.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g.cpu(), w)


# ---- 8. host pieces, in a fresh process ---------------------------------------------------------------------

CHILD = r"""
import os, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import fim_ref
from shredword.encoder import BPEEncoder
MERGES = np.array([[97, 98, 256], [256, 256, 257]], dtype=np.int32)
e = BPEEncoder.from_merges(MERGES, special_tokens=[b"<|s|>"])
rng = np.random.default_rng(61)
n = 6000
ids = rng.integers(97, 100, size=n).astype(np.int32)
row = np.unique(np.concatenate([rng.integers(0, 2000, 25), rng.integers(3500, n, 25), [0, 2000, 3500, n]])).astype(np.int64)
row = np.concatenate([row[:5], row[4:5], row[4:]])  # a row of 1500 ids, and two empty ones
assert np.diff(row).max() >= 1500
cuts = []
for L in np.diff(row):
    a, b = sorted(int(v) for v in rng.integers(0, L + 1, size=2))
    cuts.append((-1, -1, -1) if rng.random() < 0.3 else (a, b, int(rng.integers(2))))
cuts = np.array(cuts, dtype=np.int64)
kw = dict(pre_id=900, suf_id=901, mid_id=902, seed=77, row_base=123456789012)
for r, c in ((row, None), (row, cuts), (None, None), (None, np.array([[17, 4000, 1]]))):
    want = fim_ref.fim_ref(ids, r, cuts=c, **kw)
    os.environ.pop("SHREDWORD_BATCH_PIECE", None)
    whole = e.fim_rows(ids, r, cuts=c, src=True, seg=True, info=True, **kw)
    for piece in sys.argv[3:]:
        os.environ["SHREDWORD_BATCH_PIECE"] = piece
        got = e.fim_rows(ids, r, cuts=c, src=True, seg=True, info=True, **kw)
        for k in range(5):
            assert np.array_equal(got[k], want[k]) and np.array_equal(got[k], whole[k]), (piece, k)
e.destroy()
print("pieces ok")
"""


def test_host_pieces_in_a_fresh_process(tmp_path):
    """SHREDWORD_BATCH_PIECE of 1, 7 and values below the longest row: equal to the one-piece result and to
    the reference, at a row_base, with and without explicit cuts."""
    from conftest import PKG, TESTS
    script = tmp_path / "pieces.py"
    script.write_text(CHILD)
    env = dict(os.environ, SHREDWORD_BATCH_PIECE="7")
    r = subprocess.run([sys.executable, str(script), TESTS, PKG, "1", "7", "999", "1025"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pieces ok" in r.stdout, r.stdout + r.stderr


# ---- 9. character level -----------------------------------------------------------------------------------

DOCS = ["ab naïve abab café c".encode(), b"", "€€ab€€".encode(), b"\x80\x80\x80\x80\x80", b"abab ab <|s|> abab c ab",
        "😀ab😀".encode(), b"c", b"ab<|s|>ab"]


def test_character_cuts(enc):
    import torch
    from shredword.encoder import join_docs
    docs = DOCS * 40
    buf, off = join_docs(docs)
    kw = dict(fim_rate=0.8, spm_rate=0.5, seed=9, row_base=3)
    want = fim_ref.fim_cuts_ref(bytes(buf), off, **kw)
    assert set(want[1].tolist()) == {-1, 0, 1}
    d_buf = _dev(np.array(buf))
    piece, mode, ms = enc.fim_cuts_device(d_buf, _dev(np.array(off)), **kw)
    assert piece.dtype == torch.int64 and mode.dtype == torch.int8 and ms >= 0
    assert np.array_equal(piece.cpu().numpy(), want[0]) and np.array_equal(mode.cpu().numpy(), want[1])
    one = fim_ref.fim_cuts_ref(bytes(buf), None, **dict(kw, fim_rate=1.0))
    piece, mode, _ = enc.fim_cuts_device(d_buf, None, **dict(kw, fim_rate=1.0))
    assert np.array_equal(piece.cpu().numpy(), one[0]) and np.array_equal(mode.cpu().numpy(), one[1])
    ml = fim_ref.fim_cuts_ref(bytes(buf), off, **dict(kw, min_len=6))
    piece, mode, _ = enc.fim_cuts_device(d_buf, _dev(np.array(off)), **dict(kw, min_len=6))
    assert np.array_equal(piece.cpu().numpy(), ml[0]) and np.array_equal(mode.cpu().numpy(), ml[1])
    with pytest.raises(ValueError):
        bad = np.array(off)
        bad[3] = bad[4] + 1
        enc.fim_cuts_device(d_buf, _dev(bad), **kw)


def test_encode_fim(enc):
    from shredword.encoder import join_docs
    docs = DOCS * 25
    buf, off = join_docs(docs)
    text = bytes(buf)
    draw = dict(fim_rate=0.8, spm_rate=0.5, seed=13)
    split = 0
    for specials in (False, True):
        encode = lambda b: enc.encode(b, specials=specials)
        want, ids_in, row_in, cuts = fim_ref.fim_chars_ref(encode, text, off, **SENT, **draw)
        *got, starts, ms = enc.encode_fim(docs, specials=specials, starts=True, src=True, seg=True, info=True,
                                          **SENT, **draw)
        _same("char", [t.cpu().numpy() for t in got], want)
        # starts[out_src] are the tokens' byte offsets: those of the pieces, each encoded alone
        piece, _ = fim_ref.fim_cuts_ref(text, off, **draw)
        st = []
        for k in range(piece.size - 1):
            st += (enc.encode_spans(text[piece[k]:piece[k + 1]], specials=specials)[1] + piece[k]).tolist()
        st, src = np.array(st, dtype=np.int64), want[2]
        assert np.array_equal(starts.cpu().numpy(), st)
        assert np.array_equal(starts.cpu().numpy()[src[src >= 0]], st[src[src >= 0]])
        if specials:  # a special straddling a cut is ordinary text on both sides
            for k, doc in enumerate(docs):
                at = doc.find(b"<|s|>")
                if at < 0 or cuts[k][2] < 0:
                    continue
                inside = [c for c in piece[3 * k + 1:3 * k + 3] - piece[3 * k] if at < c < at + 5]
                whole = (ids_in[row_in[k]:row_in[k + 1]] == SP).any()
                assert whole == (not inside)
                split += bool(inside)
        res = enc.encode_fim(text, doc_offsets=off, specials=specials, **SENT, **draw)
        assert len(res) == 3 and np.array_equal(res[0].cpu().numpy(), want[0])
        # token level: fim_rows on encode_batch
        ids, row = enc.encode_batch(docs, specials=specials)
        tok = enc.fim_rows(ids, row, src=True, seg=True, info=True, **SENT, **draw)
        *got, ms = enc.encode_fim(docs, level="token", specials=specials, src=True, seg=True, info=True, **SENT, **draw)
        _same("token", [t.cpu().numpy() for t in got], tok)
        _same("token", tok, fim_ref.fim_ref(ids, row, **SENT, **draw))
    assert split >= 1
    lines = b"ab abab\nc ab\n\nabab"
    ids, line = enc.encode_lines(lines)
    *got, starts, ms = enc.encode_fim(lines, level="token", starts=True, **SENT, **draw)
    _same("lines", [t.cpu().numpy() for t in got], fim_ref.fim_ref(ids, line, **SENT, **draw)[:2])
    assert np.array_equal(starts.cpu().numpy(), enc.encode_spans(lines)[1])
    with pytest.raises(ValueError):
        enc.encode_fim(docs, level="word", **SENT)
