"""GPU tests of the span-corruption calls (include/shredword_encode.h, shred_corrupt_*): every case runs
through both ABIs, device tensors and host rows, and is compared exactly (both streams, both offset
arrays, in_src and both counts) with tests/corrupt_ref.py, which tests/test_corrupt_ref_cpu.py pins.

The encoders come from from_merges with the merges "ab" and "abab" and one special, as in
test_gpu_mlm.py.  The shapes are the smallest at which the kernels can go wrong: the edges of a tile of
BATCH_TILE ids, spans that reach from one tile into the next, row boundaries beside a tile boundary,
rows beyond one BATCH_STAGE, more runs than sentinels, views that are only element-aligned, caps that
are exact or one short, and pieces smaller than a row.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import corrupt_ref
from corrupt_ref import uniform_cum

pytestmark = pytest.mark.gpu

A, B, C, Z = ord("a"), ord("b"), ord("c"), ord("z")
MERGES = np.array([[A, B, 256], [256, 256, 257]], dtype=np.int32)  # "ab", "abab"
SPECIAL = b"<|s|>"
SP = 258            # the special's id
S0 = 999            # sentinels 999, 998, ..
DEFAULT = dict(sentinel_first=S0, p_start=0.08, lengths=(1, 5), seed=3)


@pytest.fixture(scope="module")
def enc():
    from shredword.encoder import BPEEncoder
    e = BPEEncoder.from_merges(MERGES, special_tokens=[SPECIAL])
    assert e.special_tokens[SPECIAL] == SP
    yield e
    e.destroy()


def fixed(L):
    return [0] * (L - 1) + [1.0] if L > 1 else [1.0]


def _ref(e, ids, row, *, sentinel_first, sentinel_step=-1, sentinels=100, p_start, lengths=(1, 5), length_probs=None,
         seed=0, final_sentinel=True, protect=(), protect_specials=True, index_base=0):
    cum, _ = e.corrupt_lengths(lengths, length_probs)
    V = 256 + e.num_merges
    return corrupt_ref.corrupt_ref(ids, row, p_start=p_start, len_cum=cum, seed=seed, sentinel_first=sentinel_first,
                                   sentinel_step=sentinel_step, sentinel_n=sentinels, final_sentinel=final_sentinel,
                                   protect=protect, protect_specials=protect_specials,
                                   specials=(V, V + len(e.special_tokens)), index_base=index_base)


def _dev(a, dt):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype=dt)).cuda()


def _same(name, got, want):
    """(in_ids, in_row, tgt_ids, tgt_row, in_src) against the reference's."""
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, k, g[:20], w[:20])


def _both(e, ids, row=None, **kw):
    """The call on host rows and on device tensors, both compared with the reference; -> the reference's."""
    import torch
    ids = np.asarray(ids, dtype=np.int32)
    row = None if row is None else np.asarray(row, dtype=np.int64)
    want = _ref(e, ids, row, **kw)
    _same("host", e.corrupt_rows(ids, row, src=True, **kw), want)
    d_ids = _dev(ids, np.int32)
    *got, ms = e.corrupt_device(d_ids, _dev(row, np.int64), src=True, **kw)
    assert ms >= 0 and torch.equal(d_ids.cpu(), torch.from_numpy(ids)), "the input tensor is untouched"
    _same("device", [t.cpu().numpy() for t in got], want)
    assert len(e.corrupt_rows(ids, row, **kw)) == 4  # without in_src
    return want


def _stream(n, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([A, B, C, 256, 257, SP, -1], dtype=np.int32), size=n,
                      p=[.2, .2, .2, .15, .15, .05, .05]).astype(np.int32)


def _rows(n, rows, seed):
    """rows + 1 offsets with runs of empty rows."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, n + 1, size=max(rows - 1, 0)))
    return np.concatenate([[0], cuts, [n]]).astype(np.int64)


# ---- 1. tile edges ------------------------------------------------------------------------------------

def test_tile_edges(enc):
    from shredword.encoder import BATCH_TILE
    for n in (0, 1, 3, BATCH_TILE - 1, BATCH_TILE, BATCH_TILE + 1):
        ids = _stream(n, n)
        kw = dict(DEFAULT, seed=n + 1)
        _both(enc, ids, None, **kw)
        _both(enc, ids, _rows(n, 5, n), **kw)


# ---- 2. the halo: spans that start in one tile and cover the head of the next ---------------------------

def _straddlers(ids, row, kw, edge):
    """Starts in [edge - 31, edge) of the reference whose reach passes `edge`."""
    hit = 0
    for k in range(edge - 31, edge):
        if (corrupt_ref.d(kw["seed"], k, corrupt_ref.START) >> 32) < corrupt_ref.T(kw["p_start"]):
            end = min(k + 32, int(row[np.searchsorted(row, k, side="right")]))
            hit += end > edge
    return hit


def test_halo(enc):
    from shredword.encoder import BATCH_TILE
    n = 2 * BATCH_TILE + 5
    ids = _stream(n, 77)
    kw = dict(sentinel_first=S0, p_start=0.02, length_probs=fixed(32), seed=5)
    seen = 0
    for row in (np.array([0, n]), np.array([0, BATCH_TILE + 1, 2 * BATCH_TILE + 1, n]),
                np.array([0, 7, BATCH_TILE - 3, BATCH_TILE, 2 * BATCH_TILE - 1, n])):
        for seed in (5, 6, 7, 8):
            kw["seed"] = seed
            for edge in (BATCH_TILE, 2 * BATCH_TILE):
                seen += _straddlers(ids, row, kw, edge)
            want = _both(enc, ids, row, **kw)
            if row.size == 2:
                assert np.array_equal(want[0], _both(enc, ids, None, **kw)[0])
    assert seen >= 1, "spans straddle the tile edges"
    # the clip: a span started before the tile edge ends with its row, one id after the edge
    row = np.array([0, BATCH_TILE + 1, n])
    clipped = 0
    for seed in range(5, 25):
        kw["seed"] = seed
        if _straddlers(ids, row, kw, BATCH_TILE):
            clipped += 1
            _both(enc, ids, row, **kw)
    assert clipped >= 1


# ---- 3. rows ------------------------------------------------------------------------------------------

def test_rows(enc):
    from shredword.encoder import BATCH_STAGE
    n = 2000
    ids = _stream(n, 21)
    kw = dict(DEFAULT, p_start=0.1)
    _both(enc, ids, _rows(n, BATCH_STAGE + 88, 4), **kw)          # 600 rows, many of them empty
    empty = np.concatenate([np.zeros(40, np.int64), np.full(30, 7, np.int64), np.full(50, n, np.int64)])
    _both(enc, ids, empty, **kw)
    _both(enc, ids, np.arange(n + 1), **kw)                       # rows of length 1
    _both(enc, np.zeros(0, np.int32), np.zeros(9, np.int64), **kw)  # rows, no ids
    _both(enc, np.zeros(0, np.int32), None, **kw)
    _both(enc, ids, _rows(n, 90, 5), final_sentinel=False, **kw)


# ---- 4. more runs than sentinels ------------------------------------------------------------------------

def test_sentinel_exhaustion(enc):
    from shredword.encoder import BATCH_TILE
    n = BATCH_TILE + 300
    ids = _stream(n, 31)
    row = np.array([0, 700, n])
    kw = dict(sentinel_first=S0, p_start=0.5, length_probs=fixed(1), seed=2)
    want = _both(enc, ids, row, sentinels=100, **kw)  # a row with more than 100 runs, across the tile edge
    assert (want[0][:want[1][1]] == S0 - 98).sum() == 1 and (want[0] == S0 - 99).sum() == 0
    assert want[2][want[3][1] - 1] == S0 - 99
    _both(enc, ids, row, sentinels=2, **kw)           # Rmax = 1
    _both(enc, ids, row, sentinels=2, final_sentinel=False, **kw)
    _both(enc, ids, row, sentinels=1, **kw)           # Rmax = 0: only closing sentinels
    for fin in (False, True):
        want = _both(enc, ids, row, sentinels=0, final_sentinel=fin, **kw)
        assert np.array_equal(want[0], ids) and want[2].size == 0


# ---- 5. protection --------------------------------------------------------------------------------------

def test_protection(enc):
    n = 1500
    ids = _stream(n, 41)
    row = _rows(n, 12, 41)
    kw = dict(sentinel_first=S0, p_start=0.1, lengths=(2, 6), seed=8)
    on = _both(enc, ids, row, protect_specials=True, **kw)
    off = _both(enc, ids, row, protect_specials=False, **kw)
    assert (on[0] == SP).sum() == (ids == SP).sum() > (off[0] == SP).sum()
    lst = _both(enc, ids, row, protect=[-1, C, 77], **kw)
    assert (lst[0] == C).sum() == (ids == C).sum() and (lst[0] == -1).sum() == (ids == -1).sum()
    _both(enc, ids, row, protect=list(range(90, 106)), **kw)  # 16 ids, B and C among them
    allp = _both(enc, np.full(300, C, np.int32), np.array([0, 100, 300]), protect=[C], **kw)
    assert np.array_equal(allp[0], np.full(300, C)) and allp[2].tolist() == [S0, S0]


# ---- 6. extremes ----------------------------------------------------------------------------------------

def test_extremes(enc):
    from shredword.encoder import BATCH_TILE
    n = BATCH_TILE + 9
    ids = _stream(n, 51)
    row = _rows(n, 7, 51)
    base = dict(sentinel_first=S0, seed=4, protect_specials=False)
    one = _both(enc, ids, row, p_start=1.0, **base)
    R = row.size - 1
    assert one[0].size == (np.diff(row) > 0).sum() and one[2].size == n + R + one[0].size
    zero = _both(enc, ids, row, p_start=0.0, **base)
    assert np.array_equal(zero[0], ids) and np.array_equal(zero[1], row) and (zero[2] == S0).all() and zero[2].size == R
    _both(enc, ids, row, p_start=0.2, length_probs=[1.0], **base)              # len_n = 1
    _both(enc, ids, row, p_start=0.1, length_probs=[0.5, 0.0, 0.25, 0.25], **base)
    up = _both(enc, ids, row, p_start=0.1, **dict(base, sentinel_first=-5, sentinel_step=1))
    assert up[2][0] == -5 and (up[0] == -4).any()
    _both(enc, ids, row, p_start=0.1, **dict(base, sentinel_first=7, sentinel_step=0, sentinels=3))
    big = (1 << 63) + 12345
    a = _both(enc, ids, row, p_start=0.1, index_base=big, **base)
    cut = int(row[3])
    tail = _both(enc, ids[cut:], row[3:] - cut, p_start=0.1, index_base=big + cut, **base)
    assert np.array_equal(tail[0], a[0][a[1][3]:]) and np.array_equal(tail[2], a[2][a[3][3]:])
    assert not np.array_equal(a[0], _both(enc, ids, row, p_start=0.1, **dict(base, seed=5))[0])


# ---- 7. host pieces, in a fresh process -----------------------------------------------------------------

CHILD = r"""
import os, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import corrupt_ref
from shredword.encoder import BPEEncoder
MERGES = np.array([[97, 98, 256], [256, 256, 257]], dtype=np.int32)
e = BPEEncoder.from_merges(MERGES, special_tokens=[b"<|s|>"])
rng = np.random.default_rng(61)
n = 6000
ids = rng.integers(97, 100, size=n).astype(np.int32)
row = np.unique(np.concatenate([rng.integers(0, 2000, 25), rng.integers(3500, n, 25), [0, 2000, 3500, n]])).astype(np.int64)
row = np.concatenate([row[:5], row[4:5], row[4:]])  # a row of 1500 ids, and two empty ones
assert np.diff(row).max() >= 1500
kw = dict(sentinel_first=999, p_start=0.07, seed=77, index_base=123456789012)
cum, _ = e.corrupt_lengths((1, 5))
for r in (row, None):
    want = corrupt_ref.corrupt_ref(ids, r, p_start=0.07, len_cum=cum, seed=77, sentinel_first=999, specials=(258, 259),
                                   index_base=123456789012)
    os.environ.pop("SHREDWORD_BATCH_PIECE", None)
    whole = e.corrupt_rows(ids, r, src=True, **kw)
    for piece in sys.argv[3:]:
        os.environ["SHREDWORD_BATCH_PIECE"] = piece
        got = e.corrupt_rows(ids, r, src=True, **kw)
        for k in range(5):
            assert np.array_equal(got[k], want[k]) and np.array_equal(got[k], whole[k]), (piece, k)
e.destroy()
print("pieces ok")
"""


def test_host_pieces_in_a_fresh_process(tmp_path):
    """SHREDWORD_BATCH_PIECE of 1, and others below the longest row: equal to the one-piece result and to
    the reference, at an index_base."""
    from conftest import PKG, TESTS
    script = tmp_path / "pieces.py"
    script.write_text(CHILD)
    env = dict(os.environ, SHREDWORD_BATCH_PIECE="7")
    r = subprocess.run([sys.executable, str(script), TESTS, PKG, "1", "7", "999", "1025"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pieces ok" in r.stdout, r.stdout + r.stderr


# ---- 8. the C ABI: views, caps, errors ------------------------------------------------------------------

def _opts(e, **kw):
    v = dict(sentinel_first=S0, sentinel_step=-1, sentinels=100, p_start=0.1, noise_density=0.15, lengths=(1, 5),
             length_probs=None, seed=6, final_sentinel=True, protect=(), protect_specials=True, index_base=0)
    v.update(kw)
    return e._corrupt_opts(*[v[k] for k in ("sentinel_first", "sentinel_step", "sentinels", "p_start", "noise_density",
                                            "lengths", "length_probs", "seed", "final_sentinel", "protect",
                                            "protect_specials", "index_base")])


def _raw_device(e, opts, ids, row, in_ids, in_cap, in_row, in_src, tgt, tgt_cap, tgt_row):
    import torch
    from shredword.cbase import lib
    ptr = lambda t: None if t is None else t.data_ptr()
    tn, ms = ctypes.c_size_t(12345), ctypes.c_double()
    r = lib.shred_corrupt_device(e.enc, ptr(ids), ids.numel(), ptr(row), 0 if row is None else row.numel() - 1,
                                 ctypes.byref(opts), ptr(in_ids), in_cap, ptr(in_row), ptr(in_src), ptr(tgt), tgt_cap,
                                 ptr(tgt_row), ctypes.byref(tn), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                                 ctypes.byref(ms))
    return r, tn.value


def _raw_host(e, opts, ids, row, in_ids, in_cap, in_row, in_src, tgt, tgt_cap, tgt_row):
    from shredword.cbase import lib
    ptr = lambda a: None if a is None else a.ctypes.data
    tn = ctypes.c_size_t(12345)
    r = lib.shred_corrupt_rows(e.enc, ptr(ids), ids.size, ptr(row), 0 if row is None else row.size - 1,
                               ctypes.byref(opts), ptr(in_ids), in_cap, ptr(in_row), ptr(in_src), ptr(tgt), tgt_cap,
                               ptr(tgt_row), ctypes.byref(tn))
    return r, tn.value


def test_views_that_are_only_element_aligned(enc):
    """Every buffer begins one element into its allocation; full tiles and a tail."""
    import torch
    from shredword.encoder import BATCH_TILE
    n = 2 * BATCH_TILE + 7
    ids = _stream(n, 5)
    row = _rows(n, 6, 5)
    want = _ref(enc, ids, row, sentinel_first=S0, p_start=0.1, seed=6)
    opts, _keep = _opts(enc)
    ti, tt, R = want[0].size, want[2].size, row.size - 1
    lead = lambda a, dt: torch.cat([torch.full((1,), -7, dtype=dt), torch.from_numpy(a)]).cuda()
    guard = lambda k, dt: torch.full((k + 2,), -7, dtype=dt).cuda()
    t_ids, t_row = lead(ids, torch.int32), lead(row, torch.int64)
    o_in, o_src, o_tgt = guard(ti, torch.int32), guard(ti, torch.int64), guard(tt, torch.int32)
    o_ir, o_tr = guard(R + 1, torch.int64), guard(R + 1, torch.int64)
    r = _raw_device(enc, opts, t_ids[1:], t_row[1:], o_in[1:], ti, o_ir[1:], o_src[1:], o_tgt[1:], tt, o_tr[1:])
    assert r == (ti, tt)  # the caps are exactly T_in and T_tgt
    for t, w in zip((o_in, o_ir, o_tgt, o_tr, o_src), want):
        a = t.cpu().numpy()
        assert np.array_equal(a[1:-1], w) and a[0] == -7 and a[-1] == -7, "nothing is written outside the views"


def test_sizing(enc):
    """Caps one short leave the outputs untouched and return the right counts; exact caps write nothing past."""
    n = 1300
    ids = _stream(n, 9)
    row = _rows(n, 8, 9)
    want = _ref(enc, ids, row, sentinel_first=S0, p_start=0.1, seed=6)
    opts, _keep = _opts(enc)
    ti, tt, R = want[0].size, want[2].size, row.size - 1
    for d_in, d_tgt, null in ((0, 0, False), (-1, 0, False), (0, -1, False), (0, 0, True)):
        bufs = [np.full(ti + 2, -7, np.int32), np.full(R + 3, -7, np.int64), np.full(tt + 2, -7, np.int32),
                np.full(R + 3, -7, np.int64), np.full(ti + 2, -7, np.int64)]
        for name, raw, to, back in (("host", _raw_host, lambda a: a, lambda a: a),
                                    ("device", _raw_device, lambda a: _dev(a, a.dtype), lambda t: t.cpu().numpy())):
            b = [to(a) for a in bufs]
            v = lambda k: b[k][1:]
            r = raw(enc, opts, to(ids), to(row), None if null else v(0), ti + d_in, v(1), v(4), v(2), tt + d_tgt, v(3))
            assert r == (ti, tt), (name, d_in, d_tgt, null)
            got = [back(a) for a in b]
            if d_in or d_tgt or null:
                assert all((a == -7).all() for a in got), (name, d_in, d_tgt, null)
            else:
                for k, w in enumerate(want):
                    assert np.array_equal(got[k][1:1 + w.size], w) and (got[k][1 + w.size:] == -7).all(), (name, k)
                    assert got[k][0] == -7


def test_errors_write_nothing(enc):
    from shredword.cbase import ShredCorruptOpts
    n = 1200
    ids = _stream(n, 11)
    row = _rows(n, 6, 11)
    good, _keep = _opts(enc)

    def both(opts, r=row):
        res = []
        for raw, to, back in ((_raw_host, lambda a: a, lambda a: a),
                              (_raw_device, lambda a: _dev(a, a.dtype), lambda t: t.cpu().numpy())):
            b = [to(np.full(k, -7, dt)) for k, dt in ((n, np.int32), (r.size, np.int64), (2 * n + r.size, np.int32),
                                                      (r.size, np.int64), (n, np.int64))]
            code, _ = raw(enc, opts, to(ids), to(r), b[0], n, b[1], b[4], b[2], 2 * n + r.size, b[3])
            if code < 0:
                assert all((back(a) == -7).all() for a in b)
            res.append(code)
        return tuple(res)

    assert both(good)[0] >= 0
    for bad_row in ([0, 50, 40, n], [1, 50, n], [0, 50, n - 1], [0, -1, n], [0, 50, n + 1, n]):
        assert both(good, np.array(bad_row, dtype=np.int64)) == (-6, -6), bad_row

    def raw_opts(**kw):
        cum = kw.pop("cum", uniform_cum(1, 5))
        arr = (ctypes.c_uint64 * max(len(cum), 1))(*cum)
        v = dict(index_base=0, seed=1, p_start=0.1, len_cum=arr, len_n=len(cum), sentinel_first=S0, sentinel_step=-1,
                 sentinel_n=100, final_sentinel=1, protect=None, protect_n=0, protect_specials=1)
        v.update(kw)
        return ShredCorruptOpts(*[v[k] for k in ("index_base", "seed", "p_start", "len_cum", "len_n", "sentinel_first",
                                                 "sentinel_step", "sentinel_n", "final_sentinel", "protect",
                                                 "protect_n", "protect_specials")]), arr

    assert both(raw_opts()[0])[0] >= 0
    prot = (ctypes.c_int32 * 17)(*range(17))
    for bad in (dict(cum=[0, 5, (1 << 32) - 1]), dict(cum=[5, 4, 1 << 32]), dict(cum=[0] * 32 + [1 << 32]),
                dict(len_n=0), dict(len_cum=None), dict(p_start=float("nan")), dict(p_start=-0.1), dict(p_start=1.5),
                dict(sentinel_first=2 ** 31 - 3, sentinel_step=1, sentinel_n=4),
                dict(sentinel_first=-2 ** 31 + 3, sentinel_n=5), dict(sentinel_n=-1),
                dict(protect=prot, protect_n=17), dict(protect=None, protect_n=1)):
        o, _k = raw_opts(**bad)
        assert both(o) == (-1, -1), bad
    o, _k = raw_opts(sentinel_first=2 ** 31 - 3, sentinel_step=1, sentinel_n=3)  # the last sentinel is INT32_MAX
    assert both(o)[0] >= 0
    with pytest.raises(ValueError):
        enc.corrupt_rows(ids, np.array([0, 5], dtype=np.int64), sentinel_first=S0)
    for bad in (dict(p_start=2), dict(lengths=(0, 3)), dict(lengths=(1, 33)), dict(length_probs=[0.5] * 33),
                dict(sentinels=-1), dict(sentinel_first=2 ** 31 - 3, sentinel_step=1), dict(protect=range(17)),
                dict(noise_density=1.0)):
        with pytest.raises(ValueError):
            enc.corrupt_rows(ids, **dict(dict(sentinel_first=S0), **bad))


# ---- 9. composition -------------------------------------------------------------------------------------

def test_composition_with_pad_and_decode():
    import torch
    from shredword.encoder import BPEEncoder
    sent = [b"<extra_%d>" % j for j in range(4)]
    e = BPEEncoder.from_merges(MERGES, special_tokens=[SPECIAL] + sent)
    try:
        docs = [b"ab abab c abab ab c", b"abab", b"", b"c ab ababab abc ab ab", b"ab ab ab ab ab ab ab ab abab"]
        first = e.special_tokens[sent[0]]
        kw = dict(sentinel_first=first, sentinel_step=1, sentinels=4, p_start=0.2, lengths=(1, 3), seed=1)
        i, ir, t, tr, ms = e.encode_corrupted(docs, **kw)
        ids, row = e.encode_batch(docs)
        want = _ref(e, ids, row, **kw)
        _same("encode_corrupted", [x.cpu().numpy() for x in (i, ir, t, tr)], want[:4])
        assert (want[0] >= first).any()
        batch, lengths, _ = e.pad_device(i, ir, pad_id=0)
        labels, tlen, _ = e.pad_device(t, tr, pad_id=-100)
        assert batch.shape[0] == labels.shape[0] == len(docs)
        assert np.array_equal(lengths.cpu().numpy(), np.diff(want[1])) and batch.shape[1] == np.diff(want[1]).max()
        assert np.array_equal(tlen.cpu().numpy(), np.diff(want[3])) and labels.shape[1] == np.diff(want[3]).max()
        assert (labels.cpu().numpy()[np.arange(labels.shape[1])[None, :] >= np.diff(want[3])[:, None]] == -100).all()
        # the input decodes to the text with the sentinels' own bytes where the runs were
        text, off, _ = e.decode_device(i, ir)
        text, off = text.cpu().numpy().tobytes(), off.cpu().numpy()
        toks = [bytes([b]) for b in range(256)] + [b"ab", b"abab", SPECIAL] + sent
        for r in range(len(docs)):
            assert text[off[r]:off[r + 1]] == b"".join(toks[v] for v in want[0][want[1][r]:want[1][r + 1]])
            assert any(s in text[off[r]:off[r + 1]] for s in sent) == bool((want[0][want[1][r]:want[1][r + 1]] >= first).any())
    finally:
        e.destroy()


# ---- 10. ordering and lifetime --------------------------------------------------------------------------

def test_ordered_behind_a_producer_on_the_callers_stream(enc):
    """The ids are produced by a kernel still pending on a non-default stream when the call is made."""
    import torch
    n = 1 << 20
    src = torch.from_numpy(_stream(n, 71)).cuda()
    row = torch.tensor([0, n // 3, n], dtype=torch.int64).cuda()
    kw = dict(DEFAULT, lengths=(1, 3))
    want = [t.cpu() for t in enc.corrupt_device(src, row, **kw)[:4]]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ids = torch.zeros(n, dtype=torch.int32, device="cuda")
    big = torch.ones(1 << 26, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(8):
            big = big * 1.0001 + 0.5   # keeps the stream busy
        ids.copy_(src)                 # the producer, queued behind it
        got = enc.corrupt_device(ids, row, **kw)[:4]
    s.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g.cpu(), w)


def test_first_use_in_any_order():
    """An encoder that never corrupts runs the other passes and dies cleanly; one that corrupts first, or
    last, or only, gives the same streams and the same other results."""
    from shredword.encoder import BPEEncoder
    text = b"ab abab c abab\nab ab abc\n" * 40
    ids0 = _stream(1500, 61)
    row0 = _rows(1500, 12, 61)

    def others(e):
        ids, starts, line = e.encode_spans(text, lines=True)
        pad = e.pad_rows(ids, line, bos=1, max_len=9, pad_id=-1)
        win = e.window_rows(ids, line, max_len=6, stride=2)
        mlm = e.mlm_rows(ids, line, mask_id=300, seed=2)
        return [ids, starts, line, *pad, *win, *mlm[:2]]

    def corrupts(e):
        return list(_both(e, ids0, row0, **DEFAULT))

    runs = {}
    for order in (("others",), ("corrupts",), ("others", "corrupts"), ("corrupts", "others", "corrupts")):
        e = BPEEncoder.from_merges(MERGES, special_tokens=[SPECIAL])
        try:
            for what in order:
                got = others(e) if what == "others" else corrupts(e)
                want = runs.setdefault(what, got)
                assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), order
        finally:
            e.destroy()
