"""GPU tests of the masked-LM calls (include/shredword_encode.h, shred_mlm_*): every case runs through
both ABIs, device tensors and host rows, and is compared exactly (ids, labels, return value) with
tests/mlm_ref.py, which tests/test_mlm_ref_cpu.py pins.

The encoders come from from_merges with the merges "ab" and "abab", so the token shapes are under the
test's control; the shapes are the smallest at which the kernels can go wrong: the edges of a tile of
BATCH_TILE ids, words that straddle tiles or cover several, rows beyond one BATCH_STAGE, views that
are only element-aligned, and pieces smaller than a row.

Not tested: the device footprint in bytes.  The library's allocations are not visible to torch's
counters and the device's free memory moves with other processes; as test_gpu_encoder_lifetime.py
does for the other passes, the check is that the masking state is created by the first masking call in
any order of first use, that an encoder which never masks gives the other passes' results and dies
cleanly, and that calls keep succeeding.
"""
import ctypes
import re

import numpy as np
import pytest

import mlm_ref

pytestmark = pytest.mark.gpu

A, B, C, Z = ord("a"), ord("b"), ord("c"), ord("z")
MERGES = np.array([[A, B, 256], [256, 256, 257]], dtype=np.int32)  # "ab", "abab"
SPECIAL = b"<|s|>"
MASK = 300
IGN = -100


@pytest.fixture(scope="module")
def enc():
    from shredword.encoder import BPEEncoder
    e = BPEEncoder.from_merges(MERGES, special_tokens=[SPECIAL])
    yield e
    e.destroy()


def _ref(e, ids, row, starts, *, mask_id, p=0.15, seed=0, mask_prob=0.8, random_prob=0.1, random_vocab=None,
         protect=(), protect_specials=True, whole_word=False, ignore_id=IGN, index_base=0):
    V = 256 + e.num_merges
    return mlm_ref.mlm_ref(ids, row, p=p, seed=seed, p_mask=mask_prob, p_random=random_prob, mask_id=mask_id,
                           rand_vocab=V if random_vocab is None else random_vocab, protect=protect,
                           protect_specials=protect_specials, specials=(V, V + len(e.special_tokens)),
                           whole_word=whole_word, starts=starts, lens=e.token_lengths.tolist(), ignore_id=ignore_id,
                           index_base=index_base)


def _dev(a, dt):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype=dt)).cuda()


def _both(e, ids, row=None, starts=None, **kw):
    """The call on host rows and on device tensors, both compared with the reference; -> the reference's."""
    import torch
    ids = np.asarray(ids, dtype=np.int32)
    want = _ref(e, ids, row, starts, **kw)
    host = e.mlm_rows(ids, row, starts=starts, **kw)
    d_ids = _dev(ids, np.int32)
    o, l, s, ms = e.mlm_device(d_ids, _dev(row, np.int64), starts=_dev(starts, np.int64), **kw)
    assert ms >= 0 and torch.equal(d_ids.cpu(), torch.from_numpy(ids)), "the input tensor is untouched"
    for name, got in (("host", host), ("device", (o.cpu().numpy(), l.cpu().numpy(), s))):
        assert got[2] == want[2], (name, got[2], want[2])
        for k in (0, 1):
            assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (name, k)
    return want


def _stream(n, seed, p_gap=0.4):
    """n ids of the vocabulary with consistent starts: words of a few tokens, a delimiter between them."""
    rng = np.random.default_rng(seed)
    ids = rng.choice(np.array([A, B, C, 256, 257], dtype=np.int32), size=n)
    lens = np.where(ids == 256, 2, np.where(ids == 257, 4, 1)).astype(np.int64)
    gap = (rng.random(n) < p_gap).astype(np.int64)
    if n:
        gap[0] = 0
    starts = np.cumsum(lens) - lens + np.cumsum(gap)
    return ids.astype(np.int32), starts


def _rows(n, rows, seed):
    """rows + 1 offsets with runs of empty rows, some of them inside words."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, n + 1, size=max(rows - 1, 0)))
    return np.concatenate([[0], cuts, [n]]).astype(np.int64)


# ---- 1. tile boundaries -----------------------------------------------------------------------------

@pytest.mark.parametrize("whole", [False, True])
def test_tile_boundaries(enc, whole):
    from shredword.encoder import BATCH_TILE
    for n in (0, 1, 3, BATCH_TILE - 1, BATCH_TILE, BATCH_TILE + 1):
        ids, starts = _stream(n, n)
        kw = dict(mask_id=MASK, p=0.3, seed=n + 1, whole_word=whole)
        _both(enc, ids, None, starts, **kw)
        _both(enc, ids, _rows(n, 5, n), starts, **kw)


def _raw_device(e, ids_t, row_t, starts_t, out_t, lab_t, opts):
    import torch
    from shredword.cbase import lib
    ms = ctypes.c_double()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.shred_mlm_device(e.enc, ids_t.data_ptr(), ids_t.numel(), None if row_t is None else row_t.data_ptr(),
                                0 if row_t is None else row_t.numel() - 1, ctypes.byref(opts),
                                None if starts_t is None else starts_t.data_ptr(), out_t.data_ptr(), lab_t.data_ptr(),
                                st, ctypes.byref(ms))


@pytest.mark.parametrize("whole", [False, True])
def test_views_that_are_only_element_aligned(enc, whole):
    """ids, out, labels (and starts) begin 4 (8) bytes into their allocations; full tiles and a tail."""
    import torch
    from shredword.encoder import BATCH_TILE
    n = 2 * BATCH_TILE + 7
    ids, starts = _stream(n, 5)
    kw = dict(mask_id=MASK, p=0.4, seed=11, whole_word=whole)
    want = _ref(enc, ids, None, starts, **kw)
    opts, _keep = enc._mlm_opts(MASK, 0.4, 11, 0.8, 0.1, None, (), True, whole, IGN, 0)
    big = lambda a, dt, fill: torch.cat([torch.full((1,), fill, dtype=dt), torch.from_numpy(a)]).cuda()
    t_ids, t_st = big(ids, torch.int32, -7), big(starts, torch.int64, -7)
    t_out = torch.full((n + 2,), -7, dtype=torch.int32).cuda()
    t_lab = torch.full((n + 2,), -7, dtype=torch.int32).cuda()
    r = _raw_device(enc, t_ids[1:], None, t_st[1:] if whole else None, t_out[1:n + 1], t_lab[1:n + 1], opts)
    assert r == want[2]
    assert np.array_equal(t_out[1:n + 1].cpu().numpy(), want[0]) and np.array_equal(t_lab[1:n + 1].cpu().numpy(), want[1])
    for t in (t_out, t_lab):
        assert t[0].item() == -7 and t[n + 1].item() == -7, "nothing is written outside the views"


# ---- 2. whole words and tiles -------------------------------------------------------------------------

def _one_fate(labels, lo, hi):
    picked = labels[lo:hi] != IGN
    return picked.all() or not picked.any()


def test_word_across_a_tile_boundary(enc):
    """A word whose first token is the last of tile 0; the rest sits in tile 1."""
    from shredword.encoder import BATCH_TILE
    n = BATCH_TILE + 40
    ids = np.full(n, C, dtype=np.int32)
    gap = np.ones(n, dtype=np.int64)          # one-token words ...
    gap[BATCH_TILE:BATCH_TILE + 9] = 0        # ... but for the word [BATCH_TILE - 1, BATCH_TILE + 9)
    gap[0] = 0
    starts = np.arange(n, dtype=np.int64) + np.cumsum(gap)
    fates = set()
    for seed in range(8):
        _, labels, _ = _both(enc, ids, None, starts, mask_id=MASK, p=0.5, seed=seed, whole_word=True)
        assert _one_fate(labels, BATCH_TILE - 1, BATCH_TILE + 9), seed
        fates.add(bool(labels[BATCH_TILE] != IGN))
    assert fates == {False, True}


def _encoded_word(e, length, lead):
    """ids, starts of `lead` short words and then one word of `length` single-byte tokens, from the encoder."""
    text = b"ab " * lead + b"c" * length + b" abab c"
    ids, row, starts = e.encode_docs(text, None, starts=True)
    k0 = lead
    assert ids.size == lead + length + 2 and (ids[k0:k0 + length] == C).all()
    return ids, starts, k0


@pytest.mark.parametrize("length,long_words", [(1024, False), (3001, True)])
def test_word_longer_than_a_tile(length, long_words):
    from shredword.encoder import BPEEncoder
    e = BPEEncoder.from_merges(MERGES, long_words=long_words)
    try:
        ids, starts, k0 = _encoded_word(e, length, 500)  # the word starts mid-tile
        fates = set()
        for seed in range(8):
            _, labels, sel = _both(e, ids, None, starts, mask_id=MASK, p=0.5, seed=seed, whole_word=True)
            assert _one_fate(labels, k0, k0 + length), seed
            fates.add(bool(labels[k0] != IGN))
        assert fates == {False, True}
    finally:
        e.destroy()


# ---- 3. the begin rule ------------------------------------------------------------------------------

def test_documents_without_a_delimiter(enc):
    """"abab" + "abab": contiguous starts, but the row boundary begins a word."""
    ids, row, starts = enc.encode_batch([b"abab", b"abab"], starts=True)
    assert ids.tolist() == [257, 257] and starts.tolist() == [0, 4] and row.tolist() == [0, 1, 2]
    diff = 0
    for seed in range(16):
        kw = dict(mask_id=MASK, p=0.5, seed=seed, whole_word=True)
        _, two, _ = _both(enc, ids, row, starts, **kw)
        _, one, _ = _both(enc, ids, None, starts, **kw)
        assert (one[0] == IGN) == (one[1] == IGN)  # one row: one word
        diff += (two[0] == IGN) != (two[1] == IGN)
    assert diff > 0


def test_specials_inside_a_run(enc):
    text = b"ab<|s|>abab ab<|s|> <|s|>ab"
    ids, row, starts = enc.encode_docs(text, None, starts=True, specials=True)
    S = enc.special_tokens[SPECIAL]
    assert ids.tolist() == [256, S, 257, 256, S, S, 256]
    for whole in (False, True):
        kw = dict(mask_id=MASK, p=1.0, seed=3, whole_word=whole)
        _, labels, sel = _both(enc, ids, row, starts, protect_specials=True, **kw)
        assert sel == 4 and (labels[ids == S] == IGN).all() and (labels[ids != S] != IGN).all()
        _, labels, sel = _both(enc, ids, row, starts, protect_specials=False, **kw)
        assert sel == 7
    # a special is a word of its own, selected on its own
    fates = set()
    for seed in range(12):
        _, labels, _ = _both(enc, ids, row, starts, mask_id=MASK, p=0.5, seed=seed, whole_word=True,
                             protect_specials=False)
        fates.add((bool(labels[0] != IGN), bool(labels[1] != IGN), bool(labels[2] != IGN)))
    assert len(fates) > 2


def test_protected_id_inside_a_word(enc):
    ids = np.array([C, C, B, C, C, C], dtype=np.int32)
    starts = np.arange(6, dtype=np.int64)
    fates = set()
    for seed in range(12):
        _, labels, _ = _both(enc, ids, None, starts, mask_id=MASK, p=0.5, seed=seed, whole_word=True, protect=[B, 77])
        assert labels[2] == IGN and _one_fate(labels, 0, 2) and _one_fate(labels, 3, 6)
        fates.add((bool(labels[0] != IGN), bool(labels[3] != IGN)))
    assert len(fates) > 2  # the two halves are units of their own
    _both(enc, ids, None, starts, mask_id=MASK, p=1.0, whole_word=False, protect=list(range(90, 106)))  # 16 ids, B and C


def test_unk_tokens():
    from shredword.encoder import BPEEncoder
    bm = np.arange(256, dtype=np.int32)
    bm[Z] = -1
    e = BPEEncoder.from_merges(MERGES, byte_map=bm)
    try:
        ids, row, starts = e.encode_docs(b"azzb zz abz", None, starts=True)
        assert ids.tolist() == [A, -1, -1, B, -1, -1, 256, -1]
        for seed in range(4):
            for whole in (False, True):
                _, labels, _ = _both(e, ids, row, starts, mask_id=MASK, p=0.5, seed=seed, whole_word=whole)
                if whole:
                    assert _one_fate(labels, 0, 4) and _one_fate(labels, 4, 6) and _one_fate(labels, 6, 8)
        _, labels, sel = _both(e, ids, row, starts, mask_id=MASK, p=1.0, whole_word=True, protect=[-1])
        assert sel == 3 and (labels[ids == -1] == IGN).all()
    finally:
        e.destroy()


# ---- 4. rows ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("whole", [False, True])
def test_rows(enc, whole):
    from shredword.encoder import BATCH_STAGE
    n = 2500
    ids, starts = _stream(n, 21, p_gap=0.2)
    kw = dict(mask_id=MASK, p=0.3, seed=5, whole_word=whole)
    flat = _both(enc, ids, None, starts, **kw)
    one = _both(enc, ids, np.array([0, n], dtype=np.int64), starts, **kw)
    many = _both(enc, ids, _rows(n, BATCH_STAGE + 90, 4), starts, **kw)  # more rows than one stage, many of them empty
    empty = np.concatenate([np.zeros(40, np.int64), np.full(30, 7, np.int64), np.full(50, n, np.int64)])
    _both(enc, ids, empty, starts, **kw)
    _both(enc, np.zeros(0, np.int32), np.zeros(9, np.int64), np.zeros(0, np.int64), **kw)  # rows, no ids
    assert np.array_equal(flat[1], one[1])
    if not whole:  # rows do not matter per token
        assert np.array_equal(flat[0], many[0]) and np.array_equal(flat[1], many[1])
    else:
        assert not np.array_equal(flat[1], many[1])


# ---- 5. probabilities ---------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.0, 1.0])
@pytest.mark.parametrize("split", [(1.0, 0.0), (0.0, 1.0), (0.0, 0.0), (0.8, 0.1)])
def test_probabilities(enc, p, split):
    ids, starts = _stream(1500, 8)
    row = _rows(1500, 20, 8)
    for vocab in (1, 2 ** 31 - 1):
        kw = dict(mask_id=-3, p=p, seed=9, mask_prob=split[0], random_prob=split[1], random_vocab=vocab)
        out, labels, sel = _both(enc, ids, row, starts, **kw)
        assert sel == (0 if p == 0 else 1500)
        if p == 1 and split == (1.0, 0.0):
            assert (out == -3).all()
        if p == 1 and split == (0.0, 1.0):
            assert (out == 0).all() if vocab == 1 else (np.unique(out).size > 1400 and out.min() >= 0)
        if p == 0 or split == (0.0, 0.0):
            assert np.array_equal(out, ids)
        _both(enc, ids, row, starts, whole_word=True, **kw)


# ---- 6. in place ------------------------------------------------------------------------------------

@pytest.mark.parametrize("whole", [False, True])
def test_in_place(enc, whole):
    import torch
    from shredword.encoder import BATCH_TILE
    n = 3 * BATCH_TILE + 5
    ids, starts = _stream(n, 13)
    row = _rows(n, 30, 13)
    kw = dict(mask_id=MASK, p=0.4, seed=2, whole_word=whole)
    want = _both(enc, ids, row, starts, **kw)  # out of place, the input checked untouched
    d_ids = _dev(ids, np.int32)
    o, l, s, _ = enc.mlm_device(d_ids, _dev(row, np.int64), starts=_dev(starts, np.int64), out=d_ids, **kw)
    assert o.data_ptr() == d_ids.data_ptr() and s == want[2]
    assert np.array_equal(d_ids.cpu().numpy(), want[0]) and np.array_equal(l.cpu().numpy(), want[1])
    h_ids = ids.copy()  # the host call in place, through the C ABI
    from shredword.cbase import lib
    opts, _keep = enc._mlm_opts(MASK, 0.4, 2, 0.8, 0.1, None, (), True, whole, IGN, 0)
    lab = np.empty(n, dtype=np.int32)
    r = lib.shred_mlm_rows(enc.enc, h_ids.ctypes.data, n, row.ctypes.data, row.size - 1, ctypes.byref(opts),
                           starts.ctypes.data if whole else None, h_ids.ctypes.data, lab.ctypes.data)
    assert r == want[2] and np.array_equal(h_ids, want[0]) and np.array_equal(lab, want[1])


# ---- 7. host pieces ---------------------------------------------------------------------------------

@pytest.mark.parametrize("whole", [False, True])
def test_host_pieces(enc, whole, monkeypatch):
    n = 6000
    ids, starts = _stream(n, 31, p_gap=0.15)
    row = _rows(n, 60, 31)
    row = np.unique(np.concatenate([row[(row <= 2000) | (row >= 3500)], [2000, 3500]])).astype(np.int64)
    row = np.concatenate([row[:5], row[4:5], row[4:]])  # a row of 1500 ids, and two empty ones
    assert np.diff(row).max() >= 1500
    kw = dict(mask_id=MASK, p=0.3, seed=77, whole_word=whole, index_base=123456789012)
    monkeypatch.delenv("SHREDWORD_BATCH_PIECE", raising=False)
    want = _both(enc, ids, row, starts, **kw)
    flat = _both(enc, ids, None, starts, **kw)
    for piece in ("1", "7", "999", "1025"):
        monkeypatch.setenv("SHREDWORD_BATCH_PIECE", piece)
        for r, w in ((row, want), (None, flat)):
            got = enc.mlm_rows(ids, r, starts=starts, **kw)
            assert got[2] == w[2] and np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]), piece


# ---- 8. determinism ---------------------------------------------------------------------------------

def test_determinism_and_index_base(enc):
    n = 2000
    ids, starts = _stream(n, 41)
    row = _rows(n, 25, 41)
    for whole in (False, True):
        kw = dict(mask_id=MASK, p=0.3, whole_word=whole)
        a = _both(enc, ids, row, starts, seed=1, **kw)
        b = _both(enc, ids, row, starts, seed=1, **kw)
        c = _both(enc, ids, row, starts, seed=2, **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[1], c[1])
        base = (1 << 63) + 12345
        e = _both(enc, ids, row, starts, seed=1, index_base=base, **kw)
        assert not np.array_equal(a[1], e[1])
        # a shard of the stream at its own index_base is the stream's tail
        cut = int(row[10])
        tail = _both(enc, ids[cut:], row[10:] - cut, starts[cut:], seed=1, index_base=base + cut, **kw)
        assert np.array_equal(tail[0], e[0][cut:]) and np.array_equal(tail[1], e[1][cut:])


# ---- 9. errors: nothing is written ------------------------------------------------------------------

def _opts(**kw):
    from shredword.cbase import ShredMlmOpts
    v = dict(index_base=0, p=0.5, seed=1, p_mask=0.8, p_random=0.1, mask_id=MASK, ignore_id=IGN, rand_vocab=258,
             protect=None, protect_n=0, protect_specials=1, whole_word=0)
    v.update(kw)
    return ShredMlmOpts(*[v[k] for k in ("index_base", "p", "seed", "p_mask", "p_random", "mask_id", "ignore_id",
                                         "rand_vocab", "protect", "protect_n", "protect_specials", "whole_word")])


def _raw_both(e, ids, row, starts, opts):
    """The C ABI on sentinel-filled outputs, host and device -> the two return values; asserts that a
    negative one left the outputs alone."""
    import torch
    from shredword.cbase import lib
    n = ids.size
    out, lab = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    r_host = lib.shred_mlm_rows(e.enc, ids.ctypes.data, n, None if row is None else row.ctypes.data,
                                0 if row is None else row.size - 1, ctypes.byref(opts),
                                None if starts is None else starts.ctypes.data, out.ctypes.data, lab.ctypes.data)
    t_out, t_lab = _dev(out * 0 - 7, np.int32), _dev(lab * 0 - 7, np.int32)
    r_dev = _raw_device(e, _dev(ids, np.int32), _dev(row, np.int64), _dev(starts, np.int64), t_out, t_lab, opts)
    if r_host < 0:
        assert (out == -7).all() and (lab == -7).all()
    if r_dev < 0:
        assert (t_out == -7).all().item() and (t_lab == -7).all().item()
    return r_host, r_dev


def test_errors_write_nothing(enc):
    from shredword.encoder import BATCH_TILE
    n = BATCH_TILE + 100
    ids, starts = _stream(n, 51)
    row = _rows(n, 10, 51)
    assert _raw_both(enc, ids, row, starts, _opts())[0] >= 0  # the arguments are fine as they stand
    prot = (ctypes.c_int32 * 17)(*range(17))
    for bad in (dict(p=-0.01), dict(p=1.01), dict(p=float("nan")), dict(p_mask=float("nan")), dict(p_random=-1.0),
                dict(p_mask=0.75, p_random=0.5), dict(whole_word=1, _starts=None), dict(protect=prot, protect_n=17),
                dict(protect=None, protect_n=1), dict(rand_vocab=0), dict(rand_vocab=2 ** 31), dict(rand_vocab=-1)):
        st = bad.pop("_starts", starts)
        assert _raw_both(enc, ids, row, st, _opts(**bad)) == (-1, -1), bad
    assert _raw_both(enc, ids, row, starts, _opts(p_mask=0.5, p_random=0.5)) [0] >= 0  # T sum = 2^32 exactly
    assert _raw_both(enc, ids, row, starts, _opts(p_random=0.0, rand_vocab=0))[0] >= 0  # not needed without random
    for whole in (0, 1):
        for bad_row in ([0, 50, 40, n], [1, 50, n], [0, 50, n - 1], [0, -1, n], [0, 50, n + 1, n]):
            r = np.array(bad_row, dtype=np.int64)
            assert _raw_both(enc, ids, r, starts, _opts(whole_word=whole)) == (-6, -6), bad_row
    # rows without a row_off, and labels on top of an input
    from shredword.cbase import lib
    lab = np.full(n, -7, np.int32)
    o = _opts()
    assert lib.shred_mlm_rows(enc.enc, ids.ctypes.data, n, None, 3, ctypes.byref(o), None, lab.ctypes.data,
                              lab.ctypes.data) == -1
    assert lib.shred_mlm_rows(enc.enc, ids.ctypes.data, n, None, 0, ctypes.byref(o), None, lab.ctypes.data,
                              lab.ctypes.data) == -1
    assert lib.shred_mlm_rows(enc.enc, ids.ctypes.data, n, None, 0, None, None, lab.ctypes.data, lab.ctypes.data) == -1
    assert (lab == -7).all()


def test_byte_map_with_a_merged_id_refuses_whole_words():
    from shredword.encoder import BPEEncoder
    bm = np.arange(256, dtype=np.int32)
    bm[Z] = 256
    e = BPEEncoder.from_merges(MERGES, byte_map=bm)
    try:
        ids, starts = _stream(50, 1)
        assert _raw_both(e, ids, None, starts, _opts(whole_word=1)) == (-4, -4)
        assert _raw_both(e, ids, None, starts, _opts(whole_word=0))[0] >= 0
        with pytest.raises(ValueError):
            e.mlm_rows(ids, mask_id=MASK, whole_word=True, starts=starts)
    finally:
        e.destroy()


def test_python_argument_checks(enc):
    ids, starts = _stream(20, 2)
    for bad in (dict(p=2), dict(mask_prob=0.75, random_prob=0.5), dict(random_vocab=0), dict(protect=range(17)),
                dict(whole_word=True), dict(whole_word=True, starts=starts[:5]), dict(mask_id=2 ** 31)):
        with pytest.raises(ValueError):
            enc.mlm_rows(ids, **dict(dict(mask_id=MASK), **bad))
    with pytest.raises(ValueError):
        enc.mlm_rows(ids, np.array([0, 5], dtype=np.int64), mask_id=MASK)


# ---- 10. end to end ---------------------------------------------------------------------------------

DOCS = [b"ab abab c abab\nab", b"abab", b"", b"c ab\tababab abc", b"ab ab ab ab ab ab ab ab abab"]


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("truncate", ["left", "right"])
def test_encode_mlm(enc, whole, truncate):
    from shredword.encoder import join_docs
    pad_kw = dict(bos=1, eos=2, max_len=7, truncate=truncate, pad_id=0)
    kw = dict(mask_id=MASK, p=0.5, seed=6, whole_word=whole)
    batch, labels, lengths, attn, selected = (x.cpu().numpy() if hasattr(x, "cpu") else x
                                              for x in enc.encode_mlm(DOCS, **kw, **pad_kw))
    plain, plain_len = enc.encode_padded(DOCS, **pad_kw)
    assert batch.shape == labels.shape == attn.shape == plain.shape and np.array_equal(lengths, plain_len)
    cols = np.arange(batch.shape[1])[None, :]
    inside = (cols >= 1) & (cols < lengths[:, None] - 1)  # neither bos, eos nor padding
    assert np.array_equal(attn.astype(bool), cols < lengths[:, None])
    assert (labels[~inside] == IGN).all() and np.array_equal(batch[~inside], plain[~inside])
    picked = labels != IGN
    assert picked.any() and (~picked & inside).any()
    assert np.array_equal(labels[picked], plain[picked])
    assert np.array_equal(np.where(picked, labels, batch), plain)  # un-masking gives encode_padded's batch
    # the flat masking, padded by the host pad call, is the same batch
    ids, row, starts = enc.encode_batch(DOCS, starts=True)
    f_ids, f_lab, f_sel = enc.mlm_rows(ids, row, starts=starts, **kw)
    assert f_sel == selected
    assert np.array_equal(enc.pad_rows(f_ids, row, **pad_kw)[0], batch)
    assert np.array_equal(enc.pad_rows(f_lab, row, **dict(pad_kw, bos=IGN, eos=IGN, pad_id=IGN))[0], labels)
    if whole:  # the selected tokens cover whole whitespace-delimited words of the documents
        text, off = join_docs(DOCS)
        lens = enc.token_lengths
        covered = np.zeros(text.size, dtype=bool)
        for k in np.nonzero(f_lab != IGN)[0]:
            covered[starts[k]:starts[k] + lens[ids[k]]] = True
        fates = set()
        for d in range(len(DOCS)):
            for m in re.finditer(rb"[^\t\r\n ]+", DOCS[d]):
                span = covered[off[d] + m.start():off[d] + m.end()]
                assert span.all() or not span.any(), (d, m.group())
                fates.add(bool(span.all()))
        assert fates == {False, True}


# ---- 11. the masking state is created by the first masking call -------------------------------------

def test_first_use_in_any_order():
    """An encoder that never masks runs the other passes and dies cleanly; one that masks first, or last,
    or only, gives the same masking and the same other results."""
    from shredword.encoder import BPEEncoder
    text = b"ab abab c abab\nab ab abc\n" * 40
    ids0, starts0 = _stream(1500, 61)
    row0 = _rows(1500, 12, 61)

    def others(e):
        ids, starts, line = e.encode_spans(text, lines=True)
        pad = e.pad_rows(ids, line, bos=1, max_len=9, pad_id=-1)
        win = e.window_rows(ids, line, max_len=6, stride=2)
        return [ids, starts, line, *pad, *win]

    def masks(e):
        res = []
        for whole in (False, True):
            res += list(_both(e, ids0, row0, starts0, mask_id=MASK, p=0.3, seed=4, whole_word=whole)[:2])
        return res

    runs = {}
    for order in (("others",), ("masks",), ("others", "masks"), ("masks", "others", "masks")):
        e = BPEEncoder.from_merges(MERGES)
        try:
            for what in order:
                got = others(e) if what == "others" else masks(e)
                want = runs.setdefault(what, got)
                assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), order
        finally:
            e.destroy()
