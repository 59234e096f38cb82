"""GPU tests of the row decoder (include/shredword_encode.h: shred_decode_device, shred_decode_rows;
BPEEncoder.decode_rows / decode_lines / decode_device).

The expected bytes come by another route than the kernels take: encode_ref.token_bytes(merges)
joined in Python over the ids, row by row, with the separator appended and `unk` substituted for
ids outside the vocabulary.  Every case runs through both ABIs (host ids in pieces, device ids).

Cases: tiny and degenerate inputs; features on the output-tile boundary (DECODE_TILE - 1, + 0, + 1);
id counts around DECODE_CHUNK with rows on the chunk edges; ids outside the vocabulary (strict,
substituted, dropped, a dropped run longer than a tile); malformed row offsets; sizing and capacity;
host ids cut into pieces inside rows; device views from encode_spans_device, an unaligned output;
two goldens.

Not tested: the device footprint (vocabulary and scratch allocated on the first decode call).
torch.cuda.mem_get_info around the first call also sees the caching allocator's own segments for
the output tensors and other processes on the device, so the delta is not a robust observation.
The -5 branch (a vocabulary past 1 GiB) is checked by reading, not by a test.
"""
import ctypes
import re

import numpy as np
import pytest

from conftest import golden_cases
from encode_ref import derived_byte_map, model_merges, oracle_encode, token_bytes, vocab_freqs

pytestmark = pytest.mark.gpu

WORD = re.compile(rb"[^\t\r\n ]+")
REPL = b"\xef\xbf\xbd"


def _random_merges(rng, alphabet, M):
    """A trainer-like merge list over `alphabet`: operands drawn from ids that exist."""
    ids = list(alphabet)
    out = []
    seen = set()
    while len(out) < M:
        a, b = int(rng.choice(ids)), int(rng.choice(ids))
        if (a, b) in seen:
            continue
        seen.add((a, b))
        out.append([a, b, 256 + len(out)])
        ids.append(256 + len(out) - 1)
    return np.array(out, dtype=np.int32)


def _chain_merges(word: bytes, base=256):
    """Merges that fuse `word` (distinct bytes) into one token: (w0, w1), (base, w2), ..."""
    out, left = [], word[0]
    for i, c in enumerate(word[1:]):
        out.append([left, c, base + i])
        left = base + i
    return np.array(out, dtype=np.int32)


def _doubling_merges(byte, count, base):
    """(b, b), (base, base), ...: token base + i holds 2 << i copies of `byte`."""
    return np.array([[byte if i == 0 else base + i - 1, byte if i == 0 else base + i - 1, base + i]
                     for i in range(count)], dtype=np.int32)


def _tile():
    from shredword.encoder import DECODE_TILE
    return DECODE_TILE


def _chunk():
    from shredword.encoder import DECODE_CHUNK
    return DECODE_CHUNK


def _enc_from(merges, byte_map=None):
    from shredword.encoder import BPEEncoder
    return BPEEncoder.from_merges(merges, byte_map)


def _expected(toks, ids, row, sep, unk):
    """(bytes, byte_offsets) by joining token bytes in Python."""
    V = len(toks)
    bounds = [(0, len(ids))] if row is None else list(zip(row[:-1], row[1:]))
    out, boff = bytearray(), [0]
    for a, b in bounds:
        for i in ids[a:b]:
            i = int(i)
            if 0 <= i < V:
                out += toks[i]
            else:
                assert unk is not None
                out += unk
        out += sep or b""
        boff.append(len(out))
    return bytes(out), np.array(boff, dtype=np.int64)


def _check(enc, toks, ids, row=None, sep=None, unk=None):
    """decode_rows and decode_device against the Python join; returns the bytes."""
    import torch
    ids = np.asarray(ids, dtype=np.int32)
    row = None if row is None else np.asarray(row, dtype=np.int64)
    want, want_off = _expected(toks, ids, row, sep, unk)
    got, off = enc.decode_rows(ids, row, sep=sep, unk=unk)
    assert off.dtype == np.int64 and np.array_equal(off, want_off), (ids.size, sep, unk)
    assert got == want, (ids.size, sep, unk, len(got), len(want))
    d_ids = torch.from_numpy(ids).cuda()
    d_row = None if row is None else torch.from_numpy(row).cuda()
    d_out, d_off, ms = enc.decode_device(d_ids, d_row, sep=sep, unk=unk)
    assert d_out.dtype == torch.uint8 and d_off.dtype == torch.int64
    assert np.array_equal(d_off.cpu().numpy(), want_off), (ids.size, sep, unk)
    assert d_out.cpu().numpy().tobytes() == want, (ids.size, sep, unk)
    return got


def _raw_host(enc, ids, row, out, cap, boff, sep, unk, unk_len):
    from shredword.cbase import lib
    return lib.shred_decode_rows(enc.enc, ids.ctypes.data, ids.size, None if row is None else row.ctypes.data,
                                 0 if row is None else row.size - 1, None if out is None else out.ctypes.data, cap,
                                 None if boff is None else boff.ctypes.data, sep, unk, unk_len)


def _raw_dev(enc, ids, row, out, cap, boff, sep, unk, unk_len):
    import torch
    from shredword.cbase import lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.shred_decode_device(enc.enc, ids.data_ptr(), ids.numel(), None if row is None else row.data_ptr(),
                                   0 if row is None else row.numel() - 1, None if out is None else out.data_ptr(), cap,
                                   None if boff is None else boff.data_ptr(), sep, unk, unk_len, st, None)


def _raw_both(enc, ids, row, cap, sep, unk, unk_len, out_size, want_out=True):
    """Runs both ABIs on sentinel-filled buffers; returns [(result, out, byte_off)] as numpy."""
    import torch
    ids = np.asarray(ids, dtype=np.int32)
    row = None if row is None else np.asarray(row, dtype=np.int64)
    nb = 2 if row is None else row.size
    res = []
    out = np.full(out_size, 0xA5, dtype=np.uint8)
    boff = np.full(nb, -7, dtype=np.int64)
    r = _raw_host(enc, ids, row, out if want_out else None, cap, boff, sep, unk, unk_len)
    res.append((r, out, boff))
    d_ids = torch.from_numpy(ids).cuda()
    d_row = None if row is None else torch.from_numpy(row).cuda()
    d_out = torch.full((out_size,), 0xA5, dtype=torch.uint8, device="cuda")
    d_boff = torch.full((nb,), -7, dtype=torch.int64, device="cuda")
    r = _raw_dev(enc, d_ids, d_row, d_out if want_out else None, cap, d_boff, sep, unk, unk_len)
    res.append((r, d_out.cpu().numpy(), d_boff.cpu().numpy()))
    return res


def _untouched(out, boff):
    return (out == 0xA5).all() and (boff == -7).all()


# ---- 1. tiny and degenerate -------------------------------------------------------------------

def test_tiny_and_degenerate():
    rng = np.random.default_rng(3)
    merges = _random_merges(rng, [97, 98, 99, 100], 300)
    toks = token_bytes(merges)
    none = np.zeros(0, np.int32)
    with _enc_from(merges) as enc:
        data, off = enc.decode_rows(none, [0])
        assert data == b"" and off.tolist() == [0]
        data, off = enc.decode_rows(none, [0], sep=b"\n")
        assert data == b"" and off.tolist() == [0]
        data, off = enc.decode_rows(none, sep=b"\n")  # the single row's separator is still written
        assert data == b"\n" and off.tolist() == [0, 1]
        data, off = enc.decode_rows(none)
        assert data == b"" and off.tolist() == [0, 0]
        data, off = enc.decode_rows(none, [0] * 6, sep=b"\n")  # 5 empty rows
        assert data == b"\n" * 5 and off.tolist() == [0, 1, 2, 3, 4, 5]
        _check(enc, toks, none, [0])
        _check(enc, toks, none, None, sep=b"\n")
        _check(enc, toks, none, [0] * 6, sep=b"\n")
        for sep in (None, b"\n", b"\0"):
            _check(enc, toks, [300], None, sep=sep)                      # one id
            _check(enc, toks, [300], [0, 1], sep=sep)
            _check(enc, toks, [300], [0, 0, 1, 1], sep=sep)
            _check(enc, toks, rng.integers(0, 256, size=1000), None, sep=sep)   # only ids below 256
            _check(enc, toks, rng.integers(0, 256, size=1000), [0, 1, 999, 1000], sep=sep)
        ids = rng.integers(0, 556, size=10_000).astype(np.int32)
        assert enc.decode_rows(ids)[0] == enc.decode(ids)
        assert _check(enc, toks, ids) == enc.decode(ids)
        assert enc.decode_lines([97, 300, 98], [0, 1, 1, 3]) == [b"a", b"", toks[300] + b"b"]
        for bad in (b"ab", "a", 10):
            with pytest.raises(ValueError):
                enc.decode_rows(ids, sep=bad)
        with pytest.raises(ValueError):
            enc.decode_rows(ids, unk=b"123456789")


# ---- 2. output-tile boundaries ----------------------------------------------------------------

def _boundary_vocab():
    """ids 256..264: the chain of b"opqrstuvwx" (264 = the 10-byte token); 265.. : doublings of b"a"
    up to 4 * DECODE_TILE bytes; then 200 random merges over b"bcde"."""
    T = _tile()
    chain = _chain_merges(b"opqrstuvwx")
    nd = (4 * T).bit_length() - 1
    assert 2 << (nd - 1) == 4 * T
    dbl = _doubling_merges(97, nd, 256 + len(chain))
    shift = len(chain) + len(dbl)
    more = _random_merges(np.random.default_rng(18), [98, 99, 100, 101], 200)
    more = np.where(more >= 256, more + shift, more)
    merges = np.concatenate([chain, dbl, more]).astype(np.int32)
    toks = token_bytes(merges)
    tok10, tok1k, tok4t = 264, 265 + 9, 265 + nd - 1
    assert toks[tok10] == b"opqrstuvwx" and len(toks[tok1k]) == 1024 and len(toks[tok4t]) == 4 * T
    short = np.array([i for i in range(265 + nd, len(toks)) if len(toks[i]) <= 8] + [98, 99, 100, 101])
    assert short.size >= 16
    return merges, toks, tok10, tok1k, tok4t, short


def _filler(rng, toks, short, nbytes):
    """Short random tokens (1 .. a few bytes) decoding to exactly nbytes bytes."""
    ids, have = [], 0
    while have < nbytes:
        i = int(rng.choice(short))
        if have + len(toks[i]) > nbytes:
            i = 98 + int(rng.integers(0, 4))
        ids.append(i)
        have += len(toks[i])
    assert have == nbytes
    return ids


def test_output_tile_boundaries():
    T = _tile()
    merges, toks, tok10, tok1k, tok4t, short = _boundary_vocab()
    rng = np.random.default_rng(19)
    fill = lambda nbytes: _filler(rng, toks, short, nbytes)
    with _enc_from(merges) as enc:
        for d in (-1, 0, 1):
            # a 10-byte token from byte T + d - 5
            ids = fill(T + d - 5) + [tok10] + fill(100)
            got = _check(enc, toks, ids)
            assert got[T + d - 5:T + d + 5] == b"opqrstuvwx"
            _check(enc, toks, ids, [0, 7, len(ids)], sep=b"\n")
            # a separator exactly at byte T + d
            a, b = fill(T + d), fill(300)
            got = _check(enc, toks, a + b, [0, len(a), len(a), len(a) + len(b)], sep=b"\n")
            assert got[T + d:T + d + 2] == b"\n\n" and got[T + d - 1] != 10
            # T consecutive empty rows whose separators start at byte T + d: whole tiles of separators
            a, b = fill(T + d - 1), fill(77)
            row = [0] + [len(a)] * (T + 1) + [len(a) + len(b)]
            got = _check(enc, toks, a + b, row, sep=b"\n")
            assert got[T + d - 1:2 * T + d] == b"\n" * (T + 1) and got[2 * T + d] != 10
            _check(enc, toks, a + b, row)  # and without a separator
            # a 4 T-byte token from byte T + d - 3 (covers tiles that hold no token start), a 1024-byte one
            ids = fill(T + d - 3) + [tok4t] + fill(50) + [tok1k] + fill(10)
            got = _check(enc, toks, ids)
            assert got[T + d - 3:5 * T + d - 3] == b"a" * (4 * T) and got[T + d - 4] != 97
            _check(enc, toks, ids, [0, 1, len(ids) - 3, len(ids)], sep=b" ")
        for total in (2 * T, 2 * T + 1, 2 * T - 1, T, T + 1):  # total % 16 in {0, 1, 15}; ends at T, T + 1
            assert len(_check(enc, toks, fill(total))) == total
            ids = fill(total - 2)
            assert len(_check(enc, toks, ids, [0, 5, len(ids)], sep=b"\n")) == total
        assert {t % 16 for t in (2 * T, 2 * T + 1, 2 * T - 1)} == {0, 1, 15}
        # one-byte tokens only: a tile holds T of them, more than one round of the LDS staging
        ids = rng.integers(98, 102, size=3 * T + 5)
        _check(enc, toks, ids)
        _check(enc, toks, ids, [0, 1, T - 1, T - 1, 2 * T, 3 * T + 5], sep=b"\n")


# ---- 3. id-chunk boundaries -------------------------------------------------------------------

@pytest.mark.parametrize("extra", [-1, 0, 1, "3C+7"])
def test_id_chunk_boundaries(extra):
    C = _chunk()
    n = 3 * C + 7 if extra == "3C+7" else C + extra
    rng = np.random.default_rng(23)
    merges = _random_merges(rng, [97, 98, 99, 100], 300)
    toks = token_bytes(merges)
    ids = rng.integers(0, len(toks), size=n).astype(np.int32)
    edges = [e for e in range(C, n, C)]
    row = [0] + edges + [n, n]  # a row boundary on each chunk edge below n, an empty last row
    with _enc_from(merges) as enc:
        _check(enc, toks, ids)
        _check(enc, toks, ids, row, sep=b"\n")
        _check(enc, toks, ids, row)
        # an id outside the vocabulary on either side of each edge and at the very end
        for at in sorted(set([0, n - 1] + [e - 1 for e in edges] + edges)):
            bad = ids.copy()
            bad[at] = len(toks)
            with pytest.raises(ValueError):
                enc.decode_rows(bad, row, sep=b"\n")
            import torch
            with pytest.raises(ValueError):
                enc.decode_device(torch.from_numpy(bad).cuda())
        bad = ids.copy()
        bad[[0, n - 1] + [e - 1 for e in edges]] = -1
        _check(enc, toks, bad, row, sep=b"\n", unk=REPL)
        _check(enc, toks, bad, row, sep=b"\n", unk=b"")


# ---- 4. ids outside the vocabulary ------------------------------------------------------------

def test_ids_outside_the_vocabulary():
    T = _tile()
    rng = np.random.default_rng(29)
    merges = _random_merges(rng, [97, 98, 99, 100], 300)
    toks = token_bytes(merges)
    V = len(toks)
    outside = [-1, V, 2 ** 31 - 1]
    ids = rng.integers(0, V, size=3000).astype(np.int32)
    ids[rng.choice(3000, size=300, replace=False)] = rng.choice(outside, size=300)
    ids[0], ids[-1] = -1, V                       # first and last id
    ids[100:103] = [V, -1, 2 ** 31 - 1]           # a run of 3
    ids[200:210] = -1                             # a row of dropped ids only
    row = [0, 0, 200, 210, 1500, 1500, 3000]
    with _enc_from(merges) as enc:
        for r, s in ((None, None), (row, b"\n"), (row, None)):
            with pytest.raises(ValueError):
                enc.decode_rows(ids, r, sep=s)
            _check(enc, toks, ids, r, sep=s, unk=REPL)
            _check(enc, toks, ids, r, sep=s, unk=b"")
            _check(enc, toks, ids, r, sep=s, unk=b"12345678")
        assert enc.decode_lines(ids, row, unk=b"")[2] == b""
        # strict through the raw ABI: -1, nothing written
        for r, out, boff in _raw_both(enc, ids, row, 1 << 20, 10, None, -1, 1 << 20):
            assert r == -1 and _untouched(out, boff)
        for r, out, boff in _raw_both(enc, ids, row, 1 << 20, 10, REPL + b"123456", 9, 1 << 20):
            assert r == -1 and _untouched(out, boff)  # unk_len == 9
        for r, out, boff in _raw_both(enc, ids, row, 1 << 20, 256, REPL, 3, 1 << 20):
            assert r == -1 and _untouched(out, boff)  # sep out of range
        # at least a tile of dropped ids between two valid tokens: more tokens than the LDS staging holds
        for run in (T, T + 1, 3 * T + 5):
            long = [300] + [-1] * run + [301, 97] + [V] * run + [302]
            _check(enc, toks, long, unk=b"")
            _check(enc, toks, long, [0, 1, run // 2, run + 2, len(long)], sep=b"\n", unk=b"")
            _check(enc, toks, [-1] * run, [0, 5, run], sep=b"\n", unk=b"")
            _check(enc, toks, [-1] * run, unk=b"")


# ---- 5. malformed rows ------------------------------------------------------------------------

def test_malformed_rows():
    rng = np.random.default_rng(31)
    merges = _random_merges(rng, [97, 98, 99, 100], 100)
    n = 1000
    ids = rng.integers(0, 356, size=n).astype(np.int32)
    cases = [[1, 500, n],            # row_off[0] == 1
             [0, 600, 599, n],       # a decreasing pair
             [0, 500, n - 1],        # row_off[rows] == n - 1
             [0, 500, n + 1],        # row_off[rows] == n + 1
             [0, -1, n],
             [0, n + 5, n]]
    with _enc_from(merges) as enc:
        for row in cases:
            for sep in (10, -1):
                for r, out, boff in _raw_both(enc, ids, row, 1 << 16, sep, REPL, 3, 1 << 16):
                    assert r == -6 and _untouched(out, boff), (row, sep)
                for r, out, boff in _raw_both(enc, ids, row, 0, sep, None, -1, 16, want_out=False):
                    assert r == -6 and _untouched(out, boff), (row, sep)
            with pytest.raises(ValueError, match="row_offsets"):
                enc.decode_rows(ids, row, sep=b"\n")
            import torch
            with pytest.raises(ValueError, match="row_offsets"):
                enc.decode_device(torch.from_numpy(ids).cuda(), torch.tensor(row, dtype=torch.int64).cuda())
        # the encoder is still usable
        assert len(enc.decode_rows(ids, [0, 500, n], sep=b"\n")[0]) > n


# ---- 6. sizing and capacity -------------------------------------------------------------------

def test_sizing_and_capacity():
    rng = np.random.default_rng(37)
    merges = _random_merges(rng, [97, 98, 99, 100], 300)
    toks = token_bytes(merges)
    ids = rng.integers(0, len(toks), size=5000).astype(np.int32)
    row = [0, 17, 17, 4000, 5000]
    want, want_off = _expected(toks, ids, row, b"\n", None)
    need = len(want)
    flat = _expected(toks, ids, None, None, None)[0]  # one row, no separator
    with _enc_from(merges) as enc:
        for r, out, boff in _raw_both(enc, ids, row, 0, 10, None, -1, 16, want_out=False):
            assert r == need and _untouched(out, boff)               # out == NULL
        for r, out, boff in _raw_both(enc, ids, row, need - 1, 10, None, -1, need + 64):
            assert r == need and _untouched(out, boff)               # one byte short
        for r, out, boff in _raw_both(enc, ids, row, need, 10, None, -1, need + 64):
            assert r == need and out[:need].tobytes() == want and (out[need:] == 0xA5).all()
            assert np.array_equal(boff, want_off)
        for r, out, boff in _raw_both(enc, ids, None, need + 64, -1, None, -1, need + 64):
            assert r == need - 4 and out[:r].tobytes() == flat and (out[r:] == 0xA5).all()
            assert boff.tolist() == [0, r]


# ---- 7. host ids in pieces --------------------------------------------------------------------

def test_host_ids_in_pieces(monkeypatch):
    rng = np.random.default_rng(41)
    merges = _random_merges(rng, [97, 98, 99, 100], 400)
    toks = token_bytes(merges)
    n = 40_000
    ids = rng.integers(0, len(toks), size=n).astype(np.int32)
    ids[rng.choice(n, size=500, replace=False)] = -1
    ends = set(int(x) for x in rng.choice(np.arange(1, n), size=n // 300, replace=False))
    ends |= {1000, 2000, 7000, 13000, 39000}                 # rows that end exactly on a piece cut
    row = sorted(ends) + [n]
    empties = [2000, 13000, n]                               # empty rows, on piece cuts
    row = np.array([0] + sorted(row + empties), dtype=np.int64)
    rows = row.size - 1
    lens = np.diff(row)
    assert 200 < n / rows < 400 and 0.015 < (lens == 0).mean() < 0.03
    assert sum(1 for e in row[1:-1] if e % 1000 == 0) >= 6            # several rows end on a multiple of 1000
    assert ((lens == 0) & (row[1:] % 1000 == 0)).sum() >= 3           # and empty rows sit there
    with _enc_from(merges) as enc:
        one = enc.decode_rows(ids, row, sep=b"\n", unk=REPL)
        want, want_off = _expected(toks, ids, row, b"\n", REPL)
        assert one[0] == want and np.array_equal(one[1], want_off)
        monkeypatch.setenv("SHREDWORD_DECODE_PIECE", "1000")
        many = enc.decode_rows(ids, row, sep=b"\n", unk=REPL)
        assert many[0] == one[0] and np.array_equal(many[1], one[1])
        # (the ids hold byte 10 as a token too, so the rows come from the offsets, not from a split)
        assert enc.decode_lines(ids, row, unk=REPL) == [want[want_off[i]:want_off[i + 1] - 1] for i in range(rows)]
        for piece in ("1", "999", "1001"):
            monkeypatch.setenv("SHREDWORD_DECODE_PIECE", piece)
            sub = slice(0, 3000)
            r3 = row[row <= 3000]
            r3 = np.concatenate([r3, [3000]])
            got = enc.decode_rows(ids[sub], r3, sep=b"\n", unk=b"")
            w3, o3 = _expected(toks, ids[sub], r3, b"\n", b"")
            assert got[0] == w3 and np.array_equal(got[1], o3), piece
            got = enc.decode_rows(ids[sub], None, sep=b"\n", unk=b"")
            assert got[0] == _expected(toks, ids[sub], None, b"\n", b"")[0], piece


# ---- 8. device path ---------------------------------------------------------------------------

def test_device_path():
    import torch
    rng = np.random.default_rng(43)
    alpha = list(range(0x61, 0x69))
    merges = _random_merges(rng, alpha, 1000)
    toks = token_bytes(merges)
    text = b"".join(bytes(rng.choice(alpha, size=int(rng.integers(1, 50))).astype(np.uint8)) +
                    bytes([int(rng.choice([10, 32, 32, 32, 9]))]) for _ in range(30000)) + b"tail"
    with _enc_from(merges) as enc:
        d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        ids, _, line, _ = enc.encode_spans_device(d_text)
        out, boff, ms = enc.decode_device(ids, line, sep=b"\n")  # the views, as they are
        h_out, h_boff = enc.decode_rows(ids.cpu().numpy(), line.cpu().numpy(), sep=b"\n")
        assert ms > 0
        assert out.cpu().numpy().tobytes() == h_out and np.array_equal(boff.cpu().numpy(), h_boff)
        want = b"".join(WORD.findall(text))  # the identity byte map: every word's bytes, in order
        assert h_out.replace(b"\n", b"") == want and h_out.count(b"\n") == text.count(b"\n") + 1
        # an out view offset by 1 byte: the unaligned store path
        need = len(h_out)
        big = torch.full((need + 1 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        b2 = torch.full((line.numel(),), -7, dtype=torch.int64, device="cuda")
        r = _raw_dev(enc, ids, line, big[1:], need, b2, 10, None, -1)
        got = big.cpu().numpy()
        assert r == need and got[0] == 0xA5 and got[1:1 + need].tobytes() == h_out and (got[1 + need:] == 0xA5).all()
        assert np.array_equal(b2.cpu().numpy(), h_boff)
        # an empty ids tensor
        e_out, e_off, _ = enc.decode_device(ids[:0])
        assert e_out.numel() == 0 and e_off.cpu().tolist() == [0, 0]
        e_out, e_off, _ = enc.decode_device(ids[:0], line[:1], sep=b"\n")
        assert e_out.numel() == 0 and e_off.cpu().tolist() == [0]
        e_out, e_off, _ = enc.decode_device(ids[:0], sep=b"\n")
        assert e_out.cpu().tolist() == [10] and e_off.cpu().tolist() == [0, 1]
        with pytest.raises(ValueError):
            enc.decode_device(ids.cpu())                      # a host tensor
        with pytest.raises(ValueError):
            enc.decode_device(ids, line.cpu())
        with pytest.raises(ValueError):
            enc.decode_device(ids.to(torch.int64))            # the wrong dtype
        with pytest.raises(ValueError):
            enc.decode_device(ids, line.to(torch.int32))
        enc.device += 1                                       # the tensors are now on another device than the encoder
        try:
            with pytest.raises(ValueError, match="is on"):
                enc.decode_device(ids, line)
        finally:
            enc.device -= 1


# ---- 9. goldens -------------------------------------------------------------------------------

GOLDEN = [c for c in ("small_v300", "ascii1m_unk7_cov09") if c in golden_cases()]


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_round_trip(name, case_corpus, tmp_path):
    from shredword.encoder import BPEEncoder
    case, path = case_corpus(name)
    text = open(path, "rb").read()
    merges = model_merges(case["model_bytes"])
    toks = token_bytes(merges)
    freqs = vocab_freqs(case["vocab_bytes"], toks)
    unk = case["config"]["unk_id"]
    bm = derived_byte_map(merges, freqs, unk)
    (tmp_path / "g.model").write_bytes(case["model_bytes"])
    (tmp_path / "g.vocab").write_bytes(case["vocab_bytes"])
    pieces = text.split(b"\n")
    if pieces[-1] == b"":
        pieces.pop()
    with BPEEncoder(str(tmp_path / "g.model"), str(tmp_path / "g.vocab"), unk_id=unk) as enc:
        try:
            want_ids = [oracle_encode(merges, bm, p) if WORD.search(p) else np.zeros(0, np.int32) for p in pieces]
        except ValueError:  # a word longer than the encoder's limit: both reject it
            with pytest.raises(ValueError):
                enc.encode_lines(text)
            return
        ids, line = enc.encode_lines(text)
        repl = None if 0 <= unk < len(toks) else REPL  # an unk_id inside the vocabulary decodes as that id
        lines = enc.decode_lines(ids, line, unk=repl)
        assert len(lines) == len(pieces)
        want = [b"".join(toks[i] if 0 <= i < len(toks) else REPL for i in w.tolist()) for w in want_ids]
        assert lines == want
        present = np.unique(np.frombuffer(text, dtype=np.uint8))
        if np.array_equal(bm[present], present):
            assert lines == [re.sub(rb"[\t\r ]+", b"", p) for p in pieces]
