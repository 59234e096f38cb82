"""GPU tests of the encoder's token byte offsets and per-line id offsets
(include/shredword_encode.h: shred_encode_spans, shred_encode_spans_device,
shred_encoder_token_lengths; BPEEncoder.encode_spans / encode_lines / encode_spans_device).

The expected values come from the oracle encoder by another route than the kernels take:

* lines   the cumulative id counts of the oracle's encodes of text.split(b"\\n") (the final empty
          piece dropped);
* starts  a walk over re.finditer(rb"[^\\t\\r\\n ]+", text) that hands each word the next oracle ids
          until their lengths (len(token_bytes), 1 for an id below 256) sum to the word's length.

Cases: tiny and degenerate texts, features on the 4096-byte workgroup boundary (bytes 4095, 4096,
4097) under both encoder paths, 1024-byte tokens, unk / remapped bytes and NUL, host text cut
into pieces inside lines, unaligned device text and the raw ABI's capacity check, two goldens.
"""
import ctypes
import re

import numpy as np
import pytest

from conftest import golden_cases
from encode_ref import derived_byte_map, model_merges, oracle_encode, token_bytes, vocab_freqs

pytestmark = pytest.mark.gpu

WORD = re.compile(rb"[^\t\r\n ]+")
CHUNK = 4096


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


def _chain_merges(word: bytes):
    """Merges that fuse `word` (distinct bytes) into one token: (w0, w1), (256, w2), ..."""
    out, left = [], word[0]
    for i, c in enumerate(word[1:]):
        out.append([left, c, 256 + i])
        left = 256 + i
    return np.array(out, dtype=np.int32)


def _lengths(merges):
    return np.array([len(t) for t in token_bytes(merges)], dtype=np.int64)


_REF = {}


def _reference(merges, bm, text):
    """(ids, starts, line_off) from the oracle; computed once per input and never modified."""
    key = (np.asarray(merges, np.int32).tobytes(), None if bm is None else np.asarray(bm, np.int32).tobytes(), text)
    if key in _REF:
        return _REF[key]
    ids = oracle_encode(merges, bm, text) if len(text) else np.zeros(0, np.int32)
    lens = _lengths(merges)
    tl = np.where(ids < 256, 1, lens[np.maximum(ids, 0)])
    starts = np.empty(ids.size, dtype=np.int64)
    k = 0
    for m in WORD.finditer(text):
        pos = m.start()
        while pos < m.end():
            starts[k] = pos
            pos += int(tl[k])
            k += 1
        assert pos == m.end()
    assert k == ids.size
    pieces = text.split(b"\n")
    if pieces[-1] == b"":
        pieces.pop()
    counts = [len(oracle_encode(merges, bm, p)) if WORD.search(p) else 0 for p in pieces]
    line = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
    for a in (ids, starts, line):
        a.setflags(write=False)
    _REF[key] = (ids, starts, line)
    return _REF[key]


def _enc_from(merges, byte_map=None):
    from shredword.encoder import BPEEncoder
    return BPEEncoder.from_merges(merges, byte_map)


def _check(enc, merges, bm, text, identity=None):
    want_ids, want_starts, want_line = _reference(merges, bm, text)
    ids, starts, line = enc.encode_spans(text, lines=True)
    assert ids.dtype == np.int32 and starts.dtype == np.int64 and line.dtype == np.int64
    assert np.array_equal(ids, want_ids), (len(text), text[:40])
    assert np.array_equal(line, want_line), (len(text), text[:40])
    assert np.array_equal(starts, want_starts), (len(text), text[:40])
    assert line[0] == 0 and line[-1] == ids.size and np.diff(line).sum() == ids.size
    ids2, line2 = enc.encode_lines(text)
    assert np.array_equal(ids2, want_ids) and np.array_equal(line2, want_line)
    ids3, starts3 = enc.encode_spans(text)
    assert np.array_equal(ids3, want_ids) and np.array_equal(starts3, want_starts)
    if identity if identity is not None else bm is None:
        toks = token_bytes(merges)
        for k in range(0, ids.size, max(1, ids.size // 2000)):
            t = toks[ids[k]]
            assert text[starts[k]:starts[k] + len(t)] == t, k
    return ids, starts, line


def test_token_lengths():
    rng = np.random.default_rng(2)
    merges = _random_merges(rng, [97, 98, 99, 100], 300)
    with _enc_from(merges) as enc:
        got = enc.token_lengths
        assert got.dtype == np.int32 and got.shape == (556,)
        assert np.array_equal(got, _lengths(merges))
    with _enc_from(np.zeros((0, 3), np.int32)) as enc:
        assert np.array_equal(enc.token_lengths, np.ones(256, np.int32))


def test_tiny_and_degenerate():
    rng = np.random.default_rng(5)
    alpha = [97, 98, 99, 100]
    merges = _random_merges(rng, alpha, 300)
    words = [bytes(rng.choice(alpha, size=L).astype(np.uint8)) for L in (1, 2, 3, 31, 32, 33, 64, 100)]
    cases = [b"", b"\n", b"\n\n\n", b"a", b"a\n", b"a\nb", b" \t\r\n" * 100,
             b" ".join(words),                      # no '\n' at all
             b"\n".join(words),                     # ends in a word, no trailing delimiter
             b"\r\n".join(words) + b"\r\n",         # CRLF
             b"\n \n\t\nab\n\n" + words[4] + b" \n ab"]
    with _enc_from(merges) as enc:
        for text in cases:
            _check(enc, merges, None, text)
        ids, starts, line = enc.encode_spans(b"", lines=True)
        assert ids.size == 0 and starts.size == 0 and line.tolist() == [0]
        assert enc.encode_spans(b"\n\n\n", lines=True)[2].tolist() == [0, 0, 0, 0]
        assert enc.encode_lines(b"a\nb")[1].tolist() == [0, 1, 2]


def _filler(rng, alpha, nbytes):
    """Random words and delimiters (some '\\n'), exactly nbytes long, ending in a space."""
    out = bytearray()
    while len(out) < nbytes:
        out += bytes(rng.choice(alpha, size=int(rng.integers(1, 12))).astype(np.uint8))
        out += bytes([int(rng.choice([9, 10, 13, 32, 32, 32]))])
    out = out[:nbytes]
    out[-1] = 32
    return bytes(out)


def _boundary_texts():
    rng = np.random.default_rng(17)
    alpha = [97, 98, 99, 100]
    texts = []
    for d in (-1, 0, 1):
        at = CHUNK + d
        # a '\n' on the boundary, between two words and inside a run of delimiters
        texts.append(_filler(rng, alpha, at - 3) + b"abc\nabc " + _filler(rng, alpha, 5000))
        texts.append(_filler(rng, alpha, at - 2) + b" \t\n\r " + _filler(rng, alpha, 700))
        # a 10-byte word from 4090 + d to 4100 + d: fused into one token (chain merges below), and
        # of bytes no merge knows (one id per byte)
        texts.append(_filler(rng, alpha, 4090 + d) + b"opqrstuvwx" + b" " + _filler(rng, alpha, 3000))
        texts.append(_filler(rng, alpha, 4090 + d) + b"0123456789" + b"\n" + _filler(rng, alpha, 3000))
        # one whole chunk of '\n' (4096 empty lines in one workgroup when d == 0)
        texts.append(_filler(rng, alpha, at - 2) + b"ab" + b"\n" * CHUNK + b"cd " + _filler(rng, alpha, 100))
        # one whole chunk of spaces between two words
        texts.append(_filler(rng, alpha, at - 2) + b"ab" + b" " * CHUNK + b"cd\nab")
    texts.append(_filler(rng, alpha, 4 * CHUNK + 3)[:-1] + b"a")  # n % 4 == 3, ends in a word
    texts.append(_filler(rng, alpha, CHUNK + 1)[:-1] + b"\n")     # n % 4 == 1
    texts.append(_filler(rng, alpha, CHUNK))                      # exactly one chunk
    texts.append(_filler(rng, alpha, CHUNK - 1) + b"a")           # exactly one chunk, no trailing delimiter
    texts.append(_filler(rng, alpha, 2 * CHUNK - 1) + b"\n")      # two chunks, '\n' last
    return texts


def _boundary_merges():
    rng = np.random.default_rng(18)
    chain = _chain_merges(b"opqrstuvwx")  # ids 256..264
    more = _random_merges(rng, [97, 98, 99, 100], 200)
    more = np.where(more >= 256, more + len(chain), more)
    return np.concatenate([chain, more]).astype(np.int32)


@pytest.mark.parametrize("cache", ["1", "0"])
def test_chunk_boundaries(cache, monkeypatch):
    """Both encoder paths: the word cache (default) and the direct kernel."""
    monkeypatch.setenv("SHREDWORD_ENCODE_CACHE", cache)
    merges = _boundary_merges()
    with _enc_from(merges) as enc:
        for text in _boundary_texts():
            ids, starts, line = _check(enc, merges, None, text)
            i = text.find(b"opqrstuvwx")
            if i >= 0:  # one token, 10 bytes, across the boundary
                k = int(np.searchsorted(starts, i))
                assert starts[k] == i and ids[k] == 264 and (k + 1 == ids.size or starts[k + 1] >= i + 11)
            i = text.find(b"0123456789")
            if i >= 0:  # one id per byte
                k = int(np.searchsorted(starts, i))
                assert starts[k:k + 10].tolist() == list(range(i, i + 10)) and ids[k:k + 10].tolist() == list(b"0123456789")
            if b"\n" * CHUNK in text:
                assert (np.diff(line) == 0).sum() >= CHUNK - 1


def test_long_tokens():
    merges = np.array([[97 if i == 0 else 255 + i, 97 if i == 0 else 255 + i, 256 + i] for i in range(10)], np.int32)
    text = b"a" * 1024 + b"\n" + b"a" * 1023
    with _enc_from(merges) as enc:
        assert enc.token_lengths[256:].tolist() == [2 << i for i in range(10)]
        ids, starts, line = _check(enc, merges, None, text)
    assert ids.tolist() == [265, 264, 263, 262, 261, 260, 259, 258, 257, 256, 97]
    assert starts[0] == 0 and starts[1] == 1025
    # the second word's binary decomposition: 512 + 256 + ... + 2 + 1 bytes
    assert starts[1:].tolist() == (1025 + np.concatenate([[0], np.cumsum([512 >> i for i in range(9)])])).tolist()
    assert line.tolist() == [0, 1, 11]


def test_unk_nul_and_remapped_bytes():
    rng = np.random.default_rng(9)
    alpha = list(range(0x61, 0x6b))
    merges = _random_merges(rng, alpha, 500)
    bm = np.arange(256, dtype=np.int32)
    bm[0x6a] = -1  # a dropped byte -> unk (never merges)
    bm[0x80] = 3   # a byte remapped to another byte's id
    text = bytes(rng.integers(0, 256, size=100_000, dtype=np.uint8).tolist())
    words = b"".join(bytes(rng.choice(alpha, size=int(rng.integers(1, 30))).astype(np.uint8)) +
                     bytes([int(rng.choice([10, 32, 32]))]) for _ in range(5000))
    with _enc_from(merges, bm) as enc:
        for t in (text, words + text[:5000] + b"\n" + words):
            ids, _, _ = _check(enc, merges, bm, t, identity=False)  # lengths only: ids are not the text's bytes
            assert (ids == -1).any() and b"\0" in t
    bad = np.arange(256, dtype=np.int32)
    bad[0x41] = 300
    with _enc_from(merges, bad) as enc:
        assert enc.encode(b"ab A").size == 3  # plain encode still works
        with pytest.raises(ValueError):
            enc.encode_spans(b"ab A")
        with pytest.raises(ValueError):
            enc.encode_lines(b"ab A")


def test_host_text_in_pieces(monkeypatch):
    """Pieces are cut after any delimiter, so lines straddle pieces: same output as one piece."""
    rng = np.random.default_rng(8)
    alpha = [97, 98, 99]
    merges = _random_merges(rng, alpha, 400)
    text = b"".join(bytes(rng.choice(alpha, size=int(rng.integers(1, 60))).astype(np.uint8)) +
                    (b"\n" if rng.integers(0, 300) == 0 else bytes([int(rng.choice([9, 13, 32]))]))
                    for _ in range(40000))
    assert text.count(b"\n") > 50 and len(text) / (text.count(b"\n") + 1) > 5000
    with _enc_from(merges) as enc:
        one = _check(enc, merges, None, text)
        monkeypatch.setenv("SHREDWORD_ENCODE_PIECE", "5000")
        many = _check(enc, merges, None, text)
        for a, b in zip(one, many):
            assert np.array_equal(a, b)
        _check(enc, merges, None, text[:-1] + b"\n")  # ends in '\n'
        with pytest.raises(ValueError):
            enc.encode_spans(b"ab " * 3000 + b"a" * 1100 + b" ab", lines=True)


def test_device_path_and_line_cap():
    import torch
    from shredword.cbase import lib
    rng = np.random.default_rng(21)
    alpha = list(range(0x61, 0x69))
    merges = _random_merges(rng, alpha, 1000)
    text = b"".join(bytes(rng.choice(alpha, size=int(rng.integers(1, 50))).astype(np.uint8)) +
                    bytes([int(rng.choice([10, 32, 32, 32, 9]))]) for _ in range(30000)) + b"tail"
    with _enc_from(merges) as enc:
        h_ids, h_starts, h_line = _check(enc, merges, None, text)
        big = torch.from_numpy(np.frombuffer(b"x" + text, dtype=np.uint8).copy()).cuda()
        view = big[1:]  # 1-byte offset: the unaligned load path
        ids, starts, line, (enc_ms, span_ms) = enc.encode_spans_device(view)
        assert ids.dtype == torch.int32 and starts.dtype == torch.int64 and line.dtype == torch.int64
        assert enc_ms > 0 and span_ms > 0
        assert np.array_equal(ids.cpu().numpy(), h_ids)
        assert np.array_equal(starts.cpu().numpy(), h_starts)
        assert np.array_equal(line.cpu().numpy(), h_line)
        ids, starts, line, _ = enc.encode_spans_device(view, starts=False)
        assert starts is None and np.array_equal(line.cpu().numpy(), h_line)
        ids, starts, line, _ = enc.encode_spans_device(view, lines=False)
        assert line is None and np.array_equal(starts.cpu().numpy(), h_starts)
        e_ids, e_st, e_line, _ = enc.encode_spans_device(big[:0])
        assert e_ids.numel() == 0 and e_st.numel() == 0 and e_line.cpu().tolist() == [0]
        with pytest.raises(ValueError):
            enc.encode_spans_device(torch.zeros(4, dtype=torch.uint8))  # host tensor
        # the raw ABI: a line buffer one entry short is refused, L reported, nothing written
        L = h_line.size - 1
        assert L == text.count(b"\n") + 1
        out = torch.empty(view.numel(), dtype=torch.int32, device="cuda")
        lbuf = torch.full((L + 1,), -7, dtype=torch.int64, device="cuda")
        nl = ctypes.c_size_t(0)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        r = lib.shred_encode_spans_device(enc.enc, view.data_ptr(), view.numel(), out.data_ptr(), out.numel(), None,
                                          lbuf.data_ptr(), L, ctypes.byref(nl), st, None)
        assert r == -2 and nl.value == L
        assert (lbuf == -7).all().item()
        r = lib.shred_encode_spans_device(enc.enc, view.data_ptr(), view.numel(), out.data_ptr(), out.numel(), None,
                                          lbuf.data_ptr(), L + 1, ctypes.byref(nl), st, None)
        assert r == h_ids.size and nl.value == L and np.array_equal(lbuf.cpu().numpy(), h_line)
        # and the host ABI
        buf = np.frombuffer(text, dtype=np.uint8)
        hout = np.empty(buf.size, dtype=np.int32)
        hl = np.full(L + 1, -7, dtype=np.int64)
        r = lib.shred_encode_spans(enc.enc, buf.ctypes.data, buf.size, hout.ctypes.data, hout.size, None,
                                   hl.ctypes.data, L, ctypes.byref(nl))
        assert r == -2 and nl.value == L and (hl == -7).all()


GOLDEN = [c for c in ("small_v300", "ascii1m_unk7_cov09") if c in golden_cases()]


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_lines(name, case_corpus, tmp_path):
    from shredword.encoder import BPEEncoder
    case, path = case_corpus(name)
    text = open(path, "rb").read()
    merges = model_merges(case["model_bytes"])
    freqs = vocab_freqs(case["vocab_bytes"], token_bytes(merges))
    unk = case["config"]["unk_id"]
    bm = derived_byte_map(merges, freqs, unk)
    (tmp_path / "g.model").write_bytes(case["model_bytes"])
    (tmp_path / "g.vocab").write_bytes(case["vocab_bytes"])
    with BPEEncoder(str(tmp_path / "g.model"), str(tmp_path / "g.vocab"), unk_id=unk) as enc:
        try:
            want_ids, want_starts, want_line = _reference(merges, bm, text)
        except ValueError:  # a word longer than the encoder's limit: both reject it
            with pytest.raises(ValueError):
                enc.encode_lines(text)
            return
        ids, line = enc.encode_lines(text)
        assert np.array_equal(ids, want_ids) and np.array_equal(line, want_line)
        assert np.diff(line).sum() == ids.size
        assert np.array_equal(enc.encode_spans(text)[1], want_starts)
