"""GPU tests of batches of documents: rows cut at given byte offsets
(include/shredword_encode.h: shred_encode_docs, shred_encode_docs_device; BPEEncoder.encode_docs,
encode_batch, encode_docs_device and the document rows of encode_padded / encode_packed).

The expected values never come from the code under test.  Each document is taken alone:

* ids      the oracle's encode of the document; with specials the sequential rule of
           test_gpu_encode_special.py restated here (per maximal run of non-delimiter bytes the
           longest special that fits at p is taken, else p + 1; the oracle encodes the document with
           the matches blanked; both streams merged by position);
* starts   a walk over the document's words with the tokens' byte lengths, plus doc_off[d];
* row_off  the cumulative sum of the documents' id counts.

Every case runs on the host call and the device call, with the word cache (default) and on the
direct path (SHREDWORD_ENCODE_CACHE=0).
"""
import ctypes
import re

import numpy as np
import pytest

from encode_ref import oracle_encode, token_bytes

pytestmark = pytest.mark.gpu

WORD = re.compile(rb"[^\t\r\n ]+")
MAX_WORD = 1024
EOT = b"<|endoftext|>"


@pytest.fixture(autouse=True, params=[None, "0"], ids=["cache", "direct"])
def _encoder_path(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("SHREDWORD_ENCODE_CACHE", raising=False)
    else:
        monkeypatch.setenv("SHREDWORD_ENCODE_CACHE", request.param)


def _random_merges(rng, alphabet, M):
    """A trainer-like merge list over `alphabet`: operands drawn from ids that exist."""
    ids, out, seen = list(alphabet), [], set()
    while len(out) < M:
        a, b = int(rng.choice(ids)), int(rng.choice(ids))
        if (a, b) in seen:
            continue
        seen.add((a, b))
        out.append([a, b, 256 + len(out)])
        ids.append(256 + len(out) - 1)
    return np.array(out, dtype=np.int32)


def _pairs(*pairs):
    """Merges from byte-string pairs, each operand a byte or an earlier merge's token."""
    toks, out = {bytes([b]): b for b in range(256)}, []
    for a, b in pairs:
        out.append([toks[a], toks[b], 256 + len(out)])
        toks[a + b] = 256 + len(out) - 1
    return np.array(out, dtype=np.int32)


AB = _random_merges(np.random.default_rng(3), [97, 98, 99, 100], 120)  # the model most cases use
NONE = np.zeros((0, 3), np.int32)

_REF = {}


def _doc_reference(merges, bm, specials, doc):
    """(ids, starts relative to the document) of one document encoded alone; computed once per
    input, never modified.  Raises ValueError for a run past the word limit."""
    key = (np.asarray(merges, np.int32).tobytes(), None if bm is None else np.asarray(bm, np.int32).tobytes(),
           tuple(specials), doc)
    if key in _REF:
        return _REF[key]
    firsts = {s[0] for s in specials}
    masked, matches = bytearray(doc), []
    for run in WORD.finditer(doc):
        p, end = run.span()
        if end - p > MAX_WORD:
            raise ValueError("run past the word limit")
        while specials and p < end:
            best = -1
            if doc[p] in firsts:
                for i, s in enumerate(specials):
                    if len(s) <= end - p and doc[p:p + len(s)] == s and (best < 0 or len(s) > len(specials[best])):
                        best = i
            if best < 0:
                p += 1
                continue
            L = len(specials[best])
            matches.append((p, best))
            masked[p:p + L] = b" " * L
            p += L
    masked = bytes(masked)
    wids = oracle_encode(merges, bm, masked) if WORD.search(masked) else np.zeros(0, np.int32)
    lens = [len(t) for t in token_bytes(merges)]
    toks, k = [], 0
    for w in WORD.finditer(masked):
        pos = w.start()
        while pos < w.end():
            toks.append((pos, int(wids[k])))
            pos += 1 if wids[k] < 256 else lens[wids[k]]
            k += 1
        assert pos == w.end()
    assert k == wids.size
    base = 256 + len(np.asarray(merges).reshape(-1, 3))
    toks = sorted(toks + [(p, base + i) for p, i in matches])
    ids = np.array([i for _, i in toks], dtype=np.int32)
    starts = np.array([p for p, _ in toks], dtype=np.int64)
    ids.setflags(write=False)
    starts.setflags(write=False)
    _REF[key] = (ids, starts)
    return _REF[key]


def _reference(merges, bm, specials, text, off):
    """(ids, row_off, starts) of the documents text[off[d]:off[d + 1]], each encoded alone."""
    parts = [_doc_reference(merges, bm, specials, text[off[d]:off[d + 1]]) for d in range(len(off) - 1)]
    ids = np.concatenate([p[0] for p in parts] + [np.zeros(0, np.int32)]).astype(np.int32)
    starts = np.concatenate([p[1] + off[d] for d, p in enumerate(parts)] + [np.zeros(0, np.int64)]).astype(np.int64)
    row = np.concatenate([[0], np.cumsum([p[0].size for p in parts])]).astype(np.int64)
    return ids, row, starts


def _enc(merges, specials=(), byte_map=None):
    from shredword.encoder import BPEEncoder
    return BPEEncoder.from_merges(merges, byte_map, special_tokens=list(specials))


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def _dev_text(text):
    return _dev(np.frombuffer(text, dtype=np.uint8), np.uint8)


def _offsets(n, cuts):
    return [0] + sorted(cuts) + [n]


def _check(enc, merges, bm, text, off, specials=(), device=True):
    """The host call and the device call against the reference.  specials: the registered specials
    (the calls then run with specials=True), or () for the calls with specials=False."""
    want = _reference(merges, bm, list(specials), text, off)
    on = bool(specials)
    got = enc.encode_docs(text, off, starts=True, specials=on)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and got[2].dtype == np.int64
    for g, w, what in zip(got, want, ("ids", "row_off", "starts")):
        assert np.array_equal(g, w), (what, len(text), off[:8], text[:60])
    two = enc.encode_docs(text, off, specials=on)  # without starts: the same ids and rows
    assert len(two) == 2 and np.array_equal(two[0], want[0]) and np.array_equal(two[1], want[1])
    if device:
        d = enc.encode_docs_device(_dev_text(text), _dev(off, np.int64), starts=True, specials=on)
        assert len(d) == 4 and len(d[3]) == 4
        for g, w, what in zip(d[:3], want, ("ids", "row_off", "starts")):
            assert np.array_equal(g.cpu().numpy(), w), ("device " + what, len(text), off[:8], text[:60])
        d = enc.encode_docs_device(_dev_text(text), _dev(off, np.int64), specials=on)
        assert d[2] is None and np.array_equal(d[0].cpu().numpy(), want[0]) and np.array_equal(d[1].cpu().numpy(), want[1])
    return want


def _filler(rng, nbytes, delims=(9, 10, 13, 32, 32, 32)):
    out = bytearray()
    while len(out) < nbytes:
        out += bytes(rng.choice([97, 98, 99, 100], size=int(rng.integers(1, 12))).astype(np.uint8))
        out += bytes([int(rng.choice(delims))])
    return out[:nbytes]


def test_boundary_inside_a_word():
    merges = _pairs((b"a", b"b"), (b"ab", b"c"))
    text = b"abc"
    with _enc(merges) as enc:
        glued = enc.encode(text)
        assert glued.tolist() == [257]
        ids, row, starts = _check(enc, merges, None, text, [0, 1, 3])
        assert ids.tolist() == [97, 98, 99] and row.tolist() == [0, 1, 3] and starts.tolist() == [0, 1, 2]
        assert ids.tolist() != glued.tolist()
        ids, row, starts = _check(enc, merges, None, text, [0, 2, 3])
        assert ids.tolist() == [256, 99] and row.tolist() == [0, 1, 2] and starts.tolist() == [0, 2]
        assert ids.tolist() != glued.tolist()
        for off in ([0, 0, 3], [0, 3, 3], [0, 3], [0, 0, 3, 3]):  # cuts at the ends: the whole word
            ids, row, _ = _check(enc, merges, None, text, off)
            assert ids.tolist() == [257] and row[-1] == 1
        ids, row, _ = _check(enc, merges, None, text, [0, 1, 2, 3])
        assert ids.tolist() == [97, 98, 99] and row.tolist() == [0, 1, 2, 3]
        # doc_offsets=None: one document, 1 row
        ids, row = enc.encode_docs(b"abc\nabc")
        assert ids.tolist() == [257, 257] and row.tolist() == [0, 2]
        d = enc.encode_docs_device(_dev_text(b"abc\nabc"), starts=True)
        assert d[0].tolist() == [257, 257] and d[1].tolist() == [0, 2] and d[2].tolist() == [0, 4]


def test_boundaries_at_structural_edges():
    rng = np.random.default_rng(61)
    n = 4200
    base = _filler(rng, n)
    edges = [31, 32, 33, 4095, 4096, 4097, n - 1, n]
    with _enc(AB) as enc:
        for b in edges:
            variants = []
            t = bytearray(base)
            t[max(0, b - 3):min(n, b + 3)] = b"abcdab"[:min(n, b + 3) - max(0, b - 3)]  # a word straddles b
            variants.append(bytes(t))
            t[b - 1:b] = b" "  # a delimiter before the boundary
            variants.append(bytes(t))
            if b < n:
                t = bytearray(variants[0])
                t[b:b + 1] = b"\t"  # a delimiter behind it
                variants.append(bytes(t))
                t = bytearray(variants[0])
                t[b - 1:b + 1] = b"\r\n"  # "\r\n" split by the boundary
                variants.append(bytes(t))
            for text in variants:
                assert len(text) == n
                _check(enc, AB, None, text, _offsets(n, [b]))
        # all of them at once, on a text with a word across each
        t = bytearray(base)
        for b in edges[:-1]:
            t[b - 3:min(n, b + 3)] = b"dcbadc"[:min(n, b + 3) - (b - 3)]
        ids, row, _ = _check(enc, AB, None, bytes(t), _offsets(n, edges))
        assert not np.array_equal(ids, enc.encode(bytes(t)))
        assert row.size == len(edges) + 2 and row[-1] == row[-2]  # the cut at n: an empty last document


def test_empty_documents():
    merges = _pairs((b"a", b"b"), (b"ab", b"c"))
    with _enc(merges) as enc:
        text = b"abc ab c"
        for off in ([0, 0, 8], [0, 3, 3, 8], [0, 8, 8], [0, 0, 0, 4, 4, 4, 8, 8, 8]):  # first, middle, last
            _check(enc, merges, None, text, off)
        # 1000 empty documents between the halves of one would-be word
        off = [0] + [2] * 1001 + [3]
        ids, row, _ = _check(enc, merges, None, b"abc", off)
        assert ids.tolist() == [256, 99] and row.tolist() == [0] + [1] * 1001 + [2]
        # docs > n, every byte its own document and empty ones between
        off = sorted(list(range(9)) * 3)
        _check(enc, merges, None, text, off)
        # n == 0
        for docs in (1, 5):
            ids, row, starts = _check(enc, merges, None, b"", [0] * (docs + 1))
            assert ids.size == 0 and starts.size == 0 and row.tolist() == [0] * (docs + 1)
        ids, row, starts = enc.encode_docs(b"", None, starts=True)  # NULL doc_off: one empty document
        assert ids.size == 0 and starts.size == 0 and row.tolist() == [0, 0]
        d = enc.encode_docs_device(_dev_text(b""), None, starts=True)
        assert d[0].numel() == 0 and d[1].tolist() == [0, 0] and d[2].numel() == 0
        ids, row = enc.encode_docs(b"", [0])  # no document at all
        assert ids.size == 0 and row.tolist() == [0]
        d = enc.encode_docs_device(_dev_text(b""), _dev([0], np.int64))
        assert d[0].numel() == 0 and d[1].tolist() == [0]
        # all-delimiter documents are empty rows
        text = b" \n\t\r  ab \n\n  c\r\n"
        ids, row, _ = _check(enc, merges, None, text, [0, 4, 6, 9, 12, 15, len(text)])
        assert row.tolist() == [0, 0, 0, 1, 1, 2, 2]


def test_more_documents_in_a_tile_than_the_staging_holds():
    """k_docs_expand stages the offsets of up to 1024 documents per 4096-byte output tile in LDS; a
    tile that touches more searches and walks them in global memory."""
    merges = _pairs((b"a", b"b"), (b"ab", b"c"))
    rng = np.random.default_rng(66)
    with _enc(merges) as enc:
        ids, row, _ = _check(enc, merges, None, b"abc", [0] + [2] * 3000 + [3])
        assert ids.tolist() == [256, 99] and row.tolist() == [0] + [1] * 3000 + [2]
    n = 8300
    base = bytearray(_filler(rng, n))
    base[4085:4105] = b"abcdabcdabcdabcdabcd"  # one word across bytes 4090 to 4100
    text = bytes(base)
    with _enc(AB) as enc:
        for at in (3000, 4090, 4095, 4096, 4100):  # 3000 empty documents: inside a tile of the copy, and across two
            ids, row, _ = _check(enc, AB, None, text, [0] + [at] * 3001 + [n])
            assert row[1] == row[3001] and row.size == 3003
        # every byte of a stretch its own document: more than 1024 per tile, each with a byte to copy
        off = [0] + list(range(3000, 5201)) + [n]
        ids, row, _ = _check(enc, AB, None, text, off)
        assert row.size == len(off) and (np.diff(row)[1:-1] <= 1).all()
        # and both at once, with a tile's worth of text between them
        _check(enc, AB, None, text, [0] + [100] * 1500 + list(range(4090, 6000)) + [n])


def test_every_byte_value_and_the_byte_map():
    rng = np.random.default_rng(62)
    merges = _pairs((b"\n", b"\n"), (b"\0", b"\xff"), (b"a", b"\x80"), (b"a\x80", b"\0\xff"))
    raw = rng.choice(np.frombuffer(b"\n\n\t\0\0\xff\xff\x80\x80aab \r\xc3\xa9\xfe", dtype=np.uint8), size=3000)
    text = raw.tobytes() + bytes(range(256)) * 2
    cuts = sorted(int(x) for x in rng.integers(0, len(text) + 1, size=25))
    bm = np.arange(256, dtype=np.int32)
    bm[[0, 0x80, 0xFE, ord("b")]] = -1
    for m in (None, bm):
        with _enc(merges, byte_map=m) as enc:
            ids, row, _ = _check(enc, merges, m, text, _offsets(len(text), cuts))
            assert (ids == 10).sum() == 0  # '\n' stays a delimiter inside a document
            if m is not None:
                assert (ids == -1).any()
    bad = np.arange(256, dtype=np.int32)
    bad[ord("q")] = 300
    with _enc(merges, byte_map=bad) as enc:  # an id >= 256 in the byte map: -4, with or without starts
        with pytest.raises(ValueError):
            enc.encode_docs(b"ab ab", [0, 2, 5], starts=True)
        with pytest.raises(ValueError):
            enc.encode_docs(b"ab ab", [0, 2, 5])
        with pytest.raises(ValueError):
            enc.encode_docs_device(_dev_text(b"ab ab"), _dev([0, 2, 5], np.int64))


def test_word_limit():
    with _enc(AB) as enc:
        run = (b"abcd" * 500)[:2000]
        ids, row, _ = _check(enc, AB, None, run, [0, 1000, 2000])  # cut into 1000 + 1000: passes
        assert row[1] > 0 and row[2] > row[1]
        with pytest.raises(ValueError):
            enc.encode(run)
        _check(enc, AB, None, b"ab " + run[:1024] + b"cd", [0, 3, 1027, 1029])  # a 1024-byte document
        _check(enc, AB, None, run[:1024], [0, 1024])
        text = b"ab cd\n" + run[:1025] + b" ab"
        for off in ([0, 3, len(text)], [0, 6, 6 + 1025, len(text)], [0, 5, len(text) - 1, len(text)]):
            with pytest.raises(ValueError):
                _reference(AB, None, [], text, off)
            with pytest.raises(ValueError):
                enc.encode_docs(text, off, starts=True)
            with pytest.raises(ValueError):
                enc.encode_docs_device(_dev_text(text), _dev(off, np.int64), starts=True)
        _check(enc, AB, None, text, [0, 6, 6 + 1024, len(text)])  # the same run, cut: passes


def test_specials():
    sp = [EOT]
    S = 256 + len(AB)
    with _enc(AB, sp) as enc:
        text = b"ab" + EOT + b"cd " + EOT + b" dd" + EOT
        n = len(text)
        ids, _, _ = _check(enc, AB, None, text, [0, n], specials=sp)  # wholly inside a document
        assert (ids == S).sum() == 3
        at = text.index(EOT)
        for cut in range(at + 1, at + len(EOT)):  # cut anywhere inside: no match, the bytes are words
            ids, row, _ = _check(enc, AB, None, text, [0, cut, n], specials=sp)
            assert (ids == S).sum() == 2 and (ids[:row[1]] != S).all()
        for cut in (at, at + len(EOT)):  # cut at its ends: it still matches
            ids, _, _ = _check(enc, AB, None, text, [0, cut, n], specials=sp)
            assert (ids == S).sum() == 3
        # at the first and the last bytes of a document
        doc = EOT + b"ab cd" + EOT
        ids, row, starts = _check(enc, AB, None, doc * 3, [0, len(doc), 2 * len(doc), 3 * len(doc)], specials=sp)
        for d in range(3):
            assert ids[row[d]] == S and ids[row[d + 1] - 1] == S
            assert starts[row[d]] == d * len(doc) and starts[row[d + 1] - 1] == (d + 1) * len(doc) - len(EOT)
        # specials=False never matches
        ids, _, _ = _check(enc, AB, None, text, [0, 7, n])
        assert (ids == S).sum() == 0
        # the run limit is that of the document's run, before the special cuts it
        long = b"a" * 600 + EOT + b"a" * 500
        with pytest.raises(ValueError):
            enc.encode_docs(long, [0, len(long)], specials=True)
        _check(enc, AB, None, long, [0, 600, len(long)], specials=sp)


def _raw_host(enc, text, off, n=None, cap=None, starts=True):
    """shred_encode_docs through ctypes with sentinel-filled outputs -> (code, row_off, starts)."""
    from shredword.cbase import lib
    buf = np.frombuffer(text, dtype=np.uint8)
    o = np.array(off, dtype=np.int64)
    out = np.empty(max(1, buf.size), dtype=np.int32)
    row = np.full(o.size, -77, dtype=np.int64)
    st = np.full(out.size, -77, dtype=np.int64)
    r = lib.shred_encode_docs(enc.enc, buf.ctypes.data, buf.size if n is None else n, o.ctypes.data, o.size - 1, 0,
                              out.ctypes.data, out.size if cap is None else cap, st.ctypes.data if starts else None,
                              row.ctypes.data)
    return r, row, st


def _raw_device(enc, text, off, n=None, cap=None):
    import torch
    from shredword.cbase import lib
    t, o = _dev_text(text), _dev(off, np.int64)
    out = torch.empty(max(1, t.numel()), dtype=torch.int32, device="cuda")
    row = torch.full((o.numel(),), -77, dtype=torch.int64, device="cuda")
    st = torch.full((out.numel(),), -77, dtype=torch.int64, device="cuda")
    r = lib.shred_encode_docs_device(enc.enc, t.data_ptr(), t.numel() if n is None else n, o.data_ptr(), o.numel() - 1,
                                     0, out.data_ptr(), out.numel() if cap is None else cap, st.data_ptr(),
                                     row.data_ptr(), None, None)
    torch.cuda.synchronize()
    return r, row.cpu().numpy(), st.cpu().numpy()


def test_bad_doc_off():
    text = b"ab cd ab cd ab"
    n = len(text)
    with _enc(AB) as enc:
        cases = [([1, 5, n], None),          # first entry != 0
                 ([0, 9, 5, n], None),       # a decrease
                 ([0, 5, n - 1], None),      # last entry != n
                 ([0, 5, n + 2], None),      # last entry > n
                 ([0, -1, n], None),
                 ([3], None),                # no document, but text
                 ([0, 5, n], n - 4)]         # the offsets of a longer text
        for off, short in cases:
            for raw in (_raw_host, _raw_device):
                r, row, st = raw(enc, text, off, n=short)
                assert r == -6, (off, raw.__name__, r)
                assert (row == -77).all() and (st == -77).all(), (off, raw.__name__)
            with pytest.raises(ValueError):
                enc.encode_docs(text[:short], off)
            with pytest.raises(ValueError):
                enc.encode_docs_device(_dev_text(text[:short]), _dev(off, np.int64))
        with pytest.raises(ValueError):
            enc.encode_docs(text, [])
        # a cap smaller than the result: -2, nothing written to row_off / starts
        want = _reference(AB, None, [], text, [0, 5, n])
        for raw in (_raw_host, _raw_device):
            r, row, st = raw(enc, text, [0, 5, n], cap=want[0].size - 1)
            assert r == -2, (raw.__name__, r)
            assert (row == -77).all() and (st == -77).all()
            r, row, st = raw(enc, text, [0, 5, n], cap=want[0].size)  # exactly enough
            assert r == want[0].size and np.array_equal(row, want[1]) and np.array_equal(st[:r], want[2])


def test_host_pieces(monkeypatch):
    """Pieces of at most 1026 bytes of copy, each of whole documents; one document longer than a piece."""
    rng = np.random.default_rng(63)
    sp = [b"<s>", EOT]
    docs = [bytes(_filler(rng, int(rng.integers(300, 701)), delims=(10, 32, 32, 9))) for _ in range(20)]
    for i in (3, 8, 15):
        docs[i] = docs[i][:100] + b"<s>" + docs[i][100:] + EOT
    docs.insert(11, bytes(_filler(rng, 5000, delims=(10, 32, 32, 13))))
    docs.insert(5, b"")
    text = b"".join(docs)
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).tolist()
    with _enc(AB, sp) as enc:
        one = _check(enc, AB, None, text, off)
        one_sp = _check(enc, AB, None, text, off, specials=sp)
        monkeypatch.setenv("SHREDWORD_ENCODE_PIECE", "1026")
        many = _check(enc, AB, None, text, off, device=False)
        many_sp = _check(enc, AB, None, text, off, specials=sp, device=False)
        for a, b in zip(one + one_sp, many + many_sp):
            assert np.array_equal(a, b)
        # a cap below the text's non-delimiter bytes, in pieces: the exact count passes, one less is -2
        r, row, st = _raw_host(enc, text, off, cap=one[0].size)
        assert r == one[0].size and np.array_equal(row, one[1]) and np.array_equal(st[:r], one[2])
        r, row, st = _raw_host(enc, text, off, cap=one[0].size - 1)
        assert r == -2 and (row == -77).all() and (st == -77).all()


def _random_case(rng):
    n = int(rng.integers(0, 6001))
    t = rng.choice(np.frombuffer(b"aaabbbccdd<|>  \n\t\r", dtype=np.uint8), size=n)
    for _ in range(n // 500):  # specials where there is room
        at = int(rng.integers(0, max(1, n - len(EOT))))
        if at + len(EOT) <= n:
            t[at:at + len(EOT)] = np.frombuffer(EOT, dtype=np.uint8)
    k = int(rng.integers(0, 41))
    cuts = rng.integers(0, n + 1, size=k)
    if k > 2 and rng.integers(0, 2):
        cuts[k // 2:] = cuts[:k - k // 2]  # repeats: empty documents
    return t.tobytes(), _offsets(n, [int(c) for c in cuts])


RANDOM_SPECIALS = [EOT, b"<|", b"ab"]


@pytest.mark.parametrize("seed", [700, 701, 702, 703])
def test_random_differential(seed):
    rng = np.random.default_rng(seed)
    with _enc(AB, RANDOM_SPECIALS) as enc:
        for i in range(50):
            text, off = _random_case(rng)
            if i % 2:
                _check(enc, AB, None, text, off, specials=RANDOM_SPECIALS)
            else:
                _check(enc, AB, None, text, off)


def test_downstream():
    rng = np.random.default_rng(64)
    docs = [bytes(_filler(rng, int(rng.integers(0, 200)), delims=(10, 32, 32, 9))) for _ in range(30)]
    docs[7] = b"\n\n \n"
    docs[12] = "é ab\ncd"  # a str member
    as_bytes = [d.encode() if isinstance(d, str) else d for d in docs]
    with _enc(AB) as enc:
        ids, row = enc.encode_batch(docs)
        text, off = b"".join(as_bytes), np.concatenate([[0], np.cumsum([len(d) for d in as_bytes])])
        want = _reference(AB, None, [], text, off.tolist())
        assert np.array_equal(ids, want[0]) and np.array_equal(row, want[1])
        got = enc.encode_batch(docs, starts=True)
        assert len(got) == 3 and np.array_equal(got[2], want[2])
        ids0, row0 = enc.encode_batch([])
        assert ids0.dtype == np.int32 and ids0.size == 0 and row0.dtype == np.int64 and row0.tolist() == [0]
        # decode_rows: row d is the document's own round trip
        data, boff = enc.decode_rows(ids, row)
        for d, doc in enumerate(as_bytes):
            assert data[boff[d]:boff[d + 1]] == enc.decode(enc.encode(doc)) == re.sub(rb"[\t\r\n ]", b"", doc)
        # encode_padded / encode_packed of a list, a tuple, or a text with doc_offsets
        pad_kw = dict(eos=7, pad_id=-1, mask=True)
        pack_kw = dict(seq_len=16, bos=5, pad_id=-1, positions=True, segments=True)
        for call, rows_call, kw in ((enc.encode_padded, enc.pad_rows, pad_kw), (enc.encode_packed, enc.pack_rows, pack_kw)):
            exp = rows_call(want[0], want[1], **kw)
            for got in (call(docs, **kw), call(tuple(docs), **kw), call(text, doc_offsets=off, **kw)):
                assert len(got) == len(exp)
                for g, e in zip(got, exp):
                    assert np.array_equal(g, e)
        # called as before: rows are lines
        lids, line = enc.encode_lines(text)
        assert line.size != row.size
        for g, e in zip(enc.encode_padded(text, **pad_kw), enc.pad_rows(lids, line, **pad_kw)):
            assert np.array_equal(g, e)
        for g, e in zip(enc.encode_packed(text, **pack_kw), enc.pack_rows(lids, line, **pack_kw)):
            assert np.array_equal(g, e)
        with pytest.raises(ValueError):
            enc.encode_padded(docs, doc_offsets=off)


def test_identity_with_lines():
    rng = np.random.default_rng(65)
    text = bytes(_filler(rng, 9000, delims=(10, 10, 32, 32, 9, 13))) + b"\n"
    off = [0] + (np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10) + 1).tolist()
    assert off[-1] == len(text)
    with _enc(AB) as enc:
        ids, starts, line = enc.encode_spans(text, lines=True)
        got = enc.encode_docs(text, off, starts=True)
        assert np.array_equal(got[0], ids) and np.array_equal(got[1], line) and np.array_equal(got[2], starts)
        assert np.array_equal(ids, oracle_encode(AB, None, text))
        d = enc.encode_docs_device(_dev_text(text), _dev(off, np.int64), starts=True)
        assert np.array_equal(d[0].cpu().numpy(), ids) and np.array_equal(d[1].cpu().numpy(), line)
        assert np.array_equal(d[2].cpu().numpy(), starts)
        assert d[3][0] > 0 and d[3][1] > 0 and d[3][2] == 0 and d[3][3] > 0
