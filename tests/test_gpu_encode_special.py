"""GPU tests of special tokens matched in the text and decoded back
(include/shredword_encode.h: shred_encoder_set_specials, shred_encode_special,
shred_encode_special_device; BPEEncoder(special_tokens=...), set_special_tokens and the
specials=True keyword of the encode calls).

The expected values come from a sequential scan in this file and the oracle encoder, never from the
code under test:

* matches  per maximal run of non-delimiter bytes, left to right: the longest special that equals
           the bytes at p and fits inside the run is taken and the scan continues behind it, else
           at p + 1; a run longer than 1024 bytes is refused;
* ids      the oracle's encode of the text with the matches blanked, its starts from a walk over
           the blanked text's words with the tokens' byte lengths, merged with the matches by
           position (special i has id 256 + merges + i);
* lines    for every '\\n' the number of merged tokens that start before it.

Every case runs on the host call and the device call, with the word cache (default) and on the
direct path (SHREDWORD_ENCODE_CACHE=0).
"""
import re

import numpy as np
import pytest

from encode_ref import oracle_encode, token_bytes

pytestmark = pytest.mark.gpu

WORD = re.compile(rb"[^\t\r\n ]+")
CHUNK, SPAN, MAX_WORD = 4096, 32, 1024


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


def _reference(merges, bm, specials, text):
    """(ids, starts, line_off) by the sequential rule; computed once per input, never modified.
    Raises ValueError for a run past the word limit."""
    key = (np.asarray(merges, np.int32).tobytes(), None if bm is None else np.asarray(bm, np.int32).tobytes(),
           tuple(specials), text)
    if key in _REF:
        return _REF[key]
    firsts = {s[0] for s in specials}
    masked, matches = bytearray(text), []
    for run in WORD.finditer(text):
        p, end = run.span()
        if end - p > MAX_WORD:
            raise ValueError("run past the word limit")
        while p < end:
            best = -1
            if text[p] in firsts:
                for i, s in enumerate(specials):
                    if len(s) <= end - p and text[p:p + len(s)] == s and (best < 0 or len(s) > len(specials[best])):
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
    starts = np.array([p for p, _ in toks], dtype=np.int64)
    ids = np.array([i for _, i in toks], dtype=np.int32)
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
    line = np.concatenate([[0], np.searchsorted(starts, nl), [ids.size] if text and text[-1] != 10 else []])
    line = line.astype(np.int64)
    for a in (ids, starts, line):
        a.setflags(write=False)
    _REF[key] = (ids, starts, line)
    return _REF[key]


def _enc(merges, specials, byte_map=None):
    from shredword.encoder import BPEEncoder
    return BPEEncoder.from_merges(merges, byte_map, special_tokens=list(specials))


def _device_text(text):
    import torch
    return torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()


def _check(enc, merges, bm, specials, text, device=True):
    """The host call and the device call against the reference: ids, starts, line_off."""
    want = _reference(merges, bm, specials, text)
    ids, starts, line = enc.encode_spans(text, lines=True, specials=True)
    assert ids.dtype == np.int32 and starts.dtype == np.int64 and line.dtype == np.int64
    for got, exp, what in zip((ids, starts, line), want, ("ids", "starts", "line_off")):
        assert np.array_equal(got, exp), (what, len(text), text[:60])
    assert np.array_equal(enc.encode(text, specials=True), want[0])
    if device and text:
        d_ids, d_starts, d_line, ms = enc.encode_spans_device(_device_text(text), specials=True)
        assert len(ms) == 3
        for got, exp, what in zip((d_ids, d_starts, d_line), want, ("ids", "starts", "line_off")):
            assert np.array_equal(got.cpu().numpy(), exp), ("device " + what, len(text), text[:60])
    return want


def test_placement():
    sp = [b"<s>", b"<|e|>"]
    S, E = 256 + len(AB), 257 + len(AB)
    with _enc(AB, sp) as enc:
        assert enc.special_tokens == {b"<s>": S, b"<|e|>": E}
        assert enc.token_lengths.tolist()[256 + len(AB):] == [3, 5]
        for text in (b"<s>abc dab", b"abc dab<s>", b"<s>", b"<s><s>", b"<s><|e|><s> ab", b"ab <s><|e|> cd",
                     b"abcd<s>abcd<|e|>dcba", b"\n<s>", b"<s> <s>\t<|e|>\r\n"):
            _check(enc, AB, None, sp, text)
        assert enc.encode(b"<s>", specials=True).tolist() == [S]
        assert enc.encode(b"<s><|e|><s>", specials=True).tolist() == [S, E, S]
        # both sides of '\n', and a line with nothing else: one id in that row
        text = b"ab<s>\n<|e|>cd\n<s>\n\n  <|e|>  \nab"
        ids, _, line = _check(enc, AB, None, sp, text)
        rows = [ids[line[i]:line[i + 1]].tolist() for i in range(line.size - 1)]
        assert rows[2] == [S] and rows[3] == [] and rows[4] == [E] and rows[0][-1] == S and rows[1][0] == E
        # the device call reports the time of the special passes
        assert enc.encode_spans_device(_device_text(text), specials=True)[3][2] > 0


def test_no_merge_across_a_special():
    merges = _pairs((b"o", b"<"), (b"b", b"a"), (b"f", b"o"), (b">", b"ba"))
    sp = [b"<|x|>"]
    text = b"foo<|x|>bar"
    with _enc(merges, sp) as enc:
        ids, starts, _ = _check(enc, merges, None, sp, text)
        assert ids.tolist() == [258, ord("o"), 260, 257, ord("r")] and starts.tolist() == [0, 2, 3, 8, 10]
        plain = enc.encode(text)
        assert np.array_equal(plain, oracle_encode(merges, None, text))
        assert 256 in plain and 259 in plain and plain.tolist() != ids.tolist()  # "o<" and ">ba" merged


def test_longest_match_and_blocking():
    for sp, want in (([b"ab", b"abc"], [257, ord("d")]), ([b"abc", b"ab"], [256, ord("d")]),
                     ([b"abc", b"cd"], [256, ord("d")]), ([b"cd", b"abc"], [257, ord("d")]),
                     ([b"bc", b"abcd", b"abc"], [257])):
        with _enc(NONE, sp) as enc:
            ids, _, _ = _check(enc, NONE, None, sp, b"abcd")
            assert ids.tolist() == want, sp


def test_self_overlap():
    with _enc(AB, [b"aa"]) as enc:
        S = 256 + len(AB)
        text = b" ".join(b"a" * k for k in range(1, 10))
        ids, starts, _ = _check(enc, AB, None, [b"aa"], text)
        assert (ids == S).sum() == sum(k // 2 for k in range(1, 10))
        assert (ids == 97).sum() == 5  # the odd runs' last byte
        ids, _, _ = _check(enc, AB, None, [b"aa"], b"a" * MAX_WORD)  # the longest chain
        assert ids.tolist() == [S] * (MAX_WORD // 2)
        ids, _, _ = _check(enc, AB, None, [b"aa"], b"ab " + b"a" * (MAX_WORD - 1) + b"\nb")
        assert (ids == S).sum() == MAX_WORD // 2 - 1
    with _enc(AB, [b"aba"]) as enc:
        ids, starts, _ = _check(enc, AB, None, [b"aba"], b"ababa")
        assert ids[0] == 256 + len(AB) and starts.tolist()[:2] == [0, 3]


RANDOM_SPECIALS = [b"ab", b"aba", b"bb", b"a" * 64]


def _random_text(rng, n):
    """Over {a, b, ' ', '\\n'}, with a few runs of 64 or more 'a' where there is room."""
    t = rng.choice(np.frombuffer(b"aaabbb  \n", dtype=np.uint8), size=n)
    for _ in range(n // 600):
        at = int(rng.integers(0, n - 70))
        t[at:at + int(rng.integers(64, 71))] = 97
    return t.tobytes()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 4095, 4096, 4097, 3 * 4096 + 5])
def test_random(n):
    rng = np.random.default_rng(1000 + n)
    with _enc(AB, RANDOM_SPECIALS) as enc:
        for _ in range(3 if n < 100 else 1):
            text = _random_text(rng, n)
            ids, _, _ = _check(enc, AB, None, RANDOM_SPECIALS, text)
        if n > 4000:
            for i in range(4):
                assert (ids == 256 + len(AB) + i).any(), i


def _filler(rng, nbytes):
    out = bytearray()
    while len(out) < nbytes:
        out += bytes(rng.choice([97, 98, 99, 100], size=int(rng.integers(1, 12))).astype(np.uint8))
        out += bytes([int(rng.choice([9, 10, 13, 32, 32, 32]))])
    return out[:nbytes]


def test_chunk_and_span_boundaries():
    """A 64-byte special across every offset of a 4096-byte chunk boundary and of a 32-byte span
    boundary, glued to whatever the filler holds there."""
    rng = np.random.default_rng(44)
    big = b"<" + b"x" * 62 + b">"
    sp = [big, b"<x"]  # the short one matches where the long one is cut off
    text = (_filler(rng, 5003) * 54)[:65 * CHUNK]
    hits = []
    for d in range(1, 64):
        for at in (d * CHUNK - d, d * CHUNK + 40 * SPAN - d):
            text[at:at + 64] = big
            hits.append(at)
    text = bytes(text)
    with _enc(AB, sp) as enc:
        ids, starts, _ = _check(enc, AB, None, sp, text)
        at = starts[ids == 256 + len(AB)]
        assert at.tolist() == sorted(hits)
        # past the end of the text, and past the end of the run: no match of the long one
        for tail in (b"ab " + big[:-1], b"ab " + big[:-1] + b" >", b"ab " + big[:-1] + b"\n>"):
            ids, _, _ = _check(enc, AB, None, sp, tail)
            assert (ids == 257 + len(AB)).sum() == 1 and not (ids == 256 + len(AB)).any()
        cut = text[:hits[-1] + 63]  # the last special of the text lacks its last byte
        ids, _, _ = _check(enc, AB, None, sp, cut)
        assert (ids == 256 + len(AB)).sum() == len(hits) - 1 and ids[-62:].tolist() == [257 + len(AB)] + [120] * 61


def test_host_pieces(monkeypatch):
    """Pieces of at most 1026 bytes, each cut after a delimiter: specials on both sides of every cut."""
    rng = np.random.default_rng(45)
    sp = [b"<s>", b"ab", b"<|end|>"]
    words = []
    while sum(len(w) + 1 for w in words) < 5000:
        w = bytes(rng.choice([97, 98, 99], size=int(rng.integers(0, 9))).astype(np.uint8))
        k = int(rng.integers(0, 4))
        words.append((w + sp[k] if k < 3 else w + b"c") if rng.integers(0, 2) else (sp[k % 3] + w))
    text = b"".join(w + (b"\n" if i % 7 == 0 else b" ") for i, w in enumerate(words))[:5000]
    with _enc(AB, sp) as enc:
        one = _check(enc, AB, None, sp, text)
        monkeypatch.setenv("SHREDWORD_ENCODE_PIECE", "1026")
        many = _check(enc, AB, None, sp, text)
        for a, b in zip(one, many):
            assert np.array_equal(a, b)


def test_word_limit():
    sp = [b"abcde", b"abcd"]
    with _enc(AB, sp) as enc:
        for text in (b"abcde" * 205, b"ab " + b"abcde" * 205 + b" ab", b"d" + b"abcd" * 256):  # 1025-byte runs
            assert len(WORD.search(text[3:] if text[2:3] == b" " else text).group()) == MAX_WORD + 1
            with pytest.raises(ValueError):
                _reference(AB, None, sp, text)
            with pytest.raises(ValueError):
                enc.encode(text, specials=True)
            with pytest.raises(ValueError):
                enc.encode_spans(text, lines=True, specials=True)
            with pytest.raises(ValueError):
                enc.encode_spans_device(_device_text(text), specials=True)
        ids, _, _ = _check(enc, AB, None, sp, b"abcd" * 256)  # 1024 bytes pass
        assert ids.tolist() == [257 + len(AB)] * 256
        _check(enc, AB, None, sp, b"ab\n" + b"abcd" * 256 + b" ab")


def test_rejected_sets_leave_the_previous_one():
    sp = [b"<s>", b"<e>"]
    with _enc(AB, sp) as enc:
        for bad in ([b""], [b"<s>", b"x" * 65], [b"<a>", b"<b>", b"<a>"], [b"a\tb"], [b"a\rb"], [b"a\nb"], [b"a b"],
                    [b"<%d>" % i for i in range(257)]):
            with pytest.raises(ValueError):
                enc.set_special_tokens(bad)
            assert list(enc.special_tokens) == sp and enc.token_lengths.size == 256 + len(AB) + 2
            _check(enc, AB, None, sp, b"ab<s>cd <e>", device=False)
        most = [b"<%d>" % i for i in range(255)] + [b"y" * 64]  # the limits themselves pass
        enc.set_special_tokens(most)
        assert len(enc.special_tokens) == 256
        _check(enc, AB, None, most, b"ab<7>cd <255> <254>" + b"y" * 64 + b"<0>")
        enc.set_special_tokens("é<s>".split("<"))  # str tokens are their UTF-8 bytes
        assert list(enc.special_tokens) == ["é".encode(), b"s>"]


def test_opt_in():
    sp = [b"<s>", b"ab"]
    text = b"ab<s>cd abab\n<s> dcab<s>\n"
    with _enc(AB, sp) as enc:
        want = oracle_encode(AB, None, text)
        assert np.array_equal(enc.encode(text), want)
        assert np.array_equal(enc.encode_spans(text)[0], want)
        assert np.array_equal(enc.encode_lines(text)[0], want)
        assert np.array_equal(enc.encode_spans_device(_device_text(text))[0].cpu().numpy(), want)
        assert not np.array_equal(enc.encode(text, specials=True), want)
        enc.set_special_tokens([])  # K = 0: specials=True is encode_spans
        assert enc.special_tokens == {} and enc.token_lengths.size == 256 + len(AB)
        for a, b in zip(enc.encode_spans(text, lines=True, specials=True), enc.encode_spans(text, lines=True)):
            assert np.array_equal(a, b)
        assert np.array_equal(enc.encode(text, specials=True), want)
        d = enc.encode_spans_device(_device_text(text), specials=True)
        assert np.array_equal(d[0].cpu().numpy(), want) and d[3][2] == 0


def test_unk_byte_next_to_a_special(tmp_path):
    from shredword.encoder import BPEEncoder
    merges = _pairs((b"a", b"b"), (b"ab", b"z"), (b"z", b"<"))
    toks = token_bytes(merges)
    used = {ord("a"), ord("b"), ord("z"), ord("<")}
    # 'q' has frequency 0 and no merge uses it: the coverage rule dropped it
    vocab = b"".join(t.replace(b"\0", b"") + (b" 0\n" if t == b"q" else b" 1\n") for t in toks)
    (tmp_path / "m.model").write_bytes(merges.tobytes())
    (tmp_path / "m.vocab").write_bytes(vocab)
    bm = np.arange(256, dtype=np.int32)
    bm[ord("q")] = -1
    sp = [b"<s>"]
    assert ord("q") not in used
    with BPEEncoder(str(tmp_path / "m.model"), str(tmp_path / "m.vocab"), unk_id=-1, special_tokens=sp) as enc:
        assert np.array_equal(enc.byte_map, bm)
        text = b"abq<s>qab q<s> <s>q\nabz<s>z<s"
        ids, _, _ = _check(enc, merges, bm, sp, text)
        assert ids.tolist()[:5] == [256, -1, 259, -1, 256]


def test_round_trip():
    import torch
    sp = [b"<s>", b"<|e|>"]
    rng = np.random.default_rng(46)
    words = [bytes(rng.choice([97, 98, 99, 100], size=int(rng.integers(1, 9))).astype(np.uint8)) for _ in range(300)]
    text = b"".join(w + [b" ", b"<s> ", b"\n", b"<|e|>", b"<s>\n", b"\t"][int(rng.integers(0, 6))] for w in words)
    want = [re.sub(rb"[\t\r ]", b"", line) for line in text.split(b"\n")]
    if want[-1] == b"":
        want.pop()
    with _enc(AB, sp) as enc:
        ids, line = enc.encode_lines(text, specials=True)
        assert np.array_equal(ids, _reference(AB, None, sp, text)[0])
        d_ids, d_line = torch.from_numpy(ids).cuda(), torch.from_numpy(line).cuda()

        def rows(unk):
            data, off = enc.decode_rows(ids, line, sep=b"\n", unk=unk)
            dd, doff, _ = enc.decode_device(d_ids, d_line, sep=b"\n", unk=unk)
            assert dd.cpu().numpy().tobytes() == data and np.array_equal(doff.cpu().numpy(), off)
            return [data[off[i]:off[i + 1] - 1] for i in range(off.size - 1)]

        assert rows(None) == want and rows(b"?") == want
        assert enc.decode_lines(ids, line) == want and enc.decode(ids) == b"".join(want)
        enc.set_special_tokens([])  # the special range is outside the vocabulary again
        with pytest.raises(ValueError):
            enc.decode_rows(ids, line, sep=b"\n")
        with pytest.raises(ValueError):
            enc.decode_device(d_ids, d_line, sep=b"\n")
        with pytest.raises(ValueError):
            enc.decode(ids)
        assert rows(b"?") == [w.replace(b"<s>", b"?").replace(b"<|e|>", b"?") for w in want]
        enc.set_special_tokens([b"[END]", b"[S]", b"[unused]"])  # the same ids, other bytes
        assert rows(None) == rows(b"?") == [w.replace(b"<s>", b"[END]").replace(b"<|e|>", b"[S]") for w in want]


def test_packed_batch():
    sp = [b"<s>", b"<|e|>"]
    text = b"ab<s>cd abab\n<s> dcab<|e|>\n\n<|e|>\nabcdabcd<s>abcd d<s>"
    with _enc(AB, sp) as enc:
        ids, _, line = _reference(AB, None, sp, text)
        kw = dict(seq_len=8, pad_id=-1, positions=True, segments=True)
        for got, want in zip(enc.encode_packed(text, specials=True, **kw), enc.pack_rows(ids, line, **kw)):
            assert np.array_equal(got, want)
        assert (enc.encode_packed(text, specials=True, **kw)[0] == 256 + len(AB)).sum() == 4
        for got, want in zip(enc.encode_padded(text, specials=True, eos=7), enc.pad_rows(ids, line, eos=7)):
            assert np.array_equal(got, want)
