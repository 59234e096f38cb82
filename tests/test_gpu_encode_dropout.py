"""GPU tests of BPE-dropout (include/shredword_encode.h: shred_encoder_set_dropout;
csrc/hip/encode_dropout.hip; BPEEncoder(dropout=, seed=) / set_dropout).

Every case compares the ids exactly with the Python reference of encode_dropout_ref.py, which
test_encode_dropout_ref_cpu.py pins (hash, threshold, p = 0 against the oracle).  The real model is the
golden mixed2m_v4000 (3,744 merges); no text is above 64 KB.
"""
import numpy as np
import pytest

from conftest import load_case
from encode_dropout_ref import WORD, ref_dropout_docs, ref_dropout_encode
from encode_long_ref import AA, AA_AAAA, LOCAL_MIN, LOCAL_MIN_2, pairs, ref_starts
from encode_ref import derived_byte_map, model_merges, token_bytes, vocab_freqs
from encode_shapes import SHAPES, UNUSED_BYTE

pytestmark = pytest.mark.gpu

GOLDEN = "mixed2m_v4000"
BANANA = pairs((b"a", b"n"), (b"an", b"a"))
HAND = {"aa": AA, "aa_aaaa": AA_AAAA, "local_min": LOCAL_MIN, "local_min_2": LOCAL_MIN_2, "banana": BANANA}
EOT = b"<|endoftext|>"
DELIMS = np.frombuffer(b"\t\r\n ", dtype=np.uint8)


def _enc(merges, bm=None, **kw):
    from shredword.encoder import BPEEncoder
    return BPEEncoder.from_merges(merges, bm, **kw)


def _dev(data: bytes):
    import torch
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def _device_ids(enc, text: bytes) -> np.ndarray:
    return enc.encode_device(_dev(text))[0].cpu().numpy()


_REF = {}


def _ref(merges, bm, text, p, seed, base=0):
    """The reference's ids: computed once per input, shared by the cases, never modified."""
    key = (merges.tobytes(), None if bm is None else bm.tobytes(), text, p, seed, base)
    if key not in _REF:
        ids = ref_dropout_encode(merges, bm, text, p, seed, base)
        ids.setflags(write=False)
        _REF[key] = ids
    return _REF[key]


@pytest.fixture(scope="module")
def model(case_corpus):
    """(merges, byte map, corpus bytes, the corpus without its delimiters) of the golden model."""
    case, path = case_corpus(GOLDEN)
    merges = model_merges(case["model_bytes"])
    freqs = vocab_freqs(case["vocab_bytes"], token_bytes(merges))
    bm = derived_byte_map(merges, freqs, case["config"]["unk_id"])
    corpus = open(path, "rb").read()[:256 * 1024]
    arr = np.frombuffer(corpus, dtype=np.uint8)
    solid = arr[~np.isin(arr, DELIMS)].tobytes()
    assert UNUSED_BYTE not in corpus
    return merges, bm, corpus, solid


def _cut(corpus, lo, hi):
    """corpus[lo:hi] moved to whole words: from behind a delimiter to behind a delimiter."""
    lo = corpus.index(b" ", lo) + 1
    return corpus[lo:corpus.rindex(b" ", lo, hi) + 1]


# ---- hand tables -----------------------------------------------------------------------------------

def _hand_text():
    rng = np.random.default_rng(12)
    words = [bytes(rng.choice(list(b"abcdxy"), size=int(rng.integers(1, 41))).tolist()) for _ in range(120)]
    words += [b"a" * k for k in (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 64, 100)]
    seps = [b" ", b"\n", b"\t", b" \r\n"]
    return b"".join(w + seps[i % 4] for i, w in enumerate(words)) + b"banana " * 800 + b"abcd"


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("table", sorted(HAND))
def test_hand_tables(table, p):
    merges, text = HAND[table], _hand_text()
    assert len(text) > 2 * 4096
    with _enc(merges) as enc:
        for seed in (1, 2 ** 63 + 5):
            enc.set_dropout(p, seed)
            assert enc.dropout == (p, seed)
            want = _ref(merges, None, text, p, seed)
            assert np.array_equal(enc.encode(text), want)
            assert np.array_equal(_device_ids(enc, text), want)


def test_same_pair_twice_in_a_word_is_decided_per_boundary():
    """banana holds (a, n) at two boundaries: at p = 0.5 words with exactly one of them merged exist,
    which a decision per word (or per pair) could not produce."""
    text = b"banana " * 600
    with _enc(BANANA, dropout=0.5, seed=3) as enc:
        ids = enc.encode(text)
    assert np.array_equal(ids, _ref(BANANA, None, text, 0.5, 3))
    starts = ref_starts(BANANA, text, ids)
    per_word = np.bincount(starts // 7, weights=((ids == 256) | (ids == 257)).astype(float), minlength=600)
    assert {0, 1, 2} <= set(per_word.astype(int).tolist())


# ---- word-length edges under a real model ------------------------------------------------------------

@pytest.mark.parametrize("packing", ["packed", "unpacked"])
def test_word_length_edges(model, packing):
    """Words of 1 .. 1024 bytes: the LDS strip limit kStrip = 32 and the global-scratch form up to its
    limit, on 16-bit packed strips and, with a byte of no text sent to -1, on the unpacked ones."""
    merges, bm, corpus, solid = model
    if packing == "unpacked":
        bm = bm.copy()
        bm[UNUSED_BYTE] = -1
    words, at = [], 0
    for rep in range(3):
        for L in (1, 2, 31, 32, 33, 64, 1023, 1024):
            words.append(solid[at:at + L])
            at += L + 13
    text = b" ".join(words) + b"\n"
    with _enc(merges, bm) as enc:
        for p, seed in ((0.1, 4), (0.5, 5)):
            enc.set_dropout(p, seed)
            want = _ref(merges, bm, text, p, seed)
            assert np.array_equal(enc.encode(text), want)
            assert np.array_equal(_device_ids(enc, text), want)
            plain = _ref(merges, bm, text, 0.0, 0)
            assert want.size > plain.size


# ---- geometry ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("start", [0, 31, 32, 4095, 4096, 4080])
def test_word_at_span_and_chunk_edges(model, start):
    """One 40-byte word (the global-scratch form) beginning at a span or chunk edge, or straddling the
    chunk seam at 4096; n is no multiple of 32."""
    merges, bm, corpus, solid = model
    word = solid[1000:1040]
    prefix = corpus[:start - 1] + b" " if start else b""
    text = prefix + word + b" " + _cut(corpus, 9000, 9300) + b"end"
    text += b"x" * (len(text) % 32 == 0)
    assert len(prefix) == start and len(text) % 32 != 0
    assert any(m.start() == start and m.end() == start + 40 for m in WORD.finditer(text))
    with _enc(merges, bm, dropout=0.5, seed=8) as enc:
        want = _ref(merges, bm, text, 0.5, 8)
        assert np.array_equal(enc.encode(text), want)
        assert np.array_equal(_device_ids(enc, text), want)


@pytest.mark.parametrize("packing", ["packed", "unpacked"])
def test_unaligned_device_view(model, packing):
    """A device text that begins one byte behind an aligned address: the kernels' unaligned instance;
    the positions count from the view's first byte."""
    merges, bm, corpus, solid = model
    if packing == "unpacked":
        bm = bm.copy()
        bm[UNUSED_BYTE] = -1
    text = _cut(corpus, 20000, 30000) + solid[300:700] + b" x"
    whole = _dev(b"#" + text)
    assert whole.data_ptr() % 16 == 0
    with _enc(merges, bm, dropout=0.1, seed=21) as enc:
        ids = enc.encode_device(whole[1:])[0].cpu().numpy()
        assert np.array_equal(ids, _ref(merges, bm, text, 0.1, 21))


# ---- staging invariance ---------------------------------------------------------------------------------

def _staging_text(corpus, solid):
    """64 KB: natural text with words of 1024, 1000, 700 and 300 bytes put in, some at a line's end."""
    parts, at = [], 0
    for i, L in enumerate((1024, 300, 1000, 700, 1024, 33)):
        parts += [_cut(corpus, at, at + 9500), solid[2000 * i:2000 * i + L], b"\n" if i % 2 else b" "]
        at += 9500
    text = b"".join(parts)
    text += _cut(corpus, at, at + 65536 - len(text))
    assert 60000 < len(text) <= 65536 and max(len(w) for w in WORD.findall(text)) == 1024
    return text


def test_staging_invariance(model, monkeypatch):
    """The host calls in pieces of 1026 bytes give the ids of the default piece, of the device call and
    of the reference: a piece adds its own offset to the positions."""
    merges, bm, corpus, solid = model
    text = _staging_text(corpus, solid)
    # documents of every size, cut at any byte: inside runs too (which only shortens the words)
    rng = np.random.default_rng(3)
    cuts = np.unique(np.concatenate([rng.integers(0, len(text), 40), np.arange(30000, 30400, 50)]))
    off = np.concatenate([[0], cuts, [cuts[-1]], [len(text)]]).astype(np.int64)  # one empty document
    p, seed = 0.5, 17
    want = _ref(merges, bm, text, p, seed)
    want_docs, want_row = ref_dropout_docs(merges, bm, text, off, p, seed)
    with _enc(merges, bm, dropout=p, seed=seed) as enc:
        for piece in (None, "1026"):
            if piece:
                monkeypatch.setenv("SHREDWORD_ENCODE_PIECE", piece)
            assert np.array_equal(enc.encode(text), want)
            ids, starts, line = enc.encode_spans(text, lines=True)
            assert np.array_equal(ids, want)
            assert np.array_equal(starts, ref_starts(merges, text, want))
            assert line[0] == 0 and line[-1] == want.size
            ids, row = enc.encode_docs(text, off)
            assert np.array_equal(ids, want_docs) and np.array_equal(row, want_row)
        assert np.array_equal(_device_ids(enc, text), want)


# ---- every path equals the reference, and host equals device --------------------------------------------

def _lines_from_starts(text, starts, T):
    """line_off as the header defines it, from the token starts."""
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
    off = [0] + np.searchsorted(starts, nl).tolist()
    if not text.endswith(b"\n"):
        off.append(T)
    else:
        off[-1] = T
    return np.array(off, dtype=np.int64)


def test_encode_and_spans_paths(model):
    merges, bm, corpus, solid = model
    text = _cut(corpus, 40000, 62000)
    p, seed = 0.1, 31
    want = _ref(merges, bm, text, p, seed)
    want_starts = ref_starts(merges, text, want)
    want_lines = _lines_from_starts(text, want_starts, want.size)
    with _enc(merges, bm, dropout=p, seed=seed) as enc:
        assert np.array_equal(enc.encode(text), want)
        assert np.array_equal(_device_ids(enc, text), want)
        ids, starts, line = enc.encode_spans(text, lines=True)
        assert np.array_equal(ids, want) and np.array_equal(starts, want_starts) and np.array_equal(line, want_lines)
        ids, starts, line, _ = enc.encode_spans_device(_dev(text))
        assert np.array_equal(ids.cpu().numpy(), want) and np.array_equal(starts.cpu().numpy(), want_starts)
        assert np.array_equal(line.cpu().numpy(), want_lines)
        ids, line = enc.encode_lines(text)
        assert np.array_equal(ids, want) and np.array_equal(line, want_lines)


def test_specials_path(model):
    """<|endoftext|> inside runs: the match keeps its id, no merge reaches across it, and the words on
    either side are dropped by their own positions (the blanked copy has the text's offsets)."""
    merges, bm, corpus, solid = model
    body = _cut(corpus, 70000, 82000)
    cuts = [m.start() + len(m.group()) // 2 for i, m in enumerate(WORD.finditer(body)) if i % 97 == 5 and len(m.group()) > 3]
    assert len(cuts) > 5
    text = b"".join(body[a:b] + EOT for a, b in zip([0] + cuts, cuts)) + body[cuts[-1]:]
    text = EOT + text + b" " + EOT + EOT + b"\n"
    at = [i for i in range(len(text)) if text.startswith(EOT, i)]
    blank = text.replace(EOT, b" " * len(EOT))
    sid = 256 + len(merges)
    p, seed = 0.5, 41
    words = _ref(merges, bm, blank, p, seed)
    items = sorted(list(zip(ref_starts(merges, blank, words).tolist(), words.tolist())) + [(a, sid) for a in at])
    want = np.array([i for _, i in items], dtype=np.int32)
    want_starts = np.array([s for s, _ in items], dtype=np.int64)
    with _enc(merges, bm, special_tokens=[EOT], dropout=p, seed=seed) as enc:
        ids, starts = enc.encode_spans(text, specials=True)
        assert int(np.count_nonzero(ids == sid)) == len(at)
        assert np.array_equal(ids, want) and np.array_equal(starts, want_starts)
        assert np.array_equal(enc.encode(text, specials=True), want)
        dids, dstarts, _, _ = enc.encode_spans_device(_dev(text), lines=False, specials=True)
        assert np.array_equal(dids.cpu().numpy(), want) and np.array_equal(dstarts.cpu().numpy(), want_starts)
        # without specials=True the same bytes are ordinary words, dropped at the same positions
        assert np.array_equal(enc.encode(text), _ref(merges, bm, text, p, seed))


def test_docs_paths(model):
    """Documents: the positions are those of the copy (offset + d); an empty document and a boundary
    inside a run are among them."""
    import torch
    merges, bm, corpus, solid = model
    text = _cut(corpus, 90000, 102000)
    run = next(m for m in WORD.finditer(text, 3000) if len(m.group()) >= 6)
    off = np.array([0, 700, 700, run.start() + 3, 8000, len(text)], dtype=np.int64)
    p, seed = 0.5, 53
    want, want_row = ref_dropout_docs(merges, bm, text, off, p, seed)
    assert want_row[2] == want_row[1]
    # the copy's positions, not the text's: the reference without the + d differs
    flat = np.concatenate([ref_dropout_encode(merges, bm, text[a:b], p, seed, int(a)) for a, b in zip(off, off[1:])])
    assert not np.array_equal(flat, want)
    docs = [text[a:b] for a, b in zip(off, off[1:])]
    with _enc(merges, bm, dropout=p, seed=seed) as enc:
        ids, row, starts = enc.encode_docs(text, off, starts=True)
        assert np.array_equal(ids, want) and np.array_equal(row, want_row)
        assert np.array_equal(starts, np.concatenate(
            [a + ref_starts(merges, d, want[r0:r1]) for a, d, r0, r1 in zip(off, docs, want_row, want_row[1:])]))
        ids, row = enc.encode_batch(docs)
        assert np.array_equal(ids, want) and np.array_equal(row, want_row)
        ids, row, _, _ = enc.encode_docs_device(_dev(text), torch.from_numpy(off).cuda())
        assert np.array_equal(ids.cpu().numpy(), want) and np.array_equal(row.cpu().numpy(), want_row)
        # the convenience calls only pass the state on
        two = [docs[0], docs[3]]
        w2, r2 = ref_dropout_docs(merges, bm, b"".join(two), [0, len(two[0]), len(two[0]) + len(two[1])], p, seed)
        batch, lengths = enc.encode_padded(two, pad_id=-7)
        assert lengths.tolist() == np.diff(r2).tolist()
        for r in range(2):
            assert np.array_equal(batch[r, :lengths[r]], w2[r2[r]:r2[r + 1]])
            assert (batch[r, lengths[r]:] == -7).all()


# ---- invariants ---------------------------------------------------------------------------------------

def test_invariants(model):
    merges, bm, corpus, solid = model
    text = _staging_text(corpus, solid)
    with _enc(merges) as enc:  # (the identity byte map: decode spells the text)
        plain = enc.encode(text)
        enc.set_dropout(0.1, 1)
        a = enc.encode(text)
        assert np.array_equal(enc.encode(text), a)          # the same seed twice
        assert np.array_equal(_device_ids(enc, text), a)
        enc.set_dropout(0.1, 2)
        b = enc.encode(text)
        assert not np.array_equal(a, b)                     # another seed
        for ids in (a, b):
            assert ids.size >= plain.size
            assert enc.decode(ids) == enc.decode(plain) == b"".join(WORD.findall(text))
        enc.set_dropout(1.0, 2)
        assert np.array_equal(enc.encode(text), np.frombuffer(b"".join(WORD.findall(text)), dtype=np.uint8))


# ---- off means off ----------------------------------------------------------------------------------------

def test_off_means_off(monkeypatch, capfd):
    """After set_dropout(0) the calls are routed as before: the word cache serves them (seen by its
    growth line under a small slot count) and nothing reruns on the direct path."""
    s = SHAPES["cache_grow"]
    monkeypatch.delenv("SHREDWORD_ENCODE_CACHE", raising=False)
    with _enc(s.merges) as never:
        want = never.encode(s.text)
        assert never.dropout == (0.0, 0)
    with _enc(s.merges) as enc:
        enc.set_dropout(0.5, 3)
        assert not np.array_equal(enc.encode(s.text), want)
        enc.set_dropout(0.0, 0)
        monkeypatch.setenv("SHREDWORD_ENCODE_DEBUG", "1")
        monkeypatch.setenv("SHREDWORD_ENCODE_CACHE_SLOTS", s.claims["slots"])
        capfd.readouterr()
        got = enc.encode(s.text)
        err = capfd.readouterr().err
        assert np.array_equal(got, want)
        assert "word cache grows" in err and "direct path" not in err
        # a threshold of 0 is off as well
        enc.set_dropout(1e-10, 9)
        assert np.array_equal(enc.encode(s.text), want)
        err = capfd.readouterr().err
        assert "word cache grows" in err and "direct path" not in err
        # with dropout on, the direct kernels run: no cache line of either kind
        enc.set_dropout(0.5, 3)
        enc.encode(s.text)
        err = capfd.readouterr().err
        assert "word cache" not in err


# ---- long words ----------------------------------------------------------------------------------------

def test_long_words_are_not_dropped():
    merges = pairs((b"a", b"b"))
    text = b"ab " * 8 + b"ab" * 513 + b" ab"
    with _enc(merges, long_words=True, dropout=1.0, seed=4) as enc:
        want = [97, 98] * 8 + [256] * 513 + [97, 98]
        assert enc.encode(text).tolist() == want
        assert _device_ids(enc, text).tolist() == want
        enc.long_words = False
        with pytest.raises(ValueError, match="1024"):
            enc.encode(text)


# ---- errors -------------------------------------------------------------------------------------------

def test_bad_probability_keeps_the_setting():
    text = b"banana " * 50
    with _enc(BANANA, dropout=0.5, seed=6) as enc:
        want = _ref(BANANA, None, text, 0.5, 6)
        for bad in (-0.1, 1.0000001, float("nan")):
            with pytest.raises(ValueError):
                enc.set_dropout(bad, 99)
            assert enc.dropout == (0.5, 6)
            assert np.array_equal(enc.encode(text), want)
    from shredword.encoder import BPEEncoder
    with pytest.raises(ValueError):
        BPEEncoder.from_merges(BANANA, dropout=2.0)
