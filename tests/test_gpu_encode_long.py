"""GPU tests of words above SHRED_ENCODE_MAX_WORD bytes (include/shredword_encode.h:
shred_encoder_set_long_words; csrc/hip/encode_long.hip; BPEEncoder(long_words=True)).

Every case compares the ids with the Python reference of encode_long_ref.py, which
test_encode_long_ref_cpu.py pins against the oracle on words the oracle takes; starts, line_off and
row_off are checked where the case says so.  The merge tables are tiny unless stated.
"""
import os
import re

import numpy as np
import pytest

import corpora
from conftest import GOLDEN, PKG
from encode_long_ref import AA, AA_AAAA, LOCAL_MIN, LOCAL_MIN_2, ref_encode, ref_starts
from encode_ref import model_merges

pytestmark = pytest.mark.gpu

CSRC = os.path.join(PKG, "csrc")
MAX_WORD = 1024


def _const(rel, name):
    src = open(os.path.join(CSRC, rel)).read()
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([^;]+);", src)
    assert m, f"{name} not found in {rel}"
    return m.group(1).strip()


LDS = int(_const("hip/encode_long.hip", "kLongLds"))          # tokens a long word keeps in LDS
THREADS = int(_const("hip/encode_long.hip", "kLongThreads"))
SLAB = int(_const("hip/encode_long.hip", "kLongSlab"))
SPAN, CHUNK = 32, 4096                                         # encode_words.h (test_encode_shapes_cpu.py guards them)


def _enc(merges, bm=None, **kw):
    from shredword.encoder import BPEEncoder
    return BPEEncoder.from_merges(merges, bm, long_words=True, **kw)


_REF = {}


def _reference(merges, bm, text):
    """(ids, starts) of the reference: computed once per input, shared by the cases, never modified."""
    key = (merges.tobytes(), None if bm is None else bm.tobytes(), text)
    if key not in _REF:
        ids = ref_encode(merges, bm, text)
        _REF[key] = (ids, ref_starts(merges, text, ids))
    return _REF[key]


def _check(enc, merges, text, bm=None):
    """ids and starts of the host call against the reference; returns the ids."""
    exp, exp_starts = _reference(merges, bm, text)
    ids, starts = enc.encode_spans(text)
    assert np.array_equal(ids, exp)
    assert np.array_equal(starts, exp_starts)
    assert np.array_equal(enc.encode(text), exp)
    return ids


def _aa_closed_form(L):
    """b"a" * L under (a,a)->A, (A,A)->B: floor(L / 4) B, then an A for bit 1 of L, then an a for bit 0."""
    return [257] * (L // 4) + [256] * ((L % 4) // 2) + [97] * (L % 2)


@pytest.fixture(params=[None, "0"], ids=["cache", "direct"])
def core_path(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("SHREDWORD_ENCODE_CACHE", raising=False)
    else:
        monkeypatch.setenv("SHREDWORD_ENCODE_CACHE", request.param)
    return request.param


def test_default_unchanged():
    from shredword.encoder import MAX_LONG_WORD, BPEEncoder
    assert MAX_LONG_WORD == 1 << 20
    text = b"ab " + b"a" * (MAX_WORD + 1) + b" ba\n"
    with BPEEncoder.from_merges(AA) as enc:
        assert enc.long_words is False
        with pytest.raises(ValueError, match="1024"):
            enc.encode(text)
        enc.long_words = True
        assert enc.long_words is True
        _check(enc, AA, text)
        enc.long_words = False
        with pytest.raises(ValueError, match="1024"):
            enc.encode_lines(text)
    with BPEEncoder.from_merges(AA, long_words=False) as enc:
        with pytest.raises(ValueError):
            enc.encode_batch([text])
    with _enc(AA) as enc:
        assert enc.long_words is True
        _check(enc, AA, text)


@pytest.mark.parametrize("L", [MAX_WORD, MAX_WORD + 1, LDS - 1, LDS, LDS + 1])
def test_dispatch_edges(L, core_path):
    rng = np.random.default_rng(L)
    word = bytes(rng.choice(list(b"abcd"), size=L).tolist())
    with _enc(LOCAL_MIN) as enc:
        _check(enc, LOCAL_MIN, b"dc " + word + b" ab\n")
    with _enc(AA_AAAA) as enc:
        ids = _check(enc, AA_AAAA, b"a" * L)
        assert ids.tolist() == _aa_closed_form(L)


def test_dispatch_largest(core_path):
    from shredword.encoder import MAX_LONG_WORD
    with _enc(AA_AAAA) as enc:
        for L in (MAX_LONG_WORD - 1, MAX_LONG_WORD):
            text = b"aaa " + b"a" * L + b"\naa"
            ids = enc.encode(text)
            assert ids.tolist() == [256, 97] + _aa_closed_form(L) + [256]
        text = b"aaa " + b"a" * MAX_LONG_WORD
        ids = _check(enc, AA_AAAA, text)                       # the reference, and starts at full length
        assert ids.tolist() == [256, 97] + _aa_closed_form(MAX_LONG_WORD)   # the closed form is the reference's
        with pytest.raises(ValueError, match=str(MAX_LONG_WORD)):
            enc.encode(b"aaa " + b"a" * (MAX_LONG_WORD + 1) + b"\naa")
        with pytest.raises(ValueError):
            enc.encode_batch([b"a", b"a" * (MAX_LONG_WORD + 1)])


def test_run_parity(core_path):
    runs = b"b".join(b"a" * k for k in range(1, 10))          # runs of every length 1..9
    mixed = (runs + b"b") * (4000 // (len(runs) + 1)) + b"ab"
    mixed += b"a" * (4000 - len(mixed))
    assert len(mixed) == 4000
    with _enc(AA) as enc:
        for L in (MAX_WORD + 1, MAX_WORD + 2, 2049, 2050, THREADS * 2 + 1, THREADS * SLAB + 1, LDS + THREADS * SLAB + 1):
            ids = _check(enc, AA, b"ba " + b"a" * L + b" a")
            assert ids.tolist() == [98, 97] + [256] * (L // 2) + [97] * (L % 2) + [97]
        _check(enc, AA, mixed)
        # a run that starts at every offset of a slab, across the slab boundary of every thread
        for lead in range(SLAB + 1):
            _check(enc, AA, b"b" * lead + b"a" * (THREADS * SLAB + 1) + b"b")
            _check(enc, AA, b"b" * lead + b"a" * (3 * LDS + 5) + b"b")


@pytest.mark.parametrize("merges", [LOCAL_MIN, LOCAL_MIN_2], ids=["cd_rank5", "cd_rank2"])
def test_local_minimum_counter_example(merges, core_path):
    with _enc(merges) as enc:
        ids = _check(enc, merges, b"abcd" * 300)
        assert ids.tolist() == [257, 100] * 300
        _check(enc, merges, b"abcd" * (2 * LDS // 4 + 1))


def _golden():
    with open(os.path.join(GOLDEN, "c1_ascii10m_v8192", "model.bin"), "rb") as f:
        return model_merges(f.read())


def test_many_ranks(tmp_path, core_path):
    merges = _golden()
    path = str(tmp_path / "c.txt")
    corpora.gen_synthetic(path, 80000, 1, "ascii")
    words = open(path, "rb").read().split()
    glued = b"".join(words)
    assert len(glued) >= LDS + 3000
    with _enc(merges) as enc:
        before = enc.long_word_stats["rounds"]
        ids = _check(enc, merges, b"the " + glued[:3000] + b" end\n")
        assert len(set(ids.tolist())) > 100                    # many distinct merges applied
        assert enc.long_word_stats["rounds"] - before >= 2 * 100   # two encodes of the word, hundreds of rounds
        _check(enc, merges, glued[:LDS + 2077] + b"\n" + glued[5:3005])   # starts in global scratch, ends in LDS


GEOMETRY = {
    "at_byte_0": lambda w: w + b" ab cd\n",
    "span_last_byte": lambda w: b"ab " + b" " * (SPAN - 4) + w + b" cd",
    "chunk_last_byte": lambda w: b"ab " + b"cd " * ((CHUNK - 4) // 3) + b" " * ((CHUNK - 4) % 3) + w + b" cd\n",
    "ends_the_text": lambda w: b"ab cd " + w,
    "two_in_a_chunk": lambda w: b"dc " + w[:1100] + b" " + w[:1300] + b" ab",
    "short_words_behind": lambda w: b"ab " + w + b" a ab abc abcd " + b"abcd " * 40,
}


@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_position_in_the_geometry(name, core_path):
    rng = np.random.default_rng(7)
    word = bytes(rng.choice(list(b"abcd"), size=1500).tolist())
    text = GEOMETRY[name](word)
    if name == "span_last_byte":
        assert text.index(word) == SPAN - 1
    if name == "chunk_last_byte":
        assert text.index(word) == CHUNK - 1
    with _enc(LOCAL_MIN) as enc:
        _check(enc, LOCAL_MIN, text)


def test_cache_growth_with_a_long_word(monkeypatch, capfd):
    rng = np.random.default_rng(11)
    short = b" ".join(bytes(rng.choice(list(b"abcd"), size=int(rng.integers(1, 12))).tolist()) for _ in range(3000))
    text = short + b" " + b"abcd" * 500 + b" " + short[:999]
    monkeypatch.delenv("SHREDWORD_ENCODE_CACHE", raising=False)
    monkeypatch.setenv("SHREDWORD_ENCODE_CACHE_SLOTS", "128")
    monkeypatch.setenv("SHREDWORD_ENCODE_DEBUG", "1")
    with _enc(LOCAL_MIN) as enc:
        _check(enc, LOCAL_MIN, text)
    assert "word cache grows" in capfd.readouterr().err


def test_host_staging_in_small_pieces(monkeypatch):
    rng = np.random.default_rng(13)
    long1, long2 = (bytes(rng.choice(list(b"abcd"), size=5000).tolist()) for _ in range(2))
    text = b"ab cd " * 300 + long1 + b" " + b"abcd a " * 200 + b"\n" + long2
    with _enc(LOCAL_MIN) as enc:
        whole = _check(enc, LOCAL_MIN, text)
        monkeypatch.setenv("SHREDWORD_ENCODE_PIECE", "1026")
        assert np.array_equal(enc.encode(text), whole)
        ids, starts, line = enc.encode_spans(text, lines=True)
        assert np.array_equal(ids, whole) and np.array_equal(starts, ref_starts(LOCAL_MIN, text, whole))
        first = len(ref_encode(LOCAL_MIN, None, text[:text.index(b"\n")]))
        assert line.tolist() == [0, first, len(whole)]
        ids, row = enc.encode_batch([text[:3000], text[3000:]])   # the boundary cuts long1
        exp = [ref_encode(LOCAL_MIN, None, t) for t in (text[:3000], text[3000:])]
        assert np.array_equal(ids, np.concatenate(exp)) and row.tolist() == [0, len(exp[0]), len(exp[0]) + len(exp[1])]
        with pytest.raises(ValueError):
            enc.encode(b"ab " * 500 + b"a" * ((1 << 20) + 1) + b" ab")


W2000 = bytes(np.random.default_rng(17).choice(list(b"abcd"), size=2000).tolist())
EOT = b"<|eot|>"


def test_entry_points_lines_and_spans(core_path):
    text = b"ab cd\n" + W2000 + b" ab\n\ncd " + W2000[:1500]
    exp = ref_encode(LOCAL_MIN, None, text)
    rows = [len(ref_encode(LOCAL_MIN, None, l)) for l in text.split(b"\n")]
    with _enc(LOCAL_MIN) as enc:
        _check(enc, LOCAL_MIN, text)
        ids, line = enc.encode_lines(text)
        assert np.array_equal(ids, exp) and line.tolist() == np.concatenate([[0], np.cumsum(rows)]).tolist()
        batch, lengths = enc.encode_padded(text, pad_id=-7)
        assert lengths.tolist() == rows and batch.shape == (4, max(rows))
        for r, n in enumerate(rows):
            assert np.array_equal(batch[r, :n], exp[line[r]:line[r + 1]]) and (batch[r, n:] == -7).all()
        data, boff = enc.decode_rows(ids, line)
        assert data == b"".join(text.split())


def test_entry_points_specials(core_path):
    cut = W2000[:700] + EOT + W2000[700:]                      # one run of 2007 bytes, cut in two words
    text = b"ab " + cut + b" cd"
    with _enc(LOCAL_MIN, special_tokens=[EOT]) as enc:
        eot = enc.special_tokens[EOT]
        exp = np.concatenate([ref_encode(LOCAL_MIN, None, b"ab " + W2000[:700]), [eot],
                              ref_encode(LOCAL_MIN, None, W2000[700:] + b" cd")])
        assert np.array_equal(enc.encode(text, specials=True), exp)
        ids, starts = enc.encode_spans(text, specials=True)
        lens = enc.token_lengths
        assert np.array_equal(ids, exp)
        ends = starts + lens[np.maximum(ids, 0)]
        assert starts[0] == 0 and ends[-1] == len(text)
        assert sorted(set(range(len(text))) - {p for s, e in zip(starts, ends) for p in range(s, e)}) == \
            [2, len(text) - 3]                                 # the tokens tile the non-delimiter bytes
        # the long limit applies to the run before it is cut
        run = b"a" * (1 << 19) + EOT + b"a" * ((1 << 19) + 1 - len(EOT))
        assert len(run) == (1 << 20) + 1
        with pytest.raises(ValueError):
            enc.encode(b"ab " + run, specials=True)


def test_entry_points_docs_and_device(core_path):
    import torch
    text = b"ab " + W2000 + b"cd\n" + W2000[:1200]
    off = np.array([0, 3 + 900, 3 + 900, len(text)], dtype=np.int64)   # a boundary inside the 2000-byte run
    docs = [text[off[d]:off[d + 1]] for d in range(3)]
    exp = [ref_encode(LOCAL_MIN, None, d) for d in docs]
    row_exp = np.concatenate([[0], np.cumsum([len(e) for e in exp])])
    st_exp = np.concatenate([ref_starts(LOCAL_MIN, d, e) + off[i] for i, (d, e) in enumerate(zip(docs, exp))])
    with _enc(LOCAL_MIN) as enc:
        ids, row, starts = enc.encode_docs(text, off, starts=True)
        assert np.array_equal(ids, np.concatenate(exp)) and np.array_equal(row, row_exp)
        assert np.array_equal(starts, st_exp)
        dev = torch.device("cuda", enc.device)
        t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
        ids, row, starts, _ = enc.encode_docs_device(t, torch.from_numpy(off).to(dev), starts=True)
        assert np.array_equal(ids.cpu().numpy(), np.concatenate(exp)) and np.array_equal(row.cpu().numpy(), row_exp)
        assert np.array_equal(starts.cpu().numpy(), st_exp)
        # an unaligned view of a device tensor
        view = torch.frombuffer(bytearray(b"xyz" + text), dtype=torch.uint8).to(dev)[3:]
        whole = ref_encode(LOCAL_MIN, None, text)
        ids, starts, line, _ = enc.encode_spans_device(view)
        assert np.array_equal(ids.cpu().numpy(), whole)
        assert np.array_equal(starts.cpu().numpy(), ref_starts(LOCAL_MIN, text, whole))
        assert line.cpu().numpy().tolist() == [0, len(ref_encode(LOCAL_MIN, None, text[:text.index(b"\n")])), len(whole)]
        ids, _ = enc.encode_device(view)
        assert np.array_equal(ids.cpu().numpy(), whole)


def test_byte_map_unk(core_path):
    bm = np.arange(256, dtype=np.int32)
    bm[ord("c")] = -1                                          # no merge may touch a dropped byte
    rng = np.random.default_rng(19)
    word = bytes(rng.choice(list(b"aabcd"), size=LDS + 100).tolist())
    with _enc(LOCAL_MIN_2, bm) as enc:
        ids = _check(enc, LOCAL_MIN_2, b"ab " + word + b" c", bm)
        assert (ids == -1).sum() == word.count(b"c") + 1
        assert not np.isin(ids, [257, 258]).any()              # (ab, c) and (c, d) never applied
    with _enc(AA, bm) as enc:
        _check(enc, AA, b"c" * 1500 + b" " + b"acca" * 500, bm)


def test_no_scratch_without_long_words():
    text = b"ab cd " * 2000 + b"a" * MAX_WORD + b"\n"
    with _enc(AA) as enc:
        _check(enc, AA, text)
        assert enc.long_word_stats == {"scratch_bytes": 0, "words": 0, "rounds": 0}
        _check(enc, AA, text + b"a" * (MAX_WORD + 1))
        st = enc.long_word_stats
        assert st["scratch_bytes"] > 0 and st["words"] == 2 and st["rounds"] == 2   # (encode_spans and encode)
