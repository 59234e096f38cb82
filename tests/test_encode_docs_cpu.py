"""join_docs (shredword/encoder.py): the documents of encode_batch joined into the text and the
offsets that encode_docs takes.  Pure host code: no GPU."""
import numpy as np


def _join(texts):
    from shredword.encoder import join_docs
    buf, off = join_docs(texts)
    assert isinstance(buf, np.ndarray) and buf.dtype == np.uint8 and buf.ndim == 1
    assert isinstance(off, np.ndarray) and off.dtype == np.int64 and off.ndim == 1
    return buf.tobytes(), off.tolist()


def test_str_and_bytes_mixed():
    text, off = _join(["ab", b"cd e", "éx", bytearray(b"zz")])
    assert text == b"abcd e\xc3\xa9xzz"
    assert off == [0, 2, 6, 9, 11]


def test_empty_list():
    text, off = _join([])
    assert text == b"" and off == [0]
    text, off = _join(())
    assert text == b"" and off == [0]


def test_empty_members():
    text, off = _join([b"", "ab", "", b"", "c", ""])
    assert text == b"abc"
    assert off == [0, 0, 2, 2, 2, 3, 3]
    text, off = _join(["", b""])
    assert text == b"" and off == [0, 0, 0]


def test_newline_and_nul_stay():
    docs = [b"a\nb\n", b"\0", "x\0\ny", b"\n"]
    text, off = _join(docs)
    assert text == b"a\nb\n\0x\0\ny\n"
    assert off == [0, 4, 5, 9, 10]
    for d, doc in enumerate(docs):
        assert text[off[d]:off[d + 1]] == (doc.encode() if isinstance(doc, str) else doc)


def test_offsets_are_the_cumulative_lengths():
    rng = np.random.default_rng(5)
    docs = [bytes(rng.integers(0, 256, size=int(rng.integers(0, 40))).astype(np.uint8)) for _ in range(100)]
    text, off = _join(docs)
    assert text == b"".join(docs)
    assert off == np.concatenate([[0], np.cumsum([len(d) for d in docs])]).tolist()
    assert off[0] == 0 and off[-1] == len(text) and len(off) == len(docs) + 1
