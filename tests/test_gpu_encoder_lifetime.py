"""GPU tests of what the encoder keeps on the device between calls: every pass family's scratch is
allocated on the family's first call, grown by a larger call, reused by a smaller one, and freed
with the encoder.  The feature tests (test_gpu_encode*.py, test_gpu_decode.py, test_gpu_batch.py)
check what the passes compute; these check that reused, regrown and freshly created state gives the
same results, in any order of first use, and that partly used encoders die cleanly.

The expected output of a call is that of a fresh encoder given only that call (computed once per
family and text); the plain ids are also compared with the CPU oracle once per text.

Not tested: the device footprint.  torch.cuda's memory counters do not see the library's own
allocations, so a leak would not show there; the check is that calls keep succeeding.
"""
import functools

import numpy as np
import pytest

from encode_ref import oracle_encode, token_bytes

pytestmark = pytest.mark.gpu

# "th", "the", "at", "cat", "sat", "mat", "on", "that", "hat", "then", "in", "ing"
MERGES = np.array([[ord("t"), ord("h"), 256], [256, ord("e"), 257], [ord("a"), ord("t"), 258],
                   [ord("c"), 258, 259], [ord("s"), 258, 260], [ord("m"), 258, 261], [ord("o"), ord("n"), 262],
                   [256, 258, 263], [ord("h"), 258, 264], [257, ord("n"), 265], [ord("i"), ord("n"), 266],
                   [266, ord("g"), 267]], dtype=np.int32)
SPECIAL = b"<|s|>"
WORDS = [b"the", b"cat", b"sat", b"on", b"that", b"mat", b"then", b"hat", b"thing", b"x", SPECIAL,
         b"thethatcatsatmatonthenhatthinginthecat"]  # the last: longer than an LDS strip
SIZES = (100, 3 * 4096 + 1, 100)
FAMILIES = ("encode", "spans", "special", "docs", "decode", "pad", "pack")


@functools.lru_cache(maxsize=None)
def _text(k):
    rng = np.random.default_rng(17 + k)
    parts, size = [], 0
    while size < SIZES[k]:
        parts.append(WORDS[int(rng.integers(len(WORDS)))] + (b"\n" if rng.integers(6) == 0 else b" "))
        size += len(parts[-1])
    return b"".join(parts)[:SIZES[k]]


@functools.lru_cache(maxsize=None)
def _oracle_ids(k):
    ids = oracle_encode(MERGES, None, _text(k))
    ids.setflags(write=False)
    return ids


def _rows(k):
    """Three rows of the text's ids, the middle one empty."""
    T = _oracle_ids(k).size
    return np.array([0, T // 3, T // 3, T], dtype=np.int64)


def _docs(k):
    n = SIZES[k]
    return np.array([0, n // 3, 2 * n // 3, n], dtype=np.int64)


def _new_encoder(specials=(SPECIAL,)):
    from shredword.encoder import BPEEncoder
    return BPEEncoder.from_merges(MERGES, special_tokens=list(specials))


def _plain(res):
    """The arrays and bytes of a call's result, device tensors on the host, the timings dropped."""
    import torch
    out = []
    for x in res if isinstance(res, tuple) else (res,):
        if isinstance(x, torch.Tensor):
            out.append(x.cpu().numpy().copy())
        elif isinstance(x, (np.ndarray, bytes)):
            out.append(x)
    return out


def _run(enc, family, k):
    """One call of the family on device tensors and one through its host-buffer entry point."""
    import torch
    text = _text(k)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    t = dev(np.frombuffer(text, dtype=np.uint8))
    ids, rows = _oracle_ids(k), _rows(k)
    if family == "encode":
        res = enc.encode_device(t), enc.encode(text)
    elif family == "spans":
        res = enc.encode_spans_device(t, starts=True, lines=True), enc.encode_spans(text, lines=True)
    elif family == "special":
        res = enc.encode_spans_device(t, specials=True), enc.encode_spans(text, lines=True, specials=True)
    elif family == "docs":
        res = enc.encode_docs_device(t, dev(_docs(k)), starts=True), enc.encode_docs(text, _docs(k), starts=True)
    elif family == "decode":
        res = enc.decode_device(dev(ids), dev(rows), sep=b"\n"), enc.decode_rows(ids, rows, sep=b"\n")
    elif family == "pad":
        kw = dict(bos=1, max_len=8, pad_id=-1, mask=True)
        res = enc.pad_device(dev(ids), dev(rows), **kw), enc.pad_rows(ids, rows, **kw)
    else:
        kw = dict(seq_len=16, eos=0, pad_id=-1, positions=True, segments=True)
        res = enc.pack_device(dev(ids), dev(rows), **kw), enc.pack_rows(ids, rows, **kw)
    return _plain(res[0]) + _plain(res[1])


@functools.lru_cache(maxsize=None)
def _fresh(family, k):
    """The family's outputs from an encoder that has seen nothing else."""
    enc = _new_encoder()
    try:
        return _run(enc, family, k)
    finally:
        enc.destroy()


def _check(got, family, k):
    want = _fresh(family, k)
    assert len(got) == len(want), (family, k)
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, bytes):
            assert g == w, (family, k, i)
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (family, k, i)


def test_oracle_ids():
    """The reference the other tests compare with is itself right: plain ids against the CPU oracle."""
    for k in range(len(SIZES)):
        dev_ids, host_ids = _fresh("encode", k)
        assert np.array_equal(dev_ids, _oracle_ids(k)) and np.array_equal(host_ids, _oracle_ids(k)), k
        assert _oracle_ids(k).size < SIZES[k]  # merges applied


def test_grow_then_shrink():
    """One encoder, every family on 100 B, 3 * 4096 + 1 B and 100 B again: scratch that was grown and
    is then reused for a smaller call carries nothing over."""
    enc = _new_encoder()
    try:
        for k in range(len(SIZES)):
            for family in FAMILIES:
                _check(_run(enc, family, k), family, k)
    finally:
        enc.destroy()


@pytest.mark.parametrize("order", [("decode", "pad", "pack", "docs", "special", "spans", "encode"),
                                   ("encode", "spans", "special", "docs", "pack", "pad", "decode")],
                         ids=["decode_first", "encode_first"])
def test_first_touch_order(order):
    """The families' states are created in the order of first use, whichever that is; a second round on
    the large text then grows each."""
    enc = _new_encoder()
    try:
        for k in (0, 1):
            for family in order:
                _check(_run(enc, family, k), family, k)
    finally:
        enc.destroy()


def test_partial_lifetime():
    """Encoders that used one pass family only are destroyed, again and again; the next encoder works."""
    for _ in range(3):
        for family in ("spans", "special", "docs", "decode", "pad"):
            enc = _new_encoder()
            _check(_run(enc, family, 0), family, 0)
            enc.destroy()
            enc = _new_encoder()
            _check(_run(enc, "encode", 1), "encode", 1)
            enc.destroy()


def test_set_specials_between_decodes():
    """set_special_tokens replaces the set: the decode vocabulary (and the span passes' length table)
    built from the first set are rebuilt from the second."""
    import torch
    toks = token_bytes(MERGES)
    V = len(toks)
    first, second = [b"<|a|>"], [b"<|bb|>", b"<|c|>"]
    ids = np.array([257, V, 259, V + 1], dtype=np.int32)
    rows = np.array([0, 2, 4], dtype=np.int64)
    dev = lambda a: torch.from_numpy(a).cuda()
    enc = _new_encoder(first)
    try:
        for specials, n in ((first, 3), (second, 4)):
            enc.set_special_tokens(specials)
            vocab = toks + specials
            want = b"".join(vocab[i] for i in ids[:n])
            got, off, _ = enc.decode_device(dev(ids[:n]))
            assert got.cpu().numpy().tobytes() == want and off.cpu().tolist() == [0, len(want)]
            assert enc.decode_rows(ids[:n])[0] == want
        want = b"the<|bb|>\ncat<|c|>\n"
        assert enc.decode_device(dev(ids), dev(rows), sep=b"\n")[0].cpu().numpy().tobytes() == want
        assert enc.decode_rows(ids, rows, sep=b"\n")[0] == want
        # the span passes' length table follows the set too
        text = b"the <|c|>cat <|bb|> <|a|>"
        other = _new_encoder(second)
        try:
            want = other.encode_spans(text, lines=True, specials=True)
        finally:
            other.destroy()
        got = enc.encode_spans(text, lines=True, specials=True)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert got[0].tolist().count(V) == 1 and got[0].tolist().count(V + 1) == 1
    finally:
        enc.destroy()
