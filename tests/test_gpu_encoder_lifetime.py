"""GPU tests of what the encoder keeps on the device between calls: every pass family's scratch is
allocated on the family's first call, grown by a larger call, reused by a smaller one, and freed
with the encoder.  The feature tests (test_gpu_encode*.py, test_gpu_decode.py, test_gpu_batch.py)
check what the passes compute; these check that reused, regrown and freshly created state gives the
same results, in any order of first use, and that partly used encoders die cleanly.

The expected output of a call is that of a fresh encoder given only that call (computed once per
family, text and encoder configuration); the plain ids are also compared once per text with the CPU
oracle, and those of the long-word and the dropout encoder with their Python references.  The families
are the encode, span, special-token, document, decode, pad, pack, window, pair and masked-LM passes,
each through its device and its host entry point.

Not tested: the device footprint.  torch.cuda's memory counters do not see the library's own
allocations, so a leak would not show there; the check is that calls keep succeeding.
"""
import functools

import numpy as np
import pytest

import encode_dropout_ref
import encode_long_ref
import window_ref
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
FAMILIES = ("encode", "spans", "special", "docs", "decode", "pad", "pack", "window", "pair", "mlm")
# The encoder configurations: "long" takes words above MAX_WORD bytes (its large text holds one of
# LONG_WORD bytes), "dropout" drops merges at random.
CONFIGS = {"plain": {}, "long": dict(long_words=True), "dropout": dict(dropout=0.3, seed=7)}
LONG_WORD = 1500
PIECE = "999"  # SHREDWORD_BATCH_PIECE of the host calls in test_host_and_device_forms_interleaved


@functools.lru_cache(maxsize=None)
def _text(k, cfg="plain"):
    rng = np.random.default_rng(17 + k)
    parts, size = [], 0
    while size < SIZES[k]:
        parts.append(WORDS[int(rng.integers(len(WORDS)))] + (b"\n" if rng.integers(6) == 0 else b" "))
        size += len(parts[-1])
    text = b"".join(parts)[:SIZES[k]]
    if cfg == "long" and k == 1:
        at = text.index(b" ", SIZES[k] // 2) + 1
        text = text[:at] + (WORDS[-1] * LONG_WORD)[:LONG_WORD] + b" " + text[at:]
    return text


@functools.lru_cache(maxsize=None)
def _oracle_ids(k, cfg="plain"):
    """The plain ids of the text by the configuration's reference."""
    if cfg == "long":
        ids = encode_long_ref.ref_encode(MERGES, None, _text(k, cfg))
    elif cfg == "dropout":
        ids = encode_dropout_ref.ref_dropout_encode(MERGES, None, _text(k, cfg), CONFIGS[cfg]["dropout"],
                                                    CONFIGS[cfg]["seed"])
    else:
        ids = oracle_encode(MERGES, None, _text(k, cfg))
    ids.setflags(write=False)
    return ids


def _rows(k, cfg="plain"):
    """Three rows of the text's ids, the middle one empty."""
    T = _oracle_ids(k, cfg).size
    return np.array([0, T // 3, T // 3, T], dtype=np.int64)


def _reversed_rows(k, cfg="plain"):
    """(ids, offsets) of the same rows in reverse order: the second segment of the pair family."""
    ids, T = _oracle_ids(k, cfg), _oracle_ids(k, cfg).size
    return np.concatenate([ids[T // 3:], ids[:T // 3]]), np.array([0, T - T // 3, T - T // 3, T], dtype=np.int64)


def _docs(k, cfg="plain"):
    n = len(_text(k, cfg))
    return np.array([0, n // 3, 2 * n // 3, n], dtype=np.int64)


def _new_encoder(specials=(SPECIAL,), cfg="plain"):
    from shredword.encoder import BPEEncoder
    return BPEEncoder.from_merges(MERGES, special_tokens=list(specials), **CONFIGS[cfg])


@functools.lru_cache(maxsize=None)
def _starts(k, cfg="plain"):
    """The byte offset of every id, from encode_spans of an encoder of its own (so that the masked-LM
    family touches no other family's state), checked against the reference's."""
    enc = _new_encoder(cfg=cfg)
    try:
        ids, starts = enc.encode_spans(_text(k, cfg))
    finally:
        enc.destroy()
    assert np.array_equal(ids, _oracle_ids(k, cfg))
    assert np.array_equal(starts, encode_long_ref.ref_starts(MERGES, _text(k, cfg), ids))
    starts.setflags(write=False)
    return starts


def _plain(res):
    """The arrays, bytes and counts of a call's result, device tensors on the host, the timings dropped."""
    import torch
    out = []
    for x in res if isinstance(res, tuple) else (res,):
        if isinstance(x, torch.Tensor):
            out.append(x.cpu().numpy().copy())
        elif isinstance(x, (np.ndarray, bytes)):
            out.append(x)
        elif isinstance(x, (int, np.integer)) and not isinstance(x, bool):
            out.append(np.array(int(x)))
    return out


PAD = dict(bos=1, max_len=8, pad_id=-1, mask=True)
PACK = dict(seq_len=16, eos=0, pad_id=-1, positions=True, segments=True)
WINDOW = dict(max_len=8, stride=3, bos=1, mask=True)
PAIR = dict(max_len=16, truncation="window_second", stride=2, max_first=4, bos=1, sep=(2,), eos=3, mask=True)
MLM = dict(mask_id=300, p=0.3, seed=5)


def _run(enc, family, k, cfg="plain", abi="both"):
    """One call of the family on device tensors and one through its host-buffer entry point (abi:
    "device" or "host" for one of the two); the masked-LM family calls per token and per whole word."""
    import torch
    text = _text(k, cfg)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    t = lambda: dev(np.frombuffer(text, dtype=np.uint8))
    ids, rows = _oracle_ids(k, cfg), _rows(k, cfg)
    if family == "encode":
        calls = (lambda: enc.encode_device(t()), lambda: enc.encode(text))
    elif family == "spans":
        calls = (lambda: enc.encode_spans_device(t(), starts=True, lines=True),
                 lambda: enc.encode_spans(text, lines=True))
    elif family == "special":
        calls = (lambda: enc.encode_spans_device(t(), specials=True),
                 lambda: enc.encode_spans(text, lines=True, specials=True))
    elif family == "docs":
        calls = (lambda: enc.encode_docs_device(t(), dev(_docs(k, cfg)), starts=True),
                 lambda: enc.encode_docs(text, _docs(k, cfg), starts=True))
    elif family == "decode":
        calls = (lambda: enc.decode_device(dev(ids), dev(rows), sep=b"\n"),
                 lambda: enc.decode_rows(ids, rows, sep=b"\n"))
    elif family == "pad":
        calls = (lambda: enc.pad_device(dev(ids), dev(rows), **PAD), lambda: enc.pad_rows(ids, rows, **PAD))
    elif family == "pack":
        calls = (lambda: enc.pack_device(dev(ids), dev(rows), **PACK), lambda: enc.pack_rows(ids, rows, **PACK))
    elif family == "window":
        calls = (lambda: enc.window_device(dev(ids), dev(rows), **WINDOW), lambda: enc.window_rows(ids, rows, **WINDOW))
    elif family == "pair":
        ids_b, rows_b = _reversed_rows(k, cfg)
        calls = (lambda: enc.pair_device(dev(ids), dev(rows), dev(ids_b), dev(rows_b), **PAIR),
                 lambda: enc.pair_rows(ids, rows, ids_b, rows_b, **PAIR))
    else:
        starts = _starts(k, cfg)
        whole = dict(MLM, whole_word=True)
        calls = (lambda: (enc.mlm_device(dev(ids), dev(rows), **MLM)
                          + enc.mlm_device(dev(ids), dev(rows), starts=dev(starts), **whole)),
                 lambda: enc.mlm_rows(ids, rows, **MLM) + enc.mlm_rows(ids, rows, starts=starts, **whole))
    return [x for call, name in zip(calls, ("device", "host")) if abi in ("both", name) for x in _plain(call())]


@functools.lru_cache(maxsize=None)
def _fresh(family, k, cfg="plain"):
    """The family's outputs from an encoder that has seen nothing else: (the device call's, the host call's)."""
    enc = _new_encoder(cfg=cfg)
    try:
        device = _run(enc, family, k, cfg, "device")
        return device, _run(enc, family, k, cfg, "host")
    finally:
        enc.destroy()


def _check(got, family, k, cfg="plain", abi="both"):
    device, host = _fresh(family, k, cfg)
    want = {"both": device + host, "device": device, "host": host}[abi]
    assert len(got) == len(want), (family, k, cfg, abi)
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, bytes):
            assert g == w, (family, k, cfg, abi, i)
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (family, k, cfg, abi, i)


def _step(enc, step, k, cfg="plain"):
    """One step of an order of first use: a family (both ABIs) or a (family, abi) pair."""
    family, abi = (step, "both") if isinstance(step, str) else step
    _check(_run(enc, family, k, cfg, abi), family, k, cfg, abi)


def test_oracle_ids():
    """The reference the other tests compare with is itself right: plain ids against the CPU oracle, and
    those of the long-word and the dropout encoder against their references."""
    for k in range(len(SIZES)):
        (dev_ids,), (host_ids,) = _fresh("encode", k)
        assert np.array_equal(dev_ids, _oracle_ids(k)) and np.array_equal(host_ids, _oracle_ids(k)), k
        assert _oracle_ids(k).size < SIZES[k]  # merges applied
    for cfg in ("long", "dropout"):
        for k in (0, 1):
            (dev_ids,), (host_ids,) = _fresh("encode", k, cfg)
            want = _oracle_ids(k, cfg)
            assert np.array_equal(dev_ids, want) and np.array_equal(host_ids, want), (cfg, k)
    assert len(_text(1, "long")) == SIZES[1] + LONG_WORD + 1
    assert max(len(w) for w in encode_long_ref.WORD.findall(_text(1, "long"))) >= LONG_WORD  # a long word is there
    assert _oracle_ids(1, "dropout").size > _oracle_ids(1).size  # merges were dropped


def test_grow_then_shrink():
    """One encoder, every family on 100 B, 3 * 4096 + 1 B and 100 B again: scratch that was grown and
    is then reused for a smaller call carries nothing over."""
    enc = _new_encoder()
    try:
        for k in range(len(SIZES)):
            for family in FAMILIES:
                _step(enc, family, k)
    finally:
        enc.destroy()


ORDERS = {
    "decode_first": ("decode", "pad", "pack", "window", "pair", "mlm", "docs", "special", "spans", "encode"),
    "encode_first": ("encode", "spans", "special", "docs", "mlm", "pair", "window", "pack", "pad", "decode"),
    # the host paths of the batch families first, then their device paths, then the rest
    "host_first": (("window", "host"), ("pack", "host"), ("pad", "host"), ("pair", "host"),
                   ("window", "device"), ("pack", "device"), ("pad", "device"), ("pair", "device"),
                   "mlm", "decode", "docs", "special", "spans", "encode"),
}


@pytest.mark.parametrize("order", list(ORDERS))
def test_first_touch_order(order):
    """The families' states are created in the order of first use, whichever that is; a second round on
    the large text then grows each."""
    enc = _new_encoder()
    try:
        for k in (0, 1):
            for step in ORDERS[order]:
                _step(enc, step, k)
    finally:
        enc.destroy()


def test_partial_lifetime():
    """Encoders that used one pass family only are destroyed, again and again; the next encoder works."""
    for _ in range(3):
        for family in ("spans", "special", "docs", "decode", "pad", "window", "pair", "mlm"):
            enc = _new_encoder()
            _step(enc, family, 0)
            enc.destroy()
            enc = _new_encoder()
            _step(enc, "encode", 1)
            enc.destroy()


def _by_loops(family, k):
    """The outputs of the pad, pack and window families' calls by plain Python loops over the rows."""
    ids, rows = _oracle_ids(k).tolist(), _rows(k).tolist()
    kept = [ids[a:b] for a, b in zip(rows[:-1], rows[1:])]
    if family == "window":
        return list(window_ref.windows(ids, rows, **{n: v for n, v in WINDOW.items() if n != "mask"}))
    if family == "pad":
        em = [[PAD["bos"]] + r[:PAD["max_len"] - 1] for r in kept]
        W = max(len(e) for e in em)
        return [np.array([e + [PAD["pad_id"]] * (W - len(e)) for e in em], dtype=np.int32),
                np.array([len(e) for e in em], dtype=np.int32),
                np.array([[1] * len(e) + [0] * (W - len(e)) for e in em], dtype=np.uint8)]
    L, em = PACK["seq_len"], [r + [PACK["eos"]] for r in kept]
    fill = -sum(len(e) for e in em) % L
    cut = lambda v, pad: np.array(v + [pad] * fill, dtype=np.int32).reshape(-1, L)
    return [cut([x for e in em for x in e], PACK["pad_id"]),
            np.cumsum([0] + [len(e) for e in em], dtype=np.int64),
            cut([i for e in em for i in range(len(e))], 0), cut([r for r, e in enumerate(em) for _ in e], -1)]


def test_host_and_device_forms_interleaved(monkeypatch):
    """pad, pack and window share the batch state's staging (the three int32 outputs of a piece lie one
    capacity apart, the offsets and row_start in two halves of one buffer), and the window state's prefix
    sum is filled by a scan in the device call and uploaded by the host call.  Here they change hands
    between the two forms at 100 B, 3 * 4096 + 1 B and 100 B again, the host pad and window in pieces of
    less than a row; every result is that of a fresh encoder that was given the call alone, unpieced,
    and those are first compared with plain Python loops (a fresh encoder runs the same library, so by
    itself it would hide a staging error that does not depend on what the encoder has seen)."""
    monkeypatch.delenv("SHREDWORD_BATCH_PIECE", raising=False)
    for k in range(len(SIZES)):
        for family in ("window", "pad", "pack"):
            want = _by_loops(family, k)
            for abi, got in zip(("device", "host"), _fresh(family, k)):  # made before any piece size is set
                assert len(got) == len(want), (family, k, abi)
                for i, (g, w) in enumerate(zip(got, want)):
                    assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (family, k, abi, i)
    enc = _new_encoder()
    try:
        for k in range(len(SIZES)):
            for family, abi, piece in (("window", "device", None), ("pad", "host", PIECE), ("window", "host", PIECE),
                                       ("pack", "device", None), ("pack", "host", None), ("pad", "device", None)):
                if piece is None:
                    monkeypatch.delenv("SHREDWORD_BATCH_PIECE", raising=False)
                else:
                    monkeypatch.setenv("SHREDWORD_BATCH_PIECE", piece)
                _step(enc, (family, abi), k)
    finally:
        monkeypatch.delenv("SHREDWORD_BATCH_PIECE", raising=False)
        enc.destroy()


@pytest.mark.parametrize("order", ["decode_first", "encode_first"])
@pytest.mark.parametrize("cfg", ["long", "dropout"])
def test_configured_encoder_first_touch_order(cfg, order):
    """An encoder with long_words=True (one word of 1500 bytes in the large text) or with dropout set
    gives, in either order of first use, what a fresh encoder of the same configuration gives; with
    dropout turned off again it gives what a plain encoder gives."""
    enc = _new_encoder(cfg=cfg)
    try:
        for k in (0, 1):
            for step in ORDERS[order]:
                _step(enc, step, k, cfg)
        if cfg == "long":
            assert enc.long_word_stats["words"] > 0
        else:
            assert enc.dropout == (0.3, 7)
            enc.set_dropout(0, 0)
            for step in ORDERS[order]:
                _step(enc, step, 1)
    finally:
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
