"""GPU tests of what the fill-in-the-middle passes keep on the device between calls, in the manner of
test_gpu_encoder_lifetime.py: their state is created on the first FIM call, whatever ran before, grown
by a larger call, reused by a smaller one and freed with the encoder; two encoders do not share it.
What the passes compute is checked in test_gpu_fim.py; here the same calls must give the same results
in any order of first use, and encoders that did or did not run them must die cleanly.
"""
import numpy as np
import pytest

import fim_ref

pytestmark = pytest.mark.gpu

MERGES = np.array([[97, 98, 256], [256, 256, 257]], dtype=np.int32)  # "ab", "abab"
SPECIAL = b"<|s|>"
SENT = dict(pre_id=900, suf_id=901, mid_id=902)
TEXT = b"ab abab c abab\nab ab abc\n" * 40


def _rows(k):
    rng = np.random.default_rng(90 + k)
    row = np.concatenate([[0], np.cumsum(rng.integers(0, 12, size=(40, 3000, 7)[k]))]).astype(np.int64)
    return rng.integers(97, 100, size=int(row[-1])).astype(np.int32), row


def _new():
    from shredword.encoder import BPEEncoder
    return BPEEncoder.from_merges(MERGES, special_tokens=[SPECIAL])


def _others(e):
    ids, starts, line = e.encode_spans(TEXT, lines=True)
    pad = e.pad_rows(ids, line, bos=1, max_len=9, pad_id=-1)
    win = e.window_rows(ids, line, max_len=6, stride=2)
    mlm = e.mlm_rows(ids, line, mask_id=300, seed=2)
    cor = e.corrupt_rows(ids, line, sentinel_first=999, seed=2)
    return [ids, starts, line, *pad, *win, *mlm[:2], *cor]


def _fims(e, k):
    """Host and device calls on the k-th rows (small, large, small), and the character-level path."""
    import torch
    ids, row = _rows(k)
    kw = dict(SENT, seed=5 + k, src=True, seg=True, info=True)
    host = e.fim_rows(ids, row, **kw)
    *dev, ms = e.fim_device(torch.from_numpy(ids).cuda(), torch.from_numpy(row).cuda(), **kw)
    want = fim_ref.fim_ref(ids, row, seed=5 + k, **SENT)
    for got in (host, [t.cpu().numpy() for t in dev]):
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    *ch, ms = e.encode_fim([TEXT[:50 + 100 * k], b"", "é€ab".encode() * 9], seed=k, src=True, **SENT)
    return [*host, *[t.cpu().numpy() for t in ch]]


def test_first_fim_call_in_any_order():
    """An encoder that never runs FIM dies cleanly; one that runs it first, after other batch calls or
    between them gives the same results, through growth and reuse of the scratch."""
    runs = {}
    for order in (("others",), ("fim0",), ("others", "fim0", "fim1", "fim2"), ("fim1", "others", "fim0", "fim2", "fim1")):
        e = _new()
        try:
            for what in order:
                got = _others(e) if what == "others" else _fims(e, int(what[3]))
                want = runs.setdefault(what, got)
                assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), (order, what)
        finally:
            e.destroy()


def test_destroy_after_fim_calls_and_two_encoders_interleaved():
    a, b = _new(), _new()
    try:
        first = _fims(a, 0)
        big = _fims(b, 1)
        for k, (e, want) in enumerate(((b, first), (a, big), (a, first), (b, big))):
            got = _fims(e, 0 if want is first else 1)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), k
        a.destroy()
        a.destroy()                                    # a second destroy is a no-op
        got = _fims(b, 1)                              # b's state is its own
        assert all(np.array_equal(g, w) for g, w in zip(got, big))
        with _new() as c:                              # created after a's scratch was freed
            assert all(np.array_equal(g, w) for g, w in zip(_fims(c, 2), _fims(b, 2)))
    finally:
        a.destroy()
        b.destroy()
