"""GPU tests of the encoder core on its structural edges (tests/encode_shapes.py; the claims of every
shape are verified on the CPU by tests/test_encode_shapes_cpu.py).

Every shape runs packed and forced unpacked, on the word-cache path (default) and the direct kernel
(SHREDWORD_ENCODE_CACHE=0), through host `encode` and `encode_device` on an aligned tensor and on one
sliced at a 1-byte offset.  Ids are compared bit for bit with the oracle encoder.

The word-cache path heals itself: a wrong compare, a wrong inline copy or a mis-staged byte raises a
flag and the call reruns on the direct path with exact ids.  So every cached case also runs under
SHREDWORD_ENCODE_DEBUG and asserts that the library printed no "direct path" line: the cached kernels
themselves produced the result.  SHREDWORD_ENCODE_CACHE_SLOTS brings the table's growth, and the
overflow after growth, within reach of a few thousand words.
"""
import ctypes
import re

import numpy as np
import pytest

import encode_shapes as es
from encode_ref import oracle_encode, token_bytes

pytestmark = pytest.mark.gpu

PATHS = ("cache", "direct")
ENTRIES = ("host", "device", "device_off1")
C = es.K_CHUNK


def _enc(name, packing):
    from shredword.encoder import BPEEncoder
    return BPEEncoder.from_merges(es.SHAPES[name].merges, es.byte_map(packing))  # a fresh encoder per case


def _set_path(monkeypatch, path):
    monkeypatch.delenv("SHREDWORD_ENCODE_CACHE_SLOTS", raising=False)
    monkeypatch.delenv("SHREDWORD_ENCODE_PIECE", raising=False)
    monkeypatch.setenv("SHREDWORD_ENCODE_DEBUG", "1")
    if path == "cache":
        monkeypatch.delenv("SHREDWORD_ENCODE_CACHE", raising=False)
    else:
        monkeypatch.setenv("SHREDWORD_ENCODE_CACHE", "0")


def _device_text(text, entry):
    import torch
    if entry == "device":
        return torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    return torch.from_numpy(np.frombuffer(b"x" + text, dtype=np.uint8).copy()).cuda()[1:]  # unaligned base


def _encode(enc, text, entry):
    if entry == "host":
        return enc.encode(text)
    ids, _ = enc.encode_device(_device_text(text, entry))
    return ids.cpu().numpy()


def _debug_lines(capfd):
    err = capfd.readouterr().err
    return [l for l in err.splitlines() if "encoder: word cache" in l]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("packing", es.PACKINGS)
@pytest.mark.parametrize("name", es.MATRIX)
def test_shape_matches_oracle(name, packing, path, entry, monkeypatch, capfd):
    s = es.SHAPES[name]
    want = es.expected(name, packing)
    _set_path(monkeypatch, path)
    if s.family == "max_word" and entry == "host":
        monkeypatch.setenv("SHREDWORD_ENCODE_PIECE", str(es.K_MAX_WORD + 2))  # pieces cut around the word
    with _enc(name, packing) as enc:
        capfd.readouterr()
        if s.claims.get("raises"):
            assert want is None
            with pytest.raises(ValueError):
                _encode(enc, s.text, entry)
        else:
            got = _encode(enc, s.text, entry)
            assert got.dtype == np.int32
            assert got.size == want.size and np.array_equal(got, want), (name, np.flatnonzero(got != want)[:8])
            if s.family == "id16_edge":
                assert (got == s.claims["top_id"]).any()
        lines = _debug_lines(capfd)
    # the cached path produced this itself: no table growth at this size, no rerun on the direct path
    assert lines == [], lines


def _grow_case(monkeypatch, capfd, name, packing, entry, slots):
    s = es.SHAPES[name]
    _set_path(monkeypatch, "cache")
    monkeypatch.setenv("SHREDWORD_ENCODE_CACHE_SLOTS", slots)
    with _enc(name, packing) as enc:
        capfd.readouterr()
        got = _encode(enc, s.text, entry)
        lines = _debug_lines(capfd)
    assert got.dtype == np.int32 and np.array_equal(got, es.expected(name, packing))
    grows = [int(re.search(r"grows to (\d+) slots", l).group(1)) for l in lines if "grows to" in l]
    direct = [l for l in lines if "direct path" in l]
    assert len(grows) + len(direct) == len(lines)
    return lines, grows, direct


@pytest.mark.parametrize("entry", ("host", "device"))
@pytest.mark.parametrize("packing", es.PACKINGS)
def test_cache_grow(packing, entry, monkeypatch, capfd):
    """3000 distinct words into 1024 slots: the table grows (4x per step) and the cached path finishes."""
    lines, grows, direct = _grow_case(monkeypatch, capfd, "cache_grow", packing, entry,
                                      es.SHAPES["cache_grow"].claims["slots"])
    assert grows and grows[0] == 4096 and grows == [4096 * 4 ** k for k in range(len(grows))], lines
    assert direct == [], lines


@pytest.mark.parametrize("entry", ("host", "device"))
@pytest.mark.parametrize("packing", es.PACKINGS)
def test_cache_grow_then_direct(packing, entry, monkeypatch, capfd):
    """6000 distinct words, 1024 slots and a ceiling of 4096: one growth, then the direct path."""
    lines, grows, direct = _grow_case(monkeypatch, capfd, "cache_grow_then_direct", packing, entry,
                                      es.SHAPES["cache_grow_then_direct"].claims["slots"])
    assert grows == [4096] and len(direct) == 1, lines
    assert "grows to" in lines[0] and "direct path" in lines[1] and "(4096 slots)" in lines[1], lines


@pytest.mark.parametrize("slots,want_grows,want_direct", [
    ("1", [512, 2048, 8192], None),          # clamped up to one workgroup of slots (128)
    ("1000:1000", [], "(1024 slots)"),       # rounded up to a power of two; start == ceiling: no growth
    ("100:50", [], "(128 slots)"),           # ceiling below start: start holds
    ("2048:5000", [8192], None),             # ceiling rounded up to 8192
    ("999999999999", [], None),              # clamped down to the allocated table
])
def test_cache_slots_values(slots, want_grows, want_direct, monkeypatch, capfd):
    lines, grows, direct = _grow_case(monkeypatch, capfd, "cache_grow", "packed", "device", slots)
    assert grows == want_grows, lines
    if want_direct is None:
        assert direct == [], lines
    else:
        assert len(direct) == 1 and want_direct in direct[0], lines


@pytest.mark.parametrize("packing", es.PACKINGS)
def test_arena_overflow_reruns_and_is_named(packing, monkeypatch, capfd):
    """All-distinct short words need more arena than one int per text byte: exact ids from the direct
    path, and the line names the arena (the unencoded slots raise the collision flag as well)."""
    _set_path(monkeypatch, "cache")
    name = "arena_short_words"
    with _enc(name, packing) as enc:
        capfd.readouterr()
        got = _encode(enc, es.SHAPES[name].text, "device")
        lines = _debug_lines(capfd)
    assert got.dtype == np.int32 and np.array_equal(got, es.expected(name, packing))
    assert len(lines) == 1 and "arena overflow" in lines[0] and "direct path" in lines[0], lines


def _last_chunk_ids(s, want):
    """Ids of the words that start in the text's last chunk."""
    last = (len(s.text) - 1) // C * C
    first = min(m.start() for m in es.WORD.finditer(s.text) if m.start() >= last)
    return want.size - oracle_encode(s.merges, None, s.text[:first]).size


@pytest.mark.parametrize("entry", ("host", "device"))
@pytest.mark.parametrize("path", PATHS)
def test_capacity_over_several_chunks(path, entry, monkeypatch, capfd):
    """A too-small output over four chunks with ids in each: -2, and no id lands past cap (the cached
    path writes every chunk that fits in place and skips the others)."""
    import torch
    from shredword.cbase import lib
    s = es.SHAPES["capacity"]
    want = es.expected("capacity")
    T, tail = want.size, _last_chunk_ids(s, want)
    assert 0 < tail < T - 1
    _set_path(monkeypatch, path)
    GUARD, MARK = 64, -7
    with _enc("capacity", "packed") as enc:
        capfd.readouterr()
        if entry == "device":
            text = _device_text(s.text, "device")
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        else:
            text = np.frombuffer(s.text, dtype=np.uint8)
        for cap in (0, 1, T - tail - 1, T - 1, T):
            if entry == "device":
                out = torch.full((cap + GUARD,), MARK, dtype=torch.int32, device="cuda")
                r = lib.shred_encode_device(enc.enc, text.data_ptr(), text.numel(), out.data_ptr(), cap, st, None)
                got = out.cpu().numpy()
            else:
                got = np.full(cap + GUARD, MARK, dtype=np.int32)
                r = lib.shred_encode(enc.enc, text.ctypes.data, text.size, got.ctypes.data, cap)
            assert r == (T if cap == T else -2), (cap, r)
            assert (got[cap:] == MARK).all(), (cap, np.flatnonzero(got[cap:] != MARK)[:8])
            if cap == T:
                assert np.array_equal(got[:T], want)
        assert _debug_lines(capfd) == []


def test_reuse_across_sizes_and_paths(monkeypatch, capfd):
    """One encoder: 40 KB, 5 bytes, another 40 KB, the path flipped between calls; then the span calls,
    which share the scratch."""
    _set_path(monkeypatch, "cache")
    names = ("reuse_a", "reuse_short", "reuse_b")
    toks = token_bytes(es.MERGES)
    with _enc("reuse_a", "packed") as enc:
        capfd.readouterr()
        k = 0
        for _ in range(2):  # every text on both paths
            for name in names:
                _set_path(monkeypatch, PATHS[k % 2])
                k += 1
                got = enc.encode(es.SHAPES[name].text)
                assert got.dtype == np.int32 and np.array_equal(got, es.expected(name)), (name, k)
        for name in names:
            _set_path(monkeypatch, PATHS[k % 2])
            k += 1
            text = es.SHAPES[name].text
            ids, starts = enc.encode_spans(text)
            assert np.array_equal(ids, es.expected(name)), name
            assert all(text[p:p + len(toks[i])] == toks[i] for i, p in zip(ids.tolist(), starts.tolist())), name
        assert _debug_lines(capfd) == []
