"""GPU tests of where the encoder's device calls are queued: a call on device tensors must run behind
the work already queued on the caller's stream (include/shredword_encode.h: "queued on `stream` and
synchronised before return"), whichever stream that is.  The feature tests upload finished inputs and
stay on one stream, so they cannot see an entry point that runs on another stream than its caller's.

Every case makes the call's input late: on the caller's stream a spin kernel of nominally 50 ms runs
first, then a copy that turns well-formed stale content (spaces for text, id 0 for ids) into the real
input, then an event.  The event must still be pending when the call is made (else the case shows
nothing and fails with "delay too short"), must have completed when the call returns, and the outputs
must equal those of the same call on ready inputs, which are compared once per entry point with the
host-ABI method (the feature tests pin those against the Python references).  The offsets arrays are
passed ready, so a stale read changes results and never makes a call fail on malformed offsets.

The three stream modes: the caller on torch's default stream (the handle 0, which the C ABI reads as
"no stream given": BPEEncoder._stream orders the call behind that stream), inside torch.cuda.stream(s),
and on the default stream with the keyword stream=s.cuda_stream and the producer on s.

Observed on an MI355X before BPEEncoder._stream existed: every default-stream case failed, each
call returning while the copy into its input was still pending (its kernels had run on the encoder's
own stream, which the default stream does not order); the side-stream and keyword cases passed.

Not tested: that a call inside torch.cuda.stream(s) queues nothing on the default stream.  A pending
event on the default stream can only be kept pending by a second spin kernel there, and "the call
returned before it ended" would then assert how long the call takes, a timing assumption beyond the
one above.

The spin kernel counts shader cycles; its length comes from the device's clock rate, which this torch's
get_device_properties does not carry, so it is read from the HIP runtime when the attribute is absent.
"""
import ctypes

import numpy as np
import pytest

from encode_ref import oracle_encode
from test_gpu_encoder_lifetime import MERGES, SPECIAL, WORDS

pytestmark = pytest.mark.gpu

SIZE = 3 * 4096 + 1  # bytes of text: more than one encode chunk
LONG_WORD = 1500     # bytes of the word only the long-word encoder takes
DELAY_MS = 50
MASK = 300
MODES = ("default", "side", "keyword")
HIP_DEVICE_ATTRIBUTE_CLOCK_RATE = 5  # hipDeviceAttributeClockRate, in kHz


def _make_text(long_word):
    rng = np.random.default_rng(18)
    parts, size = [], 0
    while size < SIZE:
        parts.append(WORDS[int(rng.integers(len(WORDS)))] + (b"\n" if rng.integers(6) == 0 else b" "))
        size += len(parts[-1])
    text = b"".join(parts)[:SIZE]
    if long_word:
        at = text.index(b" ", SIZE // 2) + 1
        text = (text[:at] + (WORDS[-1] * LONG_WORD)[:LONG_WORD] + b" " + text[at:])[:SIZE]
    return text


class Data:
    """The inputs, on the host and ready on the device: the text, its ids in three rows with the middle
    one empty, the same rows reversed (the second segment of a pair), document offsets, token starts."""

    def __init__(self, enc):
        import torch
        dev = lambda a: torch.from_numpy(np.array(a)).cuda()
        self.text = _make_text(False)
        self.long_text = _make_text(True)
        self.ids = oracle_encode(MERGES, None, self.text)
        T = self.ids.size
        assert 0 < T < SIZE
        self.rows = np.array([0, T // 3, T // 3, T], dtype=np.int64)
        self.width = int(np.diff(self.rows).max()) + 1  # the longest row and its bos
        self.docs = np.array([0, SIZE // 3, 2 * SIZE // 3, SIZE], dtype=np.int64)
        self.ids_b = np.concatenate([self.ids[T // 3:], self.ids[:T // 3]])
        self.rows_b = np.array([0, T - T // 3, T - T // 3, T], dtype=np.int64)
        ids, self.starts = enc.encode_spans(self.text)
        assert np.array_equal(ids, self.ids)
        self.t_text = dev(np.frombuffer(self.text, dtype=np.uint8))
        self.t_long_text = dev(np.frombuffer(self.long_text, dtype=np.uint8))
        self.t_ids, self.t_rows, self.t_docs = dev(self.ids), dev(self.rows), dev(self.docs)
        self.t_ids_b, self.t_rows_b, self.t_starts = dev(self.ids_b), dev(self.rows_b), dev(self.starts)
        torch.cuda.synchronize()


PAD = dict(bos=1, pad_id=-1, mask=True)  # and the width given: Data.width
PACK = dict(seq_len=16, eos=0, pad_id=-1, positions=True, segments=True)
WINDOW = dict(max_len=8, stride=3, bos=1, mask=True)
PAIR = dict(max_len=16, truncation="window_second", stride=2, max_first=4, bos=1, sep=(2,), eos=3, mask=True)
MLM = dict(mask_id=MASK, p=0.3, seed=5)

# name -> (the attribute of Data that arrives late, the device call on it, the host-ABI call); "long" runs
# on the encoder with long_words=True
ENTRIES = {
    "encode": ("t_text", lambda e, d, x, **s: e.encode_device(x, **s), lambda e, d: (e.encode(d.text),)),
    "long": ("t_long_text", lambda e, d, x, **s: e.encode_device(x, **s), lambda e, d: (e.encode(d.long_text),)),
    "spans": ("t_text", lambda e, d, x, **s: e.encode_spans_device(x, lines=False, **s),
              lambda e, d: e.encode_spans(d.text)),
    "special": ("t_text", lambda e, d, x, **s: e.encode_spans_device(x, lines=False, specials=True, **s),
                lambda e, d: e.encode_spans(d.text, specials=True)),
    "docs": ("t_text", lambda e, d, x, **s: e.encode_docs_device(x, d.t_docs, starts=True, **s),
             lambda e, d: e.encode_docs(d.text, d.docs, starts=True)),
    "decode": ("t_ids", lambda e, d, x, **s: e.decode_device(x, d.t_rows, sep=b"\n", **s),
               lambda e, d: e.decode_rows(d.ids, d.rows, sep=b"\n")),
    "pad": ("t_ids", lambda e, d, x, **s: e.pad_device(x, d.t_rows, width=d.width, **PAD, **s),
            lambda e, d: e.pad_rows(d.ids, d.rows, width=d.width, **PAD)),
    "pack": ("t_ids", lambda e, d, x, **s: e.pack_device(x, d.t_rows, **PACK, **s),
             lambda e, d: e.pack_rows(d.ids, d.rows, **PACK)),
    "window": ("t_ids", lambda e, d, x, **s: e.window_device(x, d.t_rows, **WINDOW, **s),
               lambda e, d: e.window_rows(d.ids, d.rows, **WINDOW)),
    "pair": ("t_ids", lambda e, d, x, **s: e.pair_device(x, d.t_rows, d.t_ids_b, d.t_rows_b, **PAIR, **s),
             lambda e, d: e.pair_rows(d.ids, d.rows, d.ids_b, d.rows_b, **PAIR)),
    "mlm": ("t_ids", lambda e, d, x, **s: e.mlm_device(x, d.t_rows, **MLM, **s),
            lambda e, d: e.mlm_rows(d.ids, d.rows, **MLM)),
    "mlm_whole": ("t_ids",
                  lambda e, d, x, **s: e.mlm_device(x, d.t_rows, whole_word=True, starts=d.t_starts, **MLM, **s),
                  lambda e, d: e.mlm_rows(d.ids, d.rows, whole_word=True, starts=d.starts, **MLM)),
}


@pytest.fixture(scope="module")
def encs():
    from shredword.encoder import BPEEncoder
    both = {False: BPEEncoder.from_merges(MERGES, special_tokens=[SPECIAL]),
            True: BPEEncoder.from_merges(MERGES, special_tokens=[SPECIAL], long_words=True)}
    yield both
    for e in both.values():
        e.destroy()


@pytest.fixture(scope="module")
def data(encs):
    return Data(encs[False])


@pytest.fixture(scope="module")
def cycles():
    """Shader cycles of the spin kernel for a nominal DELAY_MS."""
    import torch
    khz = getattr(torch.cuda.get_device_properties(0), "clock_rate", None)
    if not khz:
        hip = ctypes.CDLL("libamdhip64.so")  # the runtime already in the process
        v = ctypes.c_int(0)
        assert hip.hipDeviceGetAttribute(ctypes.byref(v), HIP_DEVICE_ATTRIBUTE_CLOCK_RATE, 0) == 0
        khz = v.value
    assert khz > 0
    return int(khz) * DELAY_MS


def _plain(res):
    """What a call computed, on the host: tensors, arrays and bytes as arrays, counts as they are; the
    device times (floats, tuples of floats) and absent outputs (None) dropped."""
    import torch
    out = []
    for x in res if isinstance(res, tuple) else (res,):
        if isinstance(x, torch.Tensor):
            out.append(x.cpu().numpy().copy())
        elif isinstance(x, np.ndarray):
            out.append(x)
        elif isinstance(x, bytes):
            out.append(np.frombuffer(x, dtype=np.uint8))
        elif isinstance(x, (int, np.integer)) and not isinstance(x, bool):
            out.append(np.array(int(x)))
    return out


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, i)


_HOST_CHECKED = set()


def _want(encs, data, name, call):
    """Steps 1 and 2: the call on ready inputs (made as the observed call will be, so that every
    allocation it needs has happened), compared once per entry point with the host-ABI method."""
    import torch
    src_name, dev_call, host_call = ENTRIES[name]
    want = _plain(call(getattr(data, src_name)))
    torch.cuda.synchronize()
    if name not in _HOST_CHECKED:
        host = _plain(host_call(encs[name == "long"], data))
        assert sum(a.size for a in want) > SIZE // 12, "the entry point computes something"
        _same(want, host, (name, "device call against host call"))
        _HOST_CHECKED.add(name)
    return want


def _late_call(src, stale, producer, cycles, call):
    """Steps 3 to 7: the call on an input that the producer stream is still writing."""
    import torch
    late = torch.full_like(src, stale)
    ev = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(producer):
        torch.cuda._sleep(cycles)
        late.copy_(src)
        ev.record()
    assert not ev.query(), "delay too short"
    res = call(late)
    assert ev.query(), "the call returned before the work queued ahead of it on the caller's stream had run"
    got = _plain(res)
    torch.cuda.synchronize()
    return got


def _caller(enc, data, name, mode, side):
    """-> (call(x) made as the mode makes it, the stream the producer runs on)."""
    import torch
    dev_call = ENTRIES[name][1]
    if mode == "default":
        return (lambda x: dev_call(enc, data, x)), torch.cuda.default_stream()
    if mode == "keyword":
        return (lambda x: dev_call(enc, data, x, stream=side.cuda_stream)), side

    def in_side(x):
        with torch.cuda.stream(side):
            return dev_call(enc, data, x)
    return in_side, side


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(ENTRIES))
def test_call_runs_behind_its_stream(encs, data, cycles, name, mode):
    import torch
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
    assert torch.cuda.default_stream().cuda_stream == 0, "torch's default stream is the handle 0"
    enc = encs[name == "long"]
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    call, producer = _caller(enc, data, name, mode, side)
    want = _want(encs, data, name, call)
    src = getattr(data, ENTRIES[name][0])
    stale = 32 if src.dtype == torch.uint8 else 0
    got = _late_call(src, stale, producer, cycles, call)
    _same(got, want, (name, mode))


def _chain(enc, text_t, rows_t):
    """encode_spans_device -> pad_device -> masked-LM -> decode_device, each output fed to the next, with no
    host synchronisation of the caller's in between."""
    ids, starts, _, _ = enc.encode_spans_device(text_t, starts=True, lines=False)
    batch, lengths, mask, _ = enc.pad_device(ids, rows_t, bos=1, eos=2, pad_id=0, mask=True)
    masked, labels, selected, _ = enc.mlm_device(batch.view(-1), None, **MLM, protect=(0, 1, 2))
    data, boff, _ = enc.decode_device(masked, None, unk=b"?")
    return _plain((ids, starts, batch, lengths, mask, masked, labels, selected, data, boff))


def test_chain_on_a_side_stream(encs, data):
    """The chain on a side stream gives what it gives on the default stream."""
    import torch
    enc = encs[False]
    want = _chain(enc, data.t_text, data.t_rows)
    torch.cuda.synchronize()
    assert want[0].size == data.ids.size and np.array_equal(want[0], data.ids)
    assert want[7] > 0 and want[8].size >= data.ids.size  # tokens were selected, bytes came back
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _chain(enc, data.t_text, data.t_rows)
    torch.cuda.synchronize()
    _same(got, want, "chain")


@pytest.mark.parametrize("name", ["spans", "window", "mlm_whole"])
def test_alternating_streams_share_one_state(encs, data, name):
    """One entry point on two side streams and the default stream in turn, three rounds on one encoder:
    the pass's state and its timing events are shared by the streams."""
    import torch
    enc = encs[False]
    src_name, dev_call, _ = ENTRIES[name]
    src = getattr(data, src_name)
    want = _want(encs, data, name, lambda x: dev_call(enc, data, x))
    sides = [torch.cuda.Stream(), torch.cuda.Stream()]
    for rnd in range(3):
        for s in sides + [None]:
            if s is None:
                got = _plain(dev_call(enc, data, src))
            else:
                with torch.cuda.stream(s):
                    got = _plain(dev_call(enc, data, src))
            _same(got, want, (name, rnd, "default" if s is None else "side"))
    torch.cuda.synchronize()
