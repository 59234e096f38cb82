"""BPEEncoder — applies a trained ``.model`` to text on the GPU.

The reference writes ``.model`` / ``.vocab`` (shredword/csrc/bpe/bpe.cpp:388-432) but ships no
loader or encoder for them.  This one defines encoding as the trainer's own merge application
replayed on new text (include/shredword_encode.h): words are the runs of bytes outside
``"\\t\\r\\n "``, bytes map to symbol ids (bytes the trainer's coverage rule dropped map to
``unk_id`` when the ``.vocab`` is given), and the merges apply in training order.  Encoding the
training corpus reproduces the trainer's segmentation, so the id counts equal the ``.vocab``
frequencies.  Every call runs the gfx950 kernels through libtrainer.so; there is no CPU path.
"""
import atexit
import ctypes
import weakref

import numpy as np

from .cbase import ShredCorruptOpts, ShredFimOpts, ShredMlmOpts, lib

MAX_WORD = 1024  # SHRED_ENCODE_MAX_WORD
MAX_LONG_WORD = 1 << 20  # SHRED_ENCODE_MAX_LONG_WORD
MAX_UNK = 8      # SHRED_DECODE_MAX_UNK
MAX_SPECIALS = 256     # SHRED_SPECIAL_MAX
MAX_SPECIAL_LEN = 64   # SHRED_SPECIAL_MAX_LEN
# decode_device.hip: output bytes per workgroup of the expansion kernel (kTile), ids per workgroup of
# the strict-mode id check (kChunk)
DECODE_TILE = 4096
DECODE_CHUNK = 4096
# batch_device.hip: output entries per workgroup of the pad, pack and window kernels (kTile), rows the
# pack and window kernels stage in LDS per round (kStage)
BATCH_TILE = 1024
BATCH_STAGE = 512
# batch_pair.hip: the strategies of shred_pair_*, by number
PAIR_TRUNCATION = ("longest_first", "only_first", "only_second", "window_second")
MLM_MAX_PROTECT = 16   # SHRED_MLM_MAX_PROTECT
CORRUPT_MAX_SPAN = 32  # SHRED_CORRUPT_MAX_SPAN

# Encoders still alive at interpreter exit are destroyed while the HIP runtime is up (a destructor
# that ran after the runtime's own teardown would free its device memory twice).
_LIVE = weakref.WeakSet()


@atexit.register
def _destroy_live():
    for e in list(_LIVE):
        e.destroy()


def join_docs(texts):
    """A sequence of bytes / str documents (str as UTF-8) -> (uint8 array of the documents joined with
    nothing between them, int64 offsets with len(texts) + 1 entries): document d is
    array[offsets[d]:offsets[d + 1]], the form encode_docs takes."""
    docs = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in texts]
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], dtype=np.int64, out=off[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), off


class BPEEncoder:
    def __init__(self, model_path: str, vocab_path: str = None, unk_id: int = 0, device: int = 0,
                 special_tokens=None, *, long_words: bool = False, dropout: float = 0.0, seed: int = 0):
        """special_tokens: None or a list of bytes / str, see set_special_tokens.  long_words: see the
        property of that name.  dropout, seed: see set_dropout."""
        self.enc = lib.shred_encoder_load(model_path.encode("utf-8"),
                                          vocab_path.encode("utf-8") if vocab_path else None,
                                          int(unk_id), int(device))
        self.device = int(device)
        if not self.enc:
            raise RuntimeError(f"Failed to create the encoder for {model_path} (see stderr; a GPU is required)")
        _LIVE.add(self)
        self._specials = []
        self.long_words = long_words
        self.set_dropout(dropout, seed)
        if special_tokens:
            self.set_special_tokens(special_tokens)

    @classmethod
    def from_merges(cls, merges, byte_map=None, device: int = 0, special_tokens=None, *, long_words: bool = False,
                    dropout: float = 0.0, seed: int = 0):
        """merges: (M, 3) int32 array of (first, second, 256 + m) as in a .model file."""
        m = np.ascontiguousarray(np.asarray(merges, dtype=np.int32).reshape(-1, 3))
        bm = None if byte_map is None else np.ascontiguousarray(np.asarray(byte_map, dtype=np.int32))
        if bm is not None and bm.shape != (256,):
            raise ValueError("byte_map must hold 256 ids")
        self = cls.__new__(cls)
        self.enc = lib.shred_encoder_create(m.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), m.shape[0],
                                            None if bm is None else bm.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                            int(device))
        self.device = int(device)
        if not self.enc:
            raise RuntimeError("Failed to create the encoder (invalid merges or no GPU; see stderr)")
        _LIVE.add(self)
        self._specials = []
        self.long_words = long_words
        self.set_dropout(dropout, seed)
        if special_tokens:
            self.set_special_tokens(special_tokens)
        return self

    @property
    def long_words(self) -> bool:
        """False (the default): a word longer than MAX_WORD bytes fails the call with ValueError.  True:
        every encode call takes words of up to MAX_LONG_WORD bytes; one workgroup encodes each word above
        MAX_WORD, to the ids the merge list defines for it.  A call then reads the text once more to find
        such words."""
        return bool(lib.shred_encoder_long_words(self.enc))

    @long_words.setter
    def long_words(self, on: bool):
        lib.shred_encoder_set_long_words(self.enc, int(bool(on)))

    @property
    def long_word_stats(self) -> dict:
        """The long-word pass so far: scratch_bytes it has allocated on the device (0 until a call meets a
        long word), the long words it has encoded, the rounds it has run."""
        v = [ctypes.c_uint64() for _ in range(3)]
        lib.shred_encoder_long_stats(self.enc, *(ctypes.byref(x) for x in v))
        return dict(zip(("scratch_bytes", "words", "rounds"), (x.value for x in v)))

    def set_dropout(self, p: float, seed: int = 0):
        """BPE-dropout (subword regularisation): with p > 0 every encode call drops each candidate merge
        with probability p, so a word's segmentation varies with its place in the text and with the seed;
        p = 0 (the default) is the canonical segmentation, p = 1 leaves every byte on its own.  A candidate
        is dropped once and for all, as a function of (seed, byte position in the text, merge rank): the
        same (text, p, seed) always gives the same ids, on host and device calls alike, and a new seed (one
        per epoch, say) a new segmentation.  Words above MAX_WORD bytes (long_words) are never dropped.
        p outside [0, 1] raises ValueError and leaves the setting as it was."""
        if lib.shred_encoder_set_dropout(self.enc, float(p), int(seed) & (2 ** 64 - 1)):
            raise ValueError("dropout must be a probability in [0, 1]")

    @property
    def dropout(self) -> tuple:
        """(p, seed) as set_dropout set them."""
        p, seed = ctypes.c_double(), ctypes.c_uint64()
        lib.shred_encoder_dropout(self.enc, ctypes.byref(p), ctypes.byref(seed))
        return p.value, seed.value

    def set_special_tokens(self, tokens):
        """Replaces the encoder's special tokens (an empty list clears them).  tokens: bytes / str, at most
        256 distinct ones of 1 to 64 bytes without a delimiter byte (tab, CR, LF, space); token i gets id
        256 + num_merges + i.  They are matched only by the calls given specials=True (leftmost, then
        longest, without overlap; no merge reaches across a match), and every decode call turns their
        ids back into their bytes.  A rejected list raises ValueError and leaves the set as it was."""
        toks = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in tokens]
        data = np.frombuffer(b"".join(toks) or b"\0", dtype=np.uint8)
        off = (ctypes.c_size_t * (len(toks) + 1))(*np.cumsum([0] + [len(t) for t in toks]).tolist())
        if lib.shred_encoder_set_specials(self.enc, data.ctypes.data, off, len(toks)):
            raise ValueError(f"special tokens must be at most {MAX_SPECIALS} distinct byte strings of 1 to "
                             f"{MAX_SPECIAL_LEN} bytes without a delimiter byte")
        self._specials = toks

    @property
    def special_tokens(self) -> dict:
        """The registered special tokens: bytes -> id."""
        base = 256 + self.num_merges
        return {t: base + i for i, t in enumerate(self._specials)}

    @property
    def num_merges(self) -> int:
        n = ctypes.c_size_t()
        lib.shred_encoder_info(self.enc, ctypes.byref(n), None)
        return n.value

    @property
    def byte_map(self) -> np.ndarray:
        out = np.empty(256, dtype=np.int32)
        lib.shred_encoder_info(self.enc, None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        return out

    @property
    def token_lengths(self) -> np.ndarray:
        """Source bytes each id covers: int32, 256 + num_merges entries (ids below 256: 1), then one per
        special token."""
        out = np.empty(256 + self.num_merges + len(self._specials), dtype=np.int32)
        if lib.shred_encoder_token_lengths(self.enc, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), out.size):
            raise RuntimeError("token_lengths failed")
        return out

    def _check(self, r: int) -> int:
        if r == -3:
            raise ValueError(f"a word is longer than {MAX_LONG_WORD if self.long_words else MAX_WORD} bytes")
        if r == -4:
            raise ValueError("the byte map holds an id >= 256: token lengths are undefined")
        if r < 0:
            raise RuntimeError(f"encode failed (code {r})")
        return r

    @staticmethod
    def _stream(stream, device):
        """The hipStream_t of a device call as the C ABI takes it: `stream` (a handle), or for None the
        caller's current torch stream on `device`.  The handle 0, torch's default stream, reads as "no
        stream given" in the C ABI, which then queues on the encoder's own non-blocking stream; that
        stream is not ordered with the legacy default stream.  So work already queued there (the
        producer of the call's inputs, say) is waited for here, and the call, which synchronises its
        stream before it returns, is ordered behind it."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(device).cuda_stream
        if not stream:
            torch.cuda.default_stream(device).synchronize()
        return ctypes.c_void_p(stream)

    @staticmethod
    def _host_text(text) -> np.ndarray:
        if isinstance(text, str):
            text = text.encode("utf-8")
        return np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) \
            else np.ascontiguousarray(text, dtype=np.uint8)

    def encode(self, text, specials: bool = False) -> np.ndarray:
        """bytes / str / uint8 array -> int32 ids of every word, in text order.  specials: match the
        registered special tokens in the text (set_special_tokens)."""
        if specials:
            return self._spans_host(text, False, False, True)[0]
        buf = self._host_text(text)
        out = np.empty(max(1, buf.size), dtype=np.int32)
        r = self._check(lib.shred_encode(self.enc, buf.ctypes.data, buf.size, out.ctypes.data, out.size))
        return out[:r].copy()

    def encode_device(self, text, out=None, stream=None):
        """text: 1-D uint8 torch tensor on the encoder's GPU -> (int32 tensor view of the ids,
        device milliseconds of the encode kernels)."""
        import torch
        if text.dtype != torch.uint8 or text.dim() != 1 or not text.is_cuda or not text.is_contiguous():
            raise ValueError("text must be a contiguous 1-D uint8 CUDA tensor")
        if text.device.index != self.device:
            raise ValueError(f"text is on {text.device}, the encoder on cuda:{self.device}")
        n = text.numel()
        if out is None:
            out = torch.empty(max(1, n), dtype=torch.int32, device=text.device)
        elif out.dtype != torch.int32 or not out.is_cuda or not out.is_contiguous() or out.device != text.device:
            raise ValueError("out must be a contiguous int32 tensor on the text's device")
        ms = ctypes.c_double()
        st = self._stream(stream, text.device)
        r = self._check(lib.shred_encode_device(self.enc, text.data_ptr(), n, out.data_ptr(), out.numel(),
                                                st, ctypes.byref(ms)))
        return out[:r], ms.value

    def _spans_host(self, text, want_starts, want_lines, specials=False):
        buf = self._host_text(text)
        out = np.empty(max(1, buf.size), dtype=np.int32)
        starts = np.empty(out.size, dtype=np.int64) if want_starts else None
        line = np.empty(np.count_nonzero(buf == 10) + 2, dtype=np.int64) if want_lines else None
        nl = ctypes.c_size_t()
        call = lib.shred_encode_special if specials else lib.shred_encode_spans
        r = self._check(call(self.enc, buf.ctypes.data, buf.size, out.ctypes.data, out.size,
                             None if starts is None else starts.ctypes.data,
                             None if line is None else line.ctypes.data,
                             0 if line is None else line.size, ctypes.byref(nl)))
        return (out[:r].copy(), None if starts is None else starts[:r].copy(),
                None if line is None else line[:nl.value + 1].copy())

    def encode_lines(self, text, specials: bool = False):
        """-> (ids, line_offsets): line i (split on '\\n' only) holds ids[line_offsets[i]:line_offsets[i + 1]];
        int64, lines + 1 entries, where a text not ending in '\\n' has a last line of its own.
        specials: as encode."""
        ids, _, line = self._spans_host(text, False, True, specials)
        return ids, line

    def encode_spans(self, text, lines: bool = False, specials: bool = False):
        """-> (ids, starts) or (ids, starts, line_offsets).  starts[k] (int64) is the byte offset in
        the text of token k's first byte; the token ends at starts[k] + token_lengths[max(ids[k], 0)]
        (an id below 256 covers 1 byte), and begins a word iff k == 0 or it does not start where
        token k - 1 ended.  specials: as encode; a special token starts at its match, covers its own
        bytes and is a word of its own."""
        ids, starts, line = self._spans_host(text, True, lines, specials)
        return (ids, starts, line) if lines else (ids, starts)

    def encode_spans_device(self, text, starts: bool = True, lines: bool = True, stream=None,
                            specials: bool = False):
        """text: 1-D uint8 torch tensor on the encoder's GPU -> (ids, starts or None, line_offsets or
        None, (encode_ms, spans_ms)): int32 / int64 / int64 tensor views on the text's device.
        specials: as encode; the times are then (encode_ms, spans_ms, specials_ms)."""
        import torch
        if text.dtype != torch.uint8 or text.dim() != 1 or not text.is_cuda or not text.is_contiguous():
            raise ValueError("text must be a contiguous 1-D uint8 CUDA tensor")
        if text.device.index != self.device:
            raise ValueError(f"text is on {text.device}, the encoder on cuda:{self.device}")
        n = text.numel()
        out = torch.empty(max(1, n), dtype=torch.int32, device=text.device)
        st_t = torch.empty(max(1, n), dtype=torch.int64, device=text.device) if starts else None
        ln_t = torch.empty(int((text == 10).sum().item()) + 1 + 1, dtype=torch.int64, device=text.device) \
            if lines else None
        ms = (ctypes.c_double * 3)()
        nl = ctypes.c_size_t()
        st = self._stream(stream, text.device)
        call = lib.shred_encode_special_device if specials else lib.shred_encode_spans_device
        r = self._check(call(
            self.enc, text.data_ptr(), n, out.data_ptr(), out.numel(),
            None if st_t is None else st_t.data_ptr(), None if ln_t is None else ln_t.data_ptr(),
            0 if ln_t is None else ln_t.numel(), ctypes.byref(nl), st, ms))
        return (out[:r], None if st_t is None else st_t[:r], None if ln_t is None else ln_t[:nl.value + 1],
                (ms[0], ms[1], ms[2]) if specials else (ms[0], ms[1]))

    # ---- batches of documents: rows cut at given byte offsets (include/shredword_encode.h) --------

    def _check_docs(self, r: int) -> int:
        if r == -6:
            raise ValueError("doc_offsets must be 0 = doc_offsets[0] <= ... <= doc_offsets[docs] = len(text)")
        return self._check(r)

    def encode_docs(self, text, doc_offsets=None, *, starts: bool = False, specials: bool = False):
        """-> (ids, row_offsets) or (ids, row_offsets, starts).  text holds the documents concatenated with
        nothing between them; document d is text[doc_offsets[d]:doc_offsets[d + 1]] (docs + 1 offsets from
        0 to len(text), non-decreasing; None: one document).  Each document is encoded as if alone: no
        word, merge or special token reaches across a boundary, and a '\\n' inside a document is an
        ordinary delimiter.  Row d of the result is ids[row_offsets[d]:row_offsets[d + 1]] (int64, docs
        + 1 entries, the line_offsets format: pad_rows, pack_rows and decode_rows take it).  starts: the
        byte offset of every token in `text`.  specials: as encode."""
        buf = self._host_text(text)
        off = None if doc_offsets is None else np.ascontiguousarray(doc_offsets, dtype=np.int64).reshape(-1)
        if off is not None and off.size == 0:
            raise ValueError("doc_offsets must hold docs + 1 entries")
        docs = 0 if off is None else off.size - 1
        out = np.empty(max(1, buf.size), dtype=np.int32)
        st = np.empty(out.size, dtype=np.int64) if starts else None
        row = np.empty((docs if off is not None else 1) + 1, dtype=np.int64)
        r = self._check_docs(lib.shred_encode_docs(
            self.enc, buf.ctypes.data, buf.size, None if off is None else off.ctypes.data, docs, int(bool(specials)),
            out.ctypes.data, out.size, None if st is None else st.ctypes.data, row.ctypes.data))
        return (out[:r].copy(), row, st[:r].copy()) if starts else (out[:r].copy(), row)

    def encode_batch(self, texts, *, starts: bool = False, specials: bool = False):
        """A sequence of bytes / str documents -> encode_docs of them joined (join_docs): one row per
        document, whatever '\\n' bytes the documents hold.  An empty sequence gives no id and row_offsets [0]."""
        buf, off = join_docs(texts)
        return self.encode_docs(buf, off, starts=starts, specials=specials)

    def encode_docs_device(self, text, doc_offsets=None, *, starts: bool = False, specials: bool = False, stream=None):
        """encode_docs on device tensors: text a 1-D uint8 torch tensor on the encoder's GPU, doc_offsets None
        or a 1-D int64 tensor there (validated on the device) -> (ids, row_offsets, starts or None,
        (encode_ms, spans_ms, specials_ms, docs_ms)): int32 / int64 / int64 tensor views on the text's device."""
        import torch
        for name, t, dt in (("text", text, torch.uint8), ("doc_offsets", doc_offsets, torch.int64)):
            if t is None and name != "text":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or not t.is_cuda \
                    or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous 1-D {dt} CUDA tensor")
            if t.device.index != self.device:
                raise ValueError(f"{name} is on {t.device}, the encoder on cuda:{self.device}")
        if doc_offsets is not None and doc_offsets.numel() == 0:
            raise ValueError("doc_offsets must hold docs + 1 entries")
        n = text.numel()
        docs = 0 if doc_offsets is None else doc_offsets.numel() - 1
        out = torch.empty(max(1, n), dtype=torch.int32, device=text.device)
        st_t = torch.empty(max(1, n), dtype=torch.int64, device=text.device) if starts else None
        row = torch.empty((docs if doc_offsets is not None else 1) + 1, dtype=torch.int64, device=text.device)
        ms = (ctypes.c_double * 4)()
        st = self._stream(stream, text.device)
        r = self._check_docs(lib.shred_encode_docs_device(
            self.enc, text.data_ptr(), n, None if doc_offsets is None else doc_offsets.data_ptr(), docs,
            int(bool(specials)), out.data_ptr(), out.numel(), None if st_t is None else st_t.data_ptr(),
            row.data_ptr(), st, ms))
        return out[:r], row, None if st_t is None else st_t[:r], (ms[0], ms[1], ms[2], ms[3])

    def decode(self, ids) -> bytes:
        """Concatenated bytes of the ids (whitespace between words is not restored)."""
        a = np.ascontiguousarray(ids, dtype=np.int32)
        need = lib.shred_decode(self.enc, a.ctypes.data, a.size, None, 0)
        if need < 0:
            raise ValueError("id outside the vocabulary")
        out = np.empty(max(1, need), dtype=np.uint8)
        lib.shred_decode(self.enc, a.ctypes.data, a.size, out.ctypes.data, out.size)
        return out[:need].tobytes()

    @staticmethod
    def _decode_args(sep, unk):
        if sep is not None and (not isinstance(sep, (bytes, bytearray)) or len(sep) != 1):
            raise ValueError("sep must be None or one byte")
        if unk is not None and (not isinstance(unk, (bytes, bytearray)) or len(unk) > MAX_UNK):
            raise ValueError(f"unk must be None or at most {MAX_UNK} bytes")
        return (-1 if sep is None else sep[0]), (None if unk is None else bytes(unk)), (-1 if unk is None else len(unk))

    @staticmethod
    def _check_decode(r: int) -> int:
        if r == -6:
            raise ValueError("row_offsets must be 0 = row_offsets[0] <= ... <= row_offsets[rows] = len(ids)")
        if r == -5:
            raise RuntimeError("the vocabulary's bytes exceed the device decoder's limit")
        if r < 0:
            raise RuntimeError(f"decode failed (code {r})")
        return r

    def decode_rows(self, ids, row_offsets=None, sep=None, unk=None):
        """-> (bytes, byte_offsets).  Row r holds ids[row_offsets[r]:row_offsets[r + 1]] (the
        line_offsets format of encode_lines; None: one row of all ids).  sep: None or one byte
        written after every row, empty rows included.  unk: None (an id outside the vocabulary
        raises ValueError) or at most 8 bytes that every such id decodes to (b"" drops it).
        byte_offsets (int64, rows + 1 entries): row r without its separator is
        bytes[byte_offsets[r]:byte_offsets[r + 1] - len(sep or b"")].  Decoded on the GPU."""
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        row = None if row_offsets is None else np.ascontiguousarray(row_offsets, dtype=np.int64).reshape(-1)
        if row is not None and row.size == 0:
            raise ValueError("row_offsets must hold rows + 1 entries")
        s, u, ul = self._decode_args(sep, unk)
        rows = 0 if row is None else row.size - 1
        args = (self.enc, a.ctypes.data, a.size, None if row is None else row.ctypes.data, rows)
        need = lib.shred_decode_rows(*args, None, 0, None, s, u, ul)
        if need == -1 and unk is None:
            raise ValueError("id outside the vocabulary")
        self._check_decode(need)
        out = np.empty(max(1, need), dtype=np.uint8)
        boff = np.empty((rows if row is not None else 1) + 1, dtype=np.int64)
        r = self._check_decode(lib.shred_decode_rows(*args, out.ctypes.data, need, boff.ctypes.data, s, u, ul))
        return out[:r].tobytes(), boff

    def decode_lines(self, ids, line_offsets, unk=None):
        """The inverse of encode_lines up to the delimiters inside a line: -> list of bytes, one per row."""
        data, boff = self.decode_rows(ids, line_offsets, sep=b"\n", unk=unk)
        return [data[boff[i]:boff[i + 1] - 1] for i in range(boff.size - 1)]

    def decode_device(self, ids, row_offsets=None, sep=None, unk=None, stream=None):
        """ids: 1-D int32 torch tensor on the encoder's GPU, row_offsets: None or a 1-D int64 tensor
        there (the views encode_spans_device returns fit) -> (uint8 tensor, int64 byte_offsets
        tensor, device milliseconds of the decode passes); arguments as decode_rows."""
        import torch
        for name, t, dt in (("ids", ids, torch.int32), ("row_offsets", row_offsets, torch.int64)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or not t.is_cuda \
                    or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous 1-D {dt} CUDA tensor")
            if t.device.index != self.device:
                raise ValueError(f"{name} is on {t.device}, the encoder on cuda:{self.device}")
        if row_offsets is not None and row_offsets.numel() == 0:
            raise ValueError("row_offsets must hold rows + 1 entries")
        s, u, ul = self._decode_args(sep, unk)
        rows = 0 if row_offsets is None else row_offsets.numel() - 1
        st = self._stream(stream, ids.device)
        args = (self.enc, ids.data_ptr(), ids.numel(), None if row_offsets is None else row_offsets.data_ptr(), rows)
        ms0, ms1 = ctypes.c_double(), ctypes.c_double()
        need = lib.shred_decode_device(*args, None, 0, None, s, u, ul, st, ctypes.byref(ms0))
        if need == -1 and unk is None:
            raise ValueError("id outside the vocabulary (or a device error; see stderr)")
        self._check_decode(need)
        out = torch.empty(max(1, need), dtype=torch.uint8, device=ids.device)
        boff = torch.empty((rows if row_offsets is not None else 1) + 1, dtype=torch.int64, device=ids.device)
        r = self._check_decode(lib.shred_decode_device(*args, out.data_ptr(), need, boff.data_ptr(), s, u, ul, st,
                                                       ctypes.byref(ms1)))
        return out[:r], boff, ms1.value

    # ---- rows of ids to padded batches and packed sequences (include/shredword_encode.h) ----------

    @staticmethod
    def _int32(name, v):
        v = int(v)
        if not -2 ** 31 <= v < 2 ** 31:
            raise ValueError(f"{name} must fit an int32")
        return v

    @classmethod
    def _batch_args(cls, bos, eos, max_len, truncate, pad_id):
        """-> (bos pointer, eos pointer, max_len, trunc_side, pad_id) as the C ABI takes them."""
        if truncate not in ("left", "right"):
            raise ValueError('truncate must be "left" or "right"')
        add = (bos is not None) + (eos is not None)
        ml = 0 if max_len is None else int(max_len)
        if ml < 0 or (ml and ml < add):
            raise ValueError(f"max_len must leave room for the {add} added ids")
        ptr = lambda name, v: None if v is None else ctypes.byref(ctypes.c_int32(cls._int32(name, v)))
        return ptr("bos", bos), ptr("eos", eos), ml, int(truncate == "left"), cls._int32("pad_id", pad_id)

    @staticmethod
    def _check_batch(r: int) -> int:
        if r == -6:
            raise ValueError("row_offsets must be 0 = row_offsets[0] <= ... <= row_offsets[rows] = len(ids)")
        if r < 0:
            raise RuntimeError(f"batch call failed (code {r})")
        return r

    @staticmethod
    def _host_rows(ids, row_offsets):
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        row = None if row_offsets is None else np.ascontiguousarray(row_offsets, dtype=np.int64).reshape(-1)
        if row is not None and row.size == 0:
            raise ValueError("row_offsets must hold rows + 1 entries")
        return a, row, (1 if row is None else row.size - 1)

    def _device_rows(self, ids, row_offsets):
        import torch
        for name, t, dt in (("ids", ids, torch.int32), ("row_offsets", row_offsets, torch.int64)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or not t.is_cuda \
                    or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous 1-D {dt} CUDA tensor")
            if t.device.index != self.device:
                raise ValueError(f"{name} is on {t.device}, the encoder on cuda:{self.device}")
        if row_offsets is not None and row_offsets.numel() == 0:
            raise ValueError("row_offsets must hold rows + 1 entries")
        return 1 if row_offsets is None else row_offsets.numel() - 1

    def pad_rows(self, ids, row_offsets=None, *, bos=None, eos=None, max_len=None, truncate="right", pad_id=0,
                 pad="right", width=None, mask=False):
        """-> (batch, lengths) or (batch, lengths, mask): the padded batch of the rows
        ids[row_offsets[r]:row_offsets[r + 1]] (the line_offsets format of encode_lines; None: one row).
        Each row becomes [bos] + its ids + [eos], cut to max_len ids in all (None or 0: no limit) by
        dropping ids on the `truncate` side, and padded with pad_id on the `pad` side to `width`
        (None: the longest emitted row).  batch: int32 [rows, width]; lengths: int32 [rows], the
        emitted lengths; mask: uint8 [rows, width], 1 on tokens.  Built on the GPU."""
        if pad not in ("left", "right"):
            raise ValueError('pad must be "left" or "right"')
        b, e, ml, ts, pid = self._batch_args(bos, eos, max_len, truncate, pad_id)
        a, row, R = self._host_rows(ids, row_offsets)
        args = (self.enc, a.ctypes.data, a.size, None if row is None else row.ctypes.data,
                0 if row is None else R, b, e, ml, ts)
        ps = int(pad == "left")
        if width is None:
            width = self._check_batch(lib.shred_pad_rows(*args, 0, pid, ps, None, 0, None, None))
        W = int(width)
        if W < 0:
            raise ValueError("width must not be negative")
        out = np.empty(max(1, R * W), dtype=np.int32)
        lengths = np.empty(max(1, R), dtype=np.int32)
        m = np.empty(max(1, R * W), dtype=np.uint8) if mask else None
        need = self._check_batch(lib.shred_pad_rows(*args, W, pid, ps, out.ctypes.data, R * W, lengths.ctypes.data,
                                                    None if m is None else m.ctypes.data))
        if need > W:
            raise ValueError(f"width {W} is smaller than the longest row ({need} ids)")
        res = (out[:R * W].reshape(R, W), lengths[:R])
        return res + (m[:R * W].reshape(R, W),) if mask else res

    def pack_rows(self, ids, row_offsets=None, *, seq_len, bos=None, eos=None, max_len=None, truncate="right",
                  pad_id=0, drop_last=False, positions=False, segments=False):
        """-> (seqs, row_start[, positions][, segments]).  The rows, each emitted as in pad_rows, are
        concatenated into one stream and cut into sequences of seq_len: seqs is int32 [S, seq_len], the
        last sequence filled with pad_id, or dropped with drop_last when it is not full.  row_start
        (int64, rows + 1): the stream offset of every emitted row, row_start[rows] the stream's
        length.  positions / segments (int32 [S, seq_len]): each token's index inside its emitted
        row, and its row; padding gets 0 and -1.  Built on the GPU."""
        if int(seq_len) < 1:
            raise ValueError("seq_len must be at least 1")
        L = int(seq_len)
        b, e, ml, ts, pid = self._batch_args(bos, eos, max_len, truncate, pad_id)
        a, row, R = self._host_rows(ids, row_offsets)
        args = (self.enc, a.ctypes.data, a.size, None if row is None else row.ctypes.data,
                0 if row is None else R, b, e, ml, ts, L, pid, int(bool(drop_last)))
        S = self._check_batch(lib.shred_pack_rows(*args, None, 0, None, None, None))
        out = np.empty(max(1, S * L), dtype=np.int32)
        pos = np.empty(max(1, S * L), dtype=np.int32) if positions else None
        seg = np.empty(max(1, S * L), dtype=np.int32) if segments else None
        start = np.empty(R + 1, dtype=np.int64)
        self._check_batch(lib.shred_pack_rows(*args, out.ctypes.data, S * L, None if pos is None else pos.ctypes.data,
                                              None if seg is None else seg.ctypes.data, start.ctypes.data))
        res = (out[:S * L].reshape(S, L), start)
        res += (pos[:S * L].reshape(S, L),) if positions else ()
        return res + ((seg[:S * L].reshape(S, L),) if segments else ())

    def pad_device(self, ids, row_offsets=None, *, bos=None, eos=None, max_len=None, truncate="right", pad_id=0,
                   pad="right", width=None, mask=False, stream=None):
        """pad_rows on device tensors: ids a 1-D int32 torch tensor on the encoder's GPU, row_offsets None
        or a 1-D int64 tensor there (the views encode_spans_device returns fit) -> (batch, lengths[,
        mask], device milliseconds of the batch passes), tensors on the same device."""
        import torch
        if pad not in ("left", "right"):
            raise ValueError('pad must be "left" or "right"')
        b, e, ml, ts, pid = self._batch_args(bos, eos, max_len, truncate, pad_id)
        R = self._device_rows(ids, row_offsets)
        st = self._stream(stream, ids.device)
        args = (self.enc, ids.data_ptr(), ids.numel(), None if row_offsets is None else row_offsets.data_ptr(),
                0 if row_offsets is None else R, b, e, ml, ts)
        ps = int(pad == "left")
        ms = ctypes.c_double()
        if width is None:
            width = self._check_batch(lib.shred_pad_device(*args, 0, pid, ps, None, 0, None, None, st, None))
        W = int(width)
        if W < 0:
            raise ValueError("width must not be negative")
        out = torch.empty(max(1, R * W), dtype=torch.int32, device=ids.device)
        lengths = torch.empty(max(1, R), dtype=torch.int32, device=ids.device)
        m = torch.empty(max(1, R * W), dtype=torch.uint8, device=ids.device) if mask else None
        need = self._check_batch(lib.shred_pad_device(*args, W, pid, ps, out.data_ptr(), R * W, lengths.data_ptr(),
                                                      None if m is None else m.data_ptr(), st, ctypes.byref(ms)))
        if need > W:
            raise ValueError(f"width {W} is smaller than the longest row ({need} ids)")
        res = (out[:R * W].view(R, W), lengths[:R])
        return res + ((m[:R * W].view(R, W),) if mask else ()) + (ms.value,)

    def pack_device(self, ids, row_offsets=None, *, seq_len, bos=None, eos=None, max_len=None, truncate="right",
                    pad_id=0, drop_last=False, positions=False, segments=False, stream=None):
        """pack_rows on device tensors (as pad_device takes them) -> (seqs, row_start[, positions][,
        segments], device milliseconds of the batch passes)."""
        import torch
        if int(seq_len) < 1:
            raise ValueError("seq_len must be at least 1")
        L = int(seq_len)
        b, e, ml, ts, pid = self._batch_args(bos, eos, max_len, truncate, pad_id)
        R = self._device_rows(ids, row_offsets)
        st = self._stream(stream, ids.device)
        args = (self.enc, ids.data_ptr(), ids.numel(), None if row_offsets is None else row_offsets.data_ptr(),
                0 if row_offsets is None else R, b, e, ml, ts, L, pid, int(bool(drop_last)))
        ms = ctypes.c_double()
        S = self._check_batch(lib.shred_pack_device(*args, None, 0, None, None, None, st, None))
        new = lambda dt, k: torch.empty(max(1, k), dtype=dt, device=ids.device)
        out = new(torch.int32, S * L)
        pos = new(torch.int32, S * L) if positions else None
        seg = new(torch.int32, S * L) if segments else None
        start = new(torch.int64, R + 1)
        self._check_batch(lib.shred_pack_device(*args, out.data_ptr(), S * L, None if pos is None else pos.data_ptr(),
                                                None if seg is None else seg.data_ptr(), start.data_ptr(), st,
                                                ctypes.byref(ms)))
        res = (out[:S * L].view(S, L), start)
        res += (pos[:S * L].view(S, L),) if positions else ()
        return res + ((seg[:S * L].view(S, L),) if segments else ()) + (ms.value,)

    # ---- long rows cut into overlapping windows (include/shredword_encode.h, shred_window_*) -------

    @classmethod
    def _window_args(cls, bos, eos, max_len, stride, pad_id, pad):
        """-> (bos pointer, eos pointer, max_len, stride, pad_id, pad_side) as the C ABI takes them."""
        if pad not in ("left", "right"):
            raise ValueError('pad must be "left" or "right"')
        add = (bos is not None) + (eos is not None)
        ml, sd = int(max_len), int(stride)
        if not add < ml < 2 ** 31:
            raise ValueError(f"max_len must hold the {add} added ids and at least one more, and fit an int32")
        if not 0 <= sd < ml - add:
            raise ValueError(f"stride must be in [0, max_len - {add}): a window must move on by at least one id")
        b, e, _, _, pid = cls._batch_args(bos, eos, ml, "right", pad_id)
        return b, e, ml, sd, pid, int(pad == "left")

    def window_rows(self, ids, row_offsets=None, *, max_len, stride=0, bos=None, eos=None, pad_id=0, pad="right",
                    width=None, mask=False):
        """-> (batch, lengths, window_rows, window_src, row_windows[, mask]): every row
        ids[row_offsets[r]:row_offsets[r + 1]] (None: one row) cut into windows of at most max_len ids,
        [bos] and [eos] included, that overlap by `stride` ids ("overflowing tokens with a stride").
        Nothing is dropped: a row longer than a window takes several rows of the batch, and an empty
        row one.  batch: int32 [windows, width] (width None: the longest window), padded with pad_id on
        the `pad` side; lengths: int32 [windows]; window_rows: int32 [windows], the row of each window;
        window_src: int64 [windows], the index in ids of the window's first id (ids[window_src[w] + c -
        (bos is not None)] sits at batch[w, c], and the same index into the starts of encode_spans /
        encode_docs is its byte offset); row_windows: int64 [rows + 1], row r owns the windows
        [row_windows[r], row_windows[r + 1]); mask: uint8 [windows, width], 1 on tokens.  Built on the GPU."""
        b, e, ml, sd, pid, ps = self._window_args(bos, eos, max_len, stride, pad_id, pad)
        a, row, R = self._host_rows(ids, row_offsets)
        args = (self.enc, a.ctypes.data, a.size, None if row is None else row.ctypes.data,
                0 if row is None else R, b, e, ml, sd)
        widest = ctypes.c_size_t()
        Wn = self._check_batch(lib.shred_window_rows(*args, 0, pid, ps, None, 0, None, None, None, None, None,
                                                     ctypes.byref(widest)))
        W = widest.value if width is None else int(width)
        if W < widest.value:
            raise ValueError(f"width {W} is smaller than the longest window ({widest.value} ids)")
        out = np.empty(max(1, Wn * W), dtype=np.int32)
        lengths, wrow = (np.empty(max(1, Wn), dtype=np.int32) for _ in range(2))
        wsrc = np.empty(max(1, Wn), dtype=np.int64)
        roww = np.empty(R + 1, dtype=np.int64)
        m = np.empty(max(1, Wn * W), dtype=np.uint8) if mask else None
        self._check_batch(lib.shred_window_rows(*args, W, pid, ps, out.ctypes.data, Wn * W, lengths.ctypes.data,
                                                None if m is None else m.ctypes.data, wrow.ctypes.data,
                                                wsrc.ctypes.data, roww.ctypes.data, None))
        res = (out[:Wn * W].reshape(Wn, W), lengths[:Wn], wrow[:Wn], wsrc[:Wn], roww)
        return res + ((m[:Wn * W].reshape(Wn, W),) if mask else ())

    def window_device(self, ids, row_offsets=None, *, max_len, stride=0, bos=None, eos=None, pad_id=0, pad="right",
                      width=None, mask=False, stream=None):
        """window_rows on device tensors (as pad_device takes them) -> (batch, lengths, window_rows,
        window_src, row_windows[, mask], device milliseconds of the window passes)."""
        import torch
        b, e, ml, sd, pid, ps = self._window_args(bos, eos, max_len, stride, pad_id, pad)
        R = self._device_rows(ids, row_offsets)
        st = self._stream(stream, ids.device)
        args = (self.enc, ids.data_ptr(), ids.numel(), None if row_offsets is None else row_offsets.data_ptr(),
                0 if row_offsets is None else R, b, e, ml, sd)
        widest, ms = ctypes.c_size_t(), ctypes.c_double()
        Wn = self._check_batch(lib.shred_window_device(*args, 0, pid, ps, None, 0, None, None, None, None, None,
                                                       ctypes.byref(widest), st, None))
        W = widest.value if width is None else int(width)
        if W < widest.value:
            raise ValueError(f"width {W} is smaller than the longest window ({widest.value} ids)")
        new = lambda dt, k: torch.empty(max(1, k), dtype=dt, device=ids.device)
        out, lengths, wrow = new(torch.int32, Wn * W), new(torch.int32, Wn), new(torch.int32, Wn)
        wsrc, roww = new(torch.int64, Wn), new(torch.int64, R + 1)
        m = new(torch.uint8, Wn * W) if mask else None
        self._check_batch(lib.shred_window_device(*args, W, pid, ps, out.data_ptr(), Wn * W, lengths.data_ptr(),
                                                  None if m is None else m.data_ptr(), wrow.data_ptr(),
                                                  wsrc.data_ptr(), roww.data_ptr(), None, st, ctypes.byref(ms)))
        res = (out[:Wn * W].view(Wn, W), lengths[:Wn], wrow[:Wn], wsrc[:Wn], roww)
        return res + ((m[:Wn * W].view(Wn, W),) if mask else ()) + (ms.value,)

    def _encode_rows(self, text, specials, doc_offsets):
        """(ids, row_offsets): documents when text is a list / tuple or doc_offsets is given, else lines."""
        if isinstance(text, (list, tuple)):
            if doc_offsets is not None:
                raise ValueError("doc_offsets goes with one text, not with a list of documents")
            return self.encode_batch(text, specials=specials)
        if doc_offsets is not None:
            return self.encode_docs(text, doc_offsets, specials=specials)
        return self.encode_lines(text, specials)

    def encode_padded(self, text, *, specials: bool = False, doc_offsets=None, **kw):
        """encode_lines, then pad_rows(**kw): one row of the batch per '\\n' line of the text.  With a
        list / tuple of documents (encode_batch) or with doc_offsets (encode_docs): one row per document."""
        ids, row = self._encode_rows(text, specials, doc_offsets)
        return self.pad_rows(ids, row, **kw)

    def encode_packed(self, text, *, specials: bool = False, doc_offsets=None, **kw):
        """encode_lines, then pack_rows(**kw): every '\\n' line of the text is one row of the stream.  With
        a list / tuple of documents (encode_batch) or with doc_offsets (encode_docs): every document is."""
        ids, row = self._encode_rows(text, specials, doc_offsets)
        return self.pack_rows(ids, row, **kw)

    def encode_windows(self, text, *, specials: bool = False, doc_offsets=None, **kw):
        """encode_lines, then window_rows(**kw): every '\\n' line of the text is cut into windows.  With
        a list / tuple of documents (encode_batch) or with doc_offsets (encode_docs): every document is."""
        ids, row = self._encode_rows(text, specials, doc_offsets)
        return self.window_rows(ids, row, **kw)

    # ---- row pairs to one model input (include/shredword_encode.h, shred_pair_*) -------------------

    @classmethod
    def _pair_args(cls, max_len, truncation, stride, max_first, bos, sep, eos, truncate, pad_id, pad):
        """-> (bos, mid, mid_n, eos, max_len, trunc_side, strategy, max_a, stride) as the C ABI takes them, then
        (pad_id, pad_side)."""
        if pad not in ("left", "right"):
            raise ValueError('pad must be "left" or "right"')
        if truncate not in ("left", "right"):
            raise ValueError('truncate must be "left" or "right"')
        if truncation not in PAIR_TRUNCATION:
            raise ValueError(f"truncation must be one of {PAIR_TRUNCATION}")
        sep = (sep,) if isinstance(sep, (int, np.integer)) else tuple(sep)
        if len(sep) > 2:
            raise ValueError("sep holds at most two ids")
        add = (bos is not None) + len(sep) + (eos is not None)
        ml = 0 if max_len is None else int(max_len)
        if ml < 0 or (ml and ml < add):
            raise ValueError(f"max_len must leave room for the {add} added ids")
        sd, mf = int(stride), 0 if max_first is None else int(max_first)
        if sd < 0 or mf < 0:
            raise ValueError("stride and max_first must not be negative")
        if truncation == "window_second":
            if not 0 < ml < 2 ** 31:
                raise ValueError("window_second needs a max_len, and one that fits an int32")
            if mf and ml - add - mf < sd + 1:
                raise ValueError(f"max_len - {add} - max_first must be at least stride + 1: a window must move on by "
                                 "at least one id")
        elif sd or mf:
            raise ValueError("stride and max_first go with truncation=\"window_second\"")
        ptr = lambda name, v: None if v is None else ctypes.byref(ctypes.c_int32(cls._int32(name, v)))
        mid = (ctypes.c_int32 * 2)(*[cls._int32("sep", v) for v in sep]) if sep else None
        return (ptr("bos", bos), mid, len(sep), ptr("eos", eos), ml, int(truncate == "left"),
                PAIR_TRUNCATION.index(truncation), mf, sd), (cls._int32("pad_id", pad_id), int(pad == "left"))

    @classmethod
    def _check_pair(cls, r: int) -> int:
        if r == -7:
            raise ValueError("a pair cannot be made to fit max_len by this truncation (the segment that is never cut "
                             "is too long)")
        if r == -6:
            raise ValueError("row offsets must be 0 = row[0] <= ... <= row[rows] = len(ids), for both segments")
        return cls._check_batch(r)

    def pair_rows(self, ids_a, row_a, ids_b, row_b, *, max_len=None, truncation="longest_first", stride=0,
                  max_first=None, bos=None, sep=(), eos=None, truncate="right", pad_id=0, pad="right", width=None,
                  mask=False, types=True):
        """-> (batch, lengths, pair_rows, seg_len, seg_src, row_windows[, types][, mask]): example r is the pair of
        ids_a[row_a[r]:row_a[r + 1]] and ids_b[row_b[r]:row_b[r + 1]] (both offset arrays in the line_offsets
        format, rows + 1 entries each), emitted as [bos] + kept_a + sep + kept_b + [eos] (sep: up to two ids).
        max_len (None: no limit) bounds an emitted row, the added ids included.  truncation: "longest_first"
        removes ids from the longer segment (from the second on a tie) until the pair fits; "only_first" /
        "only_second" cut that segment alone (ValueError when the other is too long on its own);
        "window_second" keeps the first segment (its first max_first ids, None: all) in every emitted row and
        cuts the second into windows that overlap by `stride` ids, as window_rows does (the question-answering
        form).  truncate: the side of a cut segment that is dropped.
        batch: int32 [emitted, width] (width None: the longest emitted row), padded with pad_id on the `pad`
        side; lengths: int32 [emitted]; pair_rows: int32 [emitted], the example of each emitted row; seg_len:
        int32 [emitted, 2], (ka, kb); seg_src: int64 [emitted, 2], the index in ids_a / ids_b of the first kept
        id of each segment (the same index into the starts of encode_docs is that token's byte offset);
        row_windows: int64 [rows + 1], example r owns the emitted rows [row_windows[r], row_windows[r + 1]);
        types: uint8 [emitted, width], 1 on kept_b and eos; mask: uint8 [emitted, width], 1 on tokens.
        Built on the GPU."""
        head, (pid, ps) = self._pair_args(max_len, truncation, stride, max_first, bos, sep, eos, truncate, pad_id, pad)
        if row_a is None or row_b is None:
            raise ValueError("row_a and row_b must hold rows + 1 entries")
        a, ra, R = self._host_rows(ids_a, row_a)
        b, rb, Rb = self._host_rows(ids_b, row_b)
        if R != Rb:
            raise ValueError("row_a and row_b must hold the same number of rows")
        args = (self.enc, a.ctypes.data, a.size, ra.ctypes.data, b.ctypes.data, b.size, rb.ctypes.data, R) + head
        widest = ctypes.c_size_t()
        Wn = self._check_pair(lib.shred_pair_rows(*args, 0, pid, ps, None, 0, None, None, None, None, None, None, None,
                                                  ctypes.byref(widest)))
        W = widest.value if width is None else int(width)
        if W < widest.value:
            raise ValueError(f"width {W} is smaller than the longest emitted row ({widest.value} ids)")
        out = np.empty(max(1, Wn * W), dtype=np.int32)
        lengths, wrow = (np.empty(max(1, Wn), dtype=np.int32) for _ in range(2))
        slen = np.empty(max(1, 2 * Wn), dtype=np.int32)
        ssrc = np.empty(max(1, 2 * Wn), dtype=np.int64)
        roww = np.empty(R + 1, dtype=np.int64)
        t = np.empty(max(1, Wn * W), dtype=np.uint8) if types else None
        m = np.empty(max(1, Wn * W), dtype=np.uint8) if mask else None
        self._check_pair(lib.shred_pair_rows(*args, W, pid, ps, out.ctypes.data, Wn * W,
                                             None if t is None else t.ctypes.data, None if m is None else m.ctypes.data,
                                             lengths.ctypes.data, wrow.ctypes.data, slen.ctypes.data, ssrc.ctypes.data,
                                             roww.ctypes.data, None))
        res = (out[:Wn * W].reshape(Wn, W), lengths[:Wn], wrow[:Wn], slen[:2 * Wn].reshape(Wn, 2),
               ssrc[:2 * Wn].reshape(Wn, 2), roww)
        res += (t[:Wn * W].reshape(Wn, W),) if types else ()
        return res + ((m[:Wn * W].reshape(Wn, W),) if mask else ())

    def pair_device(self, ids_a, row_a, ids_b, row_b, *, max_len=None, truncation="longest_first", stride=0,
                    max_first=None, bos=None, sep=(), eos=None, truncate="right", pad_id=0, pad="right", width=None,
                    mask=False, types=True, stream=None):
        """pair_rows on device tensors (ids 1-D int32, offsets 1-D int64, on the encoder's GPU) -> (batch, lengths,
        pair_rows, seg_len, seg_src, row_windows[, types][, mask], device milliseconds of the pair passes)."""
        import torch
        head, (pid, ps) = self._pair_args(max_len, truncation, stride, max_first, bos, sep, eos, truncate, pad_id, pad)
        if row_a is None or row_b is None:
            raise ValueError("row_a and row_b must hold rows + 1 entries")
        R = self._device_rows(ids_a, row_a)
        if R != self._device_rows(ids_b, row_b):
            raise ValueError("row_a and row_b must hold the same number of rows")
        st = self._stream(stream, ids_a.device)
        args = (self.enc, ids_a.data_ptr(), ids_a.numel(), row_a.data_ptr(), ids_b.data_ptr(), ids_b.numel(),
                row_b.data_ptr(), R) + head
        widest, ms = ctypes.c_size_t(), ctypes.c_double()
        Wn = self._check_pair(lib.shred_pair_device(*args, 0, pid, ps, None, 0, None, None, None, None, None, None,
                                                    None, ctypes.byref(widest), st, None))
        W = widest.value if width is None else int(width)
        if W < widest.value:
            raise ValueError(f"width {W} is smaller than the longest emitted row ({widest.value} ids)")
        new = lambda dt, k: torch.empty(max(1, k), dtype=dt, device=ids_a.device)
        out, lengths, wrow = new(torch.int32, Wn * W), new(torch.int32, Wn), new(torch.int32, Wn)
        slen, ssrc, roww = new(torch.int32, 2 * Wn), new(torch.int64, 2 * Wn), new(torch.int64, R + 1)
        t = new(torch.uint8, Wn * W) if types else None
        m = new(torch.uint8, Wn * W) if mask else None
        self._check_pair(lib.shred_pair_device(*args, W, pid, ps, out.data_ptr(), Wn * W,
                                               None if t is None else t.data_ptr(), None if m is None else m.data_ptr(),
                                               lengths.data_ptr(), wrow.data_ptr(), slen.data_ptr(), ssrc.data_ptr(),
                                               roww.data_ptr(), None, st, ctypes.byref(ms)))
        res = (out[:Wn * W].view(Wn, W), lengths[:Wn], wrow[:Wn], slen[:2 * Wn].view(Wn, 2), ssrc[:2 * Wn].view(Wn, 2),
               roww)
        res += (t[:Wn * W].view(Wn, W),) if types else ()
        return res + ((m[:Wn * W].view(Wn, W),) if mask else ()) + (ms.value,)

    def encode_pairs(self, texts_a, texts_b, *, starts: bool = False, specials: bool = False, **kw):
        """Two equally long sequences of bytes / str documents -> pair_device(**kw) of their ids: both lists are
        encoded on the GPU as encode_docs_device encodes them (one row per document) and the ids stay there.
        Returns pair_device's tuple (torch tensors on the encoder's device, then the device milliseconds); with
        starts=True two more int64 tensors follow, the byte offset of every token of texts_a in the joined texts_a
        (join_docs) and the same for texts_b: seg_src indexes them."""
        import torch
        if len(texts_a) != len(texts_b):
            raise ValueError("texts_a and texts_b must hold the same number of documents")
        sides = []
        for texts in (texts_a, texts_b):
            buf, off = join_docs(texts)
            d_buf = torch.from_numpy(buf.copy()).cuda(self.device)
            ids, row, st, _ = self.encode_docs_device(d_buf, torch.from_numpy(off).cuda(self.device), starts=starts,
                                                      specials=specials)
            sides.append((ids, row, st))
        (ia, ra, sa), (ib, rb, sb) = sides
        res = self.pair_device(ia, ra, ib, rb, **kw)
        return res + ((sa, sb) if starts else ())

    # ---- masked-LM inputs (include/shredword_encode.h, shred_mlm_*) ---------------------------------

    def _mlm_opts(self, mask_id, p, seed, mask_prob, random_prob, random_vocab, protect, protect_specials, whole_word,
                  ignore_id, index_base):
        """-> (ShredMlmOpts as the C ABI takes it, the array its protect pointer keeps alive)."""
        p, pm, pr = float(p), float(mask_prob), float(random_prob)
        for name, q in (("p", p), ("mask_prob", pm), ("random_prob", pr)):
            if not 0.0 <= q <= 1.0:
                raise ValueError(f"{name} must be a probability in [0, 1]")
        if int(pm * 4294967296.0) + int(pr * 4294967296.0) > 2 ** 32:
            raise ValueError("mask_prob + random_prob must be at most 1")
        rv = 256 + self.num_merges if random_vocab is None else int(random_vocab)
        if pr > 0 and not 1 <= rv < 2 ** 31:
            raise ValueError("random_vocab must be in [1, INT32_MAX] when random_prob > 0")
        prot = np.array([self._int32("protect", v) for v in protect], dtype=np.int32)
        if prot.size > MLM_MAX_PROTECT:
            raise ValueError(f"protect holds at most {MLM_MAX_PROTECT} ids")
        base = int(index_base)
        if not 0 <= base < 2 ** 64:
            raise ValueError("index_base must fit a uint64")
        opts = ShredMlmOpts(base, p, int(seed) & (2 ** 64 - 1), pm, pr, self._int32("mask_id", mask_id),
                            self._int32("ignore_id", ignore_id), rv if pr > 0 else 0,
                            prot.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if prot.size else None, prot.size,
                            int(bool(protect_specials)), int(bool(whole_word)))
        return opts, prot

    def _check_mlm(self, r: int) -> int:
        if r == -4:
            raise ValueError("the byte map holds an id >= 256: token lengths are undefined")
        return self._check_batch(r)

    def mlm_rows(self, ids, row_offsets=None, *, mask_id, p=0.15, seed=0, mask_prob=0.8, random_prob=0.1,
                 random_vocab=None, protect=(), protect_specials=True, whole_word=False, starts=None, ignore_id=-100,
                 index_base=0):
        """-> (masked_ids, labels, selected): masked-language-model inputs of the rows
        ids[row_offsets[r]:row_offsets[r + 1]] (None: one row), before pad / pack / window / pair.  Every
        token is selected with probability p; of the selected, the share mask_prob becomes mask_id, the
        share random_prob a uniform id in [0, random_vocab) (None: 256 + num_merges) and the rest keep
        their id; labels holds the original id of a selected token and ignore_id elsewhere.  protect: up
        to 16 ids that are never selected; protect_specials: nor are the registered special tokens.
        whole_word: the tokens of a word are selected together (starts: the byte offsets encode_spans /
        encode_docs return for the ids; a row's first token, a special and a protected id begin a word).
        A decision is a function of (seed, index_base + the token's index) alone: the same arguments
        always give the same result, on host and device calls alike, and a new seed (one per epoch, say)
        a new masking.  Pad the labels with pad_id = bos = eos = ignore_id.  Built on the GPU."""
        opts, _keep = self._mlm_opts(mask_id, p, seed, mask_prob, random_prob, random_vocab, protect,
                                     protect_specials, whole_word, ignore_id, index_base)
        a, row, R = self._host_rows(ids, row_offsets)
        st = None
        if whole_word:
            if starts is None:
                raise ValueError("whole_word needs starts, one byte offset per id")
            st = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
            if st.size != a.size:
                raise ValueError("whole_word needs starts, one byte offset per id")
        out, labels = np.empty(max(1, a.size), dtype=np.int32), np.empty(max(1, a.size), dtype=np.int32)
        r = self._check_mlm(lib.shred_mlm_rows(self.enc, a.ctypes.data, a.size, None if row is None else row.ctypes.data,
                                               0 if row is None else R, ctypes.byref(opts),
                                               None if st is None else st.ctypes.data, out.ctypes.data,
                                               labels.ctypes.data))
        return out[:a.size], labels[:a.size], r

    def mlm_device(self, ids, row_offsets=None, *, mask_id, p=0.15, seed=0, mask_prob=0.8, random_prob=0.1,
                   random_vocab=None, protect=(), protect_specials=True, whole_word=False, starts=None, ignore_id=-100,
                   index_base=0, out=None, stream=None):
        """mlm_rows on device tensors (ids 1-D int32, row_offsets and starts 1-D int64, on the encoder's GPU;
        views that are only element-aligned fit) -> (masked_ids, labels, selected, device milliseconds of the
        masking passes).  out: None, or an int32 tensor for the masked ids; out=ids masks in place."""
        import torch
        opts, _keep = self._mlm_opts(mask_id, p, seed, mask_prob, random_prob, random_vocab, protect,
                                     protect_specials, whole_word, ignore_id, index_base)
        R = self._device_rows(ids, row_offsets)
        n = ids.numel()
        for name, t, dt in (("starts", starts if whole_word else None, torch.int64), ("out", out, torch.int32)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or not t.is_cuda \
                    or not t.is_contiguous() or t.device != ids.device or t.numel() != n:
                raise ValueError(f"{name} must be a contiguous 1-D {dt} tensor of len(ids) entries on the ids' device")
        if whole_word and starts is None:
            raise ValueError("whole_word needs starts, one byte offset per id")
        if out is None:
            out = torch.empty(max(1, n), dtype=torch.int32, device=ids.device)[:n]
        labels = torch.empty(max(1, n), dtype=torch.int32, device=ids.device)[:n]
        ms = ctypes.c_double()
        st = self._stream(stream, ids.device)
        r = self._check_mlm(lib.shred_mlm_device(
            self.enc, ids.data_ptr(), n, None if row_offsets is None else row_offsets.data_ptr(),
            0 if row_offsets is None else R, ctypes.byref(opts), starts.data_ptr() if whole_word else None,
            out.data_ptr(), labels.data_ptr(), st, ctypes.byref(ms)))
        return out, labels, r, ms.value

    def encode_mlm(self, text, *, mask_id, p=0.15, seed=0, mask_prob=0.8, random_prob=0.1, random_vocab=None,
                   protect=(), protect_specials=True, whole_word=False, ignore_id=-100, index_base=0,
                   doc_offsets=None, specials: bool = False, **pad_kw):
        """Text to masked-LM model inputs on the GPU: encode_docs_device (one row per document of a list /
        tuple, or per doc_offsets entry of one text; None: one document), mlm_device, then pad_device twice
        with **pad_kw (bos, eos, max_len, truncate, pad_id, pad, width): the masked ids with the caller's
        bos / eos / pad_id, the labels with ignore_id in their place.  -> (batch, labels, lengths,
        attention_mask, selected): int32 [rows, width] twice, int32 [rows], uint8 [rows, width] tensors on
        the encoder's device, and the number of selected tokens (before any truncation)."""
        import torch
        if isinstance(text, (list, tuple)):
            if doc_offsets is not None:
                raise ValueError("doc_offsets goes with one text, not with a list of documents")
            buf, off = join_docs(text)
        else:
            buf = self._host_text(text)
            off = None if doc_offsets is None else np.ascontiguousarray(doc_offsets, dtype=np.int64).reshape(-1)
        pad_kw.pop("mask", None)
        d_buf = torch.from_numpy(np.array(buf)).cuda(self.device)
        d_off = None if off is None else torch.from_numpy(np.array(off)).cuda(self.device)
        ids, row, st, _ = self.encode_docs_device(d_buf, d_off, starts=whole_word, specials=specials)
        masked, labels, selected, _ = self.mlm_device(
            ids, row, mask_id=mask_id, p=p, seed=seed, mask_prob=mask_prob, random_prob=random_prob,
            random_vocab=random_vocab, protect=protect, protect_specials=protect_specials, whole_word=whole_word,
            starts=st, ignore_id=ignore_id, index_base=index_base)
        batch, lengths, attn, _ = self.pad_device(masked, row, mask=True, **pad_kw)
        lab_kw = dict(pad_kw, pad_id=ignore_id, width=batch.shape[1])
        for k in ("bos", "eos"):
            if lab_kw.get(k) is not None:
                lab_kw[k] = ignore_id
        lab_batch = self.pad_device(labels, row, **lab_kw)[0]
        return batch, lab_batch, lengths, attn, selected

    # ---- span-corruption inputs and targets (include/shredword_encode.h, shred_corrupt_*) -----------

    @staticmethod
    def corrupt_lengths(lengths=(1, 5), length_probs=None):
        """-> (len_cum, mean): the C ABI's C_1 .. C_m (Python ints, C_i = 2^32 * P(L <= i), C_m = 2^32) and the
        mean span length.  lengths=(lo, hi): uniform on lo .. hi (C_i = 0 below lo, then equal steps);
        length_probs: P(L = 1), .., P(L = m) directly."""
        if length_probs is not None:
            probs = [float(q) for q in length_probs]
            if not 1 <= len(probs) <= CORRUPT_MAX_SPAN or any(not 0.0 <= q <= 1.0 for q in probs):
                raise ValueError(f"length_probs holds 1 to {CORRUPT_MAX_SPAN} probabilities")
            cum = [min(int(sum(probs[:i]) * 4294967296.0), 2 ** 32) for i in range(1, len(probs) + 1)]
            cum[-1] = 2 ** 32
            if any(a > b for a, b in zip(cum, cum[1:])):
                raise ValueError("length_probs must sum to 1")
            total = sum(probs)
            return cum, sum((i + 1) * q for i, q in enumerate(probs)) / (total if total > 0 else 1.0)
        lo, hi = (int(v) for v in lengths)
        if not 1 <= lo <= hi <= CORRUPT_MAX_SPAN:
            raise ValueError(f"lengths must be (lo, hi) with 1 <= lo <= hi <= {CORRUPT_MAX_SPAN}")
        k = hi - lo + 1
        return [0 if i < lo else ((i - lo + 1) * 2 ** 32) // k for i in range(1, hi + 1)], (lo + hi) / 2.0

    def _corrupt_opts(self, sentinel_first, sentinel_step, sentinels, p_start, noise_density, lengths, length_probs,
                      seed, final_sentinel, protect, protect_specials, index_base):
        """-> (ShredCorruptOpts as the C ABI takes it, the arrays its pointers keep alive)."""
        import math
        cum, mean = self.corrupt_lengths(lengths, length_probs)
        if p_start is None:
            nd = float(noise_density)
            if not 0.0 <= nd < 1.0:
                raise ValueError("noise_density must be in [0, 1)")
            p_start = min(1.0, -math.log(1.0 - nd) / mean)
        p_start = float(p_start)
        if not 0.0 <= p_start <= 1.0:
            raise ValueError("p_start must be a probability in [0, 1]")
        first, step, sn = self._int32("sentinel_first", sentinel_first), self._int32("sentinel_step", sentinel_step), \
            int(sentinels)
        if not 0 <= sn < 2 ** 31:
            raise ValueError("sentinels must be in [0, INT32_MAX]")
        if sn:
            self._int32("the last sentinel", first + (sn - 1) * step)
        prot = np.array([self._int32("protect", v) for v in protect], dtype=np.int32)
        if prot.size > MLM_MAX_PROTECT:
            raise ValueError(f"protect holds at most {MLM_MAX_PROTECT} ids")
        base = int(index_base)
        if not 0 <= base < 2 ** 64:
            raise ValueError("index_base must fit a uint64")
        c_cum = (ctypes.c_uint64 * len(cum))(*cum)
        opts = ShredCorruptOpts(base, int(seed) & (2 ** 64 - 1), p_start, c_cum, len(cum), first, step, sn,
                                int(bool(final_sentinel)),
                                prot.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if prot.size else None, prot.size,
                                int(bool(protect_specials)))
        return opts, (c_cum, prot)

    def corrupt_rows(self, ids, row_offsets=None, *, sentinel_first, sentinel_step=-1, sentinels=100, p_start=None,
                     noise_density=0.15, lengths=(1, 5), length_probs=None, seed=0, final_sentinel=True, protect=(),
                     protect_specials=True, index_base=0, src=False):
        """-> (in_ids, in_row_offsets, tgt_ids, tgt_row_offsets[, in_src]): span-corruption (T5 / UL2
        denoising) inputs and targets of the rows ids[row_offsets[r]:row_offsets[r + 1]] (None: one row),
        both as flat streams with their own offsets, so pad / pack / window / decode take them unchanged.
        Every position starts a span with probability p_start; a span's length is drawn from `lengths`
        (lo, hi: uniform) or from length_probs (P(L = 1), ..); spans end with their row, and overlapping or
        touching spans make one run.  In the input every run becomes one sentinel (sentinel j is
        sentinel_first + j * sentinel_step; T5: V - 1 downwards); the target holds each sentinel and then
        its run, and with final_sentinel the row's next unused sentinel at the end.  Runs beyond the
        available sentinels are kept.  protect: up to 16 ids that are never noise (they split a span);
        protect_specials: nor are the registered special tokens.  src: also in_src, int64 per input id, the
        index in ids of a kept token or of a run's first token.
        p_start None: -ln(1 - noise_density) / mean length, a first-order choice: the exact expected noise
        share without protection is 1 - prod_{i >= 0} (1 - p_start * P(L > i)), 0.1528 for the defaults.
        A decision is a function of (seed, index_base + the token's index) alone.  Built on the GPU."""
        opts, _keep = self._corrupt_opts(sentinel_first, sentinel_step, sentinels, p_start, noise_density, lengths,
                                         length_probs, seed, final_sentinel, protect, protect_specials, index_base)
        a, row, R = self._host_rows(ids, row_offsets)
        n = a.size
        in_ids, tgt_ids = np.empty(max(1, n), dtype=np.int32), np.empty(2 * n + R, dtype=np.int32)
        in_row, tgt_row = np.empty(R + 1, dtype=np.int64), np.empty(R + 1, dtype=np.int64)
        in_src = np.empty(max(1, n), dtype=np.int64) if src else None
        t_tgt = ctypes.c_size_t()
        t_in = self._check_batch(lib.shred_corrupt_rows(
            self.enc, a.ctypes.data, n, None if row is None else row.ctypes.data, 0 if row is None else R,
            ctypes.byref(opts), in_ids.ctypes.data, n, in_row.ctypes.data, None if in_src is None else in_src.ctypes.data,
            tgt_ids.ctypes.data, tgt_ids.size, tgt_row.ctypes.data, ctypes.byref(t_tgt)))
        res = (in_ids[:t_in], in_row, tgt_ids[:t_tgt.value], tgt_row)
        return res + ((in_src[:t_in],) if src else ())

    def corrupt_device(self, ids, row_offsets=None, *, sentinel_first, sentinel_step=-1, sentinels=100, p_start=None,
                       noise_density=0.15, lengths=(1, 5), length_probs=None, seed=0, final_sentinel=True, protect=(),
                       protect_specials=True, index_base=0, src=False, stream=None):
        """corrupt_rows on device tensors (ids 1-D int32, row_offsets 1-D int64, on the encoder's GPU; views
        that are only element-aligned fit) -> (in_ids, in_row_offsets, tgt_ids, tgt_row_offsets[, in_src],
        device milliseconds of the corruption passes).  The streams are views of tensors sized for the
        bound (len(ids) and 2 len(ids) + rows), so the call runs once."""
        import torch
        opts, _keep = self._corrupt_opts(sentinel_first, sentinel_step, sentinels, p_start, noise_density, lengths,
                                         length_probs, seed, final_sentinel, protect, protect_specials, index_base)
        R = self._device_rows(ids, row_offsets)
        n = ids.numel()
        new = lambda dt, k: torch.empty(max(1, k), dtype=dt, device=ids.device)
        in_ids, tgt_ids = new(torch.int32, n), new(torch.int32, 2 * n + R)
        in_row, tgt_row = new(torch.int64, R + 1), new(torch.int64, R + 1)
        in_src = new(torch.int64, n) if src else None
        t_tgt, ms = ctypes.c_size_t(), ctypes.c_double()
        st = self._stream(stream, ids.device)
        t_in = self._check_batch(lib.shred_corrupt_device(
            self.enc, ids.data_ptr(), n, None if row_offsets is None else row_offsets.data_ptr(),
            0 if row_offsets is None else R, ctypes.byref(opts), in_ids.data_ptr(), n, in_row.data_ptr(),
            None if in_src is None else in_src.data_ptr(), tgt_ids.data_ptr(), 2 * n + R, tgt_row.data_ptr(),
            ctypes.byref(t_tgt), st, ctypes.byref(ms)))
        res = (in_ids[:t_in], in_row, tgt_ids[:t_tgt.value], tgt_row)
        return res + ((in_src[:t_in],) if src else ()) + (ms.value,)

    def encode_corrupted(self, text, *, specials: bool = False, doc_offsets=None, **kw):
        """encode_lines, then corrupt_device(**kw) on the encoder's GPU: every '\\n' line of the text is one row.
        With a list / tuple of documents (encode_batch) or with doc_offsets (encode_docs): every document is.
        -> corrupt_device's tuple."""
        import torch
        ids, row = self._encode_rows(text, specials, doc_offsets)[:2]
        d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).cuda(self.device)
        d_row = torch.from_numpy(np.ascontiguousarray(row, dtype=np.int64)).cuda(self.device)
        return self.corrupt_device(d_ids, d_row, **kw)

    # ---- fill-in-the-middle rows (include/shredword_encode.h, shred_fim_*) ---------------------------

    def _fim_opts(self, pre_id, suf_id, mid_id, fim_rate, spm_rate, seed, min_len, row_base):
        """-> ShredFimOpts as the C ABI takes it."""
        fr, sr = float(fim_rate), float(spm_rate)
        for name, q in (("fim_rate", fr), ("spm_rate", sr)):
            if not 0.0 <= q <= 1.0:
                raise ValueError(f"{name} must be a probability in [0, 1]")
        ml, base = int(min_len), int(row_base)
        if not 0 <= ml < 2 ** 63:
            raise ValueError("min_len must be in [0, INT64_MAX]")
        if not 0 <= base < 2 ** 64:
            raise ValueError("row_base must fit a uint64")
        return ShredFimOpts(base, int(seed) & (2 ** 64 - 1), fr, sr, ml, self._int32("pre_id", pre_id),
                            self._int32("suf_id", suf_id), self._int32("mid_id", mid_id))

    @staticmethod
    def _check_fim(r: int) -> int:
        if r == -8:
            raise ValueError("cuts must hold, per row, -1 -1 -1 or 0 <= a <= b <= len(row) and a mode of 0 or 1")
        return BPEEncoder._check_batch(r)

    def fim_rows(self, ids, row_offsets=None, *, pre_id, suf_id, mid_id, fim_rate=0.5, spm_rate=0.5, seed=0,
                 min_len=0, row_base=0, cuts=None, src=False, seg=False, info=False):
        """-> (out_ids, out_row_offsets[, out_src][, out_seg][, row_info]): fill-in-the-middle rows of the rows
        ids[row_offsets[r]:row_offsets[r + 1]] (None: one row), a flat stream with its own offsets, so pad /
        pack / window / decode take it unchanged.  A row of at least min_len ids is transformed with
        probability fim_rate: cut at two uniform points into prefix, middle and suffix and re-emitted as
        pre_id prefix suf_id suffix mid_id middle (PSM), or with probability spm_rate as pre_id suf_id suffix
        mid_id prefix middle (SPM).  Other rows are copied.  cuts: None, or [rows, 3] int64 (a, b, mode) per
        row, -1 -1 -1 for a row to copy: the rows are assembled by it and nothing is drawn.  src: also
        out_src, int64 per output id, the index in ids of the token or -1 for a sentinel.  seg: also out_seg,
        uint8 per output id: 0 row not transformed, 1 prefix, 2 suffix, 3 middle, 4 sentinel.  info: also
        row_info, [rows, 3] int64 in the format of cuts, what was drawn or given.
        A decision is a function of (seed, row_base + the row's index, the row's length) alone.  Built on
        the GPU."""
        opts = self._fim_opts(pre_id, suf_id, mid_id, fim_rate, spm_rate, seed, min_len, row_base)
        a, row, R = self._host_rows(ids, row_offsets)
        n = a.size
        c = None
        if cuts is not None:
            c = np.ascontiguousarray(cuts, dtype=np.int64).reshape(-1)
            if c.size != 3 * R:
                raise ValueError("cuts must hold 3 entries per row")
        cap = n + 3 * R
        out, out_row = np.empty(cap, dtype=np.int32), np.empty(R + 1, dtype=np.int64)
        o_src = np.empty(cap, dtype=np.int64) if src else None
        o_seg = np.empty(cap, dtype=np.uint8) if seg else None
        o_info = np.empty((R, 3), dtype=np.int64) if info else None
        ptr = lambda x: None if x is None else x.ctypes.data
        t = self._check_fim(lib.shred_fim_rows(
            self.enc, a.ctypes.data, n, ptr(row), 0 if row is None else R, ctypes.byref(opts), ptr(c), out.ctypes.data,
            cap, out_row.ctypes.data, ptr(o_src), ptr(o_seg), ptr(o_info)))
        return (out[:t], out_row) + ((o_src[:t],) if src else ()) + ((o_seg[:t],) if seg else ()) \
            + ((o_info,) if info else ())

    def fim_device(self, ids, row_offsets=None, *, pre_id, suf_id, mid_id, fim_rate=0.5, spm_rate=0.5, seed=0,
                   min_len=0, row_base=0, cuts=None, src=False, seg=False, info=False, stream=None):
        """fim_rows on device tensors (ids 1-D int32, row_offsets 1-D int64, cuts [rows, 3] int64, on the
        encoder's GPU; views that are only element-aligned fit) -> (out_ids, out_row_offsets[, out_src]
        [, out_seg][, row_info], device milliseconds of the FIM passes).  The stream is a view of a tensor
        sized for the bound (len(ids) + 3 rows), so the call runs once."""
        import torch
        opts = self._fim_opts(pre_id, suf_id, mid_id, fim_rate, spm_rate, seed, min_len, row_base)
        R = self._device_rows(ids, row_offsets)
        n = ids.numel()
        if cuts is not None:
            if not isinstance(cuts, torch.Tensor) or cuts.dtype != torch.int64 or not cuts.is_cuda \
                    or not cuts.is_contiguous() or cuts.device != ids.device or cuts.numel() != 3 * R:
                raise ValueError("cuts must be a contiguous int64 tensor of 3 entries per row on the ids' device")
        cap = n + 3 * R
        new = lambda dt, k: torch.empty(k, dtype=dt, device=ids.device)
        out, out_row = new(torch.int32, cap), new(torch.int64, R + 1)
        o_src = new(torch.int64, cap) if src else None
        o_seg = new(torch.uint8, cap) if seg else None
        o_info = new(torch.int64, 3 * R).view(R, 3) if info else None
        ptr = lambda x: None if x is None else x.data_ptr()
        ms = ctypes.c_double()
        st = self._stream(stream, ids.device)
        t = self._check_fim(lib.shred_fim_device(
            self.enc, ids.data_ptr(), n, ptr(row_offsets), 0 if row_offsets is None else R, ctypes.byref(opts),
            ptr(cuts), out.data_ptr(), cap, out_row.data_ptr(), ptr(o_src), ptr(o_seg), ptr(o_info), st,
            ctypes.byref(ms)))
        return (out[:t], out_row) + ((o_src[:t],) if src else ()) + ((o_seg[:t],) if seg else ()) \
            + ((o_info,) if info else ()) + (ms.value,)

    def fim_cuts_device(self, text, doc_offsets=None, *, fim_rate=0.5, spm_rate=0.5, seed=0, min_len=0, row_base=0,
                        stream=None):
        """Character-level cuts of the documents text[doc_offsets[d]:doc_offsets[d + 1]] (device tensors as
        encode_docs_device takes them) -> (piece_offsets, doc_mode, device milliseconds): 3 docs + 1 int64
        offsets that cut every document into prefix, middle and suffix at UTF-8 character boundaries (a
        document that is not transformed into itself and two empty pieces), and int8 per document: -1 not
        transformed, 0 PSM, 1 SPM.  min_len is in bytes."""
        import torch
        opts = self._fim_opts(0, 0, 0, fim_rate, spm_rate, seed, min_len, row_base)
        for name, t, dt in (("text", text, torch.uint8), ("doc_offsets", doc_offsets, torch.int64)):
            if t is None and name != "text":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or not t.is_cuda \
                    or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous 1-D {dt} CUDA tensor")
            if t.device.index != self.device:
                raise ValueError(f"{name} is on {t.device}, the encoder on cuda:{self.device}")
        if doc_offsets is not None and doc_offsets.numel() == 0:
            raise ValueError("doc_offsets must hold docs + 1 entries")
        D = 1 if doc_offsets is None else doc_offsets.numel() - 1
        piece = torch.empty(3 * D + 1, dtype=torch.int64, device=text.device)
        mode = torch.empty(max(1, D), dtype=torch.int8, device=text.device)[:D]
        ms = ctypes.c_double()
        st = self._stream(stream, text.device)
        self._check_docs(lib.shred_fim_cuts_device(
            self.enc, text.data_ptr(), text.numel(), None if doc_offsets is None else doc_offsets.data_ptr(),
            0 if doc_offsets is None else D, ctypes.byref(opts), piece.data_ptr(), mode.data_ptr(), st,
            ctypes.byref(ms)))
        return piece, mode, ms.value

    def encode_fim(self, text, *, doc_offsets=None, specials: bool = False, level: str = "char", starts: bool = False,
                   **kw):
        """Text to fill-in-the-middle rows on the GPU -> fim_device's tuple, with starts=True the byte offset
        of every encoded token (int64, indexed by out_src) before the milliseconds.  **kw: fim_device's.
        level="token": the rows are encoded (lines, or documents with a list / tuple or doc_offsets, as
        encode_corrupted takes them) and fim_device cuts them between tokens.
        level="char" (documents only; one text without doc_offsets is one document): fim_cuts_device cuts
        the text of every document between characters, with min_len in bytes; encode_docs_device encodes
        every piece as if alone, so the model sees the broken tokens at the joins; fim_device assembles
        the rows by the pieces' lengths.  A cut that falls inside a special token's bytes leaves ordinary
        text on both sides: neither part is matched as that special."""
        import torch
        if level not in ("char", "token"):
            raise ValueError('level must be "char" or "token"')
        if isinstance(text, (list, tuple)):
            if doc_offsets is not None:
                raise ValueError("doc_offsets goes with one text, not with a list of documents")
            buf, off = join_docs(text)
        else:
            buf = self._host_text(text)
            off = None if doc_offsets is None else np.ascontiguousarray(doc_offsets, dtype=np.int64).reshape(-1)
        dev = lambda a: torch.from_numpy(np.array(a)).cuda(self.device)
        if level == "token":
            if off is None:
                ids, st, row = self._spans_host(buf, starts, True, specials)
            else:
                ids, row, *st = self.encode_docs(buf, off, starts=starts, specials=specials)
                st = st[0] if starts else None
            res = self.fim_device(dev(np.ascontiguousarray(ids, dtype=np.int32)),
                                  dev(np.ascontiguousarray(row, dtype=np.int64)), **kw)
            return res[:-1] + ((dev(st),) if starts else ()) + res[-1:]
        if "cuts" in kw:
            raise ValueError('level="char" draws the cuts itself')
        d_buf, d_off = dev(buf), None if off is None else dev(off)
        draw = {k: kw[k] for k in ("fim_rate", "spm_rate", "seed", "min_len", "row_base") if k in kw}
        piece, mode, _ = self.fim_cuts_device(d_buf, d_off, **draw)
        ids, row3, st, _ = self.encode_docs_device(d_buf, piece, starts=starts, specials=specials)
        first = row3[0:-1:3]
        m = mode.to(torch.int64)
        keep = m >= 0
        cuts = torch.stack([torch.where(keep, row3[1::3] - first, m), torch.where(keep, row3[2::3] - first, m), m],
                           dim=1).contiguous()
        res = self.fim_device(ids, row3[0::3].contiguous(), **dict(kw, min_len=0, cuts=cuts))
        return res[:-1] + ((st,) if starts else ()) + res[-1:]

    def destroy(self):
        if getattr(self, "enc", None):
            lib.shred_encoder_destroy(self.enc)
            self.enc = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
