"""Encoder timing on one corpus: python enc_bench.py prepare CORPUS BYTES DIR  (generate + train + save)
                                   python enc_bench.py run CORPUS DIR [reps] [spans | decode | batch | window | pair | special | docs | long | mlm | corrupt | fim] [--dropout P [--seed S]]   (SHREDWORD_LIB picks the build)
With --dropout P (anywhere on the line) the encoder is created with BPE-dropout (P, seed S, default 0): every
leg then runs the direct dropout kernels, and the first line also reports P, the seed and the ids per byte.
With a trailing `spans`, run also times encode_spans_device (token starts + line offsets); with a
trailing `decode`, decode_device on the corpus's ids and line offsets (median / min / max ms and
GB/s of output), and the host loop shred_decode on the same ids (wall time) for comparison; with a
trailing `batch`, the decode leg and then pad_device (rows cut to 1024 ids, with the mask) and
pack_device (an eos per row, sequences of 2048, positions and segments) on the corpus's ids and line
offsets: device ms and effective GB/s by the traffic model of batch_device.hip, and the torch
composition (torch.full, an index from repeat_interleave of the lengths, a scatter) on the same
tensors, timed with device events in the same process after a warm-up; with a trailing `window`,
window_device (max_len 1024, stride 128, with the mask) on the corpus's ids and line offsets: device ms
and effective GB/s by the traffic model of batch_device.hip, pad_device at the same width on the same
rows (rows cut to 1024 ids: the same output size when no line is longer than a window), and a torch
gather (an index of window starts plus columns, a masked take) on the same tensors; with a trailing `pair`,
pair_device (window_second, max_len 512, stride 128, bos, one sep, eos, with types and mask) on 65,536 seeded
examples of 8..32 and 200..1500 random ids (the corpus is not used): device ms and effective GB/s by the traffic
model of batch_pair.hip, checked against a torch gather of the same rows; with a trailing `special`,
"<|endoftext|>" is put in front of the first '\\n' after every 2048th byte of the corpus, and that
text is timed through encode_spans_device without and with specials=True (the encode, span and
special passes of one call each); with a trailing `docs`, the corpus is one document per line (doc_offsets
after every '\\n') and goes through encode_docs_device with starts, then, after a warm-up,
encode_spans_device(lines=True) on the same text, each also as a whole call between device events, and a
device-to-device copy of the text's bytes is timed beside the copy kernel of the document passes, whose
time the library prints under SHREDWORD_ENCODE_DEBUG (set here for the last calls: the corpus one document
per line, as one document and as 16 documents), and beside a copy of 1 GiB, which the cache does not hold; with
a trailing `long`, the long-word mode (long_words=True): encode_device on the corpus as it is (no long word: the
cost of the find pass, against the first line's time with the mode off), on the corpus with the delimiters of a
4 KB stretch taken out after every 64 KB (one long word per 64 KB), and on single words of 4 KB, 64 KB and 1 MB
cut from the corpus without its delimiters, with the rounds each word took; with a trailing `mlm`, mlm_device on
2^26 seeded ids of the vocabulary in rows of 200..500 (the corpus is not used), per token and per whole word (starts
from the token lengths, a delimiter before 30 % of the tokens), p = 0.15 with four protected ids: device ms (median of
7 after two warm-up calls) and GB/s by the traffic model of batch_mask.hip, beside the torch composition on the same
tensors in the same process (rand for selection and action, an isin protect mask, where for ids and labels; whole
words: begins from starts, a cumsum for the word of every token and one draw per word gathered back); with a trailing
`corrupt`, corrupt_device on the same ids and rows (default options: p_start from a noise density of 0.15, lengths 1..5,
100 sentinels, the closing one, four protected ids, with in_src): device ms (median of 7 after two warm-up calls) and GB/s
by the traffic model of batch_corrupt.hip, beside a torch composition of the same definition on the same tensors in the
same process (rand and randint for start and length, a difference array and a cumsum for the coverage with the reach cut
at the row's end by bucketize, run firsts, a cumsum for the rank within the row, cumsums of the two emit counts, masked
scatters for both streams, the offsets and the closing sentinels); with a trailing `fim`, fim_device on the same ids and
rows (fim_rate = spm_rate = 0.5, with out_src, out_seg and row_info): device ms (median of 7 after two warm-up calls) and
GB/s by the traffic model of batch_fim.hip, beside a torch composition of the same definition on the same tensors in the
same process (the per-row draws by the same hash in int64 arithmetic, a cumsum for the output offsets, bucketize for every
output position's row, where for its source index and one gather); the two results must be equal, or the leg fails."""
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def option(name, conv, default):
    """The value behind `name` on the command line, taken out of sys.argv."""
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    value = conv(sys.argv[i + 1])
    del sys.argv[i:i + 2]
    return value


dropout, seed = option("--dropout", float, 0.0), option("--seed", int, 0)
mode, corpus = sys.argv[1], sys.argv[2]
if mode == "prepare":
    nbytes, d = int(sys.argv[3]), sys.argv[4]
    os.makedirs(d, exist_ok=True)
    subprocess.run([os.path.join(HERE, "..", "bin", "gen_corpus"), "--bytes", str(nbytes), "--seed", "2",
                    "--script", "utf8", "--out", corpus], check=True)
    from shredword.trainer import BPETrainer
    t = BPETrainer(vocab_size=8192, min_pair_freq=2000)
    t.set_option("log", 0)
    t.load_corpus(corpus)
    t._train(t.trainer)
    t._save(t.trainer, os.path.join(d, "m.model").encode(), os.path.join(d, "m.vocab").encode())
    t.destroy()
else:
    args = sys.argv[3:]
    spans, batch = args[-1] == "spans", args[-1] == "batch"
    decode = batch or args[-1] == "decode"
    special, docs, window = args[-1] == "special", args[-1] == "docs", args[-1] == "window"
    long_leg, pair, corrupt, fim = args[-1] == "long", args[-1] == "pair", args[-1] == "corrupt", args[-1] == "fim"
    mlm = corrupt or fim or args[-1] == "mlm"  # the corrupt and fim legs run on the mlm leg's stream, in its place
    if spans or decode or special or docs or window or long_leg or pair or mlm:
        args = args[:-1]
    d = args[0]
    reps = int(args[1]) if len(args) > 1 else 5
    import torch
    from shredword.encoder import BPEEncoder
    enc = BPEEncoder(os.path.join(d, "m.model"), os.path.join(d, "m.vocab"), unk_id=0, dropout=dropout, seed=seed)
    text = torch.from_numpy(np.fromfile(corpus, dtype=np.uint8)).cuda()
    out = torch.empty(text.numel(), dtype=torch.int32, device="cuda")
    ids, _ = enc.encode_device(text, out)
    ms = sorted(enc.encode_device(text, out)[1] for _ in range(reps))
    print(os.environ.get("SHREDWORD_LIB", "default"), "ids", ids.numel(), "ms", ms[len(ms) // 2],
          "GB/s", text.numel() / ms[len(ms) // 2] / 1e6, "min", ms[0], "max", ms[-1],
          *(("dropout", dropout, "seed", seed, "ids/byte", ids.numel() / text.numel()) if dropout else ()), flush=True)
    if spans:
        del out
        enc.encode_spans_device(text)  # first call: allocates the span scratch
        runs = sorted((enc.encode_spans_device(text)[3] for _ in range(reps)), key=lambda t: t[1])
        encode_ms, spans_ms = sorted(t[0] for t in runs)[reps // 2], runs[reps // 2][1]
        print("spans: encode_ms", encode_ms, "spans_ms", spans_ms, "ratio", spans_ms / encode_ms,
              "spans min", runs[0][1], "max", runs[-1][1], flush=True)
    if special:
        del out
        tok = np.frombuffer(b"<|endoftext|>", dtype=np.uint8)
        host = text.cpu().numpy()
        nl = np.flatnonzero(host == 10)
        at = np.unique(nl[np.searchsorted(nl, np.arange(2048, host.size, 2048))[:-1]])
        text = torch.from_numpy(np.insert(host, np.repeat(at, tok.size), np.tile(tok, at.size))).cuda()
        enc.set_special_tokens([tok.tobytes()])
        med = lambda runs, i: sorted(t[i] for t in runs)[len(runs) // 2]
        enc.encode_spans_device(text)  # first calls: allocate the scratch
        plain = [enc.encode_spans_device(text)[3] for _ in range(reps)]
        ids = enc.encode_spans_device(text, specials=True)[0]
        found = int((ids == 256 + enc.num_merges).sum().item())
        assert found == at.size, (found, at.size)
        runs = [enc.encode_spans_device(text, specials=True)[3] for _ in range(reps)]
        print("special: bytes", text.numel(), "matches", found, "plain encode_ms", med(plain, 0), "spans_ms",
              med(plain, 1), "| specials=True encode_ms", med(runs, 0), "spans_ms", med(runs, 1), "special_ms",
              med(runs, 2), "min", min(t[2] for t in runs), "max", max(t[2] for t in runs), flush=True)
    if long_leg:
        reps = max(reps, 5)
        stats = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))
        off_ms = stats([enc.encode_device(text, out)[1] for _ in range(reps)])
        enc.long_words = True
        assert torch.equal(enc.encode_device(text, out)[0], ids)
        on_ms = stats([enc.encode_device(text, out)[1] for _ in range(reps)])
        print("long: no long word, bytes", text.numel(), "| mode off ms", off_ms[0], "min", off_ms[1], "max", off_ms[2],
              "| mode on ms", on_ms[0], "min", on_ms[1], "max", on_ms[2], "ratio", on_ms[0] / off_ms[0],
              "scratch", enc.long_word_stats["scratch_bytes"], flush=True)
        host = text.cpu().numpy()
        glued = host.copy()
        delim = np.isin(host, np.frombuffer(b"\t\r\n ", dtype=np.uint8))
        for at in range(65536, host.size - 4096, 65536):
            glued[at:at + 4096][delim[at:at + 4096]] = ord("x")
        gt = torch.from_numpy(glued).cuda()
        before = enc.long_word_stats
        enc.encode_device(gt, out)
        words = enc.long_word_stats["words"] - before["words"]
        ms = stats([enc.encode_device(gt, out)[1] for _ in range(reps)])
        print("long: one 4 KB word per 64 KB, long words", words, "ms", ms[0], "min", ms[1], "max", ms[2], "GB/s",
              gt.numel() / ms[0] / 1e6, "scratch", enc.long_word_stats["scratch_bytes"], flush=True)
        solid = host[~delim]
        for size in (4096, 65536, 1 << 20):
            if solid.size < size:
                break
            w = torch.from_numpy(solid[:size].copy()).cuda()
            o = torch.empty(size, dtype=torch.int32, device="cuda")
            before = enc.long_word_stats["rounds"]
            got = enc.encode_device(w, o)[0].numel()
            rounds = enc.long_word_stats["rounds"] - before
            ms = stats([enc.encode_device(w, o)[1] for _ in range(3 if size > 65536 else reps)])
            print("long: one word of", size, "bytes: ids", got, "rounds", rounds, "of", enc.num_merges, "merges | ms", ms[0],
                  "min", ms[1], "max", ms[2], "MB/s", size / ms[0] / 1e3, flush=True)
        enc.long_words = False
    if docs:
        del out
        reps = max(reps, 5)
        n = text.numel()
        nl = torch.nonzero(text == 10).flatten() + 1
        if nl.numel() == 0 or int(nl[-1].item()) != n:
            nl = torch.cat([nl, nl.new_tensor([n])])
        off = torch.cat([nl.new_zeros(1), nl]).contiguous()
        med = lambda v: sorted(v)[len(v) // 2]

        def whole(fn):
            """median device ms of the whole call fn() over reps runs"""
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            return med(ms)

        run_docs = lambda: enc.encode_docs_device(text, off, starts=True)
        run_spans = lambda: enc.encode_spans_device(text, starts=True, lines=True)
        got = run_docs()  # first calls: allocate the scratch
        ref = run_spans()
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[2]) and torch.equal(got[2], ref[1])
        run_docs()
        run_spans()
        dt = [run_docs()[3] for _ in range(reps)]
        st = [run_spans()[3] for _ in range(reps)]
        call_docs, call_spans = whole(run_docs), whole(run_spans)
        dst = torch.empty_like(text)
        copy_ms = whole(lambda: dst.copy_(text))
        big = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")  # past the last-level cache
        big_dst = torch.empty_like(big)
        big_ms = whole(lambda: big_dst.copy_(big))
        del big, big_dst
        docs_ms = med([t[3] for t in dt])
        print("docs: bytes", n, "documents", off.numel() - 1, "ids", got[0].numel(), "| encode_docs_device encode_ms",
              med([t[0] for t in dt]), "spans_ms", med([t[1] for t in dt]), "docs_ms", docs_ms, "min",
              min(t[3] for t in dt), "max", max(t[3] for t in dt), "| encode_spans_device encode_ms",
              med([t[0] for t in st]), "spans_ms", med([t[1] for t in st]), "| whole call ms docs", call_docs, "spans",
              call_spans, "ratio", call_docs / call_spans, "| d2d copy of the text ms", copy_ms, "GB/s (read + write)",
              2 * n / copy_ms / 1e6, "| d2d copy of 1 GiB ms", big_ms, "GB/s", 2 * (1 << 30) / big_ms / 1e6, flush=True)
        # the library prints the split of the document passes; the same text as one document (no
        # boundary: no search, no byte walk) and as 16 documents (searches of 4 steps, next to no walk)
        # shows what the copy kernel pays for the documents
        os.environ["SHREDWORD_ENCODE_DEBUG"] = "1"
        few = off[torch.arange(17, device="cuda") * (off.numel() - 1) // 16].contiguous()
        for name, o in (("one per line", off), ("one document", None), ("16 documents", few)):
            print("document passes,", name, file=sys.stderr, flush=True)
            for _ in range(4):
                enc.encode_docs_device(text, o, starts=True)
        del os.environ["SHREDWORD_ENCODE_DEBUG"]
    if decode:
        del out
        ids, _, line, _ = enc.encode_spans_device(text, starts=False)
        for name, row, sep in (("decode", None, None), ("decode rows+sep", line, b"\n")):
            dec, _, _ = enc.decode_device(ids, row, sep=sep)  # first call: allocates the vocabulary and the scratch
            ms = sorted(enc.decode_device(ids, row, sep=sep)[2] for _ in range(max(reps, 5)))
            med = ms[len(ms) // 2]
            print(name + ": ids", ids.numel(), "bytes", dec.numel(), "ids/byte", ids.numel() / dec.numel(),
                  "ms", med, "GB/s", dec.numel() / med / 1e6, "min", ms[0], "max", ms[-1], flush=True)
        h_ids = ids.cpu().numpy()
        want = enc.decode(h_ids)  # warm-up
        assert want == enc.decode_device(ids)[0].cpu().numpy().tobytes()
        host = []
        for _ in range(max(reps, 5)):
            t0 = time.perf_counter()
            enc.decode(h_ids)  # sizing pass + copy pass of shred_decode
            host.append((time.perf_counter() - t0) * 1e3)
        host.sort()
        print("host shred_decode (sizing + copy, wall): ms", host[len(host) // 2], "GB/s",
              len(want) / host[len(host) // 2] / 1e6, "min", host[0], "max", host[-1], flush=True)
    if batch:
        reps = max(reps, 5)
        R, n, W, L = line.numel() - 1, ids.numel(), 1024, 2048

        def timed(fn):
            """median / min / max device ms of fn() over reps runs, after two warm-up runs"""
            for _ in range(2):
                fn()
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            ms.sort()
            return ms[len(ms) // 2], ms[0], ms[-1]

        def torch_rows(lens, width):
            """(row, column, source index) of every kept id: the index built from repeat_interleave"""
            total = int(lens.sum().item())
            row = torch.repeat_interleave(torch.arange(R, device="cuda"), lens, output_size=total)
            col = torch.arange(total, device="cuda") - torch.repeat_interleave(lens.cumsum(0) - lens, lens,
                                                                              output_size=total)
            return row, col, torch.repeat_interleave(line[:-1], lens, output_size=total) + col

        def torch_pad():
            lens = (line[1:] - line[:-1]).clamp(max=W)
            out = torch.full((R, W), -1, dtype=torch.int32, device="cuda")
            mask = torch.zeros((R, W), dtype=torch.uint8, device="cuda")
            row, col, src = torch_rows(lens, W)
            out[row, col] = ids[src]
            mask[row, col] = 1
            return out, lens.to(torch.int32), mask

        def torch_pack():
            lens = line[1:] - line[:-1]
            e = lens + 1
            start = torch.cat([e.new_zeros(1), e.cumsum(0)])
            T = int(start[-1].item())
            S = -(-T // L)
            out = torch.full((S * L,), -1, dtype=torch.int32, device="cuda")
            pos = torch.zeros(S * L, dtype=torch.int32, device="cuda")
            seg = torch.full((S * L,), -1, dtype=torch.int32, device="cuda")
            row, col, src = torch_rows(lens, 0)
            out[start[:-1][row] + col] = ids[src]
            out[start[1:] - 1] = 0  # the eos of every row
            seg[:T] = torch.repeat_interleave(torch.arange(R, device="cuda", dtype=torch.int32), e, output_size=T)
            pos[:T] = (torch.arange(T, device="cuda") - torch.repeat_interleave(start[:-1], e, output_size=T)).int()
            return out.view(S, L), start, pos.view(S, L), seg.view(S, L)

        pad_kw = dict(max_len=W, width=W, pad_id=-1, mask=True)
        pack_kw = dict(seq_len=L, eos=0, pad_id=-1, positions=True, segments=True)
        ours = enc.pad_device(ids, line, **pad_kw)  # first call: allocates the batch scratch
        assert all(torch.equal(a, b) for a, b in zip(ours[:3], torch_pad()))
        ms = sorted(enc.pad_device(ids, line, **pad_kw)[3] for _ in range(reps))
        fill = ours[1].sum().item() / (R * W)
        nbytes = R * W * (4 + 4 * fill + 1) + 16 * R
        t, c = timed(torch_pad), timed(lambda: enc.pad_device(ids, line, **pad_kw))
        print("pad: rows", R, "width", W, "fill", fill, "ms", ms[len(ms) // 2], "GB/s", nbytes / ms[len(ms) // 2] / 1e6,
              "of 8 TB/s", nbytes / ms[len(ms) // 2] / 1e6 / 8000, "min", ms[0], "max", ms[-1],
              "| whole call (sizing call, allocation, passes) ms", c[0],
              "| torch ms", t[0], "min", t[1], "max", t[2], flush=True)
        ours = enc.pack_device(ids, line, **pack_kw)
        assert all(torch.equal(a, b) for a, b in zip(ours[:4], torch_pack()))
        ms = sorted(enc.pack_device(ids, line, **pack_kw)[4] for _ in range(reps))
        nbytes = ours[0].numel() * 16 + 16 * R
        t, c = timed(torch_pack), timed(lambda: enc.pack_device(ids, line, **pack_kw))
        print("pack: rows", R, "ids", n, "sequences", ours[0].shape[0], "ms", ms[len(ms) // 2], "GB/s",
              nbytes / ms[len(ms) // 2] / 1e6, "of 8 TB/s", nbytes / ms[len(ms) // 2] / 1e6 / 8000, "min", ms[0],
              "max", ms[-1], "| whole call (sizing call, allocation, passes) ms", c[0],
              "| torch ms", t[0], "min", t[1], "max", t[2], flush=True)
    if window:
        del out
        reps = max(reps, 5)
        ids, _, line, _ = enc.encode_spans_device(text, starts=False)
        R, n, W, S = line.numel() - 1, ids.numel(), 1024, 128
        step = W - S

        def timed(fn):
            """median / min / max device ms of fn() over reps runs, after two warm-up runs"""
            for _ in range(2):
                fn()
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            ms.sort()
            return ms[len(ms) // 2], ms[0], ms[-1]

        def torch_window():
            lens = line[1:] - line[:-1]
            w = torch.where(lens <= W, torch.ones_like(lens), 1 + (lens - W + step - 1) // step)
            wo = torch.cat([w.new_zeros(1), w.cumsum(0)])
            Wn = int(wo[-1].item())
            wrow = torch.repeat_interleave(torch.arange(R, device="cuda"), w, output_size=Wn)
            src = line[:-1][wrow] + (torch.arange(Wn, device="cuda") - wo[:-1][wrow]) * step
            cnt = (line[1:][wrow] - src).clamp(max=W)
            col = torch.arange(W, device="cuda")
            m = col[None, :] < cnt[:, None]
            out = torch.where(m, ids[(src[:, None] + col[None, :]).clamp(max=max(n - 1, 0))], -1)
            return out, cnt.to(torch.int32), wrow.to(torch.int32), src, wo, m.to(torch.uint8)

        kw = dict(max_len=W, stride=S, width=W, pad_id=-1, mask=True)
        ours = enc.window_device(ids, line, **kw)  # first call: allocates the window scratch
        assert all(torch.equal(a, b) for a, b in zip(ours[:6], torch_window()))
        Wn = ours[0].shape[0]
        ms = sorted(enc.window_device(ids, line, **kw)[6] for _ in range(reps))
        fill = ours[1].sum().item() / (Wn * W)
        nbytes = Wn * W * (4 + 4 * fill + 1) + 16 * Wn + 40 * R
        t, c = timed(torch_window), timed(lambda: enc.window_device(ids, line, **kw))
        print("window: rows", R, "windows", Wn, "width", W, "stride", S, "fill", fill, "ms", ms[len(ms) // 2], "GB/s",
              nbytes / ms[len(ms) // 2] / 1e6, "of 8 TB/s", nbytes / ms[len(ms) // 2] / 1e6 / 8000, "min", ms[0], "max",
              ms[-1], "| whole call (sizing call, allocation, passes) ms", c[0],
              "| torch gather ms", t[0], "min", t[1], "max", t[2], flush=True)
        pad_kw = dict(max_len=W, width=W, pad_id=-1, mask=True)
        ours = enc.pad_device(ids, line, **pad_kw)
        ms = sorted(enc.pad_device(ids, line, **pad_kw)[3] for _ in range(reps))
        fill = ours[1].sum().item() / (R * W)
        nbytes = R * W * (4 + 4 * fill + 1) + 16 * R
        print("pad at the same width: rows", R, "fill", fill, "ms", ms[len(ms) // 2], "GB/s",
              nbytes / ms[len(ms) // 2] / 1e6, "min", ms[0], "max", ms[-1], flush=True)
    if pair:
        del out
        reps = max(reps, 5)
        R, M, S, BOS, SEP, EOS = 65536, 512, 128, 1, 2, 3
        g = torch.Generator().manual_seed(5)
        offs = lambda lens: torch.cat([lens.new_zeros(1), lens.cumsum(0)])
        ra, rb = offs(torch.randint(8, 33, (R,), generator=g)), offs(torch.randint(200, 1501, (R,), generator=g))
        ids_a, ids_b = (torch.randint(10, 50_000, (int(r[-1]),), generator=g, dtype=torch.int32).cuda() for r in (ra, rb))
        ra, rb = ra.cuda(), rb.cuda()

        def torch_pair():
            la, lb = ra[1:] - ra[:-1], rb[1:] - rb[:-1]
            C = M - 3 - la
            step = C - S
            w = torch.where(lb <= C, torch.ones_like(lb), 1 + (lb - C + step - 1) // step)
            wo = offs(w)
            Wn = int(wo[-1].item())
            prow = torch.repeat_interleave(torch.arange(R, device="cuda"), w, output_size=Wn)
            bsrc = rb[:-1][prow] + (torch.arange(Wn, device="cuda") - wo[:-1][prow]) * step[prow]
            ka, asrc = la[prow], ra[:-1][prow]
            kb = torch.minimum(rb[1:][prow] - bsrc, C[prow])
            e = 3 + ka + kb
            col = torch.arange(M, device="cuda")[None, :]
            ja, jb = col - 1, col - 2 - ka[:, None]
            out = torch.where(col < e[:, None], EOS, -1).to(torch.int32)  # the eos is what no other rule overwrites
            out = torch.where((jb >= 0) & (jb < kb[:, None]), ids_b[(bsrc[:, None] + jb).clamp(0, ids_b.numel() - 1)], out)
            out = torch.where(jb == -1, SEP, out)
            out = torch.where((ja >= 0) & (ja < ka[:, None]), ids_a[(asrc[:, None] + ja).clamp(0, ids_a.numel() - 1)], out)
            out[:, 0] = BOS
            return (out, e.to(torch.int32), prow.to(torch.int32), torch.stack([ka, kb], 1).to(torch.int32),
                    torch.stack([asrc, bsrc], 1), wo, ((jb >= 0) & (col < e[:, None])).to(torch.uint8),
                    (col < e[:, None]).to(torch.uint8))

        kw = dict(max_len=M, truncation="window_second", stride=S, bos=BOS, sep=(SEP,), eos=EOS, width=M, pad_id=-1,
                  types=True, mask=True)
        ours = enc.pair_device(ids_a, ra, ids_b, rb, **kw)  # first call: allocates the pair scratch
        assert all(torch.equal(a, b) for a, b in zip(ours[:8], torch_pair()))
        Wn = ours[0].shape[0]
        for _ in range(5):
            enc.pair_device(ids_a, ra, ids_b, rb, **kw)
        ms = sorted(enc.pair_device(ids_a, ra, ids_b, rb, **kw)[8] for _ in range(reps))
        fill = ours[1].sum().item() / (Wn * M)
        nbytes = Wn * M * (4 + 4 * fill + 2) + 32 * Wn + 64 * R
        print("pair: examples", R, "ids", ids_a.numel(), "+", ids_b.numel(), "emitted rows", Wn, "width", M, "stride", S,
              "fill", fill, "ms", ms[len(ms) // 2], "GB/s", nbytes / ms[len(ms) // 2] / 1e6, "of 8 TB/s",
              nbytes / ms[len(ms) // 2] / 1e6 / 8000, "min", ms[0], "max", ms[-1], flush=True)
    if mlm:
        del out
        reps = max(reps, 7)
        n, P, MASK, IGN = 1 << 26, 0.15, 4, -100
        V = 256 + enc.num_merges
        g = torch.Generator().manual_seed(7)
        rl = torch.randint(200, 501, (n // 350 + 1,), generator=g)
        row = torch.cat([rl.new_zeros(1), rl.cumsum(0)])
        row = torch.cat([row[row < n], row.new_tensor([n])]).cuda()
        ids = torch.randint(5, V, (n,), generator=g, dtype=torch.int32).cuda()
        lens_t = torch.from_numpy(enc.token_lengths).cuda()
        tl = lens_t[ids.long()].long()
        gap = (torch.rand(n, generator=g) < 0.3).cuda().long()  # a delimiter before the token: words of 3.3 tokens
        gap[0] = 0
        starts = (tl.cumsum(0) - tl + gap.cumsum(0)).contiguous()
        del tl, gap
        prot = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device="cuda")

        def events(fn):
            """median / min / max device ms of fn() over reps runs, after two warm-up runs"""
            for _ in range(2):
                fn()
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            ms.sort()
            return ms[len(ms) // 2], ms[0], ms[-1]

        def torch_apply(sel):
            """the collator's tail: labels, then 80 % mask, 10 % random, 10 % kept"""
            labels = torch.where(sel, ids, IGN)
            act = torch.rand(n, device="cuda")
            rnd = torch.randint(0, V, (n,), dtype=torch.int32, device="cuda")
            return torch.where(sel & (act < 0.8), MASK, torch.where(sel & (act < 0.9), rnd, ids)), labels

        def torch_token():
            return torch_apply((torch.rand(n, device="cuda") < P) & ~torch.isin(ids, prot))

        def torch_whole():
            """word begins from starts, the rows and the protected ids; one draw per word, gathered per token"""
            guarded = torch.isin(ids, prot)
            begin = torch.ones(n, dtype=torch.bool, device="cuda")
            begin[1:] = (starts[1:] != starts[:-1] + lens_t[ids[:-1].long()]) | guarded[1:] | guarded[:-1]
            begin[row[:-1]] = True
            word = begin.cumsum(0) - 1
            return torch_apply((torch.rand(int(word[-1].item()) + 1, device="cuda")[word] < P) & ~guarded)

        kw = dict(mask_id=MASK, p=P, seed=1, random_vocab=V, protect=(0, 1, 2, 3))
        legs = (("token", False, 12, torch_token), ("whole-word", True, 44, torch_whole))
        for name, whole, per_id, ref in () if corrupt or fim else legs:
            run = lambda: enc.mlm_device(ids, row, whole_word=whole, starts=starts, **kw)
            run()  # first call: allocates the masking scratch
            run()
            res = [run() for _ in range(reps)]
            ms = sorted(r[3] for r in res)
            med = ms[len(ms) // 2]
            t, c = events(ref), events(run)
            picked = int((ref()[1] != IGN).sum().item())
            print("mlm", name + ": ids", n, "rows", row.numel() - 1, "selected", res[0][2], "share", res[0][2] / n,
                  "| ms", med, "GB/s at", per_id, "B per id", per_id * n / med / 1e6, "min", ms[0], "max", ms[-1],
                  "| whole call (allocation, passes) ms", c[0], "| torch composition ms", t[0], "min", t[1], "max", t[2],
                  "selected share", picked / n, "| torch / ours", t[0] / med, flush=True)
    if corrupt:
        del starts
        import math
        R, S0, SN = row.numel() - 1, V + 99, 100
        p_start, RMAX = -math.log(1 - 0.15) / 3.0, SN - 1
        ar = torch.arange(n, device="cuda")

        def torch_corrupt():
            start = torch.rand(n, device="cuda") < p_start
            L = torch.randint(1, 6, (n,), device="cuda")
            k = start.nonzero().squeeze(1)
            end = torch.minimum(k + L[k], row[torch.bucketize(k, row, right=True)])  # the reach, cut at the row's end
            delta = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
            delta.index_add_(0, k, torch.ones_like(k, dtype=torch.int32))
            delta.index_add_(0, end, -torch.ones_like(k, dtype=torch.int32))
            noise = (delta.cumsum(0)[:n] > 0) & ~torch.isin(ids, prot)
            begin = torch.zeros(n, dtype=torch.bool, device="cuda")
            begin[row[:-1][row[:-1] < n]] = True
            first = noise.clone()
            first[1:] &= begin[1:] | ~noise[:-1]
            c = first.cumsum(0)
            base = (c - first.long())[begin.nonzero().squeeze(1)]        # runs before each non-empty row
            rank = c - 1 - base[begin.cumsum(0) - 1]
            gone = noise & (rank < RMAX)
            sent = (S0 - rank).int()
            keep = ~gone | first
            in_ids, in_src = torch.where(gone, sent, ids)[keep], ar[keep]
            kc = torch.cat([keep.new_zeros(1, dtype=torch.long), keep.cumsum(0)])
            tg = gone.long() + (gone & first).long()
            tc = torch.cat([tg.new_zeros(1), tg.cumsum(0)])
            in_row, tgt_row = kc[row], tc[row] + torch.arange(R + 1, device="cuda")
            tgt = torch.empty(int(tgt_row[-1].item()), dtype=torch.int32, device="cuda")
            at = tc[:n] + torch.bucketize(ar, row, right=True) - 1   # the rows before close with one sentinel each
            gf = gone & first
            tgt[at[gf]] = sent[gf]
            tgt[(at + first)[gone]] = ids[gone]
            cp = torch.cat([c.new_zeros(1), c])
            tgt[tgt_row[1:] - 1] = (S0 - (cp[row[1:]] - cp[row[:-1]]).clamp(max=RMAX)).int()
            return in_ids, in_row, tgt, tgt_row, in_src

        run = lambda: enc.corrupt_device(ids, row, sentinel_first=S0, seed=1, protect=(0, 1, 2, 3), src=True)
        run()  # first call: allocates the corruption scratch
        run()
        res = [run() for _ in range(reps)]
        ms = sorted(r[5] for r in res)
        med = ms[len(ms) // 2]
        t, c = events(torch_corrupt), events(run)
        ref = torch_corrupt()
        t_in, t_tgt = res[0][0].numel(), res[0][2].numel()
        nbytes = 11 * n + 12 * t_in + 4 * t_tgt + 40 * R
        print("corrupt: ids", n, "rows", R, "input ids", t_in, "target ids", t_tgt, "noise share",
              (t_tgt - R + n - t_in) / 2 / n, "| ms", med, "GB/s by the traffic model", nbytes / med / 1e6, "min", ms[0], "max", ms[-1],
              "| whole call (allocation, passes) ms", c[0], "| torch composition ms", t[0], "min", t[1], "max", t[2],
              "input ids", ref[0].numel(), "target ids", ref[2].numel(), "| torch / ours", t[0] / med, flush=True)
    if fim:
        del starts
        R, SEED, PRE, SUF, MID = row.numel() - 1, 1, V, V + 1, V + 2
        s64 = lambda v: v - (1 << 64) if v >= 1 << 63 else v           # a uint64 constant as torch's int64 holds it
        lsr = lambda x, s: (x >> s) & ((1 << (64 - s)) - 1)            # the logical shift of a uint64

        def tmix(x):
            x = x ^ lsr(x, 33)
            x = x * s64(0xff51afd7ed558ccd)
            x = x ^ lsr(x, 33)
            x = x * s64(0xc4ceb9fe1a85ec53)
            return x ^ lsr(x, 33)

        def draw(h, c):
            return lsr(tmix(tmix(s64(SEED) + s64(0x9E3779B97F4A7C15) * (h + 1)) ^ c), 32)

        def torch_fim():
            """the header's definition: per-row draws by the same hash in int64 arithmetic, the output offsets by
            a cumsum, every output position's row by bucketize, its source index by where, and one gather"""
            L = row[1:] - row[:-1]
            h = torch.arange(R, device="cuda")
            on = draw(h, (1 << 40) + 4) < (1 << 31)
            x, y = (draw(h, (1 << 40) + 5) * (L + 1)) >> 32, (draw(h, (1 << 40) + 6) * (L + 1)) >> 32
            a, b = torch.minimum(x, y), torch.maximum(x, y)
            mode = torch.where(on, (draw(h, (1 << 40) + 7) < (1 << 31)).long(), -1)
            info = torch.stack([torch.where(on, a, -1), torch.where(on, b, -1), mode], dim=1)
            out_row = row + torch.cat([row.new_zeros(1), (on.long() * 3).cumsum(0)])
            T = int(out_row[-1].item())
            p = torch.arange(T, device="cuda")
            r = torch.bucketize(p, out_row, right=True) - 1
            off, pa, pb, pm = p - out_row[r], a[r], b[r], mode[r]
            tail = L[r] - pb
            spm = pm == 1
            s1 = torch.where(spm, 1, pa + 1)                # the position of suf_id, of mid_id
            s2 = torch.where(spm, 2 + tail, pa + 2 + tail)
            q = off - 3 - tail
            psm = torch.where(off <= pa, off - 1, torch.where(off < s2, pb + off - pa - 2, q))
            idx = torch.where(pm < 0, off, torch.where(spm, torch.where(off < s2, pb + off - 2, q), psm))
            sent = (pm >= 0) & ((off == 0) | (off == s1) | (off == s2))
            src = torch.where(sent, -1, row[r] + idx)
            out = torch.where(sent, torch.where(off == 0, PRE, torch.where(off == s1, SUF, MID)).int(),
                              torch.gather(ids, 0, src.clamp(min=0)))
            mid = torch.where(spm, q >= pa, off > s2)
            seg = torch.where(pm < 0, 0, torch.where(sent, 4, torch.where(mid, 3, torch.where(
                torch.where(spm, off < s2, off > pa), 2, 1)))).to(torch.uint8)
            return out, out_row, src, seg, info

        run = lambda: enc.fim_device(ids, row, pre_id=PRE, suf_id=SUF, mid_id=MID, fim_rate=0.5, spm_rate=0.5, seed=SEED,
                                     src=True, seg=True, info=True)
        run()  # first call: allocates the FIM scratch
        run()
        res = [run() for _ in range(reps)]
        ms = sorted(r[5] for r in res)
        med = ms[len(ms) // 2]
        t, c = events(torch_fim), events(run)
        ref = torch_fim()
        same = all(torch.equal(g, w) for g, w in zip(res[0][:5], ref))
        T = res[0][0].numel()
        nbytes = 17 * T + 130 * R + 48 * R  # batch_fim.hip's model, with out_src, out_seg and row_info
        print("fim: ids", n, "rows", R, "output ids", T, "transformed rows", (T - n) // 3, "spm rows",
              int((res[0][4][:, 2] == 1).sum().item()), "| ms", med, "GB/s by the traffic model", nbytes / med / 1e6,
              "min", ms[0], "max", ms[-1], "| whole call (allocation, passes) ms", c[0], "| torch composition ms", t[0],
              "min", t[1], "max", t[2], "| equal to the torch composition", same, "| torch / ours", t[0] / med, flush=True)
        assert same, "fim_device and the torch composition of the same definition differ"
    enc.destroy()
