"""Encoder timing on one corpus: python enc_bench.py prepare CORPUS BYTES DIR  (generate + train + save)
                                   python enc_bench.py run CORPUS DIR [reps] [spans | decode]   (SHREDWORD_LIB picks the build)
With a trailing `spans`, run also times encode_spans_device (token starts + line offsets); with a
trailing `decode`, decode_device on the corpus's ids and line offsets (median / min / max ms and
GB/s of output), and the host loop shred_decode on the same ids (wall time) for comparison."""
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
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
    spans, decode = args[-1] == "spans", args[-1] == "decode"
    if spans or decode:
        args = args[:-1]
    d = args[0]
    reps = int(args[1]) if len(args) > 1 else 5
    import torch
    from shredword.encoder import BPEEncoder
    enc = BPEEncoder(os.path.join(d, "m.model"), os.path.join(d, "m.vocab"), unk_id=0)
    text = torch.from_numpy(np.fromfile(corpus, dtype=np.uint8)).cuda()
    out = torch.empty(text.numel(), dtype=torch.int32, device="cuda")
    ids, _ = enc.encode_device(text, out)
    ms = sorted(enc.encode_device(text, out)[1] for _ in range(reps))
    print(os.environ.get("SHREDWORD_LIB", "default"), "ids", ids.numel(), "ms", ms[len(ms) // 2],
          "GB/s", text.numel() / ms[len(ms) // 2] / 1e6, "min", ms[0], "max", ms[-1], flush=True)
    if spans:
        del out
        enc.encode_spans_device(text)  # first call: allocates the span scratch
        runs = sorted((enc.encode_spans_device(text)[3] for _ in range(reps)), key=lambda t: t[1])
        encode_ms, spans_ms = sorted(t[0] for t in runs)[reps // 2], runs[reps // 2][1]
        print("spans: encode_ms", encode_ms, "spans_ms", spans_ms, "ratio", spans_ms / encode_ms,
              "spans min", runs[0][1], "max", runs[-1][1], flush=True)
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
    enc.destroy()
