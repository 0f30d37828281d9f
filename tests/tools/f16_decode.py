#!/usr/bin/env python
"""An F16-weight LLaMA (file type 1) on the F16 plan (plan_launch_f16, kernels/decode_f16.h) against the node-by-node executor
(option plan_f16 = 0), in one run: a synthetic model, gaussians rounded to f16.
    python tests/tools/f16_decode.py [7b | 13b | tiny] [--as-built] [--out FILE]
Three lines per leg: single-token decode (greedy, from 128 positions on), prompt feed at n_batch = 8 (256 tokens into a fresh
session) and one decode step of 4 sessions (Llama.infer_next_tokens_batch; a backend that declines steps them one by one,
`ran_batched` says which).  Every line: warm-up, REPEATS timed repeats (env F16_REPEATS, default 5), the median in tokens/s and
the spread (min, max) over the repeats.  Decode also carries the bytes a token streams (every 2-D weight but the embedding
table, of which it reads one row) and the fraction of the 8 TB/s this project uses as the HBM peak.
--as-built: touch no option and time the one leg the library runs by itself (a build without the plan_f16 key: only
`evaluate`-level calls are used).  Prints one JSON line; --out appends it to a file."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12
F16 = 1


def f16_weights(synth, hp0):
    try:
        return synth.make_llama_fast(hp0, F16)
    except KeyError:  # a build whose make_llama_fast has no F16 form: the same construction here
        pool = (0.02 * np.random.default_rng(0xF16).standard_normal(1 << 24, dtype=np.float32)).astype(np.float16)
        w = {}
        for i, (name, (ne0, ne1)) in enumerate(synth.tensor_shapes(hp0).items()):
            rng = np.random.default_rng([1234, i])
            if ne1 is None:
                w[name] = (1.0 + 0.01 * rng.standard_normal(ne0)).astype(np.float32)
                continue
            n = ne0 * ne1
            a = np.empty(n, np.float16)
            at, off = 0, int(rng.integers(0, pool.size))
            while at < n:
                k = min(n - at, pool.size - off)
                a[at:at + k] = pool[off:off + k]
                at, off = at + k, 0
            w[name] = a.view(np.uint8)
        hp = dict(hp0)
        hp["wtype"] = F16
        return hp, w


def timed(fn, tokens, repeats, sync):
    rates = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        rates.append(tokens / (time.perf_counter() - t0))
    return {"tokens_per_s": round(statistics.median(rates), 2), "min": round(min(rates), 2), "max": round(max(rates), 2),
            "repeats": repeats}


def main():
    args = sys.argv[1:]
    as_built = "--as-built" in args
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    size = next((a for a in args if a in ("7b", "13b", "tiny")), "7b")
    repeats = int(os.environ.get("F16_REPEATS", "5"))
    from llm_amd import ggml, llama, synth
    L = ggml.lib()
    hp0 = {"7b": synth.LLAMA_7B, "13b": synth.LLAMA_13B, "tiny": synth.TINY}[size]
    hp, w = f16_weights(synth, hp0)
    ctx = 64 if size == "tiny" else 2048
    n_prompt, n_feed, n_dec = (16, 24, 8) if size == "tiny" else (128, 256, 48)
    print("weights made", file=sys.stderr, flush=True)
    model = llama.Llama(hp, w, context_size=ctx)
    stream_bytes = sum(a.nbytes for name, a in w.items() if a.dtype == np.uint8 and name != "tok_embeddings.weight")
    out = {"tool": "f16_decode", "model": f"LLaMA-{size} F16 (synthetic)", "bytes_per_token": stream_bytes, "hbm_peak": HBM_PEAK, "legs": {}}
    sync = L.ggml_hip_synchronize
    toks = lambda n, k=7: ((np.arange(n, dtype=np.int32) * k + 5) % hp["n_vocab"]).astype(np.int32)  # noqa: E731
    for leg in (("as_built",) if as_built else ("plan", "executor")):
        if not as_built:
            ggml.set_option("plan_f16", 1 if leg == "plan" else 0)
        p0, g0 = ggml.get_stat("plan_tokens"), ggml.get_stat("generic_graphs")
        res = {}
        # ---- decode
        s = model.start_session(n_batch=8)
        s.feed_prompt(toks(n_prompt))
        for _ in range(4):
            s.infer_next_token()

        def decode():
            for _ in range(n_dec):
                s.infer_next_token()
        res["decode"] = timed(decode, n_dec, repeats, sync)
        res["decode"]["fraction_of_hbm_peak"] = round(res["decode"]["tokens_per_s"] * stream_bytes / HBM_PEAK, 4)
        print(leg, "decode", res["decode"], file=sys.stderr, flush=True)
        s.free()
        # ---- prompt feed at n_batch = 8
        f = model.start_session(n_batch=8)
        f.feed_prompt(toks(16))  # warm-up: the chunk plan is built and captured

        def feed():
            f.rewind(f.n_past - 16) if f.n_past > 16 else None
            f.feed_prompt(toks(n_feed, 11))
        res["feed_n_batch_8"] = timed(feed, n_feed, repeats, sync)
        print(leg, "feed", res["feed_n_batch_8"], file=sys.stderr, flush=True)
        f.free()
        # ---- one decode step of 4 sessions
        sess = [model.start_session(n_batch=8) for _ in range(4)]
        for i, b in enumerate(sess):
            b.feed_prompt(toks(n_prompt // 2 + i, 7 + i))
        ran = [True]

        def step():
            for _ in range(n_dec // 2):
                ran[0] = model.infer_next_tokens_batch(sess)[0] and ran[0]
        step()
        res["batch_4_sessions"] = timed(step, 4 * (n_dec // 2), repeats, sync)
        res["batch_4_sessions"]["ran_batched"] = bool(ran[0])
        for b in sess:
            b.free()
        res["plan_tokens"] = ggml.get_stat("plan_tokens") - p0
        res["generic_graphs"] = ggml.get_stat("generic_graphs") - g0
        out["legs"][leg] = res
    if not as_built:
        ggml.set_option("plan_f16", 1)
        out["plan_vs_executor"] = {k: round(out["legs"]["plan"][k]["tokens_per_s"] / out["legs"]["executor"][k]["tokens_per_s"], 2)
                                   for k in ("decode", "feed_n_batch_8", "batch_4_sessions")}
    model.free()
    line = json.dumps(out)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
