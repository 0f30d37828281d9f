#!/usr/bin/env python
"""A block-format LLaMA with a K-quant output matrix (Q4_0 layers and tok_embeddings, output.weight Q6_K: what llama.cpp's
quantizer writes for its "mostly Q4_0" files) on the fused plans (LlamaMatch::out_k, option plan_out_k) against the node-by-node
executor (plan_out_k = 0: what the library ran before the option existed) and against the pure Q4_0 model, in one run: synthetic
blocks from synth.make_llama_fast.
    python tests/tools/mixed_output.py [7b | 13b | tiny] [--out FILE]
Legs per model: single-token decode (greedy, from 128 positions on), prompt feed at n_batch = 8 (256 tokens into a fresh session),
a 512-token prefill (n_batch = 512) and the greedy chain of 8 sessions (Llama.infer_tokens_batch).  Every line: warm-up, REPEATS
timed repeats (env MIXED_REPEATS, default 5), the median in tokens/s and the spread (min, max).  The lm_head launch's own time
comes from the roofline replay of mat-vec kind 4 alone and in sequence (all mat-vec launches minus all but that kind), as
bench.py's roofline leg takes it.  Prints one JSON line; --out appends it to a file.
Not measured here: whether the pure Q4_0 model is as fast as before the feature.  That comparison needs the parent commit's library
and is bench.py's: its default run on this commit and on the parent built in a second tree, alternating, five runs each — this
commit's median must lie inside the parent's min-max spread (the feature adds no kernel and changes no launch the pure model uses)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
Q4_0, Q6_K = 2, 14


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


def legs_of(ggml, model, hp, size, repeats, plan_legs):
    L = ggml.lib()
    sync = L.ggml_hip_synchronize
    n_prompt, n_feed, n_fill, n_dec, n_chain = (16, 24, 40, 8, 4) if size == "tiny" else (128, 256, 512, 48, 24)
    toks = lambda n, k=7: ((np.arange(n, dtype=np.int32) * k + 5) % hp["n_vocab"]).astype(np.int32)  # noqa: E731
    keys = ("plan_tokens", "out_k_tokens", "prompt_plan_tokens", "generic_graphs", "batch_decode_steps")
    s0 = [ggml.get_stat(k) for k in keys]
    res = {}
    s = model.start_session(n_batch=8)
    s.feed_prompt(toks(n_prompt))
    for _ in range(4):
        s.infer_next_token()

    def decode():
        for _ in range(n_dec):
            s.infer_next_token()
    res["decode"] = timed(decode, n_dec, repeats, sync)
    if plan_legs:  # the lm_head launch of the single-token plan that just ran: alone, and what it costs in sequence
        rs = 50
        ms4, n4, b4 = ggml.bench_plan_class(ggml.KKIND_BASE + 4, rs)
        ms_all, _, _ = ggml.bench_plan_class(ggml.KCLASS_MMVQ, rs)
        ms_wo, _, _ = ggml.bench_plan_class(ggml.KKIND_BASE + 8 + 4, rs)
        res["lm_head"] = {"launches": n4, "bytes": int(b4 / max(n4, 1)), "alone_us": round(ms4 * 1e3 / rs / max(n4, 1), 2),
                          "in_sequence_us": round((ms_all - ms_wo) * 1e3 / rs / max(n4, 1), 2),
                          "all_mat_vecs_us_per_token": round(ms_all * 1e3 / rs, 2)}
    print("decode", res["decode"], res.get("lm_head"), file=sys.stderr, flush=True)
    s.free()
    f = model.start_session(n_batch=8)
    f.feed_prompt(toks(16))

    def feed():
        f.rewind(f.n_past - 16) if f.n_past > 16 else None
        f.feed_prompt(toks(n_feed, 11))
    res["feed_n_batch_8"] = timed(feed, n_feed, repeats, sync)
    print("feed", res["feed_n_batch_8"], file=sys.stderr, flush=True)
    f.free()
    p = model.start_session(n_batch=n_fill)
    p.feed_prompt(toks(n_fill, 13))  # warm-up: the f16 copies are made here

    def prefill():
        p.seek(0)
        p.feed_prompt(toks(n_fill, 13))
    res["prefill_%d" % n_fill] = timed(prefill, n_fill, repeats, sync)
    print("prefill", res["prefill_%d" % n_fill], file=sys.stderr, flush=True)
    p.free()
    sess = [model.start_session(n_batch=8) for _ in range(8)]
    for i, b in enumerate(sess):
        b.feed_prompt(toks(n_prompt // 2 + i, 7 + i))
    ran = [True]

    def chain():
        ran[0] = model.infer_tokens_batch(sess, n_chain)[0] and ran[0]
    chain()
    res["greedy_chain_8_sessions"] = timed(chain, 8 * n_chain, repeats, sync)
    res["greedy_chain_8_sessions"]["ran_chained"] = bool(ran[0])
    print("chain", res["greedy_chain_8_sessions"], file=sys.stderr, flush=True)
    for b in sess:
        b.free()
    res["counters"] = {k: ggml.get_stat(k) - a for k, a in zip(keys, s0)}
    return res


def main():
    args = sys.argv[1:]
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    size = next((a for a in args if a in ("7b", "13b", "tiny")), "7b")
    repeats = int(os.environ.get("MIXED_REPEATS", "5"))
    from llm_amd import ggml, llama, synth
    hp0 = {"7b": synth.LLAMA_7B, "13b": synth.LLAMA_13B, "tiny": dict(synth.TINY, n_embd=256, n_rot=64, n_ff=512)}[size]
    ctx = 128 if size == "tiny" else 2048
    hp, w = synth.make_llama_fast(hp0, Q4_0)
    pure_out = w["output.weight"]
    out = {"tool": "mixed_output", "model": f"LLaMA-{size} Q4_0 layers, Q6_K output (synthetic blocks)", "legs": {}}
    # the pure model first, then the same layers under the Q6_K output: on the plans and (plan_out_k = 0) node by node
    model = llama.Llama(hp, w, context_size=ctx)
    out["legs"]["pure_q4_0"] = legs_of(ggml, model, hp, size, repeats, True)
    model.free()
    w["output.weight"] = synth.make_llama_fast(hp0, Q6_K, only={"output.weight"})[1]["output.weight"]
    hp = dict(hp, wtypes={"output.weight": Q6_K})
    out["lm_head_bytes"] = {"q4_0": int(pure_out.nbytes), "q6_k": int(w["output.weight"].nbytes)}
    model = llama.Llama(hp, w, context_size=ctx)
    try:
        for leg, on in (("plans", 1), ("executor", 0), ("plans_again", 1), ("executor_again", 0)):
            ggml.set_option("plan_out_k", on)
            out["legs"][leg] = legs_of(ggml, model, hp, size, repeats, bool(on))
    finally:
        ggml.set_option("plan_out_k", 1)
        model.free()
    ratio = lambda a, b, k: round(out["legs"][a][k]["tokens_per_s"] / out["legs"][b][k]["tokens_per_s"], 3)  # noqa: E731
    kinds = [k for k in out["legs"]["plans"] if k not in ("lm_head", "counters")]
    out["plans_vs_executor"] = {k: ratio("plans", "executor", k) for k in kinds}
    out["plans_vs_pure_q4_0"] = {k: ratio("plans", "pure_q4_0", k) for k in kinds}
    line = json.dumps(out)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
