#!/usr/bin/env python
"""Batched multi-session decode of a K-quant model (option plan_batch_k = 1: Llama.infer_next_tokens_batch ->
ggml_hip_decode_batch on the K plan's chunk form) against the same sessions stepped one after the other (the single-token K
plan, B passes over the weights), and the greedy chain on that step (Llama.infer_tokens_batch -> ggml_hip_decode_batch_greedy),
in one run: synthetic LLaMA-7B weights of one K type, every session at about 128 positions, greedy tokens.
    python tests/tools/batch_decode_k.py [TYPE] [B ...]   (TYPE: Q2_K Q3_K Q4_K Q5_K Q6_K, default Q4_K; B default 2 4 8;
                                                           env BATCH_K_TOKENS: tokens per session and timed window, default 32;
                                                           env BATCH_K_REPS: windows per leg, default 7)
Per B three sets of sessions hold the same prompts, one per leg; the legs take turns window by window (the order rotates), so all
stand at the same positions throughout.  Reported per leg: the median aggregate tokens/s over its windows, the minimum and the
maximum, every window; and the ratios of the medians.  The chain's ids must equal the batched leg's (the same graph on the same
inputs); the one-by-one leg runs other kernels and is not compared.  No ratio is asserted: the file records what came out.
Writes profiles/batch_decode_7b_<type>.json and prints it."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

LEGS = ("batched", "one_by_one", "chain")


def main():
    from llm_amd import ggml, llama, synth
    args = sys.argv[1:]
    tname = args.pop(0).upper() if args and not args[0].isdigit() else "Q4_K"
    if tname not in ("Q2_K", "Q3_K", "Q4_K", "Q5_K", "Q6_K"):
        sys.exit("batch_decode_k.py: TYPE is one of Q2_K Q3_K Q4_K Q5_K Q6_K")
    counts = [int(a) for a in args] or [2, 4, 8]
    n = int(os.environ.get("BATCH_K_TOKENS", "32"))
    reps = int(os.environ.get("BATCH_K_REPS", "7"))
    L = ggml.lib()
    hp, w = synth.make_llama_fast(synth.LLAMA_7B, getattr(ggml, "TYPE_" + tname))
    model = llama.Llama(hp, w, context_size=2048)
    out = {"model": "LLaMA-7B %s (synthetic blocks)" % tname, "option": "plan_batch_k = 1", "positions_at_start": 128,
           "tokens_per_window": n, "windows_per_leg": reps, "runs": []}
    ggml.set_option("plan_batch_k", 1)
    try:
        for B in counts:
            sets = {}
            for leg in LEGS:
                sets[leg] = [model.start_session(n_batch=8) for _ in range(B)]
                for i, s in enumerate(sets[leg]):  # different prompts, slightly different lengths: a ragged batch
                    s.feed_prompt((np.arange(120 + i, dtype=np.int32) * (7 + i) + 5) % hp["n_vocab"])

            def window(leg, k):
                if leg == "chain":
                    ran, ids = model.infer_tokens_batch(sets[leg], k)
                    assert ran, "the backend declined the chain"
                    return ids
                rows = []
                for _ in range(k):
                    if leg == "batched":
                        ran, ids = model.infer_next_tokens_batch(sets[leg])
                        assert ran, "the backend declined the batched step"
                    else:
                        ids = np.array([s.infer_next_token() for s in sets[leg]], np.int32)
                    rows.append(ids)
                return np.stack(rows)

            for leg in LEGS:
                window(leg, 8)
            keys = ("batch_k_steps", "batch_chain_steps", "kplan_tokens", "graph_replays")
            rates = {leg: [] for leg in LEGS}
            c0 = [ggml.get_stat(k) for k in keys]
            for r in range(reps):
                ids = {}
                for j in range(len(LEGS)):
                    leg = LEGS[(r + j) % len(LEGS)]
                    L.ggml_hip_synchronize()
                    t0 = time.perf_counter()
                    ids[leg] = window(leg, n)
                    L.ggml_hip_synchronize()
                    rates[leg].append(B * n / (time.perf_counter() - t0))
                assert np.array_equal(ids["chain"], ids["batched"]), "the chain and the batched steps sampled different tokens"
            c1 = [ggml.get_stat(k) for k in keys]
            med = {leg: statistics.median(v) for leg, v in rates.items()}
            run = {"sessions": B}
            for leg in LEGS:
                run[leg] = {"aggregate_tokens_per_s": round(med[leg], 1), "min": round(min(rates[leg]), 1), "max": round(max(rates[leg]), 1),
                            "windows": [round(v, 1) for v in rates[leg]]}
            run["batched_vs_one_by_one"] = round(med["batched"] / med["one_by_one"], 3)
            run["chain_vs_one_by_one"] = round(med["chain"] / med["one_by_one"], 3)
            run["chain_vs_batched"] = round(med["chain"] / med["batched"], 3)
            run.update({k: b - a for k, a, b in zip(keys, c0, c1)})
            L.ggml_hip_timing_begin()  # the launches of ONE batched step by class (per-launch HIP events, launched eagerly for it)
            window("batched", 1)
            L.ggml_hip_timing_end()
            cls = {name: ggml.timing_query(k) for name, k in (("mmvq", ggml.KCLASS_MMVQ), ("attn", ggml.KCLASS_ATTN), ("other", ggml.KCLASS_OTHER))}
            run["batched_step_class_ms"] = {k: round(v[0], 4) for k, v in cls.items()}
            run["batched_step_class_launches"] = {k: int(v[1]) for k, v in cls.items()}
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
            for leg in sets:
                for s in sets[leg]:
                    s.free()
    finally:
        ggml.set_option("plan_batch_k", 0)
    model.free()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "batch_decode_7b_%s.json" % tname.lower()), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
