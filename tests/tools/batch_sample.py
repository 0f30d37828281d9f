#!/usr/bin/env python
"""The sampled batched chain (Llama.infer_tokens_sampled_batch -> ggml_hip_decode_batch_sampled: repetition penalty, top-k, top-p,
temperature, the draw and the next parameters on the device, the step's graph replayed) against the same sessions stepped with
Llama.infer_next_tokens_sampled_batch (one host round trip, B rows of logits read back, B partial sorts and B graphs built per
step), in one run: synthetic LLaMA-7B Q4_0, every session at about 128 positions, the reference's default sampler
(k 40, top-p 0.95, temperature 0.8, penalty 1.30).
    python tests/tools/batch_sample.py [B ...]    (default 2 4 8; env CHAIN_TOKENS: tokens per session and timed window, default 64;
                                                   env CHAIN_REPS: windows per leg, default 7)
Per B two twin sets of sessions hold the same prompts and generator states; the legs alternate window by window, so both always
stand at the same positions, and the ids and generator states of every pair of windows must be equal.  Reported: the median
aggregate tokens/s of each leg over the windows, all windows, and the ratio of the medians.  Writes
profiles/batch_sample_7b_q4_0.json and prints it."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)


def main():
    counts = [int(a) for a in sys.argv[1:]] or [2, 4, 8]
    n = int(os.environ.get("CHAIN_TOKENS", "64"))
    reps = int(os.environ.get("CHAIN_REPS", "7"))
    from llm_amd import ggml, llama, synth
    L = ggml.lib()
    hp, w = synth.make_llama_fast(synth.LLAMA_7B, ggml.TYPE_Q4_0)
    model = llama.Llama(hp, w, context_size=2048)
    out = {"model": "LLaMA-7B Q4_0 (synthetic blocks)", "positions_at_start": 128, "tokens_per_window": n, "windows_per_leg": reps,
           "sampler": {"k": 40, "top_p": 0.95, "temperature": 0.8, "penalty": 1.30},
           "runs": []}
    for B in counts:
        sets = {}
        for leg in ("chain", "stepped"):
            sets[leg] = [model.start_session(n_batch=8) for _ in range(B)]
            for i, s in enumerate(sets[leg]):  # different prompts, slightly different lengths: a ragged batch
                s.feed_prompt((np.arange(120 + i, dtype=np.int32) * (7 + i) + 5) % hp["n_vocab"])

        rngs = {leg: (np.arange(B, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) for leg in sets}

        def window(leg, k):
            if leg == "chain":
                ran, ids = model.infer_tokens_sampled_batch(sets[leg], k, rngs[leg])
                assert ran, "the backend declined the chain"
                return ids
            rows = []
            for _ in range(k):
                ran, ids = model.infer_next_tokens_sampled_batch(sets[leg], rngs[leg])
                assert ran, "the backend declined the batched step"
                rows.append(ids)
            return np.stack(rows)

        for leg in ("chain", "stepped"):
            window(leg, 8)
        rates = {"chain": [], "stepped": []}
        c0 = [ggml.get_stat(k) for k in ("batch_sample_steps", "batch_decode_steps", "graph_replays")]
        for r in range(reps):
            ids = {}
            for leg in (("chain", "stepped") if r % 2 == 0 else ("stepped", "chain")):
                L.ggml_hip_synchronize()
                t0 = time.perf_counter()
                ids[leg] = window(leg, n)
                L.ggml_hip_synchronize()
                rates[leg].append(B * n / (time.perf_counter() - t0))
            assert np.array_equal(ids["chain"], ids["stepped"]), "the two legs sampled different tokens"
            assert np.array_equal(rngs["chain"], rngs["stepped"]), "the two legs left different generator states"
        c1 = [ggml.get_stat(k) for k in ("batch_sample_steps", "batch_decode_steps", "graph_replays")]
        med = {leg: statistics.median(v) for leg, v in rates.items()}
        run = {"sessions": B,
               "chain": {"aggregate_tokens_per_s": round(med["chain"], 1), "windows": [round(v, 1) for v in rates["chain"]]},
               "stepped": {"aggregate_tokens_per_s": round(med["stepped"], 1), "windows": [round(v, 1) for v in rates["stepped"]]},
               "chain_vs_stepped": round(med["chain"] / med["stepped"], 4),
               "batch_sample_steps": c1[0] - c0[0], "batch_decode_steps": c1[1] - c0[1], "graph_replays": c1[2] - c0[2]}
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        for leg in sets:
            for s in sets[leg]:
                s.free()
    model.free()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "batch_sample_7b_q4_0.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
