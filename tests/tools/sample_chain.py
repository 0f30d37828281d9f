#!/usr/bin/env python
"""One session's sampled chain (Session.infer_tokens_sampled_device -> ggml_hip_decode_sampled_chain: repetition penalty, top-k,
top-p, temperature, the draw and the next parameters on the device — k_sample_next — between two replays of the single-token plan)
against the same session stepped with Session.infer_next_token_sampled (one host round trip, the logits read back, a partial sort
and a graph built per token), with the greedy chain (Session.infer_tokens_device) as the ceiling, in one run: synthetic LLaMA-7B,
every session at about 128 positions, the reference's default sampler (k 40, top-p 0.95, temperature 0.8, penalty 1.30).
    python tests/tools/sample_chain.py [q4_0 q4_k]    (default both; env CHAIN_TOKENS: tokens per timed window, default 64;
                                                       env CHAIN_REPS: windows per leg, default 7)
Legs: (a) stepped, (b) chain, (c) greedy chain (Q4_0 only).  (a) and (b) are twin sessions with the same prompt and generator
state; the legs alternate window by window, so all stand at the same positions, and the ids and generator states of every pair of
windows of (a) and (b) must be equal.  A window of (b) or (c) starts behind another session's evaluation, so its first token is a
stepped one that arms the chain: what a caller pays who alternates sessions.  Reported: the median tokens/s of each leg over the
windows, all windows with their min and max, whether the median of (b) exceeds the median of (a) by more than (a)'s own min-max
spread, and the distance from (b) to (c) per token.  Writes profiles/sample_chain_7b_q4_0.json and prints it."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)


def main():
    names = sys.argv[1:] or ["q4_0", "q4_k"]
    n = int(os.environ.get("CHAIN_TOKENS", "64"))
    reps = int(os.environ.get("CHAIN_REPS", "7"))
    from llm_amd import ggml, llama, synth
    L = ggml.lib()
    wtypes = {"q4_0": ggml.TYPE_Q4_0, "q4_k": ggml.TYPE_Q4_K}
    out = {"positions_at_start": 128, "tokens_per_window": n, "windows_per_leg": reps,
           "sampler": {"k": 40, "top_p": 0.95, "temperature": 0.8, "penalty": 1.30}, "runs": []}
    for name in names:
        hp, w = synth.make_llama_fast(synth.LLAMA_7B, wtypes[name])
        model = llama.Llama(hp, w, context_size=2048)
        legs = ("stepped", "chain") + (("greedy_chain",) if name == "q4_0" else ())
        sess = {leg: model.start_session(n_batch=8) for leg in legs}
        for s in sess.values():
            s.feed_prompt((np.arange(120, dtype=np.int32) * 7 + 5) % hp["n_vocab"])
        rng = {leg: np.array([0x9E3779B97F4A7C15], dtype=np.uint64) for leg in legs}
        on_device = []

        def window(leg, k):
            if leg == "chain":
                on_dev, ids = sess[leg].infer_tokens_sampled_device(k, rng[leg])
                assert on_dev >= k - 1, "the backend declined the chain"
                on_device.append(on_dev)
                return ids
            if leg == "greedy_chain":
                return sess[leg].infer_tokens_device(k)
            return np.array([sess[leg].infer_next_token_sampled(rng[leg]) for _ in range(k)], np.int32)

        for leg in legs:
            window(leg, 8)
        del on_device[:]
        rates = {leg: [] for leg in legs}
        c0 = [ggml.get_stat(k) for k in ("sample_chain_tokens", "plan_tokens", "graph_replays")]
        for r in range(reps):
            ids = {}
            for leg in (legs if r % 2 == 0 else legs[::-1]):
                L.ggml_hip_synchronize()
                t0 = time.perf_counter()
                ids[leg] = window(leg, n)
                L.ggml_hip_synchronize()
                rates[leg].append(n / (time.perf_counter() - t0))
            assert np.array_equal(ids["chain"], ids["stepped"]), "the two legs sampled different tokens"
            assert np.array_equal(rng["chain"], rng["stepped"]), "the two legs left different generator states"
        c1 = [ggml.get_stat(k) for k in ("sample_chain_tokens", "plan_tokens", "graph_replays")]
        med = {leg: statistics.median(v) for leg, v in rates.items()}
        run = {"model": "LLaMA-7B %s (synthetic blocks)" % name.upper()}
        for leg in legs:
            run[leg] = {"tokens_per_s": round(med[leg], 1), "min": round(min(rates[leg]), 1), "max": round(max(rates[leg]), 1),
                        "windows": [round(v, 1) for v in rates[leg]]}
        spread = max(rates["stepped"]) - min(rates["stepped"])
        run["chain_minus_stepped_tokens_per_s"] = round(med["chain"] - med["stepped"], 1)
        run["stepped_min_max_spread_tokens_per_s"] = round(spread, 1)
        run["chain_exceeds_stepped_by_more_than_its_spread"] = bool(med["chain"] - med["stepped"] > spread)
        run["chain_vs_stepped"] = round(med["chain"] / med["stepped"], 4)
        if "greedy_chain" in med:  # the sampler's price per token: the distance to the ceiling
            run["chain_to_greedy_chain_us_per_token"] = round(1e6 / med["chain"] - 1e6 / med["greedy_chain"], 1)
        run["tokens_drawn_on_device_per_window"] = on_device
        run["sample_chain_tokens"], run["plan_tokens"], run["graph_replays"] = (b - a for a, b in zip(c0, c1))
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        for s in sess.values():
            s.free()
        model.free()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sample_chain_7b_q4_0.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
