#!/usr/bin/env python
"""The sampled chains with the whole sampler (flat bias, frequency / presence penalty, tail-free, locally typical, top-p, min-p; or
Mirostat 2) against the stepped loop with the same sampler on the host, in tests/tools/sample_chain.py's protocol: synthetic LLaMA-7B
Q4_0, twin sessions with the same prompt and states at about 128 positions, windows of CHAIN_TOKENS (64) tokens, CHAIN_REPS (7)
windows per leg, the legs alternating window by window; the ids and states of every pair of windows must be equal.
    python tests/tools/sample_chain_ext.py [truncating mirostat default]      (default: the first two; `default` is the four-parameter
                                                                               chain through the same entries, for a kernel trace)
For each configuration: one session (Session.infer_tokens_sampled_device against infer_next_token_sampled) and B = 8
(Llama.infer_tokens_sampled_batch against infer_next_tokens_sampled_batch; aggregate tokens/s).  Reported per leg: the median with
min and max and all windows; chain / stepped as a ratio.  Prints the result as one JSON line; env SAMPLE_EXT_OUT names a file to
write it to as well (profiles/sampler_chain_ext.json was assembled from such files)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

CONFIGS = {
    "truncating": dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30, freq=0.3, presence=0.2, tail_free_z=0.9, typical_p=0.5, min_p=0.2,
                       bias=[(0, float("-inf")), (1, -1.5), (7, 3.0), (1000, 2.0), (31999, 2.5)]),
    "default": dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30),
    "mirostat": dict(k=40, top_p=1.0, temperature=0.8, penalty=1.30, mirostat=2, tau=5.0, eta=0.1, bias=[(0, float("-inf")), (1, -1.5)]),
}


def main():
    names = sys.argv[1:] or ["truncating", "mirostat"]
    n = int(os.environ.get("CHAIN_TOKENS", "64"))
    reps = int(os.environ.get("CHAIN_REPS", "7"))
    from llm_amd import ggml, llama, synth
    L = ggml.lib()
    hp, w = synth.make_llama_fast(synth.LLAMA_7B, ggml.TYPE_Q4_0)
    model = llama.Llama(hp, w, context_size=2048)
    out = {"model": "LLaMA-7B Q4_0 (synthetic blocks)", "positions_at_start": 128, "tokens_per_window": n, "windows_per_leg": reps, "runs": []}
    for name in names:
        kw = CONFIGS[name]
        miro = kw.get("mirostat", 0) == 2
        for B in (1, 8):
            legs = ("stepped", "chain")
            sess = {leg: [model.start_session(n_batch=8) for _ in range(B)] for leg in legs}
            for ss in sess.values():
                for c, s in enumerate(ss):
                    s.feed_prompt((np.arange(120, dtype=np.int32) * 7 + 5 + c) % hp["n_vocab"])
            rng = {leg: (np.arange(B, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567)).astype(np.uint64) for leg in legs}
            mu = {leg: (np.full(B, 2 * kw["tau"], np.float32) if miro else None) for leg in legs}

            def window(leg, k):
                ss, r, m = sess[leg], rng[leg], mu[leg]
                if B == 1:
                    if leg == "chain":
                        on_dev, ids = ss[0].infer_tokens_sampled_device(k, r, mu=m, **kw)
                        assert on_dev >= k - 1, "the backend declined the chain"
                        return ids
                    return np.array([ss[0].infer_next_token_sampled(r, mu=m, **kw) for _ in range(k)], np.int32)
                if leg == "chain":
                    ran, ids = model.infer_tokens_sampled_batch(ss, k, r, mu=m, **kw)
                    assert ran, "the backend declined the chain"
                    return ids
                return np.stack([model.infer_next_tokens_sampled_batch(ss, r, mu=m, **kw)[1] for _ in range(k)])

            for leg in legs:
                window(leg, 8)
            rates = {leg: [] for leg in legs}
            for r in range(reps):
                ids = {}
                for leg in (legs if r % 2 == 0 else legs[::-1]):
                    L.ggml_hip_synchronize()
                    t0 = time.perf_counter()
                    ids[leg] = window(leg, n)
                    L.ggml_hip_synchronize()
                    rates[leg].append(n * B / (time.perf_counter() - t0))
                assert np.array_equal(ids["chain"], ids["stepped"]), "the two legs sampled different tokens"
                assert np.array_equal(rng["chain"], rng["stepped"]), "the two legs left different generator states"
                assert not miro or np.array_equal(mu["chain"].view(np.uint32), mu["stepped"].view(np.uint32)), "the two legs left different mu"
            med = {leg: statistics.median(v) for leg, v in rates.items()}
            run = {"sampler": name, "sessions": B}
            for leg in legs:
                run[leg] = {"tokens_per_s": round(med[leg], 1), "min": round(min(rates[leg]), 1), "max": round(max(rates[leg]), 1),
                            "windows": [round(v, 1) for v in rates[leg]]}
            run["chain_vs_stepped"] = round(med["chain"] / med["stepped"], 4)
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
            for ss in sess.values():
                for s in ss:
                    s.free()
    model.free()
    path = os.environ.get("SAMPLE_EXT_OUT")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
