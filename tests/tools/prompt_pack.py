#!/usr/bin/env python
"""The packed prompt feed (Llama.feed_prompt_batch, ggml_hip_prompt_pack) beside feeding the same sessions one by one, in
tests/tools/pool_requests.py's protocol: synthetic LLaMA-7B Q4_0, B = 8, 32 and 64 sessions with prompts of 16, 64 and 128 tokens each.
Context 1024, not 2048: a session holds its K/V (0.5 GB here) and 3 GB of arena shadows on the device, and 68 of them beside the model
and its f16 copies are what 288 GB take.  Legs, alternating (the order reversed every other round), every leg on sessions rewound to position 0:
  packed_512 / packed_1024 / packed_2048   Llama.feed_prompt_batch with that max_rows.
  one_by_one_nb8                           Session.feed_prompt, session after session, at the reference's default n_batch = 8.
  one_by_one_nb512                         the same at n_batch = 512 (every prompt here is one evaluation), on FOUR sessions of that
                                           n_batch taken in turn (memory, above): the same launches, caches that are warmer if anything.
Then the pool's own workload end to end: 64 requests with budgets 32 * (1 + i mod 8), prompts of 64 tokens, feed + infer_until_pool over
8 columns, with the packed feed and with the one-by-one feed at n_batch = 8.
    python tests/tools/prompt_pack.py      (env PACK_B = "8,32,64", PACK_LEN = "16,64,128", PACK_REPS = 5, PACK_E2E_REPS = 3,
                                            PACK_OUT = a file to write the JSON to)
Reported per point and leg: prompt tokens/s (tokens over wall time, device synchronised) as the median with min and max and all rounds;
per point the ratio of each packed leg's median to the better one-by-one leg's median, and whether the packed leg lies below that leg's
minimum (slower by more than its own spread)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

DEFAULT = dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30)
NEVER, COLS, CTX = 3, 8, 1024


def summary(v):
    return {"tokens_per_s": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1), "rounds": [round(x, 1) for x in v]}


def main():
    sizes = [int(x) for x in os.environ.get("PACK_B", "8,32,64").split(",")]
    lens = [int(x) for x in os.environ.get("PACK_LEN", "16,64,128").split(",")]
    reps, e2e_reps = int(os.environ.get("PACK_REPS", "5")), int(os.environ.get("PACK_E2E_REPS", "3"))
    from llm_amd import ggml, llama, synth
    L = ggml.lib()
    hp, w = synth.make_llama_fast(synth.LLAMA_7B, ggml.TYPE_Q4_0)
    V = hp["n_vocab"]
    model = llama.Llama(hp, w, context_size=CTX)
    out = {"model": "LLaMA-7B Q4_0 (synthetic blocks)", "context": CTX, "rounds_per_leg": reps, "points": {}}
    Bmax = max(sizes + [64])
    set8 = [model.start_session(n_batch=8) for _ in range(Bmax)]
    set512 = [model.start_session(n_batch=512) for _ in range(4)]

    def stat(k):
        return int(L.ggml_hip_get_stat(k.encode()))

    def prompts(B, n):
        return [((np.arange(n, dtype=np.int32) * 7 + 5 + c) % V).astype(np.int32) for c in range(B)]

    def rewind(ss):
        for s in ss:
            s.seek(0)

    def packed(max_rows):
        def run(B, pr):
            rewind(set8[:B])  # (n_batch is not consulted)
            c0 = stat("prompt_pack_calls")
            assert model.feed_prompt_batch(set8[:B], pr, max_rows=max_rows) == 1, "the backend declined a round"
            return stat("prompt_pack_calls") - c0
        return run

    def one_by_one(ss):
        def run(B, pr):
            for c, p in enumerate(pr):
                s = ss[c % len(ss)]
                s.seek(0)
                s.feed_prompt(p)
            return B
        return run

    legs = {"packed_512": packed(512), "packed_1024": packed(1024), "packed_2048": packed(2048), "one_by_one_nb8": one_by_one(set8),
            "one_by_one_nb512": one_by_one(set512)}
    for name, leg in legs.items():  # plans, f16 copies of the weights, workspace: built outside the timed part
        leg(8, prompts(8, 64))
    for B in sizes:
        for n in lens:
            pr = prompts(B, n)
            rates, calls = {k: [] for k in legs}, {}
            for name, leg in legs.items():  # this point's plans
                leg(B, pr)
            for r in range(reps):
                for name in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                    L.ggml_hip_synchronize()
                    t0 = time.perf_counter()
                    calls[name] = legs[name](B, pr)
                    L.ggml_hip_synchronize()
                    rates[name].append(B * n / (time.perf_counter() - t0))
            res = {"sessions": B, "prompt_tokens": n, "rows": B * n}
            for name in legs:
                res[name] = dict(summary(rates[name]), evaluations=calls[name])
            best = max(("one_by_one_nb8", "one_by_one_nb512"), key=lambda k: res[k]["tokens_per_s"])
            res["better_one_by_one"] = best
            for name in ("packed_512", "packed_1024", "packed_2048"):
                res[name]["over_better_one_by_one"] = round(res[name]["tokens_per_s"] / res[best]["tokens_per_s"], 3)
                res[name]["below_its_min"] = bool(res[name]["tokens_per_s"] < res[best]["min"])
            out["points"]["B%d_n%d" % (B, n)] = res
            print(json.dumps({"B%d_n%d" % (B, n): res}), flush=True)
    # ---- the pool's workload end to end: feed + infer_until_pool
    N, n = 64, 64
    budgets = [32 * (1 + i % 8) for i in range(N)]
    reqs = [dict(max_tokens=b, stop=[NEVER], sampler=DEFAULT) for b in budgets]
    pr = prompts(N, n)

    def rngs():
        return (np.arange(N, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567)).astype(np.uint64)

    def e2e(feed):
        rewind(set8[:N])
        L.ggml_hip_synchronize()
        t0 = time.perf_counter()
        if feed == "packed":
            assert model.feed_prompt_batch(set8[:N], pr, max_rows=512) == 1
        else:
            for s, p in zip(set8[:N], pr):
                s.feed_prompt(p)
        L.ggml_hip_synchronize()
        t1 = time.perf_counter()
        ids, counts, why, ran = model.infer_until_pool(set8[:N], reqs, rngs(), max_cols=COLS)
        L.ggml_hip_synchronize()
        t2 = time.perf_counter()
        assert ran, "the backend declined the pool"
        return t1 - t0, t2 - t0, int(counts.sum())

    e2e("packed")
    walls = {"packed": [], "one_by_one_nb8": []}
    for r in range(e2e_reps):
        for feed in (list(walls) if r % 2 == 0 else list(walls)[::-1]):
            walls[feed].append(e2e(feed))
    res = {"requests": N, "prompt_tokens": n, "budgets": "32 * (1 + i mod 8)", "columns": COLS, "rounds_per_leg": e2e_reps}
    for feed, v in walls.items():
        res[feed] = {"feed_s": round(statistics.median(x[0] for x in v), 4), "total_s": round(statistics.median(x[1] for x in v), 4),
                     "total_s_min": round(min(x[1] for x in v), 4), "total_s_max": round(max(x[1] for x in v), 4),
                     "generated_tokens": v[0][2], "rounds": [[round(x[0], 4), round(x[1], 4)] for x in v]}
    res["total_packed_over_one_by_one"] = round(res["packed"]["total_s"] / res["one_by_one_nb8"]["total_s"], 3)
    out["end_to_end"] = res
    print(json.dumps({"end_to_end": res}), flush=True)
    for s in set8 + set512:
        s.free()
    model.free()
    path = os.environ.get("PACK_OUT")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
