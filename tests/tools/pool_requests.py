#!/usr/bin/env python
"""The request pool (Llama.infer_until_pool) beside what a caller with more requests than columns had before, in
tests/tools/chain_requests.py's protocol: synthetic LLaMA-7B Q4_0 at context 512, N = 32 and 64 sessions (0.27 GB of K/V each) behind
prompts of 120 tokens fed outside the timed part, every request the default sampler with one stop id that is never drawn and a budget
of 32 * (1 + i mod 8) tokens, 8 columns.  Legs, alternating (the order reversed every other round), every leg and round on fresh
sessions:
  pool     Llama.infer_until_pool: ended columns take waiting requests on the device.
  waves    the requests in waves of 8 in the given order through Llama.infer_until_batch: an ended column is frozen until its wave's
           longest request ends.
  stepped  Llama.infer_until_pool with option plan_batch_pool = 0: the stepped loop under the same admission rule.
    python tests/tools/pool_requests.py            (env POOL_N = "32,64", POOL_REPS = 3, POOL_OUT = a file to write the JSON to)
Reported per N and leg: useful tokens/s (evaluations over wall time) as the median with min and max and all rounds, the batched steps
the leg launched, and for the pool its steps_run (counter pool_steps) beside llm_pool_schedule's count for the budgets; and the ratio
of the pool's median to the waves' median and maximum.  A round in which a request drew the stop id is reported short."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

DEFAULT = dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30)
NEVER = 3
COLS = 8


def summary(v):
    return {"tokens_per_s": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1), "rounds": [round(x, 1) for x in v]}


def main():
    sizes = [int(x) for x in os.environ.get("POOL_N", "32,64").split(",")]
    reps = int(os.environ.get("POOL_REPS", "3"))
    from llm_amd import ggml, llama, synth
    L = ggml.lib()
    hp, w = synth.make_llama_fast(synth.LLAMA_7B, ggml.TYPE_Q4_0)
    V = hp["n_vocab"]
    model = llama.Llama(hp, w, context_size=512)
    out = {"model": "LLaMA-7B Q4_0 (synthetic blocks)", "context": 512, "prompt_tokens": 120, "columns": COLS, "rounds_per_leg": reps, "sizes": {}}

    def stat(k):
        return int(L.ggml_hip_get_stat(k.encode()))

    def sessions(N):
        ss = [model.start_session(n_batch=8) for _ in range(N)]
        for c, s in enumerate(ss):
            s.feed_prompt((np.arange(120, dtype=np.int32) * 7 + 5 + c) % V)
        return ss

    def rngs(N):
        return (np.arange(N, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567)).astype(np.uint64)

    def pool(ss, reqs, rr):
        ids, counts, why, ran = model.infer_until_pool(ss, reqs, rr, max_cols=COLS)
        assert ran, "the backend declined the pool"
        return int(counts.sum())

    def waves(ss, reqs, rr):
        got = 0
        for a in range(0, len(ss), COLS):
            r8 = np.ascontiguousarray(rr[a:a + COLS])
            ids, counts, why, ran = model.infer_until_batch(ss[a:a + COLS], reqs[a:a + COLS], r8)
            assert ran, "the backend declined the chain"
            got += int(counts.sum())
        return got

    def stepped(ss, reqs, rr):
        ggml.set_option("plan_batch_pool", 0)
        try:
            ids, counts, why, ran = model.infer_until_pool(ss, reqs, rr, max_cols=COLS)
        finally:
            ggml.set_option("plan_batch_pool", 1)
        assert not ran
        return int(counts.sum())

    legs = {"pool": pool, "waves": waves, "stepped": stepped}
    warm = sessions(COLS)  # the batched plan and its graph, the pool's tables: built outside the timed part
    pool(warm, [dict(max_tokens=4, stop=[NEVER], sampler=DEFAULT)] * COLS, rngs(COLS))
    for s in warm:
        s.free()
    for N in sizes:
        budgets = [32 * (1 + i % 8) for i in range(N)]
        reqs = [dict(max_tokens=b, stop=[NEVER], sampler=DEFAULT) for b in budgets]
        e = np.array(budgets, np.int32)
        res = {"requests": N, "evaluations": int(sum(budgets)), "steps_by_the_rule": int(llama._lib().llm_pool_schedule(e.ctypes.data, N, COLS, None, None)),
               "steps_in_waves": int(sum(max(budgets[a:a + COLS]) for a in range(0, N, COLS)))}
        rates, steps, short = {k: [] for k in legs}, {}, {}
        for r in range(reps):
            for name in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                ss, rr = sessions(N), rngs(N)
                s0 = (stat("batch_decode_steps"), stat("pool_steps"))
                L.ggml_hip_synchronize()
                t0 = time.perf_counter()
                got = legs[name](ss, reqs, rr)
                L.ggml_hip_synchronize()
                rates[name].append(got / (time.perf_counter() - t0))
                steps[name] = {"batched_steps_launched": stat("batch_decode_steps") - s0[0]}
                if name == "pool":
                    steps[name]["steps_run"] = stat("pool_steps") - s0[1]
                if got != sum(budgets):
                    short[name] = short.get(name, 0) + 1
                for s in ss:
                    s.free()
        for name in legs:
            res[name] = dict(summary(rates[name]), **steps[name])
            if name in short:
                res[name]["rounds_cut_short_by_the_stop_id"] = short[name]
        res["pool_over_waves_median"] = round(res["pool"]["tokens_per_s"] / res["waves"]["tokens_per_s"], 3)
        res["pool_median_over_waves_max"] = round(res["pool"]["tokens_per_s"] / res["waves"]["max"], 3)
        res["pool_over_stepped_median"] = round(res["pool"]["tokens_per_s"] / res["stepped"]["tokens_per_s"], 3)
        out["sizes"][str(N)] = res
        print(json.dumps({str(N): res}), flush=True)
    model.free()
    path = os.environ.get("POOL_OUT")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
