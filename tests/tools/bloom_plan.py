"""Decode rate of BLOOM on the BLOOM plan (backend option plan_bloom) against the node-by-node executor: full depth, the full 250 880-entry
vocabulary, Q4_0 random blocks (rotary_decode.fast_weights), a 128-token prompt (4 chunks of 32), batch 1.  Three forms, `--runs` alternating
runs of `--steps` timed tokens each (median and min-max of the runs' tokens/s):
  a  evaluate + argmax on the executor (plan_bloom = 0)
  b  the same loop with plan_bloom = 1                           every token's graph is still built in Python; the plan runs it
  c  Bloom.infer_tokens_device                                   one graph, then the greedy chain on the device
and of form b: the launches per token and the per-launch device time of the five layer launches, the embedding launch and the lm_head
(ggml_hip_bench_plan_class: one kind or class replayed alone) with the lm_head's share of a token's device time.  Prints one JSON line.
    python tests/tools/bloom_plan.py [--model 7b1|560m] [--steps 16] [--warmup 4] [--runs 5] [--layers N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from llm_amd import bloom, ggml  # noqa: E402
from rotary_decode import fast_weights  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X
MODELS = {"7b1": bloom.BLOOM_7B1, "560m": bloom.BLOOM_560M}


def _loop(model, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        model.evaluate(np.array([int(np.argmax(model.last_logits))], np.int32))
    return steps / (time.perf_counter() - t0)


def _chain(model, steps):
    t0 = time.perf_counter()
    model.infer_tokens_device(steps)
    return steps / (time.perf_counter() - t0)


def _stats(v):
    return {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1), "runs": [round(x, 1) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=list(MODELS), default="7b1")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--layers", type=int, default=0)
    a = ap.parse_args()
    if not ggml.has_gpu():
        raise SystemExit("bloom_plan: no HIP device visible")
    prompt = 128
    hp = dict(MODELS[a.model], wtype=ggml.TYPE_Q4_0)
    hp["n_layer"] = a.layers or hp["n_layer"]
    w = fast_weights(bloom, hp, hp["wtype"])
    model = bloom.Bloom(hp, w, n_ctx=prompt + 3 * a.runs * (a.steps + a.warmup) + 64)
    del w
    toks = np.random.default_rng(1).integers(0, hp["n_vocab"], prompt).astype(np.int32)
    for c in range(0, prompt, 32):
        model.evaluate(toks[c:c + 32])
    rate = {"a": [], "b": [], "c": []}
    m0, g0 = ggml.get_stat("bloom_plan_tokens"), ggml.get_stat("generic_graphs")
    try:
        for _ in range(a.runs):
            for form in "abc":
                ggml.set_option("plan_bloom", 0 if form == "a" else 1)
                run = _chain if form == "c" else _loop
                run(model, a.warmup)
                rate[form].append(run(model, a.steps))
        out = {"model": "bloom_" + a.model, "n_layer": hp["n_layer"], "n_vocab": hp["n_vocab"], "wtype": "q4_0", "prompt": prompt, "steps": a.steps,
               "runs": a.runs, "tokens_per_s": {k: _stats(v) for k, v in rate.items()},
               "bloom_plan_tokens": ggml.get_stat("bloom_plan_tokens") - m0, "generic_graphs": ggml.get_stat("generic_graphs") - g0}
        ta, tb, tc = (out["tokens_per_s"][k] for k in "abc")
        spread = lambda t: t["max"] - t["min"]
        out["b_above_a_by_more_than_both_spreads"] = tb["median"] - ta["median"] > max(spread(ta), spread(tb))
        out["c_above_a_by_more_than_both_spreads"] = tc["median"] - ta["median"] > max(spread(ta), spread(tc))
        ggml.set_option("plan_bloom", 1)
        model.evaluate(np.array([int(np.argmax(model.last_logits))], np.int32))  # (the plan the legs below replay)
        reps, legs = 20, {}
        for name, k in (("qkv_ln_bias_store", ggml.KKIND_BASE + 0), ("wo_bias_add", ggml.KKIND_BASE + 1), ("w1_ln_bias_gelu", ggml.KKIND_BASE + 2),
                        ("w2_bias_add", ggml.KKIND_BASE + 3), ("lm_head_ln", ggml.KKIND_BASE + 4), ("attention", ggml.KCLASS_ATTN),
                        ("get_rows_lnorm", ggml.KCLASS_OTHER)):
            ms, launches, nbytes = ggml.bench_plan_class(k, reps)
            per = ms / reps / max(launches, 1)
            legs[name] = {"launches_per_token": launches, "us_per_launch": round(per * 1e3, 2),
                          "hbm_fraction": round(nbytes / max(launches, 1) / (per * 1e-3) / HBM_PEAK, 3) if per > 0 else None}
        out["launches"] = legs
        out["launches_per_token"] = sum(v["launches_per_token"] for v in legs.values())
        dev_us = sum(v["launches_per_token"] * v["us_per_launch"] for v in legs.values())
        out["lm_head_share_of_device_time"] = round(legs["lm_head_ln"]["us_per_launch"] / dev_us, 3) if dev_us > 0 else None
        out["device"] = ggml.lib().ggml_hip_version().decode()
    finally:
        ggml.set_option("plan_bloom", 0)
        model.free()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
