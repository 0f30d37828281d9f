"""Decode rate of MPT-7B on the MPT plan (backend option plan_mpt) against the node-by-node executor: full depth, Q4_0 random blocks
(rotary_decode.fast_weights), a 128-token prompt (4 chunks of 32), batch 1.  Three forms, `--runs` alternating runs of `--steps` timed
tokens each (median and min-max of the runs' tokens/s):
  a  evaluate + argmax on the executor (plan_mpt = 0)            what tests/tools/alibi_decode.py measures
  b  the same loop with plan_mpt = 1                             every token's graph is still built in Python; the plan runs it
  c  Mpt.infer_tokens_device                                     one graph, then the greedy chain on the device
and of form b: the share of a token that is the Python graph build (time outside ggml_graph_compute), the launches per token and the
per-launch device time of the five layer launches and the lm_head (ggml_hip_bench_plan_class: one kind or class replayed alone) with
the fraction of the HBM peak their algorithmic bytes make.  Prints one JSON line.
    python tests/tools/mpt_plan.py [--steps 16] [--warmup 4] [--runs 5] [--layers 32]"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from llm_amd import ggml, mpt  # noqa: E402
from rotary_decode import fast_weights  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X


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
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--layers", type=int, default=mpt.MPT_7B["n_layer"])
    a = ap.parse_args()
    if not ggml.has_gpu():
        raise SystemExit("mpt_plan: no HIP device visible")
    prompt = 128
    hp = dict(mpt.MPT_7B, n_layer=a.layers, wtype=ggml.TYPE_Q4_0)
    w = fast_weights(mpt, hp, hp["wtype"])
    model = mpt.Mpt(hp, w, n_ctx=prompt + 3 * a.runs * (a.steps + a.warmup) + 64)
    del w
    toks = np.random.default_rng(1).integers(0, hp["n_vocab"], prompt).astype(np.int32)
    for c in range(0, prompt, 32):
        model.evaluate(toks[c:c + 32])
    rate = {"a": [], "b": [], "c": []}
    m0, g0 = ggml.get_stat("mpt_plan_tokens"), ggml.get_stat("generic_graphs")
    try:
        for _ in range(a.runs):
            for form in "abc":
                ggml.set_option("plan_mpt", 0 if form == "a" else 1)
                run = _chain if form == "c" else _loop
                run(model, a.warmup)
                rate[form].append(run(model, a.steps))
        out = {"model": "mpt_7b", "n_layer": hp["n_layer"], "wtype": "q4_0", "prompt": prompt, "steps": a.steps, "runs": a.runs,
               "tokens_per_s": {k: _stats(v) for k, v in rate.items()},
               "mpt_plan_tokens": ggml.get_stat("mpt_plan_tokens") - m0, "generic_graphs": ggml.get_stat("generic_graphs") - g0}
        ta, tb, tc = (out["tokens_per_s"][k] for k in "abc")
        out["b_above_a_by_more_than_a_spread"] = tb["median"] - ta["median"] > ta["max"] - ta["min"]
        out["c_above_b_by_more_than_b_spread"] = tc["median"] - tb["median"] > tb["max"] - tb["min"]
        # form b: where a token's time goes
        ggml.set_option("plan_mpt", 1)
        c0, n = ggml.get_stat("ns_compute"), 8
        t0 = time.perf_counter()
        for _ in range(n):
            model.evaluate(np.array([int(np.argmax(model.last_logits))], np.int32))
        wall = (time.perf_counter() - t0) / n
        comp = (ggml.get_stat("ns_compute") - c0) * 1e-9 / n
        out["form_b_ms_per_token"] = {"wall": round(wall * 1e3, 3), "inside_graph_compute": round(comp * 1e3, 3),
                                      "python_graph_build_share": round(1.0 - comp / wall, 3)}
        reps = 20
        legs = {}
        for name, k in (("wqkv_ln_store", ggml.KKIND_BASE + 0), ("out_proj_add", ggml.KKIND_BASE + 1), ("up_proj_ln_gelu", ggml.KKIND_BASE + 2),
                        ("down_proj_add", ggml.KKIND_BASE + 3), ("lm_head_ln", ggml.KKIND_BASE + 4), ("attention", ggml.KCLASS_ATTN),
                        ("get_rows", ggml.KCLASS_OTHER)):
            ms, launches, nbytes = ggml.bench_plan_class(k, reps)
            per = ms / reps / max(launches, 1)
            legs[name] = {"launches_per_token": launches, "us_per_launch": round(per * 1e3, 2),
                          "hbm_fraction": round(nbytes / max(launches, 1) / (per * 1e-3) / HBM_PEAK, 3) if per > 0 else None}
        out["launches"] = legs
        out["launches_per_token"] = sum(v["launches_per_token"] for v in legs.values())
        out["device"] = ggml.lib().ggml_hip_version().decode()
    finally:
        ggml.set_option("plan_mpt", 0)
        model.free()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
