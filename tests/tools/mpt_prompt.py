"""Prompt rate of MPT-7B on the MPT prompt plan (backend option plan_mpt_prompt) against the node-by-node executor: Q4_0 random blocks
(rotary_decode.fast_weights), one MI355X, through Mpt.feed_prompt.  Prompts of 64, 512 and 2 x 512 tokens (the second batch at n_past 512);
option 1 against option 0, `--runs` alternating runs each after one untimed run of either, median and min-max of the runs' prompt tokens/s,
and whether the plan's median is above the executor's by more than the executor's own min-max spread.  Prints one JSON line (profiles/mpt_prompt.json).
    python tests/tools/mpt_prompt.py [--runs 5] [--layers 32]"""
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


def _feed(model, toks):
    model.n_past = 0
    t0 = time.perf_counter()
    model.feed_prompt(toks, n_batch=512)
    return len(toks) / (time.perf_counter() - t0)


def _stats(v):
    return {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1), "runs": [round(x, 1) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--layers", type=int, default=mpt.MPT_7B["n_layer"])
    a = ap.parse_args()
    if not ggml.has_gpu():
        raise SystemExit("mpt_prompt: no HIP device visible")
    hp = dict(mpt.MPT_7B, n_layer=a.layers, wtype=ggml.TYPE_Q4_0)
    w = fast_weights(mpt, hp, hp["wtype"])
    model = mpt.Mpt(hp, w, n_ctx=1024)
    del w
    out = {"model": "mpt_7b", "n_layer": hp["n_layer"], "wtype": "q4_0", "runs": a.runs, "prompt_tokens_per_s": {}}
    m0, g0 = ggml.get_stat("mpt_prompt_tokens"), ggml.get_stat("generic_graphs")
    try:
        for n in (64, 512, 1024):
            toks = np.random.default_rng(n).integers(0, hp["n_vocab"], n).astype(np.int32)
            rate = {0: [], 1: []}
            for run in range(a.runs + 1):
                for on in (0, 1):
                    ggml.set_option("plan_mpt_prompt", on)
                    r = _feed(model, toks)
                    if run:  # (the first run of either: plans built, f16 copies made)
                        rate[on].append(r)
            ex, pl = _stats(rate[0]), _stats(rate[1])
            out["prompt_tokens_per_s"][str(n)] = {"executor": ex, "plan": pl,
                                                  "plan_above_executor_by_more_than_its_spread": pl["median"] - ex["median"] > ex["max"] - ex["min"]}
        out["mpt_prompt_tokens"] = ggml.get_stat("mpt_prompt_tokens") - m0
        out["generic_graphs"] = ggml.get_stat("generic_graphs") - g0
        out["device"] = ggml.lib().ggml_hip_version().decode()
    finally:
        ggml.set_option("plan_mpt_prompt", 0)
        model.free()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
