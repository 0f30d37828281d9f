"""Prompt rate of MPT-7B on the MPT chunk plan (backend option plan_mpt_chunk) against the node-by-node executor: Q4_0 random blocks
(rotary_decode.fast_weights), one MI355X, through Mpt.feed_prompt at n_batch 8 and 16 — 512 tokens from position 0, and 128 tokens at
n_batch 8 behind a prefix of 1024, 2048 and 4096 positions (n_ctx 8192, the prefix fed once by the MPT prompt plan).  Option 1 against
option 0, `--runs` alternating runs each after one untimed run of either; median and min-max of the runs' prompt tokens/s, the Python
graph build included, and whether the plan's median is above the executor's by more than the executor's own min-max spread.  Prints one
JSON line (profiles/mpt_chunk.json).
    python tests/tools/mpt_chunk.py [--runs 5] [--layers 32]"""
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
from mpt_prompt import _stats  # noqa: E402
from rotary_decode import fast_weights  # noqa: E402


def _feed(model, toks, n_batch, at):
    model.n_past = at
    t0 = time.perf_counter()
    model.feed_prompt(toks, n_batch=n_batch)
    return len(toks) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--layers", type=int, default=mpt.MPT_7B["n_layer"])
    a = ap.parse_args()
    if not ggml.has_gpu():
        raise SystemExit("mpt_chunk: no HIP device visible")
    hp = dict(mpt.MPT_7B, n_layer=a.layers, wtype=ggml.TYPE_Q4_0)
    w = fast_weights(mpt, hp, hp["wtype"])
    model = mpt.Mpt(hp, w, n_ctx=8192)
    del w
    out = {"model": "mpt_7b", "n_layer": hp["n_layer"], "wtype": "q4_0", "runs": a.runs, "prompt_tokens_per_s": {}}
    c0, g0 = ggml.get_stat("mpt_chunk_tokens"), ggml.get_stat("generic_graphs")
    rng = np.random.default_rng(1)
    try:
        fed = 0
        for at, n, n_batch in ((0, 512, 8), (0, 512, 16), (1024, 128, 8), (2048, 128, 8), (4096, 128, 8)):
            if at > fed:  # the prefix, once: the chunks behind it overwrite only their own rows
                ggml.set_option("plan_mpt_prompt", 1)
                _feed(model, rng.integers(0, hp["n_vocab"], at - fed).astype(np.int32), 512, fed)
                ggml.set_option("plan_mpt_prompt", 0)
                fed = at
            toks = rng.integers(0, hp["n_vocab"], n).astype(np.int32)
            rate = {0: [], 1: []}
            for run in range(a.runs + 1):
                for on in (0, 1):
                    ggml.set_option("plan_mpt_chunk", on)
                    r = _feed(model, toks, n_batch, at)
                    if run:  # (the first run of either: plans built)
                        rate[on].append(r)
            ex, pl = _stats(rate[0]), _stats(rate[1])
            out["prompt_tokens_per_s"][f"at{at}_n{n}_batch{n_batch}"] = {
                "executor": ex, "plan": pl, "plan_above_executor_by_more_than_its_spread": pl["median"] - ex["median"] > ex["max"] - ex["min"]}
            print(json.dumps({f"at{at}_batch{n_batch}": [ex, pl]}), file=sys.stderr, flush=True)
        out["mpt_chunk_tokens"] = ggml.get_stat("mpt_chunk_tokens") - c0
        out["generic_graphs"] = ggml.get_stat("generic_graphs") - g0
        out["device"] = ggml.lib().ggml_hip_version().decode()
    finally:
        ggml.set_option("plan_mpt_chunk", 0)
        ggml.set_option("plan_mpt_prompt", 0)
        model.free()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
