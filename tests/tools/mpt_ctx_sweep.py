"""Decode speed of MPT-7B on the MPT plan (backend option plan_mpt = 1) by context length: k_attn_decode_alibi, one workgroup per head
(option attn_split = 0), against the three position-split launches (attn_split = 2: split from two positions on, i.e. everywhere).  Q4_0
random blocks (rotary_decode.fast_weights), one MI355X, n_ctx 8192; every context is reached by Mpt.feed_prompt on the MPT prompt plan
(plan_mpt_prompt = 1), then Mpt.infer_tokens_device(16) — one evaluation and the greedy chain behind it — is timed from the same position
under either option, `--runs` alternating runs, each behind one untimed call of the same kind (setting attn_split drops the plans: the
untimed call builds the plan and captures its graphs).  The timed tokens are few (16, some 20 ms): the spread says what that costs.
Per context: median and min - max tokens/s of both forms and whether the split form's median is above the other's by more than the other's
own spread; `threshold`: the smallest swept context from which that holds at every longer one (null: at none).  The default threshold of
the MPT plan (ATTN_SPLIT_MIN_MPT, kernels/decode_attn_split.h) is read off this.  Prints one JSON line (profiles/mpt_ctx_sweep.json).
    python tests/tools/mpt_ctx_sweep.py [--runs 5] [--layers 32] [--contexts 256,512,1024,2048,4096,8000]"""
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

STEPS, N_CTX = 16, 8192


def _decode(model, ctx, logits):
    """tokens/s of infer_tokens_device(STEPS) from position ctx on"""
    model.n_past, model.last_logits = ctx, logits
    t0 = time.perf_counter()
    model.infer_tokens_device(STEPS)
    return STEPS / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--layers", type=int, default=mpt.MPT_7B["n_layer"])
    ap.add_argument("--contexts", default="256,512,1024,2048,4096,8000")
    a = ap.parse_args()
    if not ggml.has_gpu():
        raise SystemExit("mpt_ctx_sweep: no HIP device visible")
    contexts = sorted(int(c) for c in a.contexts.split(","))
    if contexts[-1] + 2 * STEPS > N_CTX:
        raise SystemExit("mpt_ctx_sweep: contexts up to %d" % (N_CTX - 2 * STEPS))
    hp = dict(mpt.MPT_7B, n_layer=a.layers, wtype=ggml.TYPE_Q4_0)
    w = fast_weights(mpt, hp, hp["wtype"])
    model = mpt.Mpt(hp, w, n_ctx=N_CTX)
    del w
    out = {"model": "mpt_7b", "n_layer": hp["n_layer"], "wtype": "q4_0", "n_ctx": N_CTX, "steps": STEPS, "runs": a.runs, "contexts": {}}
    names = ("mpt_plan_tokens", "mpt_split_tokens", "mpt_prompt_tokens", "generic_graphs")
    s0 = [ggml.get_stat(k) for k in names]
    try:
        ggml.set_option("plan_mpt", 1)
        ggml.set_option("plan_mpt_prompt", 1)
        toks = np.random.default_rng(N_CTX).integers(0, hp["n_vocab"], contexts[-1]).astype(np.int32)
        model.n_past = 0
        for ctx in contexts:
            logits = model.feed_prompt(toks[model.n_past:ctx]).copy()  # (the rows the timed tokens wrote behind the last context are fed over)
            rate = {0: [], 2: []}
            for run in range(a.runs):
                for o in (0, 2):
                    ggml.set_option("attn_split", o)
                    _decode(model, ctx, logits)
                    rate[o].append(_decode(model, ctx, logits))
                    print("context %d, run %d, attn_split %d: %.1f tok/s" % (ctx, run, o, rate[o][-1]), file=sys.stderr, flush=True)
            one, split = _stats(rate[0]), _stats(rate[2])
            out["contexts"][str(ctx)] = {"one_workgroup_per_head": one, "split": split,
                                         "split_above_by_more_than_the_spread": split["median"] - one["median"] > one["max"] - one["min"]}
            model.n_past = ctx
        wins = [out["contexts"][str(c)]["split_above_by_more_than_the_spread"] for c in contexts]
        out["threshold"] = next((c for i, c in enumerate(contexts) if all(wins[i:])), None)
        out.update({k: ggml.get_stat(k) - v for k, v in zip(names, s0)})
        out["device"] = ggml.lib().ggml_hip_version().decode()
    finally:
        ggml.set_option("attn_split", 1)
        ggml.set_option("plan_mpt", 0)
        ggml.set_option("plan_mpt_prompt", 0)
        model.free()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
