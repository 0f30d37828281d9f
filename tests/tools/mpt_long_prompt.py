"""Long prompts of MPT-7B on the MPT prompt plan (backend option plan_mpt_prompt = 1): the chunks whose rows lie behind k_p_attn_alibi's LDS
fit (n_past + N > 2240 keys at head size 128) on the streaming kernel (option mpt_attn_stream = 1) against the node-by-node executor they
fell to before it (option 0).  Q4_0 random blocks (rotary_decode.fast_weights), one MI355X, n_ctx 8192, Mpt.feed_prompt's loop of 8192 tokens
at n_batch 512 with every evaluation timed (an evaluation ends in the logits' read-back).  `--runs` alternating runs each after one untimed
run of either: median and min-max of the whole prompt's tokens/s and of the chunks behind the fit, and whether option 1's median on those
chunks is above option 0's by more than option 0's own min-max spread.  For information: one 512-token prompt with every row streamed
(option 2) against option 1 — what the three sweeps cost where the scores fit in LDS.  Prints one JSON line (profiles/mpt_long_prompt.json).
    python tests/tools/mpt_long_prompt.py [--runs 5] [--layers 32] [--tokens 8192]"""
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

FIT, BATCH = 2240, 512  # mpt_attn_queries (csrc/kernels/mpt_prompt.h) at D = 128


def _feed(model, toks):
    """(whole-prompt tokens/s, tokens/s of the chunks behind the fit)"""
    model.n_past = 0
    n_long, t_long, t_all = 0, 0.0, 0.0
    for i in range(0, len(toks), BATCH):
        chunk = toks[i:i + BATCH]
        t0 = time.perf_counter()
        model.evaluate(chunk)
        dt = time.perf_counter() - t0
        t_all += dt
        if i + len(chunk) > FIT:
            n_long, t_long = n_long + len(chunk), t_long + dt
    return len(toks) / t_all, n_long / t_long if n_long else 0.0


def _alternate(model, toks, options, runs):
    rate = {o: [] for o in options}
    for run in range(runs + 1):
        for o in options:
            ggml.set_option("mpt_attn_stream", o)
            r = _feed(model, toks)
            print("run %d, mpt_attn_stream %d: %.1f tok/s, behind the fit %.1f" % ((run, o) + r), file=sys.stderr, flush=True)
            if run:  # (the first run of either: plans built, f16 copies made)
                rate[o].append(r)
    return rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--layers", type=int, default=mpt.MPT_7B["n_layer"])
    ap.add_argument("--tokens", type=int, default=8192)
    a = ap.parse_args()
    if not ggml.has_gpu():
        raise SystemExit("mpt_long_prompt: no HIP device visible")
    hp = dict(mpt.MPT_7B, n_layer=a.layers, wtype=ggml.TYPE_Q4_0)
    w = fast_weights(mpt, hp, hp["wtype"])
    model = mpt.Mpt(hp, w, n_ctx=a.tokens)
    del w
    out = {"model": "mpt_7b", "n_layer": hp["n_layer"], "wtype": "q4_0", "n_ctx": a.tokens, "n_batch": BATCH, "runs": a.runs}
    names = ("mpt_stream_tokens", "mpt_prompt_tokens", "generic_graphs")
    s0 = [ggml.get_stat(k) for k in names]
    try:
        ggml.set_option("plan_mpt_prompt", 1)
        toks = np.random.default_rng(a.tokens).integers(0, hp["n_vocab"], a.tokens).astype(np.int32)
        rate = _alternate(model, toks, (0, 1), a.runs)
        ex, st = (_stats([r[1] for r in rate[o]]) for o in (0, 1))
        out["prompt_tokens_per_s"] = {"whole_prompt": {"executor_behind_the_fit": _stats([r[0] for r in rate[0]]), "stream": _stats([r[0] for r in rate[1]])},
                                      "chunks_behind_%d_keys" % FIT: {"executor": ex, "stream": st},
                                      "stream_above_executor_by_more_than_its_spread": st["median"] - ex["median"] > ex["max"] - ex["min"]}
        rate = _alternate(model, toks[:BATCH], (1, 2), a.runs)
        out["prompt_tokens_per_s"]["one_chunk_of_%d" % BATCH] = {"lds": _stats([r[0] for r in rate[1]]), "stream_forced": _stats([r[0] for r in rate[2]])}
        out.update({k: ggml.get_stat(k) - v for k, v in zip(names, s0)})
        out["device"] = ggml.lib().ggml_hip_version().decode()
    finally:
        ggml.set_option("plan_mpt_prompt", 0)
        ggml.set_option("mpt_attn_stream", 1)
        model.free()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
