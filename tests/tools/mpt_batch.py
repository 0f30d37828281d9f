"""Decode rate of several MPT-7B sessions on the batched MPT step (backend option plan_mpt_batch) against the same sessions stepped one by
one on the MPT decode plan (option plan_mpt): Q4_0 random blocks (rotary_decode.fast_weights), one MI355X, n_ctx 4096, B = 2, 4 and 8
sessions at equal contexts (128 positions each) and at skewed ones (one session at 4000, the others at 100; the caches hold zeros — the
rate does not depend on their contents).  Two forms: `step`, mpt.evaluate_batch against Mpt.evaluate per session, the Python graph
builds included; `chain`, mpt.infer_tokens_batch against Mpt.infer_tokens_device per session.  `--steps` tokens per session and run,
`--runs` alternating runs each after one untimed run of either; median and min-max of the runs' aggregate tokens/s, and whether the
batch's median is above the stepped sessions' by more than their own min-max spread.  Prints one JSON line (profiles/mpt_batch.json).
    python tests/tools/mpt_batch.py [--runs 5] [--steps 16] [--layers 32]"""
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


def _run(sess, pos, steps, form, batched):
    """steps tokens per session from the positions pos; aggregate tokens/s"""
    for s, p in zip(sess, pos):
        s.n_past = p
    tok = np.arange(len(sess), dtype=np.int32) + 7
    if form == "chain":  # (the chains continue an evaluation: one untimed step)
        for s, p, t in zip(sess, pos, tok):
            s.evaluate([int(t)])
    t0 = time.perf_counter()
    if form == "step":
        for _ in range(steps):
            if batched:
                mpt.evaluate_batch(sess, tok)
            else:
                for s, t in zip(sess, tok):
                    s.evaluate([int(t)])
    elif batched:
        mpt.infer_tokens_batch(sess, steps)
    else:
        for s in sess:
            s.infer_tokens_device(steps)
    return len(sess) * steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--layers", type=int, default=mpt.MPT_7B["n_layer"])
    a = ap.parse_args()
    if not ggml.has_gpu():
        raise SystemExit("mpt_batch: no HIP device visible")
    hp = dict(mpt.MPT_7B, n_layer=a.layers, wtype=ggml.TYPE_Q4_0)
    w = fast_weights(mpt, hp, hp["wtype"])
    model = mpt.Mpt(hp, w, n_ctx=4096)
    del w
    sess = [model] + [model.new_session() for _ in range(7)]
    out = {"model": "mpt_7b", "n_layer": hp["n_layer"], "wtype": "q4_0", "n_ctx": 4096, "runs": a.runs, "steps": a.steps, "aggregate_tokens_per_s": {}}
    b0, g0 = ggml.get_stat("mpt_batch_steps"), ggml.get_stat("generic_graphs")
    try:
        for B in (2, 4, 8):
            for ctx, pos in (("equal128", [128] * B), ("skewed4000_100", [4000] + [100] * (B - 1))):
                for form in ("step", "chain"):
                    rate = {0: [], 1: []}
                    for run in range(a.runs + 1):
                        for on in (0, 1):  # 0: one by one on plan_mpt; 1: the batched step
                            ggml.set_option("plan_mpt", 1 - on)
                            ggml.set_option("plan_mpt_batch", on)
                            r = _run(sess[:B], pos, a.steps, form, bool(on))
                            if run:  # (the first run of either: plans built, graphs captured)
                                rate[on].append(r)
                    one, bat = _stats(rate[0]), _stats(rate[1])
                    out["aggregate_tokens_per_s"][f"B{B}_{ctx}_{form}"] = {
                        "one_by_one_plan_mpt": one, "batched": bat, "batched_above_one_by_one_by_more_than_its_spread": bat["median"] - one["median"] > one["max"] - one["min"],
                        "batched_behind_one_by_one": bat["median"] < one["median"]}
                    print(json.dumps({f"B{B}_{ctx}_{form}": [one, bat]}), file=sys.stderr, flush=True)
        out["mpt_batch_steps"] = ggml.get_stat("mpt_batch_steps") - b0
        out["generic_graphs"] = ggml.get_stat("generic_graphs") - g0
        out["device"] = ggml.lib().ggml_hip_version().decode()
    finally:
        ggml.set_option("plan_mpt", 0)
        ggml.set_option("plan_mpt_batch", 0)
        for s in sess[::-1]:
            s.free()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
