#!/usr/bin/env python
"""Batched multi-session decode (Llama.evaluate_batch -> ggml_hip_decode_batch) against the same sessions stepped one after the
other on the model's slot, in one run: synthetic LLaMA-7B Q4_0, every session at about 128 positions, greedy tokens.
    python tests/tools/batch_decode.py [B ...]        (default 2 4 8; env BATCH_STEPS: timed steps per leg, default 96)
Per B: aggregate tokens/s of the batched step, of the one-by-one step (the single-token fused plan, B passes over the weights),
and the per-launch-class milliseconds of ONE batched step (per-launch HIP events, the step launched eagerly for it).
Writes profiles/batch_decode_7b_q4_0.json and prints it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)


def main():
    counts = [int(a) for a in sys.argv[1:]] or [2, 4, 8]
    steps = int(os.environ.get("BATCH_STEPS", "96"))
    from llm_amd import ggml, llama, synth
    L = ggml.lib()
    hp, w = synth.make_llama_fast(synth.LLAMA_7B, ggml.TYPE_Q4_0)
    model = llama.Llama(hp, w, context_size=2048)
    out = {"model": "LLaMA-7B Q4_0 (synthetic blocks)", "positions_at_start": 128, "steps_per_leg": steps, "runs": []}
    for B in counts:
        legs = {}
        for leg in ("batched", "one_by_one"):
            sess = [model.start_session(n_batch=8) for _ in range(B)]
            for i, s in enumerate(sess):  # different prompts, slightly different lengths: a ragged batch
                s.feed_prompt((np.arange(120 + i, dtype=np.int32) * (7 + i) + 5) % hp["n_vocab"])

            def step():
                if leg == "batched":
                    ran, _ = model.infer_next_tokens_batch(sess)
                    assert ran, "the backend declined the batched step"
                else:
                    for s in sess:
                        s.infer_next_token()

            for _ in range(8):
                step()
            L.ggml_hip_synchronize()
            s0, r0 = ggml.get_stat("batch_decode_steps"), ggml.get_stat("graph_replays")
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            L.ggml_hip_synchronize()
            el = time.perf_counter() - t0
            legs[leg] = {"aggregate_tokens_per_s": round(B * steps / el, 1), "ms_per_step": round(el / steps * 1e3, 4),
                         "batch_decode_steps": ggml.get_stat("batch_decode_steps") - s0,
                         "graph_replays": ggml.get_stat("graph_replays") - r0}
            if leg == "batched":
                L.ggml_hip_timing_begin()
                step()
                L.ggml_hip_timing_end()
                cls = {name: ggml.timing_query(k) for name, k in (("mmvq", ggml.KCLASS_MMVQ), ("attn", ggml.KCLASS_ATTN),
                                                                  ("other", ggml.KCLASS_OTHER))}
                legs[leg]["class_ms"] = {k: round(v[0], 4) for k, v in cls.items()}
                legs[leg]["class_launches"] = {k: int(v[1]) for k, v in cls.items()}
            for s in sess:
                s.free()
        run = {"sessions": B, **legs,
               "batched_vs_one_by_one": round(legs["batched"]["aggregate_tokens_per_s"] / legs["one_by_one"]["aggregate_tokens_per_s"], 3)}
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
    model.free()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "batch_decode_7b_q4_0.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
