"""Device time of the requantizing add of a LoRA patch on K-quant weights (k_add_k: kernels/lora.h, kernels/kquant_encode.h)
for Q4_K and Q6_K at [4096, 4096] and [4096, 11008], with k_add_q<Q4_0> at the same shapes in the same run as the yardstick.
Each figure is the device time of the one launch of the add (ggml_hip_timing_*, class "other": src1 is a leaf, so the graph
holds no other kernel), warmed up, the median of the repeats; bytes are the launch's traffic: W read, W written, src1 read.
Prints one JSON line.
    python tests/tools/lora_kquant.py [--repeats 9] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from llm_amd import ggml as G  # noqa: E402

SHAPES = [(4096, 4096), (4096, 11008)]  # (ne0, ne1)
TYPES = [G.TYPE_Q4_K, G.TYPE_Q6_K, G.TYPE_Q4_0]


def add_ms(t, w_raw, x, ne0, ne1):
    """Device milliseconds of the add's launch."""
    with G.Context(w_raw.nbytes + 4096) as wctx, G.Context(w_raw.nbytes + x.nbytes + (1 << 20)) as ctx:
        w = wctx.tensor_from(w_raw, t, (ne0, ne1))
        out = ctx.op_add(w, ctx.tensor_from(x, G.TYPE_F32, (ne0, ne1)))
        gr = ctx.graph().build_forward_expand(out)
        G.lib().ggml_hip_timing_begin()
        gr.compute()
        G.lib().ggml_hip_timing_end()
        ms, n, _ = G.timing_query(G.KCLASS_OTHER)
        if n != 1:
            raise RuntimeError(f"the graph launched {n} kernels of class 'other', expected the add alone")
        return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    res = {"repeats": a.repeats, "warmup": a.warmup, "cases": []}
    for ne0, ne1 in SHAPES:
        rng = np.random.default_rng([ne0, ne1])
        w32 = (0.02 * rng.standard_normal((ne1, ne0), dtype=np.float32))
        x = (0.01 * rng.standard_normal((ne1, ne0), dtype=np.float32))
        row = {}
        raws = {t: G.quantize(t, w32) for t in TYPES}
        times = {t: [] for t in TYPES}
        for _ in range(a.warmup + a.repeats):  # the types take turns, so a drift of the machine touches all of them alike
            for t in TYPES:
                times[t].append(add_ms(t, raws[t], x, ne0, ne1))
        for t in TYPES:
            w_raw, ms = raws[t], times[t][a.warmup:]
            med = statistics.median(ms)
            nbytes = 2 * w_raw.nbytes + x.nbytes
            row[G.TYPE_NAMES[t]] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                                    "bytes": nbytes, "gb_per_s": round(nbytes / med / 1e6, 1)}
        for name in ("q4_K", "q6_K"):
            row[name]["bytes_per_s_vs_q4_0"] = round(row[name]["gb_per_s"] / row["q4_0"]["gb_per_s"], 3)
        res["cases"].append({"ne0": ne0, "ne1": ne1, **row})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
