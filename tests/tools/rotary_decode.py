"""Decode rate of the rotary-embedding families on the generic node-by-node executor (no fused plan): full depth,
Q4_0, batch 1, a 128-token prompt (fed as 4 chunks of 32), then timed single-token steps.  Prints one JSON line per model with decode tokens/s
(host graph building + launches + device time, as a caller sees it) and the per-kernel-class device split of one
token (ggml_hip_timing_*: mmvq = quantized mat-vec, attn = F16 attention products, other = everything else).
Weights are random GGML blocks (llm_synth_blocks, the generator behind bench.py's fast weights): the same bytes per
weight as a real file, so the rate is that of the real shape.
    python tests/tools/rotary_decode.py [falcon_7b] [gptj_6b] [pythia_2_8b] [--steps 16] [--warmup 4]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from llm_amd import falcon, ggml, gptj, gptneox  # noqa: E402

MODELS = {"falcon_7b": (falcon, falcon.FALCON_7B, falcon.Falcon),
          "gptj_6b": (gptj, gptj.GPTJ_6B, gptj.GptJ),
          "pythia_2_8b": (gptneox, gptneox.PYTHIA_2_8B, gptneox.GptNeoX)}


def fast_weights(mod, hp, wtype, seed=1234, d_scale=0.0043):
    fill = ggml.lib().llm_synth_blocks
    fill.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float]
    fill.restype = None
    bs, be = ggml.BLOCK_BYTES[wtype], ggml.BLOCK_ELEMS[wtype]
    rng = np.random.default_rng(seed)
    w = {}
    for name, (ne0, ne1) in mod.tensor_shapes(hp).items():
        if ne1 is None:
            w[name] = ((1.0 if name.endswith("weight") else 0.0) + 0.01 * rng.standard_normal(ne0)).astype(np.float32)
            continue
        raw = np.empty(ne1 * (ne0 // be) * bs, dtype=np.uint8)
        fill(wtype, raw.ctypes.data, ne1 * (ne0 // be), int(rng.integers(0, 2**62)), d_scale)
        w[name] = raw
    return w


def run(name, steps, warmup, prompt=128):
    mod, hp0, cls = MODELS[name]
    hp = dict(hp0, wtype=ggml.TYPE_Q4_0)
    t0 = time.perf_counter()
    w = fast_weights(mod, hp, hp["wtype"])
    model = cls(hp, w, n_ctx=prompt + warmup + steps + 8)
    del w
    load_s = time.perf_counter() - t0
    L = ggml.lib()
    toks = np.random.default_rng(1).integers(0, hp["n_vocab"], prompt).astype(np.int32)
    for c in range(0, prompt, 32):  # prompt chunks of 32: the node-per-buffer compute context stays ~1 GB
        lg = model.evaluate(toks[c:c + 32])
    tok = int(np.argmax(lg[-1]))
    g0, p0 = ggml.get_stat("generic_graphs"), ggml.get_stat("plan_tokens")
    for _ in range(warmup):
        tok = int(np.argmax(model.evaluate(np.array([tok], np.int32))[-1]))
    per = []
    for _ in range(steps):
        ts = time.perf_counter()
        tok = int(np.argmax(model.evaluate(np.array([tok], np.int32))[-1]))
        per.append(time.perf_counter() - ts)
    L.ggml_hip_timing_begin()
    model.evaluate(np.array([tok], np.int32))
    L.ggml_hip_timing_end()
    split = {}
    for cname, k in (("mmvq", ggml.KCLASS_MMVQ), ("mmq_mfma", ggml.KCLASS_MMQ_MFMA), ("attn", ggml.KCLASS_ATTN),
                     ("other", ggml.KCLASS_OTHER)):
        ms, n, _ = ggml.timing_query(k)
        split[cname] = {"ms": round(ms, 3), "launches": n}
    out = {"model": name, "n_layer": hp["n_layer"], "wtype": "q4_0", "prompt": prompt, "steps": steps,
           "decode_tokens_per_s": round(steps / sum(per), 1),
           "ms_per_token_min_median_max": [round(x * 1e3, 3) for x in (min(per), float(np.median(per)), max(per))],
           "device_split_one_token": split,
           "device_ms_one_token": round(sum(v["ms"] for v in split.values()), 3),
           "generic_graphs": ggml.get_stat("generic_graphs") - g0, "plan_tokens": ggml.get_stat("plan_tokens") - p0,
           "load_s": round(load_s, 1), "device": L.ggml_hip_version().decode()}
    model.free()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="*", default=list(MODELS))
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    if not ggml.has_gpu():
        raise SystemExit("rotary_decode: no HIP device visible")
    for name in a.models:
        run(name, a.steps, a.warmup)


if __name__ == "__main__":
    main()
