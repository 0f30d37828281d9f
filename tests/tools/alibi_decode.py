"""Decode rate of the ALiBi families (BLOOM, MPT) on the generic node-by-node executor (no fused plan): full depth, Q4_0,
batch 1, a 128-token prompt (fed as 4 chunks of 32), then timed single-token steps, with option fuse on (the scale ->
alibi -> diag_mask_inf -> soft_max chain as one launch, k_soft_max<true, true>) and off (four launches; these graphs have
no other fusable pair: GELU, not SiLU; LayerNorm, not RMSNorm).  Prints one JSON line per model with decode tokens/s
(host graph building + launches + device time, as a caller sees it) and, per setting, the per-kernel-class device split
of one token (ggml_hip_timing_*: mmvq = quantized mat-vec, attn = F16 attention products, other = everything else).
Weights are random GGML blocks (rotary_decode.fast_weights): the same bytes per weight as a real file.
    python tests/tools/alibi_decode.py [bloom_7b1] [mpt_7b] [bloom_560m] [--steps 16] [--warmup 4]"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from llm_amd import bloom, ggml, mpt  # noqa: E402
from rotary_decode import fast_weights  # noqa: E402

MODELS = {"bloom_7b1": (bloom, bloom.BLOOM_7B1, bloom.Bloom),
          "mpt_7b": (mpt, mpt.MPT_7B, mpt.Mpt),
          "bloom_560m": (bloom, bloom.BLOOM_560M, bloom.Bloom)}
DEFAULT = ["bloom_7b1", "mpt_7b"]


def _split(model, tok):
    L = ggml.lib()
    L.ggml_hip_timing_begin()
    model.evaluate(np.array([tok], np.int32))
    L.ggml_hip_timing_end()
    split = {}
    for cname, k in (("mmvq", ggml.KCLASS_MMVQ), ("mmq_mfma", ggml.KCLASS_MMQ_MFMA), ("attn", ggml.KCLASS_ATTN),
                     ("other", ggml.KCLASS_OTHER)):
        ms, n, _ = ggml.timing_query(k)
        split[cname] = {"ms": round(ms, 3), "launches": n}
    return split


def run(name, steps, warmup, prompt=128):
    mod, hp0, cls = MODELS[name]
    hp = dict(hp0, wtype=ggml.TYPE_Q4_0)
    t0 = time.perf_counter()
    w = fast_weights(mod, hp, hp["wtype"])
    model = cls(hp, w, n_ctx=prompt + 2 * (warmup + steps) + 8)
    del w
    load_s = time.perf_counter() - t0
    toks = np.random.default_rng(1).integers(0, hp["n_vocab"], prompt).astype(np.int32)
    for c in range(0, prompt, 32):  # prompt chunks of 32: the node-per-buffer compute context stays ~1 GB
        lg = model.evaluate(toks[c:c + 32])
    tok = int(np.argmax(lg[-1]))
    out = {"model": name, "n_layer": hp["n_layer"], "n_vocab": hp["n_vocab"], "wtype": "q4_0", "prompt": prompt,
           "steps": steps}
    g0, p0 = ggml.get_stat("generic_graphs"), ggml.get_stat("plan_tokens")
    try:
        for fuse in (1, 0):
            ggml.set_option("fuse", fuse)
            for _ in range(warmup):
                tok = int(np.argmax(model.evaluate(np.array([tok], np.int32))[-1]))
            f0 = ggml.get_stat("alibi_fused")
            per = []
            for _ in range(steps):
                ts = time.perf_counter()
                tok = int(np.argmax(model.evaluate(np.array([tok], np.int32))[-1]))
                per.append(time.perf_counter() - ts)
            fused = (ggml.get_stat("alibi_fused") - f0) / steps
            split = _split(model, tok)
            out[f"fuse{fuse}"] = {
                "decode_tokens_per_s": round(steps / sum(per), 1),
                "ms_per_token_min_median_max": [round(x * 1e3, 3) for x in (min(per), float(np.median(per)), max(per))],
                "alibi_fused_per_token": fused,
                "launches_per_token": sum(v["launches"] for v in split.values()),
                "device_split_one_token": split,
                "device_ms_one_token": round(sum(v["ms"] for v in split.values()), 3)}
    finally:
        ggml.set_option("fuse", 1)
    out.update({"generic_graphs": ggml.get_stat("generic_graphs") - g0, "plan_tokens": ggml.get_stat("plan_tokens") - p0,
                "load_s": round(load_s, 1), "device": ggml.lib().ggml_hip_version().decode()})
    model.free()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="*", default=DEFAULT)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    if not ggml.has_gpu():
        raise SystemExit("alibi_decode: no HIP device visible")
    for name in a.models:
        run(name, a.steps, a.warmup)


if __name__ == "__main__":
    main()
