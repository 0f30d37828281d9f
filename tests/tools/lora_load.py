"""Load time of a LLaMA file with LoRA adapters (llm_llama_load_lora, llama.Llama.load(lora=...)): LLaMA-7B Q4_0 with no
adapter (the mmap load), with an r = 16 adapter on wq and wv, and with one on all seven matrices of every layer (f32 A and
B, alpha = 32: the patch graphs scale).  The adapted loads are split into: model file read into the owned buffer, adapter
open, patching as a whole (host graph build + device work + mirroring + the copies over the weights), the mirroring of the
CPU-backend nodes (ba, scaled, out; ggml_hip_get_stat("ns_mirror"), which includes the wait for the graph's kernels), the
device time of the kernels by class (ggml_hip_timing_*: attn = the f32 / f16 products, other = scale and the
requantizing add) and the copies over the weights.  Weights are random GGML blocks (synth.make_llama_fast) written to a
temporary GGJT file; the first load also warms the page cache.
    python tests/tools/lora_load.py [--model 7b] [--r 16] [--keep DIR]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from llm_amd import ggml, llama, synth  # noqa: E402

SEVEN = ("attention.wq", "attention.wk", "attention.wv", "attention.wo", "feed_forward.w1", "feed_forward.w2",
         "feed_forward.w3")


def write_adapter(path, hp, names, r, alpha, seed):
    shapes = synth.tensor_shapes(hp)
    rng = np.random.default_rng(seed)
    ts = {}
    for i in range(hp["n_layer"]):
        for n in names:
            name = f"layers.{i}.{n}.weight"
            ne0, ne1 = shapes[name]
            ts[name + ".loraA"] = (0.01 * rng.standard_normal((ne0, r))).astype(np.float32)
            ts[name + ".loraB"] = (0.01 * rng.standard_normal((ne1, r))).astype(np.float32)
    synth.write_ggla(path, r, alpha, ts)
    return len(ts) // 2


def timed_load(path, lora):
    L = llama._lib()
    out = np.zeros(4, np.float64)
    L.llm_lora_timing(out.ctypes.data_as(C.POINTER(C.c_double)), 1)
    m0, b0 = ggml.get_stat("ns_mirror"), ggml.get_stat("mirror_bytes")
    ggml.lib().ggml_hip_timing_begin()
    t = time.perf_counter()
    m = llama.Llama.load(path, context_size=512, lora=lora)
    wall = time.perf_counter() - t
    ggml.lib().ggml_hip_timing_end()
    L.llm_lora_timing(out.ctypes.data_as(C.POINTER(C.c_double)), 1)
    dev = {}
    for cname, k in (("attn", ggml.KCLASS_ATTN), ("other", ggml.KCLASS_OTHER)):
        ms, n, _ = ggml.timing_query(k)
        dev[cname] = {"ms": round(ms, 1), "launches": n}
    m.free()
    return {"wall_s": round(wall, 3), "read_s": round(out[0] / 1e9, 3), "adapter_open_s": round(out[1] / 1e9, 3),
            "patch_s": round(out[2] / 1e9, 3), "copy_over_w_s": round(out[3] / 1e9, 3),
            "mirror_s": round((ggml.get_stat("ns_mirror") - m0) / 1e9, 3),
            "mirror_gb": round((ggml.get_stat("mirror_bytes") - b0) / 1e9, 2), "device": dev}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7b", choices=["7b", "13b"])
    ap.add_argument("--r", type=int, default=16)
    ap.add_argument("--keep", default=None, help="directory for the files (default: a temporary one, removed)")
    a = ap.parse_args()
    hp0 = synth.LLAMA_7B if a.model == "7b" else synth.LLAMA_13B
    d = a.keep or tempfile.mkdtemp()
    model = os.path.join(d, "llama.bin")
    t = time.perf_counter()
    hp, w = synth.make_llama_fast(hp0, ggml.TYPE_Q4_0)
    synth.write_ggjt(model, hp, w)
    del w
    ad2, ad7 = os.path.join(d, "wq_wv.ggla"), os.path.join(d, "all7.ggla")
    n2 = write_adapter(ad2, hp, ("attention.wq", "attention.wv"), a.r, 2 * a.r, 1)
    n7 = write_adapter(ad7, hp, SEVEN, a.r, 2 * a.r, 2)
    print(f"files written in {time.perf_counter() - t:.1f} s", file=sys.stderr)
    res = {"model": a.model, "wtype": "q4_0", "r": a.r}
    try:
        llama.Llama.load(model, context_size=512).free()  # page cache + device init
        res["no_adapter"] = timed_load(model, ())
        res["wq_wv"] = dict(timed_load(model, [ad2]), tensors_patched=n2)
        res["all_seven"] = dict(timed_load(model, [ad7]), tensors_patched=n7)
    finally:
        if not a.keep:
            for p in (model, ad2, ad7):
                if os.path.exists(p):
                    os.remove(p)
            os.rmdir(d)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
