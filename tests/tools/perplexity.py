#!/usr/bin/env python
"""The shape of `llm perplexity` (InferenceSession::perplexity, crates/llm-base/src/inference_session.rs:519-589) over a
synthetic LLaMA-7B Q4_0, context_size = 2048, one chunk: prints `Perplexity[i]: value` per chunk and times, per n_batch,

  A1  what a user could do before Session.perplexity existed: Session.evaluate(want_all_logits=True) per batch
      (n_batch * n_vocab * 4 bytes read back per batch);
  A2  A1 plus a numpy f32 softmax of the counted rows (the reference's host work);
  B   Session.perplexity(on_device=True): the logits stay in HBM, k_row_prob reduces the counted rows;
  H   Session.perplexity(on_device=False): the reference's shape inside the library;
  F   feed_prompt of the first 2047 tokens (no logits leave the device): the floor.

Host clock around work that ends in ggml_hip_synchronize; each shape warmed once, the legs alternated in one process and
repeated --reps times (median and min..max are printed).
python tests/tools/perplexity.py [--n-batch 8 512] [--reps 3] [--legs A1 A2 B H F]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from llm_amd import ggml, llama, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n-batch", type=int, nargs="+", default=[8, 512])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--legs", nargs="+", default=["A1", "A2", "B", "H", "F"])
ap.add_argument("--context-size", type=int, default=2048)
args = ap.parse_args()

CTX = args.context_size
hp, w = synth.make_llama_fast(synth.LLAMA_7B, ggml.TYPE_Q4_0)
model = llama.Llama(hp, w, context_size=CTX)
toks = ((np.arange(CTX, dtype=np.int64) * 7919 + 5) % hp["n_vocab"]).astype(np.int32)
first, last = min(512, CTX // 2), CTX - 1
L = ggml.lib()


def leg_a(sess, n_batch, softmax):
    sess.seek(0)
    t = toks.copy()
    t[0] = 1
    nll = np.float32(0.0)
    for lo in range(0, CTX, n_batch):
        logits = sess.evaluate(t[lo:lo + n_batch], want_all_logits=True)
        a, b = max(first, lo), min(last, lo + logits.shape[0])
        if softmax and a < b:
            x = logits[a - lo:b - lo]
            e = np.exp(x - x.max(axis=1, keepdims=True))
            p = e[np.arange(b - a), toks[a + 1:b + 1]] / e.sum(axis=1, dtype=np.float32)
            nll += np.float32(-np.log(p).sum(dtype=np.float32))
    return float(np.exp(nll / np.float32(last - first))) if softmax else None


def leg_b(sess, n_batch, on_device):
    return sess.perplexity(toks, bos=1, on_device=on_device)[0]


def leg_f(sess, n_batch):
    sess.seek(0)
    sess.feed_prompt(toks[:CTX - 1])


LEGS = {"A1": lambda s, nb: leg_a(s, nb, False), "A2": lambda s, nb: leg_a(s, nb, True), "B": lambda s, nb: leg_b(s, nb, True),
        "H": lambda s, nb: leg_b(s, nb, False), "F": leg_f}

for n_batch in args.n_batch:
    sess = model.start_session(n_batch=n_batch)
    ms = {k: [] for k in args.legs}
    val = {}
    for rep in range(args.reps + 1):  # rep 0 warms every shape
        for k in args.legs:
            L.ggml_hip_synchronize()
            t0 = time.perf_counter()
            v = LEGS[k](sess, n_batch)
            L.ggml_hip_synchronize()
            if rep:
                ms[k].append((time.perf_counter() - t0) * 1e3)
            if v is not None:
                val[k] = v
    sess.free()
    for k in ("B", "H", "A2"):
        if k in val:
            print(f"n_batch={n_batch} {k}: Perplexity[0]: {val[k]:.4f}")
    for k in args.legs:
        print(f"n_batch={n_batch} {k}: median {np.median(ms[k]):.2f} ms  (min {min(ms[k]):.2f} .. max {max(ms[k]):.2f}, {args.reps} runs)")
    if "B" in ms and "F" in ms:
        print(f"n_batch={n_batch} B - F (the price of the feature): {np.median(ms['B']) - np.median(ms['F']):.2f} ms per {CTX}-token chunk")
    if "B" in ms and "A1" in ms:
        print(f"n_batch={n_batch} median B <= median A1: {np.median(ms['B']) <= np.median(ms['A1'])}")
model.free()
