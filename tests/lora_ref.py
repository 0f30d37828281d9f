"""Host restatement of a LoRA patch (crates/llm-base/src/lora.rs:86-139) and of ggml's add with a quantized or f16 src0
(upstream ggml.c of the 2023-08 window, add_q_f32 / add_f16_f32), from the oracle's primitives and NumPy:

  add_q:   per row, dequantize_row_q* (the oracle's `dequantize`, unfused `q * d + m`), y = y + x in f32, then from_float:
           quantize_row_q*_reference for Q4_0 .. Q5_1; for Q8_0 the AVX2 branch (id = 127 / amax, round half to even) by
           default, the scalar one with act_quant = 1 (the library's option, kernels/common.h), as every activation
           quantizer of the device.
  add_f16: f16(f32(a) + b), round to nearest even.
  patch:   scaled = f32(B·Aᵀ) [* s], out = add(W, scaled) — exact when the operands are dyadic (small integers times 2^-k),
           so that every product and partial sum is exact in any order and in f16."""
import numpy as np

from llm_amd import ggml as G
from oracle import oracle as O


def add_q(t, w_raw, x, act_quant=0):
    """w_raw: raw bytes of rows of ne0 weights in type t (or f16 values as uint16 / float16 for TYPE_F16); x: f32 [rows, ne0].
    Returns the raw bytes of the result (uint8)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, ne0 = x.shape
    if t == G.TYPE_F16:
        a = np.ascontiguousarray(w_raw).view(np.float16).reshape(rows, ne0).astype(np.float32)
        return (a + x).astype(np.float16).view(np.uint8).reshape(-1)
    y = O.dequantize(t, np.ascontiguousarray(w_raw).view(np.uint8), rows * ne0).reshape(rows, ne0)
    y = (y + x).astype(np.float32)
    return O.quantize_row(t, y, simd=(t == G.TYPE_Q8_0 and act_quant == 0))


def ba_exact(A, B, a_f16):
    """mul_mat(A, B) of the patch, [n_out, n_in], in f64: A as stored [n_in, r], B [n_out, r]; with an f16 A ggml rounds
    B to f16 first (vec_dot_type of F16)."""
    A64 = np.asarray(A, dtype=np.float32).astype(np.float64)
    Bf = np.asarray(B, dtype=np.float32)
    if a_f16:
        Bf = Bf.astype(np.float16).astype(np.float32)
    return Bf.astype(np.float64) @ A64.T


def patch(t, w_raw, A, B, s, act_quant=0):
    """The whole patch for dyadic A and B (the product is exact in f32): returns the new raw bytes of W."""
    ba = ba_exact(A, B, np.asarray(A).dtype == np.float16).astype(np.float32)
    if np.float32(s) != np.float32(1.0):
        ba = (ba * np.float32(s)).astype(np.float32)
    return add_q(t, w_raw, ba, act_quant)


def dyadic(rng, shape, k=7, lim=4, dtype=np.float32):
    """Small integers in [-lim, lim] times 2^-k."""
    return (rng.integers(-lim, lim + 1, size=shape).astype(np.float64) * 2.0 ** -k).astype(dtype)


def make_adapter(rng, targets, shapes, r, alpha, a_f16=False):
    """{r, alpha, tensors} with dyadic .loraA [n_in, r] (f32 or f16) and .loraB [n_out, r] (f32) for every target."""
    ts = {}
    for name in targets:
        ne0, ne1 = shapes[name]
        ts[name + ".loraA"] = dyadic(rng, (ne0, r), dtype=np.float16 if a_f16 else np.float32)
        ts[name + ".loraB"] = dyadic(rng, (ne1, r))
    return dict(r=r, alpha=alpha, tensors=ts)


def merge(w, shapes, adapters, wtype, act_quant=0):
    """lora.patch_weights restated on the host: every adapter in order, targets = adapter names minus the last component."""
    out = dict(w)
    for name, (ne0, ne1) in shapes.items():
        for ad in adapters:
            if name + ".loraA" not in ad["tensors"]:
                continue
            s = np.float32(np.float32(ad["alpha"]) / np.float32(ad["r"]))
            out[name] = patch(wtype, out[name], ad["tensors"][name + ".loraA"], ad["tensors"][name + ".loraB"], s, act_quant)
    return out
