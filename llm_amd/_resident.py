"""Shared plumbing of the generic-executor model families (gptneox.py, falcon.py, gptj.py): synthetic GGML weights
from a name -> shape table, and a model object whose weights are resident on the device with one session's f16
K/V memory.  The graphs themselves live in the family modules."""
import numpy as np

from . import ggml as G


def make_weights(shapes, wtype, seed, quantize=None, gains=()):
    """shapes: name -> (ne0, ne1 or None).  2-D weights N(0, 0.02^2) quantized to `wtype` (the reference's
    quantizer never touches 1-D tensors, crates/llm-base/src/quantize.rs:332-335); 1-D tensors stay f32:
    names in `gains` 1 + N(0, 0.01^2), every other one (biases) N(0, 0.01^2)."""
    quantize = quantize or G.quantize
    rng = np.random.default_rng(seed)
    w = {}
    for name, (ne0, ne1) in shapes.items():
        if ne1 is None:
            w[name] = ((1.0 if name in gains else 0.0) + 0.01 * rng.standard_normal(ne0)).astype(np.float32)
        else:
            w[name] = quantize(wtype, (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32))
    return w


class Resident:
    """Weights transferred to the device (every tensor: the reference's transfer_to(backend)) + one session's
    K/V memory, f16, `kv_width` elements per position and layer."""

    def __init__(self, hp, w, shapes, kv_width, n_ctx=None):
        self.hp = hp
        self.C = n_ctx or hp["n_ctx"]
        L = hp["n_layer"]
        nbytes = sum(a.nbytes for a in w.values()) + 512 * (len(w) + 4) + (1 << 16)
        self.ctx = G.Context(nbytes)
        self.t = {}
        for name, (ne0, ne1) in shapes.items():
            a = w[name]
            if ne1 is None:
                t = self.ctx.tensor_from(a, G.TYPE_F32, (ne0,))
            else:
                t = self.ctx.tensor_from(a, hp["wtype"], (ne0, ne1))
            self.t[name] = t.set_name(name[-40:]).transfer_to_gpu()
        n_kv = L * self.C * kv_width
        self.sctx = G.Context(2 * n_kv * 2 + (1 << 16))
        self.memory_k = self.sctx.new_tensor(G.TYPE_F16, n_kv).set_name("memory_k").offload_no_scratch()
        self.memory_v = self.sctx.new_tensor(G.TYPE_F16, n_kv).set_name("memory_v").offload_no_scratch()
        self.n_past = 0

    def free(self):
        self.sctx.free()
        self.ctx.free()

    def _ctx0(self, N, kq_copies=3):
        """The compute context of one evaluate(): every node keeps its own buffer (no scratch reuse across layers),
        per layer and token at most ~48*n_embd f32 activations + the KQ rows (`kq_copies`*T*n_head f32 with the views:
        BLOOM and MPT keep 4, their scale / mask / softmax are out of place), plus per layer one f16 copy of V
        (Falcon's cont(transpose), BLOOM's and MPT's permuted copy)."""
        hp = self.hp
        E, L, T = hp["n_embd"], hp["n_layer"], self.n_past + N
        return G.Context(64 * 1024 * 1024 + L * N * (48 * E + kq_copies * T * hp["n_head"]) * 4 + L * T * E * 2)
