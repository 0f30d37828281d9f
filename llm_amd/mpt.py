"""MPT through the drop-in C ABI: the graph of crates/models/mpt/src/lib.rs:93-259 built node by node with the ctypes
binding (llm_amd.ggml) and executed by ggml_graph_compute on the MI355X: node by node on the generic executor, or — backend
option plan_mpt, block-format weights, one token, every node offloaded — on the fused MPT plan (csrc/plan_decode.inc
plan_launch_mpt: five launches per layer, the captured graph replayed), which Mpt.infer_tokens_device chains on the device.  LayerNorms without bias, no linear biases at all; Wqkv split into [Q | K | V] blocks of n_embd rows (views at 0,
E and 2E); K and V stored token-major, V re-laid by cpy(permute(.., 1, 2, 0, 3)) at every use; ALiBi attention bias
with the model's alibi_bias_max, the chain built out of place; lm_head tied to transformer.wte.weight (lib.rs:244).
clip_kqv is a hyperparameter the reference reads but its graph does not use; so is it here.  The reference's scratch
buffers (lib.rs:127, 217, 233) are not used: every node keeps its own buffer.  Synthetic weights follow the loader's
names (lib.rs:50-64); 2-D weights are quantized, gains stay f32."""
import ctypes as C

import numpy as np

from . import ggml as G
from ._resident import Resident, make_weights

MPT_7B = dict(n_vocab=50432, n_ctx=2048, n_embd=4096, n_head=32, n_layer=32, alibi_bias_max=8.0, clip_kqv=0.0)
MPT_TINY = dict(n_vocab=256, n_ctx=64, n_embd=128, n_head=4, n_layer=2, alibi_bias_max=8.0, clip_kqv=0.0)
MPT_TINY_12H = dict(MPT_TINY, n_embd=192, n_head=12)  # heads 8..11 take ggml's second slope sequence


def tensor_shapes(hp):
    """name -> (ne0, ne1 or None); 2-D weights are [in_features (ne0), out_features (ne1)]."""
    E, V = hp["n_embd"], hp["n_vocab"]
    s = {"transformer.wte.weight": (E, V), "transformer.norm_f.weight": (E, None)}
    for i in range(hp["n_layer"]):
        p = f"transformer.blocks.{i}."
        s[p + "norm_1.weight"] = (E, None)
        s[p + "attn.Wqkv.weight"] = (E, 3 * E)
        s[p + "attn.out_proj.weight"] = (E, E)
        s[p + "norm_2.weight"] = (E, None)
        s[p + "ffn.up_proj.weight"] = (E, 4 * E)
        s[p + "ffn.down_proj.weight"] = (4 * E, E)
    return s


def make_mpt(hp0, wtype, seed=1234, quantize=None):
    """ggml-layout weights: dict name -> raw block bytes (quantized 2-D) or f32 array."""
    hp = dict(hp0, wtype=wtype)
    shapes = tensor_shapes(hp)
    return hp, make_weights(shapes, wtype, seed, quantize, {n for n in shapes if shapes[n][1] is None})


class Mpt(Resident):
    """Model (weights resident on the device) + one session (f16 K/V memory, both token-major).  offload=False builds
    the graph exactly as the reference does: it never calls set_offloading, so every node is CPU-backend and its
    result is mirrored to the host (and the ALiBi attention chain runs as four launches)."""

    def __init__(self, hp, w, n_ctx=None, offload=True):
        super().__init__(hp, w, tensor_shapes(hp), hp["n_embd"], n_ctx)
        self.offload = offload
        self.last_logits = None  # the last row of the last evaluation: its first maximum is the pending token

    def evaluate(self, tokens):
        """Mpt::evaluate (lib.rs:93-259): returns logits [N, n_vocab]."""
        ctx0 = self._ctx0(len(tokens), kq_copies=4)
        try:
            return self._evaluate_in(ctx0, tokens)[0]
        finally:
            ctx0.free()

    def infer_tokens_device(self, n):
        """n greedy tokens from the last evaluation's logits on: the pending token (their first maximum) is evaluated as its
        graph, and where that ran as the MPT plan the n - 1 tokens behind it are chained on the device
        (ggml_hip_decode_greedy_chain: the argmax feeds the next replay, no graph is built on the host).  Where the entry
        declines (option plan_mpt off, a shape the plan does not take, the context's end) the remaining tokens are stepped:
        evaluate + argmax each.  Returns (ids [n], the logits [n_vocab] behind the last of them) — what the stepped loop
        returns — and leaves n_past n further."""
        if self.last_logits is None:
            raise ValueError("infer_tokens_device: no evaluation to continue")
        ids = np.zeros(n, np.int32)
        if n < 1:
            return ids, self.last_logits
        ids[0] = int(np.argmax(self.last_logits))
        ctx0 = self._ctx0(1, kq_copies=4)
        done = 1
        try:
            _, gf = self._evaluate_in(ctx0, [int(ids[0])])
            if n > 1:  # (ctx0 lives on: the entry is handed the graph it names the plan by)
                tail = np.zeros(n - 1, np.int32)
                logits = np.zeros(self.hp["n_vocab"], np.float32)
                if G.lib().ggml_hip_decode_greedy_chain(C.cast(gf.ptr, C.c_void_p), n - 1, tail.ctypes.data, logits.ctypes.data) == 0:
                    ids[1:] = tail
                    self.n_past += n - 1
                    self.last_logits = logits
                    done = n
        finally:
            ctx0.free()
        for i in range(done, n):
            ids[i] = int(np.argmax(self.last_logits))
            self.evaluate([int(ids[i])])
        return ids, self.last_logits

    def _evaluate_in(self, ctx0, tokens):
        """evaluate's graph in ctx0, computed: (logits [N, n_vocab], the graph)."""
        hp, t = self.hp, self.t
        E, H, L, V = hp["n_embd"], hp["n_head"], hp["n_layer"], hp["n_vocab"]
        D, N, P, C = E // H, len(tokens), self.n_past, self.C
        T = P + N
        off = (lambda x: x.offload()) if self.offload else (lambda x: x)

        def ln(a, name):
            return off(ctx0.op_mul(off(ctx0.op_norm(a)), t[name]))

        x = off(ctx0.op_get_rows(t["transformer.wte.weight"], ctx0.tensor_from(np.asarray(tokens, np.int32))))
        gf = ctx0.graph()
        for il in range(L):
            p = f"transformer.blocks.{il}."
            cur = ln(x, p + "norm_1.weight")  # :129-130
            cur = off(ctx0.op_mul_mat(t[p + "attn.Wqkv.weight"], cur))  # :132
            nb = cur.nb[1]
            qc, kc, vc = (ctx0.op_view_2d(cur, E, N, nb, 4 * E * j) for j in range(3))  # :134-137
            k = ctx0.op_view_1d(self.memory_k, N * E, 2 * E * (il * C + P))  # :139-151
            v = ctx0.op_view_1d(self.memory_v, N * E, 2 * E * (il * C + P))
            gf.build_forward_expand(off(ctx0.op_cpy(kc, k)))
            gf.build_forward_expand(off(ctx0.op_cpy(vc, v)))
            q = ctx0.op_permute(off(ctx0.op_cpy(qc, ctx0.new_tensor(G.TYPE_F32, D, H, N))), 0, 2, 1, 3)  # :153-159
            kk = ctx0.op_permute(ctx0.op_reshape_3d(ctx0.op_view_1d(self.memory_k, T * E, il * C * 2 * E), D, H, T),
                                 0, 2, 1, 3)  # :161-173
            kq = off(ctx0.op_mul_mat(kk, q))  # :175
            kq = off(ctx0.op_scale(kq, ctx0.new_f32(np.float32(1.0) / np.sqrt(np.float32(E) / np.float32(H)))))
            kq = off(ctx0.op_alibi(kq, P, H, hp["alibi_bias_max"]))  # :180-181
            kq = off(ctx0.op_diag_mask_inf(kq, P))  # :182
            kq = off(ctx0.op_soft_max(kq))  # :183
            vt = off(ctx0.op_cpy(ctx0.op_permute(ctx0.op_reshape_3d(
                ctx0.op_view_1d(self.memory_v, T * E, il * C * 2 * E), D, H, T), 1, 2, 0, 3),
                ctx0.new_tensor(G.TYPE_F16, T, D, H)))  # :185-205
            kqv = off(ctx0.op_mul_mat(vt, kq))  # :207
            cur = off(ctx0.op_cpy(ctx0.op_permute(kqv, 0, 2, 1, 3), ctx0.new_tensor(G.TYPE_F32, E, N)))  # :208-210
            cur = off(ctx0.op_mul_mat(t[p + "attn.out_proj.weight"], cur))  # :212
            x = off(ctx0.op_add(x, cur))  # :214
            cur = ln(x, p + "norm_2.weight")  # :219-220
            cur = off(ctx0.op_gelu(off(ctx0.op_mul_mat(t[p + "ffn.up_proj.weight"], cur))))  # :222-224
            cur = off(ctx0.op_mul_mat(t[p + "ffn.down_proj.weight"], cur))  # :227
            x = off(ctx0.op_add(x, cur))  # :229
        x = ln(x, "transformer.norm_f.weight")  # :236-237
        logits = ctx0.op_mul_mat(t["transformer.wte.weight"], x)  # :244, tied to the input embedding
        gf.build_forward_expand(logits)
        gf.compute()
        self.n_past = T
        out = logits.read_data().reshape(N, V).copy()
        self.last_logits = out[-1]
        return out, gf
