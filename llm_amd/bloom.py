"""BLOOM through the drop-in C ABI: the graph of crates/models/bloom/src/lib.rs:116-342 built node by node with the
ctypes binding (llm_amd.ggml) and executed by ggml_graph_compute on the MI355X (generic executor; there is no fused
plan for it).  A LayerNorm with bias on the embeddings; fused QKV stored as [Q | K | V] blocks of n_embd rows, viewed
at offsets 0, E and 2E; K and V stored token-major, V re-laid by cpy(permute(.., 1, 2, 0, 3)) at every use; ALiBi
attention bias (ggml_alibi, bias_max 8) between the scale and the causal mask, the chain built out of place; biases on
every matrix; a separate output.weight.  Synthetic weights follow the loader's names (lib.rs:56-83); 2-D weights are
quantized, gains and biases stay f32."""
import numpy as np

from . import ggml as G
from ._resident import Resident, make_weights

BLOOM_560M = dict(n_vocab=250880, n_ctx=2048, n_embd=1024, n_head=16, n_layer=24)
BLOOM_7B1 = dict(n_vocab=250880, n_ctx=2048, n_embd=4096, n_head=32, n_layer=30)
BLOOM_TINY = dict(n_vocab=256, n_ctx=64, n_embd=128, n_head=4, n_layer=2)
BLOOM_TINY_12H = dict(BLOOM_TINY, n_embd=192, n_head=12)  # heads 8..11 take ggml's second slope sequence
ALIBI_BIAS_MAX = 8.0  # lib.rs:240


def tensor_shapes(hp):
    """name -> (ne0, ne1 or None); 2-D weights are [in_features (ne0), out_features (ne1)]."""
    E, V = hp["n_embd"], hp["n_vocab"]
    s = {"tok_embeddings.weight": (E, V), "norm.weight": (E, None), "norm.bias": (E, None),
         "output_norm.weight": (E, None), "output_norm.bias": (E, None), "output.weight": (E, V)}
    for i in range(hp["n_layer"]):
        p = f"layers.{i}."
        s[p + "attention_norm.weight"] = (E, None)
        s[p + "attention_norm.bias"] = (E, None)
        s[p + "attention.query_key_value.weight"] = (E, 3 * E)
        s[p + "attention.query_key_value.bias"] = (3 * E, None)
        s[p + "attention.wo.weight"] = (E, E)
        s[p + "attention.wo.bias"] = (E, None)
        s[p + "ffn_norm.weight"] = (E, None)
        s[p + "ffn_norm.bias"] = (E, None)
        s[p + "feed_forward.w1.weight"] = (E, 4 * E)
        s[p + "feed_forward.w1.bias"] = (4 * E, None)
        s[p + "feed_forward.w2.weight"] = (4 * E, E)
        s[p + "feed_forward.w2.bias"] = (E, None)
    return s


def make_bloom(hp0, wtype, seed=1234, quantize=None):
    """ggml-layout weights: dict name -> raw block bytes (quantized 2-D) or f32 array."""
    hp = dict(hp0, wtype=wtype)
    shapes = tensor_shapes(hp)
    return hp, make_weights(shapes, wtype, seed, quantize, {n for n in shapes if n.endswith("norm.weight")})


class Bloom(Resident):
    """Model (weights resident on the device) + one session (f16 K/V memory, both token-major).  offload=False builds
    the graph exactly as the reference does: it never calls set_offloading, so every node is CPU-backend and its
    result is mirrored to the host (and the ALiBi attention chain runs as four launches)."""

    def __init__(self, hp, w, n_ctx=None, offload=True):
        super().__init__(hp, w, tensor_shapes(hp), hp["n_embd"], n_ctx)
        self.offload = offload

    def evaluate(self, tokens):
        """Bloom::evaluate (lib.rs:116-342): returns logits [N, n_vocab]."""
        hp, t = self.hp, self.t
        E, H, L, V = hp["n_embd"], hp["n_head"], hp["n_layer"], hp["n_vocab"]
        D, N, P, C = E // H, len(tokens), self.n_past, self.C
        T = P + N
        ctx0 = self._ctx0(N, kq_copies=4)
        try:
            off = (lambda x: x.offload()) if self.offload else (lambda x: x)

            def ln(a, name):
                return off(ctx0.op_add(off(ctx0.op_mul(off(ctx0.op_norm(a)), t[name + ".weight"])), t[name + ".bias"]))

            def linear(name, a):
                return off(ctx0.op_add(off(ctx0.op_mul_mat(t[name + ".weight"], a)), t[name + ".bias"]))

            x = off(ctx0.op_get_rows(t["tok_embeddings.weight"], ctx0.tensor_from(np.asarray(tokens, np.int32))))
            x = ln(x, "norm")  # :144-147
            gf = ctx0.graph()
            for il in range(L):
                p = f"layers.{il}."
                cur = ln(x, p + "attention_norm")  # :155-159
                cur = linear(p + "attention.query_key_value", cur)  # :162-163
                nb = cur.nb[1]
                qc, kc, vc = (ctx0.op_view_2d(cur, E, N, nb, 4 * E * j) for j in range(3))  # :166-185
                k = ctx0.op_view_1d(self.memory_k, N * E, 2 * E * (il * C + P))  # :188-203
                v = ctx0.op_view_1d(self.memory_v, N * E, 2 * E * (il * C + P))
                gf.build_forward_expand(off(ctx0.op_cpy(kc, k)))
                gf.build_forward_expand(off(ctx0.op_cpy(vc, v)))
                q = ctx0.op_permute(off(ctx0.op_cpy(qc, ctx0.new_tensor(G.TYPE_F32, D, H, N))), 0, 2, 1, 3)  # :206-212
                kk = ctx0.op_permute(ctx0.op_reshape_3d(ctx0.op_view_1d(self.memory_k, T * E, il * C * 2 * E), D, H, T),
                                     0, 2, 1, 3)  # :215-227
                kq = off(ctx0.op_mul_mat(kk, q))  # :230
                kq = off(ctx0.op_scale(kq, ctx0.new_f32(np.float32(1.0) / np.sqrt(np.float32(E) / np.float32(H)))))
                kq = off(ctx0.op_alibi(kq, P, H, ALIBI_BIAS_MAX))  # :240
                kq = off(ctx0.op_diag_mask_inf(kq, P))  # :243
                kq = off(ctx0.op_soft_max(kq))  # :246
                vt = off(ctx0.op_cpy(ctx0.op_permute(ctx0.op_reshape_3d(
                    ctx0.op_view_1d(self.memory_v, T * E, il * C * 2 * E), D, H, T), 1, 2, 0, 3),
                    ctx0.new_tensor(G.TYPE_F16, T, D, H)))  # :250-270
                kqv = off(ctx0.op_mul_mat(vt, kq))  # :272
                cur = off(ctx0.op_cpy(ctx0.op_permute(kqv, 0, 2, 1, 3), ctx0.new_tensor(G.TYPE_F32, E, N)))  # :275-281
                cur = linear(p + "attention.wo", cur)  # :284-285
                ff_in = off(ctx0.op_add(cur, x))  # :287
                cur = ln(ff_in, p + "ffn_norm")  # :291-296
                cur = off(ctx0.op_gelu(linear(p + "feed_forward.w1", cur)))  # :298-304
                cur = linear(p + "feed_forward.w2", cur)  # :306-308
                x = off(ctx0.op_add(cur, ff_in))  # :310
            x = ln(x, "output_norm")  # :317-322
            logits = ctx0.op_mul_mat(t["output.weight"], x)  # :327
            gf.build_forward_expand(logits)
            gf.compute()
            self.n_past = T
            return logits.read_data().reshape(N, V).copy()
        finally:
            ctx0.free()
