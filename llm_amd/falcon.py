"""Falcon through the drop-in C ABI: the graph of crates/models/falcon/src/lib.rs:153-370 built node by node with the
ctypes binding (llm_amd.ggml) and executed by ggml_graph_compute on the MI355X (generic executor).  No linear biases;
attention and FFN in parallel off the same residual; NeoX-mode RoPE (mode 2, the whole head) applied IN PLACE to
strided Q and K views of the fused QKV output (lib.rs:218-246: rows of (n_head + 2*n_head_kv)*head_dim floats, the V
columns next to them untouched).  n_head_kv == 1 is the 7B form (one shared LayerNorm); n_head_kv > 1 the 40B form
(separate attention LayerNorm ln_attn, lib.rs:72-97 and 199-216).  Multi-query attention is the F16 mul_mat broadcast
of the K/V heads over the query heads.  2-D weights are quantized, gains and biases stay f32."""
import numpy as np

from . import ggml as G
from ._resident import Resident, make_weights

FALCON_7B = dict(n_vocab=65024, n_ctx=2048, n_embd=4544, n_head=71, n_head_kv=1, n_layer=32)
FALCON_TINY = dict(n_vocab=256, n_ctx=64, n_embd=128, n_head=4, n_head_kv=1, n_layer=2)
FALCON_40B_TINY = dict(n_vocab=256, n_ctx=64, n_embd=128, n_head=8, n_head_kv=2, n_layer=2)


def _norm_names(hp, i):
    """(input LayerNorm, attention LayerNorm or None) of layer i, lib.rs:72-81."""
    if hp["n_head_kv"] == 1:
        return f"transformer.h.{i}.input_layernorm", None
    return f"transformer.h.{i}.ln_mlp", f"transformer.h.{i}.ln_attn"


def tensor_shapes(hp):
    """name -> (ne0, ne1 or None); 2-D weights are [in_features (ne0), out_features (ne1)]."""
    E, V, H, Hkv = hp["n_embd"], hp["n_vocab"], hp["n_head"], hp["n_head_kv"]
    D = E // H
    s = {"transformer.word_embeddings.weight": (E, V), "transformer.ln_f.weight": (E, None),
         "transformer.ln_f.bias": (E, None), "lm_head.weight": (E, V)}
    for i in range(hp["n_layer"]):
        p = f"transformer.h.{i}."
        for n in _norm_names(hp, i):
            if n:
                s[n + ".weight"] = (E, None)
                s[n + ".bias"] = (E, None)
        s[p + "self_attention.query_key_value.weight"] = (E, (H + 2 * Hkv) * D)
        s[p + "self_attention.dense.weight"] = (E, E)
        s[p + "mlp.dense_h_to_4h.weight"] = (E, 4 * E)
        s[p + "mlp.dense_4h_to_h.weight"] = (4 * E, E)
    return s


def make_falcon(hp0, wtype, seed=1234, quantize=None):
    """ggml-layout weights: dict name -> raw block bytes (quantized 2-D) or f32 array."""
    hp = dict(hp0, wtype=wtype)
    shapes = tensor_shapes(hp)
    gains = {n for n in shapes if n.endswith(".weight") and shapes[n][1] is None}
    return hp, make_weights(shapes, wtype, seed, quantize, gains)


class Falcon(Resident):
    """Model (weights resident on the device) + one session (f16 K/V memory, n_head_kv*head_dim per position,
    token-major)."""

    def __init__(self, hp, w, n_ctx=None):
        super().__init__(hp, w, tensor_shapes(hp), hp["n_head_kv"] * (hp["n_embd"] // hp["n_head"]), n_ctx)

    def evaluate(self, tokens):
        """Falcon::evaluate (lib.rs:153-370): returns logits [N, n_vocab]."""
        hp, t = self.hp, self.t
        E, H, Hkv, L, V = hp["n_embd"], hp["n_head"], hp["n_head_kv"], hp["n_layer"], hp["n_vocab"]
        D, N, P, C = E // H, len(tokens), self.n_past, self.C
        T, W = P + N, Hkv * D  # W: K/V width per position
        ctx0 = self._ctx0(N)
        try:
            off = lambda x: x.offload()  # ctx0.set_offloading(true): intermediate results stay on the device
            x = off(ctx0.op_get_rows(t["transformer.word_embeddings.weight"],
                                     ctx0.tensor_from(np.asarray(tokens, np.int32))))  # :178
            gf = ctx0.graph()

            def ln(a, name):
                return off(ctx0.op_add(off(ctx0.op_mul(off(ctx0.op_norm(a)), t[name + ".weight"])), t[name + ".bias"]))

            for il in range(L):
                p = f"transformer.h.{il}."
                in_norm, attn_norm = _norm_names(hp, il)
                ln_out = ln(x, in_norm)  # :199-203
                cur = ln_out if attn_norm is None else ln(x, attn_norm)  # :205-216
                cur = off(ctx0.op_mul_mat(t[p + "self_attention.query_key_value.weight"], cur))  # :218
                row = D * (H + 2 * Hkv) * 4  # :220
                qcur = ctx0.op_view_3d(cur, D, H, N, D * 4, row, 0)  # :222-241
                kcur = ctx0.op_view_3d(cur, D, Hkv, N, D * 4, row, D * H * 4)
                vcur = ctx0.op_view_3d(cur, D, Hkv, N, D * 4, row, D * (H + Hkv) * 4)
                qcur = off(ctx0.op_rope_inplace(qcur, P, D, 2, 0))  # :245-246 mode 2 = NeoX, in place on the views
                kcur = off(ctx0.op_rope_inplace(kcur, P, D, 2, 0))
                k = ctx0.op_view_1d(self.memory_k, N * W, 2 * W * (il * C + P))  # :250-259
                v = ctx0.op_view_1d(self.memory_v, N * W, 2 * W * (il * C + P))
                gf.build_forward_expand(off(ctx0.op_cpy(kcur, k)))  # :261-262
                gf.build_forward_expand(off(ctx0.op_cpy(vcur, v)))
                q = ctx0.op_permute(qcur, 0, 2, 1, 3)  # :265
                kk = ctx0.op_permute(ctx0.op_reshape_3d(ctx0.op_view_1d(self.memory_k, T * W, il * C * 2 * W), D, Hkv, T),
                                     0, 2, 1, 3)  # :267-279
                kq = off(ctx0.op_mul_mat(kk, q))  # :282, K/V heads broadcast over the query heads
                kq = off(ctx0.op_scale_inplace(kq, ctx0.new_f32(1.0 / np.sqrt(np.float32(E) / np.float32(H)))))
                kq = off(ctx0.op_diag_mask_inf_inplace(kq, P))  # :285-292
                kq = off(ctx0.op_soft_max_inplace(kq))
                vv = ctx0.op_permute(ctx0.op_reshape_3d(ctx0.op_view_1d(self.memory_v, T * W, il * C * 2 * W), D, Hkv, T),
                                     0, 2, 1, 3)  # :294-306
                vv = off(ctx0.op_cont(ctx0.op_transpose(vv)))  # :307
                kqv = off(ctx0.op_mul_mat(vv, kq))  # :309
                cur = off(ctx0.op_cpy(ctx0.op_permute(kqv, 0, 2, 1, 3), ctx0.new_tensor(G.TYPE_F32, E, N)))  # :311-317
                cur = off(ctx0.op_mul_mat(t[p + "self_attention.dense.weight"], cur))  # :320
                attn_out = off(ctx0.op_cpy(cur, ctx0.new_tensor(G.TYPE_F32, E, N)))  # :325-327
                cur = off(ctx0.op_mul_mat(t[p + "mlp.dense_h_to_4h.weight"], ln_out))  # :329-331
                cur = off(ctx0.op_gelu(cur))
                cur = off(ctx0.op_mul_mat(t[p + "mlp.dense_4h_to_h.weight"], cur))
                cur = off(ctx0.op_add(cur, attn_out))  # :333-334
                x = off(ctx0.op_add(cur, x))
            x = ln(x, "transformer.ln_f")  # :342-347
            logits = ctx0.op_mul_mat(t["lm_head.weight"], x)  # :355, set_offloading(false)
            gf.build_forward_expand(logits)
            gf.compute()
            self.n_past = T
            return logits.read_data().reshape(N, V).copy()
        finally:
            ctx0.free()
