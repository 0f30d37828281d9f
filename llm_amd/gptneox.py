"""GPT-NeoX (Pythia, RedPajama, StableLM-alpha) through the drop-in C ABI: the graph of
crates/models/gptneox/src/lib.rs:156-350 built node by node with the ctypes binding (llm_amd.ggml) and executed by
ggml_graph_compute on the MI355X (generic executor; there is no fused plan for it).  Q/K/V are cont(view_3d) of the
per-head interleaved fused QKV; RoPE is NeoX mode (mode 2) over the first n_rot of each head's n_embd/n_head
elements, ggml's block semantics (kernels/ops.h k_rope_neox).  Both residual forms (use_parallel_residual,
lib.rs:308-330).  Synthetic weights follow the loader's names (lib.rs:58-131); 2-D weights are quantized, gains and
biases stay f32."""
import numpy as np

from . import ggml as G
from ._resident import Resident, make_weights

PYTHIA_1_4B = dict(n_vocab=50304, n_ctx=2048, n_embd=2048, n_head=16, n_layer=24, n_rot=32, use_parallel_residual=True)
PYTHIA_2_8B = dict(n_vocab=50304, n_ctx=2048, n_embd=2560, n_head=32, n_layer=32, n_rot=20, use_parallel_residual=True)
GPTNEOX_TINY = dict(n_vocab=256, n_ctx=64, n_embd=128, n_head=4, n_layer=2, n_rot=32, use_parallel_residual=True)


def tensor_shapes(hp):
    """name -> (ne0, ne1 or None); 2-D weights are [in_features (ne0), out_features (ne1)]."""
    E, V = hp["n_embd"], hp["n_vocab"]
    s = {"gpt_neox.embed_in.weight": (E, V), "gpt_neox.final_layer_norm.weight": (E, None),
         "gpt_neox.final_layer_norm.bias": (E, None), "embed_out.weight": (E, V)}
    for i in range(hp["n_layer"]):
        p = f"gpt_neox.layers.{i}."
        s[p + "input_layernorm.weight"] = (E, None)
        s[p + "input_layernorm.bias"] = (E, None)
        s[p + "attention.query_key_value.weight"] = (E, 3 * E)
        s[p + "attention.query_key_value.bias"] = (3 * E, None)
        s[p + "attention.dense.weight"] = (E, E)
        s[p + "attention.dense.bias"] = (E, None)
        s[p + "post_attention_layernorm.weight"] = (E, None)
        s[p + "post_attention_layernorm.bias"] = (E, None)
        s[p + "mlp.dense_h_to_4h.weight"] = (E, 4 * E)
        s[p + "mlp.dense_h_to_4h.bias"] = (4 * E, None)
        s[p + "mlp.dense_4h_to_h.weight"] = (4 * E, E)
        s[p + "mlp.dense_4h_to_h.bias"] = (E, None)
    return s


def _gains(hp):
    return {n for n in tensor_shapes(hp) if n.endswith("norm.weight")}


def make_gptneox(hp0, wtype, seed=1234, quantize=None):
    """ggml-layout weights: dict name -> raw block bytes (quantized 2-D) or f32 array."""
    hp = dict(hp0, wtype=wtype)
    return hp, make_weights(tensor_shapes(hp), wtype, seed, quantize, _gains(hp))


class GptNeoX(Resident):
    """Model (weights resident on the device) + one session (f16 K/V memory, V stored transposed)."""

    def __init__(self, hp, w, n_ctx=None):
        super().__init__(hp, w, tensor_shapes(hp), hp["n_embd"], n_ctx)

    def evaluate(self, tokens):
        """GptNeoX::evaluate (lib.rs:156-350): returns logits [N, n_vocab]."""
        hp, t = self.hp, self.t
        E, H, L, V, R = hp["n_embd"], hp["n_head"], hp["n_layer"], hp["n_vocab"], hp["n_rot"]
        D, N, P, C = E // H, len(tokens), self.n_past, self.C
        T = P + N
        ctx0 = self._ctx0(N)
        try:
            off = lambda x: x.offload()  # ctx0.set_offloading(true): intermediate results stay on the device
            x = off(ctx0.op_get_rows(t["gpt_neox.embed_in.weight"], ctx0.tensor_from(np.asarray(tokens, np.int32))))
            gf = ctx0.graph()

            def ln(a, name):
                return off(ctx0.op_add(off(ctx0.op_mul(off(ctx0.op_norm(a)), t[name + ".weight"])), t[name + ".bias"]))

            def ffn(p, a):  # feed_forward_network, lib.rs:493-516
                cur = ln(a, p + "post_attention_layernorm")
                cur = off(ctx0.op_add(off(ctx0.op_mul_mat(t[p + "mlp.dense_h_to_4h.weight"], cur)),
                                      t[p + "mlp.dense_h_to_4h.bias"]))
                cur = off(ctx0.op_gelu(cur))
                return off(ctx0.op_add(off(ctx0.op_mul_mat(t[p + "mlp.dense_4h_to_h.weight"], cur)),
                                       t[p + "mlp.dense_4h_to_h.bias"]))

            for il in range(L):
                p = f"gpt_neox.layers.{il}."
                cur = ln(x, p + "input_layernorm")  # :193-197
                cur = off(ctx0.op_mul_mat(t[p + "attention.query_key_value.weight"], cur))  # :200-201
                cur = off(ctx0.op_add(cur, t[p + "attention.query_key_value.bias"]))
                nb = cur.nb[1]
                qkv = [off(ctx0.op_cont(ctx0.op_view_3d(cur, D, H, N, nb // H, nb, 4 * D * j))) for j in range(3)]  # :206-223
                qcur = off(ctx0.op_rope_inplace(qkv[0], P, R, 2, 0))  # :227-228 mode 2 = NeoX
                kcur = off(ctx0.op_rope_inplace(qkv[1], P, R, 2, 0))
                vcur = ctx0.op_transpose(ctx0.op_reshape_2d(qkv[2], E, N))  # :231
                k = ctx0.op_view_1d(self.memory_k, N * E, 2 * E * (il * C + P))  # :233-247
                v = ctx0.op_view_2d(self.memory_v, N, E, C * 2, il * C * 2 * E + P * 2)
                gf.build_forward_expand(off(ctx0.op_cpy(kcur, k)))
                gf.build_forward_expand(off(ctx0.op_cpy(vcur, v)))
                q = ctx0.op_permute(qcur, 0, 2, 1, 3)  # :250
                kk = ctx0.op_permute(ctx0.op_reshape_3d(ctx0.op_view_1d(self.memory_k, T * E, il * C * 2 * E), D, H, T),
                                     0, 2, 1, 3)  # :252-264
                kq = off(ctx0.op_mul_mat(kk, q))  # :267-279
                kq = off(ctx0.op_scale_inplace(kq, ctx0.new_f32(1.0 / np.sqrt(np.float32(E) / np.float32(H)))))
                kq = off(ctx0.op_diag_mask_inf_inplace(kq, P))
                kq = off(ctx0.op_soft_max_inplace(kq))
                vv = ctx0.op_view_3d(self.memory_v, T, D, H, C * 2, C * 2 * D, il * C * 2 * E)  # :282-290
                kqv = off(ctx0.op_mul_mat(vv, kq))  # :293
                cur = off(ctx0.op_cpy(ctx0.op_permute(kqv, 0, 2, 1, 3), ctx0.new_tensor(G.TYPE_F32, E, N)))  # :295-298
                cur = off(ctx0.op_mul_mat(t[p + "attention.dense.weight"], cur))  # :301-302
                cur = off(ctx0.op_add(cur, t[p + "attention.dense.bias"]))
                if not hp["use_parallel_residual"]:  # :308-314
                    ff_in = off(ctx0.op_add(cur, x))
                    x = off(ctx0.op_add(ffn(p, ff_in), ff_in))
                else:  # :315-330
                    cur = off(ctx0.op_add(ffn(p, x), cur))
                    x = off(ctx0.op_add(cur, x))
            x = ln(x, "gpt_neox.final_layer_norm")  # :333-336
            logits = ctx0.op_mul_mat(t["embed_out.weight"], x)  # :343, set_offloading(false)
            gf.build_forward_expand(logits)
            gf.compute()
            self.n_past = T
            return logits.read_data().reshape(N, V).copy()
        finally:
            ctx0.free()
