"""GPT-J through the drop-in C ABI: the graph of crates/models/gptj/src/lib.rs:134-300 built node by node with the
ctypes binding (llm_amd.ggml) and executed by ggml_graph_compute on the MI355X (generic executor).  Separate q/k/v
projections without biases; mode-0 RoPE with n_rot < head_dim (ggml's whole-row semantics: n_rot only sets the
frequency step, kernels/ops.h k_rope); the FFN runs in parallel with attention off the same LayerNorm output; lm_head
has a bias.  Synthetic weights follow the loader's names (lib.rs:59-103); 2-D weights are quantized, gains and biases
stay f32."""
import numpy as np

from . import ggml as G
from ._resident import Resident, make_weights

GPTJ_6B = dict(n_vocab=50400, n_ctx=2048, n_embd=4096, n_head=16, n_layer=28, n_rot=64)
GPTJ_TINY = dict(n_vocab=256, n_ctx=64, n_embd=128, n_head=4, n_layer=2, n_rot=8)


def tensor_shapes(hp):
    """name -> (ne0, ne1 or None); 2-D weights are [in_features (ne0), out_features (ne1)]."""
    E, V = hp["n_embd"], hp["n_vocab"]
    s = {"transformer.wte.weight": (E, V), "transformer.ln_f.weight": (E, None), "transformer.ln_f.bias": (E, None),
         "lm_head.weight": (E, V), "lm_head.bias": (V, None)}
    for i in range(hp["n_layer"]):
        p = f"transformer.h.{i}."
        s[p + "ln_1.weight"] = (E, None)
        s[p + "ln_1.bias"] = (E, None)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s[p + f"attn.{n}.weight"] = (E, E)
        s[p + "mlp.fc_in.weight"] = (E, 4 * E)
        s[p + "mlp.fc_in.bias"] = (4 * E, None)
        s[p + "mlp.fc_out.weight"] = (4 * E, E)
        s[p + "mlp.fc_out.bias"] = (E, None)
    return s


def make_gptj(hp0, wtype, seed=1234, quantize=None):
    """ggml-layout weights: dict name -> raw block bytes (quantized 2-D) or f32 array."""
    hp = dict(hp0, wtype=wtype)
    shapes = tensor_shapes(hp)
    gains = {n for n in shapes if n.endswith("ln_1.weight") or n == "transformer.ln_f.weight"}
    return hp, make_weights(shapes, wtype, seed, quantize, gains)


class GptJ(Resident):
    """Model (weights resident on the device) + one session (f16 K/V memory, V stored transposed)."""

    def __init__(self, hp, w, n_ctx=None):
        super().__init__(hp, w, tensor_shapes(hp), hp["n_embd"], n_ctx)

    def evaluate(self, tokens):
        """GptJ::evaluate (lib.rs:134-300): returns logits [N, n_vocab]."""
        hp, t = self.hp, self.t
        E, H, L, V, R = hp["n_embd"], hp["n_head"], hp["n_layer"], hp["n_vocab"], hp["n_rot"]
        D, N, P, C = E // H, len(tokens), self.n_past, self.C
        T = P + N
        ctx0 = self._ctx0(N)
        try:
            off = lambda x: x.offload()  # ctx0.set_offloading(true): intermediate results stay on the device
            x = off(ctx0.op_get_rows(t["transformer.wte.weight"], ctx0.tensor_from(np.asarray(tokens, np.int32))))
            gf = ctx0.graph()

            def ln(a, name):
                return off(ctx0.op_add(off(ctx0.op_mul(off(ctx0.op_norm(a)), t[name + ".weight"])), t[name + ".bias"]))

            for il in range(L):
                p = f"transformer.h.{il}."
                cur = ln(x, p + "ln_1")  # :168-172, = input_sa
                q = off(ctx0.op_mul_mat(t[p + "attn.q_proj.weight"], cur))  # :178-201 mode 0, n_rot of head_dim
                qcur = off(ctx0.op_rope_inplace(ctx0.op_reshape_3d(q, D, H, N), P, R, 0, 0))
                k = off(ctx0.op_mul_mat(t[p + "attn.k_proj.weight"], cur))
                kcur = off(ctx0.op_rope_inplace(ctx0.op_reshape_3d(k, D, H, N), P, R, 0, 0))
                vcur = ctx0.op_transpose(off(ctx0.op_mul_mat(t[p + "attn.v_proj.weight"], cur)))  # :204-205
                km = ctx0.op_view_1d(self.memory_k, N * E, 2 * E * (il * C + P))  # :207-217
                vm = ctx0.op_view_2d(self.memory_v, N, E, C * 2, il * C * 2 * E + P * 2)
                gf.build_forward_expand(off(ctx0.op_cpy(kcur, km)))  # :219-220
                gf.build_forward_expand(off(ctx0.op_cpy(vcur, vm)))
                qq = ctx0.op_permute(qcur, 0, 2, 1, 3)  # :222
                kk = ctx0.op_permute(ctx0.op_reshape_3d(ctx0.op_view_1d(self.memory_k, T * E, il * C * 2 * E), D, H, T),
                                     0, 2, 1, 3)  # :223-235
                kq = off(ctx0.op_mul_mat(kk, qq))  # :237-244
                kq = off(ctx0.op_scale_inplace(kq, ctx0.new_f32(1.0 / np.sqrt(np.float32(E) / np.float32(H)))))
                kq = off(ctx0.op_diag_mask_inf_inplace(kq, P))
                kq = off(ctx0.op_soft_max_inplace(kq))
                vv = ctx0.op_view_3d(self.memory_v, T, D, H, C * 2, C * 2 * D, il * C * 2 * E)  # :246-254
                kqv = off(ctx0.op_mul_mat(vv, kq))  # :256
                att = off(ctx0.op_cpy(ctx0.op_permute(kqv, 0, 2, 1, 3), ctx0.new_tensor(G.TYPE_F32, E, N)))  # :257-262
                att = off(ctx0.op_mul_mat(t[p + "attn.out_proj.weight"], att))  # :265-268, = ff_in
                ff = off(ctx0.op_add(off(ctx0.op_mul_mat(t[p + "mlp.fc_in.weight"], cur)), t[p + "mlp.fc_in.bias"]))
                ff = off(ctx0.op_gelu(ff))  # :270-277
                ff = off(ctx0.op_add(off(ctx0.op_mul_mat(t[p + "mlp.fc_out.weight"], ff)), t[p + "mlp.fc_out.bias"]))
                x = off(ctx0.op_add(off(ctx0.op_add(ff, att)), x))  # :279-282
            x = ln(x, "transformer.ln_f")  # :286-287
            logits = off(ctx0.op_mul_mat(t["lm_head.weight"], x))  # :292
            logits = ctx0.op_add(logits, t["lm_head.bias"])  # :294-296, set_offloading(false)
            gf.build_forward_expand(logits)
            gf.compute()
            self.n_past = T
            return logits.read_data().reshape(N, V).copy()
        finally:
            ctx0.free()
