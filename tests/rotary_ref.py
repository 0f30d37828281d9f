"""CPU restatement of the rotary-embedding families' graphs for the tests (GPT-NeoX, Falcon, GPT-J:
crates/models/{gptneox,falcon,gptj}/src/lib.rs), in the form of oracle.Gpt2: NumPy orchestration over the oracle's C
primitives (LayerNorm, quantized mul_mat in each oracle mode, GELU, scale + mask + softmax, mode-0 RoPE) plus a NumPy
restatement of ggml's NeoX-mode RoPE.  Not a test module (pytest collects test_*.py only).

K/V memory is f16 in the device's layout, so a test can copy the device's cache in before each step:
  GPT-NeoX, GPT-J: memory_k [L, C, E] (token-major), memory_v [L, E, C] (transposed, lib.rs V view_2d stores);
  Falcon:          memory_k, memory_v [L, C, n_head_kv*head_dim] (token-major)."""
import ctypes
import ctypes.util

import numpy as np

from llm_amd import falcon, gptj, gptneox
from oracle import oracle as O

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
for _f in ("cosf", "sinf"):
    getattr(_libm, _f).restype = ctypes.c_float
    getattr(_libm, _f).argtypes = [ctypes.c_float]
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def rope_neox(x, n_past, n_dims, freq_base=10000.0, freq_scale=1.0, mode=2):
    """ggml_compute_forward_rope_f32, NeoX branch (mode & 2).  x: f32 [N, n_head, ne0] (numpy order; ggml
    [ne0, n_head, N]); returns the rotated copy.  For each n_dims block ib and ic = 0, 2, .., n_dims-2, the pair
    (i0, i0 + n_dims/2), i0 = ib*n_dims + ic/2, turns by theta, an f32 product iterated one step per pair from
    freq_scale*p and carried on across blocks; cosf/sinf/powf are the C library's.  Elements past
    (ne0/n_dims)*n_dims keep their value, and so do the rows i2 < n_past under mode & 1 (ggml's i2 loop starts there)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = x.copy()
    N, _, ne0 = x.shape
    half, nblk = n_dims // 2, ne0 // n_dims
    theta_scale = np.float32(_libm.powf(np.float32(freq_base), np.float32(-2.0) / np.float32(n_dims)))
    k = np.arange(nblk * half)
    i0 = (k // half) * n_dims + k % half
    for i2 in range(N):
        if mode & 1 and i2 < n_past:
            continue
        theta = np.float32(freq_scale) * np.float32(i2 if mode & 1 else n_past + i2)
        c = np.empty(k.size, np.float32)
        s = np.empty(k.size, np.float32)
        for j in range(k.size):
            c[j], s[j] = _libm.cosf(theta), _libm.sinf(theta)
            theta = np.float32(theta * theta_scale)
        x0, x1 = x[i2][:, i0], x[i2][:, i0 + half]
        y[i2][:, i0] = x0 * c - x1 * s
        y[i2][:, i0 + half] = x0 * s + x1 * c
    return y


class _Family:
    """Shared pieces: embeddings, LayerNorm with gain and bias, quantized mat-mul, attention over the f16 cache."""

    def __init__(self, hp, w, n_ctx, kv_width, v_transposed):
        self.hp, self.w = hp, w
        self.C = n_ctx or hp["n_ctx"]
        L = hp["n_layer"]
        self.memory_k = np.zeros((L, self.C, kv_width), np.float16)
        self.memory_v = np.zeros((L, kv_width, self.C) if v_transposed else (L, self.C, kv_width), np.float16)
        self.v_transposed = v_transposed
        self.n_past = 0

    def _mm(self, name, x, mode):
        return O.mul_mat(self.hp["wtype"], self.w[name], self.shapes[name][1], x.shape[-1], x, mode)

    def _ln(self, x, name):
        return O.norm(x) * self.w[name + ".weight"] + self.w[name + ".bias"]

    def _embed(self, name, tokens):
        t, E = self.hp["wtype"], self.hp["n_embd"]
        rb = O.row_bytes(t, E)
        return np.stack([O.dequantize(t, self.w[name][int(tok) * rb:(int(tok) + 1) * rb], E) for tok in tokens])

    def _attend(self, il, q, k, v, mode):
        """q [N, H, D], k/v [N, Hkv, D] f32: stores k/v (f16) at n_past and returns the merged heads [N, H*D]:
        K·Q with src1 rounded to f16 (F16 mul_mat), scale 1/sqrt(n_embd/n_head) + causal mask + softmax, V·P."""
        hp = self.hp
        N, H, D = q.shape
        Hkv, P = k.shape[1], self.n_past
        T = P + N
        self.memory_k[il, P:T] = k.reshape(N, -1).astype(np.float16)
        if self.v_transposed:
            self.memory_v[il, :, P:T] = v.reshape(N, -1).T.astype(np.float16)
            Vf = self.memory_v[il, :, :T].T.astype(np.float32).reshape(T, Hkv, D)
        else:
            self.memory_v[il, P:T] = v.reshape(N, -1).astype(np.float16)
            Vf = self.memory_v[il, :T].astype(np.float32).reshape(T, Hkv, D)
        Kf = self.memory_k[il, :T].astype(np.float32).reshape(T, Hkv, D)
        grp = np.arange(H) // (H // Hkv)  # ggml's mul_mat broadcast of src0's heads: i02 = i12 / (ne12/ne02)
        Kf, Vf = Kf[:, grp], Vf[:, grp]
        f16r = (lambda a: a.astype(np.float16).astype(np.float32)) if mode != O.MODE_MATH else (lambda a: a)
        kq = np.einsum("thd,nhd->hnt", Kf.astype(np.float64), f16r(q).astype(np.float64)).astype(np.float32)
        scale = np.float32(1.0) / np.sqrt(np.float32(hp["n_embd"]) / np.float32(hp["n_head"]))
        pr = O.scale_mask_softmax(kq, scale, P, mode)
        kqv = np.einsum("thd,hnt->nhd", Vf.astype(np.float64), f16r(pr).astype(np.float64)).astype(np.float32)
        return kqv.reshape(N, H * D)


class GptNeoX(_Family):
    """crates/models/gptneox/src/lib.rs:156-350 (both use_parallel_residual forms)."""

    def __init__(self, hp, w, n_ctx=None):
        self.shapes = gptneox.tensor_shapes(hp)
        super().__init__(hp, w, n_ctx, hp["n_embd"], True)

    def evaluate(self, tokens, mode=0):
        hp, w = self.hp, self.w
        E, H, L, R = hp["n_embd"], hp["n_head"], hp["n_layer"], hp["n_rot"]
        D, N, P = E // H, len(tokens), self.n_past
        x = self._embed("gpt_neox.embed_in.weight", tokens)

        def ffn(p, a):
            cur = self._ln(a, p + "post_attention_layernorm")
            cur = self._mm(p + "mlp.dense_h_to_4h.weight", cur, mode) + w[p + "mlp.dense_h_to_4h.bias"]
            cur = O.gelu(cur, mode)
            return self._mm(p + "mlp.dense_4h_to_h.weight", cur, mode) + w[p + "mlp.dense_4h_to_h.bias"]

        for il in range(L):
            p = f"gpt_neox.layers.{il}."
            cur = self._ln(x, p + "input_layernorm")
            qkv = self._mm(p + "attention.query_key_value.weight", cur, mode) + w[p + "attention.query_key_value.bias"]
            qkv = qkv.reshape(N, H, 3, D)  # per head: q, k, v (view_3d with nb1 = row/n_head)
            q = rope_neox(qkv[:, :, 0], P, R)
            k = rope_neox(qkv[:, :, 1], P, R)
            cur = self._attend(il, q, k, qkv[:, :, 2], mode)
            cur = self._mm(p + "attention.dense.weight", cur, mode) + w[p + "attention.dense.bias"]
            if not hp["use_parallel_residual"]:
                ff_in = cur + x
                x = ffn(p, ff_in) + ff_in
            else:
                x = (ffn(p, x) + cur) + x
        x = self._ln(x, "gpt_neox.final_layer_norm")
        self.n_past = P + N
        return self._mm("embed_out.weight", x, mode)


class Falcon(_Family):
    """crates/models/falcon/src/lib.rs:153-370 (7B form n_head_kv == 1, 40B form n_head_kv > 1)."""

    def __init__(self, hp, w, n_ctx=None):
        self.shapes = falcon.tensor_shapes(hp)
        self._norm_names = falcon._norm_names
        super().__init__(hp, w, n_ctx, hp["n_head_kv"] * (hp["n_embd"] // hp["n_head"]), False)

    def evaluate(self, tokens, mode=0):
        hp = self.hp
        E, H, Hkv, L = hp["n_embd"], hp["n_head"], hp["n_head_kv"], hp["n_layer"]
        D, N, P = E // H, len(tokens), self.n_past
        x = self._embed("transformer.word_embeddings.weight", tokens)
        for il in range(L):
            p = f"transformer.h.{il}."
            in_norm, attn_norm = self._norm_names(hp, il)
            ln_out = self._ln(x, in_norm)
            cur = ln_out if attn_norm is None else self._ln(x, attn_norm)
            qkv = self._mm(p + "self_attention.query_key_value.weight", cur, mode).reshape(N, H + 2 * Hkv, D)
            q = rope_neox(qkv[:, :H], P, D)
            k = rope_neox(qkv[:, H:H + Hkv], P, D)
            att = self._attend(il, q, k, qkv[:, H + Hkv:], mode)
            att = self._mm(p + "self_attention.dense.weight", att, mode)
            ff = O.gelu(self._mm(p + "mlp.dense_h_to_4h.weight", ln_out, mode), mode)
            ff = self._mm(p + "mlp.dense_4h_to_h.weight", ff, mode)
            x = (ff + att) + x
        x = self._ln(x, "transformer.ln_f")
        self.n_past = P + N
        return self._mm("lm_head.weight", x, mode)


class GptJ(_Family):
    """crates/models/gptj/src/lib.rs:134-300 (mode-0 RoPE over the whole head row, n_rot sets its step)."""

    def __init__(self, hp, w, n_ctx=None):
        self.shapes = gptj.tensor_shapes(hp)
        super().__init__(hp, w, n_ctx, hp["n_embd"], True)

    def evaluate(self, tokens, mode=0):
        hp, w = self.hp, self.w
        E, H, L, R = hp["n_embd"], hp["n_head"], hp["n_layer"], hp["n_rot"]
        D, N, P = E // H, len(tokens), self.n_past
        x = self._embed("transformer.wte.weight", tokens)
        for il in range(L):
            p = f"transformer.h.{il}."
            cur = self._ln(x, p + "ln_1")
            q = O.rope(self._mm(p + "attn.q_proj.weight", cur, mode).reshape(N, H, D), P, R)
            k = O.rope(self._mm(p + "attn.k_proj.weight", cur, mode).reshape(N, H, D), P, R)
            v = self._mm(p + "attn.v_proj.weight", cur, mode).reshape(N, H, D)
            att = self._mm(p + "attn.out_proj.weight", self._attend(il, q, k, v, mode), mode)
            ff = O.gelu(self._mm(p + "mlp.fc_in.weight", cur, mode) + w[p + "mlp.fc_in.bias"], mode)
            ff = self._mm(p + "mlp.fc_out.weight", ff, mode) + w[p + "mlp.fc_out.bias"]
            x = (ff + att) + x
        x = self._ln(x, "transformer.ln_f")
        self.n_past = P + N
        return self._mm("lm_head.weight", x, mode) + w["lm_head.bias"]
