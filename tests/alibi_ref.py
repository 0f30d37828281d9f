"""CPU restatement of the ALiBi families' graphs for the tests (BLOOM, MPT: crates/models/{bloom,mpt}/src/lib.rs), in
the form of rotary_ref: NumPy orchestration over the oracle's C primitives (LayerNorm, quantized mul_mat in each oracle
mode, GELU, mask + softmax) plus a NumPy restatement of ggml's ALiBi.  Not a test module (pytest collects test_*.py
only).

ggml_compute_forward_alibi_f32 (restated from upstream ggml; its source is not in the reference):
  n_floor = 1 << (int)floor(log2(n_head)),  m0 = powf(2, -bias_max / n_floor),  m1 = powf(2, -(bias_max / 2) / n_floor)
  head k: m_k = powf(m0, k + 1) if k < n_floor, else powf(m1, 2*(k - n_floor) + 1)
  element (i, j, k) of KQ [n_past + N, N, n_head]: (float)i * m_k + x, an f32 product and an f32 sum (n_past unused).
powf is the C library's (ctypes), as the reference's CPU build calls it.

The attention step is the graph's out-of-place chain: an f32 scale by 1/sqrt(n_embd/n_head), then alibi, then the
oracle's mask + softmax with scale 1.0 (an exact identity).  K/V memory is f16 in the device's layout, both token-major:
memory_k, memory_v [L, C, E] (lib.rs view_1d stores), so a test can copy the device's cache in before each step."""
import numpy as np

import rotary_ref
from llm_amd import bloom, mpt
from oracle import oracle as O

_libm = rotary_ref._libm


def slopes(n_head, bias_max):
    """ggml's per-head slope table, f32 [n_head]."""
    n_floor = 1 << int(np.floor(np.log2(n_head)))
    b = np.float32(bias_max)
    m0 = np.float32(_libm.powf(np.float32(2.0), -b / np.float32(n_floor)))
    m1 = np.float32(_libm.powf(np.float32(2.0), -(b / np.float32(2.0)) / np.float32(n_floor)))
    return np.array([_libm.powf(m0, np.float32(k + 1)) if k < n_floor else
                     _libm.powf(m1, np.float32(2 * (k - n_floor) + 1)) for k in range(n_head)], np.float32)


def alibi(x, n_past, n_head, bias_max):
    """x: f32 [n_head, N, n_past + N] (numpy order; ggml [n_past + N, N, n_head]); returns the biased copy."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    H, N, nc = x.shape
    assert H == n_head and nc == n_past + N, (x.shape, n_past, n_head)
    pos = np.arange(nc, dtype=np.float32)
    return (pos[None, None, :] * slopes(n_head, bias_max)[:, None, None]) + x


class _AlibiFamily(rotary_ref._Family):
    """Embeddings, LayerNorm and mat-mul from rotary_ref._Family; attention with ALiBi over token-major K and V."""

    def __init__(self, hp, w, n_ctx):
        super().__init__(hp, w, n_ctx, hp["n_embd"], False)

    def _attend(self, il, q, k, v, mode, bias_max):
        """q, k, v [N, H, D] f32: stores k/v (f16) at n_past and returns the merged heads [N, H*D]: K·Q with src1
        rounded to f16 (F16 mul_mat), f32 scale, alibi, causal mask + softmax, V·P with P rounded to f16."""
        hp = self.hp
        N, H, D = q.shape
        P = self.n_past
        T = P + N
        self.memory_k[il, P:T] = k.reshape(N, -1).astype(np.float16)
        self.memory_v[il, P:T] = v.reshape(N, -1).astype(np.float16)
        Kf = self.memory_k[il, :T].astype(np.float32).reshape(T, H, D)
        Vf = self.memory_v[il, :T].astype(np.float32).reshape(T, H, D)
        f16r = (lambda a: a.astype(np.float16).astype(np.float32)) if mode != O.MODE_MATH else (lambda a: a)
        kq = np.einsum("thd,nhd->hnt", Kf.astype(np.float64), f16r(q).astype(np.float64)).astype(np.float32)
        scale = np.float32(1.0) / np.sqrt(np.float32(hp["n_embd"]) / np.float32(hp["n_head"]))
        kq = alibi(kq * scale, P, H, bias_max)
        pr = O.scale_mask_softmax(kq, 1.0, P, mode)
        kqv = np.einsum("thd,hnt->nhd", Vf.astype(np.float64), f16r(pr).astype(np.float64)).astype(np.float32)
        return kqv.reshape(N, H * D)


def _split_qkv(qkv, E, H):
    """[Q | K | V] blocks of n_embd columns (the graphs' view_2d at 0, E, 2E) -> three [N, H, D]."""
    N = qkv.shape[0]
    return [qkv[:, j * E:(j + 1) * E].reshape(N, H, E // H) for j in range(3)]


class Bloom(_AlibiFamily):
    """crates/models/bloom/src/lib.rs:116-342."""

    def __init__(self, hp, w, n_ctx=None):
        self.shapes = bloom.tensor_shapes(hp)
        super().__init__(hp, w, n_ctx)

    def evaluate(self, tokens, mode=0):
        hp, w = self.hp, self.w
        E, H, L = hp["n_embd"], hp["n_head"], hp["n_layer"]
        N, P = len(tokens), self.n_past
        x = self._ln(self._embed("tok_embeddings.weight", tokens), "norm")
        for il in range(L):
            p = f"layers.{il}."
            cur = self._ln(x, p + "attention_norm")
            qkv = self._mm(p + "attention.query_key_value.weight", cur, mode) + w[p + "attention.query_key_value.bias"]
            q, k, v = _split_qkv(qkv, E, H)
            cur = self._attend(il, q, k, v, mode, bloom.ALIBI_BIAS_MAX)
            cur = self._mm(p + "attention.wo.weight", cur, mode) + w[p + "attention.wo.bias"]
            ff_in = cur + x
            cur = self._ln(ff_in, p + "ffn_norm")
            cur = O.gelu(self._mm(p + "feed_forward.w1.weight", cur, mode) + w[p + "feed_forward.w1.bias"], mode)
            cur = self._mm(p + "feed_forward.w2.weight", cur, mode) + w[p + "feed_forward.w2.bias"]
            x = cur + ff_in
        x = self._ln(x, "output_norm")
        self.n_past = P + N
        return self._mm("output.weight", x, mode)


class Mpt(_AlibiFamily):
    """crates/models/mpt/src/lib.rs:93-259 (LayerNorms without bias, no linear biases, lm_head = wte)."""

    def __init__(self, hp, w, n_ctx=None):
        self.shapes = mpt.tensor_shapes(hp)
        super().__init__(hp, w, n_ctx)

    def evaluate(self, tokens, mode=0):
        hp, w = self.hp, self.w
        E, H, L = hp["n_embd"], hp["n_head"], hp["n_layer"]
        N, P = len(tokens), self.n_past
        x = self._embed("transformer.wte.weight", tokens)
        for il in range(L):
            p = f"transformer.blocks.{il}."
            cur = O.norm(x) * w[p + "norm_1.weight"]
            q, k, v = _split_qkv(self._mm(p + "attn.Wqkv.weight", cur, mode), E, H)
            cur = self._attend(il, q, k, v, mode, hp["alibi_bias_max"])
            x = x + self._mm(p + "attn.out_proj.weight", cur, mode)
            cur = O.norm(x) * w[p + "norm_2.weight"]
            cur = O.gelu(self._mm(p + "ffn.up_proj.weight", cur, mode), mode)
            x = x + self._mm(p + "ffn.down_proj.weight", cur, mode)
        x = O.norm(x) * w["transformer.norm_f.weight"]
        self.n_past = P + N
        return self._mm("transformer.wte.weight", x, mode)
