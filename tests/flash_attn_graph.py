"""Builds GGML_OP_FLASH_ATTN graphs through the C ABI the way LLaMA's graph lays its operands out, for
tests/test_flash_attn_gpu.py and tests/tools/flash_attn_bench.py.  Not a test module.

Arrays (tests/flash_attn_ref.py): q [B][N][H D], k cache [B][C][Hkv D], v cache [B][Hkv D][C] (transposed), C >= M.
  Q = permute(0, 2, 1, 3) of the tensor [D, H, N, B]                              -> [D, N, H, B]
  K = view of the K cache: rows of one head D apart, keys Hkv D apart             -> [D, M, Hkv, B]
  V = view of the V cache: keys contiguous, channels C apart                      -> [M, D, Hkv, B]
This ABI has ggml_view_3d and no ggml_view_4d; for B > 1 the views' fourth dimension is written into the tensor header
(ne[3], nb[3], n_dims), which is all ggml_view_4d does upstream."""
import numpy as np


def _batched(t, B, nb3):
    if B > 1:
        t.t.ne[3] = B
        t.t.nb[3] = nb3
        t.t.n_dims = 4
    return t


def operands(c, G, q, kc, vc, D, H, Hkv, M, q_f16=False):
    B, N, E = q.shape
    C_, Eg = kc.shape[1], Hkv * D
    assert E == H * D and kc.shape == (B, C_, Eg) and vc.shape == (B, Eg, C_) and kc.dtype == vc.dtype and M <= C_
    es = kc.dtype.itemsize
    tq = c.tensor_from(q.astype(np.float16) if q_f16 else q.astype(np.float32), ne=(D, H, N, B) if B > 1 else (D, H, N))
    Q = c.op_permute(tq, 0, 2, 1, 3)
    mk = c.tensor_from(kc, ne=(B * C_ * Eg,))
    mv = c.tensor_from(vc, ne=(B * Eg * C_,))
    K = _batched(c.op_view_3d(mk, D, M, Hkv, Eg * es, D * es, 0), B, C_ * Eg * es)
    V = _batched(c.op_view_3d(mv, M, D, Hkv, C_ * es, C_ * D * es, 0), B, Eg * C_ * es)
    return Q, K, V


def flash(c, Q, K, V, masked):
    return c.op_flash_attn(Q, K, V, masked)


def chain(c, Q, K, V, D, P, masked):
    """The unfused form: mul_mat(K, Q) -> scale -> diag_mask_inf -> soft_max -> mul_mat(V, P), in place as LLaMA builds it."""
    scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    kq = c.op_scale_inplace(c.op_mul_mat(K, Q), c.new_f32(scale))
    if masked:
        kq = c.op_diag_mask_inf_inplace(kq, P)
    return c.op_mul_mat(V, c.op_soft_max_inplace(kq))


def context_bytes(q, kc, vc, H, M):
    """Room for the operands, the result, the unfused chain's [M, N, H, B] scores and the graph."""
    B, N, E = q.shape
    return int(2 * q.nbytes + kc.nbytes + vc.nbytes + B * N * E * 4 + B * H * N * M * 4 + (1 << 22))


def run(G, q, kc, vc, D, H, Hkv, M, masked, q_f16=False, unfused=False):
    """Computes the node (or the unfused chain) on the device; returns out [B][H][N][D] f32."""
    B, N, _ = q.shape
    with G.Context(context_bytes(q, kc, vc, H, M)) as c:
        Q, K, V = operands(c, G, q, kc, vc, D, H, Hkv, M, q_f16)
        y = chain(c, Q, K, V, D, M - N, masked) if unfused else flash(c, Q, K, V, masked)
        assert c.graph().build_forward_expand(y).compute() == 0
        return y.read_data(np.float32).reshape(B, H, N, D)
