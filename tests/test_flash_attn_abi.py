"""ggml_flash_attn at the drop-in boundary, without a device: the node it builds (op, shape, type, sources, op_params, one graph
node) for every accepted type combination and for the views LLaMA's graph hands it, and every rejection of the contract in
include/ggml_hip.h — each in a subprocess, as test_abi.py::test_out_of_path_ops_abort_not_fallback does: the library aborts
while the graph is built, with ggml_flash_attn and the violated rule in the message."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_FLASH_ATTN = 46  # include/ggml_hip.h enum ggml_op
MAX_KEYS = 37312    # internal.h FLASH_ATTN_MAX_KEYS: (150 KB - 256 - 4 x 1024) / 4, down to a multiple of 64
MAX_D = 1024


def test_op_code_is_the_headers(G):
    assert G.lib().ggml_op_name(OP_FLASH_ATTN) == b"FLASH_ATTN"
    assert MAX_KEYS == (150 * 1024 - 256 - 4 * MAX_D) // 4 // 64 * 64 and MAX_KEYS >= 8192


def _same(a, b):
    return C.addressof(a.contents) == C.addressof(b.t)


@pytest.mark.parametrize("tq,tkv", [("F32", "F32"), ("F16", "F16"), ("F32", "F16")])
@pytest.mark.parametrize("masked", [True, False])
def test_node_for_each_accepted_type_combination(G, tq, tkv, masked):
    D, N, M, H, B = 16, 3, 7, 4, 2
    with G.Context(1 << 22) as c:
        q = c.new_tensor(getattr(G, "TYPE_" + tq), D, N, H, B)
        k = c.new_tensor(getattr(G, "TYPE_" + tkv), D, M, H, B)
        v = c.new_tensor(getattr(G, "TYPE_" + tkv), M, D, H, B)
        y = c.op_flash_attn(q, k, v, masked)
        assert y.t.op == OP_FLASH_ATTN and y.t.type == G.TYPE_F32 and y.ne == (D, N, H, B) and y.t.n_dims == 4
        assert G.lib().ggml_is_contiguous(y.ptr) and y.nb == (4, 4 * D, 4 * D * N, 4 * D * N * H)
        assert y.t.data not in (q.t.data, k.t.data, v.t.data)  # a fresh tensor
        assert _same(y.t.src[0], q) and _same(y.t.src[1], k) and _same(y.t.src[2], v) and not y.t.src[3]
        assert y.t.op_params[0] == (1 if masked else 0)
        g = c.graph().build_forward_expand(y)
        assert g.n_nodes == 1 and g.n_leafs == 3 and g.node(0).t.op == OP_FLASH_ATTN


def test_llama_views_gqa_and_decode_are_accepted(G):
    """q as the permute(0, 2, 1, 3) view of [D, H, N], K and V as views into larger caches (free nb[1..3]), H a multiple of Hkv,
    a 3-D result for 3-D operands, a single query row, M == N, and rows at the limits."""
    D, H, Hkv, N, P, Cc = 32, 4, 2, 5, 9, 64
    M, Eg = N + P, Hkv * D
    with G.Context(1 << 24) as c:
        mk, mv = c.new_tensor(G.TYPE_F16, Cc * Eg), c.new_tensor(G.TYPE_F16, Cc * Eg)
        q = c.op_permute(c.new_tensor(G.TYPE_F32, D, H, N), 0, 2, 1, 3)
        assert q.ne == (D, N, H, 1) and not G.lib().ggml_is_contiguous(q.ptr)
        K = c.op_permute(c.op_reshape_3d(c.op_view_1d(mk, M * Eg, 0), D, Hkv, M), 0, 2, 1, 3)
        V = c.op_view_3d(mv, M, D, Hkv, Cc * 2, Cc * 2 * D, 0)
        assert K.ne == (D, M, Hkv, 1) and V.ne == (M, D, Hkv, 1) and V.nb[1] == Cc * 2
        y = c.op_flash_attn(q, K, V, True)
        assert y.ne == (D, N, H, 1) and y.t.n_dims == 3 and G.lib().ggml_is_contiguous(y.ptr)
        g = c.graph().build_forward_expand(y)
        assert [g.node(i).t.op for i in range(g.n_nodes)].count(OP_FLASH_ATTN) == 1 and g.node(g.n_nodes - 1).t.op == OP_FLASH_ATTN
        # decode: one row; M == N; a view that starts inside the cache (odd element offset: only element alignment is asked)
        q1 = c.new_tensor(G.TYPE_F32, D, 1, H)
        assert c.op_flash_attn(q1, K, V, True).ne == (D, 1, H, 1)
        K2 = c.op_view_3d(mk, D, N, Hkv, Eg * 2, D * 2, 2 * 3)
        V2 = c.op_view_3d(mv, N, D, Hkv, Cc * 2, Cc * 2 * D, 2 * 5)
        assert c.op_flash_attn(q, K2, V2, False).ne == (D, N, H, 1)
        # the limits themselves are inside
        kk = c.new_tensor(G.TYPE_F16, 1, MAX_KEYS)
        assert c.op_flash_attn(c.new_tensor(G.TYPE_F32, 1, 1), kk, c.new_tensor(G.TYPE_F16, MAX_KEYS, 1), True).ne[:2] == (1, 1)
        kd = c.new_tensor(G.TYPE_F32, MAX_D, 2)
        assert c.op_flash_attn(c.new_tensor(G.TYPE_F32, MAX_D, 2), kd, c.new_tensor(G.TYPE_F32, 2, MAX_D), False).ne[0] == MAX_D


# (what to build after `c`, D, N, M, H are set up;  words the message must hold)
REJECTIONS = {
    "types_f16_q_f32_kv": ("q = T(F16, D, N, H); k = T(F32, D, M, H); v = T(F32, M, D, H)", "types"),
    "types_mixed_kv": ("q = T(F32, D, N, H); k = T(F16, D, M, H); v = T(F32, M, D, H)", "types"),
    "types_quantized_k": ("q = T(F32, 32, N, H); k = T(G.TYPE_Q4_0, 32, M, H); v = T(F16, M, 32, H)", "types"),
    "v_ne0_is_not_m": ("q = T(F32, D, N, H); k = T(F16, D, M, H); v = T(F16, M + 1, D, H)", "v.ne[0] must equal k.ne[1]"),
    "v_ne1_is_not_d": ("q = T(F32, D, N, H); k = T(F16, D, M, H); v = T(F16, M, D + 1, H)", "v.ne[1] must equal D"),
    "k_ne0_is_not_d": ("q = T(F32, D, N, H); k = T(F16, D + 1, M, H); v = T(F16, M, D, H)", "k.ne[0] must equal q.ne[0]"),
    "m_below_n": ("q = T(F32, D, M + 1, H); k = T(F16, D, M, H); v = T(F16, M, D, H)", "M < N"),
    "heads_do_not_divide": ("q = T(F32, D, N, 3); k = T(F16, D, M, 2); v = T(F16, M, D, 2)", "heads"),
    "heads_k_v_differ": ("q = T(F32, D, N, 4); k = T(F16, D, M, 2); v = T(F16, M, D, 4)", "heads"),
    "batch_differs": ("q = T(F32, D, N, H, 2); k = T(F16, D, M, H, 1); v = T(F16, M, D, H, 1)", "batch"),
    "nb0_not_dense_q": ("q = c.op_transpose(T(F32, N, D, H)); k = T(F16, D, M, H); v = T(F16, M, D, H)", "nb[0] must be dense"),
    "nb0_not_dense_v": ("q = T(F32, D, N, H); k = T(F16, D, M, H); v = c.op_transpose(T(F16, D, M, H))", "nb[0] must be dense"),
    "m_beyond_lds": ("q = T(F32, 1, 1); k = T(F16, 1, %d); v = T(F16, %d, 1)" % (MAX_KEYS + 1, MAX_KEYS + 1), "FLASH_ATTN_MAX_KEYS = %d" % MAX_KEYS),
    "d_beyond_lds": ("q = T(F32, %d, 1); k = T(F32, %d, 2); v = T(F32, 2, %d)" % (MAX_D + 1, MAX_D + 1, MAX_D + 1), "FLASH_ATTN_MAX_D = %d" % MAX_D),
}


@pytest.mark.parametrize("name", sorted(REJECTIONS))
def test_rejections_abort_while_the_graph_is_built(G, name):
    build, words = REJECTIONS[name]
    code = ("import sys; sys.path.insert(0, %r); from llm_amd import ggml as G\n"
            "c = G.Context(1 << 22); F32, F16 = G.TYPE_F32, G.TYPE_F16; D, N, M, H = 16, 3, 7, 4\n"
            "T = c.new_tensor\n"
            "%s\n"
            "print('built', flush=True)\n"
            "c.op_flash_attn(q, k, v, True)\n"
            "print('accepted', flush=True)") % (ROOT, build)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert "built" in p.stdout and "accepted" not in p.stdout, (p.stdout, p.stderr)
    assert p.returncode != 0 and "ggml_flash_attn" in p.stderr and words in p.stderr, p.stderr
    assert "no CPU compute fallback" in p.stderr
