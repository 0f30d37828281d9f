"""GGML_OP_FLASH_ATTN on the device (kernels/flash_attn.h: k_flash_attn_tile, k_flash_attn_row) against the host reference of
tests/flash_attn_ref.py, through the C ABI only: Context, views, graph compute (tests/flash_attn_graph.py).  q is the
permute(0, 2, 1, 3) view of [D, H, N]; K and V are views into caches whose rows >= M are NaN, so a read behind M shows as NaN.

 exact families (one-hot, spread: P is predicted bit for bit with the device's own exp table): EVERY element within the
   reference's accumulation bound M 2^-23 sum |v| p, one-hot rows equal to their target key's V row bit for bit, no NaN.
 Gaussian family: every element inside the interval propagated through every rounding point.
The shapes are the smallest at which each kernel can still go wrong (CASES); which kernel a shape runs on is the launcher's rule
(plan_shapes.inc flash_attn_tile_queries), restated in _tile().  The worst err / bound of each case is printed."""
import numpy as np
import pytest

import flash_attn_graph as FG
import flash_attn_ref as F

pytestmark = pytest.mark.gpu

MAX_KEYS_TILE = 2368


@pytest.fixture(scope="module")
def tab(G):
    """e(arg) of the kernels for all f16 bit patterns: exp_le0's table (held to expf / f64 exp in test_prompt_plan_gpu.py)."""
    fast = np.zeros(65536, np.uint16)
    ref = np.zeros(65536, np.uint16)
    assert G.lib().ggml_hip_debug_exp_le0(fast.ctypes.data, ref.ctypes.data) == 0
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    t = fast.view(np.float16)
    assert np.all(t[x <= -20] == 0) and t[0xFC00] == 0 and t[0] == 1 and t[0x8000] == 1  # what the one-hot family relies on
    neg = 0x8000 | np.arange(0x7C01)
    assert np.array_equal(fast[neg], ref[neg])  # ... and the unfused chain's expf gives the same table on arg <= 0
    return fast


def _tile(D, N, M, C, f32):
    """The launcher's rule: the MFMA kernel takes f16 K/V, D in {32, 64, 128}, N >= 2, M <= 2368 and 16-byte aligned rows
    (a cache of C keys: V rows are 2 C bytes apart, K rows 2 Hkv D)."""
    return (not f32) and D in (32, 64, 128) and N >= 2 and M <= MAX_KEYS_TILE and C % 8 == 0


# name: (kernel, B, N, H, Hkv, D, M, C, masked, f32)
CASES = {
    "tile_second_query_tile_batch": ("tile", 2, 33, 2, 2, 32, 64, 72, True, False),   # P = 31; key-tile border 32 / 64; batch stride
    "tile_gqa_ragged_keys": ("tile", 1, 17, 4, 2, 128, 65, 72, True, False),          # P = 48; M = 65 is no tile multiple
    "tile_unmasked": ("tile", 1, 5, 2, 2, 64, 70, 72, False, False),                  # P ignored
    "row_decode_one_key": ("row", 1, 1, 2, 1, 128, 1, 8, True, False),
    "row_decode": ("row", 1, 1, 2, 1, 128, 97, 104, True, False),
    "row_decode_unaligned_cache": ("row", 1, 1, 2, 1, 128, 97, 99, True, False),      # V rows 198 bytes apart: element loads
    "row_head_size_80": ("row", 1, 3, 2, 1, 80, 33, 40, True, False),                 # P = 30
    "row_f32_masked": ("row", 1, 4, 2, 2, 32, 37, 40, True, True),
    "row_f32_unmasked_unaligned": ("row", 1, 4, 2, 2, 32, 37, 39, False, True),       # V rows 156 bytes apart
    "row_longest_decode": ("row", 1, 1, 2, 1, 64, 8192, 8192, True, False),
    "tile_longest_row": ("tile", 1, 32, 2, 1, 64, 2300, 2304, True, False),           # P = 2268: 16 queries per workgroup
    "row_beyond_the_tile_limit": ("row", 1, 2, 1, 1, 32, 2369, 2376, True, False),    # first M the tile kernel refuses
}


def _inputs(family, B, N, H, Hkv, D, M, C, f32):
    q, k, v = getattr(F, family + "_inputs")(B, N, H, Hkv, D, M, C)
    if C > M:
        assert np.isnan(k[:, M:].astype(np.float32)).all() and np.isnan(v[:, :, M:].astype(np.float32)).all()
    return (q,) + (F.as_f32_caches(k, v) if f32 else (k, v))


def _check_exact(tag, got, ref, v, H, Hkv, D):
    """One-hot rows bit for bit, every other element within the accumulation bound.  Returns the worst err / bound."""
    assert not np.isnan(got).any(), (tag, "unwritten or NaN output", np.argwhere(np.isnan(got))[:4].tolist())
    r = H // Hkv
    one = ref["target"] >= 0
    want = np.zeros(got.shape, np.float32)
    for h in range(H):
        cols = v[(h // r) * D:(h // r + 1) * D][:, np.where(one[h], ref["target"][h], 0)].T.astype(np.float32)  # [N][D]
        want[h] = cols
    mask = np.broadcast_to(one[:, :, None], got.shape)
    bad = mask & (got.view(np.uint32) != want.view(np.uint32))
    assert not bad.any(), (tag, "one-hot row differs from its V row", int(bad.sum()), np.argwhere(bad)[0].tolist())
    err = np.abs(got.astype(np.float64) - ref["out"])
    over = ~mask & (err > ref["bound"])
    if over.any():
        h, n, d = np.argwhere(over)[0]
        raise AssertionError((tag, "outside the accumulation bound", int(over.sum()), "first: head %d row %d channel %d" % (h, n, d),
                              float(got[h, n, d]), float(ref["out"][h, n, d]), "bound", float(ref["bound"][h, n, d])))
    sel = ~mask & (ref["bound"] > 0)
    return float((err[sel] / ref["bound"][sel]).max()) if sel.any() else 0.0


@pytest.mark.parametrize("name", list(CASES))
def test_exact_families_every_element(G, tab, name):
    kernel, B, N, H, Hkv, D, M, C, masked, f32 = CASES[name]
    assert _tile(D, N, M, C, f32) == (kernel == "tile"), "the case no longer runs on the kernel it is named for"
    for family in ("onehot", "spread"):
        q, k, v = _inputs(family, B, N, H, Hkv, D, M, C, f32)
        got = FG.run(G, q, k, v, D, H, Hkv, M, masked)
        n_one = 0
        worst = 0.0
        for b in range(B):
            ref = F.reference(q[b], k[b], v[b], H, Hkv, M, masked, tab, f32)
            n_one += int((ref["target"] >= 0).sum())
            worst = max(worst, _check_exact((name, family, "batch", b), got[b], ref, v[b], H, Hkv, D))
        if family == "onehot":
            assert n_one > 0, "the one-hot family must hold one-hot rows"
        print("%-30s %-7s one-hot rows %4d of %4d, worst err / bound %.3f" % (name, family, n_one, B * N * H, worst))


@pytest.mark.parametrize("name", list(CASES))
def test_gaussian_family_inside_the_interval(G, tab, name):
    kernel, B, N, H, Hkv, D, M, C, masked, f32 = CASES[name]
    q, k, v = _inputs("gauss", B, N, H, Hkv, D, M, C, f32)
    got = FG.run(G, q, k, v, D, H, Hkv, M, masked)
    assert not np.isnan(got).any()
    for b in range(B):
        lo, hi = F.interval(q[b], k[b], v[b], H, Hkv, M, masked, tab, f32)
        g = got[b].astype(np.float64)
        out = (g < lo) | (g > hi)
        pos = float(np.max(np.maximum(lo - g, g - hi) / np.maximum(hi - lo, 1e-300)))
        print("%-30s gauss batch %d: widest interval %.2e, worst excess / width %+.3f" % (name, b, float((hi - lo).max()), pos))
        assert not out.any(), (name, b, int(out.sum()), np.argwhere(out)[:4].tolist())


@pytest.mark.parametrize("name", ["tile_gqa_ragged_keys", "row_decode", "row_head_size_80"])
def test_f16_q_equals_f32_q_of_the_same_values(G, name):
    """The extension: q F32 against f16 K/V is rounded to f16 when loaded, so with f16-exact values both forms are bit-equal."""
    kernel, B, N, H, Hkv, D, M, C, masked, f32 = CASES[name]
    for family in ("spread", "gauss"):
        q, k, v = _inputs(family, B, N, H, Hkv, D, M, C, False)
        q = q.astype(np.float16).astype(np.float32)
        a = FG.run(G, q, k, v, D, H, Hkv, M, masked, q_f16=False)
        b = FG.run(G, q, k, v, D, H, Hkv, M, masked, q_f16=True)
        assert not np.isnan(a).any() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, family)


@pytest.mark.parametrize("name", ["tile_gqa_ragged_keys", "row_decode"])
def test_node_and_unfused_chain_lie_in_the_same_interval(G, tab, name):
    """mul_mat(K, Q) -> scale -> diag_mask_inf -> soft_max -> mul_mat(V, P) of this library (held to the oracle elsewhere) and the
    node, on a Gaussian case of each kernel: both inside the interval.  Their difference is printed for information only — the
    two accumulate in different orders."""
    kernel, B, N, H, Hkv, D, M, C, masked, f32 = CASES[name]
    q, k, v = _inputs("gauss", B, N, H, Hkv, D, M, C, False)
    node = FG.run(G, q, k, v, D, H, Hkv, M, masked)
    chain = FG.run(G, q, k, v, D, H, Hkv, M, masked, unfused=True)
    lo, hi = F.interval(q[0], k[0], v[0], H, Hkv, M, masked, tab)
    delta = float(np.abs(node - chain).max())
    print("%-30s node vs unfused chain: max |delta| %.3e, widest interval %.2e" % (name, delta, float((hi - lo).max())))
    for what, x in (("node", node[0]), ("chain", chain[0])):
        g = x.astype(np.float64)
        out = (g < lo) | (g > hi)
        assert not np.isnan(x).any() and not out.any(), (name, what, int(out.sum()), "max |node - chain| = %.3e (information)" % delta)


def test_counter_advances_and_the_plans_leave_the_graph_alone(G):
    """flash_attn_nodes advances by one per computed node and generic_graphs advances: the graph went node by node."""
    kernel, B, N, H, Hkv, D, M, C, masked, f32 = CASES["tile_unmasked"]
    q, k, v = _inputs("gauss", B, N, H, Hkv, D, M, C, False)
    n0, g0, p0, pp0 = (G.get_stat(s) for s in ("flash_attn_nodes", "generic_graphs", "plan_tokens", "prompt_plan_tokens"))
    FG.run(G, q, k, v, D, H, Hkv, M, masked)
    FG.run(G, q[:, :1], k, v, D, H, Hkv, M, True)
    assert G.get_stat("flash_attn_nodes") == n0 + 2 and G.get_stat("generic_graphs") == g0 + 2
    assert G.get_stat("plan_tokens") == p0 and G.get_stat("prompt_plan_tokens") == pp0
    with G.Context(FG.context_bytes(q, k, v, H, M)) as c:  # two nodes in one graph
        Q, K, V = FG.operands(c, G, q, k, v, D, H, Hkv, M)
        y = c.op_add(FG.flash(c, Q, K, V, True), FG.flash(c, Q, K, V, False))
        assert c.graph().build_forward_expand(y).compute() == 0
    assert G.get_stat("flash_attn_nodes") == n0 + 4 and G.get_stat("generic_graphs") == g0 + 3
