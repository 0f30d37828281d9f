"""The MPT chunk plan (backend option plan_mpt_chunk; csrc/plan_mpt_chunk.inc, csrc/kernels/mpt_chunk.h): evaluations of 2 .. 31
tokens of an MPT model — what feed_prompt feeds at the reference's default n_batch = 8 — against the restatement (alibi_ref.Mpt) under
the bound every MPT test here uses (EDGE), the plan's counters, and the forms it declines; and its device code alone through the hook
ggml_hip_debug_mpt_chunk: the LayerNorm columns against the executor's chain bit for bit, the K-sliced residual mat-vec and the
token-major Q|K|V pass against exact integer products, the position-split chunk attention against the f64 reference with ggml's rounding
points under twice the executor's own error.  The shapes are the smallest the plan takes:
E = 4096 (MPT-7B's width, 2 layers: down_proj has 512 blocks a row and runs as two K slices) and E = 1024 (unsliced)."""
import ctypes as C

import numpy as np
import pytest

import alibi_ref
import mul_mat_exact_ref as E
from llm_amd import mpt
from test_mpt_plan_gpu import EDGE, GUARD, _attn_ref, _bits, _executor_stage, _f16, _tie_row, _VariantMpt
from test_mpt_prompt_gpu import _attn_executor_n, _rows_vs_ref, _toks

pytestmark = pytest.mark.gpu

SHAPES = {"real": dict(mpt.MPT_7B, n_layer=2, n_vocab=512, n_ctx=64),
          "e1024": dict(mpt.MPT_TINY, n_embd=1024, n_head=8, n_vocab=512, n_ctx=64)}


def _stats(G):
    return G.get_stat("mpt_chunk_tokens"), G.get_stat("plan_tokens"), G.get_stat("generic_graphs")


def _feed(O, model, ref, toks, n_batch):
    """feed_prompt's loop, every evaluation against the restatement at the device's K/V state: |Δ|max / std per row"""
    d = []
    for i in range(0, len(toks), n_batch):
        d += _rows_vs_ref(O, model, ref, toks[i:i + n_batch])
    return d


@pytest.mark.parametrize("shape,wtype", [("real", 2), ("real", 8), ("e1024", 2), ("e1024", 8), ("e1024", 7)])
def test_chunks_of_a_prompt_match_restatement(G, O, shape, wtype):
    """19 tokens at n_batch = 8 (chunks of 8, 8 and 3) and one decode step, option 1 then 0: every row within EDGE of the restatement,
    mpt_chunk_tokens + 19 and no executor graph for the chunks; at option 0 the counter stands still (the parent's behaviour)"""
    hp, w = mpt.make_mpt(SHAPES[shape], wtype, seed=7)
    toks, d = _toks(8, 20, hp), {}
    try:
        for on in (1, 0):
            G.set_option("plan_mpt_chunk", on)
            model, ref = mpt.Mpt(hp, w), alibi_ref.Mpt(hp, w)
            c0, p0, g0 = _stats(G)
            d[on] = _feed(O, model, ref, toks[:19], 8)
            assert _stats(G) == ((c0 + 19, p0 + 19, g0) if on else (c0, p0, g0 + 3))
            d[on] += _rows_vs_ref(O, model, ref, toks[19:])  # a decode step behind the chunks (the executor's: plan_mpt is 0)
            assert G.get_stat("mpt_chunk_tokens") == c0 + 19 * on
            model.free()
    finally:
        G.set_option("plan_mpt_chunk", 0)
    print(f"{shape} type {wtype}: plan worst {max(d[1]):.2e}, executor worst {max(d[0]):.2e}")
    assert max(d[1]) <= EDGE, d[1]
    assert max(d[0]) <= EDGE, d[0]  # (the executor at option 0: the same bound, as before the option existed)


def test_twenty_tokens_in_three_passes(G, O):
    """one evaluation of 20 tokens (passes of 8, 8 and 4 columns) behind 3 tokens, so the chunk's rows start at an odd position"""
    hp, w = mpt.make_mpt(SHAPES["e1024"], 2, seed=7)
    toks = _toks(8, 23, hp)
    try:
        G.set_option("plan_mpt_chunk", 1)
        model, ref = mpt.Mpt(hp, w), alibi_ref.Mpt(hp, w)
        c0, _, g0 = _stats(G)
        d = _rows_vs_ref(O, model, ref, toks[:3]) + _rows_vs_ref(O, model, ref, toks[3:])
        assert (G.get_stat("mpt_chunk_tokens"), G.get_stat("generic_graphs")) == (c0 + 23, g0)
        model.free()
    finally:
        G.set_option("plan_mpt_chunk", 0)
    print(f"worst {max(d):.2e}")
    assert max(d) <= EDGE, d


@pytest.mark.parametrize("case", ["n1", "no_offload", "q4_k", "kv_f32", "e128"])
def test_declined_forms_run_on_the_executor(G, case):
    base = SHAPES["e1024"]
    hp0, wtype = {"q4_k": (base, 12), "e128": (mpt.MPT_TINY, 2)}.get(case, (base, 2))
    hp, w = mpt.make_mpt(hp0, wtype, seed=5)
    make = {"no_offload": lambda: mpt.Mpt(hp, w, offload=False), "kv_f32": lambda: _VariantMpt(hp, w, kv_type=G.TYPE_F32)}.get(case, lambda: mpt.Mpt(hp, w))
    toks, outs = _toks(6, 1 if case == "n1" else 8, hp), []
    try:
        for on in (1, 0):
            G.set_option("plan_mpt_chunk", on)
            model = make()
            c0, _, g0 = _stats(G)
            outs.append(model.evaluate(toks))
            assert _stats(G)[0] == c0 and _stats(G)[2] == g0 + 1
            model.free()
    finally:
        G.set_option("plan_mpt_chunk", 0)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


def test_a_chunk_behind_the_contexts_end_is_declined_by_the_matcher(G):
    hp, w = mpt.make_mpt(SHAPES["e1024"], 2, seed=5)
    model = mpt.Mpt(hp, w)
    try:
        G.set_option("plan_mpt_chunk", 1)
        for P, want in ((hp["n_ctx"] - 8, 1), (hp["n_ctx"] - 7, 0)):  # n_past + N = C, then C + 1: asked of the matcher alone, never run
            model.n_past = P
            ctx0 = model._ctx0(8, kq_copies=4)
            try:
                _, gf = _VariantMpt.build(model, ctx0, _toks(6, 8, hp))
                assert G.lib().ggml_hip_debug_mpt(3, 0, C.cast(gf.ptr, C.c_void_p), None, 0.0, 0, None, None, 0, 0, 0, 0, 0.0, None) == want
            finally:
                ctx0.free()
    finally:
        G.set_option("plan_mpt_chunk", 0)
        model.free()


# ---- the device code alone, through the hook ----
def _hook(G, op, flag, outs, w=None, x=None, gain=None, res=None, K=0, N=1, col0=0, P=0, Cc=0, mk=None, mv=None, H=0, D=0, scale=0.0):
    """one launch of the hook on byte buffers `outs` (each with room for its guard, which must come back whole)"""
    p = lambda a: None if a is None else a.ctypes.data
    arr = (C.c_void_p * 7)(*([p(o) for o in outs] + [None] * (7 - len(outs))))
    rc = G.lib().ggml_hip_debug_mpt_chunk(op, flag, w, p(x), p(gain), 1e-5, p(res), K, N, col0, P, Cc, p(mk), p(mv), H, D, scale, arr)
    assert rc == 0
    assert all((o[-GUARD:] == 0xFF).all() for o in outs if o is not None)


@pytest.mark.parametrize("f16d", [1, 0])
@pytest.mark.parametrize("K", [1024, 4096])
def test_layernorm_columns_equal_the_executors_chain(G, K, f16d):
    """planes, d, sum and the [block][8] tables, zero columns included, of 2, 8 and 9 rows: the executor's norm -> mul -> quantize bits"""
    rng = np.random.default_rng(K)
    gain = (1.0 + 0.01 * rng.standard_normal(K)).astype(np.float32)
    X = rng.standard_normal((9, K)).astype(np.float32)
    X[1], X[2] = _tie_row(K), np.full(K, 0.37, np.float32)
    X[7, K // 3] = X[8, 5] = 1e4
    want = [_executor_stage(G, X[r], gain, f16d) for r in range(9)]  # ((lo, hi, d, sum), y) per row
    nb = K // 32
    for N in (2, 8, 9):
        passes = (N + 7) // 8
        sizes = (N * K // 2, N * K // 2, N * nb * 4, N * nb * 4, passes * nb * 32, passes * nb * 32, N * K * 4)
        outs = [np.zeros(n + GUARD, np.uint8) for n in sizes]
        _hook(G, 0, f16d, outs, x=X[:N], gain=gain, K=K, N=N)
        lo, hi, d, sm, dT, sT, y = (o[:-GUARD] for o in outs)
        for i, what in enumerate(("lo", "hi", "d", "sum")):
            ref = np.concatenate([want[r][0][i].view(np.uint8) for r in range(N)])
            assert np.array_equal((lo, hi, d, sm)[i], ref), (N, what)
        assert np.array_equal(y, np.concatenate([want[r][1].view(np.uint8) for r in range(N)])), (N, "y")
        tabd, tabs = np.zeros((passes, nb, 8), np.float32), np.zeros((passes, nb, 8), np.int32)  # column r & 7 of table r >> 3, zeros behind N
        for r in range(N):
            tabd[r >> 3, :, r & 7], tabs[r >> 3, :, r & 7] = want[r][0][2], want[r][0][3]
        assert np.array_equal(dT, tabd.view(np.uint8).reshape(-1)) and np.array_equal(sT, tabs.view(np.uint8).reshape(-1)), (N, "tables")


def _exact_weight(G, ctx, t, M, K, N):
    """an exact-integer case (mul_mat_exact_ref): the device weight, X f32 [N][K], the product [N][M] (exact in any summation order) and
    the bound's scale |X| . |W|^T"""
    raw, W, X = E.exact_case(t, M, K, N, G.quantize)
    w = ctx.tensor_from(raw, t, (K, M)).set_name("w")
    w.transfer_to_gpu()
    return w, X.astype(np.float32), E.exact_product(X, W, 32), np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64).T


@pytest.mark.parametrize("t", [2, 8, 7])
@pytest.mark.parametrize("K,slices", [(16384, 2), (4096, 1)])
def test_sliced_residual_mat_vec_matches_the_exact_product(G, t, K, slices):
    """M = 32 rows, 9 columns (two passes): res + W x under the mat-vec bound of tests/test_ops_gpu.py; K = 16384 runs as two K slices"""
    M, N = 32, 9
    with G.Context(M * K * 2 + (1 << 20)) as ctx:
        w, X, ref, scale = _exact_weight(G, ctx, t, M, K, N)
        res = np.random.default_rng(K).integers(-64, 64, (N, M)).astype(np.float32)
        out = np.zeros(N * M * 4 + GUARD, np.uint8)
        _hook(G, 1, 0, [out], w=w.ptr, x=X, res=res, K=K, N=N)
        got = out[:-GUARD].view(np.float32).reshape(N, M)
        err = np.abs(got.astype(np.float64) - (ref.astype(np.float64) + res))
        assert np.all(err <= 2e-5 * scale + 1e-7), float(np.max(err / (scale + 1e-12)))
        if slices > 1:  # the plan's own choice was two slices: one slice is refused for this K
            arr = (C.c_void_p * 7)(out.ctypes.data, *([None] * 6))
            assert G.lib().ggml_hip_debug_mpt_chunk(1, 1, w.ptr, X.ctypes.data, None, 1e-5, res.ctypes.data, K, N, 0, 0, 0, None, None, 0, 0, 0.0, arr) == -1


@pytest.mark.parametrize("t", [2, 8])
def test_qkv_pass_writes_only_its_cache_rows(G, t):
    """E = 1024, columns 8 .. 10 of a chunk at n_past 5: Q exact, K and V the f16 of the exact product in rows 13 .. 15, every other byte its fill"""
    Ed, N, col0, P, Cc = 1024, 3, 8, 5, 24
    with G.Context(3 * Ed * Ed * 2 + (1 << 20)) as ctx:
        w, X, ref, scale = _exact_weight(G, ctx, t, 3 * Ed, Ed, N)
        mk, mv = (np.full(Cc * Ed * 2 + GUARD, f, np.uint8) for f in (0x5A, 0xA5))
        mk[-GUARD:] = mv[-GUARD:] = 0xFF
        out = np.zeros(N * Ed * 4 + GUARD, np.uint8)
        _hook(G, 2, 0, [out], w=w.ptr, x=X, K=Ed, N=N, col0=col0, P=P, Cc=Cc, mk=mk, mv=mv)
        assert (mk[-GUARD:] == 0xFF).all() and (mv[-GUARD:] == 0xFF).all()
        q = out[:-GUARD].view(np.float32).reshape(N, Ed)
        assert np.all(np.abs(q.astype(np.float64) - ref[:, :Ed]) <= 2e-5 * scale[:, :Ed] + 1e-7)
        for cache, fill, part in ((mk, 0x5A, ref[:, Ed:2 * Ed]), (mv, 0xA5, ref[:, 2 * Ed:])):
            rows = cache[:-GUARD].reshape(Cc, Ed * 2)
            keep = np.ones(Cc, bool)
            keep[P + col0:P + col0 + N] = False
            assert (rows[keep] == fill).all()
            assert np.array_equal(rows[~keep].reshape(-1).view(np.float16), part.astype(np.float32).astype(np.float16).reshape(-1))


# (D, H, n_past, N, S, kind)
ATTN_CASES = [(32, 4, 0, 2, 2, "random"),        # T = 2: the second range is empty
              (64, 4, 5, 8, 2, "random"),        # n_past odd
              (32, 4, 60, 8, 2, "random"),       # T = 68: the boundary at key 64 lies inside the chunk's own diagonal (queries at 60 .. 67)
              (128, 12, 994, 31, 8, "random"),   # T = 1025, heads 8 .. 11 on the second slope sequence, a full tile
              (32, 4, 200, 8, 8, "peaked_flat"),  # the maximum (key 5) in range 0 for every workgroup; query 0 is zero: the bias alone
              (64, 8, 300, 31, 16, "random")]


def test_chunk_attention_within_twice_the_executors_error(G):
    """Measured on an MI355X, worst |Δ|max / std over the cases: the executor's chain 3.555e-4, k_attn_chunk_*_alibi 3.708e-4 (both at D 64, H 8, n_past 300, N 31, S 16); T = 1025 at D 128: 1.117e-4 on both; the others 3.5e-8 .. 6.6e-7.  DESIGN.md section 4.3e."""
    err = {}
    for case in ATTN_CASES:
        D, H, P, N, S, kind = case
        rng = np.random.default_rng(1000 * D + 10 * H + P + N)
        E_, T = H * D, P + N
        Cc, bias_max = T + 3, 8.0
        slopes = alibi_ref.slopes(H, bias_max)
        scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
        q = rng.standard_normal((N, E_)).astype(np.float32)
        mk, mv = _f16(0.5 * rng.standard_normal((Cc, E_))), _f16(rng.standard_normal((Cc, E_)))
        if kind == "peaked_flat":
            mk[:] = 0
            q[0] = 0
            qq = _f16(q[-1]).astype(np.float64).reshape(H, D)
            mk[5] = _f16((30.0 / scale) * qq / (qq * qq).sum(axis=1, keepdims=True)).reshape(E_)
        mk[T:], mv[T:] = np.float16(np.nan), np.float16(np.nan)  # rows behind the last token: never read
        want = np.stack([_attn_ref(q[i], mk, mv, slopes, H, D, P + i + 1, scale) for i in range(N)])
        out = np.zeros(N * E_ * 4 + GUARD, np.uint8)
        _hook(G, 3, S, [out], x=q, gain=slopes, N=N, P=P, Cc=Cc, mk=mk.view(np.uint16), mv=mv.view(np.uint16), H=H, D=D, scale=scale)
        new = out[:-GUARD].view(np.float32).reshape(N, E_)
        assert np.isfinite(new).all(), case
        mk[T:], mv[T:] = 0, 0
        exe = _attn_executor_n(G, q, mk, mv, bias_max, H, D, P, N, Cc, scale)
        sd = float(want.std()) or 1.0
        err[case] = (float(np.max(np.abs(exe - want))) / sd, float(np.max(np.abs(new - want))) / sd)
    worst_exec, worst_new = (max(v[i] for v in err.values()) for i in (0, 1))
    print("executor worst %.3e, k_attn_chunk_*_alibi worst %.3e" % (worst_exec, worst_new), err)
    assert worst_new <= 2.0 * worst_exec, err
