"""The MPT prompt plan (backend option plan_mpt_prompt; csrc/plan_match.inc match_mpt_decode at N rows, plan_mpt_prompt.inc, kernels/mpt_prompt.h):
evaluations of mmq_min tokens and more of llm_amd.mpt's offloaded graph as nine launches per layer.  Every test restores the option to 0.
Op level through ggml_hip_debug_mpt_prompt: k_p_attn_alibi against tests/test_mpt_plan_gpu.py's f64 reference row by row, at twice the
executor's own error; the LayerNorm and GELU operands and the K/V rows bit for bit against the executor's chain.  Whole model: the
restatement tests/alibi_ref.py at the device's K/V state, EDGE per row (the bounds and their reason are tests/test_mpt_plan_gpu.py's)."""
import ctypes as C

import numpy as np
import pytest

import act_quant_ref
import alibi_ref
from llm_amd import mpt
from test_mpt_plan_gpu import EDGE, GUARD, MPT_12H, SEEDS, STRICT, _attn_ref, _bits, _dev_set, _f16, _kv, _VariantMpt

pytestmark = pytest.mark.gpu

CTX = 128  # 40 + 33 prompt tokens and six steps
SHAPES = {"tiny": dict(mpt.MPT_TINY, n_ctx=CTX), "12h": dict(MPT_12H, n_ctx=CTX)}
MPT_REAL = dict(mpt.MPT_7B, n_layer=2, n_vocab=512, n_ctx=64)


def _toks(seed, n, hp):
    return np.random.default_rng(seed).integers(0, hp["n_vocab"], n).astype(np.int32)


def _stats(G):
    return G.get_stat("mpt_prompt_tokens"), G.get_stat("prompt_plan_tokens"), G.get_stat("generic_graphs")


def _hook(G, what, flag, shape, dtype, x, x2=None, r=None, w=None, K=0, N=1, mk=None, mv=None, H=0, D=0, P=0, Cc=0, scale=0.0, n_out=1):
    """one launch of the hook; the outputs without their guards, which must have come back whole"""
    p = lambda a: None if a is None else a.ctypes.data
    bufs = [np.zeros(int(np.prod(shape)) * np.dtype(dt).itemsize + GUARD, np.uint8) for dt in (dtype, np.float32)[:n_out]]
    outs = (C.c_void_p * 2)(*([b.ctypes.data for b in bufs] + [None] * (2 - n_out)))
    assert G.lib().ggml_hip_debug_mpt_prompt(what, flag, p(x), p(x2), p(r), p(w), 1e-5, K, N, p(mk), p(mv), H, D, P, Cc, scale, outs) == 0
    assert all((b[-GUARD:] == 0xFF).all() for b in bufs)
    return [b[:-GUARD].view(dt).reshape(shape) for b, dt in zip(bufs, (dtype, np.float32))]


def _graph_rows(G, x, build):
    """a small graph on host rows x [N][K], node by node on the executor: build(ctx, tensor) -> the result node"""
    ctx = G.Context(4 * 1024 * 1024 + 16 * x.nbytes)
    y = build(ctx, ctx.tensor_from(x))
    gf = ctx.graph()
    gf.build_forward_expand(y)
    gf.compute()
    out = y.read_data().reshape(x.shape).copy()
    ctx.free()
    return out


def _operand(G, y, f16d):
    """the executor's quantizer on rows y, the GEMM operand formed as f16(d * q) in the k order: uint16 bits"""
    N, K = y.shape
    lo, hi, d, s = (np.zeros(n + GUARD, np.uint8) for n in (N * K // 2, N * K // 2, N * K // 8, N * K // 8))
    outs = (C.c_void_p * 7)(lo.ctypes.data, hi.ctypes.data, d.ctypes.data, s.ctypes.data, None, None, None)
    assert G.lib().ggml_hip_debug_act_quant(0, f16d, N, K, K, y.ctypes.data, None, None, None, 0.0, 0, 0, outs) == 0
    q = np.concatenate([lo[:N * K // 2].view(np.int8).reshape(-1, 16), hi[:N * K // 2].view(np.int8).reshape(-1, 16)], axis=1)
    return act_quant_ref.f16_operand(q, d[:N * K // 8].view(np.float32)).reshape(N, K)


# ---- 1. the plan takes it ----
def test_prompts_run_on_the_plan(G):
    hp, w = mpt.make_mpt(SHAPES["tiny"], 2, seed=5)
    model, toks = mpt.Mpt(hp, w), _toks(6, 146, hp)
    try:
        for on, at in ((1, 0), (0, 73)):
            G.set_option("plan_mpt_prompt", on)
            if not on:
                model.n_past = 0
            for n0, n in ((at, 40), (at + 40, 33)):
                m0, p0, g0 = _stats(G)
                out = model.evaluate(toks[n0:n0 + n])
                assert out.shape == (n, hp["n_vocab"]) and np.isfinite(out).all()
                assert _stats(G) == ((m0 + n, p0 + n, g0) if on else (m0, p0, g0 + 1))
    finally:
        G.set_option("plan_mpt_prompt", 0)
        model.free()


# ---- 2. the attention, every output row ----
def _attn_executor_n(G, q, mk, mv, bias_max, H, D, P, N, Cc, scale):
    """mpt.py's attention nodes on host tensors with N query rows, node by node on the executor"""
    E, T = H * D, P + N
    ctx = G.Context(8 * 1024 * 1024 + 8 * Cc * E + 64 * T * H * N)
    try:
        tk, tv = ctx.tensor_from(mk.reshape(-1)), ctx.tensor_from(mv.reshape(-1))
        tq = ctx.op_permute(ctx.tensor_from(q.reshape(N, H, D)), 0, 2, 1, 3)
        kk = ctx.op_permute(ctx.op_reshape_3d(ctx.op_view_1d(tk, T * E, 0), D, H, T), 0, 2, 1, 3)
        kq = ctx.op_alibi(ctx.op_scale(ctx.op_mul_mat(kk, tq), ctx.new_f32(np.float32(scale))), P, H, bias_max)
        kq = ctx.op_soft_max(ctx.op_diag_mask_inf(kq, P))
        vt = ctx.op_cpy(ctx.op_permute(ctx.op_reshape_3d(ctx.op_view_1d(tv, T * E, 0), D, H, T), 1, 2, 0, 3), ctx.new_tensor(G.TYPE_F16, T, D, H))
        out = ctx.op_cpy(ctx.op_permute(ctx.op_mul_mat(vt, kq), 0, 2, 1, 3), ctx.new_tensor(G.TYPE_F32, E, N))
        gf = ctx.graph()
        gf.build_forward_expand(out)
        gf.compute()
        return out.device_get().astype(np.float64).reshape(N, E)
    finally:
        ctx.free()


ATTN_CASES = [(32, 4, 0, 32, "random"), (32, 4, 0, 33, "random"), (64, 4, 5, 40, "random"), (128, 12, 0, 64, "random"), (128, 12, 31, 34, "random"),
              (32, 4, 7, 32, "peaked_flat"),
              # T = 1089: one key past 1088, the longest rows 32 score rows + the V staging fit in 152 KiB (mpt_attn_queries, kernels/mpt_prompt.h)
              (128, 2, 1057, 32, "random")]


def test_prompt_attention_within_twice_the_executors_error(G):
    """Measured on an MI355X, worst |Δ|max / std over the cases: the executor's chain 2.608e-3, k_p_attn_alibi 2.608e-3 (both at D 128, H 12,
    n_past 31, N 34); the other cases 2.4e-7 .. 1.3e-4 on both.  DESIGN.md section 4.3d."""
    err = {}
    for case in ATTN_CASES:
        D, H, P, N, kind = case
        rng = np.random.default_rng(1000 * D + 10 * H + P + N)
        E, T = H * D, P + N
        Cc, bias_max = T + 3, 8.0
        slopes = alibi_ref.slopes(H, bias_max)
        scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
        q = rng.standard_normal((N, E)).astype(np.float32)
        mk, mv = _f16(0.5 * rng.standard_normal((Cc, E))), _f16(rng.standard_normal((Cc, E)))
        if kind == "peaked_flat":  # K = 0 but row 5 along the last query (its score 30 above the rest); query 0 is zero: its row is the bias alone
            mk[:] = 0
            q[0] = 0
            qq = _f16(q[-1]).astype(np.float64).reshape(H, D)
            mk[5] = _f16((30.0 / scale) * qq / (qq * qq).sum(axis=1, keepdims=True)).reshape(E)
        mk[T:], mv[T:] = np.float16(np.nan), np.float16(np.nan)  # rows behind the last token: never read
        qkv = np.full((N, 3 * E), np.nan, np.float32)  # the K and V columns of the product: not the attention's
        qkv[:, :E] = q
        want = np.stack([_attn_ref(q[i], mk, mv, slopes, H, D, P + i + 1, scale) for i in range(N)])
        new = _hook(G, 2, 0, (N, E), np.float32, qkv, w=slopes, N=N, mk=mk.view(np.uint16), mv=mv.view(np.uint16), H=H, D=D, P=P, Cc=Cc, scale=scale)[0]
        assert np.isfinite(new).all(), case
        mk[T:], mv[T:] = 0, 0
        exe = _attn_executor_n(G, q, mk, mv, bias_max, H, D, P, N, Cc, scale)
        sd = float(want.std()) or 1.0
        err[case] = (float(np.max(np.abs(exe - want))) / sd, float(np.max(np.abs(new - want))) / sd)
    worst_exec, worst_new = (max(v[i] for v in err.values()) for i in (0, 1))
    print("executor worst %.3e, k_p_attn_alibi worst %.3e" % (worst_exec, worst_new), err)
    assert worst_new <= 2.0 * worst_exec, err


# ---- 3. / 4. the operands, bit for bit ----
@pytest.mark.parametrize("res", [0, 1])
@pytest.mark.parametrize("f16d", [1, 0])
@pytest.mark.parametrize("K", [128, 4096])
def test_layernorm_operand_equals_the_executors_chain(G, K, f16d, res):
    rng = np.random.default_rng(K + res)
    gain = (1.0 + 0.01 * rng.standard_normal(K)).astype(np.float32)
    x = np.stack([rng.standard_normal(K), np.full(K, 0.37), rng.standard_normal(K)]).astype(np.float32)
    x[2, K // 3] = 1e4
    x2, r = (0.1 * rng.standard_normal((2, 3, K))).astype(np.float32) if res else (None, None)
    xs = (x + x2) + r if res else x  # the kernel's order: the second partial, then the residual
    y = _graph_rows(G, xs, lambda ctx, t: ctx.op_mul(ctx.op_norm(t), ctx.tensor_from(gain)))
    got = _hook(G, 0, f16d, (3, K), np.uint16, x, x2, r, gain, K=K, N=3, n_out=1 + res)
    assert np.array_equal(got[0], _operand(G, y, f16d))
    assert not res or np.array_equal(_bits(got[1]), _bits(xs))


@pytest.mark.parametrize("part", [0, 1])
@pytest.mark.parametrize("F", [512, 16384])
def test_gelu_operand_equals_the_executors_chain(G, F, part):
    rng = np.random.default_rng(F + part)
    x = (2.0 * rng.standard_normal((2, F))).astype(np.float32)
    x2 = (0.1 * rng.standard_normal((2, F))).astype(np.float32) if part else None
    y = _graph_rows(G, x + x2 if part else x, lambda ctx, t: ctx.op_gelu(t))
    for f16d in (1, 0):
        assert np.array_equal(_hook(G, 1, f16d, (2, F), np.uint16, x, x2, K=F, N=2)[0], _operand(G, y, f16d))


# ---- 5. the K/V rows ----
def test_prompt_writes_only_its_cache_rows(G):
    hp, w = mpt.make_mpt(SHAPES["tiny"], 3, seed=5)
    L, E, toks = hp["n_layer"], hp["n_embd"], _toks(6, 40, hp)
    junk = (0x3000 + np.arange(L * CTX * E) % 0x0800).astype(np.uint16)  # recognisable, finite
    kv = []
    try:
        for on in (1, 0):
            G.set_option("plan_mpt_prompt", on)
            model = mpt.Mpt(hp, w)
            _dev_set(G, model.memory_k, junk)
            _dev_set(G, model.memory_v, junk[::-1])
            model.n_past = 3
            m0 = G.get_stat("mpt_prompt_tokens")
            model.evaluate(toks)
            assert G.get_stat("mpt_prompt_tokens") == m0 + 40 * on
            kv.append([a.reshape(L, CTX, E) for a in _kv(model)])
            model.free()
    finally:
        G.set_option("plan_mpt_prompt", 0)
    for got, twin, was in zip(kv[0], kv[1], (junk, junk[::-1])):
        was = was.reshape(L, CTX, E)
        assert np.array_equal(got[:, :3], was[:, :3]) and np.array_equal(got[:, 43:], was[:, 43:])
        assert np.array_equal(got[0, 3:43], twin[0, 3:43]) and not np.array_equal(got[0, 3:43], was[0, 3:43])


# ---- 6. / 7. the whole model against the restatement ----
def _rows_vs_ref(O, model, ref, toks):
    """one evaluation on the device against the restatement at the device's K/V state: |Δ|max / std per row"""
    P = model.n_past
    got = model.evaluate(toks)
    ref.memory_k[:] = model.memory_k.device_get(np.float16).reshape(ref.memory_k.shape)
    ref.memory_v[:] = model.memory_v.device_get(np.float16).reshape(ref.memory_v.shape)
    ref.n_past = P
    want = ref.evaluate(toks, mode=O.ref_mode())
    return list(np.max(np.abs(got - want), axis=1) / want.std(axis=1))


@pytest.mark.parametrize("shape,wtype", [(sh, t) for sh in ("tiny", "12h") for t in (2, 3, 6, 7, 8)] + [("real", 2)])
def test_prompt_rows_match_restatement(G, O, shape, wtype):
    """two evaluations, 40 tokens and 33 more; `real`: MPT-7B's width, 2 layers, one evaluation of 64 tokens (EDGE only, as everywhere here)"""
    ws, ts = SEEDS.get(shape, (7, 8))
    hp, w = mpt.make_mpt(SHAPES.get(shape, MPT_REAL), wtype, seed=ws)
    n1, n = (64, 64) if shape == "real" else (40, 73)
    toks, d = _toks(ts, n, hp), {}
    try:
        for on in (1, 0):
            G.set_option("plan_mpt_prompt", on)
            model, ref = mpt.Mpt(hp, w), alibi_ref.Mpt(hp, w)
            m0 = G.get_stat("mpt_prompt_tokens")
            d[on] = _rows_vs_ref(O, model, ref, toks[:n1]) + (_rows_vs_ref(O, model, ref, toks[n1:]) if n > n1 else [])
            assert G.get_stat("mpt_prompt_tokens") == m0 + n * on
            model.free()
    finally:
        G.set_option("plan_mpt_prompt", 0)
    print(f"{shape} type {wtype}: plan worst {max(d[1]):.2e}, {sum(x <= STRICT for x in d[1])}/{n} within {STRICT}; "
          f"executor worst {max(d[0]):.2e}, {sum(x <= STRICT for x in d[0])}/{n}")
    assert max(d[1]) <= EDGE, d[1]


@pytest.mark.parametrize("plan_mpt", [0, 1])
def test_steps_behind_a_plan_prompt(G, O, plan_mpt):
    hp, w = mpt.make_mpt(SHAPES["tiny"], 2, seed=5)
    model, ref, toks = mpt.Mpt(hp, w), alibi_ref.Mpt(hp, w), _toks(6, 46, hp)
    try:
        G.set_option("plan_mpt_prompt", 1)
        G.set_option("plan_mpt", plan_mpt)
        m0, s0 = G.get_stat("mpt_prompt_tokens"), G.get_stat("mpt_plan_tokens")
        model.evaluate(toks[:40])
        d = [_rows_vs_ref(O, model, ref, toks[i:i + 1])[0] for i in range(40, 46)]
        assert (G.get_stat("mpt_prompt_tokens"), G.get_stat("mpt_plan_tokens")) == (m0 + 40, s0 + 6 * plan_mpt)
    finally:
        G.set_option("plan_mpt_prompt", 0)
        G.set_option("plan_mpt", 0)
        model.free()
    print(f"plan_mpt {plan_mpt}: worst {max(d):.2e}", d)
    assert max(d) <= EDGE, d


# ---- 8. declines: on the executor, bit-identical to option 0 ----
@pytest.mark.parametrize("case", ["n31", "no_offload", "q4_k", "f16", "d16", "kv_f32"])
def test_declined_forms_run_on_the_executor(G, case):
    base = dict(mpt.MPT_TINY, n_ctx=CTX)
    hp0, wtype = {"q4_k": (dict(base, n_embd=256, n_head=8), 12), "f16": (base, 1), "d16": (dict(mpt.MPT_TINY_12H, n_ctx=CTX), 2)}.get(case, (base, 2))
    hp, w = mpt.make_mpt(hp0, wtype, seed=5)
    make = {"no_offload": lambda: mpt.Mpt(hp, w, offload=False), "kv_f32": lambda: _VariantMpt(hp, w, kv_type=G.TYPE_F32)}.get(case, lambda: mpt.Mpt(hp, w))
    toks, outs = _toks(6, 31 if case == "n31" else 40, hp), []
    try:
        for on in (1, 0):
            G.set_option("plan_mpt_prompt", on)
            model = make()
            m0, _, g0 = _stats(G)
            outs.append(model.evaluate(toks))
            assert _stats(G)[0] == m0 and _stats(G)[2] == g0 + 1
            model.free()
    finally:
        G.set_option("plan_mpt_prompt", 0)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


def test_a_prompt_behind_the_contexts_end_is_declined_by_the_matcher(G):
    hp, w = mpt.make_mpt(SHAPES["tiny"], 2, seed=5)
    model = mpt.Mpt(hp, w)
    try:
        G.set_option("plan_mpt_prompt", 1)
        for P, want in ((CTX - 40, 1), (CTX - 39, 0)):  # n_past + N = C, then C + 1: asked of the matcher alone, never run
            model.n_past = P
            ctx0 = model._ctx0(40, kq_copies=4)
            try:
                _, gf = _VariantMpt.build(model, ctx0, _toks(6, 40, hp))
                assert G.lib().ggml_hip_debug_mpt(3, 0, C.cast(gf.ptr, C.c_void_p), None, 0.0, 0, None, None, 0, 0, 0, 0, 0.0, None) == want
            finally:
                ctx0.free()
    finally:
        G.set_option("plan_mpt_prompt", 0)
        model.free()
