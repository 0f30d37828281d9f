"""The MPT decode plan (backend option plan_mpt; csrc/plan_match.inc match_mpt_decode, plan_decode.inc plan_launch_mpt, kernels/mpt_plan.h):
single-token steps of llm_amd.mpt's offloaded graph as five launches per layer, replayed from a captured graph, and Mpt.infer_tokens_device's
greedy chain on it.  Every test that sets plan_mpt restores it to 0 (the default, which tests/test_alibi_families_gpu.py pins).

Against the reference: the form, the bounds and their reasons are tests/test_alibi_families_gpu.py's — the CPU restatement tests/alibi_ref.py in
O.ref_mode() with the device's K/V copied in before every step, |Δ|max / std per step; EDGE = 8e-2 for every step (one flipped int8 quant of these
random-init models), at tiny width at least half of the steps within STRICT = 1e-5, at real width EDGE only.  The quota is the reference's own to
keep first: its scalar branch against its AVX2 branch on the same cases (weights seed, token seed; a 5-token prompt, then the 6 single steps, K/V
copied across), run on the CPU for types 2, 3, 6, 7, 8: tiny with seeds (5, 6) keeps 5, 6, 5, 5, 6 of 6 steps within STRICT; the 12-head variant
keeps 3, 4, 5, 3, 3 with (5, 6), 3, 5, 4, 2, 4 with (11, 12), 6, 2, 6, 2, 5 with (13, 14), 5, 5, 6, 3, 5 with (15, 16) and 5, 4, 5, 5, 5 with
(17, 18): (17, 18) it is, the one pair that leaves every type a step of room above the quota of 3.  The 12-head variant here has n_embd 384
(head size 32): MPT_TINY_12H's head size 16 is not the plan's and must decline.  Measured on an MI355X with these seeds: 8 of the 10 cases have
6 of 6 steps within STRICT, tiny Q5_0 5 (worst 1.7e-2), 12-head Q5_1 3 (worst 9.9e-3); real width worst 5.0e-2; the slope mutant 0.87 .. 1.40.

Op level (ggml_hip_debug_mpt): the LayerNorm staging's Q8 blocks are the executor's k_norm -> mul -> k_quantize_act chain's bit for bit; the ALiBi
attention is held to an f64 host reference with ggml's rounding points (q, K and P as f16, f32 elsewhere) at twice the worst error the executor's
own chain (k_mul_mat_f16, k_soft_max<true, true>, the V copy, k_mul_mat_f16) shows against that reference on the same inputs — the order of the f32
accumulation is the only licensed difference.  The measured pair is printed by the test and stands in its docstring and in DESIGN.md section 4.3c."""
import ctypes as C

import numpy as np
import pytest

import alibi_ref
from llm_amd import mpt

pytestmark = pytest.mark.gpu

STRICT, EDGE = 1e-5, 8e-2
MPT_12H = dict(mpt.MPT_TINY, n_embd=384, n_head=12)  # head size 32; heads 8..11 take ggml's second slope sequence
MPT_REAL = dict(mpt.MPT_7B, n_layer=2, n_vocab=512, n_ctx=64)
SEEDS = {"tiny": (5, 6), "12h": (17, 18)}  # (weights, tokens): see the module docstring
SHAPES = {"tiny": mpt.MPT_TINY, "12h": MPT_12H}
GUARD = 256


class plan_on:
    """plan_mpt = 1 inside, 0 behind it whatever happens."""

    def __init__(self, G):
        self.G = G

    def __enter__(self):
        self.G.set_option("plan_mpt", 1)

    def __exit__(self, *a):
        self.G.set_option("plan_mpt", 0)


def _kv(model):
    return model.memory_k.device_get(np.float16).view(np.uint16).copy(), model.memory_v.device_get(np.float16).view(np.uint16).copy()


def _dev_set(G, tensor, arr):
    """the device image of an offloaded tensor (the caches): ggml_hip_tensor_set"""
    arr = np.ascontiguousarray(arr)
    G.lib().ggml_hip_tensor_set(tensor.ptr, arr.ctypes.data, 0, arr.nbytes)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _step_vs_ref(O, model, ref, tok):
    """one single-token step on the device against the restatement at the device's K/V state: |Δ|max / std"""
    got = model.evaluate(np.array([tok], np.int32))
    ref.memory_k[:] = model.memory_k.device_get(np.float16).reshape(ref.memory_k.shape)
    ref.memory_v[:] = model.memory_v.device_get(np.float16).reshape(ref.memory_v.shape)
    ref.n_past = model.n_past - 1
    want = ref.evaluate(np.array([tok], np.int32), mode=O.ref_mode())
    return float(np.max(np.abs(got - want))) / float(want.std())


# ---- 1. the feature is on ----
def test_single_token_steps_run_on_the_plan(G):
    hp, w = mpt.make_mpt(mpt.MPT_TINY, 2, seed=5)
    model = mpt.Mpt(hp, w)
    try:
        model.evaluate(np.array([3, 1, 4, 1, 5], np.int32))
        with plan_on(G):
            g0, m0, r0 = G.get_stat("generic_graphs"), G.get_stat("mpt_plan_tokens"), G.get_stat("graph_replays")
            for tok in (1, 5, 9):
                model.evaluate(np.array([tok], np.int32))
            assert G.get_stat("mpt_plan_tokens") == m0 + 3
            assert G.get_stat("generic_graphs") == g0
            assert G.get_stat("graph_replays") == r0 + 3
            assert model.n_past == 8
        g0, m0, p0 = G.get_stat("generic_graphs"), G.get_stat("mpt_plan_tokens"), G.get_stat("plan_tokens")
        for tok in (2, 6):
            model.evaluate(np.array([tok], np.int32))
        assert (G.get_stat("generic_graphs"), G.get_stat("mpt_plan_tokens"), G.get_stat("plan_tokens")) == (g0 + 2, m0, p0)
    finally:
        G.set_option("plan_mpt", 0)
        model.free()


# ---- 2. against the reference ----
@pytest.mark.parametrize("wtype", [2, 3, 6, 7, 8])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_plan_steps_match_restatement(G, O, shape, wtype):
    ws, ts = SEEDS[shape]
    hp, w = mpt.make_mpt(SHAPES[shape], wtype, seed=ws)
    toks = np.random.default_rng(ts).integers(0, hp["n_vocab"], 11).astype(np.int32)
    model, ref = mpt.Mpt(hp, w), alibi_ref.Mpt(hp, w)
    try:
        with plan_on(G):
            model.evaluate(toks[:5])  # (five tokens: not the plan's, the executor)
            m0 = G.get_stat("mpt_plan_tokens")
            d = [_step_vs_ref(O, model, ref, int(t)) for t in toks[5:]]
            assert G.get_stat("mpt_plan_tokens") == m0 + 6
    finally:
        G.set_option("plan_mpt", 0)
        model.free()
    print(f"{shape} type {wtype}: worst {max(d):.2e}, {sum(x <= STRICT for x in d)}/{len(d)} within {STRICT}", d)
    assert max(d) <= EDGE, d
    assert sum(x <= STRICT for x in d) >= len(d) // 2, d


def test_plan_steps_match_restatement_real_width(G, O):
    hp, w = mpt.make_mpt(MPT_REAL, G.TYPE_Q4_0, seed=7)
    toks = np.random.default_rng(8).integers(0, hp["n_vocab"], 12).astype(np.int32)
    model, ref = mpt.Mpt(hp, w), alibi_ref.Mpt(hp, w)
    try:
        with plan_on(G):
            model.evaluate(toks[:8])
            m0 = G.get_stat("mpt_plan_tokens")
            d = [_step_vs_ref(O, model, ref, int(t)) for t in toks[8:]]
            assert G.get_stat("mpt_plan_tokens") == m0 + 4
    finally:
        G.set_option("plan_mpt", 0)
        model.free()
    print(f"real width: worst {max(d):.2e}", d)
    assert max(d) <= EDGE, d  # no STRICT quota at this width: tests/test_alibi_families_gpu.py


# ---- 3. the slope mutant: test 2 sees the ALiBi path ----
def test_slope_mutant_leaves_edge(G, O):
    hp, w = mpt.make_mpt(MPT_12H, 2, seed=5)
    toks = np.random.default_rng(6).integers(0, hp["n_vocab"], 11).astype(np.int32)
    model, ref = mpt.Mpt(hp, w), alibi_ref.Mpt(hp, w)
    hook = G.lib().ggml_hip_debug_mpt
    try:
        with plan_on(G):
            model.evaluate(toks[:5])
            assert hook(2, 1, None, None, 0.0, 0, None, None, 0, 0, 0, 0, 0.0, None) == 0
            m0 = G.get_stat("mpt_plan_tokens")
            d = [_step_vs_ref(O, model, ref, int(t)) for t in toks[5:]]
            assert G.get_stat("mpt_plan_tokens") == m0 + 6
    finally:
        hook(2, 0, None, None, 0.0, 0, None, None, 0, 0, 0, 0, 0.0, None)
        G.set_option("plan_mpt", 0)
        model.free()
    print("slope mutant:", d)
    assert min(d) > EDGE, d  # every step: positions 5 .. 10 of heads 8 .. 11 are biased by the wrong sequence


# ---- 4. exact properties ----
def _prompted(hp, w, n_ctx=None, prompt=(3, 1, 4, 1, 5)):
    model = mpt.Mpt(hp, w, n_ctx=n_ctx)
    if len(prompt):
        model.evaluate(np.array(prompt, np.int32))
    return model


def _only_row_changed(before, after, L, Cc, E, P):
    b, a = before.reshape(L, Cc, E), after.reshape(L, Cc, E)
    same = np.ones(Cc, bool)
    same[P] = False
    return np.array_equal(b[:, same], a[:, same])


def test_step_writes_only_its_cache_row(G):
    hp, w = mpt.make_mpt(mpt.MPT_TINY, 3, seed=5)
    L, Cc, E = hp["n_layer"], hp["n_ctx"], hp["n_embd"]
    model = _prompted(hp, w)
    try:
        junk = np.random.default_rng(1).integers(0, 0x7bff, L * Cc * E).astype(np.uint16).reshape(L, Cc, E)
        for mem in (model.memory_k, model.memory_v):  # rows the session has not reached: recognisable
            cur = mem.device_get(np.float16).view(np.uint16).reshape(L, Cc, E).copy()
            cur[:, 5:] = junk[:, 5:]
            _dev_set(G, mem, cur)
        with plan_on(G):
            for P in (5, 6):
                k0, v0 = _kv(model)
                m0 = G.get_stat("mpt_plan_tokens")
                model.evaluate(np.array([7], np.int32))
                assert G.get_stat("mpt_plan_tokens") == m0 + 1
                k1, v1 = _kv(model)
                assert _only_row_changed(k0, k1, L, Cc, E, P) and _only_row_changed(v0, v1, L, Cc, E, P)
                assert not np.array_equal(k0.reshape(L, Cc, E)[:, P], k1.reshape(L, Cc, E)[:, P])
    finally:
        G.set_option("plan_mpt", 0)
        model.free()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rows_behind_the_token_never_reach_the_result(G, shape):
    hp, w = mpt.make_mpt(SHAPES[shape], 2, seed=5)
    L, Cc, E = hp["n_layer"], hp["n_ctx"], hp["n_embd"]
    outs = []
    try:
        with plan_on(G):
            for fill in (0x0000, 0x7b53, 0x7e01, 0xfe00):  # 0, 6e4, two NaN patterns
                model = _prompted(hp, w)
                for mem in (model.memory_k, model.memory_v):
                    cur = mem.device_get(np.float16).view(np.uint16).reshape(L, Cc, E).copy()
                    cur[:, 6:] = fill  # the step writes row 5 and reads rows 0 .. 5
                    _dev_set(G, mem, cur)
                m0 = G.get_stat("mpt_plan_tokens")
                outs.append(model.evaluate(np.array([9], np.int32)))
                assert G.get_stat("mpt_plan_tokens") == m0 + 1
                model.free()
    finally:
        G.set_option("plan_mpt", 0)
    assert np.isfinite(outs[0]).all()
    for o in outs[1:]:
        assert np.array_equal(_bits(o), _bits(outs[0]))


def test_capture_replay_and_second_model_give_the_same_bits(G):
    hp, w = mpt.make_mpt(MPT_12H, 7, seed=5)
    runs = []
    try:
        with plan_on(G):
            for rep in range(2):
                model = _prompted(hp, w)
                state = _kv(model)
                n0 = model.n_past
                p0 = G.get_stat("plans")
                a = model.evaluate(np.array([11], np.int32))  # this model's first plan step: its plan is built now, its graph captured now
                assert G.get_stat("plans") == p0 + 1
                _dev_set(G, model.memory_k, state[0])
                _dev_set(G, model.memory_v, state[1])
                model.n_past = n0
                r0 = G.get_stat("graph_replays")
                b = model.evaluate(np.array([11], np.int32))  # the same token at the same state: a replay
                assert G.get_stat("graph_replays") == r0 + 1 and G.get_stat("plans") == p0 + 1  # of the plan that exists: nothing was built
                assert np.array_equal(_bits(a), _bits(b))
                runs.append((a, _kv(model)))
                model.free()
    finally:
        G.set_option("plan_mpt", 0)
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0]))
    assert np.array_equal(runs[0][1][0], runs[1][1][0]) and np.array_equal(runs[0][1][1], runs[1][1][1])


def _stepped(model, n):
    ids = []
    for _ in range(n):
        ids.append(int(np.argmax(model.last_logits)))
        model.evaluate(np.array([ids[-1]], np.int32))
    return np.array(ids, np.int32), model.last_logits


@pytest.mark.parametrize("on", [1, 0])
def test_infer_tokens_device_equals_the_stepped_loop(G, on):
    """option 1: the chain on the plan against stepped plan evaluations with the argmax on the host; option 0: the entry declines and
    infer_tokens_device is the stepped executor loop itself"""
    hp, w = mpt.make_mpt(mpt.MPT_TINY, 2, seed=5)
    n = 7
    res = []
    try:
        G.set_option("plan_mpt", on)
        for chained in (True, False):
            model = _prompted(hp, w)
            m0, g0 = G.get_stat("mpt_plan_tokens"), G.get_stat("generic_graphs")
            ids, lg = model.infer_tokens_device(n) if chained else _stepped(model, n)
            assert G.get_stat("mpt_plan_tokens") - m0 == (n if on else 0)
            assert G.get_stat("generic_graphs") - g0 == (0 if on else n)
            assert model.n_past == 5 + n
            res.append((ids, lg.copy(), _kv(model)))
            model.free()
    finally:
        G.set_option("plan_mpt", 0)
    (ia, la, kva), (ib, lb, kvb) = res
    assert np.array_equal(ia, ib), (ia, ib)
    assert np.array_equal(_bits(la), _bits(lb))
    assert np.array_equal(kva[0], kvb[0]) and np.array_equal(kva[1], kvb[1])


# ---- 5. positions that can go wrong ----
def test_first_token_without_a_prompt_and_the_last_slot(G, O):
    hp, w = mpt.make_mpt(mpt.MPT_TINY, 2, seed=5)
    L, Cc, E = hp["n_layer"], hp["n_ctx"], hp["n_embd"]
    model, ref = mpt.Mpt(hp, w), alibi_ref.Mpt(hp, w)

    def checked_step(P):
        k0, v0 = _kv(model)
        m0 = G.get_stat("mpt_plan_tokens")
        d = _step_vs_ref(O, model, ref, 17)
        assert G.get_stat("mpt_plan_tokens") == m0 + 1 and model.n_past == P + 1
        k1, v1 = _kv(model)
        assert _only_row_changed(k0, k1, L, Cc, E, P) and _only_row_changed(v0, v1, L, Cc, E, P)
        assert d <= EDGE, (P, d)

    try:
        with plan_on(G):
            checked_step(0)  # T = 1: no prompt, nothing in the cache
            for mem in (model.memory_k, model.memory_v):  # a cache as C - 2 tokens might have left it
                _dev_set(G, mem, (0.5 * np.random.default_rng(4).standard_normal(L * Cc * E)).astype(np.float16))
            model.n_past = Cc - 2
            ctx0 = model._ctx0(1, kq_copies=4)
            try:
                _, gf = model._evaluate_in(ctx0, [5])  # position C - 2, on the plan; one slot is left
                out, lg = np.zeros(2, np.int32), np.zeros(hp["n_vocab"], np.float32)
                m0 = G.get_stat("mpt_plan_tokens")
                k0, v0 = _kv(model)
                # two tokens more do not fit: refused with nothing executed, as the LLaMA plans' chain refuses it
                assert G.lib().ggml_hip_decode_greedy_chain(C.cast(gf.ptr, C.c_void_p), 2, out.ctypes.data, lg.ctypes.data) == -1
                assert G.get_stat("mpt_plan_tokens") == m0
                k1, v1 = _kv(model)
                assert np.array_equal(k0, k1) and np.array_equal(v0, v1)
            finally:
                ctx0.free()
            checked_step(Cc - 1)  # the last slot
            # the step behind it: its graph is built (views only: nothing is touched) and handed to the matcher alone — it declines, so
            # the plan never runs a token behind the context's end; the same graph one position earlier is taken
            hook = G.lib().ggml_hip_debug_mpt
            for P, want in ((Cc, 0), (Cc - 1, 1)):
                ctx0 = model._ctx0(1, kq_copies=4)
                try:
                    model.n_past = P
                    gf = _VariantMpt.build(model, ctx0, [5])[1]
                    m0, g0 = G.get_stat("mpt_plan_tokens"), G.get_stat("generic_graphs")
                    assert hook(3, 0, C.cast(gf.ptr, C.c_void_p), None, 0.0, 0, None, None, 0, 0, 0, 0, 0.0, None) == want, P
                    assert (G.get_stat("mpt_plan_tokens"), G.get_stat("generic_graphs")) == (m0, g0)
                finally:
                    ctx0.free()
            model.n_past = Cc
    finally:
        G.set_option("plan_mpt", 0)
        model.free()


def test_across_the_attention_workgroups_stride(G, O):
    """T = 1023 .. 1026: k_attn_decode_alibi's soft_max takes positions 1024 threads at a time"""
    hp, w = mpt.make_mpt(dict(mpt.MPT_TINY, n_ctx=1100), 2, seed=5)
    L, Cc, E = hp["n_layer"], hp["n_ctx"], hp["n_embd"]
    model, ref = mpt.Mpt(hp, w), alibi_ref.Mpt(hp, w)
    try:
        rng = np.random.default_rng(3)
        for mem in (model.memory_k, model.memory_v):  # a cache as 1022 tokens might have left it
            _dev_set(G, mem, (0.5 * rng.standard_normal(L * Cc * E)).astype(np.float16))
        model.n_past = 1022
        with plan_on(G):
            for P in (1022, 1023, 1024, 1025):
                k0, v0 = _kv(model)
                m0 = G.get_stat("mpt_plan_tokens")
                d = _step_vs_ref(O, model, ref, 21)
                assert G.get_stat("mpt_plan_tokens") == m0 + 1
                k1, v1 = _kv(model)
                assert _only_row_changed(k0, k1, L, Cc, E, P) and _only_row_changed(v0, v1, L, Cc, E, P)
                assert d <= EDGE, (P, d)
    finally:
        G.set_option("plan_mpt", 0)
        model.free()


# ---- 6. op level, through the debug hook ----
def _hook_stage(G, x, w, f16d):
    K = x.size
    lo, hi = np.zeros(K // 2 + GUARD, np.int8), np.zeros(K // 2 + GUARD, np.int8)
    d, s = np.zeros(K // 32 + GUARD // 4, np.float32), np.zeros(K // 32 + GUARD // 4, np.int32)
    outs = (C.c_void_p * 4)(lo.ctypes.data, hi.ctypes.data, d.ctypes.data, s.ctypes.data)
    assert G.lib().ggml_hip_debug_mpt(0, f16d, x.ctypes.data, w.ctypes.data, 1e-5, K, None, None, 0, 0, 0, 0, 0.0, outs) == 0
    for a, n in ((lo, K // 2), (hi, K // 2), (d.view(np.int8), K // 8), (s.view(np.int8), K // 8)):
        assert (a[n:n + GUARD].view(np.uint8) == 0xFF).all()  # the guards came back whole
    return lo[:K // 2], hi[:K // 2], d[:K // 32], s[:K // 32]


def _executor_stage(G, x, w, f16d):
    """the executor's chain on the same row: k_norm -> mul (a two-node graph, nothing offloaded) -> k_quantize_act"""
    K = x.size
    ctx = G.Context(1024 * 1024 + 16 * K * 4)  # (the graph object alone is 164 KB)
    try:
        y = ctx.op_mul(ctx.op_norm(ctx.tensor_from(x)), ctx.tensor_from(w))
        gf = ctx.graph()
        gf.build_forward_expand(y)
        gf.compute()
        yv = y.read_data().copy()
    finally:
        ctx.free()
    lo, hi = np.zeros(K // 2 + GUARD, np.int8), np.zeros(K // 2 + GUARD, np.int8)
    d, s = np.zeros(K // 32 + GUARD // 4, np.float32), np.zeros(K // 32 + GUARD // 4, np.int32)
    outs = (C.c_void_p * 7)(lo.ctypes.data, hi.ctypes.data, d.ctypes.data, s.ctypes.data, None, None, None)
    assert G.lib().ggml_hip_debug_act_quant(0, f16d, 1, K, K, yv.ctypes.data, None, None, None, 0.0, 0, 0, outs) == 0
    return (lo[:K // 2], hi[:K // 2], d[:K // 32], s[:K // 32]), yv


def _tie_row(K):
    """A row whose LayerNorm is exact — mean 0, variance 4096 (+ 1e-5 rounds away), scale 1/64 — with half-integer multiples of the block
    maximum / 127 in block 0: rounding ties at +-0.5 of a quant step."""
    ties = [127.0, 63.5, 0.5, 1.5, 2.5]
    need = K // 2 * 4096 - int(sum(t * t for t in ties))  # what the fillers' squares must add up to, per sign
    n_fill = K // 2 - len(ties)
    rest = need - (n_fill - 3) * 4096
    abc = next((a, b, c) for a in range(1, 127) for b in range(a, 127) for c in [int(round((rest - a * a - b * b) ** 0.5)) if rest - a * a - b * b > 0 else 0]
               if 1 <= c <= 126 and a * a + b * b + c * c == rest)
    half = ties + [float(v) for v in abc] + [64.0] * (n_fill - 3)
    row = np.empty(K, np.float32)
    row[0::2] = half
    row[1::2] = [-v for v in half]
    return row


@pytest.mark.parametrize("f16d", [1, 0])
@pytest.mark.parametrize("K", [128, 4096])
def test_layernorm_staging_equals_the_executors_chain(G, K, f16d):
    rng = np.random.default_rng(K)
    gain = (1.0 + 0.01 * rng.standard_normal(K)).astype(np.float32)
    rows = {"random": rng.standard_normal(K).astype(np.float32), "tie": _tie_row(K), "equal": np.full(K, 0.37, np.float32),
            "outlier": rng.standard_normal(K).astype(np.float32)}
    rows["outlier"][K // 3] = 1e4
    for name, x in rows.items():
        wv = np.ones(K, np.float32) if name == "tie" else gain
        want, y = _executor_stage(G, x, wv, f16d)
        got = _hook_stage(G, x, wv, f16d)
        if name == "tie":  # the construction holds: exact ties reach the quantizer
            r = y[:32].astype(np.float64) * (127.0 / np.abs(y[:32]).max())
            assert np.sum(np.abs(np.abs(r - np.trunc(r)) - 0.5) == 0) >= 8, r
        if name == "equal":
            assert not want[0].any() and not want[1].any()
        for a, b, what in zip(got, want, ("lo", "hi", "d", "sum")):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, what)


def _f16(a):
    return np.asarray(a).astype(np.float16)


def _attn_ref(q, mk, mv, slopes, H, D, T, scale):
    """f64 with ggml's rounding points: q, K, P as f16; the score, its scaling, the bias product and sum, 1 / sum and P in f32"""
    E = H * D
    K = mk[:T].astype(np.float64).reshape(T, H, D)
    V = mv[:T].astype(np.float64).reshape(T, H, D)
    qh = _f16(q).astype(np.float64).reshape(H, D)
    s = np.einsum("thd,hd->ht", K, qh).astype(np.float32)
    x = (np.arange(T, dtype=np.float32)[None, :] * slopes[:, None].astype(np.float32)).astype(np.float32) + (s * np.float32(scale)).astype(np.float32)
    x = x.astype(np.float32)
    mx = x.max(axis=1, keepdims=True)
    e = _f16(np.exp(_f16(x - mx).astype(np.float64))).astype(np.float64)
    inv = (1.0 / e.sum(axis=1, keepdims=True)).astype(np.float32)
    p = _f16((e.astype(np.float32) * inv).astype(np.float32)).astype(np.float64)
    return np.einsum("thd,ht->hd", V, p).reshape(E)


def _attn_hook(G, q, mk, mv, slopes, H, D, T, Cc, scale):
    E = H * D
    out = np.zeros(E + GUARD // 4, np.float32)
    outs = (C.c_void_p * 1)(out.ctypes.data)
    rc = G.lib().ggml_hip_debug_mpt(1, 0, q.ctypes.data, slopes.ctypes.data, 0.0, 0, mk.view(np.uint16).ctypes.data, mv.view(np.uint16).ctypes.data, H, D,
                                    T - 1, Cc, scale, outs)
    assert rc == 0
    assert (out[E:].view(np.uint32) == 0xFFFFFFFF).all()
    return out[:E].astype(np.float64)


def _attn_executor(G, q, mk, mv, slopes_bias, H, D, T, Cc, scale):
    """mpt.py's attention nodes on host tensors, node by node on the executor (nothing offloaded: the four-launch chain)"""
    E = H * D
    ctx = G.Context(8 * 1024 * 1024 + 8 * Cc * E + 64 * T * H)
    try:
        tk, tv = ctx.tensor_from(mk.reshape(-1)), ctx.tensor_from(mv.reshape(-1))
        tq = ctx.op_permute(ctx.tensor_from(q.reshape(1, H, D)), 0, 2, 1, 3)
        kk = ctx.op_permute(ctx.op_reshape_3d(ctx.op_view_1d(tk, T * E, 0), D, H, T), 0, 2, 1, 3)
        kq = ctx.op_mul_mat(kk, tq)
        kq = ctx.op_scale(kq, ctx.new_f32(np.float32(scale)))
        kq = ctx.op_alibi(kq, T - 1, H, slopes_bias)
        kq = ctx.op_soft_max(ctx.op_diag_mask_inf(kq, T - 1))
        vt = ctx.op_cpy(ctx.op_permute(ctx.op_reshape_3d(ctx.op_view_1d(tv, T * E, 0), D, H, T), 1, 2, 0, 3), ctx.new_tensor(G.TYPE_F16, T, D, H))
        out = ctx.op_cpy(ctx.op_permute(ctx.op_mul_mat(vt, kq), 0, 2, 1, 3), ctx.new_tensor(G.TYPE_F32, E, 1))
        gf = ctx.graph()
        gf.build_forward_expand(out)
        gf.compute()
        return out.device_get().astype(np.float64)  # (a cpy's result is not mirrored to the host: its device image)
    finally:
        ctx.free()


def test_alibi_attention_within_twice_the_executors_error(G):
    """Measured on an MI355X (worst |Δ|max / std of the reference row over the 15 cases below): the executor's chain 5.85e-7 (D 128, H 12,
    T 64), k_attn_decode_alibi 6.86e-7 (D 128, H 12, T 1025); T = 1 and the peaked row are exact on both; the case at the LDS cap (T 25573) 3.1e-7 on both.  DESIGN.md section 4.3c."""
    cases = [(D, H, T, "random") for D, H in ((32, 4), (128, 12)) for T in (1, 2, 63, 64, 65, 1025)] + [(32, 4, 65, "peaked"), (32, 4, 65, "flat")] + \
            [(32, 2, 25573, "random")]  # C = 25576: 153 584 bytes of dynamic LDS, 16 short of the 150 KiB the opt-in asks for (+ 8.3 KiB static)
    err_exec, err_new = [], []
    for D, H, T, kind in cases:
        rng = np.random.default_rng(1000 * D + 10 * H + T)
        E, Cc = H * D, T + 3
        bias_max = 8.0
        slopes = alibi_ref.slopes(H, bias_max)
        scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
        q = rng.standard_normal(E).astype(np.float32)
        mk = _f16(0.5 * rng.standard_normal((Cc, E)))
        mv = _f16(rng.standard_normal((Cc, E)))
        if kind == "flat":  # every score 0 but for the bias
            mk[:] = 0
        if kind == "peaked":  # one score 30 above the rest (which are 0): K row 40 along q
            mk[:] = 0
            qq = _f16(q).astype(np.float64).reshape(H, D)
            mk[40] = _f16((30.0 / scale) * qq / (qq * qq).sum(axis=1, keepdims=True)).reshape(E)
        mk[T:], mv[T:] = np.float16(np.nan), np.float16(np.nan)  # rows behind the token: never read
        want = _attn_ref(q, mk, mv, slopes, H, D, T, scale)
        new = _attn_hook(G, q, mk, mv, slopes, H, D, T, Cc, scale)
        mk[T:], mv[T:] = 0, 0
        exe = _attn_executor(G, q, mk, mv, bias_max, H, D, T, Cc, scale)
        sd = float(want.std()) or 1.0
        err_exec.append(float(np.max(np.abs(exe - want))) / sd)
        err_new.append(float(np.max(np.abs(new - want))) / sd)
        assert np.isfinite(new).all(), (D, H, T, kind)
    print("executor worst %.3e, k_attn_decode_alibi worst %.3e" % (max(err_exec), max(err_new)), list(zip(cases, err_exec, err_new)))
    assert max(err_new) <= 2.0 * max(err_exec), (max(err_new), max(err_exec))


# ---- 7. declines: on the executor, bit-identical to option 0 ----
def _decline_case(G, make_model, steps):
    outs = []
    for on in (1, 0):
        G.set_option("plan_mpt", on)
        model = make_model()
        m0, g0 = G.get_stat("mpt_plan_tokens"), G.get_stat("generic_graphs")
        outs.append([model.evaluate(np.array(s, np.int32)) for s in steps])
        assert G.get_stat("mpt_plan_tokens") == m0, "ran on the plan"
        assert G.get_stat("generic_graphs") == g0 + len(steps)
        model.free()
    for a, b in zip(*outs):
        assert np.array_equal(_bits(a), _bits(b))


class _VariantMpt(mpt.Mpt):
    """mpt.Mpt's graph (llm_amd/mpt.py, node for node) in the forms mpt.py itself does not build: f32 K/V memory, and the stages of a layer
    split — `first`: get_rows and the layers, the residual rows as the result (no final norm, no lm_head); `last`: the layers on residual
    rows handed in (no get_rows), then the final norm and the lm_head.  `build` is the graph alone, not computed."""

    def __init__(self, hp, w, kv_type=None, stage=None):
        super().__init__(hp, w)
        self.stage = stage
        self.kv_type = G_TYPE_F16 if kv_type is None else kv_type  # (TYPE_F32 is 0)
        if self.kv_type != G_TYPE_F16:
            from llm_amd import ggml as G
            self.sctx.free()
            n_kv = hp["n_layer"] * self.C * hp["n_embd"]
            self.sctx = G.Context(2 * n_kv * 4 + (1 << 16))
            self.memory_k = self.sctx.new_tensor(self.kv_type, n_kv).set_name("memory_k").offload_no_scratch()
            self.memory_v = self.sctx.new_tensor(self.kv_type, n_kv).set_name("memory_v").offload_no_scratch()

    @staticmethod
    def build(self, ctx0, tokens, stage=None, es=2):
        from llm_amd import ggml as G
        hp, t = self.hp, self.t
        E, H, L = hp["n_embd"], hp["n_head"], hp["n_layer"]
        D, N, P, Cc = E // H, len(tokens), self.n_past, self.C
        T = P + N
        off = lambda x: x.offload()

        def ln(a, name):
            return off(ctx0.op_mul(off(ctx0.op_norm(a)), t[name]))

        if stage == "last":  # the residual rows another stage would hand over
            rows = np.random.default_rng(int(np.sum(tokens)) + 1).standard_normal((N, E)).astype(np.float32)
            x = ctx0.tensor_from(rows)
        else:
            x = off(ctx0.op_get_rows(t["transformer.wte.weight"], ctx0.tensor_from(np.asarray(tokens, np.int32))))
        gf = ctx0.graph()
        for il in range(L):
            p = f"transformer.blocks.{il}."
            cur = off(ctx0.op_mul_mat(t[p + "attn.Wqkv.weight"], ln(x, p + "norm_1.weight")))
            qc, kc, vc = (ctx0.op_view_2d(cur, E, N, cur.nb[1], 4 * E * j) for j in range(3))
            gf.build_forward_expand(off(ctx0.op_cpy(kc, ctx0.op_view_1d(self.memory_k, N * E, es * E * (il * Cc + P)))))
            gf.build_forward_expand(off(ctx0.op_cpy(vc, ctx0.op_view_1d(self.memory_v, N * E, es * E * (il * Cc + P)))))
            q = ctx0.op_permute(off(ctx0.op_cpy(qc, ctx0.new_tensor(G.TYPE_F32, D, H, N))), 0, 2, 1, 3)
            kk = ctx0.op_permute(ctx0.op_reshape_3d(ctx0.op_view_1d(self.memory_k, T * E, il * Cc * es * E), D, H, T), 0, 2, 1, 3)
            kq = off(ctx0.op_mul_mat(kk, q))
            kq = off(ctx0.op_scale(kq, ctx0.new_f32(np.float32(1.0) / np.sqrt(np.float32(E) / np.float32(H)))))
            kq = off(ctx0.op_soft_max(off(ctx0.op_diag_mask_inf(off(ctx0.op_alibi(kq, P, H, hp["alibi_bias_max"])), P))))
            vt = off(ctx0.op_cpy(ctx0.op_permute(ctx0.op_reshape_3d(ctx0.op_view_1d(self.memory_v, T * E, il * Cc * es * E), D, H, T), 1, 2, 0, 3),
                                 ctx0.new_tensor(G.TYPE_F16, T, D, H)))
            cur = off(ctx0.op_cpy(ctx0.op_permute(off(ctx0.op_mul_mat(vt, kq)), 0, 2, 1, 3), ctx0.new_tensor(G.TYPE_F32, E, N)))
            x = off(ctx0.op_add(x, off(ctx0.op_mul_mat(t[p + "attn.out_proj.weight"], cur))))
            cur = off(ctx0.op_gelu(off(ctx0.op_mul_mat(t[p + "ffn.up_proj.weight"], ln(x, p + "norm_2.weight")))))
            cur = off(ctx0.op_mul_mat(t[p + "ffn.down_proj.weight"], cur))
            x = ctx0.op_add(x, cur) if stage == "first" and il == L - 1 else off(ctx0.op_add(x, cur))  # (a first stage's result: mirrored)
        if stage == "first":
            out = x
        else:
            out = ctx0.op_mul_mat(t["transformer.wte.weight"], ln(x, "transformer.norm_f.weight"))
        gf.build_forward_expand(out)
        return out, gf

    def _evaluate_in(self, ctx0, tokens):
        out, gf = _VariantMpt.build(self, ctx0, tokens, self.stage, 2 if self.kv_type == G_TYPE_F16 else 4)
        gf.compute()
        self.n_past += len(tokens)
        res = out.read_data().reshape(len(tokens), -1).copy()
        self.last_logits = res[-1]
        return res, gf


G_TYPE_F16 = 1  # llm_amd.ggml.TYPE_F16 (GGML_TYPE_F16)


def test_the_variant_builder_is_mpt_pys_graph(G):
    """what makes the two decline cases below mean something: with f16 K/V and no stage it builds the graph the plan takes"""
    assert G.TYPE_F16 == G_TYPE_F16
    hp, w = mpt.make_mpt(mpt.MPT_TINY, 2, seed=5)
    outs = []
    try:
        with plan_on(G):
            for cls in (mpt.Mpt, _VariantMpt):
                model = cls(hp, w)
                model.evaluate(np.array([3, 1, 4, 1, 5], np.int32))
                m0 = G.get_stat("mpt_plan_tokens")
                outs.append(model.evaluate(np.array([7], np.int32)))
                assert G.get_stat("mpt_plan_tokens") == m0 + 1
                model.free()
    finally:
        G.set_option("plan_mpt", 0)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


@pytest.mark.parametrize("case", ["n2", "no_offload", "q4_k", "f16", "d16", "kv_f32", "stage_first", "stage_last"])
def test_declined_forms_run_on_the_executor(G, case):
    prompt = [3, 1, 4, 1, 5]
    try:
        if case == "n2":
            hp, w = mpt.make_mpt(mpt.MPT_TINY, 2, seed=5)
            _decline_case(G, lambda: mpt.Mpt(hp, w), [prompt, [7, 8], [9, 2]])
        elif case == "no_offload":
            hp, w = mpt.make_mpt(mpt.MPT_TINY, 2, seed=5)
            _decline_case(G, lambda: mpt.Mpt(hp, w, offload=False), [prompt, [7], [9]])
        elif case == "q4_k":
            hp, w = mpt.make_mpt(dict(mpt.MPT_TINY, n_embd=256, n_head=8), 12, seed=5)
            _decline_case(G, lambda: mpt.Mpt(hp, w), [prompt, [7], [9]])
        elif case == "f16":
            hp, w = mpt.make_mpt(mpt.MPT_TINY, 1, seed=5)
            _decline_case(G, lambda: mpt.Mpt(hp, w), [prompt, [7], [9]])
        elif case == "d16":
            hp, w = mpt.make_mpt(mpt.MPT_TINY_12H, 2, seed=5)
            _decline_case(G, lambda: mpt.Mpt(hp, w), [prompt, [7], [9]])
        elif case == "kv_f32":
            hp, w = mpt.make_mpt(mpt.MPT_TINY, 2, seed=5)
            _decline_case(G, lambda: _VariantMpt(hp, w, kv_type=G.TYPE_F32), [prompt, [7], [9]])
        else:  # a stage of a layer split, single tokens: no lm_head behind the layers / no get_rows in front of them
            hp, w = mpt.make_mpt(mpt.MPT_TINY, 2, seed=5)
            _decline_case(G, lambda: _VariantMpt(hp, w, stage=case[6:]), [prompt, [7], [9]])
    finally:
        G.set_option("plan_mpt", 0)
