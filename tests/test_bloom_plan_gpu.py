"""The BLOOM decode plan (backend option plan_bloom; csrc/plan_match.inc match_bloom_decode, plan_decode.inc plan_launch_bloom,
kernels/bloom_plan.h): single-token steps of llm_amd.bloom's offloaded graph as one embedding launch, five launches per layer and one lm_head
launch, replayed from a captured graph, and Bloom.infer_tokens_device's greedy chain on it.  Every test that sets plan_bloom restores 0.

Against the reference: tests/test_mpt_plan_gpu.py's form and bounds (tests/test_alibi_families_gpu.py's) — tests/alibi_ref.py Bloom in O.ref_mode()
with the device's K/V copied in before every step, |Δ|max / std per step; EDGE = 8e-2 on every step, at tiny width at least half of the steps within
STRICT = 1e-5, at real width EDGE only.  The quota is the reference's own to keep first: its scalar branch against its AVX2 branch on the same cases
(weights seed, token seed; a 5-token prompt, then the 6 single steps, K/V copied across), run on the CPU for types 2, 3, 6, 7, 8.  Tiny: (5, 6) keeps
6, 6, 6, 6, 5 of 6 steps within STRICT, (13, 14) 6, 6, 4, 6, 6, (19, 20) 6, 6, 6, 5, 6 with the smallest worst step (4.5e-5): (19, 20).  The 12-head
variant (n_embd 384, head size 32: BLOOM_TINY_12H's head size 16 must decline): (5, 6) keeps 5, 5, 6, 5, 2, (13, 14) 2, 6, 6, 4, 5, (17, 18)
6, 5, 3, 4, 5, (23, 24) 4, 4, 2, 3, 3, (21, 22) 5, 5, 5, 4, 5 and (25, 26) 6, 5, 5, 6, 6: (25, 26), a step and more above the quota of 3 for every type.
Measured on an MI355X with these seeds: all ten cases keep 6 of 6 steps within STRICT (worst 1.3e-6); real width worst 3.1e-2.

Op level (ggml_hip_debug_bloom), bit for bit: the biased staging against the executor's norm -> mul -> add -> quantize chain; the launches against
tests/mul_mat_exact_ref.py's exact dots — a LayerNorm with gain 0 and bias X stages exactly the integer row X — then f32 + bias and + res / GELU /
f16 in the graph's order; the embedding launch against the executor's get_rows -> norm -> mul -> add."""
import ctypes as C

import numpy as np
import pytest

import alibi_ref
import mul_mat_exact_ref as X
from llm_amd import bloom

pytestmark = pytest.mark.gpu

STRICT, EDGE, GUARD = 1e-5, 8e-2, 256
BLOOM_12H = dict(bloom.BLOOM_TINY, n_embd=384, n_head=12)  # head size 32; heads 8..11 take ggml's second slope sequence
BLOOM_REAL = dict(bloom.BLOOM_7B1, n_layer=2, n_vocab=512, n_ctx=64)
SHAPES = {"tiny": (bloom.BLOOM_TINY, 19, 20), "12h": (BLOOM_12H, 25, 26)}  # shape, weights seed, tokens seed: see the module docstring
PROMPT = np.array([3, 1, 4, 1, 5], np.int32)
STATS = ("bloom_plan_tokens", "graph_replays", "generic_graphs")


def _stats(G):
    return np.array([G.get_stat(s) for s in STATS])


def _kv(model):
    return model.memory_k.device_get(np.float16).view(np.uint16).copy(), model.memory_v.device_get(np.float16).view(np.uint16).copy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _steps_vs_ref(G, O, hp, w, toks, n_prompt):
    """the prompt on the executor, then every further token as a single step under plan_bloom against the restatement at the device's K/V"""
    model, ref, d = bloom.Bloom(hp, w), alibi_ref.Bloom(hp, w), []
    try:
        G.set_option("plan_bloom", 1)
        model.evaluate(toks[:n_prompt])
        s0 = _stats(G)
        for tok in toks[n_prompt:]:
            got = model.evaluate(np.array([tok], np.int32))
            ref.memory_k[:] = model.memory_k.device_get(np.float16).reshape(ref.memory_k.shape)
            ref.memory_v[:] = model.memory_v.device_get(np.float16).reshape(ref.memory_v.shape)
            ref.n_past = model.n_past - 1
            want = ref.evaluate(np.array([tok], np.int32), mode=O.ref_mode())
            d.append(float(np.max(np.abs(got - want))) / float(want.std()))
        assert (_stats(G) - s0)[0] == len(toks) - n_prompt
    finally:
        G.set_option("plan_bloom", 0)
        model.free()
    print(f"worst {max(d):.2e}, {sum(x <= STRICT for x in d)}/{len(d)} within {STRICT}", d)
    return d


def test_single_token_steps_run_on_the_plan(G):
    hp, w = bloom.make_bloom(bloom.BLOOM_TINY, 2, seed=19)
    model = bloom.Bloom(hp, w)
    try:
        model.evaluate(PROMPT)
        for on, want in ((1, (3, 3, 0)), (0, (0, 0, 3))):
            G.set_option("plan_bloom", on)
            s0 = _stats(G)
            for tok in (1, 5, 9):
                model.evaluate(np.array([tok], np.int32))
            assert tuple(_stats(G) - s0) == want, on
        assert model.n_past == 11
    finally:
        G.set_option("plan_bloom", 0)
        model.free()


@pytest.mark.parametrize("wtype", [2, 3, 6, 7, 8])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_plan_steps_match_restatement(G, O, shape, wtype):
    hp0, ws, ts = SHAPES[shape]
    hp, w = bloom.make_bloom(hp0, wtype, seed=ws)
    d = _steps_vs_ref(G, O, hp, w, np.random.default_rng(ts).integers(0, hp["n_vocab"], 11).astype(np.int32), 5)
    assert max(d) <= EDGE, d
    assert sum(x <= STRICT for x in d) >= len(d) // 2, d


def test_plan_steps_match_restatement_real_width(G, O):
    hp, w = bloom.make_bloom(BLOOM_REAL, G.TYPE_Q4_0, seed=7)
    d = _steps_vs_ref(G, O, hp, w, np.random.default_rng(8).integers(0, hp["n_vocab"], 12).astype(np.int32), 8)
    assert max(d) <= EDGE, d  # no STRICT quota at this width: tests/test_alibi_families_gpu.py


# ---- op level, through the debug hook ----
def _buf(n, dtype=np.float32):
    return np.full(n * np.dtype(dtype).itemsize + GUARD, 0xFF, np.uint8)


def _whole(b, n, dtype=np.float32):
    assert (b[n * np.dtype(dtype).itemsize:] == 0xFF).all(), "a store past the end"
    return b[:n * np.dtype(dtype).itemsize].view(dtype)


def _graph_row(G, build, nbytes=0):
    """a small graph on the executor, nothing offloaded: build(ctx) -> the node whose row comes back"""
    ctx = G.Context(4 * 1024 * 1024 + nbytes)
    try:
        y = build(ctx)
        gf = ctx.graph()
        gf.build_forward_expand(y)
        gf.compute()
        return y.read_data().reshape(-1).copy()
    finally:
        ctx.free()


def _quantized(G, y, f16d):
    K = y.size
    bufs = [_buf(K // 2, np.int8), _buf(K // 2, np.int8), _buf(K // 32), _buf(K // 32, np.int32)]
    outs = (C.c_void_p * 7)(*[b.ctypes.data for b in bufs], None, None, None)
    assert G.lib().ggml_hip_debug_act_quant(0, f16d, 1, K, K, y.ctypes.data, None, None, None, 0.0, 0, 0, outs) == 0
    return [b[:n] for b, n in zip(bufs, (K // 2, K // 2, K // 8, K // 8))]


@pytest.mark.parametrize("K", [128, 4096])
def test_biased_layernorm_staging_equals_the_executors_chain(G, K):
    rng = np.random.default_rng(K)
    x, gain, nb = rng.standard_normal(K).astype(np.float32), rng.uniform(0.5, 2.0, K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    chain = lambda f: _graph_row(G, lambda c: f(c, c.op_norm(c.tensor_from(x)), c.tensor_from(gain), c.tensor_from(nb)), 16 * K * 4)
    y = chain(lambda c, n, g, b: c.op_add(c.op_mul(n, g), b))
    no_bias, bias_first = chain(lambda c, n, g, b: c.op_mul(n, g)), chain(lambda c, n, g, b: c.op_mul(c.op_add(n, b), g))
    for f16d in (1, 0):
        bufs = [_buf(K // 2, np.int8), _buf(K // 2, np.int8), _buf(K // 32), _buf(K // 32, np.int32)]
        outs = (C.c_void_p * 4)(*[b.ctypes.data for b in bufs])
        assert G.lib().ggml_hip_debug_bloom(0, f16d, None, x.ctypes.data, gain.ctypes.data, nb.ctypes.data, 1e-5, K, None, None, 0, 0, 0, None, None, outs) == 0
        got = [_whole(b, n, np.int8).view(np.uint8) for b, n in zip(bufs, (K // 2, K // 2, K // 8, K // 8))]
        for a, b, what in zip(got, _quantized(G, y, f16d), ("lo", "hi", "d", "sum")):
            assert np.array_equal(a, b), (f16d, what)
        for wrong in (no_bias, bias_first):  # the bias is large enough to tell: either mutant chain quantizes to other blocks
            assert not np.array_equal(got[0], _quantized(G, wrong, f16d)[0])


def _launch(G, ctx, t, raw, Xrow, M, K, epi, bias=None, res=None, n_past=0, Cc=0, kv=None):
    """one launch of the hook on the integer row Xrow: behind the LayerNorm as gain 0 and bias Xrow (any x), or (epilogue 10) as the plain row"""
    w = ctx.tensor_from(raw, t, (K, M)).set_name("w").transfer_to_gpu()
    x = np.random.default_rng(1).standard_normal(K).astype(np.float32) if epi != 10 else Xrow
    gain, ob = np.zeros(K, np.float32), _buf(K if epi == 8 else M)
    ptr = lambda a: None if a is None else a.ctypes.data
    assert G.lib().ggml_hip_debug_bloom(1, epi, w.ptr, ptr(x), ptr(gain), ptr(Xrow), 1e-5, K, ptr(bias), ptr(res), 0, n_past, Cc,
                                        ptr(kv and kv[0]), ptr(kv and kv[1]), (C.c_void_p * 2)(ob.ctypes.data, None)) == 0
    return _whole(ob, K if epi == 8 else M)


@pytest.mark.parametrize("wtype", X.BLOCK_TYPES)
@pytest.mark.parametrize("epi", [8, 9, 10])
def test_biased_epilogues_equal_the_exact_dot_then_the_graphs_order(G, epi, wtype):
    K, M, Cc, P = 64, 192 if epi == 8 else 64, 4, 2
    raw, W, Xi = X.exact_case(wtype, M, K, 1, quantize=G.quantize)
    dot = X.exact_product(Xi, W, 32)[0]
    rng = np.random.default_rng([epi, wtype])
    res = rng.standard_normal(M).astype(np.float32)
    # (GELU: sums inside its range; the K/V rows: inside f16's, with more bits than f16 keeps)
    bias = (rng.uniform(-4, 4, M) - dot if epi == 9 else rng.uniform(-6e4, 6e4, M) - dot if epi == 8 else 1000 * rng.standard_normal(M)).astype(np.float32)
    biased = dot + bias  # f32: one rounding
    kv = [_buf(Cc * K, np.uint16), _buf(Cc * K, np.uint16)] if epi == 8 else None
    with G.Context(raw.nbytes + (1 << 20)) as ctx:
        got = _launch(G, ctx, wtype, raw, Xi[0].astype(np.float32), M, K, epi, bias, res, P, Cc, kv)
    if epi == 8:  # q as f32; the K and V rows rounded to f16 at position P, every other row of the caches as it was
        assert np.array_equal(_bits(got), _bits(biased[:K]))
        for b, rows in zip(kv, (biased[K:2 * K], biased[2 * K:])):
            mem = _whole(b, Cc * K, np.uint16).reshape(Cc, K)
            assert np.array_equal(mem[P], rows.astype(np.float16).view(np.uint16)) and (np.delete(mem, P, 0) == 0xFFFF).all()
    elif epi == 9:
        assert np.array_equal(_bits(got), _bits(_graph_row(G, lambda c: c.op_gelu(c.tensor_from(biased)))))
    else:
        assert np.any(_bits(biased + res) != _bits(dot + (bias + res)))  # the two orders differ on these inputs: the graph's is asked for
        assert np.array_equal(_bits(got), _bits(biased + res))


@pytest.mark.parametrize("wtype", X.BLOCK_TYPES)
def test_embedding_launch_equals_the_executors_chain(G, wtype):
    for K in (128, 4096):
        rng = np.random.default_rng([K, wtype])
        raw = G.quantize(wtype, (0.02 * rng.standard_normal((8, K))).astype(np.float32))
        gain, nb = rng.uniform(0.5, 2.0, K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
        with G.Context(raw.nbytes + (1 << 20)) as ctx:
            w = ctx.tensor_from(raw, wtype, (K, 8)).set_name("wte").transfer_to_gpu()
            ob = _buf(K)
            assert G.lib().ggml_hip_debug_bloom(2, 0, w.ptr, None, gain.ctypes.data, nb.ctypes.data, 1e-5, K, None, None, 5, 0, 0, None, None,
                                                (C.c_void_p * 1)(ob.ctypes.data)) == 0
            want = _graph_row(G, lambda c: c.op_add(c.op_mul(c.op_norm(c.op_get_rows(w, c.tensor_from(np.array([5], np.int32)))), c.tensor_from(gain)),
                                                    c.tensor_from(nb)), 16 * K * 4)
        assert np.array_equal(_bits(_whole(ob, K)), _bits(want))


def test_lm_head_of_the_full_vocabulary(G):
    """250 880 rows at K = 1024 (BLOOM-560M): 62 of the launch's 64 rounds on 256 CUs.  The rows repeat a tile of 3001 — every row is
    compared, the first and the last among them, against the tile's exact dots"""
    V, K, R = 250880, 1024, 3001
    raw, W, Xi = X.exact_case(X.Q4_0, R, K, 1, quantize=G.quantize)
    full = np.resize(raw.reshape(R, -1), (V, raw.size // R)).reshape(-1)
    with G.Context(full.nbytes + (1 << 20)) as ctx:
        got = _launch(G, ctx, X.Q4_0, full, Xi[0].astype(np.float32), V, K, 0)
    assert np.array_equal(_bits(got), _bits(np.resize(X.exact_product(Xi, W, 32)[0], V)))


# ---- the chain, the long context, the declines ----
def _greedy(G, hp, w, n, chained):
    model = bloom.Bloom(hp, w)
    try:
        model.evaluate(PROMPT)
        s0 = _stats(G)
        if chained:
            ids, lg = model.infer_tokens_device(n)
        else:
            ids = np.zeros(n, np.int32)
            for i in range(n):
                ids[i] = int(np.argmax(model.last_logits))
                model.evaluate(ids[i:i + 1])
            lg = model.last_logits
        assert model.n_past == len(PROMPT) + n
        return ids, _bits(lg).copy(), _kv(model), _stats(G) - s0
    finally:
        model.free()


@pytest.mark.parametrize("on", [1, 0])
def test_infer_tokens_device_equals_the_stepped_loop(G, on):
    hp, w = bloom.make_bloom(bloom.BLOOM_TINY, 2, seed=19)
    try:
        G.set_option("plan_bloom", on)
        (ia, la, kva, sa), (ib, lb, kvb, sb) = (_greedy(G, hp, w, 6, chained) for chained in (True, False))
    finally:
        G.set_option("plan_bloom", 0)
    for s in (sa, sb):
        assert (s[0], s[2]) == ((6, 0) if on else (0, 6))
    assert np.array_equal(ia, ib) and np.array_equal(la, lb) and np.array_equal(kva[0], kvb[0]) and np.array_equal(kva[1], kvb[1])


def test_steps_across_the_split_threshold_keep_their_bits(G):
    hp, w = bloom.make_bloom(bloom.BLOOM_TINY, 2, seed=19)
    runs, split0 = [], G.get_option("attn_split")
    try:
        G.set_option("plan_bloom", 1)
        for split in (8, 0):  # positions 5 .. 10: single-workgroup attention up to T = 7, the three split launches from T = 8 on
            G.set_option("attn_split", split)
            runs.append(_greedy(G, hp, w, 6, False))
            assert runs[-1][3][0] == 6
    finally:
        G.set_option("attn_split", split0)
        G.set_option("plan_bloom", 0)
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("case", ["n2", "no_offload", "q4_k", "f16", "d16", "kv_f32"])
def test_declined_forms_run_on_the_executor(G, case):
    shape = {"q4_k": dict(bloom.BLOOM_TINY, n_embd=256, n_head=8), "d16": bloom.BLOOM_TINY_12H}.get(case, bloom.BLOOM_TINY)
    hp, w = bloom.make_bloom(shape, {"q4_k": 12, "f16": 1}.get(case, 2), seed=19)
    kw = {"no_offload": dict(offload=False), "kv_f32": dict(kv_type=G.TYPE_F32)}.get(case, {})
    outs = []
    try:
        for on in (1, 0):
            G.set_option("plan_bloom", on)
            model = bloom.Bloom(hp, w, **kw)
            model.evaluate(PROMPT)
            s0 = _stats(G)
            outs.append([model.evaluate(np.array(s, np.int32)) for s in ([[7, 8], [9, 2]] if case == "n2" else [[7], [9]])])
            assert (_stats(G) - s0)[0] == 0 and (_stats(G) - s0)[2] == 2
            model.free()
    finally:
        G.set_option("plan_bloom", 0)
    for a, b in zip(*outs):
        assert np.array_equal(_bits(a), _bits(b))
