"""Block-format LLaMA models with a K-quant output matrix (LlamaMatch::out_k, option plan_out_k): what llama.cpp's quantizer writes
for every block-format file type since June 2023 — Q4_0 … Q8_0 layers and tok_embeddings, output.weight as Q6_K.  Such a model is a
block-format model everywhere except in its lm_head launch (plan_decode.inc plan_lm_head_k): k_mmvq_kbig for a single token,
k_k_norm_quant + k_mmvq_k for chunks and batched steps, the f16 copy of the K matrix for the prompt plan's GEMM.

Held to rules the project already pins: the layers' launches are the pure model's (K/V byte-identical to a twin whose output is the
base type), the lm_head is the node-by-node executor's K mat-vec on the embedding row the evaluation returned (bit for bit), the
logits meet the oracle composition at the K plan's bound, chains and batched steps equal their stepped loops."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q6_K, Q4_K = 14, 12
TINY_K = dict(n_vocab=256, n_embd=256, n_head=4, n_head_kv=4, n_layer=2, n_rot=64, n_ff=512, n_mult=32)
GQA_K = dict(n_vocab=512, n_embd=512, n_head=8, n_head_kv=2, n_layer=3, n_rot=64, n_ff=768, n_mult=32)
WIDE_K = dict(n_vocab=256, n_embd=1024, n_head=8, n_head_kv=4, n_layer=2, n_rot=128, n_ff=2048, n_mult=32)  # E / 32 = 32: chunks of 9 .. 31 tokens on k_mmq_cols
# (base type of the layers and tok_embeddings, type of output.weight): q4_0 q4_1 q5_0 q5_1 q8_0 under Q6_K, and one Q4_K output
CASES = [(2, Q6_K), (3, Q6_K), (6, Q6_K), (7, Q6_K), (8, Q6_K), (2, Q4_K)]
CTX = 96
BOUND = {"tiny": 4e-2, "gqa": 8e-2}  # tests/test_kquant_plan_gpu.py: one rounding-edge flip of a downstream activation quant

_built = {}


def _stat(G, key):
    return int(G.lib().ggml_hip_get_stat(key.encode()))


def _stats(G, keys):
    return [_stat(G, k) for k in keys]


def _moved(G, keys, s0):
    return [b - a for a, b in zip(s0, _stats(G, keys))]


def _pair(O, hp0, base, ktype, seed):
    """The mixed model as tests/test_kquant_plan_gpu.py's _model builds it (base type, wtypes = {output.weight: ktype}) and its
    twin from the same arrays with output.weight quantized in the base type: (hp, w, hp_twin, w_twin), read-only and shared."""
    from llm_amd import synth
    key = (tuple(sorted(hp0.items())), base, ktype, seed)
    if key not in _built:
        rng = np.random.default_rng([base, seed])
        w, wt = {}, {}
        for name, (ne0, ne1) in synth.tensor_shapes(hp0).items():
            if ne1 is None:
                w[name] = wt[name] = (1.0 + 0.01 * rng.standard_normal(ne0)).astype(np.float32)
                continue
            x = (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32)
            wt[name] = O.quantize(base, x)
            w[name] = O.quantize(ktype, x) if name == "output.weight" else wt[name]
        for a in list(w.values()) + list(wt.values()):
            a.setflags(write=False)
        hp, hpt = dict(hp0, wtype=base, wtypes={"output.weight": ktype}), dict(hp0, wtype=base)
        _built[key] = (hp, w, hpt, wt)
    return _built[key]


def _executor_mul_mat(G, wtype, W_raw, M, K, X):
    """mul_mat(w, x) as a one-node graph through the C ABI: the node-by-node executor's launches (tests/test_kquant_gpu.py)"""
    N = X.shape[0]
    X = np.ascontiguousarray(X, np.float32)
    with G.Context(W_raw.nbytes + X.nbytes + M * N * 4 + (1 << 20)) as ctx:
        w = ctx.tensor_from(W_raw, wtype, (K, M)).set_name("w")
        w.transfer_to_gpu()
        x = ctx.tensor_from(X, G.TYPE_F32, (K, N)).set_name("x")
        y = ctx.op_mul_mat(w, x)
        g0 = _stat(G, "generic_graphs")
        ctx.graph().build_forward_expand(y).compute()
        assert _stat(G, "generic_graphs") - g0 == 1
        return y.read_data().reshape(N, M).copy()


PLAN_KEYS = ("plan_tokens", "out_k_tokens", "generic_graphs", "kplan_tokens", "prompt_plan_tokens")


def _prompt_and_decode(G, model, toks, n_prompt=8, emb=True):
    """an 8-token feed_prompt, then single-token evaluations: (logits rows, embedding rows, K, V, counter movements)"""
    sess = model.start_session(n_batch=8)
    s0 = _stats(G, PLAN_KEYS)
    sess.feed_prompt(toks[:n_prompt])
    outs, embs = [], []
    for i in range(n_prompt, len(toks)):
        r = sess.evaluate(toks[i:i + 1], want_embeddings=emb)
        outs.append((r[0] if emb else r)[-1].copy())
        if emb:
            embs.append(r[1].copy())
    moved = _moved(G, PLAN_KEYS, s0)
    k, v = sess.get_kv()
    sess.free()
    return outs, embs, k, v, moved


# ---- 1, 2, 3: the plans take it; the layers are the pure model's; the lm_head is the executor's ----
@pytest.mark.parametrize("base,ktype", CASES)
@pytest.mark.parametrize("cfg", ["tiny", "gqa"])
def test_decode_runs_on_the_block_plans_with_the_executors_lm_head(G, O, cfg, base, ktype):
    from llm_amd import llama
    hp, w, hpt, wt = _pair(O, {"tiny": TINY_K, "gqa": GQA_K}[cfg], base, ktype, 77)
    V, E = hp["n_vocab"], hp["n_embd"]
    toks = np.random.default_rng([base, 5]).integers(0, V, 20).astype(np.int32)
    model = llama.Llama(hp, w, context_size=CTX)
    try:
        outs, embs, k, v, moved = _prompt_and_decode(G, model, toks)
        assert moved == [20, 20, 0, 0, 0], moved  # chunk plan + 12 single tokens, every lm_head the K launch; no executor, no K plan
        G.set_option("plan_out_k", 0)
        off = _prompt_and_decode(G, model, toks)
        assert off[4] == [0, 0, 13, 0, 0], off[4]  # declined as before the option existed: 13 graphs node by node
    finally:
        G.set_option("plan_out_k", 1)
        model.free()
    twin = llama.Llama(hpt, wt, context_size=CTX)
    _, _, kt, vt, moved_t = _prompt_and_decode(G, twin, toks)
    twin.free()
    assert moved_t == [20, 0, 0, 0, 0], moved_t
    assert np.array_equal(k, kt) and np.array_equal(v, vt)  # the layers' launches never read the output matrix
    # the logits row = the executor's mul_mat(output.weight, embeddings) on the embedding row the same evaluation returned
    for i, (lg, em) in enumerate(zip(outs, embs)):
        ref = _executor_mul_mat(G, ktype, w["output.weight"], V, E, em[None, :])[0]
        assert np.array_equal(lg, ref), (i, float(np.max(np.abs(lg - ref))))
    worst = max(float(np.max(np.abs(a - b))) / float(b.std()) for a, b in zip(outs, off[0]))
    print(f"{cfg} base {base} output {ktype}: plan vs the whole model node by node, worst |dlogit|/std = {worst:.2e}")  # (measured, not gated)


@pytest.mark.parametrize("cfg,base", [("tiny", 2), ("gqa", 7)])
def test_chunk_rows_and_both_lm_head_forms(G, O, cfg, base):
    """Every row of an 8-token chunk that asked for all logits against the executor's mat-mul on the chunk's embedding rows; the big
    form (k_mmvq_kbig stages the norm itself) against the helper form (option kbig = 0): logits, K/V and greedy ids bit for bit."""
    from llm_amd import llama
    hp, w, _, _ = _pair(O, {"tiny": TINY_K, "gqa": GQA_K}[cfg], base, Q6_K, 31)
    V, E = hp["n_vocab"], hp["n_embd"]
    toks = np.random.default_rng(12).integers(0, V, 30).astype(np.int32)
    model = llama.Llama(hp, w, context_size=CTX)
    res = {}
    try:
        sess = model.start_session(n_batch=8)
        sess.feed_prompt(toks[:5])
        s0 = _stats(G, PLAN_KEYS)
        lg = sess.evaluate(toks[5:13])
        assert _moved(G, PLAN_KEYS, s0) == [8, 8, 0, 0, 0]
        em = sess.read_node(-2).reshape(8, E).copy()
        sess.free()
        ref = _executor_mul_mat(G, Q6_K, w["output.weight"], V, E, em)
        assert np.array_equal(lg, ref), float(np.max(np.abs(lg - ref)))
        for kbig in (1, 0):
            G.set_option("kbig", kbig)
            outs, _, k, v, moved = _prompt_and_decode(G, model, toks, 11)
            s = model.start_session(n_batch=8)
            s.feed_prompt(toks[:9])
            ids = [s.infer_next_token() for _ in range(12)]
            s.free()
            res[kbig] = (outs, k, v, moved, ids)
    finally:
        G.set_option("kbig", 1)
        model.free()
    assert res[1][3] == [30, 30, 0, 0, 0] and res[0][3] == [30, 30, 0, 0, 0]
    for a, b in zip(res[1][0], res[0][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(res[1][1], res[0][1]) and np.array_equal(res[1][2], res[0][2])
    assert res[1][4] == res[0][4]


def test_a_chunk_of_twelve_tokens_and_a_prompt_batch(G, O):
    """Check 1 for the other two plans: a 12-token chunk (E = 1024: every layer mat-vec on k_mmq_cols in two passes, the lm_head on
    k_mmvq_k) and a 64-token prompt batch (prompt_plan_tokens advances), each against the twin's K/V; plan_out_k = 0 declines both."""
    from llm_amd import llama
    for hp0, n, n_batch in ((WIDE_K, 12, 32), (TINY_K, 64, 64)):
        hp, w, hpt, wt = _pair(O, hp0, 2, Q6_K, 9)
        toks = np.random.default_rng(n).integers(0, hp["n_vocab"], n).astype(np.int32)
        kv, want = {}, [0, n, 0, 0, n] if n == 64 else [n, n, 0, 0, 0]
        for name, (h, ww) in {"mixed": (hp, w), "twin": (hpt, wt)}.items():
            model = llama.Llama(h, ww, context_size=CTX)
            try:
                for on in ((1, 0) if name == "mixed" else (1,)):
                    G.set_option("plan_out_k", on)
                    sess = model.start_session(n_batch=n_batch)
                    s0 = _stats(G, PLAN_KEYS)
                    lg = sess.evaluate(toks)
                    moved = _moved(G, PLAN_KEYS, s0)
                    if name == "twin":
                        assert moved == [want[0], 0, 0, 0, want[4]], (n, moved)
                    else:
                        assert moved == (want if on else [0, 0, 1, 0, 0]), (n, on, moved)
                    if on:
                        kv[name] = sess.get_kv()
                        if name == "mixed" and n == 12:  # the chunk's rows are the executor's mat-mul on its embedding rows
                            em = sess.read_node(-2).reshape(n, h["n_embd"]).copy()
                            ref = _executor_mul_mat(G, Q6_K, w["output.weight"], h["n_vocab"], h["n_embd"], em)
                            assert np.array_equal(lg, ref), float(np.max(np.abs(lg - ref)))
                    sess.free()
            finally:
                G.set_option("plan_out_k", 1)
                model.free()
        assert np.array_equal(kv["mixed"][0], kv["twin"][0]) and np.array_equal(kv["mixed"][1], kv["twin"][1]), n


# ---- 4: against the oracle ----
def _oracle_logits(O, orc, w, hp, ktype, toks):
    """the oracle composition: the twin's final norm rows (the oracle's model takes one type), then the K output through its primitive"""
    _, taps = orc.evaluate(toks, mode=O.ref_mode(), taps=True)
    return O.mul_mat(ktype, w["output.weight"], hp["n_vocab"], hp["n_embd"], taps["final_norm"], mode=O.ref_mode())


@pytest.mark.parametrize("base,ktype", CASES)
@pytest.mark.parametrize("cfg", ["tiny", "gqa"])
def test_decode_matches_the_oracle(G, O, cfg, base, ktype):
    """Teacher-forced on the session's own K/V, as test_k_plan_matches_the_oracle_and_the_executor: |dlogit| / std within that
    file's bound for these shapes."""
    from llm_amd import llama
    hp, w, hpt, wt = _pair(O, {"tiny": TINY_K, "gqa": GQA_K}[cfg], base, ktype, 77)
    toks = np.random.default_rng([base, 5]).integers(0, hp["n_vocab"], 20).astype(np.int32)
    model = llama.Llama(hp, w, context_size=CTX)
    sess = model.start_session(n_batch=8)
    orc = O.Llama(hpt, wt, CTX)
    sess.evaluate(toks[:8])
    orc.evaluate(toks[:8], mode=O.ref_mode())
    worst = 0.0
    o0 = _stat(G, "out_k_tokens")
    for i in range(8, len(toks)):
        k, v = sess.get_kv()
        orc.memory_k[:] = k[:orc.memory_k.size]
        orc.memory_v[:] = v[:orc.memory_v.size]
        got = sess.evaluate(toks[i:i + 1])[-1]
        ref = _oracle_logits(O, orc, w, hp, ktype, toks[i:i + 1])[-1]
        worst = max(worst, float(np.max(np.abs(got - ref))) / float(ref.std()))
    assert _stat(G, "out_k_tokens") - o0 == len(toks) - 8
    sess.free()
    model.free()
    print(f"{cfg} base {base} output {ktype}: plan vs oracle worst |dlogit|/std = {worst:.2e}")
    assert worst <= BOUND[cfg]


# ---- 5: chains ----
def _seed(salt=0):
    return np.array([0x9E3779B97F4A7C15 + 0x1234567 * (salt + 1)], dtype=np.uint64)


@pytest.fixture(scope="module")
def mixed(G, O):
    from llm_amd import llama
    hp, w, _, _ = _pair(O, TINY_K, 2, Q6_K, 3)
    m = llama.Llama(hp, w, context_size=CTX)
    yield m
    m.free()


def _twins(model, n_prompt=9, seed=8):
    prompt = np.random.default_rng(seed).integers(0, model.hp["n_vocab"], n_prompt).astype(np.int32)
    a, b = (model.start_session(n_batch=8) for _ in range(2))
    for s in (a, b):
        s.feed_prompt(prompt)
    assert a.snapshot() == b.snapshot()
    return a, b


def _same(a, b):
    assert a.n_past == b.n_past
    assert np.array_equal(a.last_logits(), b.last_logits())
    assert a.snapshot() == b.snapshot()


def test_greedy_tokens_one_ahead_and_the_device_greedy_chain(G, mixed):
    keys = ("tail_tokens", "tail_hits", "plan_tokens", "out_k_tokens", "generic_graphs")
    a, b = _twins(mixed)
    s0 = _stats(G, keys)
    ids = [a.infer_next_token() for _ in range(16)]  # the device runs one token ahead (k_token_tail, tail_prepare)
    moved = _moved(G, keys, s0)
    assert moved[0] == 16 and moved[1] >= 14 and moved[4] == 0, moved
    assert _stat(G, "tail_prepared_tokens") > 0
    want = []
    for _ in range(16):  # the stepped loop: the argmax of the last logits on the host, then that token fed as any other
        want.append(int(np.argmax(b.last_logits())))
        b.feed_prompt(np.array([want[-1]], np.int32))
    assert ids == want
    _same(a, b)
    s0 = _stats(G, keys)
    got = a.infer_tokens_device(12)  # ggml_hip_decode_greedy_chain
    moved = _moved(G, keys, s0)
    assert moved[2] == 12 and moved[3] == 12 and moved[4] == 0, moved
    assert got.tolist() == [b.infer_next_token() for _ in range(12)]
    _same(a, b)
    a.free()
    b.free()


@pytest.mark.parametrize("prm", [dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30), dict(k=5, top_p=0.5, temperature=1.1, penalty=1.1)],
                         ids=["default", "truncating"])
def test_the_sampled_chain_equals_its_stepped_loop(G, mixed, prm):
    keys = ("sample_chain_tokens", "out_k_tokens", "generic_graphs")
    a, b = _twins(mixed, seed=21)
    ra, rb = _seed(1), _seed(1)
    a.infer_next_token_sampled(ra, **prm)  # (the chain continues the slot's most recent evaluation: a stepped token arms it)
    s0 = _stats(G, keys)
    n_dev, ids = a.infer_tokens_sampled_device(10, ra, **prm)
    assert n_dev == 10 and _moved(G, keys, s0) == [10, 10, 0]
    b.infer_next_token_sampled(rb, **prm)
    want = [b.infer_next_token_sampled(rb, **prm) for _ in range(10)]
    assert ids.tolist() == want and int(ra[0]) == int(rb[0])
    _same(a, b)
    a.free()
    b.free()


def test_infer_until_stops_where_the_stepped_loop_stops(G, mixed):
    prm = dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30)
    prompt = np.random.default_rng(33).integers(0, mixed.hp["n_vocab"], 9).astype(np.int32)
    free, step, chain = (mixed.start_session(n_batch=8) for _ in range(3))
    for s in (free, step, chain):
        s.feed_prompt(prompt)
    rngs = [_seed(2) for _ in range(3)]
    for s, r in zip((free, step, chain), rngs):
        s.infer_next_token_sampled(r, **prm)
    ids = [free.infer_next_token_sampled(rngs[0], **prm) for _ in range(14)]
    j = next(j for j in range(4, 14) if ids[j] not in ids[:j])  # a draw whose id is new: the chain stops there, not before
    want = [step.infer_next_token_sampled(rngs[1], **prm) for _ in range(j + 1)]
    assert want == ids[:j + 1]
    o0, g0 = _stat(G, "out_k_tokens"), _stat(G, "generic_graphs")
    got, count, why, ran = chain.infer_until(14, rngs[2], stop=[ids[j]], **prm)
    assert ran is True and why == "stop" and count == j + 1 and got.tolist() == want
    assert _stat(G, "out_k_tokens") - o0 >= j + 1 and _stat(G, "generic_graphs") == g0
    assert int(rngs[2][0]) == int(rngs[1][0])
    _same(chain, step)
    for s in (free, step, chain):
        s.free()


# ---- 6: batched ----
def _kv3(hp, k, v, ctx=CTX):
    L, Egqa = hp["n_layer"], hp["n_embd"] // (hp["n_head"] // hp["n_head_kv"])
    n = L * ctx * Egqa
    return k[:n].reshape(L, ctx, Egqa), v[:n].reshape(L, Egqa, ctx)


def test_a_batched_step_equals_the_chunk_and_the_batched_chains_their_stepped_loops(G, mixed):
    """evaluate_batch at B = 3: column c is row c of a 3-token chunk, byte for byte (tests/test_batch_decode_gpu.py's rule: the
    column is a fresh session holding the source's K/V below its position); infer_tokens_batch over 6 steps against the sessions
    stepped; infer_until_pool (5 requests over 2 columns, budgets 3 .. 6) against each session alone."""
    hp, B, P = mixed.hp, 3, 7
    rng = np.random.default_rng(4)
    keys = ("batch_decode_steps", "batch_decode_tokens", "out_k_tokens", "generic_graphs")
    src = mixed.start_session(n_batch=8)
    src.feed_prompt(rng.integers(0, hp["n_vocab"], P).astype(np.int32))
    chunk = rng.integers(0, hp["n_vocab"], B).astype(np.int32)
    ref = src.evaluate(chunk)
    k, v = src.get_kv()
    src.free()
    sessions = []
    for c in range(B):
        kc, vc = k.copy(), v.copy()
        K, V = _kv3(hp, kc, vc)
        K[:, P + c:, :] = 0x5555
        V[:, :, P + c:] = 0x5555
        f = mixed.start_session(n_batch=8)
        f.set_kv(kc, vc)
        f.seek(P + c)
        sessions.append(f)
    s0 = _stats(G, keys)
    ran, logits = mixed.evaluate_batch(sessions, chunk)
    assert ran and _moved(G, keys, s0) == [1, B, B, 0]
    Ks, Vs = _kv3(hp, k, v)
    for c, f in enumerate(sessions):
        assert np.array_equal(logits[c], ref[c]), (c, float(np.max(np.abs(logits[c] - ref[c]))))
        K, V = _kv3(hp, *f.get_kv())
        assert np.array_equal(K[:, P + c, :], Ks[:, P + c, :]) and np.array_equal(V[:, :, P + c], Vs[:, :, P + c]), c
        f.free()
    # the greedy chain of three sessions against the sessions stepped one by one
    prompts = [rng.integers(0, hp["n_vocab"], n).astype(np.int32) for n in (5, 9, 12)]
    chain, step = ([mixed.start_session(n_batch=8) for _ in prompts] for _ in range(2))
    for group in (chain, step):
        for s, p in zip(group, prompts):
            s.feed_prompt(p)
    s0 = _stats(G, keys + ("batch_chain_steps",))
    ran, ids = mixed.infer_tokens_batch(chain, 6)
    moved = _moved(G, keys + ("batch_chain_steps",), s0)
    assert ran and moved == [6, 18, 18, 0, 5], moved
    want = np.array([[s.infer_next_token() for s in step] for _ in range(6)], np.int32)
    assert np.array_equal(ids, want)
    for a, b in zip(chain, step):
        _same(a, b)
    for s in chain + step:
        s.free()
    # the request pool: 5 greedy requests with budgets 3 .. 6 over 2 columns, each against its session stepped alone
    budgets = (3, 6, 4, 5, 3)
    prompts = [rng.integers(0, hp["n_vocab"], 4 + i).astype(np.int32) for i in range(5)]
    pool, alone = ([mixed.start_session(n_batch=8) for _ in prompts] for _ in range(2))
    for group in (pool, alone):
        for s, p in zip(group, prompts):
            s.feed_prompt(p)
    want = [(np.array([s.infer_next_token() for _ in range(b)], np.int32), b, "budget") for s, b in zip(alone, budgets)]
    from llm_amd import llama
    pool_keys = ("pool_calls", "pool_admitted", "batch_decode_steps", "out_k_tokens", "generic_graphs")
    s0 = _stats(G, pool_keys)
    got, counts, why, ran = mixed.infer_until_pool(pool, [dict(max_tokens=b) for b in budgets], None, max_cols=2)
    moved = _moved(G, pool_keys, s0)
    evals = np.array(budgets, np.int32)  # no request ends early: the steps are the schedule of the budgets over 2 columns
    steps = llama._lib().llm_pool_schedule(evals.ctypes.data, len(evals), 2, None, None)
    assert ran and moved == [1, len(budgets) - 2, steps, 2 * steps, 0], (moved, steps)  # three admissions; both columns' lm_head every step
    for i in range(5):
        assert got[i].tolist() == want[i][0].tolist() and counts[i] == want[i][1] and why[i] == want[i][2], i
        _same(pool[i], alone[i])
    for s in pool + alone:
        s.free()


# ---- 7: prompt plan and prompt pack ----
def test_the_prompt_plan_meets_the_oracle_and_a_pack_equals_its_sessions_alone(G, O):
    """The last row of a 64- and a 32-token prompt batch against the oracle composition, at the bound tests/test_prompt_plan_gpu.py
    holds its shape to (the f16 GEMM: rms 2e-2 and max 1e-1 of std(logits)); feed_prompt_batch of three sessions: a segment of nine
    rows or more equals its session fed alone on the prompt plan (option mmq_min = 9), tests/test_prompt_pack_gpu.py's rule."""
    from llm_amd import llama
    hp, w, hpt, wt = _pair(O, TINY_K, 2, Q6_K, 1234)
    model = llama.Llama(hp, w, context_size=128)
    orc = O.Llama(hpt, wt, 128)
    toks = np.random.default_rng(3).integers(0, hp["n_vocab"], 96).astype(np.int32)
    sess = model.start_session(n_batch=64)
    try:
        for c in (toks[:64], toks[64:96]):
            s0 = _stats(G, PLAN_KEYS)
            got = sess.evaluate(c)[-1]
            assert _moved(G, PLAN_KEYS, s0) == [0, len(c), 0, 0, len(c)]
            ref = _oracle_logits(O, orc, w, hp, Q6_K, c)[-1]
            std = float(ref.std())
            rms, mx = float(np.sqrt(np.mean((got - ref) ** 2))) / std, float(np.max(np.abs(got - ref))) / std
            print(f"prompt plan, Q4_0 layers + Q6_K output, {len(c)} tokens: last row rms {rms:.2e} max {mx:.2e} of std(logits)")
            assert rms <= 2e-2 and mx <= 1e-1
            k, v = sess.get_kv()
            orc.memory_k[:] = k[:orc.memory_k.size]
            orc.memory_v[:] = v[:orc.memory_v.size]
        sess.free()
        lens = (40, 12, 33)
        prompts = [np.random.default_rng([7, n]).integers(0, hp["n_vocab"], n).astype(np.int32) for n in lens]
        packed = [model.start_session(n_batch=192) for _ in lens]
        keys = ("prompt_pack_calls", "prompt_pack_tokens", "out_k_tokens", "generic_graphs")
        s0 = _stats(G, keys)
        assert model.feed_prompt_batch(packed, prompts) == 1
        assert _moved(G, keys, s0) == [1, sum(lens), sum(lens), 0]
        G.set_option("mmq_min", 9)
        for s, p in zip(packed, prompts):
            twin = model.start_session(n_batch=192)
            p0 = _stat(G, "prompt_plan_tokens")
            twin.feed_prompt(p)
            assert _stat(G, "prompt_plan_tokens") - p0 == len(p)
            _same(s, twin)
            twin.free()
            s.free()
    finally:
        G.set_option("mmq_min", 32)
        model.free()


# ---- 8: file ----
def test_a_block_format_file_with_a_q6_k_output_loads_and_decodes_on_the_plan(G, O, tmp_path):
    from llm_amd import llama, synth
    hp0 = dict(n_vocab=256, n_embd=256, n_head=4, n_head_kv=4, n_layer=2, n_rot=64, n_ff=512, n_mult=32)  # the file format has no n_head_kv
    hp, w, _, _ = _pair(O, hp0, 2, Q6_K, 19)
    path = tmp_path / "q4_0_q6_k_output.bin"
    synth.write_ggjt(str(path), hp, w)
    toks = np.random.default_rng(3).integers(0, hp["n_vocab"], 13).astype(np.int32)

    def run(model):
        s = model.start_session(n_batch=8)
        s.feed_prompt(toks[:12])
        s0 = _stats(G, PLAN_KEYS)
        first = s.evaluate(toks[12:13])[-1].copy()
        assert _moved(G, PLAN_KEYS, s0) == [1, 1, 0, 0, 0]  # the first decode token runs on the plan
        ids = [s.infer_next_token() for _ in range(6)]
        last = s.last_logits().copy()
        s.free()
        return first, ids, last

    mem = llama.Llama(hp, w, context_size=64)
    a = run(mem)
    mem.free()
    fil = llama.Llama.load(str(path), context_size=64)
    b = run(fil)
    fil.free()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


# ---- 9: layer split ----
def test_a_layer_split_over_two_device_slots_reproduces_the_unsplit_session(G, O):
    from llm_amd import llama
    L = G.lib()
    assert L.ggml_hip_get_main_device() == 0
    hp, w, _, _ = _pair(O, TINY_K, 2, Q6_K, 41)
    toks = np.random.default_rng(4).integers(0, hp["n_vocab"], 20).astype(np.int32)

    def last_stage_stat():
        L.ggml_hip_set_main_device(1)
        try:
            return _stat(G, "out_k_tokens")
        finally:
            L.ggml_hip_set_main_device(0)

    whole = llama.Llama(hp, w, context_size=64)
    ref = _prompt_and_decode(G, whole, toks)
    whole.free()
    assert ref[4] == [20, 20, 0, 0, 0]
    os.environ["GGML_HIP_VIRTUAL_DEVICES"] = "2"
    os.environ["GGML_HIP_LAYER_SPLIT"] = "2"
    try:
        split = llama.Llama(hp, w, context_size=64)
        assert split.stages() == [(0, 1, 0), (1, 2, 1)]
        o0 = last_stage_stat()
        got = _prompt_and_decode(G, split, toks, emb=False)
        ran_last = last_stage_stat() - o0
        split.free()
    finally:
        os.environ.pop("GGML_HIP_LAYER_SPLIT", None)
        L.ggml_hip_set_layer_split(None, 0)
        L.ggml_hip_set_main_device(0)
        os.environ.pop("GGML_HIP_VIRTUAL_DEVICES", None)
    assert got[4][0] == 20 and got[4][1] == 0 and got[4][2] == 0, got[4]  # slot 0's stage: a block-format plan without an lm_head
    assert ran_last == 20  # the last stage's lm_head ran as the K launch
    for a, b in zip(ref[0], got[0]):
        assert np.array_equal(a, b)
    assert np.array_equal(ref[2], got[2]) and np.array_equal(ref[3], got[3])
