"""Batched multi-session decode (ggml_hip_decode_batch / llm_evaluate_batch / Llama.evaluate_batch): one decode step of
2..8 sessions of one model as ONE pass over the weights — the chunk plan's launches (plan_launch_batch) with the three kernels
that place a column in a cache (k_rope_table_batch, the BATCH forms of k_mmvq_big8 / k_mmq_cols's wq|wk|wv epilogue,
k_attn_decode_batch) reading a per-column table of positions and caches.

Shapes: synth.TINY (E = 128: every mat-vec on k_mmvq_big8) and the GQA2 shape of tests/test_mmq_cols_gpu.py (E = 1024, 8 heads
over 4 K/V heads: every mat-vec on k_mmq_cols, narrow K/V rows), context 64.  Tolerances against the oracle are those documented
at the top of tests/test_llama_gpu.py (STRICT, EDGE, relative to std(logits)); against the chunk plan and against the sessions
evaluated one by one the batched step must agree BIT FOR BIT where the same kernels run on both sides."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STRICT, EDGE = 1e-5, 4e-2
GQA2 = dict(n_vocab=512, n_embd=1024, n_head=8, n_head_kv=4, n_layer=2, n_rot=128, n_ff=2816, n_mult=32)
CTX = 64
SENTINEL = 0x5555  # a finite f16 (85.3): rows past a column's position are loaded by the attention's first pass and must be ignored
CASES = [("tiny", t) for t in (2, 3, 6, 7, 8)] + [("gqa2", t) for t in (2, 8)]


def _stat(G, key):
    return int(G.lib().ggml_hip_get_stat(key.encode()))


def _hp0(cfg):
    from llm_amd import synth
    return synth.TINY if cfg == "tiny" else GQA2


def _mk(cfg, wtype, seed=1234, ctx=CTX):
    from llm_amd import llama, synth
    hp, w = synth.make_llama(_hp0(cfg), wtype, seed=seed)
    return hp, w, llama.Llama(hp, w, context_size=ctx)


def _assert_cols_path(G, O, cfg, B):
    """GQA2 is here for k_mmq_cols: the hook that launches it 'exactly as the multi-token plan' answers -1 for a shape the plan
    would give to k_mmvq_big8 instead (cols_ok).  Asked for all five mat-vec shapes of the model; TINY (4 blocks per row) must be refused."""
    hp = _hp0(cfg)
    E, F, V = hp["n_embd"], hp["n_ff"], hp["n_vocab"]
    Egqa = E // (hp["n_head"] // hp["n_head_kv"])
    assert E % 16 == 0 and Egqa % 16 == 0 and F % 16 == 0
    for M, K in ((E + 2 * Egqa, E), (E, E), (F, E), (E, F), (V, E)):
        W_raw = O.quantize(2, np.zeros((M, K), np.float32))
        out = np.zeros((B, M), np.float32)
        X = np.zeros((B, K), np.float32)
        with G.Context(W_raw.nbytes + (1 << 20)) as ctx:
            w = ctx.tensor_from(W_raw, 2, (K, M)).set_name("w")
            w.transfer_to_gpu()
            rc = G.lib().ggml_hip_debug_mul_mat_cols(w.ptr, X.ctypes.data, out.ctypes.data, B)
        assert rc == (0 if cfg == "gqa2" else -1), (cfg, M, K, rc)


def _feed(sess, toks):
    for i in range(0, len(toks), 8):
        sess.evaluate(toks[i:i + 8], want_all_logits=False)


def _kv3(hp, k, v, ctx=CTX):
    """Views of memory_k as [layer][position][channel] and of memory_v as [layer][channel][position] (kernels/decode.h
    DecMmvqArgs::mem_k / mem_v).  The session allocates n_embd elements per position; with grouped K/V heads the layers' rows,
    n_embd_gqa wide, fill the front of it."""
    L, Egqa = hp["n_layer"], hp["n_embd"] // (hp["n_head"] // hp["n_head_kv"])
    n = L * ctx * Egqa
    return k[:n].reshape(L, ctx, Egqa), v[:n].reshape(L, Egqa, ctx)


@pytest.mark.parametrize("B", [8, 3])
@pytest.mark.parametrize("cfg,wtype", CASES)
def test_batched_step_equals_the_chunk_plan_bit_for_bit(G, O, cfg, wtype, B):
    """Column c of a batched step against column c of a CHUNK of B tokens (existing code: plan_launch_multi), at non-consecutive
    positions and in different caches.  Two source sessions S0, S1 are fed prompts of 5 and 23 tokens, then each evaluates a chunk
    of B tokens (logits R_s[c]).  Batch column c (s = c mod 2) is a fresh session holding S_s's post-chunk K/V with every position
    >= P_s + c overwritten by a sentinel, seeked to P_s + c, given token chunk_s[c].  Every kernel of the plan is column-local (a
    column's arithmetic reads that column's inputs only) and column index and column count are the same on both sides, so: logits
    column c == R_s[c], position P_s + c of session c's K and V == S_s's, positions below unchanged, positions above still the
    sentinel — all bit for bit."""
    hp, w, model = _mk(cfg, wtype, seed=5)
    _assert_cols_path(G, O, cfg, B)
    rng = np.random.default_rng([wtype, B])
    P = (5, 23)
    ref, kv, chunk = [], [], []
    for s in (0, 1):
        src = model.start_session(n_batch=8)
        _feed(src, rng.integers(0, hp["n_vocab"], P[s]).astype(np.int32))
        chunk.append(rng.integers(0, hp["n_vocab"], B).astype(np.int32))
        p0 = _stat(G, "plan_tokens")
        ref.append(src.evaluate(chunk[s]))
        assert _stat(G, "plan_tokens") - p0 == B  # the chunk plan ran it
        kv.append(src.get_kv())
        src.free()
    sessions, toks, before = [], [], []
    for c in range(B):
        s = c % 2
        k, v = kv[s][0].copy(), kv[s][1].copy()
        K, V = _kv3(hp, k, v)
        K[:, P[s] + c:, :] = SENTINEL
        V[:, :, P[s] + c:] = SENTINEL
        f = model.start_session(n_batch=8)
        f.set_kv(k, v)
        f.seek(P[s] + c)
        sessions.append(f)
        toks.append(chunk[s][c])
        before.append((k, v))
    s0, t0, p0 = _stat(G, "batch_decode_steps"), _stat(G, "batch_decode_tokens"), _stat(G, "plan_tokens")
    ran, logits = model.evaluate_batch(sessions, toks)
    assert ran and _stat(G, "batch_decode_steps") - s0 == 1 and _stat(G, "batch_decode_tokens") - t0 == B
    assert _stat(G, "plan_tokens") - p0 == B
    for c, f in enumerate(sessions):
        s, at = c % 2, P[c % 2] + c
        assert np.array_equal(logits[c], ref[s][c]), (c, float(np.max(np.abs(logits[c] - ref[s][c]))))
        assert f.n_past == at + 1 and np.array_equal(f.last_logits(), logits[c])
        k, v = f.get_kv()
        K, V = _kv3(hp, k, v)
        Ks, Vs = _kv3(hp, *kv[s])
        Kb, Vb = _kv3(hp, *before[c])
        assert np.array_equal(K[:, at, :], Ks[:, at, :]) and np.array_equal(V[:, :, at], Vs[:, :, at]), c
        assert np.array_equal(K[:, :at, :], Kb[:, :at, :]) and np.array_equal(V[:, :, :at], Vb[:, :, :at]), c
        assert np.all(K[:, at + 1:, :] == SENTINEL) and np.all(V[:, :, at + 1:] == SENTINEL), c
        f.free()
    model.free()


@pytest.mark.parametrize("cfg,wtype", CASES)
def test_ragged_batch_matches_the_oracle(G, O, cfg, wtype):
    """Sessions at n_past = 0, 1, 7, 33 and 63 (the last slot of the context) in one step; each session's K/V goes into an
    oracle session (as test_logits_match_oracle_prompt_and_decode does) that evaluates the same token at the same position.
    Every column within EDGE * std(logits); how many meet STRICT is printed.  A session whose context is full is an error of
    the host call (at n_past == context no graph of that session can be built, so the backend's own -1 is reached through the
    matcher's T <= C only) and nothing is evaluated."""
    hp, w, model = _mk(cfg, wtype, seed=7)
    rng = np.random.default_rng([wtype, 2])
    pasts = (0, 1, 7, 33, 63)
    sessions, orcs = [], []
    for n in pasts:
        f = model.start_session(n_batch=8)
        if n:
            _feed(f, rng.integers(0, hp["n_vocab"], n).astype(np.int32))
        o = O.Llama(hp, w, CTX)
        k, v = f.get_kv()
        o.memory_k[:] = k[:o.memory_k.size]  # (grouped K/V heads: the session's buffer is n_embd wide, its rows n_embd_gqa)
        o.memory_v[:] = v[:o.memory_v.size]
        o.n_past = n
        sessions.append(f)
        orcs.append(o)
    toks = rng.integers(0, hp["n_vocab"], len(pasts)).astype(np.int32)
    s0 = _stat(G, "batch_decode_steps")
    ran, logits = model.evaluate_batch(sessions, toks)
    assert ran and _stat(G, "batch_decode_steps") - s0 == 1
    n_strict = 0
    for c, (f, o) in enumerate(zip(sessions, orcs)):
        ref = o.evaluate(toks[c:c + 1], mode=O.ref_mode())[0]
        d = float(np.max(np.abs(logits[c] - ref))) / float(ref.std())
        print(f"{cfg} type {wtype} n_past {pasts[c]}: gpu-vs-exact {d:.2e}")
        assert d <= EDGE, (c, pasts[c], d)
        n_strict += d <= STRICT
        assert f.n_past == pasts[c] + 1
    print(f"{cfg} type {wtype}: {n_strict} of {len(pasts)} columns within {STRICT} of the oracle")
    # the session at position 63 now stands at 64 == context: no further step, batched or not
    assert sessions[-1].n_past == CTX
    n_before = [f.n_past for f in sessions]
    s0, p0 = _stat(G, "batch_decode_steps"), _stat(G, "plan_tokens")
    with pytest.raises(ValueError):
        model.evaluate_batch(sessions, toks)
    assert [f.n_past for f in sessions] == n_before and _stat(G, "batch_decode_steps") == s0 and _stat(G, "plan_tokens") == p0
    for f in sessions:
        f.free()
    model.free()


@pytest.mark.parametrize("cfg,wtype", [("tiny", 2), ("tiny", 7), ("gqa2", 8)])
def test_steps_in_a_row_replay_one_graph_and_keep_the_sessions_books(G, O, cfg, wtype):
    """Six batched steps of four sessions with fixed, different token streams, against the same streams decoded alone (the
    single-token plan: other kernels, another summation order -> EDGE, not bits).  The step's hipGraph is captured once and
    replayed (graph_replays grows with every step from the second on, the plan count does not); n_past, last_logits and a
    rewind(1) followed by a single evaluate behave as for a session decoded alone."""
    hp, w, model = _mk(cfg, wtype, seed=9)
    rng = np.random.default_rng([wtype, 3])
    prompts = [rng.integers(0, hp["n_vocab"], n).astype(np.int32) for n in (3, 9, 14, 20)]
    streams = rng.integers(0, hp["n_vocab"], (4, 6)).astype(np.int32)
    alone_logits = []
    for p, st in zip(prompts, streams):  # each stream decoded alone
        a = model.start_session(n_batch=8)
        _feed(a, p)
        for t in st:
            last = a.evaluate([t])[0]
        alone_logits.append(last)
        assert a.n_past == len(p) + 6
        a.free()
    sessions = []
    for p in prompts:
        f = model.start_session(n_batch=8)
        _feed(f, p)
        sessions.append(f)
    s0 = _stat(G, "batch_decode_steps")
    for step in range(6):
        r0, n0 = _stat(G, "graph_replays"), _stat(G, "plans")
        ran, logits = model.evaluate_batch(sessions, streams[:, step])
        assert ran
        if step >= 1:
            assert _stat(G, "graph_replays") - r0 == 1 and _stat(G, "plans") == n0, step
        for c, f in enumerate(sessions):
            assert f.n_past == len(prompts[c]) + step + 1
            assert np.array_equal(f.last_logits(), logits[c])
    assert _stat(G, "batch_decode_steps") - s0 == 6
    for c, f in enumerate(sessions):
        d = float(np.max(np.abs(logits[c] - alone_logits[c]))) / float(alone_logits[c].std())
        print(f"{cfg} type {wtype} session {c}: batched-vs-alone {d:.2e}")
        assert d <= EDGE, (c, d)
    # rewind(1) + the last token again, alone: the session's own single-token evaluation of that position
    for c, f in enumerate(sessions):
        assert f.rewind(1) == 0 and f.n_past == len(prompts[c]) + 5
        again = f.evaluate([streams[c, 5]])[0]
        assert f.n_past == len(prompts[c]) + 6 and np.array_equal(f.last_logits(), again)
        d = float(np.max(np.abs(again - alone_logits[c]))) / float(alone_logits[c].std())
        assert d <= EDGE, (c, d)
        f.free()
    model.free()


def _one_by_one(model, prompts, toks, kv_type):
    out = []
    for p, t in zip(prompts, toks):
        a = model.start_session(n_batch=8, kv_type=kv_type)
        _feed(a, p)
        lg = a.evaluate([t])[0]
        out.append((lg, a.get_kv(np.uint8)))
        a.free()
    return out


@pytest.mark.parametrize("case", ["q4_k", "f32_kv", "nine", "plan_batch_0"])
def test_what_the_backend_declines_runs_one_by_one_with_the_same_bits(G, O, case):
    """A K-quant model, f32 K/V, nine sessions, option plan_batch = 0: the step is evaluated session after session (ran_batched
    False, batch_decode_steps does not move) and every session's logits and K/V are bit-identical to evaluating it alone."""
    from llm_amd import llama, synth
    B = 9 if case == "nine" else 3
    kv_type = G.TYPE_F32 if case == "f32_kv" else G.TYPE_F16
    if case == "q4_k":
        hp0 = dict(n_vocab=256, n_embd=256, n_head=4, n_head_kv=4, n_layer=2, n_rot=64, n_ff=512, n_mult=32)
        rng = np.random.default_rng(12)
        hp, w = dict(hp0), {}
        for name, (ne0, ne1) in synth.tensor_shapes(hp).items():
            w[name] = ((1.0 + 0.01 * rng.standard_normal(ne0)).astype(np.float32) if ne1 is None else
                       O.quantize(G.TYPE_Q4_K, (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32)))
        hp["wtype"] = G.TYPE_Q4_K
    else:
        hp, w = synth.make_llama(synth.TINY, 2, seed=3)
    model = llama.Llama(hp, w, context_size=CTX)
    rng = np.random.default_rng(4)
    prompts = [rng.integers(0, hp["n_vocab"], 2 + 3 * i).astype(np.int32) for i in range(B)]
    toks = rng.integers(0, hp["n_vocab"], B).astype(np.int32)
    want = _one_by_one(model, prompts, toks, kv_type)
    sessions = []
    for p in prompts:
        f = model.start_session(n_batch=8, kv_type=kv_type)
        _feed(f, p)
        sessions.append(f)
    if case == "plan_batch_0":
        G.set_option("plan_batch", 0)
    try:
        s0 = _stat(G, "batch_decode_steps")
        ran, logits = model.evaluate_batch(sessions, toks)
        assert not ran and _stat(G, "batch_decode_steps") == s0
    finally:
        G.set_option("plan_batch", 1)
    for c, f in enumerate(sessions):
        assert np.array_equal(logits[c], want[c][0]), c
        k, v = f.get_kv(np.uint8)
        assert np.array_equal(k, want[c][1][0]) and np.array_equal(v, want[c][1][1]), c
        assert f.n_past == len(prompts[c]) + 1
    if case == "plan_batch_0":  # ... and with the option back on the same sessions take the batched step
        ran, _ = model.evaluate_batch(sessions, toks)
        assert ran and _stat(G, "batch_decode_steps") == s0 + 1
    for f in sessions:
        f.free()
    model.free()


def test_bad_arguments_evaluate_nothing(G, O):
    """A session listed twice, a session of another model, a token outside the vocabulary: ValueError (llm_evaluate_batch -1),
    no session moves, no counter moves."""
    hp, w, model = _mk("tiny", 2, seed=3)
    hp2, w2, other = _mk("tiny", 2, seed=4)
    a, b, x = model.start_session(), model.start_session(), other.start_session()
    for f in (a, b, x):
        f.evaluate([1, 2, 3], want_all_logits=False)
    p0, s0 = _stat(G, "plan_tokens"), _stat(G, "batch_decode_steps")
    for sessions, toks in (([a, a], [5, 6]), ([a, b, a], [5, 6, 7]), ([a, x], [5, 6]), ([a, b], [5, hp["n_vocab"]]), ([a, b], [-1, 5])):
        with pytest.raises(ValueError):
            model.evaluate_batch(sessions, toks)
    assert [f.n_past for f in (a, b, x)] == [3, 3, 3]
    assert (_stat(G, "plan_tokens"), _stat(G, "batch_decode_steps")) == (p0, s0)
    ran, ids = model.infer_next_tokens_batch([a, b])  # the greedy step: the first maximum of each session's last_logits
    assert ran and a.n_past == 4 and b.n_past == 4
    for f in (a, b, x):
        f.free()
    model.free()
    other.free()


def test_greedy_batch_samples_what_the_sessions_sample_alone(G, O):
    """infer_next_tokens_batch against Session.infer_next_token on twin sessions, 5 steps: every session's id is the first maximum
    of ITS last_logits (llm_argmax_first), its token history and n_past advance by one, and the ids equal the twins' — the two
    sides run different kernels (EDGE), so a step where a twin's two best logits are closer than EDGE * std may differ, and the
    comparison of that pair of sessions ends there."""
    hp, w, model = _mk("tiny", 8, seed=21)
    rng = np.random.default_rng(8)
    prompts = [rng.integers(0, hp["n_vocab"], n).astype(np.int32) for n in (4, 11, 6)]
    twins, batch = [], []
    for p in prompts:
        for lst in (twins, batch):
            f = model.start_session(n_batch=8)
            f.feed_prompt(p)
            lst.append(f)
    live = [True] * len(prompts)
    for step in range(5):
        want = [int(np.argmax(f.last_logits())) for f in batch]
        ran, ids = model.infer_next_tokens_batch(batch)
        assert ran and list(ids) == want
        for c, t in enumerate(twins):
            top = np.sort(t.last_logits())[-2:]
            near_tie = (top[1] - top[0]) <= EDGE * float(t.last_logits().std())
            alone = t.infer_next_token()
            assert batch[c].n_past == len(prompts[c]) + step + 1
            if live[c] and ids[c] != alone:
                assert near_tie, (step, c, ids[c], alone)
                live[c] = False
    assert any(live)
    for f in twins + batch:
        f.free()
    model.free()
