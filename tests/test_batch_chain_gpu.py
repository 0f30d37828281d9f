"""The batched greedy chain (ggml_hip_decode_batch_greedy / llm_infer_tokens_greedy_batch_device / Llama.infer_tokens_batch):
n greedy tokens for each of B sessions of one model, every step one pass over the weights, the argmax and the next step's
parameters on the device (k_argmax_next, one workgroup per column) and the step's captured graph replayed — no host round trip between steps.

The chain makes the launches n calls of infer_next_tokens_batch make, on the same inputs: every comparison with that loop below
is equality (ids, and Session.snapshot() — n_past, token history, last_logits, K/V — byte for byte), with no tolerance.  Only
the comparison with a session's own single-token evaluation (other kernels) uses EDGE, the bound documented at the top of
tests/test_llama_gpu.py.  Contexts are 64."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDGE = 4e-2
GQA2 = dict(n_vocab=512, n_embd=1024, n_head=8, n_head_kv=4, n_layer=2, n_rot=128, n_ff=2816, n_mult=32)
CTX = 64
N = 6
F16 = 1  # ggml's type number of F16 weights
MODELS = [("tiny", 2), ("tiny", 7), ("tiny", 8), ("gqa2", 2), ("gqa2", 8), ("tiny", F16)]
COUNTERS = ("batch_chain_steps", "batch_chain_tokens", "batch_decode_steps", "batch_decode_tokens", "plan_tokens")


def _stat(G, key):
    return int(G.lib().ggml_hip_get_stat(key.encode()))


def _stats(G):
    return [_stat(G, k) for k in COUNTERS]


def _mk(cfg, wtype, seed):
    from llm_amd import llama, synth
    hp, w = synth.make_llama(synth.TINY if cfg == "tiny" else GQA2, wtype, seed=seed)
    return hp, llama.Llama(hp, w, context_size=CTX)


def _twins(model, prompts, **kw):
    """Two sets of sessions fed the same prompts: the same state, bit for bit."""
    a, b = [], []
    for p in prompts:
        for lst in (a, b):
            f = model.start_session(n_batch=8, **kw)
            f.feed_prompt(p)
            lst.append(f)
    for x, y in zip(a, b):
        assert x.snapshot() == y.snapshot()
    return a, b


def _stepped(model, sessions, n):
    rows, ran = [], []
    for _ in range(n):
        r, ids = model.infer_next_tokens_batch(sessions)
        rows.append(ids)
        ran.append(r)
    return ran, np.stack(rows)


def _same(chain, step):
    for c, (x, y) in enumerate(zip(chain, step)):
        assert x.n_past == y.n_past, c
        assert x.snapshot() == y.snapshot(), c


def _free(*things):
    for t in things:
        for f in (t if isinstance(t, list) else [t]):
            f.free()


# ---- the tail kernel alone ----
def _rows(B, V):
    """Column c carries row family c mod 4 of tests/test_token_tail_gpu.py's _op_cases: random, a tie of the first and the last
    entry, the maximum in the last (partial) group of four, all equal."""
    rng = np.random.default_rng([B, V])
    rows = rng.standard_normal((B, V)).astype(np.float32)
    for c in range(B):
        if c % 4 == 1:
            rows[c, 0] = rows[c, V - 1] = np.float32(9.0)
        elif c % 4 == 2:
            rows[c, V - 1] = np.float32(11.0)
        elif c % 4 == 3:
            rows[c, :] = np.float32(-0.5)
    return rows


@pytest.mark.parametrize("B", [1, 2, 8])
@pytest.mark.parametrize("V", [1, 3, 1000, 32000, 32001])
def test_k_batch_argmax_next_alone(G, V, B):
    rows = _rows(B, V)
    pos_in = (np.arange(8, dtype=np.int32) * 7 + 3) % 60
    tokens_in = np.arange(32, dtype=np.int32) + 70000  # sentinels: no id of any vocabulary here
    ids = np.full(8, -1, np.int32)
    prm, pos_out = np.full(34, -1, np.int32), np.full(8, -1, np.int32)
    rc = G.lib().ggml_hip_debug_batch_tail(rows.ctypes.data, B, V, pos_in.ctypes.data, tokens_in.ctypes.data, ids.ctypes.data,
                                           prm.ctypes.data, pos_out.ctypes.data)
    assert rc == 0
    want = [int(np.argmax(rows[c])) for c in range(B)]  # the first maximum
    assert ids[:B].tolist() == want and np.all(ids[B:] == -1)
    assert pos_out[:B].tolist() == (pos_in[:B] + 1).tolist()
    assert pos_out[B:].tolist() == pos_in[B:].tolist()  # entries from B on are not touched
    assert prm.tolist() == [int(pos_in[0]) + 1, want[0]] + want + tokens_in[B:].tolist()


# ---- the chain against the stepped loop ----
@pytest.mark.parametrize("B", [2, 5, 8])
@pytest.mark.parametrize("cfg,wtype", MODELS)
def test_chain_equals_the_stepped_loop_bit_for_bit(G, O, cfg, wtype, B):
    """Twin sets of sessions with ragged prompts: one takes one infer_tokens_batch(N), the other N infer_next_tokens_batch, twice
    over.  Ids equal, snapshots byte-identical, the counters move as documented; the second chain builds no plan and replays the
    step's graph N times (so does the stepped loop)."""
    hp, model = _mk(cfg, wtype, seed=31)
    rng = np.random.default_rng([wtype, B])
    prompts = [rng.integers(0, hp["n_vocab"], 2 + 3 * c).astype(np.int32) for c in range(B)]
    chain, step = _twins(model, prompts)
    for rnd in range(2):
        s0, p0, r0 = _stats(G), _stat(G, "plans"), _stat(G, "graph_replays")
        ran, ids = model.infer_tokens_batch(chain, N)
        assert ran is True and ids.shape == (N, B)
        d = [b - a for a, b in zip(s0, _stats(G))]
        assert d == [N - 1, (N - 1) * B, N, N * B, N * B], (rnd, d)
        if rnd == 1:
            assert _stat(G, "plans") == p0 and _stat(G, "graph_replays") - r0 == N
        s0, r0 = _stats(G), _stat(G, "graph_replays")
        ran_s, ids_s = _stepped(model, step, N)
        d = [b - a for a, b in zip(s0, _stats(G))]
        assert all(ran_s) and d == [0, 0, N, N * B, N * B], (rnd, d)
        if rnd == 1:
            assert _stat(G, "plans") == p0 and _stat(G, "graph_replays") - r0 == N
        assert np.array_equal(ids, ids_s), (rnd, ids, ids_s)
        _same(chain, step)
        for c, f in enumerate(chain):
            assert f.n_past == len(prompts[c]) + (rnd + 1) * N
    _free(chain, step, model)


def test_one_step_is_the_batched_step(G, O):
    hp, model = _mk("tiny", 2, seed=32)
    rng = np.random.default_rng(5)
    chain, step = _twins(model, [rng.integers(0, hp["n_vocab"], n).astype(np.int32) for n in (4, 9, 2)])
    s0 = _stats(G)
    ran, ids = model.infer_tokens_batch(chain, 1)
    assert ran is True and [b - a for a, b in zip(s0, _stats(G))] == [0, 0, 1, 3, 3]
    ran_s, ids_s = model.infer_next_tokens_batch(step)
    assert ran_s and np.array_equal(ids, ids_s[None, :])
    _same(chain, step)
    _free(chain, step, model)


def test_the_context_edge(G, O):
    """A session at n_past == C - N chains to the context's last position; one at C - N + 1 is refused and nothing moves."""
    hp, model = _mk("tiny", 8, seed=33)
    rng = np.random.default_rng(6)
    prompts = [rng.integers(0, hp["n_vocab"], n).astype(np.int32) for n in (CTX - N, 3, 17)]
    chain, step = _twins(model, prompts)
    ran, ids = model.infer_tokens_batch(chain, N)
    assert ran is True and chain[0].n_past == CTX
    ran_s, ids_s = _stepped(model, step, N)
    assert all(ran_s) and np.array_equal(ids, ids_s)
    _same(chain, step)
    _free(chain, step)
    late = []
    for n in (CTX - N + 1, 3):
        f = model.start_session(n_batch=8)
        f.feed_prompt(rng.integers(0, hp["n_vocab"], n).astype(np.int32))
        late.append(f)
    s0 = _stats(G)
    with pytest.raises(ValueError):
        model.infer_tokens_batch(late, N)
    assert [f.n_past for f in late] == [CTX - N + 1, 3] and _stats(G) == s0
    ran, ids = model.infer_tokens_batch(late, N - 1)  # ... and N - 1 tokens fit
    assert ran is True and late[0].n_past == CTX
    _free(late, model)


def test_bad_arguments_evaluate_nothing(G, O):
    """A session listed twice, a session of another model, n = 0: ValueError, no session moves, no counter moves."""
    hp, model = _mk("tiny", 2, seed=3)
    hp2, other = _mk("tiny", 2, seed=4)
    a, b, x = model.start_session(), model.start_session(), other.start_session()
    for f in (a, b, x):
        f.evaluate([1, 2, 3], want_all_logits=False)
    s0 = _stats(G)
    for sessions, n in (([a, a], 3), ([a, b, a], 3), ([a, x], 3), ([a, b], 0), ([a, b], -2)):
        with pytest.raises(ValueError):
            model.infer_tokens_batch(sessions, n)
    assert [f.n_past for f in (a, b, x)] == [3, 3, 3] and _stats(G) == s0
    ran, ids = model.infer_tokens_batch([a, b], 3)
    assert ran is True and a.n_past == 6 and b.n_past == 6
    _free([a, b, x], model, other)


@pytest.mark.parametrize("case", ["q4_k", "f32_kv", "nine", "plan_batch_chain_0", "plan_batch_0"])
def test_what_the_backend_declines_runs_as_the_stepped_loop(G, O, case):
    """A K-quant model, f32 K/V, nine sessions, option plan_batch_chain = 0, option plan_batch = 0: ran_chained is False, no chained
    step is counted, and ids and snapshots equal those of twins stepped with infer_next_tokens_batch under the same options."""
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
    chain, step = _twins(model, prompts, kv_type=kv_type)
    option = case[:-2] if case.endswith("_0") else None
    if option:
        G.set_option(option, 0)
    try:
        s0 = _stats(G)
        ran, ids = model.infer_tokens_batch(chain, N)
        assert ran is False and _stats(G)[:2] == s0[:2]
        ran_s, ids_s = _stepped(model, step, N)
    finally:
        if option:
            G.set_option(option, 1)
    assert all(ran_s) == (case == "plan_batch_chain_0")  # (that option leaves the single batched step alone)
    assert np.array_equal(ids, ids_s)
    _same(chain, step)
    if option:  # ... and with the option back on the same sessions chain
        s0 = _stats(G)
        ran, ids = model.infer_tokens_batch(chain, N)
        assert ran is True and _stats(G)[0] - s0[0] == N - 1
        ran_s, ids_s = _stepped(model, step, N)
        assert all(ran_s) and np.array_equal(ids, ids_s)
        _same(chain, step)
    _free(chain, step, model)


def test_after_a_chain_the_sessions_go_on_as_usual(G, O):
    """rewind(1) plus a single evaluate of the last id reproduces last_logits within EDGE (the single-token plan: other kernels);
    infer_next_token takes the first maximum of the session's last_logits; a batched step of the same sessions runs and builds no
    plan."""
    hp, model = _mk("tiny", 7, seed=34)
    rng = np.random.default_rng(9)
    prompts = [rng.integers(0, hp["n_vocab"], n).astype(np.int32) for n in (3, 9, 14, 20)]
    sessions = []
    for p in prompts:
        f = model.start_session(n_batch=8)
        f.feed_prompt(p)
        sessions.append(f)
    ran, ids = model.infer_tokens_batch(sessions, N)
    assert ran is True
    f = sessions[0]
    after = f.last_logits().copy()
    assert f.rewind(1) == 0 and f.n_past == len(prompts[0]) + N - 1
    again = f.evaluate([ids[N - 1, 0]])[0]
    assert f.n_past == len(prompts[0]) + N and np.array_equal(f.last_logits(), again)
    d = float(np.max(np.abs(again - after))) / float(after.std())
    print(f"chain-vs-alone {d:.2e}")
    assert d <= EDGE, d
    want = int(np.argmax(f.last_logits()))
    assert f.infer_next_token() == want and f.n_past == len(prompts[0]) + N + 1
    p0, s0 = _stat(G, "plans"), _stats(G)
    wants = [int(np.argmax(g.last_logits())) for g in sessions]
    ran, step_ids = model.infer_next_tokens_batch(sessions)
    assert ran and list(step_ids) == wants and _stat(G, "plans") == p0
    assert [b - a for a, b in zip(s0, _stats(G))] == [0, 0, 1, 4, 4]
    _free(sessions, model)
