"""Batched multi-session decode of K-quant models (option plan_batch_k): one decode step of 2..8 sessions of a Q2_K … Q6_K model,
uniform or mixed, as ONE pass over the weights — the K plan's chunk form (plan_decode.inc plan_launch_k, batch = true) with the three
launches that place a column read a per-column table of positions and caches: k_rope_table_batch, k_k_rope_store<true>
(kernels/kquant_plan.h) and k_attn_decode_batch.  Evaluate_batch and the two chains on it (infer_tokens_batch,
infer_tokens_sampled_batch) need nothing else: their tail kernels read logits, DecParams and BatchCols only.

The option's default is 0 (three older GPU tests pin that a Q4_K model at default options is declined), so every test here turns it
on in a try and restores 0 in a finally; each first asks for the counter batch_k_steps, which a library without the feature
answers with -1.

Shapes are those of tests/test_kquant_plan_gpu.py — TINY_K (one super-block per row), GQA_K (grouped K/V heads: the rope/store's
nq != nk split; an odd count of super-blocks in F; three layers) and GQA_K in the *_K_M mix (wv, w2, output Q6_K, the rest Q4_K:
several type runs per activation row) — at context 64, with that file's bounds against the oracle: 4e-2 * std(logits) for TINY_K,
8e-2 for GQA_K (where it explains the factor two).  Against the K chunk plan, and chain against stepped loop, everything is
array_equal: every launch is column-local and column index and column count agree on both sides."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KTYPES = [10, 11, 12, 13, 14]  # q2_K q3_K q4_K q5_K q6_K
TINY_K = dict(n_vocab=256, n_embd=256, n_head=4, n_head_kv=4, n_layer=2, n_rot=64, n_ff=512, n_mult=32)
GQA_K = dict(n_vocab=512, n_embd=512, n_head=8, n_head_kv=2, n_layer=3, n_rot=64, n_ff=768, n_mult=32)
BOUND = {"tiny": 4e-2, "gqa": 8e-2}
CTX = 64
SENTINEL = 0x5555  # a finite f16 (85.3): rows past a column's position are loaded by the attention's first pass and must be ignored
MIX = "mix"        # GQA_K, wv / w2 / output Q6_K, the rest Q4_K
CHUNK_CASES = ([("tiny", t, B) for t in KTYPES for B in (3, 8)] +     # passes of 2 + 1 columns, and of 8
               [("gqa", t, B) for t in (12, 14, MIX) for B in (2, 7)])  # a pass of 2, and passes of 4 + 2 + 1
DEFAULT = dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30)

_weights = {}


def _stat(G, key):
    return int(G.lib().ggml_hip_get_stat(key.encode()))


def _weights_of(O, cfg, wtype):
    """(hp, w) built once per (shape, type) with the oracle's quantizer, as tests/test_kquant_plan_gpu.py's _model does; never modified."""
    if (cfg, wtype) not in _weights:
        from llm_amd import synth
        hp = dict(TINY_K if cfg == "tiny" else GQA_K)
        base, wtypes = wtype, None
        if wtype == MIX:
            base, wtypes = 12, {"output.weight": 14}
            for i in range(hp["n_layer"]):
                wtypes[f"layers.{i}.attention.wv.weight"] = 14
                wtypes[f"layers.{i}.feed_forward.w2.weight"] = 14
        rng = np.random.default_rng([base, 77, len(wtypes or {})])
        w = {}
        for name, (ne0, ne1) in synth.tensor_shapes(hp).items():
            if ne1 is None:
                w[name] = (1.0 + 0.01 * rng.standard_normal(ne0)).astype(np.float32)
            else:
                w[name] = O.quantize((wtypes or {}).get(name, base), (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32))
        hp["wtype"] = base
        if wtypes:
            hp["wtypes"] = dict(wtypes)
        _weights[(cfg, wtype)] = (hp, w)
    return _weights[(cfg, wtype)]


def _mk(O, cfg, wtype):
    from llm_amd import llama
    hp, w = _weights_of(O, cfg, wtype)
    return hp, w, llama.Llama(hp, w, context_size=CTX)


def _run_on(G, f):
    """f() with plan_batch_k = 1, restored to 0 whatever happens."""
    assert _stat(G, "batch_k_steps") >= 0
    try:
        G.set_option("plan_batch_k", 1)
        return f()
    finally:
        G.set_option("plan_batch_k", 0)


def _feed(sess, toks):
    for i in range(0, len(toks), 8):
        sess.evaluate(toks[i:i + 8], want_all_logits=False)


def _kv3(hp, k, v):
    """memory_k as [layer][position][channel], memory_v as [layer][channel][position]; with grouped K/V heads the layers' rows,
    n_embd_gqa wide, fill the front of the session's n_embd-wide allocation."""
    L, Egqa = hp["n_layer"], hp["n_embd"] // (hp["n_head"] // hp["n_head_kv"])
    n = L * CTX * Egqa
    return k[:n].reshape(L, CTX, Egqa), v[:n].reshape(L, Egqa, CTX)


def _free(*things):
    for t in things:
        for f in (t if isinstance(t, list) else [t]):
            f.free()


def _sessions(model, prompts):
    out = []
    for p in prompts:
        f = model.start_session(n_batch=8)
        if len(p):
            _feed(f, p)
        out.append(f)
    return out


def _twins(model, prompts):
    a, b = [], []
    for p in prompts:
        for lst in (a, b):
            f = model.start_session(n_batch=8)
            f.feed_prompt(p)
            lst.append(f)
    return a, b


def _same(chain, step):
    for c, (x, y) in enumerate(zip(chain, step)):
        assert x.n_past == y.n_past, c
        assert np.array_equal(x.last_logits(), y.last_logits()), c
        (kx, vx), (ky, vy) = x.get_kv(np.uint8), y.get_kv(np.uint8)
        assert np.array_equal(kx, ky) and np.array_equal(vx, vy), c


# ---- 1. bit for bit against the K chunk plan ----
@pytest.mark.parametrize("cfg,wtype,B", CHUNK_CASES)
def test_batched_step_equals_the_k_chunk_plan_bit_for_bit(G, O, cfg, wtype, B):
    """tests/test_batch_decode_gpu.py's test of the same name, for the K plan.  Two source sessions at 5 and 23 tokens each evaluate a
    chunk of B tokens on the K chunk plan (kplan_tokens grows by B; B <= 8 is below k_prompt_min).  Batch column c (s = c mod 2) is a
    fresh session holding S_s's post-chunk K/V with every position >= P_s + c overwritten by a sentinel, seeked to P_s + c, given
    chunk_s[c].  Logits of column c == the chunk's row c; cache row P_s + c == the source's; rows below unchanged; rows above still
    the sentinel."""
    def run():
        hp, w, model = _mk(O, cfg, wtype)
        rng = np.random.default_rng([B, 5, len(str(wtype))])
        P = (5, 23)
        ref, kv, chunk = [], [], []
        for s in (0, 1):
            src = model.start_session(n_batch=8)
            _feed(src, rng.integers(0, hp["n_vocab"], P[s]).astype(np.int32))
            chunk.append(rng.integers(0, hp["n_vocab"], B).astype(np.int32))
            k0 = _stat(G, "kplan_tokens")
            ref.append(src.evaluate(chunk[s]))
            assert _stat(G, "kplan_tokens") - k0 == B  # premise: the K chunk plan ran it
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
        keys = ("batch_k_steps", "batch_decode_steps", "batch_decode_tokens", "plan_tokens", "kplan_tokens")
        s0 = [_stat(G, k) for k in keys]
        ran, logits = model.evaluate_batch(sessions, toks)
        assert ran
        assert [_stat(G, k) - a for k, a in zip(keys, s0)] == [1, 1, B, B, B]
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
        _free(sessions, model)
    _run_on(G, run)


# ---- 2. ragged positions against the oracle ----
PASTS = (0, 1, 7, 33, 63)


def _full_context_is_refused(G, model, sessions, toks):
    assert sessions[-1].n_past == CTX
    keys = ("batch_k_steps", "batch_decode_steps", "plan_tokens", "kplan_tokens")
    n_before, s0 = [f.n_past for f in sessions], [_stat(G, k) for k in keys]
    with pytest.raises(ValueError):
        model.evaluate_batch(sessions, toks)
    assert [f.n_past for f in sessions] == n_before and [_stat(G, k) for k in keys] == s0


@pytest.mark.parametrize("cfg,wtype", [("tiny", t) for t in KTYPES] + [("gqa", 12), ("gqa", 14)])
def test_ragged_batch_matches_the_oracle(G, O, cfg, wtype):
    """Sessions at n_past = 0, 1, 7, 33 and 63 (the context's last slot) in one step; each column against O.Llama evaluating the same
    token on the session's own K/V.  Uniform types: the oracle's model takes one."""
    def run():
        hp, w, model = _mk(O, cfg, wtype)
        rng = np.random.default_rng([wtype, 2])
        sessions = _sessions(model, [rng.integers(0, hp["n_vocab"], n).astype(np.int32) for n in PASTS])
        orcs = []
        for n, f in zip(PASTS, sessions):
            o = O.Llama(hp, w, CTX)
            k, v = f.get_kv()
            o.memory_k[:] = k[:o.memory_k.size]
            o.memory_v[:] = v[:o.memory_v.size]
            o.n_past = n
            orcs.append(o)
        toks = rng.integers(0, hp["n_vocab"], len(PASTS)).astype(np.int32)
        s0 = _stat(G, "batch_k_steps")
        ran, logits = model.evaluate_batch(sessions, toks)
        assert ran and _stat(G, "batch_k_steps") - s0 == 1
        worst = 0.0
        for c, (f, o) in enumerate(zip(sessions, orcs)):
            ref = o.evaluate(toks[c:c + 1], mode=O.ref_mode())[0]
            d = float(np.max(np.abs(logits[c] - ref))) / float(ref.std())
            worst = max(worst, d)
            assert f.n_past == PASTS[c] + 1
        print(f"{cfg} type {wtype}: batched K step vs oracle worst |dlogit|/std = {worst:.2e}")
        assert worst <= BOUND[cfg], worst
        _full_context_is_refused(G, model, sessions, toks)
        _free(sessions, model)
    _run_on(G, run)


def test_ragged_batch_of_the_mixed_model_matches_the_sessions_alone(G, O):
    """The *_K_M mix has no oracle model: the same sessions evaluated alone (the single-token K plan: other kernels), same bound."""
    def run():
        hp, w, model = _mk(O, "gqa", MIX)
        rng = np.random.default_rng(29)
        prompts = [rng.integers(0, hp["n_vocab"], n).astype(np.int32) for n in PASTS]
        toks = rng.integers(0, hp["n_vocab"], len(PASTS)).astype(np.int32)
        alone = _sessions(model, prompts)
        want = [a.evaluate([t])[0] for a, t in zip(alone, toks)]
        sessions = _sessions(model, prompts)
        s0 = _stat(G, "batch_k_steps")
        ran, logits = model.evaluate_batch(sessions, toks)
        assert ran and _stat(G, "batch_k_steps") - s0 == 1
        worst = max(float(np.max(np.abs(logits[c] - want[c]))) / float(want[c].std()) for c in range(len(PASTS)))
        print(f"gqa mixed Q4_K/Q6_K: batched K step vs alone worst |dlogit|/std = {worst:.2e}")
        assert worst <= BOUND["gqa"], worst
        _full_context_is_refused(G, model, sessions, toks)
        _free(alone, sessions, model)
    _run_on(G, run)


# ---- 3. steps in a row ----
@pytest.mark.parametrize("cfg,wtype", [("tiny", 12), ("gqa", MIX)])
def test_steps_in_a_row_replay_one_graph_and_keep_the_sessions_books(G, O, cfg, wtype):
    """Six batched steps of four sessions against the same streams decoded alone; from the second step on one graph replay per step
    and no new plan; n_past and last_logits follow; rewind(1) + a single evaluate behaves as for a session decoded alone."""
    def run():
        hp, w, model = _mk(O, cfg, wtype)
        rng = np.random.default_rng([3, len(str(wtype))])
        prompts = [rng.integers(0, hp["n_vocab"], n).astype(np.int32) for n in (3, 9, 14, 20)]
        streams = rng.integers(0, hp["n_vocab"], (4, 6)).astype(np.int32)
        alone_logits = []
        for a, st in zip(_sessions(model, prompts), streams):
            for t in st:
                last = a.evaluate([t])[0]
            alone_logits.append(last)
            a.free()
        sessions = _sessions(model, prompts)
        s0 = _stat(G, "batch_k_steps")
        for step in range(6):
            r0, n0 = _stat(G, "graph_replays"), _stat(G, "plans")
            ran, logits = model.evaluate_batch(sessions, streams[:, step])
            assert ran
            if step >= 1:
                assert _stat(G, "graph_replays") - r0 == 1 and _stat(G, "plans") == n0, step
            for c, f in enumerate(sessions):
                assert f.n_past == len(prompts[c]) + step + 1
                assert np.array_equal(f.last_logits(), logits[c])
        assert _stat(G, "batch_k_steps") - s0 == 6
        for c, f in enumerate(sessions):
            d = float(np.max(np.abs(logits[c] - alone_logits[c]))) / float(alone_logits[c].std())
            print(f"{cfg} type {wtype} session {c}: batched-vs-alone {d:.2e}")
            assert d <= BOUND[cfg], (c, d)
        for c, f in enumerate(sessions):
            assert f.rewind(1) == 0 and f.n_past == len(prompts[c]) + 5
            again = f.evaluate([streams[c, 5]])[0]
            assert f.n_past == len(prompts[c]) + 6 and np.array_equal(f.last_logits(), again)
            d = float(np.max(np.abs(again - alone_logits[c]))) / float(alone_logits[c].std())
            assert d <= BOUND[cfg], (c, d)
        _free(sessions, model)
    _run_on(G, run)


# ---- 4. / 5. the chains ----
N = 5


@pytest.mark.parametrize("B", [2, 8])
@pytest.mark.parametrize("cfg,wtype", [("tiny", 12), ("gqa", MIX)])
def test_greedy_chain_equals_the_stepped_loop_bit_for_bit(G, O, cfg, wtype, B):
    """infer_tokens_batch(N) against twins taken through N infer_next_tokens_batch steps, both with the option on: the same graph on
    the same inputs, so ids, last_logits and K/V bytes are equal with no exclusions."""
    def run():
        hp, w, model = _mk(O, cfg, wtype)
        rng = np.random.default_rng([B, 31])
        chain, step = _twins(model, [rng.integers(0, hp["n_vocab"], 2 + 3 * c).astype(np.int32) for c in range(B)])
        keys = ("batch_chain_steps", "batch_chain_tokens", "batch_k_steps", "batch_decode_tokens", "plan_tokens", "kplan_tokens")
        s0 = [_stat(G, k) for k in keys]
        ran, ids = model.infer_tokens_batch(chain, N)
        assert ran is True and ids.shape == (N, B)
        assert [_stat(G, k) - a for k, a in zip(keys, s0)] == [N - 1, (N - 1) * B, N, N * B, N * B, N * B]
        rows = []
        for _ in range(N):
            r, row = model.infer_next_tokens_batch(step)
            assert r
            rows.append(row)
        assert np.array_equal(ids, np.stack(rows))
        _same(chain, step)
        _free(chain, step, model)
    _run_on(G, run)


@pytest.mark.parametrize("B", [2, 8])
@pytest.mark.parametrize("cfg,wtype", [("tiny", 12), ("gqa", MIX)])
def test_sampled_chain_equals_the_stepped_loop_bit_for_bit(G, O, cfg, wtype, B):
    """The same with infer_tokens_sampled_batch (the default sampler's shape, distinct seeds) against N steps of
    infer_next_tokens_sampled_batch: ids, generator states, last_logits and K/V bytes equal."""
    def run():
        hp, w, model = _mk(O, cfg, wtype)
        rng = np.random.default_rng([B, 37])
        chain, step = _twins(model, [rng.integers(0, hp["n_vocab"], 2 + 3 * c).astype(np.int32) for c in range(B)])
        rc = (np.arange(B, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567)).astype(np.uint64)
        rs = rc.copy()
        keys = ("batch_sample_steps", "batch_sample_tokens", "batch_chain_steps", "batch_k_steps", "plan_tokens")
        s0 = [_stat(G, k) for k in keys]
        ran, ids = model.infer_tokens_sampled_batch(chain, N, rc, **DEFAULT)
        assert ran is True and ids.shape == (N, B)
        assert [_stat(G, k) - a for k, a in zip(keys, s0)] == [N - 1, (N - 1) * B, 0, N, N * B]
        rows = []
        for _ in range(N):
            r, row = model.infer_next_tokens_sampled_batch(step, rs, **DEFAULT)
            assert r
            rows.append(row)
        assert np.array_equal(ids, np.stack(rows))
        assert np.array_equal(rc, rs) and len(set(rc.tolist())) == B
        _same(chain, step)
        _free(chain, step, model)
    _run_on(G, run)


# ---- 6. the switch ----
def test_the_switch(G, O):
    """plan_batch_k = 0 (the default): the Q4_K model is declined — ran False, batch_k_steps and batch_decode_steps do not move — as
    the pinned q4_k cases of the older files say; the same with plan_batch_k = 1 and plan_k = 0; with both on the same sessions take
    the batched step."""
    assert _stat(G, "batch_k_steps") >= 0
    assert G.get_option("plan_batch_k") == 0
    hp, w, model = _mk(O, "tiny", 12)
    rng = np.random.default_rng(4)
    sessions = _sessions(model, [rng.integers(0, hp["n_vocab"], 2 + 3 * i).astype(np.int32) for i in range(3)])
    toks = rng.integers(0, hp["n_vocab"], 3).astype(np.int32)
    keys = ("batch_k_steps", "batch_decode_steps")
    s0 = [_stat(G, k) for k in keys]
    ran, _ = model.evaluate_batch(sessions, toks)
    assert not ran and [_stat(G, k) for k in keys] == s0
    try:
        G.set_option("plan_batch_k", 1)
        assert G.get_option("plan_batch_k") == 1
        G.set_option("plan_k", 0)
        ran, _ = model.evaluate_batch(sessions, toks)
        assert not ran and [_stat(G, k) for k in keys] == s0
        G.set_option("plan_k", 1)
        ran, _ = model.evaluate_batch(sessions, toks)
        assert ran and [_stat(G, k) - a for k, a in zip(keys, s0)] == [1, 1]
        assert [f.n_past for f in sessions] == [2 + 3 * i + 3 for i in range(3)]
    finally:
        G.set_option("plan_k", 1)
        G.set_option("plan_batch_k", 0)
    _free(sessions, model)
