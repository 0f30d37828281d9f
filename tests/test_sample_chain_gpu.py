"""The sampled chain of ONE session (ggml_hip_decode_sampled_chain / llm_infer_tokens_sampled_device /
Session.infer_tokens_sampled_device): n tokens drawn on the device by the default sampler chain — repetition penalty over the last
64 tokens, top-k, top-p, temperature, a xorshift64* draw — with k_sample_next between two replays of the session's single-token
plan, for block-format, F16 and K-quant models.

The sampler is specified on IEEE basic operations only and written once for host and device (kernels/sampler_math.h), so every
comparison below is equality: the kernel alone against tests/sampler_ref.py (a numpy restatement of the specification), the chain
against the stepped loop (ids, generator state, and Session.snapshot() byte for byte).  Contexts are 64 unless said otherwise."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GQA2 = dict(n_vocab=512, n_embd=1024, n_head=8, n_head_kv=4, n_layer=2, n_rot=128, n_ff=2816, n_mult=32)
CTX = 64
N = 6
F16 = 1  # ggml's type number of F16 weights
COUNTERS = ("sample_chain_steps", "sample_chain_tokens", "batch_sample_steps", "batch_sample_tokens", "batch_chain_steps",
            "batch_chain_tokens", "batch_decode_steps", "batch_decode_tokens", "tail_tokens", "plan_tokens")
DEFAULT = dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30)


def _stat(G, key):
    return int(G.lib().ggml_hip_get_stat(key.encode()))


def _stats(G):
    return [_stat(G, k) for k in COUNTERS]


def _moved(G, s0):
    return [b - a for a, b in zip(s0, _stats(G))]


def _seed(salt=0):
    return np.array([0x9E3779B97F4A7C15 + 0x1234567 * (salt + 1)], dtype=np.uint64)


def _q4_k(G, O):
    """the small Q4_K model of the batched test's decline case"""
    from llm_amd import synth
    hp = dict(n_vocab=256, n_embd=256, n_head=4, n_head_kv=4, n_layer=2, n_rot=64, n_ff=512, n_mult=32)
    rng = np.random.default_rng(12)
    w = {}
    for name, (ne0, ne1) in synth.tensor_shapes(hp).items():
        w[name] = ((1.0 + 0.01 * rng.standard_normal(ne0)).astype(np.float32) if ne1 is None else
                   O.quantize(G.TYPE_Q4_K, (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32)))
    hp["wtype"] = G.TYPE_Q4_K
    return hp, w


def _mk(G, O, cfg, wtype, seed, ctx=CTX):
    from llm_amd import llama, synth
    if cfg == "q4_k":
        hp, w = _q4_k(G, O)
    else:
        hp, w = synth.make_llama(synth.TINY if cfg == "tiny" else GQA2, wtype, seed=seed)
    return hp, llama.Llama(hp, w, context_size=ctx)


def _twins(model, prompt, **kw):
    """Two sessions fed the same prompt: the same state, bit for bit."""
    a, b = (model.start_session(n_batch=8, **kw) for _ in range(2))
    for f in (a, b):
        f.feed_prompt(prompt)
    assert a.snapshot() == b.snapshot()
    return a, b


def _stepped(s, n, rng, **prm):
    return np.array([s.infer_next_token_sampled(rng, **prm) for _ in range(n)], np.int32)


def _same(x, y):
    assert x.n_past == y.n_past
    assert x.snapshot() == y.snapshot()


def _free(*things):
    for t in things:
        t.free()


# ---- the kernel alone ----
# sampler_ref.ALONE: the cases tests/test_batch_sample_gpu.py runs on B columns (CAP = sampler_ref.CAP, the last row of the on-chip selection)
_rows = {}


def _family_rows(V):
    if V not in _rows:
        _rows[V] = R.rows(4, V, seed=3)
        _rows[V].setflags(write=False)
    return _rows[V]


def _hook(G, row, V, prm_s, n_past_in, tokens_in, hist, hist_n, rng, n_draws, ids, prm):
    return G.lib().ggml_hip_debug_sample_next(row.ctypes.data, V, C.addressof(prm_s), n_past_in, tokens_in.ctypes.data, hist.ctypes.data,
                                              hist_n.ctypes.data, rng.ctypes.data, n_draws, ids.ctypes.data, prm.ctypes.data)


@pytest.mark.parametrize("f", [0, 1, 2, 3])
@pytest.mark.parametrize("V,k,n_draws,top_p,temperature", R.ALONE)
def test_k_sample_next_alone(G, V, k, n_draws, top_p, temperature, f):
    """Row family f (sampler_ref.rows: ties between neighbours and -inf; equal maxima first and last; zeros of both signs with the
    maximum last; all equal — at V = CAP the row on which every pass over the value bits keeps every key) from a ring of
    0 / 5 / 64 / 30 tokens taken from inside and outside its raw top-k.  Ids, ring, count, generator state and DecParams equal the
    restatement's after n_draws launches; tokens[1 .. 31] keep their sentinels."""
    from llm_amd import llama
    row = np.ascontiguousarray(_family_rows(V)[f])
    n_past_in = 17
    tokens_in = np.arange(32, dtype=np.int32) + 70000  # sentinels: no id of any vocabulary here
    hist = np.full(64, 80000, np.int32)
    w = R.window_for(row, k, (0, 5, 64, 30)[f], seed=f)
    hist[:w.size] = w
    hist_n = np.array([w.size], np.int32)
    rng = _seed(V + f)
    want_hist, want_n, want_rng, want_ids = hist.copy(), int(hist_n[0]), int(rng[0]), []
    for _ in range(n_draws):
        tok, want_rng = R.sample(row, want_hist[:min(want_n, 64)], k, top_p, temperature, 1.30, want_rng)
        want_hist[want_n % 64] = tok
        want_n += 1
        want_ids.append(tok)
    ids, prm = np.full(n_draws, -1, np.int32), np.full(34, -1, np.int32)
    rc = _hook(G, row, V, llama.SamplerParams(k, top_p, temperature, 1.30), n_past_in, tokens_in, hist, hist_n, rng, n_draws, ids, prm)
    assert rc == 0
    assert ids.tolist() == want_ids, (ids, want_ids)
    assert int(rng[0]) == want_rng
    assert np.array_equal(hist, want_hist) and int(hist_n[0]) == want_n
    assert prm.tolist() == [n_past_in + n_draws, want_ids[-1], want_ids[-1]] + tokens_in[1:].tolist()


def test_the_hook_refuses_what_the_chain_declines(G):
    from llm_amd import llama
    row = np.ascontiguousarray(R.rows(1, 300)[0])
    z32, hist, hist_n = np.zeros(32, np.int32), np.zeros(64, np.int32), np.zeros(1, np.int32)
    rng, ids, prm = _seed(), np.zeros(1, np.int32), np.zeros(34, np.int32)
    for k, top_p, t, pen in ((0, .9, .8, 1.3), (257, .9, .8, 1.3), (301, .9, .8, 1.3), (4, 0., .8, 1.3), (4, .9, 0., 1.3), (4, .9, .8, 0.)):
        assert _hook(G, row, 300, llama.SamplerParams(k, top_p, t, pen), 0, z32, hist, hist_n, rng, 1, ids, prm) == -1
    assert int(rng[0]) == int(_seed()[0])


# ---- the chain against the stepped loop ----
@pytest.mark.parametrize("cfg,wtype", [("tiny", 2), ("tiny", 8), ("gqa2", 2), ("tiny", F16), ("q4_k", None)])
def test_chain_equals_the_stepped_loop_bit_for_bit(G, O, cfg, wtype):
    """Twin sessions: one takes infer_tokens_sampled_device(N), the other N infer_next_token_sampled, twice over — the first chain
    behind feed_prompt (one stepped token arms it: N - 1 drawn on the device), the second behind a stepped token (all N).  Ids and
    generator state equal, snapshots byte-identical; the second round builds no plan; sample_chain_* move by the device-drawn count,
    plan_tokens by every token, the batched counters and the token tail's not at all.  The K-quant model is the one no batched
    entry takes."""
    hp, model = _mk(G, O, cfg, wtype, seed=31)
    prompt = np.random.default_rng([5, wtype or 0]).integers(0, hp["n_vocab"], 11).astype(np.int32)
    chain, step = _twins(model, prompt)
    rc, rs = _seed(1), _seed(1)
    for rnd in range(2):
        # (the chain continues the slot's most recent evaluation: each twin takes its stepped token and its n tokens in one go)
        s0, p0 = _stats(G), _stat(G, "plans")
        first = [chain.infer_next_token_sampled(rc, **DEFAULT)] if rnd == 1 else []
        on_dev, ids = chain.infer_tokens_sampled_device(N, rc, **DEFAULT)
        assert on_dev == (N - 1, N)[rnd] and ids.shape == (N,)
        assert _moved(G, s0) == [on_dev, on_dev, 0, 0, 0, 0, 0, 0, 0, N + rnd], (rnd, _moved(G, s0))
        if rnd == 1:
            assert _stat(G, "plans") == p0
        s0 = _stats(G)
        first_s = [step.infer_next_token_sampled(rs, **DEFAULT)] if rnd == 1 else []
        ids_s = _stepped(step, N, rs, **DEFAULT)
        assert _moved(G, s0) == [0, 0, 0, 0, 0, 0, 0, 0, 0, N + rnd], (rnd, _moved(G, s0))
        if rnd == 1:
            assert _stat(G, "plans") == p0
        assert first == first_s
        assert np.array_equal(ids, ids_s), (rnd, ids, ids_s)
        assert np.array_equal(rc, rs) and not np.array_equal(rc, _seed(1))
        _same(chain, step)
        assert chain.n_past == len(prompt) + (rnd + 1) * N + rnd
    _free(chain, step, model)


def test_the_window_passes_64_entries_inside_the_chain(G, O):
    """Context 128, a prompt of 40 tokens, n = 40: the history grows from 40 to 80 tokens inside one chain, so the ring fills and
    wraps on the device."""
    n = 40
    hp, model = _mk(G, O, "tiny", 2, seed=35, ctx=128)
    prompt = np.random.default_rng(40).integers(0, hp["n_vocab"], 40).astype(np.int32)
    chain, step = _twins(model, prompt)
    rc, rs = _seed(2), _seed(2)
    on_dev, ids = chain.infer_tokens_sampled_device(n, rc, **DEFAULT)
    assert on_dev == n - 1
    ids_s = _stepped(step, n, rs, **DEFAULT)
    assert np.array_equal(ids, ids_s), (ids, ids_s)
    assert np.array_equal(rc, rs)
    _same(chain, step)
    _free(chain, step, model)


def test_k_1_without_a_penalty_is_the_greedy_chain(G, O):
    """k = 1, penalty = 1: the only candidate is the first maximum — ids and snapshots equal infer_tokens_device's on a twin (a
    kernel this chain shares nothing with but the replays)."""
    hp, model = _mk(G, O, "tiny", 7, seed=36)
    prompt = np.random.default_rng(8).integers(0, hp["n_vocab"], 11).astype(np.int32)
    sampled, greedy = _twins(model, prompt)
    on_dev, ids = sampled.infer_tokens_sampled_device(N, _seed(3), k=1, top_p=0.95, temperature=0.8, penalty=1.0)
    ids_g = greedy.infer_tokens_device(N)
    assert on_dev == N - 1 and np.array_equal(ids, ids_g)
    _same(sampled, greedy)
    _free(sampled, greedy, model)


def test_behind_the_run_ahead(G, O):
    """Twins take three greedy infer_next_token steps: the device is one token ahead of each and its parameters have moved on.  One
    takes the chain, the other the stepped loop: equal ids and snapshots — the ahead run's K/V rows were taken back, the
    parameters put back."""
    hp, model = _mk(G, O, "tiny", 2, seed=37)
    prompt = np.random.default_rng(9).integers(0, hp["n_vocab"], 9).astype(np.int32)
    chain, step = _twins(model, prompt)
    rc, rs = _seed(4), _seed(4)
    t0 = _stat(G, "tail_tokens")
    g_chain = [chain.infer_next_token() for _ in range(3)]
    assert _stat(G, "tail_tokens") - t0 == 3  # (every one of them ended in the token tail and started the next token's graph)
    on_dev, ids = chain.infer_tokens_sampled_device(N, rc, **DEFAULT)  # ... which is in flight, or done, when the chain begins
    assert on_dev == N
    g_step = [step.infer_next_token() for _ in range(3)]
    ids_s = _stepped(step, N, rs, **DEFAULT)
    assert g_chain == g_step
    assert np.array_equal(ids, ids_s) and np.array_equal(rc, rs)
    _same(chain, step)
    _free(chain, step, model)


def test_a_chain_across_a_change_of_attention_variant(G, O):
    """Option attn_split = 30 moves the change from one attention workgroup per head to the position-split attention to 30
    positions: a prompt of 24 tokens and n = 12 cross it inside the chain, which picks the variant per step on the host as an
    evaluation does."""
    n = 12
    hp, model = _mk(G, O, "tiny", 2, seed=38)
    prompt = np.random.default_rng(10).integers(0, hp["n_vocab"], 24).astype(np.int32)
    try:
        G.set_option("attn_split", 30)
        chain, step = _twins(model, prompt)
        rc, rs = _seed(5), _seed(5)
        on_dev, ids = chain.infer_tokens_sampled_device(n, rc, **DEFAULT)
        assert on_dev == n - 1
        b0 = _stat(G, "attn_split_tokens")
        ids_s = _stepped(step, n, rs, **DEFAULT)
        assert 0 < _stat(G, "attn_split_tokens") - b0 < n  # (the stepped twin's books: some tokens on either side)
        assert np.array_equal(ids, ids_s) and np.array_equal(rc, rs)
        _same(chain, step)
    finally:
        G.set_option("attn_split", 1)
    _free(chain, step, model)


# ---- what the backend declines ----
@pytest.mark.parametrize("case", ["plan_sample_chain_0", "f32_kv", "k_300"])
def test_what_the_backend_declines_runs_as_the_stepped_loop(G, O, case):
    """Option plan_sample_chain = 0, f32 K/V, k = 300: nothing is drawn on the device, no sample_chain_* moves, and ids, generator
    state and snapshot equal those of a twin stepped under the same conditions.  With the option back on the same session chains."""
    kv_type = G.TYPE_F32 if case == "f32_kv" else G.TYPE_F16
    prm = dict(DEFAULT, k=300) if case == "k_300" else DEFAULT
    hp, model = _mk(G, O, "gqa2" if case == "k_300" else "tiny", 2, seed=3)
    prompt = np.random.default_rng(4).integers(0, hp["n_vocab"], 8).astype(np.int32)
    chain, step = _twins(model, prompt, kv_type=kv_type)
    rc, rs = _seed(6), _seed(6)
    option = case[:-2] if case.endswith("_0") else None
    if option:
        G.set_option(option, 0)
    try:
        s0 = _stats(G)
        on_dev, ids = chain.infer_tokens_sampled_device(N, rc, **prm)
        assert on_dev == 0 and _moved(G, s0)[:2] == [0, 0]
        ids_s = _stepped(step, N, rs, **prm)
    finally:
        if option:
            G.set_option(option, 1)
    assert np.array_equal(ids, ids_s) and np.array_equal(rc, rs)
    _same(chain, step)
    if option:
        s0 = _stats(G)
        on_dev, ids = chain.infer_tokens_sampled_device(N, rc, **prm)
        assert on_dev == N - 1 and _moved(G, s0)[:2] == [N - 1, N - 1]  # (the slot's last evaluation was the twin's: one stepped token first)
        ids_s = _stepped(step, N, rs, **prm)
        assert np.array_equal(ids, ids_s) and np.array_equal(rc, rs)
        _same(chain, step)
    _free(chain, step, model)


def test_bad_arguments_move_nothing(G, O):
    """k = 0, k > V, temperature 0, top_p 0, n < 1, n beyond the context: ValueError; n_past, the generator state and the counters
    stand.  The stepped form refuses the same parameters."""
    hp, model = _mk(G, O, "tiny", 2, seed=3)
    a = model.start_session(n_batch=8)
    a.feed_prompt(np.arange(1, CTX - 2, dtype=np.int32) % hp["n_vocab"])  # a stands at CTX - 3: two tokens fit, three do not
    a.infer_next_token_sampled(_seed(9), **DEFAULT)
    at = a.n_past
    assert at == CTX - 2
    s0, rng, V = _stats(G), _seed(7), hp["n_vocab"]
    bad = [(1, dict(DEFAULT, k=0)), (1, dict(DEFAULT, k=V + 1)), (1, dict(DEFAULT, temperature=0.0)), (1, dict(DEFAULT, top_p=0.0)),
           (0, DEFAULT), (-2, DEFAULT), (2, DEFAULT)]
    for n, prm in bad:
        with pytest.raises(ValueError):
            a.infer_tokens_sampled_device(n, rng, **prm)
        if prm is not DEFAULT:
            with pytest.raises(ValueError):
                a.infer_next_token_sampled(rng, **prm)
    assert a.n_past == at and _stats(G) == s0 and np.array_equal(rng, _seed(7))
    on_dev, ids = a.infer_tokens_sampled_device(1, rng, **DEFAULT)
    assert on_dev == 1 and a.n_past == CTX - 1
    _free(a, model)
