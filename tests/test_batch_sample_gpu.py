"""The sampled batched chain (ggml_hip_decode_batch_sampled / llm_infer_tokens_sampled_batch_device /
Llama.infer_tokens_sampled_batch): n tokens for each of B sessions of one model, every step one pass over the weights, the
sampler — repetition penalty over the last 64 tokens, top-k, top-p, temperature, a xorshift64* draw — and the next step's
parameters on the device (k_sample_next, one workgroup per column), the step's captured graph replayed.

The sampler is specified on IEEE basic operations only and written once for host and device (kernels/sampler_math.h), so every
comparison below is equality: the kernel alone against tests/sampler_ref.py (a numpy restatement of the specification), the chain
against the stepped loop (ids, generator states, and Session.snapshot() byte for byte).  Contexts are 64 unless said otherwise."""
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
MODELS = [("tiny", 2), ("tiny", 8), ("gqa2", 2), ("tiny", F16)]
COUNTERS = ("batch_sample_steps", "batch_sample_tokens", "batch_chain_steps", "batch_chain_tokens", "batch_decode_steps",
            "batch_decode_tokens", "plan_tokens")
DEFAULT = dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30)


def _stat(G, key):
    return int(G.lib().ggml_hip_get_stat(key.encode()))


def _stats(G):
    return [_stat(G, k) for k in COUNTERS]


def _mk(cfg, wtype, seed, ctx=CTX):
    from llm_amd import llama, synth
    hp, w = synth.make_llama(synth.TINY if cfg == "tiny" else GQA2, wtype, seed=seed)
    return hp, llama.Llama(hp, w, context_size=ctx)


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


def _seeds(B, salt=0):
    return (np.arange(B, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567 + salt)).astype(np.uint64)


def _stepped(model, sessions, n, rngs, **prm):
    rows, ran = [], []
    for _ in range(n):
        r, ids = model.infer_next_tokens_sampled_batch(sessions, rngs, **prm)
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


# ---- the kernel alone ----
# sampler_ref.ALONE, the cases tests/test_sample_chain_gpu.py runs on one row: both selections (on chip up to V = sampler_ref.CAP, over
# global memory beyond) in batched form, and B = 1 with a BatchCols
@pytest.mark.parametrize("B", [1, 2, 8])
@pytest.mark.parametrize("V,k,n_draws,top_p,temperature", R.ALONE)
def test_k_batch_sample_next_alone(G, V, k, n_draws, top_p, temperature, B):
    """k_sample_next on B columns.  Column c carries row family c mod 4 (sampler_ref.rows) and starts from a ring of 0 / 5 / 64 / 30
    tokens taken from inside and outside its raw top-k.  Ids, rings, counts, generator states, positions and DecParams equal the
    restatement's after n_draws launches; entries from B on are untouched."""
    from llm_amd import llama
    rows = R.rows(B, V, seed=3)
    pos_in = (np.arange(8, dtype=np.int32) * 7 + 3) % 40
    tokens_in = np.arange(32, dtype=np.int32) + 70000  # sentinels: no id of any vocabulary here
    hist = np.full((8, 64), 80000, np.int32)
    hist_n = np.full(8, 7, np.int32)
    rng = _seeds(8, salt=V)
    for c in range(B):
        w = R.window_for(rows[c], k, (0, 5, 64, 30)[c % 4], seed=c)
        hist[c, :w.size] = w
        hist_n[c] = w.size
    # the restatement, column by column
    want_hist, want_n, want_rng = hist.copy(), hist_n.copy(), [int(x) for x in rng]
    want_ids = np.zeros((n_draws, B), np.int32)
    for c in range(B):
        for d in range(n_draws):
            window = want_hist[c, :min(int(want_n[c]), 64)]
            tok, want_rng[c] = R.sample(rows[c], window, k, top_p, temperature, 1.30, want_rng[c])
            want_hist[c, want_n[c] % 64] = tok
            want_n[c] += 1
            want_ids[d, c] = tok
    prm_s = llama.SamplerParams(k, top_p, temperature, 1.30)
    ids = np.full((n_draws, B), -1, np.int32)
    prm, pos_out = np.full(34, -1, np.int32), np.full(8, -1, np.int32)
    import ctypes as C
    rc = G.lib().ggml_hip_debug_batch_sample(rows.ctypes.data, B, V, C.addressof(prm_s), pos_in.ctypes.data, tokens_in.ctypes.data,
                                             hist.ctypes.data, hist_n.ctypes.data, rng.ctypes.data, n_draws, ids.ctypes.data,
                                             prm.ctypes.data, pos_out.ctypes.data)
    assert rc == 0
    assert np.array_equal(ids, want_ids), (ids, want_ids)
    assert [int(x) for x in rng] == want_rng  # (entries from B on: as they came)
    assert np.array_equal(hist, want_hist) and np.array_equal(hist_n, want_n)
    assert pos_out[:B].tolist() == (pos_in[:B] + n_draws).tolist()
    assert pos_out[B:].tolist() == pos_in[B:].tolist()
    last = want_ids[-1].tolist()
    assert prm.tolist() == [int(pos_in[0]) + n_draws, last[0]] + last + tokens_in[B:].tolist()


def test_the_hook_refuses_what_the_chain_declines(G):
    import ctypes as C
    from llm_amd import llama
    rows = R.rows(2, 300)
    z8, z32 = np.zeros(8, np.int32), np.zeros(32, np.int32)
    hist, rng, ids = np.zeros((8, 64), np.int32), _seeds(8), np.zeros((1, 2), np.int32)
    prm, pos = np.zeros(34, np.int32), np.zeros(8, np.int32)
    for k, top_p, t, pen in ((0, .9, .8, 1.3), (257, .9, .8, 1.3), (301, .9, .8, 1.3), (4, 0., .8, 1.3), (4, .9, 0., 1.3), (4, .9, .8, 0.)):
        s = llama.SamplerParams(k, top_p, t, pen)
        assert G.lib().ggml_hip_debug_batch_sample(rows.ctypes.data, 2, 300, C.addressof(s), z8.ctypes.data, z32.ctypes.data,
                                                   hist.ctypes.data, z8.ctypes.data, rng.ctypes.data, 1, ids.ctypes.data,
                                                   prm.ctypes.data, pos.ctypes.data) == -1


# ---- the chain against the stepped loop ----
@pytest.mark.parametrize("B", [2, 5, 8])
@pytest.mark.parametrize("cfg,wtype", MODELS)
def test_chain_equals_the_stepped_loop_bit_for_bit(G, O, cfg, wtype, B):
    """Twin sets of sessions with ragged prompts: one takes one infer_tokens_sampled_batch(N), the other N
    infer_next_tokens_sampled_batch, twice over.  Ids and generator states equal, snapshots byte-identical, the counters move as
    documented; the second chain builds no plan and replays the step's graph N times (so does the stepped loop)."""
    hp, model = _mk(cfg, wtype, seed=31)
    rng = np.random.default_rng([wtype, B])
    prompts = [rng.integers(0, hp["n_vocab"], 2 + 3 * c).astype(np.int32) for c in range(B)]
    chain, step = _twins(model, prompts)
    rc, rs = _seeds(B), _seeds(B)
    for rnd in range(2):
        s0, p0, r0 = _stats(G), _stat(G, "plans"), _stat(G, "graph_replays")
        ran, ids = model.infer_tokens_sampled_batch(chain, N, rc, **DEFAULT)
        assert ran is True and ids.shape == (N, B)
        d = [b - a for a, b in zip(s0, _stats(G))]
        assert d == [N - 1, (N - 1) * B, 0, 0, N, N * B, N * B], (rnd, d)
        if rnd == 1:
            assert _stat(G, "plans") == p0 and _stat(G, "graph_replays") - r0 == N
        s0, r0 = _stats(G), _stat(G, "graph_replays")
        ran_s, ids_s = _stepped(model, step, N, rs, **DEFAULT)
        d = [b - a for a, b in zip(s0, _stats(G))]
        assert all(ran_s) and d == [0, 0, 0, 0, N, N * B, N * B], (rnd, d)
        if rnd == 1:
            assert _stat(G, "plans") == p0 and _stat(G, "graph_replays") - r0 == N
        assert np.array_equal(ids, ids_s), (rnd, ids, ids_s)
        assert np.array_equal(rc, rs) and not np.array_equal(rc, _seeds(B))
        _same(chain, step)
        for c, f in enumerate(chain):
            assert f.n_past == len(prompts[c]) + (rnd + 1) * N
    _free(chain, step, model)


def test_every_window_passes_64_entries_inside_the_chain(G, O):
    """Context 128, prompts of 40 tokens, N = 40: each column's history grows from 40 to 80 tokens inside one chain, so the ring
    fills and wraps on the device."""
    n = 40
    hp, model = _mk("tiny", 2, seed=35, ctx=128)
    rng = np.random.default_rng(40)
    prompts = [rng.integers(0, hp["n_vocab"], 40).astype(np.int32) for _ in range(3)]
    chain, step = _twins(model, prompts)
    rc, rs = _seeds(3, 1), _seeds(3, 1)
    ran, ids = model.infer_tokens_sampled_batch(chain, n, rc, **DEFAULT)
    assert ran is True
    ran_s, ids_s = _stepped(model, step, n, rs, **DEFAULT)
    assert all(ran_s) and np.array_equal(ids, ids_s), (ids, ids_s)
    assert np.array_equal(rc, rs)
    _same(chain, step)
    _free(chain, step, model)


def test_k_1_without_a_penalty_is_the_greedy_chain(G, O):
    """k = 1, penalty = 1: the only candidate is the first maximum — ids and snapshots equal infer_tokens_batch's on twins (a
    kernel and a host path this chain shares nothing with but the step)."""
    hp, model = _mk("tiny", 7, seed=36)
    rng = np.random.default_rng(8)
    prompts = [rng.integers(0, hp["n_vocab"], n).astype(np.int32) for n in (3, 9, 14, 20)]
    sampled, greedy = _twins(model, prompts)
    rngs = _seeds(4)
    ran, ids = model.infer_tokens_sampled_batch(sampled, N, rngs, k=1, top_p=0.95, temperature=0.8, penalty=1.0)
    ran_g, ids_g = model.infer_tokens_batch(greedy, N)
    assert ran is True and ran_g is True and np.array_equal(ids, ids_g)
    _same(sampled, greedy)
    _free(sampled, greedy, model)


# ---- what the backend declines ----
@pytest.mark.parametrize("case", ["plan_batch_sample_0", "q4_k", "f32_kv", "nine", "k_300"])
def test_what_the_backend_declines_runs_as_the_stepped_loop(G, O, case):
    """Option plan_batch_sample = 0, a K-quant model, f32 K/V, nine sessions, k = 300: ran_chained is False, no sampled step is
    counted, and ids, generator states and snapshots equal those of twins stepped under the same conditions.  With the option back
    on the same sessions chain."""
    from llm_amd import llama, synth
    B = 9 if case == "nine" else 3
    kv_type = G.TYPE_F32 if case == "f32_kv" else G.TYPE_F16
    prm = dict(DEFAULT, k=300) if case == "k_300" else DEFAULT
    if case == "q4_k":
        hp0 = dict(n_vocab=256, n_embd=256, n_head=4, n_head_kv=4, n_layer=2, n_rot=64, n_ff=512, n_mult=32)
        rng = np.random.default_rng(12)
        hp, w = dict(hp0), {}
        for name, (ne0, ne1) in synth.tensor_shapes(hp).items():
            w[name] = ((1.0 + 0.01 * rng.standard_normal(ne0)).astype(np.float32) if ne1 is None else
                       O.quantize(G.TYPE_Q4_K, (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32)))
        hp["wtype"] = G.TYPE_Q4_K
    else:
        hp, w = synth.make_llama(GQA2 if case == "k_300" else synth.TINY, 2, seed=3)
    model = llama.Llama(hp, w, context_size=CTX)
    rng = np.random.default_rng(4)
    prompts = [rng.integers(0, hp["n_vocab"], 2 + 3 * i).astype(np.int32) for i in range(B)]
    chain, step = _twins(model, prompts, kv_type=kv_type)
    rc, rs = _seeds(B, 2), _seeds(B, 2)
    option = case[:-2] if case.endswith("_0") else None
    if option:
        G.set_option(option, 0)
    try:
        s0 = _stats(G)
        ran, ids = model.infer_tokens_sampled_batch(chain, N, rc, **prm)
        assert ran is False and _stats(G)[:4] == s0[:4]
        ran_s, ids_s = _stepped(model, step, N, rs, **prm)
    finally:
        if option:
            G.set_option(option, 1)
    assert np.array_equal(ids, ids_s) and np.array_equal(rc, rs)
    _same(chain, step)
    if option:
        s0 = _stats(G)
        ran, ids = model.infer_tokens_sampled_batch(chain, N, rc, **prm)
        assert ran is True and _stats(G)[0] - s0[0] == N - 1
        ran_s, ids_s = _stepped(model, step, N, rs, **prm)
        assert all(ran_s) and np.array_equal(ids, ids_s) and np.array_equal(rc, rs)
        _same(chain, step)
    _free(chain, step, model)


def test_bad_arguments_evaluate_nothing(G, O):
    """k = 0, k > V, temperature 0, top_p 0, a session listed twice, n < 1, a column without room for n tokens: ValueError, no
    n_past, no generator state and no counter moves."""
    hp, model = _mk("tiny", 2, seed=3)
    a, b = model.start_session(), model.start_session()
    a.evaluate([1, 2, 3], want_all_logits=False)
    b.feed_prompt(np.arange(1, CTX - 2, dtype=np.int32))  # b stands at CTX - 3: three tokens fit, four do not
    s0 = _stats(G)
    rngs = _seeds(2)
    r3 = _seeds(3)
    V = hp["n_vocab"]
    bad = [([a, b], 3, rngs, dict(DEFAULT, k=0)), ([a, b], 3, rngs, dict(DEFAULT, k=V + 1)), ([a, b], 3, rngs, dict(DEFAULT, temperature=0.0)),
           ([a, b], 3, rngs, dict(DEFAULT, top_p=0.0)), ([a, b, a], 3, r3, DEFAULT), ([a, b], 0, rngs, DEFAULT), ([a, b], -2, rngs, DEFAULT),
           ([a, b], 4, rngs, DEFAULT)]
    for sessions, n, r, prm in bad:
        with pytest.raises(ValueError):
            model.infer_tokens_sampled_batch(sessions, n, r, **prm)
        if n == 3:  # (the stepped form refuses the same sessions and parameters)
            with pytest.raises(ValueError):
                model.infer_next_tokens_sampled_batch(sessions, r, **prm)
    assert [f.n_past for f in (a, b)] == [3, CTX - 3] and _stats(G) == s0
    assert np.array_equal(rngs, _seeds(2)) and np.array_equal(r3, _seeds(3))
    ran, ids = model.infer_tokens_sampled_batch([a, b], 3, rngs, **DEFAULT)
    assert ran is True and a.n_past == 6 and b.n_past == CTX
    _free([a, b], model)


def test_after_a_sampled_chain_the_sessions_go_on_as_usual(G, O):
    """A greedy chain and a plain batched step of the same sessions run and build no plan; a sampled chain of one step equals one
    stepped call."""
    hp, model = _mk("tiny", 2, seed=37)
    rng = np.random.default_rng(9)
    prompts = [rng.integers(0, hp["n_vocab"], n).astype(np.int32) for n in (3, 9, 14)]
    chain, step = _twins(model, prompts)
    rc, rs = _seeds(3, 3), _seeds(3, 3)
    ran, ids = model.infer_tokens_sampled_batch(chain, N, rc, **DEFAULT)
    ran_s, ids_s = _stepped(model, step, N, rs, **DEFAULT)
    assert ran is True and np.array_equal(ids, ids_s)
    p0, s0 = _stat(G, "plans"), _stats(G)
    ran, ids = model.infer_tokens_batch(chain, 3)
    assert ran is True and _stat(G, "plans") == p0
    wants = [int(np.argmax(f.last_logits())) for f in chain]
    ran, step_ids = model.infer_next_tokens_batch(chain)
    assert ran and list(step_ids) == wants and _stat(G, "plans") == p0
    assert [b - a for a, b in zip(s0, _stats(G))] == [0, 0, 2, 6, 4, 12, 12]
    ran_s, ids_s = model.infer_tokens_batch(step, 3)
    ran_s, _ = model.infer_next_tokens_batch(step)
    _same(chain, step)
    s0 = _stats(G)
    ran, ids = model.infer_tokens_sampled_batch(chain, 1, rc, **DEFAULT)
    assert ran is True and [b - a for a, b in zip(s0, _stats(G))] == [0, 0, 0, 0, 1, 3, 3]
    ran_s, ids_s = model.infer_next_tokens_sampled_batch(step, rs, **DEFAULT)
    assert ran_s and np.array_equal(ids, ids_s[None, :]) and np.array_equal(rc, rs)
    _same(chain, step)
    _free(chain, step, model)
