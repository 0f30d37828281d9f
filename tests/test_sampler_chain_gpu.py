"""The whole sampler on the device (ggml_hip_decode_sampled_chain_ex / ggml_hip_decode_batch_sampled_ex and the Python entries'
new keywords): flat bias, frequency / presence penalty, tail-free, locally typical, min-p and Mirostat 2 in k_sample_next, between two
replays of the token graph, for one session and for 2 .. 8.

The sampler is specified on IEEE basic operations only and written once for host and device (kernels/sampler_math.h), so every
comparison below is equality: the kernel alone, through the hook, against tests/sampler_chain_ref.py (a numpy restatement of the
specification), the chains against the stepped loop (ids, generator states, the bits of mu, Session.snapshot() byte for byte)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_chain_ref as X  # noqa: E402
import sampler_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = R.CAP
CTX = 64
COUNTERS = ("sample_chain_steps", "sample_chain_tokens", "batch_sample_steps", "batch_sample_tokens", "batch_chain_steps",
            "batch_chain_tokens", "batch_decode_steps", "batch_decode_tokens", "tail_tokens", "plan_tokens")
TRUNC = dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30, freq=0.3, presence=0.2, tail_free_z=0.9, typical_p=0.5, min_p=0.2)
MIRO = dict(k=40, top_p=1.0, temperature=0.8, penalty=1.30, freq=0.1, presence=0.1, mirostat=2, tau=3.0, eta=0.25)


def _stats(G):
    return [int(G.lib().ggml_hip_get_stat(k.encode())) for k in COUNTERS]


def _lib_chain(ch):
    from llm_amd import llama
    return llama.sampler_chain(k=ch["k"], top_p=ch["top_p"], temperature=ch["temperature"], penalty=ch["penalty"], freq=ch["freq"],
                               presence=ch["presence"], tail_free_z=ch["z"], typical_p=ch["typical"], min_p=ch["min_p"], bias=ch["bias"],
                               mirostat=ch["mirostat"], tau=ch["tau"], eta=ch["eta"])


_rows = {}


def _family_rows(V):
    if V not in _rows:
        _rows[V] = R.rows(4, V, seed=5)
        _rows[V].setflags(write=False)
    return _rows[V]


def _alone(G, rows, ch, windows, n_draws, cols):
    """k_sample_next through the hook on the rows [B][V] from the given windows, against the restatement: ids, rings, counts,
    generator states, mu's bits, DecParams (and, with a BatchCols, the positions); entries behind column B keep their sentinels.
    cols = False: one session without a BatchCols (B = 1)."""
    B, V = rows.shape
    T = 8 if cols else 1
    n_past_in = 17
    pos_in = (np.arange(8, dtype=np.int32) * 7 + 3) % 40
    tokens_in = np.arange(32, dtype=np.int32) + 70000  # sentinels: no id of any vocabulary here
    hist = np.full((T, 64), 80000, np.int32)
    hist_n = np.full(T, 7, np.int32)
    rng = (np.arange(T, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567 + V)).astype(np.uint64)
    mu = (np.arange(T, dtype=np.float32) * np.float32(0.5) + np.float32(2 * ch["tau"])).astype(np.float32)
    for c in range(B):
        w = np.asarray(windows[c], np.int32)
        hist[c, :w.size] = w
        hist_n[c] = w.size
    want_hist, want_n, want_rng, want_mu = hist.copy(), hist_n.copy(), [int(x) for x in rng], mu.copy()
    want_ids = np.zeros((n_draws, B), np.int32)
    for c in range(B):
        for d in range(n_draws):
            window = want_hist[c, :min(int(want_n[c]), 64)]
            tok, want_rng[c], want_mu[c] = X.sample(rows[c], window, ch, want_rng[c], want_mu[c])
            want_hist[c, want_n[c] % 64] = tok
            want_n[c] += 1
            want_ids[d, c] = tok
    lc = _lib_chain(ch)
    ids = np.full((n_draws, B), -1, np.int32)
    prm, pos_out = np.full(34, -1, np.int32), np.full(8, -1, np.int32)
    rows = np.ascontiguousarray(rows)
    rc = G.lib().ggml_hip_debug_next_token_ex(rows.ctypes.data, B, V, C.addressof(lc), n_past_in, pos_in.ctypes.data if cols else None,
                                              tokens_in.ctypes.data, hist.ctypes.data, hist_n.ctypes.data, rng.ctypes.data, mu.ctypes.data,
                                              n_draws, ids.ctypes.data, prm.ctypes.data, pos_out.ctypes.data if cols else None)
    assert rc == 0
    assert np.array_equal(ids, want_ids), (ids, want_ids)
    assert [int(x) for x in rng] == want_rng  # (entries from B on: as they came)
    assert np.array_equal(mu.view(np.uint32), want_mu.view(np.uint32)), (mu, want_mu)
    assert np.array_equal(hist, want_hist) and np.array_equal(hist_n, want_n)
    last = want_ids[-1].tolist()
    if cols:
        assert pos_out[:B].tolist() == (pos_in[:B] + n_draws).tolist() and pos_out[B:].tolist() == pos_in[B:].tolist()
        assert prm.tolist() == [int(pos_in[0]) + n_draws, last[0]] + last + tokens_in[B:].tolist()
    else:
        assert prm.tolist() == [n_past_in + n_draws, last[0], last[0]] + tokens_in[1:].tolist()


def _trunc_chain(row, k, n_bias, ban):
    return X.chain(k=k, top_p=0.95, temperature=0.8, penalty=1.30, freq=0.3, presence=0.2, z=0.9, typical=0.5, min_p=0.2,
                   bias=X.bias_for(row, k, n_bias, seed=k, ban_max=ban))


def _windows(rows, k, ch, sizes):
    out = []
    for c in range(rows.shape[0]):
        w = list(R.window_for(rows[c], k, sizes[c % len(sizes)], seed=c))
        if ch["bias"] and w:
            w[len(w) // 2] = ch["bias"][-1][0]  # a biased id that is also in the window
        out.append(w)
    return out


# (V, k, bias pairs): V = 3 with k = 3; 41; 1000, no multiple of 32 and most threads without an id; both k at the last row of the
# on-chip selection and at the first of the selection over global memory; 64 bias pairs beside full windows and k = 256, where window
# and bias ids overlap and repeat (|M| < 128: test_m_of_128_ids has the disjoint case)
TRUNC_CASES = [(3, 3, 2), (41, 40, 6), (1000, 40, 6), (1000, 256, 64), (CAP, 40, 6), (CAP, 256, 64), (CAP + 1, 40, 6), (CAP + 1, 256, 64)]


@pytest.mark.parametrize("cols", [False, True], ids=["one_session", "three_columns"])
@pytest.mark.parametrize("V,k,n_bias", TRUNC_CASES)
def test_the_truncating_chain_alone(G, V, k, n_bias, cols):
    """Bias (a -inf ban of the first row's raw maximum among it), both penalties, tail-free, locally typical, top-p and min-p, three
    draws: B = 1 without a BatchCols on row family 0, B = 3 with one on families 1 - 3 (64-pair cases: every window full)."""
    rows = _family_rows(V)[:1] if not cols else _family_rows(V)[1:]
    ch = _trunc_chain(rows[0], k, n_bias, ban=True)
    sizes = (64,) if n_bias == 64 else ((5,) if not cols else (64, 30, 5))
    _alone(G, rows, ch, _windows(rows, k, ch, sizes), 3, cols)


@pytest.mark.parametrize("cols", [False, True], ids=["one_session", "three_columns"])
@pytest.mark.parametrize("V", [1000, CAP, CAP + 1])
def test_m_of_128_ids(G, V, cols):
    """|M| = 128 beside k = 256: 64 bias ids and, in every column, a full window of 64 DISTINCT ids that are none of them — half from
    the column's raw top-k, half from outside it — so every slot of the kernel's M tables is written, the gather scans 128 ids and
    k + |M| = 384 keys are sorted; on chip (1000, CAP) and over global memory (CAP + 1).  The restatement counts 128 adjusted ids
    for every column before the hook runs.  Three draws."""
    k = 256
    rows = _family_rows(V)[:1] if not cols else _family_rows(V)[1:]
    ch = _trunc_chain(rows[0], k, 64, ban=True)
    banned = {t for t, _ in ch["bias"]}
    assert len(banned) == 64
    windows = []
    for c in range(rows.shape[0]):
        top = [int(t) for t in np.lexsort((np.arange(V), -rows[c].astype(np.float64)))[:k] if int(t) not in banned]
        rest = [t for t in range(V - 1, -1, -7) if t not in banned and t not in top[:32]]
        w = [x for pair in zip(top[:32], rest[:32]) for x in pair]
        assert len(set(w)) == 64 and not set(w) & banned
        assert len(X.adjusted(rows[c], w, ch)) == 128
        windows.append(w)
    _alone(G, rows, ch, windows, 3, cols)


@pytest.mark.parametrize("stage", ["bias", "freq_presence", "tail_free", "typical", "min_p"])
def test_each_stage_alone(G, stage):
    """One stage at a time (top_p = 1) at V = 1000, k = 40, three columns, five draws."""
    kw = dict(bias={}, freq_presence=dict(freq=0.3, presence=0.2), tail_free=dict(z=0.9), typical=dict(typical=0.5), min_p=dict(min_p=0.2))[stage]
    rows = _family_rows(1000)[:3]
    ch = X.chain(k=40, top_p=1.0, temperature=0.8, penalty=1.30, **kw)
    if stage == "bias":
        ch["bias"] = X.bias_for(rows[0], 40, 6, seed=1, ban_max=True)
    _alone(G, rows, ch, _windows(rows, 40, ch, (5, 64, 30)), 5, True)


def test_the_all_equal_row(G):
    """Every logit equal, no window, no bias: tail-free meets D == 0 and is skipped, locally typical's keys are all equal and fall to
    the index."""
    row = np.ascontiguousarray(_family_rows(1000)[3:4])
    ch = X.chain(k=40, top_p=0.95, temperature=0.8, z=0.9, typical=0.5, min_p=0.2)
    cand, _, idx = X.survivors(row[0], [], ch)
    assert [i for _, i in cand] == list(range(40)) and idx == list(range(len(idx))) and 1 < len(idx) < 40
    _alone(G, row, ch, [[]], 5, False)


@pytest.mark.parametrize("cols", [False, True], ids=["one_session", "three_columns"])
@pytest.mark.parametrize("V,n_draws", [(3, 5), (41, 70), (1000, 5), (CAP, 5)])
def test_mirostat_2_alone(G, V, n_draws, cols):
    """Mirostat 2 on the row in registers, bias (a ban of the first row's maximum) and both penalties in front: the ring wraps and mu
    moves at V = 41; at V = 1000 most threads hold no id; V = CAP is the widest row the device takes."""
    rows = _family_rows(V)[:1] if not cols else _family_rows(V)[:3]
    ch = X.chain(k=40, top_p=1.0, temperature=0.8, penalty=1.30, freq=0.1, presence=0.1, mirostat=2, tau=3.0, eta=0.25,
                 bias=X.bias_for(rows[0], 40, 5, seed=2, ban_max=True))
    _alone(G, rows, ch, _windows(rows, 40, ch, (5, 64, 30)), n_draws, cols)


def test_the_hook_declines_and_moves_nothing(G):
    """Mirostat 2 at V = CAP + 1, Mirostat 2 beside a truncating sampler, z = 0, a bias id listed twice, a NaN mu: -1, generator
    states and mu as they came."""
    from llm_amd import llama
    z32, hist, hist_n = np.zeros(32, np.int32), np.zeros(64, np.int32), np.zeros(1, np.int32)
    ids, prm = np.zeros(1, np.int32), np.zeros(34, np.int32)
    wide, row = np.zeros(CAP + 1, np.float32), np.zeros(300, np.float32)
    cases = [(wide, dict(MIRO), 6.0), (row, dict(MIRO, top_p=0.9), 6.0), (row, dict(MIRO, min_p=0.1), 6.0), (row, dict(TRUNC, tail_free_z=0.0), 6.0),
             (row, dict(TRUNC, bias=[(3, 1.0), (3, 2.0)]), 6.0), (row, dict(TRUNC, bias=[(300, 1.0)]), 6.0), (row, dict(MIRO), float("nan"))]
    for x, kw, mu0 in cases:
        rng, mu = np.array([77], np.uint64), np.array([mu0], np.float32)
        lc = llama.sampler_chain(**kw)
        assert G.lib().ggml_hip_debug_next_token_ex(x.ctypes.data, 1, x.size, C.addressof(lc), 0, None, z32.ctypes.data, hist.ctypes.data,
                                                    hist_n.ctypes.data, rng.ctypes.data, mu.ctypes.data, 1, ids.ctypes.data,
                                                    prm.ctypes.data, None) == -1
        assert int(rng[0]) == 77 and (np.isnan(mu[0]) if np.isnan(mu0) else float(mu[0]) == mu0)


# ---- the chains against the stepped loop ----
def _mk(G, O, cfg):
    from llm_amd import llama, synth
    if cfg == "q4_k":  # the small Q4_K model of the sampled chains' tests
        hp = dict(n_vocab=256, n_embd=256, n_head=4, n_head_kv=4, n_layer=2, n_rot=64, n_ff=512, n_mult=32)
        rng = np.random.default_rng(12)
        w = {}
        for name, (ne0, ne1) in synth.tensor_shapes(hp).items():
            w[name] = ((1.0 + 0.01 * rng.standard_normal(ne0)).astype(np.float32) if ne1 is None else
                       O.quantize(G.TYPE_Q4_K, (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32)))
        hp["wtype"] = G.TYPE_Q4_K
    else:
        hp, w = synth.make_llama(synth.TINY, 2, seed=31)
    return hp, llama.Llama(hp, w, context_size=CTX)


def _config(name, V):
    """(keywords, first mu or None): the truncating configuration with five bias pairs, or Mirostat 2."""
    if name == "mirostat":
        return dict(MIRO, bias=[(1, -1.5), (V - 1, 2.0)]), 6.0
    return dict(TRUNC, bias=[(0, float("-inf")), (1, -1.5), (7, 3.0), (V // 2, 2.0), (V - 1, 2.5)]), None


@pytest.mark.parametrize("config", ["truncating", "mirostat"])
@pytest.mark.parametrize("cfg", ["tiny", "q4_k"])
def test_one_session_chain_equals_the_stepped_loop(G, O, cfg, config):
    """Twin sessions behind a prompt and one stepped token: one takes infer_tokens_sampled_device(6), the other six
    infer_next_token_sampled.  The device drew all six; ids, generator state, mu's bits and snapshots are equal."""
    n = 6
    hp, model = _mk(G, O, cfg)
    kw, mu0 = _config(config, hp["n_vocab"])
    prompt = np.random.default_rng([5, n]).integers(0, hp["n_vocab"], 11).astype(np.int32)
    chain, step = (model.start_session(n_batch=8) for _ in range(2))
    state = {}
    for s in (chain, step):
        s.feed_prompt(prompt)
        rng = np.array([0x9E3779B97F4A7C15], np.uint64)
        mu = None if mu0 is None else np.array([mu0], np.float32)
        first = s.infer_next_token_sampled(rng, mu=mu, **kw)
        if s is chain:
            s0 = _stats(G)
            on_dev, ids = s.infer_tokens_sampled_device(n, rng, mu=mu, **kw)
            moved = [b - a for a, b in zip(s0, _stats(G))]
            assert on_dev == n and moved == [n, n, 0, 0, 0, 0, 0, 0, 0, n], moved
        else:
            ids = np.array([s.infer_next_token_sampled(rng, mu=mu, **kw) for _ in range(n)], np.int32)
        state[s] = (first, ids.tolist(), int(rng[0]), None if mu is None else int(mu.view(np.uint32)[0]))
    assert state[chain] == state[step], (state[chain], state[step])
    assert mu0 is None or state[chain][3] != int(np.array([mu0], np.float32).view(np.uint32)[0])
    assert chain.n_past == step.n_past and chain.snapshot() == step.snapshot()
    for t in (chain, step, model):
        t.free()


@pytest.mark.parametrize("config", ["truncating", "mirostat"])
@pytest.mark.parametrize("cfg", ["tiny", "q4_k"])
def test_batched_chain_equals_the_stepped_loop(G, O, cfg, config):
    """Three sessions with ragged prompts, n = 5: one infer_tokens_sampled_batch against five infer_next_tokens_sampled_batch on
    twins (the K-quant model under option plan_batch_k).  The chain ran; ids, generator states, mu's bits and snapshots are equal."""
    n, B = 5, 3
    hp, model = _mk(G, O, cfg)
    kw, mu0 = _config(config, hp["n_vocab"])
    g = np.random.default_rng([cfg == "tiny", B])
    prompts = [g.integers(0, hp["n_vocab"], 2 + 3 * c).astype(np.int32) for c in range(B)]
    out = []
    try:
        G.set_option("plan_batch_k", 1)
        for chained in (True, False):
            sessions = [model.start_session(n_batch=8) for _ in range(B)]
            for s, p in zip(sessions, prompts):
                s.feed_prompt(p)
            rngs = (np.arange(B, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567)).astype(np.uint64)
            mu = None if mu0 is None else np.full(B, mu0, np.float32)
            if chained:
                s0 = _stats(G)
                ran, ids = model.infer_tokens_sampled_batch(sessions, n, rngs, mu=mu, **kw)
                moved = [b - a for a, b in zip(s0, _stats(G))]
                assert ran is True and moved[:4] == [0, 0, n - 1, (n - 1) * B], moved
            else:
                rows = []
                for _ in range(n):
                    ran, r = model.infer_next_tokens_sampled_batch(sessions, rngs, mu=mu, **kw)
                    assert ran is True
                    rows.append(r)
                ids = np.stack(rows)
            out.append((ids.tolist(), rngs.tolist(), None if mu is None else mu.view(np.uint32).tolist(), [s.snapshot() for s in sessions],
                        [s.n_past for s in sessions]))
            for s in sessions:
                s.free()
    finally:
        G.set_option("plan_batch_k", 0)
    assert out[0][:3] == out[1][:3], (out[0][:3], out[1][:3])
    assert out[0][3] == out[1][3] and out[0][4] == out[1][4]
    assert mu0 is None or all(m != int(np.array([mu0], np.float32).view(np.uint32)[0]) for m in out[0][2])
    model.free()


def test_the_chains_decline_and_fall_back(G, O):
    """With option plan_sample_chain off the extended chain runs as the stepped loop: nothing drawn on the device, no sampled-chain
    counter moves, ids and states equal a stepped twin's.  What the specification declines raises with nothing moved: sessions,
    generators, mu, counters."""
    hp, model = _mk(G, O, "tiny")
    V = hp["n_vocab"]
    prompt = np.random.default_rng(4).integers(0, V, 8).astype(np.int32)
    a, b = (model.start_session(n_batch=8) for _ in range(2))
    for s in (a, b):
        s.feed_prompt(prompt)
    kw = dict(TRUNC)
    ra, rb = np.array([5], np.uint64), np.array([5], np.uint64)
    a.infer_next_token_sampled(ra, **kw)
    b.infer_next_token_sampled(rb, **kw)
    s0 = _stats(G)
    try:
        G.set_option("plan_sample_chain", 0)
        on_dev, ids = a.infer_tokens_sampled_device(4, ra, **kw)
    finally:
        G.set_option("plan_sample_chain", 1)
    assert on_dev == 0 and [y - x for x, y in zip(s0, _stats(G))][:4] == [0, 0, 0, 0]
    ids_b = [b.infer_next_token_sampled(rb, **kw) for _ in range(4)]
    assert ids.tolist() == ids_b and int(ra[0]) == int(rb[0]) and a.snapshot() == b.snapshot()
    s0, at, snap = _stats(G), a.n_past, a.snapshot()
    mu = np.array([6.0], np.float32)
    for bad in (dict(MIRO, top_p=0.9), dict(MIRO, tau=0.0), dict(TRUNC, tail_free_z=0.0), dict(TRUNC, typical_p=0.0), dict(TRUNC, min_p=2.0),
                dict(TRUNC, bias=[(V, 1.0)]), dict(TRUNC, bias=[(1, 1.0), (1, 1.0)]), dict(TRUNC, bias=[(1, float("inf"))]),
                dict(TRUNC, mirostat=1), dict(TRUNC, freq=float("nan"))):
        with pytest.raises(ValueError):
            a.infer_tokens_sampled_device(3, ra, mu=mu, **bad)
        with pytest.raises(ValueError):
            model.infer_tokens_sampled_batch([a, b], 3, np.array([1, 2], np.uint64), mu=np.array([6.0, 6.0], np.float32), **bad)
    assert _stats(G) == s0 and a.n_past == at and a.snapshot() == snap and int(ra[0]) == int(rb[0]) and float(mu[0]) == 6.0
    for t in (a, b, model):
        t.free()
