"""Chains that stop (ggml_hip_decode_chain_requests / ggml_hip_decode_batch_requests, Session.infer_until, Llama.infer_until_batch):
every column carries its own sampler (or the first maximum), its own stop ids and its own budget; a column that ends is frozen while
the others go on, the call ends when none is live, and every session is left where its own last evaluation left it.

Every comparison is equality: the kernels between two steps alone, through the hook, against tests/sampler_chain_ref.py stepped per
column with that column's parameters and end rule; the chains against twins on the existing stepped entries that stop by the same
rule (ids, counts, reasons, generator states, the bits of mu, n_past, Session.snapshot() byte for byte — the snapshot holds
last_logits and the K/V memory, so it is the check that frozen replays rewrite the same bits).  Stop ids are taken from a stepped
twin's own free run: the id of a draw j whose first occurrence is j."""
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
NEW = ("chain_stopped_columns", "chain_frozen_steps", "chain_steps_cut")
DEFAULT = dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30)
TRUNC = dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30, freq=0.3, presence=0.2, tail_free_z=0.9, typical_p=0.5, min_p=0.2)
MIRO = dict(k=40, top_p=1.0, temperature=0.8, penalty=1.30, freq=0.1, presence=0.1, mirostat=2, tau=3.0, eta=0.25)
BUDGET, STOP = 1, 2


def _stats(G, keys=COUNTERS):
    return [int(G.lib().ggml_hip_get_stat(k.encode())) for k in keys]


def _lib_chain(ch):
    from llm_amd import llama
    return llama.sampler_chain(k=ch["k"], top_p=ch["top_p"], temperature=ch["temperature"], penalty=ch["penalty"], freq=ch["freq"],
                               presence=ch["presence"], tail_free_z=ch["z"], typical_p=ch["typical"], min_p=ch["min_p"], bias=ch["bias"],
                               mirostat=ch["mirostat"], tau=ch["tau"], eta=ch["eta"])


# ---- 1. the launch alone ----
_rows = {}


def _family_rows(V):
    if V not in _rows:
        _rows[V] = R.rows(4, V, seed=5)
        _rows[V].setflags(write=False)
    return _rows[V]


def _draw(row, window, ch, rng, mu):
    """One draw of a column's request: its sampler, or (ch None) the first maximum."""
    if ch is None:
        return int(np.lexsort((np.arange(row.size), -row.astype(np.float64)))[0]), rng, mu
    return X.sample(row, window, ch, rng, mu)


def _free_ids(row, window, ch, rng, mu, n):
    hist, out = list(window), []
    for _ in range(n):
        tok, rng, mu = _draw(row, hist[-64:], ch, rng, mu)
        hist.append(tok)
        out.append(tok)
    return out


def _alone(G, rows, chains, ends, windows, n_draws, cols):
    """The kernels between two steps through the hook, n_draws rounds on rows [B][V]; chains[c] a restatement dict or None (greedy),
    ends[c] = (max_draws, stop ids).  Against the restatement stepped per column under the column's own end rule: ids with their -1
    entries, rings, counts, generator states, mu's bits, DecParams and positions, the draws made and the reasons; entries from B on
    keep their sentinels."""
    from llm_amd import llama
    B, V = rows.shape
    T = 8 if cols else 1
    n_past_in = 17
    pos_in = (np.arange(8, dtype=np.int32) * 7 + 3) % 40
    tokens_in = np.arange(32, dtype=np.int32) + 70000  # sentinels: no id of any vocabulary here
    hist = np.full((T, 64), 80000, np.int32)
    hist_n = np.full(T, 7, np.int32)
    rng = (np.arange(T, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567 + V)).astype(np.uint64)
    mu = (np.arange(T, dtype=np.float32) * np.float32(0.5) + np.float32(6.0)).astype(np.float32)
    for c in range(B):
        w = np.asarray(windows[c], np.int32)
        hist[c, :w.size] = w
        hist_n[c] = w.size
    want_hist, want_n, want_rng, want_mu = hist.copy(), hist_n.copy(), [int(x) for x in rng], mu.copy()
    want_ids = np.full((n_draws, B), -1, np.int32)
    want_drawn, want_why, last = [0] * B, [0] * B, [None] * B
    for c in range(B):
        budget, stops = ends[c]
        live = budget > 0
        if not live:
            want_why[c] = BUDGET
        for d in range(n_draws):
            if not live:
                continue
            window = want_hist[c, :min(int(want_n[c]), 64)]
            tok, want_rng[c], m = _draw(rows[c], window, chains[c], want_rng[c], want_mu[c])
            want_mu[c] = m
            want_hist[c, want_n[c] % 64] = tok
            want_n[c] += 1
            want_ids[d, c] = last[c] = tok
            want_drawn[c] += 1
            if tok in stops:
                live, want_why[c] = False, STOP
            elif want_drawn[c] >= budget:
                live, want_why[c] = False, BUDGET
    lcs = [None if ch is None else _lib_chain(ch) for ch in chains]
    cptr = (C.c_void_p * B)(*[None if lc is None else C.addressof(lc) for lc in lcs])
    eptr = (llama.ChainEnd * B)(*[llama.chain_end(b, s) for b, s in ends])
    ids = np.full((n_draws, B), -5, np.int32)
    prm, pos_out = np.full(34, -1, np.int32), np.full(8, -1, np.int32)
    drawn, why = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    rows = np.ascontiguousarray(rows)
    rc = G.lib().ggml_hip_debug_next_token_req(rows.ctypes.data, B, V, cptr, eptr, n_past_in, pos_in.ctypes.data if cols else None,
                                               tokens_in.ctypes.data, hist.ctypes.data, hist_n.ctypes.data, rng.ctypes.data, mu.ctypes.data,
                                               n_draws, ids.ctypes.data, prm.ctypes.data, pos_out.ctypes.data if cols else None,
                                               drawn.ctypes.data, why.ctypes.data)
    assert rc == 0
    assert np.array_equal(ids, want_ids), (ids, want_ids)
    assert drawn.tolist() == want_drawn and why.tolist() == want_why, (drawn, want_drawn, why, want_why)
    assert [int(x) for x in rng] == want_rng  # (a frozen column's: where its last draw left it; entries from B on: as they came)
    assert np.array_equal(mu.view(np.uint32), want_mu.view(np.uint32)), (mu, want_mu)
    assert np.array_equal(hist, want_hist) and np.array_equal(hist_n, want_n)
    toks = [int(tokens_in[c]) if last[c] is None else last[c] for c in range(B)]
    if cols:
        assert pos_out[:B].tolist() == (pos_in[:B] + np.array(want_drawn, np.int32)).tolist() and pos_out[B:].tolist() == pos_in[B:].tolist()
        assert prm.tolist() == [int(pos_in[0]) + want_drawn[0], toks[0]] + toks + tokens_in[B:].tolist()
    else:
        assert prm.tolist() == [n_past_in + want_drawn[0], toks[0], toks[0]] + tokens_in[1:].tolist()
    return want_drawn, want_why


def _four_classes(V):
    """One column of each class on row families 0 .. 3: default, truncating with bias pairs, Mirostat 2 (on chip only), greedy."""
    rows = _family_rows(V)
    chains = [X.chain(**DEFAULT),
              X.chain(k=40, top_p=0.95, temperature=0.8, penalty=1.30, freq=0.3, presence=0.2, z=0.9, typical=0.5, min_p=0.2,
                      bias=X.bias_for(rows[1], 40, 6, seed=40, ban_max=True)),
              X.chain(k=40, top_p=1.0, temperature=0.8, penalty=1.30, freq=0.1, presence=0.1, mirostat=2, tau=3.0, eta=0.25), None]
    windows = [list(R.window_for(rows[c], 40, (5, 64, 30, 12)[c], seed=c)) for c in range(4)]
    if V > CAP:  # Mirostat 2 is declined beyond the on-chip selection: three columns
        keep = [0, 1, 3]
        return np.ascontiguousarray(rows[keep]), [chains[c] for c in keep], [windows[c] for c in keep]
    return rows, chains, windows


@pytest.mark.parametrize("V", [41, 1000, CAP, CAP + 1])
def test_the_launch_alone_with_a_request_per_column(G, V):
    """B = 4 (3 beyond the on-chip selection), one column of each class, three different ends — the truncating column stops on the id
    of its draw 1, the last sampled column has a budget of 2, the others never end before the fifth round — five rounds."""
    rows, chains, windows = _four_classes(V)
    B = rows.shape[0]
    rng1 = int(np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567 + V))
    free = _free_ids(rows[1], windows[1], chains[1], rng1, np.float32(6.5), 5)  # (V = 41 is peaked: draw 1 repeats draw 0, the stop comes a round sooner)
    ends = [(5, [V - 1 - int(free[0] == V - 1)])] + [(5, [free[1]])] + ([(2, [])] if B == 4 else []) + [(5, [])]
    drawn, why = _alone(G, rows, chains, ends, windows, 5, True)
    assert drawn[1] == (1 if free[1] == free[0] else 2) and why[1] == STOP and (B == 3 or (drawn[2] == 2 and why[2] == BUDGET)) and drawn[-1] == 5 and why[-1] == BUDGET


@pytest.mark.parametrize("V,cls", [(1000, "default"), (1000, "truncating"), (1000, "mirostat"), (1000, "greedy"), (CAP + 1, "default"),
                                   (CAP + 1, "truncating"), (CAP + 1, "greedy")])
def test_the_launch_alone_for_one_session(G, V, cls):
    """B = 1 without a BatchCols, each class on chip and (Mirostat 2 is declined there) over global memory, a stop on the id of draw 1
    (greedy: a budget of 2), five rounds."""
    rows, chains, windows = _four_classes(V)
    c = dict(default=0, truncating=1, mirostat=2, greedy=len(chains) - 1)[cls]
    rng0 = 0x1234567 + rows.shape[1]
    free = _free_ids(rows[c], windows[c], chains[c], rng0, np.float32(6.0), 5)
    end = (2, []) if cls == "greedy" or free[1] == free[0] else (5, [free[1]])
    drawn, why = _alone(G, rows[c:c + 1], [chains[c]], [end], [windows[c]], 5, False)
    assert drawn == [2]


def test_every_column_born_frozen_moves_nothing(G):
    rows, chains, windows = _four_classes(1000)
    drawn, why = _alone(G, rows, chains, [(0, [3])] * 4, windows, 5, True)
    assert drawn == [0] * 4 and why == [BUDGET] * 4


# ---- the chains against stepped twins ----
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
        hp, w = synth.make_llama(synth.TINY, 1 if cfg == "f16" else 2, seed=31)
    return hp, llama.Llama(hp, w, context_size=CTX)


def _config(name, V):
    """(sampler keywords or None for greedy, first mu or None)"""
    if name == "greedy":
        return None, None
    if name == "mirostat":
        return dict(MIRO, bias=[(1, -1.5), (V - 1, 2.0)]), 6.0
    if name == "default":
        return dict(DEFAULT), None
    return dict(TRUNC, bias=[(0, float("-inf")), (1, -1.5), (7, 3.0), (V // 2, 2.0), (V - 1, 2.5)]), None


def _seed(x):
    return np.array([0x9E3779B97F4A7C15 + x], np.uint64)


def _step(s, kw, rng, mu):
    return s.infer_next_token() if kw is None else s.infer_next_token_sampled(rng, mu=mu, **kw)


def _stepped_until(s, kw, rng, mu, max_tokens, stop):
    """The twin: the existing stepped entries under the reference's rule."""
    ids, why = [], "budget"
    for _ in range(max_tokens):
        if s.n_past + 1 >= CTX:
            why = "context"
            break
        ids.append(_step(s, kw, rng, mu))
        if ids[-1] in stop:
            why = "stop"
            break
    return ids, why


def _first_new(ids, lo, hi):
    """The first draw j in lo .. hi whose id occurs at j for the first time."""
    for j in range(lo, hi + 1):
        if ids[j] not in ids[:j]:
            return j
    raise AssertionError("no draw in %d .. %d whose id is new: %r — choose another seed" % (lo, hi, ids))


def _state(rng, mu):
    return (None if rng is None else int(rng[0]), None if mu is None else int(mu.view(np.uint32)[0]))


def _one_session(G, O, cfg, config, n, prompt_len, j_range, group=4, seed=7):
    """Three sessions behind the same prompt and one stepped token: `free` runs n stepped draws to find the stop id, `step` is the twin
    under the rule, `chain` takes infer_until.  Returns (j, counter movements of the chain's call)."""
    hp, model = _mk(G, O, cfg)
    kw, mu0 = _config(config, hp["n_vocab"])
    prompt = np.random.default_rng([seed, n]).integers(0, hp["n_vocab"], prompt_len).astype(np.int32)
    free, step, chain = (model.start_session(n_batch=8) for _ in range(3))
    out, j, stop, moved = {}, None, None, None
    try:
        G.set_option("chain_group", group)
        for s in (free, step, chain):
            s.feed_prompt(prompt)
            rng = None if kw is None else _seed(seed)
            mu = None if mu0 is None else np.array([mu0], np.float32)
            first = _step(s, kw, rng, mu)
            if s is free:
                ids = [_step(s, kw, rng, mu) for _ in range(n)]
                j = _first_new(ids, *j_range)
                stop = ids[j]
                other = next(t for t in range(hp["n_vocab"]) if t not in ids)  # a second stop id, never drawn
            elif s is step:
                ids, why = _stepped_until(s, kw, rng, mu, n, [stop])
                assert len(ids) == j + 1 and why == "stop"
                out[s] = (first, ids, len(ids), why, _state(rng, mu), s.n_past, s.snapshot())
            else:
                s0 = _stats(G, COUNTERS + NEW)
                got, count, why, ran = s.infer_until(n, rng, stop=[other, stop], mu=mu, **(kw or {}))
                moved = [b - a for a, b in zip(s0, _stats(G, COUNTERS + NEW))]
                assert ran is True
                out[s] = (first, got.tolist(), count, why, _state(rng, mu), s.n_past, s.snapshot())
    finally:
        G.set_option("chain_group", 8)
    assert out[chain][:6] == out[step][:6], (out[chain][:6], out[step][:6])
    assert out[chain][6] == out[step][6]
    for t in (free, step, chain, model):
        t.free()
    return j, dict(zip(COUNTERS + NEW, moved))


@pytest.mark.parametrize("config", ["truncating", "mirostat", "greedy"])
@pytest.mark.parametrize("cfg", ["tiny", "q4_k"])
def test_one_session_stops_where_the_stepped_loop_stops(G, O, cfg, config):
    """n = 12 in groups of 4, the stop id drawn at draw j (1 <= j <= n - 3): ids, count, reason, generator state, mu's bits, n_past
    and the snapshot equal the twin's.  One column stopped; the groups behind the one whose flags showed the end were never
    launched (the host looks at a group's flags once the next group is enqueued)."""
    n = 12
    j, moved = _one_session(G, O, cfg, config, n, 11, (1, n - 3))
    launched = min(n, (j // 4 + 2) * 4)
    assert moved["chain_stopped_columns"] == 1 and moved["chain_steps_cut"] == n - launched, (j, moved)
    assert moved["chain_frozen_steps"] == launched - (j + 1) and moved["plan_tokens"] == launched, (j, moved)
    assert moved["sample_chain_steps"] == (0 if config == "greedy" else launched)


def test_one_session_across_a_change_of_attention_variant(G, O):
    """Option attn_split = 24 at context 64: behind a prompt of 12 tokens and one stepped token, step i of the chain attends over
    14 + i positions, so steps 0 .. 9 take one workgroup per head and steps 10, 11 the position-split attention.  The stop falls on
    draw 8, two draws before the change: the group ends at the boundary (steps 8, 9), its flags are read before anything of the
    other variant is enqueued, and steps 10 and 11 are never launched."""
    n = 12
    try:
        G.set_option("attn_split", 24)
        j, moved = _one_session(G, O, "tiny", "truncating", n, 12, (8, 8))
    finally:
        G.set_option("attn_split", 1)
    assert j == 8 and moved["chain_stopped_columns"] == 1 and moved["chain_steps_cut"] == 2 and moved["chain_frozen_steps"] == 1, moved


def _batched(G, O, cfg, plan, n_all, group=4):
    """plan: per session (config name, prompt length, max_tokens, stop rule) with stop rule None or ("new", lo, hi) = the id of the first
    draw in lo .. hi of the session's free run that is new there, or ("at", i) = the id of draw i.  Free twins find the stop ids, `alone`
    twins run each session ALONE through the stepped entries to its own end, then one infer_until_batch.  Returns what the call moved."""
    hp, model = _mk(G, O, cfg)
    V, B = hp["n_vocab"], len(plan)
    g = np.random.default_rng([cfg == "tiny", B, n_all])
    prompts = [g.integers(0, V, p[1]).astype(np.int32) for p in plan]
    cfgs = [_config(p[0], V) for p in plan]
    stops, want = [], []
    try:
        G.set_option("plan_batch_k", 1)
        G.set_option("chain_group", group)
        for c, p in enumerate(plan):
            kw, mu0 = cfgs[c]
            stop = []
            if p[3] is not None:
                s = model.start_session(n_batch=8)
                s.feed_prompt(prompts[c])
                rng, mu = (None if kw is None else _seed(c)), (None if mu0 is None else np.array([mu0], np.float32))
                ids = [_step(s, kw, rng, mu) for _ in range(min(p[2], CTX - 1 - s.n_past))]
                stop = [ids[_first_new(ids, p[3][1], p[3][2])]] if p[3][0] == "new" else [ids[p[3][1]]]
                s.free()
            stops.append(stop)
            s = model.start_session(n_batch=8)
            s.feed_prompt(prompts[c])
            rng, mu = (None if kw is None else _seed(c)), (None if mu0 is None else np.array([mu0], np.float32))
            ids, why = _stepped_until(s, kw, rng, mu, p[2], stop)
            want.append((ids, why, _state(rng, mu), s.n_past, s.snapshot()))
            s.free()
        sessions = [model.start_session(n_batch=8) for _ in range(B)]
        for s, pr in zip(sessions, prompts):
            s.feed_prompt(pr)
        rngs = np.array([int(_seed(c)[0]) for c in range(B)], np.uint64)
        mus = np.array([6.0 if m is None else m for _, m in cfgs], np.float32)
        reqs = [dict(max_tokens=p[2], stop=stops[c], sampler=cfgs[c][0]) for c, p in enumerate(plan)]
        s0 = _stats(G, COUNTERS + NEW)
        ids, counts, reasons, ran = model.infer_until_batch(sessions, reqs, rngs, mu=mus)
        moved = dict(zip(COUNTERS + NEW, [b - a for a, b in zip(s0, _stats(G, COUNTERS + NEW))]))
        assert ran is True
        assert ids.shape == (max(p[2] for p in plan), B)
        for c in range(B):
            w_ids, w_why, w_state, w_past, w_snap = want[c]
            col = ids[:, c].tolist()
            assert col == w_ids + [-1] * (ids.shape[0] - len(w_ids)), (c, col, w_ids)
            assert int(counts[c]) == len(w_ids) and reasons[c] == w_why, (c, counts, reasons, w_why)
            kw, mu0 = cfgs[c]
            got_state = (None if kw is None else int(rngs[c]), None if mu0 is None else int(mus[c:c + 1].view(np.uint32)[0]))
            assert got_state == w_state, (c, got_state, w_state)
            assert sessions[c].n_past == w_past and sessions[c].snapshot() == w_snap, c
        for s in sessions:
            s.free()
    finally:
        G.set_option("plan_batch_k", 0)
        G.set_option("chain_group", 8)
    model.free()
    return moved, [len(w[0]) for w in want]


@pytest.mark.parametrize("cfg", ["tiny", "q4_k", "f16"])
def test_batched_ragged_requests_equal_each_session_alone(G, O, cfg):
    """B = 3, ragged prompts, n = 8: a truncating column that stops at draw j (1 <= j <= 5), a Mirostat column with a budget of 2, a
    greedy column that runs all eight — each against its own session stepped alone to its own end."""
    n = 8
    moved, lens = _batched(G, O, cfg, [("truncating", 2, n, ("new", 1, n - 3)), ("mirostat", 5, 2, None), ("greedy", 8, n, None)], n)
    assert lens[1] == 2 and lens[2] == n and 2 <= lens[0] <= n - 2
    assert moved["chain_stopped_columns"] == 1 and moved["chain_steps_cut"] == 0, moved
    assert moved["chain_frozen_steps"] == (n - lens[0]) + (n - 2) and moved["batch_sample_steps"] == n - 1, moved


def test_batched_all_columns_end_early_and_the_call_is_cut(G, O):
    """Every column ends by step 3 of 16 (a stop on the id of its draw 2, or a budget of 2), groups of 4: the flags behind steps
    0 .. 3 are read once steps 4 .. 7 are enqueued, and the last eight steps are never launched; their rows of the ids are -1
    (compared in _batched with every other row)."""
    n = 16
    moved, lens = _batched(G, O, "tiny", [("truncating", 3, n, ("at", 2)), ("default", 6, n, ("at", 2)), ("greedy", 4, 2, None)], n)
    assert max(lens) <= 3, lens
    assert moved["chain_steps_cut"] >= 8, moved
    assert moved["plan_tokens"] == 3 * (n - moved["chain_steps_cut"])


def test_a_session_with_little_room_is_batched_with_one_that_has_plenty(G, O):
    """Context 64: a session at n_past = 61 may draw twice more (inference_session.rs:388), its neighbour eight times.  The existing
    batched chain with n = 8 declines the pair as a whole (ValueError, nothing moved); the requests chain runs, the first session ends
    after two tokens on the context, and both equal their stepped twins (compared in _batched)."""
    hp, model = _mk(G, O, "tiny")
    a, b = model.start_session(n_batch=8), model.start_session(n_batch=8)
    g = np.random.default_rng([1, 2, 8])
    a.feed_prompt(g.integers(0, hp["n_vocab"], 61).astype(np.int32))
    b.feed_prompt(g.integers(0, hp["n_vocab"], 7).astype(np.int32))
    snaps, s0 = (a.snapshot(), b.snapshot()), _stats(G)
    with pytest.raises(ValueError):
        model.infer_tokens_sampled_batch([a, b], 8, np.array([1, 2], np.uint64), **DEFAULT)
    assert (a.snapshot(), b.snapshot()) == snaps and _stats(G) == s0 and a.n_past == 61
    for t in (a, b, model):
        t.free()
    moved, lens = _batched(G, O, "tiny", [("default", 61, 8, None), ("truncating", 7, 8, None)], 8)
    assert lens == [2, 8] and moved["chain_steps_cut"] == 0 and moved["chain_frozen_steps"] == 6, (lens, moved)


# ---- 6. no stop configured ----
@pytest.mark.parametrize("config", ["truncating", "greedy"])
def test_one_session_without_a_stop_is_the_existing_chain(G, O, config):
    """infer_until with no stop id against infer_tokens_sampled_device / infer_tokens_device on a twin: ids, states, snapshots and the
    movements of the existing counters are equal; nothing was frozen or cut."""
    n = 6
    hp, model = _mk(G, O, "tiny")
    kw, mu0 = _config(config, hp["n_vocab"])
    prompt = np.random.default_rng([5, n]).integers(0, hp["n_vocab"], 11).astype(np.int32)
    new, old = (model.start_session(n_batch=8) for _ in range(2))
    out = {}
    for s in (new, old):
        s.feed_prompt(prompt)
        rng = None if kw is None else _seed(3)
        first = _step(s, kw, rng, None)
        s0 = _stats(G, COUNTERS + NEW)
        if s is new:
            ids, count, why, ran = s.infer_until(n, rng, **(kw or {}))
            assert ran is True and count == n and why == "budget"
        elif kw is None:
            ids = s.infer_tokens_device(n)
        else:
            on_dev, ids = s.infer_tokens_sampled_device(n, rng, **kw)
            assert on_dev == n
        moved = [b - a for a, b in zip(s0, _stats(G, COUNTERS + NEW))]
        out[s] = (first, ids.tolist(), _state(rng, None), s.n_past, moved, s.snapshot())
    assert out[new][:5] == out[old][:5], (out[new][:5], out[old][:5])
    assert out[new][5] == out[old][5] and out[new][4][-3:] == [0, 0, 0]
    for t in (new, old, model):
        t.free()


def test_batched_without_a_stop_is_the_existing_chain(G, O):
    """infer_until_batch with equal budgets, one sampler and no stop ids against infer_tokens_sampled_batch on twins."""
    n, B = 5, 3
    hp, model = _mk(G, O, "tiny")
    kw, _ = _config("truncating", hp["n_vocab"])
    g = np.random.default_rng([1, B])
    prompts = [g.integers(0, hp["n_vocab"], 2 + 3 * c).astype(np.int32) for c in range(B)]
    out = []
    for new in (True, False):
        sessions = [model.start_session(n_batch=8) for _ in range(B)]
        for s, p in zip(sessions, prompts):
            s.feed_prompt(p)
        rngs = (np.arange(B, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567)).astype(np.uint64)
        s0 = _stats(G, COUNTERS + NEW)
        if new:
            ids, counts, reasons, ran = model.infer_until_batch(sessions, [dict(max_tokens=n, sampler=kw)] * B, rngs)
            assert counts.tolist() == [n] * B and reasons == ["budget"] * B
        else:
            ran, ids = model.infer_tokens_sampled_batch(sessions, n, rngs, **kw)
        assert ran is True
        moved = [b - a for a, b in zip(s0, _stats(G, COUNTERS + NEW))]
        out.append((ids.tolist(), rngs.tolist(), [s.n_past for s in sessions], moved, [s.snapshot() for s in sessions]))
        for s in sessions:
            s.free()
    assert out[0][:4] == out[1][:4], (out[0][:4], out[1][:4])
    assert out[0][4] == out[1][4] and out[0][3][-3:] == [0, 0, 0]
    model.free()


# ---- 7. declines ----
def test_bad_requests_raise_and_the_options_fall_back_to_the_stepped_loop(G, O):
    """What the entries decline raises ValueError with counters, sessions, generators and mu unmoved: more than the vocabulary holds in
    a stop id, a negative one, max_tokens = 0, what the sampler's specification declines, Mirostat 2 without mu.  The backend entries
    return -1 for a stop id outside the vocabulary, and the hook for Mirostat 2 beyond the on-chip selection.  With plan_sample_chain
    / plan_batch_sample off the stepped loop runs under the same rule and gives what the chain gives."""
    from llm_amd import llama
    hp, model = _mk(G, O, "tiny")
    V = hp["n_vocab"]
    prompt = np.random.default_rng(4).integers(0, V, 8).astype(np.int32)
    a, b, c, d = (model.start_session(n_batch=8) for _ in range(4))
    ra, rb = _seed(1), _seed(1)
    for s, r in ((a, ra), (b, rb), (c, None), (d, None)):
        s.feed_prompt(prompt)
        if r is not None:
            s.infer_next_token_sampled(r, **TRUNC)
    s0, snap, mu = _stats(G, COUNTERS + NEW), a.snapshot(), np.array([6.0], np.float32)
    for bad in (dict(stop=[V]), dict(stop=[-1]), dict(max_tokens=0), dict(tail_free_z=0.0), dict(mirostat=1), dict(bias=[(V, 1.0)])):
        kw = dict(TRUNC, max_tokens=4, stop=[])
        kw.update(bad)
        with pytest.raises(ValueError):
            a.infer_until(kw.pop("max_tokens"), ra, mu=mu, **kw)
        req = dict(max_tokens=dict(bad).get("max_tokens", 4), stop=dict(bad).get("stop", []),
                   sampler=dict(TRUNC, **{k: v for k, v in bad.items() if k not in ("stop", "max_tokens")}))
        with pytest.raises(ValueError):
            model.infer_until_batch([a, b], [req, dict(max_tokens=4, sampler=TRUNC)], np.array([1, 2], np.uint64))
    with pytest.raises(ValueError):
        a.infer_until(4, ra, **MIRO)  # (no mu)
    with pytest.raises(ValueError):
        a.infer_until(4, ra, stop=list(range(9)), **TRUNC)
    assert _stats(G, COUNTERS + NEW) == s0 and a.snapshot() == snap and int(ra[0]) == int(rb[0]) and float(mu[0]) == 6.0
    # the hook: Mirostat 2 beyond the on-chip selection, a stop id outside the vocabulary
    wide = np.zeros(CAP + 1, np.float32)
    z32, hist, hist_n = np.zeros(32, np.int32), np.zeros(64, np.int32), np.zeros(1, np.int32)
    ids, prm, one = np.zeros(1, np.int32), np.zeros(34, np.int32), np.zeros(1, np.int32)
    for x, kw, end in ((wide, MIRO, llama.chain_end(1)), (wide[:300], TRUNC, llama.chain_end(1, [300])), (wide[:300], TRUNC, llama.chain_end(2))):
        rng, m = np.array([77], np.uint64), np.array([6.0], np.float32)
        lc = llama.sampler_chain(**kw)
        cptr, eptr = (C.c_void_p * 1)(C.addressof(lc)), (llama.ChainEnd * 1)(end)
        assert G.lib().ggml_hip_debug_next_token_req(x.ctypes.data, 1, x.size, cptr, eptr, 0, None, z32.ctypes.data, hist.ctypes.data,
                                                     hist_n.ctypes.data, rng.ctypes.data, m.ctypes.data, 1, ids.ctypes.data, prm.ctypes.data,
                                                     None, one.ctypes.data, one.ctypes.data) == -1
        assert int(rng[0]) == 77 and float(m[0]) == 6.0
    # options off: the stepped loop under the same rule
    free = [b.infer_next_token_sampled(rb, **TRUNC) for _ in range(6)]
    stop = free[_first_new(free, 1, 4)]
    want = free[:free.index(stop) + 1]
    s0 = _stats(G)
    try:
        G.set_option("plan_sample_chain", 0)
        got, count, why, ran = a.infer_until(6, ra, stop=[stop], **TRUNC)
    finally:
        G.set_option("plan_sample_chain", 1)
    assert ran is False and got.tolist() == want and count == len(want) and why == "stop"
    assert [y - x for x, y in zip(s0, _stats(G))][:4] == [0, 0, 0, 0]
    rngs_c, rngs_d = np.array([5, 6], np.uint64), np.array([5, 6], np.uint64)
    reqs = [dict(max_tokens=4, sampler=TRUNC), dict(max_tokens=2, sampler=DEFAULT)]
    try:
        G.set_option("plan_batch_sample", 0)
        ids_off, counts_off, why_off, ran_off = model.infer_until_batch([c, d], reqs, rngs_c)
    finally:
        G.set_option("plan_batch_sample", 1)
    e, f = model.start_session(n_batch=8), model.start_session(n_batch=8)
    e.feed_prompt(prompt)
    f.feed_prompt(prompt)
    ids_on, counts_on, why_on, ran_on = model.infer_until_batch([e, f], reqs, rngs_d)
    assert ran_off is False and ran_on is True
    assert ids_off.tolist() == ids_on.tolist() and counts_off.tolist() == counts_on.tolist() == [4, 2] and why_off == why_on == ["budget"] * 2
    assert rngs_c.tolist() == rngs_d.tolist() and c.snapshot() == e.snapshot() and d.snapshot() == f.snapshot()
    for t in (a, b, c, d, e, f, model):
        t.free()
