"""The packed prompt batch (ggml_hip_prompt_pack, plan_pack.inc, kernels/prompt_pack.h): the prompt rows of several sessions of one
model as ONE pass of the prompt plan, each session's rows at its own positions in its own cache.

What a segment of 9 rows or more is held to: the same session evaluated ALONE with option mmq_min = 9, which runs the very launches
the pack restates (plan_launch_prompt: the same GEMMs with the same K split at these shapes, the same fused attention tiles) — bit
for bit, every logits row, the embedding row, K/V and the snapshot.  A segment of 1 .. 8 rows has no partner on the same arithmetic
when fed alone (the chunk plan computes exact integer block dots): it is held to itself in another pack, at another row0 and beside
other neighbours, bit for bit, and to the CPU oracle within the f16 GEMM's bound of tests/test_prompt_plan_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CTX = 512
# the models of tests/test_prompt_plan_gpu.py: D = 32, 64 and 128, grouped-query attention, GEMMs that split K
GQA = dict(n_vocab=256, n_embd=128, n_head=4, n_head_kv=2, n_layer=2, n_rot=32, n_ff=352, n_mult=32)
WIDE = dict(n_vocab=320, n_embd=256, n_head=4, n_head_kv=4, n_layer=3, n_rot=64, n_ff=512, n_mult=32)
SPLITK = dict(n_vocab=256, n_embd=1024, n_head=8, n_head_kv=4, n_layer=2, n_rot=128, n_ff=2048, n_mult=32)
COUNTERS = ("prompt_pack_calls", "prompt_pack_segments", "prompt_pack_tokens", "prompt_plan_tokens", "plan_tokens", "generic_graphs")

_weights = {}


def _stats(G, keys=COUNTERS):
    return [int(G.lib().ggml_hip_get_stat(k.encode())) for k in keys]


def _mk(cfg, wtype, seed=5):
    from llm_amd import llama, synth
    key = (cfg, wtype, seed)
    if key not in _weights:
        _weights[key] = synth.make_llama({"tiny": synth.TINY, "gqa": GQA, "wide": WIDE, "splitk": SPLITK}[cfg], wtype, seed=seed)
    hp, w = _weights[key]
    return hp, w, llama.Llama(hp, w, context_size=CTX)


def _tokens(hp, seed, lens):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, hp["n_vocab"], n).astype(np.int32) for n in lens]


def _alone(G, model, hp, pieces):
    """A twin fed `pieces` alone, each as ONE evaluation on the prompt plan (mmq_min = 9): per piece (logits [N, V], embedding row)."""
    V, E = hp["n_vocab"], hp["n_embd"]
    s = model.start_session(n_batch=192)
    outs = []
    G.set_option("mmq_min", 9)
    try:
        for c in pieces:
            p0 = _stats(G, ("prompt_plan_tokens",))[0]
            s.feed_prompt(c)
            assert _stats(G, ("prompt_plan_tokens",))[0] - p0 == len(c), len(c)  # the prompt plan took it
            emb = s.read_node(-2)
            assert emb.size == len(c) * E
            outs.append((s.read_node(-1).reshape(len(c), V).copy(), emb.reshape(len(c), E)[-1].copy()))
    finally:
        G.set_option("mmq_min", 32)
    return s, outs


ROUND1, ROUND2 = (40, 9, 33, 70, 12, 64), (17, 23, 64, 10, 37, 9)


@pytest.mark.parametrize("cfg,wtype", [("tiny", 2), ("tiny", 7), ("gqa", 2), ("gqa", 7), ("wide", 2), ("wide", 7), ("splitk", 2)])
def test_every_segment_of_nine_rows_or_more_equals_its_session_alone_bit_for_bit(G, cfg, wtype):
    """Two rounds over six sessions: odd and even cache positions, segment boundaries inside a 32-query tile, a 64-token V tile and a
    128-row GEMM tile, key rows crossing 32-key tiles, R (228, 160) no multiple of 32 in round 1."""
    hp, w, model = _mk(cfg, wtype)
    r1, r2 = _tokens(hp, [wtype, len(cfg), 1], ROUND1), _tokens(hp, [wtype, len(cfg), 2], ROUND2)
    sessions = [model.start_session(n_batch=192) for _ in ROUND1]
    got = []
    for pieces in (r1, r2):
        s0 = _stats(G)
        rc, logits, emb = model.prompt_pack(sessions, pieces)
        R = sum(len(c) for c in pieces)
        assert rc == 0 and [b - a for a, b in zip(s0, _stats(G))] == [1, 6, R, R, 0, 0]
        got.append((logits, emb))
    for i, s in enumerate(sessions):
        twin, outs = _alone(G, model, hp, [r1[i], r2[i]])
        for rnd in range(2):
            lg, em = got[rnd][0][i], got[rnd][1][i]
            assert lg.shape == outs[rnd][0].shape
            assert np.array_equal(lg, outs[rnd][0]), (cfg, wtype, i, rnd, float(np.max(np.abs(lg - outs[rnd][0]))))
            assert np.array_equal(em, outs[rnd][1]), (cfg, wtype, i, rnd)
        assert s.n_past == twin.n_past == ROUND1[i] + ROUND2[i]
        for a, b in zip(s.get_kv(), twin.get_kv()):
            assert np.array_equal(a, b), (cfg, wtype, i)
        assert s.snapshot() == twin.snapshot(), (cfg, wtype, i)
        twin.free()
        s.free()
    model.free()


def test_the_raw_entry_takes_staged_graphs(G):
    """ggml_hip_prompt_pack on graphs staged by hand: the K/V rows land although the mirror's bookkeeping never ran."""
    hp, w, model = _mk("tiny", 2)
    a, b = model.start_session(n_batch=192), model.start_session(n_batch=192)
    ta, tb = _tokens(hp, 77, (13, 35))
    s0 = _stats(G)
    assert G.prompt_pack([a.stage_rows(ta), b.stage_rows(tb)]) == 0
    assert [y - x for x, y in zip(s0, _stats(G))] == [1, 2, 48, 48, 0, 0]
    assert a.n_past == 0 and b.n_past == 0
    for s, t in ((a, ta), (b, tb)):
        twin, _ = _alone(G, model, hp, [t])
        for x, y in zip(s.get_kv(), twin.get_kv()):
            assert np.array_equal(x, y)
        twin.free()
        s.free()
    model.free()


SHORT1, SHORT2 = (1, 3, 8, 2, 40, 5), (3, 1, 2, 8, 5, 40)  # round 2: a 1-row segment at the odd n_past 3


@pytest.mark.parametrize("cfg", ["tiny", "gqa"])
def test_short_segments_do_not_depend_on_row0_or_neighbours_and_agree_with_the_oracle(G, O, cfg):
    hp, w, model = _mk(cfg, 2, seed=1234)
    V = hp["n_vocab"]
    r1, r2 = _tokens(hp, [len(cfg), 11], SHORT1), _tokens(hp, [len(cfg), 12], SHORT2)
    x1, x2 = _tokens(hp, [len(cfg), 13], (50, 20))
    A = [model.start_session(n_batch=192) for _ in SHORT1]
    Bs = [model.start_session(n_batch=192) for _ in SHORT1]
    extra = model.start_session(n_batch=192)
    orcs = [O.Llama(hp, w, CTX) for _ in SHORT1]

    def oracle(i, piece, got):
        ref = orcs[i].evaluate(piece, mode=O.ref_mode())
        std = float(ref.std())
        rms = float(np.sqrt(np.mean((got - ref) ** 2))) / std
        assert rms <= 2e-2, (cfg, i, len(piece), rms)
        assert float(np.max(np.abs(got - ref))) / std <= 1e-1, (cfg, i, len(piece))

    # round 1: A in order; B reversed behind a 50-row session
    rc, la, _ = model.prompt_pack(A, r1)
    assert rc == 0
    rc, lb, _ = model.prompt_pack([extra] + Bs[::-1], [x1] + r1[::-1])
    assert rc == 0
    lb = lb[1:][::-1]
    for i in range(6):
        assert np.array_equal(la[i], lb[i]), (cfg, 1, i)
        oracle(i, r1[i], la[i])
        k, v = A[i].get_kv()
        orcs[i].memory_k[:] = k[:orcs[i].memory_k.size]  # (the session's caches have room for n_embd channels; n_embd_gqa are in use)
        orcs[i].memory_v[:] = v[:orcs[i].memory_v.size]
    # round 2: another order again, the extra session in the middle
    order = [2, 0, 5, 1, 3, 4]
    rc, la, _ = model.prompt_pack(A, r2)
    assert rc == 0
    rc, lb2, _ = model.prompt_pack([Bs[j] for j in order[:2]] + [extra] + [Bs[j] for j in order[2:]],
                                   [r2[j] for j in order[:2]] + [x2] + [r2[j] for j in order[2:]])
    assert rc == 0
    lb2 = lb2[:2] + lb2[3:]
    for pos, j in enumerate(order):
        assert np.array_equal(la[j], lb2[pos]), (cfg, 2, j)
    for i in range(6):
        assert la[i].shape == (SHORT2[i], V)
        oracle(i, r2[i], la[i])
        for a, b in zip(A[i].get_kv(), Bs[i].get_kv()):
            assert np.array_equal(a, b), (cfg, i)
        assert A[i].snapshot() == Bs[i].snapshot()
    for s in A + Bs + [extra]:
        s.free()
    model.free()


def _canary(hp):
    n = hp["n_layer"] * CTX * hp["n_embd"]  # (the caches have room for n_embd channels; the layers use n_embd_gqa each, back to back)
    return (0x2C00 + (np.arange(n, dtype=np.int64) * 7 % 1021)).astype(np.uint16)  # finite f16 values around 0.06 .. 0.12


def _outside_is_canary(hp, s, can, n_past, N):
    L, E = hp["n_layer"], hp["n_embd"] // hp["n_head"] * hp["n_head_kv"]
    k, v = s.get_kv()
    used = L * CTX * E
    assert np.array_equal(k[used:], can[used:]) and np.array_equal(v[used:], can[used:])
    k, ck = k[:used].reshape(L, CTX, E), can[:used].reshape(L, CTX, E)
    v, cv = v[:used].reshape(L, E, CTX), can[:used].reshape(L, E, CTX)  # V lies transposed: a row per channel
    keep = np.ones(CTX, bool)
    keep[n_past:n_past + N] = False
    assert np.array_equal(k[:, keep, :], ck[:, keep, :]) and np.array_equal(v[:, :, keep], cv[:, :, keep])
    if N:
        assert not np.array_equal(k[:, ~keep, :], ck[:, ~keep, :]) and not np.array_equal(v[:, :, ~keep], cv[:, :, ~keep])


def test_nothing_outside_the_segments_rows_is_touched(G):
    hp, w, model = _mk("gqa", 2)
    can = _canary(hp)
    starts = (0, 7, 64, 33, 129, 2)
    pieces = _tokens(hp, 21, ROUND1)
    sessions = [model.start_session(n_batch=192) for _ in ROUND1]
    for s, p in zip(sessions, starts):
        s.set_kv(can, can)
        s.seek(p)
    seventh = model.start_session(n_batch=192)
    seventh.feed_prompt(_tokens(hp, 22, (12,))[0])
    k7, v7 = seventh.get_kv()
    l7 = seventh.last_logits()
    rc, _, _ = model.prompt_pack(sessions, pieces)
    assert rc == 0
    for s, p, n in zip(sessions, starts, ROUND1):
        _outside_is_canary(hp, s, can, p, n)
        assert s.n_past == p + n
    k, v = seventh.get_kv()
    assert np.array_equal(k, k7) and np.array_equal(v, v7) and np.array_equal(seventh.last_logits(), l7)
    for s in sessions + [seventh]:
        s.free()
    model.free()


def _q4k_model(G, O):
    from llm_amd import llama, synth
    hp = dict(n_vocab=256, n_embd=256, n_head=4, n_head_kv=4, n_layer=2, n_rot=64, n_ff=512, n_mult=32)
    rng = np.random.default_rng(12)
    w = {}
    for name, (ne0, ne1) in synth.tensor_shapes(hp).items():
        w[name] = ((1.0 + 0.01 * rng.standard_normal(ne0)).astype(np.float32) if ne1 is None else
                   O.quantize(G.TYPE_Q4_K, (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32)))
    hp["wtype"] = G.TYPE_Q4_K
    return hp, llama.Llama(hp, w, context_size=CTX)


def _declined(G, hp, call, sessions):
    """`call` answers -1; the sessions' caches (canary) and the counters are as before."""
    can = _canary(hp)
    for s in sessions:
        s.set_kv(can, can)
    s0 = _stats(G)
    assert call() == -1
    assert _stats(G) == s0
    for s in sessions:
        _outside_is_canary(hp, s, can, 0, 0)
        assert s.n_past == 0


def _stepped_equals_feed_prompt(G, model, hp, lens=(40, 9, 3)):
    """feed_prompt_batch answers 0 and leaves what feed_prompt alone leaves."""
    pieces = _tokens(hp, 31, lens)
    ss = [model.start_session(n_batch=8) for _ in lens]
    s0 = _stats(G, COUNTERS[:3])
    assert model.feed_prompt_batch(ss, pieces) == 0
    assert _stats(G, COUNTERS[:3]) == s0
    for s, c in zip(ss, pieces):
        twin = model.start_session(n_batch=8)
        twin.feed_prompt(c)
        assert np.array_equal(s.last_logits(), twin.last_logits())
        for a, b in zip(s.get_kv(), twin.get_kv()):
            assert np.array_equal(a, b)
        assert s.snapshot() == twin.snapshot()
        twin.free()
        s.free()


@pytest.mark.parametrize("why", ["twice", "two_models", "q4_k", "f16", "plan_prompt_pack", "attn_fused", "context"])
def test_a_declined_pack_leaves_no_trace(G, O, why):
    from llm_amd import llama, synth
    other = None
    if why == "q4_k":
        hp, model = _q4k_model(G, O)
    elif why == "f16":
        hp, w = synth.make_llama(synth.TINY, 1, seed=31)
        model = llama.Llama(hp, w, context_size=CTX)
    else:
        hp, w, model = _mk("tiny", 2)
    a, b = model.start_session(n_batch=192), model.start_session(n_batch=192)
    ta, tb = _tokens(hp, 41, (20, 11))
    try:
        if why == "twice":
            _declined(G, hp, lambda: G.prompt_pack([a.stage_rows(ta), a.stage_rows(tb)]), [a, b])
            with pytest.raises(ValueError):
                model.feed_prompt_batch([a, a], [ta, tb])
        elif why == "two_models":
            hp2, w2, other = _mk("tiny", 2, seed=6)
            c = other.start_session(n_batch=192)
            _declined(G, hp, lambda: G.prompt_pack([a.stage_rows(ta), c.stage_rows(tb)]), [a, c])
            with pytest.raises(ValueError):
                model.feed_prompt_batch([a, c], [ta, tb])
            c.free()
        elif why == "context":
            b.seek(CTX - 5)
            can = _canary(hp)
            b.set_kv(can, can)
            s0 = _stats(G)
            assert model.prompt_pack([a, b], [ta, tb])[0] == -1 and _stats(G) == s0
            _outside_is_canary(hp, b, can, 0, 0)
            assert (a.n_past, b.n_past) == (0, CTX - 5)
            with pytest.raises(ValueError):
                model.feed_prompt_batch([a, b], [ta, tb])
        else:
            if why in ("plan_prompt_pack", "attn_fused"):
                G.set_option(why, 0)
            _declined(G, hp, lambda: model.prompt_pack([a, b], [ta, tb])[0], [a, b])
            _declined(G, hp, lambda: G.prompt_pack([a.stage_rows(ta), b.stage_rows(tb)]), [a, b])
            _stepped_equals_feed_prompt(G, model, hp)
    finally:
        G.set_option("plan_prompt_pack", 1)
        G.set_option("attn_fused", 1)
        a.free()
        b.free()
        model.free()
        if other:
            other.free()


def test_feed_prompt_batch_runs_the_rounds_of_the_schedule_and_every_session_equals_its_twin(G):
    from llm_amd import llama
    hp, w, model = _mk("tiny", 2)
    counts, max_rows = (70, 9, 33, 120, 12), 96
    prompts = _tokens(hp, 51, counts)
    c = np.array(counts, np.int32)
    L = llama._lib()
    rounds = L.llm_pack_schedule(c.ctypes.data, len(c), max_rows, None)
    take = np.zeros((rounds, len(c)), np.int32)
    L.llm_pack_schedule(c.ctypes.data, len(c), max_rows, take.ctypes.data)
    assert rounds == 3 and take.tolist() == [[70, 9, 17, 0, 0], [0, 0, 16, 80, 0], [0, 0, 0, 40, 12]]  # the 120-token prompt spans two, the 33 two
    sessions = [model.start_session(n_batch=192) for _ in counts]  # (n_batch is not consulted: no round has 192 rows of one session)
    s0 = _stats(G)
    assert model.feed_prompt_batch(sessions, prompts, max_rows=max_rows) == 1
    assert [b - a for a, b in zip(s0, _stats(G))] == [rounds, int((take > 0).sum()), sum(counts), sum(counts), 0, 0]
    twins = []
    for i, s in enumerate(sessions):
        pieces, at = [], 0
        for r in range(rounds):
            if take[r, i]:
                pieces.append(prompts[i][at:at + take[r, i]])
                at += take[r, i]
        assert all(len(p) >= 9 for p in pieces)
        twin, _ = _alone(G, model, hp, pieces)
        assert s.n_past == twin.n_past == counts[i]
        assert np.array_equal(s.last_logits(), twin.last_logits()), i
        for a, b in zip(s.get_kv(), twin.get_kv()):
            assert np.array_equal(a, b), i
        assert s.snapshot() == twin.snapshot(), i
        twins.append(twin)
    reqs = [dict(max_tokens=6) for _ in counts]
    ids_a, n_a, why_a, _ = model.infer_until_pool(sessions, reqs, None, max_cols=4)
    ids_b, n_b, why_b, _ = model.infer_until_pool(twins, reqs, None, max_cols=4)
    assert [list(x) for x in ids_a] == [list(x) for x in ids_b] and list(n_a) == list(n_b) and why_a == why_b
    for s in sessions + twins:
        s.free()
    model.free()
