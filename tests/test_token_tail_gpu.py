"""Greedy decode one token ahead of its caller: k_token_tail as the last launch of a token's graph (argmax, the next replay's
parameters and the results' way into a pinned slot in one kernel), two result sets that swap, a hit that enqueues one graph launch
and one event record.  llm_infer_next_token_greedy arms it for its session (ggml_hip_expect_greedy_next), option speculate_next
arms it for an unchanged caller; option token_tail = 0 switches it off.  Every case here is held against the same calls with it
off: ids equal, logits and embedding rows bit-identical for every token."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CTX = 256


def _stat(G, key):
    return int(G.lib().ggml_hip_get_stat(key.encode()))


@pytest.fixture(scope="module")
def model(G):
    from llm_amd import ggml, llama, synth
    hp, w = synth.make_llama_fast(synth.TINY, ggml.TYPE_Q4_0, seed=77)
    m = llama.Llama(hp, w, context_size=CTX)
    yield m
    G.set_option("token_tail", 1)
    G.set_option("speculate_next", 0)
    m.free()


def _prompt(model, seed, n=12):
    return np.random.default_rng(seed).integers(0, model.hp["n_vocab"], n).astype(np.int32)


def _seen(s):
    """what the caller holds after a token: the logits and the embedding row in the nodes' HOST memory"""
    return s.last_logits(), s.read_node_host(1)


def _walk(model, toks, script, hook=None):
    """script: ('greedy', n) = infer_next_token | ('argmax', n) = the unchanged sequence: evaluate(argmax of the last logits) |
    ('token', id) | ('rewind', n); returns (id, logits, embedding row) per evaluated token"""
    s = model.start_session(n_batch=8)
    s.feed_prompt(toks)
    out = []
    for op, arg in script:
        if op == "greedy":
            for _ in range(arg):
                t = s.infer_next_token()
                out.append((t,) + _seen(s))
                if hook:
                    hook(s, out)
        elif op == "argmax":
            for _ in range(arg):
                t = int(np.argmax(s.last_logits()))
                lg = s.evaluate(np.array([t], np.int32))[-1].copy()
                assert np.array_equal(lg, s.last_logits())
                out.append((t,) + _seen(s))
                if hook:
                    hook(s, out)
        elif op == "token":
            s.evaluate(np.array([arg], np.int32))
            out.append((arg,) + _seen(s))
        elif op == "rewind":
            assert s.rewind(arg) == 0
    s.free()
    return out


def _same(ref, got):
    assert len(ref) == len(got)
    for i, ((ta, la, ea), (tb, lb, eb)) in enumerate(zip(ref, got)):
        assert ta == tb, i
        assert np.array_equal(la, lb), i
        assert np.array_equal(ea, eb), i


def _off_on(G, fn, speculate_next=0):
    """fn() with the feature off, then on"""
    try:
        G.set_option("speculate_next", 0)
        G.set_option("token_tail", 0)
        t0 = _stat(G, "tail_tokens")
        ref = fn()
        assert _stat(G, "tail_tokens") == t0  # off is off
        G.set_option("token_tail", 1)
        G.set_option("speculate_next", speculate_next)
        got = fn()
    finally:
        G.set_option("speculate_next", 0)
        G.set_option("token_tail", 1)
    return ref, got


def test_24_greedy_tokens_and_the_steady_state(G, model):
    toks = _prompt(model, 1)
    marks = []

    def hook(s, out):
        marks.append((_stat(G, "result_copies"), _stat(G, "tail_tokens"), _stat(G, "tail_hits")))

    ref, got = _off_on(G, lambda: (marks.clear(), _walk(model, toks, [("greedy", 24)], hook))[1])
    _same(ref, got)
    assert len(marks) == 24  # (of the run with the feature on)
    # after the first two tokens: no stream copy for parameters or results, one slot delivery per token
    assert marks[-1][0] == marks[1][0], marks
    assert [b[1] - a[1] for a, b in zip(marks[1:], marks[2:])] == [1] * 22
    assert [b[2] - a[2] for a, b in zip(marks[1:], marks[2:])] == [1] * 22  # every token is a hit (tail_hits: spec_hits are the option's)


def test_the_unchanged_caller_under_speculate_next(G, model):
    toks = _prompt(model, 2)
    marks = []

    def hook(s, out):
        marks.append((_stat(G, "result_copies"), _stat(G, "tail_tokens"), _stat(G, "spec_hits")))

    ref, got = _off_on(G, lambda: (marks.clear(), _walk(model, toks, [("argmax", 24)], hook))[1], speculate_next=1)
    _same(ref, got)
    assert marks[-1][0] == marks[1][0], marks
    assert [b[1] - a[1] for a, b in zip(marks[1:], marks[2:])] == [1] * 22
    assert [b[2] - a[2] for a, b in zip(marks[1:], marks[2:])] == [1] * 22  # every token is a hit
    # ... and the same ids and logits as the greedy entry point gives
    G.set_option("token_tail", 0)
    try:
        _same(ref, _walk(model, toks, [("greedy", 24)]))
    finally:
        G.set_option("token_tail", 1)


def test_a_miss_then_hits_again_after_the_cool_down(G, model):
    toks = _prompt(model, 3)
    probe = _walk(model, toks, [("greedy", 7)])
    other = (probe[6][0] + 1) % model.hp["n_vocab"]  # not the argmax after six greedy tokens
    script = [("argmax", 6), ("token", other), ("argmax", 14)]
    marks = []

    def hook(s, out):
        marks.append((len(out), _stat(G, "spec_hits"), _stat(G, "spec_misses")))

    ref, got = _off_on(G, lambda: (marks.clear(), _walk(model, toks, script, hook))[1], speculate_next=1)
    _same(ref, got)
    by_n = {n: (h, m) for n, h, m in marks}
    assert by_n[8][1] - by_n[6][1] == 1 and by_n[21][1] == by_n[8][1]  # one miss: the forced token
    # the guessing pauses: the miss and the seven evaluations behind it run nothing ahead, the eighth does, from the ninth on every token hits
    assert by_n[14][0] == by_n[8][0]
    assert by_n[21][0] - by_n[14][0] == 7


def test_a_miss_of_a_caller_that_announced_itself(G, model):
    """the default path: armed by llm_infer_next_token_greedy's hint alone, a forced token in between"""
    toks = _prompt(model, 13)
    probe = _walk(model, toks, [("greedy", 7)])
    other = (probe[6][0] + 1) % model.hp["n_vocab"]
    script = [("greedy", 6), ("token", other), ("greedy", 14)]
    marks = []

    def run():
        marks.clear()
        marks.append((_stat(G, "tail_hits"), _stat(G, "tail_misses"), _stat(G, "spec_hits"), _stat(G, "spec_misses")))
        out = _walk(model, toks, script)
        marks.append((_stat(G, "tail_hits"), _stat(G, "tail_misses"), _stat(G, "spec_hits"), _stat(G, "spec_misses")))
        return out

    ref, got = _off_on(G, run)
    _same(ref, got)
    d = [b - a for a, b in zip(*marks)]
    # hits: tokens 2..6, and the last seven (the miss and the six evaluations behind it arm nothing, the seventh runs ahead again,
    # from the eighth on every token hits); one miss; the option's own books do not move
    assert d == [5 + 7, 1, 0, 0], d


def test_rewind_after_hits(G, model):
    toks = _prompt(model, 4)
    script = [("greedy", 8), ("rewind", 3), ("greedy", 6)]
    ref, got = _off_on(G, lambda: _walk(model, toks, script))
    _same(ref, got)


def test_the_caches_hold_what_a_session_that_never_ran_ahead_holds(G, model):
    """the token that ran ahead wrote the K/V rows of a position its session has not reached: a read from outside, and a miss,
    take them back (k_kv_row_save / k_kv_row_restore) — the WHOLE caches are equal, not only the rows reached"""
    toks = _prompt(model, 10)
    probe = _walk(model, toks, [("greedy", 7)])
    other = (probe[6][0] + 1) % model.hp["n_vocab"]

    def run():
        s = model.start_session(n_batch=8)
        s.feed_prompt(toks)
        kv = []
        for _ in range(6):
            s.infer_next_token()
        kv += list(s.get_kv())  # with the device one token ahead
        s.infer_next_token()
        s.evaluate(np.array([other], np.int32))  # a miss at the position the ahead run wrote
        kv += list(s.get_kv())
        for _ in range(3):
            s.infer_next_token()
        assert s.rewind(2) == 0
        kv += list(s.get_kv())
        s.free()
        return kv

    ref, got = _off_on(G, run)
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)


def test_a_session_freed_with_a_token_in_flight_delivers_nothing_stale(G, model):
    ta, tb = _prompt(model, 5), _prompt(model, 6)

    def run():
        a = _walk(model, ta, [("greedy", 5)])  # (freed with the device one token ahead)
        b = _walk(model, tb, [("greedy", 7)])
        return a + b

    ref, got = _off_on(G, run)
    _same(ref, got)


def test_two_sessions_alternating_on_one_slot(G, model):
    prompts = [_prompt(model, 7), _prompt(model, 8)]

    def run():
        ss = [model.start_session(n_batch=8) for _ in range(2)]
        for s, t in zip(ss, prompts):
            s.feed_prompt(t)
        out = []
        for i in range(16):
            s = ss[i % 2] if i < 10 else ss[1]
            out.append((s.infer_next_token(),) + _seen(s))
        for s in ss:
            s.free()
        return out

    ref, got = _off_on(G, run)
    _same(ref, got)


def test_device_side_readers_of_a_session_another_one_has_overtaken(G, model):
    """A hits (its last token sits in result set 1, the run ahead of it has written set 0), B evaluates on the same slot: A's top-k
    and A's nodes read on the device are still A's last evaluated token"""
    a, b = model.start_session(n_batch=8), model.start_session(n_batch=8)
    try:
        a.feed_prompt(_prompt(model, 14))
        b.feed_prompt(_prompt(model, 15))
        for n_a in (10, 11, 10):  # (long enough to hit again behind the pause B's miss causes; A's last token in either set)
            h0 = _stat(G, "tail_hits")
            for _ in range(n_a):
                a.infer_next_token()
            assert _stat(G, "tail_hits") - h0 >= 4
            lg, emb = _seen(a)
            b.infer_next_token()
            b.evaluate(np.array([5, 6, 7], np.int32))
            vals, ids = a.top_k(5)
            order = np.lexsort((np.arange(lg.size), -lg))[:5]
            assert np.array_equal(ids, order.astype(np.int32)) and np.array_equal(vals, lg[order])
            n = a.graph_stats()[0]
            assert np.array_equal(a.read_node(index=n - 1)[-lg.size:], lg)
            assert np.array_equal(a.read_node(index=n - 2), emb)
    finally:
        a.free()
        b.free()


@pytest.mark.parametrize("option", ["plan", "plan_multi"])
def test_a_chunk_run_node_by_node_behind_an_ahead_run(G, model, option):
    """greedy tokens, then a chunk the plans do not take (it runs node by node and writes the cache rows the ahead run wrote),
    then a token: the ahead run is taken back BEFORE the chunk, never over it — whole caches, ids and logits equal"""
    toks = _prompt(model, 16)

    def run():
        s = model.start_session(n_batch=16)
        s.feed_prompt(toks)
        out = []
        for _ in range(5):
            out.append((s.infer_next_token(),) + _seen(s))
        if option == "plan":  # (no plan is dropped by this one: the ahead run is still pending when the chunk comes)
            G.set_option("plan", 0)
        else:
            G.set_option("plan_multi", 0)
        try:
            s.evaluate(np.arange(10, 22, dtype=np.int32))
        finally:
            G.set_option(option, 1)
        out.append((-1,) + _seen(s))
        for _ in range(3):
            out.append((s.infer_next_token(),) + _seen(s))
        kv = s.get_kv()
        s.free()
        return out, kv

    (ref, kv0), (got, kv1) = _off_on(G, run)
    _same(ref, got)
    assert np.array_equal(kv0[0], kv1[0]) and np.array_equal(kv0[1], kv1[1])


def test_device_side_readers_directly_after_a_hit(G, model):
    toks = _prompt(model, 9)
    s = model.start_session(n_batch=8)
    try:
        s.feed_prompt(toks)
        for i in range(10):
            c0, t0 = _stat(G, "result_copies"), _stat(G, "tail_tokens")
            s.infer_next_token()
            hit = _stat(G, "result_copies") == c0 and _stat(G, "tail_tokens") == t0 + 1
            assert hit == (i >= 1), i
            lg, emb = _seen(s)
            vals, ids = s.top_k(5)
            order = np.lexsort((np.arange(lg.size), -lg))[:5]
            assert np.array_equal(ids, order.astype(np.int32)) and np.array_equal(vals, lg[order]), i
            n = s.graph_stats()[0]
            assert np.array_equal(s.read_node(index=n - 1)[-lg.size:], lg), i
            assert np.array_equal(s.read_node(index=n - 2), emb), i
    finally:
        s.free()


# ---- op level: k_token_tail alone, beside k_argmax_next ----
def _tail(G, logits, emb, misalign=0, n_past=41):
    V = logits.size
    ia, ib, prm = C.c_int32(-1), C.c_int32(-1), np.zeros(3, np.int32)
    sl = np.zeros(V, np.float32)
    se = np.zeros(emb.size, np.float32)
    rc = G.lib().ggml_hip_debug_token_tail(logits.ctypes.data, V, emb.ctypes.data, emb.size, n_past, misalign, C.byref(ia), C.byref(ib),
                                           sl.ctypes.data, se.ctypes.data, prm.ctypes.data)
    assert rc == 0
    return ia.value, ib.value, sl, se, prm


def _op_cases():
    rng = np.random.default_rng(11)
    cases = []
    for V in (1, 3, 1000, 32000, 32001):
        x = rng.standard_normal(V).astype(np.float32)
        cases.append((f"random-{V}", x))
        t = x.copy()
        t[0] = t[V - 1] = np.float32(9.0)
        cases.append((f"tie-first-last-{V}", t))
        if V & 3:
            g = x.copy()
            g[V - 1] = np.float32(11.0)
            cases.append((f"max-in-last-partial-group-{V}", g))
        cases.append((f"all-equal-{V}", np.full(V, np.float32(-0.5))))
    return cases


@pytest.mark.parametrize("name,logits", _op_cases(), ids=[c[0] for c in _op_cases()])
def test_k_token_tail_alone(G, name, logits):
    emb = np.random.default_rng(12).standard_normal(128).astype(np.float32)
    want = int(np.argmax(logits))  # the first maximum
    for misalign in (0, 1):
        it, ia, sl, se, prm = _tail(G, logits, emb, misalign)
        assert it == ia == want, (misalign, it, ia, want)
        assert sl.tobytes() == logits.tobytes() and se.tobytes() == emb.tobytes(), misalign
        assert prm.tolist() == [42, want, want], misalign  # (misalign moves the embedding row too: the kernel's 4-byte row path)
