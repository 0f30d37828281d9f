"""A greedy token's k_token_tail prepares the next token (option tail_prepare): the embedding row, the RoPE table and the granule
epoch, the saved cache rows — so that the graph launched directly behind it opens with its layer-0 launch.  The kernel alone is held
against k_get_rows_q, k_rope_table and k_kv_row_save on the same inputs (ggml_hip_debug_token_tail_prepare); whole sessions are
held against the same calls with the option off (every greedy token's graph then opens with those three launches): ids equal,
logits, caches and snapshots bit-identical."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CTX = 256
L, E, V, D = 2, 128, 256, 32  # synth.TINY: layers, width (= the K/V width: no GQA), vocabulary, head size


def _stat(G, key):
    return int(G.lib().ggml_hip_get_stat(key.encode()))


STATS = ("tail_hits", "tail_misses", "tail_prepared_tokens", "tail_tokens", "attn_split_tokens")


def _stats(G):
    return np.array([_stat(G, k) for k in STATS], np.int64)


@pytest.fixture(scope="module")
def model(G):
    from llm_amd import ggml, llama, synth
    hp, w = synth.make_llama_fast(synth.TINY, ggml.TYPE_Q4_0, seed=78)
    m = llama.Llama(hp, w, context_size=CTX)
    yield m
    for k in ("token_tail", "tail_prepare", "attn_split"):
        G.set_option(k, 1)
    m.free()


def _prompt(seed, n=12):
    return np.random.default_rng(seed).integers(0, V, n).astype(np.int32)


def _settle(model):
    """nine evaluations nobody announced as greedy: whatever pause a miss of an earlier test left behind (eight evaluations) is over,
    so the counters of the run that follows do not depend on what ran before it"""
    s = model.start_session(n_batch=8)
    for t in range(9):
        s.evaluate(np.array([t], np.int32))
    s.free()


def _off_on(G, model, fn, off=("tail_prepare", 0)):
    """fn() with `off` set, then with the defaults; each returns (result, the counters' movement)"""
    runs = []
    try:
        for key, val in (off, (off[0], 1)):
            G.set_option(key, val)
            _settle(model)
            s0 = _stats(G)
            r = fn()
            runs.append((r, dict(zip(STATS, (_stats(G) - s0).tolist()))))
    finally:
        G.set_option(off[0], 1)
    return runs


def _same(ref, got):
    assert len(ref) == len(got)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a[0] == b[0], i
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x, y), i


# ---- 1. the kernel alone ----
@pytest.fixture(scope="module")
def op_inputs():
    rng = np.random.default_rng(21)
    return dict(wte=rng.standard_normal((V, E)).astype(np.float32),
                mem_k=rng.integers(0, 1 << 16, L * CTX * E, dtype=np.uint16), mem_v=rng.integers(0, 1 << 16, L * E * CTX, dtype=np.uint16),
                noise=rng.standard_normal(V).astype(np.float32))


def _prepare(G, inp, raw, wtype, logits, n_past, epoch_in, parity, zeroed=0):
    i32, u32, f32, u16 = np.int32, np.uint32, np.float32, np.uint16
    o = dict(id=np.full(1, -1, i32), prm=np.zeros(5, i32))
    for sfx in ("", "_ref"):
        o["row" + sfx], o["table" + sfx], o["epoch" + sfx], o["save" + sfx] = np.zeros(E, f32), np.zeros(128, f32), np.zeros(1, u32), np.zeros(2 * L * E, u16)
    p = lambda a: a.ctypes.data
    rc = G.lib().ggml_hip_debug_token_tail_prepare(
        p(logits), V, p(raw), wtype, E, n_past, epoch_in, parity, zeroed, L, CTX, E, p(inp["mem_k"]), p(inp["mem_v"]),
        float(np.float32(10000.0) ** np.float32(-2.0 / D)), 1.0, D // 2, p(o["id"]), p(o["prm"]), p(o["row"]), p(o["table"]), p(o["epoch"]),
        p(o["save"]), p(o["row_ref"]), p(o["table_ref"]), p(o["epoch_ref"]), p(o["save_ref"]))
    assert rc == 0
    return o


def _bits(a):
    return a.view(np.uint8)


@pytest.mark.parametrize("tname", ["Q4_0", "Q4_1", "Q5_0", "Q5_1", "Q8_0"])
def test_the_tail_prepares_what_the_three_launches_make(G, op_inputs, tname):
    wtype = getattr(G, "TYPE_" + tname)
    raw = G.quantize(wtype, op_inputs["wte"])
    ids = {}
    ids["row-0"] = op_inputs["noise"].copy()
    ids["row-0"][0] = 9.0
    ids["last-row"] = op_inputs["noise"].copy()
    ids["last-row"][V - 1] = 9.0
    ids["first-of-two-maxima"] = op_inputs["noise"].copy()
    ids["first-of-two-maxima"][[77, 201]] = 9.0
    want = {"row-0": 0, "last-row": V - 1, "first-of-two-maxima": 77}
    n = 0
    for n_past in (0, 1, CTX - 3):
        for name, logits in ids.items():
            parity, epoch_in = n & 1, (0xFFFFFFFF if n == 4 else 7 + n)
            n += 1
            o = _prepare(G, op_inputs, raw, wtype, logits, n_past, epoch_in, parity)
            tag = (tname, n_past, name)
            assert int(o["id"][0]) == want[name], tag
            assert np.array_equal(_bits(o["row"]), _bits(o["row_ref"])), tag
            assert np.array_equal(_bits(o["table"]), _bits(o["table_ref"])), tag  # (the canary behind the D / 2 pairs included)
            assert np.isfinite(o["table"][:D]).all() and (_bits(o["table"][D:]) == 0xFF).all(), tag
            assert np.array_equal(o["save"], o["save_ref"]), tag
            # ... which is the K row and the V column of position n_past + 1, every layer
            k = op_inputs["mem_k"].reshape(L, CTX, E)[:, n_past + 1, :].reshape(-1)
            v = op_inputs["mem_v"].reshape(L, E, CTX)[:, :, n_past + 1].reshape(-1)
            assert np.array_equal(o["save"], np.concatenate([k, v])), tag
            assert int(o["epoch"][0]) == int(o["epoch_ref"][0]) == (1 if epoch_in == 0xFFFFFFFF else epoch_in + 1), tag
            pos_tail = [n_past, n_past]
            pos_tail[parity ^ 1] = n_past + 1  # its own word is read, the other parity's written
            assert o["prm"].tolist() == [n_past + 1, want[name], want[name]] + pos_tail, tag
    # a zeroed struct: the launch writes none of it (every buffer keeps its canary, the epoch and both position words stand)
    o = _prepare(G, op_inputs, raw, wtype, ids["last-row"], 5, 41, 0, zeroed=1)
    assert int(o["id"][0]) == V - 1 and o["prm"].tolist() == [6, V - 1, V - 1, 5, 5]
    for key in ("row", "table", "save"):
        assert (_bits(o[key]) == 0xFF).all(), key
    assert int(o["epoch"][0]) == 41 and int(o["epoch_ref"][0]) == 42


# ---- 2. greedy runs ----
def _greedy(model, toks, n):
    s = model.start_session(n_batch=8)
    s.feed_prompt(toks)
    out = []
    for _ in range(n):
        t = s.infer_next_token()
        out.append((t, s.last_logits()))
    snap = s.snapshot()
    s.free()
    return out, snap


@pytest.mark.parametrize("split_from", [1, 30])
def test_40_greedy_tokens_with_and_without(G, model, split_from):
    """split_from 30: option attn_split moves the change of the attention variant (one workgroup per head -> the position-split
    attention) to 30 positions, so the run crosses it at its 18th token — an ahead graph of one variant directly behind a tail graph
    of the other; with the default (768 positions) a context of 256 never crosses."""
    toks = _prompt(31)
    try:
        G.set_option("attn_split", split_from)
        ((ref, snap0), d0), ((got, snap1), d1) = _off_on(G, model, lambda: _greedy(model, toks, 40))
    finally:
        G.set_option("attn_split", 1)
    _same(ref, got)
    assert snap0 == snap1
    assert d0["tail_prepared_tokens"] == 0 and d0["tail_hits"] == 39
    assert d1["tail_prepared_tokens"] == d1["tail_hits"] == 39  # all but the first: no prologue launch
    for d in (d0, d1):
        assert d["attn_split_tokens"] == (0 if split_from == 1 else 12 + 40 - 29)  # positions 29 .. 51 attend over >= 30


# ---- 3. a miss ----
def _stale_rows(s):
    """40 greedy tokens, back by 38, one token that is NOT the one decoded there before: the rows of the positions ahead now hold
    what the first pass left (different from row to row, and different from what this pass will write there), so a cache row put
    back from the wrong save area, or not at all, shows when the whole caches are compared; returns what the caller saw"""
    out = [(s.infer_next_token(), s.last_logits()) for _ in range(40)]
    assert s.rewind(38) == 0
    other = (out[2][0] + 1) % V  # (out[k] was evaluated at position 12 + k: this one sits at 14 again)
    s.evaluate(np.array([other], np.int32))
    out.append((other, s.last_logits()))
    return out


def test_a_miss_takes_the_prepared_run_back(G, model):
    toks = _prompt(32)
    hits = []

    def run():
        s = model.start_session(n_batch=8)
        s.feed_prompt(toks)
        out, kv = _stale_rows(s), []  # (its last evaluation was a miss: the next six arm nothing, the seventh runs ahead, then hits)
        for _ in range(12):
            out.append((s.infer_next_token(), s.last_logits()))
        # a token that is not the first maximum, at the position the ahead run wrote
        other = (int(np.argmax(s.last_logits())) + 1) % V
        s.evaluate(np.array([other], np.int32))
        out.append((other, s.last_logits()))
        kv += s.get_kv()
        h0 = _stat(G, "tail_hits")
        for _ in range(14):
            out.append((s.infer_next_token(), s.last_logits()))
        hits.append(_stat(G, "tail_hits") - h0)
        # ... and a miss somewhere else: the row the ahead run wrote is not written again before the caches are read
        assert s.rewind(3) == 0
        s.evaluate(np.array([other], np.int32))
        out.append((other, s.last_logits()))
        kv += s.get_kv()
        s.free()
        return out, kv

    ((ref, kv0), d0), ((got, kv1), d1) = _off_on(G, model, run, off=("token_tail", 0))  # against a session that never ran ahead
    _same(ref, got)
    for a, b in zip(kv0, kv1):
        assert np.array_equal(a, b)
    assert d0["tail_tokens"] == 0 and hits[0] == 0
    # behind a miss: it and the six evaluations behind it arm nothing, the seventh runs ahead again, from the eighth on every token hits
    assert hits[1] == 7
    assert d1["tail_misses"] == 3 and d1["tail_prepared_tokens"] == d1["tail_hits"] == 39 + 5 + 7, d1


# ---- 4. something overtakes the prepared run ----
@pytest.mark.parametrize("what", ["chunk", "rewind", "second-session", "kv-read"])
def test_between_two_greedy_tokens(G, model, what):
    toks, toks_b = _prompt(33), _prompt(34)

    def run():
        s = model.start_session(n_batch=8)
        s.feed_prompt(toks)
        b = model.start_session(n_batch=8) if what == "second-session" else None
        if b:
            b.feed_prompt(toks_b)
        out, extra = _stale_rows(s), []
        for i in range(24):
            out.append((s.infer_next_token(), s.last_logits()))
            if i % 12 != 11:  # (after tokens 12 and 24: hits have come back in between, a run ahead is pending)
                continue
            if what == "chunk":
                s.feed_prompt(np.arange(40 + i, 45 + i, dtype=np.int32))
                extra.append(s.last_logits())
            elif what == "rewind":
                assert s.rewind(2) == 0
            elif what == "second-session":
                extra.append(np.array([b.infer_next_token()]))
                extra.append(b.last_logits())
            extra += s.get_kv()
        extra.append(np.frombuffer(s.snapshot(), np.uint8))
        s.free()
        if b:
            extra += b.get_kv()
            b.free()
        return out, extra

    ((ref, x0), d0), ((got, x1), d1) = _off_on(G, model, run)
    _same(ref, got)
    assert len(x0) == len(x1)
    for a, b in zip(x0, x1):
        assert np.array_equal(a, b)
    assert d0["tail_prepared_tokens"] == 0
    assert d1["tail_hits"] == d0["tail_hits"] and d1["tail_misses"] == d0["tail_misses"]
    assert d1["tail_prepared_tokens"] == d1["tail_hits"] >= 39 + 5


# ---- 5. the end of the context ----
def test_greedy_up_to_the_last_position(G, model):
    toks = _prompt(35, 200)

    def run():
        s = model.start_session(n_batch=8)
        s.feed_prompt(toks)
        out = []
        while s.n_past + 1 < CTX:  # (behind that the session answers ContextFull, as the reference does)
            out.append((s.infer_next_token(), s.last_logits()))
        assert len(out) == CTX - 1 - 200
        s.free()
        return out

    (ref, d0), (got, d1) = _off_on(G, model, run)
    _same(ref, got)
    assert d1["tail_prepared_tokens"] == d1["tail_hits"] == d0["tail_hits"] > 40  # (the last positions have no next token to run ahead)


# ---- 6. a plan that keeps its prologue ----
def test_an_f16_model_keeps_its_prologue(G):
    from llm_amd import ggml, llama, synth
    hp, w = synth.make_llama(synth.TINY, ggml.TYPE_F16, seed=36)
    m = llama.Llama(hp, w, context_size=CTX)
    try:
        ((ref, snap0), d0), ((got, snap1), d1) = _off_on(G, m, lambda: _greedy(m, _prompt(37), 16))
    finally:
        m.free()
    _same(ref, got)
    assert snap0 == snap1
    assert d0["tail_prepared_tokens"] == d1["tail_prepared_tokens"] == 0
    assert d0["tail_hits"] == d1["tail_hits"] == 15
