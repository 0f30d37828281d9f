"""The F16 plan (plan_decode.inc plan_launch_f16, kernels/decode_f16.h): a LLaMA whose matrices are F16 (file type 1) decoded, fed
in chunks of up to 31 tokens and stepped in batches of sessions as five launches per layer from a captured hipGraph instead of
the node-by-node executor (option plan_f16 = 0: what such a model ran on before).

Shapes: synth.TINY (E = 128: 16 chunks of 16 bytes per row, fewer than lanes; F = 352: a ragged tail; V = 256: fewer rows than
waves) and the GQA2 shape of tests/test_batch_decode_gpu.py (E = 1024, 8 heads over 4 K/V heads, F = 2816), context 64.
Tolerances against the oracle and the executor are those documented at the top of tests/test_llama_gpu.py (STRICT, EDGE,
relative to std(logits)).  Where the kernel's design rule applies — a row's result is a pure function of the row's bytes, the staged
column and K — the comparison is bit for bit: a chunk against the same tokens one by one, a batched step against the chunk."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STRICT, EDGE = 1e-5, 4e-2
GQA2 = dict(n_vocab=512, n_embd=1024, n_head=8, n_head_kv=4, n_layer=2, n_rot=128, n_ff=2816, n_mult=32)
CTX = 64
SENTINEL = 0x5555
F16 = 1
CFGS = ["tiny", "gqa2"]


def _stat(G, key):
    return int(G.lib().ggml_hip_get_stat(key.encode()))


def _hp0(cfg):
    from llm_amd import synth
    return synth.TINY if cfg == "tiny" else GQA2


def _mk(cfg, seed=1234, ctx=CTX, hp0=None):
    from llm_amd import llama, synth
    hp, w = synth.make_llama(hp0 or _hp0(cfg), F16, seed=seed)
    return hp, w, llama.Llama(hp, w, context_size=ctx)


def _feed(sess, toks):
    for i in range(0, len(toks), 8):
        sess.evaluate(toks[i:i + 8], want_all_logits=False)


def _kv3(hp, k, v, ctx=CTX):
    L, Egqa = hp["n_layer"], hp["n_embd"] // (hp["n_head"] // hp["n_head_kv"])
    n = L * ctx * Egqa
    return k[:n].reshape(L, ctx, Egqa), v[:n].reshape(L, Egqa, ctx)


def _rel(a, b):
    return float(np.max(np.abs(a - b))) / float(b.std())


@pytest.mark.parametrize("cfg", CFGS)
def test_the_plan_runs_f16_models_and_the_option_turns_it_off(G, O, cfg):
    """plan_tokens grows by the tokens evaluated for a chunk of 8, a chunk of 13 and a single token; with plan_f16 = 0 it does
    not move and the same logits (EDGE: other kernels) come from the node-by-node executor."""
    hp, w, model = _mk(cfg, seed=3)
    toks = np.random.default_rng(2).integers(0, hp["n_vocab"], 22).astype(np.int32)
    cuts = [(0, 8), (8, 21), (21, 22)]
    outs = {}
    try:
        for on in (1, 0):
            G.set_option("plan_f16", on)
            s = model.start_session(n_batch=16)
            got = []
            for lo, hi in cuts:
                p0, g0 = _stat(G, "plan_tokens"), _stat(G, "generic_graphs")
                got.append(s.evaluate(toks[lo:hi]).copy())
                ran, gen = _stat(G, "plan_tokens") - p0, _stat(G, "generic_graphs") - g0
                assert (ran == hi - lo and gen == 0) if on else (ran == 0 and gen >= 1), (on, lo, hi, ran, gen)
            outs[on] = got
            s.free()
    finally:
        G.set_option("plan_f16", 1)
        model.free()
    for a, b in zip(outs[1], outs[0]):
        assert a.shape == b.shape and _rel(a, b) <= EDGE


@pytest.mark.parametrize("cfg", CFGS)
def test_logits_match_the_oracle_and_the_executor(G, O, cfg):
    """Sessions brought to n_past = 0, 1, 7, 33 and 63 by prompts fed in chunks of 8 (every chunk compared), then one decode step
    each; the oracle evaluates the same tokens on the session's own K/V state.  Every row within EDGE * std(logits); how many
    evaluations meet STRICT is printed.  The same against the executor (plan_f16 = 0)."""
    hp, w, model = _mk(cfg, seed=7)
    rng = np.random.default_rng(11)
    n_eval = n_strict = 0
    worst = worst_x = 0.0
    try:
        for n in (0, 1, 7, 33, 63):
            toks = rng.integers(0, hp["n_vocab"], n + 1).astype(np.int32)
            s, x = model.start_session(n_batch=8), model.start_session(n_batch=8)
            orc = O.Llama(hp, w, CTX)
            cuts = [(i, min(i + 8, n)) for i in range(0, n, 8)] + [(n, n + 1)]
            for lo, hi in cuts:
                k, v = s.get_kv()
                orc.memory_k[:] = k[:orc.memory_k.size]
                orc.memory_v[:] = v[:orc.memory_v.size]
                orc.n_past = lo
                x.set_kv(k, v)
                x.seek(lo)
                p0 = _stat(G, "plan_tokens")
                got = s.evaluate(toks[lo:hi])
                assert _stat(G, "plan_tokens") - p0 == hi - lo
                ref = orc.evaluate(toks[lo:hi], mode=O.ref_mode())
                G.set_option("plan_f16", 0)
                ex = x.evaluate(toks[lo:hi])
                G.set_option("plan_f16", 1)
                for r in range(hi - lo):
                    d, dx = _rel(got[r], ref[r]), _rel(got[r], ex[r])
                    worst, worst_x = max(worst, d), max(worst_x, dx)
                    assert d <= EDGE and dx <= EDGE, (cfg, n, lo, r, d, dx)
                    n_eval += 1
                    n_strict += d <= STRICT
            s.free()
            x.free()
    finally:
        G.set_option("plan_f16", 1)
        model.free()
    print(f"{cfg}: F16 plan vs oracle worst {worst:.2e}, vs executor worst {worst_x:.2e}; {n_strict} of {n_eval} rows within {STRICT}")


@pytest.mark.parametrize("cfg", CFGS)
def test_a_chunk_equals_its_tokens_one_by_one_bit_for_bit(G, O, cfg):
    """One chunk of 8 tokens at n_past = 5 against the same 8 tokens evaluated one by one in a twin session: the logits of every
    column and K and V of every position."""
    hp, w, model = _mk(cfg, seed=5)
    rng = np.random.default_rng(6)
    prompt = rng.integers(0, hp["n_vocab"], 5).astype(np.int32)
    chunk = rng.integers(0, hp["n_vocab"], 8).astype(np.int32)
    a, b = model.start_session(n_batch=8), model.start_session(n_batch=8)
    a.evaluate(prompt, want_all_logits=False)
    ka, va = a.get_kv()
    b.set_kv(ka, va)  # (the same prefix, whichever kernels wrote it)
    b.seek(5)
    p0 = _stat(G, "plan_tokens")
    got = a.evaluate(chunk)
    singles = np.stack([b.evaluate(chunk[i:i + 1])[0] for i in range(8)])
    assert _stat(G, "plan_tokens") - p0 == 16
    assert np.array_equal(got, singles), float(np.max(np.abs(got - singles)))
    ka, va = a.get_kv()
    kb, vb = b.get_kv()
    assert np.array_equal(ka, kb) and np.array_equal(va, vb)
    a.free()
    b.free()
    model.free()


@pytest.mark.parametrize("B", [8, 3])
@pytest.mark.parametrize("cfg", CFGS)
def test_batched_step_equals_the_chunk_bit_for_bit(G, O, cfg, B):
    """The construction of tests/test_batch_decode_gpu.py: two source sessions with prompts of 5 and 23 tokens evaluate a chunk of
    B tokens each; batch column c (s = c mod 2) is a fresh session holding S_s's K/V with every position >= P_s + c overwritten by
    a sentinel, seeked to P_s + c, given token chunk_s[c].  Logits, the written K/V position, the untouched positions below and
    the sentinel above, all bit for bit; batch_decode_steps grows by 1."""
    hp, w, model = _mk(cfg, seed=5)
    rng = np.random.default_rng([F16, B])
    P = (5, 23)
    ref, kv, chunk = [], [], []
    for s in (0, 1):
        src = model.start_session(n_batch=8)
        _feed(src, rng.integers(0, hp["n_vocab"], P[s]).astype(np.int32))
        chunk.append(rng.integers(0, hp["n_vocab"], B).astype(np.int32))
        p0 = _stat(G, "plan_tokens")
        ref.append(src.evaluate(chunk[s]))
        assert _stat(G, "plan_tokens") - p0 == B
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


@pytest.mark.parametrize("cfg", CFGS)
def test_six_batched_steps_replay_one_graph(G, O, cfg):
    """Six steps of four sessions: the step's hipGraph is captured once and replayed, and every step's logits equal the sessions'
    twins decoded alone bit for bit (the same kernel with one column)."""
    hp, w, model = _mk(cfg, seed=9)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(0, hp["n_vocab"], n).astype(np.int32) for n in (3, 9, 14, 20)]
    streams = rng.integers(0, hp["n_vocab"], (4, 6)).astype(np.int32)
    sessions, twins = [], []
    for p in prompts:
        for lst in (sessions, twins):
            f = model.start_session(n_batch=8)
            _feed(f, p)
            lst.append(f)
    s0 = _stat(G, "batch_decode_steps")
    for step in range(6):
        r0, n0 = _stat(G, "graph_replays"), _stat(G, "plans")
        ran, logits = model.evaluate_batch(sessions, streams[:, step])
        assert ran
        if step >= 1:
            assert _stat(G, "graph_replays") - r0 == 1 and _stat(G, "plans") == n0, step
        for c, f in enumerate(sessions):
            assert f.n_past == len(prompts[c]) + step + 1
            assert np.array_equal(twins[c].evaluate(streams[c, step:step + 1])[0], logits[c]), (step, c)
    assert _stat(G, "batch_decode_steps") - s0 == 6
    for f in sessions + twins:
        f.free()
    model.free()


def test_long_context_runs_the_split_attention(G, O):
    """TINY at context 1024: a prompt of 600 tokens, then decode steps beyond the split threshold (option attn_split: 512 here)
    run the position-split attention (k_attn_split_one); every step within EDGE of the oracle on the session's own K/V."""
    ctx = 1024
    hp, w, model = _mk("tiny", seed=57, ctx=ctx)
    toks = np.random.default_rng(31).integers(0, hp["n_vocab"], 608).astype(np.int32)
    G.set_option("attn_split", 512)
    try:
        s = model.start_session(n_batch=8)
        p0 = _stat(G, "plan_tokens")
        s.feed_prompt(toks[:600])
        assert _stat(G, "plan_tokens") - p0 == 600  # chunks of 8 on the F16 plan
        orc = O.Llama(hp, w, ctx)
        b0 = _stat(G, "attn_split_tokens")
        worst = 0.0
        for i in range(600, 606):
            k, v = s.get_kv()
            orc.memory_k[:] = k[:orc.memory_k.size]
            orc.memory_v[:] = v[:orc.memory_v.size]
            orc.n_past = i
            got = s.evaluate(toks[i:i + 1])[0]
            ref = orc.evaluate(toks[i:i + 1], mode=O.ref_mode())[0]
            worst = max(worst, _rel(got, ref))
        split = _stat(G, "attn_split_tokens") - b0
        s.free()
    finally:
        G.set_option("attn_split", 1)
        model.free()
    print(f"long context: F16 plan vs oracle worst |dlogit|/std = {worst:.2e}")
    assert split == 6 and _stat(G, "fused_attn_timeouts") == 0
    assert worst <= EDGE


@pytest.mark.parametrize("cfg", CFGS)
def test_greedy_on_the_device_and_rewind(G, O, cfg):
    """llm_infer_tokens_greedy_device (the greedy chain on the plan) returns the ids of the host greedy loop; rewind(1) and the
    last token again give the same bits."""
    hp, w, model = _mk(cfg, seed=21)
    prompt = np.random.default_rng(8).integers(0, hp["n_vocab"], 9).astype(np.int32)
    a, b = model.start_session(n_batch=8), model.start_session(n_batch=8)
    a.feed_prompt(prompt)
    b.feed_prompt(prompt)
    host = [a.infer_next_token() for _ in range(12)]
    p0 = _stat(G, "plan_tokens")
    dev = list(b.infer_tokens_device(12))  # (one normal step arms the chain, the rest is sampled on the device)
    assert _stat(G, "plan_tokens") - p0 == 12
    assert dev == host
    last = a.last_logits().copy()
    assert a.rewind(1) == 0 and a.n_past == len(prompt) + 11
    again = a.evaluate([host[-1]])[0]  # (the last sampled token is the last one evaluated)
    assert np.array_equal(again, last) and a.n_past == len(prompt) + 12
    a.free()
    b.free()
    model.free()


def test_two_stages_of_a_layer_split_reproduce_the_unsplit_session(G, O):
    """A 4-layer F16 model layer-split over two (virtual) device slots of one process: each stage runs the F16 plan on its own
    layers (the first from get_rows, the second from the hand-off buffer to the lm_head) — logits and K/V bit-identical to the
    unsplit session."""
    from llm_amd import llama, synth
    assert G.lib().ggml_hip_get_main_device() == 0
    hp0 = dict(n_vocab=256, n_embd=256, n_head=4, n_head_kv=4, n_layer=4, n_rot=64, n_ff=512, n_mult=32)
    hp, w = synth.make_llama(hp0, F16, seed=41)
    toks = np.random.default_rng(4).integers(0, hp["n_vocab"], 20).astype(np.int32)

    def run(model):
        sess = model.start_session(n_batch=8)
        p0 = _stat(G, "plan_tokens")
        sess.feed_prompt(toks[:8])
        outs = [sess.evaluate(toks[i:i + 1])[-1].copy() for i in range(8, 20)]
        ran = _stat(G, "plan_tokens") - p0
        k, v = sess.get_kv()
        sess.free()
        return outs, k, v, ran

    whole = llama.Llama(hp, w, context_size=64)
    ref = run(whole)
    whole.free()
    assert ref[3] == 20
    os.environ["GGML_HIP_VIRTUAL_DEVICES"] = "2"
    os.environ["GGML_HIP_LAYER_SPLIT"] = "2"
    try:
        split = llama.Llama(hp, w, context_size=64)
        assert split.stages() == [(0, 2, 0), (2, 4, 1)]
        got = run(split)
        split.free()
    finally:
        os.environ.pop("GGML_HIP_LAYER_SPLIT", None)
        G.lib().ggml_hip_set_layer_split(None, 0)
        G.lib().ggml_hip_set_main_device(0)
        os.environ.pop("GGML_HIP_VIRTUAL_DEVICES", None)
    assert got[3] == 20  # (statistics are per device slot: slot 0's stage ran every token on the plan)
    for a, b in zip(ref[0], got[0]):
        assert np.array_equal(a, b)
    assert np.array_equal(ref[1], got[1]) and np.array_equal(ref[2], got[2])


def test_an_f16_file_loads_and_decodes_on_the_plan(G, O, tmp_path):
    """A GGJT v3 file with F16 tensors (file type 1) through the C++ loader: prompt feed at n_batch = 8 and greedy decode on the
    F16 plan, bit-identical to the same weights handed over in memory."""
    from llm_amd import llama, synth
    hp0 = dict(n_vocab=256, n_embd=256, n_head=4, n_head_kv=4, n_layer=3, n_rot=64, n_ff=352, n_mult=32)  # the file format has no n_head_kv
    hp, w = synth.make_llama(hp0, F16, seed=19)
    path = tmp_path / "f16.bin"
    synth.write_ggjt(str(path), hp, w)
    toks = np.random.default_rng(3).integers(0, hp["n_vocab"], 21).astype(np.int32)

    def run(model):
        s = model.start_session(n_batch=8)
        p0 = _stat(G, "plan_tokens")
        s.feed_prompt(toks)
        ids = [s.infer_next_token() for _ in range(10)]
        ran = _stat(G, "plan_tokens") - p0
        last = s.last_logits().copy()
        s.free()
        return ids, last, ran

    mem = llama.Llama(hp, w, context_size=64)
    a = run(mem)
    mem.free()
    fil = llama.Llama.load(str(path), context_size=64)
    assert fil.hp["wtype"] == F16
    b = run(fil)
    fil.free()
    assert a[2] == 31 and b[2] == 31  # chunks of 8, 8, 5 and ten single tokens: all on the plan
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
