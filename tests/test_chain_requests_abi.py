"""CPU tests of the chains that stop (no GPU, no device call): ggml_hip_decode_chain_requests / ggml_hip_decode_batch_requests and the
hook refuse NULL pointers and counts out of range before any device exists, option chain_group follows its environment variable, the
counters answer, and the end rule of the host loop — stop id, budget, context full — is checked on recorded logits rows through
llm_until_rule, which draws with llm_sample_chain, against a restatement on tests/sampler_chain_ref.py.  Child processes as in
tests/test_batch_kquant_abi.py."""
import ctypes as C
import json
import os
import subprocess
import sys
import textwrap

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_chain_ref as X  # noqa: E402
import sampler_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child_json(code, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("GGML_HIP_")}
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_both_entries_and_the_hook_refuse_bad_arguments_before_a_device_exists():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml, llama
        L = ggml.lib()
        graph = (C.c_char * 4096)()  # no graph this backend has run: never dereferenced
        graphs = (C.c_void_p * 8)(*[C.addressof(graph)] * 8)
        ids, win, wn, logits = (C.c_int32 * 256)(), (C.c_int32 * 512)(), (C.c_int32 * 8)(), (C.c_float * 64)()
        rng, mu, cnt, why = (C.c_uint64 * 8)(*[7] * 8), (C.c_float * 8)(*[6.0] * 8), (C.c_int32 * 8)(), (C.c_int32 * 8)()
        ch = llama.sampler_chain()
        chains = (C.c_void_p * 8)(*[C.addressof(ch)] * 8)
        greedy = (C.c_void_p * 8)()

        class End(C.Structure):
            _fields_ = [("budget", C.c_int32), ("n_stop", C.c_int32), ("stop_id", C.c_int32 * 8)]
        def ends(budget, n_stop=0):
            return (End * 8)(*[End(budget, n_stop) for _ in range(8)])
        one = L.ggml_hip_decode_chain_requests
        many = L.ggml_hip_decode_batch_requests
        hook = L.ggml_hip_debug_next_token_req
        p = C.addressof(ch)
        e4 = ends(4)
        out = {
            "one_null": [one(None, 4, p, e4, win, 3, rng, mu, ids, cnt, why, logits), one(graph, 4, p, None, win, 3, rng, mu, ids, cnt, why, logits),
                         one(graph, 4, p, e4, None, 3, rng, mu, ids, cnt, why, logits), one(graph, 4, p, e4, win, 3, None, mu, ids, cnt, why, logits),
                         one(graph, 4, p, e4, win, 3, rng, mu, None, cnt, why, logits), one(graph, 4, p, e4, win, 3, rng, mu, ids, None, why, logits),
                         one(graph, 4, p, e4, win, 3, rng, mu, ids, cnt, None, logits)],
            "one_counts": [one(graph, n, p, ends(b, s), win, w, rng, mu, ids, cnt, why, logits)
                           for n, b, s, w in ((0, 1, 0, 3), (-1, 1, 0, 3), (4, 0, 0, 3), (4, 5, 0, 3), (4, 4, -1, 3), (4, 4, 9, 3), (4, 4, 0, -1),
                                              (4, 4, 0, 65), (5000, 4, 0, 3))],
            "one_unknown": [one(graph, 4, p, e4, win, 3, rng, mu, ids, cnt, why, logits), one(graph, 4, None, e4, None, 0, None, None, ids, cnt, why, None)],
            "many_null": [many(None, 3, 4, chains, e4, win, wn, rng, mu, ids, cnt, why), many(graphs, 3, 4, None, e4, win, wn, rng, mu, ids, cnt, why),
                          many(graphs, 3, 4, chains, None, win, wn, rng, mu, ids, cnt, why), many(graphs, 3, 4, chains, e4, None, wn, rng, mu, ids, cnt, why),
                          many(graphs, 3, 4, chains, e4, win, None, rng, mu, ids, cnt, why), many(graphs, 3, 4, chains, e4, win, wn, None, mu, ids, cnt, why),
                          many(graphs, 3, 4, chains, e4, win, wn, rng, mu, None, cnt, why), many(graphs, 3, 4, chains, e4, win, wn, rng, mu, ids, None, why),
                          many(graphs, 3, 4, chains, e4, win, wn, rng, mu, ids, cnt, None),
                          many((C.c_void_p * 8)(), 3, 4, chains, e4, win, wn, rng, mu, ids, cnt, why)],
            "many_counts": [many(graphs, B, n, greedy, ends(b, s), None, None, None, None, ids, cnt, why)
                            for B, n, b, s in ((1, 4, 4, 0), (9, 4, 4, 0), (3, 0, 1, 0), (3, 4097, 4, 0), (3, 4, 0, 0), (3, 4, 5, 0), (3, 4, 4, -1),
                                               (3, 4, 4, 9))],
            "hook": [hook(None, 1, 64, chains, e4, 0, None, ids, win, wn, rng, mu, 4, ids, ids, None, cnt, why),
                     hook(logits, 1, 64, None, e4, 0, None, ids, win, wn, rng, mu, 4, ids, ids, None, cnt, why),
                     hook(logits, 1, 64, chains, None, 0, None, ids, win, wn, rng, mu, 4, ids, ids, None, cnt, why),
                     hook(logits, 2, 64, chains, e4, 0, None, ids, win, wn, rng, mu, 4, ids, ids, None, cnt, why),   # B = 2 without a BatchCols
                     hook(logits, 1, 64, chains, ends(5), 0, None, ids, win, wn, rng, mu, 4, ids, ids, None, cnt, why),  # budget > n_draws
                     hook(logits, 1, 64, chains, ends(2, 9), 0, None, ids, win, wn, rng, mu, 4, ids, ids, None, cnt, why),
                     hook(logits, 1, 64, chains, e4, 0, None, ids, win, wn, rng, mu, 0, ids, ids, None, cnt, why)],
            "rng": list(rng), "mu": list(mu), "cnt": list(cnt), "why": list(why),
            "stats": [ggml.get_stat(k) for k in ("chain_stopped_columns", "chain_frozen_steps", "chain_steps_cut", "plan_tokens")],
            "host": [llama._lib().llm_infer_until(None, None, None, None, None, None, None, None),
                     llama._lib().llm_infer_until_batch(None, None, 2, None, None, None, None, None, None)],
        }
        print(json.dumps(out))
    """)
    assert got == {"one_null": [-1] * 7, "one_counts": [-1] * 9, "one_unknown": [-1] * 2, "many_null": [-1] * 10, "many_counts": [-1] * 8,
                   "hook": [-1] * 7, "rng": [7] * 8, "mu": [6.0] * 8, "cnt": [0] * 8, "why": [0] * 8, "stats": [0, 0, 0, 0], "host": [-1, -1]}


def test_chain_group_follows_the_environment_and_is_clamped():
    code = """
        import json
        from llm_amd import ggml
        out = {"env": ggml.get_option("chain_group")}
        ggml.set_option("chain_group", 4)
        out["set"] = ggml.get_option("chain_group")
        ggml.set_option("chain_group", 0)
        out["low"] = ggml.get_option("chain_group")
        print(json.dumps(out))
    """
    default = child_json(code)
    assert default["env"] >= 1 and default["set"] == 4 and default["low"] == 1
    assert child_json(code, {"GGML_HIP_CHAIN_GROUP": "32"}) == {"env": 32, "set": 4, "low": 1}
    assert child_json(code, {"GGML_HIP_CHAIN_GROUP": "7"}) == {"env": 7, "set": 4, "low": 1}
    src = open(os.path.join(ROOT, "llm_amd", "csrc", "backend_state.inc")).read()
    assert '{"chain_group", &Backend::opt_chain_group, OPT_ENV, FX_NONE, 1, 4096},' in src
    for key in ("chain_stopped_columns", "chain_frozen_steps", "chain_steps_cut"):
        assert '{"%s", &Backend::stat_%s}' % (key, key) in src, key


def test_the_entries_are_bound_and_documented():
    from llm_amd import ggml, llama
    lib = C.CDLL(ggml.LIB_PATH)
    for name in ("ggml_hip_decode_chain_requests", "ggml_hip_decode_batch_requests", "ggml_hip_debug_next_token_req", "llm_infer_until",
                 "llm_infer_until_batch", "llm_infer_until_via", "llm_infer_until_batch_via", "llm_until_rule"):
        assert hasattr(lib, name), name
    assert hasattr(llama.Session, "infer_until") and hasattr(llama.Llama, "infer_until_batch")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for key in ("ggml_hip_decode_chain_requests", "ggml_hip_decode_batch_requests", "chain_group", "chain_stopped_columns",
                "chain_frozen_steps", "chain_steps_cut", "llm_infer_until", "llm_infer_until_batch"):
        assert key in doc, key


# ---- the end rule of the host loop on recorded rows ----
V = 300
ROWS = R.rows(4, V, seed=9)
ROWS.setflags(write=False)
TRUNC = dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30, freq=0.3, presence=0.2, tail_free_z=0.9, typical_p=0.5, min_p=0.2)


def _rule(rows, max_tokens, stop, sampler, window, n_past0, context, seed=0x9E3779B97F4A7C15):
    from llm_amd import llama
    req, chain = llama.until_request(max_tokens, stop, sampler)
    rows = np.ascontiguousarray(rows, np.float32)
    window = np.ascontiguousarray(window, np.int32)
    rng, mu = np.array([seed], np.uint64), np.array([6.0], np.float32)
    out, cnt, why = np.full(len(rows) + 1, -7, np.int32), C.c_int32(-1), C.c_int32(-1)
    rc = llama._lib().llm_until_rule(rows.ctypes.data, len(rows), rows.shape[1], C.addressof(req), window.ctypes.data if window.size else None,
                                     window.size, n_past0, context, rng.ctypes.data, mu.ctypes.data, out.ctypes.data, C.addressof(cnt),
                                     C.addressof(why))
    return rc, out[:max(cnt.value, 0)].tolist(), cnt.value, why.value, int(rng[0]), out


def _want(rows, max_tokens, stop, ch, window, n_past0, context, seed=0x9E3779B97F4A7C15):
    """The reference's loop restated: ContextFull before a draw (inference_session.rs:388), the draw, the evaluation (n_past + 1), then
    EndOfText for a stop id (:404-408); the budget ends it otherwise."""
    hist, rng, mu, ids, n_past = list(window), seed, np.float32(6.0), [], n_past0
    for t in range(len(rows)):
        if len(ids) >= max_tokens:
            return ids, 1, rng
        if n_past + 1 >= context:
            return ids, 3, rng
        if ch is None:
            tok = int(np.lexsort((np.arange(rows.shape[1]), -rows[t].astype(np.float64)))[0])
        else:
            tok, rng, mu = X.sample(rows[t], hist[-64:], ch, rng, mu)
        hist.append(tok)
        ids.append(tok)
        n_past += 1
        if tok in stop:
            return ids, 2, rng
    if len(ids) >= max_tokens:
        return ids, 1, rng
    return ids, (3 if n_past + 1 >= context else 0), rng


def _cases():
    ch = X.chain(k=40, top_p=0.95, temperature=0.8, penalty=1.30, freq=0.3, presence=0.2, z=0.9, typical=0.5, min_p=0.2)
    rows = np.ascontiguousarray(np.tile(ROWS, (3, 1)))  # 12 rows
    free, _, _ = _want(rows, 12, (), ch, [3, 4], 5, 64)
    j = next(i for i in range(1, 9) if free.index(free[i]) == i)
    return ch, rows, free, j


def test_the_rule_ends_on_the_stop_id_after_evaluating_it():
    ch, rows, free, j = _cases()
    rc, ids, cnt, why, rng, raw = _rule(rows, 12, [free[j], V - 1], TRUNC, [3, 4], 5, 64)
    want_ids, want_why, want_rng = _want(rows, 12, (free[j], V - 1), ch, [3, 4], 5, 64)
    assert rc == 0 and ids == want_ids == free[:j + 1] and cnt == j + 1 and why == want_why == 2 and rng == want_rng
    assert raw[cnt:].tolist() == [-7] * (len(raw) - cnt)


def test_the_rule_ends_on_the_budget_and_the_stop_id_wins_at_the_last_draw():
    ch, rows, free, j = _cases()
    rc, ids, cnt, why, rng, _ = _rule(rows, 5, [], TRUNC, [3, 4], 5, 64)
    want_ids, want_why, want_rng = _want(rows, 5, (), ch, [3, 4], 5, 64)
    assert (rc, ids, cnt, why, rng) == (0, want_ids, 5, 1, want_rng) and want_why == 1 and ids == free[:5]
    rc, ids, cnt, why, _, _ = _rule(rows, j + 1, [free[j]], TRUNC, [3, 4], 5, 64)
    assert (rc, ids, cnt, why) == (0, free[:j + 1], j + 1, 2)


def test_the_rule_ends_where_the_context_is_full():
    ch, rows, free, j = _cases()
    for n_past0, context, n, reason in ((60, 64, 3, 3), (61, 64, 2, 3), (63, 64, 0, 3), (64, 64, 0, 3), (56, 64, 7, 3), (55, 64, 8, 1)):
        rc, ids, cnt, why, rng, _ = _rule(rows, 8, [], TRUNC, [3, 4], n_past0, context)
        want_ids, want_why, want_rng = _want(rows, 8, (), ch, [3, 4], n_past0, context)
        assert (rc, ids, cnt, why, rng) == (0, want_ids, n, reason, want_rng) and want_why == reason, (n_past0, ids, why)


def test_the_greedy_rule_and_bad_requests():
    ch, rows, free, j = _cases()
    rc, ids, cnt, why, rng, _ = _rule(rows, 6, [], None, [], 0, 64)
    want_ids, want_why, _ = _want(rows, 6, (), None, [], 0, 64)
    assert (rc, ids, cnt, why) == (0, want_ids, 6, 1) and rng == 0x9E3779B97F4A7C15 and want_why == 1
    rc, ids, cnt, why, _, _ = _rule(rows, 6, [want_ids[0]], None, [], 0, 64)
    assert (rc, ids, cnt, why) == (0, want_ids[:1], 1, 2)
    for max_tokens, stop, sampler in ((0, [], TRUNC), (4, [V], TRUNC), (4, [-1], None), (4, [], dict(TRUNC, tail_free_z=0.0))):
        rc, _, cnt, why, rng, _ = _rule(rows, max_tokens, stop, sampler, [3], 0, 64)
        assert rc == -1 and cnt == -1 and why == -1 and rng == 0x9E3779B97F4A7C15
