"""CPU tests of the request pool (no GPU, no device call): ggml_hip_decode_pool_requests, llm_infer_until_pool and the hook
ggml_hip_debug_pool_admit refuse NULL pointers and counts out of range before any device exists and leave states and outputs alone,
option plan_batch_pool follows its environment variable, the names are bound and documented, and llm_pool_schedule — the admission
rule of kernels/pool_rule.h alone — equals a Python restatement of the rule on random cases and gives the step counts of the two
budget sets the pool was proposed with.  Child processes as in tests/test_chain_requests_abi.py."""
import ctypes as C
import json
import os
import subprocess
import sys
import textwrap

import numpy as np

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
        N = 64
        graph = (C.c_char * 4096)()  # no graph this backend has run: never dereferenced
        graphs = (C.c_void_p * N)(*[C.addressof(graph)] * N)
        ids, win, wn = (C.c_int32 * 4096)(*[-7] * 4096), (C.c_int32 * (64 * N))(), (C.c_int32 * N)()
        rng, mu = (C.c_uint64 * N)(*[7] * N), (C.c_float * N)(*[6.0] * N)
        col, first, cnt, why, steps = (C.c_int32 * N)(*[-7] * N), (C.c_int32 * N)(*[-7] * N), (C.c_int32 * N)(*[-7] * N), (C.c_int32 * N)(*[-7] * N), C.c_int32(-7)
        ch = llama.sampler_chain()
        chains = (C.c_void_p * N)(*[C.addressof(ch)] * N)
        greedy = (C.c_void_p * N)()

        class End(C.Structure):
            _fields_ = [("budget", C.c_int32), ("n_stop", C.c_int32), ("stop_id", C.c_int32 * 8)]
        def ends(budget, n_stop=0):
            return (End * N)(*[End(budget, n_stop) for _ in range(N)])
        pool = L.ggml_hip_decode_pool_requests
        e4 = ends(4)
        sp = C.addressof(steps)
        def call(g=graphs, P=6, B=3, n=4, c=chains, e=e4, w=win, n_w=wn, r=rng, u=mu, i=ids, co=col, f=first, k=cnt, y=why, s=sp):
            return pool(g, P, B, n, c, e, w, n_w, r, u, i, co, f, k, y, s)
        sizes = (C.c_int64 * 5)()
        L.ggml_hip_debug_pool_admit_sizes(sizes)
        blobs = [(C.c_char * int(s))() for s in sizes]
        logits, emb, sl, se = (C.c_float * (8 * 41))(), (C.c_float * (8 * 8))(), (C.c_float * (64 * 41))(), (C.c_float * (64 * 8))()
        hook = L.ggml_hip_debug_pool_admit
        def hk(t=blobs[0], r=blobs[1], s=blobs[2], p=blobs[3], b=blobs[4], z=sizes, B=3, P=6, lg=logits, em=emb, V=41, E=8, a=sl, c=se):
            return hook(t, r, s, p, b, z, B, P, lg, em, V, E, a, c)
        bad_sizes = (C.c_int64 * 5)(*[int(s) for s in sizes])
        bad_sizes[0] += 8
        out = {
            "null": [call(g=None), call(c=None), call(e=None), call(w=None), call(n_w=None), call(r=None), call(i=None), call(co=None), call(f=None),
                     call(k=None), call(y=None), call(s=None), call(g=(C.c_void_p * N)())],
            "cols": [call(B=b) for b in (-1, 0, 1, 9)],
            "pool": [call(P=p) for p in (-1, 0, 2, 65, 1000)],
            "steps": [call(n=n) for n in (-1, 0, 4097)],
            "ends": [call(c=greedy, e=ends(b, s), w=None, n_w=None, r=None, u=None) for b, s in ((0, 0), (5, 0), (-1, 0), (4, -1), (4, 9))],
            "sizes": [int(s) > 0 for s in sizes],
            "hook": [hk(t=None), hk(r=None), hk(s=None), hk(p=None), hk(b=None), hk(z=None), hk(lg=None), hk(em=None), hk(a=None), hk(c=None),
                     hk(z=bad_sizes), hk(B=1), hk(B=9), hk(P=2), hk(P=65), hk(V=0), hk(E=0),
                     hk()],  # a zeroed table: its head says 0 columns, not 3
            "rng": sorted(set(rng)), "mu": sorted(set(mu)), "outs": sorted(set(list(col) + list(first) + list(cnt) + list(why) + [steps.value] + list(ids))),
            "stats": [ggml.get_stat(k) for k in ("pool_calls", "pool_admitted", "pool_steps", "chain_frozen_steps", "plan_tokens")],
            "host": [llama._lib().llm_infer_until_pool(None, None, 2, None, None, None, 2, None, None, None),
                     llama._lib().llm_pool_schedule(None, 3, 2, None, None)],
        }
        print(json.dumps(out))
    """)
    assert got == {"null": [-1] * 13, "cols": [-1] * 4, "pool": [-1] * 5, "steps": [-1] * 3, "ends": [-1] * 5,
                   "sizes": [True] * 5, "hook": [-1] * 18, "rng": [7], "mu": [6.0], "outs": [-7], "stats": [0, 0, 0, 0, 0], "host": [-1, -1]}


def test_plan_batch_pool_follows_the_environment():
    code = """
        import json
        from llm_amd import ggml
        out = {"env": ggml.get_option("plan_batch_pool")}
        ggml.set_option("plan_batch_pool", 0)
        out["set"] = ggml.get_option("plan_batch_pool")
        print(json.dumps(out))
    """
    assert child_json(code) == {"env": 1, "set": 0}
    assert child_json(code, {"GGML_HIP_PLAN_BATCH_POOL": "0"}) == {"env": 0, "set": 0}
    assert child_json(code, {"GGML_HIP_PLAN_BATCH_POOL": "1"}) == {"env": 1, "set": 0}
    src = open(os.path.join(ROOT, "llm_amd", "csrc", "backend_state.inc")).read()
    assert '{"plan_batch_pool", &Backend::opt_plan_batch_pool, OPT_ENV},' in src
    for key in ("pool_calls", "pool_admitted", "pool_steps"):
        assert '{"%s", &Backend::stat_%s}' % (key, key) in src, key


def test_the_names_are_bound_and_documented():
    from llm_amd import ggml, llama
    lib = C.CDLL(ggml.LIB_PATH)
    for name in ("ggml_hip_decode_pool_requests", "ggml_hip_debug_pool_admit", "ggml_hip_debug_pool_admit_sizes", "llm_infer_until_pool",
                 "llm_infer_until_pool_via", "llm_pool_schedule", "llm_pool_step_cap"):
        assert hasattr(lib, name), name
    assert hasattr(llama.Llama, "infer_until_pool")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for key in ("ggml_hip_decode_pool_requests", "ggml_hip_debug_pool_admit", "plan_batch_pool", "pool_calls", "pool_admitted", "pool_steps",
                "llm_infer_until_pool", "llm_pool_schedule", "pool_rule.h"):
        assert key in doc, key


# ---- the admission rule ----
def schedule_ref(evals, n_cols):
    """The rule restated on the timeline.  A request of e evaluations that starts at step f evaluates at steps f .. f + e - 1; its last
    draw comes in the tail of step f + e - 2, so behind the tail of step f + e - 1 it is not live and was not live before that step
    ran: the column is free then, and whoever takes it starts at step f + e.  (e = 1, born ended: free behind its only step.)  Free
    columns in ascending index take the waiting requests in ascending pool index."""
    n = len(evals)
    col, first = [-1] * n, [0] * n
    free_after = [None] * n_cols  # the step behind whose tail column c becomes free
    for c in range(n_cols):
        col[c], first[c], free_after[c] = c, 0, evals[c] - 1
    cursor, s = n_cols, 0
    while cursor < n:
        for c in range(n_cols):
            if cursor < n and free_after[c] <= s:
                col[cursor], first[cursor] = c, s + 1
                free_after[c] = s + evals[cursor]
                cursor += 1
        s += 1
    return max(f + e for f, e in zip(first, evals)), col, first


def _schedule(evals, n_cols):
    from llm_amd import llama
    e = np.ascontiguousarray(evals, np.int32)
    col, first = np.full(len(e), -9, np.int32), np.full(len(e), -9, np.int32)
    steps = llama._lib().llm_pool_schedule(e.ctypes.data, len(e), n_cols, col.ctypes.data, first.ctypes.data)
    return steps, col.tolist(), first.tolist()


def test_the_schedule_equals_the_restated_rule_on_random_cases():
    rng = np.random.default_rng(20261020)
    seen_born, seen_double, seen_exact = 0, 0, 0
    for case in range(400):
        n_cols = int(rng.integers(1, 9))
        n = n_cols if case % 7 == 0 else int(rng.integers(n_cols, 65))
        hi = int(rng.choice([2, 3, 8, 40]))
        evals = rng.integers(1, hi + 1, n).tolist()
        if case % 3 == 0:  # several columns free at once: equal budgets side by side
            evals[:n_cols] = [evals[0]] * n_cols
        want = schedule_ref(evals, n_cols)
        assert _schedule(evals, n_cols) == want, (n_cols, evals)
        seen_born += 1 in evals
        seen_exact += n == n_cols
        firsts = [f for f in want[2][n_cols:]]
        seen_double += len(firsts) != len(set(firsts))
    assert seen_born > 50 and seen_double > 50 and seen_exact > 50


def test_the_schedule_by_hand():
    # three columns; request 1 is born ended, so request 3 takes column 1 at step 1; columns 0 and 2 both free behind step 2
    assert _schedule([3, 1, 3, 2, 1, 1, 4], 3) == (7, [0, 1, 2, 1, 0, 1, 2], [0, 0, 0, 1, 3, 3, 3])
    assert _schedule([2, 2], 2) == (2, [0, 1], [0, 0])
    assert _schedule([1], 1) == (1, [0], [0])


def test_the_budget_sets_of_the_proposal_give_704_and_1280_steps():
    for n, steps in ((32, 704), (64, 1280)):
        evals = [32 * (1 + i % 8) for i in range(n)]
        assert sum(evals) == {32: 4608, 64: 9216}[n]
        assert _schedule(evals, 8)[0] == steps == schedule_ref(evals, 8)[0]
        waves = sum(max(evals[i:i + 8]) for i in range(0, n, 8))
        assert waves == {32: 1024, 64: 2048}[n]


def test_bad_schedules_are_refused():
    from llm_amd import llama
    L = llama._lib()
    e = np.array([2, 3, 0], np.int32)
    ok = np.array([2, 3, 1], np.int32)
    assert L.llm_pool_schedule(e.ctypes.data, 3, 2, None, None) == -1      # an evaluation count below 1
    assert L.llm_pool_schedule(ok.ctypes.data, 3, 0, None, None) == -1
    assert L.llm_pool_schedule(ok.ctypes.data, 3, 9, None, None) == -1
    assert L.llm_pool_schedule(ok.ctypes.data, 3, 4, None, None) == -1     # fewer requests than columns
    assert L.llm_pool_schedule(ok.ctypes.data, 3, 2, None, None) == 3
