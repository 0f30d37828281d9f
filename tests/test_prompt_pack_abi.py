"""CPU tests of the packed prompt batch (no GPU, no device call): ggml_hip_prompt_pack, llm_feed_prompt_batch and llm_prompt_pack
refuse NULL pointers and counts out of range before any device exists, option plan_prompt_pack follows its environment variable, the
names are bound and documented, and llm_pack_schedule — the rule for rounds alone — equals a Python restatement of the rule on random
count vectors and at its edges.  Child processes as in tests/test_pool_requests_abi.py."""
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


def test_the_entries_refuse_bad_arguments_before_a_device_exists():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml, llama
        L, H = ggml.lib(), llama._lib()
        graph = (C.c_char * 4096)()  # no graph this backend has run: never dereferenced
        graphs = (C.c_void_p * 65)(*[C.addressof(graph)] * 65)
        holes = (C.c_void_p * 65)(*[C.addressof(graph)] * 65)
        holes[3] = None
        pack = L.ggml_hip_prompt_pack
        toks, counts = (C.c_int32 * 8)(), (C.c_int32 * 2)(4, 4)
        none = (C.c_void_p * 2)()
        out = {
            "entry": [pack(None, 2), pack(graphs, 0), pack(graphs, -1), pack(graphs, 65), pack(holes, 6)],
            "host": [H.llm_feed_prompt_batch(None, none, 2, toks, counts, 512), H.llm_prompt_pack(None, none, 2, toks, counts, None, None),
                     H.llm_pack_schedule(None, 2, 512, None)],
            "stats": [ggml.get_stat(k) for k in ("prompt_pack_calls", "prompt_pack_segments", "prompt_pack_tokens", "prompt_plan_tokens")],
        }
        print(json.dumps(out))
    """)
    assert got == {"entry": [-1] * 5, "host": [-1] * 3, "stats": [0] * 4}


def test_plan_prompt_pack_follows_the_environment():
    code = """
        import json
        from llm_amd import ggml
        out = {"env": ggml.get_option("plan_prompt_pack")}
        ggml.set_option("plan_prompt_pack", 0)
        out["set"] = ggml.get_option("plan_prompt_pack")
        print(json.dumps(out))
    """
    assert child_json(code) == {"env": 1, "set": 0}
    assert child_json(code, {"GGML_HIP_PLAN_PROMPT_PACK": "0"}) == {"env": 0, "set": 0}
    assert child_json(code, {"GGML_HIP_PLAN_PROMPT_PACK": "1"}) == {"env": 1, "set": 0}


def test_the_names_are_bound_and_documented():
    from llm_amd import ggml, llama
    lib = C.CDLL(ggml.LIB_PATH)
    for name in ("ggml_hip_prompt_pack", "llm_feed_prompt_batch", "llm_feed_prompt_batch_via", "llm_prompt_pack", "llm_prompt_pack_via",
                 "llm_pack_schedule"):
        assert hasattr(lib, name), name
    assert hasattr(llama.Llama, "feed_prompt_batch") and hasattr(llama.Llama, "prompt_pack")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for key in ("ggml_hip_prompt_pack", "plan_prompt_pack", "prompt_pack_calls", "prompt_pack_segments", "prompt_pack_tokens",
                "llm_feed_prompt_batch", "llm_pack_schedule"):
        assert key in doc, key


# ---- the rule for rounds ----
def schedule_ref(counts, max_rows):
    """In every round the sessions are visited in index order; one with tokens left takes min(left, room)."""
    left, rounds = list(counts), []
    while any(left):
        room, row = max_rows, []
        for i, n in enumerate(left):
            t = min(n, room)
            row.append(t)
            left[i] -= t
            room -= t
        rounds.append(row)
    return rounds


def _schedule(counts, max_rows):
    from llm_amd import llama
    L = llama._lib()
    c = np.array(counts, np.int32)
    n = L.llm_pack_schedule(c.ctypes.data, len(c), max_rows, None)
    if n < 0:
        return n, None
    take = np.full((n + 1, len(c)), -7, np.int32)  # one row more than it may write
    assert L.llm_pack_schedule(c.ctypes.data, len(c), max_rows, take.ctypes.data) == n
    assert (take[n] == -7).all()
    return n, take[:n].tolist()


def test_the_schedule_equals_the_restated_rule_on_random_cases():
    rng = np.random.default_rng(20261021)
    several = 0
    for case in range(400):
        B = int(rng.integers(1, 80))
        hi = int(rng.choice([1, 3, 40, 130, 600]))
        counts = rng.integers(1, hi + 1, B).tolist()
        max_rows = int(rng.choice([1, 2, 7, 32, 96, 512, 1024, 4096])) if case % 5 else int(rng.integers(1, 4097))
        if max_rows == 1 and sum(counts) > 3000:
            max_rows = 7
        n, take = _schedule(counts, max_rows)
        ref = schedule_ref(counts, max_rows)
        assert (n, take) == (len(ref), ref), (counts, max_rows)
        assert np.array(take).sum(axis=0).tolist() == counts and all(0 < sum(r) <= max_rows for r in take)
        several += n > 1
    assert several > 100


def test_the_schedule_at_its_edges():
    assert _schedule([5], 512) == (1, [[5]])                                # one session
    assert _schedule([1300], 512) == (3, [[512], [512], [276]])             # a count larger than max_rows
    assert _schedule([2, 1, 3], 1) == (6, [[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1]])  # max_rows = 1
    assert _schedule([40, 50, 6], 96) == (1, [[40, 50, 6]])                 # counts summing to exactly max_rows
    assert _schedule([40, 50, 7], 96) == (2, [[40, 50, 6], [0, 0, 1]])      # ... and one more
    assert _schedule([70, 9, 33, 120, 12], 96) == (3, [[70, 9, 17, 0, 0], [0, 0, 16, 80, 0], [0, 0, 0, 40, 12]])
    assert _schedule([600, 3], 0) == (2, [[512, 0], [88, 3]])               # 0 means 512
    from llm_amd import llama
    L = llama._lib()
    ok, bad = np.array([3, 4], np.int32), np.array([3, 0], np.int32)
    assert L.llm_pack_schedule(bad.ctypes.data, 2, 512, None) == -1         # a count below 1
    assert L.llm_pack_schedule(ok.ctypes.data, 0, 512, None) == -1
    assert L.llm_pack_schedule(ok.ctypes.data, 2, -1, None) == -1
    assert L.llm_pack_schedule(ok.ctypes.data, 2, 4097, None) == -1
    assert L.llm_pack_schedule(ok.ctypes.data, 2, 4096, None) == 1
