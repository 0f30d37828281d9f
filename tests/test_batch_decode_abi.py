"""CPU tests of the batched multi-session decode boundary (no GPU): ggml_hip_decode_batch refuses NULL and a session count
outside 2..8 before it initialises a device — on a machine without one it answers -1 where any device call would abort — and
the entry, the two llm_* calls on top of it, its option and its counters exist.  Everything runs in a child process: an abort
must fail a test, not end the run."""
import json
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child_json(code):
    e = {k: v for k, v in os.environ.items() if not k.startswith("GGML_HIP_")}
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_null_and_counts_outside_2_to_8_are_refused_without_a_device():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml
        L = ggml.lib()
        arr = (C.c_void_p * 9)(*([0x1000] * 9))  # never dereferenced for a refused count
        null8 = (C.c_void_p * 8)()               # eight NULL graphs
        out = {"null": L.ggml_hip_decode_batch(None, 0), "null4": L.ggml_hip_decode_batch(None, 4),
               "counts": [L.ggml_hip_decode_batch(arr, n) for n in (-1, 0, 1, 9, 100)],
               "null_graphs": [L.ggml_hip_decode_batch(null8, n) for n in (2, 8)]}
        print(json.dumps(out))
    """)
    assert got == {"null": -1, "null4": -1, "counts": [-1] * 5, "null_graphs": [-1, -1]}


def test_the_entry_points_the_option_and_the_counters_exist():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml, llama
        lib = C.CDLL(ggml.LIB_PATH)
        L = llama._lib()
        out = {"symbols": [hasattr(lib, n) for n in ("ggml_hip_decode_batch", "llm_evaluate_batch", "llm_infer_next_tokens_greedy_batch")],
               "bound": "ggml_hip_decode_batch" in ggml.PROTOTYPES,
               "plan_batch": ggml.get_option("plan_batch"),
               "stats": [ggml.get_stat("batch_decode_tokens"), ggml.get_stat("batch_decode_steps")],
               "bad_args": [L.llm_evaluate_batch(None, None, None, 2, None), L.llm_infer_next_tokens_greedy_batch(None, None, 2, None)]}
        ggml.set_option("plan_batch", 0)
        out["plan_batch_set"] = ggml.get_option("plan_batch")
        print(json.dumps(out))
    """)
    assert got == {"symbols": [True] * 3, "bound": True, "plan_batch": 1, "stats": [0, 0], "bad_args": [-1, -1], "plan_batch_set": 0}


def test_the_option_and_the_counters_are_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for key in ("plan_batch", "batch_decode_tokens", "batch_decode_steps", "ggml_hip_decode_batch"):
        assert "`%s`" % key in doc or key + "(" in doc, key
