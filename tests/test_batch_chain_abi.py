"""CPU tests of the batched greedy chain's boundary (no GPU): ggml_hip_decode_batch_greedy refuses NULL, a session count outside
2..8 and a step count below 1 (or beyond its cap) before it initialises a device — on a machine without one it answers -1 where
any device call would abort — and the entries, the option and the counters exist and are documented.  Everything runs in a child
process: an abort must fail a test, not end the run."""
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


def test_null_counts_outside_2_to_8_and_step_counts_below_1_are_refused_without_a_device():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml
        L = ggml.lib()
        arr = (C.c_void_p * 9)(*([0x1000] * 9))  # never dereferenced for a refused count
        null8 = (C.c_void_p * 8)()               # eight NULL graphs
        ids = (C.c_int32 * 64)()
        out = {"null": [L.ggml_hip_decode_batch_greedy(None, n, 2, ids) for n in (0, 4)],
               "counts": [L.ggml_hip_decode_batch_greedy(arr, n, 2, ids) for n in (-1, 0, 1, 9, 100)],
               "steps": [L.ggml_hip_decode_batch_greedy(arr, 4, n, ids) for n in (0, -1, -2 ** 31, 4097)],
               "null_graphs": [L.ggml_hip_decode_batch_greedy(null8, n, k, ids) for n in (2, 8) for k in (1, 2)],
               "null_ids": L.ggml_hip_decode_batch_greedy(arr, 4, 2, None),
               "hook": [L.ggml_hip_debug_batch_tail(None, 2, 4, None, None, None, None, None),
                        L.ggml_hip_debug_batch_tail(ids, 9, 4, ids, ids, ids, ids, ids),
                        L.ggml_hip_debug_batch_tail(ids, 2, 0, ids, ids, ids, ids, ids)]}
        print(json.dumps(out))
    """)
    assert got == {"null": [-1, -1], "counts": [-1] * 5, "steps": [-1] * 4, "null_graphs": [-1] * 4, "null_ids": -1, "hook": [-1] * 3}


def test_the_entry_points_the_option_and_the_counters_exist():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml, llama
        lib = C.CDLL(ggml.LIB_PATH)
        L = llama._lib()
        names = ("ggml_hip_decode_batch_greedy", "ggml_hip_debug_batch_tail", "llm_infer_tokens_greedy_batch_device",
                 "llm_infer_tokens_greedy_batch_via")
        out = {"symbols": [hasattr(lib, n) for n in names],
               "bound": ["ggml_hip_decode_batch_greedy" in ggml.PROTOTYPES, "ggml_hip_debug_batch_tail" in ggml.PROTOTYPES],
               "plan_batch_chain": ggml.get_option("plan_batch_chain"),
               "stats": [ggml.get_stat(k) for k in ("batch_chain_steps", "batch_chain_tokens", "batch_decode_steps", "batch_decode_tokens")],
               "bad_args": [L.llm_infer_tokens_greedy_batch_device(None, None, 2, 3, None)]}
        ggml.set_option("plan_batch_chain", 0)
        out["plan_batch_chain_set"] = ggml.get_option("plan_batch_chain")
        print(json.dumps(out))
    """)
    assert got == {"symbols": [True] * 4, "bound": [True, True], "plan_batch_chain": 1, "stats": [0] * 4, "bad_args": [-1],
                   "plan_batch_chain_set": 0}


def test_the_option_has_an_environment_variable_and_drops_no_plan():
    src = open(os.path.join(ROOT, "llm_amd", "csrc", "backend_state.inc")).read()
    assert '{"plan_batch_chain", &Backend::opt_plan_batch_chain, OPT_ENV},' in src
    for key in ("batch_chain_steps", "batch_chain_tokens"):
        assert '{"%s", &Backend::stat_%s}' % (key, key) in src, key


def test_the_entry_the_option_and_the_counters_are_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for key in ("plan_batch_chain", "batch_chain_steps", "batch_chain_tokens", "ggml_hip_decode_batch_greedy",
                "llm_infer_tokens_greedy_batch_device"):
        assert "`%s`" % key in doc or key + "(" in doc, key
