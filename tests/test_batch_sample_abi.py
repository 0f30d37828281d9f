"""CPU tests of the sampled batched chain's boundary (no GPU): ggml_hip_decode_batch_sampled and its test hook refuse NULL, a
session count outside 2..8, a step count below 1 (or beyond its cap) and sampler parameters out of range before they initialise a
device, and the entries, the option and the counters exist and are documented.  Everything that could touch a device runs in a
child process: an abort must fail a test, not end the run."""
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


def test_null_and_counts_out_of_range_are_refused_without_a_device():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml, llama
        L = ggml.lib()
        arr = (C.c_void_p * 9)(*([0x1000] * 9))  # never dereferenced for a refused count
        null8 = (C.c_void_p * 8)()
        ids, win, wn, rng = (C.c_int32 * 64)(), (C.c_int32 * 512)(), (C.c_int32 * 8)(), (C.c_uint64 * 8)()
        p = llama.SamplerParams(40, 0.95, 0.8, 1.3)
        pp = C.addressof(p)
        f = L.ggml_hip_decode_batch_sampled
        out = {"null": [f(None, 4, 2, pp, win, wn, rng, ids), f(arr, 4, 2, None, win, wn, rng, ids), f(arr, 4, 2, pp, None, wn, rng, ids),
                        f(arr, 4, 2, pp, win, None, rng, ids), f(arr, 4, 2, pp, win, wn, None, ids), f(arr, 4, 2, pp, win, wn, rng, None)],
               "counts": [f(arr, n, 2, pp, win, wn, rng, ids) for n in (-1, 0, 1, 9, 100)],
               "steps": [f(arr, 4, n, pp, win, wn, rng, ids) for n in (0, -1, -2 ** 31, 4097)],
               "null_graphs": [f(null8, n, k, pp, win, wn, rng, ids) for n in (2, 8) for k in (1, 2)],
               "hook": [L.ggml_hip_debug_batch_sample(None, 2, 4, pp, ids, ids, win, wn, rng, 1, ids, ids, ids),
                        L.ggml_hip_debug_batch_sample(ids, 9, 64, pp, ids, ids, win, wn, rng, 1, ids, ids, ids),
                        L.ggml_hip_debug_batch_sample(ids, 2, 64, pp, ids, ids, win, wn, rng, 0, ids, ids, ids),
                        L.ggml_hip_debug_batch_sample(ids, 2, 4, pp, ids, ids, win, wn, rng, 1, ids, ids, ids)],  # k > V
               "rng": list(rng)}
        print(json.dumps(out))
    """)
    assert got == {"null": [-1] * 6, "counts": [-1] * 5, "steps": [-1] * 4, "null_graphs": [-1] * 4, "hook": [-1] * 4, "rng": [0] * 8}


def test_the_entry_points_the_option_and_the_counters_exist():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml, llama
        lib = C.CDLL(ggml.LIB_PATH)
        L = llama._lib()
        names = ("ggml_hip_decode_batch_sampled", "ggml_hip_debug_batch_sample", "llm_sample_exact", "llm_infer_next_tokens_sampled_batch",
                 "llm_infer_tokens_sampled_batch_device", "llm_infer_next_tokens_sampled_batch_via", "llm_infer_tokens_sampled_batch_via")
        out = {"symbols": [hasattr(lib, n) for n in names],
               "bound": ["ggml_hip_decode_batch_sampled" in ggml.PROTOTYPES, "ggml_hip_debug_batch_sample" in ggml.PROTOTYPES],
               "plan_batch_sample": ggml.get_option("plan_batch_sample"),
               "stats": [ggml.get_stat(k) for k in ("batch_sample_steps", "batch_sample_tokens", "batch_chain_steps", "batch_chain_tokens")],
               "bad_args": [L.llm_infer_tokens_sampled_batch_device(None, None, 2, 3, None, None, None),
                            L.llm_infer_next_tokens_sampled_batch(None, None, 2, None, None, None)]}
        ggml.set_option("plan_batch_sample", 0)
        out["plan_batch_sample_set"] = ggml.get_option("plan_batch_sample")
        out["plan_batch_chain"] = ggml.get_option("plan_batch_chain")
        print(json.dumps(out))
    """)
    assert got == {"symbols": [True] * 7, "bound": [True, True], "plan_batch_sample": 1, "stats": [0] * 4, "bad_args": [-1, -1],
                   "plan_batch_sample_set": 0, "plan_batch_chain": 1}


def test_the_option_has_an_environment_variable_and_drops_no_plan():
    src = open(os.path.join(ROOT, "llm_amd", "csrc", "backend_state.inc")).read()
    assert '{"plan_batch_sample", &Backend::opt_plan_batch_sample, OPT_ENV},' in src
    for key in ("batch_sample_steps", "batch_sample_tokens"):
        assert '{"%s", &Backend::stat_%s}' % (key, key) in src, key


def test_the_entry_the_option_and_the_counters_are_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for key in ("plan_batch_sample", "batch_sample_steps", "batch_sample_tokens", "ggml_hip_decode_batch_sampled",
                "llm_infer_tokens_sampled_batch_device", "llm_sample_exact"):
        assert "`%s`" % key in doc or key + "(" in doc, key
