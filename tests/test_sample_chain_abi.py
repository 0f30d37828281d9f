"""CPU tests of the boundary of one session's sampled chain (no GPU): ggml_hip_decode_sampled_chain refuses NULL, an unknown graph
and counts out of range, its test hook what the chain declines, before either computes anything; the entries, the option and the
counters exist and are documented.  Everything that could touch a device runs in a child process: an abort must fail a test, not
end the run."""
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


def test_null_an_unknown_graph_and_counts_out_of_range_are_refused():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml, llama
        L = ggml.lib()
        graph = (C.c_char * 4096)()  # no graph this backend has run: never dereferenced
        ids, win, rng, logits = (C.c_int32 * 64)(), (C.c_int32 * 64)(), (C.c_uint64 * 1)(7), (C.c_float * 64)()
        p = llama.SamplerParams(40, 0.95, 0.8, 1.3)
        pp = C.addressof(p)
        f = L.ggml_hip_decode_sampled_chain
        h = L.ggml_hip_debug_sample_next
        one = (C.c_int32 * 1)(0)
        out = {"null": [f(None, 2, pp, win, 3, rng, ids, logits), f(graph, 2, None, win, 3, rng, ids, logits),
                        f(graph, 2, pp, None, 3, rng, ids, logits), f(graph, 2, pp, win, 3, None, ids, logits),
                        f(graph, 2, pp, win, 3, rng, None, logits)],
               "unknown": [f(graph, 2, pp, win, 3, rng, ids, logits), f(graph, 2, pp, None, 0, rng, ids, None)],
               "counts": [f(graph, n, pp, win, w, rng, ids, logits) for n, w in ((0, 3), (-1, 3), (-2 ** 31, 3), (2, -1), (2, 65))],
               "hook": [h(None, 64, pp, 0, ids, win, one, rng, 1, ids, ids), h(logits, 0, pp, 0, ids, win, one, rng, 1, ids, ids),
                        h(logits, 64, None, 0, ids, win, one, rng, 1, ids, ids), h(logits, 64, pp, 0, ids, win, one, rng, 0, ids, ids),
                        h(logits, 4, pp, 0, ids, win, one, rng, 1, ids, ids)],  # k > V
               "rng": list(rng)}
        print(json.dumps(out))
    """)
    assert got == {"null": [-1] * 5, "unknown": [-1] * 2, "counts": [-1] * 5, "hook": [-1] * 5, "rng": [7]}


def test_the_entry_points_the_option_and_the_counters_exist():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml, llama
        lib = C.CDLL(ggml.LIB_PATH)
        L = llama._lib()
        names = ("ggml_hip_decode_sampled_chain", "ggml_hip_debug_sample_next", "llm_infer_next_token_sampled",
                 "llm_infer_tokens_sampled_via", "llm_infer_tokens_sampled_device")
        out = {"symbols": [hasattr(lib, n) for n in names],
               "bound": ["ggml_hip_decode_sampled_chain" in ggml.PROTOTYPES, "ggml_hip_debug_sample_next" in ggml.PROTOTYPES,
                         hasattr(llama.Session, "infer_next_token_sampled"), hasattr(llama.Session, "infer_tokens_sampled_device")],
               "plan_sample_chain": ggml.get_option("plan_sample_chain"),
               "stats": [ggml.get_stat(k) for k in ("sample_chain_steps", "sample_chain_tokens")],
               "bad_args": [L.llm_infer_tokens_sampled_device(None, None, 3, None, None, None),
                            L.llm_infer_next_token_sampled(None, None, None, None)]}
        ggml.set_option("plan_sample_chain", 0)
        out["plan_sample_chain_set"] = ggml.get_option("plan_sample_chain")
        out["plan_batch_sample"] = ggml.get_option("plan_batch_sample")
        print(json.dumps(out))
    """)
    assert got == {"symbols": [True] * 5, "bound": [True] * 4, "plan_sample_chain": 1, "stats": [0, 0], "bad_args": [-1, -1],
                   "plan_sample_chain_set": 0, "plan_batch_sample": 1}


def test_the_option_has_an_environment_variable_and_drops_no_plan():
    src = open(os.path.join(ROOT, "llm_amd", "csrc", "backend_state.inc")).read()
    assert '{"plan_sample_chain", &Backend::opt_plan_sample_chain, OPT_ENV},' in src
    for key in ("sample_chain_steps", "sample_chain_tokens"):
        assert '{"%s", &Backend::stat_%s}' % (key, key) in src, key


def test_the_entry_the_option_and_the_counters_are_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for key in ("plan_sample_chain", "sample_chain_steps", "sample_chain_tokens", "ggml_hip_decode_sampled_chain",
                "llm_infer_tokens_sampled_device", "llm_infer_next_token_sampled"):
        assert "`%s`" % key in doc or key + "(" in doc, key
