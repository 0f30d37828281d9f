"""CPU tests of the MPT plan's boundary (no GPU): option plan_mpt and counter mpt_plan_tokens exist, default to 0 and read back; the
greedy chain entry answers -1 without a device or a plan; the test hook refuses what it can refuse before it touches a device; the new
symbols are exported and bound; the option's environment variable sets it.  Everything runs in a child process: an abort must fail a
test, not end the run."""
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


def test_option_counter_chain_entry_and_hook_without_a_device():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml, mpt
        L = ggml.lib()
        lib = C.CDLL(ggml.LIB_PATH)
        ids, lg = (C.c_int32 * 8)(), (C.c_float * 8)()
        x = (C.c_float * 64)()
        outs = (C.c_void_p * 4)(*([C.addressof(x)] * 4))
        out = {"symbols": [hasattr(lib, n) for n in ("ggml_hip_debug_mpt", "ggml_hip_decode_greedy_chain")],
               "bound": "ggml_hip_debug_mpt" in ggml.PROTOTYPES,
               "method": hasattr(mpt.Mpt, "infer_tokens_device"),
               "default": ggml.get_option("plan_mpt"),
               "stat": ggml.get_stat("mpt_plan_tokens"),
               "chain": [L.ggml_hip_decode_greedy_chain(None, 4, ids, lg), L.ggml_hip_decode_greedy_chain(C.addressof(x), 1, ids, lg)],
               "hook": [L.ggml_hip_debug_mpt(0, 1, None, x, 1e-5, 64, None, None, 0, 0, 0, 0, 0.0, outs),   # no row
                        L.ggml_hip_debug_mpt(0, 1, x, x, 1e-5, 48, None, None, 0, 0, 0, 0, 0.0, outs),      # not whole blocks
                        L.ggml_hip_debug_mpt(0, 1, x, x, 1e-5, 16384, None, None, 0, 0, 0, 0, 0.0, outs),   # wider than the staging
                        L.ggml_hip_debug_mpt(1, 0, x, x, 0.0, 0, None, None, 2, 32, 0, 8, 1.0, outs),       # no caches
                        L.ggml_hip_debug_mpt(1, 0, x, x, 0.0, 0, x, x, 2, 16, 0, 8, 1.0, outs),             # head size 16
                        L.ggml_hip_debug_mpt(1, 0, x, x, 0.0, 0, x, x, 2, 32, 8, 8, 1.0, outs),             # the token behind the cache
                        L.ggml_hip_debug_mpt(3, 0, None, x, 0.0, 0, x, x, 2, 32, 0, 8, 1.0, outs),          # no graph
                        L.ggml_hip_debug_mpt(4, 0, x, x, 0.0, 0, x, x, 2, 32, 0, 8, 1.0, outs)]}            # no such op
        ggml.set_option("plan_mpt", 1)
        out["set"] = ggml.get_option("plan_mpt")
        ggml.set_option("plan_mpt", 0)
        out["reset"] = ggml.get_option("plan_mpt")
        print(json.dumps(out))
    """)
    assert got == {"symbols": [True, True], "bound": True, "method": True, "default": 0, "stat": 0, "chain": [-1, -1], "hook": [-1] * 8,
                   "set": 1, "reset": 0}


def test_the_environment_variable_sets_the_option():
    e = {k: v for k, v in os.environ.items() if not k.startswith("GGML_HIP_")}
    e["GGML_HIP_PLAN_MPT"] = "1"
    r = subprocess.run([sys.executable, "-c", "from llm_amd import ggml; print(ggml.get_option('plan_mpt'))"], cwd=ROOT, env=e, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "1", (r.returncode, r.stdout, r.stderr[-2000:])
