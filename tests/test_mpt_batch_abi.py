"""CPU tests of the batched MPT step's boundary (no GPU): option plan_mpt_batch and counter mpt_batch_steps exist, default to 0 and read
back; the hook ggml_hip_debug_mpt_batch is exported and bound and refuses what it can refuse before it touches a device; Mpt.new_session
exists; the option's environment variable sets it.  Everything runs in a child process: an abort must fail a test, not end the run."""
import os
import subprocess
import sys

from test_mpt_plan_abi import ROOT, child_json


def test_option_counter_hook_and_session_without_a_device():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml, mpt
        L = ggml.lib()
        x = (C.c_float * 64)()
        pos, bad = (C.c_int32 * 8)(), (C.c_int32 * 8)(*([8] * 8))
        ptrs, null = (C.c_void_p * 8)(*([C.addressof(x)] * 8)), (C.c_void_p * 8)()
        hook = lambda *a: L.ggml_hip_debug_mpt_batch(*a)
        out = {"symbol": hasattr(C.CDLL(ggml.LIB_PATH), "ggml_hip_debug_mpt_batch"), "bound": "ggml_hip_debug_mpt_batch" in ggml.PROTOTYPES,
               "methods": [hasattr(mpt.Mpt, "new_session"), hasattr(mpt, "evaluate_batch"), hasattr(mpt, "infer_tokens_batch")],
               "default": [ggml.get_option(k) for k in ("plan_mpt_batch", "plan_mpt_chunk", "plan_mpt")], "stat": ggml.get_stat("mpt_batch_steps"),
               "hook": [hook(0, 2, None, None, x, 2, pos, 8, ptrs, ptrs, 0, 2, 32, 1.0, ptrs),     # no queries
                        hook(0, 2, None, x, x, 2, pos, 8, ptrs, ptrs, 0, 2, 32, 1.0, None),        # no outputs
                        hook(0, 2, None, x, x, 2, None, 8, ptrs, ptrs, 0, 2, 32, 1.0, ptrs),       # no positions
                        hook(0, 2, None, x, x, 2, pos, 8, null, ptrs, 0, 2, 32, 1.0, ptrs),        # no caches
                        hook(0, 2, None, x, x, 9, pos, 8, ptrs, ptrs, 0, 2, 32, 1.0, ptrs),        # nine columns
                        hook(0, 2, None, x, x, 2, bad, 8, ptrs, ptrs, 0, 2, 32, 1.0, ptrs),        # a column behind its cache
                        hook(0, 2, None, x, x, 2, pos, 8, ptrs, ptrs, 0, 2, 16, 1.0, ptrs),        # head size 16
                        hook(0, 17, None, x, x, 2, pos, 8, ptrs, ptrs, 0, 2, 32, 1.0, ptrs),       # W out of range
                        hook(1, 0, None, x, None, 2, pos, 8, ptrs, ptrs, 1024, 0, 0, 0.0, ptrs),   # no weight
                        hook(2, 2, None, x, x, 2, pos, 8, ptrs, ptrs, 0, 2, 32, 1.0, ptrs)]}       # no such op
        ggml.set_option("plan_mpt_batch", 1)
        out["set"] = ggml.get_option("plan_mpt_batch")
        ggml.set_option("plan_mpt_batch", 0)
        out["reset"] = ggml.get_option("plan_mpt_batch")
        print(json.dumps(out))
    """)
    assert got == {"symbol": True, "bound": True, "methods": [True] * 3, "default": [0, 0, 0], "stat": 0, "hook": [-1] * 10, "set": 1, "reset": 0}


def test_the_environment_variable_sets_the_option():
    e = {k: v for k, v in os.environ.items() if not k.startswith("GGML_HIP_")}
    e["GGML_HIP_PLAN_MPT_BATCH"] = "1"
    r = subprocess.run([sys.executable, "-c", "from llm_amd import ggml; print(ggml.get_option('plan_mpt_batch'), ggml.get_option('plan_mpt_chunk'))"],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "1 0", (r.returncode, r.stdout, r.stderr[-2000:])
