"""CPU tests of the MPT prompt plan's boundary (no GPU): option plan_mpt_prompt and counter mpt_prompt_tokens exist, default to 0 and read
back; the test hook is exported, bound, and refuses what it can refuse before it touches a device; Mpt.feed_prompt exists; the option's
environment variable sets it.  Everything runs in a child process: an abort must fail a test, not end the run."""
import os
import subprocess
import sys

from test_mpt_plan_abi import ROOT, child_json


def test_option_counter_and_hook_without_a_device():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml, mpt
        L = ggml.lib()
        x = (C.c_float * 64)()
        outs = (C.c_void_p * 2)(C.addressof(x), C.addressof(x))
        hook = lambda what, K, N, H, D, P, Cc, xx=x: L.ggml_hip_debug_mpt_prompt(what, 0, xx, None, None, x, 1e-5, K, N, x, x, H, D, P, Cc, 1.0, outs)
        out = {"symbol": hasattr(C.CDLL(ggml.LIB_PATH), "ggml_hip_debug_mpt_prompt"), "bound": "ggml_hip_debug_mpt_prompt" in ggml.PROTOTYPES,
               "method": hasattr(mpt.Mpt, "feed_prompt"),
               "default": [ggml.get_option("plan_mpt_prompt"), ggml.get_option("plan_mpt")], "stat": ggml.get_stat("mpt_prompt_tokens"),
               "hook": [hook(0, 64, 1, 0, 0, 0, 0, None),  # no rows
                        hook(0, 48, 1, 0, 0, 0, 0),        # not whole blocks
                        hook(0, 16384, 1, 0, 0, 0, 0),     # wider than a row in registers
                        hook(1, 48, 1, 0, 0, 0, 0),
                        hook(2, 0, 2, 2, 16, 0, 8),        # head size 16
                        hook(2, 0, 2, 2, 32, 7, 8),        # the last query behind the cache
                        hook(2, 0, 32, 2, 128, 2300, 4096),  # T behind the attention's LDS fit
                        hook(3, 64, 1, 0, 0, 0, 0)]}       # no such kernel
        ggml.set_option("plan_mpt_prompt", 1)
        out["set"] = [ggml.get_option("plan_mpt_prompt"), ggml.get_option("plan_mpt")]
        ggml.set_option("plan_mpt_prompt", 0)
        out["reset"] = ggml.get_option("plan_mpt_prompt")
        print(json.dumps(out))
    """)
    assert got == {"symbol": True, "bound": True, "method": True, "default": [0, 0], "stat": 0, "hook": [-1] * 8, "set": [1, 0], "reset": 0}


def test_the_environment_variable_sets_the_option():
    e = {k: v for k, v in os.environ.items() if not k.startswith("GGML_HIP_")}
    e["GGML_HIP_PLAN_MPT_PROMPT"] = "1"
    r = subprocess.run([sys.executable, "-c", "from llm_amd import ggml; print(ggml.get_option('plan_mpt_prompt'), ggml.get_option('plan_mpt'))"],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "1 0", (r.returncode, r.stdout, r.stderr[-2000:])
