"""CPU tests of the BLOOM plan's boundary (no GPU): option plan_bloom and counter bloom_plan_tokens exist, default to 0 and read back; the test
hook is exported and bound and refuses what it can refuse before it touches a device; Bloom.infer_tokens_device exists; the option's
environment variable sets it.  Everything runs in a child process: an abort must fail a test, not end the run."""
import json
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(code, env=()):
    e = {k: v for k, v in os.environ.items() if not k.startswith("GGML_HIP_")}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_option_counter_hook_and_method_without_a_device():
    got = child("""
        import ctypes as C, json
        from llm_amd import ggml, bloom
        L = ggml.lib()
        x = (C.c_float * 64)()
        p = C.addressof(x)
        outs = (C.c_void_p * 4)(*([p] * 4))
        hook = lambda op, flag, w, xx, gain, K, o: L.ggml_hip_debug_bloom(op, flag, w, xx, gain, gain, 1e-5, K, p, p, 0, 0, 8, p, p, o)
        out = {"symbol": hasattr(C.CDLL(ggml.LIB_PATH), "ggml_hip_debug_bloom"), "bound": "ggml_hip_debug_bloom" in ggml.PROTOTYPES,
               "method": hasattr(bloom.Bloom, "infer_tokens_device"),
               "default": ggml.get_option("plan_bloom"), "stat": ggml.get_stat("bloom_plan_tokens"),
               "hook": [hook(0, 1, None, None, p, 64, outs),    # no row
                        hook(0, 1, None, p, None, 64, outs),    # no gain, no bias
                        hook(0, 1, None, p, p, 48, outs),       # not whole blocks
                        hook(0, 1, None, p, p, 16384, outs),    # wider than the staging
                        hook(0, 1, None, p, p, 64, None),       # nowhere to put the blocks
                        hook(1, 9, None, p, p, 64, outs),       # no matrix
                        hook(2, 0, None, p, p, 64, outs),       # no embedding
                        hook(3, 0, None, p, p, 64, outs)]}      # no such op
        ggml.set_option("plan_bloom", 1)
        out["set"] = ggml.get_option("plan_bloom")
        ggml.set_option("plan_bloom", 0)
        out["reset"] = ggml.get_option("plan_bloom")
        print(json.dumps(out))
    """)
    assert got == {"symbol": True, "bound": True, "method": True, "default": 0, "stat": 0, "hook": [-1] * 8, "set": 1, "reset": 0}


def test_the_environment_variable_sets_the_option():
    assert child("import json; from llm_amd import ggml; print(json.dumps(ggml.get_option('plan_bloom')))", {"GGML_HIP_PLAN_BLOOM": "1"}) == 1
