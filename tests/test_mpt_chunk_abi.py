"""CPU tests of the MPT chunk plan's boundary (no GPU): option plan_mpt_chunk and counter mpt_chunk_tokens exist, default to 0 and read
back beside their neighbours; the option's environment variable sets it.  Everything runs in a child process: an abort must fail a
test, not end the run."""
import os
import subprocess
import sys

from test_mpt_plan_abi import ROOT, child_json


def test_option_and_counter_without_a_device():
    got = child_json("""
        import json
        from llm_amd import ggml
        opts = lambda: [ggml.get_option(k) for k in ("plan_mpt_chunk", "plan_mpt_prompt", "plan_mpt")]
        out = {"default": opts(), "stat": ggml.get_stat("mpt_chunk_tokens")}
        ggml.set_option("plan_mpt_chunk", 1)
        out["set"] = opts()
        ggml.set_option("plan_mpt_chunk", 0)
        out["reset"] = opts()
        print(json.dumps(out))
    """)
    assert got == {"default": [0, 0, 0], "stat": 0, "set": [1, 0, 0], "reset": [0, 0, 0]}


def test_the_environment_variable_sets_the_option():
    e = {k: v for k, v in os.environ.items() if not k.startswith("GGML_HIP_")}
    e["GGML_HIP_PLAN_MPT_CHUNK"] = "1"
    r = subprocess.run([sys.executable, "-c", "from llm_amd import ggml; print(ggml.get_option('plan_mpt_chunk'), ggml.get_option('plan_mpt_prompt'))"],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "1 0", (r.returncode, r.stdout, r.stderr[-2000:])
