"""CPU tests of the switch of batched decode for K-quant models (no GPU, no device call): option plan_batch_k exists, defaults to 0
(three GPU tests written before it pin that a Q4_K model at default options is declined), is settable, follows its environment
variable GGML_HIP_PLAN_BATCH_K, and the counter batch_k_steps answers.  Everything runs in a child process, as tests/test_options.py
runs its own: options are process-wide, and an unknown key aborts — which must fail a test, not end the run."""
import json
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child_json(code, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("GGML_HIP_")}
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_option_reads_0_is_settable_and_the_counter_answers_0():
    got = child_json("""
        import json
        from llm_amd import ggml
        out = {"default": ggml.get_option("plan_batch_k"), "counter": ggml.get_stat("batch_k_steps")}
        ggml.set_option("plan_batch_k", 1)
        out["set"] = ggml.get_option("plan_batch_k")
        ggml.set_option("plan_batch_k", 0)
        out["back"] = ggml.get_option("plan_batch_k")
        out["neighbours"] = [ggml.get_option(k) for k in ("plan_batch", "plan_k")]
        print(json.dumps(out))
    """)
    assert got == {"default": 0, "counter": 0, "set": 1, "back": 0, "neighbours": [1, 1]}


def test_the_environment_variable_turns_it_on_and_a_set_value_wins_over_it():
    code = """
        import json
        from llm_amd import ggml
        out = {"env": ggml.get_option("plan_batch_k"), "plan_batch": ggml.get_option("plan_batch")}
        ggml.set_option("plan_batch_k", 0)
        out["set"] = ggml.get_option("plan_batch_k")
        print(json.dumps(out))
    """
    assert child_json(code, {"GGML_HIP_PLAN_BATCH_K": "1"}) == {"env": 1, "plan_batch": 1, "set": 0}
    assert child_json(code, {"GGML_HIP_PLAN_BATCH_K": "0"}) == {"env": 0, "plan_batch": 1, "set": 0}
    assert child_json(code) == {"env": 0, "plan_batch": 1, "set": 0}


def test_the_row_drops_plans_and_its_default_is_documented_as_provisional():
    src = open(os.path.join(ROOT, "llm_amd", "csrc", "backend_state.inc")).read()
    assert '{"plan_batch_k", &Backend::opt_plan_batch_k, OPT_ENV | OPT_DROPS},' in src
    assert '{"batch_k_steps", &Backend::stat_batch_k_steps}' in src
    for name in ("DESIGN.md", "README.md"):
        doc = open(os.path.join(ROOT, name)).read()
        assert "plan_batch_k" in doc, name
