"""CPU tests of the runtime options and counters (ggml_hip_set_option / ggml_hip_get_option / ggml_hip_get_stat): no GPU, no
device call.  The library keeps ONE table of options (g_options, llm_amd/csrc/backend_state.inc); the lists below are what the
hand-written setter, the Backend initialisers and the counter chain held before that table existed, typed in, never read from the
table — a row that loses its key, its default or its field shows here or in tests/test_options_gpu.py.

Options are process-wide and logged, so everything that sets one runs in a child process: nothing leaks into the tests that
share this interpreter."""
import json
import os
import signal
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULTS = dict(
    fuse=1, plan=1, plan_k=1, plan_multi=1, plan_prompt=1, graph=1, big=1, kbig=1, chain_k=0, prepare=1, speculate_next=0,
    fuse_attn=1, fuse_wo=1, warm_mb=24, affine=1, fuse_heads=1, attn_split=1, attn_one=1, fused_fallback=1, fused_rearm_tokens=256,
    act_quant=0, mmq_i8=0, mmq_min=32, k_prompt_min=12, mmq_fuse=3, mmq_cols=1, mmq_t256=1, attn_fused=1, mmq_w16=1,
    w16_headroom_gb=16, probe=0, test_fused_timeout=0,
    timeline=0, serial_stage_slots=0,  # state outside Backend's opt_* fields: no buffer, no stages
    w16_release=-1)                    # an action: holds nothing
DEVICE_KEYS = ("timeline", "act_quant", "w16_release", "mmq_w16")  # need an initialised device: only logged without one
NO_ENV = ("timeline", "w16_release", "serial_stage_slots", "test_fused_timeout", "probe")
COUNTERS = (  # every key ggml_hip_get_stat answered, but num_cus (it initialises a device)
    "attn_split_tokens", "w16_bytes", "mmq_launches_plain", "mmq_launches_dma_p8", "mmq_launches_w16_p8", "mmq_launches_w16_256",
    "mmq_launches_i8", "prompt_plan_tokens", "plan_tokens", "graph_replays", "plans", "fused_attn_timeouts", "fused_heads_tokens",
    "kplan_tokens", "spec_hits", "spec_misses", "fused_wo_tokens", "fused_affine_tokens", "prepared_tokens", "cols_warm_launches",
    "fused_rearms", "fused_attn_tokens", "peak_concurrent_calls", "generic_graphs", "alibi_fused", "ns_match", "ns_launch",
    "ns_wait", "ns_compute", "ns_mirror", "mirror_bytes")


def child(code, env=None, timeout=120):
    """Runs `code` in a fresh interpreter without any GGML_HIP_* variable but those of `env`."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("GGML_HIP_")}
    e.update(env or {})
    return subprocess.run([sys.executable, "-c", textwrap.dedent(code)], cwd=ROOT, env=e, capture_output=True, text=True,
                          timeout=timeout)


def child_json(code, env=None, timeout=120):
    r = child(code, env, timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def answers():
    """One child, no device: the defaults, then every key set, then read back."""
    settable = {k: 2 + i for i, k in enumerate(k for k in DEFAULTS if k not in DEVICE_KEYS)}
    return settable, child_json("""
        import json
        from llm_amd import ggml
        keys, settable, counters = %r, %r, %r
        out = {"defaults": {k: ggml.get_option(k) for k in keys}}
        out["stats"] = {k: ggml.get_stat(k) for k in counters}
        out["unknown_stats"] = [ggml.get_stat("nope"), ggml.get_stat("mmq_launches_nope"), ggml.get_stat("")]
        for k, v in settable.items():
            ggml.set_option(k, v)
        out["logged"] = {k: ggml.get_option(k) for k in settable}
        ggml.set_option("chain_k", 100)
        hi = ggml.get_option("chain_k")
        ggml.set_option("chain_k", -5)
        out["chain_k"] = [hi, ggml.get_option("chain_k")]
        for k in %r:  # accepted without a device: logged (the action is not), applied by the slot that comes later
            ggml.set_option(k, 0)
        out["w16_release"] = ggml.get_option("w16_release")
        print(json.dumps(out))
    """ % (list(DEFAULTS), settable, list(COUNTERS), list(DEVICE_KEYS)))


def test_the_lists_of_this_file_are_consistent():
    assert len(DEFAULTS) == 35 and set(DEVICE_KEYS) <= set(DEFAULTS) and set(NO_ENV) <= set(DEFAULTS)


def test_every_default_is_the_initialiser_it_always_was(answers):
    assert answers[1]["defaults"] == DEFAULTS


def test_every_key_that_needs_no_device_is_accepted_without_one_and_reads_back(answers):
    settable, got = answers
    assert len(settable) == 31 and len(set(settable.values())) == 31
    assert got["logged"] == settable
    assert got["chain_k"] == [64, 0]  # what a slot would hold for 100 and for -5
    assert got["w16_release"] == -1


def test_every_counter_answers_and_an_unknown_one_is_minus_one(answers):
    stats = answers[1]["stats"]
    assert sorted(stats) == sorted(COUNTERS)
    assert all(v >= 0 for v in stats.values()), stats
    assert answers[1]["unknown_stats"] == [-1, -1, -1]


@pytest.mark.parametrize("call", ['set_option("nope", 1)', 'get_option("nope")'])
def test_an_unknown_key_aborts_with_a_message(call):
    r = child("""
        from llm_amd import ggml
        print("BEFORE", flush=True)
        ggml.%s
        print("SURVIVED", flush=True)
    """ % call)
    assert "BEFORE" in r.stdout and "SURVIVED" not in r.stdout
    assert r.returncode == -signal.SIGABRT
    assert "ggml_hip_%s: unknown key 'nope'" % call.split("(")[0] in r.stderr
