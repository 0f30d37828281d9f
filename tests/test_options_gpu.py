"""The option table (g_options, llm_amd/csrc/backend_state.inc) on a device: every key reaches its own field, through the call and
through its environment variable; the option log wins over the environment; a change of a plan-shaping option drops the cached
plans and nothing else does; the timeline option reads back as its number of sampled workgroups.

Options are process-wide, so each case runs in a fresh child process under its own time limit.  The key lists are those of
tests/test_options.py: typed in from the setter this table replaced."""
import numpy as np
import pytest

from test_options import DEFAULTS, NO_ENV, child_json

pytestmark = pytest.mark.gpu

PLAIN = [k for k in DEFAULTS if k not in ("timeline", "w16_release", "serial_stage_slots", "act_quant")]
READ_ALL = """
        import json
        from llm_amd import ggml
        ggml.lib().ggml_init_hipblas()  # slot 0 exists from here on
"""


def held(value, key):
    return min(value, 64) if key == "chain_k" else value


def test_no_two_keys_share_a_field():
    want = {k: 2 + i for i, k in enumerate(PLAIN)}
    got = child_json(READ_ALL + """
        want = %r
        for k, v in want.items():
            ggml.set_option(k, v)
        print(json.dumps({k: ggml.get_option(k) for k in want}))
    """ % (want,))
    assert len(want) == 31
    assert got == {k: held(v, k) for k, v in want.items()}


def test_every_environment_variable_reaches_its_own_field():
    want = {k: 2 + i for i, k in enumerate(k for k in DEFAULTS if k not in NO_ENV and k != "act_quant")}
    env = {"GGML_HIP_" + k.upper(): str(v) for k, v in want.items()}
    env.update(GGML_HIP_ACT_QUANT="scalar", GGML_HIP_TIMELINE="1", GGML_HIP_PROBE="1")  # the last two are no variables of the library
    got = child_json(READ_ALL + """
        print(json.dumps({k: ggml.get_option(k) for k in %r}))
    """ % (list(want) + ["act_quant", "timeline", "probe"],), env=env)
    assert len(want) == 29
    assert got == dict({k: held(v, k) for k, v in want.items()}, act_quant=1, timeline=0, probe=0)


def test_the_log_wins_over_the_environment():
    got = child_json("""
        import json
        from llm_amd import ggml
        ggml.set_option("warm_mb", 16)  # before the first device call
        before = ggml.get_option("warm_mb")
        ggml.lib().ggml_init_hipblas()
        print(json.dumps([before, ggml.get_option("warm_mb")]))
    """, env={"GGML_HIP_WARM_MB": "8"})
    assert got == [16, 16]


DECODE = """
        import json
        import numpy as np
        from llm_amd import ggml, llama, synth
        hp, w = synth.make_llama(synth.TINY, ggml.TYPE_Q4_0)
        model = llama.Llama(hp, w, context_size=64)
        sess = model.start_session(n_batch=8)
        for t in (5, 9):
            sess.evaluate(np.array([t], np.int32))
        out = {"plans": [ggml.get_stat("plans")]}
        toggle = %r
        if toggle:
            ggml.set_option("affine", ggml.get_option("affine"))  # its present value
            out["plans"].append(ggml.get_stat("plans"))
            ggml.set_option("mmq_fuse", ggml.get_option("mmq_fuse") ^ 2)  # another value of an option no plan froze
            out["plans"].append(ggml.get_stat("plans"))
            ggml.set_option("affine", 1 - ggml.get_option("affine"))  # another value of one they did
            out["plans"].append(ggml.get_stat("plans"))
        logits = np.ascontiguousarray(sess.evaluate(np.array([13], np.int32))[-1], np.float32)
        out["logits"] = logits.view(np.uint32).tolist()
        out["plans_after"] = ggml.get_stat("plans")
        print(json.dumps(out))
"""


def test_a_changed_plan_option_drops_the_plans_and_the_token_after_it_is_the_same():
    quiet, toggled = child_json(DECODE % (False,)), child_json(DECODE % (True,))
    n = quiet["plans"][0]
    assert n > 0
    assert toggled["plans"] == [n, n, n, 0]
    assert toggled["plans_after"] > 0
    a, b = np.array(quiet["logits"], np.uint32), np.array(toggled["logits"], np.uint32)
    assert a.size > 0 and np.isfinite(a.view(np.float32)).all()
    assert np.array_equal(a, b)  # bit for bit


def test_timeline_reads_back_as_its_sampled_workgroups():
    got = child_json(READ_ALL + """
        out = []
        for v in (1, 6, 0):
            ggml.set_option("timeline", v)
            out.append(ggml.get_option("timeline"))
        print(json.dumps(out))
    """)
    assert got == [4, 6, 0]
