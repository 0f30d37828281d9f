"""GPU parity of the rotary-embedding families: GPT-NeoX (crates/models/gptneox), Falcon (crates/models/falcon) and
GPT-J (crates/models/gptj), built through the C ABI (llm_amd/{gptneox,falcon,gptj}.py) and executed node by node on
the MI355X, against the CPU restatement of tests/rotary_ref.py in the reference's branch (O.ref_mode()) on identical
synthetic GGML weights, with the device's K/V cache copied into the restatement before every step.

Stated tolerance, as for GPT-2 (tests/test_gpt2_gpu.py): chunks that hit no rounding edge of the int8 activation
re-quantization agree to STRICT = 1e-5·std; a flipped quant moves the logits of these random-init models by a few
1e-2·std, so every chunk must be within EDGE = 4e-2.  Measured on an MI355X:
  TINY (5 variants x wtypes 2/3/6/7/8, 6 chunks each): 138 of 150 chunks within STRICT (2.4e-7 … 1.7e-6), the rest
  4.3e-3 … 3.8e-2 (worst: GPT-NeoX sequential, partial rotary, Q5_1); rule: all within EDGE, at least half within STRICT.
  Real widths (2 layers, Q4_0, 5 chunks each): worst 2.6e-2 (Pythia-1.4B), 2.3e-2 (Falcon-7B), 2.4e-2 (GPT-J-6B).  A
  token at these widths re-quantizes 16-36x more activations than at 128, so a chunk without any flip is the exception
  (measured 3/5, 1/5, 0/5 within STRICT): the rule there is every chunk within EDGE.  Anything structural (a wrong
  pairing, layout or position) is O(1)·std."""
import numpy as np
import pytest

import rotary_ref
from llm_amd import falcon, gptj, gptneox

pytestmark = pytest.mark.gpu

STRICT, EDGE = 1e-5, 4e-2

VARIANTS = {
    "gptneox_parallel": (gptneox.make_gptneox, gptneox.GptNeoX, rotary_ref.GptNeoX, gptneox.GPTNEOX_TINY),
    "gptneox_sequential_partial": (gptneox.make_gptneox, gptneox.GptNeoX, rotary_ref.GptNeoX,
                                   dict(gptneox.GPTNEOX_TINY, n_rot=8, use_parallel_residual=False)),
    "falcon_7b": (falcon.make_falcon, falcon.Falcon, rotary_ref.Falcon, falcon.FALCON_TINY),
    "falcon_40b": (falcon.make_falcon, falcon.Falcon, rotary_ref.Falcon, falcon.FALCON_40B_TINY),
    "gptj": (gptj.make_gptj, gptj.GptJ, rotary_ref.GptJ, gptj.GPTJ_TINY),
}

REAL = {  # real widths, 2 layers and a 512-entry vocabulary
    "pythia_1_4b": (gptneox.make_gptneox, gptneox.GptNeoX, rotary_ref.GptNeoX,
                    dict(gptneox.PYTHIA_1_4B, n_layer=2, n_vocab=512, n_ctx=64)),
    "falcon_7b": (falcon.make_falcon, falcon.Falcon, rotary_ref.Falcon,
                  dict(falcon.FALCON_7B, n_layer=2, n_vocab=512, n_ctx=64)),
    "gptj_6b": (gptj.make_gptj, gptj.GptJ, rotary_ref.GptJ, dict(gptj.GPTJ_6B, n_layer=2, n_vocab=512, n_ctx=64)),
}


def _run_chunks(O, model, ref, chunks):
    """Per chunk: device logits vs the restatement at the device's K/V state; returns the per-chunk |Δ|max/std."""
    out = []
    for chunk in chunks:
        got = model.evaluate(chunk)
        ref.memory_k[:] = model.memory_k.device_get(np.float16).reshape(ref.memory_k.shape)  # same K/V state
        ref.memory_v[:] = model.memory_v.device_get(np.float16).reshape(ref.memory_v.shape)
        ref.n_past = model.n_past - len(chunk)
        want = ref.evaluate(chunk, mode=O.ref_mode())
        out.append(float(np.max(np.abs(got - want))) / float(want.std()))
    return out


@pytest.mark.parametrize("wtype", [2, 3, 6, 7, 8])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_logits_match_restatement_prompt_and_decode(G, O, variant, wtype):
    make, Dev, Ref, hp0 = VARIANTS[variant]
    hp, w = make(hp0, wtype, seed=5)
    model = Dev(hp, w)
    toks = np.random.default_rng(6).integers(0, hp["n_vocab"], 12).astype(np.int32)
    chunks = (toks[:5], toks[5:8]) + tuple(toks[8 + i:9 + i] for i in range(4))
    try:
        d = _run_chunks(O, model, Ref(hp, w), chunks)
    finally:
        model.free()
    print(f"{variant} type {wtype}: worst {max(d):.2e}, {sum(x <= STRICT for x in d)}/{len(d)} within {STRICT}", d)
    assert max(d) <= EDGE, d
    assert sum(x <= STRICT for x in d) >= len(d) // 2, d


@pytest.mark.parametrize("family", list(REAL))
def test_real_width_q4_0_prompt_and_decode(G, O, family):
    make, Dev, Ref, hp0 = REAL[family]
    hp, w = make(hp0, G.TYPE_Q4_0, seed=7)
    model = Dev(hp, w)
    toks = np.random.default_rng(8).integers(0, hp["n_vocab"], 12).astype(np.int32)
    chunks = (toks[:8],) + tuple(toks[8 + i:9 + i] for i in range(4))
    try:
        d = _run_chunks(O, model, Ref(hp, w), chunks)
    finally:
        model.free()
    print(f"{family} real width: worst {max(d):.2e}, {sum(x <= STRICT for x in d)}/{len(d)} within {STRICT}", d)
    assert max(d) <= EDGE, d  # no STRICT quota at these widths: see the module docstring


@pytest.mark.parametrize("variant", ["gptneox_parallel", "falcon_7b", "gptj"])
def test_greedy_is_deterministic(G, variant):
    make, Dev, _, hp0 = VARIANTS[variant]
    hp, w = make(hp0, 2, seed=5)
    outs = []
    for _ in range(2):
        model = Dev(hp, w)
        lg = model.evaluate(np.array([3, 1, 4, 1, 5], np.int32))[-1]
        seq = []
        for _ in range(10):
            tok = int(np.argmax(lg))
            seq.append(tok)
            lg = model.evaluate(np.array([tok], np.int32))[-1]
        outs.append(seq)
        model.free()
    assert outs[0] == outs[1]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_llama_plan_does_not_pick_up_these_graphs(G, variant):
    """Single-token steps of these graphs run on the generic executor, never on the fused LLaMA decode plan."""
    make, Dev, _, hp0 = VARIANTS[variant]
    hp, w = make(hp0, 2, seed=5)
    model = Dev(hp, w)
    try:
        model.evaluate(np.array([3, 1, 4], np.int32))
        g0, p0 = G.get_stat("generic_graphs"), G.get_stat("plan_tokens")
        for tok in (1, 5, 9):
            model.evaluate(np.array([tok], np.int32))
        assert G.get_stat("generic_graphs") == g0 + 3
        assert G.get_stat("plan_tokens") == p0
    finally:
        model.free()
