"""CPU pins of the ALiBi families (BLOOM, MPT): the restatement in tests/alibi_ref.py, in math mode, against Hugging
Face transformers' BloomForCausalLM / MptForCausalLM on the same dequantized weights (tests/golden/make_hf_alibi_golden.py),
for the TINY models (4 heads) and their 12-head variants (heads 8..11 take ggml's second slope sequence).  An
independent implementation fixes the slopes and the sign of the bias, the [Q | K | V] fused-QKV layout and the rest of
both graphs.  Measured (restatement vs HF, max|d| / std of the logits): BLOOM 5.2e-5, BLOOM 12-head 8.4e-5, MPT 7.4e-4,
MPT 12-head 6.1e-4 (HF runs f32 with f32 K/V; the restatement rounds K/V to f16, the reference's cache type); argmax
identical at every position."""
import os

import numpy as np
import pytest

import alibi_ref
from llm_amd import bloom, mpt
from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILIES = {"bloom": (bloom.make_bloom, alibi_ref.Bloom, {"": bloom.BLOOM_TINY, "_12h": bloom.BLOOM_TINY_12H}),
            "mpt": (mpt.make_mpt, alibi_ref.Mpt, {"": mpt.MPT_TINY, "_12h": mpt.MPT_TINY_12H})}


def _math_vs_hf(family, variant):
    make, Ref, hps = FAMILIES[family]
    z = np.load(os.path.join(GOLD, f"hf_{family}_tiny.npz"))
    hp, w = make(hps[variant], int(z["wtype"]), seed=int(z["seed"]), quantize=O.quantize)
    got = Ref(hp, w).evaluate(z["tokens"], mode=O.MODE_MATH)
    hf = z["logits" + variant]
    return got, hf, float(np.max(np.abs(got - hf)) / hf.std())


@pytest.mark.parametrize("variant", ["", "_12h"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_math_mode_matches_huggingface_golden(family, variant):
    got, hf, d = _math_vs_hf(family, variant)
    assert d <= 1e-3, d
    assert (np.argmax(got, -1) == np.argmax(hf, -1)).all()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_golden_pins_the_second_slope_sequence(family, monkeypatch):
    """The 12-head fixture tells the slopes of heads 8..11 apart: giving every head the first sequence's m0^(k+1)
    moves the restatement far outside the tolerance."""
    def first_sequence_only(n_head, bias_max):
        m0 = np.float32(alibi_ref._libm.powf(np.float32(2.0), -np.float32(bias_max) / np.float32(8)))
        return np.array([alibi_ref._libm.powf(m0, np.float32(k + 1)) for k in range(n_head)], np.float32)

    monkeypatch.setattr(alibi_ref, "slopes", first_sequence_only)
    _, _, d = _math_vs_hf(family, "_12h")
    assert d > 2e-2, d


@pytest.mark.parametrize("family", list(FAMILIES))
def test_restatement_prompt_then_decode_is_consistent(family):
    """One pass over 6 tokens and 5 + 1 tokens with the cache carried: the same last-token logits (ggml-exact mode)."""
    make, Ref, hps = FAMILIES[family]
    hp, w = make(hps["_12h"], 2, seed=3, quantize=O.quantize)
    a = Ref(hp, w)
    a.evaluate(np.arange(1, 6, dtype=np.int32), mode=0)
    last = a.evaluate(np.array([6], np.int32), mode=0)
    whole = Ref(hp, w).evaluate(np.arange(1, 7, dtype=np.int32), mode=0)
    assert np.array_equal(last[-1], whole[-1])
