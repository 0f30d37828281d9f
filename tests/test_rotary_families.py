"""CPU pins of the rotary-embedding families (GPT-NeoX, Falcon): the restatement in tests/rotary_ref.py, in math mode,
against Hugging Face transformers' GPTNeoXForCausalLM / FalconForCausalLM on the same dequantized weights
(tests/golden/make_hf_rotary_golden.py).  An independent implementation fixes the NeoX pairing convention
(x[i] with x[i + n_dims/2]) and the fused-QKV layouts of both graphs, as test_llama_math_mode_matches_huggingface_golden
does for LLaMA."""
import os

import numpy as np
import pytest

import rotary_ref
from llm_amd import falcon, gptj, gptneox
from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("family", ["gptneox", "falcon"])
def test_math_mode_matches_huggingface_golden(family):
    z = np.load(os.path.join(GOLD, f"hf_{family}_tiny.npz"))
    if family == "gptneox":
        hp, w = gptneox.make_gptneox(gptneox.GPTNEOX_TINY, int(z["wtype"]), seed=int(z["seed"]), quantize=O.quantize)
        ref = rotary_ref.GptNeoX(hp, w)
    else:
        hp, w = falcon.make_falcon(falcon.FALCON_TINY, int(z["wtype"]), seed=int(z["seed"]), quantize=O.quantize)
        ref = rotary_ref.Falcon(hp, w)
    got = ref.evaluate(z["tokens"], mode=O.MODE_MATH)
    hf = z["logits"]
    # HF runs f32 with f32 K/V; the restatement rounds K/V to f16 (the reference's cache type): ~7e-4 of logits std
    assert np.max(np.abs(got - hf)) / hf.std() < 5e-3, np.max(np.abs(got - hf)) / hf.std()
    assert (np.argmax(got, -1) == np.argmax(hf, -1)).all()


def test_rope_neox_full_head_is_rotate_half():
    """n_dims == ne0: ggml's NeoX loop is HF's rotate_half with inv_freq = base^(-2i/n_dims) (to f32 rounding)."""
    x = np.random.default_rng(0).standard_normal((3, 2, 16)).astype(np.float32)
    P, D = 5, 16
    got = rotary_ref.rope_neox(x, P, D)
    ang = (P + np.arange(3))[:, None, None] * 10000.0 ** (-np.arange(0, D, 2) / D)[None, None, :]
    c, s = np.cos(np.concatenate([ang, ang], -1)), np.sin(np.concatenate([ang, ang], -1))
    rot = np.concatenate([-x[..., D // 2:], x[..., :D // 2]], -1)
    assert np.allclose(got, x * c + rot * s, atol=1e-5)


def test_rope_neox_partial_blocks_and_tail():
    """n_dims < ne0: every whole n_dims block is rotated, theta running on across blocks; the tail is untouched."""
    x = np.random.default_rng(1).standard_normal((2, 3, 40)).astype(np.float32)
    y = rotary_ref.rope_neox(x, 7, 16)
    assert np.array_equal(y[..., 32:], x[..., 32:])
    assert not np.allclose(y[..., 16:32], x[..., 16:32])
    # the second block continues where the first stopped: theta_k = p * s^k with k = 8..15
    s = np.float32(10000.0) ** np.float32(-2.0 / 16)
    th = np.float64(7) * np.float64(s) ** np.arange(8, 16)
    exp = x[0, :, 16:24] * np.cos(th) - x[0, :, 24:32] * np.sin(th)
    assert np.allclose(y[0, :, 16:24], exp, atol=1e-4)


def test_rope_neox_mode1_skips_past_rows():
    x = np.random.default_rng(2).standard_normal((4, 1, 8)).astype(np.float32)
    y = rotary_ref.rope_neox(x, 2, 8, mode=3)
    assert np.array_equal(y[:2], x[:2])
    assert np.array_equal(y[2:], rotary_ref.rope_neox(x, 0, 8, mode=3)[2:])


@pytest.mark.parametrize("family", ["gptneox", "gptneox_seq", "falcon", "falcon40", "gptj"])
def test_restatement_prompt_then_decode_is_consistent(family):
    """One pass over 6 tokens and 5 + 1 tokens with the cache carried: the same last-token logits (ggml-exact mode)."""
    mk = {"gptneox": (gptneox.make_gptneox, gptneox.GPTNEOX_TINY, rotary_ref.GptNeoX),
          "gptneox_seq": (gptneox.make_gptneox, dict(gptneox.GPTNEOX_TINY, n_rot=8, use_parallel_residual=False),
                          rotary_ref.GptNeoX),
          "falcon": (falcon.make_falcon, falcon.FALCON_TINY, rotary_ref.Falcon),
          "falcon40": (falcon.make_falcon, falcon.FALCON_40B_TINY, rotary_ref.Falcon),
          "gptj": (gptj.make_gptj, gptj.GPTJ_TINY, rotary_ref.GptJ)}[family]
    hp, w = mk[0](mk[1], 2, seed=3, quantize=O.quantize)
    a = mk[2](hp, w)
    a.evaluate(np.arange(1, 6, dtype=np.int32), mode=0)
    last = a.evaluate(np.array([6], np.int32), mode=0)
    whole = mk[2](hp, w).evaluate(np.arange(1, 7, dtype=np.int32), mode=0)
    assert np.array_equal(last[-1], whole[-1])
