"""Generates tests/golden/hf_bloom_tiny.npz and hf_mpt_tiny.npz: logits of Hugging Face transformers' BloomForCausalLM
and MptForCausalLM on the dequantized synthetic weights of llm_amd.bloom / llm_amd.mpt, for the TINY model (4 heads)
and a 12-head variant (n_embd 192) whose heads 8..11 take ggml's second slope sequence.  They pin the ALiBi slopes and
sign, the [Q | K | V] fused-QKV layout and the rest of both graphs with an implementation independent of this project.
Run in the build container (needs torch + transformers; neither is needed to USE the fixtures):
    python tests/golden/make_hf_alibi_golden.py
Four adaptations, all on the HF side:
  * HF BLOOM's query_key_value interleaves per head ([H, 3, D] rows); ggml's graph views [Q | K | V] blocks of n_embd
    rows (bloom lib.rs:166-185), so the ggml rows and bias are permuted into HF's order;
  * HF BLOOM ties lm_head to the embeddings; the ggml model has its own output.weight: untied and loaded;
  * HF MPT's MLP uses erf GELU; it is swapped for nn.GELU(approximate="tanh"), the function ggml's GELU approximates,
    so the fixture pins the architecture and not the GELU approximation;
  * HF BLOOM adds i·m to the scores and HF MPT (i - T + 1)·m: a constant per row, which softmax cancels."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from llm_amd import bloom, mpt  # noqa: E402
from oracle import oracle as O  # noqa: E402
import alibi_ref  # noqa: E402
from transformers import BloomConfig, BloomForCausalLM, MptConfig, MptForCausalLM  # noqa: E402

WTYPE, SEED = 2, 1234
HERE = os.path.dirname(os.path.abspath(__file__))


def dense(shapes, w):
    return {n: w[n] if ne1 is None else O.dequantize(WTYPE, w[n], ne0 * ne1).reshape(ne1, ne0)
            for n, (ne0, ne1) in shapes.items()}


def bloom_state(hp, w):
    E, H = hp["n_embd"], hp["n_head"]
    D = E // H
    g = dense(bloom.tensor_shapes(hp), w)
    sd = {"transformer.word_embeddings.weight": g["tok_embeddings.weight"],
          "transformer.word_embeddings_layernorm.weight": g["norm.weight"],
          "transformer.word_embeddings_layernorm.bias": g["norm.bias"],
          "transformer.ln_f.weight": g["output_norm.weight"], "transformer.ln_f.bias": g["output_norm.bias"],
          "lm_head.weight": g["output.weight"]}
    for i in range(hp["n_layer"]):
        p, h = f"layers.{i}.", f"transformer.h.{i}."
        qkv_w = g[p + "attention.query_key_value.weight"].reshape(3, H, D, E).transpose(1, 0, 2, 3).reshape(3 * E, E)
        qkv_b = g[p + "attention.query_key_value.bias"].reshape(3, H, D).transpose(1, 0, 2).reshape(3 * E)
        sd.update({h + "input_layernorm.weight": g[p + "attention_norm.weight"],
                   h + "input_layernorm.bias": g[p + "attention_norm.bias"],
                   h + "self_attention.query_key_value.weight": qkv_w, h + "self_attention.query_key_value.bias": qkv_b,
                   h + "self_attention.dense.weight": g[p + "attention.wo.weight"],
                   h + "self_attention.dense.bias": g[p + "attention.wo.bias"],
                   h + "post_attention_layernorm.weight": g[p + "ffn_norm.weight"],
                   h + "post_attention_layernorm.bias": g[p + "ffn_norm.bias"],
                   h + "mlp.dense_h_to_4h.weight": g[p + "feed_forward.w1.weight"],
                   h + "mlp.dense_h_to_4h.bias": g[p + "feed_forward.w1.bias"],
                   h + "mlp.dense_4h_to_h.weight": g[p + "feed_forward.w2.weight"],
                   h + "mlp.dense_4h_to_h.bias": g[p + "feed_forward.w2.bias"]})
    return sd


def bloom_model(hp):
    cfg = BloomConfig(vocab_size=hp["n_vocab"], hidden_size=hp["n_embd"], n_layer=hp["n_layer"], n_head=hp["n_head"],
                      layer_norm_epsilon=1e-5, apply_residual_connection_post_layernorm=False,
                      tie_word_embeddings=False, attn_implementation="eager")
    return BloomForCausalLM(cfg)


def mpt_state(hp, w):
    sd = dict(dense(mpt.tensor_shapes(hp), w))
    sd["lm_head.weight"] = sd["transformer.wte.weight"]  # tied (mpt lib.rs:244)
    return sd


def mpt_model(hp):
    cfg = MptConfig(d_model=hp["n_embd"], n_heads=hp["n_head"], n_layers=hp["n_layer"], expansion_ratio=4,
                    max_seq_len=hp["n_ctx"], vocab_size=hp["n_vocab"], layer_norm_epsilon=1e-5, no_bias=True,
                    attn_config={"alibi": True, "alibi_bias_max": int(hp["alibi_bias_max"]), "clip_qkv": None},
                    attn_implementation="eager")
    model = MptForCausalLM(cfg)
    for blk in model.transformer.blocks:
        blk.ffn.act = torch.nn.GELU(approximate="tanh")
    return model


def logits_of(model, sd, toks):
    res = model.load_state_dict({k: torch.tensor(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    with torch.no_grad():
        return model.to(torch.float32).eval()(torch.tensor(toks)[None]).logits[0].numpy().astype(np.float32)


def run(name, variants, make, state, model_of, ref_cls):
    out = dict(wtype=WTYPE, seed=SEED)
    for key, hp0 in variants.items():
        hp, w = make(hp0, WTYPE, seed=SEED, quantize=O.quantize)
        toks = np.random.default_rng(42).integers(0, hp["n_vocab"], 12).astype(np.int64)
        torch.manual_seed(0)
        logits = logits_of(model_of(hp), state(hp, w), toks)
        out["tokens"] = toks.astype(np.int32)
        out["logits" + key] = logits
        got = ref_cls(hp, w).evaluate(toks.astype(np.int32), mode=O.MODE_MATH)
        print(name + key, "restatement(math) vs HF: max|d|/std =", float(np.max(np.abs(got - logits)) / logits.std()),
              "argmax equal:", bool((got.argmax(-1) == logits.argmax(-1)).all()))
    np.savez_compressed(os.path.join(HERE, f"hf_{name}_tiny.npz"), **out)


run("bloom", {"": bloom.BLOOM_TINY, "_12h": bloom.BLOOM_TINY_12H}, bloom.make_bloom, bloom_state, bloom_model,
    alibi_ref.Bloom)
run("mpt", {"": mpt.MPT_TINY, "_12h": mpt.MPT_TINY_12H}, mpt.make_mpt, mpt_state, mpt_model, alibi_ref.Mpt)
