"""Generates tests/golden/hf_gptneox_tiny.npz and hf_falcon_tiny.npz: logits of Hugging Face transformers'
GPTNeoXForCausalLM (rotary over the whole head) and FalconForCausalLM (7B form: multi-query, parallel attention, no
biases) on the dequantized synthetic TINY weights of llm_amd.gptneox / llm_amd.falcon.  They pin the NeoX pairing
convention (x[i], x[i + n_dims/2]) and the fused-QKV layouts with an implementation independent of this project.
Run in the build container (needs torch + transformers; neither is needed to USE the fixtures):
    python tests/golden/make_hf_rotary_golden.py
HF's tanh GELU ("gelu_new") is the function ggml's GELU approximates; the tensor names are the same on both
sides but for GPT-NeoX's head (embed_out in the checkpoints, lm_head in this transformers version's module)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from llm_amd import falcon, gptneox  # noqa: E402
from oracle import oracle as O  # noqa: E402
import rotary_ref  # noqa: E402
from transformers import FalconConfig, FalconForCausalLM, GPTNeoXConfig, GPTNeoXForCausalLM  # noqa: E402

WTYPE, SEED = 2, 1234
HERE = os.path.dirname(os.path.abspath(__file__))


def hf_state(shapes, w, rename=None):
    sd = {}
    for name, (ne0, ne1) in shapes.items():
        sd[(rename or {}).get(name, name)] = w[name] if ne1 is None else O.dequantize(WTYPE, w[name], ne0 * ne1).reshape(ne1, ne0)
    return {k: torch.tensor(np.ascontiguousarray(v)) for k, v in sd.items()}


def run(name, hp, w, shapes, model, ref_cls, rename=None):
    missing = model.load_state_dict(hf_state(shapes, w, rename), strict=False)
    assert not [k for k in missing.missing_keys if "rotary" not in k and "inv_freq" not in k], missing
    assert not missing.unexpected_keys, missing
    toks = np.random.default_rng(42).integers(0, hp["n_vocab"], 12).astype(np.int64)
    with torch.no_grad():
        logits = model.eval()(torch.tensor(toks)[None]).logits[0].numpy().astype(np.float32)
    np.savez_compressed(os.path.join(HERE, f"hf_{name}_tiny.npz"), wtype=WTYPE, seed=SEED, tokens=toks.astype(np.int32),
                        logits=logits)
    got = ref_cls(hp, w).evaluate(toks.astype(np.int32), mode=O.MODE_MATH)
    print(name, "restatement(math) vs HF: max|d|/std =", float(np.max(np.abs(got - logits)) / logits.std()),
          "argmax equal:", bool((got.argmax(-1) == logits.argmax(-1)).all()))


torch.manual_seed(0)
hp, w = gptneox.make_gptneox(gptneox.GPTNEOX_TINY, WTYPE, seed=SEED, quantize=O.quantize)
E, H = hp["n_embd"], hp["n_head"]
assert hp["n_rot"] == E // H
cfg = GPTNeoXConfig(vocab_size=hp["n_vocab"], hidden_size=E, num_hidden_layers=hp["n_layer"], num_attention_heads=H,
                    intermediate_size=4 * E, hidden_act="gelu_new", max_position_embeddings=hp["n_ctx"],
                    layer_norm_eps=1e-5, use_parallel_residual=hp["use_parallel_residual"], tie_word_embeddings=False,
                    rope_parameters={"rope_type": "default", "rope_theta": 10000.0, "partial_rotary_factor": 1.0},
                    attn_implementation="eager")
run("gptneox", hp, w, gptneox.tensor_shapes(hp), GPTNeoXForCausalLM(cfg).to(torch.float32), rotary_ref.GptNeoX,
    {"embed_out.weight": "lm_head.weight"})  # the HF checkpoints' embed_out, renamed by this transformers version

hp, w = falcon.make_falcon(falcon.FALCON_TINY, WTYPE, seed=SEED, quantize=O.quantize)
E, H = hp["n_embd"], hp["n_head"]
assert hp["n_head_kv"] == 1
cfg = FalconConfig(vocab_size=hp["n_vocab"], hidden_size=E, num_hidden_layers=hp["n_layer"], num_attention_heads=H,
                   multi_query=True, new_decoder_architecture=False, parallel_attn=True, bias=False, alibi=False,
                   activation="gelu_new", layer_norm_epsilon=1e-5, max_position_embeddings=hp["n_ctx"],
                   tie_word_embeddings=False, rope_parameters={"rope_type": "default", "rope_theta": 10000.0},
                   attn_implementation="eager")
run("falcon", hp, w, falcon.tensor_shapes(hp), FalconForCausalLM(cfg).to(torch.float32), rotary_ref.Falcon)
