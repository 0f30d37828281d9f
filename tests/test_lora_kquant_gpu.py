"""GPU tests of LoRA patching on K-quant weights: ggml_add with a Q2_K .. Q6_K src0 (k_add_k: kernels/lora.h, the device
K encoder kernels/kquant_encode.h) bit for bit against the host restatement (tests/lora_ref.py add_q: the oracle's
dequantize_row_q*_K, an f32 add, the oracle's quantize_row_q*_K), a second patch of a patched weight, dyadic adapters end to
end, a *_K_M-style LLaMA file loaded with adapters (llm_llama_load_lora) against a file pre-merged on the host, and
lora.patch_weights with a type per tensor."""
import numpy as np
import pytest

import kquant_cases
import lora_ref
from llm_amd import ggml as G
from llm_amd import llama, lora, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

K_TYPES = kquant_cases.K_TYPES


@pytest.fixture(scope="module", autouse=True)
def _k_encoders_present():
    """A library without the K encoders fails this module here, in Python: its add would end the process (die())."""
    assert hasattr(G.lib(), "ggml_quantize_q4_K"), "libggml_hip.so exports no ggml_quantize_q4_K"


def _operands(t, ne0, ne1):
    """W (raw bytes of type t, the oracle's quantizer) and x f32 [ne1, ne0], 0.01 * gaussian.  W is zero in the first
    super-blocks and x holds the edge cases of kquant_cases there, so that the sum dequant(W) + x has their properties.
    Returns (w_raw, x, number of edge super-blocks)."""
    x, n_edge = kquant_cases.tensor(ne0, ne1, seed=[t, ne0, ne1], scale=0.01)
    w32 = (0.02 * np.random.default_rng([ne0, ne1, t]).standard_normal((ne1, ne0))).astype(np.float32)
    w32.reshape(-1, 256)[:n_edge] = 0.0
    return O.quantize_row(t, w32), x, n_edge


def _run_add(t, w_raw, x, ne0, ne1, inplace):
    with G.Context(w_raw.nbytes + 4096) as wctx, G.Context(w_raw.nbytes + 2 * x.nbytes + (1 << 20)) as ctx:
        w = wctx.tensor_from(w_raw, t, (ne0, ne1))  # the target in a context of its own, as a model's weight is
        b = ctx.op_cont(ctx.tensor_from(x, G.TYPE_F32, (ne0, ne1)))  # a node, as ba is
        out = ctx.op_add_inplace(w, b) if inplace else ctx.op_add(w, b)
        ctx.graph().build_forward_expand(out).compute()
        return w.read_data(np.uint8) if inplace else out.read_data(np.uint8)


@pytest.fixture(scope="module")
def cases():
    """(t, shape) -> (w_raw, x, n_edge, restatement), computed once."""
    out = {}
    for t in K_TYPES:
        for s in kquant_cases.ENC_SHAPES:
            w_raw, x, n_edge = _operands(t, *s)
            out[(t, s)] = (w_raw, x, n_edge, lora_ref.add_q(t, w_raw, x))
    return out


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("ne0,ne1", kquant_cases.ENC_SHAPES)
@pytest.mark.parametrize("t", K_TYPES)
def test_add_matches_restatement(cases, t, ne0, ne1, inplace):
    w_raw, x, n_edge, want = cases[(t, (ne0, ne1))]
    got = _run_add(t, w_raw.copy(), x, ne0, ne1, inplace)
    bs = G.BLOCK_BYTES[t]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], bad[:8] // bs)  # byte offsets, super-blocks
    # a kernel that copies W through cannot pass: over the gaussian super-blocks most bytes change (the restatement
    # alone gives 0.67 .. 0.80 for such inputs)
    changed = np.mean(got[n_edge * bs:] != w_raw[n_edge * bs:])
    assert changed >= 0.5, changed


@pytest.mark.parametrize("t", K_TYPES)
def test_second_patch_of_a_patched_weight(cases, t):
    ne0, ne1 = 768, 3
    w_raw, x, _, once = cases[(t, (ne0, ne1))]
    first = _run_add(t, w_raw.copy(), x, ne0, ne1, inplace=False)
    second = _run_add(t, first.copy(), x, ne0, ne1, inplace=True)
    assert np.array_equal(first, once)
    assert np.array_equal(second, lora_ref.add_q(t, once, x))


@pytest.mark.parametrize("a_f16", [False, True])
@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("s", [1.0, 2.0, 0.5])
@pytest.mark.parametrize("t", K_TYPES)
def test_patch_dyadic_end_to_end(t, s, r, a_f16):
    ne0, ne1 = 1024, 768
    rng = np.random.default_rng([t, r, int(a_f16)])
    w_raw = O.quantize_row(t, (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32))
    A = lora_ref.dyadic(rng, (ne0, r), dtype=np.float16 if a_f16 else np.float32)
    B = lora_ref.dyadic(rng, (ne1, r))
    out, _ = lora.patch_one(w_raw, t, ne0, ne1, A, B, np.float32(s))
    assert np.array_equal(out, lora_ref.patch(t, w_raw, A, B, s))


# ---- whole LLaMA models ---------------------------------------------------------------------------------------------
HP = dict(n_vocab=256, n_embd=512, n_head=4, n_head_kv=4, n_layer=3, n_rot=128, n_ff=768, n_mult=32)
SEVEN = ("attention.wq", "attention.wk", "attention.wv", "attention.wo", "feed_forward.w1", "feed_forward.w2",
         "feed_forward.w3")


def _k_model(wtype, mixed, seed):
    """The model of test_mixed_k_quant_file_loads_and_decodes_on_the_k_plan: every 2-D weight made by the oracle's
    quantizer; mixed: wv, w2 and output in Q6_K.  Returns (hp, w, {name: type} of the 2-D weights)."""
    rng = np.random.default_rng([wtype, seed])
    hp, w, types = dict(HP), {}, {}
    for name, (ne0, ne1) in synth.tensor_shapes(hp).items():
        if ne1 is None:
            w[name] = (1.0 + 0.01 * rng.standard_normal(ne0)).astype(np.float32)
            continue
        k_m = name == "output.weight" or name.endswith("attention.wv.weight") or name.endswith("feed_forward.w2.weight")
        types[name] = G.TYPE_Q6_K if mixed and k_m else wtype
        w[name] = O.quantize(types[name], (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32))
    hp["wtype"] = wtype
    if mixed:
        hp["wtypes"] = {n: t for n, t in types.items() if t != wtype}
    return hp, w, types


def _targets(names):
    return [f"layers.{i}.{n}.weight" for i in range(HP["n_layer"]) for n in names]


def _adapters(rng, shapes):
    return [lora_ref.make_adapter(rng, _targets(SEVEN), shapes, 16, 32),
            lora_ref.make_adapter(rng, _targets(("attention.wq", "attention.wv")), shapes, 4, 4, a_f16=True)]


def _merge(w, shapes, ads, types):
    """lora_ref.merge with the type of each tensor."""
    out = dict(w)
    for t in sorted(set(types.values())):
        out = lora_ref.merge(out, {n: s for n, s in shapes.items() if types.get(n) == t}, ads, t)
    return out


def _logits(m, toks):
    s = m.start_session(n_batch=8)
    try:
        out = [s.evaluate(toks)]
        for _ in range(3):
            out.append(s.evaluate(np.array([int(np.argmax(out[-1][-1]))], np.int32)))
        return out
    finally:
        s.free()


@pytest.mark.parametrize("wtype,mixed,gpu_layers", [(G.TYPE_Q4_K, True, -1), (G.TYPE_Q5_K, False, 1)])
def test_llama_load_lora_matches_premerged_file(tmp_path, wtype, mixed, gpu_layers):
    hp, w, types = _k_model(wtype, mixed, seed=19)
    shapes = synth.tensor_shapes(hp)
    ads = _adapters(np.random.default_rng([wtype, 5]), shapes)
    paths = []
    for i, ad in enumerate(ads):
        p = tmp_path / f"a{i}.ggla"
        synth.write_ggla(p, ad["r"], ad["alpha"], ad["tensors"])
        paths.append(p)
    base, merged = tmp_path / "base.bin", tmp_path / "merged.bin"
    synth.write_ggjt(base, hp, w)
    w_merged = _merge(w, shapes, ads, types)
    assert not np.array_equal(w_merged["layers.0.attention.wv.weight"], w["layers.0.attention.wv.weight"])
    synth.write_ggjt(merged, hp, w_merged)
    toks = np.random.default_rng(3).integers(0, HP["n_vocab"], 8).astype(np.int32)
    runs = []
    for path, lora_paths in ((merged, ()), (base, paths)):
        k0 = G.get_stat("kplan_tokens")
        m = llama.Llama.load(path, context_size=64, gpu_layers=gpu_layers, lora=lora_paths)
        try:
            runs.append(_logits(m, toks))
        finally:
            m.free()
        if gpu_layers < 0:
            assert G.get_stat("kplan_tokens") > k0  # the patched model still takes the K plan
    for g, x in zip(runs[1], runs[0]):
        assert np.array_equal(g.view(np.uint32), x.view(np.uint32))


def test_patch_weights_with_a_type_per_tensor():
    hp, w, types = _k_model(G.TYPE_Q4_K, True, seed=23)
    shapes = synth.tensor_shapes(hp)
    ads = _adapters(np.random.default_rng(29), shapes)
    got = lora.patch_weights(w, shapes, ads, types)
    want = _merge(w, shapes, ads, types)
    for n in shapes:
        assert np.array_equal(np.asarray(got[n]).view(np.uint8), np.asarray(want[n]).view(np.uint8)), n
    assert all(not np.array_equal(got[n], w[n]) for n in _targets(SEVEN))
    # one K type for every tensor, named as a plain type
    hp5, w5, types5 = _k_model(G.TYPE_Q5_K, False, seed=23)
    got5 = lora.patch_weights(w5, shapes, ads[1:], G.TYPE_Q5_K)
    want5 = _merge(w5, shapes, ads[1:], types5)
    for n in shapes:
        assert np.array_equal(np.asarray(got5[n]).view(np.uint8), np.asarray(want5[n]).view(np.uint8)), n
