"""GPU tests of LoRA patching: ggml_add with a quantized / f16 src0 (k_add_q, k_add_f16: kernels/lora.h) bit for bit
against the host restatement (tests/lora_ref.py), lora.rs's patch graph with the operand of the add pinned to what the
device mirrored, dyadic adapters end to end, whole LLaMA models loaded with adapters (llm_llama_load_lora) against files
pre-merged on the host, and the generic families through lora.patch_weights."""
import ctypes as C

import numpy as np
import pytest

import lora_ref
from llm_amd import bloom, gptneox, llama, lora, synth
from llm_amd import ggml as G

pytestmark = pytest.mark.gpu

TYPES = [G.TYPE_Q4_0, G.TYPE_Q4_1, G.TYPE_Q5_0, G.TYPE_Q5_1, G.TYPE_Q8_0, G.TYPE_F16]
SHAPES = [(32, 1), (64, 3), (1024, 1024), (4096, 4096), (4096, 11008), (11008, 4096)]  # (ne0, ne1)


def _operands(t, ne0, ne1, seed):
    """W (raw bytes of type t) and x f32 [ne1, ne0].  The first rows carry the edge cases: all-zero blocks (d = -0 for
    the symmetric types), blocks whose two extremes have equal magnitude and opposite signs (the quantizer keeps the
    first), and blocks whose largest value is negative so the opposite extreme saturates at the top code."""
    rng = np.random.default_rng(seed)
    w32 = (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32)
    x = (0.01 * rng.standard_normal((ne1, ne0))).astype(np.float32)
    w32[0, :32] = 0.0
    x[0, :32] = 0.0  # an all-zero block
    if ne0 >= 64:
        w32[0, 32:64] = 0.0
        x[0, 32:64] = np.tile(np.float32([0.5, -0.5, 0.25, -0.25]), 8)  # first-wins extremes
    if ne1 >= 2:
        w32[1, :32] = 0.0
        x[1, :32] = np.linspace(1.0, -1.0, 32, dtype=np.float32)[::-1]  # -1 first: +1 saturates (Q4_0 code 16 -> 15)
    if t == G.TYPE_F16:
        return w32.astype(np.float16).view(np.uint8).reshape(-1), x
    return G.quantize(t, w32), x


def _run_add(t, w_raw, x, ne0, ne1, inplace):
    with G.Context(w_raw.nbytes + 4096) as wctx, G.Context(w_raw.nbytes + 2 * x.nbytes + (1 << 20)) as ctx:
        w = wctx.tensor_from(w_raw, t, (ne0, ne1))  # the target in a context of its own, as a model's weight is
        b = ctx.op_cont(ctx.tensor_from(x, G.TYPE_F32, (ne0, ne1)))  # a node, as ba is
        out = ctx.op_add_inplace(w, b) if inplace else ctx.op_add(w, b)
        ctx.graph().build_forward_expand(out).compute()
        return w.read_data(np.uint8) if inplace else out.read_data(np.uint8)


@pytest.mark.parametrize("ne0,ne1", SHAPES)
@pytest.mark.parametrize("t", TYPES)
def test_add_matches_restatement(t, ne0, ne1):
    w_raw, x = _operands(t, ne0, ne1, [t, ne0, ne1])
    got = _run_add(t, w_raw, x, ne0, ne1, inplace=ne0 * ne1 < 4096 * 4096 and ne1 % 2 == 1)
    want = lora_ref.add_q(t, w_raw, x)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


@pytest.mark.parametrize("ne0,ne1", [(32, 1), (1024, 1024), (4096, 11008)])
def test_add_q8_0_follows_act_quant(ne0, ne1):
    t = G.TYPE_Q8_0
    w_raw, x = _operands(t, ne0, ne1, [9, ne0, ne1])
    x = x * np.float32(7.3)  # push more values onto rounding ties of the two branches
    results = {}
    try:
        for aq in (0, 1):
            G.set_option("act_quant", aq)
            results[aq] = _run_add(t, w_raw, x, ne0, ne1, inplace=False)
    finally:
        G.set_option("act_quant", 0)
    for aq in (0, 1):
        assert np.array_equal(results[aq], lora_ref.add_q(t, w_raw, x, act_quant=aq)), aq


@pytest.mark.parametrize("inplace", [False, True])
def test_add_in_place_and_out_of_place_agree(inplace):
    t, ne0, ne1 = G.TYPE_Q5_1, 1024, 64
    w_raw, x = _operands(t, ne0, ne1, 5)
    assert np.array_equal(_run_add(t, w_raw, x, ne0, ne1, inplace), lora_ref.add_q(t, w_raw, x))


def test_add_on_an_auto_uploaded_weight_reads_its_current_bytes():
    """A weight read by a graph first (auto-uploaded) and then patched twice: each patch stages the host bytes of that
    moment, and the stale auto record is dropped, so a later graph sees the patched bytes."""
    t, ne0, ne1 = G.TYPE_Q4_0, 256, 64
    w_raw, x = _operands(t, ne0, ne1, 6)
    with G.Context(w_raw.nbytes + 4096) as wctx:
        w = wctx.tensor_from(w_raw, t, (ne0, ne1))
        v = np.random.default_rng(0).standard_normal((4, ne0)).astype(np.float32)

        def product():
            with G.Context(1 << 20) as ctx:
                y = ctx.op_mul_mat(w, ctx.tensor_from(v, G.TYPE_F32, (ne0, 4)))
                ctx.graph().build_forward_expand(y).compute()
                return y.read_data()

        p0 = product()  # auto-uploads w
        cur = w_raw
        for _ in range(2):
            with G.Context(2 * x.nbytes + (1 << 20)) as ctx:
                out = ctx.op_add(w, ctx.op_cont(ctx.tensor_from(x, G.TYPE_F32, (ne0, ne1))))
                ctx.graph().build_forward_expand(out).compute()
                got = out.read_data(np.uint8)
            cur = lora_ref.add_q(t, cur, x)
            assert np.array_equal(got, cur)
            w.write_data(got)  # lora.rs: copy the output over the target
        p2 = product()
        with G.Context(w_raw.nbytes + (1 << 20)) as ctx:
            w2 = ctx.tensor_from(cur, t, (ne0, ne1))
            y = ctx.op_mul_mat(w2, ctx.tensor_from(v, G.TYPE_F32, (ne0, 4)))
            ctx.graph().build_forward_expand(y).compute()
            want = y.read_data()
        assert np.array_equal(p2, want) and not np.array_equal(p0, p2)


@pytest.mark.parametrize("a_f16", [False, True])
@pytest.mark.parametrize("r", [1, 4, 8, 16, 64])
@pytest.mark.parametrize("s", [1.0, 2.0, 0.5, 1.0 / 3.0])
def test_patch_graph_operand_pinned(r, a_f16, s):
    t = [G.TYPE_Q4_0, G.TYPE_Q4_1, G.TYPE_Q5_0, G.TYPE_Q5_1, G.TYPE_Q8_0][r % 5]
    ne0, ne1 = 1024, 1536
    rng = np.random.default_rng([r, int(a_f16), int(s * 3)])
    w_raw = G.quantize(t, (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32))
    A = (rng.standard_normal((ne0, r)) * 0.05).astype(np.float16 if a_f16 else np.float32)
    B = (rng.standard_normal((ne1, r)) * 0.05).astype(np.float32)
    out, scaled = lora.patch_one(w_raw, t, ne0, ne1, A, B, np.float32(s))
    assert np.array_equal(out, lora_ref.add_q(t, w_raw, scaled))
    ba = scaled / np.float32(s) if s != 1.0 else scaled
    want = lora_ref.ba_exact(A, B, a_f16)
    bf = B.astype(np.float16).astype(np.float64) if a_f16 else B.astype(np.float64)
    bound = 2e-5 * (np.abs(bf) @ np.abs(A.astype(np.float64)).T)
    if s not in (1.0, 2.0, 0.5):
        bound += np.abs(want) * 2.0 ** -22  # dividing the mirrored scaled by s again is not exact
    assert np.all(np.abs(ba.astype(np.float64) - want) <= bound)


@pytest.mark.parametrize("ne0,ne1", [(64, 32000), (32000, 64)])
@pytest.mark.parametrize("a_f16", [False, True])
def test_patch_graph_wide_shapes(ne0, ne1, a_f16):
    """M or N = 32000 (vocabulary-sized targets) through every product path: grid limits."""
    t, r = G.TYPE_Q8_0, 16
    rng = np.random.default_rng([ne0, int(a_f16)])
    w_raw = G.quantize(t, (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32))
    A = lora_ref.dyadic(rng, (ne0, r), dtype=np.float16 if a_f16 else np.float32)
    B = lora_ref.dyadic(rng, (ne1, r))
    out, _ = lora.patch_one(w_raw, t, ne0, ne1, A, B, np.float32(2.0))
    assert np.array_equal(out, lora_ref.patch(t, w_raw, A, B, 2.0))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("r,a_f16,s", [(1, False, 1.0), (4, True, 2.0), (8, True, 0.5), (16, False, 1.0 / 3.0),
                                       (64, True, 1.0)])
def test_patch_dyadic_end_to_end(t, r, a_f16, s):
    ne0, ne1 = 1024, 2048
    rng = np.random.default_rng([t, r])
    w32 = (0.02 * rng.standard_normal((ne1, ne0))).astype(np.float32)
    w_raw = w32.astype(np.float16).view(np.uint8).reshape(-1) if t == G.TYPE_F16 else G.quantize(t, w32)
    A = lora_ref.dyadic(rng, (ne0, r), dtype=np.float16 if a_f16 else np.float32)
    B = lora_ref.dyadic(rng, (ne1, r))
    out, _ = lora.patch_one(w_raw, t, ne0, ne1, A, B, np.float32(s))
    assert np.array_equal(out, lora_ref.patch(t, w_raw, A, B, s))


# ---- whole LLaMA models ---------------------------------------------------------------------------------------------
HP = dict(n_vocab=512, n_embd=1024, n_head=8, n_head_kv=8, n_layer=2, n_rot=128, n_ff=2816, n_mult=256)
QTYPES = [G.TYPE_Q4_0, G.TYPE_Q4_1, G.TYPE_Q5_0, G.TYPE_Q5_1, G.TYPE_Q8_0]
SEVEN = ("attention.wq", "attention.wk", "attention.wv", "attention.wo", "feed_forward.w1", "feed_forward.w2",
         "feed_forward.w3")


def _targets(which):
    names = ("attention.wq", "attention.wv") if which == "wq_wv" else SEVEN
    return [f"layers.{i}.{n}.weight" for i in range(HP["n_layer"]) for n in names]


def _logits(m, toks):
    s = m.start_session(n_batch=8)
    try:
        out = [s.evaluate(toks)]
        for _ in range(3):
            out.append(s.evaluate(np.array([int(np.argmax(out[-1][-1]))], np.int32)))
        return out
    finally:
        s.free()


@pytest.mark.parametrize("gpu_layers", [-1, 1])
@pytest.mark.parametrize("which", ["wq_wv", "all7_two"])
@pytest.mark.parametrize("t", QTYPES)
def test_llama_load_lora_matches_premerged_file(tmp_path, t, which, gpu_layers):
    hp, w = synth.make_llama(HP, t, seed=77)
    shapes = synth.tensor_shapes(hp)
    rng = np.random.default_rng([t, len(which), gpu_layers + 1])
    ads = [lora_ref.make_adapter(rng, _targets(which), shapes, 16, 32, a_f16=(t % 2 == 0))]
    if which == "all7_two":
        ads.append(lora_ref.make_adapter(rng, _targets("wq_wv"), shapes, 4, 4))
    paths = []
    for i, ad in enumerate(ads):
        p = tmp_path / f"a{i}.ggla"
        synth.write_ggla(p, ad["r"], ad["alpha"], ad["tensors"])
        paths.append(p)
    base, merged = tmp_path / "base.bin", tmp_path / "merged.bin"
    synth.write_ggjt(base, hp, w)
    synth.write_ggjt(merged, hp, lora_ref.merge(w, shapes, ads, t))
    toks = np.random.default_rng(3).integers(0, HP["n_vocab"], 8).astype(np.int32)
    m_ref = llama.Llama.load(merged, context_size=64, gpu_layers=gpu_layers)
    try:
        want = _logits(m_ref, toks)
    finally:
        m_ref.free()
    plan0 = G.get_stat("plan_tokens")
    m = llama.Llama.load(base, context_size=64, gpu_layers=gpu_layers, lora=paths)
    try:
        got = _logits(m, toks)
    finally:
        m.free()
    for g, x in zip(got, want):
        assert np.array_equal(g.view(np.uint32), x.view(np.uint32))
    if gpu_layers < 0:
        assert G.get_stat("plan_tokens") > plan0  # the decode plan still takes the patched model


def test_llama_load_lora_without_adapters_equals_plain_load(tmp_path):
    hp, w = synth.make_llama(HP, G.TYPE_Q4_0, seed=78)
    path = tmp_path / "m.bin"
    synth.write_ggjt(path, hp, w)
    toks = np.random.default_rng(4).integers(0, HP["n_vocab"], 8).astype(np.int32)
    m = llama.Llama.load(path, context_size=64)
    try:
        want = _logits(m, toks)
    finally:
        m.free()
    L = llama._lib()
    mp = llama._MP(64, 1, -1, 0, 1.0, 10000, 0, -1, 0)
    m2 = llama.Llama.__new__(llama.Llama)
    m2.ptr = L.llm_llama_load_lora(str(path).encode(), C.byref(mp), (C.c_char_p * 1)(), 0)
    assert m2.ptr
    m2.hp, m2.weights, m2.layer_range, m2.context_size = dict(hp), None, (0, HP["n_layer"]), 64
    m2.is_first = m2.is_last = True
    try:
        got = _logits(m2, toks)
    finally:
        m2.free()
    for g, x in zip(got, want):
        assert np.array_equal(g.view(np.uint32), x.view(np.uint32))


# ---- generic families through lora.patch_weights --------------------------------------------------------------------
@pytest.mark.parametrize("family", ["bloom_offload", "bloom_reference", "gptneox"])
def test_generic_family_patch_weights(family):
    t = G.TYPE_Q5_0
    if family.startswith("bloom"):
        hp, w = bloom.make_bloom(bloom.BLOOM_TINY, t)
        shapes = bloom.tensor_shapes(hp)
        targets = ["layers.0.attention.query_key_value.weight", "layers.1.feed_forward.w2.weight", "output.weight"]
    else:
        hp, w = gptneox.make_gptneox(gptneox.GPTNEOX_TINY, t)
        shapes = gptneox.tensor_shapes(hp)
        targets = [n for n in shapes if n.endswith(".weight") and shapes[n][1] is not None and ".layers." in n][:4]
    rng = np.random.default_rng(11)
    ads = [lora_ref.make_adapter(rng, targets, shapes, 8, 16), lora_ref.make_adapter(rng, targets[:1], shapes, 4, 2, True)]
    got_w = lora.patch_weights(w, shapes, ads, t)
    want_w = lora_ref.merge(w, shapes, ads, t)
    for n in shapes:
        assert np.array_equal(np.asarray(got_w[n]).view(np.uint8), np.asarray(want_w[n]).view(np.uint8)), n
    assert any(not np.array_equal(got_w[n], w[n]) for n in targets)
    toks = np.arange(1, 9, dtype=np.int32)
    logits = []
    for ww in (got_w, want_w):
        if family.startswith("bloom"):
            m = bloom.Bloom(hp, ww, offload=family == "bloom_offload")
        else:
            m = gptneox.GptNeoX(hp, ww)
        try:
            logits.append(m.evaluate(toks))
        finally:
            m.free()
    assert np.array_equal(logits[0].view(np.uint32), logits[1].view(np.uint32))
