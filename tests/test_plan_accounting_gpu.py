"""The launch / byte accounting of the single-token plans (plan_decode.inc LaunchCtx: `mask`, `kind_mask`, PlanStats), which
ggml_hip_bench_plan_class reports per kernel class and per mat-vec kind and the roofline leg of bench.py divides its times by.

Every expected count below is the plans' own documentation (the comments of plan_launch_all and of the K plan in
plan_decode.inc) for L layers: 4L + 1 mat-vec launches (wq|wk|wv, wo, w1|w3, w2 per layer + lm_head), L attention launches,
and get_rows + the RoPE table besides (big = 0: + two norms and a re-quantization per layer and the final norm); the K plan's
helper-launch form has 10 launches per layer.  The bytes are the algorithmic bytes of a mat-vec — every weight block once, the
activation row, the output (and the residual) — restated here from the shapes and the block sizes of the formats."""
import numpy as np
import pytest

from test_kquant_plan_gpu import TINY_K, _model

pytestmark = pytest.mark.gpu

BLOCK_BYTES = {2: 18, 7: 24}  # q4_0, q5_1: bytes per block of 32
Q4_K, Q4_K_BYTES = 12, 144    # bytes per super-block of 256
DEFAULTS = dict(fuse_attn=1, big=1, kbig=1)


def _classes(G):
    """{class: (launches, bytes)} of the last decode plan, and the five mat-vec kinds alone / all but each."""
    cls = {name: G.bench_plan_class(k, 1)[1:] for name, k in
           (("mmvq", G.KCLASS_MMVQ), ("attn", G.KCLASS_ATTN), ("other", G.KCLASS_OTHER))}
    kinds = [G.bench_plan_class(G.KKIND_BASE + k, 1)[1:] for k in range(5)]
    but = [G.bench_plan_class(G.KKIND_BASE + 8 + k, 1)[1:] for k in range(5)]
    return cls, kinds, but


def _one_token(G, model, opts):
    """Two single-token evaluations under `opts` (only single-token plans exist afterwards), then the accounting."""
    try:
        for k, v in opts.items():
            G.set_option(k, v)
        sess = model.start_session(n_batch=8)
        wo0 = G.get_stat("fused_wo_tokens")
        for t in (3, 5):
            sess.evaluate(np.array([t], np.int32))
        wo_form = G.get_stat("fused_wo_tokens") > wo0
        out = _classes(G)
        sess.free()
    finally:
        for k, v in DEFAULTS.items():
            G.set_option(k, v)
    return out + (wo_form,)


def _check_kinds(cls, kinds, but):
    n, b = cls["mmvq"]
    assert sum(k[0] for k in kinds) == n
    assert sum(k[1] for k in kinds) == pytest.approx(b, rel=1e-12)
    for k in range(5):
        assert kinds[k][0] + but[k][0] == n
        assert kinds[k][1] + but[k][1] == pytest.approx(b, rel=1e-12)


@pytest.mark.parametrize("wtype", [2, 7])
def test_block_format_plan_counts_and_bytes(G, wtype):
    from llm_amd import llama, synth
    hp, w = synth.make_llama(synth.TINY, wtype, seed=11)
    L, E, F, V = hp["n_layer"], hp["n_embd"], hp["n_ff"], hp["n_vocab"]
    model = llama.Llama(hp, w, context_size=64)
    try:
        # two-launch pair: the documented counts, and the bytes of every kind
        cls, kinds, but, _ = _one_token(G, model, dict(fuse_attn=0, big=1))
        _check_kinds(cls, kinds, but)
        assert (cls["mmvq"][0], cls["attn"][0], cls["other"][0]) == (4 * L + 1, L, 2)
        assert [k[0] for k in kinds] == [L, L, L, L, 1]
        bb, nbE, nbF, Egqa = BLOCK_BYTES[wtype], E // 32, F // 32, E
        want = [L * ((E + 2 * Egqa) * nbE * bb + nbE * 40 + (E + 2 * Egqa) * 4),  # wq|wk|wv: blocks + the Q8 row + three f32 rows
                L * (E * nbE * bb + nbE * 40 + E * 8),                            # wo: + residual in, row out
                L * (2 * F * nbE * bb + nbE * 40 + F * 4),                        # w1|w3: one gated row out
                L * (E * nbF * bb + nbF * 40 + E * 8),                            # w2
                V * nbE * bb + nbE * 40 + V * 4]                                  # lm_head
        for k in range(5):
            print(f"type {wtype} kind {k}: {kinds[k][1]:.0f} bytes, expected {want[k]}")
            assert kinds[k][1] == want[k]
        # big = 0: the same mat-vecs behind separate norm / quantization launches
        cls0, kinds0, but0, _ = _one_token(G, model, dict(fuse_attn=0, big=0))
        _check_kinds(cls0, kinds0, but0)
        assert (cls0["mmvq"][0], cls0["attn"][0], cls0["other"][0]) == (4 * L + 1, L, 3 * L + 2)
        assert [k[1] for k in kinds0] == want
        # the fused launch allowed: wq|wk|wv carries the attention, and in the WO form wo as well
        clsf, kindsf, butf, wo_form = _one_token(G, model, dict(fuse_attn=2, big=1))
        _check_kinds(clsf, kindsf, butf)
        assert kindsf[0][0] == L and kindsf[1][0] == (0 if wo_form else L)
        assert [k[0] for k in kindsf[2:]] == [L, L, 1]
        assert clsf["attn"][0] == 0
    finally:
        model.free()


def test_k_plan_counts_and_bytes(G, O):
    from llm_amd import llama
    hp, w = _model(O, TINY_K, Q4_K, 11)
    L, E, F, V = hp["n_layer"], hp["n_embd"], hp["n_ff"], hp["n_vocab"]
    model = llama.Llama(hp, w, context_size=64)
    try:
        cls, kinds, but, _ = _one_token(G, model, dict(fuse_attn=0, kbig=0))
        _check_kinds(cls, kinds, but)
        assert (cls["mmvq"][0], cls["attn"][0]) == (4 * L + 1, L)
        assert [k[0] for k in kinds] == [L, L, L, L, 1]
        # "10 launches per layer" for a uniform model; besides them the embedding rows, the RoPE table and the final norm
        assert cls["mmvq"][0] - 1 + cls["attn"][0] + cls["other"][0] - 3 == 10 * L
        nsE, nsF, kb = E // 256, F // 256, Q4_K_BYTES
        want = [L * (nsE * 292 + 3 * (E * nsE * kb + E * 4)),  # wq|wk|wv as one run: the Q8_K row once, three f32 rows out
                L * (nsE * 292 + E * nsE * kb + E * 8),
                L * (nsE * 292 + 2 * (F * nsE * kb + F * 4)),
                L * (nsF * 292 + E * nsF * kb + E * 8),
                nsE * 292 + V * nsE * kb + V * 4]
        for k in range(5):
            print(f"q4_K kind {k}: {kinds[k][1]:.0f} bytes, expected {want[k]}")
            assert kinds[k][1] == want[k]
    finally:
        model.free()
