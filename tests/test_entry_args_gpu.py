"""The argument block of the block-format decode launches (kernels/decode_big.h BigArgs, packed by big_pack from the host's DecMmvqArgs)
on the paths the bit-identity and op-level tests of the production launches do not run: the measurement instantiations (option
`timeline`: k_mmvq_big<.., INSTR = true>, k_qkv_attn<.., true>, wo_tail's stamps), the fused launch without its WO form and without the
XCD-affine dealing, and the MPT plan's instantiations, which live in a translation unit of their own and take the same struct.  A field
read from the wrong place shows as other ids / logits, as stamps out of order, or as stamps of the wrong workgroups.

The timeline buffer holds, per launch in launch order (five per layer: wq|wk|wv, attention, wo, w1|w3, w2; then lm_head), `nw` rows of
8 x int64: a mat-vec row is entry, issued, staged, barrier, first weights, exit, steps, workgroup (rows of workgroups 0, q, 2q, ..), an
attention row ends in its head, a wo_tail row in its workgroup; whatever the form, stamps 0, 1, 2, 3, 5 of a row are taken in that
order.  The slot of wq|wk|wv stays unwritten in the WO form (it has no measurement build) and is not looked at then.

MPT: one single-token step on the plan against the same step on the node-by-node executor from the same state.  The two are not the
same arithmetic (tests/test_mpt_plan_gpu.py: LayerNorm sums in another order, another association of the attention's f32 sums), so the
bound is that module's EDGE = 8e-2 of the logits' standard deviation: one flipped int8 quant of these random-init models; an argument
read from the wrong place gives an error of the order of the logits themselves (that module's slope mutant: 0.87 .. 1.40)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H8 = dict(n_vocab=256, n_embd=256, n_head=8, n_head_kv=8, n_layer=2, n_rot=32, n_ff=352, n_mult=32)  # 8 heads: the XCD-affine dealing's shape
NW = 4  # sampled workgroups per launch of option timeline = 1
EDGE = 8e-2


def _stat(G, key):
    return int(G.lib().ggml_hip_get_stat(key.encode()))


def _decode(G, model, toks, timeline):
    """6 greedy tokens behind the prompt -> ([(id, logits)], timeline rows [launch][NW][8] of the last token or None, counters)"""
    G.set_option("timeline", timeline)
    try:
        sess = model.start_session(n_batch=8)
        c0 = [_stat(G, k) for k in ("fused_attn_tokens", "fused_wo_tokens", "fused_affine_tokens")]
        sess.feed_prompt(toks)
        out = [(sess.infer_next_token(), sess.last_logits().copy()) for _ in range(6)]
        G.lib().ggml_hip_synchronize()
        rows = G.read_timeline(1024 * NW).reshape(-1, NW, 8).copy() if timeline else None
        ran = [_stat(G, k) - c for k, c in zip(("fused_attn_tokens", "fused_wo_tokens", "fused_affine_tokens"), c0)]
        assert _stat(G, "fused_attn_timeouts") == 0
        sess.free()
    finally:
        G.set_option("timeline", 0)
    return out, rows, ran


def _check_rows(rows, L, wo_form):
    """every recorded row: entry <= issued <= staged <= barrier <= exit, written by the workgroups (heads) the slot samples"""
    assert rows.shape[0] >= 5 * L + 1
    kinds = ["qkv", "attn", "wo", "gate", "down"]
    checked = 0
    for i in range(5 * L + 1):
        kind = kinds[i % 5] if i < 5 * L else "lm_head"
        if kind == "qkv" and wo_form:
            continue  # k_qkv_attn_wo has no measurement build: the slot is taken and left alone
        r = rows[i]
        t = r[:, [0, 1, 2, 3, 5]]
        assert (t[:, 0] > 0).all(), (i, kind, r)
        assert (np.diff(t, axis=1) >= 0).all(), (i, kind, r)
        who = r[:, 7]
        if kind == "attn":
            assert who.tolist() == list(range(NW)), (i, kind, who)  # 4 heads or every n_head / 4 th: h / (n_head / 4) = 0, 1, 2, 3 ...
        else:
            q = int(who[1])
            assert q >= 1 and who.tolist() == [j * q for j in range(NW)], (i, kind, who)
        checked += 1
    return checked


@pytest.mark.parametrize("wtype", [2, 7], ids=["q4_0", "q5_1"])
@pytest.mark.parametrize("form", ["default", "no_fuse_wo", "no_affine", "neither"])
def test_measurement_builds_decode_the_same_tokens_and_stamp_in_order(G, wtype, form):
    from llm_amd import llama, synth
    shape = synth.TINY if form == "default" else H8
    hp, w = synth.make_llama(shape, wtype, seed=31)
    model = llama.Llama(hp, w, context_size=96)
    toks = np.random.default_rng(8).integers(0, hp["n_vocab"], 13).astype(np.int32)
    try:
        G.set_option("fuse_wo", 0 if form in ("no_fuse_wo", "neither") else 1)
        G.set_option("affine", 0 if form in ("no_affine", "neither") else 1)
        ref, _, ran0 = _decode(G, model, toks, 0)
        got, rows, ran1 = _decode(G, model, toks, 1)
    finally:
        G.set_option("fuse_wo", 1)
        G.set_option("affine", 1)
        model.free()
    print(form, wtype, "tokens on the fused launch / its WO form / the affine dealing: production", ran0, "measurement", ran1)
    # every form runs the fused launch, with and without the option; the WO form and the affine dealing exactly where asked for (TINY
    # has 4 heads: never affine).  "no_fuse_wo" is k_qkv_attn<.., INSTR> with the affine dealing, "neither" the same kernel without it
    # (the WO form has no measurement build: "default" and "no_affine" cover wo_tail's stamps and the plain launches')
    wo = 0 if form in ("no_fuse_wo", "neither") else 6
    aff = 6 if form == "no_fuse_wo" else 0
    assert ran0 == [6, wo, aff] and ran1 == [6, wo, aff], (ran0, ran1)
    for (ta, la), (tb, lb) in zip(ref, got):
        assert ta == tb and np.array_equal(la, lb)
    # the last token's records.  The attention slot has NW rows: the 4-head model fills them with heads 0 .. 3, of 8 heads every second
    # one records (row = head / 2) — brought to 0 .. 3 here, which is what _check_rows expects
    if shape is H8:
        rows = rows.copy()
        att = rows[1:5 * hp["n_layer"]:5, :, 7]
        assert (att == np.array([0, 2, 4, 6])).all(), att
        rows[1:5 * hp["n_layer"]:5, :, 7] = att // 2
    n = _check_rows(rows, hp["n_layer"], wo_form=wo > 0)
    assert n == (4 if wo else 5) * hp["n_layer"] + 1  # every slot but the WO form's unwritten one


def test_one_mpt_plan_token_equals_its_executor_form(G):
    from llm_amd import mpt
    hp, w = mpt.make_mpt(mpt.MPT_TINY, 2, seed=5)
    res = []
    try:
        for on in (0, 1):
            G.set_option("plan_mpt", on)
            model = mpt.Mpt(hp, w)
            model.evaluate(np.array([3, 1, 4, 1, 5], np.int32))
            m0 = G.get_stat("mpt_plan_tokens")
            res.append(np.array(model.evaluate(np.array([9], np.int32)), np.float32).copy())
            assert G.get_stat("mpt_plan_tokens") - m0 == on
            model.free()
    finally:
        G.set_option("plan_mpt", 0)
    d = float(np.max(np.abs(res[1] - res[0]))) / float(res[0].std())
    print(f"MPT plan token against the executor: |d|max / std = {d:.3e}")
    assert np.isfinite(res[1]).all() and d <= EDGE, d
