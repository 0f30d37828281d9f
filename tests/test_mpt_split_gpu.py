"""The MPT plan's position-split decode attention (kernels/mpt_plan.h k_attn_split_scores_alibi / _vp_alibi / _merge_alibi; backend option
attn_split under plan_mpt; counter mpt_split_tokens) and the context cap it lifts.  The f64 reference, the executor's chain and the
whole-model bounds are tests/test_mpt_plan_gpu.py's, imported as they stand.  Every option set here is restored in a finally."""
import ctypes as C

import numpy as np
import pytest

import alibi_ref
import test_mpt_plan_gpu as base
from llm_amd import mpt

pytestmark = pytest.mark.gpu

PROMPT = np.array([3, 1, 4, 1, 5], np.int32)
# (D, H, S, T, kind), C = T + 3
CASES = [(32, 4, 2, 1, "random"),       # one key, the second range empty
         (32, 4, 16, 65, "random"),     # ranges of 64: one full, one of a single key, 14 empty
         (128, 12, 3, 129, "random"),   # ranges of 64, 64 and 1; heads 8 .. 11 on the second slope sequence
         (64, 3, 5, 700, "random"),     # D = 64, odd H and S, the last range empty
         (128, 12, 8, 1025, "random"),
         (32, 4, 4, 130, "peaked"),     # K row 64 along q: the row maximum comes from another workgroup's pmax
         (32, 4, 4, 130, "flat"),       # K = 0: the bias alone
         (32, 2, 16, 25605, "random")]  # C = 25608: the first length k_attn_decode_alibi has no LDS for (op 1 returns -1)


def _hook(G, op, flag, q, mk, mv, slopes, H, D, T, Cc, scale):
    E = H * D
    out = np.zeros(E + base.GUARD // 4, np.float32)
    rc = G.lib().ggml_hip_debug_mpt(op, flag, q.ctypes.data, slopes.ctypes.data, 0.0, 0, mk.view(np.uint16).ctypes.data, mv.view(np.uint16).ctypes.data,
                                    H, D, T - 1, Cc, scale, (C.c_void_p * 1)(out.ctypes.data))
    return rc, out


def test_split_attention_within_twice_the_executors_error(G):
    """Measured on an MI355X (worst |Δ|max / std of the reference row over the 8 cases): the executor's chain 6.91e-7 (D 64, H 3, T 700), the
    split attention 6.86e-7 (D 128, H 12, T 1025, S 8); T = 1 is exact on both.  DESIGN.md section 4.3c."""
    err_exec, err_new = [], []
    for D, H, S, T, kind in CASES:
        rng = np.random.default_rng(1000 * D + 10 * H + T)
        E, Cc = H * D, T + 3
        slopes = alibi_ref.slopes(H, 8.0)
        scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
        q = rng.standard_normal(E).astype(np.float32)
        mk = base._f16(0.5 * rng.standard_normal((Cc, E)))
        mv = base._f16(rng.standard_normal((Cc, E)))
        if kind != "random":
            mk[:] = 0
        if kind == "peaked":  # one score 30 above the rest, in the second range
            qq = base._f16(q).astype(np.float64).reshape(H, D)
            mk[64] = base._f16((30.0 / scale) * qq / (qq * qq).sum(axis=1, keepdims=True)).reshape(E)
        mk[T:], mv[T:] = np.float16(np.nan), np.float16(np.nan)  # rows at or behind T: never read
        want = base._attn_ref(q, mk, mv, slopes, H, D, T, scale)
        rc, out = _hook(G, 4, S, q, mk, mv, slopes, H, D, T, Cc, scale)
        assert rc == 0, (D, H, S, T)
        assert (out[E:].view(np.uint32) == 0xFFFFFFFF).all(), "guard"
        assert np.isfinite(out[:E]).all(), (D, H, S, T, kind)
        assert np.array_equal(_hook(G, 4, S, q, mk, mv, slopes, H, D, T, Cc, scale)[1].view(np.uint32), out.view(np.uint32))  # reproducible
        if T == 25605:
            assert _hook(G, 1, 0, q, mk, mv, slopes, H, D, T, Cc, scale)[0] == -1
        mk[T:], mv[T:] = 0, 0
        exe = base._attn_executor(G, q, mk, mv, 8.0, H, D, T, Cc, scale)
        sd = float(want.std()) or 1.0
        err_exec.append(float(np.max(np.abs(exe - want))) / sd)
        err_new.append(float(np.max(np.abs(out[:E].astype(np.float64) - want))) / sd)
    print("executor worst %.3e, split attention worst %.3e" % (max(err_exec), max(err_new)), list(zip(CASES, err_exec, err_new)))
    assert max(err_new) <= 2.0 * max(err_exec), (max(err_new), max(err_exec))


def test_context_beyond_the_old_cap_lands_on_the_plan(G):
    hp, w = mpt.make_mpt(mpt.MPT_TINY, 2, seed=5)
    rows = {}
    try:
        G.set_option("plan_mpt", 1)
        for n_ctx in (64, 26000):
            model = base._prompted(hp, w, n_ctx=n_ctx, prompt=PROMPT)
            m0, s0 = G.get_stat("mpt_plan_tokens"), G.get_stat("mpt_split_tokens")
            rows[n_ctx] = model.evaluate(np.array([7], np.int32))
            assert G.get_stat("mpt_plan_tokens") == m0 + 1, n_ctx
            assert G.get_stat("mpt_split_tokens") == s0  # six positions: k_attn_decode_alibi
            model.free()
        assert np.array_equal(base._bits(rows[64]), base._bits(rows[26000]))
        G.set_option("attn_split", 0)  # no split path to take the longer rows: declined as before, nothing executed on the plan
        model = base._prompted(hp, w, n_ctx=26000, prompt=PROMPT)
        m0, g0 = G.get_stat("mpt_plan_tokens"), G.get_stat("generic_graphs")
        model.evaluate(np.array([7], np.int32))
        assert (G.get_stat("mpt_plan_tokens"), G.get_stat("generic_graphs")) == (m0, g0 + 1)
        model.free()
    finally:
        G.set_option("attn_split", 1)
        G.set_option("plan_mpt", 0)


def test_model_and_chain_across_the_crossing(G, O):
    """attn_split = 8: the tokens at positions 5, 6 run k_attn_decode_alibi, those at 7 .. 10 (T >= 8) the three split launches"""
    hp, w = mpt.make_mpt(mpt.MPT_TINY, 2, seed=5)
    L, Cc, E = hp["n_layer"], hp["n_ctx"], hp["n_embd"]
    n, res = 6, {}
    try:
        G.set_option("plan_mpt", 1)
        ref, d = alibi_ref.Mpt(hp, w), []
        for split, form in ((8, "chain"), (8, "stepped"), (0, "fed")):
            G.set_option("attn_split", split)
            model = base._prompted(hp, w, prompt=PROMPT)
            s0, m0 = G.get_stat("mpt_split_tokens"), G.get_stat("mpt_plan_tokens")
            if form == "chain":
                ids, lg = model.infer_tokens_device(n)
            else:  # stepped: the argmax on the host (every row against the restatement), or — unsplit — the split run's ids fed again
                ids = np.zeros(n, np.int32)
                for i in range(n):
                    ids[i] = int(np.argmax(model.last_logits)) if split else res[8, "stepped"][0][i]
                    if split:
                        d.append(base._step_vs_ref(O, model, ref, int(ids[i])))
                    else:
                        model.evaluate(ids[i:i + 1])
                lg = model.last_logits
            assert G.get_stat("mpt_plan_tokens") - m0 == n
            assert G.get_stat("mpt_split_tokens") - s0 == (4 if split else 0), (split, form)
            res[split, form] = (ids, lg.copy(), base._kv(model))
            model.free()
        (ia, la, kva), (ib, lb, kvb), (_, _, kv0) = res[8, "chain"], res[8, "stepped"], res[0, "fed"]
        assert np.array_equal(ia, ib), (ia, ib)
        assert np.array_equal(base._bits(la), base._bits(lb))
        assert np.array_equal(kva[0], kvb[0]) and np.array_equal(kva[1], kvb[1])
        print("attn_split 8, stepped:", d)  # tests/test_mpt_plan_gpu.py's bounds for this model, type and weights seed
        assert max(d) <= base.EDGE, d
        assert sum(x <= base.STRICT for x in d) >= len(d) // 2, d
        for a, b in zip(kvb, kv0):  # layer 0's K/V rows depend on no attention: the same tokens leave the same rows, split or not
            assert np.array_equal(a.reshape(L, Cc, E)[0], b.reshape(L, Cc, E)[0])
    finally:
        G.set_option("attn_split", 1)
        G.set_option("plan_mpt", 0)
