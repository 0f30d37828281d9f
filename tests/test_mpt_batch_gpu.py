"""The batched MPT step (backend option plan_mpt_batch; csrc/plan_mpt_batch.inc, csrc/kernels/mpt_batch.h): one decode step of several MPT
sessions through ggml_hip_decode_batch / ggml_hip_decode_batch_greedy (llm_amd.mpt.evaluate_batch / infer_tokens_batch) against the
restatement (alibi_ref.Mpt) under the bound every MPT test here uses (EDGE), its counters, the greedy chain against stepped twins bit for
bit, and the forms it declines; and its device code alone through the hook ggml_hip_debug_mpt_batch: the batched ALiBi attention against
the f64 reference with ggml's rounding points under twice the executor's own error, the per-column Q|K|V pass against exact integer
products with every other cache byte untouched."""
import ctypes as C

import numpy as np
import pytest

import alibi_ref
from llm_amd import llama, mpt
from test_mpt_chunk_gpu import SHAPES, _exact_weight
from test_mpt_plan_gpu import EDGE, GUARD, _attn_ref, _bits, _f16, _kv, _VariantMpt
from test_mpt_prompt_gpu import _attn_executor_n, _toks

pytestmark = pytest.mark.gpu

STATS = ("mpt_batch_steps", "batch_decode_steps", "batch_decode_tokens", "plan_tokens", "generic_graphs")


def _stats(G):
    return [G.get_stat(k) for k in STATS]


def _ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


# (D, H, pos, W, kind)
ATTN_CASES = [(32, 4, [0, 0], 2, "random"),                             # one key each: Q = 1, every workgroup holds exactly one column
              (64, 4, [63, 64, 0], 2, "random"),                        # the 64-key tile boundary, B odd
              (32, 4, [200, 3, 130, 64, 0, 511, 65, 1], 4, "random"),   # shares with whole short columns and parts of others
              (128, 12, [1024, 5], 8, "random"),                        # the second slope sequence; a long column split eight ways
              (32, 4, [200, 40], 4, "peaked_flat")]                     # key 5 carries column 0's maximum: in another workgroup's share


def test_batched_attention_within_twice_the_executors_error(G):
    """Measured on an MI355X, worst |Δ|max / std over the cases: the executor's chain 4.127e-7 (D 128, pos [1024, 5]), k_attn_batch_*_alibi
    5.260e-7 (peaked_flat); an earlier MFMA form of the scores: 5.598e-6, one flipped f16(x - mx).  DESIGN.md section 4.3f."""
    err = {}
    for D, H, pos, W, kind in ATTN_CASES:
        rng = np.random.default_rng(1000 * D + 10 * H + sum(pos))
        E_, B, Cc, posa = H * D, len(pos), max(pos) + 4, np.asarray(pos, np.int32)
        slopes = alibi_ref.slopes(H, 8.0)
        scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
        q = rng.standard_normal((B, E_)).astype(np.float32)
        mk = [_f16(0.5 * rng.standard_normal((Cc, E_))) for _ in pos]
        mv = [_f16(rng.standard_normal((Cc, E_))) for _ in pos]
        if kind == "peaked_flat":
            q[1] = 0  # the bias alone
            qq = _f16(q[0]).astype(np.float64).reshape(H, D)
            for k in mk:
                k[:] = 0
                k[5] = _f16((30.0 / scale) * qq / (qq * qq).sum(axis=1, keepdims=True)).reshape(E_)
        for c, p in enumerate(pos):
            mk[c][p + 1:], mv[c][p + 1:] = np.float16(np.nan), np.float16(np.nan)  # rows behind the column's token: never read
        want = np.stack([_attn_ref(q[c], mk[c], mv[c], slopes, H, D, pos[c] + 1, scale) for c in range(B)])
        out = np.zeros(B * E_ * 4 + GUARD, np.uint8)
        rc = G.lib().ggml_hip_debug_mpt_batch(0, W, None, q.ctypes.data, slopes.ctypes.data, B, posa.ctypes.data, Cc,
                                              _ptrs([k.view(np.uint16) for k in mk]), _ptrs([v.view(np.uint16) for v in mv]), 0, H, D, scale, _ptrs([out]))
        assert rc == 0 and (out[-GUARD:] == 0xFF).all(), (D, H, pos)
        new = out[:-GUARD].view(np.float32).reshape(B, E_)
        assert np.isfinite(new).all(), (D, H, pos)
        exe = np.zeros((B, E_))
        for c, p in enumerate(pos):
            mk[c][p + 1:], mv[c][p + 1:] = 0, 0
            exe[c] = _attn_executor_n(G, q[c:c + 1], mk[c], mv[c], 8.0, H, D, p, 1, Cc, scale)[0]
        sd = float(want.std()) or 1.0
        err[(D, H, tuple(pos), W, kind)] = (float(np.max(np.abs(exe - want))) / sd, float(np.max(np.abs(new - want))) / sd)
    worst_exec, worst_new = (max(v[i] for v in err.values()) for i in (0, 1))
    print("executor worst %.3e, k_attn_batch_*_alibi worst %.3e" % (worst_exec, worst_new), err)
    assert worst_new <= 2.0 * worst_exec, err


@pytest.mark.parametrize("t", [2, 8])
def test_qkv_pass_writes_only_row_pos_of_each_columns_cache(G, t):
    """E = 1024, three caches at pos 0, 7 and C - 1: Q under the mat-vec bound, K and V the f16 of the exact product in row pos[c] of cache c"""
    Ed, Cc, pos = 1024, 24, [0, 7, 23]
    posa = np.asarray(pos, np.int32)
    with G.Context(3 * Ed * Ed * 2 + (1 << 20)) as ctx:
        w, X, ref, scale = _exact_weight(G, ctx, t, 3 * Ed, Ed, 3)
        mk, mv = ([np.full(Cc * Ed * 2 + GUARD, f + c, np.uint8) for c in range(3)] for f in (0x50, 0xA0))
        for a in mk + mv:
            a[-GUARD:] = 0xFF
        out = np.zeros(3 * Ed * 4 + GUARD, np.uint8)
        rc = G.lib().ggml_hip_debug_mpt_batch(1, 0, w.ptr, X.ctypes.data, None, 3, posa.ctypes.data, Cc, _ptrs(mk), _ptrs(mv), Ed, 0, 0,
                                              0.0, _ptrs([out]))
        assert rc == 0 and all((a[-GUARD:] == 0xFF).all() for a in mk + mv + [out])
        q = out[:-GUARD].view(np.float32).reshape(3, Ed)
        assert np.all(np.abs(q.astype(np.float64) - ref[:, :Ed]) <= 2e-5 * scale[:, :Ed] + 1e-7)
        for caches, fill, lo in ((mk, 0x50, Ed), (mv, 0xA0, 2 * Ed)):
            for c, p in enumerate(pos):
                rows = caches[c][:-GUARD].reshape(Cc, Ed * 2)
                assert (np.delete(rows, p, axis=0) == fill + c).all(), (c, p)
                assert np.array_equal(rows[p].view(np.float16), ref[c, lo:lo + Ed].astype(np.float32).astype(np.float16)), (c, p)


def _sessions(model, B, hp, lens=(1, 5, 17, 2, 9, 30, 3, 12)):
    """the model's own session and B - 1 more, prompts of different lengths fed on the executor"""
    sess = [model] + [model.new_session() for _ in range(B - 1)]
    for s, n in zip(sess, lens):
        s.evaluate(_toks(n, n, hp))
    return sess


@pytest.mark.parametrize("shape,wtype,B", [("e1024", 2, 2), ("e1024", 2, 3), ("e1024", 2, 8), ("e1024", 8, 3), ("e1024", 7, 8), ("real", 2, 3)])
def test_one_step_of_several_sessions_matches_restatement(G, O, shape, wtype, B):
    """option 1 then 0: every column within EDGE of the restatement at that session's device K/V state, only row pos[c] of session c's caches
    changed, mpt_batch_steps + 1 and batch_decode_tokens + B and no executor graph; at option 0 B executor graphs and the counters still"""
    hp, w = mpt.make_mpt(SHAPES[shape], wtype, seed=7)
    model, ref = mpt.Mpt(hp, w), alibi_ref.Mpt(hp, w)
    sess, d = _sessions(model, B, hp), {}
    try:
        for on in (1, 0):
            G.set_option("plan_mpt_batch", on)
            kv0, P, s0, toks = [_kv(s) for s in sess], [s.n_past for s in sess], _stats(G), _toks(90 + on, B, hp)
            got = mpt.evaluate_batch(sess, toks)
            assert _stats(G) == ([s0[0] + 1, s0[1] + 1, s0[2] + B, s0[3] + B, s0[4]] if on else s0[:4] + [s0[4] + B])
            d[on] = []
            for c, s in enumerate(sess):
                assert s.n_past == P[c] + 1
                for old, new, mem in zip(kv0[c], _kv(s), (ref.memory_k, ref.memory_v)):
                    rows0, rows1 = (a.reshape(hp["n_layer"], s.C, -1) for a in (old, new))
                    assert np.array_equal(np.delete(rows0, P[c], axis=1), np.delete(rows1, P[c], axis=1)), (on, c)
                    mem[:] = new.view(np.float16).reshape(mem.shape)
                ref.n_past = P[c]
                want = ref.evaluate(toks[c:c + 1], mode=O.ref_mode())[0]
                d[on].append(float(np.max(np.abs(got[c] - want)) / want.std()))
    finally:
        G.set_option("plan_mpt_batch", 0)
        for s in sess[::-1]:
            s.free()
    print(f"{shape} type {wtype} B {B}: batched worst {max(d[1]):.2e}, executor worst {max(d[0]):.2e}")
    assert max(d[1]) <= EDGE and max(d[0]) <= EDGE, d


def test_greedy_chain_equals_stepped_twins_bit_for_bit(G):
    """infer_tokens_batch(3 sessions, 6) against six evaluate_batch steps with a host argmax on twins: ids, last logits, all K/V bytes"""
    hp, w = mpt.make_mpt(SHAPES["e1024"], 2, seed=7)
    model = mpt.Mpt(hp, w)
    sess = _sessions(model, 6, hp, lens=(1, 5, 17, 1, 5, 17))
    try:
        G.set_option("plan_mpt_batch", 1)
        s0 = _stats(G)
        ids, last = mpt.infer_tokens_batch(sess[:3], 6)
        assert _stats(G) == [s0[0] + 6, s0[1] + 6, s0[2] + 18, s0[3] + 18, s0[4]]
        want = np.zeros((6, 3), np.int32)
        for i in range(6):
            want[i] = [int(np.argmax(s.last_logits)) for s in sess[3:]]
            logits = mpt.evaluate_batch(sess[3:], want[i])
        assert G.get_stat("mpt_batch_steps") == s0[0] + 12
        assert np.array_equal(ids, want) and np.array_equal(_bits(last), _bits(logits))
        for a, b in zip(sess[:3], sess[3:]):
            assert a.n_past == b.n_past and all(np.array_equal(x, y) for x, y in zip(_kv(a), _kv(b)))
    finally:
        G.set_option("plan_mpt_batch", 0)
        for s in sess[::-1]:
            s.free()


@pytest.mark.parametrize("case", ["twice", "two_models", "q4_k", "kv_f32", "d16", "ctx", "sampled"])
def test_declined_forms_answer_minus_one_with_nothing_executed(G, case):
    hp0, wtype = {"q4_k": (SHAPES["e1024"], 12), "d16": (dict(SHAPES["e1024"], n_head=64), 2)}.get(case, (SHAPES["e1024"], 2))
    hp, w = mpt.make_mpt(hp0, wtype, seed=5)
    if case == "kv_f32":
        sess = [_VariantMpt(hp, w, kv_type=G.TYPE_F32) for _ in range(2)]
        for s in sess:  # (its own graph: 4-byte cache elements)
            s._build = lambda ctx0, toks, s=s: _VariantMpt.build(s, ctx0, toks, None, 4)
    else:
        sess = [mpt.Mpt(hp, w)]
        sess.append(sess[0] if case == "twice" else mpt.Mpt(*mpt.make_mpt(hp0, wtype, seed=6)) if case == "two_models" else sess[0].new_session())
    L, ids = G.lib(), np.zeros(64, np.int32)
    entry = lambda arr: L.ggml_hip_decode_batch(arr, 2)
    if case == "ctx":  # two positions left, four steps asked for
        sess[1].n_past = hp["n_ctx"] - 2
        entry = lambda arr: L.ggml_hip_decode_batch_greedy(arr, 2, 4, ids.ctypes.data)
    if case == "sampled":
        prm, win, wn, rng = llama.SamplerParams(40, 0.95, 0.8, 1.3), (C.c_int32 * 512)(), (C.c_int32 * 8)(), (C.c_uint64 * 8)(1, 2)
        entry = lambda arr: L.ggml_hip_decode_batch_sampled(arr, 2, 2, C.addressof(prm), win, wn, rng, ids.ctypes.data)
    try:
        G.set_option("plan_mpt_batch", 1)
        kv0, s0 = [_kv(s) for s in sess], _stats(G)
        ctxs, _, arr = mpt._batch_graphs(sess, [3, 4])
        try:
            assert entry(arr) == -1
        finally:
            for c in ctxs:
                c.free()
        assert _stats(G) == s0 and all(np.array_equal(x, y) for a, s in zip(kv0, sess) for x, y in zip(a, _kv(s)))
        if case == "ctx":
            sess[1].n_past = 0
        got = mpt.evaluate_batch(sess, [3, 4])  # the fallback: one by one (the declined forms) or, ctx and sampled, the step itself
        assert got.shape == (2, hp["n_vocab"]) and np.isfinite(got).all()
        assert G.get_stat("mpt_batch_steps") == s0[0] + (1 if case in ("ctx", "sampled") else 0)
    finally:
        G.set_option("plan_mpt_batch", 0)
        for s in {id(s): s for s in sess}.values():
            s.free()
