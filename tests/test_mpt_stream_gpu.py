"""k_p_attn_alibi_stream (kernels/mpt_prompt.h; option mpt_attn_stream, counter mpt_stream_tokens): the MPT prompt plan's attention for rows
behind k_p_attn_alibi's LDS fit.  Op level through ggml_hip_debug_mpt_prompt `what 3`: bit for bit k_p_attn_alibi (`what 2`) wherever both
run, and past the fit (T = 2241) every row against tests/test_mpt_plan_gpu.py's f64 reference at twice the executor's own error.  Whole
model: forced (option 2) it leaves option 1's bits; past the fit the evaluation stays on the plan and every row holds EDGE against the
restatement tests/alibi_ref.py at the device's K/V state (0.1 s of CPU at that length).  Every test restores the options."""
import ctypes as C

import numpy as np
import pytest

import alibi_ref
from llm_amd import mpt
from test_mpt_plan_gpu import EDGE, MPT_12H, _attn_ref, _f16, _kv, _VariantMpt
from test_mpt_prompt_gpu import _attn_executor_n, _hook, _rows_vs_ref

pytestmark = pytest.mark.gpu


class options:
    """plan_mpt_prompt = 1 and mpt_attn_stream = `stream` inside; the defaults behind it whatever happens"""

    def __init__(self, G, stream):
        self.G, self.stream = G, stream

    def __enter__(self):
        self.G.set_option("plan_mpt_prompt", 1)
        self.G.set_option("mpt_attn_stream", self.stream)

    def __exit__(self, *exc):
        self.G.set_option("plan_mpt_prompt", 0)
        self.G.set_option("mpt_attn_stream", 1)


def _inputs(D, H, P, N, kind):
    """tests/test_mpt_prompt_gpu.py's attention inputs: NaN in the cache rows behind the last token and in the product's K and V columns"""
    rng = np.random.default_rng(1000 * D + 10 * H + P + N)
    E, T = H * D, P + N
    scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    q = rng.standard_normal((N, E)).astype(np.float32)
    mk, mv = _f16(0.5 * rng.standard_normal((T + 3, E))), _f16(rng.standard_normal((T + 3, E)))
    if kind == "peaked_flat":  # K = 0 but row 5 along the last query (its score 30 above the rest); query 0 is zero: its row is the bias alone
        mk[:] = 0
        q[0] = 0
        qq = _f16(q[-1]).astype(np.float64).reshape(H, D)
        mk[5] = _f16((30.0 / scale) * qq / (qq * qq).sum(axis=1, keepdims=True)).reshape(E)
    mk[T:], mv[T:] = np.float16(np.nan), np.float16(np.nan)
    qkv = np.full((N, 3 * E), np.nan, np.float32)
    qkv[:, :E] = q
    return q, qkv, mk, mv, alibi_ref.slopes(H, 8.0), scale


def _attn(G, what, flag, qkv, x2, mk, mv, slopes, H, D, P, scale):
    N = qkv.shape[0]
    return _hook(G, what, flag, (N, H * D), np.uint16 if flag else np.float32, qkv, x2, w=slopes, N=N, mk=mk.view(np.uint16), mv=mv.view(np.uint16),
                 H=H, D=D, P=P, Cc=mk.shape[0], scale=scale)[0]


# one partial block, N no multiple of 32 | D 64, odd n_past, a second partial | the diagonal crosses a 128-key block | n_past no multiple of
# 16 | three blocks: both P buffers reused, a ragged last tile | k_p_attn_alibi on its 16-query form | the peaked and the all-bias row
@pytest.mark.parametrize("D,H,P,N,kind", [(32, 4, 0, 33, "random"), (64, 4, 5, 40, "x2"), (128, 2, 0, 130, "random"), (128, 2, 97, 64, "random"),
                                          (128, 2, 250, 70, "random"), (128, 2, 1100, 40, "random"), (32, 4, 7, 32, "peaked_flat")])
def test_streaming_attention_is_the_lds_kernels_bits(G, D, H, P, N, kind):
    q, qkv, mk, mv, slopes, scale = _inputs(D, H, P, N, kind)
    x2 = None
    if kind == "x2":  # the product as a split GEMM leaves it: two partials
        x2 = (0.25 * np.random.default_rng(1).standard_normal(qkv.shape)).astype(np.float32)
        qkv[:, :H * D] -= x2[:, :H * D]
    for flag in (0, 1, 2):
        lds, new = (_attn(G, what, flag, qkv, x2, mk, mv, slopes, H, D, P, scale) for what in (2, 3))
        assert np.isfinite(new.view(np.float16) if flag else new).all()
        assert np.array_equal(lds, new), (flag, int((lds != new).sum()))


def test_rows_past_the_lds_fit_within_twice_the_executors_error(G):
    """T = 2241, the first length mpt_attn_queries refuses at D = 128.  Measured on an MI355X, worst |Δ|max / std over the 32 rows: the
    executor's chain 5.965e-7, k_p_attn_alibi_stream 3.216e-7."""
    D, H, P, N = 128, 2, 2209, 32
    q, qkv, mk, mv, slopes, scale = _inputs(D, H, P, N, "random")
    want = np.stack([_attn_ref(q[i], mk, mv, slopes, H, D, P + i + 1, scale) for i in range(N)])
    new = _attn(G, 3, 0, qkv, None, mk, mv, slopes, H, D, P, scale)
    out = np.zeros(N * H * D + 64, np.float32)
    assert G.lib().ggml_hip_debug_mpt_prompt(2, 0, qkv.ctypes.data, None, None, slopes.ctypes.data, 1e-5, 0, N, mk.ctypes.data, mv.ctypes.data, H, D, P,
                                             mk.shape[0], scale, (C.c_void_p * 2)(out.ctypes.data, None)) == -1
    mk[P + N:], mv[P + N:] = 0, 0
    exe = _attn_executor_n(G, q, mk, mv, 8.0, H, D, P, N, mk.shape[0], scale)
    sd = float(want.std())
    e_exe, e_new = float(np.max(np.abs(exe - want))) / sd, float(np.max(np.abs(new - want))) / sd
    print("executor %.3e, k_p_attn_alibi_stream %.3e" % (e_exe, e_new))
    assert np.isfinite(new).all() and e_new <= 2.0 * e_exe


@pytest.mark.parametrize("wtype", [2, 8])
def test_forced_streaming_leaves_the_models_bits(G, wtype):
    hp, w = mpt.make_mpt(dict(MPT_12H, n_ctx=128), wtype, seed=17)
    toks = np.random.default_rng(18).integers(0, hp["n_vocab"], 73).astype(np.int32)
    runs = {}
    for stream in (1, 2):
        with options(G, stream):
            model = mpt.Mpt(hp, w)
            s0, m0 = G.get_stat("mpt_stream_tokens"), G.get_stat("mpt_prompt_tokens")
            logits = np.concatenate([model.evaluate(toks[:40]), model.evaluate(toks[40:])])
            assert (G.get_stat("mpt_stream_tokens"), G.get_stat("mpt_prompt_tokens")) == (s0 + 73 * (stream == 2), m0 + 73)
            runs[stream] = (logits.view(np.uint32),) + _kv(model)
            model.free()
    assert np.isfinite(runs[2][0].view(np.float32)).all()
    assert all(np.array_equal(a, b) for a, b in zip(runs[1], runs[2]))


def test_a_prompt_past_the_lds_fit_stays_on_the_plan(G, O):
    """n_past 2201 + 40 tokens = 2241 keys; the rows against the restatement itself (not the executor's)"""
    hp, w = mpt.make_mpt(dict(mpt.MPT_TINY, n_ctx=2304), 2, seed=5)
    toks = np.random.default_rng(6).integers(0, hp["n_vocab"], 2241).astype(np.int32)
    model, ref = mpt.Mpt(hp, w), alibi_ref.Mpt(hp, w)
    try:
        with options(G, 1):
            model.feed_prompt(toks[:2201])
            for stream, want in ((0, 0), (1, 1)):  # asked of the matcher alone, never run
                G.set_option("mpt_attn_stream", stream)
                ctx0 = model._ctx0(40, kq_copies=4)
                try:
                    _, gf = _VariantMpt.build(model, ctx0, toks[2201:])
                    assert G.lib().ggml_hip_debug_mpt(3, 0, C.cast(gf.ptr, C.c_void_p), None, 0.0, 0, None, None, 0, 0, 0, 0, 0.0, None) == want
                finally:
                    ctx0.free()
            before = [G.get_stat(k) for k in ("mpt_stream_tokens", "mpt_prompt_tokens", "generic_graphs")]
            d = _rows_vs_ref(O, model, ref, toks[2201:])
            assert [G.get_stat(k) for k in ("mpt_stream_tokens", "mpt_prompt_tokens", "generic_graphs")] == [before[0] + 40, before[1] + 40, before[2]]
    finally:
        model.free()
    print("worst %.2e" % max(d), d)
    assert max(d) <= EDGE, d
