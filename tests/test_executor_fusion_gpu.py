"""The generic executor's fusion rules (backend_executor.inc execute_graph: rms_norm + mul, the deferred silu + mul,
scale -> diag_mask_inf -> soft_max) on graphs where they must NOT fire, or must fire without changing the result.  Every graph
runs with option fuse = 1 and fuse = 0 (one launch per node, in node order: ggml's semantics); the two must agree bit for bit
(the fused kernels restate the arithmetic of the separate ones), and each result is checked against numpy or the oracle."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _fuse(G, value):
    G.set_option("fuse", value)
    try:
        yield
    finally:
        G.set_option("fuse", 1)


def _run(G, fuse, build, mem=1 << 22):
    """build(ctx) -> {name: tensor}; the tensors are expanded into the graph in that order.  Returns {name: host result}."""
    with _fuse(G, fuse), G.Context(mem) as ctx:
        outs = build(ctx)
        g = ctx.graph()
        for t in outs.values():
            g.build_forward_expand(t)
        g.compute()
        return {k: t.read_data() for k, t in outs.items()}


def _both(G, build):
    fused, plain = _run(G, 1, build), _run(G, 0, build)
    for k in plain:
        assert np.array_equal(fused[k].view(np.uint32), plain[k].view(np.uint32)), f"{k}: fuse = 1 differs from fuse = 0"
    return fused


def _check_silu_mul(O, got, a, b):
    """test_silu_mul's bound: identical up to f16-boundary flips of the device expf (each one f16 ulp)"""
    ref = O.silu(a, mode=O.ref_mode()) * b
    bad = np.abs(got - ref) > 1e-6 * np.abs(ref) + 1e-9
    assert bad.mean() < 2e-3, bad.mean()
    assert np.allclose(got, ref, rtol=1.1e-3, atol=1e-6), float(np.max(np.abs(got - ref)))


def _ab(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 3).astype(np.float32), rng.standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("n", [4096, 4095])
def test_deferred_silu_not_across_a_write_of_its_operand(G, O, n):
    """a = cont(x); s = silu(a); a2 = scale_inplace(a, 2); m = mul(s, b), in the node order a, s, a2, m.  ggml's order gives
    m = silu(x) b.  Deferring s to m (the FFN gate rule) would read a after a2 doubled it: silu(2x) b — what the executor did
    before it checked that no node between the two writes bytes of the silu's operand."""
    x, b = _ab(n, 81)

    def build(ctx):
        a = ctx.op_cont(ctx.tensor_from(x))
        s = ctx.op_silu(a)
        a2 = ctx.op_scale_inplace(a, ctx.new_f32(2.0))
        return {"s": s, "a2": a2, "m": ctx.op_mul(s, ctx.tensor_from(b))}

    got = _both(G, build)
    assert np.array_equal(got["a2"], 2 * x)
    _check_silu_mul(O, got["m"], x, b)
    _check_silu_mul(O, got["s"], x, np.ones(n, np.float32))


def test_deferred_silu_across_an_unrelated_node(G, O):
    """The FFN's order, w1 x, silu, (something that writes elsewhere), mul: still right, fused or not."""
    n = 4096
    x, b = _ab(n, 82)

    def build(ctx):
        s = ctx.op_silu(ctx.op_cont(ctx.tensor_from(x)))
        c = ctx.op_scale(ctx.tensor_from(b), ctx.new_f32(2.0))
        return {"s": s, "c": c, "m": ctx.op_mul(s, c)}

    got = _run(G, 1, build)
    plain = _run(G, 0, build)
    assert np.array_equal(got["m"], plain["m"]) and np.array_equal(got["c"], 2 * b)
    _check_silu_mul(O, got["m"], x, 2 * b)


def test_silu_with_two_consumers(G, O):
    """s = silu(a) read by mul(s, b) and by add(s, b): running it fused with the mul would leave s unwritten for the add."""
    n = 4096
    x, b = _ab(n, 83)

    def build(ctx):
        s = ctx.op_silu(ctx.op_cont(ctx.tensor_from(x)))
        tb = ctx.tensor_from(b)
        return {"s": s, "m": ctx.op_mul(s, tb), "r": ctx.op_add(s, tb)}

    got = _both(G, build)
    _check_silu_mul(O, got["s"], x, np.ones(n, np.float32))
    assert np.array_equal(got["m"], got["s"] * b) and np.array_equal(got["r"], got["s"] + b)


def test_mul_with_silu_as_second_operand(G, O):
    """mul(b, silu(a)): the rule matches src[0] only; the plain multiply must run."""
    n = 4096
    x, b = _ab(n, 84)
    got = _both(G, lambda ctx: {"m": ctx.op_mul(ctx.tensor_from(b), ctx.op_silu(ctx.op_cont(ctx.tensor_from(x))))})
    _check_silu_mul(O, got["m"], x, b)


def test_silu_then_mul_by_a_row(G, O):
    """silu(a) [E, N] times a row b [E]: the fused kernel takes same-size operands only."""
    E, N = 100, 7
    x, _ = _ab(E * N, 85)
    row = np.random.default_rng(86).standard_normal(E).astype(np.float32)
    got = _both(G, lambda ctx: {"m": ctx.op_mul(ctx.op_silu(ctx.op_cont(ctx.tensor_from(x.reshape(N, E)))), ctx.tensor_from(row))})
    _check_silu_mul(O, got["m"], x, np.tile(row, N))


def _rms_inputs(E, N, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((N, E)) * 3).astype(np.float32), (1 + 0.01 * rng.standard_normal(E)).astype(np.float32),
            rng.standard_normal((N, E)).astype(np.float32))


def _close(got, ref):
    return np.allclose(got.reshape(ref.shape), ref, rtol=3e-7, atol=1e-7)  # test_rms_norm_and_weight's bound


def test_rms_norm_with_two_consumers(G, O):
    """n = rms_norm(x) read by mul(n, w) and by add(n, y): fusing the multiply would leave n unwritten for the add."""
    E, N = 257, 4
    x, w, y = _rms_inputs(E, N, 87)

    def build(ctx):
        nrm = ctx.op_rms_norm(ctx.tensor_from(x), 5e-6)
        return {"mul": ctx.op_mul(nrm, ctx.tensor_from(w)), "add": ctx.op_add(nrm, ctx.tensor_from(y))}

    got = _both(G, build)
    ref = O.rms_norm(x, 5e-6)
    assert _close(got["mul"], ref * w) and _close(got["add"], ref + y)


def test_rms_norm_then_mul_by_a_full_tensor(G, O):
    """the second operand is [E, N], not a weight row: the fused kernel would index it as a row."""
    E, N = 257, 4
    x, _, y = _rms_inputs(E, N, 88)
    got = _both(G, lambda ctx: {"mul": ctx.op_mul(ctx.op_rms_norm(ctx.tensor_from(x), 5e-6), ctx.tensor_from(y))})
    assert _close(got["mul"], O.rms_norm(x, 5e-6) * y)


SMS = dict(H=3, N=4, nc=257)


def _sms_inputs(seed):
    H, N, nc = SMS["H"], SMS["N"], SMS["nc"]
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((H, N, nc)) * 4).astype(np.float32)
    bias = rng.standard_normal((H, N, nc)).astype(np.float32)
    return x, bias, np.float32(1.0) / np.sqrt(np.float32(128.0)), nc - N


def _check_probs(O, got, x, sc, n_past):
    ref = O.scale_mask_softmax(x, float(sc), n_past, mode=O.ref_mode())
    got = got.reshape(ref.shape)
    assert np.allclose(got, ref, rtol=1.5e-3, atol=1e-7), float(np.max(np.abs(got - ref)))  # test_scale_mask_softmax's bound
    assert np.allclose(got.sum(-1), 1.0, atol=1e-5)


@pytest.mark.parametrize("reader_first", [True, False])
def test_scale_mask_softmax_in_place_with_a_second_reader(G, O, reader_first):
    """The in-place chain whose scaled tensor has a second reader, add(s, bias).  Expanded before the mask, the reader sits
    between scale and mask and sees x s; expanded after the chain, it reads the bytes the soft_max left there (ggml's in-place
    semantics): p + bias.  Either way the chain's own result is the probabilities."""
    x, bias, sc, n_past = _sms_inputs(89)
    H, N, nc = SMS["H"], SMS["N"], SMS["nc"]

    def build(ctx):
        src = ctx.op_cont(ctx.tensor_from(x, G.TYPE_F32, (nc, N, H)))
        s = ctx.op_scale_inplace(src, ctx.new_f32(float(sc)))
        r = ctx.op_add(s, ctx.tensor_from(bias, G.TYPE_F32, (nc, N, H)))
        p = ctx.op_soft_max_inplace(ctx.op_diag_mask_inf_inplace(s, n_past))
        return {"r": r, "p": p} if reader_first else {"p": p, "r": r}

    got = _both(G, build)
    _check_probs(O, got["p"], x, sc, n_past)
    seen = x * sc if reader_first else got["p"].reshape(x.shape)
    assert np.array_equal(got["r"].reshape(x.shape), seen + bias)


def test_scale_mask_softmax_out_of_place_with_a_second_reader(G, O):
    """The same chain built out of place: nothing fuses, every node keeps its own result."""
    x, bias, sc, n_past = _sms_inputs(90)
    H, N, nc = SMS["H"], SMS["N"], SMS["nc"]

    def build(ctx):
        s = ctx.op_scale(ctx.op_cont(ctx.tensor_from(x, G.TYPE_F32, (nc, N, H))), ctx.new_f32(float(sc)))
        p = ctx.op_soft_max(ctx.op_diag_mask_inf(s, n_past))
        return {"p": p, "r": ctx.op_add(s, ctx.tensor_from(bias, G.TYPE_F32, (nc, N, H))), "s": s}

    got = _both(G, build)
    _check_probs(O, got["p"], x, sc, n_past)
    assert np.array_equal(got["s"].reshape(x.shape), x * sc)
    assert np.array_equal(got["r"].reshape(x.shape), x * sc + bias)
