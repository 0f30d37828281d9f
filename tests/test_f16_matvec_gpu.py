"""The F16 plan's mat-vec k_mmvq_f16 (kernels/decode_f16.h) at op level: ONE launch (one per pass of 8 / 4 / 2 / 1 columns) through
ggml_hip_debug_mat_vec_f16, with the (activation source, epilogue) pairs plan_launch_f16 launches.

KE_ROW against the oracle's F16 mul_mat (mode 0: exact products of the f16 operands summed in double) with the operand PINNED:
the oracle multiplies the row the kernel staged (the host row, or the device's own normed row y_out), so both sides round the
same f32 row to the same f16 values and what is left is the device's f32 accumulation.  The bound is derived, not measured: K
products, each added into an f32 partial sum whose magnitude never exceeds S = sum|a_i b_i| — every addition (64 lanes' chains and
the reduction tree together add each product once, through at most K roundings) errs by at most 2^-24 of a partial sum <= S —
and the reference's own rounding to f32 and the comparison take 2^-23 |ref|:
    |dev - ref| <= K 2^-24 sum|a_i b_i| + 2^-23 |ref|      (+ 2^-24 |out| for the f32 addition of `res`)
a, b: the f16-rounded operands; sum|a_i b_i| in numpy float64 from the same rounded values.

The other epilogues are checked against the device's own KE_ROW results, bit for bit — legitimate by the kernel's design rule (a
row's result is a pure function of the row's bytes, the staged column and K), which is itself tested here: column c of a launch
of 8 (and of 3) columns equals the single-column launch of that column."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 256
KNORM, KF32, KSILU = 1, 2, 3  # kernels/kquant_big.h KX_*
KROW, KGATE, KQKV = 0, 1, 2   # ... KE_*
T_F16 = 1
EPS = 1e-5
SENTINEL = 0x5555  # a finite f16: what the caches hold where nothing may be written


def _buf(n, dtype=np.float32, init=None):
    b = np.full(n * np.dtype(dtype).itemsize + GUARD, 0xFF, np.uint8)
    v = b[:n * np.dtype(dtype).itemsize].view(dtype)
    if init is not None:
        v[:] = init
    return b, v


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _w16(rng, M, K):
    return (0.05 * rng.standard_normal((M, K))).astype(np.float16)


def _x(rng, n, K):
    x = rng.standard_normal((n, K)).astype(np.float32)
    x[:, ::7] *= 4.0
    return x


def _hook(G, ws, xsrc, epi, x, xw=None, res=None, y=False, qkv=None):
    """ws: f16 matrices [M_i, K]; x [ncols, K].  Returns (rc, out [ncols, M], y_out [ncols, K] or None, K cache, V cache)."""
    ncols, K = x.shape
    Ms = [w.shape[0] for w in ws]
    n_out = ncols * (Ms[0] if epi in (KGATE, KQKV) else sum(Ms))
    ob, out = _buf(n_out)
    yb, yv = _buf(ncols * K) if y else (None, None)
    kb = vb = kc = vc = None
    n_past, D, C = 0, 0, 0
    if qkv is not None:
        n_past, D, C = qkv["n_past"], qkv["D"], qkv["C"]
        kb, kc = _buf(C * Ms[1], np.uint16, SENTINEL)
        vb, vc = _buf(C * Ms[1], np.uint16, SENTINEL)
    x = np.ascontiguousarray(x, np.float32)
    xw = None if xw is None else np.ascontiguousarray(xw, np.float32)
    res = None if res is None else np.ascontiguousarray(res, np.float32)
    with G.Context(sum(w.nbytes for w in ws) + (1 << 20)) as ctx:
        ps = []
        for i, w in enumerate(ws):
            t = ctx.tensor_from(np.ascontiguousarray(w).view(np.uint8).reshape(-1), T_F16, (w.shape[1], w.shape[0])).set_name(f"w{i}")
            t.transfer_to_gpu()
            ps.append(t.ptr)
        ps += [None] * (3 - len(ps))
        rc = G.lib().ggml_hip_debug_mat_vec_f16(ps[0], ps[1], ps[2], xsrc, epi, _ptr(x), _ptr(xw), EPS, _ptr(res), _ptr(ob), _ptr(yb),
                                                n_past, D, 10000.0, 1.0, C, _ptr(kb), _ptr(vb), ncols)
    if rc != 0:
        return rc, None, None, None, None
    assert not np.any(ob[:n_out * 4] .view(np.uint32) == 0xFFFFFFFF), "an output element never written"
    assert np.all(ob[n_out * 4:] == 0xFF), "out: a store past the end"
    if y:
        assert not np.any(yb[:ncols * K * 4].view(np.uint32) == 0xFFFFFFFF) and np.all(yb[ncols * K * 4:] == 0xFF), "y_out"
    if qkv is not None:
        assert np.all(kb[C * Ms[1] * 2:] == 0xFF) and np.all(vb[C * Ms[1] * 2:] == 0xFF), "a cache store past the end"
    M = n_out // ncols
    return rc, out.reshape(ncols, M).copy(), None if yv is None else yv.reshape(ncols, K).copy(), kc, vc


def _check_rows(name, O, got, w, a_f32, res=None):
    """got [n, M] against the oracle on the staged operand a_f32 [n, K] (rounded to f16 by both sides)."""
    M, K = w.shape
    a = a_f32.astype(np.float16)
    ref = O.mul_mat(T_F16, np.ascontiguousarray(w).view(np.uint8).reshape(-1), M, K, a.astype(np.float32), mode=0).astype(np.float64)
    S = np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)).T  # [n, M]
    bound = K * 2.0 ** -24 * S + 2.0 ** -23 * np.abs(ref)
    want = ref
    if res is not None:
        want = ref + res.astype(np.float64)
        bound = bound + 2.0 ** -24 * np.abs(got.astype(np.float64))
    err = np.abs(got.astype(np.float64) - want)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{name}: worst |dev - ref| / bound = {worst:.3g} over {got.size} elements")
    assert np.all(err <= bound), f"{name}: {int(np.count_nonzero(err > bound))} elements beyond the bound, worst {worst:.3g}"


def _executor_norm(G, x, w):
    with G.Context(x.nbytes * 4 + (1 << 20)) as ctx:
        tx, tw = ctx.tensor_from(x), ctx.tensor_from(w)
        y = ctx.op_mul(ctx.op_rms_norm(tx, EPS), tw)
        ctx.graph().build_forward_expand(y).compute()
        return y.read_data().reshape(x.shape).copy()


def _executor_silu_mul(G, a, b):
    with G.Context(a.nbytes * 6 + (1 << 20)) as ctx:
        ta, tb = ctx.tensor_from(a.reshape(-1)), ctx.tensor_from(b.reshape(-1))
        y = ctx.op_mul(ctx.op_silu(ctx.op_cont(ta)), tb)
        ctx.graph().build_forward_expand(y).compute()
        return y.read_data().reshape(a.shape).copy()


def _executor_rope(G, x, H, D, n_past):
    """x [n, H * D] -> RoPE mode 0 of token i at position n_past + i (k_rope: the expression and table arithmetic of k_k_rope_store)."""
    n = x.shape[0]
    with G.Context(x.nbytes * 4 + (1 << 20)) as ctx:
        tx = ctx.tensor_from(np.ascontiguousarray(x), G.TYPE_F32, (D, H, n))
        out = ctx.op_cont(ctx.op_rope_inplace(tx, n_past, D, 0, 0))
        ctx.graph().build_forward_expand(out).compute()
        return out.read_data().reshape(n, H * D).copy()


@pytest.mark.parametrize("ncols", [1, 3, 8])
@pytest.mark.parametrize("M", [2, 256, 514])
@pytest.mark.parametrize("K", [128, 352, 2816])
def test_rows_match_the_oracle_and_the_design_rule_holds(G, O, K, M, ncols):
    """KE_ROW with every source and with / without res; y_out against the executor's normed row; column c of the launch against
    the single-column launch of column c."""
    rng = np.random.default_rng([K, M, ncols])
    w = _w16(rng, M, K)
    x = _x(rng, ncols, K)
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
    res = rng.standard_normal((ncols, M)).astype(np.float32)
    tag = f"K {K} M {M} ncols {ncols}"
    # KX_F32
    rc, out, _, _, _ = _hook(G, [w], KF32, KROW, x)
    assert rc == 0
    _check_rows(tag + " f32", O, out, w, x)
    rc, out_r, _, _, _ = _hook(G, [w], KF32, KROW, x, res=res)
    assert rc == 0
    _check_rows(tag + " f32 + res", O, out_r, w, x, res)
    assert np.array_equal(out_r, out + res)  # the same row sums, one f32 addition
    # KX_NORM with the tap: the normed rows are the executor's, bit for bit; the oracle multiplies them
    rc, out_n, y, _, _ = _hook(G, [w], KNORM, KROW, x, nw, y=True)
    assert rc == 0
    assert np.array_equal(y, _executor_norm(G, x, nw)), tag + ": y_out differs from the executor's normed row"
    _check_rows(tag + " norm", O, out_n, w, y)
    rc, out_n2, _, _, _ = _hook(G, [w], KNORM, KROW, x, nw)  # ... and without it: the same results
    assert rc == 0 and np.array_equal(out_n2, out_n)
    rc, out_nr, _, _, _ = _hook(G, [w], KNORM, KROW, x, nw, res=res)
    assert rc == 0
    _check_rows(tag + " norm + res", O, out_nr, w, y, res)
    # the design rule: a column's results do not depend on the columns beside it, on their number or on its index
    if ncols > 1:
        for c in range(ncols):
            rc, one, _, _, _ = _hook(G, [w], KF32, KROW, x[c:c + 1])
            assert rc == 0 and np.array_equal(one[0], out[c]), (tag, c)
            rc, one, y1, _, _ = _hook(G, [w], KNORM, KROW, x[c:c + 1], nw, y=True)
            assert rc == 0 and np.array_equal(one[0], out_n[c]) and np.array_equal(y1[0], y[c]), (tag, c)


@pytest.mark.parametrize("ncols", [1, 8])
@pytest.mark.parametrize("K,M", [(128, 352), (1024, 2816), (352, 6)])
def test_silu_mul_source_stages_the_executors_row(G, O, K, M, ncols):
    """KX_SILU_MUL (w2 behind a w1 | w3 pair that was not gated in its epilogue): the staged row is silu(a) * b with the
    executor's SiLU — the launch equals the KX_F32 launch of the executor's product, bit for bit."""
    rng = np.random.default_rng([K, M, ncols, 5])
    w = _w16(rng, M, K)
    a, b = 3.0 * _x(rng, ncols, K), _x(rng, ncols, K)
    res = rng.standard_normal((ncols, M)).astype(np.float32)
    rc, out, _, _, _ = _hook(G, [w], KSILU, KROW, a, b, res=res)
    assert rc == 0
    prod = _executor_silu_mul(G, a, b)
    rc, want, _, _, _ = _hook(G, [w], KF32, KROW, prod, res=res)
    assert rc == 0 and np.array_equal(out, want)


@pytest.mark.parametrize("ncols", [1, 3, 8])
@pytest.mark.parametrize("K,F", [(128, 352), (1024, 2816), (352, 2)])
def test_gate_is_the_executors_silu_of_the_row_results(G, O, K, F, ncols):
    """KE_GATE = silu(a) * b with a, b the device's own KE_ROW results for w1 and w3 and the SiLU the executor's k_unary applies
    (a one-node graph), bit for bit."""
    rng = np.random.default_rng([K, F, ncols, 1])
    w1, w3 = _w16(rng, F, K), _w16(rng, F, K)
    x = _x(rng, ncols, K)
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
    rc, gate, _, _, _ = _hook(G, [w1, w3], KNORM, KGATE, x, nw)
    assert rc == 0 and gate.shape == (ncols, F)
    rc, rows, _, _, _ = _hook(G, [w1, w3], KNORM, KROW, x, nw)  # both matrices as plain rows: [ncols][F + F]
    assert rc == 0 and rows.shape == (ncols, 2 * F)
    a, b = np.ascontiguousarray(rows[:, :F]), np.ascontiguousarray(rows[:, F:])
    rc, a1, _, _, _ = _hook(G, [w1], KNORM, KROW, x, nw)  # (a row's result does not depend on the matrices beside it either)
    assert rc == 0 and np.array_equal(a1, a)
    assert np.array_equal(gate, _executor_silu_mul(G, a, b))


QKV_SHAPES = {"tiny": (128, 128, 128, 32), "gqa2": (1024, 1024, 512, 128)}  # K, E, Egqa, D
QKV_AT = [(0, 1), (7, 1), (63, 1), (0, 8), (7, 8), (56, 8)]  # (n_past, ncols) with n_past + ncols <= C = 64


@pytest.mark.parametrize("n_past,ncols", QKV_AT)
@pytest.mark.parametrize("shape", list(QKV_SHAPES))
def test_qkv_rotates_and_stores_the_row_results(G, O, shape, n_past, ncols):
    """KE_QKV: Q = the rotation (k_rope: k_k_rope_store's expression on k_rope_table's angles) of wq's KE_ROW results, the K
    cache rows of positions n_past + c = f16 of the rotated wk results, the V cache columns = f16 of wv's; every other cache
    element is still the sentinel."""
    K, E, Eg, D = QKV_SHAPES[shape]
    C = 64
    rng = np.random.default_rng([K, n_past, ncols])
    wq, wk, wv = _w16(rng, E, K), _w16(rng, Eg, K), _w16(rng, Eg, K)
    x = _x(rng, ncols, K)
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
    rc, q, _, kc, vc = _hook(G, [wq, wk, wv], KNORM, KQKV, x, nw, qkv=dict(n_past=n_past, D=D, C=C))
    assert rc == 0 and q.shape == (ncols, E)
    rc, rows, _, _, _ = _hook(G, [wq, wk, wv], KNORM, KROW, x, nw)
    assert rc == 0
    rq, rk, rv = rows[:, :E], rows[:, E:E + Eg], rows[:, E + Eg:]
    assert np.array_equal(q, _executor_rope(G, rq, E // D, D, n_past))
    kr = _executor_rope(G, rk, Eg // D, D, n_past).astype(np.float16).view(np.uint16)
    mk, mv = kc.reshape(C, Eg), vc.reshape(Eg, C)
    at = slice(n_past, n_past + ncols)
    assert np.array_equal(mk[at], kr)
    assert np.array_equal(mv[:, at], rv.astype(np.float16).view(np.uint16).T)
    others = np.ones(C, bool)
    others[at] = False
    assert np.all(mk[others] == SENTINEL) and np.all(mv[:, others] == SENTINEL)


def test_the_hook_refuses_what_the_plan_would_not_launch(G, O):
    rng = np.random.default_rng(3)
    one = np.ones((1, 132), np.float32)
    assert _hook(G, [_w16(rng, 16, 132)], KF32, KROW, one)[0] == -1  # K % 8 != 0
    x = _x(rng, 1, 128)
    nw = np.ones(128, np.float32)
    ws = [_w16(rng, 33, 128), _w16(rng, 33, 128), _w16(rng, 33, 128)]
    assert _hook(G, ws, KNORM, KQKV, x, nw, qkv=dict(n_past=0, D=1, C=8))[0] == -1    # an odd M with KE_QKV (whatever D says)
    assert _hook(G, ws, KNORM, KQKV, x, nw, qkv=dict(n_past=0, D=33, C=8))[0] == -1
    ok = [_w16(rng, 64, 128), _w16(rng, 32, 128), _w16(rng, 32, 128)]
    assert _hook(G, ok, KNORM, KQKV, x, nw, qkv=dict(n_past=8, D=32, C=8))[0] == -1   # the column's position outside the cache
    assert _hook(G, ok, KNORM, KQKV, x, nw, qkv=dict(n_past=7, D=32, C=8))[0] == 0
    assert _hook(G, [ok[0]], KF32, KGATE, x)[0] == -1                                 # a pair no plan launches
