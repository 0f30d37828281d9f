"""GPU parity, op by op, of the kernels the generic executor runs node by node for every family but LLaMA (GPT-2, GPT-NeoX,
Falcon, GPT-J, BLOOM, MPT): kernels/ops.h k_norm, k_unary / k_unary4 (the SiLU and GELU f16 tables), k_cpy, k_bin / k_bin4,
k_mul_mat_f32 / k_mul_mat_f16 (and the fall-back from k_gemm_f16), k_scale, k_diag_mask_inf, k_soft_max, k_get_rows, k_rms_norm.
The whole-model tests of those families bound logits at 4e-2 sigma; here every op is held to an exact or derived bound at the
shapes, layouts and values where such kernels go wrong.

Every case is a graph of a few nodes computed once through ggml_graph_compute.  No case reaches an abort of its op_* launcher
(backend_ops.inc): layouts an op refuses are left out and named in the test's docstring.  Results that are not contiguous
nodes are not mirrored to the host: they are read with device_get on the parent tensor, which was filled with a sentinel first,
and every byte outside the destination view must still hold it."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = 0xA5  # sentinel byte: 0xA5A5A5A5 is a finite f32 (-2.9e-16), 0xA5A5 a finite f16, both unlike any expected result


@contextlib.contextmanager
def _fuse(G, value):
    G.set_option("fuse", value)
    try:
        yield
    finally:
        G.set_option("fuse", 1)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(got, exp):
    """bit for bit where exp is a number, NaN (any payload) where exp is NaN"""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return False
    if exp.dtype.kind != "f":
        return bool(np.array_equal(got, exp))
    nan = np.isnan(exp)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(exp)[~nan]))


def _gtype(G, dt):
    return {np.dtype(np.float32): G.TYPE_F32, np.dtype(np.float16): G.TYPE_F16, np.dtype(np.int32): G.TYPE_I32}[np.dtype(dt)]


def _sentinel(G, ctx, dt, *ne):
    """a tensor of ggml shape ne whose bytes are all SENT, and the numpy array (reversed shape) it holds"""
    t = ctx.new_tensor(_gtype(G, dt), *ne)
    fill = np.full(int(np.prod(ne)) * np.dtype(dt).itemsize, SENT, np.uint8)
    t.write_data(fill)
    return t, fill.view(dt).reshape(tuple(reversed(ne))).copy()


def _compute(ctx, *outs):
    g = ctx.graph()
    for t in outs:
        g.build_forward_expand(t)
    g.compute()


# ---------------------------------------------------------------------------------------------------
# 1. LayerNorm (k_norm) against oracle.norm
# ---------------------------------------------------------------------------------------------------
NORM_E = [1, 2, 63, 64, 65, 100, 255, 256, 257, 1024, 4097]
NORM_CONST = np.array([3.25, -7.5, 1000.0, 0.0, -0.015625, 65536.0, 1.0], np.float32)  # dyadic: E copies sum exactly


def _norm_inputs(rng, shape):
    """gaussian; gaussian + 1000 (large mean); constant rows (variance 0: eps decides); one huge element per row"""
    rows = int(np.prod(shape[:-1]))
    E = shape[-1]
    g = rng.standard_normal(shape).astype(np.float32)
    const = np.repeat(NORM_CONST[np.arange(rows) % NORM_CONST.size], E).reshape(shape)
    huge = rng.standard_normal(shape).astype(np.float32).reshape(rows, E)
    huge[:, E // 2] = np.where(np.arange(rows) % 2 == 0, 1e18, -1e18).astype(np.float32)  # its square, 1e36, is finite in f32
    return {"gauss": g, "mean1000": (g + np.float32(1000.0)).astype(np.float32), "const": const, "huge": huge.reshape(shape)}


def _check_norm(O, kind, x, got, tag):
    ref = O.norm(x)
    diff = int(np.count_nonzero(_bits(got) != _bits(ref)))
    print(f"layernorm {tag} {kind}: {diff} of {ref.size} elements not bit-equal")
    if kind == "const":
        assert not got.any() and not ref.any(), (kind, tag)
    assert np.allclose(got, ref, rtol=3e-7, atol=1e-7), (kind, tag, float(np.max(np.abs(got - ref))))


@pytest.mark.parametrize("N", [1, 3, 7])
@pytest.mark.parametrize("E", NORM_E)
def test_norm_rows(G, O, E, N):
    """Bound: test_rms_norm_and_weight's (rtol 3e-7, atol 1e-7).  Both sides sum in f64 and the build has no fast-math and
    -ffp-contract=off, so the results are almost always bit-equal; the share that is not is printed, not asserted.  Rows of
    one value come out exactly 0 on both sides."""
    xs = _norm_inputs(np.random.default_rng([E, N, 1]), (N, E))
    with G.Context(1 << 22) as ctx:
        ys = {k: ctx.op_norm(ctx.tensor_from(x)) for k, x in xs.items()}
        _compute(ctx, *ys.values())
        gots = {k: y.read_data().reshape(N, E) for k, y in ys.items()}
    for k, x in xs.items():
        _check_norm(O, k, x, gots[k], f"E={E} N={N}")


@pytest.mark.parametrize("shape", [(2, 3, 100), (3, 2, 257)])
def test_norm_3d(G, O, shape):
    """[E, N, H] input: rows are indexed through nb[1] and nb[2]."""
    xs = _norm_inputs(np.random.default_rng([7, *shape]), shape)
    with G.Context(1 << 22) as ctx:
        ys = {k: ctx.op_norm(ctx.tensor_from(x)) for k, x in xs.items()}
        _compute(ctx, *ys.values())
        gots = {k: y.read_data().reshape(shape) for k, y in ys.items()}
    for k, x in xs.items():
        _check_norm(O, k, x, gots[k], f"shape={shape}")


def test_norm_strided_view(G, O):
    """A view_2d into a wider tensor at a non-zero offset: row stride 80 floats, rows of 65.  op_norm asserts nb[0] == 4 on
    both sides only, so the layout is admitted; ggml_norm has no in-place form, so the result is always a contiguous node."""
    W, R, E, N = 80, 6, 65, 4
    xs = _norm_inputs(np.random.default_rng(80), (R, W))
    with G.Context(1 << 22) as ctx:
        ys = {}
        for k, x in xs.items():
            v = ctx.op_view_2d(ctx.tensor_from(x), E, N, W * 4, (W + 7) * 4)
            assert v.nb[0] == 4 and v.nb[1] == W * 4
            ys[k] = ctx.op_norm(v)
        _compute(ctx, *ys.values())
        gots = {k: y.read_data().reshape(N, E) for k, y in ys.items()}
    for k, x in xs.items():
        _check_norm(O, k, np.ascontiguousarray(x[1:1 + N, 7:7 + E]), gots[k], "view")


# ---------------------------------------------------------------------------------------------------
# 2. SiLU and GELU over the whole f16 table
# ---------------------------------------------------------------------------------------------------
GELU_TANH_ULP = 5  # no ulp bound for tanhf is documented with the device math library shipped here: the OpenCL full-profile bound it is built to
SILU_EDGE_CAP, GELU_SATURATED, GELU_UNSTABLE_CAP = 109, 27944, 897
_TABLE = {}


def _table(O):
    """Every finite f16 value as f32, with the accepted results of silu and gelu, computed once on the host."""
    if _TABLE:
        return _TABLE
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    x = h[np.isfinite(h)].astype(np.float32)
    assert x.size == 63488
    x64 = x.astype(np.float64)
    T = {"x": x}
    # SiLU.  The oracle is f16(x / (1 + expf(-x))) in f32.  An entry whose f64 value lies within relative 2^-20 (16 f32 ulps:
    # expf, the add and the divide with room) of the midpoint of its two f16 neighbours may take either neighbour; every other
    # entry must equal the oracle.
    with np.errstate(over="ignore"):
        v = x64 / (1.0 + np.exp(-x64))
        r = v.astype(np.float16)
        up = np.nextafter(r, np.float16(np.inf)).astype(np.float64)
        dn = np.nextafter(r, np.float16(-np.inf)).astype(np.float64)
    r64 = r.astype(np.float64)
    lo, hi = np.where(r64 <= v, r64, dn), np.where(r64 <= v, up, r64)
    with np.errstate(invalid="ignore"):
        edge = np.abs(v - 0.5 * (lo + hi)) <= 2.0 ** -20 * np.abs(v)
    assert int(edge.sum()) <= SILU_EDGE_CAP, int(edge.sum())
    T["silu"] = O.silu(x, mode=O.ref_mode())
    T["silu_lo"], T["silu_hi"], T["silu_edge"] = lo.astype(np.float32), hi.astype(np.float32), edge
    assert int(np.count_nonzero(T["silu"] != r.astype(np.float32))) <= 1  # the oracle itself is f16(silu_f64) but for one entry
    # GELU.  0.5 x (1 + tanhf(arg)) cancels for negative x, so the accepted set is built from the oracle's own f32 formula with
    # tanh moved by +-GELU_TANH_ULP ulps around its correctly rounded value.
    one, half = np.float32(1.0), np.float32(0.5)
    arg = np.float32(0.79788456080286535587989211986876) * x * (one + np.float32(0.044715) * x * x)
    sat = np.abs(arg) >= 10
    assert int(sat.sum()) == GELU_SATURATED
    t = np.tanh(arg.astype(np.float64)).astype(np.float32)

    def formula(tt):
        return (half * x * (one + np.clip(tt, -one, one))).astype(np.float16).astype(np.float32)

    t_lo, t_hi = t, t
    for _ in range(GELU_TANH_ULP):
        t_lo, t_hi = np.nextafter(t_lo, np.float32(-np.inf)), np.nextafter(t_hi, np.float32(np.inf))
    a, b = formula(t_lo), formula(t_hi)
    g64 = (0.5 * x64 * (1.0 + np.tanh(0.79788456080286535587989211986876 * x64 * (1.0 + 0.044715 * x64 * x64))))
    g64 = g64.astype(np.float16).astype(np.float32)
    unstable = (a != b) & ~sat
    assert int(unstable.sum()) <= GELU_UNSTABLE_CAP, int(unstable.sum())
    T["gelu"] = O.gelu(x, mode=O.ref_mode())
    assert np.array_equal(T["gelu"][sat], np.where(x[sat] > 0, x[sat], np.float32(0.0)))  # saturated: x, or zero
    T["gelu_sat"], T["gelu_unstable"] = sat, unstable
    T["gelu_lo"], T["gelu_hi"] = np.minimum(np.minimum(a, b), g64), np.maximum(np.maximum(a, b), g64)
    _TABLE.update(T)
    return _TABLE


def _check_silu(T, got, sel):
    ref, lo, hi, edge, x = (T[k][sel] for k in ("silu", "silu_lo", "silu_hi", "silu_edge", "x"))
    ok = np.where(edge, (got == lo) | (got == hi), got == ref)  # compared as numbers: -0.0 == 0.0
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, [(float(x[i]), float(got[i]), float(ref[i]), bool(edge[i])) for i in bad[:10]]


SILU_LAUNCHES = ["plain", "fused4", "fused_n3", "fused_n2", "fused_n1", "fused_view"]


@pytest.mark.parametrize("launch", SILU_LAUNCHES)
def test_silu_table_all_f16(G, O, launch):
    """All 63488 finite f16 values through each launch shape of op_unary: plain k_unary<SILU>; k_unary4<SILU, true> (fused
    silu*b, n % 4 == 0, 16-byte aligned); the scalar k_unary<SILU, true> through n % 4 = 3, 2, 1 and through an operand that is a
    view_1d at a 4-byte offset (contiguous, not 16-byte aligned).  b holds powers of two, so got / b is the table value exactly."""
    T = _table(O)
    x = T["x"]
    n = x.size
    off = 0
    if launch.startswith("fused_n"):
        n -= 4 - int(launch[-1])
        assert n % 4 == int(launch[-1])
    elif launch == "fused_view":
        n, off = n - 4, 1
    sel = slice(off, off + n)
    b = (2.0 ** ((np.arange(n) % 5) - 2)).astype(np.float32)
    with _fuse(G, 1), G.Context(1 << 22) as ctx:
        if launch == "plain":
            y = ctx.op_silu(ctx.tensor_from(x))
            b = np.ones(n, np.float32)
        elif launch == "fused_view":
            a = ctx.op_view_1d(ctx.tensor_from(x), n, 4)
            assert G.lib().ggml_is_contiguous(a.ptr) and (a.t.data - a.t.src[0].contents.data) == 4
            y = ctx.op_mul(ctx.op_silu(a), ctx.tensor_from(b))
        else:
            y = ctx.op_mul(ctx.op_silu(ctx.tensor_from(x[:n])), ctx.tensor_from(b))
        _compute(ctx, y)
        got = y.read_data()
    _check_silu(T, got / b, sel)


def test_gelu_table_all_f16(G, O):
    """All 63488 finite f16 values through k_unary<GELU>.  Acceptance (K = GELU_TANH_ULP = 5; the device math library shipped
    here documents no ulp bound for tanhf, so the OpenCL full-profile bound it is built to is taken):
      saturated entries (|arg| >= 10 in f32, 27944 of them): exactly x for x > 0, zero for x < 0, as the oracle gives;
      other entries: with t the correctly rounded f32 tanh(arg), a and b the f16-rounded results of the oracle's f32 formula at
      t - K ulp and t + K ulp (clamped to [-1, 1]): the device lies in the closed interval spanned by a, b and
      f16(gelu_f64(x)), and equals the oracle exactly where a == b.  At most 897 entries have a != b (830 of them at x < -3).
    Found when written: x = +-0.001339, where the f32 product is an exact f16 tie and the kernel rounded it once, to the other
    neighbour (v_fma_mixlo_f16); gelu_table now rounds to f32 first, as ggml does."""
    T = _table(O)
    x = T["x"]
    with G.Context(1 << 22) as ctx:
        y = ctx.op_gelu(ctx.tensor_from(x))
        _compute(ctx, y)
        got = y.read_data()
    sat, unstable, ref = T["gelu_sat"], T["gelu_unstable"], T["gelu"]
    ok = np.where(sat | ~unstable, got == ref, (got >= T["gelu_lo"]) & (got <= T["gelu_hi"]))
    ok &= (got >= T["gelu_lo"]) & (got <= T["gelu_hi"]) | sat
    bad = np.flatnonzero(~ok)
    print(f"gelu: {bad.size} entries outside the accepted set; {int(np.count_nonzero(got != ref))} differ from the oracle")
    if bad.size:
        err = np.abs(got[bad].astype(np.float64) - ref[bad])
        late = bad[x[bad] >= -3]
        print(f"gelu: outside at x >= -3: {late.size}; max |got - oracle| over all outside entries {err.max():.3e}")
    assert bad.size == 0, [(float(x[i]), float(got[i]), float(ref[i]), float(T["gelu_lo"][i]), float(T["gelu_hi"][i]))
                           for i in bad[:10]]


def test_unary_non_finite(G, O):
    """+-inf, NaN and f32 values beyond the f16 range (f16(x) = +-inf) through the plain kernels and the fused silu*b
    (n % 4 == 0: k_unary4), against the oracle with NaN equal to NaN."""
    x = np.array([np.inf, -np.inf, 1e6, -1e6, 70000.0, -70000.0, np.nan, 65520.0], np.float32)
    with _fuse(G, 1), G.Context(1 << 20) as ctx:
        s = ctx.op_silu(ctx.tensor_from(x))
        ge = ctx.op_gelu(ctx.tensor_from(x))
        f = ctx.op_mul(ctx.op_silu(ctx.tensor_from(x)), ctx.tensor_from(np.ones(8, np.float32)))
        _compute(ctx, s, ge, f)
        got_s, got_g, got_f = s.read_data(), ge.read_data(), f.read_data()
    with np.errstate(all="ignore"):
        ref_s, ref_g = O.silu(x, mode=O.ref_mode()), O.gelu(x, mode=O.ref_mode())
    assert np.array_equal(got_s, ref_s, equal_nan=True), (got_s, ref_s)
    assert np.array_equal(got_f, ref_s, equal_nan=True), (got_f, ref_s)
    assert np.array_equal(got_g, ref_g, equal_nan=True), (got_g, ref_g)


# ---------------------------------------------------------------------------------------------------
# 3. k_cpy: every type pair, every layout
# ---------------------------------------------------------------------------------------------------
CPY_PAIRS = {"f32_f32": (np.float32, np.float32), "f32_f16": (np.float32, np.float16), "f16_f16": (np.float16, np.float16),
             "f16_f32": (np.float16, np.float32), "i32_i32": (np.int32, np.int32)}
CPY_SHAPES = [(5, 3, 7, 2), (5, 3, 10, 2)]  # ggml order; 210 elements (one workgroup) and 300 (two)


def _h(bits):
    return np.array(bits, np.uint16).view(np.float16).astype(np.float64)


def _f32_specials():
    """f32 inputs at the edges of the conversion to f16 (round to nearest even)"""
    lows = np.array([0x3C00, 0x3C01, 0x0400, 0x03FF, 0x0001, 0x0002, 0x7BFE, 0x5BFF], np.uint16)
    mids = 0.5 * (_h(lows) + _h(lows + 1))  # exact ties between f16 neighbours, even and odd lower neighbour
    pos = np.concatenate([mids, [
        65519.99, 65520.0, 1e6, 65504.0,           # the last three round to inf, inf, max: 65520 is the tie of max and 2^16
        2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -14 * (1 - 2.0 ** -12),  # smallest normal, and just below it
        2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10), 2.0 ** -26, 1e-10,  # smallest subnormal; its half ties to 0
        3 * 2.0 ** -25, 0.0, np.inf]])
    return np.concatenate([pos, -pos, [np.nan]]).astype(np.float32)


def _cpy_values(rng, n, dt):
    if np.dtype(dt) == np.float32:
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-9, 6, n)).astype(np.float32)
        s = _f32_specials()
        assert s.size <= n
        v[:s.size] = s
        return v
    if np.dtype(dt) == np.float16:
        v = rng.integers(0, 65536, n).astype(np.uint16)
        s = np.array([0, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFE01, 1, 0x8001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF], np.uint16)
        v[:s.size] = s
        return v.view(np.float16)
    v = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    v[:4] = [0, -1, 2 ** 31 - 1, -2 ** 31]
    return v


def _convert(v, dt):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(v).astype(dt)


def _np_permute(a, axes):
    """numpy twin of ggml_permute: a has the reversed ggml shape (n3, n2, n1, n0); result likewise"""
    g = a.transpose(3, 2, 1, 0)  # indexed [i0, i1, i2, i3]
    perm = [0] * 4
    for k, ax in enumerate(axes):
        perm[ax] = k  # result axis axes[k] is source axis k
    return g.transpose(perm).transpose(3, 2, 1, 0)


def _cpy_case(G, ctx, layout, sdt, ddt, shape, rng):
    """Builds one copy; returns (node, tensor to device_get, expected contents of that tensor)."""
    n0, n1, n2, n3 = shape
    n = n0 * n1 * n2 * n3
    es = np.dtype(ddt).itemsize
    vals = _cpy_values(rng, n, sdt)
    if layout == "contig":
        src = ctx.tensor_from(vals.reshape(n3, n2, n1, n0))
        dst, _ = _sentinel(G, ctx, ddt, n0, n1, n2, n3)
        return ctx.op_cpy(src, dst), dst, _convert(vals, ddt).reshape(n3, n2, n1, n0)
    if layout == "permute":  # merge heads: permute(0, 2, 1, 3) source -> contiguous
        P = vals.reshape(n3, n2, n1, n0)
        src = ctx.op_permute(ctx.tensor_from(P), 0, 2, 1, 3)
        dst, _ = _sentinel(G, ctx, ddt, n0, n2, n1, n3)
        return ctx.op_cpy(src, dst), dst, _convert(_np_permute(P, (0, 2, 1, 3)), ddt)
    if layout == "scatter":  # the V scatter: transposed source -> strided 2-D view at an offset
        m0, m1 = n0 * n1, n2 * n3
        P = vals.reshape(m1, m0)
        src = ctx.op_transpose(ctx.tensor_from(P))  # logical [m1, m0]
        C, R = m1 + 5, m0 + 3
        par, exp = _sentinel(G, ctx, ddt, C, R)
        dst = ctx.op_view_2d(par, m1, m0, C * es, (2 * C + 3) * es)
        exp[2:2 + m0, 3:3 + m1] = _convert(P.T, ddt)
        return ctx.op_cpy(src, dst), par, exp
    a, b, c = n0, n1, n2 * n3
    if layout == "reshape_contig":  # [a, b, c] -> [c, a b], both contiguous
        src = ctx.tensor_from(vals.reshape(c, b, a))
        dst, _ = _sentinel(G, ctx, ddt, c, a * b)
        return ctx.op_cpy(src, dst), dst, _convert(vals, ddt).reshape(a * b, c)
    if layout in ("reshape_ab_c", "reshape_c_ab"):  # a strided [a, b, c] source (permuted view of [a, c, b]) reshaped on the way
        P = vals.reshape(1, b, c, a)
        src = ctx.op_permute(ctx.tensor_from(P.reshape(b, c, a)), 0, 2, 1, 3)
        assert src.ne[:3] == (a, b, c)
        seq = _convert(_np_permute(P, (0, 2, 1, 3)), ddt).reshape(-1)
        if layout == "reshape_ab_c":  # -> contiguous [a b, c]
            dst, _ = _sentinel(G, ctx, ddt, a * b, c)
            return ctx.op_cpy(src, dst), dst, seq.reshape(c, a * b)
        C, R = c + 3, a * b + 2  # -> [c, a b] as a strided view at an offset
        par, exp = _sentinel(G, ctx, ddt, C, R)
        dst = ctx.op_view_2d(par, c, a * b, C * es, (C + 2) * es)
        exp[1:1 + a * b, 2:2 + c] = seq.reshape(a * b, c)
        return ctx.op_cpy(src, dst), par, exp
    if layout == "4d":  # ne3 = 2 on both sides, both strided: permute(1, 0, 3, 2) source -> permute(0, 2, 1, 3) view
        P = vals.reshape(n3, n2, n1, n0)
        src = ctx.op_permute(ctx.tensor_from(P), 1, 0, 3, 2)
        L = _np_permute(P, (1, 0, 3, 2))  # logical [n1, n0, n3, n2]
        par, _ = _sentinel(G, ctx, ddt, n1, n3, n0, n2)
        dst = ctx.op_permute(par, 0, 2, 1, 3)
        assert dst.ne == src.ne == (n1, n0, n3, n2)
        return ctx.op_cpy(src, dst), par, _convert(_np_permute(L, (0, 2, 1, 3)), ddt)  # the permutation is its own inverse
    raise AssertionError(layout)


@pytest.mark.parametrize("layout", ["contig", "permute", "scatter", "reshape_contig", "reshape_ab_c", "reshape_c_ab", "4d"])
@pytest.mark.parametrize("pair", list(CPY_PAIRS))
def test_cpy_layouts(G, pair, layout):
    """ggml_cpy for each type pair of k_cpy over each layout, at 210 and at 300 elements.  f32 -> f16 against numpy's astype
    (round to nearest even: exact ties of both parities, overflow to inf at 65520, the subnormal range, +-0, +-inf; NaN compared
    as NaN); the other pairs bit for bit.  Bytes of the parent outside a destination view keep their sentinel."""
    sdt, ddt = CPY_PAIRS[pair]
    for shape in CPY_SHAPES:
        rng = np.random.default_rng([len(pair), len(layout), shape[2]])
        with G.Context(1 << 22) as ctx:
            node, holder, exp = _cpy_case(G, ctx, layout, sdt, ddt, shape, rng)
            _compute(ctx, node)
            got = holder.device_get(ddt).reshape(exp.shape)
        assert _same(got, exp), (pair, layout, shape, np.flatnonzero(_bits(got).reshape(-1) != _bits(exp).reshape(-1))[:8])


@pytest.mark.parametrize("op", ["cont", "dup"])
@pytest.mark.parametrize("dt", [np.float32, np.float16, np.int32], ids=["f32", "f16", "i32"])
def test_cont_dup_of_permuted(G, op, dt):
    """ggml_cont and ggml_dup of a permuted source: contiguous nodes of the source's type, mirrored to the host."""
    axes = (0, 2, 1, 3) if op == "cont" else (1, 0, 3, 2)
    for shape in CPY_SHAPES:
        n0, n1, n2, n3 = shape
        P = _cpy_values(np.random.default_rng([shape[2], len(op)]), n0 * n1 * n2 * n3, dt).reshape(n3, n2, n1, n0)
        with G.Context(1 << 22) as ctx:
            y = getattr(ctx, "op_" + op)(ctx.op_permute(ctx.tensor_from(P), *axes))
            _compute(ctx, y)
            got = y.read_data(dt)
        exp = np.ascontiguousarray(_np_permute(P, axes))
        assert _same(got.reshape(exp.shape), exp), (op, shape)


def test_cpy_f16_to_f32_every_bit_pattern(G):
    """All 65536 f16 bit patterns: bit-exact f32 for every number, NaN for every NaN."""
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    with G.Context(1 << 22) as ctx:
        dst, _ = _sentinel(G, ctx, np.float32, 65536)
        _compute(ctx, ctx.op_cpy(ctx.tensor_from(h), dst))
        got = dst.device_get()
    assert _same(got, h.astype(np.float32))


def test_cpy_f32_to_f16_rounding_edges(G):
    """Every f32 special of _f32_specials and the exact tie above every fifteenth non-negative f16 value (all exponents), with
    both signs, in one contiguous copy."""
    lows = np.arange(0, 0x7C00, 15, dtype=np.uint16)  # stride 15: both parities of the lower neighbour
    ties = (0.5 * (_h(lows) + _h(lows + 1))).astype(np.float32)
    x = np.concatenate([_f32_specials(), ties, -ties])
    with G.Context(1 << 22) as ctx:
        dst, _ = _sentinel(G, ctx, np.float16, x.size)
        _compute(ctx, ctx.op_cpy(ctx.tensor_from(x), dst))
        got = dst.device_get(np.float16)
    exp = _convert(x, np.float16)
    assert _same(got, exp), [(float(x[i]), hex(int(_bits(got)[i])), hex(int(_bits(exp)[i])))
                             for i in np.flatnonzero(_bits(got) != _bits(exp))[:8]]


# ---------------------------------------------------------------------------------------------------
# 4. k_bin / k_bin4: add, mul, repeat — all exactly numpy f32
# ---------------------------------------------------------------------------------------------------
BIN_A = (12, 5, 3, 2)  # [E, N, H, B]
NP_OP = {"add": np.add, "mul": np.multiply}


def _rand(rng, *ne):
    return rng.standard_normal(tuple(reversed(ne))).astype(np.float32)


@pytest.mark.parametrize("bne", [(12,), (12, 1, 3), (12, 5, 1, 2), (12, 1, 1, 2)], ids=["E", "E1H", "EN1B", "E11B"])
@pytest.mark.parametrize("op", ["add", "mul"])
def test_bin_broadcast(G, op, bne):
    """b broadcast along each combination of dims 1..3 of a = [12, 5, 3, 2]: the `% b.ne[1..3]` arithmetic of k_bin."""
    rng = np.random.default_rng([len(bne), bne[-1]])
    a, b = _rand(rng, *BIN_A), _rand(rng, *bne)
    with G.Context(1 << 20) as ctx:
        y = getattr(ctx, "op_" + op)(ctx.tensor_from(a), ctx.tensor_from(b))
        _compute(ctx, y)
        got = y.read_data().reshape(a.shape)
    assert np.array_equal(got, NP_OP[op](a, b))


@pytest.mark.parametrize("op", ["add", "mul"])
def test_bin_tiling_b(G, op):
    """b tiles instead of broadcasting (can_repeat_rows allows any divisor): [E, N] into [E, 2N], [E, N, 2] into [E, 3N, 4]."""
    rng = np.random.default_rng(44)
    a1, b1 = _rand(rng, 12, 10), _rand(rng, 12, 5)
    a2, b2 = _rand(rng, 12, 9, 4), _rand(rng, 12, 3, 2)
    with G.Context(1 << 20) as ctx:
        f = getattr(ctx, "op_" + op)
        y1, y2 = f(ctx.tensor_from(a1), ctx.tensor_from(b1)), f(ctx.tensor_from(a2), ctx.tensor_from(b2))
        _compute(ctx, y1, y2)
        got1, got2 = y1.read_data().reshape(a1.shape), y2.read_data().reshape(a2.shape)
    assert np.array_equal(got1, NP_OP[op](a1, np.tile(b1, (2, 1))))
    assert np.array_equal(got2, NP_OP[op](a2, np.tile(b2, (2, 3, 1))))


@pytest.mark.parametrize("op", ["add", "mul"])
def test_bin_strided_operands(G, op):
    """a, then b, as a permute(0, 2, 1, 3) view: read through their strides, written to a contiguous node."""
    rng = np.random.default_rng(45)
    E, N, H, B = BIN_A
    pa, pb = _rand(rng, E, H, N, B), _rand(rng, E, H, N, B)
    full, row = _rand(rng, *BIN_A), _rand(rng, E)
    with G.Context(1 << 20) as ctx:
        f = getattr(ctx, "op_" + op)
        va = ctx.op_permute(ctx.tensor_from(pa), 0, 2, 1, 3)
        vb = ctx.op_permute(ctx.tensor_from(pb), 0, 2, 1, 3)
        y1, y2, y3 = f(va, ctx.tensor_from(row)), f(ctx.tensor_from(full), vb), f(va, vb)
        _compute(ctx, y1, y2, y3)
        got = [y.read_data().reshape(full.shape) for y in (y1, y2, y3)]
    la, lb = _np_permute(pa, (0, 2, 1, 3)), _np_permute(pb, (0, 2, 1, 3))
    assert np.array_equal(got[0], NP_OP[op](la, row))
    assert np.array_equal(got[1], NP_OP[op](full, lb))
    assert np.array_equal(got[2], NP_OP[op](la, lb))


def test_add_inplace(G):
    """ggml_add_inplace on a contiguous node (k_bin4 with d aliasing a), with a row b (k_bin), and into a strided view of a
    wider tensor: the parent's other bytes keep their sentinel."""
    rng = np.random.default_rng(46)
    a, b, row = _rand(rng, 12, 5), _rand(rng, 12, 5), _rand(rng, 12)
    with G.Context(1 << 20) as ctx:
        y1 = ctx.op_add_inplace(ctx.op_cont(ctx.tensor_from(a)), ctx.tensor_from(b))
        y2 = ctx.op_add_inplace(ctx.op_cont(ctx.tensor_from(a)), ctx.tensor_from(row))
        par, exp = _sentinel(G, ctx, np.float32, 20, 8)
        view = ctx.op_view_2d(par, 12, 5, 20 * 4, (20 + 3) * 4)
        y3 = ctx.op_add_inplace(view, ctx.tensor_from(b))
        _compute(ctx, y1, y2, y3)
        got1, got2 = y1.read_data().reshape(a.shape), y2.read_data().reshape(a.shape)
        got3 = par.device_get().reshape(exp.shape)
    assert np.array_equal(got1, a + b) and np.array_equal(got2, a + row)
    exp[1:6, 3:15] = exp[1:6, 3:15] + b
    assert _same(got3, exp)


def test_repeat(G):
    """[3, 2] into [6, 4, 2] (np.tile) and [1] into [7, 3]."""
    rng = np.random.default_rng(47)
    a, one = _rand(rng, 3, 2), _rand(rng, 1)
    with G.Context(1 << 20) as ctx:
        y1 = ctx.op_repeat(ctx.tensor_from(a), ctx.new_tensor(G.TYPE_F32, 6, 4, 2))
        y2 = ctx.op_repeat(ctx.tensor_from(one), ctx.new_tensor(G.TYPE_F32, 7, 3))
        _compute(ctx, y1, y2)
        got1, got2 = y1.read_data().reshape(2, 4, 6), y2.read_data().reshape(3, 7)
    assert np.array_equal(got1, np.tile(a, (2, 2, 2)))
    assert np.array_equal(got2, np.full((3, 7), one[0], np.float32))


@pytest.mark.parametrize("op", ["add", "mul"])
def test_bin_fast_path_boundary(G, op):
    """Same-shape contiguous operands with n % 4 == 0 take k_bin4; the same values with n % 4 != 0, and with one operand a
    view_1d at a 4-byte offset, fall back to k_bin.  All three give numpy's result, hence each other's."""
    n = 360
    rng = np.random.default_rng(48)
    a, b, tail = _rand(rng, n), _rand(rng, n), _rand(rng, 3)
    with G.Context(1 << 20) as ctx:
        f = getattr(ctx, "op_" + op)
        y4 = f(ctx.tensor_from(a), ctx.tensor_from(b))
        y3 = f(ctx.tensor_from(np.concatenate([a, tail])), ctx.tensor_from(np.concatenate([b, tail])))
        shifted = ctx.op_view_1d(ctx.tensor_from(np.concatenate([tail[:1], a])), n, 4)
        yv = f(shifted, ctx.tensor_from(b))
        yw = f(ctx.tensor_from(a), ctx.op_view_1d(ctx.tensor_from(np.concatenate([tail[:1], b])), n, 4))
        _compute(ctx, y4, y3, yv, yw)
        got4, got3, gotv, gotw = y4.read_data(), y3.read_data(), yv.read_data(), yw.read_data()
    ref = NP_OP[op](a, b)
    assert np.array_equal(got4, ref)
    assert np.array_equal(got3[:n], got4) and np.array_equal(got3[n:], NP_OP[op](tail, tail))
    assert np.array_equal(gotv, got4) and np.array_equal(gotw, got4)


# ---------------------------------------------------------------------------------------------------
# 5. k_mul_mat_f32, k_mul_mat_f16 and the fall-back from k_gemm_f16
# ---------------------------------------------------------------------------------------------------
def _mm_ref(a, b):
    """a [A3, A2, M, K], b [B3, B2, N, K] as the kernel sees them -> (ref [B3, B2, N, M] in f64, sum |a_i b_i|)"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    r3, r2 = b.shape[0] // a.shape[0], b.shape[1] // a.shape[1]
    a = np.repeat(np.repeat(a, r3, axis=0), r2, axis=1)  # ggml's broadcast: i02 = i12 / r2, i03 = i13 / r3
    return np.einsum("xymk,xynk->xynm", a, b), np.einsum("xymk,xynk->xynm", np.abs(a), np.abs(b))


def _mm_check(got, a, b, wtype):
    """|dev - ref| <= K 2^-24 sum|a_i b_i| + 2^-23 |ref| (derived in test_f16_matvec_gpu.py: every product enters an f32 partial
    sum once and passes through at most K roundings of a sum no larger than sum|a_i b_i|; the reference's rounding to f32 and the
    comparison take 2^-23 |ref|).  With f16 weights b is rounded to f16 first (ggml converts src1) and the products are exact;
    with f32 weights the product's own rounding is one more of those roundings: lanes hold ceil(K / 64) products and the wave
    reduction adds six levels, within K for every K used here but K = 1, where the single product is the single rounding."""
    if wtype == np.float16:
        b = b.astype(np.float16)
    ref, s = _mm_ref(a, b)
    K = a.shape[-1]
    err = np.abs(got.astype(np.float64) - ref)
    bound = K * 2.0 ** -24 * s + 2.0 ** -23 * np.abs(ref)
    assert np.all(err <= bound), (K, float(np.max(err - bound)))


def _mm_operands(rng, wtype, K, M, N, a_batch=(1, 1), b_batch=(1, 1)):
    a = (0.5 * rng.standard_normal((*a_batch, M, K))).astype(wtype)
    b = rng.standard_normal((*b_batch, N, K)).astype(np.float32)
    b[..., ::7] *= 4.0
    return a, b


@pytest.mark.parametrize("K", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("wtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_mul_mat_f32_f16_shapes(G, wtype, K):
    """M in {1, 3, 4, 5, 9} (one wave per row, four rows per workgroup) x N in {1, 2, 5}, all fifteen in one graph."""
    rng = np.random.default_rng([K, np.dtype(wtype).itemsize])
    cases = [(M, N, *_mm_operands(rng, wtype, K, M, N)) for M in (1, 3, 4, 5, 9) for N in (1, 2, 5)]
    with G.Context(1 << 22) as ctx:
        ys = [ctx.op_mul_mat(ctx.tensor_from(a[0, 0]), ctx.tensor_from(b[0, 0])) for _, _, a, b in cases]
        _compute(ctx, *ys)
        gots = [y.read_data() for y in ys]
    for (M, N, a, b), got in zip(cases, gots):
        _mm_check(got.reshape(1, 1, N, M), a, b, wtype)


@pytest.mark.parametrize("batch", [((1, 2), (1, 2)), ((1, 2), (1, 8)), ((2, 2), (2, 8)), ((1, 2), (2, 8))],
                         ids=["ne2", "gqa_r2_4", "ne3_2", "a_ne3_1_b_ne3_2"])
@pytest.mark.parametrize("wtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_mul_mat_batched_broadcast(G, wtype, batch):
    """a.ne[2] = 2 against b.ne[2] = 2 and 8 (a GQA broadcast, r2 = 4), ne3 = 2 on both, and a.ne[3] = 1 against b.ne[3] = 2."""
    K, M, N = 65, 5, 3
    a, b = _mm_operands(np.random.default_rng([sum(batch[0]), sum(batch[1])]), wtype, K, M, N, *batch)
    with G.Context(1 << 22) as ctx:
        y = ctx.op_mul_mat(ctx.tensor_from(a), ctx.tensor_from(b))
        assert y.ne == (M, N, batch[1][1], batch[1][0])
        _compute(ctx, y)
        got = y.read_data().reshape(*batch[1], N, M)
    _mm_check(got, a, b, wtype)


@pytest.mark.parametrize("wtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_mul_mat_strided_weight_view(G, wtype):
    """a as a view_2d whose row stride (77 elements) is wider than K = 65, at an offset.  b stays contiguous in dim 0:
    op_mul_mat asserts it."""
    K, M, N, W = 65, 5, 3, 77
    rng = np.random.default_rng(51)
    par, b = _mm_operands(rng, wtype, W, M + 2, N)
    b = np.ascontiguousarray(b[..., :K])
    es = np.dtype(wtype).itemsize
    with G.Context(1 << 22) as ctx:
        va = ctx.op_view_2d(ctx.tensor_from(par[0, 0]), K, M, W * es, (W + 6) * es)
        y = ctx.op_mul_mat(va, ctx.tensor_from(b[0, 0]))
        _compute(ctx, y)
        got = y.read_data().reshape(1, 1, N, M)
    _mm_check(got, par[:, :, 1:1 + M, 6:6 + K], b, wtype)


@pytest.mark.parametrize("layout", ["aligned", "offset2", "stride"])
def test_gemm_f16_and_its_fallback(G, layout):
    """K.Q of a prompt batch with a GQA broadcast (N = 40 >= mmq_min, r2 = 4) over an f16 cache [C rows of Hkv D] whose rows
    beyond T hold NaN.  `aligned` runs k_gemm_f16 and meets test_kv_store_and_attention_matmuls' bound for K.Q; a view at a
    2-byte offset, or with a row stride that is no multiple of 16 bytes, falls back to k_mul_mat_f16 and meets _mm_check's."""
    D, Hkv, r2, N, T, C = 32, 2, 4, 40, 45, 64
    H = Hkv * r2
    W = Hkv * D + (4 if layout == "stride" else 0)  # elements per cache row
    off = 1 if layout == "offset2" else 0
    rng = np.random.default_rng(52)
    cache = np.full(C * W + 8, np.nan, np.float16)
    cache[:T * W + off] = rng.standard_normal(T * W + off).astype(np.float16)
    q = rng.standard_normal((H, N, D)).astype(np.float32)
    assert G.get_option("mmq_min") > 0 and N >= G.get_option("mmq_min")
    with G.Context(1 << 22) as ctx:
        mk = ctx.tensor_from(cache)
        kv = ctx.op_view_3d(mk, D, T, Hkv, W * 2, D * 2, off * 2)
        aligned = (W * 2) % 16 == 0 and (D * 2) % 16 == 0 and off == 0
        assert aligned == (layout == "aligned")
        y = ctx.op_mul_mat(kv, ctx.tensor_from(q))
        assert y.ne == (T, N, H, 1)
        _compute(ctx, y)
        got = y.read_data().reshape(1, H, N, T)
    rows = cache[off:off + C * W].reshape(C, W)[:T, :Hkv * D].reshape(T, Hkv, D)
    a = np.ascontiguousarray(rows.transpose(1, 0, 2))[None]  # [1, Hkv, T, D]
    assert np.isfinite(a.astype(np.float32)).all() and np.isfinite(got).all()
    if layout == "aligned":
        ref, _ = _mm_ref(a, q.astype(np.float16)[None])
        assert np.allclose(got, ref, rtol=1e-5, atol=1e-5), float(np.max(np.abs(got - ref)))
    else:
        _mm_check(got, a, q[None], np.float16)


# ---------------------------------------------------------------------------------------------------
# 6. the stand-alone scale, diag_mask_inf, soft_max
# ---------------------------------------------------------------------------------------------------
SMS_CASES = [(nc, N) for nc in (1, 255, 256, 257, 1000) for N in (1, 4) if nc >= N]


@pytest.mark.parametrize("nc,N", SMS_CASES)
def test_scale_mask_softmax_standalone(G, O, nc, N):
    """H = 3, n_past = nc - N.  Out of place nothing fuses (fuse = 1) and each node's result is read: scale exactly x s; the
    mask exactly -inf above the diagonal and the input elsewhere; soft_max against the oracle on the device's masked input under
    test_scale_mask_softmax's bounds.  Row (0, 0) already holds -inf entries; row (1, N - 1) has one element far above the rest
    (every other exp underflows in f16).  In place, the fused launch (fuse = 1) and the three launches (fuse = 0) are
    bit-identical to each other and to the out-of-place result.  All operands are contiguous f32, which op_scale,
    op_diag_mask_inf and op_soft_max assert."""
    H, n_past = 3, nc - N
    rng = np.random.default_rng([nc, N])
    x = (rng.standard_normal((H, N, nc)) * 4).astype(np.float32)
    x[0, 0, 1::3] = -np.inf
    x[1, N - 1, 0] = 3000.0
    sc = np.float32(1.0) / np.sqrt(np.float32(128.0))

    def in_place(fuse):
        with _fuse(G, fuse), G.Context(1 << 22) as ctx:
            src = ctx.op_cont(ctx.tensor_from(x, G.TYPE_F32, (nc, N, H)))
            y = ctx.op_soft_max_inplace(ctx.op_diag_mask_inf_inplace(ctx.op_scale_inplace(src, ctx.new_f32(float(sc))), n_past))
            _compute(ctx, y)
            return y.read_data().reshape(H, N, nc)

    outs = {}
    for fuse in (0, 1):
        with _fuse(G, fuse), G.Context(1 << 22) as ctx:
            s = ctx.op_scale(ctx.tensor_from(x, G.TYPE_F32, (nc, N, H)), ctx.new_f32(float(sc)))
            m = ctx.op_diag_mask_inf(s, n_past)
            p = ctx.op_soft_max(m)
            _compute(ctx, p)
            outs[fuse] = [t.read_data().reshape(H, N, nc) for t in (s, m, p)]
    for got_s, got_m, got_p in outs.values():
        assert _same(got_s, x * sc)
        masked = np.arange(nc)[None, None, :] > n_past + np.arange(N)[None, :, None]
        assert _same(got_m, np.where(masked, np.float32(-np.inf), x * sc))
        ref = O.soft_max(got_m, mode=O.ref_mode())
        assert np.allclose(got_p, ref, rtol=1.5e-3, atol=1e-7), float(np.max(np.abs(got_p - ref)))
        assert np.allclose(got_p.sum(-1), 1.0, atol=1e-5)
        assert np.mean(np.abs(got_p - ref) > 1e-6 * np.abs(ref) + 1e-9) < 0.5
        assert np.allclose(got_p, O.soft_max(got_m, mode=1), rtol=2e-3, atol=1e-6)
        assert not got_p[masked.repeat(H, 0)].any() and not got_p[0, 0, 1::3].any()
        if nc > 1:
            assert got_p[1, N - 1, 0] == 1.0 and not got_p[1, N - 1, 1:].any()
    assert _same(outs[1][2], outs[0][2])
    fused, separate = in_place(1), in_place(0)
    assert _same(fused, separate) and _same(fused, outs[0][2])


# ---------------------------------------------------------------------------------------------------
# 7. small additions: get_rows from f32 / f16 tables, rms_norm on 3-D and strided inputs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne0", [1, 100, 257])
@pytest.mark.parametrize("dt", [np.float32, np.float16], ids=["f32", "f16"])
def test_get_rows_f32_f16(G, dt, ne0):
    """ids repeat and include the last row; ne0 = 257 crosses a workgroup, ne0 = 1 puts f16 rows at 2-byte offsets."""
    V = 9
    tab = np.random.default_rng([ne0, np.dtype(dt).itemsize]).standard_normal((V, ne0)).astype(dt)
    ids = np.array([8, 0, 8, 3, 3, 8, 7], np.int32)
    with G.Context(1 << 20) as ctx:
        y = ctx.op_get_rows(ctx.tensor_from(tab), ctx.tensor_from(ids))
        _compute(ctx, y)
        got = y.read_data().reshape(ids.size, ne0)
    assert _same(got, tab[ids].astype(np.float32))


@pytest.mark.parametrize("weight", [False, True], ids=["plain", "weight"])
@pytest.mark.parametrize("fuse", [0, 1])
def test_rms_norm_3d_and_strided(G, O, fuse, weight):
    """rms_norm on [E, N, H] = [100, 3, 2] and on a view_2d of row stride 80 > 65 at an offset (op_rms_norm asserts nb[0] == 4
    only), alone and followed by the weight multiply the executor fuses (fuse = 1).  Bound: test_rms_norm_and_weight's."""
    rng = np.random.default_rng(71)
    x3 = (rng.standard_normal((2, 3, 100)) * 3).astype(np.float32)
    par = (rng.standard_normal((6, 80)) * 3).astype(np.float32)
    w3, wv = (1 + 0.01 * rng.standard_normal(100)).astype(np.float32), (1 + 0.01 * rng.standard_normal(65)).astype(np.float32)
    with _fuse(G, fuse), G.Context(1 << 20) as ctx:
        y3 = ctx.op_rms_norm(ctx.tensor_from(x3), 5e-6)
        yv = ctx.op_rms_norm(ctx.op_view_2d(ctx.tensor_from(par), 65, 4, 80 * 4, (80 + 7) * 4), 5e-6)
        if weight:
            y3, yv = ctx.op_mul(y3, ctx.tensor_from(w3)), ctx.op_mul(yv, ctx.tensor_from(wv))
        _compute(ctx, y3, yv)
        got3, gotv = y3.read_data().reshape(x3.shape), yv.read_data().reshape(4, 65)
    ref3, refv = O.rms_norm(x3, 5e-6), O.rms_norm(np.ascontiguousarray(par[1:5, 7:72]), 5e-6)
    if weight:
        ref3, refv = ref3 * w3, refv * wv
    assert np.allclose(got3, ref3, rtol=3e-7, atol=1e-7), float(np.max(np.abs(got3 - ref3)))
    assert np.allclose(gotv, refv, rtol=3e-7, atol=1e-7), float(np.max(np.abs(gotv - refv)))
