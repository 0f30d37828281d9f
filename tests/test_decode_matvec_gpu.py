"""The single-token plans' mat-vecs at op level: ONE launch of k_mmvq_big (kernels/decode_big.h, Q4_0 .. Q8_0) or k_mmvq_kbig
(kernels/kquant_big.h, K-quants) through ggml_hip_debug_mat_vec_big / _kbig, with every (activation source, epilogue) pair the
plans launch, against the oracle with the operand PINNED: the oracle multiplies the row the kernel quantized (the host row, or
the device's own normed row), so both sides quantize the same f32 row to the same int8 blocks and the only difference left is
the f32 summation order — the mat-vec bound |got - exact| <= 2e-5 * sum|w||x| + 1e-7 of tests/test_ops_gpu.py, on EVERY row.

Where an epilogue rounds to f16 (the SiLU table's input and output, the K / V cache), an exact value within the bound of an f16
rounding midpoint may round either way: such elements may take either neighbour, are counted and printed; all others are exact.
Weights are random bytes with sane f16 scales (every bit pattern of the quants, signs of the scales included); where the
epilogue rounds to f16 (QKV, GATE) they are quantized from values aligned with the row's signs (_aligned_weights), so that the
bound is small against an f16 step and the edges are few."""
import numpy as np
import pytest

import act_quant_ref as R

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes behind every output buffer of the hooks (include/ggml_hip.h)
XQ8, XNORM, XF32 = 0, 1, 2  # k_mmvq_big sources (kernels/decode.h XSRC_*)
ESTORE, EADD, EGATE, EQKV = 0, 1, 2, 3  # ... epilogues (EPI_*)
KNORM, KF32, KSILU = 1, 2, 3  # k_mmvq_kbig sources (kernels/kquant_big.h KX_*)
KROW, KGATE, KQKV = 0, 1, 2  # ... epilogues (KE_*)
Q_TYPES = (2, 3, 6, 7, 8)  # Q4_0 Q4_1 Q5_0 Q5_1 Q8_0
K_TYPES = (10, 11, 12, 13, 14)  # Q2_K Q3_K Q4_K Q5_K Q6_K
EPS = 1e-5
TABLE = 2.0 ** -21  # RoPE: see _check_qkv


def _num_cus(G):
    return int(G.lib().ggml_hip_get_stat(b"num_cus"))


# ---- weights: random quant bytes, f16 scale fields overwritten with sane values (byte offsets in ggml's block structs)
_SCALES = {  # type: [(offset, lo, hi, signed)]
    2: [(0, 4e-3, 2e-2, True)], 3: [(0, 2e-3, 1e-2, False), (2, -0.1, 0.1, False)], 6: [(0, 2e-3, 1e-2, True)],
    7: [(0, 1e-3, 5e-3, False), (2, -0.1, 0.1, False)], 8: [(0, 5e-4, 3e-3, True)],
    10: [(80, 5e-4, 3e-3, False), (82, 0.0, 2e-3, False)], 11: [(108, 2e-4, 1e-3, True)],
    12: [(0, 1e-4, 1e-3, False), (2, 0.0, 1e-3, False)], 13: [(0, 1e-4, 5e-4, False), (2, 0.0, 1e-3, False)],
    14: [(208, 2e-5, 1e-4, True)],
}


def _weights(O, t, M, K, seed):
    rng = np.random.default_rng(seed)
    bs, ts = O.blck_size(t), O.type_size(t)
    n = M * K // bs
    raw = rng.integers(0, 256, (n, ts), dtype=np.uint8)
    for off, lo, hi, signed in _SCALES[t]:
        v = rng.uniform(lo, hi, n).astype(np.float32)
        if signed:
            v[rng.random(n) < 0.5] *= -1.0
        raw[:, off:off + 2] = v.astype(np.float16).view(np.uint8).reshape(n, 2)
    if t == 8:  # Q8_0 quants are -127 .. 127 (ggml never writes -128)
        q = raw[:, 2:]
        q[q == 0x80] = 0x81
    return raw.reshape(-1)


def _aligned_weights(O, t, M, K, signs, seed):
    """Weights whose row r is rs[r] * signs * (0.005 .. 0.015), quantized by the oracle: every dot of a row with x (signs =
    sign(x)) is +-sum|w||x|, so the mat-vec bound is 2e-5 of the value itself — well below an f16 step (2^-11 relative).
    Used where an epilogue rounds to f16: with random weights the bound spans a whole f16 step and nearly every element would
    be an 'edge' that may round either way."""
    rng = np.random.default_rng(seed)
    rs = np.where(rng.random(M) < 0.5, -1.0, 1.0).astype(np.float32)
    W = rng.uniform(0.005, 0.015, (M, K)).astype(np.float32) * rs[:, None] * signs[None, :].astype(np.float32)
    return O.quantize(t, W)


def _dots(O, t, raw, M, K, x):
    """exact = the oracle's mul_mat of the row x (mode ref), and the bound 2e-5 * sum|w||x| + 1e-7 per row (f64)."""
    exact = O.mul_mat(t, raw, M, K, x[None, :].astype(np.float32), mode=O.ref_mode())[0].astype(np.float64)
    rb, ax = O.row_bytes(t, K), np.abs(x.astype(np.float64))
    s = np.empty(M)
    step = max(1, (1 << 23) // K)
    for r0 in range(0, M, step):
        r1 = min(M, r0 + step)
        D = O.dequantize(t, raw[r0 * rb:r1 * rb], (r1 - r0) * K).reshape(r1 - r0, K)
        s[r0:r1] = np.abs(D) @ ax
    return exact, 2e-5 * s + 1e-7


def _buf(n, dtype=np.float32, init=None):
    b = np.full(n * np.dtype(dtype).itemsize + GUARD, 0xFF, np.uint8)
    v = b[:n * np.dtype(dtype).itemsize].view(dtype)
    if init is not None:
        v[:] = init
    return b, v


def _guard_ok(b, n_bytes, what):
    assert np.all(b[n_bytes:] == 0xFF), f"{what}: a store past the end"


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _run(G, O, k_hook, types, Ms, K, xsrc, epi, x, xw=None, res=None, y=False, qkv=None, seed=0, aligned=False):
    """Quantized random weights (aligned: _aligned_weights) -> one launch through the hook.
    Returns (rc, raws, out [sum M or M0], y_out, kcache, vcache)."""
    if aligned:
        raws = [_aligned_weights(O, t, M, K, np.sign(x), [seed, i, t, M, K]) for i, (t, M) in enumerate(zip(types, Ms))]
    else:
        raws = [_weights(O, t, M, K, [seed, i, t, M, K]) for i, (t, M) in enumerate(zip(types, Ms))]
    n_out = Ms[0] if epi in ((KGATE, KQKV) if k_hook else (EGATE, EQKV)) else sum(Ms)
    ob, out = _buf(n_out)
    yb, yv = _buf(K) if y else (None, None)
    kb = vb = None
    n_past, D, C, fb, fs = 0, 0, 0, 10000.0, 1.0
    if qkv is not None:
        n_past, D, C = qkv["n_past"], qkv["D"], qkv["C"]
        pat = np.random.default_rng([seed, 99]).standard_normal((2, C * Ms[1])).astype(np.float16).view(np.uint16)
        kb, _ = _buf(C * Ms[1], np.uint16, pat[0])
        vb, _ = _buf(C * Ms[1], np.uint16, pat[1])
        qkv["pattern"] = pat
    with G.Context(sum(r.nbytes for r in raws) + (1 << 20)) as ctx:
        ws = []
        for i, (t, r, M) in enumerate(zip(types, raws, Ms)):
            w = ctx.tensor_from(r, t, (K, M)).set_name(f"w{i}")
            w.transfer_to_gpu()
            ws.append(w.ptr)
        ws += [None] * (3 - len(ws))
        x = np.ascontiguousarray(x, np.float32)
        xw = None if xw is None else np.ascontiguousarray(xw, np.float32)
        res = None if res is None else np.ascontiguousarray(res, np.float32)
        f = G.lib().ggml_hip_debug_mat_vec_kbig if k_hook else G.lib().ggml_hip_debug_mat_vec_big
        rc = f(ws[0], ws[1], ws[2], xsrc, epi, _ptr(x), _ptr(xw), EPS, _ptr(res), _ptr(ob), _ptr(yb), n_past, D, fb, fs, C,
               _ptr(kb), _ptr(vb))
    if rc == 0:
        assert not np.any(np.isnan(out)), f"{int(np.isnan(out).sum())} of {n_out} outputs never written"
        _guard_ok(ob, n_out * 4, "out")
        if y:
            assert not np.any(np.isnan(yv))
            _guard_ok(yb, K * 4, "y_out")
        if qkv is not None:
            _guard_ok(kb, C * Ms[1] * 2, "mem_k")
            _guard_ok(vb, C * Ms[1] * 2, "mem_v")
    return rc, raws, out, yv, kb, vb


def _ratio(err, bound):
    return float(np.max(err / bound)) if err.size else 0.0


def _check_rows(name, got, exact, bound, res=None):
    want = exact if res is None else res.astype(np.float64) + exact
    # EPI_ADD / res: the device adds in f32 — one more rounding of the sum
    b = bound + (0.0 if res is None else np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    err = np.abs(got.astype(np.float64) - want)
    r = _ratio(err, b)
    print(f"{name}: worst |got - exact| / bound = {r:.3g} over {got.size} rows")
    bad = np.flatnonzero(err > b)
    assert bad.size == 0, f"{name}: {bad.size} rows beyond the bound, first {bad[:8]}, worst ratio {r:.3g}"


def _check_y(name, O, x, w, y):
    """The normed row the kernel staged: the oracle's rms_norm(x) * w.  Both sum x*x in f64 (other orders: the f32 mean can move
    by 1 ulp in a rare tie), then 1 / sqrtf (correctly rounded on both sides) and two f32 products: <= 4 ulp of the result."""
    ref = (O.rms_norm(x[None, :].astype(np.float32), EPS)[0] * w.astype(np.float32)).astype(np.float32)
    err = np.abs(y.astype(np.float64) - ref)
    b = 4.0 * np.spacing(np.abs(ref)).astype(np.float64)
    assert np.all(err <= b), f"{name}: normed row off by {_ratio(err, b):.3g} x 4 ulp"


def _f16_interval(lo, hi):
    """f16 roundings of the ends of [lo, hi] (f64 in, f32 values out): a value in the interval rounds to one of these or between."""
    return lo.astype(np.float16).astype(np.float64), hi.astype(np.float16).astype(np.float64)


def _check_f16(name, got16, ref, tol):
    """got16 (f16 bits) = f16(a value within tol of ref): exactly f16(ref) unless the interval holds an f16 midpoint."""
    g = got16.view(np.float16).astype(np.float64)
    lo, hi = _f16_interval(ref - tol, ref + tol)
    ok = (g >= lo) & (g <= hi)
    edge = int(np.count_nonzero(lo != hi))
    print(f"{name}: {edge} of {ref.size} elements within the bound of an f16 rounding midpoint")
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, f"{name}: {bad.size} f16 elements wrong, first {bad[:8]}: got {g[bad[:4]]} want {ref[bad[:4]]}"


def _silu64(v):
    return v / (1.0 + np.exp(-v))


def _check_gate(name, got, e1, b1, e3, b3):
    """silu_table(w1 x) * (w3 x) (decode_big.h:508, kquant_big.h:425): silu_table rounds its input to f16, computes in f32 with
    the device's expf and rounds to f16 again.  The input may round either way when w1 x lies within its bound of an f16
    midpoint, the output when the f32 SiLU lies within a few ulp of one (device vs host expf): such elements ('edges') may
    take any of the candidate f16 values; all others have ONE SiLU value s and |got - s * exact3| <= |s| * b3 + 2 ulp."""
    xa, xb = _f16_interval(e1 - b1, e1 + b1)
    cands = []
    for xf in (xa, xb):
        s = _silu64(xf)
        cands += [(s * (1 - 1e-6)).astype(np.float16).astype(np.float64), (s * (1 + 1e-6)).astype(np.float16).astype(np.float64)]
    smin, smax = np.minimum.reduce(cands), np.maximum.reduce(cands)
    edge = int(np.count_nonzero(smin != smax))
    lo3, hi3 = e3 - b3, e3 + b3
    prods = [smin * lo3, smin * hi3, smax * lo3, smax * hi3]
    lo, hi = np.minimum.reduce(prods), np.maximum.reduce(prods)
    slack = 2.0 * np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)).astype(np.float64) + 1e-30
    g = got.astype(np.float64)
    ok = (g >= lo - slack) & (g <= hi + slack)
    # worst ratio over the elements with one SiLU value
    one = smin == smax
    err = np.abs(g - smin * e3)[one]
    r = _ratio(err, (np.abs(smin) * b3 + slack)[one])
    print(f"{name}: worst |got - s * exact3| / bound = {r:.3g}; {edge} of {got.size} SiLU edges")
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, f"{name}: {bad.size} gate outputs beyond the bound, first {bad[:8]}"


def _check_qkv(name, O, got_q, kb, vb, raws, types, Ms, K, y, qkv):
    """Q = RoPE(exact wq y) in f32, K row n_past = f16(RoPE(exact wk y)), V column n_past = f16(exact wv y), all else unchanged.
    RoPE bound (decode_big.h:518-520, kquant_big.h:450-452, k_rope_table): r0 = x0 c - x1 s, r1 = x0 s + x1 c with the device's
    cosf / sinf (OCML, <= 2 ulp) where the oracle has glibc's (<= 1 ulp), the same f32 theta (same product chain): |dc|, |ds| <=
    3 * 2^-24; each side rounds two products and a sum (<= 1.5 ulp of |x0| + |x1| each); |c|, |s| <= 1 carry the dots' own
    bounds b0 + b1.  So |got - ref| <= b0 + b1 + (|x0| + |x1|) * 2^-21."""
    n_past, D, C = qkv["n_past"], qkv["D"], qkv["C"]
    E, Eg = Ms[0], Ms[1]
    ex = [_dots(O, t, r, M, K, y) for t, r, M in zip(types, raws, Ms)]

    def rope(e, b, H):
        ref = O.rope(e[0].astype(np.float32).reshape(1, H, D), n_past, D).reshape(-1).astype(np.float64)
        pb = b.reshape(-1, 2).sum(axis=1).repeat(2)
        pa = np.abs(e[0]).reshape(-1, 2).sum(axis=1).repeat(2)
        return ref, pb + pa * TABLE
    qref, qtol = rope(ex[0], ex[0][1], E // D)
    err = np.abs(got_q.astype(np.float64) - qref)
    r = _ratio(err, qtol)
    print(f"{name} Q: worst |got - rope(exact)| / bound = {r:.3g} over {E} rows")
    assert np.all(err <= qtol), f"{name} Q: {int(np.count_nonzero(err > qtol))} elements beyond the bound, worst {r:.3g}"
    kref, ktol = rope(ex[1], ex[1][1], Eg // D)
    mk = kb[:C * Eg * 2].view(np.uint16).reshape(C, Eg)
    mv = vb[:C * Eg * 2].view(np.uint16).reshape(Eg, C)
    pk, pv = qkv["pattern"][0].reshape(C, Eg), qkv["pattern"][1].reshape(Eg, C)
    _check_f16(f"{name} K row {n_past}", mk[n_past].copy(), kref, ktol)
    _check_f16(f"{name} V column {n_past}", np.ascontiguousarray(mv[:, n_past]), ex[2][0], ex[2][1])
    others = np.ones(C, bool)
    others[n_past] = False
    assert np.array_equal(mk[others], pk[others]), f"{name}: K cache rows other than {n_past} changed"
    assert np.array_equal(mv[:, others], pv[:, others]), f"{name}: V cache columns other than {n_past} changed"


def _silu_safe(rng, K):
    """w1 x values whose f16-table SiLU rounds the same way with any expf within a few ulp (the device's and the host's): f16
    inputs whose SiLU is not within 1e-6 of an f16 rounding midpoint — so the oracle can restate KX_SILU_MUL's staged row."""
    g = (3.0 * rng.standard_normal(K)).astype(np.float16).astype(np.float64)
    while True:
        s = _silu64(g)
        bad = (s * (1 - 1e-6)).astype(np.float16) != (s * (1 + 1e-6)).astype(np.float16)
        if not bad.any():
            return g.astype(np.float32)
        g[bad] = (3.0 * rng.standard_normal(int(bad.sum()))).astype(np.float16)


def _x(rng, K):
    x = rng.standard_normal(K).astype(np.float32)
    x[::7] *= 4.0
    return x


# ---- k_mmvq_big: (source, epilogue) pairs of plan_launch_all
# name: (pair, K, M or (E, Egqa) for QKV, extra)
BIG = {
    "7b_qkv": ("qkv", 4096, (4096, 4096), dict(D=128, n_past=5, C=16)),
    "7b_wo": ("wo", 4096, 4096, None),
    "7b_gate": ("gate", 4096, 11008, None),
    "7b_w2": ("w2", 11008, 4096, None),
    "7b_lm_head": ("lm", 4096, 32000, None),
    "13b_qkv": ("qkv", 5120, (5120, 5120), dict(D=128, n_past=0, C=8)),
    "13b_gate": ("gate", 5120, 13824, None),
    "13b_w2": ("w2", 13824, 5120, None),
    "65b_gate_norm8192": ("gate", 8192, 22016, None),  # the norm's staging limit: E = 8192
    "65b_w2": ("w2", 22016, 8192, None),
    "gqa_qkv_p0": ("qkv", 1024, (1024, 256), dict(D=128, n_past=0, C=40)),  # n_head_kv = n_head / 4
    "gqa_qkv_p17": ("qkv", 1024, (1024, 256), dict(D=128, n_past=17, C=40)),
    "gqa_qkv_last": ("qkv", 1024, (1024, 256), dict(D=128, n_past=39, C=40)),
    "odd_nb3_w2": ("w2", 96, 128, None),  # nb = 3, M % 128 == 0: the scale word of the last row's last block reads past the plane
    "odd_nb3_lm": ("lm", 96, 1000, None),
    "odd_nb11_gate": ("gate", 352, 1000, None),
    "odd_nb11_wo": ("wo", 352, 7, None),
    "odd_nb11_qkv": ("qkv", 352, (256, 64), dict(D=64, n_past=3, C=8)),
    "nb64_wo": ("wo", 2048, 4100, None),  # nb exactly 64
    "nb65_w2": ("w2", 2080, 4100, None),  # nb = 64 + 1: a second step of one block
    "nb65_lm": ("lm", 2080, 333, None),
    "m1_wo": ("wo", 4096, 1, None),  # M below one wave per workgroup
    "m7_lm": ("lm", 4096, 7, None),
    "m64_gate": ("gate", 4096, 64, None),
    "uneven_lm": ("lm", 1024, 8229, None),  # 8229 rows over 256 x W waves: a partial last round
    "q8src_nb1024": ("wo", 32768, 300, None),  # the Q8 source's staging limit: one thread per block, 1024 threads
    "f32src_nb768": ("w2", 24576, 300, None),  # the f32 source's: 24 elements per thread
}
_PAIRS = {"qkv": (XNORM, EQKV), "wo": (XQ8, EADD), "gate": (XNORM, EGATE), "w2": (XF32, EADD), "lm": (XNORM, ESTORE)}


def _case_big(G, O, wtype, name, pair, K, M, extra, seed):
    rng = np.random.default_rng(seed)
    xsrc, epi = _PAIRS[pair]
    x = _x(rng, K)
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32) if xsrc == XNORM else None
    tag = f"{name} type {wtype}"
    if pair == "qkv":
        E, Eg = M
        Ms = [E, Eg, Eg]
        q = dict(extra)
        rc, raws, out, y, kb, vb = _run(G, O, False, [wtype] * 3, Ms, K, xsrc, epi, x, nw, y=True, qkv=q, seed=seed, aligned=True)
        assert rc == 0
        _check_y(tag, O, x, nw, y)
        _check_qkv(tag, O, out, kb, vb, raws, [wtype] * 3, Ms, K, y, q)
        return
    Ms = [M, M] if pair == "gate" else [M]
    res = rng.standard_normal(M).astype(np.float32) if epi == EADD else None
    rc, raws, out, y, _, _ = _run(G, O, False, [wtype] * len(Ms), Ms, K, xsrc, epi, x, nw, res=res, y=xsrc == XNORM, seed=seed,
                                  aligned=pair == "gate")
    assert rc == 0
    op = x
    if xsrc == XNORM:
        _check_y(tag, O, x, nw, y)
        op = y  # pinned: the oracle multiplies the device's own normed row
    if pair == "gate":
        e1, b1 = _dots(O, wtype, raws[0], M, K, op)
        e3, b3 = _dots(O, wtype, raws[1], M, K, op)
        _check_gate(tag, out, e1, b1, e3, b3)
    else:
        e, b = _dots(O, wtype, raws[0], M, K, op)
        _check_rows(tag, out, e, b, res)


@pytest.mark.parametrize("wtype", Q_TYPES)
@pytest.mark.parametrize("name", list(BIG))
def test_big_matvec_matches_the_oracle(G, O, wtype, name):
    pair, K, M, extra = BIG[name]
    _case_big(G, O, wtype, name, pair, K, M, extra, seed=[wtype, K, len(name)])


@pytest.mark.parametrize("wtype", Q_TYPES)
def test_big_matvec_at_the_largest_dealing_and_one_row_more(G, O, wtype):
    """64 units per wave over G x 16 waves is launch_big's limit (one epilogue lane per unit): the largest matrix it takes, every
    row checked, and one row more is refused (-1, not launch_big's abort)."""
    M = 64 * 16 * _num_cus(G)
    _case_big(G, O, wtype, "largest_dealing", "wo", 32, M, None, seed=[wtype, 1])
    rc = _run(G, O, False, [wtype], [M + 1], 32, XQ8, EADD, np.ones(32, np.float32), res=np.zeros(M + 1, np.float32))[0]
    assert rc == -1


@pytest.mark.parametrize("wtype", [2, 8])
def test_big_hook_refuses_what_the_plan_cannot_stage(G, O, wtype):
    x = lambda K: np.ones(K, np.float32)  # noqa: E731
    assert _run(G, O, False, [wtype], [64], 32768 + 32, XQ8, EADD, x(32800), res=np.zeros(64, np.float32))[0] == -1  # nb 1025
    assert _run(G, O, False, [wtype], [64], 24576 + 32, XF32, EADD, x(24608), res=np.zeros(64, np.float32))[0] == -1
    assert _run(G, O, False, [wtype], [64], 8192 + 32, XNORM, ESTORE, x(8224), x(8224))[0] == -1  # the norm: 8192 at most
    assert _run(G, O, False, [wtype], [64], 256, XF32, ESTORE, x(256))[0] == -1  # a pair no plan launches


# ---- k_mmvq_kbig: (source, epilogue) pairs of plan_launch_k
KBIG = {
    "7b_qkv": ("qkv", 4096, (4096, 4096), dict(D=128, n_past=3, C=8)),
    "7b_qkv_rows": ("rows3", 4096, (4096, 4096, 4096), None),  # wq|wk|wv as plain rows (the plan's form without the RoPE epilogue)
    "7b_wo": ("wo", 4096, 4096, None),
    "7b_gate": ("gate", 4096, 11008, None),
    "7b_w2_nsb43": ("w2", 11008, 4096, None),  # nsb = 43; Q6_K: the d plane was a multiple of 256 bytes
    "7b_w2_silu": ("w2silu", 11008, 4096, None),
    "7b_w13_rows": ("rows2", 4096, (11008, 11008), None),  # a mixed w1|w3 pair's row launches
    "7b_lm_head": ("lm", 4096, 32000, None),
    "13b_gate": ("gate", 5120, 13824, None),
    "13b_w2_nsb54": ("w2", 13824, 5120, None),
    "65b_gate_norm8192": ("gate", 8192, 22016, None),  # the norm's staging limit: nsb 32
    "gqa_qkv_p0": ("qkv", 1024, (1024, 256), dict(D=128, n_past=0, C=40)),
    "gqa_qkv_p17": ("qkv", 1024, (1024, 256), dict(D=128, n_past=17, C=40)),
    "gqa_qkv_last": ("qkv", 1024, (1024, 256), dict(D=128, n_past=39, C=40)),
    "odd_nsb3_w2": ("w2", 768, 128, None),  # nsb 3, M % 128 == 0
    "odd_nsb3_gate": ("gate", 768, 1000, None),
    "odd_nsb3_qkv": ("qkv", 768, (256, 64), dict(D=64, n_past=5, C=8)),
    "nsb5_lm": ("lm", 1280, 777, None),
    "nsb64_w2": ("w2", 16384, 300, None),  # the f32 source's staging limit: 4 super-blocks per wave
    "m1_wo": ("wo", 4096, 1, None),
    "m7_lm": ("lm", 4096, 7, None),
    "m64_gate": ("gate", 4096, 64, None),
    "uneven_lm": ("lm", 1024, 8229, None),
}


def _case_kbig(G, O, kt, name, pair, K, M, extra, seed):
    rng = np.random.default_rng(seed)
    x = _x(rng, K)
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
    tag = f"{name} type {kt}"
    if pair == "qkv":
        E, Eg = M
        Ms = [E, Eg, Eg]
        q = dict(extra)
        rc, raws, out, y, kb, vb = _run(G, O, True, [kt] * 3, Ms, K, KNORM, KQKV, x, nw, y=True, qkv=q, seed=seed, aligned=True)
        assert rc == 0
        _check_y(tag, O, x, nw, y)
        _check_qkv(tag, O, out, kb, vb, raws, [kt] * 3, Ms, K, y, q)
        return
    if pair == "gate":
        rc, raws, out, y, _, _ = _run(G, O, True, [kt] * 2, [M, M], K, KNORM, KGATE, x, nw, y=True, seed=seed, aligned=True)
        assert rc == 0
        _check_y(tag, O, x, nw, y)
        e1, b1 = _dots(O, kt, raws[0], M, K, y)
        e3, b3 = _dots(O, kt, raws[1], M, K, y)
        _check_gate(tag, out, e1, b1, e3, b3)
        return
    if pair in ("rows3", "rows2", "lm"):
        Ms = list(M) if isinstance(M, tuple) else [M]
        rc, raws, out, y, _, _ = _run(G, O, True, [kt] * len(Ms), Ms, K, KNORM, KROW, x, nw, y=True, seed=seed)
        assert rc == 0
        _check_y(tag, O, x, nw, y)
        at = 0
        for i, (r, m) in enumerate(zip(raws, Ms)):
            e, b = _dots(O, kt, r, m, K, y)
            _check_rows(f"{tag} matrix {i}", out[at:at + m], e, b)
            at += m
        return
    res = rng.standard_normal(M).astype(np.float32)
    if pair == "w2silu":  # KX_SILU_MUL: the row is silu_table(w1 x) * (w3 x), made in the staging from the two f32 rows
        g1 = _silu_safe(rng, K)
        rc, raws, out, _, _, _ = _run(G, O, True, [kt], [M], K, KSILU, KROW, g1, x, res=res, seed=seed)
        assert rc == 0
        op = (O.silu(g1) * x).astype(np.float32)  # f16-table SiLU in f32 arithmetic, as the oracle's FFN computes it
    else:
        rc, raws, out, _, _, _ = _run(G, O, True, [kt], [M], K, KF32, KROW, x, res=res, seed=seed)
        assert rc == 0
        op = x
    e, b = _dots(O, kt, raws[0], M, K, op)
    _check_rows(tag, out, e, b, res)


@pytest.mark.parametrize("kt", K_TYPES)
@pytest.mark.parametrize("name", list(KBIG))
def test_kbig_matvec_matches_the_oracle(G, O, kt, name):
    pair, K, M, extra = KBIG[name]
    _case_kbig(G, O, kt, name, pair, K, M, extra, seed=[kt, K, len(name)])


@pytest.mark.parametrize("kt", K_TYPES)
def test_kbig_matvec_at_the_largest_dealing_and_one_row_more(G, O, kt):
    """kbig_ok takes a matrix of up to 21 rows per wave of G x 16 (three matrices in one launch: 63 of a wave's 64 epilogue
    lanes): the largest, every row checked; one row more is refused."""
    M = 21 * 16 * _num_cus(G)
    _case_kbig(G, O, kt, "largest_dealing", "wo", 256, M, None, seed=[kt, 1])
    rc = _run(G, O, True, [kt], [M + 1], 256, KF32, KROW, np.ones(256, np.float32))[0]
    assert rc == -1


@pytest.mark.parametrize("kt", [12, 14])
def test_kbig_hook_refuses_what_the_plan_cannot_stage(G, O, kt):
    one = lambda K: np.ones(K, np.float32)  # noqa: E731
    assert _run(G, O, True, [kt], [64], 16384 + 256, KF32, KROW, one(16640))[0] == -1  # nsb 65
    assert _run(G, O, True, [kt], [64], 22016, KF32, KROW, one(22016))[0] == -1  # 65B w2: the K plan's helper-launch form
    assert _run(G, O, True, [kt], [64], 8192 + 256, KNORM, KROW, one(8448), one(8448))[0] == -1  # the norm: 8192 at most


# ---- the quantizers inside the launches: selector weights make every output row reveal one quant (or one pair of bsums) exactly.
# The bound above lets one flipped quant pass from K of about 1200 on; here the weights are one-hot, the oracle's product on the
# same selector is the expected value and the comparison is ==, on rounding ties, two-signed extremes and the clamp
# (tests/act_quant_ref.py), under both branches of the Q8 quantizer for k_mmvq_big.
def _selector_q8_0(K):
    """Q8_0 [K][K]: row m has d = 1 everywhere and q = 1 at column m only: out[m] = q_x[m] * d_x."""
    nb = K // 32
    raw = np.zeros((K, nb, 34), np.uint8)
    raw[:, :, :2] = np.array([1.0], np.float16).view(np.uint8)
    m = np.arange(K)
    raw[m, m // 32, 2 + m % 32] = 1
    return raw.reshape(-1)


def _selector_q6_k(K):
    """Q6_K [K][K]: row m has d = 1, scale 1 for the 16 columns around m only, code 33 at column m and 32 elsewhere: the weight is
    1 at column m, 0 elsewhere, and out[m] = q8[m] * d8."""
    nsb = K // 256
    raw = np.zeros((K, nsb, 210), np.uint8)
    raw[:, :, 128:192] = 0xAA  # qh: the two high bits of every code = 2 (code 32)
    raw[:, :, 208:210] = np.array([1.0], np.float16).view(np.uint8)
    for m in range(K):
        sb, c = divmod(m, 256)
        n, r = divmod(c, 128)
        quarter, l = divmod(r, 32)
        raw[m, sb, 64 * n + l + (32 if quarter & 1 else 0)] = 1 if quarter < 2 else 0x10  # the low four bits of the code at column m
        raw[m, sb, 192 + c // 16] = 1
    return raw.reshape(-1)


def _selector_q4_k(K):
    """Q4_K [K / 32][K]: d = 0, dmin = 1, row m has min 1 for sub-block m (32 columns) only: the weight is -1 there, 0 elsewhere, and
    out[m] = -d8 * (bsums[2 j] + bsums[2 j + 1]) of that sub-block."""
    nsb = K // 256
    M = K // 32
    raw = np.zeros((M, nsb, 144), np.uint8)
    raw[:, :, 2:4] = np.array([1.0], np.float16).view(np.uint8)
    for m in range(M):
        sb, j = divmod(m, 8)
        raw[m, sb, 4 + j + 4] = 1 if j < 4 else 0x10  # get_scale_min_k4: the six-bit min of sub-block j
    return raw.reshape(-1)


def _selector_launch(G, k_hook, wptr, xsrc, epi, K, M, x, xw=None, res=None, y=False):
    ob, out = _buf(M)
    yb, yv = _buf(K) if y else (None, None)
    x = np.ascontiguousarray(x, np.float32)
    xw = None if xw is None else np.ascontiguousarray(xw, np.float32)
    res = None if res is None else np.ascontiguousarray(res, np.float32)
    f = G.lib().ggml_hip_debug_mat_vec_kbig if k_hook else G.lib().ggml_hip_debug_mat_vec_big
    rc = f(wptr, None, None, xsrc, epi, _ptr(x), _ptr(xw), EPS, _ptr(res), _ptr(ob), _ptr(yb), 0, 0, 10000.0, 1.0, 0, None, None)
    assert rc == 0
    assert not np.any(np.isnan(out))
    _guard_ok(ob, M * 4, "out")
    if y:
        assert not np.any(np.isnan(yv))
        _guard_ok(yb, K * 4, "y_out")
    return out.copy(), None if yv is None else yv.copy()


def _rows_of(pool, fam, names, per):
    """The blocks of the named families, as rows of `per` blocks (the last one filled up from the start)."""
    sel = pool[np.isin(np.array(fam), names)]
    return list(R.launches(sel, 1, per))


def _norm_rows3(K, seed):
    return R.norm_rows_input(3, K, seed), np.random.default_rng([seed, K]).uniform(0.5, 1.5, K).astype(np.float32)


def test_selector_weights_are_one_hot(O):
    for K in (32, 288):
        assert np.array_equal(O.dequantize(8, _selector_q8_0(K), K * K).reshape(K, K), np.eye(K, dtype=np.float32))
    assert np.array_equal(O.dequantize(14, _selector_q6_k(768), 768 * 768).reshape(768, 768), np.eye(768, dtype=np.float32))
    w = O.dequantize(12, _selector_q4_k(768), 24 * 768).reshape(24, 768)
    assert np.array_equal(w, -np.repeat(np.eye(24, dtype=np.float32), 32, axis=1))


@pytest.mark.parametrize("K", [32, 288])
def test_big_matvec_staging_quantizer_reveals_every_quant(G, O, K):
    """k_mmvq_big's staging quantizer (XSRC_F32 + EPI_ADD with res = 0) through a Q8_0 selector: K = 32 is the smallest the hook
    takes, 288 puts nine blocks in a row (which block meets which weight).  Every family of the Q8 set, act_quant 0 and 1: each
    result == the oracle's product of its branch, and the two differ exactly where the oracle's do."""
    pool, fam = R.q8_pool()
    rows = list(R.launches(pool, 1, K // 32)) if K > 32 else _rows_of(pool, fam, ("tie", "edge", "zero", "negzero", "single", "d_tie"), 1)
    raw = _selector_q8_0(K)
    zero = np.zeros(K, np.float32)
    got, want = {}, {}
    with G.Context(raw.nbytes + (1 << 20)) as ctx:
        w = ctx.tensor_from(raw, 8, (K, K)).set_name("selector")
        w.transfer_to_gpu()
        try:
            for aq in (0, 1):
                G.set_option("act_quant", aq)
                got[aq] = [_selector_launch(G, False, w.ptr, XF32, EADD, K, K, x[0], res=zero)[0] for x in rows]
                want[aq] = [O.mul_mat(8, raw, K, K, x, mode=O.ref_mode() if aq == 0 else O.MODE_SCALAR)[0] for x in rows]
        finally:
            G.set_option("act_quant", 0)
    ndiff = 0
    for aq in (0, 1):
        for i, (g, e) in enumerate(zip(got[aq], want[aq])):
            bad = np.flatnonzero(g != e)
            assert bad.size == 0, f"K {K} act_quant {aq} row {i}: {bad.size} outputs differ, first {bad[:8]}: got {g[bad[:4]]} want {e[bad[:4]]}"
    for g0, g1, e0, e1 in zip(got[0], got[1], want[0], want[1]):
        assert np.array_equal(g0 != g1, e0 != e1)
        ndiff += int(np.count_nonzero(g0 != g1))
    print(f"K {K}: {len(rows)} rows, the branches differ on {ndiff} outputs")
    assert ndiff > 0
    if K > 32:  # the whole set once: the count of tests/test_act_quant_ref.py
        assert ndiff == R.branch_diff_count(pool)


def test_big_matvec_norm_staging_reveals_every_quant(G, O):
    """XSRC_NORM (+ EPI_STORE): ties cannot be placed behind the launch's own norm; the revealed quants are compared exactly with
    the oracle's quantization of the tapped y_out, on rows of three magnitudes, act_quant 0 and 1."""
    K = 288
    raw = _selector_q8_0(K)
    xs, nw = _norm_rows3(K, 21)
    with G.Context(raw.nbytes + (1 << 20)) as ctx:
        w = ctx.tensor_from(raw, 8, (K, K)).set_name("selector")
        w.transfer_to_gpu()
        try:
            for aq in (0, 1):
                G.set_option("act_quant", aq)
                for i, x in enumerate(xs):
                    out, y = _selector_launch(G, False, w.ptr, XNORM, ESTORE, K, K, x, xw=nw, y=True)
                    assert np.array_equal(y.view(np.uint32), R.norm_rows(x[None], nw, EPS)[0].view(np.uint32)), f"row {i}: the normed row"
                    e = O.mul_mat(8, raw, K, K, y[None], mode=O.ref_mode() if aq == 0 else O.MODE_SCALAR)[0]
                    q, d, _ = R.q8(y, aq, True)
                    assert np.array_equal(e, (q.astype(np.float32) * d[:, None]).reshape(-1))
                    bad = np.flatnonzero(out != e)
                    assert bad.size == 0, f"act_quant {aq} row {i}: {bad.size} outputs differ, first {bad[:8]}"
        finally:
            G.set_option("act_quant", 0)


def test_kbig_matvec_staging_quantizer_reveals_quants_and_bsums(G, O):
    """k_mmvq_kbig's staging quantizer (KX_F32 + KE_ROW) through a Q6_K selector (q8 * d8 of every column) and a Q4_K matrix of
    one-hot mins (every pair of bsums), on the whole Q8_K set: ties, +max and -max at every reduction boundary, the clamp."""
    K = 768
    pool, _ = R.q8k_pool()
    rows = list(R.launches(pool, 1, K // 256))
    for t, raw, M in ((14, _selector_q6_k(K), K), (12, _selector_q4_k(K), K // 32)):
        with G.Context(raw.nbytes + (1 << 20)) as ctx:
            w = ctx.tensor_from(raw, t, (K, M)).set_name("selector")
            w.transfer_to_gpu()
            for i, x in enumerate(rows):
                out, _ = _selector_launch(G, True, w.ptr, KF32, KROW, K, M, x[0])
                e = O.mul_mat(t, raw, M, K, x, mode=O.ref_mode())[0]
                q, d, bs = R.q8k(x)
                mine = (d[:, None] * q.astype(np.float32)).reshape(-1) if t == 14 else \
                    -(d[:, None] * bs.astype(np.int32).reshape(-1, 8, 2).sum(axis=2).astype(np.float32)).reshape(-1)
                assert np.array_equal(e, mine.astype(np.float32)), f"type {t} row {i}: the oracle's product is not the revealed quantity"
                bad = np.flatnonzero(out != e)
                assert bad.size == 0, f"type {t} row {i}: {bad.size} outputs differ, first {bad[:8]}: got {out[bad[:4]]} want {e[bad[:4]]}"


def test_kbig_matvec_norm_staging_reveals_quants_and_bsums(G, O):
    """KX_NORM (+ KE_ROW): the revealed quants and bsums against the oracle's quantization of the tapped y_out, three magnitudes."""
    K = 768
    xs, nw = _norm_rows3(K, 22)
    for t, raw, M in ((14, _selector_q6_k(K), K), (12, _selector_q4_k(K), K // 32)):
        with G.Context(raw.nbytes + (1 << 20)) as ctx:
            w = ctx.tensor_from(raw, t, (K, M)).set_name("selector")
            w.transfer_to_gpu()
            for i, x in enumerate(xs):
                out, y = _selector_launch(G, True, w.ptr, KNORM, KROW, K, M, x, xw=nw, y=True)
                assert np.array_equal(y.view(np.uint32), R.norm_rows(x[None], nw, EPS)[0].view(np.uint32)), f"row {i}: the normed row"
                e = O.mul_mat(t, raw, M, K, y[None], mode=O.ref_mode())[0]
                bad = np.flatnonzero(out != e)
                assert bad.size == 0, f"type {t} row {i}: {bad.size} outputs differ, first {bad[:8]}: got {out[bad[:4]]} want {e[bad[:4]]}"
