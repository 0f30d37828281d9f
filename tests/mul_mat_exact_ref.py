"""Inputs and references that hold the quantized mul_mat kernels to exact values (tests/test_mul_mat_exact_gpu.py; the helpers
themselves are held to the oracle in tests/test_mul_mat_exact_ref.py).  Plain NumPy, no GPU.

Raw blocks.  pack_block / unpack_block (Q4_0 .. Q8_0) and pack_q2_k .. pack_q6_k build ggml's block structs from their parts:
scale fields as f16, sub-block scales and mins as integers, codes as integers, in ggml's element order.

A. Exact integers.  exact_w_block / exact_w_k and exact_x_block / exact_x_k give weights and activations for which every
quantity a format stores is an integer: all block scales are 1, the activation quantizers reproduce the integers (one +-127 in
every block of 32: d = 127 / 127 = 1 in both branches; -128 as the only value of largest magnitude in every 256: Q8_K iscale = 1).
exact_product checks that every |x| . |w| row sum stays below 2^24 and that both operands are f16 values: then every product and
every partial sum of every kernel is an exact f32 integer and the result does not depend on the summation order.

B. One-hot reveal.  With K tokens of K elements, token k holding one value at position k whose activation operand is known exactly
(127 for the block formats, 1 for Q8_K), out[k][m] = f32(x16 * w16[m][k]): one GEMM reads out the weight operand.  w16_block is its
reference for the block formats — d (code - zero) or d code + m in exact integer arithmetic (multiples of 2^-24), rounded ONCE to
f16, nearest even: what one f16 multiply or fma gives — and reveal_blocks / reveal_k_blocks pack blocks whose scales have full
11-bit significands (products land on exact ties, f16_ties counts them), either sign, zero and subnormal values.

C. Derived bound.  With x16 (act_quant_ref, element order undone) and w16 known exactly, only the f32 accumulation is left:
|got - x16 . w16| <= 2 K 2^-24 (|x16| . |w16|) (operand_product).  The mutants of test_mul_mat_exact_ref.py show what it catches."""
import numpy as np

import act_quant_ref as R

F = np.float32
Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 = 2, 3, 6, 7, 8
Q2_K, Q3_K, Q4_K, Q5_K, Q6_K = 10, 11, 12, 13, 14
BLOCK_TYPES = (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0)
K_TYPES = (Q2_K, Q3_K, Q4_K, Q5_K, Q6_K)
BLOCK_BYTES = {Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24, Q8_0: 34, Q2_K: 84, Q3_K: 110, Q4_K: 144, Q5_K: 176, Q6_K: 210}
ZERO = {Q4_0: 8, Q4_1: 0, Q5_0: 16, Q5_1: 0, Q8_0: 0}  # what the format subtracts from a code
CODES = {Q4_0: (0, 15), Q4_1: (0, 15), Q5_0: (0, 31), Q5_1: (0, 31), Q8_0: (-128, 127)}  # the codes a block can hold
HAS_M = (Q4_1, Q5_1)
F16D = (Q4_0, Q5_0, Q8_0)  # formats whose vec_dot_type is Q8_0 (d stored as f16); the others take Q8_1
W16_MAX = 65504.0 / 127.0  # part B keeps |w16| below this: 127 * w16 stays an f16-range value, as in every model file


def _h(v):
    """f16 values -> their two bytes each, [n][2]."""
    return np.ascontiguousarray(v, np.float16).view(np.uint8).reshape(-1, 2)


def row_bytes(t, K):
    return K // (32 if t in BLOCK_TYPES else 256) * BLOCK_BYTES[t]


# ---- Q4_0 .. Q8_0 ------------------------------------------------------------------------------------------------------------
def pack_block(t, d, codes, m=None):
    """d, m f16 [n], codes int [n][32] (unsigned, Q8_0: -128 .. 127) -> raw bytes.  Element j of a block: low nibble of qs[j] for
    j < 16, high nibble of qs[j - 16] else; the fifth bit is bit j of qh."""
    codes = np.asarray(codes, np.int64).reshape(-1, 32)
    n = codes.shape[0]
    lo, hi = CODES[t]
    assert codes.min() >= lo and codes.max() <= hi
    out = np.zeros((n, BLOCK_BYTES[t]), np.uint8)
    out[:, 0:2] = _h(d)
    at = 2
    if t in HAS_M:
        out[:, 2:4] = _h(m)
        at = 4
    if t == Q8_0:
        out[:, at:] = codes.astype(np.int8).view(np.uint8)
        return out.reshape(-1)
    if t in (Q5_0, Q5_1):
        bits = ((codes >> 4) & 1).astype(np.uint64)
        qh = (bits << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)
        out[:, at:at + 4] = qh.view(np.uint8).reshape(n, 4)
        at += 4
    out[:, at:] = ((codes[:, :16] & 15) | ((codes[:, 16:] & 15) << 4)).astype(np.uint8)
    return out.reshape(-1)


def unpack_block(t, raw):
    """raw bytes -> (d f16 [n], m f16 [n] or None, codes int64 [n][32])."""
    b = np.ascontiguousarray(raw, np.uint8).reshape(-1, BLOCK_BYTES[t])
    n = b.shape[0]
    d = b[:, 0:2].copy().view(np.float16).reshape(n)
    m, at = None, 2
    if t in HAS_M:
        m = b[:, 2:4].copy().view(np.float16).reshape(n)
        at = 4
    if t == Q8_0:
        return d, m, b[:, at:].copy().view(np.int8).astype(np.int64)
    high = np.zeros((n, 32), np.int64)
    if t in (Q5_0, Q5_1):
        qh = b[:, at:at + 4].copy().view(np.uint32).reshape(n).astype(np.int64)
        high = ((qh[:, None] >> np.arange(32)[None, :]) & 1) << 4
        at += 4
    qs = b[:, at:].astype(np.int64)
    return d, m, np.concatenate([qs & 15, qs >> 4], axis=1) | high


def _f16_units(v):
    """f16 -> the integer n with v = n 2^-24 (every finite f16 is such a multiple)."""
    v = np.asarray(v, np.float16).astype(np.float64)
    assert np.all(np.isfinite(v))
    return np.round(v * 2.0 ** 24).astype(np.int64)


def exact_block(t, raw):
    """The value of every weight, d (code - zero) [+ m], as float64 without any rounding: [n][32].  In units of 2^-24 it is an
    integer below 2^47, so the int64 arithmetic and the conversion are exact."""
    d, m, codes = unpack_block(t, raw)
    v = _f16_units(d)[:, None] * (codes - ZERO[t])
    if m is not None:
        v = v + _f16_units(m)[:, None]
    assert np.abs(v).max(initial=0) < 2 ** 52
    return v.astype(np.float64) * 2.0 ** -24


def round_f16(v, trunc=False):
    """float64 -> f16 with one rounding, nearest even; trunc: toward zero (the mutant of part C)."""
    v = np.asarray(v, np.float64)
    h = v.astype(np.float16)
    if trunc:
        over = np.abs(h.astype(np.float64)) > np.abs(v)
        h = np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)
    return h


def w16_block(t, raw, K, trunc=False):
    """The f16 weight operand of the GEMMs for a Q4_0 .. Q8_0 weight, [M][K] in ggml's element order: the exact value rounded
    once.  (For Q4_1 / Q5_1 this is not f16(dequantize): there the f32 sum d * code + m rounds first.)"""
    return round_f16(exact_block(t, raw), trunc).reshape(-1, K)


def f16_ties(v):
    """Mask of the float64 values that lie exactly half way between two neighbouring f16 values."""
    v = np.asarray(v, np.float64)
    h = v.astype(np.float16)
    h64 = h.astype(np.float64)
    toward = np.where(v > h64, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16)
    other = np.nextafter(h, toward).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (h64 != v) & np.isfinite(other) & (np.abs(v - h64) == np.abs(other - v))


# ---- K-quants ----------------------------------------------------------------------------------------------------------------
def _pack_k4(sc, mn):
    """Eight six-bit (scale, min) pairs in 12 bytes (ggml's get_scale_min_k4): pairs 4 .. 7 keep their high two bits in the top
    of bytes 0 .. 7."""
    sc, mn = np.asarray(sc, np.int64).reshape(-1, 8), np.asarray(mn, np.int64).reshape(-1, 8)
    assert sc.min() >= 0 and sc.max() <= 63 and mn.min() >= 0 and mn.max() <= 63
    q = np.zeros((sc.shape[0], 12), np.int64)
    q[:, 0:4] = sc[:, :4] | ((sc[:, 4:] >> 4) << 6)
    q[:, 4:8] = mn[:, :4] | ((mn[:, 4:] >> 4) << 6)
    q[:, 8:12] = (sc[:, 4:] & 15) | ((mn[:, 4:] & 15) << 4)
    return q.astype(np.uint8)


def _pack_2bit(q):
    """[n][256] values 0 .. 3 -> 64 bytes: element 128 a + 32 j + l in bits 2 j of byte 32 a + l (Q2_K, Q3_K)."""
    g = q.reshape(-1, 2, 4, 32)
    return (g[:, :, 0] | (g[:, :, 1] << 2) | (g[:, :, 2] << 4) | (g[:, :, 3] << 6)).reshape(-1, 64).astype(np.uint8)


def pack_q2_k(d, dmin, sc, mn, q):
    """d, dmin f16 [n]; sc, mn [n][16] in 0 .. 15; q [n][256] in 0 .. 3: w = d sc q - dmin mn per sub-block of 16."""
    sc, mn, q = (np.asarray(v, np.int64) for v in (sc, mn, q))
    assert min(sc.min(), mn.min(), q.min()) >= 0 and max(sc.max(), mn.max()) <= 15 and q.max() <= 3
    n = q.shape[0]
    out = np.zeros((n, 84), np.uint8)
    out[:, 0:16] = (sc | (mn << 4)).astype(np.uint8)
    out[:, 16:80] = _pack_2bit(q)
    out[:, 80:82], out[:, 82:84] = _h(d), _h(dmin)
    return out.reshape(-1)


def pack_q3_k(d, sc, q):
    """d f16 [n]; sc [n][16] in -32 .. 31; q [n][256] in -4 .. 3: w = d sc q per sub-block of 16.  The third bit of a code is bit
    e / 32 of hmask[e % 32]; the six-bit scales (sc + 32) keep their high two bits in bytes 8 .. 11."""
    sc, q = np.asarray(sc, np.int64), np.asarray(q, np.int64)
    assert sc.min() >= -32 and sc.max() <= 31 and q.min() >= -4 and q.max() <= 3
    n = q.shape[0]
    out = np.zeros((n, 110), np.uint8)
    L = q + 4
    hm = ((L >> 2).reshape(n, 8, 32) << np.arange(8)[None, :, None]).sum(axis=1)
    out[:, 0:32] = hm.astype(np.uint8)
    out[:, 32:96] = _pack_2bit(L & 3)
    l6 = sc + 32
    s = np.zeros((n, 12), np.int64)
    s[:, 0:8] = (l6[:, :8] & 15) | ((l6[:, 8:] & 15) << 4)
    for j in range(16):
        s[:, 8 + j % 4] |= (l6[:, j] >> 4) << (2 * (j // 4))
    out[:, 96:108] = s.astype(np.uint8)
    out[:, 108:110] = _h(d)
    return out.reshape(-1)


def pack_q4_k(d, dmin, sc, mn, q):
    """d, dmin f16 [n]; sc, mn [n][8] in 0 .. 63; q [n][256] in 0 .. 15: w = d sc q - dmin mn per sub-block of 32."""
    q = np.asarray(q, np.int64)
    assert q.min() >= 0 and q.max() <= 15
    n = q.shape[0]
    out = np.zeros((n, 144), np.uint8)
    out[:, 0:2], out[:, 2:4] = _h(d), _h(dmin)
    out[:, 4:16] = _pack_k4(sc, mn)
    g = q.reshape(n, 4, 2, 32)
    out[:, 16:144] = (g[:, :, 0] | (g[:, :, 1] << 4)).reshape(n, 128).astype(np.uint8)
    return out.reshape(-1)


def pack_q5_k(d, dmin, sc, mn, q):
    """As Q4_K with q in 0 .. 31: the fifth bit of element e is bit e / 32 of qh[e % 32]."""
    q = np.asarray(q, np.int64)
    assert q.min() >= 0 and q.max() <= 31
    n = q.shape[0]
    out = np.zeros((n, 176), np.uint8)
    out[:, 0:2], out[:, 2:4] = _h(d), _h(dmin)
    out[:, 4:16] = _pack_k4(sc, mn)
    out[:, 16:48] = ((q >> 4).reshape(n, 8, 32) << np.arange(8)[None, :, None]).sum(axis=1).astype(np.uint8)
    g = (q & 15).reshape(n, 4, 2, 32)
    out[:, 48:176] = (g[:, :, 0] | (g[:, :, 1] << 4)).reshape(n, 128).astype(np.uint8)
    return out.reshape(-1)


def pack_q6_k(d, sc, q):
    """d f16 [n]; sc [n][16] int8; q [n][256] in -32 .. 31: w = d sc q per sub-block of 16.  Per 128 elements: the low nibbles of
    elements l and l + 64 share byte l of ql, l + 32 and l + 96 byte l + 32; the high two bits of all four share byte l of qh."""
    sc, q = np.asarray(sc, np.int64), np.asarray(q, np.int64)
    assert sc.min() >= -128 and sc.max() <= 127 and q.min() >= -32 and q.max() <= 31
    n = q.shape[0]
    out = np.zeros((n, 210), np.uint8)
    g = (q + 32).reshape(n, 2, 4, 32)
    lo, hi = g & 15, g >> 4
    ql = np.stack([lo[:, :, 0] | (lo[:, :, 2] << 4), lo[:, :, 1] | (lo[:, :, 3] << 4)], axis=2)  # [n][2][2][32]
    out[:, 0:128] = ql.reshape(n, 128).astype(np.uint8)
    out[:, 128:192] = (hi[:, :, 0] | (hi[:, :, 1] << 2) | (hi[:, :, 2] << 4) | (hi[:, :, 3] << 6)).reshape(n, 64).astype(np.uint8)
    out[:, 192:208] = sc.astype(np.int8).view(np.uint8)
    out[:, 208:210] = _h(d)
    return out.reshape(-1)


# ---- part A: exact integers --------------------------------------------------------------------------------------------------
def _place(rng, a, width, values):
    """Puts each of the one or two `values` at its own random position of every `width` consecutive elements of the rows of a."""
    g = a.reshape(-1, width)
    rows = np.arange(g.shape[0])
    pos = rng.integers(0, width, g.shape[0])
    g[rows, pos] = values[0]
    if len(values) == 2:
        g[rows, (pos + rng.integers(1, width, g.shape[0])) % width] = values[1]
    assert len(values) <= 2
    return a


_ANCHOR = {Q4_0: (-8, 7, (-8,)), Q4_1: (0, 15, (0, 15)), Q5_0: (-16, 15, (-16,)), Q5_1: (0, 31, (0, 31)), Q8_0: (-127, 127, (127,))}


def exact_w_block(t, M, K, rng, wmax=None):
    """An integer matrix [M][K] that ggml's quantizer of type t stores with d = 1 (and m = 0): values of the format's range (cut to
    |w| <= wmax where given) with the anchor of the format in every block of 32 — the value the quantizer derives d from."""
    lo, hi, anchors = _ANCHOR[t]
    if wmax is not None:
        lo, hi = max(lo, -wmax), min(hi, wmax)
    W = rng.integers(lo, hi + 1, (M, K))
    return _place(rng, W, 32, anchors)


def exact_x_block(N, K, rng, xmax):
    """Integer activations [N][K], |x| <= xmax, with one +-127 in every block of 32: Q8_0 / Q8_1 give d = 1, q = x."""
    X = rng.integers(-xmax, xmax + 1, (N, K))
    g = X.reshape(-1, 32)
    pos = rng.integers(0, 32, g.shape[0])
    g[np.arange(g.shape[0]), pos] = np.where(rng.random(g.shape[0]) < 0.5, -127, 127)
    return X


def exact_x_k(N, K, rng, xmax):
    """Integer activations, |x| <= xmax <= 127, with one -128 in every 256: Q8_K gives iscale = 1, d = 1, q = x."""
    assert xmax <= 127
    X = rng.integers(-xmax, xmax + 1, (N, K))
    g = X.reshape(-1, 256)
    g[np.arange(g.shape[0]), rng.integers(0, 256, g.shape[0])] = -128
    return X


def exact_w_k_quantizable(t, M, K, rng):
    """Q3_K / Q6_K: an integer matrix the oracle's quantizer stores exactly — the most negative code (-4 / -32) in every 16."""
    lo, hi = {Q3_K: (-4, 3), Q6_K: (-32, 31)}[t]
    return _place(rng, rng.integers(lo, hi + 1, (M, K)), 16, (lo,))


def exact_w_k(t, M, K, rng, small=False):
    """Hand-packed K-quant blocks with d = dmin = 1: (raw bytes, the integer matrix [M][K] they stand for).  Sub-block scales and
    mins cover their whole range (the six-bit ones of sub-blocks 4 .. 7 with their split packing), codes every value; Q6_K's
    int8 scales stay within +-63 so that every weight (<= 63 * 32) is an f16 value.  small: scales and mins of at most 7, for
    rows so long that the sums would pass 2^24."""
    n = M * K // 256
    one = np.ones(n, np.float16)

    def ints(lo, hi, shape, cap=7):
        if small:
            lo, hi = max(lo, -cap), min(hi, cap)
        return rng.integers(lo, hi + 1, shape)

    if t == Q2_K:
        sc, mn, q = ints(0, 15, (n, 16)), ints(0, 15, (n, 16)), rng.integers(0, 4, (n, 256))
        return pack_q2_k(one, one, sc, mn, q), (np.repeat(sc, 16, 1) * q - np.repeat(mn, 16, 1)).reshape(M, K)
    if t == Q3_K:
        sc, q = ints(-32, 31, (n, 16)), rng.integers(-4, 4, (n, 256))
        return pack_q3_k(one, sc, q), (np.repeat(sc, 16, 1) * q).reshape(M, K)
    if t in (Q4_K, Q5_K):
        top = 16 if t == Q4_K else 32
        sc, mn, q = ints(0, 63, (n, 8)), ints(0, 63, (n, 8)), rng.integers(0, top, (n, 256))
        raw = (pack_q4_k if t == Q4_K else pack_q5_k)(one, one, sc, mn, q)
        return raw, (np.repeat(sc, 32, 1) * q - np.repeat(mn, 32, 1)).reshape(M, K)
    sc, q = ints(-63, 63, (n, 16)), rng.integers(-32, 32, (n, 256))
    return pack_q6_k(one, sc, q), (np.repeat(sc, 16, 1) * q).reshape(M, K)


def exact_product(X, W, group):
    """The preconditions of part A, then the product: X [N][K] and W [M][K] integer matrices, group = 32 or 256.
    - sum |x| |w| < 2^24 for every output: every partial sum of any summation order is an exact f32 integer;
    - |x|, |w| <= 2048: both are f16 values, their products exact in f32 (the f16 GEMMs);
    - the sums a format stores per block (Q8_1's s = d * sum q, Q8_K's bsums over 16) are integers far below 2^24 / int16.
    Returns f32 [N][M].  The matmul runs in float64, which is exact here (every sum is an integer below 2^24)."""
    X, W = np.asarray(X), np.asarray(W)
    assert np.issubdtype(X.dtype, np.integer) and np.issubdtype(W.dtype, np.integer)
    assert np.abs(X).max() <= 2048 and np.abs(W).max() <= 2048
    Xf, Wf = X.astype(np.float64), W.astype(np.float64)
    top = float((np.abs(Xf) @ np.abs(Wf).T).max())
    assert top < 2 ** 24, f"sum |x||w| reaches {top:.0f} >= 2^24: shrink the value ranges"
    per = 32 if group == 32 else 16
    assert np.abs(X.reshape(-1, per).sum(axis=1)).max() < 2 ** 15
    out = Xf @ Wf.T
    assert np.array_equal(out, np.rint(out))
    return out.astype(F)


_MEAN_W = {Q2_K: (10, 6), Q3_K: (32, 8), Q4_K: (230, 30), Q5_K: (480, 60), Q6_K: (520, 60)}  # about mean |w| of exact_w_k: full, small


def ranges_for(t, K):
    """(xmax, wmax) for a block format, (xmax, small) for a K format: value ranges that keep sum |x||w| below 2^24 at this row
    length — never a shorter K.  Block formats: the whole range up to K = 1024, beyond that |x| <= 31 and |w| <= 15, the anchors
    excepted.  K formats: scales and mins of at most 7 beyond K = 1024, and |x| cut so that K * mean |w| * mean |x| stays near
    2^23.  exact_product checks the outcome."""
    if t in BLOCK_TYPES:
        return (126, None) if K <= 1024 else (31, 15)
    small = K > 1024
    return int(np.clip(2 * (2 ** 23 // (K * _MEAN_W[t][small])), 1, 127)), small


def exact_case(t, M, K, N, quantize=None):
    """The inputs of one case of part A: (raw weight bytes, W integers [M][K], X integers [N][K]).  Block formats and, with
    quantize given for Q3_K / Q6_K, the quantizable matrices go through `quantize(t, W as f32)`; the other K weights are packed
    by hand.  The seed is the case itself."""
    rng = np.random.default_rng([t, M, K, N, 0 if quantize is None else 1])
    if t in BLOCK_TYPES:
        xmax, wmax = ranges_for(t, K)
        W = exact_w_block(t, M, K, rng, wmax)
        return quantize(t, W.astype(F)), W, exact_x_block(N, K, rng, xmax)
    xmax, small = ranges_for(t, K)
    if quantize is not None:
        assert t in (Q3_K, Q6_K)
        W = exact_w_k_quantizable(t, M, K, rng)
        return quantize(t, W.astype(F)), W, exact_x_k(N, K, rng, 127 if K <= 1024 else 31)
    raw, W = exact_w_k(t, M, K, rng, small)
    return raw, W, exact_x_k(N, K, rng, xmax)


# ---- part B: blocks for the one-hot reveal -----------------------------------------------------------------------------------
def _f16_scales(rng, n, top):
    """n f16 scales with random 11-bit significands, |d| < top, a third of them negative; then: zeros of either sign, subnormals,
    powers of two.  Returned as f16."""
    e_top = int(np.floor(np.log2(top))) - 1
    e = rng.integers(-14, e_top + 1, n)
    mant = rng.integers(0, 1024, n)
    bits = (((e + 15) << 10) | mant).astype(np.uint16)
    bits[rng.random(n) < 0.33] |= 0x8000
    fam = rng.random(n)
    bits[fam < 0.03] = 0x0000
    bits[(fam >= 0.03) & (fam < 0.05)] = 0x8000
    sub = (fam >= 0.05) & (fam < 0.15)
    bits[sub] = rng.integers(1, 1024, int(sub.sum())).astype(np.uint16) | (rng.integers(0, 2, int(sub.sum())).astype(np.uint16) << 15)
    return bits.view(np.float16)


def reveal_blocks(t, nblk, rng):
    """nblk raw blocks of type t for part B: every code (the first blocks walk through all of them, the rest are random), scales
    from _f16_scales, and for Q4_1 / Q5_1 an m of either sign that is near d * code (it cancels), far above it, far below it,
    zero or subnormal.  Every |value| stays below W16_MAX."""
    lo, hi = CODES[t]
    codes = rng.integers(lo, hi + 1, (nblk, 32))
    walk = (np.arange(nblk * 32) % (hi - lo + 1) + lo).reshape(nblk, 32)
    head = min(nblk, 16)
    codes[:head] = walk[:head]
    span = max(abs(lo - ZERO[t]), abs(hi - ZERO[t]))
    if t not in HAS_M:
        return pack_block(t, _f16_scales(rng, nblk, W16_MAX / span), codes)
    d = _f16_scales(rng, nblk, 0.5 * W16_MAX / span)
    d32 = d.astype(np.float64)
    fam = rng.integers(0, 5, nblk)
    near = -d32 * rng.integers(0, hi + 1, nblk) * rng.uniform(0.85, 1.0, nblk)  # nearly cancels against some code's product
    far_up = rng.uniform(0.1, 0.45, nblk) * W16_MAX * np.where(rng.random(nblk) < 0.5, -1, 1)
    far_down = d32 * rng.uniform(-1, 1, nblk) * 2.0 ** -8
    tiny = rng.integers(0, 1024, nblk) * 2.0 ** -24 * np.where(rng.random(nblk) < 0.5, -1, 1)  # zero or subnormal
    m = np.choose(fam, [near, far_up, far_down, tiny, np.abs(near)]).astype(np.float16)
    # a tenth of the blocks: d = (odd 11-bit significand below 4096 / 3) * 2^e >= 2, so that d * 3 is an exact f16 tie, and m one
    # or two units of 2^-24, far below the f32 rounding of the sum: the single rounding follows the sign of m, a decoder that
    # rounds the f32 sum first sees the tie itself
    sel = np.flatnonzero(rng.random(nblk) < 0.1)
    e = rng.integers(1, max(2, int(np.floor(np.log2(0.5 * W16_MAX / span)))), sel.size)
    d = d.copy()
    d.view(np.uint16)[sel] = (((e + 15) << 10) | (2 * rng.integers(0, 170, sel.size) + 1)).astype(np.uint16)
    m[sel] = (rng.integers(1, 3, sel.size) * np.where(rng.random(sel.size) < 0.5, -1, 1) * 2.0 ** -24).astype(np.float16)
    return pack_block(t, d, codes, m)


_K_SCALE_AT = {Q2_K: (80, 82), Q3_K: (108,), Q4_K: (0, 2), Q5_K: (0, 2), Q6_K: (208,)}


def reveal_k_blocks(t, nblk, rng):
    """nblk raw K-quant super-blocks: random bytes everywhere (every code, every packed scale), d / dmin from _f16_scales with
    |d| < 2^-5 (the largest weight, 128 * 32 * d for Q6_K, stays far inside the f16 range)."""
    raw = rng.integers(0, 256, (nblk, BLOCK_BYTES[t]), dtype=np.uint8)
    for at in _K_SCALE_AT[t]:
        raw[:, at:at + 2] = _h(_f16_scales(rng, nblk, 2.0 ** -5))
    return raw.reshape(-1)


def one_hot(K, value):
    """K tokens of K elements, token k with `value` at position k."""
    return (np.eye(K) * value).astype(F)


# ---- part C: the operands and the bound --------------------------------------------------------------------------------------
def x16_block(X, t):
    """The activation operand of the f16 GEMMs for a Q4_0 .. Q8_0 weight, [N][K] f16 in ggml's element order (default branch)."""
    X = np.ascontiguousarray(X, F)
    return R.q8_f16(X, 0, t in F16D, identity=True).view(np.float16).reshape(X.shape)


def x16_k(X):
    """... for a K-quant weight: f16(d8 * q8) of the Q8_K round trip."""
    X = np.ascontiguousarray(X, F)
    return R.q8k_f16(X, identity=True).view(np.float16).reshape(X.shape)


def operand_product(x16, w16):
    """(ref, S, bound): ref = x16 . w16 and S = |x16| . |w16| in float64, bound = 2 K 2^-24 S.  Every product of two f16 values
    is exact in f32, so a GEMM differs from ref by its K f32 additions only: K 2^-24 S for correctly rounded additions in any
    order, doubled because the rounding of the matrix cores' internal additions is not documented."""
    x, w = x16.astype(np.float64), w16.astype(np.float64)
    K = x.shape[1]
    S = np.abs(x) @ np.abs(w).T
    return x @ w.T, S, 2.0 * K * 2.0 ** -24 * S


def random_inputs(M, K, N, seed, nonneg=False):
    """Weights and activations of the kinds the other mul_mat tests use (gaussian weights of std 0.02, gaussian activations with
    heavier channels); nonneg: the magnitudes of both, so that a biased rounding of an operand adds up instead of averaging out."""
    rng = np.random.default_rng(seed)
    W = (0.02 * rng.standard_normal((M, K))).astype(F)
    X = rng.standard_normal((N, K)).astype(F)
    X[:, ::7] *= 4.0
    return (np.abs(W), np.abs(X)) if nonneg else (W, X)
