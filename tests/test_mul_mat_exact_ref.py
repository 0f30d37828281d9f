"""The helpers of tests/mul_mat_exact_ref.py, checked without a GPU: (a) every packer against the oracle's decoder, bit for bit;
(b) the inputs of part A meet their preconditions — the oracle decodes the weights to the intended integers, the oracle's mul_mat
(scalar and reference mode) returns the exact integer product, every row sum stays below 2^24; (c) the blocks of part B hold
every code, zero, negative and subnormal scales, and enough exact f16 rounding ties; the single-rounding reference differs from
f16(dequantize) for Q4_1 / Q5_1 and equals it for the other formats; (d) the sets are sharp: each mutant — a weight operand
truncated toward zero, one k element dropped, one code off by one — breaks part C's bound on part C's own inputs, and a dropped
element changes part A's integer result."""
import numpy as np
import pytest

import mul_mat_exact_ref as E

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _f32(h):
    return np.asarray(h, np.float16).astype(F)


# ---- (a) packers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", E.BLOCK_TYPES)
def test_block_packer_equals_the_oracle_decoder(O, t):
    rng = np.random.default_rng([t, 1])
    raw = E.reveal_blocks(t, 640, rng)
    assert raw.size == 640 * E.BLOCK_BYTES[t] == 640 * O.type_size(t) and O.blck_size(t) == 32
    d, m, codes = E.unpack_block(t, raw)
    assert np.array_equal(E.pack_block(t, d, codes, m), raw)
    c = (codes - E.ZERO[t]).astype(F)
    want = c * _f32(d)[:, None] if m is None else (c * _f32(d)[:, None]).astype(F) + _f32(m)[:, None]  # ggml's f32 decoder
    assert np.array_equal(_bits(O.dequantize(t, raw, 640 * 32)), _bits(want.reshape(-1)))
    # the exact value agrees with the f32 decoder wherever that is exact: always for d * (code - zero)
    if m is None:
        assert np.array_equal(E.exact_block(t, raw).reshape(-1), want.reshape(-1).astype(np.float64))


def _scaled(d, sc, width):
    """f32(d * sc) per element: the decoders' first product, each sub-block scale repeated over its `width` elements."""
    return (_f32(d)[:, None] * np.repeat(sc, width, 1).astype(F)).astype(F)


def _k_parts(t, n, rng):
    d, dmin = E._f16_scales(rng, n, 2.0 ** -5), E._f16_scales(rng, n, 2.0 ** -5)
    if t == E.Q2_K:
        sc, mn, q = rng.integers(0, 16, (n, 16)), rng.integers(0, 16, (n, 16)), rng.integers(0, 4, (n, 256))
        raw = E.pack_q2_k(d, dmin, sc, mn, q)
        w = _scaled(d, sc, 16) * q.astype(F) - _scaled(dmin, mn, 16)
    elif t == E.Q3_K:
        sc, q = rng.integers(-32, 32, (n, 16)), rng.integers(-4, 4, (n, 256))
        raw = E.pack_q3_k(d, sc, q)
        w = _scaled(d, sc, 16) * q.astype(F)
    elif t in (E.Q4_K, E.Q5_K):
        sc, mn, q = rng.integers(0, 64, (n, 8)), rng.integers(0, 64, (n, 8)), rng.integers(0, 16 if t == E.Q4_K else 32, (n, 256))
        raw = (E.pack_q4_k if t == E.Q4_K else E.pack_q5_k)(d, dmin, sc, mn, q)
        w = _scaled(d, sc, 32) * q.astype(F) - _scaled(dmin, mn, 32)
    else:
        sc, q = rng.integers(-128, 128, (n, 16)), rng.integers(-32, 32, (n, 256))
        raw = E.pack_q6_k(d, sc, q)
        w = _scaled(d, sc, 16) * q.astype(F)
    return raw, w.astype(F)


@pytest.mark.parametrize("t", E.K_TYPES)
def test_k_packer_equals_the_oracle_decoder(O, t):
    """Random parts over their whole range (the split six-bit scales of sub-blocks 4 .. 7, every code, scales of either sign, zero
    and subnormal) against ggml's f32 decoder restated here operation by operation."""
    raw, want = _k_parts(t, 300, np.random.default_rng([t, 2]))
    assert raw.size == 300 * E.BLOCK_BYTES[t] == 300 * O.type_size(t) and O.blck_size(t) == 256
    assert np.array_equal(_bits(O.dequantize(t, raw, 300 * 256)), _bits(want.reshape(-1)))


# ---- (b) part A ----------------------------------------------------------------------------------------------------------------
def _check_exact_case(O, t, raw, W, X, K, group):
    M = W.shape[0]
    assert raw.size == M * E.row_bytes(t, K)
    assert np.array_equal(O.dequantize(t, raw, M * K).reshape(M, K), W.astype(F))  # integer-valued, and the intended integers
    ref = E.exact_product(X, W, group)
    rows = np.unique(np.concatenate([[0, M - 1], np.random.default_rng(M).choice(M, min(M, 24), replace=False)]))
    rb = E.row_bytes(t, K)
    sub = np.concatenate([raw[r * rb:(r + 1) * rb] for r in rows])
    for mode in (0, O.ref_mode()):
        assert np.array_equal(O.mul_mat(t, sub, len(rows), K, X.astype(F), mode=mode), ref[:, rows]), (t, K, mode)
    return ref


BLOCK_KS = (96, 128, 352, 1024, 4096, 11008)
K_KS = (256, 1024, 2816, 4096, 11008)


@pytest.mark.parametrize("t", E.BLOCK_TYPES)
def test_exact_block_cases_meet_their_preconditions(O, t):
    for K in BLOCK_KS:
        raw, W, X = E.exact_case(t, 70, K, 9, O.quantize)
        lo, hi, anchors = E._ANCHOR[t]
        for a in anchors:
            assert np.all((W.reshape(-1, 32) == a).any(axis=1))
        d, m, codes = E.unpack_block(t, raw)
        assert np.all(_f32(d) == 1.0) and (m is None or not m.any())
        assert np.all((np.abs(X).reshape(-1, 32) == 127).sum(axis=1) >= 1) and np.abs(X).max() == 127
        _check_exact_case(O, t, raw, W, X, K, 32)
        if K <= 1024:  # the whole range of the format is there
            assert W.min() == lo and W.max() == hi
        # the activation quantizers return the integers with d = 1 in both branches
        for branch in (0, 1):
            q, dq, _ = E.R.q8(X.astype(F), branch, t in E.F16D)
            assert np.array_equal(q.reshape(X.shape), X) and np.all(dq == 1.0)


@pytest.mark.parametrize("t", E.K_TYPES)
def test_exact_k_cases_meet_their_preconditions(O, t):
    for K in K_KS:
        for quantize in (None, O.quantize) if t in (E.Q3_K, E.Q6_K) else (None,):
            raw, W, X = E.exact_case(t, 40, K, 9, quantize)
            assert np.all((X.reshape(-1, 256) == -128).sum(axis=1) == 1) and np.abs(X).max() == 128
            q, dq, bs = E.R.q8k(X.astype(F))
            assert np.array_equal(q.reshape(X.shape), X) and np.all(dq == 1.0)
            assert np.array_equal(E.R.round_f16(W.astype(F)), W.astype(F))  # every weight is an f16 value
            _check_exact_case(O, t, raw, W, X, K, 256)
    # the hand-packed blocks of the short rows use every code and the whole range of their scales and mins
    n = 4096
    rng = np.random.default_rng(t)
    raw, W = E.exact_w_k(t, n, 256, rng)
    if t in (E.Q4_K, E.Q5_K):
        top = 15 if t == E.Q4_K else 31
        assert W.max() == 63 * top and W.min() == -63
    if t == E.Q6_K:
        assert W.max() == 63 * 32 and W.min() == -63 * 32 + 63 - 63
    if t == E.Q2_K:
        assert W.max() == 45 and W.min() == -15
    if t == E.Q3_K:
        assert W.max() == 128 and W.min() == -124


def test_a_dropped_element_changes_the_integer_result(O):
    for t in E.BLOCK_TYPES + E.K_TYPES:
        K = 1024
        raw, W, X = E.exact_case(t, 33, K, 5, O.quantize if t in E.BLOCK_TYPES else None)
        ref = E.exact_product(X, W, 32 if t in E.BLOCK_TYPES else 256)
        changed = 0
        for k in (0, 31, 517, K - 1):
            Wm = W.copy()
            Wm[:, k] = 0
            changed += int(np.any(E.exact_product(X, Wm, 32 if t in E.BLOCK_TYPES else 256) != ref))
        assert changed >= 3, (t, changed)  # (an element may be zero in every row of one column, never in all four)


# ---- (c) part B ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", E.BLOCK_TYPES)
@pytest.mark.parametrize("K", [256, 96])
def test_reveal_blocks_hold_the_families_and_the_ties(O, t, K):
    M = 130
    raw = E.reveal_blocks(t, M * K // 32, np.random.default_rng([t, K, 3]))
    d, m, codes = E.unpack_block(t, raw)
    lo, hi = E.CODES[t]
    assert set(np.unique(codes)) == set(range(lo, hi + 1))
    db = d.view(np.uint16)
    assert (db == 0).any() and (db == 0x8000).any()  # d = 0 of either sign
    assert ((db & 0x7C00) == 0)[(db & 0x3FF) != 0].any()  # subnormal d
    assert (db & 0x8000).any() and (~db & 0x8000).any()
    normal = (db & 0x7C00) != 0
    assert np.unique(db[normal] & 0x3FF).size > 200 and ((db[normal] & 1) == 1).any()  # full 11-bit significands
    v = E.exact_block(t, raw)
    assert np.abs(v).max() <= E.W16_MAX
    ties = E.f16_ties(v)
    share = ties.mean()
    print(f"type {t} K {K}: {int(ties.sum())} of {v.size} revealed values are exact f16 ties ({100 * share:.1f} %)")
    assert share >= 0.01
    w16 = E.w16_block(t, raw, K)
    lower, upper = E.round_f16(v, trunc=True).reshape(-1, K), w16
    assert (lower != upper).any()  # the truncating mutant differs on the set
    deq = O.dequantize(t, raw, M * K).reshape(M, K).astype(np.float16)
    if m is None:  # one f32 product, exact: its f16 rounding is the single rounding
        assert np.array_equal(w16, deq)
    else:  # the f32 sum rounds first: double rounding differs somewhere on this set
        mv = m.view(np.uint16)
        assert (mv & 0x8000).any() and (~mv & 0x8000).any() and ((mv & 0x7FFF) < 0x400).any()
        n_diff = int(np.count_nonzero(w16 != deq))
        print(f"type {t} K {K}: f16(dequantize) differs from the single rounding on {n_diff} values")
        assert n_diff > 0


def test_the_tie_detector():
    h = np.array([1.0, 1.0 + 2.0 ** -10, 2.0 ** -24, 0.0, 1024.0], np.float64)
    assert not E.f16_ties(h).any()
    mid = np.array([1.0 + 2.0 ** -11, -(1.0 + 3 * 2.0 ** -11), 2.0 ** -25, 3 * 2.0 ** -25, 1024.5, 2049.0], np.float64)
    assert E.f16_ties(mid).all()
    assert not E.f16_ties(mid * (1 + 2.0 ** -30)).any()
    # nearest even on both sides of a tie
    assert E.round_f16(1.0 + 2.0 ** -11) == np.float16(1.0) and E.round_f16(1.0 + 3 * 2.0 ** -11) == np.float16(1.0 + 2.0 ** -9)
    assert E.round_f16(2.0 ** -25) == 0 and E.round_f16(3 * 2.0 ** -25) == np.float16(2.0 ** -23)
    assert E.round_f16(1.0 + 3 * 2.0 ** -11, trunc=True) == np.float16(1.0 + 2.0 ** -10)


@pytest.mark.parametrize("t", E.K_TYPES)
def test_reveal_k_blocks_hold_the_families(O, t):
    M, K = 8192 + 130, 256
    raw = E.reveal_k_blocks(t, M, np.random.default_rng([t, 4]))
    w = O.dequantize(t, raw, M * K)
    assert np.all(np.isfinite(w)) and np.abs(w).max() < 65504
    w16 = w.astype(np.float16)
    assert (w16.astype(F) != w).mean() > 0.2  # the f16 rounding of the copy is visible
    b = raw.reshape(M, E.BLOCK_BYTES[t])
    for at in E._K_SCALE_AT[t]:
        db = b[:, at:at + 2].copy().view(np.uint16).reshape(-1)
        assert (db == 0).any() and (db & 0x8000).any() and ((db & 0x7C00) == 0)[(db & 0x3FF) != 0].any()
    assert np.unique(b[:, 40]).size == 256  # quant bytes: every pattern
    assert (w16[8192 * K:] != 0).any()  # rows of the second chunk carry weights


# ---- (d) part C and its mutants ------------------------------------------------------------------------------------------------
def _operands(O, t, M, K, N, nonneg):
    W, X = E.random_inputs(M, K, N, [t, M, K, N, int(nonneg)], nonneg)
    raw = O.quantize(t, W)
    if t in E.BLOCK_TYPES:
        return raw, E.x16_block(X, t), E.w16_block(t, raw, K)
    return raw, E.x16_k(X), O.dequantize(t, raw, M * K).reshape(M, K).astype(np.float16)


@pytest.mark.parametrize("t", E.BLOCK_TYPES + E.K_TYPES)
def test_the_bound_of_part_c_catches_a_dropped_element_and_a_wrong_code(O, t):
    M, K, N = 300, 256, 300
    raw, x16, w16 = _operands(O, t, M, K, N, False)
    ref, S, bound = E.operand_product(x16, w16)
    assert np.all(bound >= 0) and np.isclose(2.0 * K * 2.0 ** -24, 3.05e-5, rtol=1e-2)
    x, w = x16.astype(np.float64), w16.astype(np.float64)
    # one k element dropped, in every row
    k = 77
    dropped = ref - np.outer(x[:, k], w[:, k])
    assert np.any(np.abs(dropped - ref) > bound)
    # ... and counted twice in one row only
    twice = ref.copy()
    twice[:, 5] += x[:, k] * w[5, k]
    assert np.any(np.abs(twice - ref) > bound)
    # one code off by one in a single block (at the column of the largest activation)
    n0, k0 = np.unravel_index(np.argmax(np.abs(x)), x.shape)
    m0 = 11
    raw2 = raw.copy()
    rb = E.row_bytes(t, K)
    if t in E.BLOCK_TYPES:
        d, m, codes = E.unpack_block(t, raw2[m0 * rb:(m0 + 1) * rb])
        lo, hi = E.CODES[t]
        c = codes[k0 // 32, k0 % 32]
        codes[k0 // 32, k0 % 32] = c + 1 if c < hi else c - 1
        raw2[m0 * rb:(m0 + 1) * rb] = E.pack_block(t, d, codes, m)
        w2 = E.w16_block(t, raw2[m0 * rb:(m0 + 1) * rb], K)[0].astype(np.float64)
    else:  # flip the lowest bit of the code's byte: every K format keeps the low bits of its codes in plain bytes
        qs_at = {E.Q2_K: 16, E.Q3_K: 32, E.Q4_K: 16, E.Q5_K: 48, E.Q6_K: 0}[t]
        sb, e = divmod(int(k0), 256)
        byte = {E.Q2_K: 32 * (e // 128) + e % 32, E.Q3_K: 32 * (e // 128) + e % 32, E.Q4_K: 32 * (e // 64) + e % 32,
                E.Q5_K: 32 * (e // 64) + e % 32, E.Q6_K: 64 * (e // 128) + e % 64}[t]
        shift = {E.Q2_K: 2 * ((e % 128) // 32), E.Q3_K: 2 * ((e % 128) // 32), E.Q4_K: 4 * ((e % 64) // 32), E.Q5_K: 4 * ((e % 64) // 32),
                 E.Q6_K: 4 * ((e % 128) // 64)}[t]
        raw2[m0 * rb + sb * E.BLOCK_BYTES[t] + qs_at + byte] ^= np.uint8(1 << shift)
        w2 = O.dequantize(t, raw2[m0 * rb:(m0 + 1) * rb], K).astype(np.float16).astype(np.float64)
    changed = np.flatnonzero(w2 != w[m0])
    assert changed.tolist() == [k0], (t, changed, k0)  # one weight moved, by one step of its code
    wrong = ref.copy()
    wrong[:, m0] = x @ w2
    assert np.abs(wrong[n0, m0] - ref[n0, m0]) > bound[n0, m0], (t, abs(wrong[n0, m0] - ref[n0, m0]) / bound[n0, m0])


@pytest.mark.parametrize("t,shape", [(E.Q4_1, (300, 256, 300)), (E.Q4_1, (1000, 1024, 513)), (E.Q5_1, (300, 256, 300)),
                                     (E.Q5_1, (1000, 1024, 513)), (E.Q4_K, (300, 256, 300))])
def test_the_bound_of_part_c_catches_a_truncated_weight_operand(O, t, shape):
    """All weights and activations non-negative: truncation moves every weight the same way, about 2^-12 S in all, where the bound
    is 2 K 2^-24 S."""
    M, K, N = shape
    raw, x16, w16 = _operands(O, t, M, K, N, True)
    assert np.all(x16 >= 0) and np.all(w16 >= 0)
    ref, S, bound = E.operand_product(x16, w16)
    if t in E.BLOCK_TYPES:
        trunc = E.w16_block(t, raw, K, trunc=True)
    else:
        trunc = E.round_f16(O.dequantize(t, raw, M * K).astype(np.float64), trunc=True).reshape(M, K)
    mut = x16.astype(np.float64) @ trunc.astype(np.float64).T
    worst = float(np.max(np.abs(mut - ref) / np.maximum(bound, 1e-300)))
    print(f"type {t} {shape}: truncated weights are off by up to {worst:.2f} x the bound")
    assert np.any(np.abs(mut - ref) > bound)
