"""The references and the input sets of the activation quantizer tests (tests/act_quant_ref.py), checked without a GPU:
(a) the NumPy references equal the oracle's quantize_row byte for byte on every input set, both branches, Q8_0 / Q8_1 / Q8_K;
(b) every input set holds the families the quantizers can go wrong on; (c) the sets are sharp: each mutant of a reference — one
decision of the arithmetic changed — differs from the reference on the set (the counts are printed); (d) the rows of the norm
kinds satisfy the midpoint condition under which the normed row can be compared bit for bit."""
import numpy as np
import pytest

import act_quant_ref as R

F = np.float32


@pytest.fixture(scope="module")
def q8_set():
    return R.q8_pool()


@pytest.fixture(scope="module")
def q8k_set():
    return R.q8k_pool()


def test_references_equal_the_oracle(O, q8_set, q8k_set):
    x, _ = q8_set
    for branch in (0, 1):
        simd = branch == 0
        assert np.array_equal(R.q8_bytes(x, branch, True), O.quantize_row(O.T_Q8_0, x, simd=simd)), ("q8_0", branch)
        assert np.array_equal(R.q8_bytes(x, branch, False), O.quantize_row(O.T_Q8_1, x, simd=simd)), ("q8_1", branch)
        if simd and O.have_avx2():  # ... and the intrinsics themselves, where this host has them
            assert np.array_equal(R.q8_bytes(x, 0, True), O.quantize_row(O.T_Q8_0, x, simd="avx2"))
            assert np.array_equal(R.q8_bytes(x, 0, False), O.quantize_row(O.T_Q8_1, x, simd="avx2"))
    xk, _ = q8k_set
    assert np.array_equal(R.q8k_bytes(xk), O.quantize_row(O.T_Q8_K, xk))
    # the Q8 set read as super-blocks and the Q8_K set read as blocks: more of the same, for free
    assert np.array_equal(R.q8k_bytes(x), O.quantize_row(O.T_Q8_K, x))
    for branch in (0, 1):
        assert np.array_equal(R.q8_bytes(xk, branch, True), O.quantize_row(O.T_Q8_0, xk, simd=branch == 0))
    # a larger random draw, all magnitudes
    rng = np.random.default_rng(7)
    y = (rng.standard_normal((512, 256)) * 2.0 ** rng.integers(-16, 15, (512, 1))).astype(F)
    for branch in (0, 1):
        assert np.array_equal(R.q8_bytes(y, branch, True), O.quantize_row(O.T_Q8_0, y, simd=branch == 0))
        assert np.array_equal(R.q8_bytes(y, branch, False), O.quantize_row(O.T_Q8_1, y, simd=branch == 0))
    assert np.array_equal(R.q8k_bytes(y), O.quantize_row(O.T_Q8_K, y))


def test_q8_set_holds_the_families(q8_set):
    x, fam = q8_set
    fam = np.array(fam)
    assert x.shape == (72, 32) and np.all(np.isfinite(x))
    amax = np.abs(x).max(axis=1)
    assert not np.any((amax > 0) & (amax < 2.0 ** -100))
    rnd = amax[fam == "random"]
    assert rnd.min() < 2.0 ** -13 and rnd.max() > 2.0 ** 13 and (fam == "random").sum() >= 31
    z = x[fam == "zero"]
    assert z.shape[0] == 1 and not z.any() and not np.signbit(z).any()
    nz = x[fam == "negzero"]
    assert nz.shape[0] == 1 and not nz.any() and np.signbit(nz).all()
    assert np.all((x[fam == "single"] != 0).sum(axis=1) == 1) and (fam == "single").sum() >= 2
    # exact ties: amax = 127 * 2^k, both multipliers 2^-k, the other products n + 0.5 with n of both parities and signs
    ties = x[fam == "tie"]
    assert ties.shape[0] >= 6
    ks = set()
    for b in ties:
        a = np.abs(b).max()
        k = np.log2(a / 127.0)
        assert k == np.round(k)
        ks.add(int(k))
        i0, i1 = F(127.0) / F(a), F(1.0) / (F(a) / F(127.0))
        assert i0 == i1 == F(2.0 ** -k)
        p = (b * i0).astype(F)
        half = p[np.abs(p) < 127]
        assert half.size == 31 and np.all(half % 1 == 0.5)
        n = np.floor(half).astype(int)
        assert (n % 2 == 0).any() and (n % 2 == 1).any() and (half > 0).any() and (half < 0).any()
    assert len(ks) >= 4
    # near-edge: the multipliers differ, and some values round apart between the branches without being ties
    for b in x[fam == "edge"]:
        a = F(np.abs(b).max())
        i0, i1 = F(127.0) / a, F(1.0) / (a / F(127.0))
        assert i0 != i1
        p0, p1 = (b * i0).astype(F), (b * i1).astype(F)
        apart = (R.q8(b, 0, True)[0][0] != R.q8(b, 1, True)[0][0]) & (p0 % 1 != 0.5) & (p1 % 1 != 0.5)
        assert apart.sum() >= 8
    assert (fam == "edge").sum() >= 4
    # d rounded to f16: subnormal, on a rounding tie (both directions), at the top of the range
    d = (amax / F(127.0)).astype(F)
    ds = d[fam == "d_subnormal"]
    assert ds.size >= 2 and np.all((ds > 0) & (ds < 2.0 ** -14))
    dt = d[fam == "d_tie"].astype(np.float64)
    lo = dt.astype(np.float16).astype(np.float64)
    assert dt.size >= 2 and np.all(dt != lo)
    up, dn = np.nextafter(dt.astype(np.float16), np.float16(np.inf)), np.nextafter(dt.astype(np.float16), np.float16(-np.inf))
    other = np.where(lo > dt, dn, up).astype(np.float64)
    assert np.all(np.abs(lo - dt) == np.abs(other - dt)), "d is not on an f16 rounding tie"
    assert (lo > dt).any() and (lo < dt).any()
    top = d[fam == "d_top"]
    assert top.size >= 2 and np.all(top > 65000) and np.all(np.isfinite(top.astype(np.float16))) and (top == 65504).any()
    # saturation of the f16 operand: d * q beyond 65504
    q, dd, _ = R.q8(x[fam == "saturate"], 0, True)
    assert (np.abs(dd[:, None] * q.astype(F)) > 65504).any()


def test_q8k_set_holds_the_families(q8k_set):
    x, fam = q8k_set
    fam = np.array(fam)
    assert x.shape == (36, 256) and np.all(np.isfinite(x))
    amax = np.abs(x).max(axis=1)
    assert not np.any((amax > 0) & (amax < 2.0 ** -100))
    rnd = amax[fam == "random"]
    assert rnd.min() < 2.0 ** -13 and rnd.max() > 2.0 ** 13
    assert (fam == "zero").sum() == 1 and not x[fam == "zero"].any() and not np.signbit(x[fam == "zero"]).any()
    assert (fam == "negzero").sum() == 1 and np.signbit(x[fam == "negzero"]).all()
    assert np.all((x[fam == "single"] != 0).sum(axis=1) == 1)
    signs, ks = set(), set()
    for b in x[fam == "tie"]:
        i = np.abs(b).argmax()
        k = np.log2(abs(b[i]) / 128.0)
        assert k == np.round(k)
        ks.add(int(k))
        signs.add(float(np.sign(b[i])))
        p = (F(-128.0) / b[i] * b).astype(F)
        half = np.delete(p, i)
        assert np.all(half % 1 == 0.5)
        n = np.floor(half).astype(int)
        assert (n % 2 == 0).any() and (n % 2 == 1).any() and (half > 0).any() and (half < 0).any()
    assert signs == {1.0, -1.0} and len(ks) >= 3
    # +max and -max in one super-block: first occurrence at either sign, at both sides of every reduction boundary
    seen = set()
    for b in x[fam == "extremes"]:
        at = np.flatnonzero(np.abs(b) == np.abs(b).max())
        assert at.size == 2 and b[at[0]] == -b[at[1]]
        seen.add((int(at[0]), int(at[1]), float(np.sign(b[at[0]]))))
        q = R.q8k(b)[0][0]
        assert q[at[0]] == -128 and q[at[1]] == 127  # the clamp: +128 -> 127
    for pair in R.EXTREME_PAIRS:
        assert (pair[0], pair[1], 1.0) in seen and (pair[0], pair[1], -1.0) in seen
    for need in ((0, 255), (63, 64), (15, 16), (3, 4)):
        assert need in R.EXTREME_PAIRS
    assert any(a // 4 == b // 4 for a, b in R.EXTREME_PAIRS), "two values of one lane's 4-vector"
    q, d, _ = R.q8k(x[fam == "saturate"])
    assert (np.abs(d[:, None] * q.astype(F)) > 65504).any()


def _count(a, b):
    return int(np.count_nonzero(np.asarray(a) != np.asarray(b)))


def _differs(ref, mutant):
    return sum(_count(r, m) for r, m in zip(ref, mutant))


def test_the_sets_are_sharp(q8_set, q8k_set):
    x, _ = q8_set
    xk, _ = q8k_set
    counts = {}
    for f16d in (True, False):
        r0, r1 = R.q8(x, 0, f16d), R.q8(x, 1, f16d)
        tag = "q8_0" if f16d else "q8_1"
        counts[f"{tag} branch 0 vs branch 1 (quants)"] = _count(r0[0], r1[0])
        counts[f"{tag} half-away for half-even"] = _differs(r0, R.q8(x, 0, f16d, rounding="away"))
        counts[f"{tag} half-even for half-away"] = _differs(r1, R.q8(x, 1, f16d, rounding="even"))
        counts[f"{tag} 1/d for 127/amax"] = _differs(r0, R.q8(x, 0, f16d, mult="1/d"))
        counts[f"{tag} 127/amax for 1/d"] = _differs(r1, R.q8(x, 1, f16d, mult="127/amax"))
        counts[f"{tag} sum of the low half"] = _differs(r0, R.q8(x, 0, f16d, sum_half=0))
        counts[f"{tag} sum of the high half"] = _differs(r0, R.q8(x, 0, f16d, sum_half=1))
        counts[f"{tag} f16 operand: identity for the k-permutation"] = _count(R.q8_f16(x, 0, f16d), R.q8_f16(x, 0, f16d, identity=True))
    for branch in (0, 1):
        ref = R.q8(x, branch, True)
        counts[f"q8_0 branch {branch} id from the f16-rounded d"] = _differs(ref, R.q8(x, branch, True, mult="1/d16"))
        counts[f"q8_0 branch {branch} d truncated to f16"] = _differs(ref, R.q8(x, branch, True, d16_trunc=True))
        # the f16 operand: multiplying with the unrounded d where the kind rounds it, and the reverse
        q, d, _ = R.q8(x, branch, False)
        counts[f"q8_0 branch {branch} f16 operand from the unrounded d"] = _count(R.q8_f16(x, branch, True), R.f16_operand(q, d))
    rk = R.q8k(xk)
    counts["q8_k last for first extreme"] = _differs(rk, R.q8k(xk, extreme="last"))
    counts["q8_k |max| for max"] = _differs(rk, R.q8k(xk, signed=False))
    counts["q8_k no clamp at 127"] = _differs(rk, R.q8k(xk, clamp=False))
    counts["q8_k bsums over the wrong 16"] = _count(rk[2], R.q8k(xk, bsum="cols")[2])
    counts["q8_k half-away for half-even"] = _count(rk[0], _q8k_away(xk))
    counts["q8_k f16 operand: identity for the k-permutation"] = _count(R.q8k_f16(xk), R.q8k_f16(xk, identity=True))
    counts["w16: identity for the k-permutation"] = _count(R.w16(x), R.w16(x, identity=True))
    for name, c in counts.items():
        print(f"{name}: {c} differing elements")
    zero = [n for n, c in counts.items() if c == 0]
    assert not zero, f"the input sets cannot tell these mutants from the reference: {zero}"


def _q8k_away(xk):
    """Q8_K with roundf in place of nearest_int (quants only)."""
    q = []
    for b in xk:
        a = np.abs(b)
        if a.max() == 0:
            q.append(np.zeros(256, np.int8))
            continue
        isc = F(-128.0) / b[a.argmax()]
        q.append(np.minimum(R._round_away((isc * b).astype(F)), 127).astype(np.int8))
    return np.stack(q)


def test_the_k_permutation_is_the_header_s(G):
    """kperm() is written from the comment in kernels/mmq.h; the header's own mmq_kperm_inv (element -> position) must be its inverse."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llm_amd", "csrc", "kernels", "mmq.h")).read()
    assert re.search(r"return 8 \* k \+ 4 \* h \+ \(\(\(i & 1\) << 1\) \| \(i >> 1\)\);", src)
    inv = [8 * ((e & 15) >> 2) + 4 * (e >> 4) + (((e & 3) & 1) << 1 | ((e & 3) >> 1)) for e in range(32)]
    p = R.kperm()
    assert sorted(p) == list(range(32)) and all(inv[p[i]] == i for i in range(32))


def test_norm_rows_satisfy_the_midpoint_condition():
    for E in (32, 256, 288, 768, 1056, 8192, 8224):
        x = R.norm_rows_input(3, E, seed=5)
        for r in x:
            assert R.norm_mean(r)[1] > 1e-12
        # the exactly rounded sum and a plain f64 sum in two other orders give the same f32 mean under the condition
        for r in x:
            sq = (r * r).astype(F).astype(np.float64)
            m = R.norm_mean(r)[0]
            assert F(sq.sum() / E) == m and F(sq[::-1].sum() / E) == m and F(np.add.reduce(sq.reshape(-1, 32).sum(axis=0)) / E) == m
    # ties behind the norm: the weight found makes y an exact tie where `found`
    x = R.norm_rows_input(1, 1056, seed=9)[0]
    w, found = R.norm_tie_weight(x, 1e-5, 32, seed=9)
    y = R.norm_rows(x[None], w, 1e-5)[0]
    assert found.mean() > 0.5
    assert _count(R.q8(y, 0, True)[0], R.q8(y, 1, True)[0]) > 0
