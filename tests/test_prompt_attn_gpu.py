"""The attention of a prompt batch — k_p_attn (kernels/prompt_attn.h, one launch, the prompt plan's default) and the
three-launch path k_gemm_f16 / k_p_soft_max / k_gemm_f16_b16 — against the host reference of tests/prompt_attn_ref.py, on EVERY
row, head and channel, each device path on its own (two implementations agreeing is not a reference).

Three input families (prompt_attn_ref.py; their premises are pinned without a GPU in test_prompt_attn_ref.py):
 (a) one-hot rows: one visible key beats every other by >= 20 after scaling, so p is one 1.0 and out[n, head h] must equal a
     column of V BIT FOR BIT, with no assumption about accumulation order.  The maximum sits on the row's last visible key
     (the first masked key scores higher still), on key 0, or on a chosen key at a tile / chunk border; rows whose chosen key is
     still masked tie over all visible keys and are checked as (b).  Scores reach f16 -inf arguments (a = 320 / 640).
 (b) exact scores, spread rows: every score is exact in f32 in any order (also under an MFMA that keeps 24 significant bits
     relative to its largest addend — nobody has measured that hardware's internal rounding here), the exponential is pinned by
     the device's own table (ggml_hip_debug_exp_le0, held to f64 exp in test_prompt_plan_gpu.py), so the host predicts P bit
     for bit, f16 subnormals and zeros included; only the f32 accumulation of V . P is free:
     |got - V.p| <= T * 2^-23 * sum_j |v_j| p_j for every element.  The worst err / bound per case is printed.
 (c) Gaussian rows: a per-element interval propagated through every rounding point (prompt_attn_ref.interval) instead of
     one absolute tolerance; the counts of f16 edges are printed.

The plan form of k_p_attn (RoPE while Q is staged, two K-split partials added first, the Q8 re-quantizing epilogue) runs
through ggml_hip_debug_prompt_attention_plan and is compared as f16 BITS with the re-quantization restated in NumPy.

Measured on an MI355X (this file's output, 312 exact-family launches and 12 Gaussian ones): worst err / bound of (b) 0.085 (short
rows), 0.007 (rows of 1040 .. 2368 keys), 0.037 (512 / 1024 workgroups); of the tied rows of (a) 0.038.  Edges of (c), arg / p of
visible elements: 783 / 961 of 8320 (T = 64), 3533 / 10867 of 34122 (T = 533), 74812 / 224135 of 300200 (T = 800, D = 128),
13239 / 44735 of 365760 (T = 1000), 7055 / 24242 of 78132 (T = 1157), 5328 / 19297 of 164206 (T = 2237); the worst element sits
at 0.006 of its interval's width inside the nearer end at T = 64 and at 0.32 .. 0.45 on the longer rows; widest interval 1.6e-3.
The matrix cores keep f16 subnormal probabilities (read back through an identity V while looking for the defect below).

What these tests found: k_p_attn computed p = f16(e * inv) with ONE rounding — (_Float16)(e * inv) is selected as
v_fma_mixlo_f16 — where ggml, the three-launch path and the reference round the product to f32 first.  Family (b), N = 1, H = 8,
D = 64, n_past = 16: head 6, key 11, p 0x1270 expected, 0x126f computed, 7 elements of out 4.3 bounds off.  Fixed in
kernels/prompt_attn.h (f16_of_f32_product); since then the two device paths agree bit for bit on every Gaussian case here
(before: 1 .. 8 % of the rows differed, which the older test's docstring put down to the scores' last bit)."""
import numpy as np
import pytest

import prompt_attn_ref as R

pytestmark = pytest.mark.gpu

PATHS = (1, 0)  # fused, three-launch


@pytest.fixture(scope="module")
def tabs(G):
    """e(arg) of each device path for all f16 bit patterns: exp_le0 (fused) / expf (three-launch)."""
    fast = np.zeros(65536, np.uint16)
    ref = np.zeros(65536, np.uint16)
    assert G.lib().ggml_hip_debug_exp_le0(fast.ctypes.data, ref.ctypes.data) == 0
    return {1: fast, 0: ref}


def _attn(G, q, k, v, H, n_past, scale, fused):
    N, E = q.shape
    C, Eg = k.shape
    out = np.zeros((N, E), np.float32)
    rc = G.lib().ggml_hip_debug_prompt_attention(q.ctypes.data, k.ctypes.data, v.ctypes.data, out.ctypes.data, N, E, Eg, H, n_past, C,
                                                 scale, fused)
    return rc, out


def _expected_columns(ref, v, H, Hkv, D):
    """out of the one-hot (n, h): V[head h // r, :, target] as f32; mask [N][E] of those elements."""
    N = ref["target"].shape[0]
    want = np.zeros((N, H * D), np.float32)
    mask = np.zeros((N, H * D), bool)
    r = H // Hkv
    for h in range(H):
        t = ref["target"][:, h]
        one = t >= 0
        cols = v[(h // r) * D:(h // r + 1) * D][:, np.where(one, t, 0)].T.astype(np.float32)  # [N][D]
        want[:, h * D:(h + 1) * D] = cols
        mask[:, h * D:(h + 1) * D] = one[:, None]
    return want, mask


def _check_exact(tag, got, ref, v, H, Hkv, D):
    """One-hot rows bit for bit, every other element within the accumulation bound.  Returns the worst err / bound."""
    assert not np.isnan(got).any(), (tag, "unwritten or NaN output", np.argwhere(np.isnan(got))[:4].tolist())
    want, mask = _expected_columns(ref, v, H, Hkv, D)
    bad = mask & (got.view(np.uint32) != want.view(np.uint32))
    if bad.any():
        n, c = np.argwhere(bad)[0]
        raise AssertionError((tag, "one-hot row differs from its V column", int(bad.sum()), "first: row %d head %d channel %d" % (n, c // D, c % D),
                              float(got[n, c]), float(want[n, c]), "target key", int(ref["target"][n, c // D])))
    err = np.abs(got.astype(np.float64) - ref["out"])
    over = ~mask & (err > ref["bound"])
    if over.any():
        n, c = np.argwhere(over)[0]
        raise AssertionError((tag, "outside the accumulation bound", int(over.sum()), "first: row %d head %d channel %d" % (n, c // D, c % D),
                              float(got[n, c]), float(ref["out"][n, c]), "bound", float(ref["bound"][n, c])))
    sel = ~mask & (ref["bound"] > 0)
    return float((err[sel] / ref["bound"][sel]).max()) if sel.any() else 0.0


COMBOS = [(32, 4, 4), (64, 4, 2), (128, 4, 1), (64, 8, 1), (128, 2, 2), (32, 8, 2)]  # D, H, Hkv: H / Hkv = 1, 2, 4, 8
NS = [1, 15, 16, 17, 31, 32, 33, 64, 100, 512]


def _cache_len(T, i):
    """C == T (no spare cache row: the K clamp min(.., C - 1) is live) where T allows (C % 8 == 0), else up to 23 spare rows."""
    return T if (T % 8 == 0 and i % 2 == 0) else (T + 7) // 8 * 8 + 8 * (i % 3)


def _short_cases():
    """Every N of the issue x n_past = 0, odd, and T on and next to multiples of 16, 32, 64, 128 and 512 (npad, nkt, load_v's
    `valid` of 0, 1..7 and 8, k_p_soft_max's nc <= 512 branch and its multi-pass branch); the head shapes take turns."""
    cases, i = [], 0
    for N in NS:
        pasts = {0, 7}
        for t in (16, 17, 31, 32, 33, 48, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1024):
            if t - N >= 0:
                pasts.add(t - N)
        for n_past in sorted(pasts):
            D, H, Hkv = COMBOS[i % len(COMBOS)]
            cases.append((N, H, Hkv, D, n_past, _cache_len(n_past + N, i), 160))
            i += 1
    for D, H, Hkv in COMBOS[:3]:  # every head size on the ragged batches, whatever the rotation above gave them
        for N, n_past in ((17, 0), (33, 449), (100, 31)):
            cases.append((N, H, Hkv, D, n_past, _cache_len(n_past + N, i), 160))
            i += 1
    return cases


def _long_cases():
    """Rows of 819 keys and more: f16 -inf arguments (a = 640 up to 1152 keys, a = 320 from 1638 on), the boundaries of
    prompt_attn_queries (T = 1152 | 1153: 32 | 16 queries per workgroup; 2368: the last T the fused kernel takes), and the
    16-query workgroups' ragged last tiles (waves of 4 rows: nrow = 4, 1..3, <= 0)."""
    t32, t16 = R.boundaries()
    assert (t32, t16) == (1152, 2368)
    return [(64, 4, 2, 64, t32 - 64, t32, 640), (64, 4, 4, 128, t32 - 64, t32 + 8, 160), (33, 2, 2, 32, 1000, 1040, 640),
            (512, 4, 4, 128, t32 - 512, t32, 640), (512, 2, 1, 64, t32 + 1 - 512, t32 + 8, 160),
            (16, 4, 1, 128, t32 + 1 - 16, t32 + 8, 160), (1, 4, 4, 32, 1300, 1304, 160), (15, 4, 2, 64, 1200, 1216, 160),
            (17, 2, 2, 128, 1500, 1520, 160), (31, 8, 1, 32, 2000, 2032, 320), (33, 4, 4, 64, 2300, 2336, 320),
            (100, 4, 2, 128, t16 - 100, t16, 320), (512, 2, 2, 32, t16 - 512, t16, 320)]


def _run_exact_family(G, tabs, family, cases):
    worst = 0.0
    for N, H, Hkv, D, n_past, C, a in cases:
        if family == "onehot":
            q, k, v, want = R.onehot_inputs(N, H, Hkv, D, n_past, C, a=a)
            scale = R.ONEHOT_SCALE
        else:
            q, k, v = R.spread_inputs(N, H, Hkv, D, n_past, C)
            scale = R.SPREAD_SCALE
        for fused in PATHS:
            ref = R.reference(q, k, v, H, Hkv, n_past, scale, tabs[fused])
            if family == "onehot":  # the rows are one-hot where the construction says so, under THIS path's table
                assert np.array_equal(ref["target"], want), (N, H, D, n_past, fused)
            rc, got = _attn(G, q, k, v, H, n_past, scale, fused)
            tag = (family, "fused" if fused else "three-launch", "N %d H %d Hkv %d D %d n_past %d C %d a %d" % (N, H, Hkv, D, n_past, C, a))
            assert rc == 0, tag
            ratio = _check_exact(tag, got, ref, v, H, Hkv, D)
            worst = max(worst, ratio)
            print("%-7s %-12s N %3d H %2d Hkv %2d D %3d n_past %4d C %4d a %3d: one-hot rows %5d of %5d, worst err / bound %.3f"
                  % (family, tag[1], N, H, Hkv, D, n_past, C, a, int((ref["target"] >= 0).sum()), N * H, ratio))
    print("%s: %d cases x 2 paths, worst err / bound %.3f" % (family, len(cases), worst))


def test_device_tables_make_one_hot_rows(tabs):
    """What family (a) relies on, asserted on the device's tables before anything leans on it: e(arg) == 0 for every f16
    arg <= -20 (f16 -inf included), e(+-0) == 1, in exp_le0's table and in expf's."""
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    for fused in PATHS:
        t = tabs[fused].view(np.float16)
        assert np.all(t[x <= -20] == 0) and t[0xFC00] == 0 and t[0] == 1 and t[0x8000] == 1, fused


@pytest.mark.parametrize("rows", ["short", "long"])
@pytest.mark.parametrize("family", ["onehot", "spread"])
def test_every_row_against_the_exact_reference(G, tabs, family, rows):
    """Families (a) and (b) on both device paths; shapes in _short_cases / _long_cases.
    The worst err / bound is printed per case and per path (figures in the module docstring)."""
    _run_exact_family(G, tabs, family, _short_cases() if rows == "short" else _long_cases())


def test_launcher_boundaries_on_the_device(G, tabs):
    """prompt_attn_queries' refusal: T = 2369 is the first the fused kernel does not take (-1) and the three-launch path still
    runs it, against the reference; T > C is refused by both.  (T = 1152 | 1153 | 2368 run in the "long" cases above.)"""
    t16 = R.boundaries()[1]
    N, H, Hkv, D = 33, 2, 1, 64
    n_past = t16 + 1 - N
    for family in ("onehot", "spread"):
        if family == "onehot":
            q, k, v, _ = R.onehot_inputs(N, H, Hkv, D, n_past, t16 + 8, a=320)
            scale = R.ONEHOT_SCALE
        else:
            q, k, v = R.spread_inputs(N, H, Hkv, D, n_past, t16 + 8)
            scale = R.SPREAD_SCALE
        assert _attn(G, q, k, v, H, n_past, scale, 1)[0] == -1
        rc, got = _attn(G, q, k, v, H, n_past, scale, 0)
        assert rc == 0
        ref = R.reference(q, k, v, H, Hkv, n_past, scale, tabs[0])
        print(family, "T", t16 + 1, "three-launch: worst err / bound %.3f" % _check_exact((family, "T 2369"), got, ref, v, H, Hkv, D))
    q, k, v = R.spread_inputs(16, 2, 2, 32, 48, 64)
    for fused in PATHS:
        assert _attn(G, q, k[:56].copy(), v[:, :56].copy(), 2, 48, 0.5, fused)[0] == -1  # T = 64 > C = 56


def test_more_workgroups_than_compute_units(G, tabs):
    """The query tiles behind r1 (qt = rank - r1, dealt shortest-first) run only with more workgroups than CUs and two of them per
    CU: N = 512, H = 32, D = 128 (512 workgroups, r1 = num_cus / 32) and more heads than CUs (H = 2 num_cus, D = 32, N = 64:
    r1 = 1).  One-hot rows make a wrongly mapped tile an exact mismatch; the spread family checks the same tiles' arithmetic."""
    cus = int(G.lib().ggml_hip_get_stat(b"num_cus"))
    assert cus >= 8
    cases = [(512, 32, 32, 128, 0, 512, 160), (64, 2 * cus, cus // 2, 32, 0, 72, 160)]
    for N, H, Hkv, D, n_past, C, a in cases:
        ntile = (N + 31) // 32
        assert ntile * H > cus and max(1, min(ntile, cus // H)) < ntile  # the launcher's r1 < ntile
    _run_exact_family(G, tabs, "onehot", cases)
    _run_exact_family(G, tabs, "spread", cases)


GAUSS = [(64, 4, 4, 32, 0), (33, 2, 1, 64, 500), (100, 4, 2, 128, 700), (96, 4, 4, 32, 904), (17, 4, 2, 64, 1140), (37, 2, 2, 32, 2200)]


def test_gaussian_rows_within_the_propagated_interval(G, tabs):
    """Family (c): N(0,1) operands, scale 1 / sqrt(D), EVERY element of out inside prompt_attn_ref.interval — the tolerance is
    the interval, no share of rows is left out.  Printed per case: the widest interval and the edges (visible elements whose
    arg / p interval holds more than one f16 value)."""
    for N, H, Hkv, D, n_past in GAUSS:
        T = n_past + N
        q, k, v = R.gauss_inputs(N, H, Hkv, D, n_past, (T + 7) // 8 * 8 + 8)
        scale = float(np.float32(1.0 / np.sqrt(D)))
        both = {}
        for fused in PATHS:
            lo, hi, edges = R.interval(q, k, v, H, Hkv, n_past, scale, tabs[fused])
            rc, got = _attn(G, q, k, v, H, n_past, scale, fused)
            both[fused] = got
            assert rc == 0 and not np.isnan(got).any()
            g = got.astype(np.float64)
            out = (g < lo) | (g > hi)
            pos = float(np.max(np.maximum(lo - g, g - hi) / (hi - lo)))
            print("gauss %-12s N %3d H %d Hkv %d D %3d n_past %4d: widest interval %.2e, worst excess / width %+.3f, edges arg %d p %d of %d"
                  % ("fused" if fused else "three-launch", N, H, Hkv, D, n_past, float((hi - lo).max()), pos, edges["arg"], edges["p"],
                     edges["visible"]))
            assert not out.any(), (N, H, Hkv, D, n_past, fused, int(out.sum()), np.argwhere(out)[:4].tolist())
        diff = both[1] != both[0]  # information: the two paths against each other
        print("      fused vs three-launch: %d of %d elements differ, max |delta| %.2e" % (int(diff.sum()), diff.size, float(np.abs(both[1] - both[0]).max())))


# ---- the plan form
def _plan(G, q1, q2, rope, k, v, H, n_past, scale, f16d):
    N, E = q1.shape
    C, Eg = k.shape
    x16 = np.zeros(N * E + 128, np.uint16)   # + 256 guard bytes
    out = np.zeros(N * E + 64, np.float32)
    rc = G.lib().ggml_hip_debug_prompt_attention_plan(q1.ctypes.data, q2.ctypes.data if q2 is not None else None, rope.ctypes.data,
                                                      k.ctypes.data, v.ctypes.data, x16.ctypes.data, out.ctypes.data, N, E, Eg, H, n_past,
                                                      C, scale, f16d)
    assert rc == 0
    assert np.all(x16[N * E:] == 0xFFFF), "a store behind x16"
    assert np.all(out.view(np.uint32) == 0xFFFFFFFF), "the f32 out is not written in this form"
    return x16[:N * E].reshape(N, E)


def _split(q_raw, seed):
    """Two partials whose f32 sum is exactly q_raw (integers, or multiples of 1/4, far below 2^24)."""
    qa = np.random.default_rng(seed).integers(-8, 9, q_raw.shape).astype(np.float32)
    qb = (q_raw - qa).astype(np.float32)
    assert np.array_equal(qa + qb, q_raw)
    return qa, qb


def _blocks_differ(a, b):
    d = np.argwhere(a != b)
    return [] if d.size == 0 else ["%d elements, first row %d channel %d: %04x / %04x" % (len(d), d[0][0], d[0][1], a[d[0][0], d[0][1]], b[d[0][0], d[0][1]])]


PLAN = [(33, 4, 2, 32, 0, 40), (64, 4, 4, 64, 37, 104), (100, 4, 1, 128, 449, 552), (17, 2, 2, 128, 1200, 1224), (512, 8, 8, 128, 0, 512)]


@pytest.mark.parametrize("family", ["onehot", "spread"])
def test_plan_form_rotates_adds_partials_and_requantizes(G, tabs, family):
    """ggml_hip_debug_prompt_attention_plan: (i) with every RoPE angle a multiple of a quarter turn and q_raw the inverse rotation of
    a family (a) / (b) Q, given whole or as two partials with an exact sum, the kernel's rotated Q is exactly that Q; (iii) x16 must
    then equal, as f16 BITS, the block re-quantization (prompt_attn_ref.requant_x16) of the plain form's out for that Q — for
    f16d 0 and 1 and option act_quant 0 and 1.  For (a) the one-hot blocks are ALSO compared with the re-quantized V columns, so
    the check does not lean on the two forms sharing an accumulation order; for (b) it does, as the kernel header claims.  The
    one-hot V holds an all-zero block (amax = 0) and a block that clamps (d = 65504 / 127 -> f16 516: 516 x 127 > 65504)."""
    for N, H, Hkv, D, n_past, C in PLAN:
        if family == "onehot":
            q, k, v, _ = R.onehot_inputs(N, H, Hkv, D, n_past, C)
            v[0:32, 0] = 0                          # rows of heads on K/V head 0 that pick key 0: an all-zero block
            v[0:32, n_past + 3] = np.float16(1000)  # row 3 of head 0 picks its last visible key: a block that clamps
            v[5, n_past + 3] = np.float16(-65504)
            scale = R.ONEHOT_SCALE
        else:
            q, k, v = R.spread_inputs(N, H, Hkv, D, n_past, C)
            scale = R.SPREAD_SCALE
        tabq = R.rope_table_quarter_turns(N, D, seed=N)
        q_raw = R.rotate(q, tabq, H, inverse=True)
        assert np.array_equal(R.rotate(q_raw, tabq, H), q)
        rc, plain = _attn(G, q, k, v, H, n_past, scale, 1)
        assert rc == 0
        ref = R.reference(q, k, v, H, Hkv, n_past, scale, tabs[1])
        _check_exact((family, "plain", N, D, n_past), plain, ref, v, H, Hkv, D)
        cols, mask = _expected_columns(ref, v, H, Hkv, D)
        if family == "onehot":
            blocks = plain.reshape(N, -1, 32)
            assert (np.abs(blocks).max(axis=2) == 0).any() and (np.abs(blocks) == 65504).any()
        try:
            for aq in (0, 1):
                G.set_option("act_quant", aq)
                for f16d in (0, 1):
                    want = R.requant_x16(plain, f16d, scalar=bool(aq))
                    for parts in (1, 2):
                        qa, qb = (q_raw, None) if parts == 1 else _split(q_raw, N)
                        got = _plan(G, qa, qb, tabq, k, v, H, n_past, scale, f16d)
                        tag = (family, N, H, Hkv, D, n_past, "act_quant", aq, "f16d", f16d, "partials", parts)
                        assert not _blocks_differ(got, want), (tag, _blocks_differ(got, want))
                        if family == "onehot":
                            want_v = R.requant_x16(np.where(mask, cols, 0), f16d, scalar=bool(aq))
                            assert np.array_equal(got[mask], want_v[mask]), tag
        finally:
            G.set_option("act_quant", 0)
        print("plan form %-7s N %3d H %d Hkv %d D %3d n_past %4d: x16 identical for act_quant x f16d x partials (8 launches)"
              % (family, N, H, Hkv, D, n_past))


def test_plan_form_with_a_real_rope_table(G):
    """(ii) cos / sin of real angles, Gaussian q_raw (whole, and as two Gaussian partials added in f32 first): the rotation restated
    in f32 (x0 c - x1 s, x0 s + x1 c, every operation rounded on its own) feeds the plain form; its re-quantized out must be the
    plan form's x16 bit for bit."""
    for N, H, Hkv, D, n_past, C in [(33, 4, 2, 32, 0, 40), (100, 4, 4, 64, 449, 552), (64, 2, 1, 128, 1100, 1168)]:
        _, k, v = R.gauss_inputs(N, H, Hkv, D, n_past, C)
        rng = np.random.default_rng([N, D, 9])
        qa = rng.standard_normal((N, H * D)).astype(np.float32)
        qb = rng.standard_normal((N, H * D)).astype(np.float32)
        tab = R.rope_table_real(N, D, n_past)
        scale = float(np.float32(1.0 / np.sqrt(D)))
        for parts in (1, 2):
            q_raw = qa if parts == 1 else (qa + qb).astype(np.float32)
            rc, plain = _attn(G, R.rotate(q_raw, tab, H), k, v, H, n_past, scale, 1)
            assert rc == 0 and not np.isnan(plain).any()
            for f16d in (0, 1):
                got = _plan(G, qa, None if parts == 1 else qb, tab, k, v, H, n_past, scale, f16d)
                want = R.requant_x16(plain, f16d)
                assert not _blocks_differ(got, want), (N, D, n_past, parts, f16d, _blocks_differ(got, want))
