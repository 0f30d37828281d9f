"""CPU pins of tests/prompt_attn_ref.py: the host reference of the prompt batch attention and the three input families of
tests/test_prompt_attn_gpu.py are held to their premises here, without a GPU — the reference against the oracle's
scale -> mask -> softmax, the one-hot family to "exactly one 1.0 at the intended key, and the masked bait outranks it", the
exact-score family to order-independent scores and rows that contain subnormal and zero exponentials, and the interval of the
Gaussian family to containing the f64 result while EXCLUDING index mistakes at T = 1000 (causal limit off by one either way, a
key dropped, a head on the wrong K/V head), of which the older absolute tolerance (4e-3 * max|ref| on four rows) lets the
off-by-one limits through."""
import numpy as np
import pytest

import prompt_attn_ref as R


@pytest.fixture(scope="module")
def tab():
    return R.host_exp_table()


def test_exp_table_premises(tab):
    """What family (a) relies on: e(arg) == 0 for every f16 arg <= -20 (-inf included), e(0) == 1; and what the interval relies
    on only for tightness: the table is monotone on arg <= 0."""
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    t = tab.view(np.float16)
    assert np.all(t[x <= -20] == 0) and (x <= -20).sum() > 1000 and t[0xFC00] == 0
    assert t[0] == 1 and t[0x8000] == 1
    neg = t[0x8000 | np.arange(0x7C01)].astype(np.float64)
    assert np.all(np.diff(neg) <= 0)
    assert np.exp(-18.0) < 2.0 ** -25  # below half of f16's smallest subnormal: rounds to zero


def test_launcher_boundaries():
    """prompt_attn_queries restated: 32 queries per workgroup up to 1152 keys (32 x (1152 x 4 + 16) = 147968 <= 153600 bytes;
    1153 rounds up to 1216 keys: 156160), 16 up to 2368 (16 x (2368 x 4 + 16) = 151808; 2369 -> 2432: 155904)."""
    assert R.boundaries(128) == (1152, 2368) and R.boundaries(32) == (1152, 2368)
    assert [R.queries_per_workgroup(64, t) for t in (1, 1152, 1153, 2368, 2369)] == [32, 32, 16, 16, 0]
    assert R.queries_per_workgroup(96, 64) == 0


@pytest.mark.parametrize("N,H,Hkv,D,n_past", [(5, 2, 1, 32, 0), (17, 4, 2, 32, 3), (33, 2, 2, 64, 30), (8, 1, 1, 128, 57)])
def test_reference_probabilities_are_the_oracles(O, tab, N, H, Hkv, D, n_past):
    """P of the reference == f16(O.scale_mask_softmax(scores)) in the reference's branch, for the exact-score family (the scores
    handed to the oracle are then the very f32 values) and both scales."""
    T = n_past + N
    q, k, v = R.spread_inputs(N, H, Hkv, D, n_past, T + 8)
    s = np.stack([R.head_scores(q, k, T, h, h // (H // Hkv), D) for h in range(H)]).astype(np.float32)
    for scale in (R.SPREAD_SCALE, 0.125):
        want = O.scale_mask_softmax(s, scale, n_past, mode=O.ref_mode()).astype(np.float16)
        ref = R.reference(q, k, v, H, Hkv, n_past, scale, tab, keep=True)
        for h in range(H):
            assert np.array_equal(ref["heads"][h][0].view(np.uint16), want[h].view(np.uint16)), (h, scale)


ONEHOT = [(33, 4, 2, 32, 0, 160), (64, 2, 1, 64, 37, 160), (100, 3, 3, 128, 449, 160), (40, 2, 2, 32, 1700, 320),
          (17, 2, 1, 64, 1000, 640), (1, 2, 2, 32, 0, 160)]


@pytest.mark.parametrize("N,H,Hkv,D,n_past,a", ONEHOT)
def test_onehot_family_premises(tab, N, H, Hkv, D, n_past, a):
    T = n_past + N
    q, k, v, want = R.onehot_inputs(N, H, Hkv, D, n_past, T + 8, a=a)
    assert np.array_equal(q, q.astype(np.float16).astype(np.float32))  # f16-exact
    assert np.isnan(k[T:].astype(np.float32)).all() and np.isnan(v[:, T:].astype(np.float32)).all()
    vv = v[:, :T]
    assert np.isfinite(vv.astype(np.float32)).all() and np.all(np.abs(vv) >= np.float16(2.0 ** -14))  # normal numbers only
    for hk in range(Hkv):
        cols = vv[hk * D:(hk + 1) * D].view(np.uint16).T
        assert len({c.tobytes() for c in cols}) == T  # distinct columns: a wrong key is a mismatch
    ref = R.reference(q, k, v, H, Hkv, n_past, R.ONEHOT_SCALE, tab, keep=True)
    assert np.array_equal(ref["target"], want)
    modes = (np.arange(N)[:, None] + np.arange(H)[None, :]) % 3
    saw_inf = False
    for h in range(H):
        s = R.head_scores(q, k, T, h, h // (H // Hkv), D) * R.ONEHOT_SCALE
        assert np.array_equal(s, np.rint(s)) and np.abs(s).max() * 8 < 2 ** 24
        p, e, arg = ref["heads"][h]
        saw_inf |= bool(np.isinf(arg.astype(np.float32)).any())
        for n in range(N):
            lim = n_past + n
            if want[n, h] >= 0:
                assert p[n, want[n, h]] == 1 and (p[n] != 0).sum() == 1
                others = np.delete(s[n, :lim + 1], want[n, h])
                assert others.size == 0 or s[n, want[n, h]] - others.max() >= 20  # beats every other visible key by >= 20
            else:  # the indicator key is masked: a tie over all visible keys, the bait behind the limit
                assert modes[n, h] == 2 and np.all(s[n, :lim + 1] == 0) and s[n, lim + 1:].max() >= 20
                assert np.all(p[n, :lim + 1] == np.float16(np.float32(1.0 / (lim + 1))))
            if modes[n, h] == 0 and lim + 1 < T:
                assert s[n, lim + 1] > s[n, lim]  # the first masked key outranks the target: a limit one too far picks it
    assert saw_inf == (a * 0.125 * (T - 1) > 65520)
    # alternation: neighbouring rows of one head want different things
    assert all(len({int(modes[n, 0]) for n in range(n0, min(n0 + 3, N))}) == min(3, N - n0) for n0 in range(0, N, 3))


SPREAD = [(64, 2, 1, 32, 0), (33, 2, 2, 64, 100), (100, 1, 1, 128, 412), (16, 2, 1, 32, 1200)]


@pytest.mark.parametrize("N,H,Hkv,D,n_past", SPREAD)
def test_spread_family_premises(tab, N, H, Hkv, D, n_past):
    """Scores identical when accumulated in f32 forwards, backwards and in f64; each case's rows (cases of 64 keys or more: a
    shorter row cannot promise a span of 17) contain subnormal and zero e next to normal ones; p * v exact in f32."""
    T = n_past + N
    q, k, v = R.spread_inputs(N, H, Hkv, D, n_past, T + 8)
    assert np.array_equal(q, q.astype(np.float16).astype(np.float32))
    ref = R.reference(q, k, v, H, Hkv, n_past, R.SPREAD_SCALE, tab, keep=True)
    vis = R.visible(N, T, n_past)
    for h in range(H):
        hk = h // (H // Hkv)
        qh = q[:, h * D:(h + 1) * D].astype(np.float32)
        kh = k[:T, hk * D:(hk + 1) * D].astype(np.float32)
        fwd = np.zeros((N, T), np.float32)
        bwd = np.zeros((N, T), np.float32)
        for d in range(D):
            fwd += qh[:, d:d + 1] * kh[None, :, d]
            bwd += qh[:, D - 1 - d:D - d] * kh[None, :, D - 1 - d]
        s64 = R.head_scores(q, k, T, h, hk, D)
        assert np.array_equal(fwd.astype(np.float64), s64) and np.array_equal(bwd.astype(np.float64), s64)
        p, e, arg = ref["heads"][h]
        ev = e[vis].astype(np.float64)
        assert ((ev > 0) & (ev < 2.0 ** -14)).any() and (ev == 0).any() and (ev >= 2.0 ** -14).sum() > N
        vh = v[hk * D:(hk + 1) * D, :T].astype(np.float64)
        prod = p.astype(np.float64)[:, None, :8] * vh[None, :, :8]
        assert np.array_equal(prod.astype(np.float32).astype(np.float64), prod)


def _outside(x, lo, hi):
    return int(((x < lo) | (x > hi)).sum())


def test_interval_contains_the_f64_result_and_excludes_index_mistakes(tab):
    """The interval of the Gaussian family at T = 1000 (96 queries behind 904 keys, as a case of the older test): it contains the
    f64 attention, and does NOT contain the same with the causal limit one key further, one key nearer, one key dropped, or
    one head reading the other K/V head.  The older tolerance (4e-3 * max(1, max|ref|), rows 0 and N - 1 of heads 0 and H - 1)
    accepts the first two (a dropped key it sees only where the key's weight is large), which is what this file's tests are for."""
    N, H, Hkv, D, n_past = 96, 4, 2, 32, 904
    T = n_past + N
    scale = 1.0 / np.sqrt(D)
    q, k, v = R.gauss_inputs(N, H, Hkv, D, n_past, T + 8)
    lo, hi, edges = R.interval(q, k, v, H, Hkv, n_past, scale, tab)
    good = R.plain_f64(q, k, v, H, Hkv, n_past, scale)
    assert np.all(lo <= hi) and _outside(good, lo, hi) == 0
    width = float(np.max(hi - lo))
    print("interval: worst width %.2e, edges arg %d p %d of %d visible" % (width, edges["arg"], edges["p"], edges["visible"]))
    old_atol = 4e-3 * max(1.0, float(np.abs(good).max()))
    assert width < old_atol / 5  # (and the median far below: most elements have few edges)
    for name, kw in [("limit + 1", dict(limit_shift=1)), ("limit - 1", dict(limit_shift=-1)), ("key 500 dropped", dict(drop_key=500)),
                     ("head 1 on K/V head 1", dict(wrong_head=(1, 1)))]:
        bad = R.plain_f64(q, k, v, H, Hkv, n_past, scale, **kw)
        n_out = _outside(bad, lo, hi)
        rows = [(n, h) for n in (0, N - 1) for h in (0, H - 1)]  # what the older check looks at
        d = max(float(np.max(np.abs((bad - good)[n, h * D:(h + 1) * D]))) for n, h in rows)
        print("%-22s max|delta| on the older check's rows %.2e (its atol %.1e), %d of %d elements outside the interval"
              % (name, d, old_atol, n_out, bad.size))
        assert n_out > 0, name
        if "limit" in name:
            assert d <= old_atol, (name, d)  # the older tolerance does not see it


def test_plan_form_restatements():
    """mmq_kperm_inv is a permutation with the 8-byte groups of kernels/prompt.h (4 adjacent elements -> k order {0, 2, 1, 3});
    quarter-turn tables rotate exactly and the inverse rotation undoes them; the re-quantization on a hand-made block."""
    perm = [R.kperm_inv(e) for e in range(32)]
    assert sorted(perm) == list(range(32))
    assert perm[:4] == [0, 2, 1, 3] and perm[16:20] == [4, 6, 5, 7] and perm[4:8] == [8, 10, 9, 11]
    tabq = R.rope_table_quarter_turns(7, 64)
    x = np.random.default_rng(0).integers(-40, 41, (7, 128)).astype(np.float32)
    y = R.rotate(R.rotate(x, tabq, 2, inverse=True), tabq, 2)
    assert np.array_equal(y, x)
    out = np.zeros((1, 64), np.float32)
    out[0, :32] = np.arange(32) - 10       # amax 21: d = 21 / 127
    out[0, 32:] = 0                         # all-zero block: id = 0, every code 0
    for f16d in (0, 1):
        for scalar in (False, True):
            bits = R.requant_x16(out, f16d, scalar)
            got = bits.view(np.float16).astype(np.float32)[0]
            assert np.all(got[32:] == 0)
            back = np.array([got[R.kperm_inv(e)] for e in range(32)])
            assert np.allclose(back, out[0, :32], rtol=0, atol=21 / 127 * 0.51 + 21 * 2.0 ** -10)
    big = np.full((1, 32), 1000.0, np.float32)
    big[0, 5] = -65504.0  # d = 515.78 -> f16 516: 516 * 127 = 65532 clamps to 65504
    got = R.requant_x16(big, 1).view(np.float16).astype(np.float32)[0]
    assert got[R.kperm_inv(5)] == -65504.0 and np.isfinite(got).all()
