"""CPU pins of tests/flash_attn_ref.py, the host reference tests/test_flash_attn_gpu.py holds GGML_OP_FLASH_ATTN to: the mask rule,
the unmasked form, the batch and f32 variants, and that reference(), interval() and the plain f64 attention agree with each
other as far as each one's derivation says they must.

On "the reference equals plain_f64 to within its own bound": reference()'s bound covers the free f32 accumulation of V . P only;
the reference exists to model the f16 rounding points of arg, e and p, which the plain f64 attention does not have (a row 25
below its maximum carries an arg spacing of 2^-6: e moves by up to 0.8 %).  So the literal statement holds exactly where p has
no such rounding — the one-hot family, every row, asserted below (with the f32 routine's exp(-20) tails accounted for) — and
the spread family's reference is held to interval(), which accounts for every one of those roundings, on every element."""
import numpy as np
import pytest

import flash_attn_ref as F
import prompt_attn_ref as R


@pytest.fixture(scope="module")
def tab():
    return F.host_exp_table()


def test_scale_and_mask_rule():
    """scale = 1.0f / sqrtf(D) in f32; key j of row i is kept when j <= P + i, P = M - N; unmasked keeps all and ignores P."""
    assert F.scale_of(64) == np.float32(0.125) and F.scale_of(16) == np.float32(0.25)
    assert F.scale_of(80).dtype == np.float32 and abs(float(F.scale_of(80)) - 80 ** -0.5) < 2.0 ** -26
    vis = F.kept(3, 5, True)  # P = 2
    assert vis.tolist() == [[1, 1, 1, 0, 0], [1, 1, 1, 1, 0], [1, 1, 1, 1, 1]]
    assert F.kept(1, 4, True).all() and F.kept(4, 4, True).tolist() == np.tril(np.ones((4, 4), bool)).tolist()
    assert F.kept(3, 5, False).all()
    for N, M in ((3, 5), (1, 1), (7, 7)):  # the restatement through prompt_attn_ref.visible
        for masked in (True, False):
            assert np.array_equal(R.visible(N, M, F._n_past_for(N, M, masked)), F.kept(N, M, masked))


def test_onehot_a_gives_one_hot_rows(tab):
    """a * scale >= 20 for every head size, a multiple of 32 inside onehot_inputs' limits; e(arg <= -20) == 0 on the table."""
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    assert np.all(tab.view(np.float16)[x <= -20] == 0)
    for D in (32, 64, 80, 96, 128, 256):
        a = F.onehot_a(D)
        assert a % 32 == 0 and 64 * a <= 40960 and a * float(F.scale_of(D)) >= 20.0
    assert F.onehot_a(64) == 160


CASES = [(2, 33, 2, 2, 32, 64), (1, 17, 4, 2, 128, 65), (1, 5, 2, 2, 64, 70), (1, 1, 2, 1, 128, 97), (1, 3, 2, 1, 80, 33),
         (1, 4, 2, 2, 32, 37)]  # B, N, H, Hkv, D, M


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("B,N,H,Hkv,D,M", CASES)
def test_onehot_reference_equals_plain_f64_within_its_bound(tab, B, N, H, Hkv, D, M, masked, f32):
    """Every row of the one-hot family is one-hot or a tie: the reference and the plain f64 attention differ by no more than
    the reference's bound plus the tie rows' one rounding of p (2^-11, or 2^-24 in f32, relative: sum |v| p times that)."""
    q, k, v = F.onehot_inputs(B, N, H, Hkv, D, M, M + 8)
    assert np.isnan(k[:, M:].astype(np.float32)).all() and np.isnan(v[:, :, M:].astype(np.float32)).all()
    if f32:
        k, v = F.as_f32_caches(k, v)
    n_one = 0
    for b in range(B):
        ref = F.reference(q[b], k[b], v[b], H, Hkv, M, masked, tab, f32)
        plain = F.plain_f64(q[b], k[b], v[b], H, Hkv, M, masked, f32)
        one = ref["target"] >= 0
        n_one += int(one.sum())
        # f32 p: the plain attention keeps the tails the f16 e drops — every other kept key weighs at most exp(-20) (its score
        # lies 20 below the target's), and the target's own weight falls short of 1 by at most M exp(-20).  An f16 p rounds
        # them to zero as the reference's e does.
        vis = F.kept(N, M, masked).astype(np.float64)
        r = H // Hkv
        absv = np.stack([vis @ np.abs(v[b][(h // r) * D:(h // r + 1) * D, :M].astype(np.float64)).T for h in range(H)])
        tail = np.exp(-20.0) * (absv + M * np.abs(ref["out"])) if f32 else 0.0
        assert np.all((np.abs(ref["out"] - plain) <= ref["bound"] + tail)[one])
        p_round = ref["bound"] / (M * 2.0 ** -23) * (2.0 ** -24 if f32 else 2.0 ** -11)
        assert np.all(np.abs(ref["out"] - plain) <= ref["bound"] + p_round + tail)
        # one-hot rows reproduce their target key's V row exactly
        r = H // Hkv
        for h in range(H):
            for n in np.nonzero(one[h])[0]:
                col = v[b][(h // r) * D:(h // r + 1) * D, ref["target"][h, n]].astype(np.float64)
                assert np.array_equal(ref["out"][h, n], col)
        if masked:  # the family's own prediction of the targets (its limit is n_past + n = P + i)
            want = np.stack([R.onehot_inputs(N, H, Hkv, D, M - N, M + 8, a=F.onehot_a(D), seed=b)[3]]).reshape(N, H).T
            assert np.array_equal(ref["target"], want)
        else:  # every key is kept: rows that aim at their last visible key now land on the last key of all
            assert (ref["target"] == M - 1).any() or N * H < 3
    assert n_one > 0


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("B,N,H,Hkv,D,M", CASES)
def test_interval_contains_the_exact_family_reference_and_plain_f64(tab, B, N, H, Hkv, D, M, masked, f32):
    """interval() run on exact inputs contains reference()'s out on every element, for the spread and the one-hot family.  (The
    plain f64 attention need not lie inside: where an element's arg interval is a single f16 value the interval holds the
    ROUNDED exponential only.)"""
    for fam in (F.spread_inputs, F.onehot_inputs):
        q, k, v = fam(B, N, H, Hkv, D, M, M + 8)
        if f32:
            k, v = F.as_f32_caches(k, v)
        for b in range(B):
            ref = F.reference(q[b], k[b], v[b], H, Hkv, M, masked, tab, f32)
            lo, hi = F.interval(q[b], k[b], v[b], H, Hkv, M, masked, tab, f32)
            assert np.all(lo <= hi)
            assert np.all((ref["out"] >= lo) & (ref["out"] <= hi)), fam.__name__


def test_spread_family_premises(tab):
    """Scores exact in f32 forwards and backwards; rows of some hundred keys hold normal, subnormal and zero e; p v exact."""
    B, N, H, Hkv, D, M = 1, 16, 2, 1, 128, 300
    q, k, v = F.spread_inputs(B, N, H, Hkv, D, M, M + 4)
    assert np.array_equal(q, q.astype(np.float16).astype(np.float32))
    qh = q[0][:, :D].astype(np.float32)
    kh = k[0][:M, :D].astype(np.float32)
    fwd = np.zeros((N, M), np.float32)
    bwd = np.zeros((N, M), np.float32)
    for d in range(D):
        fwd += qh[:, d:d + 1] * kh[None, :, d]
        bwd += qh[:, D - 1 - d:D - d] * kh[None, :, D - 1 - d]
    s64 = qh.astype(np.float64) @ kh.astype(np.float64).T
    assert np.array_equal(fwd.astype(np.float64), s64) and np.array_equal(bwd.astype(np.float64), s64)
    _, e, _ = R.softmax_p(s64, F._n_past_for(N, M, False), F.scale_of(D), tab)
    ev = e.astype(np.float64)
    assert ((ev > 0) & (ev < 2.0 ** -14)).any() and (ev == 0).any() and (ev >= 2.0 ** -14).sum() > N


def test_unmasked_ignores_p_and_batches_are_independent(tab):
    """Unmasked: a query row's result depends on the keys alone, not on its position — rows taken alone (N = 1, another P) give
    the same out; masked they do not.  A batch entry's reference depends on that entry only."""
    B, N, H, Hkv, D, M = 2, 5, 2, 1, 32, 40
    q, k, v = F.gauss_inputs(B, N, H, Hkv, D, M, M + 8)
    full = F.plain_f64(q[0], k[0], v[0], H, Hkv, M, False)
    alone = F.plain_f64(q[0][:1], k[0], v[0], H, Hkv, M, False)
    assert np.array_equal(full[:, :1], alone)
    fm = F.plain_f64(q[0], k[0], v[0], H, Hkv, M, True)
    am = F.plain_f64(q[0][:1], k[0], v[0], H, Hkv, M, True)
    assert not np.array_equal(fm[:, :1], am)
    assert not np.array_equal(F.plain_f64(q[1], k[1], v[1], H, Hkv, M, False), full)
    lo, hi = F.interval(q[0], k[0], v[0], H, Hkv, M, False, tab)
    one = F.reference(q[0], k[0], v[0], H, Hkv, M, False, tab, exact=False)["out"]
    assert np.all((one >= lo) & (one <= hi))
    assert np.abs(one - full).max() < 2.0 ** -8  # and the rounded evaluation is the attention (p carries 2^-11, arg up to 2^-9)


def test_interval_excludes_index_mistakes(tab):
    """The interval of a Gaussian case contains the reference's evaluation of it and does not contain the same evaluation with the
    mask limit one key off either way, the mask ignored, or the heads on the other K/V head."""
    B, N, H, Hkv, D, M = 1, 17, 4, 2, 64, 65
    q, k, v = F.gauss_inputs(B, N, H, Hkv, D, M, M + 7)
    q, k, v = q[0], k[0], v[0]
    for f32 in (False, True):
        if f32:
            k, v = F.as_f32_caches(k, v)
        lo, hi = F.interval(q, k, v, H, Hkv, M, True, tab, f32)

        def outside(x):
            return int(((x < lo) | (x > hi)).sum())

        assert outside(F.reference(q, k, v, H, Hkv, M, True, tab, f32, exact=False)["out"]) == 0
        assert outside(F.reference(q, k, v, H, Hkv, M, False, tab, f32, exact=False)["out"]) > 0
        for shift in (1, -1):
            assert outside(F.reference(q, k, v, H, Hkv, M, True, tab, f32, exact=False, shift=shift)["out"]) > 0, shift
        q2 = q.reshape(N, H, D)[:, [2, 3, 0, 1]].reshape(N, H * D)  # heads 0, 1 <-> 2, 3: each reads the other K/V head
        assert outside(F.reference(q2, k, v, H, Hkv, M, True, tab, f32, exact=False)["out"][[2, 3, 0, 1]]) > 0
