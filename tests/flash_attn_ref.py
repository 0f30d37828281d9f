"""Host reference of GGML_OP_FLASH_ATTN (ggml_flash_attn, include/ggml_hip.h; kernels/flash_attn.h) for the tests: NumPy, f64
where it matters.  Not a test module (pytest collects test_*.py only).  It builds on tests/prompt_attn_ref.py — softmax_p, the
exp tables, the method of interval(), the input families — and adds what the operator has and the prompt plan's attention has
not: `masked` on or off, a batch dimension, f32 operands, any head size, and the operator's own scale 1 / sqrtf(D).

The rounding points (row (i, h, b); P = M - N; key j is kept when not masked or j <= P + i):
  f16 K/V: q -> f16; s = q . k exact products, f32 sum; v = f32(s * scale); max over the kept keys; arg = f16(f32(v - max));
           e = f16(exp(arg)) from a table; sum of e exact; inv = f32(1 / sum); p = f16(f32(e * inv)); out = sum v p in f32.
  f32 K/V: q stays f32; products of the dot rounded; p = f32(e * inv) stays f32; out = sum v p in f32, products rounded.

Layouts (what the GPU test lays out as LLaMA's graph does): q [B][N][H * D] (token-major; the node sees its permute(0, 2, 1, 3)
view), k cache [B][C][Hkv * D], v cache [B][Hkv * D][C] (transposed), C >= M, cache rows >= M NaN; out [B][H][N][D].

Every bound below is a count of roundings times 2^-24 (one rounding to nearest of an f32, relative) or its double 2^-23;
nothing is tuned against a device."""
import numpy as np

import prompt_attn_ref as R

host_exp_table = R.host_exp_table


def scale_of(D):
    """1.0f / sqrtf((float)D): what the launcher computes (both operations correctly rounded in f32)."""
    return np.float32(1.0) / np.sqrt(np.float32(D))


def kept(N, M, masked, shift=0):
    """[N][M] bool: key j of row i is kept.  masked: j <= P + i with P = M - N; else every key (P plays no part).
    shift models an index mistake for the tests of the tests: the limit moved by that many keys."""
    if not masked:
        return np.ones((N, M), bool)
    return np.arange(M)[None, :] <= (M - N) + np.arange(N)[:, None] + shift


def _n_past_for(N, M, masked, shift=0):
    """prompt_attn_ref.visible(N, T, n_past) is j <= n_past + n: n_past = P restates the mask, n_past = M keeps every key."""
    return M - N + shift if masked else M


def _operands(q, k, v, M, h, hk, D, f32):
    """Head h of q [N][E] and K/V head hk in f64: (qh [N][D], kh [M][D], vh [D][M]); q rounded to f16 unless f32."""
    qh = q[:, h * D:(h + 1) * D]
    qh = qh.astype(np.float64) if f32 else qh.astype(np.float16).astype(np.float64)
    return qh, k[:M, hk * D:(hk + 1) * D].astype(np.float64), v[hk * D:(hk + 1) * D, :M].astype(np.float64)


def softmax_p32(s, N, M, masked, scale, tab, shift=0):
    """prompt_attn_ref.softmax_p with p left in f32 (the f32 routine): p = f32(e * inv), dropped entries zero."""
    vis = kept(N, M, masked, shift)
    _, e, _ = R.softmax_p(s, _n_past_for(N, M, masked, shift), scale, tab)
    ssum = e.astype(np.float64).sum(axis=1, keepdims=True)
    inv = (1.0 / ssum).astype(np.float32)
    p = (e.astype(np.float32) * inv).astype(np.float32)
    return np.where(vis, p, np.float32(0))


def reference(q, k, v, H, Hkv, M, masked, tab, f32=False, exact=True, shift=0):
    """One batch entry, inputs whose scores are exact in f32 in any order (the exact families): P is predicted bit for bit.
    exact=False takes arbitrary inputs: the f64 scores rounded to f32 are then ONE of the values the device may compute (a
    point inside interval(), not a prediction); shift: see kept().
    q [N][H D], k [C][Hkv D], v [Hkv D][C].  Returns out [H][N][D] f64 = V . p in f64; bound [H][N][D]; target [H][N] = the key
    a row puts its whole weight on (p is one 1.0 and zeros), else -1.
    bound: f16 K/V: the products v p are exact in f32 (11 x 11 significant bits), M - 1 additions, each rounded by at most 2^-24
    relative to a partial sum that is at most sum |v| p (1 + 2^-24)^M: M 2^-23 sum |v| p is more than twice that count.
    f32 K/V: p has 24 significant bits, so each of the M products is rounded as well: 2 M - 1 roundings of 2^-24 — below the
    same M 2^-23 sum |v| p."""
    N = q.shape[0]
    D, r = q.shape[1] // H, H // Hkv
    scale = scale_of(D)
    out = np.zeros((H, N, D))
    bound = np.zeros((H, N, D))
    target = np.full((H, N), -1, np.int64)
    for h in range(H):
        qh, kh, vh = _operands(q, k, v, M, h, h // r, D, f32)
        s = qh @ kh.T
        assert not exact or np.array_equal(s.astype(np.float32).astype(np.float64), s), "scores must be exact in f32 here"
        s = s.astype(np.float32).astype(np.float64)
        if f32:
            p = softmax_p32(s, N, M, masked, scale, tab, shift)
        else:
            p = R.softmax_p(s, _n_past_for(N, M, masked, shift), scale, tab)[0]
        pf = p.astype(np.float64)
        out[h] = pf @ vh.T
        bound[h] = M * 2.0 ** -23 * (pf @ np.abs(vh).T)
        one = ((p != 0).sum(axis=1) == 1) & ((p == 1).sum(axis=1) == 1)
        target[h, one] = np.argmax(p, axis=1)[one]
    return dict(out=out, bound=bound, target=target)


def interval(q, k, v, H, Hkv, M, masked, tab, f32=False):
    """prompt_attn_ref.interval's method for the operator: per-element [lo, hi] that the device's out must lie in for ARBITRARY
    inputs.  Scores: f16 K/V: exact products, D - 1 additions: ds = D 2^-23 sum |q||k| (twice the count);  f32 K/V: D products
    and D - 1 additions, 2 D - 1 roundings of 2^-24: below the same ds.  Scaled: one more rounding.  From there every step is
    monotone: the row maximum lies between the maxima of the ends, arg between the f16 roundings of the ends of v - max, e
    between the table's monotone envelopes, sum / inv / p between what the ends give (p rounded to f16, or left in f32), out
    between the sign-aware sums over [p_lo, p_hi] widened by reference()'s accumulation term on p_hi.
    Returns lo, hi [H][N][D] f64."""
    N = q.shape[0]
    D, r = q.shape[1] // H, H // Hkv
    t16 = np.ascontiguousarray(tab, np.uint16).view(np.float16)
    tm = t16[0x8000 | np.arange(0x7C01)].astype(np.float64)  # by magnitude: 0, -2^-24, ..., -inf
    e_min = np.minimum.accumulate(tm)
    e_max = np.maximum.accumulate(tm[::-1])[::-1]
    vis = kept(N, M, masked)
    sc = float(scale_of(D))
    lo = np.zeros((H, N, D))
    hi = np.zeros((H, N, D))
    for h in range(H):
        qh, kh, vh = _operands(q, k, v, M, h, h // r, D, f32)
        vt = (qh @ kh.T) * sc
        ds = D * 2.0 ** -23 * (np.abs(qh) @ np.abs(kh).T) * sc
        dv = ds + (np.abs(vt) + ds) * 2.0 ** -24
        v_lo = np.where(vis, vt - dv, -np.inf)
        v_hi = np.where(vis, vt + dv, -np.inf)
        mx_lo = v_lo.max(axis=1, keepdims=True)
        mx_hi = v_hi.max(axis=1, keepdims=True)
        d_lo = np.where(vis, v_lo - mx_hi, 0.0).astype(np.float32)
        d_hi = np.minimum(np.where(vis, v_hi - mx_lo, 0.0), 0.0).astype(np.float32)
        with np.errstate(over="ignore"):
            a_lo, a_hi = d_lo.astype(np.float16), d_hi.astype(np.float16)
        m_lo = (a_lo.view(np.uint16) & 0x7FFF).astype(np.int64)
        m_hi = (a_hi.view(np.uint16) & 0x7FFF).astype(np.int64)
        e_lo = np.where(vis, e_min[m_lo], 0.0)
        e_hi = np.where(vis, e_max[m_hi], 0.0)
        inv_lo = (1.0 / e_hi.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
        inv_hi = (1.0 / e_lo.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
        p_lo, p_hi = (e_lo * inv_lo).astype(np.float32), (e_hi * inv_hi).astype(np.float32)
        if not f32:
            p_lo, p_hi = p_lo.astype(np.float16), p_hi.astype(np.float16)
        p_lo, p_hi = p_lo.astype(np.float64), p_hi.astype(np.float64)
        vp, vn = np.maximum(vh, 0.0), np.minimum(vh, 0.0)
        acc = M * 2.0 ** -23 * (p_hi @ np.abs(vh).T)
        lo[h] = p_lo @ vp.T + p_hi @ vn.T - acc
        hi[h] = p_hi @ vp.T + p_lo @ vn.T + acc
    return lo, hi


def plain_f64(q, k, v, H, Hkv, M, masked, f32=False):
    """The attention in f64 with only the operand roundings (q -> f16 unless f32; p -> f16 unless f32): [H][N][D]."""
    N = q.shape[0]
    D, r = q.shape[1] // H, H // Hkv
    vis = kept(N, M, masked)
    out = np.zeros((H, N, D))
    for h in range(H):
        qh, kh, vh = _operands(q, k, v, M, h, h // r, D, f32)
        s = np.where(vis, (qh @ kh.T) * float(scale_of(D)), -np.inf)
        e = np.exp(s - s.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
        p = p.astype(np.float32 if f32 else np.float16).astype(np.float64)
        out[h] = p @ vh.T
    return out


# ---- input families: prompt_attn_ref's, per batch entry, for the operator's scale.  Each returns q [B][N][E] f32,
# k [B][C][Eg] f16, v [B][Eg][C] f16 with cache rows >= M NaN.
def onehot_a(D):
    """prompt_attn_ref.onehot_inputs' `a` for scale 1 / sqrt(D): adjacent keys differ by a * scale >= 20 (one e is 1, the rest
    0: asserted on the table by the tests), a multiple of 32.  D = 64: 160, the value its own scale 1/8 uses."""
    return 32 * int(np.ceil(20.0 * np.sqrt(D) / 32.0))


def onehot_inputs(B, N, H, Hkv, D, M, C):
    parts = [R.onehot_inputs(N, H, Hkv, D, M - N, C, a=onehot_a(D), seed=b)[:3] for b in range(B)]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3))


SPREAD_M = 15


def spread_inputs(B, N, H, Hkv, D, M, C, seed=0):
    """prompt_attn_ref.spread_inputs' recipe with the entry range chosen for scale 1 / sqrt(D) instead of 1 / 2: Q and K entries
    are multiples of 1/4 with |x| <= 15/4, so every product is a multiple of 1/16 and every partial sum, in any order, an integer
    number of sixteenths below D 15^2 < 2^24 — exact in f32.  The scaled scores have a standard deviation of m (m + 1) / 48 = 5
    for every D, so a row of some hundred keys spans about 0 to -25 below its maximum: e covers normals, f16 subnormals and
    zeros.  V entries multiples of 1/8 with |v| <= 2: each p v is exact in f32 for an f16 p."""
    assert D * SPREAD_M ** 2 < 2 ** 24
    m = SPREAD_M
    E, Eg = H * D, Hkv * D
    rng = np.random.default_rng([seed, B, N, H, D, M, 1])
    k = np.full((B, C, Eg), np.nan, np.float16)
    v = np.full((B, Eg, C), np.nan, np.float16)
    q = (rng.integers(-m, m + 1, (B, N, E)) / 4.0).astype(np.float32)
    k[:, :M] = (rng.integers(-m, m + 1, (B, M, Eg)) / 4.0).astype(np.float16)
    v[:, :, :M] = (rng.integers(-16, 17, (B, Eg, M)) / 8.0).astype(np.float16)
    return q, k, v


def gauss_inputs(B, N, H, Hkv, D, M, C):
    parts = [R.gauss_inputs(N, H, Hkv, D, M - N, C, seed=b) for b in range(B)]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3))


def as_f32_caches(k, v):
    """The same values as f32 caches (the f32 routine's operands); NaN rows stay NaN."""
    return k.astype(np.float32), v.astype(np.float32)
