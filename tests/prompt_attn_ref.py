"""Host reference of the prompt batch attention (plan_prompt.inc prompt_attention: kernels/prompt_attn.h k_p_attn, and the
three-launch path k_gemm_f16 / k_p_soft_max / k_gemm_f16_b16) for the tests, NumPy with f64 where it matters, plus the three
input families the tests run it on.  Not a test module (pytest collects test_*.py only).

The reference restates ggml's rounding points as both device paths document them (crates/models/llama/src/lib.rs:246-299):
q -> f16;  s = q . k;  v = f32(s * scale);  row n sees keys j <= n_past + n;  row max;  arg = f16(f32(v - max));
e = f16(exp(arg));  sum of e in f64;  inv = f32(1 / sum);  p = f16(f32(e * inv)), zero behind the limit;  out = V . p.
The build uses -ffp-contract=off: the multiply and the subtraction round separately.  e(arg) is a function of an f16 and is
taken from a TABLE of 65536 f16 bit patterns indexed by arg's bits: the device's own (ggml_hip_debug_exp_le0, which
test_prompt_plan_gpu.py holds to f64 exp exhaustively) on the GPU, the C library's expf (what the oracle executes) on the host.

Layouts are the device hook's: q [N][E] f32, k [C][Egqa] f16 (token-major), v [Egqa][C] f16 (transposed), out [N][E]."""
import ctypes
import ctypes.util

import numpy as np

PATTN_Q = 32
LDS_LIMIT = 150 * 1024
F16_MAX = 65504.0


# ---- the launcher's choice of queries per workgroup (plan_shapes.inc prompt_attn_row_bytes / prompt_attn_queries), restated
def row_bytes(T):
    return ((T + 63) & ~63) * 4 + 16


def queries_per_workgroup(D, T):
    """32, 16 (long rows), or 0 = the fused kernel refuses the shape."""
    if D not in (32, 64, 128):
        return 0
    if PATTN_Q * row_bytes(T) <= LDS_LIMIT:
        return PATTN_Q
    if 16 * row_bytes(T) <= LDS_LIMIT:
        return 16
    return 0


def boundaries(D=128):
    """(last T on 32 queries per workgroup, last T the fused kernel takes), derived from the functions above."""
    t32 = max(t for t in range(1, 4096) if queries_per_workgroup(D, t) == 32)
    t16 = max(t for t in range(1, 4096) if queries_per_workgroup(D, t) == 16)
    return t32, t16


# ---- exp tables
def host_exp_table():
    """f16(expf(x)) for all 65536 f16 bit patterns x with the C library's expf: orc_scale_mask_softmax's expression."""
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    m.expf.restype = ctypes.c_float
    m.expf.argtypes = [ctypes.c_float]
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)
    y = np.array([m.expf(float(v)) for v in x], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return y.astype(np.float16).view(np.uint16)


def _tab16(tab):
    return np.ascontiguousarray(tab, np.uint16).view(np.float16)


# ---- the reference
def head_scores(q, k, T, h, hk, D):
    """q . k of head h against K/V head hk in f64 (exact whenever every partial sum fits 53 bits): [N][T]."""
    qh = q[:, h * D:(h + 1) * D].astype(np.float16).astype(np.float64)
    kh = k[:T, hk * D:(hk + 1) * D].astype(np.float64)
    return qh @ kh.T


def visible(N, T, n_past):
    return np.arange(T)[None, :] <= n_past + np.arange(N)[:, None]


def softmax_p(s, n_past, scale, tab):
    """Rows of scores s [N][T] (values an f32 holds exactly) -> (p f16 [N][T], e f16, arg f16), masked entries zero."""
    N, T = s.shape
    vis = visible(N, T, n_past)
    v = s.astype(np.float32) * np.float32(scale)
    mx = np.where(vis, v, -np.inf).max(axis=1, keepdims=True).astype(np.float32)
    d = np.where(vis, v - mx, np.float32(0)).astype(np.float32)
    with np.errstate(over="ignore"):
        arg = d.astype(np.float16)  # below -65520: -inf
    e = np.where(vis, _tab16(tab)[arg.view(np.uint16)], np.float16(0))
    ssum = e.astype(np.float64).sum(axis=1, keepdims=True)  # exact: f16-valued terms
    inv = (1.0 / ssum).astype(np.float32)
    p = (e.astype(np.float32) * inv).astype(np.float16)
    return np.where(vis, p, np.float16(0)), e, np.where(vis, arg, np.float16(0))


def reference(q, k, v, H, Hkv, n_past, scale, tab, keep=False):
    """The attention of the batch with P predicted exactly (inputs whose scores are exact in f32 in any order).
    Returns dict: out [N][E] f64 = V . p in f64;  bound [N][E] = T * 2^-23 * sum_j |v_j| p_j (the free f32 accumulation of
    V . P: T - 1 additions, each rounded by at most 2^-23 relative, the products p * v exact);  target [N][H] = the key a row
    puts its whole weight on (p is one 1.0 and zeros), else -1;  with keep: p / e / arg per head."""
    N, E = q.shape
    D, r, T = E // H, H // Hkv, n_past + N
    out = np.zeros((N, E))
    bound = np.zeros((N, E))
    target = np.full((N, H), -1, np.int64)
    kept = []
    for h in range(H):
        hk = h // r
        p, e, arg = softmax_p(head_scores(q, k, T, h, hk, D), n_past, scale, tab)
        pf = p.astype(np.float64)
        vh = v[hk * D:(hk + 1) * D, :T].astype(np.float64)
        out[:, h * D:(h + 1) * D] = pf @ vh.T
        bound[:, h * D:(h + 1) * D] = T * 2.0 ** -23 * (pf @ np.abs(vh).T)
        one = ((p != 0).sum(axis=1) == 1) & ((p == 1).sum(axis=1) == 1)
        target[one, h] = np.argmax(p, axis=1)[one]
        if keep:
            kept.append((p, e, arg))
    return dict(out=out, bound=bound, target=target, heads=kept)


def interval(q, k, v, H, Hkv, n_past, scale, tab):
    """Per-element interval [lo, hi] that the device's out must lie in for ARBITRARY inputs (family (c)).  The f32 scores carry
    ds = D * 2^-23 * sum|q||k| (D - 1 additions and the products' exactness: f16 x f16 fits an f32) and, scaled, one more rounding;
    the row maximum lies between the maxima of the ends; arg between the f16 roundings of the ends of v - max; e between the
    table's values over that range (its monotone envelopes: running minimum / maximum, equal to the table wherever it is
    monotone); the sum, inv and p between what those ends give (every step is monotone); out between the sign-aware sums over
    [p_lo, p_hi], widened by the accumulation term of reference().  Counts "edges": visible elements whose arg or p interval holds
    more than one f16 value.  Returns lo, hi [N][E] f64 and the counts."""
    N, E = q.shape
    D, r, T = E // H, H // Hkv, n_past + N
    t16 = _tab16(tab)
    tm = t16[0x8000 | np.arange(0x7C01)].astype(np.float64)  # by magnitude: 0, -2^-24, ..., -inf
    e_min = np.minimum.accumulate(tm)              # least value over [arg, 0]
    e_max = np.maximum.accumulate(tm[::-1])[::-1]  # greatest value over [-inf, arg]
    vis = visible(N, T, n_past)
    sc = float(np.float32(scale))
    lo = np.zeros((N, E))
    hi = np.zeros((N, E))
    edges = dict(arg=0, p=0, visible=int(vis.sum()) * H)
    for h in range(H):
        hk = h // r
        qh = q[:, h * D:(h + 1) * D].astype(np.float16).astype(np.float64)
        kh = k[:T, hk * D:(hk + 1) * D].astype(np.float64)
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
        p_lo16 = (e_lo * inv_lo).astype(np.float32).astype(np.float16)
        p_hi16 = (e_hi * inv_hi).astype(np.float32).astype(np.float16)
        edges["arg"] += int((vis & (m_lo != m_hi)).sum())
        edges["p"] += int((vis & (p_lo16 != p_hi16)).sum())
        p_lo, p_hi = p_lo16.astype(np.float64), p_hi16.astype(np.float64)
        vh = v[hk * D:(hk + 1) * D, :T].astype(np.float64)
        vp, vn = np.maximum(vh, 0.0), np.minimum(vh, 0.0)
        acc = T * 2.0 ** -23 * (p_hi @ np.abs(vh).T)
        lo[:, h * D:(h + 1) * D] = p_lo @ vp.T + p_hi @ vn.T - acc
        hi[:, h * D:(h + 1) * D] = p_hi @ vp.T + p_lo @ vn.T + acc
    return lo, hi, edges


def plain_f64(q, k, v, H, Hkv, n_past, scale, limit_shift=0, drop_key=None, wrong_head=None):
    """The attention in f64 with only the operand roundings (q -> f16, p -> f16): the value every interval must contain.
    limit_shift: row n sees keys j <= n_past + n + limit_shift;  drop_key: that key is left out of every row that sees it;
    wrong_head = (h, hk): head h reads K/V head hk.  Each models one index mistake of a kernel."""
    N, E = q.shape
    D, r, T = E // H, H // Hkv, n_past + N
    out = np.zeros((N, E))
    vis = np.arange(T)[None, :] <= np.minimum(n_past + np.arange(N)[:, None] + limit_shift, T - 1)
    if drop_key is not None:
        vis = vis & (np.arange(T)[None, :] != drop_key)
    for h in range(H):
        hk = h // r
        if wrong_head is not None and wrong_head[0] == h:
            hk = wrong_head[1]
        s = head_scores(q, k, T, h, hk, D) * float(np.float32(scale))
        s = np.where(vis, s, -np.inf)
        e = np.exp(s - s.max(axis=1, keepdims=True))
        p = (e / e.sum(axis=1, keepdims=True)).astype(np.float16).astype(np.float64)
        out[:, h * D:(h + 1) * D] = p @ v[hk * D:(hk + 1) * D, :T].astype(np.float64).T
    return out


# ---- input families.  Every generator returns (q [N][E] f32, k [C][Egqa] f16, v [Egqa][C] f16, ...); K and V rows >= T are
# NaN (an unwritten cache must not matter) and rows between a query's limit and T hold the next tokens' real values.
def _cache(C, Eg):
    return np.full((C, Eg), np.nan, np.float16), np.full((Eg, C), np.nan, np.float16)


def _normal_f16(rng, shape):
    """N(0,1) as f16 without subnormals or zeros (whether the matrix cores keep f16 subnormal INPUTS is not a premise here)."""
    x = rng.standard_normal(shape).astype(np.float16)
    x[np.abs(x) < np.float16(2.0 ** -14)] = np.float16(1.0)
    return x


def indicator_keys(T, n_past, D):
    """The keys that get a spare K dimension of their own: tile and chunk borders, the last key, the first new one."""
    last_tile = ((T - 1) // 32) * 32
    want = [31, 32, 63, 64, 511, 512, 15, 16, T - 1, last_tile, last_tile - 1, n_past, n_past - 1, 1, 7, 8, 1151, 1152]
    keys = []
    for j in want:
        if 0 <= j < T and j not in keys:
            keys.append(j)
    return keys[:D - 2]


ONEHOT_SCALE = 0.125


def onehot_inputs(N, H, Hkv, D, n_past, C, a=160, seed=0):
    """Family (a).  k_j = [j mod 64, j div 64, indicators...], scale 1/8.  Row (n, h) by (n + h) mod 3:
       0: q = +[a, 64 a, 0..]: score a j / 8 — the maximum on the row's LAST visible key, the first masked key higher still;
       1: q = -[a, 64 a, 0..]: the maximum on key 0;
       2: q = a on the spare dimension of one indicator key: that key if the row sees it, else every visible score ties at 0
          (p = f16(f32(1 / L)) on L keys: family (b)'s check) and the masked indicator key is the bait.
    Adjacent keys differ by a / 8 >= 20 after scaling, so one e is 1 and the rest are 0 (asserted on the table by the tests).
    All operands are f16-exact and every score is an integer below 2^24: exact in f32 in any order.  a = 320 (640) makes
    f32(v - max) pass -65504 from 1638 (819) keys on: arg is f16 -inf.  Returns q, k, v, want [N][H]: the key, or -1 for a tie."""
    assert a % 32 == 0 and 64 * a <= 40960 and a * max(n_past + N, 1) < 2 ** 24
    rng = np.random.default_rng([seed, N, H, D, n_past])
    E, Eg, T = H * D, Hkv * D, n_past + N
    k, v = _cache(C, Eg)
    j = np.arange(T)
    keys = indicator_keys(T, n_past, D)
    kh = np.zeros((T, D), np.float16)
    kh[:, 0] = j % 64
    kh[:, 1] = j // 64
    for i, key in enumerate(keys):
        kh[key, 2 + i] = 1
    for hk in range(Hkv):
        k[:T, hk * D:(hk + 1) * D] = kh
    v[:, :T] = _normal_f16(rng, (Eg, T))
    q = np.zeros((N, E), np.float32)
    want = np.zeros((N, H), np.int64)
    for n in range(N):
        for h in range(H):
            mode = (n + h) % 3
            if mode == 0:
                q[n, h * D], q[n, h * D + 1], want[n, h] = a, 64 * a, n_past + n
            elif mode == 1:
                q[n, h * D], q[n, h * D + 1], want[n, h] = -a, -64 * a, 0
            else:
                i = (5 * n + 3 * h) % len(keys) if keys else 0
                if keys:
                    q[n, h * D + 2 + i] = a
                want[n, h] = keys[i] if keys and keys[i] <= n_past + n else (0 if n_past + n == 0 else -1)
    return q, k, v, want


SPREAD_M = {32: 8, 64: 7, 128: 6}  # entries are integers in [-m, m] times 1/4
SPREAD_SCALE = 0.5


def spread_inputs(N, H, Hkv, D, n_past, C, seed=0):
    """Family (b).  Q and K entries multiples of 1/4 with |x| <= m / 4 <= 2: every product is a multiple of 1/16 and every
    partial sum, in any order, an integer number of sixteenths below 2^24 — exact in f32.  With scale 1/2 the scaled scores
    have a standard deviation of sqrt(D) m (m + 1) / 96 ~ 4.5 .. 5, so a row of some hundred keys spans about 0 to -25 below
    its maximum: e covers normals, f16 subnormals (arg below -9.7) and zeros (below -17.4).  V entries multiples of 1/8 with
    |v| <= 2: each p * v is exact in f32."""
    m = SPREAD_M[D]
    rng = np.random.default_rng([seed, N, H, D, n_past, 1])
    E, Eg, T = H * D, Hkv * D, n_past + N
    k, v = _cache(C, Eg)
    q = (rng.integers(-m, m + 1, (N, E)) / 4.0).astype(np.float32)
    k[:T] = (rng.integers(-m, m + 1, (T, Eg)) / 4.0).astype(np.float16)
    v[:, :T] = (rng.integers(-16, 17, (Eg, T)) / 8.0).astype(np.float16)
    return q, k, v


def gauss_inputs(N, H, Hkv, D, n_past, C, seed=0):
    """Family (c): N(0,1) operands as in test_fused_prompt_attention_kernel_matches_the_three_launch_path; scale 1 / sqrt(D)."""
    rng = np.random.default_rng([seed, N, H, D, n_past, 2])
    E, Eg, T = H * D, Hkv * D, n_past + N
    k, v = _cache(C, Eg)
    q = rng.standard_normal((N, E)).astype(np.float32)
    k[:T] = rng.standard_normal((T, Eg)).astype(np.float16)
    v[:, :T] = _normal_f16(rng, (Eg, T))
    return q, k, v


# ---- the plan form: RoPE while Q is staged, K-split partials, the Q8 re-quantizing epilogue
def rope_table_quarter_turns(N, D, seed=0):
    """[N][128] f32 in k_rope_table's layout ((cos, sin) of pair kk of token n at [n][2 kk], [n][2 kk + 1]) with every angle a
    multiple of a quarter turn: rotating by it is exact."""
    rng = np.random.default_rng([seed, N, D, 3])
    cs = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)], np.float32)[rng.integers(0, 4, (N, 64))]
    tab = cs.reshape(N, 128).copy()
    tab[:, D:] = np.nan  # pairs beyond the head: never read
    return tab


def rope_table_real(N, D, n_past, freq_base=10000.0):
    theta = (n_past + np.arange(N))[:, None] * freq_base ** (-2.0 * np.arange(64)[None, :] / D)
    tab = np.stack([np.cos(theta), np.sin(theta)], axis=2).astype(np.float32).reshape(N, 128)
    tab[:, D:] = np.nan
    return tab


def rotate(q, tab, H, inverse=False):
    """k_p_attn's staging arithmetic in f32, each operation rounded on its own: (x0, x1) of pair kk of every head ->
    (x0 c - x1 s, x0 s + x1 c) with (c, s) = tab[n][2 kk], tab[n][2 kk + 1]; inverse: the rotation by -angle."""
    N, E = q.shape
    D = E // H
    x = q.reshape(N, H, D // 2, 2).astype(np.float32)
    c = tab[:, None, 0:D:2]
    s = tab[:, None, 1:D:2]
    if inverse:
        s = -s
    x0, x1 = x[..., 0], x[..., 1]
    o = np.stack([x0 * c - x1 * s, x0 * s + x1 * c], axis=3).astype(np.float32)
    return o.reshape(N, E)


def kperm_inv(e):
    """kernels/mmq.h mmq_kperm_inv: element e (0..31) of a block -> its position in the GEMM's k order."""
    h, k, i = e >> 4, (e & 15) >> 2, e & 3
    return 8 * k + 4 * h + (((i & 1) << 1) | (i >> 1))


def requant_x16(out, f16d, scalar=False):
    """What the epilogue makes of the f32 attention output [N][E]: per 32-channel block amax, d = amax / 127, id = 127 / amax
    (scalar: 1 / d), q = rint(v * id) (scalar: roundf), d rounded to f16 first when f16d, f16(clamp(d * q, +-65504)) stored at
    kperm_inv(channel).  f32 arithmetic, each operation rounded on its own.  Returns the f16 BITS [N][E]."""
    N, E = out.shape
    x = np.ascontiguousarray(out, np.float32).reshape(N, E // 32, 32)
    amax = np.abs(x).max(axis=2, keepdims=True)
    d = amax / np.float32(127.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        if scalar:
            idv = np.where(d != 0, np.float32(1.0) / d, np.float32(0)).astype(np.float32)
        else:
            idv = np.where(amax != 0, np.float32(127.0) / amax, np.float32(0)).astype(np.float32)
    y = (x * idv).astype(np.float32)
    if scalar:  # roundf: half away from zero
        t = np.trunc(y)
        qv = t + np.where(np.abs(y - t) >= 0.5, np.sign(y), 0.0).astype(np.float32)
    else:
        qv = np.rint(y)
    qv = qv.astype(np.int32)  # the code is an integer: a rounded -0.3 is 0, not -0
    dq = d.astype(np.float16).astype(np.float32) if f16d else d
    rq = np.clip((dq * qv.astype(np.float32)).astype(np.float32), -F16_MAX, F16_MAX).astype(np.float16)
    res = np.empty((N, E // 32, 32), np.float16)
    res[:, :, [kperm_inv(e) for e in range(32)]] = rq
    return res.reshape(N, E).view(np.uint16)
