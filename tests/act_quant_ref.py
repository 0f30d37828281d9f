"""Plain NumPy restatements of ggml's activation quantizers, and the input sets the quantizer tests run on.

Every quantized mat-vec and GEMM of the device multiplies by an activation row that a kernel has re-quantized first: to Q8_0 /
Q8_1 blocks of 32 (ggml's quantize_row_q8_0 / _q8_1: the AVX2 branch `id = 127 / amax`, round half to even, is the default,
option act_quant = 0; the scalar branch `id = 1 / d`, roundf, is act_quant = 1) or to Q8_K super-blocks of 256
(quantize_row_q8_K: the FIRST value of largest magnitude gives iscale = -128 / max, q = min(127, nearest_int(iscale * x)),
d = 1 / iscale, sums over 16).  The functions here state that arithmetic once more, in f32 NumPy operations, with every
decision a kernel could get wrong as a parameter — so the same function is the reference and, with one parameter changed, a
mutant the input sets must tell from it (tests/test_act_quant_ref.py).  tests/test_act_quant_gpu.py compares the kernels with
these references byte for byte.

Forms: planar Q8 (quants, d, integer sum), the f16 GEMM operand f16(clamp(dq * q, +-65504)) in the GEMM's k order (dq = d after
its f16 round trip for the Q8_0 kind), and Q8_K (quants, d, bsums) with its f16 operand.

Left out of the input sets: NaN and inf; blocks with 0 < amax < 2^-100, where 127 / amax overflows and ggml defines nothing."""
import math

import numpy as np

F = np.float32
F16_MAX = F(65504.0)


# ---- rounding ----------------------------------------------------------------------------------------------------------
def _round_even(v):
    return np.rint(v).astype(np.int64)  # nearbyintf / lrintf / v_rndne_f32 in the default rounding mode


def _round_away(v):
    v64 = v.astype(np.float64)  # |v| + 0.5 is exact in f64
    return (np.sign(v64) * np.floor(np.abs(v64) + 0.5)).astype(np.int64)  # roundf


def round_f16(d, trunc=False):
    """f32 -> f16 -> f32: round to nearest even as ggml_fp32_to_fp16; trunc: toward zero (a mutant)."""
    d = np.asarray(d, F)
    h = d.astype(np.float16)
    if trunc:
        over = np.abs(h.astype(F)) > np.abs(d)
        h = np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)
    return h.astype(F)


# ---- Q8_0 / Q8_1 -------------------------------------------------------------------------------------------------------
def q8(x, branch, f16d, rounding=None, mult=None, d16_trunc=False, sum_half=None):
    """x [..., 32 n] f32 -> (q int8 [nblk][32], d f32 [nblk] as the kind stores it, sum int32 [nblk]).
    branch 0: id = 127 / amax, half to even; 1: id = 1 / d, half away.  f16d: d stored after its f16 round trip (Q8_0); the
    multiplier always comes from the unrounded values.  Mutants: rounding 'even' / 'away', mult '127/amax' / '1/d' / '1/d16'
    (from the f16-rounded d), d16_trunc, sum_half 0 / 1 (the sum of one half only)."""
    xb = np.ascontiguousarray(x, F).reshape(-1, 32)
    amax = np.max(np.abs(xb), axis=1).astype(F)
    d = (amax / F(127.0)).astype(F)
    rounding = rounding or ("even" if branch == 0 else "away")
    mult = mult or ("127/amax" if branch == 0 else "1/d")
    with np.errstate(divide="ignore", invalid="ignore"):
        if mult == "127/amax":
            inv = np.where(amax != 0, F(127.0) / amax, F(0)).astype(F)
        elif mult == "1/d":
            inv = np.where(d != 0, F(1.0) / d, F(0)).astype(F)
        else:
            d16 = round_f16(d)
            inv = np.where(d16 != 0, F(1.0) / d16, F(0)).astype(F)
    v = (xb * inv[:, None]).astype(F)
    qi = _round_even(v) if rounding == "even" else _round_away(v)
    q = qi.astype(np.int8)
    qs = q.astype(np.int32)
    s = qs.sum(axis=1) if sum_half is None else qs[:, 16 * sum_half:16 * sum_half + 16].sum(axis=1)
    return q, (round_f16(d, d16_trunc) if f16d else d), s.astype(np.int32)


def q8_bytes(x, branch, f16d):
    """The raw ggml blocks (block_q8_0: f16 d, 32 quants; block_q8_1: f32 d, f32 s = d * sum, 32 quants)."""
    q, d, s = q8(x, branch, f16d)
    n = q.shape[0]
    if f16d:
        out = np.zeros((n, 34), np.uint8)
        out[:, :2] = d.astype(np.float16).view(np.uint8).reshape(n, 2)
        out[:, 2:] = q.view(np.uint8)
    else:
        out = np.zeros((n, 40), np.uint8)
        out[:, :4] = d.view(np.uint8).reshape(n, 4)
        out[:, 4:8] = (d * s.astype(F)).astype(F).view(np.uint8).reshape(n, 4)
        out[:, 8:] = q.view(np.uint8)
    return out.reshape(-1)


def planar(q):
    """q [nblk][32] -> (lo [nblk][16], hi [nblk][16]): elements 0 .. 15 and 16 .. 31 of every block (the mat-vecs' layout)."""
    return np.ascontiguousarray(q[:, :16]), np.ascontiguousarray(q[:, 16:])


def tables(v, rows, nblk):
    """v [rows * nblk] (d or sum, row-major) -> the [ceil(rows / 8)][nblk][8] tables k_mmq_cols stages: row r in column r % 8 of
    table r / 8.  Returns the tables and the mask of the entries that belong to a row (the others are never written)."""
    ntab = (rows + 7) // 8
    t = np.zeros((ntab, nblk, 8), v.dtype)
    m = np.zeros((ntab, nblk, 8), bool)
    vv = v.reshape(rows, nblk)
    for r in range(rows):
        t[r // 8, :, r % 8] = vv[r]
        m[r // 8, :, r % 8] = True
    return t, m


# ---- the GEMM's k order (kernels/mmq.h) -----------------------------------------------------------------------------------
def kperm():
    """Position p (0 .. 31) of the permuted order inside a block -> element index of the ggml block: with k = p / 8, j = p % 8,
    jj = j % 4 it is 4 k + {0, 2, 1, 3}[jj], plus 16 when j >= 4 (the order the weights' nibble trick produces)."""
    return np.array([4 * (p >> 3) + (0, 2, 1, 3)[p & 3] + (16 if p & 4 else 0) for p in range(32)])


def permute(v, identity=False):
    """v [..., 32 n] in ggml's element order -> the GEMM's k order inside every 32."""
    b = v.reshape(-1, 32)
    return (b if identity else b[:, kperm()]).reshape(v.shape)


def f16_operand(q, dq, identity=False):
    """f16(clamp(dq * q, +-65504)) per block, permuted: uint16 bits [nblk * 32].  dq: the scale the kind multiplies with."""
    r = (np.asarray(dq, F)[:, None] * q.astype(F)).astype(F)
    r = np.minimum(np.maximum(r, -F16_MAX), F16_MAX)
    return permute(r.astype(np.float16), identity).view(np.uint16).reshape(-1)


def q8_f16(x, branch, f16d, **mut):
    identity = mut.pop("identity", False)
    q, d, _ = q8(x, branch, f16d, **mut)
    return f16_operand(q, d, identity)


def w16(x, identity=False):
    """k_f32_to_w16: f16(clamp(x)) in the k order."""
    v = np.minimum(np.maximum(np.ascontiguousarray(x, F).reshape(-1), -F16_MAX), F16_MAX)
    return permute(v.astype(np.float16), identity).view(np.uint16)


# ---- Q8_K ------------------------------------------------------------------------------------------------------------------
def q8k(x, extreme="first", signed=True, clamp=True, bsum="rows"):
    """x [..., 256 n] -> (q int8 [nsb][256], d f32 [nsb], bsums int16 [nsb][16]).  Mutants: extreme 'last', signed False (|max|),
    clamp False, bsum 'cols' (sixteen strided elements instead of sixteen consecutive ones)."""
    xb = np.ascontiguousarray(x, F).reshape(-1, 256)
    ax = np.abs(xb)
    amax = ax.max(axis=1)
    hit = ax == amax[:, None]
    idx = hit.argmax(axis=1) if extreme == "first" else 255 - hit[:, ::-1].argmax(axis=1)
    mx = xb[np.arange(xb.shape[0]), idx]
    if not signed:
        mx = np.abs(mx)
    nz = amax != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        iscale = np.where(nz, F(-128.0) / np.where(nz, mx, F(1)), F(0)).astype(F)
        d = np.where(nz, F(1.0) / np.where(nz, iscale, F(1)), F(0)).astype(F)
    qi = _round_even((iscale[:, None] * xb).astype(F))
    if clamp:
        qi = np.minimum(qi, 127)
    q = qi.astype(np.int8)
    g = q.astype(np.int32).reshape(-1, 16, 16)
    bs = g.sum(axis=2) if bsum == "rows" else g.sum(axis=1)
    return q, d, bs.astype(np.int16)


def q8k_bytes(x):
    """block_q8_K: f32 d, 256 quants, 16 int16 sums."""
    q, d, bs = q8k(x)
    n = q.shape[0]
    out = np.zeros((n, 292), np.uint8)
    out[:, :4] = d.view(np.uint8).reshape(n, 4)
    out[:, 4:260] = q.view(np.uint8)
    out[:, 260:] = bs.view(np.uint8).reshape(n, 32)
    return out.reshape(-1)


def q8k_f16(x, identity=False, **mut):
    q, d, _ = q8k(x, **mut)
    r = (d[:, None] * q.astype(F)).astype(F)
    r = np.minimum(np.maximum(r, -F16_MAX), F16_MAX)
    return permute(r.astype(np.float16), identity).view(np.uint16).reshape(-1)


# ---- rms_norm * w ----------------------------------------------------------------------------------------------------------
def norm_mean(x):
    """The f32 mean of squares of one row, from the exactly rounded f64 sum of the f32 squares, and its relative distance (in
    f64, of the quotient) from the nearest f32 rounding midpoint.  The kernels add the same f32 squares in f64 in a thread
    order; their sum is within a few f64 ulp of the exact one, so when the quotient is not within 1e-12 relative of a midpoint
    the f32 mean, and everything computed from it, does not depend on the order."""
    x = np.ascontiguousarray(x, F)
    sq = (x * x).astype(F).astype(np.float64)
    tot = math.fsum(sq.tolist())
    m64 = tot / float(x.size)
    m = F(m64)
    lo, hi = np.nextafter(m, F(-np.inf)), np.nextafter(m, F(np.inf))
    mids = [(float(lo) + float(m)) / 2.0, (float(hi) + float(m)) / 2.0]
    dist = min(abs(m64 - t) for t in mids) / max(abs(m64), 1e-300)
    return m, dist


def norm_scale(x, eps):
    m, dist = norm_mean(x)
    assert dist > 1e-12, f"the mean of this row lies within {dist:.3g} of an f32 rounding midpoint: choose another row"
    return F(1.0) / np.sqrt(F(m + F(eps)), dtype=F)


def norm_rows(x, w, eps):
    """(x * scale) * w per row, f32: x [rows][E], w [E]."""
    x = np.ascontiguousarray(x, F)
    return np.stack([((r * norm_scale(r, eps)).astype(F) * w).astype(F) for r in x])


def factor(t, v):
    """w with f32(t * w) == v where one exists near v / t: (w, found).  Lets exact ties stand behind a product (the norm weight,
    the w3 x of the SiLU kinds)."""
    t, v = np.asarray(t, F), np.asarray(v, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        w0 = np.where(t != 0, v / np.where(t != 0, t, F(1)), F(0)).astype(F)
    best, found = w0.copy(), np.zeros(v.shape, bool)
    cand = w0
    for step in (0, 1, -1, 2, -2):
        c = cand
        for _ in range(abs(step)):
            c = np.nextafter(c, F(np.inf) if step > 0 else F(-np.inf)).astype(F)
        ok = ((t * c).astype(F) == v) & ~found
        best[ok] = c[ok]
        found |= ok
    return best, found


# ---- input sets ------------------------------------------------------------------------------------------------------------
def _ulps(x, n):
    x = np.asarray(x, F).copy()
    for _ in range(abs(n)):
        x = np.nextafter(x, F(np.inf) if n > 0 else F(-np.inf)).astype(F)
    return x


def _near_edge_block(rng):
    """A block whose two multipliers differ (127 / amax != 1 / (amax / 127) in f32), with values within a few ulp of
    (n + 0.5) / id on which the branches round apart although neither product is a tie."""
    while True:
        amax = F(rng.uniform(0.5, 2.0) * 2.0 ** int(rng.integers(-6, 7)))
        d = F(amax / F(127.0))
        i0, i1 = F(F(127.0) / amax), F(F(1.0) / d)
        if i0 == i1:
            continue
        vals = []
        for n in rng.permutation(np.arange(-126, 126)):
            x0 = F((n + 0.5) / float(i0))
            for u in range(-3, 4):
                x = _ulps(x0, u)
                p0, p1 = F(x * i0), F(x * i1)
                if abs(p0) > 126.6 or p0 % 1 == 0.5 or p1 % 1 == 0.5:
                    continue
                if int(np.rint(p0)) != int(_round_away(np.array([p1], F))[0]):
                    vals.append(x)
                    break
            if len(vals) == 24:
                break
        if len(vals) >= 8:
            b = np.zeros(32, F)
            b[:len(vals)] = vals
            b[len(vals):] = (rng.standard_normal(32 - len(vals)) * 0.3 * amax).astype(F)
            b[31] = amax if rng.random() < 0.5 else -amax
            return b[rng.permutation(32)]


def q8_pool():
    """72 blocks of 32 (8 rows of 9 blocks) and the family of each: the Q8 input set."""
    rng = np.random.default_rng(1234)
    blocks, fam = [], []

    def add(name, b):
        blocks.append(np.asarray(b, F).reshape(32))
        fam.append(name)

    for e in range(-16, 15):  # 31 random blocks, magnitudes 2^-16 .. 2^14
        add("random", rng.standard_normal(32) * 2.0 ** e)
    add("zero", np.zeros(32))
    add("negzero", np.full(32, -0.0))
    for pos, val in ((0, 3.25), (17, -1e-3), (31, 1000.0)):
        b = np.zeros(32)
        b[pos] = val
        add("single", b)
    for k in (-10, -3, 0, 4, 7, 11):  # amax = 127 * 2^k: both multipliers are 2^-k, the products n + 0.5 exactly
        for _ in range(2):
            n = rng.integers(-126, 126, 32)
            b = (n + 0.5) * 2.0 ** k
            b[int(rng.integers(0, 32))] = (127.0 if rng.random() < 0.5 else -127.0) * 2.0 ** k
            add("tie", b)
    for _ in range(8):
        add("edge", _near_edge_block(rng))
    for amax in (1.0e-3, 0.7e-3, 3.1e-3):  # d = amax / 127 is an f16 subnormal
        b = rng.standard_normal(32) * amax / 3
        b[5] = -amax
        add("d_subnormal", np.clip(b, -amax, amax))
    for m in (1024 + 1, 1024 + 2, 2047, 1500):  # d = (m + 0.5) * 2^-14: an f16 rounding tie (m odd rounds up, even down)
        d = (m + 0.5) * 2.0 ** -14
        b = rng.standard_normal(32) * 127 * d / 3
        b[20] = 127 * d
        add("d_tie", np.clip(b, -127 * d, 127 * d))
    for d in (65504.0, 65472.0, 65510.0):  # d at the top of the f16 range (d * q saturates the f16 operand)
        b = rng.standard_normal(32) * 127 * d / 3
        b[2] = -127 * d
        add("d_top", np.clip(b, -127 * d, 127 * d))
    b = rng.standard_normal(32) * 3e4
    b[9] = 1.0e5
    add("saturate", np.clip(b, -1e5, 1e5))  # d * q up to 1e5 > 65504
    while len(blocks) < 72:
        add("random", rng.standard_normal(32) * rng.uniform(0.01, 10.0))
    assert len(blocks) == 72
    return np.stack(blocks), fam


# (first, second) index of the two extremes of opposite sign in a super-block: both sides of every reduction boundary — the
# ends, waves (64), 16-lane rows, a lane's 4-vector of the four-per-lane forms — and two values inside one 4-vector
EXTREME_PAIRS = ((0, 255), (63, 64), (15, 16), (3, 4), (127, 128), (191, 192), (41, 42), (252, 254))


def q8k_pool():
    """36 super-blocks of 256 and the family of each: the Q8_K input set."""
    rng = np.random.default_rng(4321)
    blocks, fam = [], []

    def add(name, b):
        blocks.append(np.asarray(b, F).reshape(256))
        fam.append(name)

    for e in range(-16, 15, 5):  # 7 random super-blocks, 2^-16 .. 2^14
        add("random", rng.standard_normal(256) * 2.0 ** e)
    add("zero", np.zeros(256))
    add("negzero", np.full(256, -0.0))
    for pos, val in ((0, -2.5), (200, 7e-4)):
        b = np.zeros(256)
        b[pos] = val
        add("single", b)
    for k in (-8, 0, 5):  # max = +-128 * 2^k: iscale = -+2^-k, the products n + 0.5 exactly
        for sgn in (1.0, -1.0):
            n = rng.integers(-127, 127, 256)
            b = (n + 0.5) * 2.0 ** k
            b[int(rng.integers(0, 256))] = sgn * 128.0 * 2.0 ** k
            add("tie", b)
    for first, second in EXTREME_PAIRS:  # +max and -max in one super-block; the second one maps to +128 and is clamped to 127
        for sgn in (1.0, -1.0):
            mx = F(rng.uniform(1.0, 5.0))
            b = rng.uniform(-0.9, 0.9, 256) * mx
            b[first], b[second] = sgn * mx, -sgn * mx
            add("extremes", b)
    b = rng.standard_normal(256) * 3e4
    b[77] = -1.0e5
    add("saturate", np.clip(b, -1e5, 1e5))
    while len(blocks) < 36:
        add("random", rng.standard_normal(256) * rng.uniform(0.01, 10.0))
    assert len(blocks) == 36
    return np.stack(blocks), fam


def launches(pool, rows, per_row, cap=None):
    """The pool cut into inputs [rows][per_row blocks] that cover it once, the last one filled up from the start."""
    n, per = pool.shape[0], rows * per_row
    count = -(-n // per)
    if cap:
        count = min(count, cap)
    for i in range(count):
        idx = (np.arange(per) + i * per) % n
        yield pool[idx].reshape(rows, per_row * pool.shape[1])


def norm_rows_input(rows, E, seed):
    """Rows of three magnitudes (1e-3, 1, 300) for the norm kinds, each checked against norm_mean's midpoint condition."""
    rng = np.random.default_rng([seed, rows, E])
    out = []
    for r in range(rows):
        while True:
            x = (rng.standard_normal(E) * (1e-3, 1.0, 300.0)[r % 3]).astype(F)
            if norm_mean(x)[1] > 1e-12:
                break
        out.append(x)
    return np.stack(out)


def norm_tie_weight(x0, eps, block_elems, seed):
    """A norm weight w [E] that places exact ties behind the norm of row x0: y = (x0 * scale) * w is, block after block, a tie
    block of the pool's kind (magnitudes of order one) wherever `factor` finds the weight; elsewhere w is of order one."""
    rng = np.random.default_rng([seed, x0.size])
    t = (x0 * norm_scale(x0, eps)).astype(F)
    E = x0.size
    v = np.empty(E, F)
    for b in range(E // block_elems):
        k = int(rng.integers(-8, -4))  # ties of order one behind a weight of order one
        top = 127.0 if block_elems == 32 else 128.0
        n = rng.integers(-int(top) + 1, int(top) - 1, block_elems)
        blk = (n + 0.5) * 2.0 ** k
        blk[int(rng.integers(0, block_elems))] = (top if rng.random() < 0.5 else -top) * 2.0 ** k
        v[b * block_elems:(b + 1) * block_elems] = blk
    w, found = factor(t, v)
    found &= (np.abs(w) >= 2.0 ** -8) & (np.abs(w) <= 2.0 ** 8)  # a weight of another order would only move the block's scale out of range
    w = np.where(found, w, rng.uniform(0.5, 1.5, E).astype(F)).astype(F)
    return w, found


def silu_safe(rng, n):
    """n f16-valued inputs whose SiLU is not within 1e-6 relative of an f16 rounding midpoint: ggml's f16-table SiLU of them is the
    same f16 value with any expf accurate to a few ulp (the device's and the host's)."""
    g = (3.0 * rng.standard_normal(n)).astype(np.float16).astype(np.float64)
    while True:
        s = g / (1.0 + np.exp(-g))
        bad = (s * (1 - 1e-6)).astype(np.float16) != (s * (1 + 1e-6)).astype(np.float16)
        bad |= np.abs(s) < 1e-3  # keep the factor away from zero: `factor` divides by it
        if not bad.any():
            return g.astype(F)
        g[bad] = (3.0 * rng.standard_normal(int(bad.sum()))).astype(np.float16)


def branch_diff_count(x, f16d=True):
    """Elements of the set on which the two branches of the Q8 quantizer give different quants."""
    return int(np.count_nonzero(q8(x, 0, f16d)[0] != q8(x, 1, f16d)[0]))
