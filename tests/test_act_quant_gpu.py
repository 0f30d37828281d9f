"""Every activation quantizer kernel, launched alone through ggml_hip_debug_act_quant with its call site's launch geometry, against
the NumPy restatements of ggml's arithmetic (tests/act_quant_ref.py; held to the oracle in tests/test_act_quant_ref.py), byte for
byte: quants, scales, sums, bsums, the [block][8] tables, the f16 operands in the GEMM's k order; guards intact; what a launch has
no business writing still 0xFF.  The inputs are the sets of act_quant_ref: exact rounding ties, near-edge values, f16 edges of d,
+max and -max in one super-block at every reduction boundary, the clamp, the f16 saturation.

Q8 kinds run under option act_quant 0 and 1: each result equals its own branch's reference, and the two device results differ on
exactly the elements where the references differ — on the whole set that is act_quant_ref.branch_diff_count (non-zero: the test
can tell the branches apart).  Norm kinds: the normed row the kernel taps is compared bit for bit with the reference norm (under
the midpoint condition of norm_mean), the quantized output with the reference quantization of that tapped row; the norm weight
places exact ties behind row 0.  SiLU kinds: the oracle's f16-table SiLU times g3 in f32, then the quantizer; g3 places the set's
values, ties included, behind the product where an exact factor exists."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import act_quant_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 256
EPS = 1e-5
(QUANTIZE_ACT, QUANT_ROW, RMSNORM_QUANT, RMSNORM_QUANT_WARM, QUANT_ACT_I8, QUANT_ACT_F16, P_QUANT4, P_SILU_MUL_QUANT, P_NORM_QUANT,
 QUANT_ACT_F16_K, F32_TO_W16, QUANT_Q8K, K_NORM_QUANT, K_QUANT, K_SILU_MUL_QUANT) = range(15)
F16D, TABLES, K8 = 1, 2, 4
POISON = F(3.0e38)  # fills what a kernel must not read: it would become the block's maximum


@functools.lru_cache(None)
def _q8_pool():
    return R.q8_pool()[0]


@functools.lru_cache(None)
def _q8k_pool():
    return R.q8k_pool()[0]


def _ptr(a):
    return None if a is None else a.ctypes.data


def _call(G, kind, flags, rows, K, a, sizes, stride=0, b=None, r=None, w=None, eps=0.0, part=0, zp=0):
    """One launch.  sizes: bytes of every output slot (None: not passed).  Returns (rc, outputs without their guards)."""
    bufs = [None if n is None else np.full(n + GUARD, 0xFF, np.uint8) for n in sizes]
    arr = (C.c_void_p * 8)(*([_ptr(x) for x in bufs] + [None] * (8 - len(bufs))))
    ins = [None if v is None else np.ascontiguousarray(v, F) for v in (a, b, r, w)]
    rc = G.lib().ggml_hip_debug_act_quant(kind, flags, rows, K, stride, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(ins[3]), eps, part,
                                          zp, arr)
    if rc != 0:
        return rc, None
    outs = []
    for i, (buf, n) in enumerate(zip(bufs, sizes)):
        if buf is None:
            outs.append(None)
            continue
        assert np.all(buf[n:] == 0xFF), f"kind {kind}: a store past the end of output {i}"
        outs.append(buf[:n])
    return 0, outs


@contextlib.contextmanager
def _branch(G, aq):
    G.set_option("act_quant", aq)
    try:
        yield
    finally:
        G.set_option("act_quant", 0)


def _strided(x, stride):
    """x [rows][K] -> [rows][stride] with the padding poisoned."""
    rows, K = x.shape
    a = np.full((rows, stride), POISON, F)
    a[:, :K] = x
    return a


def _eq(tag, what, got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (tag, what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{tag}: {what}: {bad.size} of {got.size} differ, first at {bad[:8]}: got {got[bad[:8]]} want {want[bad[:8]]}"


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _both_branches(G, run, full=None):
    """run(aq) -> {tag: (device quants or operand, its reference)} with each result already held to its own reference.  The two
    device results must differ exactly where the references do; `full`: the tag of the launch over the whole Q8 set, whose count
    must be branch_diff_count."""
    res = {}
    for aq in (0, 1):
        with _branch(G, aq):
            res[aq] = run(aq)
    total = 0
    for tag in res[0]:
        d0, r0 = res[0][tag]
        d1, r1 = res[1][tag]
        assert np.array_equal(d0 != d1, r0 != r1), f"{tag}: the device's branches differ on other elements than the references'"
        total += int(np.count_nonzero(d0 != d1))
    if full is not None:
        d0, d1 = res[0][full][0], res[1][full][0]
        want = R.branch_diff_count(_q8_pool())
        got = int(np.count_nonzero(d0 != d1))
        print(f"{full}: the branches differ on {got} elements of the set (reference: {want})")
        assert got == want and want > 0
    return total


# ---- planar Q8 ---------------------------------------------------------------------------------------------------------------
def _planar_sizes(rows, nblk, tabs, y):
    nt = (rows + 7) // 8 * nblk * 32
    return [rows * nblk * 16, rows * nblk * 16, rows * nblk * 4, rows * nblk * 4, nt if tabs else None, nt if tabs else None,
            rows * nblk * 128 if y else None]


def _check_planar(tag, outs, x, aq, f16d, rows, nblk, tabs):
    q, d, s = R.q8(x, aq, f16d)
    lo, hi = R.planar(q)
    _eq(tag, "lo", outs[0].view(np.int8), lo)
    _eq(tag, "hi", outs[1].view(np.int8), hi)
    _eq(tag, "d", outs[2].view(np.uint32), _bits(d))
    _eq(tag, "sum", outs[3].view(np.int32), s)
    if tabs:
        for what, o, v in (("dT", outs[4], _bits(d)), ("sT", outs[5], s.view(np.uint32))):
            t, m = R.tables(v, rows, nblk)
            got = o.view(np.uint32).reshape(t.shape)
            _eq(tag, what, got[m], t[m])
            assert np.all(got[~m] == 0xFFFFFFFF), f"{tag}: {what}: an entry of a row that does not exist was written"
    dev_q = np.concatenate([outs[0].view(np.int8).reshape(-1, 16), outs[1].view(np.int8).reshape(-1, 16)], axis=1)
    return dev_q, q


SHAPES32 = [(rows, nblk) for rows in (1, 3, 8, 9) for nblk in (1, 7, 8, 9)]


@pytest.mark.parametrize("f16d", [1, 0])
@pytest.mark.parametrize("kind,tabs", [(QUANTIZE_ACT, 0), (QUANT_ROW, 0), (QUANT_ROW, 1)])
def test_planar_q8_rows(G, kind, tabs, f16d):
    """k_quantize_act (rows strided) and k_quant_row (without and with its tables; 9 rows: a second table with one column)."""
    pool = _q8_pool()

    def run(aq):
        out = {}
        for rows, nblk in SHAPES32:
            for i, x in enumerate(R.launches(pool, rows, nblk, cap=None if (rows, nblk) == (8, 9) else 3)):
                tag = f"kind {kind} tables {tabs} f16d {f16d} act_quant {aq} rows {rows} nblk {nblk} launch {i}"
                K = nblk * 32
                stride = K + 40 if kind == QUANTIZE_ACT else 0
                a = _strided(x, stride) if stride else x
                rc, outs = _call(G, kind, f16d | (TABLES if tabs else 0), rows, K, a, _planar_sizes(rows, nblk, tabs, False), stride=stride)
                assert rc == 0, tag
                out[(rows, nblk, i)] = _check_planar(tag, outs, x, aq, f16d, rows, nblk, tabs)
        return out
    _both_branches(G, run, full=(8, 9, 0))


@functools.lru_cache(None)
def _norm_case(rows, E, block, seed=3):
    x = R.norm_rows_input(rows, E, seed)
    w, found = R.norm_tie_weight(x[0], EPS, block, seed)
    return x, w, R.norm_rows(x, w, EPS), int(found.sum())


@pytest.mark.parametrize("f16d", [1, 0])
@pytest.mark.parametrize("E", [32, 1056, 8192, 8224])
def test_rmsnorm_quant_and_its_warming_form(G, E, f16d):
    """k_rmsnorm_quant with its y tap and tables (E = 8224: the loop path, which a chunk of a model wider than 8192 reaches), and
    k_rmsnorm_quant_warm on its call site's grid with warming off: the same bytes."""
    nblk = E // 32

    def run(aq):
        out = {}
        for rows in (1, 3, 8, 9):
            x, w, y_ref, nties = _norm_case(rows, E, 32)
            tag = f"k_rmsnorm_quant E {E} rows {rows} f16d {f16d} act_quant {aq}"
            sizes = _planar_sizes(rows, nblk, True, True)
            rc, outs = _call(G, RMSNORM_QUANT, f16d | TABLES, rows, E, x, sizes, w=w, eps=EPS)
            assert rc == 0, tag
            y = outs[6].view(F).reshape(rows, E)
            _eq(tag, f"y ({nties} elements of row 0 placed on ties)", _bits(y), _bits(y_ref))
            out[rows] = _check_planar(tag, outs, y, aq, f16d, rows, nblk, True)
            if rows <= 8:
                rc, warm = _call(G, RMSNORM_QUANT_WARM, f16d | TABLES, rows, E, x, sizes, w=w, eps=EPS)
                assert rc == 0, tag
                for i, (p, q) in enumerate(zip(outs, warm)):
                    _eq(tag, f"k_rmsnorm_quant_warm output {i}", q, p)
            # without the tap and the tables: the same quants
            rc, bare = _call(G, RMSNORM_QUANT, f16d, rows, E, x, _planar_sizes(rows, nblk, False, False), w=w, eps=EPS)
            assert rc == 0
            for i in range(4):
                _eq(tag, f"output {i} without tap and tables", bare[i], outs[i])
        return out
    total = _both_branches(G, run)
    if E >= 1056:
        assert total > 0, "no tie behind the norm told the branches apart"


# ---- int8 for the i8 GEMM ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16d,zp", [(1, 8), (1, 16), (1, 0), (0, 0)])
def test_quant_act_i8(G, f16d, zp):
    pool = _q8_pool()

    def run(aq):
        out = {}
        for rows, nblk in SHAPES32:
            for i, x in enumerate(R.launches(pool, rows, nblk, cap=None if (rows, nblk) == (8, 9) else 2)):
                tag = f"k_quant_act_i8 f16d {f16d} zp {zp} act_quant {aq} rows {rows} nblk {nblk} launch {i}"
                K, n = nblk * 32, rows * nblk
                rc, outs = _call(G, QUANT_ACT_I8, f16d, rows, K, _strided(x, K + 8), [n * 32, n * 4, n * 4], stride=K + 8, zp=zp)
                assert rc == 0, tag
                q, d, s = R.q8(x, aq, bool(f16d))
                _eq(tag, "q8", outs[0].view(np.int8), q)
                _eq(tag, "d", outs[1].view(np.uint32), _bits(d))
                if f16d:  # the zero-point term as int32 bits
                    _eq(tag, "xs", outs[2].view(np.int32), -zp * s)
                else:  # Q8_1's s = d * sum
                    _eq(tag, "xs", outs[2].view(np.uint32), _bits(d * s.astype(F)))
                out[(rows, nblk, i)] = (outs[0].view(np.int8).reshape(-1, 32).copy(), q)
        return out
    _both_branches(G, run, full=(8, 9, 0))


# ---- the f16 GEMM operand ----------------------------------------------------------------------------------------------------
def _silu_inputs(O, x, seed):
    """g1 (SiLU-safe) and g3 with f32(silu(g1) * g3) == x where an exact factor exists; the product row the quantizer sees."""
    rng = np.random.default_rng([seed, x.size])
    g1 = R.silu_safe(rng, x.size).reshape(x.shape)
    s = O.silu(g1)
    g3, found = R.factor(s, x)
    g3 = np.where(np.isfinite(g3), g3, F(0)).astype(F)
    return g1, g3, (s * g3).astype(F), int(found.sum())


@pytest.mark.parametrize("f16d", [1, 0])
@pytest.mark.parametrize("kind", [QUANT_ACT_F16, P_QUANT4, P_SILU_MUL_QUANT])
def test_f16_operand_q8_kinds(G, O, kind, f16d):
    """k_quant_act_f16 (strided rows), k_p_quant4 and k_p_silu_mul_quant (part4 zero and non-zero): 3 rows of 96 give n4 = 72, a
    partial workgroup; 8 rows of 9 blocks two workgroups and a partial third."""
    pool = _q8_pool()
    shapes = SHAPES32 if kind == QUANT_ACT_F16 else [(1, 1), (3, 3), (3, 7), (8, 9), (9, 9)]

    def run(aq):
        out = {}
        for rows, nblk in shapes:
            for i, x in enumerate(R.launches(pool, rows, nblk, cap=None if (rows, nblk) in ((8, 9), (3, 3)) else 2)):
                K = nblk * 32
                for part in ((0, 1) if kind == P_SILU_MUL_QUANT else (0,)):
                    tag = f"kind {kind} f16d {f16d} act_quant {aq} rows {rows} nblk {nblk} launch {i} part {part}"
                    if kind == QUANT_ACT_F16:
                        rc, outs = _call(G, kind, f16d, rows, K, _strided(x, K + 24), [rows * K * 2], stride=K + 24)
                        seen = x
                    elif kind == P_QUANT4:
                        rc, outs = _call(G, kind, f16d, rows, K, x, [rows * K * 2])
                        seen = x
                    else:
                        g1, g3, seen, nfound = _silu_inputs(O, x, i)
                        if part:  # two partials each, `part` floats apart (halves: their sum is exact), poison between them
                            p = rows * K + 64
                            a, b = np.full(p + rows * K, POISON, F), np.full(p + rows * K, POISON, F)
                            for arr, v in ((a, g1), (b, g3)):
                                arr[:rows * K] = (v * F(0.5)).reshape(-1)
                                arr[p:] = (v - v * F(0.5)).reshape(-1)
                            assert np.array_equal(a[:rows * K] + a[p:], g1.reshape(-1)) and np.array_equal(b[:rows * K] + b[p:], g3.reshape(-1))
                            rc, outs = _call(G, kind, f16d, rows, K, a, [rows * K * 2], b=b, part=p)
                        else:
                            rc, outs = _call(G, kind, f16d, rows, K, g1, [rows * K * 2], b=g3)
                    assert rc == 0, tag
                    ref = R.q8_f16(seen, aq, bool(f16d))
                    _eq(tag, "x16", outs[0].view(np.uint16), ref)
                    out[(rows, nblk, i, part)] = (outs[0].view(np.uint16).copy(), ref)
        return out
    total = _both_branches(G, run)
    assert total > 0


@functools.lru_cache(None)
def _p_norm_case(rows, E, block, add, seed=11):
    rng = np.random.default_rng([seed, rows, E, add])
    if not add:
        x = R.norm_rows_input(rows, E, seed)
        xs, x2, r = x, None, None
    else:
        while True:
            x = R.norm_rows_input(rows, E, seed)
            x2 = (rng.standard_normal((rows, E)) * np.abs(x).mean(axis=1, keepdims=True)).astype(F) if add == 2 else None
            r = (rng.standard_normal((rows, E)) * np.abs(x).mean(axis=1, keepdims=True)).astype(F)
            xs = ((x + x2).astype(F) + r).astype(F) if add == 2 else (x + r).astype(F)
            if all(R.norm_mean(row)[1] > 1e-12 for row in xs):
                break
            seed += 1
    w, found = R.norm_tie_weight(xs[0], EPS, block, seed)
    return x, x2, r, xs, w, R.norm_rows(xs, w, EPS)


@pytest.mark.parametrize("f16d", [1, 0])
@pytest.mark.parametrize("E", [32, 288, 8192])
def test_p_norm_quant(G, E, f16d):
    """k_p_norm_quant<F16D, ADD>: plain, with the residual, with the residual and a second partial; xsum and y_f32 come back too."""
    def run(aq):
        out = {}
        for rows in (1, 3):
            for add in (0, 1, 2):
                x, x2, r, xs, w, y_ref = _p_norm_case(rows, E, 32, add)
                tag = f"k_p_norm_quant E {E} rows {rows} add {add} f16d {f16d} act_quant {aq}"
                rc, outs = _call(G, P_NORM_QUANT, f16d, rows, E, x, [rows * E * 2, rows * E * 4 if add else None, rows * E * 4], b=x2, r=r, w=w,
                                 eps=EPS)
                assert rc == 0, tag
                if add:
                    _eq(tag, "xsum", outs[1].view(np.uint32), _bits(xs))
                y = outs[2].view(F).reshape(rows, E)
                _eq(tag, "y", _bits(y), _bits(y_ref))
                ref = R.q8_f16(y, aq, bool(f16d))
                _eq(tag, "x16", outs[0].view(np.uint16), ref)
                rc, bare = _call(G, P_NORM_QUANT, f16d, rows, E, x, [rows * E * 2, rows * E * 4 if add else None, None], b=x2, r=r, w=w, eps=EPS)
                assert rc == 0
                _eq(tag, "x16 without the tap", bare[0], outs[0])
                out[(rows, add)] = (outs[0].view(np.uint16).copy(), ref)
        return out
    total = _both_branches(G, run)
    if E >= 288:
        assert total > 0, "no tie behind the norm told the branches apart"


@pytest.mark.parametrize("E", [256, 768, 8192])
def test_p_norm_quant_k8(G, E):
    for rows in (1, 3):
        for add in (0, 1, 2):
            x, x2, r, xs, w, y_ref = _p_norm_case(rows, E, 256, add)
            tag = f"k_p_norm_quant K8 E {E} rows {rows} add {add}"
            rc, outs = _call(G, P_NORM_QUANT, K8, rows, E, x, [rows * E * 2, rows * E * 4 if add else None, rows * E * 4], b=x2, r=r, w=w, eps=EPS)
            assert rc == 0, tag
            if add:
                _eq(tag, "xsum", outs[1].view(np.uint32), _bits(xs))
            y = outs[2].view(F).reshape(rows, E)
            _eq(tag, "y", _bits(y), _bits(y_ref))
            _eq(tag, "x16", outs[0].view(np.uint16), R.q8k_f16(y))


@pytest.mark.parametrize("kind", [QUANT_ACT_F16_K, P_QUANT4, P_SILU_MUL_QUANT])
def test_f16_operand_q8k_kinds(G, O, kind):
    """k_quant_act_f16_k (strided rows) and the K8 forms of k_p_quant4 / k_p_silu_mul_quant: K in {256, 768}, 1 and 3 rows."""
    pool = _q8k_pool()
    for rows in (1, 3):
        for nsb in (1, 3):
            K = nsb * 256
            for i, x in enumerate(R.launches(pool, rows, nsb)):
                tag = f"kind {kind} K8 rows {rows} nsb {nsb} launch {i}"
                if kind == QUANT_ACT_F16_K:
                    rc, outs = _call(G, kind, 0, rows, K, _strided(x, K + 16), [rows * K * 2], stride=K + 16)
                    seen = x
                elif kind == P_QUANT4:
                    rc, outs = _call(G, kind, K8, rows, K, x, [rows * K * 2])
                    seen = x
                else:
                    g1, g3, seen, _ = _silu_inputs(O, x, i)
                    rc, outs = _call(G, kind, K8, rows, K, g1, [rows * K * 2], b=g3)
                assert rc == 0, tag
                _eq(tag, "x16", outs[0].view(np.uint16), R.q8k_f16(seen))


def test_f32_to_w16(G):
    pool = _q8_pool()
    for rows, nblk in ((1, 1), (3, 7), (8, 9), (9, 9)):
        for i, x in enumerate(R.launches(pool, rows, nblk, cap=2)):
            rc, outs = _call(G, F32_TO_W16, 0, rows, nblk * 32, x, [x.size * 2])
            assert rc == 0
            _eq(f"k_f32_to_w16 rows {rows} nblk {nblk} launch {i}", "w16", outs[0].view(np.uint16), R.w16(x))


# ---- Q8_K --------------------------------------------------------------------------------------------------------------------
def _check_q8k(tag, outs, seen):
    q, d, bs = R.q8k(seen)
    _eq(tag, "q8", outs[0].view(np.int8), q)
    _eq(tag, "d8", outs[1].view(np.uint32), _bits(d))
    _eq(tag, "bsums", outs[2].view(np.int16), bs)


@pytest.mark.parametrize("kind", [QUANT_Q8K, K_QUANT, K_SILU_MUL_QUANT])
def test_q8k_kinds(G, O, kind):
    """k_quant_q8k (strided rows), k_k_quant, k_k_silu_mul_quant: nsb in {1, 3}, 1 and 3 rows, the whole Q8_K set through each shape."""
    pool = _q8k_pool()
    for rows in (1, 3):
        for nsb in (1, 3):
            K, n = nsb * 256, rows * nsb
            sizes = [n * 256, n * 4, n * 32]
            for i, x in enumerate(R.launches(pool, rows, nsb)):
                tag = f"kind {kind} rows {rows} nsb {nsb} launch {i}"
                if kind == QUANT_Q8K:
                    rc, outs = _call(G, kind, 0, rows, K, _strided(x, K + 32), sizes, stride=K + 32)
                    seen = x
                elif kind == K_QUANT:
                    rc, outs = _call(G, kind, 0, rows, K, x, sizes)
                    seen = x
                else:
                    g1, g3, seen, _ = _silu_inputs(O, x, i)
                    rc, outs = _call(G, kind, 0, rows, K, g1, sizes, b=g3)
                assert rc == 0, tag
                _check_q8k(tag, outs, seen)


@pytest.mark.parametrize("E", [256, 768])
def test_k_norm_quant(G, E):
    for rows in (1, 3):
        x, w, y_ref, nties = _norm_case(rows, E, 256)
        n = rows * E // 256
        tag = f"k_k_norm_quant E {E} rows {rows}"
        rc, outs = _call(G, K_NORM_QUANT, 0, rows, E, x, [n * 256, n * 4, n * 32, rows * E * 4], w=w, eps=EPS)
        assert rc == 0, tag
        y = outs[3].view(F).reshape(rows, E)
        _eq(tag, f"y ({nties} elements of row 0 placed on ties)", _bits(y), _bits(y_ref))
        _check_q8k(tag, outs, y)
        rc, bare = _call(G, K_NORM_QUANT, 0, rows, E, x, [n * 256, n * 4, n * 32, None], w=w, eps=EPS)
        assert rc == 0
        for i in range(3):
            _eq(tag, f"output {i} without the tap", bare[i], outs[i])


# ---- what the hook refuses ---------------------------------------------------------------------------------------------------
def test_the_hook_refuses_what_no_call_site_launches(G):
    one = lambda n: np.ones(n, F)  # noqa: E731
    big = [1 << 20] * 7
    assert _call(G, QUANT_ROW, 0, 1, 48, one(48), big)[0] == -1  # not whole blocks
    assert _call(G, K_QUANT, 0, 1, 288, one(288), big[:3])[0] == -1  # not whole super-blocks
    assert _call(G, P_QUANT4, K8, 1, 288, one(288), big[:1])[0] == -1
    assert _call(G, QUANTIZE_ACT, 0, 2, 64, one(128), big[:4], stride=32)[0] == -1  # rows that overlap
    assert _call(G, P_NORM_QUANT, 0, 1, 8224, one(8224), big[:3], w=one(8224))[0] == -1  # the prompt plan aborts above 8192
    assert _call(G, RMSNORM_QUANT, 0, 1, 16384, one(16384), big, w=one(16384))[0] == -1  # the row does not fit the dynamic LDS
    assert _call(G, RMSNORM_QUANT_WARM, 0, 9, 32, one(9 * 32), big, w=one(32))[0] == -1  # the warming form: chunks of up to 8 rows
    assert _call(G, QUANT_ROW, 0, 32, 32, one(32 * 32), big)[0] == -1  # more rows than a chunk has
    assert _call(G, QUANT_ACT_I8, F16D, 1, 32, one(32), big[:3], zp=4)[0] == -1  # no weight type has this zero point
    assert _call(G, QUANT_ROW, 0, 1, 32, one(32), [64, 64, None, 64])[0] == -1  # a missing output
