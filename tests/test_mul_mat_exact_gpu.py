"""Every quantized mul_mat kernel against exact references, on EVERY output (helpers: tests/mul_mat_exact_ref.py, held to the
oracle without a GPU in tests/test_mul_mat_exact_ref.py).

A. Exact integers.  Weights and activations whose every stored quantity is an integer and whose row sums |x| . |w| stay below
2^24: every partial sum of any summation order is an exact f32 integer, so the MFMA accumulation, the K split, atomics, DPP trees
and block order cannot differ and the result must EQUAL the integer product — through every dispatch regime of mul_mat_q /
mul_mat_k (csrc/backend_ops.inc): the mat-vecs k_mmvq / k_mmvq_k / k_mmvq_k2, k_mmq_dma_p8 (by default below 64 tokens, and
forced), k_mmq (K / 32 odd), k_mmq_w16_p8, k_mmq_w16_256, k_mmq_i8 with and without its K split, the K-quant weight's resident f16
copy on both tile sizes (8192 + 130 rows: the second chunk of ensure_w16_k), k_mmq_cols, k_mmvq_big and k_mmvq_kbig.  The
mmq_launches_* counters (the MMVQ timing class for the mat-vecs) say that the named kernel ran.

B. One-hot activations.  K tokens, token k with one value at position k whose activation operand is exactly 127 (1 for Q8_K):
out[k][m] == f32(127 * w16[m][k]), so one GEMM reads out the whole f16 weight operand — k_dequant_w16 (through both resident-copy
kernels), the slice decoder of k_mmq_dma_p8, both decoders of k_mmq, the K-quant copy across the 8192-row chunk boundary — and it
must equal, bit for bit, the exact value rounded once to f16 (K-quants: f16 of the oracle's f32 decoder).  The blocks hold every
code, scales with full significands (6 .. 12 % of the values are exact rounding ties), negative, zero and subnormal scales.

C. Random inputs against the exact operands.  ref = x16 . w16 in float64 with x16 from act_quant_ref and w16 as in B; what is
left is the f32 accumulation: |got - ref| <= 2 K 2^-24 S, S = |x16| . |w16| (K correctly rounded additions, doubled because the
rounding inside the matrix cores is not documented) — 3e-5 S at K = 256 where the oracle tests allow 1.1e-3 S, and no allowance
for operand rounding at all.  A second class has only non-negative weights and activations, where a biased operand rounding adds
up (truncation: 4 .. 18 x this bound) instead of averaging out.

Largest accumulation error seen on an MI355X, as a multiple of K 2^-24 S (the bound is 2; each test prints its own):
    kernel                        signed inputs          non-negative inputs
    k_mmq_w16_p8                  0.009 (K 1024: 0.002)  0.027 (K 1024: 0.008)
    k_mmq_w16_256                 0.009 (K 1024: 0.002)  0.027 (K 1024: 0.008)
    k_mmq_dma_p8                  0.009 (K 1024: 0.002)  0.027 (K 1024: 0.008)
    k_mmq (K = 352)               0.005                  0.021
    K-quant copy, k_mmq_w16_p8    0.008                  0.023
    K-quant copy, k_mmq_w16_256   0.008                  0.023
The three block-format GEMMs are bit-identical to each other, hence the equal figures.  Parts A and B held exactly on every
output, blocks with subnormal f16 scales included: neither the decoders nor the matrix cores flush f16 subnormals."""
import contextlib

import numpy as np
import pytest

import mul_mat_exact_ref as E
import test_decode_matvec_gpu as DM  # the launch helpers of the k_mmvq_big / k_mmvq_kbig hooks
from test_mmq256_gpu import SHAPES as MMQ256_SHAPES
from test_mmq_cols_gpu import _cols
from test_ops_gpu import _mul_mat_gpu

pytestmark = pytest.mark.gpu

F = np.float32
MMQ_KERNELS = ("plain", "dma_p8", "w16_p8", "w16_256", "i8")
W16_P8, W16_256, DMA_P8 = dict(mmq_t256=0), dict(mmq_t256=2), dict(mmq_t256=0, mmq_w16=0)


@contextlib.contextmanager
def _options(G, **opts):
    old = {k: G.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            G.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            G.set_option(k, v)


def _launches(G):
    return {k: int(G.lib().ggml_hip_get_stat(("mmq_launches_" + k).encode())) for k in MMQ_KERNELS}


def _gemm(G, t, raw, M, K, X, kernel, **opts):
    """The public op under `opts`; the counters must name `kernel` and nothing else."""
    with _options(G, **opts):
        c0 = _launches(G)
        got = _mul_mat_gpu(G, t, raw, M, K, np.ascontiguousarray(X, F))
        c1 = _launches(G)
    ran = [k for k in MMQ_KERNELS if c1[k] > c0[k]]
    assert ran == [kernel], (kernel, ran, opts)
    return got


def _matvec(G, t, raw, M, K, X, **opts):
    """The public op on the mat-vec kernels: no GEMM launch, and launches of the MMVQ timing class."""
    with _options(G, **opts):
        c0 = _launches(G)
        G.lib().ggml_hip_timing_begin()
        try:
            got = _mul_mat_gpu(G, t, raw, M, K, np.ascontiguousarray(X, F))
        finally:
            G.lib().ggml_hip_timing_end()
        c1 = _launches(G)
    assert c1 == c0, "a GEMM kernel ran where the mat-vec was meant"
    assert G.timing_query(G.KCLASS_MMVQ)[1] >= 1
    return got


def _same(tag, got, want):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (f"{tag}: {bad.shape[0]} of {got.size} outputs differ, first (token, row) {bad[:6].tolist()}: got "
                               f"{[float(got[tuple(b)]) for b in bad[:6]]} want {[float(want[tuple(b)]) for b in bad[:6]]}")


def _exact(O, t, M, K, N, quantize=None):
    """One case of part A with its preconditions checked on the CPU: (raw, X f32, the integer product f32 [N][M])."""
    block = t in E.BLOCK_TYPES
    raw, W, X = E.exact_case(t, M, K, N, O.quantize if block else quantize)
    assert raw.size == M * E.row_bytes(t, K)
    step = max(1, (1 << 24) // K)
    for r0 in range(0, M, step):  # the oracle decodes the raw weights to the intended integers
        r1 = min(M, r0 + step)
        part = raw[r0 * E.row_bytes(t, K):r1 * E.row_bytes(t, K)]
        assert np.array_equal(O.dequantize(t, part, (r1 - r0) * K), W[r0:r1].reshape(-1).astype(F))
    ref = E.exact_product(X, W, 32 if block else 256)  # < 2^24, f16 values, integer block sums
    rows = np.unique(np.concatenate([[0, M - 1], np.random.default_rng(M).choice(M, min(M, 14), replace=False)]))
    rb = E.row_bytes(t, K)
    sub = np.concatenate([raw[r * rb:(r + 1) * rb] for r in rows])
    cols = slice(0, min(N, 64))
    assert np.array_equal(O.mul_mat(t, sub, len(rows), K, X[cols].astype(F), mode=O.ref_mode()), ref[cols][:, rows])
    return raw, X.astype(F), ref


def _k_variants(t):
    return (False, True) if t in (E.Q3_K, E.Q6_K) else (False,)


# ---- A: exact integers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", E.BLOCK_TYPES)
@pytest.mark.parametrize("shape", [(257, 1024), (33, 4096), (130, 352)])
def test_exact_integers_on_the_mat_vec(G, O, t, shape):
    """k_mmvq at 1, 3, 8 and 13 tokens, and at 40 tokens with the GEMM switched off (mmq_min = 0)."""
    M, K = shape
    raw, X, ref = _exact(O, t, M, K, 40)
    for N in (1, 3, 8, 13):
        _same(f"k_mmvq type {t} {shape} N {N}", _matvec(G, t, raw, M, K, X[:N]), ref[:N])
    _same(f"k_mmvq type {t} {shape} N 40 mmq_min 0", _matvec(G, t, raw, M, K, X, mmq_min=0), ref)


@pytest.mark.parametrize("t", E.K_TYPES)
@pytest.mark.parametrize("shape", [(257, 1024), (130, 2816), (64, 11008)])
def test_exact_integers_on_the_k_mat_vec(G, O, t, shape):
    """k_mmvq_k (Q4_K, Q6_K) / k_mmvq_k2 (Q2_K, Q3_K, Q5_K): hand-packed blocks with d = dmin = 1, for Q3_K / Q6_K also integer
    matrices through the oracle's quantizer."""
    M, K = shape
    for quantized in _k_variants(t):
        raw, X, ref = _exact(O, t, M, K, 40, O.quantize if quantized else None)
        for N in (1, 3, 8, 13):
            _same(f"K mat-vec type {t} {shape} N {N} quantized {quantized}", _matvec(G, t, raw, M, K, X[:N]), ref[:N])
        _same(f"K mat-vec type {t} {shape} N 40 mmq_min 0 quantized {quantized}", _matvec(G, t, raw, M, K, X, mmq_min=0), ref)


@pytest.mark.parametrize("t", E.BLOCK_TYPES)
@pytest.mark.parametrize("shape,kernel", [((200, 128, 33), "dma_p8"), ((130, 1024, 63), "dma_p8"), ((200, 96, 33), "plain"),
                                          ((384, 352, 100), "plain")])
def test_exact_integers_on_the_default_gemm_below_64_tokens_and_at_odd_k(G, O, t, shape, kernel):
    """32 .. 63 tokens meet no resident copy: k_mmq_dma_p8 by default; K / 32 odd: k_mmq."""
    M, K, N = shape
    raw, X, ref = _exact(O, t, M, K, N)
    _same(f"k_mmq_{kernel} type {t} {shape}", _gemm(G, t, raw, M, K, X, kernel), ref)


@pytest.mark.parametrize("t", E.BLOCK_TYPES)
@pytest.mark.parametrize("shape", MMQ256_SHAPES)
def test_exact_integers_on_the_resident_copy_gemms(G, O, t, shape):
    """k_mmq_w16_p8 (mmq_t256 = 0) and k_mmq_w16_256 (mmq_t256 = 2) on the shapes of tests/test_mmq256_gpu.py: one / two / many
    k-stages, ragged tiles both ways, K splits with atomics, more items than workgroups."""
    M, K, N = shape
    raw, X, ref = _exact(O, t, M, K, N)
    _same(f"k_mmq_w16_p8 type {t} {shape}", _gemm(G, t, raw, M, K, X, "w16_p8", **W16_P8), ref)
    _same(f"k_mmq_w16_256 type {t} {shape}", _gemm(G, t, raw, M, K, X, "w16_256", **W16_256), ref)


@pytest.mark.parametrize("t", E.BLOCK_TYPES)
@pytest.mark.parametrize("shape", [(300, 256, 300), (130, 4096, 70)])
def test_exact_integers_on_the_forced_dma_gemm(G, O, t, shape):
    M, K, N = shape
    raw, X, ref = _exact(O, t, M, K, N)
    _same(f"k_mmq_dma_p8 type {t} {shape}", _gemm(G, t, raw, M, K, X, "dma_p8", **DMA_P8), ref)


@pytest.mark.parametrize("t", E.BLOCK_TYPES)
@pytest.mark.parametrize("shape", [(128, 64, 32), (256, 4096, 100), (130, 1024, 300)])
def test_exact_integers_on_the_integer_gemm(G, O, t, shape):
    """k_mmq_i8: one stage, no split; 64 and 16 stages on few tiles (its K split with atomics), whole and ragged tiles."""
    M, K, N = shape
    raw, X, ref = _exact(O, t, M, K, N)
    _same(f"k_mmq_i8 type {t} {shape}", _gemm(G, t, raw, M, K, X, "i8", mmq_i8=1), ref)


@pytest.mark.parametrize("t", E.K_TYPES)
@pytest.mark.parametrize("shape", [(300, 256, 300), (130, 4096, 70), (8192 + 130, 256, 64)])
def test_exact_integers_on_the_k_quant_gemm(G, O, t, shape):
    """A K-quant weight's resident f16 copy on both tile sizes; 8192 + 130 rows cross the chunk boundary of ensure_w16_k."""
    M, K, N = shape
    for quantized in _k_variants(t):
        raw, X, ref = _exact(O, t, M, K, N, O.quantize if quantized else None)
        _same(f"K GEMM w16_p8 type {t} {shape} quantized {quantized}", _gemm(G, t, raw, M, K, X, "w16_p8", **W16_P8), ref)
        _same(f"K GEMM w16_256 type {t} {shape} quantized {quantized}", _gemm(G, t, raw, M, K, X, "w16_256", **W16_256), ref)


@pytest.mark.parametrize("t", E.BLOCK_TYPES)
@pytest.mark.parametrize("shape", [(48, 1280), (272, 2816), (16000, 1024)])
def test_exact_integers_on_the_cols_kernel(G, O, t, shape):
    """k_mmq_cols through its hook (the hook launches nothing else), 2, 5 and 8 tokens."""
    M, K = shape
    raw, X, ref = _exact(O, t, M, K, 8)
    for N in (2, 5, 8):
        rc, got = _cols(G, t, raw, M, K, X[:N])
        assert rc == 0
        _same(f"k_mmq_cols type {t} {shape} N {N}", got, ref[:N])


def _hook_launch(G, k_hook, t, raw, M, K, x):
    with G.Context(raw.nbytes + (1 << 20)) as ctx:
        w = ctx.tensor_from(raw, t, (K, M)).set_name("w")
        w.transfer_to_gpu()
        if k_hook:  # the f32 row staged and quantized in the launch, plain rows out
            return DM._selector_launch(G, True, w.ptr, DM.KF32, DM.KROW, K, M, x)[0]
        return DM._selector_launch(G, False, w.ptr, DM.XQ8, DM.EADD, K, M, x, res=np.zeros(M, F))[0]  # a planar Q8 row, + 0


@pytest.mark.parametrize("t", E.BLOCK_TYPES)
@pytest.mark.parametrize("name", ["odd_nb11_wo", "7b_wo"])
def test_exact_integers_on_the_big_mat_vec(G, O, t, name):
    """k_mmvq_big in its plainest form (the wo launch: a Q8 row in, a residual of zeros added): one narrow and the 7B case."""
    _, K, M, _ = DM.BIG[name]
    raw, X, ref = _exact(O, t, M, K, 1)
    _same(f"k_mmvq_big {name} type {t}", _hook_launch(G, False, t, raw, M, K, X[0])[None, :], ref)


@pytest.mark.parametrize("t", E.K_TYPES)
@pytest.mark.parametrize("name", ["odd_nsb3_w2", "7b_wo"])
def test_exact_integers_on_the_big_k_mat_vec(G, O, t, name):
    """k_mmvq_kbig in its plainest form (an f32 row staged in the launch, plain rows out)."""
    _, K, M, _ = DM.KBIG[name]
    for quantized in _k_variants(t):
        raw, X, ref = _exact(O, t, M, K, 1, O.quantize if quantized else None)
        _same(f"k_mmvq_kbig {name} type {t} quantized {quantized}", _hook_launch(G, True, t, raw, M, K, X[0])[None, :], ref)


# ---- B: the weight operand, read out bit for bit ---------------------------------------------------------------------------------
def _reveal_message(tag, got, want, t, raw, K):
    bad = got != want
    if not bad.any():
        return ""
    msg = f"{tag}: {int(bad.sum())} of {got.size} revealed weights differ"
    if t in E.BLOCK_TYPES:
        d = E.unpack_block(t, raw)[0].view(np.uint16)
        sub = np.repeat(((d & 0x7C00) == 0) & ((d & 0x3FF) != 0), 32).reshape(-1, K).T
        ties = E.f16_ties(E.exact_block(t, raw)).reshape(-1, K).T
        tiny = (np.abs(want) < 127 * 2.0 ** -14) & (want != 0)
        msg += (f"; {int((bad & sub).sum())} of them in blocks with a subnormal d, {int((bad & ties).sum())} at exact ties, "
                f"{int((bad & tiny).sum())} with a subnormal f16 value")
    at = np.argwhere(bad)[:6]
    return msg + f"; first (k, row) {at.tolist()}: got {[float(got[tuple(a)]) for a in at]} want {[float(want[tuple(a)]) for a in at]}"


@pytest.mark.parametrize("t", E.BLOCK_TYPES)
@pytest.mark.parametrize("kernel,K,opts", [("w16_p8", 256, W16_P8), ("w16_256", 256, W16_256), ("dma_p8", 256, DMA_P8), ("plain", 96, {})])
def test_one_hot_activations_reveal_the_f16_weight_operand(G, t, kernel, K, opts):
    """k_dequant_w16 behind both resident-copy kernels, the slice decoder of k_mmq_dma_p8, and k_mmq (K = 96: its first stage
    decodes whole blocks, its second one slices)."""
    M = 130
    raw = E.reveal_blocks(t, M * K // 32, np.random.default_rng([t, K, 3]))
    X = E.one_hot(K, 127.0)
    assert np.array_equal(E.x16_block(X, t).astype(F), X)  # the activation operand is exactly 127 or 0
    w16 = E.w16_block(t, raw, K)
    assert np.abs(w16.astype(F)).max() <= E.W16_MAX and E.f16_ties(E.exact_block(t, raw)).mean() >= 0.01
    want = (F(127.0) * w16.astype(F)).T  # exact in f32; every other product of a sum is 0 * w16 = 0
    got = _gemm(G, t, raw, M, K, X, kernel, **opts)
    assert got.shape == want.shape
    assert np.array_equal(got, want), _reveal_message(f"k_mmq_{kernel} type {t}", got, want, t, raw, K)


@pytest.mark.parametrize("t", E.K_TYPES)
def test_one_hot_activations_reveal_the_k_quant_copy_across_the_chunk_boundary(G, O, t):
    """ensure_w16_k decodes 8192 rows at a time: 8192 + 130 rows, every one revealed; the copy is f16 of the oracle's f32 decoder."""
    M, K = 8192 + 130, 256
    raw = E.reveal_k_blocks(t, M, np.random.default_rng([t, 4]))
    X = E.one_hot(K, 1.0)
    assert np.array_equal(E.x16_k(X).astype(F), X)
    w16 = np.clip(O.dequantize(t, raw, M * K), -65504.0, 65504.0).astype(np.float16).reshape(M, K)
    want = w16.astype(F).T
    for kernel, opts in (("w16_p8", W16_P8), ("w16_256", W16_256)):
        got = _gemm(G, t, raw, M, K, X, kernel, **opts)
        bad = np.argwhere(got != want)
        assert bad.shape[0] == 0, (f"{kernel} type {t}: {bad.shape[0]} of {got.size} revealed weights differ, "
                                   f"{int((bad[:, 1] >= 8192).sum())} of them in rows of the second chunk; first (k, row) {bad[:6].tolist()}")


# ---- C: random inputs, the exact operands, the accumulation bound ----------------------------------------------------------------
def _held_to_the_bound(tag, got, x16, w16):
    ref, S, bound = E.operand_product(x16, w16)
    err = np.abs(got.astype(np.float64) - ref)
    K = x16.shape[1]
    ratio = float(np.max(err[S > 0] / (K * 2.0 ** -24 * S[S > 0])))
    print(f"part C {tag}: max |got - x16 . w16| / (K 2^-24 S) = {ratio:.3f} (bound 2)")
    assert np.all(got[S == 0] == 0)
    bad = np.argwhere(err > bound)
    assert bad.shape[0] == 0, (f"{tag}: {bad.shape[0]} of {got.size} outputs beyond 2 K 2^-24 S, worst {ratio:.3f} x K 2^-24 S, "
                               f"first {bad[:6].tolist()}")


def _block_case(G, t, M, K, N, nonneg):
    W, X = E.random_inputs(M, K, N, [t, M, K, N, int(nonneg)], nonneg)
    raw = G.quantize(t, W)
    x16, w16 = E.x16_block(X, t), E.w16_block(t, raw, K)
    if nonneg:
        assert np.all(x16 >= 0) and np.all(w16 >= 0)
    return raw, X, x16, w16


C_BLOCK = [(t, False) for t in E.BLOCK_TYPES] + [(E.Q4_1, True), (E.Q5_1, True)]


@pytest.mark.parametrize("t,nonneg", C_BLOCK)
@pytest.mark.parametrize("shape", [(300, 256, 300), (1000, 1024, 513)])
def test_random_inputs_within_the_accumulation_bound_on_the_f16_gemms(G, t, nonneg, shape):
    M, K, N = shape
    raw, X, x16, w16 = _block_case(G, t, M, K, N, nonneg)
    for kernel, opts in (("w16_p8", W16_P8), ("w16_256", W16_256), ("dma_p8", DMA_P8)):
        _held_to_the_bound(f"k_mmq_{kernel} type {t} {shape} nonneg {nonneg}", _gemm(G, t, raw, M, K, X, kernel, **opts), x16, w16)


@pytest.mark.parametrize("t,nonneg", C_BLOCK)
def test_random_inputs_within_the_accumulation_bound_on_the_odd_k_gemm(G, t, nonneg):
    M, K, N = 384, 352, 100
    raw, X, x16, w16 = _block_case(G, t, M, K, N, nonneg)
    _held_to_the_bound(f"k_mmq (plain) type {t} nonneg {nonneg}", _gemm(G, t, raw, M, K, X, "plain"), x16, w16)


@pytest.mark.parametrize("t,nonneg", [(t, False) for t in E.K_TYPES] + [(E.Q4_K, True)])
def test_random_inputs_within_the_accumulation_bound_on_the_k_quant_gemm(G, O, t, nonneg):
    M, K, N = 300, 256, 300
    W, X = E.random_inputs(M, K, N, [t, M, K, N, int(nonneg)], nonneg)
    raw = O.quantize(t, W)
    x16 = E.x16_k(X)
    w16 = np.clip(O.dequantize(t, raw, M * K), -65504.0, 65504.0).astype(np.float16).reshape(M, K)
    if nonneg:
        assert np.all(x16 >= 0) and np.all(w16 >= 0)
    for kernel, opts in (("w16_p8", W16_P8), ("w16_256", W16_256)):
        _held_to_the_bound(f"K GEMM {kernel} type {t} nonneg {nonneg}", _gemm(G, t, raw, M, K, X, kernel, **opts), x16, w16)
