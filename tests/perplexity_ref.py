"""A numpy restatement of InferenceSession::perplexity (crates/llm-base/src/inference_session.rs:519-589) and of
util::softmax (util.rs:143-151) over a callback evaluate(tokens) -> logits[N][V], in two forms:

* f32_sequential — the reference's arithmetic: f32 max, f32 left-to-right sum of f32 exponentials, f32 ln, f32 running nll;
* exact          — f64 throughout (the expected value of the GPU tests).

plus the error bounds the tests assert and the logits rows the op-level tests feed (shared by the CPU test, which shows that
the reference's own form passes what the device is asked to pass, and the GPU test).  No device, no product code."""
import math

import numpy as np

EPS = 2.0 ** -24  # half an ulp of f32 relative to the value: one rounding


def window(context_size):
    """[first, last) of inference_session.rs:577: positions min(512, context_size / 2) .. context_size - 2."""
    return min(512, context_size // 2), context_size - 1


def prob_exact(row, t):
    """softmax(row)[t] in f64."""
    x = np.asarray(row, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mx = np.fmax.reduce(x)  # f32::max ignores a NaN operand
        return float(np.exp(x[t] - mx) / np.sum(np.exp(x - mx)))


def prob_f32_sequential(row, t):
    """softmax(row)[t] as util.rs:143-151 computes it: everything f32, the sum left to right."""
    x = np.asarray(row, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        mx = np.fmax.reduce(x)
        e = np.exp(x - mx)  # f32 in, f32 out
        s = np.cumsum(e, dtype=np.float32)[-1]  # cumsum adds in index order, in f32
        return np.float32(e[t] / s)


def bound_device(V, dt, T=1024):
    """Allowed relative error of k_row_prob for a row of V entries whose target sits dt = x_t - max below the maximum:
    T lanes each add ceil(V / T) exponentials in sequence, a tree of log2(T) levels joins them, 4 roundings for the two expf
    (<= 1 ulp each), the subtraction and the division; |dt| for the rounding of x_t - max carried through the exponential."""
    return (math.ceil(V / T) + math.log2(T) + 4 + abs(dt)) * EPS


def bound_sequential(V, dt):
    """The same for the reference's form: V sequential adds."""
    return (V + 3 + abs(dt)) * EPS


def perplexity(evaluate, tokens, context_size, n_batch, bos=1, form="exact", new_chunk=None):
    """The reference loop.  evaluate(tokens int32[N]) -> logits [N, V] is Model::evaluate with OutputRequest.all_logits;
    new_chunk() (optional) is called before each chunk's first batch (the product starts every chunk at n_past = 0).
    Returns ([value handed to perplexity_callback(i, .) for every chunk], probs [n_chunk, last - first])."""
    assert form in ("exact", "f32_sequential")
    tokens = np.array(tokens, dtype=np.int32)  # :527 a copy: `let mut tokens`
    f = np.float32 if form == "f32_sequential" else np.float64
    prob = prob_f32_sequential if form == "f32_sequential" else prob_exact
    count = 0
    n_chunk = len(tokens) // context_size
    nll = f(0.0)
    first, last = window(context_size)
    out, probs = [], np.zeros((n_chunk, max(last - first, 0)), dtype=f)
    for i in range(n_chunk):
        start, end = i * context_size, (i + 1) * context_size
        num_batches = (context_size + n_batch - 1) // n_batch
        logits = []
        if new_chunk:
            new_chunk()
        for j in range(num_batches):
            batch_start = start + j * n_batch
            batch_size = min(end - batch_start, n_batch)
            token_org = tokens[batch_start]
            if j == 0:
                tokens[batch_start] = bos
            logits.append(np.array(evaluate(tokens[batch_start:batch_start + batch_size].copy()), dtype=np.float32))
            tokens[batch_start] = token_org
        logits = np.concatenate(logits, axis=0)
        for j in range(first, last):
            p = prob(logits[j], int(tokens[start + j + 1]))
            probs[i, j - first] = p
            with np.errstate(divide="ignore"):
                nll = f(nll + -np.log(f(p)))
            count += 1
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            out.append(float(np.exp(f(nll / f(count)))) if count else float("nan"))
    return out, probs


# ---- the rows of the op-level tests --------------------------------------------------------------------------------------
KINDS8 = ("gauss_argmax", "gauss_argmin", "peaked_random", "flat_random", "neginf_finite", "neginf_target", "far_below", "nan")
KINDS = KINDS8 + ("gauss_random", "peaked_argmax")
OP_CASES = [(1, 1, 0), (1, 8, 0), (256, 1, 0), (256, 8, 0), (256, 512, 0), (32000, 1, 0), (32000, 8, 3), (32000, 512, 0),
            (50257, 1, 0), (50257, 8, 0), (50257, 512, 0),
            (32001, 8, 1), (32764, 24, 0)]  # (V, n_rows, row_begin); the last two: rows kept in registers, unaligned / aligned


def op_rows(V, n_rows, seed=0):
    """(x [n_rows, V] f32, targets int32, kinds): gaussian N(0, 3^2) rows, peaked ones (one entry at +40), nearly flat ones,
    rows with -inf entries (target finite / the target itself -inf), a target 130 below the maximum, a NaN row; targets the
    argmax, the argmin, random.  No row has its target between 80 and 120 below the maximum.  V = 1 admits only the plain
    row (probability 1) and the NaN row; a single row is a gaussian one with a random target."""
    rng = np.random.default_rng([V, n_rows, seed])
    x = (3.0 * rng.standard_normal((n_rows, V))).astype(np.float32)
    t = rng.integers(0, V, n_rows).astype(np.int32)
    kinds = []
    for r in range(n_rows):
        if n_rows == 1:
            kind = "gauss_random"
        elif V == 1:
            kind = "nan" if r % 4 == 3 else "gauss_random"
        else:
            kind = (KINDS8 if n_rows <= 8 else KINDS)[r % (8 if n_rows <= 8 else len(KINDS))]
        kinds.append(kind)
        if kind == "gauss_argmax":
            t[r] = np.argmax(x[r])
        elif kind == "gauss_argmin":
            t[r] = np.argmin(x[r])
        elif kind in ("peaked_random", "peaked_argmax"):
            k = int(rng.integers(0, V))
            x[r, k] = 40.0
            if kind == "peaked_argmax":
                t[r] = k
        elif kind == "flat_random":
            x[r] *= np.float32(1e-3 / 3.0)
        elif kind in ("neginf_finite", "neginf_target"):
            hole = rng.random(V) < 1.0 / 3.0
            hole[int(t[r])] = kind == "neginf_target"
            hole[(int(t[r]) + 1) % V] = False  # at least one finite entry
            x[r, hole] = -np.inf
        elif kind == "far_below":
            x[r] = (x[r] / 3.0).astype(np.float32)
            x[r, t[r]] = -np.inf
            x[r, t[r]] = np.max(x[r]) - np.float32(130.0)
        elif kind == "nan":
            x[r, int(rng.integers(0, V))] = np.nan
    return x, t, kinds


def check_op_rows(x, t, kinds, got, bound):
    """Every row against the exact form: `bound(V, dt)` relative on rows whose target is >= -80 from the maximum, exactly 0
    where the target is -inf or >= 120 below the maximum, NaN for a NaN row.  Returns the worst error / bound ratio."""
    V = x.shape[1]
    worst = 0.0
    for r in range(x.shape[0]):
        if kinds[r] == "nan":
            assert np.isnan(got[r]), (r, kinds[r], got[r])
            continue
        dt = float(x[r, t[r]]) - float(np.max(x[r]))
        if kinds[r] in ("neginf_target", "far_below"):
            assert dt <= -120.0 and got[r] == 0.0, (r, kinds[r], dt, got[r])
            continue
        assert dt >= -80.0, (r, kinds[r], dt)  # no row between -80 and -120 (denormals, the flush mode)
        want = prob_exact(x[r], int(t[r]))
        rel = abs(float(got[r]) - want) / want
        b = bound(V, dt)
        assert rel <= b, (r, kinds[r], V, dt, float(got[r]), want, rel, b)
        worst = max(worst, rel / b)
    return worst
