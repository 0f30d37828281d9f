"""The sampled batched chain's sampler, restated in numpy from its written specification (not from the C++): f32 arrays with every
product, sum and quotient rounded to f32, f64 for the accumulations, Python integers for the generator.

One step, from a row of logits (free of NaN), a window of token ids and {k, top_p, temperature, penalty}:
  1. candidates: the k largest raw logits (value descending, lower id first among equals) and the window's tokens, each id once;
     a window token's value v becomes v / penalty if v > 0 else v * penalty; sorted by (value descending, id ascending), k kept;
  2. top-p (skipped when top_p >= 1): q_i = exp_(v_i - v_0), Q = sum q_i in f64 in candidate order, the shortest prefix m >= 1
     with sum_{i<m} q_i >= (double)top_p * Q;
  3. p_i = exp_((v_i - v_0) / temperature), S = sum_{i<m} p_i in f64; xorshift64*; u = ((x * 0x2545F4914F6CDD1D) >> 11) / 2^53 * S;
     the first i with u < acc_i, else candidate m - 1.
exp_ is sampler_exp: Cephes' expf scheme in separate f32 operations, exactly 0 below -80."""
import os
import re

import numpy as np

F = np.float32
MASK = (1 << 64) - 1
WINDOW = 64
_C = [F(1.9875691500e-4), F(1.3981999507e-3), F(8.3334519073e-3), F(4.1665795894e-2), F(1.6666665459e-1), F(5.0000001201e-1)]


def sampler_exp(x):
    """Vectorised over an f32 array of arguments <= 0 (or NaN / -inf, which give 0)."""
    x = np.asarray(x, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        live = x >= F(-80.0)
        xs = np.where(live, x, F(0.0)).astype(F)
        n = np.rint(xs * F(1.44269504)).astype(F)
        r = (xs - n * F(0.693359375)).astype(F)
        r = (r - n * F(-2.12194440e-4)).astype(F)
        r2 = (r * r).astype(F)
        p = np.full_like(xs, _C[0])
        for c in _C[1:]:
            p = ((p * r).astype(F) + c).astype(F)
        y = (((p * r2).astype(F) + r).astype(F) + F(1.0)).astype(F)
        scale = ((n.astype(np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(F)
        return np.where(live, (y * scale).astype(F), F(0.0)).astype(F)


def xorshift64star(x):
    """Returns (new state, the 53-bit integer the draw scales)."""
    x ^= x >> 12
    x ^= (x << 25) & MASK
    x ^= x >> 27
    return x, ((x * 0x2545F4914F6CDD1D) & MASK) >> 11


def candidates(logits, window, k, penalty):
    """[(value f32, id)] — step 1."""
    logits = np.asarray(logits, dtype=F)
    V = logits.size
    win = []
    for t in list(window)[-WINDOW:]:
        if int(t) not in win:
            win.append(int(t))
    order = np.lexsort((np.arange(V), -logits.astype(np.float64)))[:k]  # value descending (f32 -> f64 is exact), id ascending
    cand = {}
    for i in order:
        cand[int(i)] = logits[i]
    pen = F(penalty)
    with np.errstate(invalid="ignore"):
        for t in win:
            v = logits[t]
            cand[t] = F(v / pen) if v > 0 else F(v * pen)
    items = sorted(cand.items(), key=lambda kv: (-float(kv[1]), kv[0]))[:k]  # (-0.0 and 0.0 compare equal: the id decides)
    return [(v, i) for i, v in items]


def sample(logits, window, k, top_p, temperature, penalty, rng):
    """One draw: returns (id, new generator state)."""
    cand = candidates(logits, window, k, penalty)
    v = np.array([c[0] for c in cand], dtype=F)
    with np.errstate(invalid="ignore"):
        d = (v - v[0]).astype(F)
        q = sampler_exp(d)
        p = sampler_exp((d / F(temperature)).astype(F))
    m = len(cand)
    if F(top_p) < F(1.0):
        Q = 0.0
        for x in q:
            Q += float(x)
        need = float(F(top_p)) * Q
        acc = 0.0
        for i, x in enumerate(q):
            acc += float(x)
            if acc >= need:
                m = i + 1
                break
    S = 0.0
    for x in p[:m]:
        S += float(x)
    rng, bits = xorshift64star(int(rng))
    u = float(bits) / 9007199254740992.0 * S
    acc = 0.0
    for i in range(m):
        acc += float(p[i])
        if u < acc:
            return cand[i][1], rng
    return cand[m - 1][1], rng


# ---- row families shared by the CPU and GPU tests: column c of a [B][V] block carries family c mod 4
def rows(B, V, seed=0):
    """0: random with ties between neighbours and -inf entries; 1: the first and the last entry equal maxima; 2: the maximum in the
    last entry, zeros and negative zeros around; 3: all equal."""
    g = np.random.default_rng([B, V, seed])
    x = (3.0 * g.standard_normal((B, V))).astype(F)
    for c in range(B):
        f = c % 4
        if f == 0:
            if V >= 8:
                x[c, 1::7] = x[c, 0::7][: x[c, 1::7].size]  # equal values: the id decides
                x[c, 5::11] = -np.inf
        elif f == 1:
            x[c, 0] = x[c, V - 1] = F(9.0)
        elif f == 2:
            x[c, 0::5] = F(0.0)
            x[c, 2::5] = F(-0.0)
            x[c, V - 1] = F(11.0)
        else:
            x[c, :] = F(-0.5)
    return x


def window_for(row, k, n, seed=0):
    """n history tokens for a row: some of its raw top-k (so penalised values of every sign move inside and out of it), some random
    ids, with repeats."""
    V = row.size
    g = np.random.default_rng([V, k, n, seed])
    top = np.lexsort((np.arange(V), -row.astype(np.float64)))[: max(1, min(k, V))]
    picks = []
    for i in range(n):
        picks.append(int(top[g.integers(0, top.size)]) if i % 2 == 0 else int(g.integers(0, V)))
    return np.array(picks, dtype=np.int32)


# ---- the cases of "the kernel alone", for one session (tests/test_sample_chain_gpu.py) and for B columns (tests/test_batch_sample_gpu.py)
def _cap():
    """Rows up to this many entries take the on-chip selection, longer ones topk_kth_key over global memory (kernels/sample.h)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "llm_amd", "csrc", "kernels", "sample.h")).read()
    per_thread = int(re.search(r"constexpr int SELECT_PER_THREAD = (\d+);", src).group(1))
    assert "constexpr int SELECT_CAP = 1024 * SELECT_PER_THREAD;" in src
    return 1024 * per_thread


CAP = _cap()
# (V, k, n_draws, top_p, temperature): k = min(40, V) and k = 256 at V = 1000; 70 draws on a small V fill the ring and wrap it; V =
# 32000 and 32001, where the vector loads' tail appears; then the last row of the on-chip selection and the first of the selection
# over global memory, each with k = 40 and k = 256
ALONE = [(1, 1, 3, 0.95, 0.8), (3, 3, 3, 1.0, 1.0), (41, 40, 70, 0.95, 0.8), (1000, 40, 3, 1e-6, 0.1), (1000, 256, 3, 0.95, 1.0),
         (32000, 40, 3, 0.95, 0.8), (32001, 40, 2, 0.95, 0.8),
         (CAP, 40, 3, 0.95, 0.8), (CAP, 256, 3, 0.95, 0.8), (CAP + 1, 40, 3, 0.95, 0.8), (CAP + 1, 256, 3, 0.95, 0.8)]
