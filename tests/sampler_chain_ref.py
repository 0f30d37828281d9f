"""The extended sampler chain, restated in numpy from the written specification at the head of llm_amd/csrc/kernels/sampler_math.h
(not from the C++): np.float32 scalars with every operation rounded to f32, Python floats (IEEE f64) for the accumulations, Python
integers for the generator.  sampler_ref.py holds the default chain's restatement, its exponential and the row families; this file
adds what the specification adds: flat bias, frequency / presence penalty, tail-free, locally typical, min-p and Mirostat 2.

chain(...) below is a dict of the parameters: k, top_p, temperature, penalty, freq, presence, z, typical, min_p, bias [(id, b)],
mirostat, tau, eta."""
import math
import struct

import numpy as np

import sampler_ref as R

F = np.float32
NEUTRAL = dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30, freq=0.0, presence=0.0, z=1.0, typical=1.0, min_p=0.0, bias=(),
               mirostat=0, tau=5.0, eta=0.1)
LN2 = F(0.693147182)


def chain(**kw):
    c = dict(NEUTRAL)
    c.update(kw)
    return c


def adjusted(logits, window, ch):
    """A: {id: adjusted value} over M, the window's distinct ids united with the bias ids."""
    logits = np.asarray(logits, dtype=F)
    win = [int(t) for t in list(window)[-R.WINDOW:]]
    bias = {int(i): F(b) for i, b in ch["bias"]}
    pen, freq, presence = F(ch["penalty"]), F(ch["freq"]), F(ch["presence"])
    out = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for t in list(dict.fromkeys(win)) + [i for i in bias if i not in win]:
            v = logits[t]
            if t in bias:
                v = F(v + bias[t])
            c = win.count(t)
            if c > 0:
                v = F(v / pen) if v > 0 else F(v * pen)
                if not (freq == 0 and presence == 0):
                    v = F(v - F(F(F(c) * freq) + presence))
            out[t] = v
    return out


def candidates(logits, window, ch):
    """B: [(value, id)], the k best of the raw top-k united with M."""
    logits = np.asarray(logits, dtype=F)
    V, k = logits.size, ch["k"]
    order = np.lexsort((np.arange(V), -logits.astype(np.float64)))[:k]
    cand = {int(i): logits[i] for i in order}
    cand.update(adjusted(logits, window, ch))
    items = sorted(cand.items(), key=lambda kv: (-float(kv[1]), kv[0]))[:k]
    return [(v, i) for i, v in items]


def tail_free(q, z):
    """C.1: how many entries of the list stay."""
    n = len(q)
    if F(z) >= F(1.0) or n < 3:
        return n
    d2 = [abs((float(q[i]) - float(q[i + 1])) - (float(q[i + 1]) - float(q[i + 2]))) for i in range(n - 2)]
    D = 0.0
    for d in d2:
        D += d
    if not D > 0.0:
        return n
    need = float(F(z)) * D
    run = 0.0
    for i, d in enumerate(d2):
        run += d
        if run > need:
            return max(i, 1)
    return n


def typical(v, q, typical_p):
    """C.2: the indices that stay, ascending."""
    n = len(q)
    if F(typical_p) >= F(1.0):
        return list(range(n))
    with np.errstate(invalid="ignore"):
        s = [F(v[0] - v[i]) for i in range(n)]
    Q = 0.0
    for x in q:
        Q += float(x)
    A = 0.0
    for i in range(n):
        if q[i] > 0:
            A += float(q[i]) * float(s[i])
    mean = A / Q if Q != 0.0 else float("nan")
    t = [abs(float(s[i]) - mean) if q[i] > 0 else math.inf for i in range(n)]
    need = float(F(typical_p)) * Q
    acc, keep = 0.0, []
    for i in sorted(range(n), key=lambda i: (t[i], i)):
        keep.append(i)
        acc += float(q[i])
        if acc > need:
            break
    return sorted(keep)


def survivors(logits, window, ch):
    """B and C: (candidates, p, the surviving indices in list order)."""
    cand = candidates(logits, window, ch)
    v = np.array([c[0] for c in cand], dtype=F)
    with np.errstate(invalid="ignore"):
        d = (v - v[0]).astype(F)
        q = R.sampler_exp(d)
        p = R.sampler_exp((d / F(ch["temperature"])).astype(F))
    n = tail_free(q, ch["z"])
    idx = typical(v[:n], q[:n], ch["typical"])
    if F(ch["top_p"]) < F(1.0):
        Q = 0.0
        for j in idx:
            Q += float(q[j])
        need = float(F(ch["top_p"])) * Q
        acc = 0.0
        for m, j in enumerate(idx):
            acc += float(q[j])
            if acc >= need:
                idx = idx[:m + 1]
                break
    if F(ch["min_p"]) > 0:
        least = F(F(ch["min_p"]) * q[idx[0]])
        idx = [j for j in idx if q[j] >= least]
    return cand, p, idx


def sampler_log2(r):
    """E's logarithm: f64 in, f32 out."""
    r = float(r)
    if not r >= 2.2250738585072014e-308 or not r <= 1.7976931348623157e308:
        return F(-1022.0)
    b = struct.unpack("<Q", struct.pack("<d", r))[0]
    E = (b >> 52) - 1023
    m = struct.unpack("<d", struct.pack("<Q", (b & 0xFFFFFFFFFFFFF) | 0x3FF0000000000000))[0]
    if m >= 1.4142135623730951:
        m = m * 0.5
        E += 1
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    t = 1.0 / 15.0
    for d in (13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        t = t * s2 + 1.0 / d
    t = t * s2 + 1.0
    ln = (2.0 * s) * t
    return F(float(E) + ln * 1.4426950408889634)


def mirostat2(logits, window, ch, rng, mu):
    """E: returns (id, new generator state, new mu as f32)."""
    a = np.array(logits, dtype=F)
    for t, v in adjusted(logits, window, ch).items():
        a[t] = v
    V = a.size
    amax = a.max()
    first = int(np.flatnonzero(a == amax)[0])
    with np.errstate(invalid="ignore"):
        e = R.sampler_exp(((a - amax).astype(F) / F(ch["temperature"])).astype(F))

    def block_sums(keep):
        """S_b of every block (f64, id order inside the block, from 0) and their sum in block order: column j of the [blocks][32]
        layout is added to all blocks' sums at once, which is each block's own sequence of additions."""
        nb = (V + 31) // 32
        pad = np.zeros(nb * 32, np.float64)
        pad[:V] = np.where(keep, e.astype(np.float64), 0.0)
        live = np.zeros(nb * 32, bool)
        live[:V] = keep
        pad, live = pad.reshape(nb, 32), live.reshape(nb, 32)
        sums = np.zeros(nb, np.float64)
        for j in range(32):
            sums = np.where(live[:, j], sums + pad[:, j], sums)
        tot = 0.0
        for s in sums:
            tot += float(s)
        return [float(s) for s in sums], tot

    _, S = block_sums(np.ones(V, bool))
    mu = F(mu)
    if mu < 0:
        keep = np.zeros(V, bool)
    else:
        least = S * float(R.sampler_exp(F(-mu * LN2)))
        keep = e.astype(np.float64) >= least
    keep[first] = True
    sums, S_R = block_sums(keep)
    rng, bits = R.xorshift64star(int(rng))
    u = float(bits) / 9007199254740992.0 * S_R
    sel, run = None, 0.0
    for b, s in enumerate(sums):
        before = run
        run += s
        if run > u:
            ids = [i for i in range(32 * b, min(32 * b + 32, V)) if keep[i]]
            acc, sel = 0.0, ids[-1]
            for i in ids:
                acc += float(e[i])
                if u - before < acc:
                    sel = i
                    break
            break
    if sel is None:
        sel = int(np.flatnonzero(keep)[-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.float64(e[sel]) / np.float64(S_R))
    s_obs = F(-sampler_log2(ratio))
    mu = F(mu - F(F(ch["eta"]) * F(s_obs - F(ch["tau"]))))
    return sel, rng, mu


def sample(logits, window, ch, rng, mu):
    """One step: returns (id, new generator state, new mu as f32)."""
    if ch["mirostat"] == 2:
        return mirostat2(logits, window, ch, rng, mu)
    cand, p, idx = survivors(logits, window, ch)
    S = 0.0
    for j in idx:
        S += float(p[j])
    rng, bits = R.xorshift64star(int(rng))
    u = float(bits) / 9007199254740992.0 * S
    acc = 0.0
    for j in idx:
        acc += float(p[j])
        if u < acc:
            return cand[j][1], rng, F(mu)
    return cand[idx[-1]][1], rng, F(mu)


def bias_for(row, k, n, seed=0, ban_max=False):
    """n bias pairs for a row: ids from inside its raw top-k and from outside it, values of both signs; with ban_max the first entry
    bans the raw maximum (b = -inf)."""
    V = row.size
    g = np.random.default_rng([V, k, n, seed, 99])
    top = np.lexsort((np.arange(V), -row.astype(np.float64)))
    ids = []
    if ban_max:
        ids.append(int(top[0]))
    inside = [int(t) for t in top[:max(1, min(k, V))]]
    for i in range(4 * n + 8):
        if len(ids) >= min(n, V):
            break
        t = inside[int(g.integers(0, len(inside)))] if i % 2 == 0 else int(g.integers(0, V))
        if t not in ids:
            ids.append(t)
    for t in range(V):  # (a small vocabulary: fill up in id order)
        if len(ids) >= min(n, V):
            break
        if t not in ids:
            ids.append(t)
    out = []
    for j, t in enumerate(ids):
        b = -math.inf if (ban_max and j == 0) else float(F(g.uniform(-6.0, 6.0)))
        out.append((t, b))
    return out
