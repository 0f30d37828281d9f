"""CPU tests of the whole sampler (no GPU): llm_sample_chain — kernels/sampler_math.h compiled for the host, the header the device
kernel compiles too — against tests/sampler_chain_ref.py, a numpy restatement of the written specification at the head of that
header.  Ids, generator states and the bit pattern of Mirostat's mu are compared for equality; sampler_log2 is measured against
math.log2."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_chain_ref as X  # noqa: E402
import sampler_ref as R  # noqa: E402

VS = [(3, 3), (41, 40), (1000, 40), (32000, 40)]  # (V, k)
# each stage alone (top_p = 1, so that nothing else truncates), then every truncating stage together behind bias and both penalties
STAGES = {
    "bias": dict(top_p=1.0, n_bias=6),
    "freq_presence": dict(top_p=1.0, freq=0.3, presence=0.2),
    "tail_free": dict(top_p=1.0, z=0.9),
    "typical": dict(top_p=1.0, typical=0.5),
    "min_p": dict(top_p=1.0, min_p=0.2),
    "all": dict(top_p=0.95, freq=0.3, presence=0.2, z=0.9, typical=0.5, min_p=0.2, n_bias=6),
}
_rows = {}


def _family_rows(V):
    if V not in _rows:
        _rows[V] = R.rows(4, V, seed=11)
        _rows[V].setflags(write=False)
    return _rows[V]


def _chain_for(row, k, stage, f, ban=False):
    """The restatement's chain dict of a stage: bias ids from inside and outside the row's raw top-k (bias_for), the first of them
    taken from the window too where there is one; with `ban` the raw maximum gets -inf."""
    kw = dict(STAGES[stage])
    n_bias = kw.pop("n_bias", 0)
    ch = X.chain(k=k, temperature=0.8, penalty=1.30, **kw)
    if n_bias:
        ch["bias"] = X.bias_for(row, k, n_bias, seed=f, ban_max=ban)
    return ch


def _window_with(row, k, n, f, ch):
    w = list(R.window_for(row, k, n, seed=f))
    if ch["bias"] and w:
        w[len(w) // 2] = ch["bias"][-1][0]  # a biased id that is also in the window
    return w


def _lib_kw(ch):
    return dict(k=ch["k"], top_p=ch["top_p"], temperature=ch["temperature"], penalty=ch["penalty"], freq=ch["freq"], presence=ch["presence"],
                tail_free_z=ch["z"], typical_p=ch["typical"], min_p=ch["min_p"], bias=ch["bias"], mirostat=ch["mirostat"], tau=ch["tau"],
                eta=ch["eta"])


def _draw(row, window, rng, mu, ch):
    from llm_amd import llama
    state = np.array([rng], dtype=np.uint64)
    m = np.array([mu], dtype=np.float32)
    tok = llama.sample_chain(row, window, state, m if ch["mirostat"] else None, **_lib_kw(ch))
    return tok, int(state[0]), m.view(np.uint32)[0]


def _bits(mu):
    return np.array([mu], np.float32).view(np.uint32)[0]


@pytest.mark.parametrize("stage", list(STAGES))
@pytest.mark.parametrize("V,k", VS)
def test_ids_and_states_equal_the_specification(V, k, stage):
    """Four row families, windows of 0 / 5 / 64 / 80 tokens from inside and outside the raw top-k, each moving on over the ids
    drawn; bias ids inside and outside the raw top-k, one of them in the window, and (second round) a -inf ban of the raw maximum."""
    rows = _family_rows(V)
    for f in range(4):
        for n_window, ban in ((0, False), (5, True), (64, False), (80, True)):
            ch = _chain_for(rows[f], k, stage, f, ban)
            window = _window_with(rows[f], k, n_window, f, ch)
            rng = 0x9E3779B97F4A7C15 ^ (V * 1000003 + f * 101 + n_window)
            for draw in range(3):
                want, want_rng, _ = X.sample(rows[f], window, ch, rng, 0.0)
                got, got_rng, _ = _draw(rows[f], window, rng, 0.0, ch)
                assert (got, got_rng) == (want, want_rng), (f, n_window, draw)
                window.append(got)
                rng = got_rng


@pytest.mark.parametrize("V,k,n_draws", [(3, 3, 70), (41, 40, 70), (1000, 40, 70), (32000, 40, 70)])
def test_mirostat_2_equals_the_specification(V, k, n_draws):
    """Mirostat 2 over 70 consecutive draws on every row family (the window fills and wraps, mu moves every time), with bias — a ban
    of the raw maximum among it — and both penalties; ids, generator state and mu's bits."""
    rows = _family_rows(V)
    for f in range(4):
        ch = X.chain(k=k, top_p=1.0, temperature=0.8, penalty=1.30, freq=0.1, presence=0.1, mirostat=2, tau=3.0, eta=0.25,
                     bias=X.bias_for(rows[f], k, 5, seed=f, ban_max=f == 1))
        window = _window_with(rows[f], k, 5, f, ch)
        rng, mu = 0xD1B54A32D192ED03 + f, np.float32(2 * 3.0)
        for draw in range(n_draws):
            want, want_rng, want_mu = X.sample(rows[f], window, ch, rng, mu)
            got, got_rng, got_mu = _draw(rows[f], window, rng, mu, ch)
            assert (got, got_rng, got_mu) == (want, want_rng, _bits(want_mu)), (f, draw)
            window.append(got)
            rng, mu = got_rng, want_mu
        assert _bits(mu) != _bits(6.0)


def test_mirostat_2_below_zero_keeps_the_maximum_alone():
    row = np.ascontiguousarray(_family_rows(41)[0])
    ch = X.chain(top_p=1.0, mirostat=2, tau=3.0, eta=0.25)
    want, want_rng, want_mu = X.sample(row, [], ch, 99, np.float32(-0.5))
    got, got_rng, got_mu = _draw(row, [], 99, -0.5, ch)
    assert want == int(np.argmax(row)) and (got, got_rng, got_mu) == (want, want_rng, _bits(want_mu))


@pytest.mark.parametrize("f", [0, 1, 2, 3])
@pytest.mark.parametrize("V,k,n_draws,top_p,temperature", R.ALONE)
def test_neutral_extras_are_the_default_chain(V, k, n_draws, top_p, temperature, f):
    """With neutral extras llm_sample_chain gives llm_sample_exact's id and generator state (and leaves mu alone), on every case of
    sampler_ref.ALONE."""
    from llm_amd import llama
    row = np.ascontiguousarray(_family_rows(V)[f]) if V in (3, 41, 1000, 32000) else np.ascontiguousarray(R.rows(4, V, seed=11)[f])
    window = list(R.window_for(row, k, (0, 5, 64, 30)[f], seed=f))
    a, b = np.array([12345 + V + f], np.uint64), np.array([12345 + V + f], np.uint64)
    mu = np.array([7.5], np.float32)
    for _ in range(n_draws):
        want = llama.sample_exact(row, window, a, k=k, top_p=top_p, temperature=temperature, penalty=1.30)
        got = llama.sample_chain(row, window, b, mu, k=k, top_p=top_p, temperature=temperature, penalty=1.30)
        assert got == want and int(a[0]) == int(b[0]) and float(mu[0]) == 7.5
        window.append(got)


def _survivor_counts(stage, neutral_key, neutral_value):
    """[(survivors with the stage's chain, survivors with that filter made neutral)] over the stage's cases — the restatement alone."""
    out = []
    for V, k in VS:
        rows = _family_rows(V)
        for f in range(4):
            ch = _chain_for(rows[f], k, stage, f)
            window = _window_with(rows[f], k, 5, f, ch)
            off = dict(ch)
            off[neutral_key] = neutral_value
            out.append((len(X.survivors(rows[f], window, ch)[2]), len(X.survivors(rows[f], window, off)[2])))
    return out


@pytest.mark.parametrize("stage,key,neutral", [("tail_free", "z", 1.0), ("typical", "typical", 1.0), ("min_p", "min_p", 0.0),
                                               ("all", "z", 1.0), ("all", "typical", 1.0), ("all", "min_p", 0.0)])
def test_every_filter_bites_on_its_cases(stage, key, neutral):
    """A property of the inputs, asserted on the numpy restatement alone: over the cases of a stage its filter drops a candidate in
    at least one and leaves more than one in at least one (a filter that never acts, or always cuts to one, would test nothing)."""
    counts = _survivor_counts(stage, key, neutral)
    print(stage, key, counts)
    assert any(a < b for a, b in counts), counts
    assert any(a > 1 for a, _ in counts), counts


def test_bias_and_penalties_move_candidates():
    """... and so do the value stages: with bias / frequency and presence the ordered candidate list differs from the default's."""
    for stage in ("bias", "freq_presence"):
        moved = 0
        for V, k in VS:
            rows = _family_rows(V)
            for f in range(4):
                ch = _chain_for(rows[f], k, stage, f, ban=True)
                window = _window_with(rows[f], k, 5, f, ch)
                moved += X.candidates(rows[f], window, ch) != X.candidates(rows[f], window, X.chain(k=k, temperature=0.8, top_p=1.0))
        assert moved >= 4, (stage, moved)


def test_sampler_log2_against_f64_log2():
    """Over the ratios Mirostat 2 forms — e an f32 in (1e-35, 1] over S in [1, 32768], and exact powers of two: measured maximum
    relative error of the f32 result against math.log2 5.952e-8 (1.0 * 2^-24: the final rounding); asserted at twice that, 1.19e-7 —
    the figure written beside sampler_log2 in the header.  Exactly the exponent at powers of two, 0 at 1.  The library's function
    equals the restatement's on every point."""
    from llm_amd import llama
    g = np.random.default_rng(77)
    e = np.exp(g.uniform(math.log(1e-35), 0.0, 200_000)).astype(np.float32).astype(np.float64)
    S = np.exp(g.uniform(0.0, math.log(32768.0), 200_000))
    r = np.concatenate([e / S, e, 1.0 / S, 2.0 ** np.arange(-140, 1, dtype=np.float64), [np.nextafter(1.0, 0.0), np.nextafter(0.5, 1.0)]])
    r = np.ascontiguousarray(r[r > 0])
    out = np.zeros(r.size, np.float32)
    llama._lib().llm_sampler_log2(r.ctypes.data, r.size, out.ctypes.data)
    ref = np.array([math.log2(x) for x in r])
    mine = np.array([X.sampler_log2(x) for x in r[:20000]], np.float32)
    assert np.array_equal(mine.view(np.uint32), out[:20000].view(np.uint32))
    nz = ref != 0
    err = float(np.max(np.abs(out.astype(np.float64)[nz] - ref[nz]) / np.abs(ref[nz])))
    print(f"sampler_log2 max relative error {err:.3e}")
    assert err <= 1.19e-7, err
    p2 = 2.0 ** np.arange(-140, 1, dtype=np.float64)
    out2 = np.zeros(p2.size, np.float32)
    llama._lib().llm_sampler_log2(p2.ctypes.data, p2.size, out2.ctypes.data)
    assert np.array_equal(out2, np.arange(-140, 1, dtype=np.float32))


DECLINED = [dict(k=0), dict(k=17), dict(temperature=0.0), dict(top_p=0.0), dict(penalty=0.0), dict(temperature=float("nan")),
            dict(freq=float("nan")), dict(presence=float("nan")), dict(tail_free_z=0.0), dict(tail_free_z=float("nan")),
            dict(typical_p=0.0), dict(typical_p=-1.0), dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=float("nan")),
            dict(bias=[(16, 1.0)]), dict(bias=[(-1, 1.0)]), dict(bias=[(3, 1.0), (3, 2.0)]), dict(bias=[(3, float("nan"))]),
            dict(bias=[(3, float("inf"))]), dict(mirostat=1), dict(mirostat=3), dict(mirostat=2, top_p=0.9),
            dict(mirostat=2, top_p=1.0, tail_free_z=0.9), dict(mirostat=2, top_p=1.0, typical_p=0.9), dict(mirostat=2, top_p=1.0, min_p=0.1),
            dict(mirostat=2, top_p=1.0, tau=0.0), dict(mirostat=2, top_p=1.0, eta=-0.1), dict(tau=float("nan")), dict(eta=float("nan")),
            dict(tau=-1.0), dict(eta=-1.0)]


@pytest.mark.parametrize("kw", DECLINED, ids=[",".join(f"{k}={v}" for k, v in d.items()) for d in DECLINED])
def test_what_is_declined_moves_no_state(kw):
    from llm_amd import llama
    row = np.zeros(16, np.float32)
    state, mu = np.array([77], dtype=np.uint64), np.array([6.0], np.float32)
    with pytest.raises(ValueError):
        llama.sample_chain(row, [1, 2], state, mu, **kw)
    assert int(state[0]) == 77 and float(mu[0]) == 6.0


def test_more_declines():
    """A NaN mu under Mirostat 2, n_bias outside 0 .. 64 (set in the struct: the keyword form cannot say it), a window token outside
    the vocabulary; a -inf bias and k left at 40 under Mirostat 2 on 16 entries are fine."""
    import ctypes as C
    from llm_amd import llama
    row = np.zeros(16, np.float32)
    state, mu = np.array([77], dtype=np.uint64), np.array([np.nan], np.float32)
    with pytest.raises(ValueError):
        llama.sample_chain(row, [1], state, mu, mirostat=2, top_p=1.0)
    with pytest.raises(ValueError):
        llama.sample_chain(row, [1, 16], state, None)
    assert int(state[0]) == 77
    L, win = llama._lib(), np.array([1], np.int32)
    for n_bias in (-1, 65):
        c = llama.sampler_chain(k=4)
        c.n_bias = n_bias
        assert L.llm_sample_chain(row.ctypes.data, 16, win.ctypes.data, 1, C.addressof(c), state.ctypes.data, None) == -1
    assert int(state[0]) == 77
    mu[0] = 6.0
    assert 0 <= llama.sample_chain(row, [1], state, mu, k=40, mirostat=2, top_p=1.0, bias=[(0, -math.inf)]) < 16
    assert int(state[0]) != 77 and float(mu[0]) != 6.0
