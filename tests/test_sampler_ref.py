"""CPU tests of the sampled batched chain's sampler (no GPU): llm_sample_exact — kernels/sampler_math.h compiled for the host, the
header the device kernel compiles too — against tests/sampler_ref.py, a numpy restatement of the written specification.  Ids and
generator states are compared for equality; sampler_exp is measured against numpy's f64 exp."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as R  # noqa: E402


def _draw(logits, window, rng, **kw):
    from llm_amd import llama
    state = np.array([rng], dtype=np.uint64)
    tok = llama.sample_exact(logits, window, state, **kw)
    return tok, int(state[0])


CASES = [(1, 1), (8, 8), (41, 40), (1000, 40)]  # (V, k): V = 1 with k = 1, V = k, ...


@pytest.mark.parametrize("V,k", CASES)
@pytest.mark.parametrize("top_p", [1.0, 0.95, 1e-6])
@pytest.mark.parametrize("temperature", [0.1, 0.8, 1.0])
def test_ids_and_generator_states_equal_the_specification(V, k, top_p, temperature):
    """Four row families (equal values, -inf entries, zeros of both signs, an all-equal row), windows of 0 / 5 / 64 / 80 tokens taken
    from inside and outside the raw top-k (penalised values of every sign), each window moving on over the ids drawn: 4 x 4 x 5
    draws per case, 2880 in all."""
    rows = R.rows(4, V, seed=7)
    for c in range(4):
        for n_window in (0, 5, 64, 80):
            window = list(R.window_for(rows[c], k, n_window, seed=c))
            rng = 0x9E3779B97F4A7C15 ^ (V * 1000003 + c * 101 + n_window)
            for draw in range(5):
                want, want_rng = R.sample(rows[c], window, k, top_p, temperature, 1.30, rng)
                got, got_rng = _draw(rows[c], window, rng, k=k, top_p=top_p, temperature=temperature, penalty=1.30)
                assert (got, got_rng) == (want, want_rng), (c, n_window, draw)
                window.append(got)
                rng = got_rng


def test_the_candidates_are_the_raw_top_k_and_the_window_penalised():
    """The candidate set is the specification's: the raw top-k united with the window's tokens, penalised, the k best kept.  A window
    token from below the raw top-k can enter only by value; one inside it that the penalty pushes down is NOT replaced by the raw
    (k + 1)-th logit — where that matters the set is narrower than penalise-everything-then-top-k, on the host and on the device
    alike.  Every candidate is drawn at temperature 1."""
    V, k = 64, 4
    row = np.linspace(-2.0, 4.0, V).astype(np.float32)
    window = [63, 62, 0, 61]
    pen = row.copy()
    for t in set(window):
        pen[t] = row[t] / np.float32(1.3) if row[t] > 0 else row[t] * np.float32(1.3)
    pool = {60, 61, 62, 63, 0}  # raw top-4 and the window
    want = sorted(pool, key=lambda i: (-float(pen[i]), i))[:k]
    assert want == [60, 63, 62, 61]
    assert [i for _, i in R.candidates(row, window, k, 1.3)] == want
    seen = set()
    rng = 12345
    for _ in range(200):
        tok, rng = _draw(row, window, rng, k=k, top_p=1.0, temperature=1.0, penalty=1.30)
        seen.add(tok)
    assert seen == set(want)


def test_bad_arguments_move_no_generator():
    from llm_amd import llama
    row = np.zeros(16, np.float32)
    for kw in (dict(k=0), dict(k=17), dict(temperature=0.0), dict(top_p=0.0), dict(penalty=0.0), dict(temperature=-1.0)):
        state = np.array([77], dtype=np.uint64)
        with pytest.raises(ValueError):
            llama.sample_exact(row, [1, 2], state, **kw)
        assert int(state[0]) == 77
    state = np.array([77], dtype=np.uint64)
    with pytest.raises(ValueError):
        llama.sample_exact(row, [1, 16], state)  # a window token outside the vocabulary
    assert int(state[0]) == 77


def test_sampler_exp_against_f64_exp():
    """Over 3 000 001 evenly spaced f32 points of [-80, 0] and 10^6 random ones: measured maximum relative error against numpy's f64
    exp 7.934e-8 (1.33 * 2^-24); asserted at twice that, 1.587e-7.  Exactly 1 at 0 (and -0), exactly 0 below -80 and for -inf;
    monotone on the sorted sample."""
    g = np.random.default_rng(2024)
    x = np.concatenate([np.linspace(-80.0, 0.0, 3_000_001).astype(np.float32), (-80.0 * g.random(1_000_000)).astype(np.float32)])
    x = np.sort(x)
    y = R.sampler_exp(x)
    ref = np.exp(x.astype(np.float64))
    err = float(np.max(np.abs(y.astype(np.float64) - ref) / ref))
    print(f"sampler_exp max relative error {err:.3e}")
    assert err <= 1.587e-7, err
    assert np.all(np.diff(y) >= 0)
    assert R.sampler_exp(np.float32(0.0)) == np.float32(1.0) and R.sampler_exp(np.float32(-0.0)) == np.float32(1.0)
    below = np.array([np.nextafter(np.float32(-80.0), np.float32(-np.inf)), -81.0, -1e30, -np.inf], dtype=np.float32)
    assert np.all(R.sampler_exp(below) == 0.0) and R.sampler_exp(np.float32(-80.0)) > 0


def test_the_library_computes_that_exponential():
    """Two candidates, top_p = 1, temperature 1: candidate 0 is drawn iff u * (1 + sampler_exp(d)) < 1, so the draws depend on the
    library's sampler_exp(d) alone.  2000 values of d over [-80, 0] and beyond it, three draws each, equal to the restatement's (the
    one test_sampler_exp_against_f64_exp measures)."""
    g = np.random.default_rng(5)
    ds = np.concatenate([(-80.0 * g.random(1990)).astype(np.float32), np.array([0, -0.0, -80, -80.00001, -100, -1e-7, -1e-3, -0.5,
                                                                                 -79.9999, -17.32868], dtype=np.float32)])
    for d in ds:
        row = np.array([0.0, d], dtype=np.float32)
        rng = int(g.integers(1, 2 ** 63))
        for _ in range(3):
            want, want_rng = R.sample(row, [], 2, 1.0, 1.0, 1.30, rng)
            got, got_rng = _draw(row, [], rng, k=2, top_p=1.0, temperature=1.0, penalty=1.30)
            assert (got, got_rng) == (want, want_rng), d
            rng = got_rng


def test_frequencies_follow_the_softmax():
    """20 000 draws from an 8-candidate row (top_p = 1, no window) with one fixed seed land within 5 sigma of the f64 softmax of
    logits / temperature; the outcome is deterministic."""
    row = np.array([2.0, 1.5, 1.0, 0.5, 0.0, -0.5, -1.0, -3.0], dtype=np.float32)
    T, n = 0.8, 20000
    e = np.exp((row.astype(np.float64) - 2.0) / T)
    prob = e / e.sum()
    counts = np.zeros(8, np.int64)
    rng = 0x0123456789ABCDEF
    for _ in range(n):
        tok, rng = _draw(row, [], rng, k=8, top_p=1.0, temperature=T, penalty=1.30)
        counts[tok] += 1
    sigma = np.sqrt(n * prob * (1 - prob))
    z = np.abs(counts - n * prob) / sigma
    print("z", np.round(z, 2))
    assert np.all(z <= 5.0), (counts, z)
