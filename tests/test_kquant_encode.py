"""Host K-quant encoders of the ABI (ggml_quantize_q2_K .. q6_K, ggml_quantize_chunk: llm_amd/csrc/ggml_core.cpp) byte for
byte against the oracle's quantize_row_q*_K, the fit every K-quant weight of this project is made with
(oracle/SEMANTICS.md; parity with upstream's scale search is unpinned).  Runs on the CPU."""
import ctypes as C

import numpy as np
import pytest

import kquant_cases
from llm_amd import ggml as G
from oracle import oracle as O

SHAPES = [(256, 1), (768, 3), (11008, 2)]  # the last: 43 super-blocks per row


@pytest.fixture(scope="module")
def inputs():
    return {s: kquant_cases.tensor(*s, seed=[7, *s])[0] for s in SHAPES}


@pytest.mark.parametrize("ne0,ne1", SHAPES)
@pytest.mark.parametrize("t", kquant_cases.K_TYPES)
def test_quantize_matches_the_oracle(inputs, t, ne0, ne1):
    x = inputs[(ne0, ne1)]
    got, want = G.quantize(t, x), O.quantize_row(t, x)
    assert got.size == G.row_bytes(t, ne0) * ne1
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8] // G.BLOCK_BYTES[t]


@pytest.mark.parametrize("t", kquant_cases.K_TYPES)
def test_every_edge_block_alone(t):
    """One super-block per call (k = n = 256), so a mismatch names its case."""
    for i, b in enumerate(kquant_cases.edge_blocks(np.random.default_rng(3), np.float32(0.02))):
        assert np.array_equal(G.quantize(t, b), O.quantize_row(t, b)), i


@pytest.mark.parametrize("t", kquant_cases.K_TYPES)
def test_return_value_and_untouched_hist(inputs, t):
    x = inputs[(768, 3)]
    out = np.zeros(G.row_bytes(t, x.size), np.uint8)
    pattern = np.arange(16, dtype=np.int64) * 1000003 - 17
    hist = pattern.copy()
    fn = getattr(G.lib(), "ggml_quantize_" + G.TYPE_NAMES[t])
    assert fn(x.ctypes.data, out.ctypes.data, x.size, 768, hist.ctypes.data) == G.row_bytes(t, 768) * 3
    assert np.array_equal(hist, pattern)
    assert np.array_equal(out, O.quantize_row(t, x))
    assert fn(x.ctypes.data, out.ctypes.data, x.size, 768, None) == out.size  # a NULL hist is accepted


@pytest.mark.parametrize("t", kquant_cases.K_TYPES)
def test_chunk_in_two_halves_equals_the_whole(inputs, t):
    x = inputs[(11008, 2)].reshape(-1)
    n, start = x.size, 256 * 37
    whole, halves = np.zeros(G.row_bytes(t, n), np.uint8), np.zeros(G.row_bytes(t, n), np.uint8)
    pattern = np.full(16, 5, np.int64)
    hist = pattern.copy()
    L = G.lib()
    assert L.ggml_quantize_chunk(t, x.ctypes.data, whole.ctypes.data, 0, n, hist.ctypes.data) == whole.size
    assert L.ggml_quantize_chunk(t, x.ctypes.data, halves.ctypes.data, 0, start, hist.ctypes.data) == G.row_bytes(t, start)
    assert L.ggml_quantize_chunk(t, x.ctypes.data, halves.ctypes.data, start, n - start, hist.ctypes.data) == G.row_bytes(t, n - start)
    assert np.array_equal(whole, halves) and np.array_equal(whole, O.quantize_row(t, x))
    assert np.array_equal(hist, pattern)
