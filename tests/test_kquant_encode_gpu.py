"""GPU test of the device K-quant encoder (ggml_hip_quantize for Q2_K .. Q6_K: kernels/kquant_encode.h k_quantize_k, one wave
per super-block): byte for byte the oracle's quantize_row_q*_K on gaussian tensors whose first super-blocks are the cases
where the kernel can go wrong (tests/kquant_cases.py), at one super-block, at counts that are no multiple of the four per
workgroup, at an odd count per row and at a mid-size tensor."""
import numpy as np
import pytest

import kquant_cases
from llm_amd import ggml as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _k_encoders_present():
    """A library without the K encoders fails this module here, in Python, before any device call."""
    assert hasattr(G.lib(), "ggml_quantize_q4_K"), "libggml_hip.so exports no ggml_quantize_q4_K"


@pytest.fixture(scope="module")
def inputs():
    return {s: kquant_cases.tensor(*s, seed=[11, *s])[0] for s in kquant_cases.ENC_SHAPES}


@pytest.mark.parametrize("ne0,ne1", kquant_cases.ENC_SHAPES)
@pytest.mark.parametrize("t", kquant_cases.K_TYPES)
def test_device_encoder_matches_the_oracle(inputs, t, ne0, ne1):
    x = inputs[(ne0, ne1)]
    got, hist = G.quantize_on_device(t, x)
    want = O.quantize_row(t, x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], bad[:8] // G.BLOCK_BYTES[t])  # byte offsets, super-blocks (the first ones: kquant_cases)
    assert not hist.any()  # no histogram for the K types: hist is left as it was


@pytest.mark.parametrize("t", kquant_cases.K_TYPES)
def test_every_edge_block_in_one_tensor(t):
    """All edge super-blocks of kquant_cases in one 13-block tensor, each reported by its index."""
    blocks = kquant_cases.edge_blocks(np.random.default_rng(5), np.float32(0.02))
    x = np.stack(blocks + [np.linspace(-0.05, 0.05, 256, dtype=np.float32)])
    bs = G.BLOCK_BYTES[t]
    got = G.quantize_on_device(t, x)[0].reshape(-1, bs)
    want = O.quantize_row(t, x).reshape(-1, bs)
    assert [i for i in range(len(x)) if not np.array_equal(got[i], want[i])] == []
    assert np.array_equal(got.reshape(-1), G.quantize(t, x))  # and the host function of the ABI
