"""ggml_alibi as a graph node (llm_amd/csrc/ggml_core.cpp), on the CPU: the accepted layout (KQ f32 [n_past + N, N,
n_head], the one BLOOM bloom/src/lib.rs:240 and MPT mpt/src/lib.rs:180-181 build) makes a view of `a` with
op_params {n_past, n_head, bits of bias_max}; every other layout aborts at construction with the out-of-path message.
Both are run in a subprocess, so a library that aborts on the accepted layout fails the test instead of pytest.
The slope table of alibi_ref (ggml's) is also checked against Hugging Face BLOOM's and MPT's formulas."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import alibi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRELUDE = "import sys; sys.path.insert(0, %r); from llm_amd import ggml as G\n" % ROOT


def _run(code):
    return subprocess.run([sys.executable, "-c", PRELUDE + code], capture_output=True, text=True)


@pytest.mark.parametrize("n_past,N,H,bias_max", [(0, 7, 4, 8.0), (127, 1, 32, 8.0), (3, 2, 12, 4.0), (0, 1, 256, 8.0)])
def test_accepted_layout_is_a_view_with_op_params(n_past, N, H, bias_max):
    code = ("import ctypes, json, struct\n"
            f"c = G.Context(1 << 24); a = c.new_tensor(G.TYPE_F32, {n_past + N}, {N}, {H})\n"
            f"r = c.op_alibi(a, {n_past}, {H}, {bias_max})\n"
            "p = list(r.t.op_params)\n"
            "print(json.dumps(dict(op=G.lib().ggml_op_name(r.t.op).decode(),\n"
            "    src0=ctypes.addressof(r.t.src[0].contents) == ctypes.addressof(a.t), src1=bool(r.t.src[1]),\n"
            "    data=r.t.data == a.t.data, ne=list(r.ne), nb=list(r.nb) == list(a.nb), type=r.t.type,\n"
            "    params=p[:2], bias=struct.unpack('<f', struct.pack('<i', p[2]))[0], rest=p[3:])))")
    p = _run(code)
    assert p.returncode == 0, p.stderr
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["op"] == "ALIBI" and got["src0"] and not got["src1"]
    assert got["data"] and got["nb"] and got["type"] == 0  # a view of a: ALiBi works in place
    assert got["ne"] == [n_past + N, N, H, 1]
    assert got["params"] == [n_past, H] and got["bias"] == bias_max and got["rest"] == [0] * 5


@pytest.mark.parametrize("ne,n_past,H,bias_max", [
    ((9, 2, 3), 7, 4, 8.0),        # ne[2] != n_head
    ((9, 2, 4, 2), 7, 4, 8.0),     # ne[3] != 1
    ((10, 2, 4), 7, 4, 8.0),       # ne[0] != n_past + ne[1]
    ((9, 2, 300), 7, 300, 8.0),    # n_head > 256
    ((9, 2, 4), 7, 4, "float('inf')"),  # bias_max not finite
])
def test_rejected_layouts_abort_without_fallback(ne, n_past, H, bias_max):
    code = (f"c = G.Context(1 << 24); a = c.new_tensor(G.TYPE_F32, {', '.join(map(str, ne))})\n"
            f"c.op_alibi(a, {n_past}, {H}, {bias_max})\nprint('constructed')")
    p = _run(code)
    assert p.returncode != 0 and "no CPU compute fallback" in p.stderr and "constructed" not in p.stdout, p


def _hf_bloom_slopes(n):
    """transformers' build_alibi_tensor (BLOOM): f32 base per sequence, torch.pow in f32."""
    cp2 = 2 ** math.floor(math.log2(n))
    base = np.float32(2 ** (-(2 ** -(math.log2(cp2) - 3))))
    s = [np.float32(np.float64(base) ** p) for p in range(1, 1 + cp2)]
    if cp2 != n:
        extra = np.float32(2 ** (-(2 ** -(math.log2(2 * cp2) - 3))))
        s += [np.float32(np.float64(extra) ** p) for p in range(1, 1 + 2 * min(cp2, n - cp2), 2)]
    return np.array(s, np.float32)


def _hf_mpt_slopes(n, bias_max):
    """transformers' build_mpt_alibi_tensor: 2^ceil(log2 n) slopes 1/2^(k*bias_max/n_pow2), the odd-indexed ones first
    when n is not a power of two."""
    n2 = 2 ** math.ceil(math.log2(n))
    base = np.arange(1, n2 + 1, dtype=np.float32) * np.float32(bias_max / n2)
    s = (np.float32(1.0) / np.power(np.float32(2.0), base)).astype(np.float32)
    if n2 != n:
        s = np.concatenate([s[1::2], s[::2]])[:n]
    return s


@pytest.mark.parametrize("n_head", range(1, 129))
def test_slopes_match_huggingface_bloom_and_mpt(n_head):
    """Same table, also when n_head is not a power of two, to f32 rounding: ggml and HF BLOOM raise an f32 base to the
    power p = k + 1 or 2(k - n_floor) + 1 (powf vs torch.pow); HF MPT takes 2^(-p*bias_max/n) directly, so its base's
    rounding is not raised to the power: the relative gap is bounded by (p + 1) * 2^-24."""
    got = alibi_ref.slopes(n_head, 8.0)
    n_floor = 1 << int(math.floor(math.log2(n_head)))
    k = np.arange(n_head)
    p = np.where(k < n_floor, k + 1, 2 * (k - n_floor) + 1)
    for want in (_hf_bloom_slopes(n_head), _hf_mpt_slopes(n_head, 8.0)):
        assert want.shape == got.shape
        rel = np.abs(got.astype(np.float64) - want) / want
        assert (rel <= (p + 1) * 2.0 ** -24).all(), (rel.max(), (rel / ((p + 1) * 2.0 ** -24)).max())


def test_alibi_restatement_elementwise():
    """(float)i * m_k + x with i the key position (column), n_past not in the bias; f32 product and sum."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((5, 3, 7)).astype(np.float32)
    y = alibi_ref.alibi(x, 4, 5, 8.0)
    m = alibi_ref.slopes(5, 8.0)
    for k in range(5):
        for j in range(3):
            for i in range(7):
                assert y[k, j, i] == np.float32(np.float32(i) * m[k]) + x[k, j, i]
    # n_floor = 4: m0 = 2^(-8/4), heads 0..3 take m0^1..m0^4; m1 = 2^(-4/4), head 4 takes m1^1
    assert list(m) == [0.25, 2.0 ** -4, 2.0 ** -6, 2.0 ** -8, 0.5]
