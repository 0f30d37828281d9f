"""GPU parity of NeoX-mode RoPE (mode & 2: GPT-NeoX, Falcon; kernels/ops.h k_rope_neox) against the NumPy restatement
of ggml's NeoX loop (tests/rotary_ref.py rope_neox), and of mode 0 with n_dims < ne0 (GPT-J) against the oracle.
Tolerance as test_rope: the device's cosf/sinf vs glibc's differ by a few ulp at |theta| up to 2e3, so
atol = 2e-5·max|x|; elements RoPE does not rotate must come through bit-identical."""
import numpy as np
import pytest

import rotary_ref

pytestmark = pytest.mark.gpu


def _tail(ne0, n_dims):
    return (ne0 // n_dims) * n_dims


@pytest.mark.parametrize("ne0,n_dims", [(128, 32), (96, 24), (64, 64), (40, 16)])
@pytest.mark.parametrize("n_past", [0, 1, 37, 2047])
@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("inplace", [True, False])
def test_rope_neox(G, ne0, n_dims, n_past, N, mode, inplace):
    H = 3
    x = np.random.default_rng([ne0, n_dims, n_past, N, mode]).standard_normal((N, H, ne0)).astype(np.float32)
    with G.Context(x.nbytes * 4 + (1 << 20)) as ctx:
        tx = ctx.tensor_from(x, G.TYPE_F32, (ne0, H, N))
        if inplace:
            out = ctx.op_cont(ctx.op_rope_inplace(tx, n_past, n_dims, mode, 0))  # the view through a real node
        else:
            out = ctx.op_rope(tx, n_past, n_dims, mode, 0)
        ctx.graph().build_forward_expand(out).compute()
        got = out.read_data().reshape(N, H, ne0)
    ref = rotary_ref.rope_neox(x, n_past, n_dims, mode=mode)
    assert np.allclose(got, ref, rtol=0, atol=2e-5 * np.abs(x).max()), np.max(np.abs(got - ref))
    t = _tail(ne0, n_dims)
    assert np.array_equal(got[..., t:], x[..., t:])  # past the last whole block: passed through
    if mode & 1:
        assert np.array_equal(got[:n_past], x[:n_past])  # rows ggml's i2 loop skips


def test_rope_neox_custom_freq(G):
    H, D, N, n_past = 2, 64, 3, 100
    x = np.random.default_rng(3).standard_normal((N, H, D)).astype(np.float32)
    with G.Context(1 << 20) as ctx:
        tx = ctx.tensor_from(x, G.TYPE_F32, (D, H, N))
        out = ctx.op_cont(ctx.op_rope_custom_inplace(tx, n_past, D, 2, 1, 26000.0, 0.5))
        ctx.graph().build_forward_expand(out).compute()
        got = out.read_data().reshape(N, H, D)
    ref = rotary_ref.rope_neox(x, n_past, D, 26000.0, 0.5)
    assert np.allclose(got, ref, rtol=0, atol=2e-5 * np.abs(x).max())


@pytest.mark.parametrize("H,Hkv,N", [(71, 1, 5), (8, 2, 1), (4, 1, 3)])
def test_rope_neox_in_place_on_fused_qkv_views(G, H, Hkv, N):
    """Falcon (falcon/src/lib.rs:218-246): Q and K are strided views of one fused [(H + 2*Hkv)*D, N] buffer, roped
    in place; the V columns next to them must come out bit-identical."""
    D, n_past = 64, 9
    W = (H + 2 * Hkv) * D
    buf = np.random.default_rng([H, Hkv, N]).standard_normal((N, W)).astype(np.float32)
    with G.Context(buf.nbytes * 4 + (1 << 20)) as ctx:
        t = ctx.tensor_from(buf, G.TYPE_F32, (W, N))
        q = ctx.op_view_3d(t, D, H, N, D * 4, W * 4, 0)
        k = ctx.op_view_3d(t, D, Hkv, N, D * 4, W * 4, H * D * 4)
        gf = ctx.graph()
        gf.build_forward_expand(ctx.op_rope_inplace(q, n_past, D, 2, 0))
        gf.build_forward_expand(ctx.op_rope_inplace(k, n_past, D, 2, 0))
        gf.compute()
        got = t.device_get().reshape(N, W)
    rq = rotary_ref.rope_neox(buf[:, :H * D].reshape(N, H, D), n_past, D).reshape(N, -1)
    rk = rotary_ref.rope_neox(buf[:, H * D:(H + Hkv) * D].reshape(N, Hkv, D), n_past, D).reshape(N, -1)
    tol = 2e-5 * np.abs(buf).max()
    assert np.allclose(got[:, :H * D], rq, rtol=0, atol=tol)
    assert np.allclose(got[:, H * D:(H + Hkv) * D], rk, rtol=0, atol=tol)
    assert np.array_equal(got[:, (H + Hkv) * D:], buf[:, (H + Hkv) * D:])


@pytest.mark.parametrize("n_past", [0, 37, 2047])
def test_rope_mode0_partial_n_dims(G, O, n_past):
    """GPT-J (gptj/src/lib.rs:178-200): mode 0 with n_dims 64 of a 256-wide head, ggml's whole-row semantics."""
    H, D, N, R = 2, 256, 5, 64
    x = np.random.default_rng(n_past).standard_normal((N, H, D)).astype(np.float32)
    with G.Context(x.nbytes * 4 + (1 << 20)) as ctx:
        tx = ctx.tensor_from(x, G.TYPE_F32, (D, H, N))
        out = ctx.op_cont(ctx.op_rope_inplace(tx, n_past, R, 0, 0))
        ctx.graph().build_forward_expand(out).compute()
        got = out.read_data().reshape(N, H, D)
    ref = O.rope(x, n_past, R)
    assert np.allclose(got, ref, rtol=0, atol=2e-5 * np.abs(x).max()), np.max(np.abs(got - ref))
