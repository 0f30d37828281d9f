"""GPU tests of ggml_alibi through the C ABI: k_alibi (kernels/ops.h) bit for bit against the restatement
(tests/alibi_ref.py: libm powf slopes, f32 product and f32 sum), and the fused scale -> alibi -> diag_mask_inf ->
soft_max launch (k_soft_max<true, true>) bit for bit against the same chain run as four launches (option fuse 0),
with the `alibi_fused` counter showing which path ran; both then against the oracle's mask + softmax.

Numeric mutants, each run once against this file and caught: every head given the first slope sequence m0^(k+1)
(fails every case with n_head not a power of two), and the position taken as i + 1 (fails every case)."""
import numpy as np
import pytest

import alibi_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bias_max", [8.0, 4.0])
@pytest.mark.parametrize("n_past", [0, 1, 127])
@pytest.mark.parametrize("N", [1, 7, 33])
@pytest.mark.parametrize("H", [1, 2, 4, 5, 12, 32, 112])
def test_alibi_matches_restatement_bit_for_bit(G, H, N, n_past, bias_max):
    T = n_past + N
    x = (np.random.default_rng([H, N, n_past]).standard_normal((H, N, T)) * 4).astype(np.float32)
    with G.Context(x.nbytes * 4 + (1 << 20)) as ctx:
        kq = ctx.op_cont(ctx.tensor_from(x, G.TYPE_F32, (T, N, H)))  # a node, as KQ is
        y = ctx.op_alibi(kq, n_past, H, bias_max)
        ctx.graph().build_forward_expand(y).compute()
        got = y.read_data().reshape(H, N, T)
    want = alibi_ref.alibi(x, n_past, H, bias_max)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.max(np.abs(got - want))


def _chain(G, x, n_past, bias_max, scale, fuse, form):
    """KQ -> scale -> alibi -> diag_mask_inf -> soft_max, as `form`:
      out_of_place  BLOOM's and MPT's graph (new S, A a view of S, new M, new P), S / A / M offloaded;
      in_place      every step in place, so P aliases KQ; S / A / M offloaded;
      mirrored      out of place with S / A / M CPU-backend nodes (mirrored to the host: must not fuse).
    Returns (P [H, N, T], fused chains counted)."""
    H, N, T = x.shape
    G.set_option("fuse", fuse)
    f0 = G.get_stat("alibi_fused")
    try:
        with G.Context(x.nbytes * 8 + (1 << 20)) as ctx:
            kq = ctx.op_cont(ctx.tensor_from(x, G.TYPE_F32, (T, N, H)))
            s = ctx.new_f32(float(scale))
            if form == "in_place":
                S = ctx.op_scale_inplace(kq, s)
                A = ctx.op_alibi(S, n_past, H, bias_max)
                M = ctx.op_diag_mask_inf_inplace(A, n_past)
                P = ctx.op_soft_max_inplace(M)
            else:
                S = ctx.op_scale(kq, s)
                A = ctx.op_alibi(S, n_past, H, bias_max)
                M = ctx.op_diag_mask_inf(A, n_past)
                P = ctx.op_soft_max(M)
            if form != "mirrored":
                for t in (S, A, M):
                    t.offload()
            ctx.graph().build_forward_expand(P).compute()
            got = P.read_data().reshape(H, N, T)
    finally:
        G.set_option("fuse", 1)
    return got, G.get_stat("alibi_fused") - f0


CHAINS = [(4, 1, 0), (12, 7, 0), (32, 1, 127), (5, 33, 1), (112, 1, 300), (32, 128, 0)]


@pytest.mark.parametrize("bias_max", [8.0, 4.0])
@pytest.mark.parametrize("form", ["out_of_place", "in_place"])
@pytest.mark.parametrize("H,N,n_past", CHAINS)
def test_fused_chain_equals_four_launches_and_restatement(G, O, H, N, n_past, form, bias_max):
    T = n_past + N
    x = (np.random.default_rng([H, N, n_past]).standard_normal((H, N, T)) * 4).astype(np.float32)
    scale = np.float32(1.0) / np.sqrt(np.float32(128.0))
    fused, n_fused = _chain(G, x, n_past, bias_max, scale, 1, form)
    plain, n_plain = _chain(G, x, n_past, bias_max, scale, 0, form)
    assert n_fused == 1 and n_plain == 0
    assert np.array_equal(fused.view(np.uint32), plain.view(np.uint32)), np.max(np.abs(fused - plain))
    ref = O.scale_mask_softmax(alibi_ref.alibi(x * scale, n_past, H, bias_max), 1.0, n_past, mode=O.ref_mode())
    # as tests/test_ops_gpu.py::test_scale_mask_softmax: exp goes through f16 on both sides, device expf vs glibc expf
    # may land on the other side of an f16 rounding boundary for a few elements (one f16 ulp, renormalised)
    assert np.allclose(fused, ref, rtol=1.5e-3, atol=1e-7), np.max(np.abs(fused - ref))
    assert np.allclose(fused.sum(-1), 1.0, atol=1e-5)
    assert np.mean(np.abs(fused - ref) > 1e-6 * np.abs(ref) + 1e-9) < 0.5


@pytest.mark.parametrize("H,N,n_past", [(12, 7, 0), (32, 1, 127)])
def test_chain_mirrored_to_host_is_not_fused(G, H, N, n_past):
    """The reference's own graph (no set_offloading): S, A and M are mirrored to the host, so they must be computed;
    the chain runs as four launches and gives the same P."""
    T = n_past + N
    x = (np.random.default_rng([H, N]).standard_normal((H, N, T)) * 4).astype(np.float32)
    scale = np.float32(0.125)
    got, n = _chain(G, x, n_past, 8.0, scale, 1, "mirrored")
    want, _ = _chain(G, x, n_past, 8.0, scale, 0, "out_of_place")
    assert n == 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
