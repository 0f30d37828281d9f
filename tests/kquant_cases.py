"""Inputs for the K-quant encoder tests (host: test_kquant_encode.py, device: test_kquant_encode_gpu.py, the requantizing
add: test_lora_kquant_gpu.py): scale * gaussian f32 [ne1, ne0] whose first super-blocks (256 values, in memory order)
are overwritten with the cases where an encoder can go wrong.  No f32 subnormals anywhere."""
import numpy as np

K_TYPES = (10, 11, 12, 13, 14)  # Q2_K, Q3_K, Q4_K, Q5_K, Q6_K
ENC_SHAPES = [(256, 1), (256, 5), (768, 3), (11008, 2), (4096, 64)]  # (ne0, ne1): one super-block; a count that is no
# multiple of the four per workgroup; an odd count per row; 43 per row; a mid-size tensor


def edge_blocks(rng, scale):
    """The edge super-blocks, each f32 [256]."""
    def gauss(n=256):
        return (scale * rng.standard_normal(n)).astype(np.float32)

    a = np.float32(2.5 * scale)
    out = []
    out.append(np.zeros(256, np.float32))  # an all-zero super-block
    b = gauss(); b[32:64] = 0.0; out.append(b)  # an all-zero sub-block inside a non-zero super-block
    b = gauss(); b[64:96] = np.abs(b[64:96]) + np.float32(1e-3 * scale); out.append(b)  # only positive: lo stays 0, min 0
    out.append(np.abs(gauss()))  # only non-negative values in the whole super-block: max_min == 0, inv_min = 0
    b = gauss(); b[0:32] = -np.abs(b[0:32]) - np.float32(1e-3 * scale); out.append(b)  # a sub-block of only negative values
    b = gauss() * np.float32(0.1)  # [+a, -a, ...] and [-a, +a, ...]: the first value of largest magnitude wins
    b[0:16] = np.tile(np.float32([a, -a]), 8)
    b[16:32] = np.tile(np.float32([-a, a]), 8)
    b[32:64] = np.tile(np.float32([a, -a]), 16)
    out.append(b)
    b = gauss() * np.float32(0.1)  # two sub-block scales of equal magnitude and opposite sign, the positive extreme first
    b[5 * 16 + 7] = a
    b[9 * 16 + 2] = -a
    out.append(b)
    b = gauss() * np.float32(0.1)  # the same, the negative extreme first
    b[3 * 16 + 15] = -a
    b[12 * 16 + 0] = a
    out.append(b)
    b = gauss() * np.float32(1e-3); b[128:160] = gauss(32); out.append(b)  # one sub-block 1000 x the rest: scale codes 0
    out.append((np.float32(1e-9) * rng.choice(np.float32([-1.0, 1.0]), 256)).astype(np.float32))  # f16(d) underflows to 0
    b = gauss(); b[::3] = np.float32(-0.0); b[96:128] = np.float32(-0.0); out.append(b)  # -0.0 entries, a -0.0 sub-block
    out.append(np.full(256, -0.0, np.float32))  # nothing but -0.0
    return out


def tensor(ne0, ne1, seed, scale=0.02):
    """scale * gaussian f32 [ne1, ne0]; the first super-blocks are the edge cases (at least the last one stays gaussian).
    Returns (x, number of edge super-blocks written)."""
    assert ne0 % 256 == 0
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal((ne1, ne0))).astype(np.float32)
    flat = x.reshape(-1, 256)
    edges = edge_blocks(rng, np.float32(scale))
    n = min(len(edges), flat.shape[0] - 1)
    for i in range(n):
        flat[i] = edges[i]
    tiny = np.abs(x[x != 0])
    assert tiny.size == 0 or tiny.min() >= np.float32(1.2e-38)  # no subnormals
    return x, n
