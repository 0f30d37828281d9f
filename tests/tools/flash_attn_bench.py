#!/usr/bin/env python3
"""GGML_OP_FLASH_ATTN against the unfused chain it replaces, on the same inputs and the same (generic) executor.

  python tests/tools/flash_attn_bench.py [--rounds 7] [--reps 20] [--out profiles/flash_attn.json]

Per shape: the flash node and the chain mul_mat(K, Q) -> scale -> diag_mask_inf -> soft_max -> mul_mat(V, P) are each built
once in one context and computed `reps` times per round, the two alternating round by round after a warm-up round of each.
The time is the sum of the device-event intervals around every launch of the graph (ggml_hip_timing_*: what the device spent
in the kernels; the gaps between the chain's launches are NOT in it, which favours the chain), per compute, and the median
over the rounds is reported with the fastest and slowest round.  The host wall time per compute (it ends in the read-back of the
result and includes the upload of the operands, the same bytes for both) is reported beside it for information.
For the tile shape a second yardstick is k_p_attn on contiguous inputs (ggml_hip_debug_prompt_attention), timed the same way.
A run without a GPU fails; nothing here falls back."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import flash_attn_graph as FG  # noqa: E402
import flash_attn_ref as F  # noqa: E402
from llm_amd import ggml as G  # noqa: E402

# name: B, N, H, Hkv, D, M, masked, f32
SHAPES = {
    "prompt_7b": (1, 512, 32, 32, 128, 512, True, False),    # LLaMA-7B prompt batch, P = 0: k_flash_attn_tile
    "decode_7b": (1, 1, 32, 32, 128, 2048, True, False),     # one token behind 2047: k_flash_attn_row
    "prompt_f32": (1, 64, 16, 16, 64, 576, True, True),      # an f32 graph (GPT-2 sized heads), P = 512: k_flash_attn_row
}


def _device_ms():
    return sum(G.timing_query(k)[0] for k in (G.KCLASS_MMVQ, G.KCLASS_MMQ_MFMA, G.KCLASS_ATTN, G.KCLASS_OTHER))


def _launches():
    return sum(G.timing_query(k)[1] for k in (G.KCLASS_MMVQ, G.KCLASS_MMQ_MFMA, G.KCLASS_ATTN, G.KCLASS_OTHER))


def _timed(fn, reps):
    """(device-event us per call, launches per call, wall us per call) of `reps` calls of fn."""
    L = G.lib()
    L.ggml_hip_synchronize()
    L.ggml_hip_timing_begin()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    L.ggml_hip_synchronize()
    wall = time.perf_counter() - t0
    L.ggml_hip_timing_end()
    return _device_ms() * 1e3 / reps, _launches() / reps, wall * 1e6 / reps


def _summary(rows):
    dev = [r[0] for r in rows]
    return dict(device_us_median=statistics.median(dev), device_us_min=min(dev), device_us_max=max(dev), launches=rows[0][1],
                wall_us_median=statistics.median(r[2] for r in rows))


def bench_shape(name, rounds, reps):
    B, N, H, Hkv, D, M, masked, f32 = SHAPES[name]
    C_ = M
    q, k, v = F.gauss_inputs(B, N, H, Hkv, D, M, C_)
    if f32:
        k, v = F.as_f32_caches(k, v)
    res = dict(shape=dict(B=B, N=N, H=H, Hkv=Hkv, D=D, M=M, masked=masked, kv="f32" if f32 else "f16"))
    with G.Context(FG.context_bytes(q, k, v, H, M)) as c:
        Q, K, V = FG.operands(c, G, q, k, v, D, H, Hkv, M)
        yf = FG.flash(c, Q, K, V, masked)
        yc = FG.chain(c, Q, K, V, D, M - N, masked)
        gf = c.graph().build_forward_expand(yf)
        gc = c.graph().build_forward_expand(yc)
        runs = {"flash": gf.compute, "chain": gc.compute}
        for fn in runs.values():  # warm-up: code objects, LDS attributes, device shadows
            _timed(fn, 3)
        rows = {"flash": [], "chain": []}
        for _ in range(rounds):
            for key, fn in runs.items():
                rows[key].append(_timed(fn, reps))
        a = yf.read_data(np.float32)
        b = yc.read_data(np.float32)
        res["max_abs_diff_flash_vs_chain"] = float(np.abs(a - b).max())
        assert not np.isnan(a).any() and res["max_abs_diff_flash_vs_chain"] < 1e-2
    for key in rows:
        res[key] = _summary(rows[key])
    if name == "prompt_7b":  # k_p_attn on contiguous inputs, the same values
        E = H * D
        out = np.zeros((N, E), np.float32)
        q2, k2, v2 = np.ascontiguousarray(q[0]), np.ascontiguousarray(k[0]), np.ascontiguousarray(v[0])
        scale = float(F.scale_of(D))

        def pattn():
            assert G.lib().ggml_hip_debug_prompt_attention(q2.ctypes.data, k2.ctypes.data, v2.ctypes.data, out.ctypes.data, N, E, Hkv * D,
                                                           H, M - N, C_, scale, 1) == 0

        _timed(pattn, 3)
        res["k_p_attn"] = _summary([_timed(pattn, reps) for _ in range(rounds)])
        res["tile_over_k_p_attn"] = res["flash"]["device_us_median"] / res["k_p_attn"]["device_us_median"]
    res["chain_over_flash"] = res["chain"]["device_us_median"] / res["flash"]["device_us_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="", help="recorded in the output")
    args = ap.parse_args()
    if not G.has_gpu():
        raise SystemExit("flash_attn_bench: no HIP device")
    res = dict(tool="tests/tools/flash_attn_bench.py", device=G.lib().ggml_hip_version().decode(), commit=args.commit, rounds=args.rounds,
               reps=args.reps, unit="us per graph compute, sum of device-event intervals around the launches", shapes={})
    for name in SHAPES:
        r = bench_shape(name, args.rounds, args.reps)
        res["shapes"][name] = r
        print("%-11s flash %8.1f us (%d launch)   chain %8.1f us (%d launches)   chain / flash %.2f%s" % (
            name, r["flash"]["device_us_median"], r["flash"]["launches"], r["chain"]["device_us_median"], r["chain"]["launches"],
            r["chain_over_flash"], "   k_p_attn %.1f us, tile / k_p_attn %.2f" % (r["k_p_attn"]["device_us_median"], r["tile_over_k_p_attn"])
            if "k_p_attn" in r else ""), flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
