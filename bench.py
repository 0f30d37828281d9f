#!/usr/bin/env python
"""bench.py — decode tokens/s of LLaMA-7B Q4_0 on MI355X through the drop-in C ABI (BASELINE.json metric); with --full
also the mat-vec kernel's HBM roofline, the oracle parity check and the restated ggml CPU path timed beside it.

  python bench.py --gpus 1 --steps K --warmup W [--full] [--dump-outputs DIR]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A plain run sets up (weights, upload, prompt), warms up W steps, times K steps and prints one JSON line; --full adds every
other leg of the decode run (parity check, roofline replays, call-sequence / device-sampling / long-context legs, steady prompt
feed, prefill leg, CPU baseline).  --dump-outputs DIR writes the last timed step's token id and logits as DIR/*.npy; the inputs
are seeded, so two builds given the same arguments can be compared output for output.

A "step" is one greedy decode token of one sequence per pipeline slot: InferenceSession::infer_next_token
(host argmax + Model::evaluate of N=1) exactly as crates/llm-base/src/inference_session.rs:381-424 drives it.
N=1 workload = BASELINE.json configs[1]: LLaMA-7B Q4_0 single-token decode, 128-token synthetic prompt,
context 2048, f16 KV, weights resident in HBM before the timed region.
N>1 = ggml-style layer split: rank r owns layers [r*L/N, (r+1)*L/N); the residual [E] f32
crosses each boundary by RCCL send/recv; N independent sequences are kept in flight (one per stage), so per-GPU
work per step is constant ("weak"): value = tokens of all sequences / time.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md "HBM3E peak BW 8.0 TB/s"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=128, help="timed decode tokens (BASELINE.md section 3: 128)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--model", default="7b", choices=["7b", "13b", "65b", "tiny"])
    ap.add_argument("--wtype", default="q4_0", choices=["q4_0", "q4_1", "q5_0", "q5_1", "q8_0", "q2_k", "q3_k", "q4_k", "q5_k", "q6_k"])
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--cpu-secs", type=float, default=15.0, help="budget of the CPU-baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity-check", action="store_true", help="skip the oracle check of the token after the timed loop")
    ap.add_argument("--no-per-layer-check", action="store_true", help="... keep the whole-model check, skip the one-layer-at-a-time one")
    ap.add_argument("--roofline-steps", type=int, default=20)
    ap.add_argument("--headline-only", action="store_true", help="stop the decode run behind the timed steps + roofline replays: no call-sequence, device-sampling or long-context legs (the PMC passes: every dispatch then runs at the context the roofline bytes are stated for)")
    ap.add_argument("--split", type=int, default=2, help="--mode split: device slots ONE session is layer-split over (one process)")
    ap.add_argument("--sessions", default="1,2,4", help="--mode sessions: session counts to run, comma-separated")
    ap.add_argument("--sessions-unchanged-caller", action="store_true",
                    help="--mode sessions: every thread only calls start_session() / infer; slots are assigned by the backend under GGML_HIP_SESSION_SLOTS")
    ap.add_argument("--mode", default="decode", choices=["decode", "prefill", "feed", "split", "sessions"],
                    help="decode = BASELINE configs[1] (the metric); prefill = configs[2], 512-token prompt batch on MFMA; "
                         "feed = InferenceSession::feed_prompt in chunks of --n-batch (profiling leg)")
    ap.add_argument("--n-batch", type=int, default=8, help="--mode feed: tokens per Model::evaluate (the reference's default is 8)")
    ap.add_argument("--prefill-tokens", type=int, default=512)
    ap.add_argument("--prefill-steps", type=int, default=5, help="timed 512-token prefill steps of the default run's configs[2] leg (0 = skip)")
    ap.add_argument("--weights", default="gaussian", choices=["gaussian", "blocks"],
                    help="gaussian = BASELINE.md section 4 (N(0, 0.02^2) quantized by ggml_quantize_q*); blocks = random valid blocks (faster to make)")
    ap.add_argument("--full", action="store_true",
                    help="--mode decode: also run everything beside the headline (oracle parity check, roofline replays, call-sequence, "
                         "device-sampling and long-context legs, steady prompt feed, prefill leg, CPU baseline); without it the run sets "
                         "up, warms up, times --steps tokens and prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="--mode decode, one GPU: after the timed steps write what the last timed step handed its caller as DIR/<name>.npy "
                         "(token.npy: the token id infer_next_token returned, float64 [1]; last_logits.npy: the session's logits, float32 [n_vocab])")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and (args.mode != "decode" or args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        ap.error("--dump-outputs is implemented for --mode decode on one GPU")
    return args


def dump_outputs(path, arrays):
    """--dump-outputs: one DIR/<name>.npy per array, float32 or float64, 64 MB at most in all."""
    total = sum(a.nbytes for a in arrays.values())
    if total > 64 << 20 or any(a.dtype not in (np.float32, np.float64) for a in arrays.values()):
        raise SystemExit(f"bench.py: --dump-outputs takes float32 / float64 arrays of 64 MB at most ({total} bytes)")
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))


def build_model(args, layer_range=None):
    from llm_amd import ggml, llama, synth
    hp = {"7b": synth.LLAMA_7B, "13b": synth.LLAMA_13B, "65b": synth.LLAMA_65B, "tiny": synth.TINY}[args.model]
    wtype = {"q4_0": ggml.TYPE_Q4_0, "q4_1": ggml.TYPE_Q4_1, "q5_0": ggml.TYPE_Q5_0, "q5_1": ggml.TYPE_Q5_1,
             "q8_0": ggml.TYPE_Q8_0, "q2_k": ggml.TYPE_Q2_K, "q3_k": ggml.TYPE_Q3_K, "q4_k": ggml.TYPE_Q4_K, "q5_k": ggml.TYPE_Q5_K,
             "q6_k": ggml.TYPE_Q6_K}[args.wtype]
    if wtype in ggml.K_TYPES and args.weights == "gaussian":
        args.weights = "blocks"  # the library has no K-quant encoder
    t0 = time.perf_counter()
    hp, w = (synth.make_llama_gaussian if args.weights == "gaussian" else synth.make_llama_fast)(hp, wtype)
    t1 = time.perf_counter()
    ctx = 2048 if args.model != "tiny" else 256
    model = llama.Llama(hp, w, context_size=ctx)
    t2 = time.perf_counter()
    return hp, w, model, {"gen_s": t1 - t0, "upload_s": t2 - t1}


def weight_bytes_per_token(hp, wtype_bytes, blck=32):
    E, F, V, L = hp["n_embd"], hp["n_ff"], hp["n_vocab"], hp["n_layer"]
    Egqa = E // (hp["n_head"] // hp["n_head_kv"])
    params = L * (2 * E * E + 2 * E * Egqa + 3 * E * F) + V * E  # 7 mat-vecs per layer + lm_head
    return params // blck * wtype_bytes, params


def cpu_quota():
    """CPUs' worth of time the container may use (cgroup v2 cpu.max / v1 cfs quota), None = unlimited or unknown: a box that
    shows 256 CPUs but is capped at 32 explains a team-size calibration that peaks at 32 threads."""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else round(int(q) / int(p), 2)
    except Exception:
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else round(q / p, 2)
    except Exception:
        return None


def cpu_baseline(args, hp, w, budget_s):
    """ggml's CPU path as the reference's build selects it (crates/ggml/sys/build.rs:46-62: -mavx2 -mfma -mf16c), restated
    with the AVX2 intrinsics themselves (oracle mode 3: _mm256_maddubs_epi16 / _mm256_madd_epi16 block dots, 8-lane fmadd,
    _mm256_round_ps activation quantizer, F16C attention dots; bit-identical to the order restatement the CPU tests pin),
    OpenMP over rows where ggml uses its thread pool, timed on this host's cores.  Falls back to the scalar restatement
    (mode 0, kind "port") on a host without AVX2."""
    from llm_amd import synth
    from oracle import oracle
    mode = 3 if oracle.have_avx2() else 0
    os.environ.setdefault("OMP_WAIT_POLICY", "PASSIVE")
    ncpu = len(os.sched_getaffinity(0))
    tok = np.array([1], np.int32)
    L = oracle.lib()
    L.orc_first_touch_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
    L.orc_pin_threads.restype = ctypes.c_int
    shapes = synth.tensor_shapes(hp)

    def placed(thr):
        """The model with its OpenMP team pinned (spread over the host's CPUs) and every matrix copied so that the thread that
        will read a row is the one that first touched its pages (NUMA first-touch; on a two-socket host the un-placed copy made
        the team SLOWER beyond 16 threads in round 3).  Untimed: ggml's mmap'd weights settle the same way after a few tokens."""
        L.orc_set_num_threads(thr)
        L.orc_pin_threads()
        w2 = {}
        for name, a in w.items():
            ne1 = shapes[name][1]
            if ne1 is None:
                w2[name] = a
                continue
            c = np.empty_like(a)  # untouched pages
            L.orc_first_touch_copy(c.ctypes.data, a.ctypes.data, ne1, a.nbytes // ne1)
            w2[name] = c
        return oracle.Llama(hp, w2, 256)

    best, tried = None, {}
    spent = 0.0
    # calibrate the team size: one warm-up token (page faults of the K/V cache, thread start) + two timed tokens each (the better counts)
    for thr in sorted({t for t in (8, 16, 32, 64, 128, ncpu) if t <= ncpu} | {min(ncpu, 8)}):
        o = placed(thr)
        o.evaluate(tok, mode=mode)
        dt = None
        for _ in range(2):  # the better of two timed tokens: on a shared host one token caught a neighbour's burst often enough to pick a team half the size
            t = time.perf_counter()
            o.evaluate(tok, mode=mode)
            d1 = time.perf_counter() - t
            dt = d1 if dt is None else min(dt, d1)
            spent += d1
        spent += dt
        tried[thr] = round(dt, 3)
        # a team bigger than the cgroup's CPU quota runs one token at full speed and is throttled as soon as the sample lasts
        # longer than a scheduler period (seen: 32 threads on a 16-CPU quota, 0.036 s for the calibration token, 0.11 s per
        # token over the 60-token sample): rank the team sizes by the time the quota lets them sustain
        q = cpu_quota()
        eff = dt * max(1.0, thr / q) if q else dt
        if best is None or eff < best[2]:
            best = (thr, dt, eff)
        del o
        if spent > 0.5 * budget_s:
            break
    thr, dt1 = best[0], best[2]
    orc = placed(thr)
    orc.evaluate(tok, mode=mode)
    n = int(max(1, min(60, (budget_s - spent) / max(dt1, 1e-3))))
    t = time.perf_counter()
    for _ in range(n):
        orc.evaluate(tok, mode=mode)
    el = time.perf_counter() - t
    L.orc_unpin_threads()
    L.orc_set_num_threads(min(ncpu, 16))
    return {"value": round(n / el, 3), "unit": "tokens/s", "cores": thr, "kind": "port-avx2" if mode == 3 else "port",
            "sample": f"{n} single-token decode steps of the same {args.model} {args.wtype} weights at short context "
                      f"(oracle mode {mode}, OpenMP, {thr} pinned threads = the fastest of the calibrated team sizes the CPU quota sustains; "
                      "weights first-touched by the threads that read them)",
            "calibration_s_per_token": {str(k): v for k, v in tried.items()}, "host_cpus": ncpu,
            "host_cpu_quota": cpu_quota(),
            "note": ("ggml's AVX2 code path restated with the same intrinsics (block dots by maddubs/madd, fmadd lanes, F16C), "
                     "bit-identical to oracle mode 2; not ggml's binary (its C sources are an empty submodule in the reference "
                     "tree), so thread pool and cache blocking are this port's") if mode == 3 else
                    "scalar restatement of ggml's CPU path (-O3 -mavx2): a lower bound on the reference"}


MMQ_KERNELS = (  # stat key suffix -> what the launch is (ggml_hip_get_stat("mmq_launches_<key>"))
    ("w16_256", "k_mmq_w16_256 (persistent 256x256x64 f16 GEMM, 8 waves in two staggered groups, both operands by LDS-DMA from "
                "resident f16 copies of the quantized weights, v_mfma_f32_32x32x16_f16)"),
    ("w16_p8", "k_mmq_w16_p8 (persistent 128x128x64 f16 GEMM, 8 waves, both operands by LDS-DMA from resident f16 copies of the "
               "quantized weights, v_mfma_f32_32x32x16_f16)"),
    ("dma_p8", "k_mmq_dma_p8 (persistent 128x128x64 GEMM, 8 waves, quantized blocks by LDS-DMA, in-LDS dequant to f16, "
               "v_mfma_f32_32x32x16_f16)"),
    ("plain", "k_mmq (K/32 odd only: one workgroup per tile, register-staged, in-LDS dequant to f16)"),
    ("i8", "k_mmq_i8 (integer MFMA, exact block dots)"),
)


def mmq_counts(L):
    return {k: int(L.ggml_hip_get_stat(("mmq_launches_" + k).encode())) for k, _ in MMQ_KERNELS}


def mmq_label(before, after):
    """Names the prompt-GEMM kernels that actually ran between two mmq_counts() snapshots, most launches first."""
    d = {k: after[k] - before[k] for k in after}
    ran = sorted((k for k in d if d[k] > 0), key=lambda k: -d[k])
    names = dict(MMQ_KERNELS)
    return "; ".join(f"{d[k]} x {names[k]}" for k in ran) or "none", d


PARITY_EDGE = 4e-2  # tests/test_llama_gpu.py EDGE: one int8 activation quant on a rounding edge


def parity_check(args, hp, w, sess):
    """The token the timed loop would evaluate next, evaluated by the device AND by the CPU oracle from the same K/V state —
    the oracle in the mode that restates what the reference's build EXECUTES (crates/ggml/sys/build.rs:46-62: ggml's AVX2
    branches = mode 3 / 2; the device's activation quantizer follows that branch), with the scalar branch (mode 0) printed
    beside it: the session's K/V cache (what the timed steps wrote) is copied into the oracle, both
    evaluate argmax(last logits) at the session's n_past.  The yardstick is the reference's OWN ambiguity measured in the
    same run: the oracle with its f32 block sums added in reverse order (a second legal order of ggml's vec_dot; upstream's
    scalar and AVX2 branches differ by as much) gives `band`, the math mode (no activation quantization) the noise floor.
    With the gaussian weights of BASELINE.md section 4 a LLaMA-7B is far more sensitive than with random blocks (band
    ~1e-1 std vs ~3e-3, tests/test_c3_gpu.py).  The run FAILS if the device is further from the oracle than
    max(PARITY_EDGE, 2 * band) or than the floor.  The oracle is the checker here, never the thing measured."""
    from oracle import oracle
    ctx = sess.model.context_size
    n_past = sess.n_past
    tok = np.array([int(np.argmax(sess.last_logits()))], np.int32)
    k, v = sess.get_kv()
    orcs = [oracle.Llama(hp, w, ctx) for _ in range(4)]
    mode = oracle.ref_mode()
    for o in orcs:
        o.memory_k[:] = k
        o.memory_v[:] = v
        o.n_past = n_past
    assert sess.infer_next_token() == int(tok[0])  # InferenceSession::infer_next_token: argmax of the last logits, evaluated
    got = sess.last_logits()
    t = time.perf_counter()
    ref_all, taps = orcs[0].evaluate(tok, mode=mode, taps=True)
    ref = ref_all[-1]
    ref_s = time.perf_counter() - t
    rev = orcs[1].evaluate(tok, mode=mode, reverse_blocks=True)[-1]
    mth = orcs[2].evaluate(tok, mode=1)[-1]
    sca = orcs[3].evaluate(tok, mode=0)[-1]  # ggml's scalar branch, for the record
    k2, v2 = sess.get_kv()
    std = float(mth.std())
    d = float(np.max(np.abs(got - ref))) / std
    rms = float(np.sqrt(np.mean((got - ref) ** 2))) / std
    band = float(np.max(np.abs(ref - rev))) / std
    floor = float(np.max(np.abs(ref - mth))) / std
    d_scalar = float(np.max(np.abs(got - sca))) / std
    branches = float(np.max(np.abs(ref - sca))) / std
    # K/V rows the token wrote: layer 0 depends on the embedding and wk / wv only (must agree up to a last-bit rounding of a few
    # halves); deeper layers of a random-init model amplify a last-bit difference chaotically (that is what `band` measures)
    Eg = hp["n_embd"] // (hp["n_head"] // hp["n_head_kv"])
    kg, ko = k2[n_past * Eg:(n_past + 1) * Eg], orcs[0].memory_k[n_past * Eg:(n_past + 1) * Eg]
    vg, vo = v2[:ctx * Eg].reshape(Eg, ctx)[:, n_past], orcs[0].memory_v[:ctx * Eg].reshape(Eg, ctx)[:, n_past]
    nk0 = int(np.count_nonzero(kg != ko)) + int(np.count_nonzero(vg != vo))
    nk = int(np.count_nonzero(k2 != orcs[0].memory_k)) + int(np.count_nonzero(v2 != orcs[0].memory_v))
    bound = max(PARITY_EDGE, 2.0 * band)
    # ... and no further than the math mode is (dropping the activation quantization altogether) — unless the oracle's own two
    # summation orders already differ by more than that (6-bit weights: floor ~ band ~ 5e-2)
    # (K-quant lines: random valid blocks, where the three yardsticks and the device's distance are all the same size — Q6_K at 264
    # positions: d 0.0557, floor 0.0550, band 0.0528 — so the second clause has 25 % of slack there; the headline's has none)
    slack = 1.25 if args.wtype.endswith("_k") else 1.0
    ok = d <= bound and d <= slack * max(floor, PARITY_EDGE, band) and nk0 <= 0.01 * 2 * Eg
    out = {"max_over_std": float(f"{d:.3e}"), "rms_over_std": float(f"{rms:.3e}"),
           "argmax_equal": bool(int(np.argmax(got)) == int(np.argmax(ref))),
           "oracle_fwd_vs_rev_band_over_std": float(f"{band:.3e}"), "oracle_exact_vs_math_floor_over_std": float(f"{floor:.3e}"),
           "second_clause_slack": slack,
           "bound_over_std": float(f"{bound:.3e}"), "passed": bool(ok),
           "kv_layer0_halves_that_differ": nk0, "kv_layer0_halves_written": int(2 * Eg),
           "kv_all_layers_halves_that_differ": nk, "kv_all_layers_halves_written": int(2 * hp["n_layer"] * Eg),
           "n_past": int(n_past),
           "oracle": f"oracle/ggml_oracle.c mode {mode} (ggml's AVX2 branch, what the reference's build runs: crates/ggml/sys/"
                     "build.rs:46-62; restated, parity unpinned: DESIGN.md section 5); the device's activation quantizer follows "
                     "that branch (option act_quant = 0)",
           "vs_scalar_branch_mode0": {"device_max_over_std": float(f"{d_scalar:.3e}"),
                                      "avx2_vs_scalar_oracle_max_over_std": float(f"{branches:.3e}")},
           "oracle_s": round(ref_s, 2),
           "what": "logits of the next decode token after the timed steps, device vs CPU oracle on the session's own K/V; band = "
                   "the oracle against itself with the block sums in reverse order, floor = against its math mode"}
    if not ok:
        print(json.dumps({"parity_check": out}), flush=True)
        raise SystemExit(f"bench.py: parity check failed: max |dlogit| = {d:.3e} std > bound {bound:.3e} (band {band:.3e}, floor {floor:.3e})")
    if not args.no_per_layer_check:
        # K-quant lines (random valid blocks, Q8_K activations: ONE scale per 256 values, so one flipped quant moves a layer's output about
        # twice as far as with 32-value blocks — Q6_K, round 5's kernels and this round's alike: 1.4e-2 in one layer of 32): 2e-2
        out["per_layer"] = per_layer_check(hp, w, k, v, n_past, tok, ctx, taps, ref, std, edge=2e-2 if args.wtype.endswith("_k") else None)
        sess.infer_next_token()  # freeing the stage models' device tensors dropped the cached plans: one more token rebuilds the session's
        out["whole_model_note"] = ("max_over_std / bound_over_std above compare LOGITS behind the whole stack: information (the bound is the "
                                   "oracle's own two-order band, which a deep random-init stack makes wide); per_layer is the check")
        if not out["per_layer"]["passed"]:
            print(json.dumps({"parity_check": out}), flush=True)
            raise SystemExit(f"bench.py: per-layer parity check failed: worst {out['per_layer']['worst_max']} > bound {out['per_layer']['bound_max']}")
    return out


LAYER_STRICT, LAYER_CAP = 2e-5, 1e-1  # tests/test_ref_branch_gpu.py: an evaluation without a flipped quant; the cap on any layer
# ... and what ONE int8 activation quant on a rounding edge does to one layer's output (a quarter of the whole-model PARITY_EDGE).  Only
# the random-BLOCK weights of --weights blocks ever need it: there most layers agree to 1e-5 and the oracle's own two orders differ by
# 2e-3 in the one layer where THEY flip a quant, so "2 x band" is one coin against another (gpurun_out/r6/run21: layer 0 device 5.6e-3,
# band 1.9e-3; layer 13 device 6.4e-4, band 1.1e-5).  With the gaussian weights of the driver's run 2 x band = 5e-2 rules.
LAYER_EDGE = 1e-2


def per_layer_check(hp, w, k, v, n_past, tok, ctx, taps, ref_logits, logit_std, edge=None):
    """EVERY layer of the bench's model, alone, at the bench's own operating point (the session's n_past, the kernels the timed
    steps ran): layer il is a one-layer stage on the device (crates/models/llama/src/lib.rs:174-338 for that layer; the last one
    with the final norm and lm_head, :340-352) fed with the ORACLE's input row of that layer and the session's K/V of the positions
    before the token, its output row held against the oracle's.  Yardstick per layer = the oracle against itself with its block
    sums in reverse order on the same row (tests/test_ref_branch_gpu.py _layers_alone: the same method on five layers of a
    six-layer stack at position 21).  A 32-layer stack of gaussian weights amplifies one flipped int8 quant chaotically — the
    whole-model number above is information; ONE layer cannot hide behind that."""
    import ctypes as C
    from oracle import oracle
    from llm_amd import ggml, llama, synth
    L, E = hp["n_layer"], hp["n_embd"]
    Eg = E // (hp["n_head"] // hp["n_head_kv"])
    per = ctx * Eg
    mode = oracle.ref_mode()
    rows, worst, band_mx, band_rms, n_strict = [], 0.0, 0.0, 0.0, 0
    fw0 = int(ggml.lib().ggml_hip_get_stat(b"fused_wo_tokens"))
    fa0 = int(ggml.lib().ggml_hip_get_stat(b"fused_attn_tokens"))
    t0 = time.perf_counter()
    for il in range(L):
        last = il == L - 1
        rows_in = taps["inpL0"] if il == 0 else taps["layer_out_all"][il - 1]
        want = ref_logits[None, :] if last else taps["layer_out_all"][il]
        kl, vl = k[il * per:(il + 1) * per], v[il * per:(il + 1) * per]
        # the oracle's second order on the same input: a one-layer model of layer il's weights (+ norm / lm_head for the last)
        hp1 = dict(hp)
        hp1["n_layer"] = 1
        w1 = {kk: vv for kk, vv in w.items() if not kk.startswith("layers.")}
        for kk, vv in w.items():
            if kk.startswith(f"layers.{il}."):
                w1["layers.0." + kk.split(".", 2)[2]] = vv
        o = oracle.Llama(hp1, w1, ctx)
        o.memory_k[:], o.memory_v[:], o.n_past = kl, vl, n_past
        lg, tt = o.evaluate(tok, mode=mode, taps=True, reverse_blocks=True, inp=rows_in)
        rev = lg[-1][None, :] if last else tt["layer_out_all"][0]
        # the device: the same layer as a stage of a layer split
        names = synth.stage_tensor_names(hp, il, il + 1)
        stage = llama.Llama(hp, {kk: vv for kk, vv in w.items() if kk in names}, context_size=ctx, layer_range=(il, il + 1))
        ss = stage.start_session(n_batch=8)
        in_dev, out_dev, _ = ss.stage_buffers()
        ss.set_kv(kl, vl)
        ss.seek(n_past)
        x = np.ascontiguousarray(rows_in, np.float32)
        if il > 0:
            ggml.lib().ggml_hip_memcpy(C.c_void_p(in_dev), C.c_void_p(x.ctypes.data), x.nbytes, 0)
        lgd = ss.evaluate(tok, want_all_logits=last)
        if last:
            got = lgd[-1][None, :]
        else:
            got = np.zeros_like(x)
            ggml.lib().ggml_hip_memcpy(C.c_void_p(got.ctypes.data), C.c_void_p(out_dev), got.nbytes, 1)
        ss.free()
        stage.free()
        s_ = float(logit_std) if last else float((want - rows_in).std())  # the size of what the layer adds to the residual
        d, dr = np.abs(got - want), np.abs(rev - want)
        mx, rms = float(d.max()) / s_, float(np.sqrt(np.mean(d ** 2))) / s_
        bmx, brms = float(dr.max()) / s_, float(np.sqrt(np.mean(dr ** 2))) / s_
        rows.append({"layer": il, "max": float(f"{mx:.3e}"), "rms": float(f"{rms:.3e}"), "band_max": float(f"{bmx:.3e}"),
                     "band_rms": float(f"{brms:.3e}")})
        worst, band_mx, band_rms = max(worst, mx), max(band_mx, bmx), max(band_rms, brms)
        n_strict += mx <= LAYER_STRICT
    edge = LAYER_EDGE if edge is None else edge
    bound = max(2.0 * band_mx, 10.0 * LAYER_STRICT, edge)
    bound_rms = max(2.0 * band_rms, 10.0 * LAYER_STRICT, edge / 4)
    ok = all(r["max"] <= min(bound, LAYER_CAP) * (1 + 1e-3) and r["rms"] <= bound_rms * (1 + 1e-3) for r in rows)
    return {"layers": rows, "worst_max": float(f"{worst:.3e}"), "band_max": float(f"{band_mx:.3e}"), "band_rms": float(f"{band_rms:.3e}"),
            "bound_max": float(f"{min(bound, LAYER_CAP):.3e}"), "bound_rms": float(f"{bound_rms:.3e}"),
            "layers_within_strict_2e-5": int(n_strict), "passed": bool(ok), "n_past": int(n_past),
            "stage_tokens_on_the_fused_wo_launch": int(ggml.lib().ggml_hip_get_stat(b"fused_wo_tokens")) - fw0,
            "stage_tokens_on_a_fused_attention_launch": int(ggml.lib().ggml_hip_get_stat(b"fused_attn_tokens")) - fa0,
            "seconds": round(time.perf_counter() - t0, 1),
            "what": "every layer ALONE as a one-layer stage on the device, on the oracle's input row of that layer and the session's "
                    "K/V, at the timed steps' n_past; max / rms of (device - oracle) over the std of the layer's update (the last "
                    "entry: final norm + lm_head, over the std of the logits); band = the oracle with its block sums in reverse "
                    "order on the same row; fails above max(2 x worst band, 10 x 2e-5, 1e-2 = one flipped activation quant) or above 1e-1"}


def prefill_leg(L, ggml, model, hp, n, steps, warmup, wname):
    """BASELINE configs[2] on the resident model: one step = Model::evaluate of an n-token prompt batch (n_batch = n)
    at n_past = 1.  MFMA roofline of the quantized GEMM launches from per-launch HIP events of one extra step."""
    sess = model.start_session(n_batch=n)
    prompt = np.random.default_rng(42).integers(0, hp["n_vocab"], n).astype(np.int32)
    sess.feed_prompt(prompt[:1])  # rewind() must leave one token (RewindError::NotEnoughTokens otherwise)

    def step():
        sess.feed_prompt(prompt)
        assert sess.rewind(n) == 0

    w16_before = int(L.ggml_hip_get_stat(b"w16_bytes"))
    tb = time.perf_counter()
    for _ in range(max(warmup, 1)):  # the first step also builds the resident f16 weight copies (if HBM has room)
        step()
    L.ggml_hip_synchronize()
    warm_s = time.perf_counter() - tb
    w16_bytes = int(L.ggml_hip_get_stat(b"w16_bytes"))
    per_step = []
    t0 = time.perf_counter()
    for _ in range(steps):
        ts = time.perf_counter()
        step()
        L.ggml_hip_synchronize()
        per_step.append(time.perf_counter() - ts)
    elapsed = time.perf_counter() - t0
    c0 = mmq_counts(L)
    L.ggml_hip_timing_begin()
    step()
    L.ggml_hip_timing_end()
    label, counts = mmq_label(c0, mmq_counts(L))
    cls = {}
    for name, k in (("mmq_mfma", ggml.KCLASS_MMQ_MFMA), ("mmvq", ggml.KCLASS_MMVQ), ("attn", ggml.KCLASS_ATTN),
                    ("other", ggml.KCLASS_OTHER)):
        cls[name] = ggml.timing_query(k)
    ms, launches, flops = cls["mmq_mfma"]
    achieved = flops / 1e12 / (ms / 1e3) if ms > 0 else 0.0
    sess.free()
    return {"tokens": n, "steps": steps, "tokens_per_s": round(n * steps / elapsed, 1),
            "dtype": "f16 x f16 MFMA, f32 accumulate: weights f16(d*q) from the resident copy (or dequantized in LDS), activations "
                     "re-quantized to Q8 as ggml does and then f16(d*q) (north_star: MFMA-f16 tiles for batched prefill); attention "
                     "f16 K/V x f16-rounded Q / probabilities, f32 accumulate",
            "ms_per_step": round(elapsed / steps * 1e3, 3),
            "ms_per_step_min_median_max": [round(x * 1e3, 3) for x in (min(per_step), float(np.median(per_step)), max(per_step))],
            "weights_f16_copy_bytes": w16_bytes,
            "weights_f16_copy_note": (f"resident f16 copy of the quantized 2-D weights, {w16_bytes / 1e9:.2f} GB of HBM next to the "
                                      f"{wname.upper()} blocks, built by k_dequant_w16 inside the first (untimed) prompt batch: "
                                      f"{'built by this leg, ' if w16_before == 0 else 'already resident, '}"
                                      f"{warm_s * 1e3:.0f} ms for the {max(warmup, 1)} warm-up batches incl. that pass; "
                                      "decode keeps streaming the quantized blocks") if w16_bytes else
                                     "no f16 copy (option off or HBM short): the GEMM dequantizes the blocks in LDS",
            "roofline": {"bound": "mfma", "kernel": label + " — wq|wk|wv, wo, w1|w3, w2 per layer + lm_head",
                         "kernel_launch_counts": {k: v for k, v in counts.items() if v},
                         "achieved": round(achieved, 1), "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(achieved / MFMA_F16_PEAK_TFLOPS, 4), "launches_per_step": launches,
                         "algo_flops_per_step": flops, "avg_launch_us": round(ms * 1e3 / max(launches, 1), 2),
                         "method": "per-launch HIP events on the backend stream, one extra untimed step"},
            "logits_read_back": "the last token's row only (128 KB): feed_prompt evaluates with OutputRequest::default() "
                                "(crates/llm-base/src/inference_session.rs:315-316), so the host mirror keeps the [n_vocab, N] logits node on "
                                "the device and read_last_token fetches one row; an evaluation that asks for all logits reads all 65 MB back",
            "class_ms_per_step": {k: round(v[0], 3) for k, v in cls.items()},
            "class_launches_per_step": {k: v[1] for k, v in cls.items()}}


def roofline_leg(args, ggml, hp, sess, elapsed, fused_tokens, fused_wo_tokens):
    """--full: the decode path's HBM roofline, taken at the context length the timed steps ended on, before the other legs move
    the session on.  Per launch kind: two HIP events on the backend's own stream around `rs` replays of a hipGraph that holds
    only that launch of every layer (32 per replay): the average launch PERIOD, kernel-to-kernel boundary included.
    rocprofv3's per-kernel duration of the same launches agrees with it (profiles/), so this is the roofline figure;
    the same for every mat-vec kind and for all 129 mat-vec launches of a token replayed together."""
    rs = max(args.roofline_steps, 1)
    roofline_ctx = int(sess.n_past)  # positions in the session's K/V: what the fused launch's attention reads per replay
    kinds = {"qkv": 0, "wo": 1, "gate_up": 2, "down": 3, "lm_head": 4}
    per_kind = {}
    for name, k in kinds.items():
        kms, kn, kb = ggml.bench_plan_class(ggml.KKIND_BASE + k, rs)
        per_kind[name] = {"launches": kn, "bytes_per_launch": int(kb / max(kn, 1)),
                          "us_per_launch": round(kms * 1e3 / max(kn * rs, 1), 3),
                          "GBps": round(kb * rs / 1e9 / (kms / 1e3), 1) if kms > 0 else 0.0}
    ms, launches, algo_bytes = ggml.bench_plan_class(ggml.KCLASS_MMVQ, rs)
    # what each kind costs IN SEQUENCE: all mat-vec launches minus all but that kind.  A launch replayed alone does not show what
    # it owes its predecessor (w1|w3 finds its first 24 MB in L2, warmed by the fused launch in front of it: kernels/decode_fused.h
    # NextWarm) nor what it pays for its successor (that warm-up's 24 MB pass through the fused launch's window)
    for name, kind in kinds.items():
        if name in per_kind and per_kind[name]["launches"] > 0:
            ms_wo, _, _ = ggml.bench_plan_class(ggml.KKIND_BASE + 8 + kind, rs)
            us_seq = (ms - ms_wo) * 1e3 / rs / per_kind[name]["launches"]
            per_kind[name]["in_sequence_us_per_launch"] = round(us_seq, 3)
            per_kind[name]["in_sequence_frac"] = round(per_kind[name]["bytes_per_launch"] / 1e3 / us_seq / HBM_PEAK_GBS, 4) if us_seq > 0 else None
    att_ms, att_n, att_bytes = ggml.bench_plan_class(ggml.KCLASS_ATTN, rs)
    oth_ms, oth_n, _ = ggml.bench_plan_class(ggml.KCLASS_OTHER, rs)
    # the DOMINANT kernel = the launch kind with the most device time per token (launches x period), whatever its name
    dom_kind = max(per_kind, key=lambda k: per_kind[k]["launches"] * per_kind[k]["us_per_launch"])
    dom = per_kind[dom_kind]
    for k, v in per_kind.items():
        v["us_per_token"] = round(v["launches"] * v["us_per_launch"], 2)
        v["frac"] = round(v["GBps"] / HBM_PEAK_GBS, 4)
    achieved = dom["GBps"]
    wb, nparams = weight_bytes_per_token(hp, ggml.BLOCK_BYTES[hp["wtype"]], ggml.BLOCK_ELEMS[hp["wtype"]])
    traffic, traffic_from, traffic_all, traffic_ctx = None, None, None, None
    for tp in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json"):
        tpath = os.path.join(ROOT, "profiles", tp)
        if os.path.exists(tpath) and args.model == "7b" and args.wtype == "q4_0":
            tj = json.load(open(tpath))
            traffic_all = {k: v["hbm_bytes_per_launch"] for k, v in tj.items() if isinstance(v, dict) and "hbm_bytes_per_launch" in v}
            traffic = traffic_all.get(dom_kind)
            traffic_ctx = tj.get("context_positions")  # mean context of the profiled dispatches (tests/tools/pmc_traffic.py)
            traffic_from = ("profiles/" + tp + ": a COMMITTED figure from separate rocprofv3 --pmc passes of this kernel "
                            "(FETCH_SIZE x2 gfx950 correction + WRITE_SIZE), not measured in this run"
                            + ("" if traffic is not None else "; it holds no entry for this launch kind"))
            break
    is_k = args.wtype.endswith("_k")
    Egqa_b = hp["n_embd"] // (hp["n_head"] // hp["n_head_kv"])
    warm_mb = int(os.environ.get("GGML_HIP_WARM_MB", "24"))  # the library's default (llm_amd/csrc/backend_state.inc opt_warm_mb)
    row_b = hp["n_embd"] // 32 * ggml.BLOCK_BYTES[hp["wtype"]] if not args.wtype.endswith("_k") else 0
    warm_bytes = (min((int(warm_mb * 1e6 / (2.0 * row_b)) & ~7), hp["n_ff"]) * 2 * row_b) if (row_b and fused_wo_tokens) else 0
    W = args.wtype.upper()
    labels = {"gate_up": f"k_mmvq_big<{W}, EPI_GATE, XSRC_NORM> (w1|w3 mat-vec, rms_norm + Q8 staging and silu(w1 x)*(w3 x) epilogue fused)",
              "qkv": ((f"k_qkv_attn_wo<{W}> (wq|wk|wv mat-vec with rms_norm + Q8 staging, RoPE and K/V store on G - n_head workgroups, the "
                       "attention of the token on n_head workgroups of the same launch, and wo + residual as the mat-vec workgroups' second "
                       "phase; bytes = wq|wk|wv + wo + the K/V the attention reads)") if fused_wo_tokens else
                      (f"k_qkv_attn<{W}> (wq|wk|wv mat-vec with rms_norm + Q8 staging, RoPE and K/V store on G - n_head workgroups + the "
                       "attention of the token on n_head workgroups of the same launch; bytes = weights + the K/V the attention reads)"))
                     if fused_tokens else f"k_mmvq_big<{W}, EPI_QKV, XSRC_NORM> (wq|wk|wv mat-vec, rms_norm + Q8 staging, RoPE and K/V store fused)",
              "down": f"k_mmvq_big<{W}, EPI_ADD, XSRC_F32> (w2 mat-vec, Q8 staging of the gate and residual add fused)",
              "wo": f"k_mmvq_big<{W}, EPI_ADD, XSRC_Q8> (wo mat-vec + residual add)",
              "lm_head": f"k_mmvq_big<{W}, EPI_STORE, XSRC_NORM> (final norm + lm_head)"}
    kernel_label = (f"k_mmvq_kbig / k_qkv_attn_k<{W}> (K plan on big workgroups, launch kind '{dom_kind}': the activation is normed / "
                    "quantized to Q8_K in the launch's own staging)") if is_k else labels[dom_kind]
    kernel_label += f"; {dom['launches']} launches per token = {dom['us_per_token']} us, the largest share of the token's device time"
    roofline = {"bound": "hbm", "kernel": kernel_label, "kernel_kind": dom_kind,
                "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": traffic, "traffic_from": traffic_from,
                # the PMC passes ran at their own context length: the ratio is taken against the algorithmic bytes AT THAT context (the
                # fused launch's bytes hold the K/V the attention reads: 4 bytes x n_embd_gqa per position and launch)
                "traffic_context_positions": traffic_ctx,
                # ... and the fused launch also pulls the first warm_mb (24) MB of w1|w3 through its idle window for the NEXT launch
                # (kernels/decode_fused.h NextWarm): bytes the memory side sees in THIS launch by design, not re-reads.  (Under the
                # profiler's per-dispatch serialisation w1|w3 then fetches them again — its own figure stays at its algorithmic bytes;
                # in a hipGraph replay it finds them in L2: in_sequence_us_per_launch below.)
                "traffic_next_launch_warm_bytes": warm_bytes if dom_kind == "qkv" else 0,
                "traffic_over_algo": round(traffic / (dom["bytes_per_launch"] + (warm_bytes if dom_kind == "qkv" else 0)
                                                      + ((traffic_ctx - roofline_ctx) * Egqa_b * 4 if (traffic_ctx and dom_kind == "qkv") else 0)), 4) if traffic else None,
                "traffic_per_kind": traffic_all,
                "avg_launch_us": dom["us_per_launch"], "algo_bytes_per_launch": dom["bytes_per_launch"],
                "context_positions": roofline_ctx,
                "method": f"{rs} replays of a hipGraph with that launch of every layer between two HIP events on the "
                          "backend stream: launch period incl. the kernel boundary (= rocprofv3's per-kernel duration)",
                "per_kind": per_kind,
                "all_matvecs_per_token": {"launches": launches, "algo_bytes": int(algo_bytes), "weights_bytes": wb,
                                          "ms": round(ms / rs, 4),
                                          "GBps": round(algo_bytes * rs / 1e9 / (ms / 1e3), 1) if ms > 0 else 0.0,
                                          "frac": round(algo_bytes * rs / 1e9 / (ms / 1e3) / HBM_PEAK_GBS, 4) if ms > 0 else 0.0},
                "whole_token": {"algo_bytes": int(algo_bytes), "ms": round(elapsed / args.steps * 1e3, 4),
                                "frac": round(algo_bytes / 1e6 / (elapsed / args.steps * 1e3) / HBM_PEAK_GBS, 4)},
                "class_ms_per_token": {"mmvq": round(ms / rs, 4), "attn": round(att_ms / rs, 4),
                                       "other": round(oth_ms / rs, 4)},
                "class_launches_per_token": {"mmvq": launches, "attn": att_n, "other": oth_n}}
    return roofline


def run_single(args):
    from llm_amd import ggml
    if not ggml.has_gpu():
        raise SystemExit("bench.py: no HIP device visible; the hot path has no CPU fallback")
    L = ggml.lib()
    hp, w, model, prep = build_model(args)
    sess = model.start_session(n_batch=8)
    prompt = np.random.default_rng(42).integers(0, hp["n_vocab"], args.prompt).astype(np.int32)
    L.ggml_hip_synchronize()
    tp = time.perf_counter()
    sess.feed_prompt(prompt)  # untimed for the metric; reported as config.prompt_feed (n_batch = 8: multi-token plan)
    L.ggml_hip_synchronize()
    prompt_s = time.perf_counter() - tp
    # the same chunks again (rewind to the first chunk, feed the rest): the plan of the 8-token chunk is cached and captured
    # now, this is the steady-state rate of InferenceSession::feed_prompt at the reference's default n_batch = 8
    n_again = (args.prompt - 8) // 8 * 8
    prompt2_s = 0.0
    if args.full and n_again > 0 and sess.rewind(args.prompt - 8) == 0:
        L.ggml_hip_synchronize()
        tp2 = time.perf_counter()
        sess.feed_prompt(prompt[8:8 + n_again])
        L.ggml_hip_synchronize()
        prompt2_s = time.perf_counter() - tp2
        if 8 + n_again < args.prompt:
            sess.feed_prompt(prompt[8 + n_again:])
    for _ in range(args.warmup):
        sess.infer_next_token()
    L.ggml_hip_synchronize()
    stat = lambda k: int(L.ggml_hip_get_stat(k.encode()))
    h0 = {k: stat(k) for k in ("ns_match", "ns_launch", "ns_wait", "ns_compute", "plan_tokens")}
    fused0 = stat("fused_attn_tokens")
    fused_wo0 = stat("fused_wo_tokens")
    sess.host_timing(reset=True)
    per_step = np.zeros(args.steps)
    t0 = time.perf_counter()
    tprev = t0
    for i in range(args.steps):
        tok = sess.infer_next_token()  # returns after the token's logits are back on the host (the reference's contract)
        tnow = time.perf_counter()
        per_step[i] = tnow - tprev
        tprev = tnow
    L.ggml_hip_synchronize()
    elapsed = time.perf_counter() - t0
    tok_s = args.steps / elapsed
    if args.dump_outputs:  # before any leg below moves the session on
        dump_outputs(args.dump_outputs, {"token": np.array([tok], np.float64), "last_logits": sess.last_logits()})
    fused_tokens = stat("fused_attn_tokens") - fused0
    fused_wo_tokens = stat("fused_wo_tokens") - fused_wo0
    fused_timeouts = stat("fused_attn_timeouts")
    if fused_timeouts:
        raise SystemExit(f"bench.py: {fused_timeouts} attention workgroup(s) of k_qkv_attn gave up waiting for their rows")
    parity = parity_check(args, hp, w, sess) if args.full and not args.no_parity_check else None
    if stat("plan_tokens") == h0["plan_tokens"]:  # e.g. GGML_HIP_PLAN_K=0: the node-by-node executor ran, nothing to replay
        print(json.dumps({"metric": f"decode tokens/s LLaMA-{args.model.upper()} {args.wtype.upper()}", "value": round(tok_s, 2),
                          "unit": "tokens/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": DTYPES[args.wtype], "parity_check": parity, "data": "synthetic",
                          "config": {"workload": f"LLaMA-{args.model.upper()} {args.wtype.upper()} single-token greedy decode on the "
                                                 "node-by-node executor (no decode plan matched or the plan option is off)"},
                          "roofline": None, "cpu_baseline": None}), flush=True)
        sess.free()
        return
    is_k = args.wtype.endswith("_k")
    roofline = roofline_leg(args, ggml, hp, sess, elapsed, fused_tokens, fused_wo_tokens) if args.full else None
    ht = [x / args.steps / 1e3 for x in sess.host_timing()]  # us per token
    h1 = {k: stat(k) - v for k, v in h0.items()}
    reference_sequence, dev_s, dev8_s, long_ctx = None, None, None, None
    if args.full and not args.headline_only:
        # the same steps through the reference's OWN call sequence: InferenceSession::compute builds the graph and then calls
        # ggml_graph_compute synchronously (crates/llm-base/src/inference_session.rs:220-295) — no ggml_hip_graph_compute_begin / _end,
        # nothing built ahead: what a rustformers/llm binary gets by linking this library with no source change at all
        # Every leg below starts again at the position the timed steps started at (InferenceSession::rewind): a leg that simply went
        # on from where the one before it stopped would decode against a longer context than the headline (the device-sampling
        # leg of round 5 ran at ~700 positions, on the 2-workgroups-per-head attention) and the legs could not be held against
        # each other.
        leg_start = args.prompt + args.warmup

        def back_to_start():
            k = int(sess.n_past) - leg_start
            if k > 0:
                sess.rewind(k)

        sess.set_speculate(False)
        back_to_start()
        for _ in range(4):
            sess.infer_next_token()
        L.ggml_hip_synchronize()
        n_ref = max(16, args.steps // 2)
        sess.host_timing(reset=True)
        tr = time.perf_counter()
        for _ in range(n_ref):
            sess.infer_next_token()
        L.ggml_hip_synchronize()
        ref_s = time.perf_counter() - tr
        ht_ref = [x / n_ref / 1e3 for x in sess.host_timing()]
        # ... and with the backend's own speculation (option speculate_next / GGML_HIP_SPECULATE_NEXT=1, off by default): behind every
        # token the device samples the greedy token and runs the next token's plan at once; the caller's unchanged sequence finds its
        # results on their way whenever it did take the first maximum (it does here: greedy decode)
        ggml.set_option("speculate_next", 1)
        back_to_start()
        for _ in range(4):
            sess.infer_next_token()
        L.ggml_hip_synchronize()
        hits0 = stat("spec_hits")
        tr = time.perf_counter()
        for _ in range(n_ref):
            sess.infer_next_token()
        L.ggml_hip_synchronize()
        spec_s = time.perf_counter() - tr
        spec_hits = stat("spec_hits") - hits0
        sess.set_speculate(True)
        back_to_start()
        for _ in range(4):
            sess.infer_next_token()
        L.ggml_hip_synchronize()
        tr = time.perf_counter()
        for _ in range(n_ref):
            sess.infer_next_token()
        L.ggml_hip_synchronize()
        spec2_s = time.perf_counter() - tr
        ggml.set_option("speculate_next", 0)
        sess.infer_next_token()
        # the same unchanged sequence for a caller that SAMPLES (the reference's default chain: repetition penalty over 64 tokens,
        # top-k 40, ..., temperature 0.8: crates/llm-base/src/samplers.rs:97-188), speculation off: all n_vocab logits read back and
        # searched on the host, as the reference does, against the k best + the penalty window's logits taken on the device
        # (llm_session_topk: 104 pairs instead of 128 KB).  Both draw the same tokens (tests/test_device_tools_gpu.py).
        import ctypes
        sampler_legs = {}
        sess.set_speculate(False)  # the UNCHANGED sequence: nothing built ahead between begin and end
        for dev_topk in (0, 1):
            rng = ctypes.c_uint64(0x9E3779B97F4A7C15)
            back_to_start()
            for _ in range(4):
                sess.infer_next_token_topk(rng, 40, 0.8, bool(dev_topk))
            L.ggml_hip_synchronize()
            tr = time.perf_counter()
            for _ in range(n_ref):
                sess.infer_next_token_topk(rng, 40, 0.8, bool(dev_topk))
            L.ggml_hip_synchronize()
            dt = time.perf_counter() - tr
            sampler_legs["device_topk_40" if dev_topk else "full_logits_read_back"] = {
                "tokens_per_s": round(n_ref / dt, 2), "ms_per_token": round(dt / n_ref * 1e3, 4), "tokens": n_ref,
                "bytes_read_back_per_token": (40 + 64) * 8 if dev_topk else 4 * hp["n_vocab"]}
        sess.set_speculate(True)
        sess.infer_next_token_topk(ctypes.c_uint64(1), 40, 0.8, False)  # (refreshes the host copy of the last logits for the legs below)
        sess.infer_next_token()
        reference_sequence = {"tokens_per_s": round(n_ref / ref_s, 2), "ms_per_token": round(ref_s / n_ref * 1e3, 4), "tokens": n_ref,
                              "default_sampler_shape": dict(sampler_legs, what="the unchanged sequence sample -> Model::evaluate with the reference's default "
                                                            "sampler shape (repetition penalty over the last 64 tokens, top-k 40, temperature 0.8) instead "
                                                            "of argmax, backend speculation off: candidates from all logits on the host vs from "
                                                            "llm_session_topk on the device"),
                              "with_backend_speculation": {"tokens_per_s": round(n_ref / spec_s, 2), "ms_per_token": round(spec_s / n_ref * 1e3, 4),
                                                           "hits": int(spec_hits), "of": n_ref,
                                                           "what": "the same unchanged call sequence with GGML_HIP_SPECULATE_NEXT=1 (the device runs the "
                                                                   "greedy next token behind every token; a caller that sampled another token waits for "
                                                                   "that run and then for its own)",
                                                           "and_begin_end_sequence_tokens_per_s": round(n_ref / spec2_s, 2)},
                              "graph_build_us_per_token": round(ht_ref[0], 1),
                              "what": "build the token's graph, then ggml_graph_compute (synchronous): InferenceSession::compute as the reference "
                                      "has it (inference_session.rs:220-295), zero caller-side changes"}
        # the same greedy decode with the sampler on the device: ids identical to the loop above
        # (tests/test_llama_gpu.py), no logits read-back / host sync per token.  Reported beside the metric, not as it.
        back_to_start()
        sess.infer_next_token()
        L.ggml_hip_synchronize()
        td = time.perf_counter()
        sess.infer_tokens_device(args.steps)
        L.ggml_hip_synchronize()
        dev_s = time.perf_counter() - td
        # ... and with 8 tokens per hipGraph launch (option chain_k): what the graph-launch gap between tokens costs
        dev8_s = None
        if hasattr(ggml, "set_option"):
            ggml.set_option("chain_k", 8)
            try:
                back_to_start()
                sess.infer_next_token()
                sess.infer_tokens_device(8)  # captures the 8-token graph
                L.ggml_hip_synchronize()
                td = time.perf_counter()
                sess.infer_tokens_device(args.steps)
                L.ggml_hip_synchronize()
                dev8_s = time.perf_counter() - td
            finally:
                ggml.set_option("chain_k", 0)
        # the same decode deep into the context (n_past ~1800 of 2048): attention split over positions (decode_attn_split.h)
        long_ctx = None
        if args.model != "tiny":
            ls = model.start_session(n_batch=512)
            ls.feed_prompt(np.random.default_rng(43).integers(0, hp["n_vocab"], 1792).astype(np.int32))
            for _ in range(8):
                ls.infer_next_token()
            L.ggml_hip_synchronize()
            tl0 = time.perf_counter()
            for _ in range(32):
                ls.infer_next_token()
            L.ggml_hip_synchronize()
            long_s = time.perf_counter() - tl0
            long_ctx = {"n_past_at_start": 1800, "tokens": 32, "tokens_per_s": round(32 / long_s, 2),
                        "ms_per_token": round(long_s / 32 * 1e3, 4)}
            ls.free()  # freeing device tensors drops the cached plans: one more token rebuilds the main session's
            sess.infer_next_token()
            L.ggml_hip_synchronize()
    host_split = {"plan_tokens": h1["plan_tokens"],
                  "graph_build_and_sampling_ms": round((elapsed * 1e9 - h1["ns_compute"]) / args.steps / 1e6, 4),
                  "match_ms": round(h1["ns_match"] / args.steps / 1e6, 4),
                  "enqueue_ms": round(h1["ns_launch"] / args.steps / 1e6, 4),
                  "device_wait_ms": round(h1["ns_wait"] / args.steps / 1e6, 4),
                  "host_phases_us": {"adopt_or_build_graph": round(ht[0], 1), "token_write_and_plan": round(ht[1], 1),
                                     "compute_begin": round(ht[2], 1), "speculative_build_next": round(ht[3], 1),
                                     "compute_end_wait_and_copy": round(ht[4], 1), "argmax": round(ht[5], 1),
                                     "evaluate_total": round(ht[6], 1)}}

    prefill = None
    if args.full and args.prefill_steps > 0 and args.model != "tiny":
        sess.free()
        sess = None
        prefill = prefill_leg(L, ggml, model, hp, args.prefill_tokens, args.prefill_steps, 2, args.wtype)
    cpu = None
    if args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline(args, hp, w, args.cpu_secs)
    out = {"metric": f"decode tokens/s LLaMA-{args.model.upper()} {args.wtype.upper()}", "value": round(tok_s, 2),
           "unit": "tokens/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(elapsed / args.steps * 1e3, 4),
           "ms_per_step_min_median_max": [round(float(x) * 1e3, 4) for x in (per_step.min(), np.median(per_step), per_step.max())],
           "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": DTYPES[args.wtype], "parity_check": parity,
           "data": "synthetic", "full": bool(args.full),
           "config": {"workload": f"LLaMA-{args.model.upper()} {args.wtype.upper()} single-token greedy decode "
                                  f"(BASELINE configs[1]), {args.prompt}-token prompt, ctx 2048, f16 KV, batch 1",
                      "n_past_at_start": args.prompt + args.warmup, "parallelism": "1 GPU",
                      "call_sequence": {"value_uses": "InferenceSession::compute of the host mirror with the next token's graph built between "
                                                      "ggml_hip_graph_compute_begin and _end while the device runs (two extension entry points; "
                                                      "a caller-side change of ~10 lines, INTEGRATION.md section 2)",
                                        "reference_call_sequence": reference_sequence,
                                        "legs_start_at_n_past": args.prompt + args.warmup,
                                        "legs_note": "every leg of call_sequence and device_sampling rewinds the session to the position the timed "
                                                     "steps started at and decodes from there (4 untimed tokens first): same context as `value`"},
                      "weights_in_hbm_before_timing": True, "host_split_per_token": host_split,
                      "decode_launches": {"qkv_and_attention_in_one_launch_tokens": int(fused_tokens), "of_timed_tokens": int(args.steps),
                                          "per_layer": "K plan on big workgroups, 4 launches: k_qkv_attn_k (norm + Q8_K staged, wq|wk|wv, RoPE + K/V store, the attention "
                                                       "on n_head workgroups of the same launch) -> wo (Q8_K staged) + residual -> w1|w3 (norm + Q8_K staged, "
                                                       "silu*mul epilogue) -> w2 (Q8_K staged) + residual; beyond the split threshold wq|wk|wv -> k_attn_split_one" if is_k else
                                                       "k_qkv_attn_wo (wq|wk|wv mat-vec on G - n_head workgroups + one attention workgroup per head + wo "
                                                       "as the mat-vec workgroups' second phase, all hand-offs as epoch-tagged 8-byte granules) -> w1|w3 -> w2"
                                                       if fused_wo_tokens else
                                                       "k_qkv_attn (wq|wk|wv mat-vec on G - n_head workgroups + one attention workgroup per head "
                                                       "in the same launch, rows handed over as epoch-tagged 8-byte granules) -> wo -> w1|w3 -> w2"
                                                       if fused_tokens else "wq|wk|wv -> k_attn_decode -> wo -> w1|w3 -> w2",
                                          "wo_in_the_attention_launch_tokens": int(fused_wo_tokens),
                                          "k_plan_tokens": stat("kplan_tokens") if is_k else None,
                                          "note": "roofline.per_kind.qkv is the fused launch when it ran: its bytes include the K/V read of the "
                                                  "attention, its time the hand-off wait and the attention tail"},
                      "long_context": long_ctx,
                      "device_sampling": None if not dev_s else
                                         {"tokens_per_s": round(args.steps / dev_s, 2), "ms_per_token": round(dev_s / args.steps * 1e3, 4),
                                          "note": "same greedy tokens via llm_infer_tokens_greedy_device (argmax kernel feeds the next "
                                                  "replay; logits stay in HBM until the last token)",
                                          "eight_tokens_per_graph_launch": None if not dev8_s else
                                          {"tokens_per_s": round(args.steps / dev8_s, 2), "ms_per_token": round(dev8_s / args.steps * 1e3, 4)}},
                      "prefill": prefill,
                      "weights": ("BASELINE.md section 4: N(0, 0.02^2) rows quantized by ggml_quantize_q* (gaussians from the "
                                  "library's counter-based generator)") if args.weights == "gaussian" else "random valid GGML blocks",
                      "prompt_feed": {"tokens": int(args.prompt), "n_batch": 8, "ms": round(prompt_s * 1e3, 1),
                                      "tokens_per_s": round(args.prompt / prompt_s, 1),
                                      "note": "first call of the process: includes hipGraph capture of the plans",
                                      "steady": {"tokens": n_again, "ms": round(prompt2_s * 1e3, 2),
                                                 "tokens_per_s": round(n_again / prompt2_s, 1) if prompt2_s > 0 else None,
                                                 "note": "the same 8-token chunks fed again after a rewind (plans cached)"} if args.full else None}, "prep": {k: round(v, 2) for k, v in prep.items()}},
           "roofline": roofline, "cpu_baseline": cpu}
    print(json.dumps(out), flush=True)
    if sess is not None:
        sess.free()
    model.free()


DTYPES = {  # the arithmetic the decode path computes in: ggml's block dot of the weight type with its vec_dot_type
    "q4_0": "i8*i4->i32 block dots, f32 accumulate (W4A8 = ggml's Q4_0·Q8_0)",
    "q4_1": "i8*u4->i32 block dots + m*s term, f32 accumulate (ggml's Q4_1·Q8_1)",
    "q5_0": "i8*i5->i32 block dots, f32 accumulate (ggml's Q5_0·Q8_0)",
    "q5_1": "i8*u5->i32 block dots + m*s term, f32 accumulate (ggml's Q5_1·Q8_1)",
    "q8_0": "i8*i8->i32 block dots, f32 accumulate (ggml's Q8_0·Q8_0)",
    "q4_k": "i8*u4->i32 sub-block dots with 6-bit scales, f32 accumulate (ggml's Q4_K·Q8_K)",
    "q6_k": "i8*i6->i32 sub-block dots with 8-bit scales, f32 accumulate (ggml's Q6_K·Q8_K)",
    "q5_k": "i8*u5->i32 sub-block dots with 6-bit scales and mins, f32 accumulate (ggml's Q5_K·Q8_K)",
    "q3_k": "i8*i3->i32 sub-block dots with 6-bit scales, f32 accumulate (ggml's Q3_K·Q8_K)",
    "q2_k": "i8*u2->i32 sub-block dots with 4-bit scales and mins, f32 accumulate (ggml's Q2_K·Q8_K)",
}
MFMA_F16_PEAK_TFLOPS = 2500.0  # MI355X dense f16 MFMA peak, MI355X_MICROARCH.md "BF16/F16 ~2.5 PF dense"


def run_prefill(args):
    """BASELINE configs[2]: one step = Model::evaluate of a 512-token prompt batch (n_batch = 512) into an empty
    context; tokens/s = 512 / step time.  Roofline leg: the quantized GEMM launches (k_mmq, f16 MFMA) timed
    with HIP events on the backend stream in a separate, untimed pass."""
    from llm_amd import ggml
    if not ggml.has_gpu():
        raise SystemExit("bench.py: no HIP device visible; the hot path has no CPU fallback")
    L = ggml.lib()
    hp, w, model, prep = build_model(args)
    n = args.prefill_tokens
    sess = model.start_session(n_batch=n)
    prompt = np.random.default_rng(42).integers(0, hp["n_vocab"], n).astype(np.int32)

    sess.feed_prompt(prompt[:1])  # rewind() must leave one token (RewindError::NotEnoughTokens otherwise)

    def step():
        sess.feed_prompt(prompt)
        assert sess.rewind(n) == 0

    for _ in range(max(args.warmup, 1)):
        step()
    L.ggml_hip_synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    L.ggml_hip_synchronize()
    elapsed = time.perf_counter() - t0
    c0 = mmq_counts(L)
    L.ggml_hip_timing_begin()
    step()
    L.ggml_hip_timing_end()
    label, counts = mmq_label(c0, mmq_counts(L))
    cls = {}
    for name, k in (("mmq_mfma", ggml.KCLASS_MMQ_MFMA), ("mmvq", ggml.KCLASS_MMVQ), ("attn", ggml.KCLASS_ATTN),
                    ("other", ggml.KCLASS_OTHER)):
        ms, launches, work = ggml.timing_query(k)
        cls[name] = (ms, launches, work)
    ms, launches, flops = cls["mmq_mfma"]
    achieved = flops / 1e12 / (ms / 1e3) if ms > 0 else 0.0
    roofline = {"bound": "mfma", "kernel": label + " — wq|wk|wv, wo, w1|w3, w2 per layer + lm_head",
                "kernel_launch_counts": {k: v for k, v in counts.items() if v},
                "achieved": round(achieved, 1), "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(achieved / MFMA_F16_PEAK_TFLOPS, 4), "traffic": None,
                "avg_launch_us": round(ms * 1e3 / max(launches, 1), 2), "launches_per_step": launches,
                "algo_flops_per_step": flops,
                "method": "per-launch HIP events on the backend stream, one extra untimed step",
                "class_ms_per_step": {k: round(v[0], 3) for k, v in cls.items()},
                "class_launches_per_step": {k: v[1] for k, v in cls.items()}}
    out = {"metric": f"prefill tokens/s LLaMA-{args.model.upper()} {args.wtype.upper()}",
           "value": round(n * args.steps / elapsed, 1), "unit": "tokens/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None,
           "dtype": "f16 x f16 MFMA, f32 accumulate (weights f16(d*q) from the resident copy or dequantized in LDS; activations "
                    "Q8-requantized as ggml does, then f16(d*q))",
           "data": "synthetic",
           "config": {"workload": f"LLaMA-{args.model.upper()} {args.wtype.upper()} {n}-token prefill batch "
                                  f"(BASELINE configs[2]) at n_past=1, ctx 2048, f16 KV", "parallelism": "1 GPU",
                      "weights_in_hbm_before_timing": True, "prep": {k: round(v, 2) for k, v in prep.items()}},
           "roofline": roofline, "cpu_baseline": None}
    print(json.dumps(out), flush=True)
    sess.free()
    model.free()


def run_feed(args):
    """feed_prompt of --prompt tokens in chunks of --n-batch (inference_session.rs:315-316), --steps times over (rewind in
    between): the steady rate of the multi-token plan, and a workload rocprofv3 can be pointed at."""
    from llm_amd import ggml
    L = ggml.lib()
    hp, w, model, prep = build_model(args)
    nb = args.n_batch
    sess = model.start_session(n_batch=nb)
    prompt = np.random.default_rng(42).integers(0, hp["n_vocab"], args.prompt).astype(np.int32)
    sess.feed_prompt(prompt)
    n_again = (args.prompt - nb) // nb * nb
    times = []
    for _ in range(max(1, args.steps)):
        assert sess.rewind(n_again) == 0
        L.ggml_hip_synchronize()
        t0 = time.perf_counter()
        sess.feed_prompt(prompt[args.prompt - n_again:])
        L.ggml_hip_synchronize()
        times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    print(json.dumps({"metric": f"prompt feed tokens/s LLaMA-{args.model.upper()} {args.wtype.upper()} n_batch={nb}",
                      "value": round(n_again / t, 1), "unit": "tokens/s", "n_gpus": 1, "steps": len(times),
                      "ms_per_chunk": round(t * 1e3 / (n_again // nb), 4), "tokens_per_pass": n_again, "n_batch": nb,
                      "n_past_range": [args.prompt - n_again, args.prompt], "data": "synthetic"}), flush=True)
    sess.free()
    model.free()


def run_split(args):
    """ONE InferenceSession layer-split over --split device slots of this process (the ggml-style split:
    contiguous layer ranges, the f32 residual crosses with ggml_hip_copy_between_devices = a peer copy over xGMI between two
    GPUs), single-stream greedy decode, against the unsplit session in the same process: the flat curve a layer split of
    batch-1 decode gives, and what a hop costs.  With fewer visible GPUs than slots the slots are virtual (several on one
    GPU, the hop a device copy) and the figure isolates the host + hand-off overhead of the split itself."""
    from llm_amd import ggml, llama
    L = ggml.lib()
    G = max(1, args.split)
    n_dev = L.ggml_hip_device_count()
    virtual = n_dev < G
    res = {}
    for name, split in (("unsplit", 0), ("split", G)):
        if split:
            if virtual:
                os.environ["GGML_HIP_VIRTUAL_DEVICES"] = str(G)
            os.environ["GGML_HIP_LAYER_SPLIT"] = str(G)
        hp, w, model, prep = build_model(args)
        stages = model.stages()
        sess = model.start_session(n_batch=8)
        prompt = np.random.default_rng(42).integers(0, hp["n_vocab"], args.prompt).astype(np.int32)
        sess.feed_prompt(prompt)
        ids = [sess.infer_next_token() for _ in range(args.warmup)]
        for sl in range(G if split else 1):
            L.ggml_hip_bind_thread_device(sl)
            L.ggml_hip_synchronize()
        L.ggml_hip_bind_thread_device(0)
        t0 = time.perf_counter()
        ids += [sess.infer_next_token() for _ in range(args.steps)]
        elapsed = time.perf_counter() - t0
        res[name] = {"tokens_per_s": round(args.steps / elapsed, 2), "ms_per_token": round(elapsed / args.steps * 1e3, 4),
                     "stages": stages, "ids": ids}
        sess.free()
        model.free()
        os.environ.pop("GGML_HIP_LAYER_SPLIT", None)
    os.environ.pop("GGML_HIP_VIRTUAL_DEVICES", None)
    same = res["unsplit"]["ids"] == res["split"]["ids"]
    hop_us = (res["split"]["ms_per_token"] - res["unsplit"]["ms_per_token"]) * 1e3 / max(G - 1, 1)
    out = {"metric": f"decode tokens/s LLaMA-{args.model.upper()} {args.wtype.upper()}, ONE session layer-split over {G} device slots of one process",
           "value": res["split"]["tokens_per_s"], "unit": "tokens/s", "n_gpus": min(n_dev, G), "device_slots": G,
           "virtual_slots": virtual, "steps": args.steps, "warmup": args.warmup, "ms_per_step": res["split"]["ms_per_token"],
           "higher_is_better": True, "scaling": "strong", "data": "synthetic",
           "unsplit": {k: v for k, v in res["unsplit"].items() if k != "ids"},
           "split": {k: v for k, v in res["split"].items() if k != "ids"},
           "same_greedy_ids": same, "overhead_per_hop_us": round(hop_us, 1),
           "config": {"workload": f"LLaMA-{args.model.upper()} {args.wtype.upper()} single-stream greedy decode, {args.prompt}-token prompt, ctx 2048"}}
    print(json.dumps(out), flush=True)
    if not same:
        raise SystemExit("bench.py --mode split: the split session produced different tokens")


def run_sessions_unchanged(args, counts):
    """The same measurement for a caller that CHANGES NOTHING: every thread calls model.start_session() and infer — no slot argument,
    no bind call (crates/llm-base/src/inference_session.rs:43-48) — and the one opt-in is the environment variable
    GGML_HIP_SESSION_SLOTS=n, under which the backend assigns a thread its own sibling slot of the GPU when it creates its first
    K/V memory (include/ggml_hip.h ggml_hip_thread_session_slot)."""
    import threading
    os.environ["GGML_HIP_SESSION_SLOTS"] = str(max(counts))
    from llm_amd import ggml
    L = ggml.lib()
    hp, w, model, prep = build_model(args)
    prompt = np.random.default_rng(42).integers(0, hp["n_vocab"], args.prompt).astype(np.int32)
    runs = []
    for n in counts:
        ready, start = threading.Barrier(n + 1), threading.Barrier(n + 1)
        lat, ids, slots = [None] * n, [None] * n, [None] * n

        def run(i):
            s = model.start_session(n_batch=8)
            slots[i] = int(L.ggml_hip_thread_session_slot())
            s.feed_prompt(prompt)
            for _ in range(args.warmup):
                s.infer_next_token()
            L.ggml_hip_synchronize()
            ready.wait()
            start.wait()
            t0 = time.perf_counter()
            ids[i] = [s.infer_next_token() for _ in range(args.steps)]
            lat[i] = (time.perf_counter() - t0) / args.steps
            s.free()

        th = [threading.Thread(target=run, args=(i,)) for i in range(n)]
        for t in th:
            t.start()
        ready.wait()
        start.wait()
        t0 = time.perf_counter()
        for t in th:
            t.join()
        el = time.perf_counter() - t0
        timeouts = int(L.ggml_hip_get_stat(b"fused_attn_timeouts"))
        runs.append({"sessions": n, "aggregate_tokens_per_s": round(n * args.steps / el, 1),
                     "per_session_ms_per_token": [round(x * 1e3, 4) for x in lat], "slot_of_each_thread": slots,
                     "all_sessions_same_ids": all(x == ids[0] for x in ids), "fused_attn_timeouts": timeouts})
        if not runs[-1]["all_sessions_same_ids"]:
            print(json.dumps(runs[-1]), flush=True)
            raise SystemExit("bench.py --mode sessions: a session diverged")
    one = runs[0]["aggregate_tokens_per_s"] if runs[0]["sessions"] == 1 else None
    for r in runs:
        r["vs_one_session"] = round(r["aggregate_tokens_per_s"] / one, 3) if one else None
    best = runs[-1]
    print(json.dumps({"metric": f"aggregate decode tokens/s LLaMA-{args.model.upper()} {args.wtype.upper()}, {best['sessions']} concurrent sessions of one model on one GPU",
                      "value": best["aggregate_tokens_per_s"], "unit": "tokens/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": round(1e3 / best["aggregate_tokens_per_s"], 4), "higher_is_better": True, "scaling": "weak",
                      "data": "synthetic", "runs": runs,
                      "config": {"workload": f"LLaMA-{args.model.upper()} {args.wtype.upper()} greedy decode, {args.prompt}-token prompt per session, ctx 2048, "
                                             "one thread per session, each thread only calls start_session() / infer (no extension call); "
                                             f"GGML_HIP_SESSION_SLOTS={max(counts)} in the environment; one resident copy of the weights"}}), flush=True)
    model.free()


def run_sessions(args):
    """Several InferenceSessions of ONE model decoding concurrently on one GPU, one thread each (the reference's contract:
    crates/llm-base/src/inference_session.rs:43-48, model/mod.rs:275-276).  Every session lives on its own device slot of the
    model's GPU (llm_start_session_on: own stream, arena shadows, K/V, plan cache) and streams the model's one copy of the
    weights; value = aggregate tokens/s of the largest session count, next to one session alone in the same process."""
    import threading
    counts = sorted({max(1, int(c)) for c in args.sessions.split(",")})
    if args.sessions_unchanged_caller:
        return run_sessions_unchanged(args, counts)
    os.environ["GGML_HIP_VIRTUAL_DEVICES"] = str(max(counts))
    from llm_amd import ggml
    L = ggml.lib()
    hp, w, model, prep = build_model(args)
    prompt = np.random.default_rng(42).integers(0, hp["n_vocab"], args.prompt).astype(np.int32)
    runs = []
    for n in counts:
        sess = [model.start_session_on(i, n_batch=8) for i in range(n)]
        for s in sess:
            s.feed_prompt(prompt)
            for _ in range(args.warmup):
                s.infer_next_token()
        for i in range(n):
            L.ggml_hip_bind_thread_device(i)
            L.ggml_hip_synchronize()
        L.ggml_hip_bind_thread_device(0)
        start = threading.Barrier(n + 1)
        lat, ids = [None] * n, [None] * n

        def run(i):
            start.wait()
            t0 = time.perf_counter()
            ids[i] = [sess[i].infer_next_token() for _ in range(args.steps)]
            lat[i] = (time.perf_counter() - t0) / args.steps

        th = [threading.Thread(target=run, args=(i,)) for i in range(n)]
        for t in th:
            t.start()
        start.wait()
        t0 = time.perf_counter()
        for t in th:
            t.join()
        el = time.perf_counter() - t0
        timeouts = int(L.ggml_hip_get_stat(b"fused_attn_timeouts"))
        runs.append({"sessions": n, "aggregate_tokens_per_s": round(n * args.steps / el, 1),
                     "per_session_ms_per_token": [round(x * 1e3, 4) for x in lat],
                     "all_sessions_same_ids": all(x == ids[0] for x in ids), "fused_attn_timeouts": timeouts})
        for s in sess:
            s.free()
        if timeouts or not runs[-1]["all_sessions_same_ids"]:
            print(json.dumps(runs[-1]), flush=True)
            raise SystemExit("bench.py --mode sessions: a session diverged or a hand-off gave up")
    one = runs[0]["aggregate_tokens_per_s"] if runs[0]["sessions"] == 1 else None
    for r in runs:
        r["vs_one_session"] = round(r["aggregate_tokens_per_s"] / one, 3) if one else None
    best = runs[-1]
    print(json.dumps({"metric": f"aggregate decode tokens/s LLaMA-{args.model.upper()} {args.wtype.upper()}, {best['sessions']} concurrent sessions of one model on one GPU",
                      "value": best["aggregate_tokens_per_s"], "unit": "tokens/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": round(1e3 / best["aggregate_tokens_per_s"], 4), "higher_is_better": True, "scaling": "weak",
                      "data": "synthetic", "runs": runs,
                      "config": {"workload": f"LLaMA-{args.model.upper()} {args.wtype.upper()} greedy decode, {args.prompt}-token prompt per session, ctx 2048, "
                                             "one thread and one device slot per session, one resident copy of the weights"}}), flush=True)
    model.free()


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 or world > 1:
        from llm_amd import pipeline
        pipeline.run_bench(args)
        return
    if args.mode == "prefill":
        run_prefill(args)
        return
    if args.mode == "feed":
        run_feed(args)
        return
    if args.mode == "split":
        run_split(args)
        return
    if args.mode == "sessions":
        run_sessions(args)
        return
    run_single(args)


if __name__ == "__main__":
    main()
