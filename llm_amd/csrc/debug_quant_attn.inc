// debug_quant_attn.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip, inside its anonymous
// namespace where noted): the test hooks of the activation quantizers and of the prompt attention (both forms, and its exponential).  At file scope.
extern "C" {
// Test hook: the attention of a prompt batch on host arrays through either path of the prompt plan (plan_prompt.inc
// prompt_attention): q [N][E] f32 with RoPE applied, mem_k [C][Egqa] / mem_v [Egqa][C] f16 of one layer, out [N][E] f32.
// Returns 0, or -1 when `fused` is asked for a shape the fused kernel does not take.
int ggml_hip_debug_prompt_attention(const float *q, const uint16_t *mem_k, const uint16_t *mem_v, float *out, int N, int E, int Egqa,
                                    int H, int n_past, int64_t C, float scale, int fused) {
    DebugRun run;
    const int64_t D = E / H, Hkv = Egqa / D, T = (int64_t)n_past + N, Tp = (T + 7) & ~(int64_t)7;
    if (T > C || (fused && !prompt_attn_fits(D, T))) return -1;
    const size_t nq = (size_t)N * E * 4, nkv = (size_t)C * Egqa * 2, nsc = (size_t)H * N * T * 4, np = (size_t)H * N * Tp * 2;
    char *dq = run.raw(nq, q), *dk = run.raw(nkv, mem_k), *dv = run.raw(nkv, mem_v);
    char *dout = run.raw(nq), *dsc = run.raw(nsc), *dp = run.raw(np);  // (the scores and probabilities: the unfused path's workspace)
    HIP_CHECK(hipMemsetAsync(dout, 0xFF, nq, g.stream));
    prompt_attention(fused != 0, (const float *)dq, (const __half *)dk, (const __half *)dv, (float *)dout, (float *)dsc, (_Float16 *)dp, N, E,
                     Egqa, H, Hkv, D, n_past, C, scale);
    run.back(out, dout, nq);
    return run.finish();
}

// Test hook: ONE launch of an activation quantizer kernel on host arrays, through the launcher its call sites use (backend_ops.inc
// launch_*: the same grid, block and dynamic LDS).  rows x K f32 in, the kernel's outputs back; every output buffer is followed by
// DEBUG_GUARD bytes, outputs and guards are 0xFF before the launch and come back whole.  The branch of the Q8 quantizer is the
// option act_quant's, as everywhere.  kind (include/ggml_hip.h GGML_HIP_AQ_*), its inputs and its outputs outs[i]:
//   planar Q8 — lo, hi [rows][K/2] i8; d [rows][nb] f32; sum [rows][nb] i32; dT, sT [ceil(rows/8)][nb][8] (flags & 2); y [rows][K] f32
//     0 k_quantize_act   a [rows][stride]                                     outs: lo hi d sum
//     1 k_quant_row      a [rows][K]                                          outs: lo hi d sum (dT sT)
//     2 k_rmsnorm_quant  a [rows][K], w [K], eps                              outs: lo hi d sum (dT sT) (y: outs[6] nullable)
//     3 k_rmsnorm_quant_warm on its call site's grid, warming off (cw.n = 0): as 2, rows <= 8
//   int8 — 4 k_quant_act_i8  a [rows][stride], zp (8, 16, 0; read only with flags & 1)   outs: q8 [rows][K], d [rows][nb], xs [rows][nb]
//   f16 operand in the GEMM's k order — x16 [rows][K] f16
//     5 k_quant_act_f16  a [rows][stride]                                     outs: x16
//     6 k_p_quant4       a [rows][K]                                          outs: x16
//     7 k_p_silu_mul_quant  a, b [rows][K] (part != 0: second partials `part` floats on, both arrays part + rows * K floats)   outs: x16
//     8 k_p_norm_quant   a [rows][K], b = x2 (nullable, only with r), r (nullable: the ADD form), w [K], eps
//                                                                             outs: x16, xsum [rows][K] f32 (with r), y (outs[2] nullable)
//     9 k_quant_act_f16_k  a [rows][stride]                                   outs: x16
//    10 k_f32_to_w16     a [rows][K]                                          outs: w16 [rows][K] f16
//   Q8_K — q8 [rows][K] i8; d8 [rows][nsb] f32; bs [rows][nsb][16] i16
//    11 k_quant_q8k      a [rows][stride]                                     outs: q8 d8 bs
//    12 k_k_norm_quant   a [rows][K], w [K], eps                              outs: q8 d8 bs (y: outs[3] nullable)
//    13 k_k_quant        a [rows][K]                                          outs: q8 d8 bs
//    14 k_k_silu_mul_quant  a, b [rows][K]                                    outs: q8 d8 bs
// flags: 1 = the Q8_0 kind (d after its f16 round trip; else Q8_1's f32 d), 2 = with the [block][8] tables, 4 = the K8 form of kinds
// 6 .. 8 (the Q8_K round trip).  -1 for what no call site could launch: K not a multiple of the block (32; 256 for Q8_K and K8), a
// stride below K, a row of k_rmsnorm_quant that does not fit the dynamic LDS, more than 8192 elements for k_p_norm_quant (the plan
// aborts there), more rows than a chunk has (MULTI_MAX_N) for the plans' kernels, a missing array.
int ggml_hip_debug_act_quant(int kind, int flags, int64_t rows, int64_t K, int64_t stride, const float *a, const float *b, const float *r,
                             const float *w, float eps, int64_t part, int zp, void *const *outs) {
    DebugRun run;
    const bool f16d = (flags & 1) != 0, tabs = (flags & 2) != 0, k8 = (flags & 4) != 0;
    const bool strided = kind == GGML_HIP_AQ_QUANTIZE_ACT || kind == GGML_HIP_AQ_QUANT_ACT_I8 || kind == GGML_HIP_AQ_QUANT_ACT_F16 ||
                         kind == GGML_HIP_AQ_QUANT_ACT_F16_K || kind == GGML_HIP_AQ_QUANT_Q8K;
    const bool planar = kind >= GGML_HIP_AQ_QUANTIZE_ACT && kind <= GGML_HIP_AQ_RMSNORM_QUANT_WARM;
    const bool q8k = kind >= GGML_HIP_AQ_QUANT_Q8K && kind <= GGML_HIP_AQ_K_SILU_MUL_QUANT;
    const bool p_kind = kind >= GGML_HIP_AQ_P_QUANT4 && kind <= GGML_HIP_AQ_P_NORM_QUANT;
    const bool norm = kind == GGML_HIP_AQ_RMSNORM_QUANT || kind == GGML_HIP_AQ_RMSNORM_QUANT_WARM || kind == GGML_HIP_AQ_P_NORM_QUANT ||
                      kind == GGML_HIP_AQ_K_NORM_QUANT;
    const bool two = kind == GGML_HIP_AQ_P_SILU_MUL_QUANT || kind == GGML_HIP_AQ_K_SILU_MUL_QUANT;
    const bool plan = kind == GGML_HIP_AQ_QUANT_ROW || kind == GGML_HIP_AQ_RMSNORM_QUANT || kind == GGML_HIP_AQ_RMSNORM_QUANT_WARM ||
                      (kind >= GGML_HIP_AQ_K_NORM_QUANT && kind <= GGML_HIP_AQ_K_SILU_MUL_QUANT);
    if (kind < 0 || kind > GGML_HIP_AQ_K_SILU_MUL_QUANT || !a || !outs || rows < 1 || rows > 65535 || K < 32) return -1;
    const bool blk256 = q8k || kind == GGML_HIP_AQ_QUANT_ACT_F16_K || (p_kind && k8);
    if (K % (blk256 ? 256 : 32)) return -1;
    if (!strided) stride = K;
    if (stride < K) return -1;
    if ((norm && !w) || (two && !b) || (tabs && !(kind >= GGML_HIP_AQ_QUANT_ROW && kind <= GGML_HIP_AQ_RMSNORM_QUANT_WARM))) return -1;
    if (k8 && !p_kind) return -1;
    if (plan && rows > MULTI_MAX_N) return -1;
    if (kind == GGML_HIP_AQ_RMSNORM_QUANT_WARM && (rows > 8 || rows + 8 > g.num_cus)) return -1;  // cols_warm_of's condition
    if ((kind == GGML_HIP_AQ_RMSNORM_QUANT || kind == GGML_HIP_AQ_RMSNORM_QUANT_WARM) && (size_t)K * 4 + 1024 > 64 * 1024) return -1;
    if (kind == GGML_HIP_AQ_P_NORM_QUANT && (K > 8192 || (b && !r))) return -1;
    if (kind != GGML_HIP_AQ_P_NORM_QUANT && r) return -1;
    if (part && (kind != GGML_HIP_AQ_P_SILU_MUL_QUANT || part < rows * K || part % 4)) return -1;
    if (kind == GGML_HIP_AQ_QUANT_ACT_I8 && f16d && zp != 0 && zp != 8 && zp != 16) return -1;
    const int64_t nb = K / 32, nsb = K / 256, ntab = (rows + 7) / 8;
    // the outputs of this kind: host pointer, bytes
    struct Out { void *host; size_t n; char *dev; };
    std::vector<Out> o;
    auto want = [&](int i, size_t n, bool optional = false) {
        o.push_back(Out{outs[i], (optional && !outs[i]) ? 0 : n, nullptr});
        return optional || outs[i] != nullptr;
    };
    bool ok = true;
    const size_t nel = (size_t)rows * K;
    if (planar) {
        ok = want(0, nel / 2) && want(1, nel / 2) && want(2, (size_t)rows * nb * 4) && want(3, (size_t)rows * nb * 4);
        if (ok && kind != GGML_HIP_AQ_QUANTIZE_ACT) {
            if (tabs) ok = want(4, (size_t)ntab * nb * 32) && want(5, (size_t)ntab * nb * 32);
            else { o.push_back(Out{nullptr, 0, nullptr}); o.push_back(Out{nullptr, 0, nullptr}); }
            if (kind != GGML_HIP_AQ_QUANT_ROW) want(6, nel * 4, true);
        }
    } else if (kind == GGML_HIP_AQ_QUANT_ACT_I8) {
        ok = want(0, nel) && want(1, (size_t)rows * nb * 4) && want(2, (size_t)rows * nb * 4);
    } else if (q8k) {
        ok = want(0, nel) && want(1, (size_t)rows * nsb * 4) && want(2, (size_t)rows * nsb * 32);
        if (kind == GGML_HIP_AQ_K_NORM_QUANT) want(3, nel * 4, true);
    } else {
        ok = want(0, nel * 2);
        if (kind == GGML_HIP_AQ_P_NORM_QUANT) {
            if (r) ok = ok && want(1, nel * 4);
            else o.push_back(Out{nullptr, 0, nullptr});
            want(2, nel * 4, true);
        }
    }
    if (!ok) return -1;
    for (Out &e : o)
        if (e.n) e.dev = run.buf(e.n);
    auto dev = [&](size_t i) { return i < o.size() ? o[i].dev : nullptr; };
    const size_t n_in = part ? (size_t)part + nel : (size_t)(rows - 1) * stride + K;
    const char *da = run.buf(n_in * 4, a);
    const char *db = b ? run.buf((two ? n_in : nel) * 4, b) : nullptr;
    const char *dr = r ? run.buf(nel * 4, r) : nullptr;
    const char *dw = norm ? run.buf((size_t)K * 4, w) : nullptr;
    ColsWarm cw;
    memset(&cw, 0, sizeof(cw));
    switch (kind) {
        case GGML_HIP_AQ_QUANTIZE_ACT:
            launch_quantize_act(f16d, da, stride * 4, nb, rows, (int8_t *)dev(0), (int8_t *)dev(1), (float *)dev(2), (int *)dev(3));
            break;
        case GGML_HIP_AQ_QUANT_ROW:
            launch_quant_row(f16d, (const float *)da, nb, rows, (int8_t *)dev(0), (int8_t *)dev(1), (float *)dev(2), (int *)dev(3), (float *)dev(4),
                             (int *)dev(5));
            break;
        case GGML_HIP_AQ_RMSNORM_QUANT:
        case GGML_HIP_AQ_RMSNORM_QUANT_WARM:
            launch_rmsnorm_quant(f16d, (const float *)da, (const float *)dw, eps, K, rows, (float *)dev(6), (int8_t *)dev(0), (int8_t *)dev(1),
                                 (float *)dev(2), (int *)dev(3), (float *)dev(4), (int *)dev(5),
                                 kind == GGML_HIP_AQ_RMSNORM_QUANT_WARM ? &cw : nullptr);
            break;
        case GGML_HIP_AQ_QUANT_ACT_I8:
            launch_quant_act_i8(f16d, da, stride * 4, nb, rows, (float)zp, (int8_t *)dev(0), (float *)dev(1), (float *)dev(2));
            break;
        case GGML_HIP_AQ_QUANT_ACT_F16: launch_quant_act_f16(f16d, da, stride * 4, nb, rows, (_Float16 *)dev(0)); break;
        case GGML_HIP_AQ_P_QUANT4: launch_p_quant4(k8, f16d, (const f32x4 *)da, (int64_t)nel / 4, (_Float16 *)dev(0)); break;
        case GGML_HIP_AQ_P_SILU_MUL_QUANT:
            launch_p_silu_mul_quant(k8, f16d, (const f32x4 *)da, (const f32x4 *)db, (int64_t)nel / 4, part / 4, (_Float16 *)dev(0));
            break;
        case GGML_HIP_AQ_P_NORM_QUANT:
            launch_p_norm_quant(k8, f16d, (const float *)da, (const float *)db, (const float *)dr, (float *)dev(1), (const float *)dw, eps, K, rows,
                                (float *)dev(2), (_Float16 *)dev(0));
            break;
        case GGML_HIP_AQ_QUANT_ACT_F16_K: launch_quant_act_f16_k(da, stride * 4, nsb, rows, (_Float16 *)dev(0)); break;
        case GGML_HIP_AQ_F32_TO_W16: launch_f32_to_w16((const float *)da, (int64_t)nel, (_Float16 *)dev(0)); break;
        case GGML_HIP_AQ_QUANT_Q8K: launch_quant_q8k(da, stride * 4, nsb, rows, (int8_t *)dev(0), (float *)dev(1), (int16_t *)dev(2)); break;
        case GGML_HIP_AQ_K_NORM_QUANT:
            launch_k_norm_quant((const float *)da, (const float *)dw, eps, K, rows, (float *)dev(3), (int8_t *)dev(0), (float *)dev(1),
                                (int16_t *)dev(2));
            break;
        case GGML_HIP_AQ_K_QUANT: launch_k_quant((const float *)da, nsb, rows, (int8_t *)dev(0), (float *)dev(1), (int16_t *)dev(2)); break;
        default:
            launch_k_silu_mul_quant((const float *)da, (const float *)db, nsb, rows, (int8_t *)dev(0), (float *)dev(1), (int16_t *)dev(2));
    }
    for (const Out &e : o)
        if (e.n) run.back(e.host, e.dev, e.n + DEBUG_GUARD);
    return run.finish();
}

// Test hook: the fused prompt attention in the form plan_launch_prompt launches it (plan_prompt.inc: prompt_attention(true, ...)
// with x16_out, rope and q_part set): q_raw [N][E] f32 the un-rotated wq product, q_raw2 (nullable) its second K-split partial —
// uploaded N * E floats behind the first, q_part = N * E as the plan's qkv_stride is a distance inside one buffer; rope [N][128]
// f32, (cos, sin) per pair in k_rope_table's layout; mem_k [C][Egqa] / mem_v [Egqa][C] f16 of one layer; f16d: the block scale
// rounded to f16 first.  x16 [N][E] f16 (+ guard): wo's GEMM operand; out [N][E] f32 (+ guard, nullable): the buffer handed over
// as `out`, which this form does not write.  Both are 0xFF before the launch and come back whole, guard included.  Returns 0,
// or -1 for a shape the fused kernel does not take.
int ggml_hip_debug_prompt_attention_plan(const float *q_raw, const float *q_raw2, const float *rope, const uint16_t *mem_k,
                                         const uint16_t *mem_v, uint16_t *x16, float *out, int N, int E, int Egqa, int H, int n_past,
                                         int64_t C, float scale, int f16d) {
    DebugRun run;
    if (!q_raw || !rope || !mem_k || !mem_v || !x16 || N < 1 || H < 1 || E % H || n_past < 0) return -1;
    const int64_t D = E / H, T = (int64_t)n_past + N;
    if (Egqa < D || Egqa % D || H % (Egqa / D) || T > C || C % 8 || !prompt_attn_fits(D, T)) return -1;
    const int64_t Hkv = Egqa / D;
    const size_t nq = (size_t)N * E * 4, nkv = (size_t)C * Egqa * 2, nx = (size_t)N * E * 2;
    char *dq = run.buf(nq * (q_raw2 ? 2 : 1));
    h2d_bulk(dq, q_raw, nq);
    if (q_raw2) h2d_bulk(dq + nq, q_raw2, nq);
    char *dr = run.buf((size_t)N * 128 * 4, rope);
    char *dk = run.buf(nkv, mem_k), *dv = run.buf(nkv, mem_v);
    char *dx = run.buf(nx), *dout = run.buf(nq);
    prompt_attention(true, (const float *)dq, (const __half *)dk, (const __half *)dv, (float *)dout, nullptr, nullptr, N, E, Egqa, H, Hkv,
                     D, n_past, C, scale, (_Float16 *)dx, f16d != 0, (const float *)dr, q_raw2 ? (int64_t)N * E : 0);
    run.back(x16, dx, nx + DEBUG_GUARD);
    if (out) run.back(out, dout, nq + DEBUG_GUARD);
    return run.finish();
}

// Test hook: f16(exp_le0(x)) (kernels/prompt_attn.h: the fused prompt attention's exponential) and f16(expf(x)) (what k_p_soft_max
// and ggml's table hold) for ALL 65536 f16 bit patterns x; out_fast / out_ref: 65536 f16 bit patterns each.
__global__ void __launch_bounds__(256) k_debug_exp_le0(uint16_t *out_fast, uint16_t *out_ref) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    const float x = __half2float(__ushort_as_half((unsigned short)i));
    out_fast[i] = __half_as_ushort(__float2half_rn(exp_le0(x)));
    out_ref[i] = __half_as_ushort(__float2half_rn(expf(x)));
}
int ggml_hip_debug_exp_le0(uint16_t *out_fast, uint16_t *out_ref) {
    DebugRun run;
    uint16_t *d = (uint16_t *)run.raw(2 * 65536 * 2);
    hipLaunchKernelGGL(k_debug_exp_le0, dim3(256), dim3(256), 0, g.stream, d, d + 65536);
    run.back(out_fast, d, 65536 * 2);
    run.back(out_ref, d + 65536, 65536 * 2);
    return run.finish();
}

}  // extern "C"
