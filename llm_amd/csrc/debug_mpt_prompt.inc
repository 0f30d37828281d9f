// debug_mpt_prompt.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip): the test hook of the MPT prompt
// plan's kernels with arithmetic of their own (kernels/mpt_prompt.h), each alone on caller-supplied arrays.  At file scope.
extern "C" {
// what 0 — k_p_lnorm_quant: x [N][K] f32, x2 (nullable: a second partial, added first), r (nullable: the residual, added next; needs
//          out[1]), w [K] the gain, eps; out[0] the f16 operand [N][K] in the GEMM's k order, out[1] the residual out [N][K] f32.
//          flag: 1 = the Q8_0 kind (d after its f16 round trip), 0 = Q8_1's f32 d.  K % 32 == 0, K <= 8192.
// what 1 — k_p_gelu_quant: x [N][K] f32, x2 (nullable: the second partial); out[0] the f16 operand [N][K].  flag as above.  K % 32 == 0.
// what 2 — k_p_attn_alibi: x = the Wqkv product [N][3 H D] f32 (its Q columns are read), x2 (nullable: the second partial), w = slopes [H],
//          mem_k / mem_v [C][H D] f16 (token-major, one layer), queries at positions n_past .. n_past + N - 1 <= C - 1; out[0] the merged
//          heads [N][H D]: flag 0 = f32, 1 / 2 = out_proj's f16 operand with Q8_1's / Q8_0's scale.  D = 32 / 64 / 128, H <= 256, and
//          n_past + N within the attention's fit (mpt_attn_queries).
// what 3 — k_p_attn_alibi_stream: what 2's arguments and outputs on the streaming kernel, at any n_past + N <= C.
// Every output comes back followed by 256 guard bytes of 0xFF.  -1 for what no call site could launch.
int ggml_hip_debug_mpt_prompt(int what, int flag, const float *x, const float *x2, const float *r, const float *w, float eps, int64_t K, int N,
                              const uint16_t *mem_k, const uint16_t *mem_v, int H, int D, int n_past, int64_t C, float scale, void *const *out) {
    if (!x || !out || !out[0] || N < 1 || N > PROMPT_PLAN_MAX) return -1;
    if (what == 0) {
        if (!w || K < 32 || K % 32 || K > 8192 || (r && !out[1]) || (x2 && !r)) return -1;
        DebugRun run;
        const size_t nx = (size_t)N * K * 4;
        const float *dx = (const float *)run.buf(nx, x), *dx2 = x2 ? (const float *)run.buf(nx, x2) : nullptr;
        const float *dr = r ? (const float *)run.buf(nx, r) : nullptr, *dw = (const float *)run.buf((size_t)K * 4, w);
        char *dsum = r ? run.buf(nx) : nullptr, *dout = run.buf(nx / 2);
        launch_mpt_lnorm_quant(g.stream, flag != 0, dx, dx2, dr, (float *)dsum, dw, eps, K, N, (_Float16 *)dout);
        run.back(out[0], dout, nx / 2 + DEBUG_GUARD);
        if (r) run.back(out[1], dsum, nx + DEBUG_GUARD);
        return run.finish();
    }
    if (what == 1) {
        if (K < 32 || K % 32) return -1;
        DebugRun run;
        const size_t nx = (size_t)N * K * 4;
        char *da = run.buf(2 * nx, nullptr);  // the product and, nx bytes on, its second partial, as a split GEMM leaves them
        h2d_bulk(da, x, nx);
        if (x2) h2d_bulk(da + nx, x2, nx);
        char *dout = run.buf(nx / 2);
        launch_mpt_gelu_quant(g.stream, flag != 0, (const float *)da, (int64_t)N * K / 4, x2 ? (int64_t)N * K / 4 : 0, (_Float16 *)dout);
        run.back(out[0], dout, nx / 2 + DEBUG_GUARD);
        return run.finish();
    }
    if (what != 2 && what != 3) return -1;
    if (!w || !mem_k || !mem_v || H < 1 || H > 256 || !(D == 32 || D == 64 || D == 128) || n_past < 0 || (int64_t)n_past + N > C || flag < 0 || flag > 2 ||
        (what == 2 && !mpt_attn_queries(D, (int64_t)n_past + N)))
        return -1;
    const int64_t E = (int64_t)H * D;
    DebugRun run;
    const size_t nq = (size_t)N * 3 * E * 4;
    char *dq = run.buf(2 * nq, nullptr);
    h2d_bulk(dq, x, nq);
    if (x2) h2d_bulk(dq + nq, x2, nq);
    const float *dsl = (const float *)run.buf((size_t)H * 4, w);
    const char *dk = run.buf((size_t)C * E * 2, mem_k), *dv = run.buf((size_t)C * E * 2, mem_v);
    const size_t no = (size_t)N * E * (flag ? 2 : 4);
    char *dout = run.buf(no);
    mpt_prompt_attention((const float *)dq, x2 ? (int64_t)N * 3 * E : 0, dk, dv, dsl, flag ? nullptr : (float *)dout, flag ? (_Float16 *)dout : nullptr, flag == 2, N, E,
                         H, D, n_past, C, scale, what == 3);
    run.back(out[0], dout, no + DEBUG_GUARD);
    return run.finish();
}
}
