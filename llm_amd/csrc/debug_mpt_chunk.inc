// debug_mpt_chunk.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip): the test hook of the MPT chunk
// plan's device code (kernels/mpt_chunk.h), each piece alone on caller-supplied arrays, launched as plan_mpt_chunk.inc launches it.  At file scope.
namespace {
int debug_mpt_chunk_attn(int S, const float *q, const float *slopes, int N, int n_past, int64_t C, const uint16_t *mem_k, const uint16_t *mem_v, int H, int D,
                         float scale, void *const *out) {
    if (!q || !slopes || !mem_k || !mem_v || !out || !out[0] || N < 1 || N > MULTI_MAX_N || H < 1 || H > 256 || !(D == 32 || D == 64 || D == 128) || S < 1 ||
        S > 16 || n_past < 0 || (int64_t)n_past + N > C || mpt_chunk_attn_lds(attn_split_chunk_max(C, S)) > 150 * 1024)
        return -1;
    const int64_t E = (int64_t)H * D, nb = E / 32;
    DebugRun run;
    DecParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.n_past = n_past;
    const float *dq = (const float *)run.buf((size_t)N * E * 4, q), *dsl = (const float *)run.buf((size_t)H * 4, slopes);
    const char *dk = run.buf((size_t)C * E * 2, mem_k), *dv = run.buf((size_t)C * E * 2, mem_v);
    const size_t no = (size_t)N * E * 4, passes = ((size_t)N + 7) / 8;
    char *dout = run.buf(no), *sc = run.buf((size_t)H * 32 * C * 4), *pmax = run.buf((size_t)H * S * 32 * 4), *part = run.buf((size_t)H * S * 32 * D * 4);
    char *lo = run.buf((size_t)N * E / 2), *hi = run.buf((size_t)N * E / 2), *d = run.buf((size_t)N * nb * 4), *s = run.buf((size_t)N * nb * 4);
    char *dT = run.buf(passes * nb * 32), *sT = run.buf(passes * nb * 32);
    mpt_chunk_attention(dq, E, dk, dv, run.put(hp), dsl, scale, N, D, H, S, E, C, (float *)sc, (float *)pmax, (float *)part, (float *)dout, (int8_t *)lo, (int8_t *)hi,
                        (float *)d, (int *)s, (float *)dT, (int *)sT, true);
    run.back(out[0], dout, no + DEBUG_GUARD);
    return run.finish();
}
}  // namespace
extern "C" {
// op 0 — k_lnorm_quant_cols: x [N][K] f32, gain [K], eps; flag: 1 = the Q8_0 kind (d after its f16 round trip), 0 = Q8_1's f32 d.
//        out[0] lo, out[1] hi ([N][K/32][16] int8 each), out[2] d, out[3] sum ([N][K/32]), out[4] dT, out[5] sT (ceil(N/8) tables of
//        [K/32][8]), out[6] (nullable) the normed rows [N][K] f32.  K % 32 == 0, K <= 8192, N <= MULTI_MAX_N.
// op 1 — one residual mat-vec of a chunk (mpt_cols_block: k_quant_row, then EPI_ADD in passes of 8 columns and `flag` K slices, 0 = as
//        many as mpt_chunk_slices says): w [K, M] with a device copy, x [N][K], res [N][M]; out[0] [N][M] f32.
// op 2 — one EPI_QKV_TM pass: w [K, 3 K] with a device copy, x [N][K] the pass's N <= 8 rows, columns col0 .. col0 + N - 1 of a chunk at
//        n_past; mem_k / mem_v [C][K] f16 token-major, in-out; out[0] the Q rows [N][K] f32.
// op 3 — the position-split chunk attention: x = q [N][H D] f32, gain = the slopes [H], mem_k / mem_v [C][H D] f16 token-major (read only),
//        queries at n_past .. n_past + N - 1 <= C - 1, scale, flag = S workgroups per head (1 .. 16); out[0] the merged heads [N][H D] f32.
//        D = 32 / 64 / 128 and the ranges' LDS fit.
// Every output (and both caches) comes back followed by 256 guard bytes of 0xFF; outputs are 0xFF before the launch.  -1 for what no
// call site could launch.
int ggml_hip_debug_mpt_chunk(int op, int flag, const struct ggml_tensor *w, const float *x, const float *gain, float eps, const float *res, int64_t K,
                             int N, int col0, int n_past, int64_t C, uint16_t *mem_k, uint16_t *mem_v, int H, int D, float scale, void *const *out) {
    if (op == 3) return debug_mpt_chunk_attn(flag, x, gain, N, n_past, C, mem_k, mem_v, H, D, scale, out);
    if (!x || !out || !out[0] || N < 1 || N > MULTI_MAX_N || K < 32 || K % 32) return -1;
    const int64_t nb = K / 32;
    const size_t passes = ((size_t)N + 7) / 8, nq = (size_t)N * K / 2, nd = (size_t)N * nb * 4, nt = passes * nb * 32;
    if (op == 0) {
        if (!gain || K > 8192) return -1;
        for (int i = 1; i < 6; i++)
            if (!out[i]) return -1;
        DebugRun run;
        const float *dx = (const float *)run.buf((size_t)N * K * 4, x), *dw = (const float *)run.buf((size_t)K * 4, gain);
        char *lo = run.buf(nq), *hi = run.buf(nq), *d = run.buf(nd), *s = run.buf(nd), *dT = run.buf(nt), *sT = run.buf(nt);
        char *y = out[6] ? run.buf((size_t)N * K * 4) : nullptr;
        launch_mpt_lnorm_cols(g.stream, flag != 0, dx, dw, eps, K, N, (float *)y, (int8_t *)lo, (int8_t *)hi, (float *)d, (int *)s, (float *)dT, (int *)sT);
        char *const dev[6] = {lo, hi, d, s, dT, sT};
        const size_t bytes[6] = {nq, nq, nd, nd, nt, nt};
        for (int i = 0; i < 6; i++) run.back(out[i], dev[i], bytes[i] + DEBUG_GUARD);
        if (y) run.back(out[6], y, (size_t)N * K * 4 + DEBUG_GUARD);
        return run.finish();
    }
    if ((op != 1 && op != 2) || !w || qt_of(w->type) < 0 || !wants_soa(w) || w->ne[0] != K) return -1;
    const int qt = qt_of(w->type);
    const int64_t M = w->ne[1];
    if (M % 16) return -1;
    DebugRun run;  // (the shapes below ask the device for its CUs)
    if (op == 1) {
        const int slices = flag ? flag : mpt_chunk_slices((int)(M / 16), (int)nb);
        if (!res || slices < 1 || nb % (4 * slices) || !cols_shape((int)(M / 16), 1, (int)(nb / slices)).kc) return -1;
    } else if (M != 3 * K || N > 8 || col0 < 0 || !mem_k || !mem_v || n_past < 0 || (int64_t)n_past + col0 + N > C || !cols_shape((int)(M / 16), 1, (int)nb).kc) {
        return -1;
    }
    debug_hot_line();
    const float *dx = (const float *)run.buf((size_t)N * K * 4, x);
    char *lo = run.buf(nq), *hi = run.buf(nq), *d = run.buf(nd), *s = run.buf(nd), *dT = run.raw(nt), *sT = run.raw(nt);
    HIP_CHECK(hipMemsetAsync(dT, 0, nt, g.stream));  // (as a plan's pool is made: k_quant_row leaves the columns behind N alone)
    HIP_CHECK(hipMemsetAsync(sT, 0, nt, g.stream));
    launch_quant_row(qt_f16d(qt), dx, nb, N, (int8_t *)lo, (int8_t *)hi, (float *)d, (int *)s, (float *)dT, (int *)sT);
    HIP_CHECK(hipGetLastError());
    DecMmvqArgs a;
    memset(&a, 0, sizeof(a));
    a.w[0] = qweight_of(w);
    a.x = QAct{(const i32x4 *)lo, (const i32x4 *)hi, (const float *)d, (const int *)s};
    a.nb = nb;
    if (op == 1) {
        const size_t no = (size_t)N * M * 4;
        char *dout = run.buf(no);
        a.dst = (float *)dout;
        a.res = (const float *)run.buf(no, res);
        mpt_cols_block(qt, EPI_ADD, a, N, M, M, (int)M, (const float *)dT, (const int *)sT, flag ? flag : mpt_chunk_slices((int)(M / 16), (int)nb));
        run.back(out[0], dout, no + DEBUG_GUARD);
        return run.finish();
    }
    DecParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.n_past = n_past;
    const size_t nkv = (size_t)C * K * 2, no = (size_t)N * K * 4;
    char *dk = run.buf(nkv, mem_k), *dv = run.buf(nkv, mem_v), *dout = run.buf(no);
    a.dst = (float *)dout; a.prm = run.put(hp); a.mem_k = (__half *)dk; a.mem_v = (__half *)dv; a.Egqa = K; a.C = C;
    ColsArgs c;
    memset(&c, 0, sizeof(c));
    c.d = a; c.ncols = N; c.col0 = col0; c.ldd = K; c.dxT = (const float *)dT; c.sxT = (const int *)sT; c.hot = g.hot_line;
    mpt_cols_launch(qt, EPI_QKV_TM, c, (int)M);
    run.back(out[0], dout, no + DEBUG_GUARD);
    run.back(mem_k, dk, nkv + DEBUG_GUARD);
    run.back(mem_v, dv, nkv + DEBUG_GUARD);
    return run.finish();
}
}
