// debug_mpt_batch.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip): the test hook of the batched MPT
// step's device code (kernels/mpt_batch.h), each piece alone on caller-supplied arrays, launched as plan_mpt_batch.inc launches it.  At file scope.
extern "C" {
// op 0 — the batched ALiBi decode attention (three launches): x = q [B][H D] f32, slopes [H], pos [B], mem_k / mem_v = B pointers to
//        [C][H D] f16 token-major caches (read only; rows behind pos[c] are never read), scale, W workgroups per head (1 .. 16);
//        out[0] the merged heads [B][H D] f32.  D = 32 / 64 / 128 and a share's p values fit in LDS.
// op 1 — one EPI_QKV_TM_BATCH pass: w [K, 3 K] with a device copy, x [B][K]; mem_k / mem_v = B pointers to [C][K] f16 caches, in-out:
//        column c's K and V rows land in row pos[c] of cache c; out[0] the Q rows [B][K] f32.
// Every output and (op 1) every cache comes back followed by 256 guard bytes of 0xFF; outputs are 0xFF before the launch.  -1 for what
// no call site could launch.
int ggml_hip_debug_mpt_batch(int op, int W, const struct ggml_tensor *w, const float *x, const float *slopes, int B, const int32_t *pos, int64_t C,
                             uint16_t *const *mem_k, uint16_t *const *mem_v, int64_t K, int H, int D, float scale, void *const *out) {
    if ((op != 0 && op != 1) || !x || !pos || !mem_k || !mem_v || !out || !out[0] || B < 1 || B > BATCH_COLS_MAX || C < 1) return -1;
    for (int c = 0; c < B; c++)
        if (!mem_k[c] || !mem_v[c] || pos[c] < 0 || pos[c] >= C) return -1;
    if (op == 0) {
        if (!slopes || H < 1 || H > 256 || !(D == 32 || D == 64 || D == 128) || W < 1 || W > 16 || mpt_batch_attn_lds(C, B, W) > 150 * 1024) return -1;
        K = (int64_t)H * D;
    } else if (!w || qt_of(w->type) < 0 || !wants_soa(w) || K < 32 || K % 32 || w->ne[0] != K || w->ne[1] != 3 * K) {
        return -1;
    }
    const int64_t nb = K / 32;
    DebugRun run;  // (the shapes below ask the device for its CUs)
    if (op == 1 && !cols_shape((int)(3 * K / 16), 1, (int)nb).kc) return -1;
    const size_t nkv = (size_t)C * K * 2, no = (size_t)B * K * 4, nq = (size_t)B * K / 2, nd = (size_t)B * nb * 4, nt = (size_t)nb * 32;
    BatchCols hb;
    memset(&hb, 0, sizeof(hb));
    for (int c = 0; c < B; c++) {
        hb.pos[c] = pos[c];
        hb.mem_k[c] = (__half *)run.buf(nkv, mem_k[c]);
        hb.mem_v[c] = (__half *)run.buf(nkv, mem_v[c]);
    }
    const BatchCols *db = run.put(hb);
    const float *dx = (const float *)run.buf(no, x);
    char *dout = run.buf(no), *lo = run.buf(nq), *hi = run.buf(nq), *d = run.buf(nd), *s = run.buf(nd), *dT = run.raw(nt), *sT = run.raw(nt);
    HIP_CHECK(hipMemsetAsync(dT, 0, nt, g.stream));  // (as a plan's pool is made)
    HIP_CHECK(hipMemsetAsync(sT, 0, nt, g.stream));
    if (op == 0) {
        const float *dsl = (const float *)run.buf((size_t)H * 4, slopes);
        char *sc = run.buf((size_t)B * H * C * 4), *pmax = run.buf((size_t)H * B * W * 4), *part = run.buf((size_t)H * B * W * D * 4);
        mpt_batch_attention(dx, K, db, 0, dsl, scale, B, D, H, W, K, C, (float *)sc, (float *)pmax, (float *)part, (float *)dout, (int8_t *)lo, (int8_t *)hi,
                            (float *)d, (int *)s, (float *)dT, (int *)sT, true);
        run.back(out[0], dout, no + DEBUG_GUARD);
        return run.finish();
    }
    const int qt = qt_of(w->type);
    debug_hot_line();
    launch_quant_row(qt_f16d(qt), dx, nb, B, (int8_t *)lo, (int8_t *)hi, (float *)d, (int *)s, (float *)dT, (int *)sT);
    HIP_CHECK(hipGetLastError());
    DecMmvqArgs a;
    memset(&a, 0, sizeof(a));
    a.w[0] = qweight_of(w);
    a.x = QAct{(const i32x4 *)lo, (const i32x4 *)hi, (const float *)d, (const int *)s};
    a.nb = nb; a.dst = (float *)dout; a.Egqa = K; a.C = C; a.D = D;
    mpt_cols_block(qt, EPI_QKV_TM_BATCH, a, B, K, 0, (int)(3 * K), (const float *)dT, (const int *)sT, 1, db, 0);
    run.back(out[0], dout, no + DEBUG_GUARD);
    for (int c = 0; c < B; c++) {
        run.back(mem_k[c], hb.mem_k[c], nkv + DEBUG_GUARD);
        run.back(mem_v[c], hb.mem_v[c], nkv + DEBUG_GUARD);
    }
    return run.finish();
}
}
