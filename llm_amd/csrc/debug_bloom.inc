// debug_bloom.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip): the test hook of the BLOOM plan's own
// kernels (kernels/bloom_plan.h), each as plan_launch_bloom launches it, on caller-supplied buffers.  At file scope.
extern "C" {
// op 0 — the biased LayerNorm staging of k_mmvq_big<.., XSRC_LNORM_B>: x [K] f32, gain [K], nbias [K] (the LayerNorm's bias), eps; out[0] lo,
//        out[1] hi ([K/2] int8 each: elements 0..15 / 16..31 of every block), out[2] d [K/32] f32, out[3] sum [K/32] i32 — the planar Q8
//        blocks one workgroup leaves in LDS.  flag: 1 = the Q8_0 kind (d after its f16 round trip), 0 = Q8_1's f32 d.  K % 32 == 0, K <= 8192.
// op 1 — one mat-vec launch: w a block-format matrix [K, M] with a device copy, flag = the epilogue:
//        EPI_QKV_TM_B (8)  behind the biased LayerNorm of x (gain, nbias, eps); M = 3 K; bias [M]; out[0] q [K] f32, and the K and V rows as
//                          f16 at position n_past of mem_k / mem_v [C][K] (in-out, guards and all)
//        EPI_GELU_B   (9)  behind the biased LayerNorm; bias [M]; out[0] [M] f32
//        EPI_ADD_B    (10) x [K] a plain f32 row; bias [M], res [M]; out[0] [M] f32
//        EPI_STORE    (0)  behind the biased LayerNorm, no matrix bias (the lm_head); out[0] [M] f32, out[1] (nullable) [K] the normed row
// op 2 — k_get_rows_lnorm: row `token` of w [K, V], LayerNorm with gain and nbias; out[0] [K] f32.  K <= 8192.
// Every output comes back followed by 256 guard bytes of 0xFF.  -1, before a device is touched, for what no call site could launch.
int ggml_hip_debug_bloom(int op, int flag, const struct ggml_tensor *w, const float *x, const float *gain, const float *nbias, float eps, int64_t K,
                         const float *bias, const float *res, int token, int n_past, int64_t C, uint16_t *mem_k, uint16_t *mem_v, void *const *out) {
    const bool plain = op == 1 && flag == EPI_ADD_B;  // no LayerNorm in front: a row of up to 24 elements a thread
    if (op < 0 || op > 2 || (!plain && (!gain || !nbias)) || !out || !out[0] || K < 32 || K % 32 || K > (plain ? 24 * BIG_T : 8192)) return -1;
    const int64_t nb = K / 32;
    if (op == 0) {
        if (!x) return -1;
        for (int i = 1; i < 4; i++)
            if (!out[i]) return -1;
        DebugRun run;
        BigArgs ba;
        memset(&ba, 0, sizeof(ba));
        ba.xf = (const float *)run.buf((size_t)K * 4, x);
        ba.xw = (const float *)run.buf((size_t)K * 4, gain);
        ba.xb = (const float *)run.buf((size_t)K * 4, nbias);
        ba.eps = eps; ba.nb = (int)nb; ba.T = 1024; ba.G = 1;
        char *lo = run.buf((size_t)K / 2), *hi = run.buf((size_t)K / 2), *d = run.buf((size_t)nb * 4), *sum = run.buf((size_t)nb * 4);
        launch_bloom_stage_dump(g.stream, flag != 0, &ba, lo, hi, (float *)d, (int *)sum, (size_t)((nb + 63) / 64 * 64) * 40);
        run.back(out[0], lo, (size_t)K / 2 + DEBUG_GUARD);
        run.back(out[1], hi, (size_t)K / 2 + DEBUG_GUARD);
        run.back(out[2], d, (size_t)nb * 4 + DEBUG_GUARD);
        run.back(out[3], sum, (size_t)nb * 4 + DEBUG_GUARD);
        return run.finish();
    }
    if (!w || qt_of(w->type) < 0 || w->ne[0] != K || w->ne[2] != 1 || w->ne[3] != 1 || !wants_soa(w)) return -1;
    const int qt = qt_of(w->type);
    const int64_t M = w->ne[1];
    if (op == 2) {
        if (token < 0 || token >= M) return -1;
        DebugRun run;
        const QWeight qw = qweight_of(w);
        const int *dtok = (const int *)run.buf(4, &token);
        char *dout = run.buf((size_t)K * 4);
        if (launch_bloom_embed(g.stream, qt, &qw, dtok, (const float *)run.buf((size_t)K * 4, gain), (const float *)run.buf((size_t)K * 4, nbias), eps, (float *)dout))
            return -1;
        run.back(out[0], dout, (size_t)K * 4 + DEBUG_GUARD);
        return run.finish();
    }
    const int epi = flag, xsrc = epi == EPI_ADD_B ? XSRC_F32 : XSRC_LNORM_B;
    if (!x || (epi != EPI_QKV_TM_B && epi != EPI_GELU_B && epi != EPI_ADD_B && epi != EPI_STORE) || (epi != EPI_STORE && !bias) || (epi == EPI_ADD_B && !res)) return -1;
    if (epi == EPI_QKV_TM_B && (M != 3 * K || !mem_k || !mem_v || n_past < 0 || n_past >= C)) return -1;
    DebugRun run;  // (the shape below asks the device for its CUs)
    if (!big_shape(xsrc, epi, nb, M).ok) return -1;
    debug_hot_line();
    DecMmvqArgs a;
    memset(&a, 0, sizeof(a));
    a.w[0] = qweight_of(w); a.nb = nb; a.eps = eps;
    a.xf = (const float *)run.buf((size_t)K * 4, x);
    const float *dnb = nullptr;
    if (xsrc == XSRC_LNORM_B) {
        a.xw = (const float *)run.buf((size_t)K * 4, gain);
        dnb = (const float *)run.buf((size_t)K * 4, nbias);
    }
    const float *dbias = bias ? (const float *)run.buf((size_t)M * 4, bias) : nullptr;
    if (epi == EPI_ADD_B) a.res = (const float *)run.buf((size_t)M * 4, res);
    const size_t n_out = (size_t)(epi == EPI_QKV_TM_B ? K : M) * 4, nkv = (size_t)C * K * 2;
    char *dout = run.buf(n_out), *dk = nullptr, *dv = nullptr;
    a.dst = (float *)dout;
    if (epi == EPI_QKV_TM_B) {
        DecParams hp;
        memset(&hp, 0, sizeof(hp));
        hp.n_past = n_past;
        dk = run.buf(nkv, mem_k);
        dv = run.buf(nkv, mem_v);
        a.prm = run.put(hp); a.mem_k = (__half *)dk; a.mem_v = (__half *)dv; a.Egqa = K; a.C = C;
    }
    char *dy = epi == EPI_STORE && out[1] ? run.buf((size_t)K * 4) : nullptr;
    launch_big_bloom(qt, epi, xsrc, big_pack(a, (float *)dy, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, g.hot_line), dnb, dbias);
    run.back(out[0], dout, n_out + DEBUG_GUARD);
    if (dy) run.back(out[1], dy, (size_t)K * 4 + DEBUG_GUARD);
    if (dk) {
        run.back(mem_k, dk, nkv + DEBUG_GUARD);
        run.back(mem_v, dv, nkv + DEBUG_GUARD);
    }
    return run.finish();
}
}
