// debug_mpt.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip): the test hook of the two kernels of
// the MPT plan that have arithmetic of their own (kernels/mpt_plan.h), on caller-supplied buffers.  At file scope.
extern "C" {
// op 0 — the LayerNorm staging of k_mmvq_big<.., XSRC_LNORM>: x [K] f32, w [K] f32 (the gain), eps; out[0] lo, out[1] hi ([K/2] int8
//        each: elements 0..15 / 16..31 of every block), out[2] d [K/32] f32, out[3] sum [K/32] i32 — the planar Q8 blocks one workgroup
//        leaves in LDS.  flag: 1 = the Q8_0 kind (d after its f16 round trip), 0 = Q8_1's f32 d.  K % 32 == 0, K <= 8192.
// op 1 — k_attn_decode_alibi: x = q [H * D] f32, mem_k / mem_v [C][H * D] f16 (token-major, one layer), w = slopes [H] f32, the token
//        at position n_past (T = n_past + 1 <= C); out[0] [H * D] f32, the merged heads.  D % 32 == 0, D <= 128, H <= 256.
// op 2 — test-only state, no device work: flag != 0 makes every MPT plan BUILT from now on carry a slope table with every head on the
//        first sequence (the mutant tests/test_mpt_plan_gpu.py must see); flag 0 ends that.  Cached plans are dropped either way.
// op 3 — the matcher alone: x = a ggml_cgraph *; 1 if match_mpt_decode takes the graph under the slot's options, 0 if it declines.  Nothing of
//        the graph is executed or uploaded (a test can ask about a graph it must not run: a token behind the context's end).
// Every output comes back followed by 256 guard bytes of 0xFF.  -1 for what no call site could launch.
int ggml_hip_debug_mpt(int op, int flag, const float *x, const float *w, float eps, int64_t K, const uint16_t *mem_k, const uint16_t *mem_v,
                       int H, int D, int n_past, int64_t C, float scale, void *const *out) {
    if (op == 2) {
        DebugRun run;
        g_mpt_slope_mutant = flag != 0;
        drop_all_plans();
        return 0;
    }
    if (op == 3) {
        if (!x) return -1;
        DebugRun run;
        LlamaMatch m;
        return match_mpt_decode((ggml_cgraph *)const_cast<float *>(x), m) ? 1 : 0;
    }
    if (op == 0) {
        if (!x || !w || !out || K < 32 || K % 32 || K > 8192) return -1;
        for (int i = 0; i < 4; i++)
            if (!out[i]) return -1;
        DebugRun run;
        const int64_t nb = K / 32;
        BigArgs ba;
        memset(&ba, 0, sizeof(ba));
        ba.xf = (const float *)run.buf((size_t)K * 4, x);
        ba.xw = (const float *)run.buf((size_t)K * 4, w);
        ba.eps = eps;
        ba.nb = (int)nb;
        ba.T = 1024;
        ba.G = 1;
        char *lo = run.buf((size_t)K / 2), *hi = run.buf((size_t)K / 2), *d = run.buf((size_t)nb * 4), *sum = run.buf((size_t)nb * 4);
        launch_mpt_stage_dump(g.stream, flag != 0, &ba, lo, hi, (float *)d, (int *)sum, (size_t)((nb + 63) / 64 * 64) * 40);
        run.back(out[0], lo, (size_t)K / 2 + DEBUG_GUARD);
        run.back(out[1], hi, (size_t)K / 2 + DEBUG_GUARD);
        run.back(out[2], d, (size_t)nb * 4 + DEBUG_GUARD);
        run.back(out[3], sum, (size_t)nb * 4 + DEBUG_GUARD);
        return run.finish();
    }
    if (op != 1) return -1;
    if (!x || !w || !mem_k || !mem_v || !out || !out[0] || H < 1 || H > 256 || D < 32 || D % 32 || D > 128 || n_past < 0 || (int64_t)n_past + 1 > C)
        return -1;
    const int64_t E = (int64_t)H * D, Clds = (C + 7) & ~(int64_t)7;
    if (attn_decode_lds(Clds, D) > ATTN_DECODE_LDS_MAX) return -1;
    DebugRun run;
    DecParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.n_past = n_past;
    DecParams *prm = run.put(hp);
    const float *dq = (const float *)run.buf((size_t)E * 4, x), *dsl = (const float *)run.buf((size_t)H * 4, w);
    const char *dk = run.buf((size_t)C * E * 2, mem_k), *dv = run.buf((size_t)C * E * 2, mem_v);
    char *dout = run.buf((size_t)E * 4);
    if (launch_mpt_attn(g.stream, H, dq, dk, dv, prm, scale, dsl, D, E, (float *)dout, Clds, attn_decode_lds(Clds, D))) return -1;
    run.back(out[0], dout, (size_t)E * 4 + DEBUG_GUARD);
    return run.finish();
}
}
