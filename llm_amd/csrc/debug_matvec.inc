// debug_matvec.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip, inside its anonymous
// namespace where noted): the test hooks of the mat-vec kernels — k_mmq_cols, k_mmvq_big, k_mmvq_kbig, k_mmvq_f16 — on host arrays.  At file scope.
extern "C" {
// Test hook: one weight matrix times N (2..8) activation rows through k_mmq_cols exactly as the multi-token plan launches it
// (k_quant_row with its [block][8] tables, then the EPI_STORE launch).  w: a quantized 2-D weight with a device copy;
// x: host [N][K] f32; out: host [N][M] f32.  Returns 0, or -1 when the plan would not take this shape on k_mmq_cols.
int ggml_hip_debug_mul_mat_cols(const struct ggml_tensor *w, const float *x, float *out, int N) {
    DebugRun run;
    const int qt = qt_of(w->type);
    if (qt < 0 || N < 2 || N > 8) return -1;
    const QWeight qw = qweight_of(w);
    const int64_t K = w->ne[0], M = w->ne[1], nb = K / 32;
    if (!cols_ok((int)M, 1, nb, {M})) return -1;
    char *dx = run.raw((size_t)N * K * 4, x);
    char *dlo = run.raw((size_t)N * K / 2), *dhi = run.raw((size_t)N * K / 2);
    char *dd = run.raw((size_t)N * nb * 4), *ds = run.raw((size_t)N * nb * 4);
    char *ddT = run.raw((size_t)nb * 32), *dsT = run.raw((size_t)nb * 32);
    char *dout = run.raw((size_t)N * M * 4);
    HIP_CHECK(hipMemsetAsync(ddT, 0, (size_t)nb * 32, g.stream));
    HIP_CHECK(hipMemsetAsync(dsT, 0, (size_t)nb * 32, g.stream));
    HIP_CHECK(hipMemsetAsync(dout, 0xFF, (size_t)N * M * 4, g.stream));
    launch_quant_row(qt_f16d(qt), (const float *)dx, nb, N, (int8_t *)dlo, (int8_t *)dhi, (float *)dd, (int *)ds, (float *)ddT, (int *)dsT);
    HIP_CHECK(hipGetLastError());
    ColsArgs c;
    memset(&c, 0, sizeof(c));
    c.d.w[0] = qw;
    c.d.x = QAct{(const i32x4 *)dlo, (const i32x4 *)dhi, (const float *)dd, (const int *)ds};
    c.d.nb = nb;
    c.d.dst = (float *)dout;
    c.ncols = N;
    c.ldd = M;
    c.ldr = M;
    c.dxT = (const float *)ddT;
    c.sxT = (const int *)dsT;
    with_qt(qt, [&](auto QT) { launch_cols<CT(QT), EPI_STORE>(c, (int)M); });
    run.back(out, dout, (size_t)N * M * 4);
    return run.finish();
}

// Test hooks of the decode mat-vecs: ONE launch of k_mmvq_big (Q4_0 .. Q8_0) or k_mmvq_kbig (K-quants) on host arrays, with the
// source / epilogue pairs and the arguments the single-token plans launch them with (plan_launch_all, plan_launch_k).  Every
// output buffer (and the K / V caches, uploaded from the host first) is followed by DEBUG_GUARD bytes; outputs and guards are
// 0xFF (NaN) before the launch and come back whole, guard included, so a test sees an element never written and a store past
// the end.  -1 for a shape or a pair the plans would not launch.

// k_mmvq_big: w0 (w1, w2) quantized weights with device copies, all of one type and width K.  Pairs (plan_launch_all):
//   XSRC_NORM + EPI_QKV (wq, wk, wv), XSRC_Q8 + EPI_ADD (wo), XSRC_NORM + EPI_GATE (w1, w3), XSRC_F32 + EPI_ADD (w2),
//   XSRC_NORM + EPI_STORE (lm_head).
// x [K]: the f32 row (XSRC_Q8: quantized by k_quant_row first, as wo's input is a Q8 row); norm_w [K], eps: XSRC_NORM; res [M]:
// EPI_ADD.  out: [M] (+ guard), QKV: Q [M0] after RoPE.  y_out [K] (+ guard), XSRC_NORM only: the normed row the launch staged
// (EPI_STORE's tap; for the other epilogues the tap of an EPI_STORE launch of w0 on the same row, run after it — the same
// staging code).  QKV: n_past, head size D, RoPE parameters, cache length C; mem_k [C][M1] / mem_v [M2][C] f16 in-out.
int ggml_hip_debug_mat_vec_big(const struct ggml_tensor *w0, const struct ggml_tensor *w1, const struct ggml_tensor *w2, int xsrc,
                               int epi, const float *x, const float *norm_w, float eps, const float *res, float *out, float *y_out,
                               int n_past, int D, float freq_base, float freq_scale, int64_t C, uint16_t *mem_k, uint16_t *mem_v) {
    DebugRun run;
    const bool pair_ok = (xsrc == XSRC_NORM && epi == EPI_QKV) || (xsrc == XSRC_Q8 && epi == EPI_ADD) ||
                         (xsrc == XSRC_NORM && epi == EPI_GATE) || (xsrc == XSRC_F32 && epi == EPI_ADD) ||
                         (xsrc == XSRC_NORM && epi == EPI_STORE);
    const int nw = epi == EPI_QKV ? 3 : epi == EPI_GATE ? 2 : 1;
    const ggml_tensor *ts[3] = {w0, w1, w2};
    if (!pair_ok || !x) return -1;
    for (int i = 0; i < nw; i++)
        if (!ts[i] || qt_of(ts[i]->type) < 0 || ts[i]->type != w0->type || ts[i]->ne[0] != w0->ne[0] || !wants_soa(ts[i])) return -1;
    const int qt = qt_of(w0->type);
    const int64_t K = w0->ne[0], nb = K / 32, M0 = w0->ne[1], M1 = nw > 1 ? w1->ne[1] : 0, M2 = nw > 2 ? w2->ne[1] : 0;
    if ((xsrc == XSRC_NORM && !norm_w) || (epi == EPI_ADD && !res)) return -1;
    if (epi == EPI_GATE && M1 != M0) return -1;
    if (epi == EPI_QKV && !debug_qkv_ok(mem_k, mem_v, D, M0, M1, M2, n_past, 1, C)) return -1;
    // staging limits (BigX): the norm 8192 elements over 1024 threads, launch_big's wave counts up to BIG_W, LDS; and the dealing
    // launch_big would abort on
    if (xsrc == XSRC_NORM && nb * 8 > (int64_t)BigX<XSRC_NORM>::MAXIT * BigX<XSRC_NORM>::NT) return -1;
    const BigShape bsh = big_shape(xsrc, epi, nb, (M0 + M1 + M2) / (epi == EPI_QKV ? 2 : 1));
    if (big_min_waves(xsrc, epi, nb) > BIG_W || bsh.lds > 64 * 1024 || !bsh.ok) return -1;

    debug_hot_line();
    DecMmvqArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < nw; i++) a.w[i] = qweight_of(ts[i]);
    a.nb = nb;
    char *dx = run.buf((size_t)K * 4, x);
    a.xf = (const float *)dx;
    if (xsrc == XSRC_NORM) {
        a.xw = (const float *)run.buf((size_t)K * 4, norm_w);
        a.eps = eps;
    }
    if (xsrc == XSRC_Q8) {  // the planar Q8 row, as k_quant_row makes it
        char *dlo = run.buf((size_t)K / 2), *dhi = run.buf((size_t)K / 2);
        char *dd = run.buf((size_t)nb * 4), *ds = run.buf((size_t)nb * 4);
        launch_quant_row(qt_f16d(qt), (const float *)dx, nb, 1, (int8_t *)dlo, (int8_t *)dhi, (float *)dd, (int *)ds, nullptr, nullptr);
        HIP_CHECK(hipGetLastError());
        a.x = QAct{(const i32x4 *)dlo, (const i32x4 *)dhi, (const float *)dd, (const int *)ds};
    }
    if (epi == EPI_ADD) a.res = (const float *)run.buf((size_t)M0 * 4, res);
    const size_t n_out = (size_t)M0 * 4;  // (QKV: Q)
    char *dout = run.buf(n_out);
    a.dst = (float *)dout;
    char *dy = (xsrc == XSRC_NORM && y_out) ? run.buf((size_t)K * 4) : nullptr;
    DebugQkv kv;
    if (epi == EPI_QKV) {
        kv = debug_qkv(run, n_past, 1, D, freq_base, freq_scale, C, M1, mem_k, mem_v);
        a.prm = kv.prm;
        a.mem_k = (__half *)kv.dk;
        a.mem_v = (__half *)kv.dv;
        a.Egqa = M1;
        a.C = C;
        a.D = D;
        a.theta_scale = kv.theta_scale;
        a.freq_scale = freq_scale;
    }
    // the launcher plan_launch_all uses (no timeline, no probe, no granules; the dealing is launch_big's)
    const BigArgs ba = big_pack(a, epi == EPI_STORE ? (float *)dy : nullptr, nullptr, 0, kv.rope, 0, nullptr, nullptr, 0, g.hot_line);
    with_qt(qt, [&](auto QT) {
        switch (epi) {
            case EPI_QKV: launch_big<CT(QT), EPI_QKV, XSRC_NORM>(ba); break;
            case EPI_GATE: launch_big<CT(QT), EPI_GATE, XSRC_NORM>(ba); break;
            case EPI_STORE: launch_big<CT(QT), EPI_STORE, XSRC_NORM>(ba); break;
            default:
                if (xsrc == XSRC_Q8)
                    launch_big<CT(QT), EPI_ADD, XSRC_Q8>(ba);
                else
                    launch_big<CT(QT), EPI_ADD, XSRC_F32>(ba);
        }
    });
    HIP_CHECK(hipGetLastError());
    if (dy && epi != EPI_STORE) {  // the normed row of the same staging code: the tap of an EPI_STORE launch of w0
        DecMmvqArgs t = a;
        t.w[1] = t.w[2] = QWeight{};
        t.dst = (float *)run.buf((size_t)M0 * 4);
        with_qt(qt, [&](auto QT) { launch_big<CT(QT), EPI_STORE, XSRC_NORM>(big_pack(t, (float *)dy, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, g.hot_line)); });
    }
    return debug_matvec_finish(run, out, dout, n_out, y_out, dy, (size_t)K * 4, kv);
}

namespace {
// what the K-quant and the F16 hook vet alike: 1 .. 3 matrices by epilogue, several of them only behind the norm, a residual only for one
// matrix's rows.  Returns the number of matrices, 0 for a combination neither launches.
int debug_kx_matrices(const ggml_tensor *w0, const ggml_tensor *w1, const ggml_tensor *w2, int xsrc, int epi, const float *x, const float *xw,
                      const float *res) {
    const int nw = epi == KE_QKV ? 3 : epi == KE_GATE ? 2 : !w1 ? 1 : !w2 ? 2 : 3;
    if (!x || !w0 || (xsrc != KX_F32 && !xw)) return 0;
    if (xsrc != KX_NORM && nw > 1) return 0;
    if (res && (epi != KE_ROW || nw > 1)) return 0;
    return nw;
}
}  // namespace

// k_mmvq_kbig: w0 (w1, w2) K-quant weights with device copies, of width K.  Pairs (plan_launch_k), xsrc KX_* / epi KE_*:
//   KX_NORM + KE_QKV (wq, wk, wv: one launch per run of equal types, as the plan splits a mixed file), KX_NORM + KE_ROW (1-3
//   matrices, runs of equal types: wq|wk|wv without the RoPE epilogue, a mixed w1|w3, lm_head), KX_NORM + KE_GATE (w1, w3 of one
//   type), KX_F32 + KE_ROW with res (wo; w2 behind the gate launch), KX_SILU_MUL + KE_ROW with res (w2 behind a mixed w1|w3).
// x [K]: the f32 row (KX_SILU_MUL: w1 x); xw [K]: the norm weight (KX_NORM) or w3 x (KX_SILU_MUL); res [M0] nullable.
// out: KE_ROW the matrices' rows one after the other [M0 + M1 + M2], KE_GATE [M0], KE_QKV Q [M0]; (+ guard).  y_out, KX_NORM only:
// the normed row (KE_ROW's tap; for the other epilogues the tap of a KE_ROW launch of w0, run after it).  QKV as for
// ggml_hip_debug_mat_vec_big.
int ggml_hip_debug_mat_vec_kbig(const struct ggml_tensor *w0, const struct ggml_tensor *w1, const struct ggml_tensor *w2, int xsrc,
                                int epi, const float *x, const float *xw, float eps, const float *res, float *out, float *y_out,
                                int n_past, int D, float freq_base, float freq_scale, int64_t C, uint16_t *mem_k, uint16_t *mem_v) {
    DebugRun run;
    const bool pair_ok = (xsrc == KX_NORM && (epi == KE_QKV || epi == KE_ROW || epi == KE_GATE)) ||
                         ((xsrc == KX_F32 || xsrc == KX_SILU_MUL) && epi == KE_ROW);
    const ggml_tensor *ts[3] = {w0, w1, w2};
    const int nw = pair_ok ? debug_kx_matrices(w0, w1, w2, xsrc, epi, x, xw, res) : 0;
    if (!nw) return -1;
    const int64_t K = w0->ne[0], nsb = K / 256;
    int64_t Ms[3] = {0, 0, 0};
    for (int i = 0; i < nw; i++) {
        const ggml_tensor *t = ts[i];
        if (!t || kt_of(t->type) < 0 || t->ne[0] != K || !wants_ksoa(t)) return -1;
        Ms[i] = t->ne[1];
        // kbig_ok's limits: the staging (KBIG_SBW super-blocks per wave, the norm's two 4096-element passes) and 21 rows per wave
        if (!kbig_weight_ok(kt_of(t->type), nsb, Ms[i], xsrc == KX_NORM ? K : 0)) return -1;
    }
    if (epi == KE_GATE && (w1->type != w0->type || Ms[1] != Ms[0])) return -1;
    if (epi == KE_QKV && !debug_qkv_ok(mem_k, mem_v, D, Ms[0], Ms[1], Ms[2], n_past, 1, C)) return -1;

    debug_hot_line();
    KWeight kw[3];
    for (int i = 0; i < nw; i++) kw[i] = kweight_of(ts[i]);
    char *dx = run.buf((size_t)K * 4, x);
    char *dxw = xw ? run.buf((size_t)K * 4, xw) : nullptr;
    char *dres = res ? run.buf((size_t)Ms[0] * 4, res) : nullptr;
    const int64_t Mrow = epi == KE_ROW ? Ms[0] + Ms[1] + Ms[2] : Ms[0];
    const size_t n_out = (size_t)Mrow * 4;
    char *dout = run.buf(n_out);
    char *dy = (xsrc == KX_NORM && y_out) ? run.buf((size_t)K * 4) : nullptr;
    const RowSrc src{xsrc, (const float *)dx, (const float *)dxw, eps, epi == KE_ROW ? (float *)dy : nullptr};
    DebugQkv kv;
    if (epi == KE_QKV) {  // as plan_launch_k: one launch per run of equal types, seg_kind = the matrices' kinds
        kv = debug_qkv(run, n_past, 1, D, freq_base, freq_scale, C, Ms[1], mem_k, mem_v);
        const KWeight *ws3[3] = {&kw[0], &kw[1], &kw[2]};
        float *ds3[3] = {(float *)dout, nullptr, nullptr};
        for_each_type_run(ws3, 3, [&](int i, int j) {
            KBigArgs qa;
            memset(&qa, 0, sizeof(qa));
            for (int k = i; k < j; k++) qa.seg_kind[k - i] = k;
            qa.rope = kv.rope; qa.prm = kv.prm; qa.mem_k = (__half *)kv.dk; qa.mem_v = (__half *)kv.dv; qa.Egqa = Ms[1]; qa.C = C; qa.D = D;
            launch_kbig(j - i, ws3 + i, ds3 + i, src, nullptr, KE_QKV, &qa);
        });
    } else if (epi == KE_GATE) {
        const KWeight *ws2[2] = {&kw[0], &kw[1]};
        float *ds2[2] = {(float *)dout, (float *)run.buf((size_t)Ms[1] * 4)};
        launch_kbig(2, ws2, ds2, src, nullptr, KE_GATE);
    } else {  // as plan_launch_k's mmvq
        const KWeight *ws[3] = {&kw[0], &kw[1], &kw[2]};
        float *ds[3] = {(float *)dout, (float *)dout + Ms[0], (float *)dout + Ms[0] + Ms[1]};
        for_each_type_run(ws, nw, [&](int i, int j) { launch_kbig(j - i, ws + i, ds + i, src, (const float *)dres); });
    }
    if (dy && epi != KE_ROW) {  // the normed row of the same staging code: the tap of a KE_ROW launch of w0
        const KWeight *ws1[1] = {&kw[0]};
        float *ds1[1] = {(float *)run.buf((size_t)Ms[0] * 4)};
        launch_kbig(1, ws1, ds1, RowSrc{KX_NORM, (const float *)dx, (const float *)dxw, eps, (float *)dy}, nullptr);
    }
    return debug_matvec_finish(run, out, dout, n_out, y_out, dy, (size_t)K * 4, kv);
}

// k_mmvq_f16: w0 (w1, w2) F16 matrices of width K (device copies where they have one, else uploaded here).  Pairs (plan_launch_f16),
// xsrc KX_* / epi KE_* as for ggml_hip_debug_mat_vec_kbig: KX_NORM + KE_QKV (wq, wk, wv), KX_NORM + KE_ROW (1-3 matrices), KX_NORM +
// KE_GATE (w1, w3), KX_F32 / KX_SILU_MUL + KE_ROW (one matrix, res nullable).  ncols columns, as a chunk of ncols tokens launches them
// (passes of 8 / 4 / 2 / 1): x [ncols][K]; xw [K] (KX_NORM) or [ncols][K] (KX_SILU_MUL); res [ncols][M0]; out [ncols][M] with M = M0 +
// M1 + M2 (KE_ROW: the matrices' rows one after the other per column) or M0 (KE_GATE; KE_QKV: Q); y_out [ncols][K].  QKV: column c sits
// at position n_past + c.  Everything else as for ggml_hip_debug_mat_vec_kbig.
int ggml_hip_debug_mat_vec_f16(const struct ggml_tensor *w0, const struct ggml_tensor *w1, const struct ggml_tensor *w2, int xsrc,
                               int epi, const float *x, const float *xw, float eps, const float *res, float *out, float *y_out,
                               int n_past, int D, float freq_base, float freq_scale, int64_t C, uint16_t *mem_k, uint16_t *mem_v,
                               int ncols) {
    DebugRun run;
    const ggml_tensor *ts[3] = {w0, w1, w2};
    const int nw = (out && ncols >= 1 && ncols <= MULTI_MAX_N) ? debug_kx_matrices(w0, w1, w2, xsrc, epi, x, xw, res) : 0;
    if (!nw) return -1;
    const int64_t K = w0->ne[0];
    int64_t Ms[3] = {0, 0, 0};
    for (int i = 0; i < nw; i++) {
        const ggml_tensor *t = ts[i];
        if (!t || t->type != GGML_TYPE_F16 || t->ne[0] != K || t->ne[2] != 1 || t->ne[3] != 1 || !ggml_is_contiguous(t)) return -1;
        Ms[i] = t->ne[1];
    }
    if (K % 8 != 0) return -1;  // (before anything is uploaded: rows of 16-byte chunks)
    if (epi == KE_QKV && !debug_qkv_ok(mem_k, mem_v, D, Ms[0], Ms[1], Ms[2], n_past, ncols, C)) return -1;
    debug_hot_line();
    F16W fw[3];
    for (int i = 0; i < nw; i++) {
        const ggml_tensor *t = ts[i];
        DevTensor *e = extra_of(t);
        if (!e) e = find_tensor((uintptr_t)t->data);
        const char *d = e && !e->soa && !e->ksoa ? e->dev + ((uintptr_t)t->data - e->host) : run.buf(ggml_nbytes(t), t->data);
        fw[i] = F16W{(const __half *)d, (int64_t)t->nb[1] / 2, Ms[i]};
    }
    if (!f16_launch_ok(nw, fw, K, xsrc, epi)) return -1;
    const size_t nx = (size_t)ncols * K * 4;
    char *dx = run.buf(nx, x);
    char *dxw = xw ? run.buf(xsrc == KX_SILU_MUL ? nx : (size_t)K * 4, xw) : nullptr;
    char *dres = res ? run.buf((size_t)ncols * Ms[0] * 4, res) : nullptr;
    const int64_t Mrow = epi == KE_ROW ? Ms[0] + Ms[1] + Ms[2] : Ms[0];
    const size_t n_out = (size_t)ncols * Mrow * 4;
    char *dout = run.buf(n_out);
    char *dy = (xsrc == KX_NORM && y_out) ? run.buf(nx) : nullptr;
    const RowSrc src{xsrc, (const float *)dx, (const float *)dxw, eps, epi == KE_ROW ? (float *)dy : nullptr};
    DebugQkv kv;
    if (epi == KE_QKV) {
        kv = debug_qkv(run, n_past, ncols, D, freq_base, freq_scale, C, Ms[1], mem_k, mem_v);
        F16Qkv qa;
        memset(&qa, 0, sizeof(qa));
        qa.rope = kv.rope; qa.prm = kv.prm; qa.mem_k = (__half *)kv.dk; qa.mem_v = (__half *)kv.dv; qa.Egqa = Ms[1]; qa.C = C; qa.D = D;
        float *ds3[3] = {(float *)dout, nullptr, nullptr};
        const int kinds[3] = {0, 1, 2};
        launch_f16(3, fw, ds3, K, src, nullptr, ncols, KE_QKV, &qa, kinds);
    } else if (epi == KE_GATE) {
        float *ds2[2] = {(float *)dout, nullptr};
        launch_f16(2, fw, ds2, K, src, nullptr, ncols, KE_GATE);
    } else if (nw == 1) {
        float *ds1[1] = {(float *)dout};
        launch_f16(1, fw, ds1, K, src, (const float *)dres, ncols);
    } else {  // several matrices behind the norm: the kernel writes [ncols][M_i] per matrix; gathered into [ncols][M0 + M1 + M2] here
        float *ds[3] = {nullptr, nullptr, nullptr};
        for (int i = 0; i < nw; i++) ds[i] = (float *)run.buf((size_t)ncols * Ms[i] * 4);
        launch_f16(nw, fw, ds, K, src, nullptr, ncols);
        int64_t at = 0;
        for (int i = 0; i < nw; i++) {
            HIP_CHECK(hipMemcpy2DAsync(dout + at * 4, (size_t)Mrow * 4, ds[i], (size_t)Ms[i] * 4, (size_t)Ms[i] * 4, (size_t)ncols, hipMemcpyDeviceToDevice, g.stream));
            at += Ms[i];
        }
    }
    if (dy && epi != KE_ROW) {  // the normed rows of the same staging code: the tap of a KE_ROW launch of w0
        float *ds1[1] = {(float *)run.buf((size_t)ncols * Ms[0] * 4)};
        launch_f16(1, fw, ds1, K, RowSrc{KX_NORM, (const float *)dx, (const float *)dxw, eps, (float *)dy}, nullptr, ncols);
    }
    return debug_matvec_finish(run, out, dout, n_out, y_out, dy, nx, kv);
}

}  // extern "C"
