// backend_tools.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip, inside its anonymous
// namespace where noted): measurement and test hooks — launch probes, timeline read-back, debug entry points, counters, version.  At file scope.
namespace {
template <int NARG>
struct EmptyArgs {
    long long *ts;
    int idx;
    int pad[(NARG - 12) / 4];
};
template <int NARG>
__global__ void __launch_bounds__(1024) k_empty(const EmptyArgs<NARG> a, int last_arg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    long long t0;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0));
    const int v = a.pad[(NARG - 12) / 4 - 1] + last_arg;  // the far end of the kernarg segment
    long long t1 = v != 0x7fffffff ? (long long)wall_clock64() : 0;
    if (v == 0x12345678) smem[threadIdx.x] = 1;  // keeps the dynamic LDS allocation referenced
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        a.ts[a.idx * 4] = t0;
        a.ts[a.idx * 4 + 1] = t1;
        a.ts[a.idx * 4 + 2] = (long long)wall_clock64();
    }
}
template <int NARG>
void empty_launch(int wgs, int threads, int lds, long long *ts, int idx) {
    EmptyArgs<NARG> a;
    memset(&a, 0, sizeof(a));
    a.ts = ts;
    a.idx = idx;
    lds_opt_in<k_empty<NARG>>((size_t)lds, 160 * 1024);
    hipLaunchKernelGGL(k_empty<NARG>, dim3(wgs), dim3(threads), (size_t)lds, g.stream, a, 0);
}
}  // namespace
extern "C" {
int ggml_hip_bench_empty(int wgs, int threads, int lds_bytes, int kernarg_bytes, int n_launch, int replays, double *out) {
    SlotLock lk;
    ensure_init();
    if (n_launch < 2 || n_launch > 512 || replays < 1 || threads < 64 || threads > 1024 || lds_bytes > 160 * 1024) return -1;
    long long *ts = nullptr;
    HIP_CHECK(hipMalloc((void **)&ts, (size_t)n_launch * 32));
    HIP_CHECK(hipMemsetAsync(ts, 0, (size_t)n_launch * 32, g.stream));
    hipGraph_t gr = nullptr;
    hipGraphExec_t ex = nullptr;
    HIP_CHECK(hipStreamBeginCapture(g.stream, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < n_launch; i++) {
        if (kernarg_bytes <= 64) empty_launch<64>(wgs, threads, lds_bytes, ts, i);
        else if (kernarg_bytes <= 192) empty_launch<192>(wgs, threads, lds_bytes, ts, i);
        else empty_launch<448>(wgs, threads, lds_bytes, ts, i);
    }
    HIP_CHECK(hipStreamEndCapture(g.stream, &gr));
    HIP_CHECK(hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0));
    HIP_CHECK(hipGraphLaunch(ex, g.stream));
    hipEvent_t a, b;
    HIP_CHECK(hipEventCreate(&a));
    HIP_CHECK(hipEventCreate(&b));
    HIP_CHECK(hipEventRecord(a, g.stream));
    for (int i = 0; i < replays; i++) HIP_CHECK(hipGraphLaunch(ex, g.stream));
    HIP_CHECK(hipEventRecord(b, g.stream));
    HIP_CHECK(hipStreamSynchronize(g.stream));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    std::vector<long long> h((size_t)n_launch * 4);
    HIP_CHECK(hipMemcpy(h.data(), ts, (size_t)n_launch * 32, hipMemcpyDeviceToHost));
    double gap = 0, karg = 0;
    for (int i = 1; i < n_launch; i++) {
        gap += (double)(h[i * 4] - h[(i - 1) * 4 + 2]) / 100.0;
        karg += (double)(h[i * 4 + 1] - h[i * 4]) / 100.0;
    }
    out[0] = (double)ms * 1e3 / ((double)n_launch * replays);
    out[1] = gap / (n_launch - 1);
    out[2] = karg / (n_launch - 1);
    HIP_CHECK(hipEventDestroy(a));
    HIP_CHECK(hipEventDestroy(b));
    HIP_CHECK(hipGraphExecDestroy(ex));
    HIP_CHECK(hipGraphDestroy(gr));
    HIP_CHECK(hipFree(ts));
    return 0;
}

// Test hook: the attention of a prompt batch on host arrays through either path of the prompt plan (plan_prompt.inc
// prompt_attention): q [N][E] f32 with RoPE applied, mem_k [C][Egqa] / mem_v [Egqa][C] f16 of one layer, out [N][E] f32.
// Returns 0, or -1 when `fused` is asked for a shape the fused kernel does not take.
int ggml_hip_debug_prompt_attention(const float *q, const uint16_t *mem_k, const uint16_t *mem_v, float *out, int N, int E, int Egqa,
                                    int H, int n_past, int64_t C, float scale, int fused) {
    SlotLock lk;
    ensure_init();
    finish_pending();
    const int64_t D = E / H, Hkv = Egqa / D, T = (int64_t)n_past + N, Tp = (T + 7) & ~(int64_t)7;
    if (T > C || (fused && !prompt_attn_fits(D, T))) return -1;
    char *dq, *dk, *dv, *dout, *dsc, *dp;
    const size_t nq = (size_t)N * E * 4, nkv = (size_t)C * Egqa * 2, nsc = (size_t)H * N * T * 4, np = (size_t)H * N * Tp * 2;
    dev_malloc((void **)&dq, nq, "debug q");
    dev_malloc((void **)&dk, nkv, "debug k");
    dev_malloc((void **)&dv, nkv, "debug v");
    dev_malloc((void **)&dout, nq, "debug out");
    dev_malloc((void **)&dsc, nsc, "debug scores");
    dev_malloc((void **)&dp, np, "debug probabilities");
    h2d_bulk(dq, q, nq);
    h2d_bulk(dk, mem_k, nkv);
    h2d_bulk(dv, mem_v, nkv);
    HIP_CHECK(hipMemsetAsync(dout, 0xFF, nq, g.stream));
    prompt_attention(fused != 0, (const float *)dq, (const __half *)dk, (const __half *)dv, (float *)dout, (float *)dsc, (_Float16 *)dp, N, E,
                     Egqa, H, Hkv, D, n_past, C, scale);
    d2h_queue(out, dout, nq);
    d2h_finish();
    for (char *b : {dq, dk, dv, dout, dsc, dp}) HIP_CHECK(hipFree(b));
    return 0;
}

// Test hook: one weight matrix times N (2..8) activation rows through k_mmq_cols exactly as the multi-token plan launches it
// (k_quant_row with its [block][8] tables, then the EPI_STORE launch).  w: a quantized 2-D weight with a device copy;
// x: host [N][K] f32; out: host [N][M] f32.  Returns 0, or -1 when the plan would not take this shape on k_mmq_cols.
int ggml_hip_debug_mul_mat_cols(const struct ggml_tensor *w, const float *x, float *out, int N) {
    SlotLock lk;
    ensure_init();
    finish_pending();
    const int qt = qt_of(w->type);
    if (qt < 0 || N < 2 || N > 8) return -1;
    const QWeight qw = qweight_of(w);
    const int64_t K = w->ne[0], M = w->ne[1], nb = K / 32;
    if (!cols_ok((int)M, 1, nb, {M})) return -1;
    char *dx, *dlo, *dhi, *dd, *ds, *ddT, *dsT, *dout;
    dev_malloc((void **)&dx, (size_t)N * K * 4, "debug x");
    dev_malloc((void **)&dlo, (size_t)N * K / 2, "debug lo");
    dev_malloc((void **)&dhi, (size_t)N * K / 2, "debug hi");
    dev_malloc((void **)&dd, (size_t)N * nb * 4, "debug d");
    dev_malloc((void **)&ds, (size_t)N * nb * 4, "debug s");
    dev_malloc((void **)&ddT, (size_t)nb * 32, "debug dT");
    dev_malloc((void **)&dsT, (size_t)nb * 32, "debug sT");
    dev_malloc((void **)&dout, (size_t)N * M * 4, "debug out");
    h2d_bulk(dx, x, (size_t)N * K * 4);
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
    HIP_CHECK(hipGetLastError());
    d2h_queue(out, dout, (size_t)N * M * 4);
    d2h_finish();
    for (char *b : {dx, dlo, dhi, dd, ds, ddT, dsT, dout}) HIP_CHECK(hipFree(b));
    return 0;
}

// Test hooks of the decode mat-vecs: ONE launch of k_mmvq_big (Q4_0 .. Q8_0) or k_mmvq_kbig (K-quants) on host arrays, with the
// source / epilogue pairs and the arguments the single-token plans launch them with (plan_launch_all, plan_launch_k).  Every
// output buffer (and the K / V caches, uploaded from the host first) is followed by DEBUG_GUARD bytes; outputs and guards are
// 0xFF (NaN) before the launch and come back whole, guard included, so a test sees an element never written and a store past
// the end.  -1 for a shape or a pair the plans would not launch.
namespace {
constexpr size_t DEBUG_GUARD = 256;
// n bytes + the guard on the device: `init`'s n bytes (nullptr: 0xFF) followed by 0xFF
char *debug_buf(size_t n, const void *init, std::vector<char *> &owned) {
    char *d;
    dev_malloc((void **)&d, n + DEBUG_GUARD, "a debug buffer");
    owned.push_back(d);
    if (init) {
        h2d_bulk(d, init, n);
        HIP_CHECK(hipMemsetAsync(d + n, 0xFF, DEBUG_GUARD, g.stream));
    } else {
        HIP_CHECK(hipMemsetAsync(d, 0xFF, n + DEBUG_GUARD, g.stream));
    }
    return d;
}
void debug_hot_line() {
    if (!g.hot_line) {  // as plan building makes it
        dev_malloc(&g.hot_line, 256, "the dummy ring steps' line");
        HIP_CHECK(hipMemsetAsync(g.hot_line, 0, 256, g.stream));
    }
}
// the token's DecParams (n_past; store_at 0 = n_past) and its RoPE table, made by k_rope_table as the plans make it
void debug_rope(int n_past, int D, float freq_base, float freq_scale, std::vector<char *> &owned, DecParams **prm, float **rope) {
    DecParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.n_past = n_past;
    dev_malloc((void **)prm, sizeof(DecParams), "debug params");
    dev_malloc((void **)rope, 256 * 4, "debug rope table");
    owned.push_back((char *)*prm);
    owned.push_back((char *)*rope);
    h2d_bulk((char *)*prm, &hp, sizeof(hp));
    const float theta_scale = powf(freq_base, -2.0f / (float)D);  // n_dims = the head size, as in LlamaMatch
    hipLaunchKernelGGL(k_rope_table, dim3(1), dim3(128), 0, g.stream, (const DecParams *)*prm, theta_scale, freq_scale, D >> 1, *rope,
                       (unsigned *)nullptr);
    HIP_CHECK(hipGetLastError());
}
}  // namespace

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
    SlotLock lk;
    ensure_init();
    finish_pending();
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
    if (epi == EPI_QKV && (!mem_k || !mem_v || D < 2 || D % 2 || D > 256 || M0 % D || M1 % D || M1 != M2 || n_past < 0 || n_past >= C))
        return -1;
    // staging limits (BigX): the norm 8192 elements over 1024 threads, launch_big's wave counts up to BIG_W, LDS; and the dealing
    // launch_big would abort on
    if (xsrc == XSRC_NORM && nb * 8 > (int64_t)BigX<XSRC_NORM>::MAXIT * BigX<XSRC_NORM>::NT) return -1;
    const BigShape bsh = big_shape(xsrc, epi, nb, (M0 + M1 + M2) / (epi == EPI_QKV ? 2 : 1));
    if (big_min_waves(xsrc, epi, nb) > BIG_W || bsh.lds > 64 * 1024 || !bsh.ok) return -1;

    std::vector<char *> owned;
    debug_hot_line();
    DecMmvqArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < nw; i++) a.w[i] = qweight_of(ts[i]);
    a.nb = nb;
    char *dx = debug_buf((size_t)K * 4, x, owned);
    a.xf = (const float *)dx;
    if (xsrc == XSRC_NORM) {
        a.xw = (const float *)debug_buf((size_t)K * 4, norm_w, owned);
        a.eps = eps;
    }
    if (xsrc == XSRC_Q8) {  // the planar Q8 row, as k_quant_row makes it
        char *dlo = debug_buf((size_t)K / 2, nullptr, owned), *dhi = debug_buf((size_t)K / 2, nullptr, owned);
        char *dd = debug_buf((size_t)nb * 4, nullptr, owned), *ds = debug_buf((size_t)nb * 4, nullptr, owned);
        launch_quant_row(qt_f16d(qt), (const float *)dx, nb, 1, (int8_t *)dlo, (int8_t *)dhi, (float *)dd, (int *)ds, nullptr, nullptr);
        HIP_CHECK(hipGetLastError());
        a.x = QAct{(const i32x4 *)dlo, (const i32x4 *)dhi, (const float *)dd, (const int *)ds};
    }
    if (epi == EPI_ADD) a.res = (const float *)debug_buf((size_t)M0 * 4, res, owned);
    const size_t n_out = (size_t)M0 * 4;  // (QKV: Q)
    char *dout = debug_buf(n_out, nullptr, owned);
    a.dst = (float *)dout;
    char *dy = (xsrc == XSRC_NORM && y_out) ? debug_buf((size_t)K * 4, nullptr, owned) : nullptr;
    float *rope = nullptr;
    char *dk = nullptr, *dv = nullptr;
    const size_t nkv = epi == EPI_QKV ? (size_t)C * M1 * 2 : 0;
    if (epi == EPI_QKV) {
        DecParams *prm;
        debug_rope(n_past, D, freq_base, freq_scale, owned, &prm, &rope);
        dk = debug_buf(nkv, mem_k, owned);
        dv = debug_buf(nkv, mem_v, owned);
        a.prm = prm;
        a.mem_k = (__half *)dk;
        a.mem_v = (__half *)dv;
        a.Egqa = M1;
        a.C = C;
        a.D = D;
        a.theta_scale = powf(freq_base, -2.0f / (float)D);
        a.freq_scale = freq_scale;
    }
    // the launcher plan_launch_all uses (no timeline, no probe, no granules; the dealing is launch_big's)
    const BigArgs ba{a, epi == EPI_STORE ? (float *)dy : nullptr, nullptr, 0, rope, 0, nullptr, nullptr, 0, g.hot_line};
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
        t.dst = (float *)debug_buf((size_t)M0 * 4, nullptr, owned);
        with_qt(qt, [&](auto QT) { launch_big<CT(QT), EPI_STORE, XSRC_NORM>(BigArgs{t, (float *)dy, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, g.hot_line}); });
        HIP_CHECK(hipGetLastError());
    }
    d2h_queue(out, dout, n_out + DEBUG_GUARD);
    if (dy) d2h_queue(y_out, dy, (size_t)K * 4 + DEBUG_GUARD);
    if (dk) {
        d2h_queue(mem_k, dk, nkv + DEBUG_GUARD);
        d2h_queue(mem_v, dv, nkv + DEBUG_GUARD);
    }
    d2h_finish();
    for (char *b : owned) HIP_CHECK(hipFree(b));
    return 0;
}

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
    SlotLock lk;
    ensure_init();
    finish_pending();
    const bool pair_ok = (xsrc == KX_NORM && (epi == KE_QKV || epi == KE_ROW || epi == KE_GATE)) ||
                         ((xsrc == KX_F32 || xsrc == KX_SILU_MUL) && epi == KE_ROW);
    const ggml_tensor *ts[3] = {w0, w1, w2};
    const int nw = epi == KE_QKV ? 3 : epi == KE_GATE ? 2 : !w1 ? 1 : !w2 ? 2 : 3;
    if (!pair_ok || !x || !w0 || (xsrc != KX_F32 && !xw)) return -1;
    if ((xsrc != KX_NORM || epi != KE_ROW) && nw > 1 && epi == KE_ROW) return -1;  // several matrices: only behind the norm
    if (res && (epi != KE_ROW || nw > 1)) return -1;
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
    if (epi == KE_QKV && (!mem_k || !mem_v || D < 2 || D % 2 || D > 256 || Ms[0] % D || Ms[1] % D || Ms[1] != Ms[2] || Ms[0] % 2 ||
                          Ms[1] % 2 || n_past < 0 || n_past >= C))
        return -1;

    std::vector<char *> owned;
    debug_hot_line();
    KWeight kw[3];
    for (int i = 0; i < nw; i++) kw[i] = kweight_of(ts[i]);
    char *dx = debug_buf((size_t)K * 4, x, owned);
    char *dxw = xw ? debug_buf((size_t)K * 4, xw, owned) : nullptr;
    char *dres = res ? debug_buf((size_t)Ms[0] * 4, res, owned) : nullptr;
    const int64_t Mrow = epi == KE_ROW ? Ms[0] + Ms[1] + Ms[2] : Ms[0];
    const size_t n_out = (size_t)Mrow * 4;
    char *dout = debug_buf(n_out, nullptr, owned);
    char *dy = (xsrc == KX_NORM && y_out) ? debug_buf((size_t)K * 4, nullptr, owned) : nullptr;
    const RowSrc src{xsrc, (const float *)dx, (const float *)dxw, eps, epi == KE_ROW ? (float *)dy : nullptr};
    char *dk = nullptr, *dv = nullptr;
    const size_t nkv = epi == KE_QKV ? (size_t)C * Ms[1] * 2 : 0;
    if (epi == KE_QKV) {  // as plan_launch_k: one launch per run of equal types, seg_kind = the matrices' kinds
        DecParams *prm;
        float *rope;
        debug_rope(n_past, D, freq_base, freq_scale, owned, &prm, &rope);
        dk = debug_buf(nkv, mem_k, owned);
        dv = debug_buf(nkv, mem_v, owned);
        const KWeight *ws3[3] = {&kw[0], &kw[1], &kw[2]};
        float *ds3[3] = {(float *)dout, nullptr, nullptr};
        for_each_type_run(ws3, 3, [&](int i, int j) {
            KBigArgs qa;
            memset(&qa, 0, sizeof(qa));
            for (int k = i; k < j; k++) qa.seg_kind[k - i] = k;
            qa.rope = rope; qa.prm = prm; qa.mem_k = (__half *)dk; qa.mem_v = (__half *)dv; qa.Egqa = Ms[1]; qa.C = C; qa.D = D;
            launch_kbig(j - i, ws3 + i, ds3 + i, src, nullptr, KE_QKV, &qa);
        });
    } else if (epi == KE_GATE) {
        const KWeight *ws2[2] = {&kw[0], &kw[1]};
        float *ds2[2] = {(float *)dout, (float *)debug_buf((size_t)Ms[1] * 4, nullptr, owned)};
        launch_kbig(2, ws2, ds2, src, nullptr, KE_GATE);
    } else {  // as plan_launch_k's mmvq
        const KWeight *ws[3] = {&kw[0], &kw[1], &kw[2]};
        float *ds[3] = {(float *)dout, (float *)dout + Ms[0], (float *)dout + Ms[0] + Ms[1]};
        for_each_type_run(ws, nw, [&](int i, int j) { launch_kbig(j - i, ws + i, ds + i, src, (const float *)dres); });
    }
    if (dy && epi != KE_ROW) {  // the normed row of the same staging code: the tap of a KE_ROW launch of w0
        const KWeight *ws1[1] = {&kw[0]};
        float *ds1[1] = {(float *)debug_buf((size_t)Ms[0] * 4, nullptr, owned)};
        launch_kbig(1, ws1, ds1, RowSrc{KX_NORM, (const float *)dx, (const float *)dxw, eps, (float *)dy}, nullptr);
    }
    d2h_queue(out, dout, n_out + DEBUG_GUARD);
    if (dy) d2h_queue(y_out, dy, (size_t)K * 4 + DEBUG_GUARD);
    if (dk) {
        d2h_queue(mem_k, dk, nkv + DEBUG_GUARD);
        d2h_queue(mem_v, dv, nkv + DEBUG_GUARD);
    }
    d2h_finish();
    for (char *b : owned) HIP_CHECK(hipFree(b));
    return 0;
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
    SlotLock lk;
    ensure_init();
    finish_pending();
    const ggml_tensor *ts[3] = {w0, w1, w2};
    const int nw = epi == KE_QKV ? 3 : epi == KE_GATE ? 2 : !w1 ? 1 : !w2 ? 2 : 3;
    if (!x || !w0 || !out || ncols < 1 || ncols > MULTI_MAX_N || (xsrc != KX_F32 && !xw)) return -1;
    if (xsrc != KX_NORM && nw > 1) return -1;  // several matrices: only behind the norm
    if (res && (epi != KE_ROW || nw > 1)) return -1;
    const int64_t K = w0->ne[0];
    int64_t Ms[3] = {0, 0, 0};
    for (int i = 0; i < nw; i++) {
        const ggml_tensor *t = ts[i];
        if (!t || t->type != GGML_TYPE_F16 || t->ne[0] != K || t->ne[2] != 1 || t->ne[3] != 1 || !ggml_is_contiguous(t)) return -1;
        Ms[i] = t->ne[1];
    }
    if (K % 8 != 0) return -1;  // (before anything is uploaded: rows of 16-byte chunks)
    if (epi == KE_QKV && (!mem_k || !mem_v || D < 2 || D % 2 || D > 256 || Ms[0] % D || Ms[1] % D || Ms[1] != Ms[2] || n_past < 0 ||
                          n_past + ncols > C))
        return -1;
    std::vector<char *> owned;
    debug_hot_line();
    F16W fw[3];
    for (int i = 0; i < nw; i++) {
        const ggml_tensor *t = ts[i];
        DevTensor *e = extra_of(t);
        if (!e) e = find_tensor((uintptr_t)t->data);
        const char *d = e && !e->soa && !e->ksoa ? e->dev + ((uintptr_t)t->data - e->host) : debug_buf(ggml_nbytes(t), t->data, owned);
        fw[i] = F16W{(const __half *)d, (int64_t)t->nb[1] / 2, Ms[i]};
    }
    if (!f16_launch_ok(nw, fw, K, xsrc, epi)) {
        for (char *b : owned) HIP_CHECK(hipFree(b));
        return -1;
    }
    const size_t nx = (size_t)ncols * K * 4;
    char *dx = debug_buf(nx, x, owned);
    char *dxw = xw ? debug_buf(xsrc == KX_SILU_MUL ? nx : (size_t)K * 4, xw, owned) : nullptr;
    char *dres = res ? debug_buf((size_t)ncols * Ms[0] * 4, res, owned) : nullptr;
    const int64_t Mrow = epi == KE_ROW ? Ms[0] + Ms[1] + Ms[2] : Ms[0];
    const size_t n_out = (size_t)ncols * Mrow * 4;
    char *dout = debug_buf(n_out, nullptr, owned);
    char *dy = (xsrc == KX_NORM && y_out) ? debug_buf(nx, nullptr, owned) : nullptr;
    const RowSrc src{xsrc, (const float *)dx, (const float *)dxw, eps, epi == KE_ROW ? (float *)dy : nullptr};
    char *dk = nullptr, *dv = nullptr;
    const size_t nkv = epi == KE_QKV ? (size_t)C * Ms[1] * 2 : 0;
    if (epi == KE_QKV) {
        DecParams hp;
        memset(&hp, 0, sizeof(hp));
        hp.n_past = n_past;
        DecParams *prm = (DecParams *)debug_buf(sizeof(DecParams), &hp, owned);
        float *rope = (float *)debug_buf((size_t)ncols * 128 * 4, nullptr, owned);
        hipLaunchKernelGGL(k_rope_table, dim3((unsigned)ncols), dim3(128), 0, g.stream, (const DecParams *)prm, powf(freq_base, -2.0f / (float)D),
                           freq_scale, D >> 1, rope, (unsigned *)nullptr);
        HIP_CHECK(hipGetLastError());
        dk = debug_buf(nkv, mem_k, owned);
        dv = debug_buf(nkv, mem_v, owned);
        F16Qkv qa;
        memset(&qa, 0, sizeof(qa));
        qa.rope = rope; qa.prm = prm; qa.mem_k = (__half *)dk; qa.mem_v = (__half *)dv; qa.Egqa = Ms[1]; qa.C = C; qa.D = D;
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
        for (int i = 0; i < nw; i++) ds[i] = (float *)debug_buf((size_t)ncols * Ms[i] * 4, nullptr, owned);
        launch_f16(nw, fw, ds, K, src, nullptr, ncols);
        int64_t at = 0;
        for (int i = 0; i < nw; i++) {
            HIP_CHECK(hipMemcpy2DAsync(dout + at * 4, (size_t)Mrow * 4, ds[i], (size_t)Ms[i] * 4, (size_t)Ms[i] * 4, (size_t)ncols, hipMemcpyDeviceToDevice, g.stream));
            at += Ms[i];
        }
    }
    if (dy && epi != KE_ROW) {  // the normed rows of the same staging code: the tap of a KE_ROW launch of w0
        float *ds1[1] = {(float *)debug_buf((size_t)ncols * Ms[0] * 4, nullptr, owned)};
        launch_f16(1, fw, ds1, K, RowSrc{KX_NORM, (const float *)dx, (const float *)dxw, eps, (float *)dy}, nullptr, ncols);
    }
    d2h_queue(out, dout, n_out + DEBUG_GUARD);
    if (dy) d2h_queue(y_out, dy, nx + DEBUG_GUARD);
    if (dk) {
        d2h_queue(mem_k, dk, nkv + DEBUG_GUARD);
        d2h_queue(mem_v, dv, nkv + DEBUG_GUARD);
    }
    d2h_finish();
    for (char *b : owned) HIP_CHECK(hipFree(b));
    return 0;
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
    SlotLock lk;
    ensure_init();
    finish_pending();
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
    std::vector<char *> owned;
    for (Out &e : o)
        if (e.n) e.dev = debug_buf(e.n, nullptr, owned);
    auto dev = [&](size_t i) { return i < o.size() ? o[i].dev : nullptr; };
    const size_t n_in = part ? (size_t)part + nel : (size_t)(rows - 1) * stride + K;
    const char *da = debug_buf(n_in * 4, a, owned);
    const char *db = b ? debug_buf((two ? n_in : nel) * 4, b, owned) : nullptr;
    const char *dr = r ? debug_buf(nel * 4, r, owned) : nullptr;
    const char *dw = norm ? debug_buf((size_t)K * 4, w, owned) : nullptr;
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
    HIP_CHECK(hipGetLastError());
    for (const Out &e : o)
        if (e.n) d2h_queue(e.host, e.dev, e.n + DEBUG_GUARD);
    d2h_finish();
    for (char *p : owned) HIP_CHECK(hipFree(p));
    return 0;
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
    SlotLock lk;
    ensure_init();
    finish_pending();
    if (!q_raw || !rope || !mem_k || !mem_v || !x16 || N < 1 || H < 1 || E % H || n_past < 0) return -1;
    const int64_t D = E / H, T = (int64_t)n_past + N;
    if (Egqa < D || Egqa % D || H % (Egqa / D) || T > C || C % 8 || !prompt_attn_fits(D, T)) return -1;
    const int64_t Hkv = Egqa / D;
    std::vector<char *> owned;
    const size_t nq = (size_t)N * E * 4, nkv = (size_t)C * Egqa * 2, nx = (size_t)N * E * 2;
    char *dq = debug_buf(nq * (q_raw2 ? 2 : 1), nullptr, owned);
    h2d_bulk(dq, q_raw, nq);
    if (q_raw2) h2d_bulk(dq + nq, q_raw2, nq);
    char *dr = debug_buf((size_t)N * 128 * 4, rope, owned);
    char *dk = debug_buf(nkv, mem_k, owned), *dv = debug_buf(nkv, mem_v, owned);
    char *dx = debug_buf(nx, nullptr, owned), *dout = debug_buf(nq, nullptr, owned);
    prompt_attention(true, (const float *)dq, (const __half *)dk, (const __half *)dv, (float *)dout, nullptr, nullptr, N, E, Egqa, H, Hkv,
                     D, n_past, C, scale, (_Float16 *)dx, f16d != 0, (const float *)dr, q_raw2 ? (int64_t)N * E : 0);
    d2h_queue(x16, dx, nx + DEBUG_GUARD);
    if (out) d2h_queue(out, dout, nq + DEBUG_GUARD);
    d2h_finish();
    for (char *b : owned) HIP_CHECK(hipFree(b));
    return 0;
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
    SlotLock lk;
    ensure_init();
    finish_pending();
    uint16_t *d;
    dev_malloc((void **)&d, 2 * 65536 * 2, "debug exp");
    hipLaunchKernelGGL(k_debug_exp_le0, dim3(256), dim3(256), 0, g.stream, d, d + 65536);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(g.stream));
    HIP_CHECK(hipMemcpy(out_fast, d, 65536 * 2, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out_ref, d + 65536, 65536 * 2, hipMemcpyDeviceToHost));
    HIP_CHECK(hipFree(d));
    return 0;
}

// ---- test hook: k_token_tail alone, beside k_argmax_next on the same logits (tests/test_token_tail_gpu.py) ----
// logits[V] and emb[E] (nullable) go to the device (both `misalign` floats off a 16-byte boundary: the kernel's 4-byte paths), both
// kernels start from parameters {n_past, token 0}.  Out: the two ids, the slot's logits / row (the bytes the host would be handed),
// prm_out[0..2] = n_past, token, tokens[0] as k_token_tail left them.  0, or -1 for arguments it cannot take.
int ggml_hip_debug_token_tail(const float *logits, int V, const float *emb, int E, int n_past, int misalign, int32_t *id_tail,
                              int32_t *id_argmax, float *slot_logits, float *slot_emb, int32_t *prm_out) {
    if (!logits || V < 1 || (emb && E < 1) || misalign < 0 || misalign > 3 || !id_tail || !id_argmax || !slot_logits || !prm_out) return -1;
    SlotLock lk;
    ensure_init();
    finish_pending();
    const size_t lb = ((size_t)(V + 4) * 4 + 255) & ~(size_t)255, eb = ((size_t)(std::max(E, 1) + 4) * 4 + 255) & ~(size_t)255;
    const size_t emb_off = ((size_t)V * 4 + 255) & ~(size_t)255, id_off = emb_off + eb;
    char *d = nullptr, *slot = nullptr;
    dev_malloc((void **)&d, lb + eb + 1024, "debug token tail");
    HIP_CHECK(hipHostMalloc((void **)&slot, id_off + 256, hipHostMallocDefault));
    memset(slot, 0xff, id_off + 256);
    float *dl = (float *)d + misalign, *de = (float *)(d + lb) + misalign;
    DecParams *pa = (DecParams *)(d + lb + eb), *pb = pa + 1;
    int *ida = (int *)(pb + 1);
    DecParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.n_past = n_past;
    HIP_CHECK(hipStreamSynchronize(g.stream));
    HIP_CHECK(hipMemcpy(dl, logits, (size_t)V * 4, hipMemcpyHostToDevice));
    if (emb) HIP_CHECK(hipMemcpy(de, emb, (size_t)E * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(pa, &hp, sizeof(hp), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(pb, &hp, sizeof(hp), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_argmax_next, dim3(1), dim3(1024), 0, g.stream, (const float *)dl, V, pa, (BatchCols *)nullptr, ida);
    hipLaunchKernelGGL(k_token_tail, dim3(TOKEN_TAIL_WGS), dim3(1024), 0, g.stream, (const float *)dl, V, emb ? (const float *)de : (const float *)nullptr,
                       E, pb, slot, (int)emb_off, (int)id_off, TailPrep{});
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(g.stream));
    HIP_CHECK(hipMemcpy(id_argmax, ida, 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(&hp, pb, sizeof(hp), hipMemcpyDeviceToHost));
    prm_out[0] = hp.n_past;
    prm_out[1] = hp.token;
    prm_out[2] = hp.tokens[0];
    *id_tail = *(const int32_t *)(slot + id_off);
    memcpy(slot_logits, slot, (size_t)V * 4);
    if (emb && slot_emb) memcpy(slot_emb, slot + emb_off, (size_t)E * 4);
    HIP_CHECK(hipHostFree(slot));
    HIP_CHECK(hipFree(d));
    return 0;
}

// ---- test hook: k_token_tail with a TailPrep, beside the three launches it stands for (tests/test_token_tail_prepare_gpu.py) ----
// logits[V]; wte_raw: V rows of E elements in ggml's block format `wtype` (Q4_0 .. Q8_0), relaid as an upload relays them; mem_k
// [L][C][Egqa] / mem_v [L][Egqa][C] f16; the parameters start at {n_past, token 0, pos_tail = n_past, n_past}, the epoch at epoch_in.
// One launch of k_token_tail of parity `parity` (a graph's tail_prep_args: it reads pos_tail[parity], writes pos_tail[parity ^ 1])
// prepares position n_past + 1; `zeroed` != 0: the same launch with a zeroed TailPrep.  Beside it, on a second set of parameters:
// k_argmax_next, then k_get_rows_q, k_rope_table and k_kv_row_save as a token's graph opens with them.  Out, from the tail / from the
// reference launches: row [E], table [128], epoch, save [2 * L * Egqa] halves — each 0xFF where never written — and prm_out[0..4] =
// n_past, token, tokens[0], pos_tail[0], pos_tail[1] as the tail left them, id_out = the id in its slot.  0, or -1 for arguments
// it cannot take.
int ggml_hip_debug_token_tail_prepare(const float *logits, int V, const void *wte_raw, int wtype, int E, int n_past, uint32_t epoch_in,
                                      int parity, int zeroed, int L, int C, int Egqa, const uint16_t *mem_k, const uint16_t *mem_v,
                                      float theta_scale, float freq_scale, int half_d, int32_t *id_out, int32_t *prm_out, float *row,
                                      float *table, uint32_t *epoch_out, uint16_t *save, float *row_ref, float *table_ref,
                                      uint32_t *epoch_ref, uint16_t *save_ref) {
    const int qt = qt_of((ggml_type)wtype);
    if (!logits || V < 1 || !wte_raw || qt < 0 || E < 32 || E % 32 || n_past < 0 || n_past + 1 >= C || (parity & ~1) || L < 1 || Egqa < 1 ||
        !mem_k || !mem_v || half_d < 1 || half_d > 64 || !id_out || !prm_out || !row || !table || !epoch_out || !save || !row_ref ||
        !table_ref || !epoch_ref || !save_ref)
        return -1;
    SlotLock lk;
    ensure_init();
    finish_pending();
    std::vector<char *> owned;
    const int64_t nb = E / 32;
    const size_t raw_bytes = (size_t)V * nb * (size_t)blk_bytes(qt), nkv = (size_t)L * C * Egqa * 2, nsave = (size_t)L * Egqa * 4;
    char *draw = debug_buf(raw_bytes, wte_raw, owned);
    size_t off[5];
    char *dsoa = debug_buf(qw_layout(qt, V, nb, off), nullptr, owned);
    relayout_launch(draw, qt, V, nb, dsoa);
    const QWeight w = qw_at(dsoa, qt, V, nb);
    char *dl = debug_buf((size_t)V * 4, logits, owned);
    char *dk = debug_buf(nkv, mem_k, owned), *dv = debug_buf(nkv, mem_v, owned);
    DecParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.n_past = hp.pos_tail[0] = hp.pos_tail[1] = n_past;
    DecParams *prm[2];
    unsigned *ep[2];
    char *drow[2], *dtab[2], *dsave[2];
    for (int i = 0; i < 2; i++) {  // 0: the tail's, 1: the reference launches'
        prm[i] = (DecParams *)debug_buf(sizeof(hp), &hp, owned);
        ep[i] = (unsigned *)debug_buf(4, &epoch_in, owned);
        drow[i] = debug_buf((size_t)E * 4, nullptr, owned);
        dtab[i] = debug_buf(128 * 4, nullptr, owned);
        dsave[i] = debug_buf(nsave, nullptr, owned);
    }
    int *ida = (int *)debug_buf(4, nullptr, owned);
    char *slot = nullptr;
    const size_t id_off = ((size_t)V * 4 + 255) & ~(size_t)255;
    HIP_CHECK(hipHostMalloc((void **)&slot, id_off + 256, hipHostMallocDefault));
    memset(slot, 0xff, id_off + 256);
    TailPrep tp;
    memset(&tp, 0, sizeof(tp));
    if (!zeroed) {
        tp.xnext = (float *)drow[0];
        tp.wte = w;
        tp.rope = (float *)dtab[0]; tp.epoch = ep[0];
        tp.theta_scale = theta_scale; tp.freq_scale = freq_scale; tp.half_d = half_d;
        tp.mem_k = (const __half *)dk; tp.mem_v = (const __half *)dv; tp.save = (__half *)dsave[0];
        tp.L = L; tp.C = C; tp.Egqa = Egqa;
        tp.pos_in = &prm[0]->pos_tail[parity]; tp.pos_out = &prm[0]->pos_tail[parity ^ 1];
    }
    hipLaunchKernelGGL(k_token_tail, dim3(token_tail_grid(!zeroed, (long)L * Egqa)), dim3(1024), 0, g.stream, (const float *)dl, V,
                       (const float *)nullptr, 0, prm[0], slot, (int)id_off, (int)id_off, tp);
    hipLaunchKernelGGL(k_argmax_next, dim3(1), dim3(1024), 0, g.stream, (const float *)dl, V, prm[1], (BatchCols *)nullptr, ida);
    hipLaunchKernelGGL(k_kv_row_save, dim3((unsigned)std::min<int64_t>(256, ((int64_t)L * Egqa + 255) / 256)), dim3(256), 0, g.stream,
                       (const DecParams *)prm[1], (const __half *)dk, (const __half *)dv, (__half *)dsave[1], L, C, Egqa);
    hipLaunchKernelGGL(k_get_rows_q, dim3((unsigned)((nb + 255) / 256), 1), dim3(256), 0, g.stream, w, (const int *)&prm[1]->token,
                       (float *)drow[1], (int64_t)E);
    hipLaunchKernelGGL(k_rope_table, dim3(1), dim3(128), 0, g.stream, (const DecParams *)prm[1], theta_scale, freq_scale, half_d,
                       (float *)dtab[1], ep[1]);
    HIP_CHECK(hipGetLastError());
    float *rows[2] = {row, row_ref}, *tabs[2] = {table, table_ref};
    uint32_t *eps[2] = {epoch_out, epoch_ref};
    uint16_t *saves[2] = {save, save_ref};
    for (int i = 0; i < 2; i++) {
        d2h_queue(rows[i], drow[i], (size_t)E * 4);
        d2h_queue(tabs[i], dtab[i], 128 * 4);
        d2h_queue(eps[i], (const char *)ep[i], 4);
        d2h_queue(saves[i], dsave[i], nsave);
    }
    d2h_queue(&hp, (const char *)prm[0], sizeof(hp));
    d2h_finish();
    prm_out[0] = hp.n_past;
    prm_out[1] = hp.token;
    prm_out[2] = hp.tokens[0];
    prm_out[3] = hp.pos_tail[0];
    prm_out[4] = hp.pos_tail[1];
    *id_out = *(const int32_t *)(slot + id_off);
    HIP_CHECK(hipHostFree(slot));
    for (char *b : owned) HIP_CHECK(hipFree(b));
    return 0;
}

int ggml_hip_decode_greedy_chain(struct ggml_cgraph *last, int n, int32_t *out_tokens, float *last_logits) {
    SlotLock lk;
    return decode_greedy_chain(last, n, out_tokens, last_logits);
}

int ggml_hip_decode_batch(struct ggml_cgraph *const *graphs, int n_graphs) {
    if (!graphs || n_graphs < 2 || n_graphs > BATCH_COLS_MAX) return -1;  // (before any device is touched)
    for (int i = 0; i < n_graphs; i++)
        if (!graphs[i]) return -1;
    SlotLock lk;
    const uint64_t t0 = now_ns();
    const int r = decode_batch(graphs, n_graphs);
    g.ns_compute += now_ns() - t0;
    return r;
}

int ggml_hip_decode_batch_greedy(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, int32_t *out_ids) {
    if (!graphs || n_graphs < 2 || n_graphs > BATCH_COLS_MAX || n_steps < 1 || n_steps > BATCH_CHAIN_MAX_STEPS) return -1;  // (before any device is touched)
    if (n_steps > 1 && !out_ids) return -1;
    for (int i = 0; i < n_graphs; i++)
        if (!graphs[i]) return -1;
    SlotLock lk;
    const uint64_t t0 = now_ns();
    const int r = decode_batch_steps(graphs, n_graphs, n_steps, out_ids, true);
    g.ns_compute += now_ns() - t0;
    return r;
}

int ggml_hip_decode_batch_sampled_ex(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, const ggml_hip_sampler_chain *chain,
                                     const int32_t *windows, const int32_t *window_n, uint64_t *rng, float *mu, int32_t *out_ids) {
    if (!graphs || n_graphs < 2 || n_graphs > BATCH_COLS_MAX || n_steps < 1 || n_steps > BATCH_CHAIN_MAX_STEPS) return -1;  // (before any device is touched)
    if (!chain || !windows || !window_n || !rng || (n_steps > 1 && !out_ids)) return -1;
    for (int i = 0; i < n_graphs; i++)
        if (!graphs[i]) return -1;
    SlotLock lk;
    const uint64_t t0 = now_ns();
    const BatchSample smp = {chain, windows, window_n, rng, mu};
    const int r = decode_batch_steps(graphs, n_graphs, n_steps, out_ids, true, &smp);
    g.ns_compute += now_ns() - t0;
    return r;
}
int ggml_hip_decode_batch_sampled(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, const ggml_hip_sampler *params,
                                  const int32_t *windows, const int32_t *window_n, uint64_t *rng, int32_t *out_ids) {
    if (!params) return -1;
    const ggml_hip_sampler_chain chain = sample_neutral(params);
    return ggml_hip_decode_batch_sampled_ex(graphs, n_graphs, n_steps, &chain, windows, window_n, rng, nullptr, out_ids);
}

int ggml_hip_decode_sampled_chain_ex(struct ggml_cgraph *last, int n, const ggml_hip_sampler_chain *chain, const int32_t *window, int window_n,
                                     uint64_t *rng, float *mu, int32_t *out_tokens, float *last_logits) {
    if (!last || n < 1 || !chain || !rng || !out_tokens || window_n < 0 || window_n > SAMPLER_WINDOW || (window_n > 0 && !window))
        return -1;  // (before any device is touched)
    SlotLock lk;
    const BatchSample smp = {chain, window, &window_n, rng, mu};
    return decode_chain(last, n, out_tokens, last_logits, &smp);
}
int ggml_hip_decode_sampled_chain(struct ggml_cgraph *last, int n, const ggml_hip_sampler *params, const int32_t *window, int window_n,
                                  uint64_t *rng, int32_t *out_tokens, float *last_logits) {
    if (!params) return -1;
    const ggml_hip_sampler_chain chain = sample_neutral(params);
    return ggml_hip_decode_sampled_chain_ex(last, n, &chain, window, window_n, rng, nullptr, out_tokens, last_logits);
}

// ---- the chains that stop: a request per column (plan_run.inc ChainRequests) ----
int ggml_hip_decode_chain_requests(struct ggml_cgraph *last, int n, const ggml_hip_sampler_chain *chain, const ggml_hip_chain_end *end,
                                   const int32_t *window, int window_n, uint64_t *rng, float *mu, int32_t *out_tokens, int32_t *n_drawn,
                                   int32_t *ended_by, float *last_logits) {
    if (!last || n < 1 || n > BATCH_CHAIN_MAX_STEPS || !end || !out_tokens || !n_drawn || !ended_by) return -1;  // (before any device is touched)
    if (window_n < 0 || window_n > SAMPLER_WINDOW || (window_n > 0 && !window) || (chain && !rng)) return -1;
    if (end->budget < 1 || end->budget > n || end->n_stop < 0 || end->n_stop > CHAIN_STOP_MAX) return -1;
    SlotLock lk;
    const int32_t none[1] = {0};
    uint64_t r = rng ? *rng : 0;  // (copies: nothing moves unless the chain ran)
    float u = mu ? *mu : 0.0f;
    int32_t count = 0, why = 0;
    ChainRequests req = {&chain, end, window ? window : none, &window_n, &r, mu ? &u : nullptr, &count, &why, 0, {0, 0, 0, 0}};
    std::vector<int32_t> ids((size_t)end->budget);
    if (decode_chain(last, end->budget, ids.data(), last_logits, nullptr, &req) != 0) return -1;
    for (int i = 0; i < n; i++) out_tokens[i] = i < end->budget ? ids[(size_t)i] : -1;
    if (rng) *rng = r;
    if (mu) *mu = u;
    *n_drawn = count;
    *ended_by = why;
    return 0;
}
int ggml_hip_decode_batch_requests(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, const ggml_hip_sampler_chain *const *chains,
                                   const ggml_hip_chain_end *ends, const int32_t *windows, const int32_t *window_n, uint64_t *rng, float *mu,
                                   int32_t *out_ids, int32_t *n_evaluated, int32_t *ended_by) {
    if (!graphs || n_graphs < 2 || n_graphs > BATCH_COLS_MAX || n_steps < 1 || n_steps > BATCH_CHAIN_MAX_STEPS) return -1;  // (before any device is touched)
    if (!chains || !ends || !n_evaluated || !ended_by || (n_steps > 1 && !out_ids)) return -1;
    for (int i = 0; i < n_graphs; i++) {
        if (!graphs[i] || (chains[i] && (!windows || !window_n || !rng))) return -1;
        if (ends[i].budget < 1 || ends[i].budget > n_steps || ends[i].n_stop < 0 || ends[i].n_stop > CHAIN_STOP_MAX) return -1;
    }
    SlotLock lk;
    const uint64_t t0 = now_ns();
    std::vector<uint64_t> r((size_t)n_graphs, 0);  // (copies: nothing moves unless the chain ran)
    std::vector<float> u((size_t)n_graphs, 0.0f);
    std::vector<int32_t> count((size_t)n_graphs), why((size_t)n_graphs);
    for (int i = 0; i < n_graphs; i++) {
        if (rng) r[(size_t)i] = rng[i];
        if (mu) u[(size_t)i] = mu[i];
    }
    ChainRequests req = {chains, ends, windows, window_n, r.data(), mu ? u.data() : nullptr, count.data(), why.data(), 1, {0, 0, 0, 0}};
    const int rc = decode_batch_steps(graphs, n_graphs, n_steps, out_ids, true, nullptr, &req);
    g.ns_compute += now_ns() - t0;
    if (rc != 0) return -1;
    for (int i = 0; i < n_graphs; i++) {
        if (rng && chains[i]) rng[i] = r[(size_t)i];
        if (mu && chains[i]) mu[i] = u[(size_t)i];
        n_evaluated[i] = count[(size_t)i];
        ended_by[i] = why[(size_t)i];
    }
    return 0;
}

// ---- the request pool: more requests than columns (plan_pool.inc) ----
int ggml_hip_decode_pool_requests(struct ggml_cgraph *const *graphs, int n_pool, int n_cols, int n_steps, const ggml_hip_sampler_chain *const *chains,
                                  const ggml_hip_chain_end *ends, const int32_t *windows, const int32_t *window_n, uint64_t *rng, float *mu,
                                  int32_t *out_ids, int32_t *col, int32_t *first_step, int32_t *n_evaluated, int32_t *ended_by, int32_t *steps_run) {
    if (!graphs || n_cols < 2 || n_cols > BATCH_COLS_MAX || n_pool < n_cols || n_pool > POOL_REQUESTS_MAX) return -1;  // (before any device is touched)
    if (n_steps < 1 || n_steps > BATCH_CHAIN_MAX_STEPS) return -1;
    if (!chains || !ends || !col || !first_step || !n_evaluated || !ended_by || !steps_run || (n_steps > 1 && !out_ids)) return -1;
    for (int i = 0; i < n_pool; i++) {
        if (!graphs[i] || (chains[i] && (!windows || !window_n || !rng))) return -1;
        if (ends[i].budget < 1 || ends[i].budget > n_steps || ends[i].n_stop < 0 || ends[i].n_stop > CHAIN_STOP_MAX) return -1;
    }
    SlotLock lk;
    const uint64_t t0 = now_ns();
    std::vector<uint64_t> r((size_t)n_pool, 0);  // (copies: nothing moves unless the pool ran)
    std::vector<float> u((size_t)n_pool, 0.0f);
    std::vector<int32_t> c((size_t)n_pool), f((size_t)n_pool), count((size_t)n_pool), why((size_t)n_pool);
    for (int i = 0; i < n_pool; i++) {
        if (rng) r[(size_t)i] = rng[i];
        if (mu) u[(size_t)i] = mu[i];
    }
    int32_t steps = 0;
    ChainRequests req = {chains, ends, windows, window_n, r.data(), mu ? u.data() : nullptr, count.data(), why.data(), 1, {0, 0, 0, 0}};
    const PoolResults res = {c.data(), f.data(), count.data(), why.data(), &steps};
    const int rc = decode_pool_requests(graphs, n_pool, n_cols, n_steps, out_ids, req, res);
    g.ns_compute += now_ns() - t0;
    if (rc != 0) return -1;
    for (int i = 0; i < n_pool; i++) {
        if (rng && chains[i]) rng[i] = r[(size_t)i];
        if (mu && chains[i]) mu[i] = u[(size_t)i];
        col[i] = c[(size_t)i];
        first_step[i] = f[(size_t)i];
        n_evaluated[i] = count[(size_t)i];
        ended_by[i] = why[(size_t)i];
    }
    *steps_run = steps;
    return 0;
}

// ---- the packed prompt batch: the prompt rows of several sessions as one pass of the prompt plan (plan_pack.inc) ----
int ggml_hip_prompt_pack(struct ggml_cgraph *const *graphs, int n_graphs) {
    if (!graphs || n_graphs < 1 || n_graphs > PACK_SEGS_MAX) return -1;  // (before any device is touched)
    for (int i = 0; i < n_graphs; i++)
        if (!graphs[i]) return -1;
    SlotLock lk;
    const uint64_t t0 = now_ns();
    const int r = prompt_pack(graphs, n_graphs);
    g.ns_compute += now_ns() - t0;
    return r;
}

// ---- test hook: one launch of k_pool_admit on the caller's tables (tests/test_pool_requests_gpu.py) ----
void ggml_hip_debug_pool_admit_sizes(int64_t *sizes) {
    if (!sizes) return;
    sizes[0] = (int64_t)sizeof(PoolTable);
    sizes[1] = (int64_t)sizeof(SampleReqs);
    sizes[2] = (int64_t)sizeof(SampleCols);
    sizes[3] = (int64_t)sizeof(DecParams);
    sizes[4] = (int64_t)sizeof(BatchCols);
}
int ggml_hip_debug_pool_admit(void *table, void *reqs, void *scols, void *prm, void *bcols, const int64_t *sizes, int n_cols, int n_pool,
                              const float *logits, const float *emb, int V, int E, float *slot_logits, float *slot_emb) {
    if (!table || !reqs || !scols || !prm || !bcols || !sizes || !logits || !emb || !slot_logits || !slot_emb) return -1;
    if (n_cols < 2 || n_cols > BATCH_COLS_MAX || n_pool < n_cols || n_pool > POOL_REQUESTS_MAX || V < 1 || E < 1) return -1;
    int64_t own[5];
    ggml_hip_debug_pool_admit_sizes(own);
    for (int i = 0; i < 5; i++)
        if (sizes[i] != own[i]) return -1;
    {  // the kernel clamps and checks every index it reads; the hook refuses what a call would never stage all the same
        const PoolTable *t = (const PoolTable *)table;
        if (t->head.n_cols != n_cols || t->head.n_pool != n_pool || t->head.cursor < 0 || t->head.cursor > n_pool) return -1;
        for (int c = 0; c < n_cols; c++)
            if (t->head.owner[c] < -1 || t->head.owner[c] >= n_pool) return -1;
        for (int r = 0; r < n_pool; r++)
            if (t->in[r].cls < 0 || t->in[r].cls >= SAMPLE_CLASSES) return -1;
    }
    SlotLock lk;
    ensure_init();
    finish_pending();
    std::vector<char *> owned;
    char *dt = debug_buf(sizeof(PoolTable), table, owned);
    char *dr = debug_buf(sizeof(SampleReqs), reqs, owned);
    char *ds = debug_buf(sizeof(SampleCols), scols, owned);
    char *dp = debug_buf(sizeof(DecParams), prm, owned);
    char *db = debug_buf(sizeof(BatchCols), bcols, owned);
    const float *dl = (const float *)debug_buf((size_t)n_cols * V * 4, logits, owned);
    const float *de = (const float *)debug_buf((size_t)n_cols * E * 4, emb, owned);
    float *sl = (float *)debug_buf((size_t)n_pool * V * 4, slot_logits, owned);
    float *se = (float *)debug_buf((size_t)n_pool * E * 4, slot_emb, owned);
    launch_pool_admit(g.stream, dt, dr, ds, dp, db, dl, de, V, E, sl, se);
    HIP_CHECK(hipGetLastError());
    d2h_queue(table, dt, sizeof(PoolTable));
    d2h_queue(reqs, dr, sizeof(SampleReqs));
    d2h_queue(scols, ds, sizeof(SampleCols));
    d2h_queue(prm, dp, sizeof(DecParams));
    d2h_queue(bcols, db, sizeof(BatchCols));
    d2h_queue(slot_logits, (const char *)sl, (size_t)n_pool * V * 4);
    d2h_queue(slot_emb, (const char *)se, (size_t)n_pool * E * 4);
    d2h_finish();
    for (char *b : owned) HIP_CHECK(hipFree(b));
    return 0;
}

// ---- test hook: the kernels between two steps of the chains that stop, alone (tests/test_chain_requests_gpu.py).  debug_next_token's
// shape with a request per column; a budget here is the number of draws, 0 .. n_draws. ----
int ggml_hip_debug_next_token_req(const float *logits, int B, int V, const ggml_hip_sampler_chain *const *chains, const ggml_hip_chain_end *ends,
                                  int n_past_in, const int32_t *pos_in, const int32_t *tokens_in, int32_t *hist, int32_t *hist_n, uint64_t *rng,
                                  float *mu, int n_draws, int32_t *ids_out, int32_t *prm_out, int32_t *pos_out, int32_t *n_drawn,
                                  int32_t *ended_by) {
    const int T = pos_in ? BATCH_COLS_MAX : 1;
    if (!logits || B < 1 || B > T || V < 1 || !chains || !ends || !tokens_in || !hist || !hist_n || !rng || !ids_out || !prm_out ||
        (pos_in && !pos_out) || !n_drawn || !ended_by || n_draws < 1 || n_draws > BATCH_CHAIN_MAX_STEPS)
        return -1;
    int32_t wn[BATCH_COLS_MAX];
    for (int c = 0; c < B; c++) {
        if (hist_n[c] < 0) return -1;
        wn[c] = std::min(hist_n[c], SAMPLER_WINDOW);
    }
    std::vector<int32_t> count((size_t)B), why((size_t)B);
    ChainRequests req = {chains, ends, hist, wn, rng, mu, count.data(), why.data(), 0, {0, 0, 0, 0}};
    if (!chain_requests_ok(req, B, V, 0, n_draws)) return -1;
    SlotLock lk;
    ensure_init();
    finish_pending();
    DecParams hp;
    BatchCols hb;
    SampleCols hs;
    SampleReqs ht;
    memset(&hp, 0, sizeof(hp));
    memset(&hb, 0, sizeof(hb));
    memset(&hs, 0, sizeof(hs));
    for (int i = 0; i < 32; i++) hp.tokens[i] = tokens_in[i];
    hp.n_past = pos_in ? pos_in[0] : n_past_in;
    hp.token = tokens_in[0];
    for (int i = 0; pos_in && i < BATCH_COLS_MAX; i++) hb.pos[i] = pos_in[i];
    memcpy(hs.hist, hist, (size_t)T * SAMPLER_WINDOW * 4);
    memcpy(hs.hist_n, hist_n, (size_t)T * 4);
    chain_req_table(ht, req, B);
    for (int i = 0; i < T; i++) {  // (entries from B on make the round trip untouched)
        ht.back.state.rng[i] = rng[i];
        if (mu) ht.back.state.mu[i] = mu[i];
    }
    std::vector<char *> owned;
    const float *dl = (const float *)debug_buf((size_t)B * V * 4, logits, owned);
    DecParams *dp = (DecParams *)debug_buf(sizeof(hp), &hp, owned);
    BatchCols *db = pos_in ? (BatchCols *)debug_buf(sizeof(hb), &hb, owned) : nullptr;
    SampleCols *ds = (SampleCols *)debug_buf(sizeof(hs), &hs, owned);
    char *dt = debug_buf(sizeof(ht), &ht, owned);
    int *dids = (int *)debug_buf((size_t)n_draws * B * 4, nullptr, owned);
    for (int i = 0; i < n_draws; i++) launch_next_token_req(g.stream, req.n_class, dl, V, dp, db, ds, dt, dids + (size_t)i * B);
    HIP_CHECK(hipGetLastError());
    d2h_queue(ids_out, (const char *)dids, (size_t)n_draws * B * 4);
    d2h_queue(&hp, (const char *)dp, sizeof(hp));
    if (db) d2h_queue(&hb, (const char *)db, sizeof(hb));
    d2h_queue(&hs, (const char *)ds, sizeof(hs));
    d2h_queue(&ht.back, (const char *)dt, sizeof(ht.back));
    d2h_finish();
    prm_out[0] = hp.n_past;
    prm_out[1] = hp.token;
    for (int i = 0; i < 32; i++) prm_out[2 + i] = hp.tokens[i];
    for (int i = 0; pos_in && i < BATCH_COLS_MAX; i++) pos_out[i] = hb.pos[i];
    memcpy(hist, hs.hist, (size_t)T * SAMPLER_WINDOW * 4);
    memcpy(hist_n, hs.hist_n, (size_t)T * 4);
    for (int i = 0; i < T; i++) {
        rng[i] = ht.back.state.rng[i];
        if (mu) mu[i] = ht.back.state.mu[i];
    }
    for (int c = 0; c < B; c++) {
        n_drawn[c] = ht.back.n_drawn[c];
        ended_by[c] = ht.back.ended_by[c];
    }
    for (char *b : owned) HIP_CHECK(hipFree(b));
    return 0;
}

// ---- test hooks: the kernel between two steps of a chain, alone.  One body of the three hooks below. ----
// logits [B][V]; tokens_in[32] go to the device as DecParams::tokens (token = tokens_in[0]) at n_past, pos_in[8] as a step's
// BatchCols::pos (null: no BatchCols, one session at n_past).  Without params: k_argmax_next on B workgroups.  With params: the sampler,
// in the form a chain picks for V, on the caller's rings, counts and generator states — T entries each, in / out, T = 8 with a BatchCols
// and 1 without (mu likewise; may be null without Mirostat); a count beyond 64 is a full ring; entries from B on are not checked and
// make the round trip untouched.  n_draws
// launches on the same rows.  Out: ids_out[n_draws][B], prm_out[34] = n_past, token, tokens[0..32), pos_out[8] (with a BatchCols).
// 0, or -1 for arguments the hook or the chain cannot take.
static int debug_next_token(const float *logits, int B, int V, const ggml_hip_sampler_chain *params, int n_past, const int32_t *pos_in,
                            const int32_t *tokens_in, int32_t *hist, int32_t *hist_n, uint64_t *rng, float *mu, int n_draws,
                            int32_t *ids_out, int32_t *prm_out, int32_t *pos_out) {
    const int T = pos_in ? BATCH_COLS_MAX : 1;
    int stages = SAMPLE_DEFAULT;
    if (!logits || B < 1 || B > T || V < 1 || !tokens_in || !ids_out || !prm_out || (pos_in && !pos_out) || n_draws < 1 ||
        n_draws > BATCH_CHAIN_MAX_STEPS)
        return -1;
    if (params) {
        if (!hist || !hist_n || !rng) return -1;
        int32_t wn[BATCH_COLS_MAX];
        for (int c = 0; c < B; c++) {
            if (hist_n[c] < 0) return -1;
            wn[c] = std::min(hist_n[c], SAMPLER_WINDOW);
        }
        const BatchSample smp = {params, hist, wn, rng, mu};
        if (!batch_sample_ok(smp, B, V)) return -1;
        stages = smp.stages();
    }
    SlotLock lk;
    ensure_init();
    finish_pending();
    DecParams hp;
    BatchCols hb;
    SampleCols hs;
    SampleHead hh;
    SampleState &hst = hh.state;
    memset(&hp, 0, sizeof(hp));
    memset(&hb, 0, sizeof(hb));
    memset(&hs, 0, sizeof(hs));
    memset(&hh, 0, sizeof(hh));
    for (int i = 0; i < 32; i++) hp.tokens[i] = tokens_in[i];
    hp.n_past = n_past;
    hp.token = tokens_in[0];
    for (int i = 0; pos_in && i < BATCH_COLS_MAX; i++) hb.pos[i] = pos_in[i];
    if (params) {
        memcpy(hs.hist, hist, (size_t)T * SAMPLER_WINDOW * 4);
        memcpy(hs.hist_n, hist_n, (size_t)T * 4);
        sample_cols_params(hs, *params);
        sample_head_bias(hh, *params);
        for (int i = 0; i < T; i++) {
            hst.rng[i] = rng[i];
            if (mu) hst.mu[i] = mu[i];
        }
    }
    std::vector<char *> owned;
    const float *dl = (const float *)debug_buf((size_t)B * V * 4, logits, owned);
    DecParams *dp = (DecParams *)debug_buf(sizeof(hp), &hp, owned);
    BatchCols *db = pos_in ? (BatchCols *)debug_buf(sizeof(hb), &hb, owned) : nullptr;
    SampleCols *ds = (SampleCols *)debug_buf(sizeof(hs), &hs, owned);
    unsigned long long *dr = (unsigned long long *)(debug_buf(sizeof(hh), &hh, owned) + sizeof(SampleBias));
    int *dids = (int *)debug_buf((size_t)n_draws * B * 4, nullptr, owned);
    for (int i = 0; i < n_draws; i++) {
        if (params) launch_sample_next(g.stream, B, dl, V, dp, db, ds, dr, dids + (size_t)i * B, stages);
        else hipLaunchKernelGGL(k_argmax_next, dim3((unsigned)B), dim3(1024), 0, g.stream, dl, V, dp, db, dids + (size_t)i * B);
    }
    HIP_CHECK(hipGetLastError());
    d2h_queue(ids_out, (const char *)dids, (size_t)n_draws * B * 4);
    d2h_queue(&hp, (const char *)dp, sizeof(hp));
    if (db) d2h_queue(&hb, (const char *)db, sizeof(hb));
    if (params) {
        d2h_queue(&hs, (const char *)ds, sizeof(hs));
        d2h_queue(&hst, (const char *)dr, sizeof(hst));
    }
    d2h_finish();
    prm_out[0] = hp.n_past;
    prm_out[1] = hp.token;
    for (int i = 0; i < 32; i++) prm_out[2 + i] = hp.tokens[i];
    for (int i = 0; pos_in && i < BATCH_COLS_MAX; i++) pos_out[i] = hb.pos[i];
    if (params) {
        memcpy(hist, hs.hist, (size_t)T * SAMPLER_WINDOW * 4);
        memcpy(hist_n, hs.hist_n, (size_t)T * 4);
        for (int i = 0; i < T; i++) {
            rng[i] = hst.rng[i];
            if (mu) mu[i] = hst.mu[i];
        }
    }
    for (char *b : owned) HIP_CHECK(hipFree(b));
    return 0;
}
// k_argmax_next with a BatchCols, once (tests/test_batch_chain_gpu.py): n_past = pos_in[0]
int ggml_hip_debug_batch_tail(const float *logits, int B, int V, const int32_t *pos_in, const int32_t *tokens_in, int32_t *ids_out,
                              int32_t *prm_out, int32_t *pos_out) {
    if (!pos_in) return -1;
    return debug_next_token(logits, B, V, nullptr, pos_in[0], pos_in, tokens_in, nullptr, nullptr, nullptr, nullptr, 1, ids_out, prm_out, pos_out);
}
// k_sample_next with a BatchCols (tests/test_batch_sample_gpu.py): hist [8][64], hist_n[8], rng[8]
int ggml_hip_debug_batch_sample(const float *logits, int B, int V, const ggml_hip_sampler *params, const int32_t *pos_in,
                                const int32_t *tokens_in, int32_t *hist, int32_t *hist_n, uint64_t *rng, int n_draws, int32_t *ids_out,
                                int32_t *prm_out, int32_t *pos_out) {
    if (!params || !pos_in) return -1;
    const ggml_hip_sampler_chain chain = sample_neutral(params);
    return debug_next_token(logits, B, V, &chain, pos_in[0], pos_in, tokens_in, hist, hist_n, rng, nullptr, n_draws, ids_out, prm_out, pos_out);
}
// k_sample_next for one session at n_past_in (tests/test_sample_chain_gpu.py): one row, hist[64], *hist_n, *rng
int ggml_hip_debug_sample_next(const float *logits, int V, const ggml_hip_sampler *params, int n_past_in, const int32_t *tokens_in,
                               int32_t *hist, int32_t *hist_n, uint64_t *rng, int n_draws, int32_t *ids_out, int32_t *prm_out) {
    if (!params) return -1;
    const ggml_hip_sampler_chain chain = sample_neutral(params);
    return debug_next_token(logits, 1, V, &chain, n_past_in, nullptr, tokens_in, hist, hist_n, rng, nullptr, n_draws, ids_out, prm_out, nullptr);
}
// ... and both with the whole sampler: pos_in null = one session at n_past_in, else the batched form at pos_in[0]
int ggml_hip_debug_next_token_ex(const float *logits, int B, int V, const ggml_hip_sampler_chain *chain, int n_past_in, const int32_t *pos_in,
                                 const int32_t *tokens_in, int32_t *hist, int32_t *hist_n, uint64_t *rng, float *mu, int n_draws,
                                 int32_t *ids_out, int32_t *prm_out, int32_t *pos_out) {
    if (!chain) return -1;
    return debug_next_token(logits, B, V, chain, pos_in ? pos_in[0] : n_past_in, pos_in, tokens_in, hist, hist_n, rng, mu, n_draws, ids_out,
                            prm_out, pos_out);
}

int64_t ggml_hip_get_stat(const char *key) {
    SlotLock lk;
    for (const StatRow &c : g_counters)  // the plain counters (backend_state.inc); the rest is computed here
        if (!strcmp(c.key, key)) return (int64_t)(g.*c.field);
    const std::string k(key);
    if (k == "w16_bytes") return (int64_t)g.w16_bytes;  // HBM held by resident f16 weight copies
    if (k.rfind("mmq_launches_", 0) == 0) {                 // prompt-GEMM launches by kernel since library load
        static const char *names[Backend::MMQ_K_COUNT] = {"plain", "dma_p8", "w16_p8", "w16_256", "i8"};
        for (int i = 0; i < Backend::MMQ_K_COUNT; i++)
            if (k.substr(13) == names[i]) return (int64_t)g.stat_mmq[i];
        return -1;
    }
    if (k == "graph_replays") {
        int64_t n = 0;
        for (auto *p : g_plans) n += (int64_t)p->replays;
        return n;
    }
    if (k == "plans") return (int64_t)g_plans.size();
    if (k == "num_cus") {  // workgroups of a full-chip mat-vec launch (k_mmvq_big, k_mmvq_kbig)
        ensure_init();
        return (int64_t)g.num_cus;
    }
    if (k == "fused_attn_timeouts") {  // attention workgroups of k_qkv_attn that gave up waiting (must stay 0)
        int64_t n = (int64_t)g.stat_fused_timeouts;  // tokens the host saw the error word for (re-run or fatal) + a word still set
        if (g.inited) HIP_CHECK(hipStreamSynchronize(g.stream));
        if (g.ferr_pin) n += *(volatile unsigned *)g.ferr_pin;
        return n;
    }
    if (k == "peak_concurrent_calls") return (int64_t)g_calls_inside_peak.load();  // threads that were inside entry points (on different slots) at once
    return -1;
}
size_t ggml_hip_read_timeline(int64_t *dst, size_t max_records) {
    SlotLock lk;
    if (!g.timeline) return 0;
    const size_t n = std::min(max_records, g.timeline_bytes / 64);
    HIP_CHECK(hipStreamSynchronize(g.stream));
    HIP_CHECK(hipMemcpy(dst, g.timeline, n * 64, hipMemcpyDeviceToHost));
    return n;
}
const char *ggml_hip_version(void) { return "libggml_hip 0.1 (gfx950)"; }

}  // extern "C"
