// plan_decode.inc — the single-token launch sequences of a DecodePlan: plan_launch_all (block formats), plan_launch_k
// (K-quants, which also takes chunks of up to 31 tokens), plan_launch_f16 (F16 weights: decode, chunks and batched steps) and plan_launch_mpt (an MPT graph,
// block formats), and the launchers they share with plan_prompt.inc and the test hooks.
// per-class launch/byte accounting of one token (filled by the launch sequences when given)
struct PlanStats {
    double bytes[GGML_HIP_KCLASS_COUNT] = {0, 0, 0, 0};
    int64_t launches[GGML_HIP_KCLASS_COUNT] = {0, 0, 0, 0};
};
// What a launch sequence is asked to enqueue, and its books.  `mask` selects kernel classes (bit k = GGML_HIP_KCLASS k) and
// `kind_mask` mat-vec kinds (bit k = GGML_HIP_KKIND k: 0 wq|wk|wv, 1 wo, 2 w1|w3, 3 w2, 4 lm_head): the roofline leg replays one
// class or kind alone to time it without event overhead.  `st`, when given, takes the launches and algorithmic bytes per class.
// The last two are what the capture of a greedy token's graph chooses (plan_run.inc launch_tail); every other launch of a plan — an
// evaluation's plain graph, the re-run, the chain, a roofline leg — keeps their defaults.
struct LaunchCtx {
    unsigned mask = ~0u, kind_mask = ~0u;
    PlanStats *st = nullptr;
    int ts_idx = 0;  // timeline: one timeline_wgs x 8 x int64 record per big launch, in launch order
    int out_set = 0;        // the result set the final norm / lm_head aim at (DecodePlan::res_logits): 1 only in a graph of parity 1
    bool prepared = false;  // a TAIL_AHEAD graph of the block-format plan (tail_prepares: no other plan is asked for it): plan_launch_all
                            // opens with neither get_rows nor k_rope_table, layer 0 reads xnext
    bool want(int k, double bytes) {
        if (!(mask & (1u << k))) return false;
        if (st) {
            st->bytes[k] += bytes;
            st->launches[k]++;
        }
        return true;
    }
    long long *next_ts() {
        if (!g.timeline) return nullptr;
        if ((size_t)(ts_idx + 1) * g.timeline_wgs * 8 * 8 > g.timeline_bytes) return nullptr;
        return g.timeline + (size_t)(ts_idx++) * g.timeline_wgs * 8;
    }
    template <class F>
    void mmvq(int kind, double bytes, F &&launch) {  // one mat-vec launch of `kind`
        if (!(kind_mask & (1u << kind)) || !want(GGML_HIP_KCLASS_MMVQ, bytes)) return;
        Timed tm(GGML_HIP_KCLASS_MMVQ, bytes);
        launch();
        HIP_CHECK(hipGetLastError());
    }
    template <class F>
    void other(double bytes, F &&launch) {  // one launch of the "everything else" class
        if (!want(GGML_HIP_KCLASS_OTHER, bytes)) return;
        Timed tm(GGML_HIP_KCLASS_OTHER, bytes);
        launch();
        HIP_CHECK(hipGetLastError());
    }
};
template <int QT, int EPI, int XSRC>
static void launch_dec(const DecMmvqArgs &a, int nwg) {
    hipLaunchKernelGGL((k_mmvq_dec<QT, EPI, XSRC>), dim3(nwg), dim3(256), (size_t)a.nb * 40, g.stream, a);
}
template <int QT, int EPI, int XSRC>
static void launch_big(const BigArgs &a) {
    const int64_t Mtot = a.M[0] + (EPI == EPI_QKV ? a.M[1] + a.M[2] : 0);
    const int64_t units = Mtot / (EPI == EPI_QKV ? 2 : 1);
    const BigShape sh = big_shape(XSRC, EPI, a.nb, units);
    if (!sh.ok) {
        fprintf(stderr, "ggml-hip: k_mmvq_big: %lld units over %d x %d waves exceed 64 per wave\n", (long long)units, sh.G, sh.W);
        abort();
    }
    // the norm is staged by all 16 waves (BigX<XSRC_NORM>): such a launch always has 1024 threads, W of its waves take units
    BigArgs b = a;
    int threads = sh.W * 64;
    if (XSRC == XSRC_NORM) {
        threads = BigX<XSRC_NORM>::NT;
        b.wdeal = sh.W;
    }
    b.T = threads;  // the kernel reads neither blockDim nor gridDim (BigArgs: the entry block)
    b.G = sh.G;
    with_bool(a.probe || a.ts, [&](auto INSTR) {  // true: measurement build (tests/tools/launch_probe.py, timeline.py)
        hipLaunchKernelGGL((k_mmvq_big<QT, EPI, XSRC, CT(INSTR)>), dim3(sh.G), dim3(threads), sh.lds, g.stream, b);
    });
}
// the mat-vec workgroups' view of a fused launch of sh.G workgroups: the attention workgroups in front (n_head x S), themselves behind
static BigArgs fused_big_args(const BigArgs &a, const FusedAttnArgs &fa, const FusedShape &sh) {
    BigArgs b = a;
    b.T = 1024;
    b.n_attn = fa.n_head * (fa.S > 1 ? fa.S : 1);
    b.G = sh.G - b.n_attn;
    return b;
}
template <int QT>
static void launch_qkv_attn(const BigArgs &a, const FusedAttnArgs &fa, const FusedShape &sh, size_t lds) {
    const BigArgs ba = fused_big_args(a, fa, sh);
    with_bool(ba.probe || ba.ts, [&](auto INSTR) {
        lds_opt_in<k_qkv_attn<QT, CT(INSTR)>>(lds, ATTN_DECODE_LDS_MAX);  // (a context whose score rows exceed the default)
        hipLaunchKernelGGL((k_qkv_attn<QT, CT(INSTR)>), dim3(sh.G), dim3(1024), lds, g.stream, ba, fa);
    });
}
template <int QT>
static void launch_qkv_attn_wo(const BigArgs &a, const FusedAttnArgs &fa, const WoTailArgs &wt, const FusedShape &sh, size_t lds) {
    const BigArgs ba = fused_big_args(a, fa, sh);
    const bool two = (wt.w.nb + 63) / 64 <= 2;  // blocks of a row per lane: 2 steps up to 4096-wide rows, else up to 4
    with_bool(two, [&](auto TWO) {
        constexpr int STEPS = CT(TWO) ? 2 : 4;
        lds_opt_in<k_qkv_attn_wo<QT, STEPS>>(lds, ATTN_DECODE_LDS_MAX);
        hipLaunchKernelGGL((k_qkv_attn_wo<QT, STEPS>), dim3(sh.G), dim3(1024), lds, g.stream, ba, fa, wt);
    });
}
// THE launch of k_attn_decode, for all three plans that have one: a grid of heads x N queries (query n attends to positions
// <= n_past + n) of layer il, `rows` positions in its LDS arrays.  f16d / out_f32: the re-quantized row for wo as Q8 with an
// f16-rounded scale or not (p->e_*), and (K plan) the f32 row as well; dT / sT: the chunk plan's transposed scale tables.
static void launch_attn_decode(const DecodePlan *p, int il, int N, int64_t rows, bool f16d, float *out_f32, long long *ts,
                               float *dT = nullptr, int *sT = nullptr) {
    const LlamaMatch &m = p->m;
    with_bool(f16d, [&](auto F16D) {
        lds_opt_in<k_attn_decode<CT(F16D)>>(attn_decode_lds(rows, m.D), ATTN_DECODE_LDS_MAX);
        hipLaunchKernelGGL(k_attn_decode<CT(F16D)>, dim3((unsigned)m.H, (unsigned)N), dim3(1024), attn_decode_lds(rows, m.D), g.stream,
                           (const float *)p->q, (const __half *)p->mem_k_at(il), (const __half *)p->mem_v_at(il), (const DecParams *)p->prm,
                           m.kq_scale, (int)m.D, (int)(m.H / m.Hkv), m.Egqa, m.C, out_f32, p->e_lo, p->e_hi, p->e_d, p->e_s, ts, (int)m.H,
                           rows, dT, sT);
    });
    HIP_CHECK(hipGetLastError());
}
// the attention workgroups' arguments of a fused wq|wk|wv + attention launch of layer il (k_qkv_attn, k_qkv_attn_wo, k_qkv_attn_k):
// S workgroups per head, Clds positions in their LDS arrays
static FusedAttnArgs fused_attn_args(const DecodePlan *p, int il, int S, int64_t Clds) {
    const LlamaMatch &m = p->m;
    FusedAttnArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.mem_k = p->mem_k_at(il); fa.mem_v = p->mem_v_at(il); fa.prm = p->prm; fa.epoch = p->epoch; fa.gran = p->gran_at(il);
    fa.k_pair0 = (int)(m.E / 2); fa.v_pair0 = (int)((m.E + m.Egqa) / 2);
    fa.scale = m.kq_scale; fa.D = (int)m.D; fa.n_rep = (int)(m.H / m.Hkv); fa.n_head = (int)m.H;
    fa.Egqa = m.Egqa; fa.C = m.C; fa.Clds = Clds;
    fa.err = p->ferr; fa.S = S; fa.layer = il;
    return fa;
}
// the position-split attention of layer il as one launch (k_attn_split_one, kernels/decode_attn_split.h): every CU pulls a piece
// of the cache.  `a` alone serves the three-launch form, given its scratch (sc, pmax, part).
static AttnSplitOneArgs split_attn_args(const DecodePlan *p, int il) {
    const LlamaMatch &m = p->m;
    AttnSplitOneArgs oa;
    memset(&oa, 0, sizeof(oa));
    AttnSplitArgs &sa = oa.a;
    sa.q = p->q; sa.mem_k = p->mem_k_at(il); sa.mem_v = p->mem_v_at(il); sa.prm = p->prm; sa.scale = m.kq_scale; sa.D = (int)m.D;
    sa.n_rep = (int)(m.H / m.Hkv); sa.n_head = (int)m.H; sa.S = p->att_S; sa.Egqa = m.Egqa; sa.C = m.C;
    sa.lo = p->e_lo; sa.hi = p->e_hi; sa.dq = p->e_d; sa.sumq = p->e_s;
    oa.mx_g = p->att_mxg_at(il); oa.sum_g = p->att_sumg_at(il); oa.part_g = p->att_partg_at(il); oa.cnt = p->att_cnt; oa.epoch = p->epoch; oa.layer = il;
    oa.err = p->ferr;
    return oa;
}
static void launch_attn_split_one(const DecodePlan *p, const AttnSplitOneArgs &oa, bool f16d) {
    const dim3 grid((unsigned)p->m.H, (unsigned)oa.a.S);
    with_bool(f16d, [&](auto F16D) {
        hipLaunchKernelGGL(k_attn_split_one<CT(F16D)>, grid, dim3(1024), attn_split_chunk_max(p->m.C, oa.a.S) * 6, g.stream, oa);
    });
}
// the planar arrays of a block-format weight with nb blocks per row, and the bytes of a row in each: f(base, row_bytes)
// (arrays a type does not have alias the next one (qw_at): by type)
template <class F>
static void for_each_weight_array(int qt, const QWeight &q, int64_t nb, F &&f) {
    f((const void *)q.qs, (size_t)nb * 16);
    if (qt == QT_Q8_0) f((const void *)q.qs2, (size_t)nb * 16);
    if (qt == QT_Q5_0 || qt == QT_Q5_1) f((const void *)q.qh, (size_t)nb * 4);
    f((const void *)q.d, (size_t)nb * 2);
    if (qt == QT_Q4_1 || qt == QT_Q5_1) f((const void *)q.m, (size_t)nb * 2);
}
// matrices that share an activation row go out as one launch per run of equal K types (a *_K_M file mixes Q4_K and Q6_K):
// f(i, j) for every run ws[i .. j)
template <class F>
static void for_each_type_run(const KWeight *const *ws, int n, F &&f) {
    for (int i = 0; i < n;) {
        int j = i + 1;
        while (j < n && ws[j]->kt == ws[i]->kt) j++;
        f(i, j);
        i = j;
    }
}
// where a plan's final norm and lm_head write: result set 0, or set 1 in a greedy token's graph of parity 1 (LaunchCtx::out_set)
struct ResultDst {
    float *emb;
    char *logits;
};
static ResultDst plan_result_dst(const DecodePlan *p, const LaunchCtx &cx) { return ResultDst{p->res_emb(cx.out_set), p->res_logits(cx.out_set)}; }
static void plan_lm_head_k(DecodePlan *p, LaunchCtx &cx, const ResultDst &dst);  // (behind launch_kbig below)
// ---- what the K plan and the F16 plan share: everything around their mat-vecs ----
// The opening: the residual rows from the hand-off buffer, or the embedding rows of the N token ids (`embed`: the plan's own get_rows
// launch, embed_bytes per element its books); then one (cos, sin) table per column, 128 floats apart (batch: each at its own session's position)
template <class F>
static void plan_open_rows(DecodePlan *p, LaunchCtx &cx, bool batch, double embed_bytes, F &&embed) {
    const LlamaMatch &m = p->m;
    const int N = m.N;
    const float theta_scale = powf(m.freq_base, -2.0f / m.n_dims);
    if (!m.wte) {
        if (cx.want(GGML_HIP_KCLASS_OTHER, (double)N * m.E * 8.0))
            HIP_CHECK(hipMemcpyAsync(p->xa, p->stage_in, (size_t)N * m.E * 4, hipMemcpyDeviceToDevice, g.stream));
    } else {  // DecParams::tokens[0] == token: the ids of the chunk / of the step's columns
        cx.other((double)N * m.E * embed_bytes, embed);
    }
    cx.other((double)N * m.D * 4.0, [&] {
        if (batch)
            hipLaunchKernelGGL(k_rope_table_batch, dim3((unsigned)N), dim3(128), 0, g.stream, (const BatchCols *)p->bcols, theta_scale, m.freq_scale,
                               (int)(m.D >> 1), p->rope);
        else
            hipLaunchKernelGGL(k_rope_table, dim3((unsigned)N), dim3(128), 0, g.stream, (const DecParams *)p->prm, theta_scale, m.freq_scale,
                               (int)(m.D >> 1), p->rope, p->epoch);  // block 0 also opens the token's epoch (the tag of k_attn_split_one's granules)
    });
}
// The attention of layer il: the f32 row of the merged heads in p->k_att for wo's staging (the Q8_0 copy of the heads' outputs goes to
// the plan's unused E-wide Q8_0 row).  long_ctx: every CU pulls a piece of the cache (k_attn_split_one, kernels/decode_attn_split.h)
static void launch_attn_decode_batch(const DecodePlan *p, int il, int N, bool f16d, float *out_f32);
static void plan_attn_f32(DecodePlan *p, LaunchCtx &cx, int il, bool long_ctx, bool batch) {
    const LlamaMatch &m = p->m;
    const int N = m.N;
    const double bytes = (double)N * ((double)(m.n_past + N) * m.Egqa * 4.0 + m.E * 9.0);
    if (!cx.want(GGML_HIP_KCLASS_ATTN, bytes)) return;
    Timed tm(GGML_HIP_KCLASS_ATTN, bytes);
    if (batch)
        launch_attn_decode_batch(p, il, N, true, p->k_att);
    else if (long_ctx) {
        AttnSplitOneArgs oa = split_attn_args(p, il);
        oa.out_f32 = p->k_att;
        launch_attn_split_one(p, oa, true);
    } else
        launch_attn_decode(p, il, N, m.C, true, p->k_att, nullptr);
    HIP_CHECK(hipGetLastError());
}
// The tail of a stage that is not the last of a layer split: its residual rows into the outgoing hand-off buffer (true: no lm_head follows)
static bool plan_hand_on(DecodePlan *p, LaunchCtx &cx) {
    const LlamaMatch &m = p->m;
    if (m.output) return false;
    if (cx.want(GGML_HIP_KCLASS_OTHER, (double)m.N * m.E * 8.0))
        HIP_CHECK(hipMemcpyAsync(p->stage_out, p->xa, (size_t)m.N * m.E * 4, hipMemcpyDeviceToDevice, g.stream));
    return true;
}

// enqueues the whole token on g.stream (eagerly, or into a stream capture); cx: what of it, and the books (LaunchCtx).
// g.opt_big : 1 (default) = k_mmvq_big, norm / re-quantization fused into its staging (3 launches per layer with the fused
//             wq|wk|wv + attention + wo launch, 5 without it);
//             0 = k_mmvq_dec behind separate k_rmsnorm_quant / k_quant_row launches (8 per layer; kept for the tests).
static void plan_launch_all(DecodePlan *p, int av, LaunchCtx cx) {
    const bool long_ctx = av == AV_SPLIT;
    const LlamaMatch &m = p->m;
    const int qt = qt_of(m.wtype);
    const bool f16d = qt_f16d(qt);
    const bool big = g.opt_big != 0;            // one-wave-of-big-workgroups mat-vec (kernels/decode_big.h)
    const bool fuse_x = big;  // norm / re-quantization fused into the mat-vec's staging
    const int64_t E = m.E, F = m.F, nbE = E / 32, nbF = F / 32;
    const QAct actE{(const i32x4 *)p->e_lo, (const i32x4 *)p->e_hi, p->e_d, p->e_s};
    const QAct actF{(const i32x4 *)p->f_lo, (const i32x4 *)p->f_hi, p->f_d, p->f_s};
    const float theta_scale = powf(m.freq_base, -2.0f / m.n_dims);
    const double bb = (double)blk_bytes(qt);
    // rms_norm + weight + Q8 of the E-wide residual row (separate launch)
    auto rmsq = [&](const float *x, const float *w, float *y) {
        cx.other((double)E * 9.25, [&] {
            launch_rmsnorm_quant(f16d, x, w, m.eps, E, 1, y, p->e_lo, p->e_hi, p->e_d, p->e_s, nullptr, nullptr, nullptr);
        });
    };
    // one mat-vec launch: k_mmvq_big with the staging XSRC, or (option big = 0) k_mmvq_dec on nwg workgroups — behind the separate
    // norm / quantization launches (XSRC_Q8), its own fused staging XDEC being compiled but tied to `big` like everything fused
    auto matvec = [&](int kind, auto EPI, auto XSRC, auto XDEC, const DecMmvqArgs &a, float *y_out, const float *rope, int nwg, double bytes) {
        cx.mmvq(kind, bytes, [&] {
            with_qt(qt, [&](auto QT) {
                if (big)
                    launch_big<CT(QT), CT(EPI), CT(XSRC)>(big_pack(a, y_out, cx.next_ts(), g.timeline_wgs, rope, g.opt_probe, nullptr, nullptr, 0, p->hot));
                else
                    fuse_x ? launch_dec<CT(QT), CT(EPI), CT(XDEC)>(a, nwg) : launch_dec<CT(QT), CT(EPI), XSRC_Q8>(a, nwg);
            });
        });
    };
    constexpr std::integral_constant<int, EPI_QKV> epi_qkv{};
    constexpr std::integral_constant<int, EPI_ADD> epi_add{};
    constexpr std::integral_constant<int, EPI_GATE> epi_gate{};
    constexpr std::integral_constant<int, EPI_STORE> epi_store{};
    constexpr std::integral_constant<int, XSRC_NORM> x_norm{};
    constexpr std::integral_constant<int, XSRC_Q8> x_q8{};
    constexpr std::integral_constant<int, XSRC_F32> x_f32{};
    // A stage of a layer split: its first layer reads the residual straight from the hand-off buffer (xin below) and its last layer's
    // w2 launch writes straight into the outgoing one — no copy node at either end of the stage (each was a copy-engine start + a
    // boundary on the token's path: ~5 us per stage boundary and side)
    // A greedy token's graph launched directly behind another one (TAIL_AHEAD, plan_run.inc) opens with neither launch below: that
    // graph's k_token_tail has left this token's row in p->xnext, its table in p->rope and its epoch open
    const bool prepared = cx.prepared;
    if (m.wte && !prepared)  // token embedding: get_rows(wte, embd)
        cx.other((double)E * 4.6, [&] {
            hipLaunchKernelGGL(k_get_rows_q, dim3((unsigned)((nbE + 255) / 256), 1), dim3(256), 0, g.stream, p->wte,
                               (const int *)&p->prm->token, p->xa, E);
        });
    // wq|wk|wv + attention as one launch (kernels/decode_fused.h) below the split-attention threshold
    const FusedShape fsh = long_ctx ? FusedShape{} : fused_qkv_shape(m, av_heads_split(av));
    // this position's RoPE table, shared by all layers; it also opens the token's granule epoch, so a replay of the mat-vec
    // class alone (roofline leg) takes it along when the fused launch is part of that class — the hand-off wait is then
    // inside the measured time, not skipped on stale-but-equal tags
    const bool rope_for_fused = fsh.ok && (cx.mask & (1u << GGML_HIP_KCLASS_MMVQ)) && (cx.kind_mask & 1u) && !(cx.mask & (1u << GGML_HIP_KCLASS_OTHER));
    if (big && !prepared && (cx.want(GGML_HIP_KCLASS_OTHER, (double)m.D * 4.0) || rope_for_fused)) {
        hipLaunchKernelGGL(k_rope_table, dim3(1), dim3(128), 0, g.stream, (const DecParams *)p->prm, theta_scale,
                           m.freq_scale, (int)(m.D >> 1), p->rope, p->epoch);
        HIP_CHECK(hipGetLastError());
    }
    // experiment hook (GGML_HIP_BENCH_SAME_LAYER=1, roofline replays only): every iteration uses layer 0's weights, so
    // a 50 MB matrix is re-read from the 256 MB Infinity Cache instead of HBM — measures what a MALL hit is worth
    static const bool same_layer = getenv("GGML_HIP_BENCH_SAME_LAYER") && atoi(getenv("GGML_HIP_BENCH_SAME_LAYER"));
    // the WO form needs the wo launch's kind in the replay too (a roofline replay of kind 0 alone would wait for nothing: fine —
    // and one of kind 1 alone has no wo launch to time: the kind reports 0 launches)
    const bool fuse_wo = fsh.ok && fsh.wo && p->ogran != nullptr;
    const double wo_bytes = (double)E * nbE * bb + nbE * 40.0 + E * 8.0;
    for (int il = 0; il < m.L; il++) {
        const int wl = (same_layer && cx.kind_mask != ~0u) ? 0 : il;
        const DecodePlan::LW &w = p->lw[wl];
        const DecodePlan::LayerNorms &ln = p->ln[wl];
        // ---- attention norm + wq|wk|wv + rope + KV store ----
        float *const xin = il != 0 ? p->xa : !m.wte ? p->stage_in : prepared ? p->xnext : p->xa;  // the layer's input row (residual stream)
        float *const xout = (il == m.L - 1 && !m.output) ? p->stage_out : p->xa;        // ... and where its w2 + residual goes
        if (!fuse_x) rmsq(xin, ln.attn_norm, nullptr);
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.wq; a.w[1] = w.wk; a.w[2] = w.wv;
            a.wg_begin[0] = 0;
            a.wg_begin[1] = (int)((E + 7) / 8);
            a.wg_begin[2] = a.wg_begin[1] + (int)((m.Egqa + 7) / 8);
            const int nwg = a.wg_begin[2] + (int)((m.Egqa + 7) / 8);
            a.x = actE; a.xf = xin; a.xw = ln.attn_norm; a.eps = m.eps;
            a.nb = nbE; a.dst = p->q; a.prm = p->prm; a.mem_k = p->mem_k_at(il); a.mem_v = p->mem_v_at(il);
            a.Egqa = m.Egqa; a.C = m.C; a.D = (int)m.D; a.theta_scale = theta_scale; a.freq_scale = m.freq_scale;
            const double qkv_bytes = (double)(E + 2 * m.Egqa) * nbE * bb + nbE * 40.0 + (E + 2 * m.Egqa) * 4.0;
            if (fsh.ok) {  // the attention workgroups ride in the same launch; no k_attn_decode below
                const double att_bytes = (double)(m.n_past + 1) * m.Egqa * 4.0 + m.E * 9.0;
                cx.mmvq(0, qkv_bytes + att_bytes + (fuse_wo ? wo_bytes : 0.0), [&] {
                    BigArgs ba = big_pack(a, nullptr, cx.next_ts(), g.timeline_wgs, p->rope, g.opt_probe, p->gran_at(il), p->epoch, fsh.W, p->hot);
                    FusedAttnArgs fa = fused_attn_args(p, il, fsh.S, attn_decode_rows(m.C, 1, m.H));
                    if (fsh.affine) {
                        ba.aff_hpl = (int)(m.H / 8);
                        ba.aff_shift = m.D == 128 ? 6 : m.D == 64 ? 5 : 4;
                        fa.local_rows = 1;
                    }
                    fa.lo = p->e_lo; fa.hi = p->e_hi; fa.dq = p->e_d; fa.sumq = p->e_s;
                    fa.ts = cx.next_ts(); fa.ts_heads = g.timeline_wgs;
                    fa.mx_g = p->att_mxg_at(il); fa.sum_g = p->att_sumg_at(il); fa.part_g = p->att_partg_at(il); fa.cnt = p->att_cnt;
                    if (g.opt_test_fused_timeout && il == 0) fa.gran = p->dead_gran;  // test hook: layer 0's attention never gets its rows
                    const size_t lds = std::max(attn_decode_lds(fa.Clds, m.D), (size_t)((nbE + 63) / 64 * 64) * 40);
                    if (!fuse_wo) {
                        with_qt(qt, [&](auto QT) { launch_qkv_attn<CT(QT)>(ba, fa, fsh, lds); });
                        return;
                    }
                    // wo + residual ride along too: no wo launch below
                    fa.ogran = p->ogran + (size_t)il * (size_t)(nbE * OGRAN);
                    WoTailArgs wt;
                    memset(&wt, 0, sizeof(wt));
                    wt.w = w.wo; wt.res = xin; wt.dst = p->xb;
                    wt.ts = cx.next_ts(); wt.ts_wgs = g.timeline_wgs;  // (the slot the wo launch would have taken)
                    if (g.opt_warm_mb > 0 && big && (cx.kind_mask & 5u) == 5u && g.num_cus % 8 == 0 && F >= (int64_t)g.num_cus * BIG_W) {  // (w1|w3 on num_cus workgroups: rows = x mod 8 on XCD x)  // the first rows of w1|w3 into L2 while the attention runs (NextWarm); not in a replay that has no w1|w3 launch to profit
                        NextWarm &nw = wt.warm;
                        int64_t wrows = (int64_t)((double)g.opt_warm_mb * 1e6 / (2.0 * (double)nbE * bb)) & ~(int64_t)7;
                        wrows = std::min<int64_t>(wrows, F);
                        for (const QWeight *q : {&w.w1, &w.w3})
                            for_each_weight_array(qt, *q, nbE, [&](const void *b, size_t rb) {
                                if (b && nw.n < WARM_MAX) { nw.base[nw.n] = (const uint8_t *)b; nw.row_bytes[nw.n] = (uint32_t)rb; nw.rows_of[nw.n++] = (int)wrows; }
                            });
                        nw.rows = (int)wrows;
                        nw.bcast = (const uint8_t *)ln.ffn_norm; nw.bcast_bytes = (int)(E * 4);
                        wt.warm_wave = 15;
                    }
                    with_qt(qt, [&](auto QT) { launch_qkv_attn_wo<CT(QT)>(ba, fa, wt, fsh, lds); });
                });
            } else
                matvec(0, epi_qkv, x_norm, x_norm, a, nullptr, p->rope, nwg, qkv_bytes);
        }
        // ---- attention over the cache; output re-quantized for wo ----
        if (!fsh.ok) {
            const double bytes = (double)(m.n_past + 1) * m.Egqa * 4.0 + m.E * 9.0;
            if (cx.want(GGML_HIP_KCLASS_ATTN, bytes)) {
                Timed tm(GGML_HIP_KCLASS_ATTN, bytes);
                long long *ts_attn = cx.next_ts();
                if (!long_ctx) {
                    launch_attn_decode(p, il, 1, attn_decode_rows(m.C, 1, m.H), f16d, nullptr, ts_attn);
                } else {  // every CU pulls a piece of the cache (kernels/decode_attn_split.h)
                    AttnSplitOneArgs oa = split_attn_args(p, il);
                    AttnSplitArgs &sa = oa.a;
                    sa.sc = p->att_sc; sa.pmax = p->att_pmax; sa.part = p->att_part;
                    const dim3 grid((unsigned)m.H, (unsigned)sa.S);
                    if (attn_one_ok(m, p->att_S)) {  // the three phases as ONE launch (k_attn_split_one)
                        launch_attn_split_one(p, oa, f16d);
                    } else {
                        hipLaunchKernelGGL(k_attn_split_scores, grid, dim3(1024), 0, g.stream, sa);
                        hipLaunchKernelGGL(k_attn_split_vp, grid, dim3(1024), attn_split_chunk_max(m.C, sa.S) * 2, g.stream, sa);
                        with_bool(f16d, [&](auto F16D) { hipLaunchKernelGGL(k_attn_split_out<CT(F16D)>, dim3((unsigned)m.H), dim3(256), 0, g.stream, sa); });
                    }
                }
                HIP_CHECK(hipGetLastError());
            }
        }
        // ---- wo + residual ----
        if (!fuse_wo) {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.wo; a.x = actE; a.nb = nbE; a.dst = p->xb; a.res = xin;
            matvec(1, epi_add, x_q8, x_q8, a, nullptr, nullptr, (int)((E + 7) / 8), wo_bytes);
        }
        // ---- ffn norm + silu(w1 x) * (w3 x) ----
        if (!fuse_x) rmsq(p->xb, ln.ffn_norm, nullptr);
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.w1; a.w[1] = w.w3; a.x = actE; a.xf = p->xb; a.xw = ln.ffn_norm; a.eps = m.eps; a.nb = nbE;
            a.dst = p->gate;
            matvec(2, epi_gate, x_norm, x_norm, a, nullptr, nullptr, (int)((F + 7) / 8), 2.0 * F * nbE * bb + nbE * 40.0 + F * 4.0);
        }
        // ---- re-quantize the gate, w2 + residual → next layer's input ----
        if (!fuse_x)
            cx.other((double)F * 5.25, [&] {
                launch_quant_row(f16d, (const float *)p->gate, nbF, 1, p->f_lo, p->f_hi, p->f_d, p->f_s, nullptr, nullptr);
            });
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.w2; a.x = actF; a.xf = p->gate; a.nb = nbF; a.dst = xout; a.res = p->xb;
            matvec(3, epi_add, x_f32, x_f32, a, nullptr, nullptr, (int)((E + 7) / 8), (double)E * nbF * bb + nbF * 40.0 + E * 8.0);
        }
    }
    if (!m.output) return;  // not the last stage: the last layer's w2 launch has written the residual into the outgoing hand-off buffer
    const ResultDst dst = plan_result_dst(p, cx);
    if (m.out_k) return plan_lm_head_k(p, cx, dst);  // a K output under these layers: the K plan's tail (its own norm staging or norm launch)
    if (!big) rmsq(p->xa, p->norm, dst.emb);  // final norm: f32 copy for OutputRequest.embeddings + Q8 for lm_head
    {
        DecMmvqArgs a;
        memset(&a, 0, sizeof(a));
        a.w[0] = p->output; a.x = actE; a.nb = nbE; a.dst = (float *)dst.logits;
        a.xf = p->xa; a.xw = p->norm; a.eps = m.eps;
        matvec(4, epi_store, x_norm, x_q8, a, dst.emb, nullptr, (int)((m.V + 7) / 8), (double)m.V * nbE * bb + nbE * 40.0 + m.V * 4.0);
    }
}

// ---------------------------------------------------------------------------------------------------
// The K plan: single-token decode of a LLaMA whose matrices are K-quants (any mix of Q2_K … Q6_K per tensor, as the
// *_K_S / *_K_M file types of crates/llm-base/src/loader.rs:80-93 mix them).  10-13 launches per layer (kernels/kquant_plan.h):
//   norm+Q8_K | wq|wk|wv | rope + K/V store | attention | Q8_K | wo+residual | norm+Q8_K | w1|w3 | silu·mul+Q8_K | w2+residual
// (matrices that share an activation row go out as ONE launch per run of equal types: 10 launches per layer for a uniform
// model, up to 13 for a mixed one); chunks of 2..31 tokens and batched steps of 2..8 sessions (option plan_batch_k) are the same launches
// with N rows, the mat-vecs in passes of 8 / 4 / 2 / 1 columns
// the mat-vecs are the node-by-node executor's k_mmvq_k / k_mmvq_k2 (same row sums), the attention is k_attn_decode over the
// whole context.  Same `mask` / `kind_mask` protocol as plan_launch_all for the roofline leg (kinds: 0 wq+wk+wv, 1 wo,
// 2 w1+w3, 3 w2, 4 lm_head).
// ---------------------------------------------------------------------------------------------------
// launches over up to three matrices of ONE type that share the activation rows (rows of all of them dealt together); N columns
// in chunks of 8 / 4 / 2 / 1 as the node-by-node executor takes them (mul_mat_k): dsts[i] is [N][M_i], res like dsts[0]
static void launch_mmvq_kn(int nseg, const KWeight *const *ws, float *const *dsts, const KAct &x, int N, const float *res) {
    const KWeight &w = *ws[0];
    const int64_t K = w.nsb * 256, nsb = w.nsb;
    int64_t Mt = 0;
    for (int i = 0; i < nseg; i++) Mt += ws[i]->M;
    const size_t col_lds = (size_t)K + (size_t)nsb * (4 + 64);
    for (int c0 = 0; c0 < N;) {
        int ncols = 8;
        while (ncols > 1 && (ncols > N - c0 || (size_t)ncols * col_lds > 150 * 1024)) ncols >>= 1;
        const size_t lds = (size_t)ncols * col_lds;
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (150 * 1024) / std::max<size_t>(lds, 1)));
        const int nwg = (int)std::min<int64_t>((Mt + 3) / 4, (int64_t)g.num_cus * per_cu);
        MmvqKArgs a;
        memset(&a, 0, sizeof(a));
        a.w = w;
        a.x.q8 = x.q8 + (int64_t)c0 * K;
        a.x.d8 = x.d8 + (int64_t)c0 * nsb;
        a.x.bs = x.bs + (int64_t)c0 * nsb * 16;
        a.dst = dsts[0] + (int64_t)c0 * ws[0]->M;
        a.ldd = ws[0]->M;
        a.res = res ? res + (int64_t)c0 * ws[0]->M : nullptr;
        a.nseg = nseg;
        if (nseg > 1) { a.wb = *ws[1]; a.dst_b = dsts[1] + (int64_t)c0 * ws[1]->M; a.ldd_b = ws[1]->M; }
        if (nseg > 2) { a.wc = *ws[2]; a.dst_c = dsts[2] + (int64_t)c0 * ws[2]->M; a.ldd_c = ws[2]->M; }
        with_kt(w.kt, [&](auto KT) { launch_mmvq_k_c<CT(KT)>(a, ncols, nwg, lds); });
        HIP_CHECK(hipGetLastError());
        c0 += ncols;
    }
}
// the decode mat-vec of Q4_K / Q6_K matrices as one wave of 1024-thread workgroups that stage the activation themselves
// (kernels/kquant_big.h): xsrc says what the row is made from (KX_NORM: rms_norm(xf) * xw; KX_F32: xf; KX_SILU_MUL: silu(xf) * xw);
// the F16 plan's mat-vec (k_mmvq_f16) stages its rows from the same description
struct RowSrc {
    int xsrc;
    const float *xf, *xw;
    float eps;
    float *y_out;
};
template <int KT>
static void launch_qkv_attn_k(const KBigArgs &ka, const FusedAttnArgs &fa, size_t lds) {
    lds_opt_in<k_qkv_attn_k<KT>>(lds, ATTN_DECODE_LDS_MAX);
    hipLaunchKernelGGL((k_qkv_attn_k<KT>), dim3((unsigned)g.num_cus), dim3(KBIG_T), lds, g.stream, ka, fa);
}
template <int KT>
static void launch_kbig_x(const KBigArgs &a, int xsrc, size_t lds, int epi) {
    const dim3 grid((unsigned)g.num_cus), block(KBIG_T);
    if (epi == KE_GATE) {  // silu(w1 x) * (w3 x): always behind the ffn norm
        hipLaunchKernelGGL((k_mmvq_kbig<KT, KX_NORM, KE_GATE>), grid, block, lds, g.stream, a);
        return;
    }
    if (epi == KE_QKV) {  // RoPE + K/V store in the epilogue: always behind the attention norm
        hipLaunchKernelGGL((k_mmvq_kbig<KT, KX_NORM, KE_QKV>), grid, block, lds, g.stream, a);
        return;
    }
    switch (xsrc) {
        case KX_NORM: hipLaunchKernelGGL((k_mmvq_kbig<KT, KX_NORM>), grid, block, lds, g.stream, a); break;
        case KX_F32: hipLaunchKernelGGL((k_mmvq_kbig<KT, KX_F32>), grid, block, lds, g.stream, a); break;
        default: hipLaunchKernelGGL((k_mmvq_kbig<KT, KX_SILU_MUL>), grid, block, lds, g.stream, a); break;
    }
}
static void launch_kbig(int nseg, const KWeight *const *ws, float *const *dsts, const RowSrc &src, const float *res, int epi = KE_ROW,
                        const KBigArgs *qkv = nullptr, const FusedAttnArgs *fused = nullptr) {
    const KWeight &w = *ws[0];
    const int64_t K = w.nsb * 256, nsb = w.nsb;
    KBigArgs ka;
    memset(&ka, 0, sizeof(ka));
    MmvqKArgs &a = ka.m;
    a.w = w;
    a.dst = dsts[0];
    a.ldd = ws[0]->M;
    a.res = res;
    a.nseg = nseg;
    if (nseg > 1) { a.wb = *ws[1]; a.dst_b = dsts[1]; a.ldd_b = ws[1]->M; }
    if (nseg > 2) { a.wc = *ws[2]; a.dst_c = dsts[2]; a.ldd_c = ws[2]->M; }
    ka.xf = src.xf; ka.xw = src.xw; ka.eps = src.eps; ka.y_out = src.y_out;
    if (qkv) {
        for (int i = 0; i < 3; i++) ka.seg_kind[i] = qkv->seg_kind[i];
        ka.rope = qkv->rope; ka.prm = qkv->prm; ka.mem_k = qkv->mem_k; ka.mem_v = qkv->mem_v; ka.Egqa = qkv->Egqa; ka.C = qkv->C; ka.D = qkv->D;
        ka.gran = qkv->gran; ka.epoch = qkv->epoch;
    }
    ka.hot = g.hot_line;
    {   // waves that take units: the count in [8, 16] that deals the launch's units most evenly (as launch_big does)
        int64_t Mt = 0;
        for (int i = 0; i < nseg; i++) Mt += ws[i]->M;
        const int64_t units = epi == KE_GATE ? ws[0]->M : epi == KE_QKV ? Mt / 2 : Mt;
        // (measured, LLaMA-7B Q4_K: dealing wq|wk|wv's 6144 row pairs over 12 waves — two each — is no faster than over all 16:
        //  the K dots are VALU-bound, every wave that sits out costs issue slots; GGML_HIP_KBIG_WAVES=0 selects the even dealing)
        static const int kw = getenv("GGML_HIP_KBIG_WAVES") ? atoi(getenv("GGML_HIP_KBIG_WAVES")) : 16;
        ka.wdeal = kw == 0 ? big_waves(units, g.num_cus, 8) : std::min(16, std::max(8, kw));
    }
    const size_t lds = (size_t)K + (size_t)((nsb + 3) & ~(int64_t)3) * 4 + (size_t)nsb * 64;
    if (fused) {  // the attention workgroups ride in this launch
        ka.wdeal = 0;
        const size_t lds2 = std::max(lds, attn_decode_lds(fused->Clds, fused->D));
        with_kt(w.kt, [&](auto KT) { launch_qkv_attn_k<CT(KT)>(ka, *fused, lds2); });
    } else
        with_kt(w.kt, [&](auto KT) { launch_kbig_x<CT(KT)>(ka, src.xsrc, lds, epi); });
    HIP_CHECK(hipGetLastError());
}
// The lm_head of an out_k plan (block-format layers under a K output matrix: plan_launch_all, plan_launch_chunk) over the N rows of
// p->xa — the K plan's tail, nothing new.  A single token whose matrix k_mmvq_kbig takes (out_k_big): that one launch, which stages the
// final norm itself and taps the embedding row.  Otherwise k_k_norm_quant over the N rows (f32 copy into dst.emb, Q8_K into the plan's
// k_* rows) and k_mmvq_k in passes of 8 / 4 / 2 / 1 columns.  Both repeat the node-by-node executor's Q8_K quantizer and row sums.
static void plan_lm_head_k(DecodePlan *p, LaunchCtx &cx, const ResultDst &dst) {
    const LlamaMatch &m = p->m;
    const int N = m.N;
    const KWeight *const ws[1] = {&p->k_output};
    float *const ds[1] = {(float *)dst.logits};
    const double bytes = (double)N * ws[0]->nsb * 292.0 + (double)ws[0]->M * ws[0]->nsb * k_block_bytes(ws[0]->kt) + (double)N * ws[0]->M * 4.0;
    if (out_k_big(m)) {
        cx.mmvq(4, bytes, [&] { launch_kbig(1, ws, ds, RowSrc{KX_NORM, p->xa, p->norm, m.eps, dst.emb}, nullptr); });
        return;
    }
    cx.other((double)N * m.E * 9.3, [&] { launch_k_norm_quant(p->xa, p->norm, m.eps, m.E, N, dst.emb, p->k_q8, p->k_d8, p->k_bs); });
    cx.mmvq(4, bytes, [&] { launch_mmvq_kn(1, ws, ds, KAct{p->k_q8, p->k_d8, p->k_bs}, N, nullptr); });
}
// batch: a batched step (plan_launch_batch) — the chunk's helper-launch form with column c at its own session's position and cache
// (BatchCols): the RoPE tables, the rope/store and the attention are the three launches that read the table; AV_SHORT always
static void plan_launch_k(DecodePlan *p, int av, LaunchCtx cx, bool batch = false) {
    const bool long_ctx = av == AV_SPLIT;
    const bool kbig = kbig_ok(p);
    if (batch && (kbig || long_ctx || !p->bcols)) die("K plan: a batched step runs on the helper-launch form at AV_SHORT (N %d)", p->m.N);
    const LlamaMatch &m = p->m;
    const int64_t E = m.E, F = m.F, nsbE = E / 256, nsbF = F / 256;
    const int N = m.N;  // 1 = decode; 2..8 = a prompt chunk (rows of every activation buffer, columns of every mat-vec)
    const KAct act{p->k_q8, p->k_d8, p->k_bs};
    // bytes of one launch over ws[i .. j): the activation rows + every matrix and its output (`out`: bytes per output element)
    auto run_bytes = [&](const KWeight *const *ws, int i, int j, double out) {
        double bytes = (double)N * ws[i]->nsb * 292.0;
        for (int k = i; k < j; k++) bytes += (double)ws[k]->M * ws[k]->nsb * k_block_bytes(ws[k]->kt) + (double)N * ws[k]->M * out;
        return bytes;
    };
    // matrices of one kind that share the activation row: one launch per run of equal types (a *_K_M file mixes Q4_K and Q6_K)
    // src: what the big-workgroup form stages the activation from (kbig); the helper-launch form reads the Q8_K row `act`
    auto mmvq = [&](int kind, std::initializer_list<const KWeight *> wl, std::initializer_list<float *> dl, const float *res,
                    const RowSrc &src) {
        const KWeight *const *ws = wl.begin();
        float *const *ds = dl.begin();
        auto run = [&](int i, int j) {
            cx.mmvq(kind, run_bytes(ws, i, j, res ? 8.0 : 4.0), [&] {
                if (kbig)
                    launch_kbig(j - i, ws + i, ds + i, src, res);
                else
                    launch_mmvq_kn(j - i, ws + i, ds + i, act, N, res);
            });
        };
        if (g.opt_plan_k == 2)  // one launch per matrix (tests)
            for (int i = 0; i < (int)wl.size(); i++) run(i, i + 1);
        else
            for_each_type_run(ws, (int)wl.size(), run);
    };
    auto norm_quant = [&](const float *x, const float *w, float *y) {
        if (kbig) return;  // staged by the mat-vec that follows
        cx.other((double)N * E * 9.3, [&] {
            launch_k_norm_quant(x, w, m.eps, E, N, y, p->k_q8, p->k_d8, p->k_bs);
        });
    };
    plan_open_rows(p, cx, batch, 4.6, [&] { dequant_k_rows(p->k_wte, (const int *)p->prm->tokens, N, p->xa, E); });
    for (int il = 0; il < m.L; il++) {
        const DecodePlan::KLW &w = p->klw[il];
        const DecodePlan::LayerNorms &nw = p->ln[il];
        __half *mk = batch ? nullptr : p->mem_k_at(il), *mv = batch ? nullptr : p->mem_v_at(il);
        norm_quant(p->xa, nw.attn_norm, nullptr);
        // big-workgroup form: RoPE and the K/V store ride in the epilogue of the wq / wk / wv launches (a unit = two adjacent rows of a
        // matrix, k_k_rope_store's expressions); one launch per run of equal types, as below
        const bool kqkv = kbig && g.opt_plan_k != 2 && m.D % 2 == 0 && E % 2 == 0 && m.Egqa % 2 == 0;
        // ... and, while one attention workgroup per head suffices and the three matrices are of one type, the attention itself
        // (k_qkv_attn_k): no k_attn_decode launch below
        const bool kfused = kqkv && w.wq.kt == w.wk.kt && w.wk.kt == w.wv.kt && kfused_ok(p, av) && (cx.mask & (1u << GGML_HIP_KCLASS_MMVQ)) && (cx.kind_mask & 1u);
        const RowSrc attn_normed{KX_NORM, p->xa, nw.attn_norm, m.eps, nullptr};
        if (kqkv) {
            const KWeight *ws3[3] = {&w.wq, &w.wk, &w.wv};
            float *ds3[3] = {p->q, p->k_kf, p->k_vf};
            for_each_type_run(ws3, 3, [&](int i, int j) {
                cx.mmvq(0, run_bytes(ws3, i, j, 4.0), [&] {
                    KBigArgs qa;
                    memset(&qa, 0, sizeof(qa));
                    for (int k = i; k < j; k++) qa.seg_kind[k - i] = k;
                    qa.rope = p->rope; qa.prm = p->prm; qa.mem_k = mk; qa.mem_v = mv; qa.Egqa = m.Egqa; qa.C = m.C; qa.D = (int)m.D;
                    if (!kfused) {
                        launch_kbig(j - i, ws3 + i, ds3 + i, attn_normed, nullptr, KE_QKV, &qa);
                        return;
                    }
                    qa.gran = p->gran_at(il); qa.epoch = p->epoch;
                    FusedAttnArgs fa = fused_attn_args(p, il, 1, m.C);
                    fa.out_f32 = p->k_att;
                    launch_kbig(j - i, ws3 + i, ds3 + i, attn_normed, nullptr, KE_QKV, &qa, &fa);
                });
            });
        } else {
            mmvq(0, {&w.wq, &w.wk, &w.wv}, {p->q, p->k_kf, p->k_vf}, nullptr, attn_normed);
            cx.other((double)N * (E + 2 * m.Egqa) * 6.0, [&] {
                KRopeStoreArgs ra;
                memset(&ra, 0, sizeof(ra));
                ra.q = p->q; ra.k = p->k_kf; ra.v = p->k_vf; ra.rope = p->rope; ra.prm = p->prm; ra.mem_k = mk; ra.mem_v = mv;
                if (batch) { ra.bc = p->bcols; ra.kv_off = p->kv_off(il); }
                ra.E = E; ra.Egqa = m.Egqa; ra.C = m.C; ra.D = (int)m.D;
                const dim3 grid(grid1(E / 2 + m.Egqa / 2 + m.Egqa).x, (unsigned)N);
                with_bool(batch, [&](auto BATCH) { hipLaunchKernelGGL(k_k_rope_store<CT(BATCH)>, grid, dim3(256), 0, g.stream, ra); });
            });
        }
        if (!kfused) plan_attn_f32(p, cx, il, long_ctx, batch);
        if (!kbig) cx.other((double)N * E * 5.3, [&] { launch_k_quant((const float *)p->k_att, nsbE, N, p->k_q8, p->k_d8, p->k_bs); });
        mmvq(1, {&w.wo}, {p->xb}, p->xa, RowSrc{KX_F32, p->k_att, nullptr, 0.0f, nullptr});
        norm_quant(p->xb, nw.ffn_norm, nullptr);
        // w1 and w3 of one type: one launch whose epilogue is silu(w1 x) * (w3 x) (the product lands in p->gate, w2 stages it as a
        // plain f32 row); a mixed pair keeps two row launches and the SiLU·mul in w2's staging
        const bool kgate = kbig && w.w1.kt == w.w3.kt && w.w1.M == w.w3.M && g.opt_plan_k != 2;
        const RowSrc ffn_normed{KX_NORM, p->xb, nw.ffn_norm, m.eps, nullptr};
        if (kgate) {
            const KWeight *ws2[2] = {&w.w1, &w.w3};
            float *ds2[2] = {p->gate, p->k_g3};
            const double bytes = (double)w.w1.nsb * 292.0 + 2.0 * (double)w.w1.M * w.w1.nsb * k_block_bytes(w.w1.kt) + (double)w.w1.M * 4.0;
            cx.mmvq(2, bytes, [&] { launch_kbig(2, ws2, ds2, ffn_normed, nullptr, KE_GATE); });
        } else {
            mmvq(2, {&w.w1, &w.w3}, {p->gate, p->k_g3}, nullptr, ffn_normed);
        }
        if (!kbig) cx.other((double)N * F * 9.3, [&] {
            launch_k_silu_mul_quant((const float *)p->gate, (const float *)p->k_g3, nsbF, N, p->k_q8, p->k_d8, p->k_bs);
        });
        mmvq(3, {&w.w2}, {p->xa}, p->xb, kgate ? RowSrc{KX_F32, p->gate, nullptr, 0.0f, nullptr} : RowSrc{KX_SILU_MUL, p->gate, p->k_g3, 0.0f, nullptr});
    }
    if (plan_hand_on(p, cx)) return;
    const ResultDst dst = plan_result_dst(p, cx);
    norm_quant(p->xa, p->norm, dst.emb);  // all N rows: f32 copy (embedding_result node) + Q8_K
    mmvq(4, {&p->k_output}, {(float *)dst.logits}, nullptr, RowSrc{KX_NORM, p->xa, p->norm, m.eps, dst.emb});
}
// ---------------------------------------------------------------------------------------------------
// The F16 plan: a LLaMA whose matrices are F16 (file type 1).  Five launches per layer (kernels/decode_f16.h):
//   norm + wq|wk|wv + RoPE + K/V store | attention | wo + residual | norm + silu(w1 x) * (w3 x) | w2 + residual
// for single-token decode, for a chunk of 2..31 tokens (the same launches with N columns, in passes of 8 / 4 / 2 / 1 columns per
// mat-vec, whichever its LDS holds) and for a batched step (`batch`: column c sits at its own session's position and cache, BatchCols).
// A row's result does not depend on the columns beside it (the kernel's design rule): the chunk equals N single tokens and the
// batched step equals the chunk, bit for bit.  Same `mask` / `kind_mask` protocol as the other plans.
// ---------------------------------------------------------------------------------------------------
struct F16Qkv {
    const float *rope;
    const DecParams *prm;
    const BatchCols *bc;
    int64_t kv_off;
    __half *mem_k, *mem_v;
    int64_t Egqa, C;
    int D;
};
template <int XSRC, int EPI, int NCOLS>
static void launch_f16_inst(const F16Args &a, int G, size_t lds) {
    lds_opt_in<k_mmvq_f16<XSRC, EPI, NCOLS>>(lds, 150 * 1024);
    hipLaunchKernelGGL((k_mmvq_f16<XSRC, EPI, NCOLS>), dim3((unsigned)G), dim3(F16_T), lds, g.stream, a);
}
template <int XSRC, int EPI>
static void launch_f16_cols(const F16Args &a, int ncols, int G, size_t lds) {
    switch (ncols) {
        case 8: launch_f16_inst<XSRC, EPI, 8>(a, G, lds); break;
        case 4: launch_f16_inst<XSRC, EPI, 4>(a, G, lds); break;
        case 2: launch_f16_inst<XSRC, EPI, 2>(a, G, lds); break;
        default: launch_f16_inst<XSRC, EPI, 1>(a, G, lds); break;
    }
}
// whether launch_f16 takes these matrices with this source / epilogue pair (the pairs plan_launch_f16 launches)
static bool f16_launch_ok(int nseg, const F16W *ws, int64_t K, int xsrc, int epi) {
    const bool pair_ok = (xsrc == KX_NORM && (epi == KE_QKV || epi == KE_ROW || epi == KE_GATE)) || ((xsrc == KX_F32 || xsrc == KX_SILU_MUL) && epi == KE_ROW);
    if (!pair_ok || nseg < 1 || nseg > 3 || (epi == KE_GATE && nseg != 2)) return false;
    int64_t Mt = 0;
    for (int i = 0; i < nseg; i++) {
        if (!f16_weight_ok(ws[i]) || ws[i].ld < K) return false;
        if (epi == KE_QKV && ws[i].M % 2) return false;
        Mt += ws[i].M;
    }
    if (epi == KE_GATE && ws[0].M != ws[1].M) return false;
    return f16_launch_shape_ok(K, epi == KE_GATE ? ws[0].M : epi == KE_QKV ? Mt / 2 : Mt);
}
// one mat-vec of the F16 plan over N columns: dsts[i] is [N][M_i], res like dsts[0]; seg_kind (KE_QKV): which of wq / wk / wv ws[i] is
static void launch_f16(int nseg, const F16W *ws, float *const *dsts, int64_t K, const RowSrc &src, const float *res, int N, int epi = KE_ROW,
                       const F16Qkv *qkv = nullptr, const int *seg_kind = nullptr) {
    if (!f16_launch_ok(nseg, ws, K, src.xsrc, epi)) die("k_mmvq_f16: a launch the F16 plan's preconditions exclude (K %lld)", (long long)K);
    int64_t Mt = 0;
    for (int i = 0; i < nseg; i++) Mt += ws[i].M;
    const int64_t units = epi == KE_GATE ? ws[0].M : epi == KE_QKV ? Mt / 2 : Mt;
    const int G = big_groups(units, g.num_cus);
    for (int c0 = 0; c0 < N;) {
        const int ncols = f16_pass_cols(K, N - c0);
        F16Args a;
        memset(&a, 0, sizeof(a));
        a.nseg = nseg;
        a.K = (int)K;
        for (int i = 0; i < nseg; i++) {
            a.w[i] = ws[i].p; a.M[i] = ws[i].M; a.ld[i] = ws[i].ld;
            a.dst[i] = dsts[i] ? dsts[i] + (int64_t)c0 * ws[i].M : nullptr;
            if (seg_kind) a.seg_kind[i] = seg_kind[i];
        }
        a.res = res ? res + (int64_t)c0 * ws[0].M : nullptr;
        a.xf = src.xf + (int64_t)c0 * K;
        a.xw = src.xsrc == KX_SILU_MUL ? src.xw + (int64_t)c0 * K : src.xw;
        a.eps = src.eps;
        a.y_out = src.y_out ? src.y_out + (int64_t)c0 * K : nullptr;
        a.col0 = c0;
        if (qkv) {
            a.rope = qkv->rope + (int64_t)c0 * 128; a.prm = qkv->prm; a.bc = qkv->bc; a.kv_off = qkv->kv_off;
            a.mem_k = qkv->mem_k; a.mem_v = qkv->mem_v; a.Egqa = qkv->Egqa; a.C = qkv->C; a.D = qkv->D;
        }
        a.hot = g.hot_line;
        const size_t lds = (size_t)ncols * (size_t)K * 2;
        if (epi == KE_QKV) launch_f16_cols<KX_NORM, KE_QKV>(a, ncols, G, lds);
        else if (epi == KE_GATE) launch_f16_cols<KX_NORM, KE_GATE>(a, ncols, G, lds);
        else if (src.xsrc == KX_NORM) launch_f16_cols<KX_NORM, KE_ROW>(a, ncols, G, lds);
        else if (src.xsrc == KX_F32) launch_f16_cols<KX_F32, KE_ROW>(a, ncols, G, lds);
        else launch_f16_cols<KX_SILU_MUL, KE_ROW>(a, ncols, G, lds);
        HIP_CHECK(hipGetLastError());
        c0 += ncols;
    }
}
static void plan_launch_f16(DecodePlan *p, int av, LaunchCtx cx, bool batch = false) {
    const bool long_ctx = av == AV_SPLIT;
    const LlamaMatch &m = p->m;
    const int64_t E = m.E, F = m.F;
    const int N = m.N;
    // bytes of one launch: the matrices, the activation rows and the outputs (`out`: bytes per output element)
    auto mv_bytes = [&](std::initializer_list<const F16W *> wl, int64_t K, double out) {
        double bytes = (double)N * K * 4.0;
        for (const F16W *w : wl) bytes += (double)w->M * K * 2.0 + (double)N * w->M * out;
        return bytes;
    };
    plan_open_rows(p, cx, batch, 6.0, [&] {
        hipLaunchKernelGGL(k_get_rows<__half>, dim3((unsigned)((E + 255) / 256), (unsigned)N), dim3(256), 0, g.stream, (const char *)p->f_wte.p,
                           p->f_wte.ld * 2, (const int *)p->prm->tokens, p->xa, E);
    });
    for (int il = 0; il < m.L; il++) {
        const DecodePlan::FLW &w = p->flw[il];
        const DecodePlan::LayerNorms &nw = p->ln[il];
        {   // norm + wq|wk|wv + RoPE + K/V store
            const F16W ws3[3] = {w.wq, w.wk, w.wv};
            float *ds3[3] = {p->q, nullptr, nullptr};
            const int kinds[3] = {0, 1, 2};
            F16Qkv qa;
            memset(&qa, 0, sizeof(qa));
            qa.rope = p->rope; qa.prm = p->prm; qa.Egqa = m.Egqa; qa.C = m.C; qa.D = (int)m.D;
            if (batch) { qa.bc = p->bcols; qa.kv_off = p->kv_off(il); }
            else { qa.mem_k = p->mem_k_at(il); qa.mem_v = p->mem_v_at(il); }
            cx.mmvq(0, mv_bytes({&w.wq, &w.wk, &w.wv}, E, 4.0), [&] {
                launch_f16(3, ws3, ds3, E, RowSrc{KX_NORM, p->xa, nw.attn_norm, m.eps, nullptr}, nullptr, N, KE_QKV, &qa, kinds);
            });
        }
        plan_attn_f32(p, cx, il, long_ctx, batch);
        {
            float *d1[1] = {p->xb};
            cx.mmvq(1, mv_bytes({&w.wo}, E, 8.0), [&] { launch_f16(1, &w.wo, d1, E, RowSrc{KX_F32, p->k_att, nullptr, 0.0f, nullptr}, p->xa, N); });
        }
        {
            const F16W ws2[2] = {w.w1, w.w3};
            float *d2[2] = {p->gate, nullptr};
            cx.mmvq(2, (double)N * E * 4.0 + 2.0 * (double)F * E * 2.0 + (double)N * F * 4.0,
                    [&] { launch_f16(2, ws2, d2, E, RowSrc{KX_NORM, p->xb, nw.ffn_norm, m.eps, nullptr}, nullptr, N, KE_GATE); });
        }
        {
            float *d1[1] = {p->xa};
            cx.mmvq(3, mv_bytes({&w.w2}, F, 8.0), [&] { launch_f16(1, &w.w2, d1, F, RowSrc{KX_F32, p->gate, nullptr, 0.0f, nullptr}, p->xb, N); });
        }
    }
    if (plan_hand_on(p, cx)) return;
    const ResultDst dst = plan_result_dst(p, cx);
    float *d1[1] = {(float *)dst.logits};
    cx.mmvq(4, mv_bytes({&p->f_output}, E, 4.0),
            [&] { launch_f16(1, &p->f_output, d1, E, RowSrc{KX_NORM, p->xa, p->norm, m.eps, dst.emb}, nullptr, N); });
}
// ---------------------------------------------------------------------------------------------------
// The MPT plan: single-token decode of an MPT graph (LlamaMatch::mpt), block-format weights.  Five launches per layer, every
// dependency a kernel boundary, one stream:
//   LayerNorm + Wqkv + K/V store | ALiBi attention | out_proj + residual | LayerNorm + up_proj + GELU | down_proj + residual
// then LayerNorm + the tied lm_head, which taps the embedding row.  The first, the fourth and the last are k_mmvq_big with the LayerNorm
// staging (XSRC_LNORM) out of the plan's own code object (mpt_plan.hip, with the attention); the two residual launches are the LLaMA
// plan's own wo / w2 instantiations (EPI_ADD over a plain f32 row).  The reference's per-token copy of the layer's whole V cache is not
// made: the attention reads memory_v's rows.  Same `mask` / `kind_mask` protocol as the other plans (kinds: 0 Wqkv, 1 out_proj,
// 2 up_proj, 3 down_proj, 4 lm_head).
// ---------------------------------------------------------------------------------------------------
static void launch_big_lnorm(int qt, int epi, const BigArgs &a) {
    const BigShape sh = big_shape(XSRC_LNORM, epi, a.nb, a.M[0]);
    if (!sh.ok) die("MPT plan: a launch the matcher's preconditions exclude (%lld rows)", (long long)a.M[0]);
    BigArgs b = a;
    b.wdeal = sh.W;  // all 16 waves stage the norm, W of them take rows (as launch_big does for XSRC_NORM)
    b.T = BigX<XSRC_NORM>::NT;
    b.G = sh.G;
    if (launch_mpt_big(g.stream, qt, epi, &b, sh.G, sh.lds)) die("MPT plan: no k_mmvq_big instantiation for type %d, epilogue %d", qt, epi);
}
static void plan_launch_mpt(DecodePlan *p, LaunchCtx cx) {
    const LlamaMatch &m = p->m;
    const int qt = qt_of(m.wtype);
    const int64_t E = m.E, F = m.F, nbE = E / 32, nbF = F / 32;
    const double bb = (double)blk_bytes(qt);
    const int64_t Clds = (m.C + 7) & ~(int64_t)7;
    auto big_args = [&](const DecMmvqArgs &a, float *y_out) {
        return big_pack(a, y_out, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, p->hot);  // (no timeline, no probe: the production instantiations)
    };
    auto residual = [&](int kind, const QWeight &w, const float *xf, int64_t nb, const float *res, float *dst) {
        DecMmvqArgs a;
        memset(&a, 0, sizeof(a));
        a.w[0] = w; a.xf = xf; a.nb = nb; a.dst = dst; a.res = res;
        cx.mmvq(kind, (double)E * nb * bb + nb * 40.0 + E * 8.0, [&] { with_qt(qt, [&](auto QT) { launch_big<CT(QT), EPI_ADD, XSRC_F32>(big_args(a, nullptr)); }); });
    };
    cx.other((double)E * 4.6, [&] {
        hipLaunchKernelGGL(k_get_rows_q, dim3((unsigned)((nbE + 255) / 256), 1), dim3(256), 0, g.stream, p->wte, (const int *)&p->prm->token, p->xa, E);
    });
    for (int il = 0; il < m.L; il++) {
        const DecodePlan::LW &w = p->lw[il];
        const DecodePlan::LayerNorms &ln = p->ln[il];
        {   // LayerNorm + Wqkv; q as f32, the K and V rows as f16 at position n_past of the layer's caches
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.wq; a.xf = p->xa; a.xw = ln.attn_norm; a.eps = m.eps; a.nb = nbE; a.dst = p->q; a.prm = p->prm;
            a.mem_k = p->mem_k_at(il); a.mem_v = p->mem_v_at(il); a.Egqa = E; a.C = m.C; a.D = (int)m.D;
            cx.mmvq(0, 3.0 * E * nbE * bb + nbE * 40.0 + E * 8.0, [&] { launch_big_lnorm(qt, EPI_QKV_TM, big_args(a, nullptr)); });
        }
        {
            const double bytes = (double)(m.n_past + 1) * E * 4.0 + E * 8.0;
            if (cx.want(GGML_HIP_KCLASS_ATTN, bytes)) {
                Timed tm(GGML_HIP_KCLASS_ATTN, bytes);
                if (launch_mpt_attn(g.stream, (int)m.H, p->q, p->mem_k_at(il), p->mem_v_at(il), p->prm, m.kq_scale, p->alibi, (int)m.D, E, p->k_att,
                                    Clds, attn_decode_lds(Clds, m.D)))
                    die("MPT plan: the attention's LDS opt-in failed");
                HIP_CHECK(hipGetLastError());
            }
        }
        residual(1, w.wo, p->k_att, nbE, p->xa, p->xb);
        {   // LayerNorm + up_proj + GELU
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.w1; a.xf = p->xb; a.xw = ln.ffn_norm; a.eps = m.eps; a.nb = nbE; a.dst = p->gate;
            cx.mmvq(2, (double)F * nbE * bb + nbE * 40.0 + F * 4.0, [&] { launch_big_lnorm(qt, EPI_GELU, big_args(a, nullptr)); });
        }
        residual(3, w.w2, p->gate, nbF, p->xb, p->xa);
    }
    const ResultDst dst = plan_result_dst(p, cx);
    DecMmvqArgs a;
    memset(&a, 0, sizeof(a));
    a.w[0] = p->output; a.xf = p->xa; a.xw = p->norm; a.eps = m.eps; a.nb = nbE; a.dst = (float *)dst.logits;
    cx.mmvq(4, (double)m.V * nbE * bb + nbE * 40.0 + m.V * 4.0, [&] { launch_big_lnorm(qt, EPI_STORE, big_args(a, dst.emb)); });
}
// the decode launches of a plan, whichever kind it is
static void plan_launch_decode(DecodePlan *p, int av = AV_SHORT, LaunchCtx cx = {}) {
    if (p->m.mpt)
        plan_launch_mpt(p, cx);
    else if (p->m.f16w)
        plan_launch_f16(p, av, cx);
    else if (p->m.kquant)
        plan_launch_k(p, av, cx);
    else
        plan_launch_all(p, av, cx);
}
