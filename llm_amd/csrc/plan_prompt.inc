// plan_prompt.inc — the launch sequences of evaluations of several tokens: plan_launch_multi (a chunk of 2..31 tokens, block
// formats; captured like the decode plans), plan_launch_batch (the same launches for one token each of 2..8 sessions) and
// plan_launch_prompt (a batch from mmq_min tokens on, launched eagerly).
template <int QT, int EPI, bool BATCH = false>
static void launch_big8(const Big8Args &a) {
    const int64_t Mtot = a.d.w[0].M + (EPI == EPI_QKV ? a.d.w[1].M + a.d.w[2].M : 0);
    const int64_t units = Mtot / (EPI == EPI_QKV ? 2 : 1);
    const int nwg = big_groups(units, g.num_cus);
    // waves per workgroup as for k_mmvq_big; the staging needs ncols*nb <= 4 blocks per thread and 512 RoPE threads
    const int W = big_waves(units, nwg, std::max<int>(8, (int)((a.ncols * a.d.nb + 4 * 64 - 1) / (4 * 64))));
    const size_t lds = (size_t)8 * ((a.d.nb + 63) / 64 * 64) * 40;
    lds_opt_in<k_mmvq_big8<QT, EPI, BATCH>>(lds, 152 * 1024);  // up to 150 KB of dynamic LDS
    hipLaunchKernelGGL((k_mmvq_big8<QT, EPI, BATCH>), dim3(nwg), dim3(W * 64), lds, g.stream, a);
}
// ---- the same launches on the integer matrix cores (kernels/mmq_cols.h) ----
template <int QT, int EPI, bool BATCH = false>
static void launch_cols(const ColsArgs &a0, int M_total) {
    ColsArgs a = a0;
    a.ngroups = M_total / 16 / (EPI == EPI_GATE ? 2 : 1);
    const ColsShape sh = cols_shape(a.ngroups, EPI == EPI_GATE ? 2 : 1, (int)a.d.nb);
    a.gq = a.ngroups / sh.G;
    a.gr = a.ngroups % sh.G;
    if (!a.ts || BATCH) {
        lds_opt_in<k_mmq_cols<QT, EPI, false, BATCH>>(sh.lds, 152 * 1024);
        hipLaunchKernelGGL((k_mmq_cols<QT, EPI, false, BATCH>), dim3(sh.G), dim3(COLS_T), sh.lds, g.stream, a);
    } else {  // measurement build (tests/tools/cols_timeline.py)
        lds_opt_in<k_mmq_cols<QT, EPI, true>>(sh.lds, 152 * 1024);
        hipLaunchKernelGGL((k_mmq_cols<QT, EPI, true>), dim3(sh.G), dim3(COLS_T), sh.lds, g.stream, a);
    }
}
// k_attn_decode's batched form for layer il of a batched step: a grid of heads x columns, the whole context in its LDS arrays
static void launch_attn_decode_batch(const DecodePlan *p, int il, int N, bool f16d, float *out_f32 = nullptr) {
    const LlamaMatch &m = p->m;
    with_bool(f16d, [&](auto F16D) {
        lds_opt_in<k_attn_decode_batch<CT(F16D)>>(attn_decode_lds(m.C, m.D), ATTN_DECODE_LDS_MAX);
        hipLaunchKernelGGL(k_attn_decode_batch<CT(F16D)>, dim3((unsigned)m.H, (unsigned)N), dim3(1024), attn_decode_lds(m.C, m.D), g.stream,
                           (const float *)p->q, (const BatchCols *)p->bcols, p->kv_off(il), m.kq_scale, (int)m.D, (int)(m.H / m.Hkv), m.Egqa,
                           m.C, p->e_lo, p->e_hi, p->e_d, p->e_s, (int)m.H, m.C, p->e_dT, p->e_sT, out_f32);
    });
    HIP_CHECK(hipGetLastError());
}
// The multi-token plan: a prompt chunk of 2..8 tokens (InferenceSession::feed_prompt at the default n_batch = 8) as
// 8 launches per layer — k_rmsnorm_quant (N rows), k_mmvq_big8<QKV>, k_attn_decode (grid heads x N: query n attends
// to positions <= n_past + n), k_mmvq_big8<ADD> (wo), k_rmsnorm_quant, k_mmvq_big8<GATE>, k_quant_row, k_mmvq_big8<ADD>
// (w2) — every weight matrix streamed once per chunk instead of once per token-column pass of the generic executor.
// Each mat-vec runs on k_mmq_cols in passes of 8 columns instead where its shape allows (multi_cols; chunks of 9..31 tokens
// only so).
// batch: the N columns are one token each of N different sessions of the model (DecodePlan::bcols says where each sits) instead of
// N consecutive positions of one: the same launches, but the three that place a column in a cache — the RoPE tables, the
// wq|wk|wv epilogue and the attention — in their batched forms.  Everything else is column-local and does not know the difference.
static void plan_launch_chunk(DecodePlan *p, const bool batch) {
    const LlamaMatch &m = p->m;
    LaunchCtx cx;  // everything is launched; the timeline has one record per k_mmq_cols launch, in launch order
    const int N = m.N, qt = qt_of(m.wtype);
    const bool f16d = qt_f16d(qt);
    const int64_t E = m.E, F = m.F, nbE = E / 32, nbF = F / 32;
    const QAct actE{(const i32x4 *)p->e_lo, (const i32x4 *)p->e_hi, p->e_d, p->e_s};
    const QAct actF{(const i32x4 *)p->f_lo, (const i32x4 *)p->f_hi, p->f_d, p->f_s};
    const float theta_scale = powf(m.freq_base, -2.0f / m.n_dims);
    const MultiCols cols = multi_cols(m);
    // the rows the NEXT launch (k_mmq_cols over `ws`, nsub = 2: w1 and w3 as pairs of groups) will read first, for the idle workgroups of
    // the norm launch to pull into the right L2s (ColsWarm, kernels/decode.h): as many leading groups per workgroup as warm_mb buys
    auto cols_warm_of = [&](bool on_cols, std::initializer_list<const QWeight *> ws, int nsub, int64_t nb) {
        ColsWarm cw;
        memset(&cw, 0, sizeof(cw));
        if (!on_cols || g.opt_warm_mb <= 0 || g.xcd_labels != 1 || N < 2 || N > 8 || N + 8 > g.num_cus) return cw;
        int64_t Mt = 0;
        for (const QWeight *q : ws) Mt += q->M;
        const int ngroups = (int)(Mt / 16 / nsub);
        const ColsShape sh = cols_shape(ngroups, nsub, (int)nb);
        if (sh.G != g.num_cus) return cw;  // (one workgroup per CU: the placement the labels were probed for)
        double row_bytes = 0;
        int64_t row0 = 0;
        for (const QWeight *q : ws) {
            for_each_weight_array(qt, *q, nb, [&](const void *b, size_t rb) {
                if (!b || cw.n >= CW_MAX) return;
                cw.base[cw.n] = (const uint8_t *)b; cw.row_bytes[cw.n] = (uint32_t)rb; cw.row0[cw.n] = (int)row0; cw.rows[cw.n] = (int)q->M;
                cw.n++;
                row_bytes += (double)rb;
            });
            if (nsub == 1) row0 += q->M;  // wq | wk | wv are one row space; w1 and w3 share theirs
        }
        if (nsub == 1) row_bytes /= (double)ws.size();  // bytes per row of the launch's row space (gate: both matrices' rows per group)
        cw.G = sh.G; cw.gq = ngroups / sh.G; cw.gr = ngroups % sh.G;
        // budget: 14 MB per launch at most (sweep r6_colswarm2.sh: 12-16 MB = one leading group of wq|wk|wv and lm_head per workgroup
        // 3.48k -> 3.51k tok/s at n_batch 8; 20 MB = two groups + one of w1|w3 3.50k; 8 MB = nothing fits)
        const double budget_mb = std::min(14.0, (double)g.opt_warm_mb);
        cw.wg = (int)std::min<double>((double)cw.gq + 1.0, floor(budget_mb * 1e6 / ((double)sh.G * 16.0 * row_bytes)));
        if (cw.wg < 1) cw.n = 0;
        return cw;
    };
    auto rmsq = [&](const float *x, const float *w, float *y, const ColsWarm &cw) {
        cx.other((double)N * E * 9.25, [&] {
            if (cw.n > 0) g.stat_cols_warm_launches++;  // N norm workgroups + one warming workgroup on every other CU
            launch_rmsnorm_quant(f16d, x, w, m.eps, E, N, y, p->e_lo, p->e_hi, p->e_d, p->e_s, p->e_dT, p->e_sT, cw.n > 0 ? &cw : nullptr);
        });
    };
    const double bb = (double)blk_bytes(qt);
    // One mat-vec block of the chunk, epilogue EPI over M_total rows of `a`'s matrices, scale tables dT / sT: on_cols = k_mmq_cols in
    // passes of 8 columns (one pass for the default n_batch = 8; chunks of 9..31 tokens stream the weights once per pass): pass i
    // takes rows 8i.. of the activations, of dst / res, of the RoPE table, and table i of the scales; else one k_mmvq_big8 launch
    auto block = [&](int kind, auto EPI, bool on_cols, const Big8Args &a, int M_total, const float *dT, const int *sT) {
        const int64_t nb = a.d.nb;
        const double bytes = (double)M_total * nb * bb;
        constexpr bool qkv = CT(EPI) == EPI_QKV;  // the one epilogue with a batched form
        if (!on_cols) {
            cx.mmvq(kind, bytes, [&] {
                with_qt(qt, [&](auto QT) {
                    if constexpr (qkv) {
                        if (batch) return launch_big8<CT(QT), CT(EPI), true>(a);
                    }
                    launch_big8<CT(QT), CT(EPI)>(a);
                });
            });
            return;
        }
        for (int c0 = 0; c0 < N; c0 += 8) {
            ColsArgs c;
            memset(&c, 0, sizeof(c));
            c.d = a.d; c.ldd = a.ldd; c.ldr = a.ldr;
            c.ncols = std::min(8, N - c0);
            c.col0 = c0;
            c.d.x.lo = a.d.x.lo + (int64_t)c0 * nb;
            c.d.x.hi = a.d.x.hi + (int64_t)c0 * nb;
            c.d.x.d = a.d.x.d + (int64_t)c0 * nb;
            c.d.x.sum = a.d.x.sum + (int64_t)c0 * nb;
            c.d.dst = a.d.dst + (int64_t)c0 * a.ldd;
            if (a.d.res) c.d.res = a.d.res + (int64_t)c0 * a.ldr;
            if (a.rope) c.rope = a.rope + (int64_t)c0 * 128;
            c.dxT = dT + (int64_t)(c0 / 8) * nb * 8;
            c.sxT = sT + (int64_t)(c0 / 8) * nb * 8;
            c.ts = cx.next_ts();
            c.ts_wgs = g.timeline_wgs;
            c.hot = g.hot_line;
            c.bc = a.bc; c.kv_off = a.kv_off;
            cx.mmvq(kind, bytes, [&] {
                with_qt(qt, [&](auto QT) {
                    if constexpr (qkv) {
                        if (batch) return launch_cols<CT(QT), CT(EPI), true>(c, M_total);
                    }
                    launch_cols<CT(QT), CT(EPI)>(c, M_total);
                });
            });
        }
    };
    if (!m.wte) {
        HIP_CHECK(hipMemcpyAsync(p->xa, p->stage_in, (size_t)N * E * 4, hipMemcpyDeviceToDevice, g.stream));
    } else {
        cx.other((double)N * E * 4.6, [&] {
            hipLaunchKernelGGL(k_get_rows_q, dim3((unsigned)((nbE + 255) / 256), (unsigned)N), dim3(256), 0, g.stream, p->wte,
                               (const int *)p->prm->tokens, p->xa, E);
        });
    }
    // RoPE tables of the chunk's N positions, shared by all layers
    if (batch)
        hipLaunchKernelGGL(k_rope_table_batch, dim3((unsigned)N), dim3(128), 0, g.stream, (const BatchCols *)p->bcols, theta_scale,
                           m.freq_scale, (int)(m.D >> 1), p->rope);
    else
        hipLaunchKernelGGL(k_rope_table, dim3((unsigned)N), dim3(128), 0, g.stream, (const DecParams *)p->prm, theta_scale,
                           m.freq_scale, (int)(m.D >> 1), p->rope);
    HIP_CHECK(hipGetLastError());
    for (int il = 0; il < m.L; il++) {
        const DecodePlan::LW &w = p->lw[il];
        const DecodePlan::LayerNorms &ln = p->ln[il];
        rmsq(p->xa, ln.attn_norm, nullptr, cols_warm_of(cols.qkv, {&w.wq, &w.wk, &w.wv}, 1, nbE));
        {
            Big8Args a;
            memset(&a, 0, sizeof(a));
            a.d.w[0] = w.wq; a.d.w[1] = w.wk; a.d.w[2] = w.wv;
            a.d.x = actE; a.d.nb = nbE; a.d.dst = p->q; a.d.prm = p->prm; a.d.mem_k = p->mem_k_at(il); a.d.mem_v = p->mem_v_at(il);
            a.d.Egqa = m.Egqa; a.d.C = m.C; a.d.D = (int)m.D; a.d.theta_scale = theta_scale; a.d.freq_scale = m.freq_scale;
            a.ncols = N; a.ldd = E; a.ldr = E; a.rope = p->rope;
            if (batch) {
                a.d.mem_k = a.d.mem_v = nullptr;
                a.bc = p->bcols; a.kv_off = p->kv_off(il);
            }
            block(0, std::integral_constant<int, EPI_QKV>{}, cols.qkv, a, (int)(E + 2 * m.Egqa), p->e_dT, p->e_sT);
        }
        {
            Timed tm(GGML_HIP_KCLASS_ATTN, (double)N * (m.n_past + N) * m.Egqa * 4.0);
            if (batch)
                launch_attn_decode_batch(p, il, N, f16d);
            else
                launch_attn_decode(p, il, N, m.C, f16d, nullptr, nullptr, p->e_dT, p->e_sT);
        }
        {
            Big8Args a;
            memset(&a, 0, sizeof(a));
            a.d.w[0] = w.wo; a.d.x = actE; a.d.nb = nbE; a.d.dst = p->xb; a.d.res = p->xa;
            a.ncols = N; a.ldd = E; a.ldr = E;
            block(1, std::integral_constant<int, EPI_ADD>{}, cols.wo, a, (int)E, p->e_dT, p->e_sT);
        }
        rmsq(p->xb, ln.ffn_norm, nullptr, cols_warm_of(cols.gate, {&w.w1, &w.w3}, 2, nbE));
        {
            Big8Args a;
            memset(&a, 0, sizeof(a));
            a.d.w[0] = w.w1; a.d.w[1] = w.w3; a.d.x = actE; a.d.nb = nbE; a.d.dst = p->gate;
            a.ncols = N; a.ldd = F; a.ldr = F;
            block(2, std::integral_constant<int, EPI_GATE>{}, cols.gate, a, (int)(2 * F), p->e_dT, p->e_sT);
        }
        cx.other((double)N * F * 5.25, [&] {
            launch_quant_row(f16d, (const float *)p->gate, nbF, N, p->f_lo, p->f_hi, p->f_d, p->f_s, p->f_dT, p->f_sT);
        });
        {
            Big8Args a;
            memset(&a, 0, sizeof(a));
            a.d.w[0] = w.w2; a.d.x = actF; a.d.nb = nbF; a.d.dst = p->xa; a.d.res = p->xb;
            a.ncols = N; a.ldd = E; a.ldr = E;
            block(3, std::integral_constant<int, EPI_ADD>{}, cols.w2, a, (int)E, p->f_dT, p->f_sT);
        }
    }
    if (!m.output) {
        HIP_CHECK(hipMemcpyAsync(p->stage_out, p->xa, (size_t)N * E * 4, hipMemcpyDeviceToDevice, g.stream));
        return;
    }
    if (m.out_k) return plan_lm_head_k(p, cx, ResultDst{p->emb_out, p->logits_out});  // a K output under these layers: the K plan's tail over the N rows
    // final norm of all N rows: f32 copy (embedding_result node) + Q8
    rmsq(p->xa, p->norm, p->emb_out, cols_warm_of(cols.out, {&p->output}, 1, nbE));
    {
        Big8Args a;
        memset(&a, 0, sizeof(a));
        a.d.w[0] = p->output; a.d.x = actE; a.d.nb = nbE; a.d.dst = (float *)p->logits_out;
        a.ncols = N; a.ldd = m.V; a.ldr = m.V;
        block(4, std::integral_constant<int, EPI_STORE>{}, cols.out, a, (int)m.V, p->e_dT, p->e_sT);
    }
}
static void plan_launch_multi(DecodePlan *p) { plan_launch_chunk(p, false); }
// One decode step of N = 2..8 sessions of one model as one pass over the weights (ggml_hip_decode_batch, plan_run.inc decode_batch)
static void plan_launch_batch(DecodePlan *p) {
    if (p->m.f16w)
        plan_launch_f16(p, AV_SHORT, LaunchCtx{}, true);
    else if (p->m.kquant)
        plan_launch_k(p, AV_SHORT, LaunchCtx{}, true);
    else
        plan_launch_chunk(p, true);
}

// ---------------------------------------------------------------------------------------------------
// The prompt plan: a batch of N >= mmq_min tokens (crates/llm-base/src/inference_session.rs:315-316 feeds n_batch tokens
// per evaluate) through the same graph.  The quantized mat-muls run on the matrix cores (mmq_f16_launch, as in the
// node-by-node executor), K.Q and V.P on k_gemm_f16 — V.P writes the merged-heads layout directly — and everything
// between two GEMMs is one launch (kernels/prompt.h): 13 launches per layer instead of 24, the same bits.
// Launched eagerly (a few hundred launches of tens of microseconds each: no hipGraph needed).
// ---------------------------------------------------------------------------------------------------
template <int D, bool INSTR = false, int QR = PATTN_Q>
static void launch_p_attn(const PAttnArgs &pa, dim3 grid, size_t lds) {
    lds_opt_in<k_p_attn<D, INSTR, QR>>(lds, 150 * 1024);
    hipLaunchKernelGGL((k_p_attn<D, INSTR, QR>), grid, dim3(256), lds, g.stream, pa);
}
// Attention of a prompt batch (lib.rs:246-307): q [N][E] f32 (RoPE applied), mk / mv this layer's cache, out [N][E] f32 in
// the merged-heads layout.  fused: one launch with the scores in LDS (kernels/prompt_attn.h); else K.Q -> k_p_soft_max ->
// V.P with the scores (sc: [H][N][T] f32) and probabilities (p16: [H][N][Tp] f16, Tp = T rounded up to 8) in HBM.
static void prompt_attention(bool fused, const float *q, const __half *mk, const __half *mv, float *out, float *sc, _Float16 *p16,
                             int N, int64_t E, int64_t Egqa, int64_t H, int64_t Hkv, int64_t D, int n_past, int64_t C, float scale,
                             _Float16 *x16_out = nullptr /* fused only: write wo's re-quantized f16 operand instead of `out` */,
                             bool f16d = false, const float *rope = nullptr /* fused only: q is un-rotated (+ q_part) */, int64_t q_part = 0) {
    const int64_t T = (int64_t)n_past + N, Tp = (T + 7) & ~(int64_t)7;
    if (fused) {
        PAttnArgs pa;
        pa.q = q; pa.mem_k = mk; pa.mem_v = mv; pa.out = out;
        pa.N = N; pa.E = (int)E; pa.Egqa = (int)Egqa; pa.H = (int)H; pa.r = (int)(H / Hkv); pa.n_past = n_past;
        pa.C = C; pa.scale = scale; pa.row_bytes = prompt_attn_row_bytes(T);
        pa.x16 = x16_out; pa.f16d = f16d ? 1 : 0;
        pa.rope = rope; pa.q_part = q_part;
        const int QR = prompt_attn_queries(D, T);
        const dim3 grid((unsigned)(((N + QR - 1) / QR) * H));
        const size_t lds = (size_t)QR * std::max<size_t>(pa.row_bytes, 2 * D + 16);  // score rows (the staged Q tile borrows them)
        {   // two workgroups per CU (LDS permitting) and more workgroups than CUs: the first num_cus workgroups take the longest tiles,
            // the rest come shortest first so that a CU's two workgroups add up to the same work everywhere (kernels/prompt_attn.h);
            // worth 0.4 % of a 512-token batch (r06_sweeps.txt 15: a tile's duration is its own dependent chain, not its neighbour's)
            const int ntile = (N + QR - 1) / QR;
            const bool two_per_cu = 2 * (lds + 1024) <= 160 * 1024 && (int64_t)ntile * H > g.num_cus;
            pa.r1 = two_per_cu ? std::max(1, std::min(ntile, (int)(g.num_cus / H))) : ntile;
        }
        Timed tm(GGML_HIP_KCLASS_ATTN, (double)T * Egqa * 4.0 + (double)N * E * 8.0);
        pa.ts = nullptr;
        const bool instr = QR != 16 && g.timeline && D == 128 && (size_t)grid.x * 64 <= g.timeline_bytes;  // measurement build (tests/tools/pattn_timeline.py)
        if (QR != 16 && !instr) {
            if (D == 128) launch_p_attn<128>(pa, grid, lds);
            else if (D == 64) launch_p_attn<64>(pa, grid, lds);
            else launch_p_attn<32>(pa, grid, lds);
        } else if (QR == 16) {
            if (D == 128) launch_p_attn<128, false, 16>(pa, grid, lds);
            else if (D == 64) launch_p_attn<64, false, 16>(pa, grid, lds);
            else launch_p_attn<32, false, 16>(pa, grid, lds);
        } else {
            pa.ts = g.timeline;
            launch_p_attn<128, true>(pa, grid, lds);
        }
        HIP_CHECK(hipGetLastError());
        return;
    }
    {  // scores = K . Q  (lib.rs:248-266): [T, N, H]
        GemmF16Args ga;
        ga.a = (const char *)mk; ga.a_nb1 = Egqa * 2; ga.a_nb2 = D * 2; ga.a_nb3 = 0;
        ga.b = (const char *)q; ga.b_nb1 = E * 4; ga.b_nb2 = D * 4; ga.b_nb3 = 0;
        ga.d = (char *)sc; ga.d_nb1 = T * 4; ga.d_nb2 = (int64_t)N * T * 4; ga.d_nb3 = 0;
        ga.M = T; ga.N = N; ga.K = D; ga.ne12 = H; ga.r2 = H / Hkv; ga.r3 = 1;
        ga.causal = 1; ga.causal_past = n_past;
        ga.tiles_n = (N + 127) / 128;
        const int tiles_m = (int)((T + 127) / 128);
        Timed tm(GGML_HIP_KCLASS_ATTN, (double)T * Egqa * 2.0 + (double)N * E * 4.0 + (double)H * N * T * 4.0);
        lds_opt_in<k_gemm_f16>(MMQ_LDS, MMQ_LDS);
        hipLaunchKernelGGL(k_gemm_f16, dim3((unsigned)(tiles_m * ga.tiles_n), (unsigned)H), dim3(256), MMQ_LDS, g.stream, ga);
        HIP_CHECK(hipGetLastError());
    }
    {
        const int64_t rows = (int64_t)H * N;
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)rows * T * 8.0);
        hipLaunchKernelGGL(k_p_soft_max, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, g.stream, sc, rows, (int)T, N, scale, n_past, p16, Tp);
        HIP_CHECK(hipGetLastError());
    }
    {  // V . P (lib.rs:284-300), written in the merged-heads layout [E, N] (the permute + cpy of lib.rs:302-307)
        GemmF16Args ga;
        ga.a = (const char *)mv; ga.a_nb1 = C * 2; ga.a_nb2 = C * D * 2; ga.a_nb3 = 0;
        ga.b = (const char *)p16; ga.b_nb1 = Tp * 2; ga.b_nb2 = (int64_t)N * Tp * 2; ga.b_nb3 = 0;  // f16 rows
        ga.d = (char *)out; ga.d_nb1 = E * 4; ga.d_nb2 = D * 4; ga.d_nb3 = 0;
        ga.M = D; ga.N = N; ga.K = T; ga.ne12 = H; ga.r2 = H / Hkv; ga.r3 = 1;
        ga.causal = 2; ga.causal_past = n_past;
        ga.tiles_n = (N + 127) / 128;
        const int tiles_m = (int)((D + 127) / 128);
        Timed tm(GGML_HIP_KCLASS_ATTN, (double)T * Egqa * 2.0 + (double)H * N * T * 2.0 + (double)N * E * 4.0);
        lds_opt_in<k_gemm_f16_b16>(MMQ_LDS, MMQ_LDS);
        hipLaunchKernelGGL(k_gemm_f16_b16, dim3((unsigned)(tiles_m * ga.tiles_n), (unsigned)H), dim3(256), MMQ_LDS, g.stream, ga);
        HIP_CHECK(hipGetLastError());
    }
}
// the fused attention of a packed batch: k_p_attn_seg over the call's attention tiles (the table is in dealing order), LDS for
// the longest segment; wo's re-quantized f16 operand out, Q rotated while it is loaded, as the one-session plan's fused launch
static void prompt_attention_pack(const PackLaunch &pk, int il, const float *q, _Float16 *x16_out, int64_t E, int64_t Egqa, int64_t H, int64_t Hkv,
                                  int64_t D, int64_t C, float scale, bool f16d, const float *rope, int64_t q_part) {
    PAttnArgs pa;
    pa.q = q; pa.mem_k = nullptr; pa.mem_v = nullptr; pa.out = nullptr;
    pa.N = 0; pa.E = (int)E; pa.Egqa = (int)Egqa; pa.H = (int)H; pa.r = (int)(H / Hkv); pa.n_past = 0;
    pa.C = C; pa.scale = scale; pa.row_bytes = prompt_attn_row_bytes(pk.T_max);
    pa.x16 = x16_out; pa.f16d = f16d ? 1 : 0;
    pa.rope = rope; pa.q_part = q_part;
    pa.r1 = 0; pa.ts = nullptr;
    const size_t lds = (size_t)PATTN_Q * std::max<size_t>(pa.row_bytes, 2 * D + 16);
    Timed tm(GGML_HIP_KCLASS_ATTN, (double)pk.T_max * Egqa * 4.0 * pk.n_segs + (double)pk.n_atiles * PATTN_Q * E * 8.0);
    if (launch_p_attn_seg(g.stream, (int)D, &pa, pk.segs + (size_t)il * pk.n_segs, pk.atiles, pk.n_atiles, lds)) die("prompt pack: the fused attention's LDS opt-in failed");
    HIP_CHECK(hipGetLastError());
}
// pk: a packed batch (plan_pack.inc) — the N rows are segments of several sessions; the three launches that place a row in a sequence
// (RoPE table, K/V store, attention) run in their segment forms (kernels/prompt_pack.h), everything else is the same launch over N rows
static void plan_launch_prompt(DecodePlan *p, const PackLaunch *pk = nullptr) {
    const LlamaMatch &m = p->m;
    const bool kq = m.kquant;  // K-quant model: the GEMMs' token operand is the Q8_K round trip, the weights their f16 copies (k_prompt_weights)
    const int N = m.N, qt = kq ? QT_Q8_0 : qt_of(m.wtype);
    const bool f16d = !kq && qt_f16d(qt);
    const int64_t E = m.E, F = m.F, nbE = E / 32, nbF = F / 32, T = pk ? pk->T_max : (int64_t)m.n_past + N;
    const int64_t Tp = (T + 7) & ~(int64_t)7;  // row length of the f16 probabilities (16-byte aligned rows)
    const float theta_scale = powf(m.freq_base, -2.0f / m.n_dims);
    const bool fused_attn = g.opt_attn_fused && prompt_attn_fits(m.D, T);
    {   // Transient buffers from the executor's grow-only workspace (rewound at the start of every graph), shared by all
        // prompt plans: sized by this evaluation's T, not by the context (scores of a 512-token batch at 16k context
        // would otherwise pin 1.5 GB per cached plan).  GEMM outputs have room for the two partials of a K split.
        const size_t R = (size_t)N;
        p->p_te = (float *)ws_alloc(2 * R * E * 4);
        p->p_mg = (float *)ws_alloc(R * E * 4);
        p->p_qf = (float *)ws_alloc(2 * R * (E + 2 * m.Egqa) * 4);  // q | k | v
        p->p_kf = p->p_qf + R * E;
        p->p_vf = p->p_kf + R * m.Egqa;
        p->p_g1 = (float *)ws_alloc(2 * R * 2 * F * 4);  // w1 x | w3 x
        p->p_g3 = p->p_g1 + R * F;
        if (!fused_attn) {  // the three-launch attention keeps the scores of all heads in HBM
            p->p_sc = (float *)ws_alloc((size_t)m.H * R * T * 4);
            p->p_p16 = (_Float16 *)ws_alloc((size_t)m.H * R * Tp * 2);
        }
        p->p_x16 = (_Float16 *)ws_alloc(R * std::max(E, F) * 2);
    }
    // the f16 copies are a cache (dev_malloc may have released them, also just above); a K-quant model has no other operand
    if (kq && p->w16_gen != g.w16_gen && !k_prompt_weights(m, p))
        die("prompt plan: no room for the f16 copies of the K-quant weights any more (set GGML_HIP_PLAN_K=0 to run the node-by-node executor)");
    if (!kq && p->w16_gen != g.w16_gen) {
        // out_k: the lm_head GEMM has no operand but the f16 copy of the K output (plan_build.inc out_k_prompt_weight) — made, if it has
        // to be, before any pointer below is read again
        if (m.out_k && !out_k_prompt_weight(m, p))
            die("prompt plan: no room for the f16 copy of the K-quant output matrix any more (set GGML_HIP_PLAN_OUT_K=0 to run the node-by-node executor)");
        auto w16_of = [](const ggml_tensor *t) { DevTensor *e = plan_rec(t); return e ? e->qw.w16 : nullptr; };
        for (int il = 0; il < m.L; il++)
            for (int i = 0; i < LAYER_MATS; i++) p->lw[il].at(i).w16 = w16_of(m.layers[il].at(i));
        if (m.output && !m.out_k) p->output.w16 = w16_of(m.output);
        p->w16_gen = g.w16_gen;
    }
    // [x + r ->] rms_norm * w -> Q8 -> f16 operand of the next GEMM
    // k_row: the operand of a GEMM on the f16 copy of a K matrix under block-format layers (out_k's lm_head): the Q8_K round trip
    auto norm_quant = [&](const float *x, const float *x2, const float *r, float *xsum, const float *w, float *y_f32, bool k_row = false) {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * (r ? 18.0 : 6.0));
        if (E > 8192) die("prompt plan: rows of %lld elements (k_p_norm_quant holds a row of up to 8192 in registers)", (long long)E);
        launch_p_norm_quant(kq || k_row, f16d, x, x2, r, xsum, w, m.eps, E, N, y_f32, p->p_x16);
        HIP_CHECK(hipGetLastError());
    };
    // A GEMM whose tile count leaves CUs idle splits K in two (mmq_auto_splits, as in the node-by-node executor).  There
    // the halves meet through f32 atomics in a zeroed dst; here each half stores its partial tile (`stride` floats
    // apart) and the kernel that consumes the result adds the two — the same two addends, no memset, no atomics
    // (an E x E GEMM at 512 tokens: 41 -> ~31 us).  Returns the number of splits used.
    const int tiles_n = (N + MMQ_TN - 1) / MMQ_TN;
    const int64_t te_stride = (int64_t)N * E, qkv_stride = (int64_t)N * (E + 2 * m.Egqa), g13_stride = (int64_t)N * 2 * F;
    int sp_qkv = 1, sp_13 = 1, sp_w2 = 1;
    auto gemm = [&](const QWeight &w, float *dst, int64_t nb, int64_t stride) {
        const MmqSegHost seg{w, dst, w.M};
        const int sp = mmq_auto_splits((int)((w.M + MMQ_TM - 1) / MMQ_TM) * tiles_n, nb, true);
        mmq_f16_launch_multi(qt, 1, &seg, p->p_x16, N, nb, true, sp, false, stride);
        return sp;
    };
    // matrices that share the activations go out as ONE launch when each of them would take the same K split on its own
    // (same arithmetic as separate launches, bit for bit); their outputs are one contiguous buffer starting at dsts[0]
    auto gemm_multi = [&](int nseg, const QWeight *const *ws, float *const *dsts, int64_t nb, int64_t stride) {
        MmqSegHost segs[3];
        int splits = 0;
        bool same = (g.opt_mmq_fuse & (nseg == 3 ? 1 : 2)) != 0;  // option mmq_fuse: bit 0 = wq|wk|wv, bit 1 = w1|w3
        for (int i = 0; i < nseg; i++) {
            segs[i] = MmqSegHost{*ws[i], dsts[i], ws[i]->M};
            const int sp = mmq_auto_splits((int)((ws[i]->M + MMQ_TM - 1) / MMQ_TM) * tiles_n, nb, true);
            if (i == 0) splits = sp;
            same = same && sp == splits;
        }
        if (!same) {  // separate launches, each with its own split; the consumer adds partials for all matrices or for
                      // none, so an unsplit matrix next to a split one gets a zero second partial
            int any = 1;
            for (int i = 0; i < nseg; i++) any = std::max(any, gemm(*ws[i], dsts[i], nb, stride));
            if (any > 1)
                for (int i = 0; i < nseg; i++)
                    if (mmq_auto_splits((int)((ws[i]->M + MMQ_TM - 1) / MMQ_TM) * tiles_n, nb, true) == 1)
                        HIP_CHECK(hipMemsetAsync(dsts[i] + stride, 0, (size_t)ws[i]->M * N * 4, g.stream));
            return any;
        }
        mmq_f16_launch_multi(qt, nseg, segs, p->p_x16, N, nb, true, splits, false, stride);
        return splits;
    };
    if (!m.wte) {
        HIP_CHECK(hipMemcpyAsync(p->xa, p->stage_in, (size_t)N * E * 4, hipMemcpyDeviceToDevice, g.stream));
    } else if (kq) {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 4.6);
        dequant_k_rows(p->k_wte, (const int *)p->p_tok, N, p->xa, E);
    } else {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 4.6);
        hipLaunchKernelGGL(k_get_rows_q, dim3((unsigned)((nbE + 255) / 256), (unsigned)N), dim3(256), 0, g.stream, p->wte,
                           (const int *)p->p_tok, p->xa, E);
        HIP_CHECK(hipGetLastError());
    }
    if (pk)
        launch_rope_table_rows(g.stream, N, pk->pos, theta_scale, m.freq_scale, (int)(m.D >> 1), p->rope);
    else
        hipLaunchKernelGGL(k_rope_table, dim3((unsigned)N), dim3(128), 0, g.stream, (const DecParams *)p->prm, theta_scale,
                           m.freq_scale, (int)(m.D >> 1), p->rope);
    HIP_CHECK(hipGetLastError());
    for (int il = 0; il < m.L; il++) {
        const DecodePlan::LW &w = p->lw[il];
        const DecodePlan::LayerNorms &ln = p->ln[il];
        __half *mk = pk ? nullptr : p->mem_k_at(il), *mv = pk ? nullptr : p->mem_v_at(il);
        // inpSA (xa) = the previous layer's inpFF + its w2 output; cur = rms_norm(inpSA) * attn_norm
        if (il == 0)
            norm_quant(p->xa, nullptr, nullptr, nullptr, ln.attn_norm, nullptr);
        else
            norm_quant(p->p_te, sp_w2 > 1 ? p->p_te + te_stride : nullptr, p->xb, p->xa, ln.attn_norm, nullptr);
        {
            const QWeight *ws[3] = {&w.wq, &w.wk, &w.wv};
            float *ds[3] = {p->p_qf, p->p_kf, p->p_vf};
            sp_qkv = gemm_multi(3, ws, ds, nbE, qkv_stride);
        }
        if (pk) {
            PQkvPostSeg a;
            a.q = p->p_qf; a.kf = p->p_kf; a.vf = p->p_vf; a.tab = p->rope;
            a.segs = pk->segs + (size_t)il * pk->n_segs; a.row_seg = pk->row_seg; a.vtiles = pk->vtiles;
            a.R = N; a.E = (int)E; a.Egqa = (int)m.Egqa; a.D = (int)m.D; a.C = m.C;
            a.skip_q = 1;  // (a pack runs the fused attention only)
            a.nb_rope = (int)(((int64_t)N * (m.Egqa / 4) + 255) / 256);
            a.part = sp_qkv > 1 ? qkv_stride : 0;
            a.vt_n = pk->n_vtiles;
            a.vt_m = (int)((m.Egqa + 63) / 64);
            Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * (E * 8.0 + m.Egqa * 12.0));
            launch_p_qkv_post_seg(g.stream, &a);
            HIP_CHECK(hipGetLastError());
        } else {
            PQkvPost a;
            a.q = p->p_qf; a.kf = p->p_kf; a.vf = p->p_vf; a.tab = p->rope; a.mem_k = mk; a.mem_v = mv;
            a.N = N; a.E = (int)E; a.Egqa = (int)m.Egqa; a.D = (int)m.D; a.n_past = m.n_past; a.C = m.C;
            a.skip_q = fused_attn ? 1 : 0;  // the fused attention kernel rotates Q while loading it
            a.nb_rope = (int)(((int64_t)N * (((fused_attn ? 0 : E) + m.Egqa) / 4) + 255) / 256);
            a.part = sp_qkv > 1 ? qkv_stride : 0;
            a.vt_n = (N + 63) / 64;
            a.vt_m = (int)((m.Egqa + 63) / 64);
            Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * (E * 8.0 + m.Egqa * 12.0));
            hipLaunchKernelGGL(k_p_qkv_post, dim3((unsigned)(a.nb_rope + a.vt_n * a.vt_m)), dim3(256), 0, g.stream, a);
            HIP_CHECK(hipGetLastError());
        }
        // the fused attention kernel hands wo its GEMM operand directly (k_p_quant4's arithmetic in its epilogue)
        // (K-quant model: a Q8_K super-block spans two heads, so the attention writes f32 and k_p_quant4 makes the operand)
        if (pk)
            prompt_attention_pack(*pk, il, p->p_qf, p->p_x16, E, m.Egqa, m.H, m.Hkv, m.D, m.C, m.kq_scale, f16d, p->rope, sp_qkv > 1 ? qkv_stride : 0);
        else
            prompt_attention(fused_attn, p->p_qf, mk, mv, p->p_mg, p->p_sc, p->p_p16, N, E, m.Egqa, m.H, m.Hkv, m.D, m.n_past, m.C, m.kq_scale,
                             fused_attn && !kq ? p->p_x16 : nullptr, f16d, fused_attn ? p->rope : nullptr, fused_attn && sp_qkv > 1 ? qkv_stride : 0);
        if (!fused_attn || kq) {
            Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 6.0);
            const int64_t n4 = (int64_t)N * E / 4;
            launch_p_quant4(kq, f16d, (const f32x4 *)p->p_mg, n4, p->p_x16);
            HIP_CHECK(hipGetLastError());
        }
        const int sp_wo = gemm(w.wo, p->p_te, nbE, te_stride);
        norm_quant(p->p_te, sp_wo > 1 ? p->p_te + te_stride : nullptr, p->xa, p->xb, ln.ffn_norm, nullptr);  // inpFF (xb) = wo output + inpSA
        {
            const QWeight *ws[2] = {&w.w1, &w.w3};
            float *ds[2] = {p->p_g1, p->p_g3};
            sp_13 = gemm_multi(2, ws, ds, nbE, g13_stride);
        }
        {
            const int64_t n4 = (int64_t)N * F / 4;
            Timed tm(GGML_HIP_KCLASS_OTHER, (double)n4 * 40.0);
            launch_p_silu_mul_quant(kq, f16d, (const f32x4 *)p->p_g1, (const f32x4 *)p->p_g3, n4, sp_13 > 1 ? g13_stride / 4 : 0, p->p_x16);
            HIP_CHECK(hipGetLastError());
        }
        sp_w2 = gemm(w.w2, p->p_te, nbF, te_stride);
    }
    if (!m.output) {  // a stage of a layer split hands the residual on: out = w2 output + inpFF
        const int64_t n4 = (int64_t)N * E / 4;
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 12.0);
        if (sp_w2 > 1) {
            hipLaunchKernelGGL(k_bin4<BIN_ADD>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, g.stream, (const f32x4 *)p->p_te,
                               (const f32x4 *)(p->p_te + te_stride), (f32x4 *)p->p_te, n4);
            HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_bin4<BIN_ADD>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, g.stream, (const f32x4 *)p->p_te,
                           (const f32x4 *)p->xb, (f32x4 *)p->stage_out, n4);
        HIP_CHECK(hipGetLastError());
        return;
    }
    norm_quant(p->p_te, sp_w2 > 1 ? p->p_te + te_stride : nullptr, p->xb, p->xa, p->norm, p->emb_out, m.out_k);
    mmq_f16_launch(m.out_k ? QT_Q8_0 : qt, p->output, p->p_x16, (float *)p->logits_out, m.V, N, nbE, true);
}
