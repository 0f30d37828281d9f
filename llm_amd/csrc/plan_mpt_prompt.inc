// plan_mpt_prompt.inc — the MPT prompt plan: an evaluation of N >= mmq_min tokens of an MPT graph (LlamaMatch::mpt && prompt; option
// plan_mpt_prompt) as nine launches per layer, launched eagerly as plan_launch_prompt is:
//   k_p_lnorm_quant -> Wqkv GEMM -> k_p_qkv_post_tm -> k_p_attn_alibi -> out_proj GEMM -> k_p_lnorm_quant (+ residual) -> up_proj GEMM ->
//   k_p_gelu_quant -> down_proj GEMM
// (k_p_attn_alibi_stream in k_p_attn_alibi's place for rows behind its LDS fit: option mpt_attn_stream)
// then the final LayerNorm and the tied lm_head GEMM over all N rows.  The GEMMs are the executor's (mmq_f16_launch_multi on the resident
// f16 copies, the K split of mmq_auto_splits per matrix); a split GEMM stores two partials `stride` floats apart and its consumer adds
// them, as in the LLaMA prompt plan: no memset, no atomics.  Everything between them is kernels/mpt_prompt.h (mpt_prompt.hip).  The
// reference's re-copy of the V cache (cpy(permute(V, 1, 2, 0, 3))) is matched and never made: the attention reads token-major V.

// the attention launch of one layer; x16 == nullptr: `out` (f32 merged heads) is written instead (the test hook); force_stream: the
// streaming kernel also where the rows fit
static void mpt_prompt_attention(const float *qkv, int64_t q_part, const void *mk, const void *mv, const float *slopes, float *out, _Float16 *x16,
                                 bool f16d, int N, int64_t E, int64_t H, int64_t D, int n_past, int64_t C, float scale, bool force_stream) {
    const int64_t T = (int64_t)n_past + N;
    const bool stream = force_stream || !mpt_attn_queries(D, T);
    const int QR = stream ? 32 : mpt_attn_queries(D, T);
    MptAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.qkv = qkv; a.q_part = q_part; a.mem_k = mk; a.mem_v = mv; a.slopes = slopes; a.out = out; a.x16 = x16;
    a.N = N; a.E = (int)E; a.H = (int)H; a.n_past = n_past; a.f16d = f16d ? 1 : 0;
    a.row_bytes = mpt_attn_row_bytes(T);
    a.C = C; a.scale = scale;
    const size_t lds = stream ? mpt_attn_stream_lds(D) : mpt_attn_lds(QR, D, T);
    const int ntile = (N + QR - 1) / QR;
    // two workgroups per CU where the LDS allows and there are more workgroups than CUs: the first num_cus take the longest tiles, the
    // rest come shortest first (k_p_attn's dealing, plan_prompt.inc prompt_attention)
    const bool two_per_cu = 2 * (lds + 1024) <= 160 * 1024 && (int64_t)ntile * H > g.num_cus;
    a.r1 = two_per_cu ? std::max(1, std::min(ntile, (int)(g.num_cus / H))) : ntile;
    Timed tm(GGML_HIP_KCLASS_ATTN, (double)T * E * (stream ? 8.0 : 4.0) + (double)N * E * 6.0);  // (the streaming kernel reads K three times)
    if (stream ? launch_mpt_attn_alibi_stream(g.stream, (int)D, &a, (unsigned)(ntile * H)) : launch_mpt_attn_alibi(g.stream, (int)D, QR, &a, (unsigned)(ntile * H), lds))
        die("MPT prompt plan: the attention launch for head size %lld failed", (long long)D);
    HIP_CHECK(hipGetLastError());
}

static void plan_launch_mpt_prompt(DecodePlan *p) {
    const LlamaMatch &m = p->m;
    const int N = m.N, qt = qt_of(m.wtype);
    const bool f16d = qt_f16d(qt);
    const int64_t E = m.E, F = m.F, nbE = E / 32, nbF = F / 32;
    const size_t R = (size_t)N;
    // transient buffers from the executor's workspace (rewound at the start of every graph); GEMM outputs have room for two partials
    float *te = (float *)ws_alloc(2 * R * E * 4);
    float *qkv = (float *)ws_alloc(2 * R * 3 * E * 4);
    float *up = (float *)ws_alloc(2 * R * F * 4);
    _Float16 *x16 = (_Float16 *)ws_alloc(R * F * 2);
    if (p->w16_gen != g.w16_gen) {  // the f16 copies are a cache (dev_malloc may have released them, also just above)
        auto w16_of = [](const ggml_tensor *t) { DevTensor *e = plan_rec(t); return e ? e->qw.w16 : nullptr; };
        for (int il = 0; il < m.L; il++)
            for (int i = 0; i < LAYER_MATS; i++) p->lw[il].at(i).w16 = w16_of(m.layers[il].at(i));
        p->output.w16 = w16_of(m.output);
        p->w16_gen = g.w16_gen;
    }
    const int tiles_n = (N + MMQ_TN - 1) / MMQ_TN;
    const int64_t te_stride = (int64_t)N * E, qkv_stride = (int64_t)N * 3 * E, up_stride = (int64_t)N * F;
    auto gemm = [&](const QWeight &w, float *dst, int64_t nb, int64_t stride) {  // returns the K splits used
        const MmqSegHost seg{w, dst, w.M};
        const int sp = mmq_auto_splits((int)((w.M + MMQ_TM - 1) / MMQ_TM) * tiles_n, nb, true);
        mmq_f16_launch_multi(qt, 1, &seg, x16, N, nb, true, sp, false, stride);
        return sp;
    };
    // [x (+ x2) + r -> xsum ->] norm * w -> Q8 -> the f16 operand
    auto lnorm_quant = [&](const float *x, const float *x2, const float *r, float *xsum, const float *w) {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * (r ? 18.0 : 6.0));
        launch_mpt_lnorm_quant(g.stream, f16d, x, x2, r, xsum, w, m.eps, E, N, x16);
        HIP_CHECK(hipGetLastError());
    };
    {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 4.6);
        hipLaunchKernelGGL(k_get_rows_q, dim3((unsigned)((nbE + 255) / 256), (unsigned)N), dim3(256), 0, g.stream, p->wte, (const int *)p->p_tok, p->xa, E);
        HIP_CHECK(hipGetLastError());
    }
    int sp_dn = 1;
    for (int il = 0; il < m.L; il++) {
        const DecodePlan::LW &w = p->lw[il];
        const DecodePlan::LayerNorms &ln = p->ln[il];
        // inpSA (xa) = the previous layer's inpFF (xb) + its down_proj output
        if (il == 0)
            lnorm_quant(p->xa, nullptr, nullptr, nullptr, ln.attn_norm);
        else
            lnorm_quant(te, sp_dn > 1 ? te + te_stride : nullptr, p->xb, p->xa, ln.attn_norm);
        const int sp_qkv = gemm(w.wq, qkv, nbE, qkv_stride);
        {
            Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 12.0);
            launch_mpt_qkv_post_tm(g.stream, qkv, sp_qkv > 1 ? qkv_stride : 0, p->mem_k_at(il), p->mem_v_at(il), N, E, m.n_past);
            HIP_CHECK(hipGetLastError());
        }
        mpt_prompt_attention(qkv, sp_qkv > 1 ? qkv_stride : 0, p->mem_k_at(il), p->mem_v_at(il), p->alibi, nullptr, x16, f16d, N, E, m.H, m.D, m.n_past,
                             m.C, m.kq_scale, g.opt_mpt_attn_stream == 2);
        const int sp_o = gemm(w.wo, te, nbE, te_stride);
        lnorm_quant(te, sp_o > 1 ? te + te_stride : nullptr, p->xa, p->xb, ln.ffn_norm);  // inpFF (xb) = out_proj output + inpSA
        const int sp_up = gemm(w.w1, up, nbE, up_stride);
        {
            const int64_t n4 = (int64_t)N * F / 4;
            Timed tm(GGML_HIP_KCLASS_OTHER, (double)n4 * 24.0);
            launch_mpt_gelu_quant(g.stream, f16d, up, n4, sp_up > 1 ? up_stride / 4 : 0, x16);
            HIP_CHECK(hipGetLastError());
        }
        sp_dn = gemm(w.w2, te, nbF, te_stride);
    }
    lnorm_quant(te, sp_dn > 1 ? te + te_stride : nullptr, p->xb, p->xa, p->norm);
    mmq_f16_launch(qt, p->output, x16, (float *)p->logits_out, m.V, N, nbE, true);
}
