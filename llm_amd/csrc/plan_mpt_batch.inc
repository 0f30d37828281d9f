// plan_mpt_batch.inc — the batched MPT step: one decode step of B = 2 .. 8 single-token MPT graphs of ONE model, each session at its own
// position in its own token-major caches, as one pass over the weights (plan_run.inc decode_batch_steps; option plan_mpt_batch).  It is
// plan_launch_mpt_chunk's launch sequence at N = B (plan_mpt_chunk.inc: every mat-vec on k_mmq_cols, one pass of up to 8 columns) with two
// pieces of its own, both out of mpt_batch.hip (kernels/mpt_batch.h): Wqkv's epilogue EPI_QKV_TM_BATCH places column c's K and V rows at
// BatchCols::pos[c] of session c's caches, and the batched ALiBi decode attention runs column c against that cache.  Positions and caches
// are read on the device: one captured hipGraph per (B, model, context) serves every step, those of a greedy chain included, whose
// k_argmax_next moves pos itself.  Results: rows of the plan's pool (logits_out, emb_out), as every batched step's.
// the three launches of the batched attention on H x W, H x W and B workgroups
static void mpt_batch_attention(const float *q, int64_t ldq, const BatchCols *bc, int64_t kv_off, const float *slopes, float scale, int B, int D, int H, int W,
                                int64_t E, int64_t C, float *sc, float *pmax, float *part, float *out, int8_t *lo, int8_t *hi, float *d, int *s, float *dT, int *sT,
                                bool f16d) {
    MptBatchAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = ldq; a.bc = bc; a.kv_off = kv_off; a.slopes = slopes; a.scale = scale; a.B = B; a.D = D; a.H = H; a.W = W; a.f16d = f16d ? 1 : 0;
    a.E = E; a.C = C; a.sc = sc; a.pmax = pmax; a.part = part; a.out = out; a.lo = lo; a.hi = hi; a.dq = d; a.sumq = s; a.dT = dT; a.sT = sT;
    if (launch_mpt_batch_attn(g.stream, &a, mpt_batch_attn_lds_dyn(C, B, W))) die("batched MPT step: the attention launch for head size %d failed", D);
    HIP_CHECK(hipGetLastError());
}
static void plan_launch_mpt_batch(DecodePlan *p) {
    const LlamaMatch &m = p->m;
    const int B = m.N, qt = qt_of(m.wtype);
    const bool f16d = qt_f16d(qt);
    const int64_t E = m.E, F = m.F, nbE = E / 32, nbF = F / 32;
    const QAct actE{(const i32x4 *)p->e_lo, (const i32x4 *)p->e_hi, p->e_d, p->e_s};
    const QAct actF{(const i32x4 *)p->f_lo, (const i32x4 *)p->f_hi, p->f_d, p->f_s};
    const int dn_slices = mpt_chunk_slices((int)(E / 16), (int)nbF);
    if (dn_slices < 1) die("batched MPT step: down_proj of %lld blocks a row has no K slicing", (long long)nbF);
    float *qkv = p->gate;  // the Q columns of the Wqkv product, rows 3 E apart (gate is free until up_proj)
    auto lnorm = [&](const float *x, const float *w, float *y) {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)B * E * 9.25);
        launch_mpt_lnorm_cols(g.stream, f16d, x, w, m.eps, E, B, y, p->e_lo, p->e_hi, p->e_d, p->e_s, p->e_dT, p->e_sT);
        HIP_CHECK(hipGetLastError());
    };
    {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)B * E * 4.6);
        hipLaunchKernelGGL(k_get_rows_q, dim3((unsigned)((nbE + 255) / 256), (unsigned)B), dim3(256), 0, g.stream, p->wte, (const int *)p->prm->tokens, p->xa, E);
        HIP_CHECK(hipGetLastError());
    }
    for (int il = 0; il < m.L; il++) {
        const DecodePlan::LW &w = p->lw[il];
        const DecodePlan::LayerNorms &ln = p->ln[il];
        lnorm(p->xa, ln.attn_norm, nullptr);
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.wq; a.x = actE; a.nb = nbE; a.dst = qkv; a.Egqa = E; a.C = m.C; a.D = (int)m.D;
            mpt_cols_block(qt, EPI_QKV_TM_BATCH, a, B, 3 * E, 0, (int)(3 * E), p->e_dT, p->e_sT, 1, p->bcols, p->kv_off(il));
        }
        {
            Timed tm(GGML_HIP_KCLASS_ATTN, (double)(m.n_past + 1) * B * E * 4.0 + (double)B * E * 12.0);
            mpt_batch_attention(qkv, 3 * E, p->bcols, p->kv_off(il), p->alibi, m.kq_scale, B, (int)m.D, (int)m.H, p->att_S, E, m.C, p->att_sc, p->att_pmax,
                                p->att_part, p->k_att, p->e_lo, p->e_hi, p->e_d, p->e_s, p->e_dT, p->e_sT, f16d);
        }
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.wo; a.x = actE; a.nb = nbE; a.dst = p->xb; a.res = p->xa;
            mpt_cols_block(qt, EPI_ADD, a, B, E, E, (int)E, p->e_dT, p->e_sT, 1);
        }
        lnorm(p->xb, ln.ffn_norm, nullptr);
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.w1; a.x = actE; a.nb = nbE; a.dst = p->gate;
            mpt_cols_block(qt, EPI_GELU, a, B, F, 0, (int)F, p->e_dT, p->e_sT, 1);
        }
        {
            Timed tm(GGML_HIP_KCLASS_OTHER, (double)B * F * 5.25);
            launch_quant_row(f16d, p->gate, nbF, B, p->f_lo, p->f_hi, p->f_d, p->f_s, p->f_dT, p->f_sT);
            HIP_CHECK(hipGetLastError());
        }
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.w2; a.x = actF; a.nb = nbF; a.dst = p->xa; a.res = p->xb;
            mpt_cols_block(qt, EPI_ADD, a, B, E, E, (int)E, p->f_dT, p->f_sT, dn_slices);
        }
    }
    lnorm(p->xa, p->norm, p->emb_out);
    DecMmvqArgs a;
    memset(&a, 0, sizeof(a));
    a.w[0] = p->output; a.x = actE; a.nb = nbE; a.dst = (float *)p->logits_out;
    mpt_cols_block(qt, EPI_STORE, a, B, m.V, 0, (int)m.V, p->e_dT, p->e_sT, 1);
}
