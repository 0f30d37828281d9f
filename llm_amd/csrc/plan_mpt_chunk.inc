// plan_mpt_chunk.inc — the MPT chunk plan: an evaluation of 2 .. MULTI_MAX_N tokens of an MPT graph (LlamaMatch::mpt, N > 1, !prompt;
// option plan_mpt_chunk) — the chunks InferenceSession::feed_prompt feeds at its default n_batch = 8 — captured as one linear hipGraph
// per N and replayed: n_past is read from prm on the device.  Per layer (mat-vecs once per pass of 8 columns):
//   k_lnorm_quant_cols -> Wqkv (EPI_QKV_TM: Q as f32, K and V into the token-major caches) -> the position-split chunk attention (three
//   launches: scores, softmax + V.P, merge + Q8) -> out_proj + residual (EPI_ADD) -> k_lnorm_quant_cols -> up_proj (EPI_GELU) ->
//   k_quant_row -> down_proj + residual
// then the final LayerNorm (with the f32 rows of the embedding result) and the tied lm_head (EPI_STORE) over all N rows.  Every mat-vec is
// k_mmq_cols in passes of 8 columns, as plan_launch_chunk's `block` runs them: the two plain epilogues out of the main code object, the
// MPT ones and the attention (kernels/mpt_chunk.h) out of mpt_chunk.hip.  A matrix whose K exceeds the kernel's LDS staging (down_proj of
// MPT-7B: 512 blocks a row, 160 KiB) runs as mpt_chunk_slices consecutive EPI_ADD_KS launches over equal K slices: the first adds the
// residual, each next one adds the previous launch's dst in place.  The reference's re-copy of the V cache is matched and never made.
// Results: rows of the plan's pool (logits_out, emb_out), as the MPT decode plan's.
static void mpt_cols_launch(int qt, int epi, ColsArgs c, int M_total) {
    c.ngroups = M_total / 16;
    const ColsShape sh = cols_shape(c.ngroups, 1, (int)c.d.nb);
    if (!sh.G) die("MPT chunk plan: a launch the matcher's preconditions exclude (%d rows of %lld blocks)", M_total, (long long)c.d.nb);
    c.gq = c.ngroups / sh.G;
    c.gr = c.ngroups % sh.G;
    if (epi == EPI_ADD)
        with_qt(qt, [&](auto QT) { launch_cols<CT(QT), EPI_ADD>(c, M_total); });
    else if (epi == EPI_STORE)
        with_qt(qt, [&](auto QT) { launch_cols<CT(QT), EPI_STORE>(c, M_total); });
    else if (epi == EPI_QKV_TM_BATCH ? launch_mpt_batch_cols(g.stream, qt, &c, sh.G, sh.lds) : launch_mpt_cols(g.stream, qt, epi, &c, sh.G, sh.lds))
        die("MPT chunk plan: no k_mmq_cols instantiation for type %d, epilogue %d", qt, epi);
    HIP_CHECK(hipGetLastError());
}
// One mat-vec of the chunk over N columns: passes of 8 columns, `slices` equal K slices each (1 but for EPI_ADD).  a: the whole-chunk
// arguments (x, dst, res: row 0; nb: blocks of a whole row), dT / sT: the [block][8] tables, one per pass; bc, kv_off: EPI_QKV_TM_BATCH's
static void mpt_cols_block(int qt, int epi, const DecMmvqArgs &a, int N, int64_t ldd, int64_t ldr, int M_total, const float *dT, const int *sT, int slices,
                           const BatchCols *bc = nullptr, int64_t kv_off = 0) {
    const int64_t nb = a.nb, nbs = nb / slices;
    for (int c0 = 0; c0 < N; c0 += 8) {
        for (int s = 0; s < slices; s++) {
            ColsArgs c;
            memset(&c, 0, sizeof(c));
            const int64_t b0 = s * nbs;
            c.d = a; c.ldd = ldd; c.ldr = ldr;
            c.ncols = std::min(8, N - c0);
            c.col0 = c0;
            c.d.nb = nbs;
            c.d.x.lo = a.x.lo + c0 * nb + b0;
            c.d.x.hi = a.x.hi + c0 * nb + b0;
            c.d.x.d = a.x.d + c0 * nb + b0;
            c.d.x.sum = a.x.sum + c0 * nb + b0;
            c.d.dst = a.dst + c0 * ldd;
            if (a.res) c.d.res = (s == 0 ? a.res + c0 * ldr : c.d.dst);
            if (s > 0) c.ldr = ldd;
            c.dxT = dT + ((int64_t)(c0 / 8) * nb + b0) * 8;
            c.sxT = sT + ((int64_t)(c0 / 8) * nb + b0) * 8;
            c.hot = g.hot_line;
            c.bc = bc; c.kv_off = kv_off;
            if (slices > 1) {  // the slice's first block of every weight row; the rows stay QWeight::nb blocks apart
                QWeight &w = c.d.w[0];
                w.qs += b0 * 16;
                if (w.qs2) w.qs2 += b0 * 16;
                if (w.qh) w.qh += b0;
                w.d += b0;
                if (w.m) w.m += b0;
            }
            Timed tm(GGML_HIP_KCLASS_MMVQ, (double)M_total * nbs * (double)blk_bytes(qt));
            mpt_cols_launch(qt, slices > 1 ? EPI_ADD_KS : epi, c, M_total);
        }
    }
}
// the three launches of the position-split chunk attention (kernels/mpt_chunk.h) on H x S, H x S and N workgroups
static void mpt_chunk_attention(const float *q, int64_t ldq, const void *mk, const void *mv, const DecParams *prm, const float *slopes, float scale, int N, int D,
                                int H, int S, int64_t E, int64_t C, float *sc, float *pmax, float *part, float *out, int8_t *lo, int8_t *hi, float *d, int *s,
                                float *dT, int *sT, bool f16d) {
    MptChunkAttnArgs a;
    memset(&a, 0, sizeof(a));
    const size_t chunk = attn_split_chunk_max(C, S);
    a.q = q; a.ldq = ldq; a.mem_k = (const __half *)mk; a.mem_v = (const __half *)mv; a.prm = prm; a.slopes = slopes; a.scale = scale;
    a.N = N; a.D = D; a.S = S; a.f16d = f16d ? 1 : 0; a.E = E; a.C = C; a.sc = sc; a.pmax = pmax; a.part = part; a.out = out;
    a.lo = lo; a.hi = hi; a.dq = d; a.sumq = s; a.dT = dT; a.sT = sT; a.rb = mpt_chunk_attn_row_bytes(chunk);
    if (launch_mpt_chunk_attn(g.stream, &a, H, mpt_chunk_attn_lds(chunk))) die("MPT chunk plan: the attention launch for head size %d failed", D);
    HIP_CHECK(hipGetLastError());
}
static void plan_launch_mpt_chunk(DecodePlan *p) {
    const LlamaMatch &m = p->m;
    const int N = m.N, qt = qt_of(m.wtype);
    const bool f16d = qt_f16d(qt);
    const int64_t E = m.E, F = m.F, nbE = E / 32, nbF = F / 32;
    const QAct actE{(const i32x4 *)p->e_lo, (const i32x4 *)p->e_hi, p->e_d, p->e_s};
    const QAct actF{(const i32x4 *)p->f_lo, (const i32x4 *)p->f_hi, p->f_d, p->f_s};
    const int dn_slices = mpt_chunk_slices((int)(E / 16), (int)nbF);
    if (dn_slices < 1) die("MPT chunk plan: down_proj of %lld blocks a row has no K slicing", (long long)nbF);
    float *qkv = p->gate;  // the Q columns of the Wqkv product, rows 3 E apart as the attention reads them (gate is free until up_proj)
    auto lnorm = [&](const float *x, const float *w, float *y) {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 9.25);
        launch_mpt_lnorm_cols(g.stream, f16d, x, w, m.eps, E, N, y, p->e_lo, p->e_hi, p->e_d, p->e_s, p->e_dT, p->e_sT);
        HIP_CHECK(hipGetLastError());
    };
    auto quant = [&](const float *x, int64_t nb, int8_t *lo, int8_t *hi, float *d, int *s, float *dT, int *sT) {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * nb * 32 * 5.25);
        launch_quant_row(f16d, x, nb, N, lo, hi, d, s, dT, sT);
        HIP_CHECK(hipGetLastError());
    };
    {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 4.6);
        hipLaunchKernelGGL(k_get_rows_q, dim3((unsigned)((nbE + 255) / 256), (unsigned)N), dim3(256), 0, g.stream, p->wte, (const int *)p->prm->tokens, p->xa, E);
        HIP_CHECK(hipGetLastError());
    }
    for (int il = 0; il < m.L; il++) {
        const DecodePlan::LW &w = p->lw[il];
        const DecodePlan::LayerNorms &ln = p->ln[il];
        lnorm(p->xa, ln.attn_norm, nullptr);
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.wq; a.x = actE; a.nb = nbE; a.dst = qkv; a.prm = p->prm; a.mem_k = p->mem_k_at(il); a.mem_v = p->mem_v_at(il);
            a.Egqa = E; a.C = m.C; a.D = (int)m.D;
            mpt_cols_block(qt, EPI_QKV_TM, a, N, 3 * E, 0, (int)(3 * E), p->e_dT, p->e_sT, 1);
        }
        {
            Timed tm(GGML_HIP_KCLASS_ATTN, (double)(m.n_past + N) * E * 4.0 + (double)N * E * 12.0);
            mpt_chunk_attention(qkv, 3 * E, p->mem_k_at(il), p->mem_v_at(il), p->prm, p->alibi, m.kq_scale, N, (int)m.D, (int)m.H, p->att_S, E, m.C, p->att_sc,
                                p->att_pmax, p->att_part, p->k_att, p->e_lo, p->e_hi, p->e_d, p->e_s, p->e_dT, p->e_sT, f16d);
        }
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.wo; a.x = actE; a.nb = nbE; a.dst = p->xb; a.res = p->xa;
            mpt_cols_block(qt, EPI_ADD, a, N, E, E, (int)E, p->e_dT, p->e_sT, 1);
        }
        lnorm(p->xb, ln.ffn_norm, nullptr);
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.w1; a.x = actE; a.nb = nbE; a.dst = p->gate;
            mpt_cols_block(qt, EPI_GELU, a, N, F, 0, (int)F, p->e_dT, p->e_sT, 1);
        }
        quant(p->gate, nbF, p->f_lo, p->f_hi, p->f_d, p->f_s, p->f_dT, p->f_sT);
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.w2; a.x = actF; a.nb = nbF; a.dst = p->xa; a.res = p->xb;
            mpt_cols_block(qt, EPI_ADD, a, N, E, E, (int)E, p->f_dT, p->f_sT, dn_slices);
        }
    }
    lnorm(p->xa, p->norm, p->emb_out);
    DecMmvqArgs a;
    memset(&a, 0, sizeof(a));
    a.w[0] = p->output; a.x = actE; a.nb = nbE; a.dst = (float *)p->logits_out;
    mpt_cols_block(qt, EPI_STORE, a, N, m.V, 0, (int)m.V, p->e_dT, p->e_sT, 1);
}
