// debug_token.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip, inside its anonymous
// namespace where noted): the test hooks of what runs between two tokens — k_token_tail, the next-token kernels (argmax, samplers, requests), k_pool_admit.  At file scope.
extern "C" {
// ---- test hook: k_token_tail alone, beside k_argmax_next on the same logits (tests/test_token_tail_gpu.py) ----
// logits[V] and emb[E] (nullable) go to the device (both `misalign` floats off a 16-byte boundary: the kernel's 4-byte paths), both
// kernels start from parameters {n_past, token 0}.  Out: the two ids, the slot's logits / row (the bytes the host would be handed),
// prm_out[0..2] = n_past, token, tokens[0] as k_token_tail left them.  0, or -1 for arguments it cannot take.
int ggml_hip_debug_token_tail(const float *logits, int V, const float *emb, int E, int n_past, int misalign, int32_t *id_tail,
                              int32_t *id_argmax, float *slot_logits, float *slot_emb, int32_t *prm_out) {
    if (!logits || V < 1 || (emb && E < 1) || misalign < 0 || misalign > 3 || !id_tail || !id_argmax || !slot_logits || !prm_out) return -1;
    DebugRun run;
    const size_t lb = ((size_t)(V + 4) * 4 + 255) & ~(size_t)255, eb = ((size_t)(std::max(E, 1) + 4) * 4 + 255) & ~(size_t)255;
    const size_t emb_off = ((size_t)V * 4 + 255) & ~(size_t)255, id_off = emb_off + eb;
    char *d = run.raw(lb + eb + 1024), *slot = run.host_slot(id_off + 256);
    float *dl = (float *)d + misalign, *de = (float *)(d + lb) + misalign;
    DecParams *pa = (DecParams *)(d + lb + eb), *pb = pa + 1;
    int *ida = (int *)(pb + 1);
    DecParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.n_past = n_past;
    h2d_bulk((char *)dl, logits, (size_t)V * 4);
    if (emb) h2d_bulk((char *)de, emb, (size_t)E * 4);
    h2d_bulk((char *)pa, &hp, sizeof(hp));
    h2d_bulk((char *)pb, &hp, sizeof(hp));
    hipLaunchKernelGGL(k_argmax_next, dim3(1), dim3(1024), 0, g.stream, (const float *)dl, V, pa, (BatchCols *)nullptr, ida);
    hipLaunchKernelGGL(k_token_tail, dim3(TOKEN_TAIL_WGS), dim3(1024), 0, g.stream, (const float *)dl, V, emb ? (const float *)de : (const float *)nullptr,
                       E, pb, slot, (int)emb_off, (int)id_off, TailPrep{});
    run.back(id_argmax, ida, 4);
    run.back(&hp, pb);
    run.finish();
    prm_out[0] = hp.n_past;
    prm_out[1] = hp.token;
    prm_out[2] = hp.tokens[0];
    *id_tail = *(const int32_t *)(slot + id_off);
    memcpy(slot_logits, slot, (size_t)V * 4);
    if (emb && slot_emb) memcpy(slot_emb, slot + emb_off, (size_t)E * 4);
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
    DebugRun run;
    const int64_t nb = E / 32;
    const size_t raw_bytes = (size_t)V * nb * (size_t)blk_bytes(qt), nkv = (size_t)L * C * Egqa * 2, nsave = (size_t)L * Egqa * 4;
    char *draw = run.buf(raw_bytes, wte_raw);
    size_t off[5];
    char *dsoa = run.buf(qw_layout(qt, V, nb, off));
    relayout_launch(draw, qt, V, nb, dsoa);
    const QWeight w = qw_at(dsoa, qt, V, nb);
    char *dl = run.buf((size_t)V * 4, logits);
    char *dk = run.buf(nkv, mem_k), *dv = run.buf(nkv, mem_v);
    DecParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.n_past = hp.pos_tail[0] = hp.pos_tail[1] = n_past;
    DecParams *prm[2];
    unsigned *ep[2];
    char *drow[2], *dtab[2], *dsave[2];
    for (int i = 0; i < 2; i++) {  // 0: the tail's, 1: the reference launches'
        prm[i] = run.put(hp);
        ep[i] = run.put(epoch_in);
        drow[i] = run.buf((size_t)E * 4);
        dtab[i] = run.buf(128 * 4);
        dsave[i] = run.buf(nsave);
    }
    int *ida = (int *)run.buf(4);
    const size_t id_off = ((size_t)V * 4 + 255) & ~(size_t)255;
    char *slot = run.host_slot(id_off + 256);
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
    float *rows[2] = {row, row_ref}, *tabs[2] = {table, table_ref};
    uint32_t *eps[2] = {epoch_out, epoch_ref};
    uint16_t *saves[2] = {save, save_ref};
    for (int i = 0; i < 2; i++) {
        run.back(rows[i], drow[i], (size_t)E * 4);
        run.back(tabs[i], dtab[i], 128 * 4);
        run.back(eps[i], ep[i], 4);
        run.back(saves[i], dsave[i], nsave);
    }
    run.back(&hp, prm[0]);
    run.finish();
    prm_out[0] = hp.n_past;
    prm_out[1] = hp.token;
    prm_out[2] = hp.tokens[0];
    prm_out[3] = hp.pos_tail[0];
    prm_out[4] = hp.pos_tail[1];
    *id_out = *(const int32_t *)(slot + id_off);
    return 0;
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
    DebugRun run;
    void *host[7] = {table, reqs, scols, prm, bcols, slot_logits, slot_emb};  // in-out, each with a guard on the device
    const size_t n[7] = {sizeof(PoolTable), sizeof(SampleReqs), sizeof(SampleCols), sizeof(DecParams), sizeof(BatchCols),
                         (size_t)n_pool * V * 4, (size_t)n_pool * E * 4};
    char *d[7];
    for (int i = 0; i < 7; i++) d[i] = run.buf(n[i], host[i]);
    const float *dl = (const float *)run.buf((size_t)n_cols * V * 4, logits);
    const float *de = (const float *)run.buf((size_t)n_cols * E * 4, emb);
    launch_pool_admit(g.stream, d[0], d[1], d[2], d[3], d[4], dl, de, V, E, (float *)d[5], (float *)d[6]);
    for (int i = 0; i < 7; i++) run.back(host[i], d[i], n[i]);
    return run.finish();
}

// ---- the next-token hooks: their state is debug_run.inc's DebugToken; each is left with its table and its launch loop ----
// what all of them take: B rows of V logits (B up to the T entries: 8 with a BatchCols, 1 without), 1 .. BATCH_CHAIN_MAX_STEPS draws
static bool debug_token_args_ok(const float *logits, int B, int V, const int32_t *pos_in, const int32_t *tokens_in, int n_draws,
                                const int32_t *ids_out, const int32_t *prm_out, const int32_t *pos_out) {
    return logits && B >= 1 && B <= (pos_in ? BATCH_COLS_MAX : 1) && V >= 1 && tokens_in && ids_out && prm_out && (!pos_in || pos_out) &&
           n_draws >= 1 && n_draws <= BATCH_CHAIN_MAX_STEPS;
}
// the rings' counts as a chain's window lengths (a count beyond the ring is a full ring); false for a negative count
static bool debug_window_n(const int32_t *hist_n, int B, int32_t *wn) {
    for (int c = 0; c < B; c++) {
        if (hist_n[c] < 0) return false;
        wn[c] = std::min(hist_n[c], SAMPLER_WINDOW);
    }
    return true;
}

// ---- test hook: the kernels between two steps of the chains that stop, alone (tests/test_chain_requests_gpu.py).  debug_next_token's
// shape with a request per column; a budget here is the number of draws, 0 .. n_draws. ----
int ggml_hip_debug_next_token_req(const float *logits, int B, int V, const ggml_hip_sampler_chain *const *chains, const ggml_hip_chain_end *ends,
                                  int n_past_in, const int32_t *pos_in, const int32_t *tokens_in, int32_t *hist, int32_t *hist_n, uint64_t *rng,
                                  float *mu, int n_draws, int32_t *ids_out, int32_t *prm_out, int32_t *pos_out, int32_t *n_drawn,
                                  int32_t *ended_by) {
    if (!debug_token_args_ok(logits, B, V, pos_in, tokens_in, n_draws, ids_out, prm_out, pos_out)) return -1;
    if (!chains || !ends || !hist || !hist_n || !rng || !n_drawn || !ended_by) return -1;
    int32_t wn[BATCH_COLS_MAX];
    if (!debug_window_n(hist_n, B, wn)) return -1;
    std::vector<int32_t> count((size_t)B), why((size_t)B);
    ChainRequests req = {chains, ends, hist, wn, rng, mu, count.data(), why.data(), 0, {0, 0, 0, 0}};
    if (!chain_requests_ok(req, B, V, 0, n_draws)) return -1;
    DebugRun run;
    DebugToken tok(pos_in ? pos_in[0] : n_past_in, pos_in, tokens_in, hist, hist_n);
    SampleReqs ht;
    chain_req_table(ht, req, B);
    tok.state_in(ht.back.state, rng, mu);
    tok.upload(run, logits, B, V, n_draws);
    char *dt = (char *)run.put(ht);
    for (int i = 0; i < n_draws; i++) launch_next_token_req(g.stream, req.n_class, tok.dl, V, tok.dp, tok.db, tok.ds, dt, tok.dids + (size_t)i * B);
    run.back(&ht.back, dt, sizeof(ht.back));
    tok.finish(run, ids_out, prm_out, pos_out, hist, hist_n);
    tok.state_out(ht.back.state, rng, mu);
    for (int c = 0; c < B; c++) {
        n_drawn[c] = ht.back.n_drawn[c];
        ended_by[c] = ht.back.ended_by[c];
    }
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
    int stages = SAMPLE_DEFAULT;
    if (!debug_token_args_ok(logits, B, V, pos_in, tokens_in, n_draws, ids_out, prm_out, pos_out)) return -1;
    if (params) {
        int32_t wn[BATCH_COLS_MAX];
        if (!hist || !hist_n || !rng || !debug_window_n(hist_n, B, wn)) return -1;
        const BatchSample smp = {params, hist, wn, rng, mu};
        if (!batch_sample_ok(smp, B, V)) return -1;
        stages = smp.stages();
    } else {
        hist = hist_n = nullptr;  // (no sampler: no rings)
    }
    DebugRun run;
    DebugToken tok(n_past, pos_in, tokens_in, hist, hist_n);
    SampleHead hh;
    memset(&hh, 0, sizeof(hh));
    if (params) {
        sample_cols_params(tok.hs, *params);
        sample_head_bias(hh, *params);
        tok.state_in(hh.state, rng, mu);
    }
    tok.upload(run, logits, B, V, n_draws);
    unsigned long long *dr = (unsigned long long *)&run.put(hh)->state;
    for (int i = 0; i < n_draws; i++) {
        if (params) launch_sample_next(g.stream, B, tok.dl, V, tok.dp, tok.db, tok.ds, dr, tok.dids + (size_t)i * B, stages);
        else hipLaunchKernelGGL(k_argmax_next, dim3((unsigned)B), dim3(1024), 0, g.stream, tok.dl, V, tok.dp, tok.db, tok.dids + (size_t)i * B);
    }
    if (params) run.back(&hh.state, dr, sizeof(hh.state));
    tok.finish(run, ids_out, prm_out, pos_out, hist, hist_n);
    if (params) tok.state_out(hh.state, rng, mu);
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

}  // extern "C"
