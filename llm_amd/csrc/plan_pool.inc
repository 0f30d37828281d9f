// plan_pool.inc — ggml_hip_decode_pool_requests: the batched chain that stops (plan_run.inc decode_batch_steps with a ChainRequests)
// over a POOL of requests, more of them than the step has columns.  Entries 0 .. n_cols - 1 start in the columns, the rest wait in
// order; behind the tail of every step k_pool_admit (kernels/pool_admit.h) hands every free column (kernels/pool_rule.h) to the next
// waiting request on the device, and the same captured graph is replayed.  The host stages every request's tables once, and reads
// the pool's head back behind every group of steps as the chains that stop read their live flags.
struct PoolResults {
    int32_t *col, *first_step, *n_evaluated, *ended_by, *steps_run;
};
// request r's staged entry: what chain_req_table writes for a column, kept per request
static void pool_in_fill(PoolIn &d, const ChainRequests &r, int i, int32_t token, int pos, __half *mk, __half *mv) {
    SampleReqs one;  // (one place knows how a request becomes table entries: chain_req_table, here on column 0)
    ChainRequests q = r;
    const ggml_hip_sampler_chain *chain = r.chains[i];
    uint64_t rng = r.rng ? r.rng[i] : 0;
    float mu = r.mu ? r.mu[i] : 0.0f;
    q.chains = &chain;
    q.ends = r.ends + i;
    q.rng = &rng;
    q.mu = r.mu ? &mu : nullptr;
    chain_req_table(one, q, 1);
    memset(&d, 0, sizeof(d));
    d.mem_k = mk;
    d.mem_v = mv;
    d.rng = one.back.state.rng[0];
    d.mu = one.back.state.mu[0];
    d.token = token;
    d.pos = pos;
    d.max_draws = one.max_draws[0];
    d.n_stop = one.n_stop[0];
    d.cls = chain_req_class(chain);
    memcpy(d.stop_id, one.stop_id[0], sizeof(d.stop_id));
    if (r.windows && r.window_n) {
        d.hist_n = r.window_n[i];
        for (int j = 0; j < r.window_n[i]; j++) d.hist[j] = r.windows[(size_t)i * SAMPLER_WINDOW + j];
    }
    d.prm = one.prm[0];
    d.bias = one.bias[0];
}
// the pool's head behind a group of steps: into pinned memory of parity q, an event behind it (chain_live_queue's way)
static void pool_head_queue(DecodePlan *p, int q) {
    if (!g.pool_pin) {
        HIP_CHECK(hipHostMalloc((void **)&g.pool_pin, 2 * sizeof(PoolHead), hipHostMallocDefault));
        for (int i = 0; i < 2; i++) HIP_CHECK(hipEventCreateWithFlags(&g.pool_ev[i], hipEventDisableTiming));
    }
    HIP_CHECK(hipMemcpyAsync(g.pool_pin + q, p->pool_tab, sizeof(PoolHead), hipMemcpyDeviceToHost, g.stream));
    HIP_CHECK(hipEventRecord(g.pool_ev[q], g.stream));
}
// The host's "done" test.  `busy` is what the last admission of the group found: a column live, or a request waiting.  The group's
// last step was enqueued BEHIND that admission, so a column that ended in the last tail, or a request admitted born ended, has had
// its last evaluation: no column is live, none awaits its last evaluation and the cursor is at the end exactly when busy is 0.
static bool pool_busy(int q) {
    HIP_CHECK(hipEventSynchronize(g.pool_ev[q]));
    return g.pool_pin[q].busy != 0 || g.pool_pin[q].cursor < g.pool_pin[q].n_pool;
}

static int decode_pool_requests(ggml_cgraph *const *graphs, int n_pool, int B, int n_steps, int32_t *out_ids, ChainRequests &req,
                                const PoolResults &res) {
    ensure_init();
    finish_pending();
    spec_cancel();
    g.chain_plan = nullptr;
    res_settle();
    if (g.prep) g.prep->gr = nullptr;
    if (!g.opt_plan || !g.opt_plan_batch || !g.opt_plan_batch_chain || !g.opt_plan_batch_pool) return -1;
    if (req.any_sampled(n_pool) && !g.opt_plan_batch_sample) return -1;
    const uint64_t t0 = now_ns();
    // every graph up front, as decode_batch_steps checks its columns: nothing runs unless the whole pool can
    std::vector<LlamaMatch> ms((size_t)n_pool);
    std::vector<uint64_t> sig;
    for (int r = 0; r < n_pool; r++) {
        LlamaMatch &m = ms[(size_t)r];
        if (!match_llama_decode(graphs[r], m)) return -1;
        if (m.kquant && !(g.opt_plan_batch_k && g.opt_plan_k)) return -1;
        if (m.N != 1 || m.prompt || !m.wte || !m.output || !m.embd || !m.logits || !m.embedding) return -1;
        const int room = std::max(1, std::min(n_steps, (int)req.ends[r].budget));  // a request's budget against its own session's room
        if (m.n_past + room > m.C || (qt_of(m.wtype) < 0 && !m.f16w && !m.kquant)) return -1;
        for (const ggml_tensor *t : {m.memory_k, m.memory_v}) {
            const DevTensor *e = (const DevTensor *)t->extra;
            if (e && e->magic == 0x48495054 && e->slot != g_cur_slot()) return -1;
        }
        const int32_t tok = ((const int32_t *)m.embd->data)[0];
        if (tok < 0 || tok >= m.wte->ne[1]) return -1;
    }
    if (attn_decode_lds(ms[0].C, ms[0].D) > ATTN_DECODE_LDS_MAX || (!ms[0].f16w && !ms[0].kquant && !multi_shape_ok(ms[0], B))) return -1;
    if (!chain_requests_ok(req, n_pool, ms[0].V, 1, n_steps)) return -1;
    ws_reset();
    for (int r = 0; r < n_pool; r++) {
        const LlamaMatch &m = ms[(size_t)r];
        if (!plan_weights_resident(m)) {
            upload_inputs(graphs[r]);
            if (!plan_weights_resident(m)) return -1;
        }
        std::vector<uint64_t> s = plan_signature(m, false);
        if (r == 0) sig = std::move(s);
        else if (s != sig) return -1;
    }
    std::vector<__half *> mk((size_t)n_pool), mv((size_t)n_pool);
    for (int r = 0; r < n_pool; r++) {
        mk[(size_t)r] = (__half *)dev_ptr(ms[(size_t)r].memory_k);
        mv[(size_t)r] = (__half *)dev_ptr(ms[(size_t)r].memory_v);
        for (int d = 0; d < r; d++)
            if (mk[(size_t)d] == mk[(size_t)r] || mv[(size_t)d] == mv[(size_t)r]) return -1;  // one session twice in the pool
    }
    LlamaMatch mb = ms[0];
    mb.N = B;
    mb.n_past = 0;
    sig[0] = (uint64_t)B;
    sig.push_back(0x6261746368ull);  // the batched step's plan (decode_batch_steps): the same plan, the same captured graph
    DecodePlan *p = find_or_build_plan(mb, sig, true);
    if (!p->scols || !p->bcols) return -1;
    for (int c = 0; c < B; c++) mb.n_past = std::max(mb.n_past, ms[(size_t)c].n_past);
    p->m.n_past = mb.n_past;
    const uint64_t t1 = now_ns();
    const size_t V = (size_t)ms[0].V, E = (size_t)ms[0].E;
    DecParams hp;
    BatchCols hb;
    memset(&hp, 0, sizeof(hp));
    memset(&hb, 0, sizeof(hb));
    std::vector<PoolTable> pt_(1);  // (64 KB: not on the stack)
    PoolTable *pt = pt_.data();
    memset(pt, 0, sizeof(PoolTable));
    int n_of_class[SAMPLE_CLASSES] = {0, 0, 0, 0};
    for (int r = 0; r < n_pool; r++) {
        const LlamaMatch &m = ms[(size_t)r];
        pool_in_fill(pt->in[r], req, r, ((const int32_t *)m.embd->data)[0], m.n_past, mk[(size_t)r], mv[(size_t)r]);
        n_of_class[pt->in[r].cls]++;
        PoolOut &o = pt->out[r];
        o.rng = pt->in[r].rng;
        o.mu = pt->in[r].mu;
        o.col = r < B ? r : -1;
    }
    for (int c = 0; c < BATCH_COLS_MAX; c++) pt->head.owner[c] = c < B ? c : -1;
    for (int c = 0; c < B; c++) {
        hp.tokens[c] = pt->in[c].token;
        hb.pos[c] = pt->in[c].pos;
        hb.mem_k[c] = mk[(size_t)c];
        hb.mem_v[c] = mv[(size_t)c];
        pt->head.was_live[c] = pt->in[c].max_draws > 0;
    }
    hp.n_past = hb.pos[0];
    hp.token = hp.tokens[0];
    pt->head.cursor = B;
    pt->head.n_pool = n_pool;
    pt->head.n_cols = B;
    h2d_small((char *)p->prm, &hp, sizeof(hp));
    h2d_small((char *)p->bcols, &hb, sizeof(hb));
    if (!p->pool_tab) HIP_CHECK(hipMalloc((void **)&p->pool_tab, sizeof(PoolTable)));
    const size_t rows = (size_t)n_pool * (V + E);
    if (p->pool_rows_cap < rows) {
        if (p->pool_rows) HIP_CHECK(hipFree(p->pool_rows));
        HIP_CHECK(hipMalloc((void **)&p->pool_rows, rows * 4));
        p->pool_rows_cap = rows;
    }
    float *slot_logits = p->pool_rows, *slot_emb = p->pool_rows + (size_t)n_pool * V;
    const auto step = [&] {
        if (g.opt_graph && !g.timing.on) {
            HIP_CHECK(hipGraphLaunch(plain_graph(p, AV_SHORT, [&] { plan_launch_batch(p); }).exec, g.stream));
            p->replays++;
        } else {
            plan_launch_batch(p);
        }
    };
    step();
    // the first n_cols requests' table as the batched chain's; the host's n_class[] is each class's upper bound, min(columns, pool
    // entries of that class): the surplus workgroups return on the device-side n_list check
    ChainRequests first = req;
    chain_req_fill(p, first, B, std::max(1, (n_steps - 1) * B));
    int n_class[SAMPLE_CLASSES];
    bool busy = n_pool > B;
    for (int s = 0; s < SAMPLE_CLASSES; s++) n_class[s] = std::min(B, n_of_class[s]);
    for (int c = 0; c < B; c++) busy = busy || pt->in[c].max_draws > 0;
    h2d_small(p->pool_tab, pt, sizeof(PoolTable));
    const int G = std::max(1, g.opt_chain_group);
    int i = 1, pending = -1, q = 0;
    while (i < n_steps && busy) {
        for (const int e = std::min(n_steps, (i / G + 1) * G); i < e; i++) {
            launch_next_token_req(g.stream, n_class, (const float *)p->logits_out, (int)V, p->prm, p->bcols, p->scols, p->chain_req,
                                  p->chain_out + (size_t)(i - 1) * B);
            launch_pool_admit(g.stream, p->pool_tab, p->chain_req, p->scols, p->prm, p->bcols, (const float *)p->logits_out, p->emb_out, (int)V,
                              (int)E, slot_logits, slot_emb);
            step();
        }
        pool_head_queue(p, q);
        if (pending >= 0) busy = pool_busy(pending);
        pending = q;
        q ^= 1;
    }
    const int launched = i;
    HIP_CHECK(hipGetLastError());
    SampleReqBack back;
    d2h_queue(&back, (const char *)p->chain_req, sizeof(back));
    d2h_queue(pt, p->pool_tab, offsetof(PoolTable, in));  // the head and every request's back record
    if (launched > 1) d2h_queue(out_ids, (const char *)p->chain_out, (size_t)(launched - 1) * B * 4);
    d2h_finish();
    for (size_t k = (size_t)(launched - 1) * B; k < (size_t)(n_steps - 1) * B; k++) out_ids[k] = -1;  // rows never launched
    p->m.n_past = mb.n_past + launched - 1;
    // every request that ran: its results where an evaluation of its graph alone leaves them, from its retire slot or from its column
    int steps_run = 0, admitted = 0;
    uint64_t evaluated = 0;
    for (int r = 0; r < n_pool; r++) {
        PoolOut &o = pt->out[r];
        res.col[r] = -1;
        res.first_step[r] = res.n_evaluated[r] = res.ended_by[r] = 0;
        if (o.col < 0 || o.col >= B) continue;  // it never left the queue: untouched
        const int c = o.col;
        if (!o.retired) {
            if (pt->head.owner[c] != r) die("request pool: request %d neither retired nor in column %d", r, c);
            o.rng = back.state.rng[c];
            o.mu = back.state.mu[c];
            o.n_drawn = back.n_drawn[c];
            o.ended_by = back.ended_by[c];
        }
        const LlamaMatch &m = ms[(size_t)r];
        const char *lrow = o.retired ? (const char *)(slot_logits + (size_t)r * V) : p->logits_out + (size_t)c * V * 4;
        const char *erow = o.retired ? (const char *)(slot_emb + (size_t)r * E) : (const char *)p->emb_out + (size_t)c * E * 4;
        if (m.logits->backend == GGML_BACKEND_CPU) d2h_queue(m.logits->data, lrow, V * 4);
        else HIP_CHECK(hipMemcpyAsync(dev_ptr(m.logits), lrow, V * 4, hipMemcpyDeviceToDevice, g.stream));
        HIP_CHECK(hipMemcpyAsync(dev_ptr(m.embedding), erow, E * 4, hipMemcpyDeviceToDevice, g.stream));
        if (m.embedding->data) d2h_queue(m.embedding->data, erow, E * 4);
        if (req.chains[r]) {
            req.rng[r] = o.rng;
            if (req.mu && req.chains[r]->mirostat == 2) req.mu[r] = o.mu;
        }
        res.col[r] = c;
        res.first_step[r] = o.first_step;
        res.n_evaluated[r] = o.n_drawn + 1;
        res.ended_by[r] = o.ended_by;
        if (o.ended_by == CHAIN_END_STOP) g.stat_chain_stopped_columns++;
        steps_run = std::max(steps_run, o.first_step + o.n_drawn + 1);
        evaluated += (uint64_t)(o.n_drawn + 1);
        admitted += r >= B;
    }
    *res.steps_run = steps_run;
    const uint64_t t2 = now_ns();
    const uint64_t n = (uint64_t)launched;
    g.stat_pool_calls++;
    g.stat_pool_admitted += (uint64_t)admitted;
    g.stat_pool_steps += (uint64_t)steps_run;  // (the steps that were launched count in batch_decode_steps)
    g.stat_chain_steps_cut += (uint64_t)(n_steps - launched);
    g.stat_chain_frozen_steps += n * (uint64_t)B - evaluated;  // column-steps that replayed an ended request's last token
    g.stat_plan_tokens += (uint64_t)B * n;
    g.stat_batch_tokens += (uint64_t)B * n;
    g.stat_batch_steps += n;
    if (ms[0].kquant) {
        g.stat_kplan_tokens += (uint64_t)B * n;
        g.stat_batch_k_steps += n;
    }
    if (ms[0].out_k) g.stat_out_k_tokens += (uint64_t)B * n;
    if (req.any_sampled(n_pool)) {
        g.stat_batch_sample_steps += n - 1;
        g.stat_batch_sample_tokens += (n - 1) * (uint64_t)B;
    } else {
        g.stat_batch_chain_steps += n - 1;
        g.stat_batch_chain_tokens += (n - 1) * (uint64_t)B;
    }
    d2h_finish();
    g.ns_match += t1 - t0;
    g.ns_launch += t2 - t1;
    g.ns_wait += now_ns() - t2;
    return 0;
}
