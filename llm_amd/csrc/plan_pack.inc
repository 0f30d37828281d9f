// plan_pack.inc — ggml_hip_prompt_pack: the prompt rows of 1..64 sessions of ONE model as one pass of the prompt plan.  Graph i is
// the reference's unchanged N_i-token graph of its own session (own memory_k / memory_v, own n_past); segment i is rows
// [row0_i, row0_i + N_i) of the R = sum N_i packed rows, in graph order.  plan_launch_prompt runs once over the R rows — embedding rows,
// norms, the five GEMMs per layer with the K split of R rows, the re-quantizing launches, the final norm, the lm_head — and its three
// launches that place a row in a sequence run in their segment forms (kernels/prompt_pack.h) on the tables built here: every row's
// position and segment, the segments' caches per layer, the 64-token V tiles (none across two segments) and the attention tiles
// in dealing order.  One plan per (R rounded up to 128, model, context); launched eagerly like the prompt plan, results where an
// evaluation of each graph alone leaves them.  -1 with nothing executed and nothing written when the graphs are not that.
#define PACK_DECLINE()                                                                                         \
    do {                                                                                                       \
        if (getenv("GGML_HIP_PACK_TRACE")) fprintf(stderr, "ggml_hip_prompt_pack declines at plan_pack.inc:%d\n", __LINE__); \
        return -1;                                                                                             \
    } while (0)
static int prompt_pack(ggml_cgraph *const *graphs, int B) {
    ensure_init();
    finish_pending();
    spec_cancel();
    g.chain_plan = nullptr;
    res_settle();  // (every segment's results go to its graph's own nodes: result set 0)
    if (g.prep) g.prep->gr = nullptr;
    if (!g.opt_plan || !g.opt_plan_prompt || !g.opt_plan_prompt_pack || !g.opt_attn_fused || g.opt_mmq_i8) PACK_DECLINE();
    const uint64_t t0 = now_ns();
    std::vector<LlamaMatch> ms((size_t)B);
    int64_t R = 0, T_max = 0;
    for (int i = 0; i < B; i++) {
        LlamaMatch &m = ms[(size_t)i];
        tl_match_pack = true;
        const bool matched = match_llama_decode(graphs[i], m);
        tl_match_pack = false;
        if (!matched) PACK_DECLINE();
        if (!m.wte || !m.output || !m.embd || !m.logits || !m.embedding) PACK_DECLINE();  // (a stage of a layer split)
        if (m.kquant || m.f16w || qt_of(m.wtype) < 0) PACK_DECLINE();                     // block formats only (a K output under block-format layers included: out_k)
        if (m.N < 1 || m.n_past + m.N > m.C || m.E > 8192) PACK_DECLINE();                // (f16 K/V, D, E, F: the matcher's own preconditions)
        if (prompt_attn_queries(m.D, (int64_t)m.n_past + m.N) != PATTN_Q) PACK_DECLINE();
        for (const ggml_tensor *t : {m.memory_k, m.memory_v}) {  // a session of another slot keeps its cache to itself (extra_of would abort)
            const DevTensor *e = (const DevTensor *)t->extra;
            if (e && e->magic == 0x48495054 && e->slot != g_cur_slot()) PACK_DECLINE();
        }
        const int32_t *ids = (const int32_t *)m.embd->data;
        for (int n = 0; n < m.N; n++)
            if (ids[n] < 0 || ids[n] >= m.wte->ne[1]) PACK_DECLINE();
        R += m.N;
        T_max = std::max<int64_t>(T_max, (int64_t)m.n_past + m.N);
    }
    if (R > PROMPT_PLAN_MAX) PACK_DECLINE();
    ws_reset();
    std::vector<uint64_t> sig;
    for (int i = 0; i < B; i++) {
        const LlamaMatch &m = ms[(size_t)i];
        if (!plan_weights_resident(m)) {  // first evaluation of a model or a session: its leaves go up as for any graph
            upload_inputs(graphs[i]);
            if (!plan_weights_resident(m)) PACK_DECLINE();
        }
        std::vector<uint64_t> s = plan_signature(m, false);  // same weight records, dims, context, RoPE parameters
        s[0] = 0;                                            // (... whatever the number of rows)
        if (i == 0) sig = std::move(s);
        else if (s != sig) PACK_DECLINE();
    }
    if (ms[0].out_k && !out_k_prompt_weight(ms[0], nullptr)) PACK_DECLINE();  // a K output under block-format layers: no room for its f16 copy
    std::vector<__half *> mk((size_t)B), mv((size_t)B);
    for (int i = 0; i < B; i++) {
        mk[(size_t)i] = (__half *)dev_ptr(ms[(size_t)i].memory_k);
        mv[(size_t)i] = (__half *)dev_ptr(ms[(size_t)i].memory_v);
        for (int d = 0; d < i; d++)
            if (mk[(size_t)d] == mk[(size_t)i] || mv[(size_t)d] == mv[(size_t)i]) PACK_DECLINE();  // one session twice: two segments, one cache
    }
    LlamaMatch mb = ms[0];  // the plan's shape: its pool holds R rounded up to 128 rows, so packs of nearby sizes share a plan
    const int64_t R_cap = std::min<int64_t>(PROMPT_PLAN_MAX, (R + 127) & ~(int64_t)127);
    mb.N = (int)R_cap;
    mb.n_past = 0;
    mb.prompt = true;
    sig[0] = (uint64_t)R_cap;
    sig.push_back(0x7061636bull);  // "pack": never another plan's signature
    DecodePlan *p = find_or_build_plan(mb, sig);
    p->m.N = (int)R;
    p->m.n_past = (int)(T_max - 1);  // (not read by the pack's launches)
    const uint64_t t1 = now_ns();
    const LlamaMatch &m0 = ms[0];
    const int L = m0.L;
    const size_t V = (size_t)m0.V, E = (size_t)m0.E;
    // ---- the tables
    std::vector<int> pos((size_t)R), row_seg((size_t)R), tok((size_t)R);
    std::vector<PackSeg> segs((size_t)L * B);
    std::vector<PackTile> vtiles;
    struct ATile {
        int seg, qt, keys;
    };
    std::vector<ATile> at;
    int row0 = 0;
    for (int i = 0; i < B; i++) {
        const LlamaMatch &m = ms[(size_t)i];
        const int32_t *ids = (const int32_t *)m.embd->data;
        for (int n = 0; n < m.N; n++) {
            pos[(size_t)(row0 + n)] = m.n_past + n;
            row_seg[(size_t)(row0 + n)] = i;
            tok[(size_t)(row0 + n)] = ids[n];
        }
        for (int il = 0; il < L; il++) {
            const size_t off = (size_t)il * (size_t)m.C * (size_t)m.Egqa;
            segs[(size_t)il * B + i] = PackSeg{mk[(size_t)i] + off, mv[(size_t)i] + off, row0, m.N, m.n_past, 0};
        }
        for (int n0 = 0; n0 < m.N; n0 += 64) vtiles.push_back(PackTile{i, n0});
        for (int qt = 0; qt * PATTN_Q < m.N; qt++) at.push_back(ATile{i, qt, std::min(m.n_past + (qt + 1) * PATTN_Q, m.n_past + m.N)});
        row0 += m.N;
    }
    // the dealing rule of the one-session launch (prompt_attention): the CUs' first slots take the longest tiles, the ranks behind
    // them come shortest first — here over the tiles of all segments, by each tile's key count
    std::stable_sort(at.begin(), at.end(), [](const ATile &a, const ATile &b) { return a.keys < b.keys; });
    const int ntile = (int)at.size();
    const size_t lds = (size_t)PATTN_Q * std::max<size_t>((size_t)prompt_attn_row_bytes(T_max), 2 * (size_t)m0.D + 16);
    const bool two_per_cu = 2 * (lds + 1024) <= 160 * 1024 && (int64_t)ntile * m0.H > g.num_cus;
    const int r1 = two_per_cu ? std::max(1, std::min(ntile, (int)(g.num_cus / m0.H))) : ntile;
    std::vector<int> atiles((size_t)ntile * 2);
    for (int rank = 0; rank < ntile; rank++) {
        const ATile &t = at[(size_t)(rank < r1 ? ntile - 1 - rank : rank - r1)];
        atiles[(size_t)rank * 2] = t.seg;
        atiles[(size_t)rank * 2 + 1] = t.qt;
    }
    PackLaunch pk;
    {
        auto up = [&](const void *src, size_t bytes) {
            char *d = ws_alloc(bytes);
            h2d_small(d, src, bytes);
            return d;
        };
        pk.pos = (const int *)up(pos.data(), pos.size() * 4);
        pk.row_seg = (const int *)up(row_seg.data(), row_seg.size() * 4);
        pk.segs = (const PackSeg *)up(segs.data(), segs.size() * sizeof(PackSeg));
        pk.vtiles = (const PackTile *)up(vtiles.data(), vtiles.size() * sizeof(PackTile));
        pk.atiles = (const int *)up(atiles.data(), atiles.size() * 4);
        pk.n_segs = B;
        pk.n_vtiles = (int)vtiles.size();
        pk.n_atiles = ntile;
        pk.T_max = T_max;
    }
    h2d_small((char *)p->p_tok, tok.data(), tok.size() * 4);
    // the packed results: rows of the workspace, handed to every graph's own nodes below
    p->logits_out = ws_alloc((size_t)R * V * 4);
    p->emb_out = (float *)ws_alloc((size_t)R * E * 4);
    plan_launch_prompt(p, &pk);
    row0 = 0;
    for (int i = 0; i < B; i++) {
        const LlamaMatch &m = ms[(size_t)i];
        const size_t nl = (size_t)m.N * V * 4, ne = (size_t)m.N * E * 4;
        const char *lrow = p->logits_out + (size_t)row0 * V * 4, *erow = (const char *)p->emb_out + (size_t)row0 * E * 4;
        HIP_CHECK(hipMemcpyAsync(dev_ptr(m.embedding), erow, ne, hipMemcpyDeviceToDevice, g.stream));
        if (m.logits->backend != GGML_BACKEND_CPU) HIP_CHECK(hipMemcpyAsync(dev_ptr(m.logits), lrow, nl, hipMemcpyDeviceToDevice, g.stream));
        row0 += m.N;
    }
    row0 = 0;
    for (int i = 0; i < B; i++) {  // (behind every device copy: a large read-back waits for the stream piece by piece)
        const LlamaMatch &m = ms[(size_t)i];
        const char *lrow = p->logits_out + (size_t)row0 * V * 4, *erow = (const char *)p->emb_out + (size_t)row0 * E * 4;
        if (m.logits->backend == GGML_BACKEND_CPU) d2h_queue(m.logits->data, lrow, (size_t)m.N * V * 4);
        if (m.embedding->data && emb_rows_fit(m)) d2h_queue(m.embedding->data, erow, (size_t)m.N * E * 4);
        row0 += m.N;
    }
    const uint64_t t2 = now_ns();
    g.stat_prompt_plan_tokens += (uint64_t)R;
    g.stat_prompt_pack_calls++;
    g.stat_prompt_pack_segments += (uint64_t)B;
    g.stat_prompt_pack_tokens += (uint64_t)R;
    if (m0.out_k) g.stat_out_k_tokens += (uint64_t)R;
    d2h_finish();
    g.ns_match += t1 - t0;
    g.ns_launch += t2 - t1;
    g.ns_wait += now_ns() - t2;
    return 0;
}
#undef PACK_DECLINE
