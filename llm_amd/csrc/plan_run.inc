// plan_run.inc — running a plan: capture and replay of its hipGraphs, the results' way to the host, the speculative next token,
// the re-run of a token whose in-launch hand-off gave up, the greedy and the sampled chain of one session, the batched step.
// An evaluation (try_decode_plan) is the sequence of its steps, each a function of its own in front of it: resolve_plan (the graph's
// match and plan), settle_ahead (was the run ahead of the caller this evaluation?), host_dec_params (the parameters the host uploads;
// also the re-run's and the chain's), run_prompt_plan, plan_sync_dev_gen, launch_tail (a greedy token's graph; result set and
// prepared opening are arguments of the launch sequence, LaunchCtx), plain_graph (every other graph) and count_token_forms.
// begin capture, launch, end capture, instantiate: the launches of `launch` as a graph and its first executable instance
template <class F>
static void capture_into(hipGraph_t *graph, hipGraphExec_t *exec, F &&launch) {
    HIP_CHECK(hipStreamBeginCapture(g.stream, hipStreamCaptureModeThreadLocal));
    launch();
    HIP_CHECK(hipStreamEndCapture(g.stream, graph));
    HIP_CHECK(hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0));
}
// the plain graphs of attention variant v (result set 0, no tail), captured from `launch` if there is none yet: .exec is ready to launch
template <class F>
static VariantGraphs &plain_graph(DecodePlan *p, int v, F &&launch) {
    VariantGraphs &vg = p->graphs[v];
    if (!vg.exec) capture_into(&vg.graph, &vg.exec, launch);
    return vg;
}
// room for n sampled ids in the plan's chain_out
static void chain_out_reserve(DecodePlan *p, int n) {
    if (p->chain_cap >= n) return;
    if (p->chain_out) (void)hipFree(p->chain_out);
    p->chain_cap = std::max(n, 256);
    HIP_CHECK(hipMalloc((void **)&p->chain_out, (size_t)p->chain_cap * 4));
}
// The DecParams the host uploads for the evaluation m describes: its position, its token ids (a prompt plan takes its ids from p_tok),
// each checked against the vocabulary.  pos_tail is n_past for every caller.  Only k_token_tail with a TailPrep reads it, i.e. a
// tail graph; the two callers that are not an evaluation (token_finish's re-run, decode_greedy_chain) have cancelled the ahead run
// and cleared prm_ahead, so the next tail graph is launched by an evaluation that found nothing pending: behind its own upload.
static DecParams host_dec_params(const LlamaMatch &m) {
    DecParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.n_past = hp.pos_tail[0] = hp.pos_tail[1] = m.n_past;
    hp.token = m.embd ? ((const int32_t *)m.embd->data)[0] : 0;
    for (int i = 0; i < 32; i++) {
        hp.tokens[i] = (m.embd && i < m.N && !m.prompt) ? ((const int32_t *)m.embd->data)[i] : 0;
        if (m.wte && (hp.tokens[i] < 0 || hp.tokens[i] >= m.wte->ne[1])) die("token id %d out of range", hp.tokens[i]);
    }
    return hp;
}
// results the host reads, queued behind the evaluation's kernels: the logits (CPU-backend node, model/common.rs:6-38) ...
static bool emb_rows_fit(const LlamaMatch &m) { return (size_t)m.N * (size_t)m.E * 4 <= ((size_t)128 << 10); }  // (what is mirrored at all, see queue_results)
static bool emb_row_mirrored(const DecodePlan *p) {
    const LlamaMatch &m = p->m;
    return m.embedding && m.embedding->data && p->emb_out && emb_rows_fit(m);
}
static void queue_results(const DecodePlan *p) {
    const LlamaMatch &m = p->m;
    if (m.N == 1 && !m.prompt) g.stat_result_copies += (m.logits && m.logits->backend == GGML_BACKEND_CPU ? 1 : 0) + (emb_row_mirrored(p) ? 1 : 0);
    if (m.logits && m.logits->backend == GGML_BACKEND_CPU) d2h_queue(m.logits->data, p->logits_out, (size_t)m.V * m.N * 4);
    // the embedding_result node is offloaded in the reference's graph, yet common::extract_embeddings reads its HOST pointer
    // (crates/llm-base/src/model/common.rs:41-59): a decode token's / prompt chunk's rows (16 KB per token) are mirrored to the node's
    // host data with the logits, so that an unchanged caller reads what the device computed.  (Bigger evaluations keep the node on
    // the device only: 8 MB per 512-token batch nobody may want — read it with ggml_hip_tensor_get, INTEGRATION.md.)
    if (emb_row_mirrored(p)) d2h_queue(m.embedding->data, (const char *)p->emb_out, (size_t)m.N * (size_t)m.E * 4);
}
// ---- the end of a single-token plan run: wait, deliver the results, and look at the plan's error word ----
// k_qkv_attn / k_attn_split_one contain workgroups that wait for rows or partial results of OTHER workgroups of the same launch.
// That is only live while the whole launch is resident (one 1024-thread workgroup per CU).  Several slots of one process on a GPU
// are accounted for (fused_qkv_shape, attn_one_ok); another PROCESS on the GPU, or a CU mask, is invisible from here: the waits are
// bounded (GRAN_SPIN_MAX), the error word comes back with the token's results, and a token whose hand-off gave up is re-run on
// the kernels that do not wait inside a launch (k_mmvq_big + k_attn_decode / the three split launches — bit-identical results),
// which the slot then keeps; option fused_fallback = 0, a stage of a layer split (its garbage residual has already travelled
// on) and a device-sampled chain abort with the message instead.  SURVEY 8b: no error returns; never silent garbage.
static void token_results_queue(DecodePlan *p) {
    if (p->m.N != 1 || p->m.prompt || !p->ferr) return;
    g.ferr_plan = p;  // the word itself needs no copy: the kernels write it into pinned host memory, visible once the token's
                      // result copies (queued behind its kernels) are done
}
// a greedy token's results: out of the slot its graph's k_token_tail filled, into the caller's memory (as d2h_finish moves its staging);
// the id that came with them is the token the device fed the run it started behind that graph
static void tail_deliver(const Backend::TailWait &tw) {
    const DecodePlan *tp = tw.plan;
    const char *sl = tp->slot[tw.q];
    if (tw.logits_dst) memcpy(tw.logits_dst, sl, (size_t)tp->m.V * 4);
    if (tw.emb_dst) memcpy(tw.emb_dst, sl + tp->slot_emb_off, (size_t)tp->m.E * 4);
    if (g.spec.pending && g.spec.plan == tw.plan && g.spec.parity == (tw.q ^ 1)) {
        g.spec.fed_id = *(const int32_t *)(sl + tp->slot_id_off);
        g.spec.fed_id_valid = true;
    }
}
static void token_finish(bool can_rerun = true) {
    const Backend::TailWait tw = g.tail;
    g.tail = Backend::TailWait{};
    if (tw.plan) {  // the token's own event, recorded directly behind its graph: whatever runs behind that is not waited for
        HIP_CHECK(hipEventSynchronize(tw.plan->slot_ev[tw.q]));
        if (!stg.pending.empty()) d2h_finish();
        else if (tw.staged) stg.small_off = 0;
    } else {
        d2h_finish();
    }
    DecodePlan *p = g.ferr_plan;
    g.ferr_plan = nullptr;
    if (!p || !g.ferr_pin || !*(volatile unsigned *)g.ferr_pin) {
        if (tw.plan) tail_deliver(tw);
        return;
    }
    spec_cancel();  // (first: a run ahead of this token, still in flight on the same launches, may raise the word again)
    *(volatile unsigned *)g.ferr_pin = 0;
    g.stat_fused_timeouts++;
    static const char *what =
        "an attention workgroup of k_qkv_attn / k_attn_split_one gave up waiting for rows of its own launch (these launches "
        "need all their workgroups resident at once: is another process, or a CU mask, holding compute units of this GPU?)";
    if (!live_plan(p)) die("%s", what);
    const bool whole = p->m.wte && p->m.output;  // a stage's garbage residual has already been handed on
    if (!g.opt_fused_fallback || !can_rerun || !whole || p->m.N != 1)
        die("%s; set GGML_HIP_FUSE_ATTN=0 GGML_HIP_ATTN_ONE=0 to run the two-launch forms", what);
    static bool warned = false;
    if (!warned) fprintf(stderr, "libggml_hip: %s — re-running the token on the two-launch forms and keeping them on this device slot\n", what);
    warned = true;
    if (g.opt_fuse_attn || g.opt_attn_one) {  // what comes back after a clean stretch (try_decode_plan)
        g.fused_saved_fuse_attn = g.opt_fuse_attn;
        g.fused_saved_attn_one = g.opt_attn_one;
    }
    g.fused_rearm_stretch = g.fused_rearm_stretch ? g.fused_rearm_stretch * 2 : (uint64_t)std::max(0, g.opt_fused_rearm_tokens);
    g.fused_rearm_at = g.opt_fused_rearm_tokens > 0 ? g.stat_plan_tokens + g.fused_rearm_stretch : 0;
    g.opt_fuse_attn = 0;
    g.opt_attn_one = 0;
    if (!g.opt_test_fused_timeout) g.opt_affine = 0;  // (stays off when the fused forms come back: a placement the dealing cannot rely on is the likeliest cause)
    g.opt_test_fused_timeout = 0;
    for (auto *q : g_plans) drop_plan_graphs(q);
    const LlamaMatch &m = p->m;
    {   // this token and position again: a speculative run queued behind the token has moved the device's parameters on
        const DecParams hp = host_dec_params(m);
        h2d_small((char *)p->prm, &hp, sizeof(hp));
        g.stat_result_copies++;
        p->prm_ahead = false;
    }
    plan_launch_decode(p, attn_variant(m, p, m.n_past + 1));
    g.res_plan = nullptr;  // (launched outside a graph: result set 0)
    queue_results(p);  // the copies try_decode_plan queued for this token, again (a greedy token: instead of its slot)
    d2h_finish();
    if (*(volatile unsigned *)g.ferr_pin) die("%s — and again on the re-run", what);
}
// the wait a ggml_hip_graph_compute_begin left for later (defer_wait below)
void finish_pending() {
    if (!g.pending_wait) return;
    const uint64_t t = now_ns();
    g.pending_wait = false;
    token_finish();
    g.ns_wait += now_ns() - t;
}

// ggml_hip_graph_prepare: the match of the NEXT token's graph, made while the device runs the current one.  Only the plain case is
// remembered — a single-token decode graph whose weights are resident and whose plan exists; everything else takes the usual way
// at its begin().  Nothing of the plan is touched here: the token in flight may still need DecodePlan::m for a re-run.
struct PrepMatch {
    ggml_cgraph *gr = nullptr;
    LlamaMatch m;
    DecodePlan *p = nullptr;
    uint64_t arena_seq = 0, wgen = 0;
    int opt_gen = 0;
};
static bool prepare_decode_plan(ggml_cgraph *gr) {
    if (!g.prep) g.prep = new PrepMatch();
    PrepMatch *pm = g.prep;
    pm->gr = nullptr;
    if (!g.opt_plan || !g.opt_prepare || !gr) return false;
    LlamaMatch m;
    if (!match_llama_decode(gr, m) || m.prompt || m.N != 1 || !plan_weights_resident(m)) return false;
    const std::vector<uint64_t> sig = plan_signature(m);
    const uint64_t wgen = g_dev_wgen[g.device & 63].load(std::memory_order_acquire);
    DecodePlan *p = nullptr;
    for (auto *q : g_plans)
        if (q->sig == sig && q->wgen == wgen) p = q;
    if (!p) return false;  // the first token of a shape builds its plan the usual way
    pm->m = m;
    pm->p = p;
    pm->arena_seq = g_arena_seq.load(std::memory_order_acquire);
    pm->wgen = wgen;
    pm->opt_gen = g.opt_gen;
    pm->gr = gr;
    return true;
}

// the cached plan of signature `sig`, built for `m` if there is none; either way it holds m afterwards: the same device buffers, the
// fresh tensor pointers of this evaluation (n_past, embd).  Also where captured graphs of another slot count of the device go.
static DecodePlan *find_or_build_plan(const LlamaMatch &m, const std::vector<uint64_t> &sig, bool batch = false) {
    const uint64_t wgen = g_dev_wgen[g.device & 63].load(std::memory_order_acquire);
    {   // plans built before some weight record of this device was freed (perhaps by a sibling slot): gone before anything matches them
        bool stale = false;
        for (auto *q : g_plans) stale = stale || q->wgen != wgen;
        if (stale) drop_all_plans();
    }
    DecodePlan *p = nullptr;
    for (auto *q : g_plans)
        if (q->sig == sig) p = q;
    if (!p) {
        if (g_plans.size() >= 32) drop_all_plans();
        p = build_plan(m, sig, batch);
        p->wgen = wgen;
        g_plans.push_back(p);
    } else {
        p->m = m;
    }
    return p;
}

// the two result slots of a plan's greedy tokens and their events (DecodePlan::slot), made at the first such token
static void tail_slots(DecodePlan *p) {
    if (p->slot[0]) return;
    p->slot_emb_off = ((size_t)p->m.V * 4 + 255) & ~(size_t)255;
    p->slot_id_off = p->slot_emb_off + (((size_t)p->m.E * 4 + 255) & ~(size_t)255);
    for (int q = 0; q < 2; q++) {
        HIP_CHECK(hipHostMalloc((void **)&p->slot[q], p->slot_id_off + 256, hipHostMallocDefault));
        HIP_CHECK(hipEventCreateWithFlags(&p->slot_ev[q], hipEventDisableTiming));
    }
}
// whether the plan's greedy tokens prepare their successors (option tail_prepare): the block-format plan on the big workgroups, whole
// model.  K-quant plans, F16 plans, option big = 0 and the stages of a split keep their prologue launches.
static bool tail_prepares(const DecodePlan *p) {
    const LlamaMatch &m = p->m;
    return g.opt_tail_prepare && g.opt_big && !m.kquant && !m.f16w && !m.mpt && m.N == 1 && m.wte && m.output && qt_of(m.wtype) >= 0 && p->xnext && p->kv_save[0] && p->mem_k &&
           p->mem_v && m.D / 2 <= 64 && m.E % 32 == 0;
}
// what the tail of the graph of parity q prepares: the next token's row, its table and epoch, and the cache rows the graph of parity
// q ^ 1 will write, into that parity's save area (where spec_take_back looks for them)
static TailPrep tail_prep_args(const DecodePlan *p, int q) {
    const LlamaMatch &m = p->m;
    TailPrep tp;
    memset(&tp, 0, sizeof(tp));
    tp.xnext = p->xnext;
    tp.wte = p->wte;
    tp.rope = p->rope; tp.epoch = p->epoch;
    tp.theta_scale = powf(m.freq_base, -2.0f / m.n_dims); tp.freq_scale = m.freq_scale; tp.half_d = (int)(m.D >> 1);
    tp.mem_k = p->mem_k; tp.mem_v = p->mem_v; tp.save = p->kv_save[q ^ 1];
    tp.L = m.L; tp.C = (int)m.C; tp.Egqa = (int)m.Egqa;
    tp.pos_in = &p->prm->pos_tail[q]; tp.pos_out = &p->prm->pos_tail[q ^ 1];
    return tp;
}
// ---- an evaluation's steps, in the order try_decode_plan takes them ----
// The plan for this graph, holding its match (copied into m as well); null: not a graph for the plans (nothing has been enqueued but
// perhaps the graph's leaves).  A match made ahead of time (ggml_hip_graph_prepare) is taken if nothing has happened since that could
// change the answer; otherwise the matcher, the leaves' upload, the K-prompt fallback and find_or_build_plan.
static DecodePlan *resolve_plan(ggml_cgraph *gr, LlamaMatch &m) {
    if (PrepMatch *pm = g.prep) {
        DecodePlan *p = nullptr;
        if (pm->gr == gr && pm->arena_seq == g_arena_seq.load(std::memory_order_acquire) && pm->opt_gen == g.opt_gen &&
            pm->wgen == g_dev_wgen[g.device & 63].load(std::memory_order_acquire))
            p = live_plan(pm->p);
        pm->gr = nullptr;
        if (p) {
            m = pm->m;
            p->m = m;
            g.stat_prepared_tokens++;
            return p;
        }
    }
    if (!match_llama_decode(gr, m)) {  // not LLaMA's graph: MPT's (option plan_mpt), or nothing for the plans
        m = LlamaMatch{};
        if (!match_mpt_decode(gr, m)) return nullptr;
    }
    if (!plan_weights_resident(m)) {
        // first evaluation of a model: tok_embeddings is a leaf the caller never offloads (models/llama lib.rs:52);
        // upload the graph's leaves the way the generic executor would, then look again
        upload_inputs(gr);
        if (!plan_weights_resident(m)) return nullptr;
    }
    if (m.prompt && m.kquant && !k_prompt_weights(m, nullptr)) {  // (before anything is built or launched) no room for the copies:
        if (m.N > MULTI_MAX_N) return nullptr;                     // the node-by-node executor, or for up to 31 tokens the K plan's chunks
        LlamaMatch m2;
        tl_k_prompt_off = true;
        const bool ok = match_llama_decode(gr, m2);
        tl_k_prompt_off = false;
        if (!ok) return nullptr;
        m = m2;
    }
    if (m.prompt && m.out_k && !out_k_prompt_weight(m, nullptr)) return nullptr;  // (likewise: no room for the f16 copy of the K output, the node-by-node executor)
    return find_or_build_plan(m, plan_signature(m));
}
// One token ahead: is this evaluation the one the device is already running?  Returns the parity of the ahead run on a hit, -1
// otherwise.  A miss keeps the books, pauses the guessing and takes the run's cache rows back; whatever is not a hit settles the
// result sets (behind the ahead run, in front of whatever this evaluation writes).
static int settle_ahead(DecodePlan *p, const LlamaMatch &m) {
    int hit_q = -1;
    if (g.spec.pending) {
        g.spec.pending = false;
        const bool same = g.spec.plan == p && m.N == 1 && !m.prompt && m.embd && m.n_past == g.spec.n_past &&
                          attn_variant(m, p, m.n_past + 1) == g.spec.av && g.opt_graph && !g.timing.on;
        // the id the device fed that run came to the host with the previous token's slot (tail_deliver): no synchronisation here
        const bool hit = same && g.spec.fed_id_valid && g.spec.fed_id == ((const int32_t *)m.embd->data)[0];
        // (spec_hits / spec_misses are the books of option speculate_next, the guess about an unchanged caller; a caller that announced
        // itself shows in tail_tokens and in result_copies standing still)
        if (hit) {
            hit_q = g.spec.parity;
            if (g.opt_speculate_next) g.stat_spec_hits++;
            if (g.spec.prepared) g.stat_tail_prepared_tokens++;
        } else {
            if (g.opt_speculate_next) g.stat_spec_misses++;
            g.spec.cooldown = 8;  // a sampler that does not take the first maximum: stop guessing for a while
            spec_take_back();     // the cache rows it wrote go back to what they were, behind it and in front of this evaluation
        }
        (hit ? g.stat_tail_hits : g.stat_tail_misses)++;
    }
    if (hit_q < 0) res_settle();
    return hit_q;
}
// The prompt plan's evaluation behind the parameter upload: all token ids, launched eagerly, the logits queued, the books, the wait
// (or, defer_wait, the note for ggml_hip_graph_compute_end: a batch of feed_prompt behind which another follows).
static void run_prompt_plan(DecodePlan *p, const LlamaMatch &m, bool defer_wait, uint64_t t0, uint64_t t1) {
    if (m.wte) {
        const int32_t *ids = (const int32_t *)m.embd->data;
        for (int i = 0; i < m.N; i++)
            if (ids[i] < 0 || ids[i] >= m.wte->ne[1]) die("token id %d out of range", ids[i]);
        h2d_small((char *)p->p_tok, ids, (size_t)m.N * 4);
    }
    plan_launch_prompt(p);
    if (m.logits && m.logits->backend == GGML_BACKEND_CPU)  // (the logits alone: the embedding rows of a batch stay on the device, queue_results)
        d2h_queue(m.logits->data, p->logits_out, (size_t)m.V * m.N * 4);
    const uint64_t t2 = now_ns();
    g.ns_match += t1 - t0;
    g.ns_launch += t2 - t1;
    g.stat_prompt_plan_tokens += (uint64_t)m.N;
    if (m.out_k) g.stat_out_k_tokens += (uint64_t)m.N;
    if (defer_wait) {
        g.pending_wait = true;
        g.pending_light = true;
        return;
    }
    d2h_finish();
    g.ns_wait += now_ns() - t2;
}
// graphs captured while this device had another number of slots on it froze another choice of kernels: dropped behind what they run
static void plan_sync_dev_gen(DecodePlan *p) {
    const uint64_t dgen = g_dev_gen[g.device & 63].load(std::memory_order_relaxed);
    if (p->dev_gen == dgen) return;
    if (p->dev_gen) {
        HIP_CHECK(hipStreamSynchronize(g.stream));
        drop_plan_graphs(p);
    }
    p->dev_gen = dgen;
}
// Launches the plan's greedy-token graph of variant v, parity q — result set q, slot q — and records the slot's event directly behind
// it; returns its flavour.  `ahead`: directly behind another tail graph of this plan (the evaluation's second launch and nothing
// else); where the plan's tails prepare the next token (tail_prepares) that is flavour TAIL_AHEAD, whose first kernel is the layer-0
// launch, and every other launch is TAIL_FIRST.  The set and the prepared opening reach the launch sequence as its arguments.
static int launch_tail(DecodePlan *p, int v, int q, bool ahead) {
    const LlamaMatch &m = p->m;
    const bool prep = tail_prepares(p);
    const int fl = prep && ahead ? TAIL_AHEAD : TAIL_FIRST;
    VariantGraphs &vg = p->graphs[v];
    if (!vg.tail_exec[fl][q]) {
        tail_slots(p);
        LaunchCtx cx;
        cx.out_set = q;
        cx.prepared = fl == TAIL_AHEAD;
        capture_into(&vg.tail_graph[fl][q], &vg.tail_exec[fl][q], [&] {
            if (!prep)  // (a preparing tail has saved this graph's rows already, or the token was asked for and is never taken back)
                hipLaunchKernelGGL(k_kv_row_save, dim3(kv_row_grid(p)), dim3(256), 0, g.stream, (const DecParams *)p->prm, (const __half *)p->mem_k,
                                   (const __half *)p->mem_v, p->kv_save[q], (int)m.L, (int)m.C, (int)m.Egqa);
            plan_launch_decode(p, v, cx);
            const TailPrep tp = prep ? tail_prep_args(p, q) : TailPrep{};
            hipLaunchKernelGGL(k_token_tail, dim3(token_tail_grid(prep, (long)m.L * m.Egqa)), dim3(1024), 0, g.stream, (const float *)p->res_logits(q), (int)m.V,
                               emb_rows_fit(m) ? (const float *)p->res_emb(q) : (const float *)nullptr, (int)m.E, p->prm, p->slot[q], (int)p->slot_emb_off,
                               (int)p->slot_id_off, tp);
        });
    }
    HIP_CHECK(hipGraphLaunch(vg.tail_exec[fl][q], g.stream));
    HIP_CHECK(hipEventRecord(p->slot_ev[q], g.stream));
    p->prm_ahead = true;
    return fl;
}
// the per-token counters of the forms a single-token or chunk evaluation ran as (the greedy chain keeps fewer of them: see there)
static void count_token_forms(const LlamaMatch &m, int av) {
    const bool long_ctx = av == AV_SPLIT;
    g.stat_plan_tokens += (uint64_t)m.N;
    if (long_ctx) g.stat_split_tokens++;
    if (m.N == 1 && !long_ctx) {
        const FusedShape fs = fused_qkv_shape(m, av_heads_split(av));
        if (fs.ok) g.stat_fused_tokens++;
        if (fs.ok && fs.wo) g.stat_fused_wo_tokens++;
        if (fs.ok && fs.affine) g.stat_fused_affine_tokens++;
    }
    if (av >= AV_FUSED2) g.stat_fused_heads_tokens++;
    if (m.kquant) g.stat_kplan_tokens += (uint64_t)m.N;
    if (m.out_k) g.stat_out_k_tokens += (uint64_t)m.N;
    if (m.mpt) g.stat_mpt_plan_tokens += (uint64_t)m.N;
}
static bool try_decode_plan(ggml_cgraph *gr, bool defer_wait = false) {
    g.chain_plan = nullptr;  // any new graph ends the chainable state; a single-token plan run re-arms it below
    const bool greedy_next = g.greedy_hint;  // ggml_hip_expect_greedy_next spoke of THIS graph, whatever it turns out to be
    g.greedy_hint = false;
    if (!g.opt_plan) return false;
    if (g.fused_rearm_at && g.stat_plan_tokens >= g.fused_rearm_at) {  // a clean stretch behind a hand-off that gave up: the fused forms again
        g.fused_rearm_at = 0;
        g.opt_fuse_attn = g.fused_saved_fuse_attn;
        g.opt_attn_one = g.fused_saved_attn_one;
        g.stat_fused_rearms++;
        spec_cancel();
        if (g.stream) HIP_CHECK(hipStreamSynchronize(g.stream));
        for (auto *q : g_plans) drop_plan_graphs(q);
    }
    const uint64_t t0 = now_ns();
    LlamaMatch m;
    DecodePlan *p = resolve_plan(gr, m);
    if (!p) return false;
    const uint64_t t1 = now_ns();
    const int hit_q = settle_ahead(p, m);
    const bool spec_hit = hit_q >= 0;
    const DecParams hp = host_dec_params(m);  // (checks the ids on a hit too)
    if (!spec_hit) {  // (a hit: the device wrote exactly these itself)
        h2d_small((char *)p->prm, &hp, sizeof(hp));
        p->prm_ahead = false;
        if (m.N == 1 && !m.prompt) g.stat_result_copies++;
    }
    if (m.prompt) {
        run_prompt_plan(p, m, defer_wait, t0, t1);
        return true;
    }
    const bool use_graph = g.opt_graph && !g.timing.on;
    plan_sync_dev_gen(p);
    // the attention variant for this context length (a graph each of the same plan)
    const int av = attn_variant(m, p, m.n_past + 1);
    auto launch = [&] {
        if (m.N > 1 && !m.kquant && !m.f16w)
            plan_launch_multi(p);
        else
            plan_launch_decode(p, av);
    };
    // ---- a greedy token (the caller said so, or option speculate_next does): its graph ends in k_token_tail, and the next token's
    // graph goes right behind it.  After a miss the guessing pauses; the last positions of the context have no next token. ----
    if (g.spec.cooldown > 0) g.spec.cooldown--;
    const bool tail = g.opt_token_tail && (g.opt_speculate_next || greedy_next) && g.spec.cooldown == 0 && use_graph && m.N == 1 && m.logits && m.wte &&
                      m.output && m.embd && p->logits_alt && m.n_past + 2 < m.C && !m.mpt;  // (an MPT plan: no token runs ahead — k_kv_row_save knows LLaMA's V layout alone)
    int tail_q = -1;  // the slot this token's results come through, if any
    if (spec_hit) {
        tail_q = hit_q;  // already enqueued behind the previous token (same plan, position, token and attention variant): only the host's part is missing
        p->replays++;
    } else if (tail) {
        tail_q = 0;
        launch_tail(p, av, tail_q, false);
        p->replays++;
    } else if (use_graph) {
        HIP_CHECK(hipGraphLaunch(plain_graph(p, av, launch).exec, g.stream));
        p->replays++;
    } else {
        launch();
    }
    if (tail_q >= 0) {  // nothing is queued: the slot holds the results once its event is done (token_finish)
        g.stat_tail_tokens++;
        g.tail.plan = p;
        g.tail.q = tail_q;
        g.tail.logits_dst = m.logits->backend == GGML_BACKEND_CPU ? m.logits->data : nullptr;
        g.tail.emb_dst = emb_row_mirrored(p) ? m.embedding->data : nullptr;
        g.tail.staged = !spec_hit;
        p->cur_set = tail_q;  // what every device-side reader sees from now on (result_dev_ptr); the ahead run below writes the other set
        g.res_plan = p;
    } else {
        queue_results(p);
    }
    token_results_queue(p);
    if (tail) {  // the next token, before the host waits for this one
        const int av2 = attn_variant(m, p, m.n_past + 2);
        // (directly behind this token's own tail graph: launched above, or — a hit — behind the previous token with nothing of this
        // plan in between; whatever else comes between two evaluations finds the ahead run pending and takes it back)
        g.spec.prepared = launch_tail(p, av2, tail_q ^ 1, true) == TAIL_AHEAD;
        g.spec.pending = true;
        g.spec.plan = p;
        g.spec.n_past = m.n_past + 1;
        g.spec.av = av2;
        g.spec.parity = tail_q ^ 1;
        g.spec.fed_id_valid = false;
    }
    const uint64_t t2 = now_ns();
    g.ns_match += t1 - t0;
    g.ns_launch += t2 - t1;
    count_token_forms(m, av);
    g.chain_plan = (m.N == 1 && m.logits && m.wte) ? p : nullptr;  // whole model, one token: chainable
    g.chain_graph = gr;
    if (defer_wait) {  // ggml_hip_graph_compute_begin: the caller overlaps host work, then ..._end() waits
        g.pending_wait = true;
        g.pending_light = m.N > 1;  // (the waiting launches — fused attention, the one-launch split attention — are single-token forms)
        return true;
    }
    token_finish();
    g.ns_wait += now_ns() - t2;
    return true;
}

// ---- what the device-sampled chains share: their caps, a sampled chain's arguments and what its tail can take ----
constexpr int BATCH_CHAIN_MAX_STEPS = 4096;
// chain_out of a sampled chain: a SampleHead — the bias table, which only goes up, then the SampleState (generator states, Mirostat's mu) —
// then the ids; the read-back begins at the state
constexpr int SAMPLE_BIAS_WORDS = (int)(sizeof(SampleBias) / 4), SAMPLE_RNG_WORDS = (int)(sizeof(SampleState) / 4);
struct BatchSample {
    const ggml_hip_sampler_chain *prm;
    const int32_t *windows;   // [B][64]: column c's last window_n[c] tokens, oldest first
    const int32_t *window_n;  // [B], 0 .. 64
    uint64_t *rng;            // [B], in / out
    float *mu;                // [B], in / out; may be null without Mirostat
    int stages() const { return prm->mirostat == 2 ? SAMPLE_MIROSTAT : (sampler_chain_is_default(*prm) ? SAMPLE_DEFAULT : SAMPLE_FULL); }
};
// the four-parameter entries' chain: neutral extras
static ggml_hip_sampler_chain sample_neutral(const ggml_hip_sampler *params) { return sampler_chain_neutral<ggml_hip_sampler_chain>(*params); }
// what the sampled chain's tail can take (checked before anything runs)
static bool batch_sample_ok(const BatchSample &s, int B, int64_t V) {
    if (!sampler_chain_ok(*s.prm, V, SAMPLER_K_MAX)) return false;
    if (s.prm->mirostat == 2) {  // on the row in registers only; every column's state a number
        if (V > SELECT_CAP || !s.mu) return false;
        for (int c = 0; c < B; c++)
            if (s.mu[c] != s.mu[c]) return false;
    }
    for (int c = 0; c < B; c++) {
        if (s.window_n[c] < 0 || s.window_n[c] > SAMPLER_WINDOW) return false;
        for (int i = 0; i < s.window_n[c]; i++)
            if (s.windows[c * SAMPLER_WINDOW + i] < 0 || s.windows[c * SAMPLER_WINDOW + i] >= V) return false;
    }
    return true;
}
// the parameters of a chain into a SampleCols (the rings are the caller's)
static void sample_cols_params(SampleCols &hs, const ggml_hip_sampler_chain &q) {
    hs.k = q.base.k;
    hs.top_p = q.base.top_p;
    hs.temperature = q.base.temperature;
    hs.penalty = q.base.penalty;
    hs.freq = q.freq;
    hs.presence = q.presence;
    hs.tail_free_z = q.tail_free_z;
    hs.typical_p = q.typical_p;
    hs.min_p = q.min_p;
    hs.mirostat = q.mirostat;
    hs.tau = q.tau;
    hs.eta = q.eta;
    hs.n_bias = q.n_bias;
}
// ... and its bias table into the SampleHead that heads chain_out
static void sample_head_bias(SampleHead &h, const ggml_hip_sampler_chain &q) {
    for (int i = 0; i < q.n_bias; i++) {
        h.bias.id[i] = q.bias_id[i];
        h.bias.b[i] = q.bias[i];
    }
}
// A sampled chain's state goes up, once per call: the B columns' history rings and the parameters into the plan's SampleCols, the B
// generator states and Mirostat states (a SampleState) to the front of chain_out, which gets room for n_ids ids behind them.  Returns
// where the ids start.
static int sample_cols_fill(DecodePlan *p, const BatchSample &s, int B, int n_ids) {
    chain_out_reserve(p, SAMPLE_BIAS_WORDS + SAMPLE_RNG_WORDS + n_ids);
    SampleCols hs;
    memset(&hs, 0, sizeof(hs));
    for (int c = 0; c < B; c++) {
        hs.hist_n[c] = s.window_n[c];
        for (int i = 0; i < s.window_n[c]; i++) hs.hist[c][i] = s.windows[c * SAMPLER_WINDOW + i];
    }
    sample_cols_params(hs, *s.prm);
    h2d_small((char *)p->scols, &hs, sizeof(hs));
    SampleHead h;
    memset(&h, 0, sizeof(h));
    for (int c = 0; c < B; c++) {
        h.state.rng[c] = s.rng[c];
        if (s.mu) h.state.mu[c] = s.mu[c];
    }
    sample_head_bias(h, *s.prm);
    h2d_small((char *)p->chain_out, &h, sizeof(h));
    return SAMPLE_BIAS_WORDS + SAMPLE_RNG_WORDS;
}
// ... and comes back out of the chain's read-back of chain_out (the SampleState, then the ids); out_ids may be null
static void sample_cols_back(const std::vector<int32_t> &sample_back, const BatchSample &s, int B, int32_t *out_ids) {
    SampleState st;
    memcpy(&st, sample_back.data(), sizeof(st));
    for (int c = 0; c < B; c++) {
        s.rng[c] = st.rng[c];
        if (s.mu && s.prm->mirostat == 2) s.mu[c] = st.mu[c];
    }
    if (out_ids) memcpy(out_ids, sample_back.data() + SAMPLE_RNG_WORDS, (sample_back.size() - SAMPLE_RNG_WORDS) * 4);
}
// The kernel between two steps of a chain: every column's next token from its row of `logits`, into the parameters of the step's next
// replay and out[c] — the first maximum, or (sampled) a draw of the sampler whose state sample_cols_fill has uploaded.  p->bcols is
// null on a single-token plan: one session at DecParams::n_past.
static void launch_next_token(DecodePlan *p, int B, const float *logits, const BatchSample *smp, int *out) {
    if (smp)
        launch_sample_next(g.stream, B, logits, (int)p->m.V, p->prm, p->bcols, p->scols, (unsigned long long *)(p->chain_out + SAMPLE_BIAS_WORDS), out, smp->stages());
    else
        hipLaunchKernelGGL(k_argmax_next, dim3((unsigned)B), dim3(1024), 0, g.stream, logits, (int)p->m.V, p->prm, p->bcols, out);
}

// ---- the chains that stop (ggml_hip_decode_chain_requests, ggml_hip_decode_batch_requests): a request per column ----
struct ChainRequests {
    const ggml_hip_sampler_chain *const *chains;  // [B]; a null entry: the first maximum
    const ggml_hip_chain_end *ends;               // [B]
    const int32_t *windows, *window_n;            // [B][64], [B]: as a BatchSample's; may be null when every column is greedy
    uint64_t *rng;                                // [B], in / out (likewise)
    float *mu;                                    // [B], in / out; may be null without Mirostat
    int32_t *n_count, *ended_by;                  // [B], out: draws (one session) / evaluations (batched); CHAIN_END_*
    int draws_off;                                // a column may draw budget - draws_off times: 0 for one session, 1 batched (step 0 is an evaluation, not a draw)
    int n_class[SAMPLE_CLASSES];                  // (chain_req_fill) how many columns need each instantiation
    bool any_sampled(int B) const {
        for (int c = 0; c < B; c++)
            if (chains[c]) return true;
        return false;
    }
    // whether some column can end before the call's last step: otherwise the call enqueues what its siblings enqueue, nothing polled
    bool can_end_early(int B, int steps) const {
        for (int c = 0; c < B; c++)
            if (ends[c].n_stop > 0 || ends[c].budget != steps) return true;
        return false;
    }
};
static int chain_req_class(const ggml_hip_sampler_chain *q) {
    return !q ? SAMPLE_GREEDY : (q->mirostat == 2 ? SAMPLE_MIROSTAT : (sampler_chain_is_default(*q) ? SAMPLE_DEFAULT : SAMPLE_FULL));
}
// what the request table can take, per column (checked before anything runs): the sampler as batch_sample_ok, the end rule; a budget
// in lo .. hi
static bool chain_requests_ok(const ChainRequests &r, int B, int64_t V, int lo, int hi) {
    for (int c = 0; c < B; c++) {
        const ggml_hip_chain_end &e = r.ends[c];
        if (e.n_stop < 0 || e.n_stop > CHAIN_STOP_MAX || e.budget < lo || e.budget > hi) return false;
        for (int j = 0; j < e.n_stop; j++)
            if (e.stop_id[j] < 0 || e.stop_id[j] >= V) return false;
        if (r.chains[c]) {
            if (!r.windows || !r.window_n || !r.rng) return false;
            const BatchSample one = {r.chains[c], r.windows + (size_t)c * SAMPLER_WINDOW, r.window_n + c, r.rng + c, r.mu ? r.mu + c : nullptr};
            if (!batch_sample_ok(one, 1, V)) return false;
        } else if (r.windows && r.window_n) {
            if (r.window_n[c] < 0 || r.window_n[c] > SAMPLER_WINDOW) return false;
            for (int i = 0; i < r.window_n[c]; i++)
                if (r.windows[c * SAMPLER_WINDOW + i] < 0 || r.windows[c * SAMPLER_WINDOW + i] >= V) return false;
        }
    }
    return true;
}
// the rings of the B columns into a SampleCols (its parameters stay zero: the requests carry them)
static void chain_req_rings(SampleCols &hs, const ChainRequests &r, int B) {
    memset(&hs, 0, sizeof(hs));
    for (int c = 0; c < B && r.windows && r.window_n; c++) {
        hs.hist_n[c] = r.window_n[c];
        for (int i = 0; i < r.window_n[c]; i++) hs.hist[c][i] = r.windows[c * SAMPLER_WINDOW + i];
    }
}
// the request table of a call: every column's parameters, bias table, end rule and state, and the compacted column list of every class
static void chain_req_table(SampleReqs &t, ChainRequests &r, int B) {
    memset(&t, 0, sizeof(t));
    for (int c = 0; c < B; c++) {
        const ggml_hip_sampler_chain *q = r.chains[c];
        const int cls = chain_req_class(q);
        t.list[cls][t.n_list[cls]++] = c;
        if (q) {
            SampleCols one;  // (the one place that knows the parameters' names: sample_cols_params)
            memset(&one, 0, sizeof(one));
            sample_cols_params(one, *q);
            SampleReqParams &d = t.prm[c];
            d.k = one.k; d.top_p = one.top_p; d.temperature = one.temperature; d.penalty = one.penalty;
            d.freq = one.freq; d.presence = one.presence; d.tail_free_z = one.tail_free_z; d.typical_p = one.typical_p; d.min_p = one.min_p;
            d.mirostat = one.mirostat; d.tau = one.tau; d.eta = one.eta; d.n_bias = one.n_bias;
            for (int i = 0; i < q->n_bias; i++) {
                t.bias[c].id[i] = q->bias_id[i];
                t.bias[c].b[i] = q->bias[i];
            }
            t.back.state.rng[c] = r.rng[c];
            if (r.mu) t.back.state.mu[c] = r.mu[c];
        }
        const ggml_hip_chain_end &e = r.ends[c];
        t.max_draws[c] = e.budget - r.draws_off;
        t.n_stop[c] = e.n_stop;
        for (int j = 0; j < e.n_stop; j++) t.stop_id[c][j] = e.stop_id[j];
        t.back.live[c] = t.max_draws[c] > 0;
        t.back.ended_by[c] = t.back.live[c] ? CHAIN_END_NONE : CHAIN_END_BUDGET;
    }
    for (int s = 0; s < SAMPLE_CLASSES; s++) r.n_class[s] = t.n_list[s];
}
// ... goes up, once per call: the rings into the plan's SampleCols, the table into DecodePlan::chain_req (a buffer of its own, made
// at the first such call: no buffer of the plan moves), chain_out gets room for n_ids ids (which start at its front)
static void chain_req_fill(DecodePlan *p, ChainRequests &r, int B, int n_ids) {
    chain_out_reserve(p, n_ids);
    if (!p->chain_req) HIP_CHECK(hipMalloc((void **)&p->chain_req, sizeof(SampleReqs)));
    SampleCols hs;
    chain_req_rings(hs, r, B);
    h2d_small((char *)p->scols, &hs, sizeof(hs));
    SampleReqs t;
    chain_req_table(t, r, B);
    h2d_small((char *)p->chain_req, &t, sizeof(t));
}
// ... and what comes back of it with the ids (SampleReqBack): states, counts, reasons
static void chain_req_back(const SampleReqBack &b, const ChainRequests &r, int B) {
    for (int c = 0; c < B; c++) {
        if (r.chains[c]) {
            r.rng[c] = b.state.rng[c];
            if (r.mu && r.chains[c]->mirostat == 2) r.mu[c] = b.state.mu[c];
        }
        r.n_count[c] = b.n_drawn[c] + r.draws_off;
        r.ended_by[c] = b.ended_by[c];
        if (b.ended_by[c] == CHAIN_END_STOP) g.stat_chain_stopped_columns++;
    }
}
static void launch_next_token_requests(DecodePlan *p, const ChainRequests &r, const float *logits, int *out) {
    launch_next_token_req(g.stream, r.n_class, logits, (int)p->m.V, p->prm, p->bcols, p->scols, p->chain_req, out);
}
// The columns' live flags behind a group of steps: a small copy into pinned memory of parity q and an event behind it.  The host
// waits on that event (never on memory), and only once the NEXT group is enqueued, so the device never idles.
static void chain_live_queue(DecodePlan *p, int q) {
    if (!g.chain_live_pin) {
        HIP_CHECK(hipHostMalloc((void **)&g.chain_live_pin, 2 * BATCH_COLS_MAX * 4, hipHostMallocDefault));
        for (int i = 0; i < 2; i++) HIP_CHECK(hipEventCreateWithFlags(&g.chain_live_ev[i], hipEventDisableTiming));
    }
    HIP_CHECK(hipMemcpyAsync(g.chain_live_pin + q * BATCH_COLS_MAX, (const char *)p->chain_req + offsetof(SampleReqBack, live), BATCH_COLS_MAX * 4,
                             hipMemcpyDeviceToHost, g.stream));
    HIP_CHECK(hipEventRecord(g.chain_live_ev[q], g.stream));
}
static bool chain_live_any(int q, int B) {
    HIP_CHECK(hipEventSynchronize(g.chain_live_ev[q]));
    for (int c = 0; c < B; c++)
        if (g.chain_live_pin[q * BATCH_COLS_MAX + c]) return true;
    return false;
}
// Enqueues steps first .. last - 1 of a chain that stops — enqueue(i) is step i's launches, the kernel between two steps and the
// replay — and returns the step behind the last one enqueued.  When no column can end early that is the plain loop.  Otherwise the
// steps go in groups of option chain_group: behind each group the live flags are read back, waited for once the next group is
// enqueued, and nothing more is launched once no column was found live.  variant(i) (one session) is the attention variant the host
// picks for step i from the position it EXPECTS; a frozen session sits at a lower one, and two variants are not known to agree bit
// for bit at one position — so a group never spans a variant boundary, and a group of another variant is enqueued only after the
// previous group's flags have been read and the session is still live.  (The batched step has one variant.)
template <class Enqueue, class Variant>
static int chain_req_run(DecodePlan *p, const ChainRequests &r, int B, int first, int last, bool early, Enqueue &&enqueue, Variant &&variant) {
    int i = first;
    if (!early) {
        for (; i < last; i++) enqueue(i);
        return i;
    }
    const int G = std::max(1, g.opt_chain_group);
    int pending = -1, q = 0, av_prev = 0;
    bool live = false;
    for (int c = 0; c < B; c++) live = live || r.ends[c].budget - r.draws_off > 0;
    while (i < last && live) {
        const int av = variant(i);
        if (pending >= 0 && av != av_prev) {  // across a variant boundary only behind a look at the flags
            live = chain_live_any(pending, B);
            pending = -1;
            if (!live) break;
        }
        // (groups are counted from step 0, which a batched call has run before its first tail: its first group is one step shorter)
        for (const int e = std::min(last, (i / G + 1) * G); i < e && variant(i) == av; i++) enqueue(i);
        chain_live_queue(p, q);
        if (pending >= 0) live = chain_live_any(pending, B);
        pending = q;
        q ^= 1;
        av_prev = av;
    }
    return i;
}

// SURVEY section 8f N3: n greedy tokens back to back without a host round trip per token.  `last` must be the cgraph
// of the caller's most recent ggml_graph_compute (a single-token LLaMA evaluation that ran as the fused plan, whole
// model on this device); the plan's decode parameters still hold that token and position on the device, and its
// logits are in HBM.  Per token: k_argmax_next (argmax -> parameters of the next replay) + one replay of the plan.
// Returns 0 and fills out_tokens[n] (and last_logits[V] with the logits after the n-th token, if not NULL); -1 if
// the precondition does not hold (the caller then decodes token by token).
//
// ggml_hip_decode_sampled_chain is the same chain with k_sample_next (kernels/sample.h) between two replays (`smp`, one column of a
// BatchSample): the session's history ring and the four parameters go up once per call (column 0 of DecodePlan::scols), the generator
// state sits in front of the ids in chain_out and comes back with them in one copy (sample_cols_fill / sample_cols_back, as for the
// batched chain).  Every plan the greedy chain runs is run: block-format, K-quant, F16.  Option chain_k does not apply: the K-token
// graph stays greedy-only.  Counted in sample_chain_steps / sample_chain_tokens and, as the greedy chain, in plan_tokens,
// fused_tokens, fused_heads_tokens and graph_replays.
//
// ggml_hip_decode_chain_requests is the chain with a request (`req`, one column: sampler or first maximum, stop ids, a budget of n
// draws) and the kernels of sample_req.hip between two replays; it may end before its n-th step (chain_req_run), and the session's
// position moves by the draws that were made.
static int decode_chain(ggml_cgraph *last, int n, int32_t *out_tokens, float *last_logits, const BatchSample *smp = nullptr,
                        ChainRequests *req = nullptr) {
    finish_pending();
    DecodePlan *p = live_plan(g.chain_plan);
    if (!p || g.chain_graph != last || n < 1) return -1;
    const LlamaMatch &m = p->m;
    if (m.N != 1 || !m.logits || !m.wte || m.n_past + 1 + n > m.C) return -1;
    if (m.mpt && (smp || req)) return -1;  // an MPT plan: the greedy chain alone
    if (smp && (!g.opt_plan_sample_chain || !batch_sample_ok(*smp, 1, m.V))) return -1;
    if (req && ((req->chains[0] && !g.opt_plan_sample_chain) || !p->scols || !chain_requests_ok(*req, 1, m.V, n, n))) return -1;
    if (p->prm_ahead) {  // a token tail has moved the parameters on (and a run ahead of the caller may be in flight): back to the last evaluated token
        if (!m.embd) return -1;
        const DecParams hp = host_dec_params(m);
        h2d_small((char *)p->prm, &hp, sizeof(hp));
        p->prm_ahead = false;
    }
    spec_cancel();
    // the first argmax reads the set the last evaluated token sits in; every replay below writes set 0
    const float *first_logits = (const float *)plan_cur_logits(p);
    g.res_plan = nullptr;
    if (!p->chain_ring) HIP_CHECK(hipMalloc((void **)&p->chain_ring, 64 * 4));
    int ids_off = 0;
    if (req) chain_req_fill(p, *req, 1, n);
    else if (smp) ids_off = sample_cols_fill(p, *smp, 1, n);  // the ring, the parameters, the generator state: once per call
    else chain_out_reserve(p, n);
    int *ids = p->chain_out + ids_off;
    const bool use_graph = g.opt_graph && !g.timing.on && p->any_captured();
    int i0 = 0;
    // option chain_k = K (> 1): K tokens per graph launch — every kernel of the plan reads its token and position from the
    // DecParams that k_argmax_next advances on the device, so the launches of consecutive tokens are the same launches.  Only
    // while the whole group stays on the short-context attention variant; the graph's sampled ids land in chain_out[i0 ..].
    if (use_graph && g.opt_chain_k > 1 && !smp && !req) {
        const int K = g.opt_chain_k;
        if ((const char *)first_logits != p->logits_out) {  // the K-token graph's first argmax is captured on set 0
            HIP_CHECK(hipMemcpyAsync(p->logits_out, first_logits, (size_t)m.V * 4, hipMemcpyDeviceToDevice, g.stream));
            first_logits = (const float *)p->logits_out;
        }
        const auto long_at = [&](int i) { return attn_variant(m, p, m.n_past + 1 + i + 1) != AV_SHORT; };
        while (i0 + K <= n && !long_at(i0 + K - 1)) {
            if (!p->exec_chain || p->chain_k != K) {  // (the graph writes its ids to a fixed ring: reusable at any offset)
                if (p->exec_chain) (void)hipGraphExecDestroy(p->exec_chain);
                if (p->graph_chain) (void)hipGraphDestroy(p->graph_chain);
                capture_into(&p->graph_chain, &p->exec_chain, [&] {
                    for (int k = 0; k < K; k++) {
                        launch_next_token(p, 1, (const float *)p->logits_out, nullptr, p->chain_ring + k);
                        plan_launch_decode(p, AV_SHORT);
                    }
                });
                p->chain_k = K;
            }
            HIP_CHECK(hipGraphLaunch(p->exec_chain, g.stream));
            if (fused_qkv_shape(m).ok) g.stat_fused_tokens += (uint64_t)K;
            HIP_CHECK(hipMemcpyAsync(p->chain_out + i0, p->chain_ring, (size_t)K * 4, hipMemcpyDeviceToDevice, g.stream));
            i0 += K;
        }
    }
    // the token of step i sits at position n_past + 1 + i; same rule as try_decode_plan for the attention variant
    const auto variant = [&](int i) { return attn_variant(m, p, m.n_past + 1 + i + 1); };
    const auto enqueue = [&](int i) {
        if (req) launch_next_token_requests(p, *req, i == 0 ? first_logits : (const float *)p->logits_out, ids + i);
        else launch_next_token(p, 1, i == 0 ? first_logits : (const float *)p->logits_out, smp, ids + i);
        const int av = variant(i);
        // (the chain's books are not count_token_forms': no fused_wo_tokens, fused_affine_tokens or split_tokens — values tests read; left as they are)
        if (av != AV_SPLIT && fused_qkv_shape(m, av_heads_split(av)).ok) g.stat_fused_tokens++;
        if (av >= AV_FUSED2) g.stat_fused_heads_tokens++;
        if (use_graph) {
            VariantGraphs &vg = plain_graph(p, av, [&] { plan_launch_decode(p, av); });  // (captured here: the chain crossed into a variant no evaluation has captured yet)
            if (!vg.exec2) HIP_CHECK(hipGraphInstantiate(&vg.exec2, vg.graph, nullptr, nullptr, 0));
            HIP_CHECK(hipGraphLaunch((i & 1) ? vg.exec2 : vg.exec, g.stream));
        } else {
            plan_launch_decode(p, av);
        }
    };
    int launched = n;  // steps enqueued: all of them, unless a request ended the chain early
    if (req) launched = chain_req_run(p, *req, 1, i0, n, req->can_end_early(1, n), enqueue, variant);
    else
        for (int i = i0; i < n; i++) enqueue(i);
    HIP_CHECK(hipGetLastError());
    std::vector<int32_t> sample_back;  // a sampled chain's read-back: the generator state, then the ids
    SampleReqBack req_back;
    if (req) {
        d2h_queue(&req_back, (const char *)p->chain_req, sizeof(req_back));
        if (launched) d2h_queue(out_tokens, (const char *)p->chain_out, (size_t)launched * 4);
    } else if (smp) {
        sample_back.resize((size_t)(SAMPLE_RNG_WORDS + n));
        d2h_queue(sample_back.data(), (const char *)(p->chain_out + SAMPLE_BIAS_WORDS), sample_back.size() * 4);
    } else {
        d2h_queue(out_tokens, (const char *)p->chain_out, (size_t)n * 4);
    }
    if (last_logits) d2h_queue(last_logits, p->logits_out, (size_t)m.V * 4);
    token_results_queue(p);
    token_finish(false);  // a hand-off that gave up inside the chain has already fed the sampler garbage: abort
    if (smp) {
        sample_cols_back(sample_back, *smp, 1, out_tokens);
        g.stat_sample_chain_steps += (uint64_t)n;
        g.stat_sample_chain_tokens += (uint64_t)n;
    }
    int moved = n;  // positions the session moved by
    if (req) {  // the draws that were made; the steps behind them replayed the last one's evaluation, the rest was never launched
        chain_req_back(req_back, *req, 1);
        moved = req_back.n_drawn[0];
        for (int i = launched; i < n; i++) out_tokens[i] = -1;
        g.stat_chain_frozen_steps += (uint64_t)(launched - moved);
        g.stat_chain_steps_cut += (uint64_t)(n - launched);
        if (req->chains[0]) {
            g.stat_sample_chain_steps += (uint64_t)launched;
            g.stat_sample_chain_tokens += (uint64_t)launched;
        }
        n = launched;
    }
    p->m.n_past += moved;
    p->replays += use_graph ? (uint64_t)n : 0;
    g.stat_plan_tokens += (uint64_t)n;
    if (m.out_k) g.stat_out_k_tokens += (uint64_t)n;
    if (m.mpt) g.stat_mpt_plan_tokens += (uint64_t)n;
    g.chain_plan = nullptr;  // the caller's next evaluation re-arms it
    return 0;
}
static int decode_greedy_chain(ggml_cgraph *last, int n, int32_t *out_tokens, float *last_logits) { return decode_chain(last, n, out_tokens, last_logits); }

// ggml_hip_decode_batch: one decode step of B = 2..8 single-token LLaMA graphs of ONE model, each the reference's unchanged graph for
// its own session (own memory_k / memory_v, own n_past, own token), as ONE pass over the weights: the chunk plan's launches
// (plan_launch_batch) with column c placed by the per-column table instead of "position n_past + c of one cache".  Block-format and
// F16 models; K-quant models (the K plan's chunk form) under option plan_batch_k.  One plan per
// (B, model, context) and one hipGraph of it; a step uploads DecParams (the token ids) and BatchCols (positions, caches) and replays.
// -1 with nothing executed when the graphs are not that; the caller then computes them one by one.
//
// ggml_hip_decode_batch_greedy: the same step, then n_steps - 1 more of the same B sessions, each on the first maximum of its
// column's logits, without a host round trip between them: k_argmax_next (kernels/decode.h) on B workgroups samples every column and
// writes the parameters the step's kernels read (DecParams::tokens[c], BatchCols::pos[c]), and the SAME graph is replayed — the
// launches n batched steps of a greedy caller make, on the same inputs, so the same bits.  The tail kernel is an ordinary launch
// between two graph launches; the step's graph is the one ggml_hip_decode_batch captured.  The sampled ids [n_steps - 1][B] collect
// on the device and come back with the results of the last step, which go where a single step leaves them.  Nothing of this
// outlives the call: the next step of any kind uploads its own parameters.
//
// ggml_hip_decode_batch_sampled: the same chain with k_sample_next (kernels/sample.h), B workgroups, as the tail — repetition penalty
// over the column's last 64 tokens, top-k, top-p, temperature and one xorshift64* draw, in the arithmetic of kernels/sampler_math.h,
// which the host mirror compiles too.  The columns' history rings and the four parameters go up once per call (DecodePlan::scols); the
// generator states sit in front of the sampled ids in chain_out and come back with them in one copy.
//
// ggml_hip_decode_batch_requests: the same chain with a request per column (`req`) and the kernels of sample_req.hip as the tail: a
// column that ends is frozen while the others go on, and the call ends once no column is live (chain_req_run).
static int decode_batch_steps(ggml_cgraph *const *graphs, int B, int n_steps, int32_t *out_ids, bool chain, const BatchSample *smp = nullptr,
                              ChainRequests *req = nullptr) {
    ensure_init();
    finish_pending();
    spec_cancel();
    g.chain_plan = nullptr;
    res_settle();  // (every column's results go to its graph's own nodes: result set 0)
    if (g.prep) g.prep->gr = nullptr;
    if (!g.opt_plan || !g.opt_plan_batch || (chain && !g.opt_plan_batch_chain) || (smp && !g.opt_plan_batch_sample)) return -1;
    if (req && req->any_sampled(B) && !g.opt_plan_batch_sample) return -1;
    if (n_steps < 1 || n_steps > BATCH_CHAIN_MAX_STEPS) return -1;
    const uint64_t t0 = now_ns();
    std::vector<LlamaMatch> ms((size_t)B);
    std::vector<uint64_t> sig;
    for (int c = 0; c < B; c++) {
        LlamaMatch &m = ms[(size_t)c];
        if (!match_llama_decode(graphs[c], m)) return -1;
        if (m.kquant && !(g.opt_plan_batch_k && g.opt_plan_k)) return -1;  // a K-quant model: under option plan_batch_k, on the K plan
        if (m.N != 1 || m.prompt || !m.wte || !m.output || !m.embd || !m.logits || !m.embedding) return -1;
        const int room = req ? std::max(1, std::min(n_steps, (int)req->ends[c].budget)) : n_steps;  // (a budget out of range is declined below)
        if (m.n_past + room > m.C || (qt_of(m.wtype) < 0 && !m.f16w && !m.kquant)) return -1;  // (f16 K/V, D, E, F: the matcher's own preconditions)
        for (const ggml_tensor *t : {m.memory_k, m.memory_v}) {  // a session of another slot keeps its cache to itself (extra_of would abort)
            const DevTensor *e = (const DevTensor *)t->extra;
            if (e && e->magic == 0x48495054 && e->slot != g_cur_slot()) return -1;
        }
    }
    // the whole context in k_attn_decode's LDS arrays (a column may sit anywhere in it), 8 Q8 columns of the widest row in k_mmvq_big8's
    // (an F16 model: k_mmvq_f16 stages as many columns per pass as its LDS holds; a K-quant model: so does launch_mmvq_kn, and what a
    // column of the K plan needs the matcher has checked for every graph)
    if (attn_decode_lds(ms[0].C, ms[0].D) > ATTN_DECODE_LDS_MAX || (!ms[0].f16w && !ms[0].kquant && !multi_shape_ok(ms[0], B))) return -1;
    if (smp && !batch_sample_ok(*smp, B, ms[0].V)) return -1;
    if (req && !chain_requests_ok(*req, B, ms[0].V, 1, n_steps)) return -1;
    ws_reset();
    for (int c = 0; c < B; c++) {
        const LlamaMatch &m = ms[(size_t)c];
        if (!plan_weights_resident(m)) {  // first evaluation of a model or a session: its leaves go up as for any graph
            upload_inputs(graphs[c]);
            if (!plan_weights_resident(m)) return -1;
        }
        std::vector<uint64_t> s = plan_signature(m, false);  // same weight records, dims, context, RoPE parameters
        if (c == 0) sig = std::move(s);
        else if (s != sig) return -1;
    }
    std::vector<__half *> mk((size_t)B), mv((size_t)B);
    for (int c = 0; c < B; c++) {
        mk[(size_t)c] = (__half *)dev_ptr(ms[(size_t)c].memory_k);
        mv[(size_t)c] = (__half *)dev_ptr(ms[(size_t)c].memory_v);
        for (int d = 0; d < c; d++)
            if (mk[(size_t)d] == mk[(size_t)c] || mv[(size_t)d] == mv[(size_t)c]) return -1;  // one session twice: two columns, one cache row
    }
    LlamaMatch mb = ms[0];  // the plan's shape: B columns
    mb.N = B;
    mb.n_past = 0;
    sig[0] = (uint64_t)B;
    sig.push_back(0x6261746368ull);  // "batch": never a chunk plan's signature
    DecodePlan *p = find_or_build_plan(mb, sig, true);
    for (int c = 0; c < B; c++) mb.n_past = std::max(mb.n_past, ms[(size_t)c].n_past);
    p->m.n_past = mb.n_past;  // (the attention's byte count for the timing books)
    const uint64_t t1 = now_ns();
    DecParams hp;  // (not host_dec_params: one id per column, from B matches; a batched step has no tail graph to read pos_tail)
    BatchCols hb;
    memset(&hp, 0, sizeof(hp));
    memset(&hb, 0, sizeof(hb));
    for (int c = 0; c < B; c++) {
        const LlamaMatch &m = ms[(size_t)c];
        hp.tokens[c] = ((const int32_t *)m.embd->data)[0];
        if (hp.tokens[c] < 0 || hp.tokens[c] >= m.wte->ne[1]) die("token id %d out of range", hp.tokens[c]);
        hb.pos[c] = m.n_past;
        hb.mem_k[c] = mk[(size_t)c];
        hb.mem_v[c] = mv[(size_t)c];
    }
    hp.n_past = hb.pos[0];
    hp.token = hp.tokens[0];
    h2d_small((char *)p->prm, &hp, sizeof(hp));
    h2d_small((char *)p->bcols, &hb, sizeof(hb));
    std::vector<int32_t> sample_back;  // a sampled chain's read-back: generator states, then ids
    const auto step = [&] {
        if (g.opt_graph && !g.timing.on) {
            HIP_CHECK(hipGraphLaunch(plain_graph(p, AV_SHORT, [&] { plan_launch_batch(p); }).exec, g.stream));
            p->replays++;
        } else {
            plan_launch_batch(p);
        }
    };
    step();
    int launched = n_steps;  // steps enqueued: all of them, unless every request ended early
    SampleReqBack req_back;
    if (req) {  // ids of step i at chain_out[(i - 1) * B ..], -1 where the column sat the step out
        chain_req_fill(p, *req, B, std::max(1, (n_steps - 1) * B));
        launched = chain_req_run(p, *req, B, 1, n_steps, req->can_end_early(B, n_steps),
                                 [&](int i) {
                                     launch_next_token_requests(p, *req, (const float *)p->logits_out, p->chain_out + (size_t)(i - 1) * B);
                                     step();
                                 },
                                 [](int) { return AV_SHORT; });
        HIP_CHECK(hipGetLastError());
        d2h_queue(&req_back, (const char *)p->chain_req, sizeof(req_back));
        if (launched > 1) d2h_queue(out_ids, (const char *)p->chain_out, (size_t)(launched - 1) * B * 4);
        p->m.n_past = mb.n_past + launched - 1;
        for (size_t i = (size_t)(launched - 1) * B; i < (size_t)(n_steps - 1) * B; i++) out_ids[i] = -1;  // rows never launched
        g.stat_chain_steps_cut += (uint64_t)(n_steps - launched);
        n_steps = launched;  // (the books below count the device's work)
    } else if (n_steps > 1) {  // the device samples every column and moves the step's parameters on; ids of step i at chain_out[(i - 1) * B ..]
        const int n_ids = (n_steps - 1) * B;
        int ids_off = 0;
        if (smp) ids_off = sample_cols_fill(p, *smp, B, n_ids);
        else chain_out_reserve(p, n_ids);
        int *ids = p->chain_out + ids_off;
        for (int i = 1; i < n_steps; i++) {
            launch_next_token(p, B, (const float *)p->logits_out, smp, ids + (size_t)(i - 1) * B);
            step();
        }
        HIP_CHECK(hipGetLastError());
        if (smp) {  // the generator states and the ids: one copy
            sample_back.resize((size_t)(SAMPLE_RNG_WORDS + n_ids));
            d2h_queue(sample_back.data(), (const char *)(p->chain_out + SAMPLE_BIAS_WORDS), sample_back.size() * 4);
        } else if (out_ids) {
            d2h_queue(out_ids, (const char *)p->chain_out, (size_t)n_ids * 4);
        }
        p->m.n_past = mb.n_past + n_steps - 1;
    }
    // every graph's results where an evaluation of that graph alone leaves them (queue_results): the logits in the node's host data
    // (CPU-backend node) or its device copy, the embedding row in the node's device copy and host data
    for (int c = 0; c < B; c++) {
        const LlamaMatch &m = ms[(size_t)c];
        const char *lrow = p->logits_out + (size_t)c * m.V * 4, *erow = (const char *)p->emb_out + (size_t)c * m.E * 4;
        if (m.logits->backend == GGML_BACKEND_CPU) d2h_queue(m.logits->data, lrow, (size_t)m.V * 4);
        else HIP_CHECK(hipMemcpyAsync(dev_ptr(m.logits), lrow, (size_t)m.V * 4, hipMemcpyDeviceToDevice, g.stream));
        HIP_CHECK(hipMemcpyAsync(dev_ptr(m.embedding), erow, (size_t)m.E * 4, hipMemcpyDeviceToDevice, g.stream));
        if (m.embedding->data) d2h_queue(m.embedding->data, erow, (size_t)m.E * 4);
    }
    const uint64_t t2 = now_ns();
    g.stat_plan_tokens += (uint64_t)B * (uint64_t)n_steps;
    g.stat_batch_tokens += (uint64_t)B * (uint64_t)n_steps;
    g.stat_batch_steps += (uint64_t)n_steps;
    if (ms[0].kquant) {
        g.stat_kplan_tokens += (uint64_t)B * (uint64_t)n_steps;
        g.stat_batch_k_steps += (uint64_t)n_steps;
    }
    if (ms[0].out_k) g.stat_out_k_tokens += (uint64_t)B * (uint64_t)n_steps;
    if (smp || (req && req->any_sampled(B))) {  // (a sampled step is not a greedy one: batch_chain_* count ggml_hip_decode_batch_greedy's alone)
        g.stat_batch_sample_steps += (uint64_t)(n_steps - 1);
        g.stat_batch_sample_tokens += (uint64_t)(n_steps - 1) * (uint64_t)B;
    } else {
        g.stat_batch_chain_steps += (uint64_t)(n_steps - 1);
        g.stat_batch_chain_tokens += (uint64_t)(n_steps - 1) * (uint64_t)B;
    }
    d2h_finish();
    if (!sample_back.empty()) sample_cols_back(sample_back, *smp, B, out_ids);
    if (req) {
        chain_req_back(req_back, *req, B);
        for (int c = 0; c < B; c++) g.stat_chain_frozen_steps += (uint64_t)(launched - req->n_count[c]);
    }
    g.ns_match += t1 - t0;
    g.ns_launch += t2 - t1;
    g.ns_wait += now_ns() - t2;
    return 0;
}
static int decode_batch(ggml_cgraph *const *graphs, int B) { return decode_batch_steps(graphs, B, 1, nullptr, false); }
