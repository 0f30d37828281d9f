// plan_build.inc — from a LlamaMatch to a DecodePlan: resident weights, the signature plans are cached by, the activation pool.
// the device record of a graph leaf: offloaded by the caller, or uploaded by the executor
static DevTensor *plan_rec(const ggml_tensor *t) {
    DevTensor *e = extra_of(t);
    if (!e) e = find_tensor((uintptr_t)t->data);
    return e;
}
static KWeight plan_kw(const ggml_tensor *t) {
    DevTensor *e = plan_rec(t);
    if (!e || !e->ksoa || (uintptr_t)t->data != e->host) die("decode plan: K-quant weight '%s' has no resident planar copy", t->name);
    return e->kw;
}
static QWeight plan_qw(const ggml_tensor *t) {
    DevTensor *e = plan_rec(t);
    if (!e || !e->soa || (uintptr_t)t->data != e->host) die("decode plan: weight '%s' has no resident SoA copy", t->name);
    return e->qw;
}
// an F16 matrix: the record's bytes are the tensor's rows — pointer, row stride and row count are all the plan keeps
static F16W plan_f16w(const ggml_tensor *t) {
    DevTensor *e = plan_rec(t);
    if (!e || e->soa || e->ksoa) die("decode plan: F16 weight '%s' has no resident copy", t->name);
    return F16W{(const __half *)(e->dev + ((uintptr_t)t->data - e->host)), (int64_t)t->nb[1] / 2, t->ne[1]};
}
static uint64_t rec_id(const ggml_tensor *t) {
    DevTensor *e = plan_rec(t);
    return e ? (uint64_t)(uintptr_t)e->dev : 0;
}

static bool plan_weights_resident(const LlamaMatch &m) {
    auto ok_q = [](const ggml_tensor *t) {
        DevTensor *e = plan_rec(t);
        if (t->type == GGML_TYPE_F16) return e && !e->soa && !e->ksoa && f16_weight_ok(plan_f16w(t));  // the raw rows
        return e && (e->soa || e->ksoa) && (uintptr_t)t->data == e->host;
    };
    auto ok_raw = [](const ggml_tensor *t) {
        DevTensor *e = plan_rec(t);
        return e && !e->soa;
    };
    if (!ok_raw(m.memory_k) || !ok_raw(m.memory_v)) return false;
    if (m.wte && !ok_q(m.wte)) return false;
    if (m.output && (!ok_q(m.output) || !ok_raw(m.norm))) return false;
    if (m.stage_in && !ok_raw(m.stage_in)) return false;
    if (m.stage_out && !ok_raw(m.stage_out)) return false;
    for (auto &l : m.layers) {
        for (int i = 0; i < LAYER_MATS; i++)
            if (!ok_q(l.at(i))) return false;
        if (!ok_raw(l.attn_norm) || !ok_raw(l.ffn_norm)) return false;
    }
    return true;
}

// session = false: what a batched step's graphs must share and its plan is cached by — the model and the shape, not the caches and result nodes
static std::vector<uint64_t> plan_signature(const LlamaMatch &m, bool session = true) {
    std::vector<uint64_t> s;
    auto f2u = [](float f) { uint32_t u; memcpy(&u, &f, 4); return (uint64_t)u; };
    s.push_back((uint64_t)m.N);
    for (uint64_t v : {(uint64_t)m.L, (uint64_t)m.E, (uint64_t)m.H, (uint64_t)m.Hkv, (uint64_t)m.D, (uint64_t)m.F,
                       (uint64_t)m.V, (uint64_t)m.C, (uint64_t)m.n_dims, (uint64_t)m.wtype, f2u(m.eps),
                       f2u(m.freq_base), f2u(m.freq_scale), f2u(m.kq_scale)})
        s.push_back(v);
    // a K output under block-format layers: its own word (the output's record, next, differs from a pure twin's too)
    s.push_back((uint64_t)m.out_k);
    if (m.mpt) {  // another family's plan altogether: its own words (a LLaMA signature never has 0x6d7074 here: the next word is a record)
        s.push_back(0x6d7074ull);
        s.push_back(f2u(m.alibi_bias_max));
    }
    for (const ggml_tensor *t : {m.wte, m.norm, m.output, m.stage_in, m.stage_out}) s.push_back(t ? rec_id(t) : 0);
    if (session)
        for (const ggml_tensor *t : {m.memory_k, m.memory_v}) s.push_back(rec_id(t));
    for (auto &l : m.layers) {
        for (const ggml_tensor *t : {l.attn_norm, l.ffn_norm}) s.push_back(rec_id(t));
        for (int i = 0; i < LAYER_MATS; i++) s.push_back(rec_id(l.at(i)));
    }
    if (m.f16w) {  // an F16 weight record is pointer, stride and rows: a view of another part of a record is another weight
        auto rec = [&](const ggml_tensor *t) {
            if (!t) return;
            s.push_back((uint64_t)(uintptr_t)t->data);
            s.push_back((uint64_t)t->nb[1]);
            s.push_back((uint64_t)t->ne[1]);
        };
        rec(m.wte);
        rec(m.output);
        for (auto &l : m.layers)
            for (int i = 0; i < LAYER_MATS; i++) rec(l.at(i));
    }
    if (!session || m.mpt) return s;  // (an MPT plan's results are rows of its pool: whichever arena the caller's graph of this token lives in)
    s.push_back(m.logits ? (uint64_t)(uintptr_t)dev_ptr(m.logits) : 0);
    s.push_back(m.embedding ? (uint64_t)(uintptr_t)dev_ptr(m.embedding) : 0);
    return s;
}
// every matrix of the model: the layers' seven each and the lm_head
static std::vector<const ggml_tensor *> plan_matrices(const LlamaMatch &m) {
    std::vector<const ggml_tensor *> ws;
    for (auto &l : m.layers)
        for (int i = 0; i < LAYER_MATS; i++) ws.push_back(l.at(i));
    if (m.output) ws.push_back(m.output);
    return ws;
}
// the bytes the resident f16 copies of `ws` would take that are not there yet (M x K x 2 each, whichever layout the record has)
static size_t w16_need(const std::vector<const ggml_tensor *> &ws) {
    size_t need = 0;
    for (auto *w : ws) {
        DevTensor *e = plan_rec(w);
        if (e && !e->w16) need += e->ksoa ? (size_t)e->kw.M * (size_t)e->kw.nsb * 512 : (size_t)e->qw.M * e->qw.nb * 64;
    }
    return need;
}
// the layers' matrices as a plan holds them: of(tensor) for each
template <class W, class F>
static std::vector<LayerMats<W>> plan_layer_weights(const LlamaMatch &m, F &&of) {
    std::vector<LayerMats<W>> v(m.layers.size());
    for (size_t il = 0; il < v.size(); il++)
        for (int i = 0; i < LAYER_MATS; i++) v[il].at(i) = of(m.layers[il].at(i));
    return v;
}
// Prompt plan of a K-quant model: its GEMMs have no operand but the resident f16 copy of each weight (mul_mat_k_gemm,
// backend_ops.inc) — every matrix must have one before anything is launched; they are made here, all or none, by the first batch
// the prompt plan sees (mmq_min = 32 tokens and more; the executor alone waits for W16_MIN_TOKENS, but without a copy its K path
// streams every matrix through the mat-vec kernel: 1.7k tok/s at n_batch = 48).  false = no room: the node-by-node executor runs.
static bool k_prompt_weights(const LlamaMatch &m, DecodePlan *p) {
    const std::vector<const ggml_tensor *> ws = plan_matrices(m);
    for (auto *w : ws) {
        DevTensor *e = plan_rec(w);
        if (!e || !e->ksoa || (uintptr_t)w->data != e->host) return false;
    }
    if (const size_t need = w16_need(ws)) {  // all or none: a model either fits twice or it does not
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need + ((size_t)1 << 30) + w16_headroom()) return false;
        for (auto *w : ws)
            if (!ensure_w16_k(plan_rec(w))) return false;
    }
    if (!p) return true;
    auto qw_of = [&](const ggml_tensor *t) {
        DevTensor *e = plan_rec(t);
        QWeight w;
        memset(&w, 0, sizeof(w));
        w.M = e->kw.M;
        w.nb = e->kw.nsb * 8;
        w.qt = QT_Q8_0;  // never read: every kernel that takes a resident copy reads only w16 (as in mul_mat_k_gemm)
        w.w16 = e->w16;
        return w;
    };
    p->lw = plan_layer_weights<QWeight>(m, qw_of);
    if (m.output) p->output = qw_of(m.output);
    p->w16_gen = g.w16_gen;
    return true;
}
// The prompt plan of an out_k model (block-format layers, K output): its lm_head GEMM has no operand but the resident f16 copy of the
// output matrix, as every GEMM of a K-quant model (k_prompt_weights).  Made here if it is not there; p: also its QWeight face into
// p->output.  false = no room for the copy: nothing has been launched, the node-by-node executor runs the batch.
static bool out_k_prompt_weight(const LlamaMatch &m, DecodePlan *p) {
    DevTensor *e = plan_rec(m.output);
    if (!e || !e->ksoa || (uintptr_t)m.output->data != e->host) return false;
    if (!e->w16) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < w16_need({m.output}) + w16_headroom()) return false;
        if (!ensure_w16_k(e)) return false;
    }
    if (!p) return true;
    memset(&p->output, 0, sizeof(p->output));
    p->output.M = e->kw.M;
    p->output.nb = e->kw.nsb * 8;
    p->output.qt = QT_Q8_0;  // never read: every kernel that takes a resident copy reads only w16 (as in mul_mat_k_gemm)
    p->output.w16 = e->w16;
    return true;
}
// Does blockIdx mod 8 name the XCD of a one-workgroup-per-CU launch on this device?  (The dispatcher deals workgroups round robin over
// the XCDs; HW_REG_XCC_ID says where each one landed.)  Looked at once per slot, outside any capture (build_plan).
static void xcd_labels_probe() {
    if (g.xcd_labels >= 0) return;
    g.xcd_labels = 0;
    if (g.num_cus % 8 != 0 || g.num_cus < 16) return;
    unsigned *d = nullptr;
    dev_malloc((void **)&d, (size_t)g.num_cus * 4, "XCD probe");
    std::vector<unsigned> id((size_t)g.num_cus);
    bool ok = true;
    for (int rep = 0; rep < 2 && ok; rep++) {
        hipLaunchKernelGGL(k_xcc_ids, dim3((unsigned)g.num_cus), dim3(1024), 0, g.stream, d);
        HIP_CHECK(hipMemcpyAsync(id.data(), d, id.size() * 4, hipMemcpyDeviceToHost, g.stream));
        HIP_CHECK(hipStreamSynchronize(g.stream));
        unsigned seen = 0;
        for (int b = 0; b < 8; b++) seen |= 1u << id[(size_t)b];
        ok = __builtin_popcount(seen) == 8;
        for (int b = 8; b < g.num_cus && ok; b++) ok = id[(size_t)b] == id[(size_t)(b & 7)];
    }
    HIP_CHECK(hipFree(d));
    g.xcd_labels = ok ? 1 : 0;
}
// One pool for all persistent activations of a plan, declared once: take(field, bytes) gives `field` the next region of the pool,
// 256-byte aligned, or leaves it null where the plan has no such buffer (bytes = 0) — the launchers test gran, ogran, logits_alt,
// bcols, the [block][8] tables and the k_* rows for exactly that.  plan_pool_layout runs twice: without a base it only adds up.
struct PoolCarver {
    char *base;
    size_t off = 0;
    template <class T>
    void take(T *&field, size_t bytes) {
        if (base && bytes) field = (T *)(base + off);
        off = (off + bytes + 255) & ~(size_t)255;
    }
};
static void plan_pool_layout(DecodePlan *p, PoolCarver &c) {
    const LlamaMatch &m = p->m;
    const size_t R = (size_t)m.N;  // activation rows: 1 for decode, 2..31 for a prompt chunk, the columns of a batched step, more for the prompt plan
    const size_t E = (size_t)m.E, F = (size_t)m.F, S = (size_t)p->att_S;
    const bool one = m.N == 1, spec = one && m.logits, multi = m.N >= 2 && !m.prompt, kq = m.kquant;
    const bool okq = m.out_k && !m.prompt;  // the Q8_K rows of the final norm for an out_k model's lm_head (plan_lm_head_k): R rows of E
    // scratch of the split attention, and the hand-off granules of the in-launch attention exchanges: one set per LAYER for a single token (the tag is the token's epoch alone)
    const size_t Lg = one ? (size_t)m.L : 1;
    c.take(p->att_sc, (size_t)m.H * m.C * 4);
    c.take(p->att_pmax, (size_t)m.H * S * 4);
    c.take(p->att_part, (size_t)m.H * S * m.D * 4);
    c.take(p->att_mxg, Lg * m.H * S * 8);
    c.take(p->att_sumg, Lg * m.H * S * 16);
    c.take(p->att_partg, one ? Lg * m.H * S * m.D * 8 : 0);
    c.take(p->att_cnt, (size_t)m.H * 4);
    c.take(p->hot, 256);
    c.take(p->logits_alt, spec ? (size_t)m.V * 4 : 0);
    c.take(p->emb_alt, spec ? E * 4 : 0);
    c.take(p->kv_save[0], spec ? (size_t)m.L * m.Egqa * 4 : 0);
    c.take(p->kv_save[1], spec ? (size_t)m.L * m.Egqa * 4 : 0);
    c.take(p->xnext, spec && m.wte && !kq && !m.f16w && !m.mpt ? E * 4 : 0);
    c.take(p->epoch, 256);
    const size_t units = (size_t)((m.E + 2 * m.Egqa) / 2);  // granules of a layer's wq|wk|wv rows
    c.take(p->gran, one ? (size_t)m.L * units * 8 : 0);
    c.take(p->dead_gran, one ? units * 8 : 0);  // never written (tag 0): option test_fused_timeout
    c.take(p->ogran, one ? (size_t)m.L * (size_t)(m.E / 32) * OGRAN * 8 : 0);  // the heads' outputs as granules (WO form)
    // a batched step's per-column table and its results, one row per column: the other plans' logits_out / emb_out are graph nodes (build_plan)
    c.take(p->bcols, p->batch ? sizeof(BatchCols) : 0);
    c.take(p->scols, p->batch || (spec && m.wte) ? sizeof(SampleCols) : 0);  // (a single-token whole-model plan: ggml_hip_decode_sampled_chain's one column)
    c.take(p->logits_out, p->batch || m.mpt ? R * m.V * 4 : 0);  // (an MPT plan's too: its caller builds every token's graph in a fresh arena)
    c.take(p->emb_out, p->batch || m.mpt ? R * E * 4 : 0);
    c.take(p->alibi, m.mpt ? 256 * 4 : 0);
    c.take(p->prm, sizeof(DecParams));
    c.take(p->rope, std::max<size_t>(8, R) * 128 * 4);
    c.take(p->xa, R * E * 4);
    c.take(p->xb, R * E * 4);
    c.take(p->q, R * E * 4);
    c.take(p->gate, R * F * 4);
    c.take(p->e_lo, R * E / 2);
    c.take(p->e_hi, R * E / 2);
    c.take(p->e_d, R * E / 32 * 4);
    c.take(p->e_s, R * E / 32 * 4);
    c.take(p->f_lo, R * F / 2);
    c.take(p->f_hi, R * F / 2);
    c.take(p->f_d, R * F / 32 * 4);
    c.take(p->f_s, R * F / 32 * 4);
    const size_t passes = (R + 7) / 8;  // multi-token plan: one [block][8] table per pass of 8 rows
    c.take(p->e_dT, multi ? passes * E / 32 * 32 : 0);
    c.take(p->e_sT, multi ? passes * E / 32 * 32 : 0);
    c.take(p->f_dT, multi ? passes * F / 32 * 32 : 0);
    c.take(p->f_sT, multi ? passes * F / 32 * 32 : 0);
    const size_t kW = okq ? E : std::max(E, F);
    c.take(p->k_kf, kq ? R * m.Egqa * 4 : 0);
    c.take(p->k_vf, kq ? R * m.Egqa * 4 : 0);
    c.take(p->k_att, kq || m.f16w || m.mpt ? R * E * 4 : 0);  // (the F16 plan's attention output too: the f32 row wo stages)
    c.take(p->k_g3, kq ? R * F * 4 : 0);
    c.take(p->k_q8, kq || okq ? R * kW : 0);
    c.take(p->k_d8, kq || okq ? R * kW / 256 * 4 : 0);
    c.take(p->k_bs, kq || okq ? R * kW / 256 * 32 : 0);
    // (the prompt plan's other buffers live only during one evaluation: shared workspace, plan_launch_prompt)
    c.take(p->p_tok, m.prompt ? R * 4 : 0);
}
// batch: the plan of a batched step (m: its first graph's match with N = the columns)
// Test-only: MPT plans built while it is set get a WRONG slope table.  Nothing but ggml_hip_debug_mpt (op 2, debug_mpt.inc) may set it, and
// whoever sets it clears it again (tests/test_mpt_plan_gpu.py does so in a finally); no option, no environment variable reaches it.
static int g_mpt_slope_mutant = 0;
static DecodePlan *build_plan(const LlamaMatch &m, std::vector<uint64_t> sig, bool batch = false) {
    if (m.prompt && !m.kquant) {  // prompt plan: resident f16 copies of the GEMM weights, all or none (a model either fits twice or not)
        const std::vector<const ggml_tensor *> ws = plan_matrices(m);
        size_t free_b = 0, total_b = 0;
        const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= w16_need(ws) + w16_headroom();
        if (room)
            for (auto *w : ws)
                if (w != m.output || !m.out_k) ensure_w16(plan_rec(w));  // (an out_k model's output: resolve_plan / prompt_pack have made its copy, out_k_prompt_weight)
    }
    xcd_labels_probe();
    if (!g.hot_line) {  // (here, not at the first launch: launches may be inside a stream capture)
        dev_malloc(&g.hot_line, 256, "the dummy ring steps' line");
        HIP_CHECK(hipMemsetAsync(g.hot_line, 0, 256, g.stream));
    }
    DecodePlan *p = new DecodePlan();
    p->sig = std::move(sig);
    p->m = m;
    if (m.wte) (m.f16w ? (void)(p->f_wte = plan_f16w(m.wte)) : m.kquant ? (void)(p->k_wte = plan_kw(m.wte)) : (void)(p->wte = plan_qw(m.wte)));
    if (m.output) {
        if (m.f16w) p->f_output = plan_f16w(m.output);
        else if (m.kquant || m.out_k) p->k_output = plan_kw(m.output);  // (out_k: the one K matrix of a block-format plan)
        else p->output = plan_qw(m.output);
        p->norm = (const float *)dev_ptr(m.norm);
        if (m.out_k && m.prompt && !out_k_prompt_weight(m, p)) die("prompt plan: no room for the f16 copy of the K-quant output matrix (set GGML_HIP_PLAN_OUT_K=0 to run the node-by-node executor)");
    }
    if (m.stage_in) p->stage_in = (float *)dev_ptr(m.stage_in);
    if (m.stage_out) p->stage_out = (float *)dev_ptr(m.stage_out);
    p->batch = batch;
    if (!batch) {
        p->mem_k = (__half *)dev_ptr(m.memory_k);
        p->mem_v = (__half *)dev_ptr(m.memory_v);
    }
    if (m.f16w) p->flw = plan_layer_weights<F16W>(m, plan_f16w);
    else if (m.kquant) p->klw = plan_layer_weights<KWeight>(m, plan_kw);
    else p->lw = plan_layer_weights<QWeight>(m, plan_qw);
    for (auto &l : m.layers) p->ln.push_back({(const float *)dev_ptr(l.attn_norm), (const float *)dev_ptr(l.ffn_norm)});
    // the results of every plan but a batched step's are the graph's own nodes; a batched step's are rows of the pool (plan_pool_layout)
    if (m.embedding && !batch && !m.mpt) p->emb_out = (float *)dev_ptr(m.embedding);
    if (m.logits && !batch && !m.mpt) p->logits_out = dev_ptr(m.logits);
    p->att_S = plan_att_S(m.H);
    PoolCarver sizes{nullptr};
    plan_pool_layout(p, sizes);
    dev_malloc((void **)&p->pool, sizes.off, "a decode plan's activation pool");
    HIP_CHECK(hipMemsetAsync(p->pool, 0, sizes.off, g.stream));
    PoolCarver carve{p->pool};
    plan_pool_layout(p, carve);
    if (!g.ferr_pin) {
        HIP_CHECK(hipHostMalloc((void **)&g.ferr_pin, 64, hipHostMallocDefault));
        *g.ferr_pin = 0;
    }
    p->ferr = g.ferr_pin;  // device-visible address of the slot's pinned word
    if (m.mpt) {  // the slope table: the executor's host routine on the graph's alibi parameters
        ggml_tensor al;
        memset(&al, 0, sizeof(al));
        al.op_params[1] = (int32_t)m.H;
        memcpy(al.op_params + 2, &m.alibi_bias_max, 4);
        AlibiSlopes sl = alibi_slopes(&al);
        if (g_mpt_slope_mutant) {  // test hook (ggml_hip_debug_mpt): every head on the first sequence
            const int n_floor = 1 << (int)floor(log2((double)m.H));
            const float m0 = powf(2.0f, -(m.alibi_bias_max) / n_floor);
            for (int k = 0; k < (int)m.H; k++) sl.m[k] = powf(m0, k + 1);
        }
        h2d_bulk((char *)p->alibi, &sl, sizeof(sl));
    }
    return p;
}
